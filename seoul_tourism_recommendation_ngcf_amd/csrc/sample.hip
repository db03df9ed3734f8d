// Unseen items per case, the reference's TourDataset._negative_sampling (utils.py:213-275) for T cases in one launch: m items the
// case's user has no stored interaction with, uniform and without replacement - 1 for a training triplet, 24 for a test candidate
// list.  Every output value is a pure function of (seed, global case number, the user's seen row).
#include "sample_device.h"

// ---------------------------------------------------------------------------------------------
// The draw itself - the case key, the partial Fisher-Yates map kept as (key, value) entries, ranks to items - is written out in
// sample_device.h, which sample_hard.hip and sample_weighted.hip share.
//
// Mapping.  m == 1 (training triplets): a lane per case, no map.  m > 1: a wave per case, 64 steps per chunk; the entries of the
// chunk in work live in the lanes, those of earlier chunks (m > 64 only) in the wave's LDS region [2][round_up(m, 64)].
// ---------------------------------------------------------------------------------------------
#define NGCF_SAMPLE_M_MAX 1023
#define NGCF_SAMPLE_WAVES 4

namespace {

__global__ __launch_bounds__(256) void sample_unseen_one_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int64_t col_offset, int64_t n_rows, int64_t n_items,
    const int64_t *__restrict__ user_ids, int64_t T, int64_t case_offset, uint64_t seed, const int64_t *__restrict__ first,
    int64_t *__restrict__ out, int64_t ld_out, int32_t *status)
{
    const int off = first ? 1 : 0;
    int bits = 0;
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < T; row += (int64_t)gridDim.x * 256) {
        if (first) out[row * ld_out] = first[row];
        int64_t lo, len, n, item = -1;
        const int bad = sample_row(rowptr, n_rows, n_items, user_ids[row], 1, lo, len, n);
        bits |= bad;
        if (!bad) {
            const int r = sample_x(sample_case_key(seed, case_offset + row), 0, n);      // step 0 reads the identity map
            item = r + seen_upto(colidx + lo, len, col_offset, r);
        }
        out[row * ld_out + off] = item;
    }
    if (bits) atomicOr(status, bits);
}

__global__ __launch_bounds__(64 * NGCF_SAMPLE_WAVES) void sample_unseen_wave_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int64_t col_offset, int64_t n_rows, int64_t n_items,
    const int64_t *__restrict__ user_ids, int64_t T, int64_t case_offset, int m, uint64_t seed, const int64_t *__restrict__ first,
    int64_t *__restrict__ out, int64_t ld_out, int32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) int sample_lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int mp = (m + 63) & ~63;
    int *Ks = sample_lds + (size_t)wave * 2 * mp, *Vs = Ks + mp;      // entries of the finished chunks (touched only when m > 64)

    for (int64_t row = (int64_t)blockIdx.x * NGCF_SAMPLE_WAVES + wave; row < T; row += (int64_t)gridDim.x * NGCF_SAMPLE_WAVES) {
        int64_t *o = out + row * ld_out;
        if (first) {
            if (lane == 0) o[0] = first[row];
            o += 1;
        }
        int64_t lo, len, n;
        const int bad = sample_row(rowptr, n_rows, n_items, user_ids[row], m, lo, len, n);     // the same in every lane
        if (bad) {
            if (lane == 0) atomicOr(status, bad);
            for (int j = lane; j < m; j += 64) o[j] = -1;
            continue;
        }
        const int32_t *seen = colidx + lo;
        const int64_t d = sample_seen_lanes(seen, len, col_offset, lane);
        const uint64_t a = sample_case_key(seed, case_offset + row);

        for (int base = 0; base < m; base += 64) {
            const int cnt = min(64, m - base);
            int K, V;
            const int R = sample_chunk(a, n, base, cnt, lane, seen, len, col_offset, d, Ks, Vs, K, V);
            if (lane < cnt) o[base + lane] = R;
            if (base + 64 < m) {
                Ks[base + lane] = K;
                Vs[base + lane] = V;
                wave_lds_sync();
            }
        }
        if (m > 64) wave_lds_sync();                                   // the next case overwrites the region
    }
}

}  // namespace

extern "C" int ngcf_sample_unseen(const int64_t *seen_rowptr, const int32_t *seen_colidx, int64_t col_offset, int64_t n_rows,
                                  int64_t n_items, const int64_t *user_ids, int64_t T, int64_t case_offset, int m, uint64_t seed,
                                  const int64_t *first, int64_t *out, int64_t ld_out, int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (m < 1 || m > NGCF_SAMPLE_M_MAX) return fail(NGCF_ERR_ARG, "sample_unseen: m=%d outside [1, %d]", m, NGCF_SAMPLE_M_MAX);
    if (int e = sample_check_items("sample_unseen", n_items)) return e;
    if (int e = sample_check_ld("sample_unseen", "ld_out", ld_out, m + (first ? 1 : 0))) return e;
    if (int e = sample_check_counts("sample_unseen", T, n_rows)) return e;
    if (T == 0) return NGCF_OK;
    if (int e = sample_check_pointers("sample_unseen", {seen_rowptr, seen_colidx, user_ids, out, status})) return e;

    if (m == 1) {
        sample_unseen_one_kernel<<<dim3((unsigned)grid_for(T, 256)), 256, 0, stream>>>(
            seen_rowptr, seen_colidx, col_offset, n_rows, n_items, user_ids, T, case_offset, seed, first, out, ld_out, status);
    } else {
        const size_t lds = m > 64 ? sizeof(int) * NGCF_SAMPLE_WAVES * 2 * (size_t)((m + 63) & ~63) : 0;      // at most 32 KiB
        sample_unseen_wave_kernel<<<dim3((unsigned)sample_blocks(T, NGCF_SAMPLE_WAVES)), 64 * NGCF_SAMPLE_WAVES, lds, stream>>>(
            seen_rowptr, seen_colidx, col_offset, n_rows, n_items, user_ids, T, case_offset, m, seed, first, out, ld_out, status);
    }
    LAUNCH_CHECK();
    return NGCF_OK;
}
