// Unseen items per case, the reference's TourDataset._negative_sampling (utils.py:213-275) for T cases in one launch: m items the
// case's user has no stored interaction with, uniform and without replacement - 1 for a training triplet, 24 for a test candidate
// list.  Every output value is a pure function of (seed, global case number, the user's seen row).
#include "common.h"

// ---------------------------------------------------------------------------------------------
// The draw.  a = fmix64(seed ^ t * GOLDEN) for global case t; step j = 0 .. m-1 of a partial Fisher-Yates shuffle over the n unseen
// ranks takes x_j = j + mulhi64(fmix64(a + (j + 1) * STEP), n - j) and reads r_j = map(x_j), then sets map(x_j) = map(j), on a map
// that starts as the identity.  Only the entries set so far are stored: entry i = (key x_i, value map(i) at step i), and map(y) at
// step j is the value of the LATEST entry i < j with x_i == y, else y.  The keys do not depend on the map, so a wave computes 64 of
// them at once, one per lane; the values are resolved step by step with a compare and a ballot over the lanes.
//
// Rank r becomes the r-th item (ascending, from 0) outside the user's seen row c_0 < c_1 < ..: r + #{k : c_k - k <= r}; c_k - k does
// not decrease with k.  A row of up to 64 ids is held one per lane (ballot + popcount per step), a longer one is searched where it
// lies, every lane for its own rank.
//
// Mapping.  m == 1 (training triplets): a lane per case, no map.  m > 1: a wave per case, 64 steps per chunk; the entries of the
// chunk in work live in the lanes, those of earlier chunks (m > 64 only) in the wave's LDS region [2][round_up(m, 64)].
// ---------------------------------------------------------------------------------------------
#define NGCF_SAMPLE_M_MAX 1023
#define NGCF_SAMPLE_WAVES 4

namespace {

constexpr uint64_t kSampleGolden = 0x9E3779B97F4A7C15ULL, kSampleStep = 0xD1B54A32D192ED03ULL;

__device__ inline uint64_t sample_case_key(uint64_t seed, int64_t t) { return fmix64(seed ^ ((uint64_t)t * kSampleGolden)); }

// x_j of the case with key a: a position in [j, n)
__device__ inline int sample_x(uint64_t a, int j, int64_t n)
{
    return j + (int)__umul64hi(fmix64(a + (uint64_t)(j + 1) * kSampleStep), (uint64_t)(n - j));
}

// #{k : c_k - k <= r} of a seen row of `len` ascending ids (stored with col_offset added): the first k with c_k - k > r
__device__ inline int seen_upto(const int32_t *__restrict__ row, int64_t len, int64_t col_offset, int r)
{
    int64_t lo = 0, hi = len;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)row[mid] - col_offset - mid <= r) lo = mid + 1;
        else hi = mid;
    }
    return (int)lo;
}

__device__ inline int wave_max(int x)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x = max(x, __shfl_xor(x, s));
    return x;
}

// user id -> its seen row and the number n of its unseen items; the status bits of a case that draws nothing (0: it draws)
__device__ inline int sample_row(const int64_t *__restrict__ rowptr, int64_t n_rows, int64_t n_items, int64_t u, int m, int64_t &lo,
                                 int64_t &len, int64_t &n)
{
    lo = len = n = 0;
    if (u < 0 || u >= n_rows) return 1;
    lo = rowptr[u];
    len = rowptr[u + 1] - lo;
    n = n_items - len;
    return n < m ? 2 : 0;
}

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
        const bool in_lanes = len <= 64;
        int64_t d = INT64_MAX;                                         // c_lane - lane; lanes past the row never count
        if (in_lanes && lane < len) d = (int64_t)seen[lane] - col_offset - lane;
        const uint64_t a = sample_case_key(seed, case_offset + row);

        for (int base = 0; base < m; base += 64) {
            const int cnt = min(64, m - base);
            const int K = lane < cnt ? sample_x(a, base + lane, n) : -1;        // keys are >= 0: -1 matches nothing
            int V = 0, R = 0;
            for (int jj = 0; jj < cnt; ++jj) {
                const int j = base + jj;
                const int xj = __builtin_amdgcn_readlane(K, jj);
                int ex = -1, ej = -1;                                            // latest entry of an earlier chunk with key x_j / j
                for (int i = lane; i < base; i += 64) {
                    const int k = Ks[i];
                    ex = k == xj ? i : ex;
                    ej = k == j ? i : ej;
                }
                const uint64_t earlier = (1ull << jj) - 1;                       // the chunk's entries set so far
                const uint64_t mx = __ballot(K == xj) & earlier, mj = __ballot(K == j) & earlier;
                int r = xj, v = j;
                if (mx) r = __builtin_amdgcn_readlane(V, 63 - __clzll(mx));
                else if (base && __any(ex >= 0)) r = Vs[wave_max(ex)];
                if (mj) v = __builtin_amdgcn_readlane(V, 63 - __clzll(mj));
                else if (base && __any(ej >= 0)) v = Vs[wave_max(ej)];
                if (in_lanes) r += __popcll(__ballot(d <= (int64_t)r));
                if (lane == jj) {
                    V = v;
                    R = r;
                }
            }
            if (lane < cnt) {
                if (!in_lanes) R += seen_upto(seen, len, col_offset, R);
                o[base + lane] = R;
            }
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
    if (n_items < 1 || n_items >= (int64_t)1 << 31)
        return fail(NGCF_ERR_ARG, "sample_unseen: n_items=%lld outside [1, 2^31)", (long long)n_items);
    if (ld_out < m + (first ? 1 : 0))
        return fail(NGCF_ERR_ARG, "sample_unseen: ld_out=%lld is below the %d columns of a row", (long long)ld_out, m + (first ? 1 : 0));
    if (T < 0 || n_rows < 0) return fail(NGCF_ERR_ARG, "sample_unseen: bad argument");
    if (T == 0) return NGCF_OK;
    if (!seen_rowptr || !seen_colidx || !user_ids || !out || !status) return fail(NGCF_ERR_ARG, "sample_unseen: null argument");

    if (m == 1) {
        sample_unseen_one_kernel<<<dim3((unsigned)grid_for(T, 256)), 256, 0, stream>>>(
            seen_rowptr, seen_colidx, col_offset, n_rows, n_items, user_ids, T, case_offset, seed, first, out, ld_out, status);
    } else {
        const size_t lds = m > 64 ? sizeof(int) * NGCF_SAMPLE_WAVES * 2 * (size_t)((m + 63) & ~63) : 0;      // at most 32 KiB
        const int blocks = (int)std::min<int64_t>((T + NGCF_SAMPLE_WAVES - 1) / NGCF_SAMPLE_WAVES, 256 * 8);
        sample_unseen_wave_kernel<<<dim3((unsigned)blocks), 64 * NGCF_SAMPLE_WAVES, lds, stream>>>(
            seen_rowptr, seen_colidx, col_offset, n_rows, n_items, user_ids, T, case_offset, m, seed, first, out, ld_out, status);
    }
    LAUNCH_CHECK();
    return NGCF_OK;
}
