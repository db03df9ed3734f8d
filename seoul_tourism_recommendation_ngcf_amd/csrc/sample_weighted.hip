// Popularity-weighted negatives: for T cases in one launch, m distinct items the case's user has no stored interaction with, drawn
// in proportion to an integer weight per item - successive sampling, np.random.choice(p=w/sum, replace=False) - and the weight of
// every drawn item with the user's unseen weight, from which the proposal probability follows exactly.  Every
// output value is a pure function of (seed, global case number, the user's seen row, the weights); the recipe is written out in
// include/ngcf_hip.h.
#include "sample_device.h"

// ---------------------------------------------------------------------------------------------
// Coordinates.  cdf[i] is the weight below item i.  A user's seen items c_0 < c_1 < .. cut their own weight out of that line: what is
// left, U = mass[u] long, is the user's unseen coordinate, and gap_k = cdf[c_k] - S_k (S_k: the weight of the seen items before
// c_k) is where c_k would stand in it.  A point r of the unseen coordinate lies above K = #{k : gap_k <= r} seen items, so it is
// the point r + S_K of the cdf line: one search of the user's gap row, one of cdf.  A drawn item is an interval (q, w) of the unseen
// coordinate; step j draws its point in [0, U_j), the coordinate with the drawn intervals cut out, and steps over them: interval i
// starts at e_i = q_i - (widths drawn below q_i) there, and every interval with e_i <= r' lies below the point.
//
// Mapping.  m == 1: a lane per case, two binary searches, no interval.  m > 1: a wave per case; lane i keeps interval i as
// (q, w, e) - an insert lowers e in the lanes with a larger q by its width -, the two sums over the intervals are butterflies, and
// both searches take 64 probes a round, one per lane (a 100 K-item cdf: 3 rounds where a lane alone takes 17).  A seen row of up
// to 64 entries sits in the lanes as (gap_k, S_k): its search is a ballot.  cdf is read where it lies: 800 KB at 100 K items, L2.
// ---------------------------------------------------------------------------------------------
#define NGCF_SAMPLE_WEIGHTED_WAVES 4

namespace {

constexpr uint64_t kNoInterval = ~0ull;          // e of a lane that holds no interval, gap of a lane past the row: above every point

__device__ inline uint64_t shfl_u64(uint64_t x, int src) { return (uint64_t)shfl_i64((int64_t)x, src); }

__device__ inline uint64_t shfl_up_u64(uint64_t x, int d)
{
    const uint32_t lo = __shfl_up((uint32_t)x, d), hi = __shfl_up((uint32_t)(x >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

__device__ inline uint64_t wave_sum_u64(uint64_t x)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += shfl_xor_u64(x, s);
    return x;
}

// #{k < n : a[k] <= x} of a non-decreasing, non-negative array: a lane on its own
__device__ inline int64_t count_le_lane(const int64_t *__restrict__ a, int64_t n, uint64_t x)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((uint64_t)a[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// .. and the whole wave for one (a, n, x), the same in every lane: lane l probes the end of the l-th of 64 pieces of [lo, hi); the
// probes that pass are a prefix of the lanes, so their count moves lo and the first that fails becomes hi
__device__ inline int64_t count_le_wave(const int64_t *__restrict__ a, int64_t n, uint64_t x, int lane)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t step = (hi - lo + 63) >> 6;
        const int64_t p = lo + (int64_t)(lane + 1) * step - 1;
        const int cnt = __popcll(__ballot(p < hi && (uint64_t)a[p] <= x));
        const int64_t failed = lo + (int64_t)(cnt + 1) * step - 1;
        lo += (int64_t)cnt * step;                       // <= hi: the last probe that passed lies below hi
        hi = failed < hi ? failed : hi;
    }
    return lo;
}

// a stored id as an index into cdf[0 .. n_items]: ngcf_weighted_prepare flags an id outside the catalogue, nothing reads through one
__device__ inline int64_t cdf_index(int64_t c, int64_t n_items) { return c < 0 ? 0 : (c > n_items ? n_items : c); }

// the item whose interval holds the point tgt of the cdf line: the largest i with cdf[i] <= tgt (cdf[0] = 0 <= tgt < cdf[n_items])
__device__ inline int64_t item_index(int64_t count_le, int64_t n_items)
{
    const int64_t c = count_le - 1;
    return c < 0 ? 0 : (c >= n_items ? n_items - 1 : c);
}

// One wave per seen row, 64 entries at a time with a carried prefix: gap_k = cdf[c_k] - S_k, mass[u] = W - S_len.  Integer adds only.
__global__ __launch_bounds__(64 * NGCF_SAMPLE_WEIGHTED_WAVES) void weighted_prepare_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int64_t col_offset, int64_t n_rows, int64_t n_items,
    const int64_t *__restrict__ cdf, int64_t *__restrict__ gap, int64_t *__restrict__ mass, int32_t *status)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t W = (uint64_t)cdf[n_items];
    int bits = 0;
    for (int64_t u = (int64_t)blockIdx.x * NGCF_SAMPLE_WEIGHTED_WAVES + wave; u < n_rows;
         u += (int64_t)gridDim.x * NGCF_SAMPLE_WEIGHTED_WAVES) {
        const int64_t lo = rowptr[u], len = rowptr[u + 1] - lo;
        uint64_t carry = 0;                                          // S at the chunk's first entry
        for (int64_t base = 0; base < len; base += 64) {
            const int64_t k = base + lane;
            const bool in_row = k < len;
            const int64_t c = in_row ? (int64_t)colidx[lo + k] - col_offset : 0;
            const bool in_catalogue = c >= 0 && c < n_items;
            if (!in_catalogue) bits = 4;
            const int64_t ci = in_catalogue ? c : 0;
            const uint64_t below = (uint64_t)cdf[ci];
            const uint64_t w = in_row && in_catalogue ? (uint64_t)cdf[ci + 1] - below : 0;
            uint64_t incl = w;                                       // the weights up to and with this lane's entry
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint64_t up = shfl_up_u64(incl, d);
                if (lane >= d) incl += up;
            }
            if (in_row) gap[lo + k] = (int64_t)(below - (carry + incl - w));
            carry += shfl_u64(incl, 63);
        }
        if (lane == 0) mass[u] = (int64_t)(W - carry);
    }
    if (bits) atomicOr(status, bits);
}

__global__ __launch_bounds__(256) void sample_weighted_one_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int64_t col_offset, int64_t n_rows, int64_t n_items,
    const int64_t *__restrict__ cdf, const int64_t *__restrict__ gap, const int64_t *__restrict__ mass,
    const int64_t *__restrict__ user_ids, int64_t T, int64_t case_offset, uint64_t seed, int64_t *__restrict__ out, int64_t ld_out,
    int64_t *__restrict__ draw_weight, int64_t ld_weight, int64_t *__restrict__ case_mass, int32_t *status)
{
    const uint64_t W = (uint64_t)cdf[n_items];
    int bits = 0;
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < T; row += (int64_t)gridDim.x * 256) {
        const int64_t u = user_ids[row];
        int64_t item = -1;
        uint64_t w = 0, U = 0;
        if (u < 0 || u >= n_rows) {
            bits |= 1;
        } else if ((U = (uint64_t)mass[u]) == 0) {
            bits |= 2;
        } else {
            const int64_t lo = rowptr[u], len = rowptr[u + 1] - lo;
            const uint64_t r = __umul64hi(fmix64(sample_case_key(seed, case_offset + row) + kSampleStep), U);
            const int64_t K = count_le_lane(gap + lo, len, r);
            const uint64_t S = K < len ? (uint64_t)cdf[cdf_index((int64_t)colidx[lo + K] - col_offset, n_items)] - (uint64_t)gap[lo + K] : W - U;
            item = item_index(count_le_lane(cdf, n_items + 1, r + S), n_items);
            w = (uint64_t)cdf[item + 1] - (uint64_t)cdf[item];
        }
        out[row * ld_out] = item;
        if (draw_weight) draw_weight[row * ld_weight] = (int64_t)w;
        if (case_mass) case_mass[row] = (int64_t)U;
    }
    if (bits) atomicOr(status, bits);
}

__global__ __launch_bounds__(64 * NGCF_SAMPLE_WEIGHTED_WAVES) void sample_weighted_wave_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int64_t col_offset, int64_t n_rows, int64_t n_items,
    const int64_t *__restrict__ cdf, const int64_t *__restrict__ gap, const int64_t *__restrict__ mass,
    const int64_t *__restrict__ user_ids, int64_t T, int64_t case_offset, int m, uint64_t seed, int64_t *__restrict__ out,
    int64_t ld_out, int64_t *__restrict__ draw_weight, int64_t ld_weight, int64_t *__restrict__ case_mass, int32_t *status)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t W = (uint64_t)cdf[n_items];
    for (int64_t row = (int64_t)blockIdx.x * NGCF_SAMPLE_WEIGHTED_WAVES + wave; row < T;
         row += (int64_t)gridDim.x * NGCF_SAMPLE_WEIGHTED_WAVES) {
        const int64_t u = user_ids[row];                                  // the same in every lane, as is all that follows from it
        int64_t item = -1;
        uint64_t width = 0, U = 0;
        int bad = 0;
        if (u < 0 || u >= n_rows) {
            bad = 1;
        } else if ((U = (uint64_t)mass[u]) == 0) {
            bad = 2;
        } else {
            const int64_t lo = rowptr[u], len = rowptr[u + 1] - lo;
            const int32_t *seen = colidx + lo;
            const int64_t *grow = gap + lo;
            const bool in_lanes = len <= 64;
            // a row of up to 64 entries, one per lane: (gap_k, S_k)
            const bool holds = in_lanes && lane < len;
            const uint64_t g = holds ? (uint64_t)grow[lane] : kNoInterval;
            const uint64_t s = holds ? (uint64_t)cdf[cdf_index((int64_t)seen[lane] - col_offset, n_items)] - g : 0;

            const uint64_t a = sample_case_key(seed, case_offset + row);
            uint64_t q = 0, e = kNoInterval, Uj = U;                        // lane i < j: interval i
            for (int j = 0; j < m; ++j) {
                if (Uj == 0) {
                    bad = 2;
                    break;
                }
                const uint64_t rp = __umul64hi(fmix64(a + (uint64_t)(j + 1) * kSampleStep), Uj);
                const uint64_t r = rp + wave_sum_u64(e <= rp ? width : 0);
                const int64_t K = in_lanes ? (int64_t)__popcll(__ballot(g <= r)) : count_le_wave(grow, len, r, lane);
                uint64_t S = W - U;
                if (K < len) S = in_lanes ? shfl_u64(s, (int)K) : (uint64_t)cdf[cdf_index((int64_t)seen[K] - col_offset, n_items)] - (uint64_t)grow[K];
                const int64_t c = item_index(count_le_wave(cdf, n_items + 1, r + S, lane), n_items);
                const uint64_t below = (uint64_t)cdf[c], cw = (uint64_t)cdf[c + 1] - below, cq = below - S;
                const uint64_t drawn_below = wave_sum_u64(e != kNoInterval && q < cq ? width : 0);
                if (e != kNoInterval && q > cq) e -= cw;
                if (lane == j) {
                    q = cq;
                    width = cw;
                    e = cq - drawn_below;
                    item = c;
                }
                Uj -= cw;
            }
        }
        if (bad && lane == 0) atomicOr(status, bad);
        if (lane < m) {
            out[row * ld_out + lane] = bad ? -1 : item;
            if (draw_weight) draw_weight[row * ld_weight + lane] = bad ? 0 : (int64_t)width;
        }
        if (case_mass && lane == 0) case_mass[row] = (int64_t)U;
    }
}

}  // namespace

extern "C" int ngcf_weighted_prepare(const int64_t *seen_rowptr, const int32_t *seen_colidx, int64_t col_offset, int64_t n_rows,
                                     int64_t n_items, const int64_t *cdf, int64_t *gap, int64_t *mass, int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int e = sample_check_items("weighted_prepare", n_items)) return e;
    if (int e = sample_check_counts("weighted_prepare", n_rows, n_rows)) return e;      // its cases are the rows
    if (n_rows == 0) return NGCF_OK;
    if (int e = sample_check_pointers("weighted_prepare", {seen_rowptr, seen_colidx, cdf, gap, mass, status})) return e;
    weighted_prepare_kernel<<<dim3((unsigned)sample_blocks(n_rows, NGCF_SAMPLE_WEIGHTED_WAVES)), 64 * NGCF_SAMPLE_WEIGHTED_WAVES, 0, stream>>>(
        seen_rowptr, seen_colidx, col_offset, n_rows, n_items, cdf, gap, mass, status);
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_sample_weighted(const int64_t *seen_rowptr, const int32_t *seen_colidx, int64_t col_offset, int64_t n_rows,
                                    int64_t n_items, const int64_t *cdf, const int64_t *gap, const int64_t *mass,
                                    const int64_t *user_ids, int64_t T, int64_t case_offset, int m, uint64_t seed, int64_t *out,
                                    int64_t ld_out, int64_t *draw_weight, int64_t ld_weight, int64_t *case_mass, int32_t *status,
                                    void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (m < 1 || m > NGCF_SAMPLE_WEIGHTED_M_MAX)
        return fail(NGCF_ERR_ARG, "sample_weighted: m=%d outside [1, %d]", m, NGCF_SAMPLE_WEIGHTED_M_MAX);
    if (int e = sample_check_items("sample_weighted", n_items)) return e;
    if (int e = sample_check_ld("sample_weighted", "ld_out", ld_out, m)) return e;
    if (draw_weight)
        if (int e = sample_check_ld("sample_weighted", "ld_weight", ld_weight, m)) return e;
    if (int e = sample_check_counts("sample_weighted", T, n_rows)) return e;
    if (T == 0) return NGCF_OK;
    if (int e = sample_check_pointers("sample_weighted", {seen_rowptr, seen_colidx, cdf, gap, mass, user_ids, out, status})) return e;

    if (m == 1) {
        sample_weighted_one_kernel<<<dim3((unsigned)grid_for(T, 256)), 256, 0, stream>>>(
            seen_rowptr, seen_colidx, col_offset, n_rows, n_items, cdf, gap, mass, user_ids, T, case_offset, seed, out, ld_out,
            draw_weight, ld_weight, case_mass, status);
    } else {
        sample_weighted_wave_kernel<<<dim3((unsigned)sample_blocks(T, NGCF_SAMPLE_WEIGHTED_WAVES)), 64 * NGCF_SAMPLE_WEIGHTED_WAVES, 0, stream>>>(
            seen_rowptr, seen_colidx, col_offset, n_rows, n_items, cdf, gap, mass, user_ids, T, case_offset, m, seed, out, ld_out,
            draw_weight, ld_weight, case_mass, status);
    }
    LAUNCH_CHECK();
    return NGCF_OK;
}
