// What the samplers share (sample.hip, sample_hard.hip, sample_weighted.hip).  Device side: the building blocks of
// the unseen-item draw, the recipe of ngcf_sample_unseen in include/ngcf_hip.h, defined once so that every kernel that draws gives
// the same items.  Host side, at the end: the argument checks the entry points state in the same words, and the cap of their grids.
#ifndef NGCF_SAMPLE_DEVICE_H
#define NGCF_SAMPLE_DEVICE_H

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
// ---------------------------------------------------------------------------------------------
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

// A seen row of up to 64 ids in the lanes: c_lane - lane, INT64_MAX in the lanes past the row (they never count) and in every lane
// of a longer row, which is searched where it lies instead
__device__ inline int64_t sample_seen_lanes(const int32_t *__restrict__ seen, int64_t len, int64_t col_offset, int lane)
{
    return len <= 64 && lane < len ? (int64_t)seen[lane] - col_offset - lane : INT64_MAX;
}

// Steps base .. base + cnt - 1 (cnt <= 64) of the case with key `a`, by the whole wave: lane jj < cnt returns the item of slot
// base + jj (the other lanes 0) and leaves in (K, V) its entry of the map, the key -1 in the lanes past cnt.  `d` is
// sample_seen_lanes' value.  Ks / Vs [base]: the entries of the steps before `base`, in the wave's LDS (never touched when base
// is 0: a draw of up to 64 items passes null pointers).
__device__ inline int sample_chunk(uint64_t a, int64_t n, int base, int cnt, int lane, const int32_t *__restrict__ seen, int64_t len,
                                   int64_t col_offset, int64_t d, const int *Ks, const int *Vs, int &K, int &V)
{
    const bool in_lanes = len <= 64;
    K = lane < cnt ? sample_x(a, base + lane, n) : -1;               // keys are >= 0: -1 matches nothing
    V = 0;
    int R = 0;
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
    if (lane < cnt && !in_lanes) R += seen_upto(seen, len, col_offset, R);
    return R;
}

// ---------------------------------------------------------------------------------------------
// Host side.  Every entry point checks its own limit of m first, then calls these in the order below, its own checks in between;
// `entry` is the name its messages carry.  Nothing to do (no cases) is decided by the entry point, before the pointers are looked at.
// ---------------------------------------------------------------------------------------------
#define NGCF_SAMPLE_BLOCKS_MAX 2048       // workgroups of a launch: 8 per CU, the most that stay resident; more cases are strided

// the grid of a kernel that gives every wave of its `waves`-wave workgroups one case at a time
inline int sample_blocks(int64_t cases, int waves) { return (int)std::min<int64_t>((cases + waves - 1) / waves, NGCF_SAMPLE_BLOCKS_MAX); }

inline int sample_check_items(const char *entry, int64_t n_items)
{
    if (n_items < 1 || n_items >= (int64_t)1 << 31) return fail(NGCF_ERR_ARG, "%s: n_items=%lld outside [1, 2^31)", entry, (long long)n_items);
    return NGCF_OK;
}

// the leading dimension `ld` (named `what`) of an array that takes `width` columns per case
inline int sample_check_ld(const char *entry, const char *what, int64_t ld, int width)
{
    if (ld < width) return fail(NGCF_ERR_ARG, "%s: %s=%lld is below the %d columns of a row", entry, what, (long long)ld, width);
    return NGCF_OK;
}

inline int sample_check_counts(const char *entry, int64_t cases, int64_t n_rows)
{
    if (cases < 0 || n_rows < 0) return fail(NGCF_ERR_ARG, "%s: bad argument", entry);
    return NGCF_OK;
}

inline int sample_check_pointers(const char *entry, std::initializer_list<const void *> required)
{
    for (const void *p : required)
        if (!p) return fail(NGCF_ERR_ARG, "%s: null argument", entry);
    return NGCF_OK;
}

}  // namespace

#endif  // NGCF_SAMPLE_DEVICE_H
