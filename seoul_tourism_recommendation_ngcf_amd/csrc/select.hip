// Exact per-group sampling: from every group g of rows mark exactly quota[g], uniformly among all subsets of that
// size - what pandas' sample(frac=) and sklearn's stratified split do to a frame (utils.py:126-148), as a radix select by group
// over keys that are never stored.
//   keys    row t has the 64-bit key fmix64(seed ^ (t * 0x9E3779B97F4A7C15)): a chain of bijections on 64-bit words, so the keys of
//           distinct rows are distinct.  There are no ties, and so there is no tie-breaking path.
//   select  eight passes, most significant byte first.  In pass p a row whose key agrees with its group's prefix in the p bytes
//           found so far counts into hist[g][byte p of the key] (pass 0: every row, so the bins of a group add up to its row count).
//           Then, per group, the bin that holds the remaining rank extends the prefix and the rows of the bins below it come off
//           the rank ("pick", its own small launch: one wave per group, which also clears the group's bins for the next pass).
//           After pass 7 the prefix is tau_g, the quota[g]-th smallest key of the group.
//   tiers   up to kSelLdsGroups groups the whole G x 256 table is a workgroup's LDS (1 KiB per group of the CU's 160 KiB): LDS
//           atomics per row, and one flush of the non-zero bins with memory atomics per workgroup - with one group every atomic of
//           the chip would otherwise land on 256 addresses.  Above that the rows add straight into the table in memory.
//   mark    mask[t] = quota[g] > 0 && key <= tau_g: exactly quota[g] rows of group g.
// Integer atomics only: counts do not depend on arrival order, and two runs give the same bytes.
// Status word (sticky, OR-ed): 1 a group id outside [0, G) (the row counts nowhere; a call that saw one marks nothing), 2 a quota
// above its group's row count (no row of that group is marked), 4 the rows changed between two passes.
#include "common.h"

namespace {

constexpr int kSelThreads = 1024;
constexpr int kSelRowsPerThread = 8;
constexpr int kSelChunk = kSelThreads * kSelRowsPerThread;      // rows of one workgroup pass
constexpr int kSelMaxBlocks = 256 * 2;                           // two workgroups of 16 waves fill a CU
constexpr int kSelBins = 256;
constexpr int kSelLdsBytes = 160 * 1024;                         // the LDS of a CU (MI355X): all of it can go to one workgroup
constexpr int kSelLdsGroups = kSelLdsBytes / (kSelBins * (int)sizeof(int32_t));   // 160: the kernel keeps nothing else in LDS
constexpr int kSelPickThreads = 256;
constexpr int kSelPickWaves = kSelPickThreads / 64;
constexpr int kSelMarkThreads = 256;
constexpr uint64_t kSelGolden = 0x9E3779B97F4A7C15ULL;

struct SelState {               // per group, between passes
    uint64_t prefix;            // the bytes of tau found so far, in place; the rest 0
    int64_t rank;               // the rank (from 1) of tau among the group's rows that agree with the prefix; 0: nothing to select
};

__device__ inline uint64_t sel_key(uint64_t seed, int64_t t) { return fmix64(seed ^ ((uint64_t)t * kSelGolden)); }

// false: an id outside [0, G)
__device__ inline bool sel_group(const int32_t *__restrict__ group, int64_t t, int64_t G, int64_t &g)
{
    g = group ? (int64_t)group[t] : 0;
    return g >= 0 && g < G;
}

// A workgroup takes the chunks blockIdx.x, blockIdx.x + gridDim.x, ... of kSelChunk rows each.  LDS: the table is s_hist, flushed
// into `hist` at the end; otherwise the rows add into `hist` directly.
template <bool LDS>
__global__ __launch_bounds__(kSelThreads) void select_hist_kernel(const int32_t *__restrict__ group, int64_t T, int64_t G, uint64_t seed, int pass,
                                                                  const SelState *__restrict__ state, int32_t *hist, int32_t *status)
{
    extern __shared__ int32_t s_hist[];                                  // G x 256 (LDS tier)
    const int tid = threadIdx.x;
    const int n_bins = LDS ? (int)G * kSelBins : 0;                      // LDS tier: G <= kSelLdsGroups
    if (LDS) {
        for (int i = tid; i < n_bins; i += kSelThreads) s_hist[i] = 0;
        __syncthreads();
    }
    const int shift = 56 - 8 * pass;
    bool bad = false;
    const int64_t n_chunks = (T + kSelChunk - 1) / kSelChunk;
    for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const int64_t base = ch * kSelChunk;
#pragma unroll
        for (int q = 0; q < kSelRowsPerThread; ++q) {
            const int64_t t = base + (int64_t)q * kSelThreads + tid;
            if (t >= T) break;
            int64_t g;
            if (!sel_group(group, t, G, g)) {
                bad = true;
                continue;
            }
            const uint64_t k = sel_key(seed, t);
            if (pass > 0) {
                const SelState st = state[g];
                if (st.rank <= 0 || ((k ^ st.prefix) >> (shift + 8)) != 0) continue;
            }
            const int64_t bin = g * kSelBins + (int64_t)((k >> shift) & 0xff);
            if (LDS) __hip_atomic_fetch_add(&s_hist[bin], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else __hip_atomic_fetch_add(&hist[bin], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = tid; i < n_bins; i += kSelThreads) {
            const int32_t c = s_hist[i];
            if (c) __hip_atomic_fetch_add(&hist[i], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (bad && pass == 0) atomicOr(status, NGCF_SELECT_GROUP);
}

// One wave per group: lane l holds bins 4l .. 4l + 3.  The lane whose running sum first reaches the rank holds the bin.
__global__ __launch_bounds__(kSelPickThreads) void select_pick_kernel(int32_t *hist, SelState *state, const int64_t *__restrict__ quota, int64_t G, int pass,
                                                                      uint64_t *__restrict__ thresholds, int32_t *status)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * kSelPickWaves + (threadIdx.x >> 6);
    if (g >= G) return;                                                  // wave-uniform
    SelState st;
    if (pass == 0) {
        st.prefix = 0;
        st.rank = quota[g];
    } else {
        st = state[g];
    }
    if (pass > 0 && st.rank <= 0) {                                      // its bins were not touched in this pass: still clear
        if (pass == 7 && thresholds && lane == 0) thresholds[g] = 0;
        return;
    }
    int4 *bins = reinterpret_cast<int4 *>(hist + g * kSelBins);
    const int4 v = bins[lane];
    bins[lane] = make_int4(0, 0, 0, 0);
    const long long s = (long long)v.x + v.y + v.z + v.w;
    long long incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    const long long total = __shfl(incl, 63);
    int flag = 0;
    if (st.rank > total) flag = pass == 0 ? NGCF_SELECT_QUOTA : NGCF_SELECT_LOST;
    if (flag || st.rank <= 0) {
        if (lane == 0) {
            state[g] = SelState{0, 0};
            if (flag) atomicOr(status, flag);
            if (pass == 7 && thresholds) thresholds[g] = 0;
        }
        return;
    }
    const unsigned long long reached = __ballot(incl >= st.rank);        // not empty: rank <= total
    if (lane == __ffsll(reached) - 1) {
        long long r = st.rank - (incl - s);                                // in [1, s]
        int j = 0;
        if (r > v.x) {
            r -= v.x;
            j = 1;
            if (r > v.y) {
                r -= v.y;
                j = 2;
                if (r > v.z) {
                    r -= v.z;
                    j = 3;
                }
            }
        }
        st.prefix |= (uint64_t)(4 * lane + j) << (56 - 8 * pass);
        st.rank = r;
        state[g] = st;
        if (pass == 7 && thresholds) thresholds[g] = st.prefix;
    }
}

__global__ __launch_bounds__(kSelMarkThreads) void select_mark_kernel(const int32_t *__restrict__ group, int64_t T, int64_t G, uint64_t seed,
                                                                      const SelState *__restrict__ state, uint8_t *__restrict__ mask,
                                                                      const int32_t *__restrict__ status)
{
    const bool none = (*status & NGCF_SELECT_GROUP) != 0;
    for (int64_t t = (int64_t)blockIdx.x * kSelMarkThreads + threadIdx.x; t < T; t += (int64_t)gridDim.x * kSelMarkThreads) {
        int64_t g;
        uint8_t m = 0;
        if (!none && sel_group(group, t, G, g)) {
            const SelState st = state[g];
            m = st.rank > 0 && sel_key(seed, t) <= st.prefix;
        }
        mask[t] = m;
    }
}

int64_t sel_workspace_bytes(int64_t G) { return G * (int64_t)(kSelBins * sizeof(int32_t) + sizeof(SelState)); }

}  // namespace

extern "C" int ngcf_select_limits(int64_t G, int *lds_groups, int64_t *workspace_bytes)
{
    if (lds_groups) *lds_groups = kSelLdsGroups;
    if (workspace_bytes) *workspace_bytes = G >= 1 && G < (1ll << 31) ? sel_workspace_bytes(G) : -1;
    return NGCF_OK;
}

extern "C" uint64_t ngcf_select_key(uint64_t seed, int64_t t) { return fmix64(seed ^ ((uint64_t)t * kSelGolden)); }

extern "C" int ngcf_select_per_group(const int32_t *group, int64_t T, int64_t G, const int64_t *quota, uint64_t seed, uint8_t *mask,
                                     uint64_t *thresholds, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (T < 0 || T >= (1ll << 31)) return fail(NGCF_ERR_ARG, "select: T=%lld outside [0, 2^31) (the bins are int32)", (long long)T);
    if (G < 1 || G >= (1ll << 31)) return fail(NGCF_ERR_ARG, "select: G=%lld outside [1, 2^31)", (long long)G);
    if (!group && G != 1 && T > 0) return fail(NGCF_ERR_ARG, "select: no group vector stands for one group, G=%lld", (long long)G);
    if (!quota || !status || !workspace || (T > 0 && !mask)) return fail(NGCF_ERR_ARG, "select: null argument");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(NGCF_ERR_ARG, "select: the workspace is not 16-byte aligned");
    if (workspace_bytes < sel_workspace_bytes(G))
        return fail(NGCF_ERR_WORKSPACE, "select: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)sel_workspace_bytes(G));
    int32_t *hist = static_cast<int32_t *>(workspace);
    SelState *state = reinterpret_cast<SelState *>(hist + G * kSelBins);
    HIP_TRY(hipMemsetAsync(hist, 0, (size_t)G * kSelBins * sizeof(int32_t), stream));
    const bool lds = G <= kSelLdsGroups && !ngcf_opts().select_no_lds;
    const size_t lds_bytes = lds ? (size_t)G * kSelBins * sizeof(int32_t) : 0;
    if (lds) HIP_TRY(allow_full_lds<select_hist_kernel<true>>(kSelLdsBytes));
    const int64_t n_chunks = (T + kSelChunk - 1) / kSelChunk;
    const dim3 hist_grid((unsigned)std::min<int64_t>(n_chunks, kSelMaxBlocks)), pick_grid((unsigned)((G + kSelPickWaves - 1) / kSelPickWaves));
    for (int pass = 0; pass < 8; ++pass) {
        if (T > 0) {
            if (lds) select_hist_kernel<true><<<hist_grid, kSelThreads, lds_bytes, stream>>>(group, T, G, seed, pass, state, hist, status);
            else select_hist_kernel<false><<<hist_grid, kSelThreads, 0, stream>>>(group, T, G, seed, pass, state, hist, status);
            LAUNCH_CHECK();
        }
        select_pick_kernel<<<pick_grid, kSelPickThreads, 0, stream>>>(hist, state, quota, G, pass, thresholds, status);
        LAUNCH_CHECK();
    }
    if (T == 0) return NGCF_OK;
    select_mark_kernel<<<dim3(grid_for(T, kSelMarkThreads)), kSelMarkThreads, 0, stream>>>(group, T, G, seed, state, mask, status);
    LAUNCH_CHECK();
    return NGCF_OK;
}
