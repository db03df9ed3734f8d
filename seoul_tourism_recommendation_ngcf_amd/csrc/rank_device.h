// What the full-catalogue ranking kernels share (rank.hip, rank_position.hip, rank_prefilter.hip; the sums and their host tail
// list_quality.hip too),
// defined once so that every kernel that orders, splits, searches or sums does it the same way.
#ifndef NGCF_RANK_DEVICE_H
#define NGCF_RANK_DEVICE_H

#include "common.h"

// ---------------------------------------------------------------------------------------------
// Pair order.  A score's key is float_key (common.h); the output order of (key, item) pairs is key descending, then item ascending.
// rank_positions counts what rank_topk lists, so both take the order from pair_before() and the padding from kPadKey / kPadIdx.
//
// Item split.  Both scoring kernels walk item tiles of kRankIT = 128 items, K in chunks of kRankTK = 32, and cut the item range by
// rank_item_split() when the row tiles alone are too few workgroups.
//
// Sums.  Per-workgroup fp64 partials are added by ONE thread per slot, blocks in ascending order: bit-identical from run to run.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr int kRankIT = 128, kRankTK = 32;      // items of a tile, columns of a K chunk

constexpr uint32_t kPadKey = 0u;                // below every score key but the one NaN pattern 0xffffffff (which ties it)
constexpr int32_t kPadIdx = 0x7fffffff;         // ... and then loses on the item index: padding sorts after every pair of a real item

__device__ inline float float_unkey(uint32_t k)   // the inverse of float_key
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ inline bool pair_before(uint32_t ka, int32_t ia, uint32_t kb, int32_t ib)   // a precedes b: key descending, item ascending
{
    return ka > kb || (ka == kb && ia < ib);
}

// Is item id `c` in the ascending row [lo, end) of a CSR whose columns carry the offset `off`?  (A lower bound, then one compare.)
__device__ inline bool row_has(const int32_t *__restrict__ colidx, int64_t lo, int64_t end, int64_t off, int64_t c)
{
    int64_t hi = end;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)colidx[mid] - off < c) lo = mid + 1; else hi = mid;
    }
    return lo < end && (int64_t)colidx[lo] - off == c;
}

// The item split of a ranking launch: enough workgroups for two per CU - the item range is cut (in whole tiles, >= 16 x 128 items a
// piece) when the user tiles alone are too few.
struct ItemSplit {
    int64_t splits, split_items;
};

inline ItemSplit rank_item_split(int64_t user_tiles, int64_t n_items)
{
    const int64_t want = (512 + user_tiles - 1) / user_tiles;
    const int64_t max_splits = std::max<int64_t>(1, n_items / (16 * kRankIT));
    const int64_t s = std::max<int64_t>(1, std::min(want, max_splits));
    const int64_t tiles = (n_items + kRankIT - 1) / kRankIT;
    ItemSplit p;
    p.split_items = (tiles + s - 1) / s * kRankIT;
    p.splits = (n_items + p.split_items - 1) / p.split_items;
    return p;
}

// ---------------------------------------------------------------------------------------------
// Streaming selection (rank.hip, rank_prefilter.hip): a user's LDS buffer of CAPP (key, item) pairs, a count and a threshold = the
// current k-th best pair; a pair enters only if it beats the threshold, a buffer that could overflow is compacted.
// ---------------------------------------------------------------------------------------------
// Compaction of the users listed in flist[0..nf): sort each one's CAPP pairs (positions >= count hold padding), keep the best k,
// pad the rest, set the threshold.  All threads of the workgroup take part; one barrier per bitonic stage.
template <int CAPP>
__device__ void rank_compact(uint32_t *bk, int32_t *bi, uint32_t *cnt, uint32_t *thk, int32_t *thi, const int *flist, int nf, int k)
{
    const int half = CAPP / 2;
    const int n_pairs = nf * half;
    for (int size = 2; size <= CAPP; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int p = threadIdx.x; p < n_pairs; p += blockDim.x) {
                const int u = flist[p / half], q = p % half;
                const int a = (q / stride) * (2 * stride) + (q % stride), b = a + stride;
                uint32_t *K = bk + u * CAPP;
                int32_t *I = bi + u * CAPP;
                const bool desc = (a & size) == 0;
                const uint32_t ka = K[a], kb = K[b];
                const int32_t ia = I[a], ib = I[b];
                if (pair_before(ka, ia, kb, ib) != desc) {
                    K[a] = kb; K[b] = ka;
                    I[a] = ib; I[b] = ia;
                }
            }
            __syncthreads();
        }
    }
    for (int p = threadIdx.x; p < nf * CAPP; p += blockDim.x) {
        const int u = flist[p / CAPP], pos = p % CAPP;
        if (pos >= k) {
            bk[u * CAPP + pos] = kPadKey;
            bi[u * CAPP + pos] = kPadIdx;
        }
    }
    for (int j = threadIdx.x; j < nf; j += blockDim.x) {
        const int u = flist[j];
        if (cnt[u] >= (uint32_t)k) {
            cnt[u] = (uint32_t)k;
            thk[u] = bk[u * CAPP + k - 1];
            thi[u] = bi[u * CAPP + k - 1];
        }
    }
    __syncthreads();
}

// Batch row b -> user row r (user_ids may be NULL); -1 past the batch, -2 out of range (status set by the caller's rule).
__device__ inline int64_t rank_user(const int64_t *user_ids, int64_t b, int64_t B, int64_t n_user_rows)
{
    if (b >= B) return -1;
    const int64_t r = user_ids ? user_ids[b] : b;
    return (r < 0 || r >= n_user_rows) ? -2 : r;
}

// Merge of the per-split lists of one batch row (item splits ascending): the same threshold / buffer / compaction, 256 pairs a round;
// out(b, j, has, key, item) writes slot j < k of the merged list (rank.hip: values and items; rank_prefilter.hip: items and threshold).
template <typename Out>
__global__ __launch_bounds__(256) void rank_merge_kernel(const uint32_t *__restrict__ part_key, const int32_t *__restrict__ part_idx,
                                                         int n_splits, int64_t B, int k, const int64_t *__restrict__ user_ids,
                                                         int64_t n_user_rows, Out out)
{
    constexpr int CAPP = 512, ROUND = 256;
    __shared__ uint32_t bk[CAPP];
    __shared__ int32_t bi[CAPP];
    __shared__ uint32_t cnt[1], thk[1];
    __shared__ int32_t thi[1];
    __shared__ int flist[1];
    const int64_t b = blockIdx.x;
    if (rank_user(user_ids, b, B, n_user_rows) < 0) return;  // status was set by the ranking launch
    const int tid = threadIdx.x;
    for (int p = tid; p < CAPP; p += 256) {
        bk[p] = kPadKey;
        bi[p] = kPadIdx;
    }
    if (tid == 0) {
        cnt[0] = 0;
        thk[0] = kPadKey;
        thi[0] = kPadIdx;
        flist[0] = 0;
    }
    __syncthreads();
    const int64_t total = (int64_t)n_splits * k;
    for (int64_t r0 = 0; r0 < total; r0 += ROUND) {
        const int64_t p = r0 + tid;
        if (p < total) {
            const int64_t o = ((p / k) * B + b) * k + p % k;
            const uint32_t key = part_key[o];
            const int32_t idx = part_idx[o];
            if (pair_before(key, idx, thk[0], thi[0])) {
                const uint32_t pos = atomicAdd(&cnt[0], 1u);
                bk[pos] = key;
                bi[pos] = idx;
            }
        }
        __syncthreads();
        if (r0 + ROUND >= total || cnt[0] > (uint32_t)(CAPP - ROUND)) rank_compact<CAPP>(bk, bi, cnt, thk, thi, flist, 1, k);
    }
    for (int j = tid; j < k; j += 256) {
        const bool has = j < (int)cnt[0];
        out(b, j, has, bk[j], bi[j]);
    }
}

// sums[s] += part[0][s] + part[1][s] + ..: one thread per slot, the workgroups' partials in ascending order
__global__ __launch_bounds__(64) void sum_partials_kernel(const double *__restrict__ part, int64_t n_blocks, int n_slots,
                                                          double *__restrict__ sums)
{
#pragma clang fp contract(off) reassociate(off)
    const int s = threadIdx.x;
    if (s >= n_slots) return;
    double a = 0.0;
    for (int64_t blk = 0; blk < n_blocks; ++blk) a += part[blk * n_slots + s];
    sums[s] += a;
}

// n_blocks x n_slots (<= 64) partials allocated on the stream, launch(part) fills them, sum_partials_kernel adds them into `sums`,
// the partials are freed on the stream; `who` names the entry point in the error text.
template <typename Launch>
int launch_with_partial_sums(const char *who, int64_t n_blocks, int n_slots, double *sums, hipStream_t stream, Launch launch)
{
    void *part = nullptr;
    HIP_TRY(hipMallocAsync(&part, sizeof(double) * (size_t)(n_blocks * n_slots), stream));
    launch(static_cast<double *>(part));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        sum_partials_kernel<<<1, 64, 0, stream>>>(static_cast<double *>(part), n_blocks, n_slots, sums);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(part, stream);
    if (e != hipSuccess) return fail(NGCF_ERR_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    return NGCF_OK;
}

}  // namespace

#endif  // NGCF_RANK_DEVICE_H
