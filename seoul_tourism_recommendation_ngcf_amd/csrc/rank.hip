// Full-catalogue ranking: score every item for every user with fp32 MFMA and keep a streaming top-k per user, never writing the
// score matrix.  Plus the held-out metrics of the NGCF protocol (Recall / NDCG / precision / hit rate @K) on the device.
// The (key, item) order, the item split, the row search and the fixed-order sums are rank_device.h's, which rank_position.hip
// shares; the score-tile walk below is restated in pos_scan_kernel there, and why, in DESIGN 4.3.15.
#include "rank_device.h"

// ---------------------------------------------------------------------------------------------
// Tiling.  A workgroup = 4 waves owns UT = 32*UB user rows and walks its item range in tiles of IT = 128 items; wave w computes
// items [32w, 32w+32) of a tile against all UT users: UB accumulators of v_mfma_f32_32x32x2_f32 with A = items (row i = item),
// B = users (column j = user), so lane l holds user (l & 31) of each 32-user block and 16 items of the tile.  The K loop walks D in
// chunks of TK = 32 through LDS (rows padded to 33 floats), the next chunk's global loads in registers while the MFMAs run.  MFMA
// step s takes k = 2s (lanes 0-31) then 2s+1 (lanes 32-63) into one accumulator: the score is one ascending-k fmaf chain from 0,
// the chain recommend_topk_kernel (ops.hip) runs on the VALU, so the two kernels give the same bits.
//
// Selection.  Per user an LDS buffer of CAPP (key, item) pairs (key = float_key of the score), a count and a threshold = the
// current k-th best pair.  A score enters only if its (key, item) beats the threshold in the output order (key descending, then
// item ascending), so the result is the exact top-k of the user's eligible items whatever order they arrive in.  A tile adds at
// most IT pairs per user; a user whose count passed CAPP - IT is compacted after the tile (bitonic sort of its buffer, keep k,
// raise the threshold), so the buffer never overflows.  Exclusions: one thread per user walks the user's ascending exclusion list
// with a cursor, one item tile at a time, into a 128-bit mask.
// ---------------------------------------------------------------------------------------------
#define NGCF_RANK_KMAX 256

namespace {

template <int UB>
__global__ __launch_bounds__(256) void rank_topk_kernel(const float *__restrict__ users, int64_t ldu, const int64_t *__restrict__ user_ids,
                                                        int64_t n_user_rows, int64_t B, const float *__restrict__ items, int64_t ldi,
                                                        int64_t n_items, int D, int k, int64_t split_items,
                                                        const int64_t *__restrict__ excl_rowptr, const int32_t *__restrict__ excl_colidx,
                                                        int64_t excl_off, float *__restrict__ out_val, int64_t *__restrict__ out_idx,
                                                        uint32_t *__restrict__ part_key, int32_t *__restrict__ part_idx, int32_t *status)
{
    constexpr int UT = 32 * UB, IT = kRankIT, TK = kRankTK, SLD = TK + 1;
    constexpr int CAPP = UB == 2 ? 256 : 512;                    // >= k + IT for every k this tile size is used for
    constexpr int NI = IT * TK / 256, NU = UT * TK / 256;        // global loads per thread and chunk
    __shared__ float sI[IT * SLD];
    __shared__ float sU[UT * SLD];
    __shared__ uint32_t cnt[UT], thk[UT], exm[UT * (IT / 32)];
    __shared__ int32_t thi[UT];
    __shared__ int64_t srow[UT];
    __shared__ int flist[UT];
    __shared__ int nflag;
    extern __shared__ uint32_t rank_dyn[];
    uint32_t *bk = rank_dyn;                                     // [UT][CAPP] keys
    int32_t *bi = reinterpret_cast<int32_t *>(rank_dyn + UT * CAPP);   // [UT][CAPP] items

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * UT;
    const int64_t i_begin = (int64_t)blockIdx.y * split_items;
    const int64_t i_end = i_begin + split_items < n_items ? i_begin + split_items : n_items;

    for (int p = tid; p < UT * CAPP; p += 256) {
        bk[p] = kPadKey;
        bi[p] = kPadIdx;
    }
    int64_t cur = 0, cur_end = 0;                                // exclusion cursor of user `tid` (threads tid < UT)
    if (tid < UT) {
        const int64_t r = rank_user(user_ids, b0 + tid, B, n_user_rows);
        if (r == -2 && blockIdx.y == 0) atomicOr(status, 1);
        srow[tid] = r;
        cnt[tid] = 0;
        thk[tid] = kPadKey;
        thi[tid] = kPadIdx;
        if (r >= 0 && excl_rowptr) {
            cur = excl_rowptr[r];
            cur_end = excl_rowptr[r + 1];
        }
    }
    __syncthreads();

    const int n_chunks = (D + TK - 1) / TK;
    const int64_t n_tiles = (i_end - i_begin + IT - 1) / IT;
    const int64_t n_steps = n_tiles * n_chunks;
    float pI[NI], pU[NU];
    auto load = [&](int64_t s) {
        const int64_t i0 = i_begin + (s / n_chunks) * IT;
        const int k0 = (int)(s % n_chunks) * TK;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int f = tid + 256 * j, it = f / TK, kk = f % TK;
            const int64_t gi = i0 + it;
            pI[j] = (gi < i_end && k0 + kk < D) ? items[gi * ldi + k0 + kk] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int f = tid + 256 * j, ur = f / TK, kk = f % TK;
            const int64_t r = srow[ur];
            pU[j] = (r >= 0 && k0 + kk < D) ? users[r * ldu + k0 + kk] : 0.f;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int f = tid + 256 * j;
            sI[(f / TK) * SLD + f % TK] = pI[j];
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int f = tid + 256 * j;
            sU[(f / TK) * SLD + f % TK] = pU[j];
        }
    };

    if (n_steps > 0) load(0);
    int64_t step = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t i0 = i_begin + t * IT;
        // this tile's exclusion masks (the previous tile's selection is past the barrier that ended its compaction)
        if (tid < UT) {
            uint32_t m[IT / 32] = {};
            while (cur < cur_end) {
                const int64_t c = (int64_t)excl_colidx[cur] - excl_off;
                if (c >= i0 + IT) break;
                if (c >= i0) m[(c - i0) >> 5] |= 1u << ((c - i0) & 31);
                ++cur;
            }
#pragma unroll
            for (int w = 0; w < IT / 32; ++w) exm[tid * (IT / 32) + w] = m[w];
        }
        f32x16 acc[UB];
#pragma unroll
        for (int ub = 0; ub < UB; ++ub)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ub][e] = 0.f;
        for (int c = 0; c < n_chunks; ++c, ++step) {
            __syncthreads();
            store();
            __syncthreads();
            if (step + 1 < n_steps) load(step + 1);          // next chunk (next tile's first one too) flies under the MFMAs
            const float *A = sI + (wave * 32 + (lane & 31)) * SLD + (lane >> 5);
            const float *Bu = sU + (lane & 31) * SLD + (lane >> 5);
#pragma unroll
            for (int s = 0; s < TK / 2; ++s) {
                const float a = A[2 * s];
#pragma unroll
                for (int ub = 0; ub < UB; ++ub)
                    acc[ub] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bu[ub * 32 * SLD + 2 * s], acc[ub], 0, 0, 0);
            }
        }
        __syncthreads();                                      // exclusion masks written
        // insert: lane holds user ub*32 + (lane&31), items 32*wave + (e&3) + 8*(e>>2) + 4*(lane>>5) of the tile
#pragma unroll
        for (int ub = 0; ub < UB; ++ub) {
            const int u = ub * 32 + (lane & 31);
            if (srow[u] < 0) continue;
            const uint32_t tk = thk[u];
            const int32_t ti = thi[u];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int il = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                const int64_t gi = i0 + il;
                if (gi >= i_end || ((exm[u * (IT / 32) + (il >> 5)] >> (il & 31)) & 1u)) continue;
                const uint32_t key = float_key(acc[ub][e]);
                if (pair_before(key, (int32_t)gi, tk, ti)) {
                    const uint32_t pos = atomicAdd(&cnt[u], 1u);
                    bk[u * CAPP + pos] = key;
                    bi[u * CAPP + pos] = (int32_t)gi;
                }
            }
        }
        if (tid == 0) nflag = 0;
        __syncthreads();
        const bool last = t + 1 == n_tiles;
        if (tid < UT && (last ? cnt[tid] > 0 : cnt[tid] > (uint32_t)(CAPP - IT))) flist[atomicAdd(&nflag, 1)] = tid;
        __syncthreads();
        if (nflag > 0) rank_compact<CAPP>(bk, bi, cnt, thk, thi, flist, nflag, k);
    }

    // out: the sorted best k (fewer if fewer were eligible: padding)
    for (int p = tid; p < UT * k; p += 256) {
        const int u = p / k, j = p % k;
        const int64_t b = b0 + u;
        if (srow[u] < 0) {
            if (srow[u] == -1 || !part_key) continue;         // past the batch / a bad final row: left as it is
        }
        const bool has = srow[u] >= 0 && j < (int)cnt[u];
        const uint32_t key = has ? bk[u * CAPP + j] : kPadKey;
        const int32_t idx = has ? bi[u * CAPP + j] : kPadIdx;
        if (part_key) {
            const int64_t o = ((int64_t)blockIdx.y * B + b) * k + j;
            part_key[o] = key;
            part_idx[o] = idx;
        } else {
            out_val[b * k + j] = has ? float_unkey(key) : -INFINITY;
            out_idx[b * k + j] = has ? (int64_t)idx : -1;
        }
    }
}

// What rank_merge_kernel writes for slot j of batch row b: the value and the item, (-inf, -1) past the eligible items.
struct RankTopkOut {
    float *val;
    int64_t *idx;
    int k;
    __device__ void operator()(int64_t b, int j, bool has, uint32_t key, int32_t item) const
    {
        val[b * k + j] = has ? float_unkey(key) : -INFINITY;
        idx[b * k + j] = has ? (int64_t)item : -1;
    }
};

struct RankPlan {
    int ub;                 // 32-user blocks per workgroup
    int64_t user_tiles, splits, split_items;
    size_t dyn_lds;
};

RankPlan rank_plan(int64_t B, int64_t n_items, int k)
{
    RankPlan p;
    p.ub = k <= 128 ? 2 : 1;
    const int64_t ut = 32 * p.ub;
    p.user_tiles = (B + ut - 1) / ut;
    const ItemSplit sp = rank_item_split(p.user_tiles, n_items);
    p.splits = sp.splits;
    p.split_items = sp.split_items;
    p.dyn_lds = (size_t)ut * (p.ub == 2 ? 256 : 512) * 8;
    return p;
}

}  // namespace

extern "C" int64_t ngcf_rank_workspace_bytes(int64_t B, int64_t n_items, int D, int k)
{
    if (B < 0 || n_items < 1 || D < 1 || k < 1 || k > NGCF_RANK_KMAX) return -1;
    const RankPlan p = rank_plan(B, n_items, k);
    if (p.splits <= 1) return 0;
    return align_up(p.splits * B * k * 4, 256) * 2;
}

extern "C" int ngcf_rank_topk_f32(const float *users, int64_t ldu, const int64_t *user_ids, int64_t n_user_rows, int64_t B,
                                  const float *items, int64_t ldi, int64_t n_items, int D, int k, const int64_t *excl_rowptr,
                                  const int32_t *excl_colidx, int64_t excl_col_offset, float *out_val, int64_t *out_idx,
                                  int32_t *status, void *workspace, int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (k < 1 || k > n_items)
        return fail(NGCF_ERR_ARG, "selected index k out of range (k=%d, row length %lld)", k, (long long)n_items);
    if (k > NGCF_RANK_KMAX)
        return fail(NGCF_ERR_ARG, "rank_topk: k=%d > %d is not supported; ngcf_recommend_topk_f32 (recommend_topk) takes k up to 1024",
                    k, NGCF_RANK_KMAX);
    if (n_items >= (int64_t)1 << 31) return fail(NGCF_ERR_ARG, "rank_topk: too many items");
    if (B < 0 || n_user_rows < 0) return fail(NGCF_ERR_ARG, "rank_topk: bad argument");
    if (B == 0) return NGCF_OK;
    if (!users || !items || !out_val || !out_idx || !status || D < 1 || ldu < D || ldi < D || (excl_rowptr && !excl_colidx))
        return fail(NGCF_ERR_ARG, "rank_topk: bad argument");
    const RankPlan p = rank_plan(B, n_items, k);
    if (p.user_tiles >= ((int64_t)1 << 31) || p.splits > 65535) return fail(NGCF_ERR_ARG, "rank_topk: batch too large");
    const int64_t need = ngcf_rank_workspace_bytes(B, n_items, D, k);
    if (need > 0 && (!workspace || workspace_bytes < need))
        return fail(NGCF_ERR_WORKSPACE, "rank_topk: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    uint32_t *pk = nullptr;
    int32_t *pi = nullptr;
    if (p.splits > 1) {
        pk = static_cast<uint32_t *>(workspace);
        pi = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + need / 2);
    }
    const dim3 grid((unsigned)p.user_tiles, (unsigned)p.splits);
#define NGCF_RANK_LAUNCH(UB_)                                                                                                   \
    do {                                                                                                                        \
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(rank_topk_kernel<UB_>),                                      \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.dyn_lds));                               \
        rank_topk_kernel<UB_><<<grid, 256, p.dyn_lds, stream>>>(users, ldu, user_ids, n_user_rows, B, items, ldi, n_items, D, k, \
                                                                p.split_items, excl_rowptr, excl_colidx, excl_col_offset,         \
                                                                out_val, out_idx, pk, pi, status);                              \
    } while (0)
    if (p.ub == 2)
        NGCF_RANK_LAUNCH(2);
    else
        NGCF_RANK_LAUNCH(1);
#undef NGCF_RANK_LAUNCH
    LAUNCH_CHECK();
    if (p.splits > 1) {
        rank_merge_kernel<<<dim3((unsigned)B), 256, 0, stream>>>(pk, pi, (int)p.splits, B, k, user_ids, n_user_rows,
                                                                 RankTopkOut{out_val, out_idx, k});
        LAUNCH_CHECK();
    }
    return NGCF_OK;
}

// ---------------------------------------------------------------------------------------------
// Held-out metrics.  One thread per batch row: the truth row is ascending (ItemSets), so each top-list entry is a binary search.
// Per-block partials in block order, then one workgroup adds the blocks in order into `sums`: bit-identical from run to run.
// Slot layout per K: recall, ndcg, precision, hr; the last slot counts the evaluated users (non-empty truth).
// ---------------------------------------------------------------------------------------------
#define NGCF_METRIC_KS 8

namespace {

__global__ __launch_bounds__(256) void rank_metrics_kernel(const int64_t *__restrict__ top_idx, int64_t B, int k,
                                                           const int64_t *__restrict__ user_ids, int64_t n_user_rows,
                                                           const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                           int64_t off, int n_ks, int ks0, int ks1, int ks2, int ks3, int ks4, int ks5,
                                                           int ks6, int ks7, float *__restrict__ per_user, double *__restrict__ part,
                                                           int32_t *status)
{
    constexpr int NK = NGCF_METRIC_KS, NS = 4 * NK + 1;
    __shared__ double sh[256];
    const int ks[NK] = {ks0, ks1, ks2, ks3, ks4, ks5, ks6, ks7};
    const int tid = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * 256 + tid;
    double v[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) v[s] = 0.0;
    if (b < B) {
        const int64_t r = user_ids ? user_ids[b] : b;
        if (r < 0 || r >= n_user_rows) {
            atomicOr(status, 1);
        } else {
            const int64_t e1 = rowptr[r + 1];
            int64_t first = rowptr[r];
            while (first < e1 && (int64_t)colidx[first] - off < 0) ++first;     // ids below 0 after the offset: not items
            int64_t nt = 0, prev = -1;                                            // |T|: distinct ids (the row is ascending)
            for (int64_t e = first; e < e1; ++e) {
                const int64_t c = (int64_t)colidx[e] - off;
                nt += c != prev;
                prev = c;
            }
            if (nt > 0) {
                double dcg[NK] = {}, idcg[NK] = {};
                int hits[NK] = {};
                for (int j = 0; j < k; ++j) {
                    const int64_t it = top_idx[b * k + j];
                    const bool hit = it >= 0 && row_has(colidx, first, e1, off, it);
                    const double g = 1.0 / log2((double)j + 2.0);
#pragma unroll
                    for (int q = 0; q < NK; ++q) {
                        if (q < n_ks && j < ks[q]) {
                            if (hit) { hits[q] += 1; dcg[q] += g; }
                            if (j < nt) idcg[q] += g;
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < NK; ++q) {
                    if (q < n_ks) {
                        v[4 * q + 0] = (double)hits[q] / (double)nt;
                        v[4 * q + 1] = dcg[q] / idcg[q];
                        v[4 * q + 2] = (double)hits[q] / (double)ks[q];
                        v[4 * q + 3] = hits[q] > 0 ? 1.0 : 0.0;
                    }
                }
                v[NS - 1] = 1.0;
            }
        }
        if (per_user) {
#pragma unroll
            for (int s = 0; s < NS - 1; ++s)
                if (s < 4 * n_ks) per_user[b * (4 * n_ks) + s] = (float)v[s];
        }
    }
    // this block's users in order, slot by slot (the count last, in slot 4*n_ks)
    const int n_slots = 4 * n_ks + 1;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int slot = s == NS - 1 ? n_slots - 1 : s;
        if (s < n_slots - 1 || s == NS - 1) {
            sh[tid] = v[s];
            __syncthreads();
            if (tid == 0) {
                double a = 0.0;
                for (int t = 0; t < 256; ++t) a += sh[t];
                part[(int64_t)blockIdx.x * n_slots + slot] = a;
            }
            __syncthreads();
        }
    }
}

}  // namespace

extern "C" int ngcf_rank_metrics(const int64_t *top_idx, int64_t B, int k, const int64_t *user_ids, int64_t n_user_rows,
                                 const int64_t *truth_rowptr, const int32_t *truth_colidx, int64_t truth_col_offset,
                                 const int32_t *ks_host, int n_ks, float *per_user, double *sums, int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_ks < 1 || n_ks > NGCF_METRIC_KS || !ks_host) return fail(NGCF_ERR_ARG, "rank_metrics: between 1 and %d cut-offs", NGCF_METRIC_KS);
    if (k < 1) return fail(NGCF_ERR_ARG, "rank_metrics: k=%d", k);
    int ks[NGCF_METRIC_KS] = {1, 1, 1, 1, 1, 1, 1, 1};
    for (int q = 0; q < n_ks; ++q) {
        if (ks_host[q] < 1 || ks_host[q] > k)
            return fail(NGCF_ERR_ARG, "rank_metrics: cut-off K=%d outside [1, k=%d]", ks_host[q], k);
        ks[q] = ks_host[q];
    }
    if (B < 0) return fail(NGCF_ERR_ARG, "rank_metrics: bad argument");
    if (B == 0) return NGCF_OK;
    if (!top_idx || !truth_rowptr || !sums || !status || (!truth_colidx && truth_rowptr == nullptr))
        return fail(NGCF_ERR_ARG, "rank_metrics: bad argument");
    const int n_slots = 4 * n_ks + 1;
    const int64_t blocks = (B + 255) / 256;
    if (blocks >= ((int64_t)1 << 31)) return fail(NGCF_ERR_ARG, "rank_metrics: batch too large");
    return launch_with_partial_sums("rank_metrics", blocks, n_slots, sums, stream, [&](double *part) {
        rank_metrics_kernel<<<dim3((unsigned)blocks), 256, 0, stream>>>(top_idx, B, k, user_ids, n_user_rows, truth_rowptr, truth_colidx,
                                                                       truth_col_offset, n_ks, ks[0], ks[1], ks[2], ks[3], ks[4],
                                                                       ks[5], ks[6], ks[7], per_user, part, status);
    });
}
