// Certified two-stage ranking: a bf16 MFMA pass over the whole catalogue keeps, per user, the `pool` items with the
// largest UPPER BOUND on their exact fp32 score; the pool alone is re-scored with rank_topk's chain, and its top-k is accepted only
// where the bound proves that no item outside the pool can reach it.  The pair order, the item split, the streaming selection and
// the merge of the split lists are rank_device.h's, as in rank.hip.
#include "rank_device.h"


namespace {

constexpr int kPfKStep = NGCF_RANK_PREFILTER_KSTEP;   // K of v_mfma_f32_32x32x16_bf16: the packed rows are padded to it

// beta of the header's bound, exact in fp64: 2^-7 + 2^-16 + (4 D + 2) 2^-24
inline double prefilter_beta(int D) { return 0x1p-7 + 0x1p-16 + (4.0 * D + 2.0) * 0x1p-24; }

// bf16 image of an fp32 value, round to nearest even on the bit pattern (what tests/prefilter_oracle.py states in integers)
__device__ inline uint16_t bf16_rne(float x)
{
    const uint32_t u = __float_as_uint(x);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ inline uint4 bf16_pack8(const float *v)
{
    uint4 o;
    o.x = (uint32_t)bf16_rne(v[0]) | ((uint32_t)bf16_rne(v[1]) << 16);
    o.y = (uint32_t)bf16_rne(v[2]) | ((uint32_t)bf16_rne(v[3]) << 16);
    o.z = (uint32_t)bf16_rne(v[4]) | ((uint32_t)bf16_rne(v[5]) << 16);
    o.w = (uint32_t)bf16_rne(v[6]) | ((uint32_t)bf16_rne(v[7]) << 16);
    return o;
}

// A regular element: 0, or a magnitude in [2^-40, 2^40] (NaN and the infinities are not): the range in which the bound's model of
// the two accumulation chains holds with no underflow or overflow.
__device__ inline bool pf_regular(float x)
{
    const float a = fabsf(x);
    return a == 0.f || (a >= 0x1p-40f && a <= 0x1p40f);
}

// The smallest fp32 value above a non-negative finite fp64 value's nearest fp32 neighbour: an fp32 upper bound of it.
__device__ inline float pf_round_up(double v)
{
    const float f = (float)v;
    return __uint_as_float(__float_as_uint(f) + 1u);
}

// One wave per item row: the bf16 image in 16-byte pieces, the row's norm rounded up, the irregular flag.
__global__ __launch_bounds__(256) void rank_pack_items_kernel(const float *__restrict__ items, int64_t ldi, int64_t n_items, int D, int Dp,
                                                              uint4 *__restrict__ out, float *__restrict__ norm_up,
                                                              int32_t *__restrict__ flags)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_items) return;
    const float *row = items + i * ldi;
    double sq = 0.0;
    bool bad = false;
    for (int p = lane; p < Dp / 8; p += 64) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = p * 8 + j;
            v[j] = c < D ? row[c] : 0.f;
            bad |= !pf_regular(v[j]);
            sq += (double)v[j] * (double)v[j];
        }
        out[i * (Dp / 8) + p] = bf16_pack8(v);
    }
    sq = wave_sum(sq);
    if (__any(bad) && lane == 0) flags[0] = 1;               // every writer stores the same word: no atomic
    if (lane == 0) norm_up[i] = pf_round_up(sqrt(sq));
}

// One wave per batch row: bu >= beta * |u| rounded up, and the user's irregular flag (a row past the table: flag and status).
__global__ __launch_bounds__(256) void rank_user_bounds_kernel(const float *__restrict__ users, int64_t ldu, const int64_t *__restrict__ user_ids,
                                                               int64_t n_user_rows, int64_t B, int D, double beta, float *__restrict__ bu,
                                                               int32_t *__restrict__ user_flags, int32_t *status)
{
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t r = rank_user(user_ids, b, B, n_user_rows);
    if (r == -1) return;
    if (r == -2) {
        if (lane == 0) {
            atomicOr(status, 1);
            bu[b] = 0.f;
            user_flags[b] = 1;
        }
        return;
    }
    const float *row = users + r * ldu;
    double sq = 0.0;
    bool bad = false;
    for (int c = lane; c < D; c += 64) {
        const float v = row[c];
        bad |= !pf_regular(v);
        sq += (double)v * (double)v;
    }
    sq = wave_sum(sq);
    const bool any_bad = __any(bad);
    if (lane == 0) {
        bu[b] = pf_round_up(beta * sqrt(sq));
        user_flags[b] = any_bad ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------
// The shortlist.  rank_topk_kernel's walk with bf16 operands: 4 waves own UT = 32*UB users and walk item tiles of IT = 128; wave w
// computes items [32w, 32w+32) against all UT users with v_mfma_f32_32x32x16_bf16 (A = items, B = users: lane l holds user l & 31 of
// each 32-user block and 16 items).  K goes through LDS in chunks of TK = 64 bf16 (rows padded to 72: 16-byte fragment reads); the
// item pieces come from the packed image as they are, the user pieces are fp32 rows converted on the way in.  The key of a pair is
// float_key(fmaf(bu, ni, score)), the selection is rank_topk's with k = pool.
// ---------------------------------------------------------------------------------------------
template <int UB>
__global__ __launch_bounds__(256) void rank_shortlist_kernel(const float *__restrict__ users, int64_t ldu, const int64_t *__restrict__ user_ids,
                                                             int64_t n_user_rows, int64_t B, const uint4 *__restrict__ packed,
                                                             const float *__restrict__ norm_up, int64_t n_items, int D, int Dp, int pool,
                                                             int64_t split_items, const int64_t *__restrict__ excl_rowptr,
                                                             const int32_t *__restrict__ excl_colidx, int64_t excl_off,
                                                             const float *__restrict__ bu, int32_t *__restrict__ pool_idx,
                                                             float *__restrict__ pool_thr, uint32_t *__restrict__ part_key,
                                                             int32_t *__restrict__ part_idx, float *__restrict__ debug_scores)
{
    constexpr int UT = 32 * UB, IT = kRankIT, TK = 64, SLD = TK + 8, PC = TK / 8;
    constexpr int CAPP = UB == 2 ? 256 : 512;                    // >= pool + IT for every pool this tile size is used for
    constexpr int NI = IT * PC / 256, NU = UT * PC / 256;        // 16-byte pieces per thread and chunk
    __shared__ __attribute__((aligned(16))) uint16_t sI[IT * SLD];
    __shared__ __attribute__((aligned(16))) uint16_t sU[UT * SLD];
    __shared__ uint32_t cnt[UT], thk[UT], exm[UT * (IT / 32)];
    __shared__ int32_t thi[UT];
    __shared__ int64_t srow[UT];
    __shared__ float sbu[UT], sni[IT];
    __shared__ int flist[UT];
    __shared__ int nflag;
    extern __shared__ uint32_t rank_dyn[];
    uint32_t *bk = rank_dyn;                                     // [UT][CAPP] keys
    int32_t *bi = reinterpret_cast<int32_t *>(rank_dyn + UT * CAPP);   // [UT][CAPP] items

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * UT;
    const int64_t i_begin = (int64_t)blockIdx.y * split_items;
    const int64_t i_end = i_begin + split_items < n_items ? i_begin + split_items : n_items;
    const int pieces_row = Dp / 8;

    for (int p = tid; p < UT * CAPP; p += 256) {
        bk[p] = kPadKey;
        bi[p] = kPadIdx;
    }
    int64_t cur = 0, cur_end = 0;                                // exclusion cursor of user `tid` (threads tid < UT)
    if (tid < UT) {
        const int64_t r = rank_user(user_ids, b0 + tid, B, n_user_rows);   // a bad row: rank_user_bounds_kernel set the status
        srow[tid] = r;
        sbu[tid] = r >= 0 ? bu[b0 + tid] : 0.f;
        cnt[tid] = 0;
        thk[tid] = kPadKey;
        thi[tid] = kPadIdx;
        if (r >= 0 && excl_rowptr) {
            cur = excl_rowptr[r];
            cur_end = excl_rowptr[r + 1];
        }
    }
    __syncthreads();

    const int n_chunks = (Dp + TK - 1) / TK;
    const int64_t n_tiles = (i_end - i_begin + IT - 1) / IT;
    const int64_t n_steps = n_tiles * n_chunks;
    uint4 pI[NI];
    float pU[NU][8];
    auto load = [&](int64_t s) {
        const int64_t i0 = i_begin + (s / n_chunks) * IT;
        const int k0 = (int)(s % n_chunks) * TK;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int f = tid + 256 * j, it = f / PC, pc = f % PC;
            const int64_t gi = i0 + it;
            pI[j] = (gi < i_end && k0 + pc * 8 < Dp) ? packed[gi * pieces_row + (k0 >> 3) + pc] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int f = tid + 256 * j, ur = f / PC, pc = f % PC;
            const int64_t r = srow[ur];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = k0 + pc * 8 + e;
                pU[j][e] = (r >= 0 && c < D) ? users[r * ldu + c] : 0.f;
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int f = tid + 256 * j;
            *reinterpret_cast<uint4 *>(sI + (f / PC) * SLD + (f % PC) * 8) = pI[j];
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int f = tid + 256 * j;
            *reinterpret_cast<uint4 *>(sU + (f / PC) * SLD + (f % PC) * 8) = bf16_pack8(pU[j]);
        }
    };

    if (n_steps > 0) load(0);
    int64_t step = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t i0 = i_begin + t * IT;
        // this tile's exclusion masks and item norms (the previous tile's selection is past the barrier that ended its compaction)
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
        if (tid >= 256 - IT) {
            const int il = tid - (256 - IT);
            sni[il] = i0 + il < i_end ? norm_up[i0 + il] : 0.f;
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
            const uint16_t *A = sI + (wave * 32 + (lane & 31)) * SLD + 8 * (lane >> 5);
            const uint16_t *Bu = sU + (lane & 31) * SLD + 8 * (lane >> 5);
#pragma unroll
            for (int s = 0; s < TK / kPfKStep; ++s) {
                const bf16x8 a = *reinterpret_cast<const bf16x8 *>(A + kPfKStep * s);
#pragma unroll
                for (int ub = 0; ub < UB; ++ub) {
                    const bf16x8 bf = *reinterpret_cast<const bf16x8 *>(Bu + ub * 32 * SLD + kPfKStep * s);
                    acc[ub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bf, acc[ub], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                      // exclusion masks and norms written
        // insert: lane holds user ub*32 + (lane&31), items 32*wave + (e&3) + 8*(e>>2) + 4*(lane>>5) of the tile
#pragma unroll
        for (int ub = 0; ub < UB; ++ub) {
            const int u = ub * 32 + (lane & 31);
            if (srow[u] < 0) continue;
            const uint32_t tk = thk[u];
            const int32_t ti = thi[u];
            const float bound = sbu[u];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int il = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                const int64_t gi = i0 + il;
                if (gi >= i_end) continue;
                const float upper = fmaf(bound, sni[il], acc[ub][e]);
                if (debug_scores) {
                    debug_scores[(b0 + u) * n_items + gi] = acc[ub][e];
                    debug_scores[(B + b0 + u) * n_items + gi] = upper;
                }
                if ((exm[u * (IT / 32) + (il >> 5)] >> (il & 31)) & 1u) continue;
                const uint32_t key = float_key(upper);
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
        if (nflag > 0) rank_compact<CAPP>(bk, bi, cnt, thk, thi, flist, nflag, pool);
    }

    // out: the sorted best `pool` (fewer if fewer were eligible: padding), and the pool-th key as the threshold
    for (int p = tid; p < UT * pool; p += 256) {
        const int u = p / pool, j = p % pool;
        const int64_t b = b0 + u;
        if (srow[u] == -1) continue;                          // past the batch
        const bool has = srow[u] >= 0 && j < (int)cnt[u];
        const uint32_t key = has ? bk[u * CAPP + j] : kPadKey;
        const int32_t idx = has ? bi[u * CAPP + j] : kPadIdx;
        if (part_key) {
            const int64_t o = ((int64_t)blockIdx.y * B + b) * pool + j;
            part_key[o] = key;
            part_idx[o] = idx;
        } else {
            pool_idx[b * pool + j] = has ? idx : -1;
            if (j == pool - 1) pool_thr[b] = has ? float_unkey(key) : -INFINITY;
        }
    }
}

// What rank_merge_kernel writes for slot j of batch row b of a shortlist: the item, and from the last slot the threshold.
struct ShortlistOut {
    int32_t *pool_idx;
    float *pool_thr;
    int pool;
    __device__ void operator()(int64_t b, int j, bool has, uint32_t key, int32_t item) const
    {
        pool_idx[b * pool + j] = has ? item : -1;
        if (j == pool - 1) pool_thr[b] = has ? float_unkey(key) : -INFINITY;
    }
};

// ---------------------------------------------------------------------------------------------
// The exact re-score, one workgroup per batch row, thread p the pool's slot p.  The user row sits in LDS; the pool's item rows pass
// through LDS in chunks of 32 columns (coalesced gathers, a row per 32 lanes), and every thread runs rank_topk's chain on its row:
// acc = fmaf(u_k, i_k, acc), k ascending from acc = 0 over D padded to 32 columns with zeros, as rank_topk_kernel's K loop pads it.
// Then a bitonic sort of the 256 (key, item) pairs by pair_before, the best k out, and the certificate.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rank_rescore_kernel(const float *__restrict__ users, int64_t ldu, const int64_t *__restrict__ user_ids,
                                                           int64_t n_user_rows, int64_t B, const float *__restrict__ items, int64_t ldi,
                                                           int64_t n_items, int D, int k, int pool, const int32_t *__restrict__ pool_idx,
                                                           const float *__restrict__ pool_thr, const int32_t *__restrict__ user_flags,
                                                           const int32_t *__restrict__ item_flags, float *__restrict__ out_val,
                                                           int64_t *__restrict__ out_idx, uint8_t *__restrict__ certified)
{
    constexpr int P = NGCF_RANK_POOL_MAX, TK = kRankTK, SLD = TK + 1;
    __shared__ float sT[P * SLD];
    __shared__ uint32_t sk[P];
    __shared__ int32_t si[P];
    extern __shared__ float pf_user[];                          // the user row, padded with zeros to whole chunks
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t r = rank_user(user_ids, b, B, n_user_rows);
    if (r < 0) {                                                 // the shortlist launch set the status; the row stays as it is
        if (tid == 0) certified[b] = 0;
        return;
    }
    const int Dk = (D + TK - 1) / TK * TK;
    for (int c = tid; c < Dk; c += 256) pf_user[c] = c < D ? users[r * ldu + c] : 0.f;
    int32_t item = tid < pool ? pool_idx[b * pool + tid] : -1;
    if (item >= n_items) item = -1;                              // never an index past the table
    si[tid] = item;
    __syncthreads();
    float acc = 0.f;
    for (int k0 = 0; k0 < Dk; k0 += TK) {
#pragma unroll 8
        for (int j = 0; j < P * TK / 256; ++j) {
            const int f = tid + 256 * j, row = f / TK, kk = f % TK;
            const int32_t it = si[row];
            sT[row * SLD + kk] = (it >= 0 && k0 + kk < D) ? items[(int64_t)it * ldi + k0 + kk] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < TK; ++kk) acc = fmaf(pf_user[k0 + kk], sT[tid * SLD + kk], acc);
        __syncthreads();
    }
    sk[tid] = item >= 0 ? float_key(acc) : kPadKey;
    si[tid] = item >= 0 ? item : kPadIdx;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (tid < P / 2) {
                const int a = (tid / stride) * (2 * stride) + (tid % stride), c = a + stride;
                const bool desc = (a & size) == 0;
                const uint32_t ka = sk[a], kc = sk[c];
                const int32_t ia = si[a], ic = si[c];
                if (pair_before(ka, ia, kc, ic) != desc) {
                    sk[a] = kc; sk[c] = ka;
                    si[a] = ic; si[c] = ia;
                }
            }
            __syncthreads();
        }
    }
    if (tid < k) {
        const bool has = si[tid] != kPadIdx;
        out_val[b * k + tid] = has ? float_unkey(sk[tid]) : -INFINITY;
        out_idx[b * k + tid] = has ? (int64_t)si[tid] : -1;
    }
    if (tid == 0) {
        const bool full = pool_idx[b * pool + pool - 1] >= 0;
        const bool regular = user_flags[b] == 0 && item_flags[0] == 0;
        // a pool that is not full holds every eligible item; a full one is proof when its k-th exact score is above every bound outside
        const bool above = si[k - 1] != kPadIdx && float_unkey(sk[k - 1]) > pool_thr[b];
        certified[b] = (regular && (!full || above)) ? 1 : 0;
    }
}

struct PrefilterPlan {
    int ub;                 // 32-user blocks per workgroup
    int64_t user_tiles, splits, split_items;
    size_t dyn_lds;
};

PrefilterPlan prefilter_plan(int64_t B, int64_t n_items, int pool)
{
    PrefilterPlan p;
    p.ub = pool <= 128 ? 2 : 1;
    const int64_t ut = 32 * p.ub;
    p.user_tiles = (B + ut - 1) / ut;
    const ItemSplit sp = rank_item_split(std::max<int64_t>(p.user_tiles, 1), n_items);
    p.splits = sp.splits;
    p.split_items = sp.split_items;
    p.dyn_lds = (size_t)ut * (p.ub == 2 ? 256 : 512) * 8;
    return p;
}

bool prefilter_sizes_ok(int64_t B, int64_t n_items, int D, int pool)
{
    return B >= 0 && n_items >= 1 && n_items < ((int64_t)1 << 31) && D >= 1 && D <= NGCF_RANK_PREFILTER_DMAX && pool >= 1 &&
           pool <= NGCF_RANK_POOL_MAX;
}

}  // namespace

extern "C" int ngcf_rank_pack_items(const float *items, int64_t ldi, int64_t n_items, int D, void *out_bf16, float *norm_up,
                                    int32_t *flags, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_items < 1 || n_items >= ((int64_t)1 << 31) || D < 1 || D > NGCF_RANK_PREFILTER_DMAX || ldi < D)
        return fail(NGCF_ERR_ARG, "rank_pack_items: bad argument (n_items=%lld, D=%d, ldi=%lld)", (long long)n_items, D, (long long)ldi);
    if (!items || !out_bf16 || !norm_up || !flags || !aligned16(out_bf16)) return fail(NGCF_ERR_ARG, "rank_pack_items: bad argument");
    const int Dp = (int)align_up(D, kPfKStep);
    HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int32_t), stream));
    rank_pack_items_kernel<<<dim3((unsigned)((n_items + 3) / 4)), 256, 0, stream>>>(items, ldi, n_items, D, Dp, static_cast<uint4 *>(out_bf16),
                                                                                   norm_up, flags);
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int64_t ngcf_rank_prefilter_workspace_bytes(int64_t B, int64_t n_items, int D, int pool)
{
    if (!prefilter_sizes_ok(B, n_items, D, pool)) return -1;
    const PrefilterPlan p = prefilter_plan(B, n_items, pool);
    const int64_t bounds = align_up(std::max<int64_t>(B, 1) * 4, 256);
    return bounds + (p.splits > 1 ? align_up(p.splits * B * pool * 4, 256) * 2 : 0);
}

extern "C" int ngcf_rank_shortlist_bf16(const float *users, int64_t ldu, const int64_t *user_ids, int64_t n_user_rows, int64_t B,
                                        const void *packed_bf16, const float *norm_up, int64_t n_items, int D, int pool,
                                        const int64_t *excl_rowptr, const int32_t *excl_colidx, int64_t excl_col_offset,
                                        int32_t *pool_idx, float *pool_thr, int32_t *user_flags, float *debug_scores, int32_t *status,
                                        void *workspace, int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!prefilter_sizes_ok(B, n_items, D, pool) || n_user_rows < 0)
        return fail(NGCF_ERR_ARG, "rank_shortlist: bad argument (B=%lld, n_items=%lld, D=%d in [1, %d], pool=%d in [1, %d])", (long long)B,
                    (long long)n_items, D, NGCF_RANK_PREFILTER_DMAX, pool, NGCF_RANK_POOL_MAX);
    if (B == 0) return NGCF_OK;
    if (!users || !packed_bf16 || !norm_up || !pool_idx || !pool_thr || !user_flags || !status || ldu < D || !aligned16(packed_bf16) ||
        (excl_rowptr && !excl_colidx))
        return fail(NGCF_ERR_ARG, "rank_shortlist: bad argument");
    const PrefilterPlan p = prefilter_plan(B, n_items, pool);
    if (p.user_tiles >= ((int64_t)1 << 31) || p.splits > 65535) return fail(NGCF_ERR_ARG, "rank_shortlist: batch too large");
    const int64_t need = ngcf_rank_prefilter_workspace_bytes(B, n_items, D, pool);
    if (!workspace || workspace_bytes < need)
        return fail(NGCF_ERR_WORKSPACE, "rank_shortlist: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    char *ws = static_cast<char *>(workspace);
    float *bu = reinterpret_cast<float *>(ws);
    const int64_t bounds = align_up(B * 4, 256);
    uint32_t *pk = nullptr;
    int32_t *pi = nullptr;
    if (p.splits > 1) {
        pk = reinterpret_cast<uint32_t *>(ws + bounds);
        pi = reinterpret_cast<int32_t *>(ws + bounds + (need - bounds) / 2);
    }
    rank_user_bounds_kernel<<<dim3((unsigned)((B + 3) / 4)), 256, 0, stream>>>(users, ldu, user_ids, n_user_rows, B, D, prefilter_beta(D), bu,
                                                                              user_flags, status);
    LAUNCH_CHECK();
    const int Dp = (int)align_up(D, kPfKStep);
    const dim3 grid((unsigned)p.user_tiles, (unsigned)p.splits);
#define NGCF_SHORTLIST_LAUNCH(UB_)                                                                                                \
    do {                                                                                                                          \
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(rank_shortlist_kernel<UB_>),                                   \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.dyn_lds));                                 \
        rank_shortlist_kernel<UB_><<<grid, 256, p.dyn_lds, stream>>>(users, ldu, user_ids, n_user_rows, B,                        \
                                                                     static_cast<const uint4 *>(packed_bf16), norm_up, n_items, D, Dp, \
                                                                     pool, p.split_items, excl_rowptr, excl_colidx, excl_col_offset, \
                                                                     bu, pool_idx, pool_thr, pk, pi, debug_scores);               \
    } while (0)
    if (p.ub == 2)
        NGCF_SHORTLIST_LAUNCH(2);
    else
        NGCF_SHORTLIST_LAUNCH(1);
#undef NGCF_SHORTLIST_LAUNCH
    LAUNCH_CHECK();
    if (p.splits > 1) {
        rank_merge_kernel<<<dim3((unsigned)B), 256, 0, stream>>>(pk, pi, (int)p.splits, B, pool, user_ids, n_user_rows,
                                                                 ShortlistOut{pool_idx, pool_thr, pool});
        LAUNCH_CHECK();
    }
    return NGCF_OK;
}

extern "C" int ngcf_rank_rescore(const float *users, int64_t ldu, const int64_t *user_ids, int64_t n_user_rows, int64_t B,
                                 const float *items, int64_t ldi, int64_t n_items, int D, int k, int pool, const int32_t *pool_idx,
                                 const float *pool_thr, const int32_t *user_flags, const int32_t *item_flags, float *out_val,
                                 int64_t *out_idx, uint8_t *certified, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!prefilter_sizes_ok(B, n_items, D, pool) || n_user_rows < 0 || k < 1 || k > pool || k > n_items)
        return fail(NGCF_ERR_ARG, "rank_rescore: bad argument (B=%lld, n_items=%lld, D=%d, k=%d, pool=%d: 1 <= k <= pool <= %d)",
                    (long long)B, (long long)n_items, D, k, pool, NGCF_RANK_POOL_MAX);
    if (B == 0) return NGCF_OK;
    if (B >= ((int64_t)1 << 31)) return fail(NGCF_ERR_ARG, "rank_rescore: batch too large");
    if (!users || !items || !pool_idx || !pool_thr || !user_flags || !item_flags || !out_val || !out_idx || !certified || ldu < D || ldi < D)
        return fail(NGCF_ERR_ARG, "rank_rescore: bad argument");
    const size_t dyn = (size_t)align_up(D, kRankTK) * sizeof(float);
    rank_rescore_kernel<<<dim3((unsigned)B), 256, dyn, stream>>>(users, ldu, user_ids, n_user_rows, B, items, ldi, n_items, D, k, pool,
                                                                pool_idx, pool_thr, user_flags, item_flags, out_val, out_idx, certified);
    LAUNCH_CHECK();
    return NGCF_OK;
}
