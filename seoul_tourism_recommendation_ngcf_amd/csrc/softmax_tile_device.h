// What the two softmax losses over a score matrix that is never in memory share (softmax_full.hip: users x the whole catalogue;
// inbatch_softmax.hip: users x the batch's own positives and E extra rows), defined once: the score-tile walk with its running
// (max, sum of exp), the merges, the fp64 tails, the role-swapped gradient tile, the plan and the workspace.
//
// Forward.  rank_topk_kernel's score-tile walk (rank.hip: 64 users x 128 columns a tile, K in chunks of 32 through LDS, one
// ascending-k fmaf chain per score), restated here as rank_position.hip restates it; instead of a selection every lane
// keeps a running (max, sum of exp) of its user over the 16 scores it holds of each tile, and picks the positive's score up when it
// passes.  The eight (wave, lane half) holders of a user merge through LDS in ascending order, the column pieces in a second stage.
//
// Gradients.  One kernel, the roles swapped: a workgroup owns 32 OUTPUT rows (users for dU, columns for dI / dC) and a slab of <= 512
// output columns, and walks the OTHER side in tiles of 128 rows.  Phase 1 recomputes the 128 x 32 score tile over the full D exactly as
// the forward does and writes g = gout/batch_size * inv_tau * (exp(z - lse) - [positive]) into LDS, transposed (rows of 129 floats);
// phase 2 is acc[32 x slab] += G[32 x 128] . W[128 x slab] with v_mfma_f32_32x32x2_f32, wave w owning the 32-column blocks
// w, w + 4, w + 8, w + 12 of the slab (64 accumulator registers a lane, kept for the whole walk).  No W element is used by two
// waves, so W goes from memory (L2) straight into the B operand, eight k steps of loads in flight: LDS would add a copy and no re-use.
// No atomics on floats, every sum in a fixed order: loss, lse and the gradients are the same bits from run to run.
//
// INBATCH = false is the full catalogue: column j is row j of `items`, row b's positive is column pos[b].  INBATCH = true: column
// j < n_first is row j of `items` (the positives p, n_first = B), column j >= n_first row j - n_first of `extra`; row b's positive is
// column b; z_bj = s_bj - q_j off the diagonal and s_bb - pos_logq[b] on it; with ids, a column j != b whose id equals ids[b] is
// masked: out of the softmax, zero gradient.  Every `if (INBATCH)` below is a compile-time branch: the full catalogue's arithmetic is
// what it was before the in-batch loss existed.
#ifndef NGCF_SOFTMAX_TILE_DEVICE_H
#define NGCF_SOFTMAX_TILE_DEVICE_H

#include "rank_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSlab = 512;                      // output columns of a gradient workgroup: 4 waves x 4 blocks of 32
constexpr int kGT = 32;                         // output rows of a gradient workgroup
constexpr int kGLD = kRankIT + 1;               // row of the transposed g tile in LDS: 129 floats (the 33 of rank.hip, for 128)
constexpr int kFinalThreads = 256;

// The operands of both losses.  The in-batch fields are never read by an INBATCH = false kernel.
struct SoftmaxSides {
    const float *users;                         // [B, D], leading dimension ldu
    int64_t ldu, B;
    const float *items;                         // the columns' first row block, leading dimension ldi; n_items columns in all
    int64_t ldi, n_items;
    int D;
    const int64_t *pos;                         // full catalogue: the positives' ids [B]
    const float *extra;                         // in-batch: columns n_first .. n_items - 1, leading dimension ldx
    int64_t ldx, n_first;
    const int64_t *ids, *xids;                  // in-batch: the columns' ids (ids NULL: no mask), [n_first] and [n_items - n_first]
    const float *logq, *xlogq, *pos_logq;       // in-batch: the columns' corrections and the diagonal's (NULL: exactly 0)
};

template <bool INBATCH>
__device__ inline const float *col_row(const SoftmaxSides &a, int64_t j)
{
    if (INBATCH && j >= a.n_first) return a.extra + (j - a.n_first) * a.ldx;
    return a.items + j * a.ldi;
}

__device__ inline int64_t col_id(const SoftmaxSides &a, int64_t j)      // (a.ids is not NULL)
{
    return j < a.n_first ? a.ids[j] : a.xids[j - a.n_first];
}

__device__ inline float col_q(const SoftmaxSides &a, int64_t j)
{
    if (j < a.n_first) return a.logq ? a.logq[j] : 0.f;
    return a.xlogq ? a.xlogq[j - a.n_first] : 0.f;
}

// (m, l) <- (m, l) merged with (mb, lb): M = max, l = l e^(m - M) + lb e^(mb - M); a maximum of -inf shifts by 0 (e^-inf = 0)
__device__ inline void lse_merge(float &m, float &l, float mb, float lb)
{
    const float M = fmaxf(m, mb);
    const float Ms = M == -INFINITY ? 0.f : M;
    l = l * expf(m - Ms) + lb * expf(mb - Ms);
    m = M;
}

template <bool INBATCH>
__global__ __launch_bounds__(256) void softmax_full_fwd_kernel(const SoftmaxSides a, float inv_tau, int64_t split_items,
                                                               float *__restrict__ part_m, float *__restrict__ part_l,
                                                               float *__restrict__ spos, int32_t *status)
{
    constexpr int UB = 2, UT = 32 * UB, IT = kRankIT, TK = kRankTK, SLD = TK + 1;
    constexpr int NI = IT * TK / 256, NU = UT * TK / 256;
    __shared__ float sI[IT * SLD];
    __shared__ float sU[UT * SLD];
    __shared__ float pm[8 * UT], pl[8 * UT];
    // in-batch: the walked tile's column ids and corrections, two buffers by tile parity (written when a tile begins, read after
    // its K loop's barriers; the next tile's write goes to the other buffer, the one after that follows the next K loop's barriers)
    __shared__ int64_t sCid[INBATCH ? 2 * IT : 1];
    __shared__ float sQ[INBATCH ? 2 * IT : 1];

    const float *__restrict__ users = a.users;
    const int64_t ldu = a.ldu, B = a.B, n_items = a.n_items;
    const int D = a.D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * UT;
    const int64_t i_begin = (int64_t)blockIdx.y * split_items;
    const int64_t i_end = i_begin + split_items < n_items ? i_begin + split_items : n_items;
    const bool has_ids = INBATCH && a.ids != nullptr;

    int64_t upos[UB], uid[UB];
    float m[UB], l[UB], uplq[UB];
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) {
        const int64_t b = b0 + ub * 32 + (lane & 31);
        if (INBATCH) {
            upos[ub] = b;
            uid[ub] = (has_ids && b < B) ? a.ids[b] : 0;
            uplq[ub] = (a.pos_logq && b < B) ? a.pos_logq[b] : 0.f;
        } else {
            upos[ub] = b < B ? a.pos[b] : -1;
        }
        m[ub] = -INFINITY;
        l[ub] = 0.f;
    }
    if (!INBATCH && tid < UT && blockIdx.y == 0 && b0 + tid < B) {
        const int64_t p = a.pos[b0 + tid];
        if (p < 0 || p >= n_items) atomicOr(status, 1);
    }

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
            pI[j] = (gi < i_end && k0 + kk < D) ? col_row<INBATCH>(a, gi)[k0 + kk] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int f = tid + 256 * j, ur = f / TK, kk = f % TK;
            const int64_t b = b0 + ur;
            pU[j] = (b < B && k0 + kk < D) ? users[b * ldu + k0 + kk] : 0.f;
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
        const int par = INBATCH ? (int)(t & 1) * IT : 0;
        if (INBATCH && tid < IT) {
            const int64_t gi = i0 + tid;
            sCid[par + tid] = (has_ids && gi < i_end) ? col_id(a, gi) : 0;
            sQ[par + tid] = gi < i_end ? col_q(a, gi) : 0.f;
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
            if (step + 1 < n_steps) load(step + 1);
            const float *A = sI + (wave * 32 + (lane & 31)) * SLD + (lane >> 5);
            const float *Bu = sU + (lane & 31) * SLD + (lane >> 5);
#pragma unroll
            for (int s = 0; s < TK / 2; ++s) {
                const float av = A[2 * s];
#pragma unroll
                for (int ub = 0; ub < UB; ++ub)
                    acc[ub] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Bu[ub * 32 * SLD + 2 * s], acc[ub], 0, 0, 0);
            }
        }
        // lane holds user ub*32 + (lane&31), columns 32*wave + (e&3) + 8*(e>>2) + 4*(lane>>5) of the tile: e ascending
#pragma unroll
        for (int ub = 0; ub < UB; ++ub) {
            const int64_t b = b0 + ub * 32 + (lane & 31);
            float sc[16];
            unsigned in = 0;                                            // bit e: score e is in the softmax
            float tm = -INFINITY;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int il = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                const int64_t gi = i0 + il;
                sc[e] = acc[ub][e] * inv_tau;
                bool ok = gi < i_end;
                if (INBATCH) {
                    const bool diag = gi == b;
                    sc[e] = sc[e] - (diag ? uplq[ub] : sQ[par + il]);
                    if (has_ids && !diag && sCid[par + il] == uid[ub]) ok = false;
                }
                if (ok) {
                    in |= 1u << e;
                    tm = fmaxf(tm, sc[e]);
                    if (gi == upos[ub] && b < B) spos[b] = sc[e];
                }
            }
            const float M = fmaxf(m[ub], tm);
            const float Ms = M == -INFINITY ? 0.f : M;
            float ll = l[ub] * expf(m[ub] - Ms);
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (in >> e & 1u) ll += expf(sc[e] - Ms);
            m[ub] = M;
            l[ub] = ll;
        }
    }
    // the eight holders of a user, (wave, lane half) ascending
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) {
        const int h = wave * 2 + (lane >> 5), u = ub * 32 + (lane & 31);
        pm[h * UT + u] = m[ub];
        pl[h * UT + u] = l[ub];
    }
    __syncthreads();
    if (tid < UT && b0 + tid < B) {
        float mm = pm[tid], ll = pl[tid];
#pragma unroll
        for (int h = 1; h < 8; ++h) lse_merge(mm, ll, pm[h * UT + tid], pl[h * UT + tid]);
        part_m[(int64_t)blockIdx.y * B + b0 + tid] = mm;
        part_l[(int64_t)blockIdx.y * B + b0 + tid] = ll;
    }
}

// One wave per batch row, four per workgroup: the column pieces merged in ascending order, lse = M + log(l), the row's term
// lse - s_pos (in-batch: lse - z_bb) and its squared norms in fp64; part[2 blk], part[2 blk + 1] = the workgroup's four rows,
// (r0 + r1) + (r2 + r3).
template <bool INBATCH>
__global__ __launch_bounds__(256) void softmax_full_rows_kernel(const SoftmaxSides a, const float *__restrict__ part_m,
                                                                const float *__restrict__ part_l, int n_pieces, float *__restrict__ lse,
                                                                float *__restrict__ spos, double *__restrict__ part)
{
    __shared__ double sh[8];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    const int64_t B = a.B;
    double term = 0.0, sq = 0.0;
    if (b < B) {
        const int64_t p = INBATCH ? b : a.pos[b];
        const bool has = INBATCH || (p >= 0 && p < a.n_items);
        double uu = 0.0, pp = 0.0;
        for (int j = lane; j < a.D; j += 64) {
            const double x = (double)a.users[b * a.ldu + j];
            uu += x * x;
            if (has) {
                const double c = (double)a.items[p * a.ldi + j];
                pp += c * c;
            }
        }
        sq = wave_sum(uu) + wave_sum(pp);
        float mm = part_m[b], ll = part_l[b];
        for (int q = 1; q < n_pieces; ++q) lse_merge(mm, ll, part_m[(int64_t)q * B + b], part_l[(int64_t)q * B + b]);
        const float v = mm + logf(ll);
        const float sp = has ? spos[b] : 0.f;
        term = (double)v - (double)sp;
        if (lane == 0) {
            lse[b] = v;
            spos[b] = sp;
        }
    }
    if (lane == 0) {
        sh[wave * 2] = term;
        sh[wave * 2 + 1] = sq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[2 * (int64_t)blockIdx.x] = (sh[0] + sh[2]) + (sh[4] + sh[6]);
        part[2 * (int64_t)blockIdx.x + 1] = (sh[1] + sh[3]) + (sh[5] + sh[7]);
    }
}

// thread t adds the workgroups t, t + 256, .. in ascending order (fp64), thread 0 the 256 results in ascending order
__global__ __launch_bounds__(kFinalThreads) void softmax_full_final_kernel(const double *__restrict__ part, int64_t n_blocks, float wd,
                                                                          float batch_size, float *__restrict__ loss)
{
    __shared__ double st[kFinalThreads], ss[kFinalThreads];
    double t = 0.0, s = 0.0;
    for (int64_t i = threadIdx.x; i < n_blocks; i += kFinalThreads) {
        t += part[2 * i];
        s += part[2 * i + 1];
    }
    st[threadIdx.x] = t;
    ss[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0, q = 0.0;
        for (int i = 0; i < kFinalThreads; ++i) {
            acc += st[i];
            q += ss[i];
        }
        *loss = (float)((acc + (double)wd * q) / (double)batch_size);
    }
}

// OUT_USERS: output rows X = users (dU), walked rows Y = columns; otherwise X = columns (dI; in-batch dC = dp over dx), Y = users.
// In-batch, the columns' gradient goes to two row blocks: rows < n_first to `out`, the others to `out2`; either may be NULL, and
// a workgroup all of whose rows go nowhere leaves at once.
template <bool OUT_USERS, bool INBATCH>
__global__ __launch_bounds__(256) void softmax_full_grad_kernel(const SoftmaxSides a, const float *__restrict__ lse, float inv_tau, float wd,
                                                                float batch_size, const float *__restrict__ gout, int64_t split_rows,
                                                                float *__restrict__ out, int64_t ldo, float *__restrict__ out2, int64_t ldo2,
                                                                float *__restrict__ part)
{
    constexpr int IT = kRankIT, TK = kRankTK, SLD = TK + 1, GT = kGT, GLD = kGLD;
    constexpr int NI = IT * TK / 256, NU = GT * TK / 256;
    __shared__ float sI[IT * SLD];
    __shared__ float sU[GT * SLD];
    __shared__ float sG[GT * GLD];
    __shared__ float sLse[IT];
    __shared__ int64_t sPos[IT];                            // the walked users' positives; in-batch: the walked rows' ids
    __shared__ int sCnt[INBATCH ? 1 : GT];
    __shared__ float sQ[INBATCH ? IT : 1];                  // in-batch: the walked columns' corrections / the walked users' pos_logq

    const int D = a.D;
    const int64_t n_out = OUT_USERS ? a.B : a.n_items, n_walk = OUT_USERS ? a.n_items : a.B;
    auto x_row = [&](int64_t r) { return OUT_USERS ? a.users + r * a.ldu : col_row<INBATCH>(a, r); };
    auto y_row = [&](int64_t r) { return OUT_USERS ? col_row<INBATCH>(a, r) : a.users + r * a.ldu; };

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int64_t o0 = (int64_t)blockIdx.x * GT;
    if (INBATCH && !OUT_USERS && !part) {
        if (!out && o0 + GT <= a.n_first) return;
        if (!out2 && o0 >= a.n_first) return;
    }
    const int64_t w_begin = (int64_t)blockIdx.y * split_rows;
    const int64_t w_end = w_begin + split_rows < n_walk ? w_begin + split_rows : n_walk;
    const int slab0 = (int)blockIdx.z * kSlab;
    const int slab_end = slab0 + kSlab < D ? slab0 + kSlab : D;
    const bool has_ids = INBATCH && a.ids != nullptr;

    const float g0 = gout[0] / batch_size;
    const float cg = g0 * inv_tau;
    const int64_t orow = o0 + (lane & 31);                  // the lane's output row in phase 1
    const bool orow_ok = orow < n_out;
    float lse_r = 0.f, q_r = 0.f;                           // q_r: the row's pos_logq (dU) / the column's correction (dC)
    int64_t pos_r = -1;                                     // in-batch: the row's / the column's id
    if (OUT_USERS && orow_ok) {
        lse_r = lse[orow];
        if (!INBATCH) pos_r = a.pos[orow];
    }
    if (INBATCH && orow_ok) {
        if (OUT_USERS) {
            pos_r = has_ids ? a.ids[orow] : 0;
            q_r = a.pos_logq ? a.pos_logq[orow] : 0.f;
        } else {
            pos_r = has_ids ? col_id(a, orow) : 0;
            q_r = col_q(a, orow);
        }
    }
    if (!INBATCH && tid < GT) sCnt[tid] = 0;
    int cnt_local = 0;

    f32x16 out_acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) out_acc[q][e] = 0.f;

    const int n_chunks = (D + TK - 1) / TK;
    const int64_t n_tiles = (w_end - w_begin + IT - 1) / IT;
    const int64_t n_steps = n_tiles * n_chunks;
    float pI[NI], pU[NU];
    auto load = [&](int64_t s) {
        const int64_t w0 = w_begin + (s / n_chunks) * IT;
        const int k0 = (int)(s % n_chunks) * TK;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int f = tid + 256 * j, it = f / TK, kk = f % TK;
            const int64_t gw = w0 + it;
            pI[j] = (gw < w_end && k0 + kk < D) ? y_row(gw)[k0 + kk] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int f = tid + 256 * j, r = f / TK, kk = f % TK;
            const int64_t go = o0 + r;
            pU[j] = (go < n_out && k0 + kk < D) ? x_row(go)[k0 + kk] : 0.f;
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
        const int64_t w0 = w_begin + t * IT;
        if (tid < IT) {                                     // what the epilogue needs of the walked rows (read after the K loop's barriers)
            const int64_t w = w0 + tid;
            if (!INBATCH && !OUT_USERS) {
                sLse[tid] = w < w_end ? lse[w] : 0.f;
                sPos[tid] = w < w_end ? a.pos[w] : -1;
            }
            if (INBATCH && OUT_USERS) {
                sPos[tid] = (has_ids && w < w_end) ? col_id(a, w) : 0;
                sQ[tid] = w < w_end ? col_q(a, w) : 0.f;
            }
            if (INBATCH && !OUT_USERS) {
                sLse[tid] = w < w_end ? lse[w] : 0.f;
                sPos[tid] = (has_ids && w < w_end) ? a.ids[w] : 0;
                sQ[tid] = (a.pos_logq && w < w_end) ? a.pos_logq[w] : 0.f;
            }
        }
        // phase 1: the score tile, as the forward computes it
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        for (int c = 0; c < n_chunks; ++c, ++step) {
            __syncthreads();
            store();
            __syncthreads();
            if (step + 1 < n_steps) load(step + 1);
            const float *A = sI + (wave * 32 + (lane & 31)) * SLD + half;
            const float *Bo = sU + (lane & 31) * SLD + half;
#pragma unroll
            for (int s = 0; s < TK / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[2 * s], Bo[2 * s], acc, 0, 0, 0);
        }
        // lane holds output row (lane&31), walked rows 32*wave + (e&3) + 8*(e>>2) + 4*half of the tile
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int il = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
            const int64_t gw = w0 + il;
            const float lb = OUT_USERS ? lse_r : sLse[il];
            float g = 0.f;
            if (INBATCH) {
                const bool diag = gw == orow;
                // dU: the row's pos_logq in q_r, the column's correction in sQ; dC: the other way round
                const float corr = (diag == OUT_USERS) ? q_r : sQ[il];
                const bool masked = has_ids && !diag && sPos[il] == pos_r;
                if (gw < w_end && orow_ok && !masked) {
                    const float z = acc[e] * inv_tau - corr;
                    g = cg * (expf(z - lb) - (diag ? 1.f : 0.f));
                }
            } else {
                const int64_t pb = OUT_USERS ? pos_r : sPos[il];
                const int64_t j = OUT_USERS ? gw : orow;
                const bool hit = j == pb;
                if (gw < w_end && orow_ok) {
                    const float s = acc[e] * inv_tau;
                    g = cg * (expf(s - lb) - (hit ? 1.f : 0.f));
                    if (!OUT_USERS && hit) ++cnt_local;
                }
            }
            sG[(lane & 31) * GLD + il] = g;
        }
        __syncthreads();
        // phase 2: out_acc[32 x slab] += G[32 x 128] . Y[128 x slab]; MFMA step s takes walked rows 2s (lanes 0-31), 2s+1 (32-63)
        const float *Ga = sG + (lane & 31) * GLD + half;
        for (int s0 = 0; s0 < IT / 2; s0 += 8) {
            float bv[8][4];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int64_t gw = w0 + 2 * (s0 + i) + half;
                const float *yr = gw < w_end ? y_row(gw) : nullptr;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int col = slab0 + (q * 4 + wave) * 32 + (lane & 31);
                    bv[i][q] = (yr && col < slab_end) ? yr[col] : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float av = Ga[2 * (s0 + i)];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (slab0 + (q * 4 + wave) * 32 < slab_end)           // wave-uniform
                        out_acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[i][q], out_acc[q], 0, 0, 0);
            }
        }
    }
    // c_j of dI: positives of this piece's users that are the lane's item, counted in integers (in-batch: [j is a walked row])
    __syncthreads();
    if (!INBATCH && !OUT_USERS && cnt_local) atomicAdd(&sCnt[lane & 31], cnt_local);
    __syncthreads();
    const float two_wd_g = 2.f * wd * g0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int col = slab0 + (q * 4 + wave) * 32 + (lane & 31);
        if (col >= slab_end) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = (e & 3) + 8 * (e >> 2) + 4 * half;
            const int64_t row = o0 + r;
            if (row >= n_out) continue;
            float v = out_acc[q][e];
            if (OUT_USERS) {
                if (blockIdx.y == 0) v = fmaf(two_wd_g, x_row(row)[col], v);
            } else if (INBATCH) {
                if (row < a.n_first && row >= w_begin && row < w_end) v = fmaf(two_wd_g, x_row(row)[col], v);
            } else if (sCnt[r]) {
                v = fmaf(two_wd_g * (float)sCnt[r], x_row(row)[col], v);
            }
            if (part) {
                part[((int64_t)blockIdx.y * n_out + row) * D + col] = v;
            } else if (INBATCH && !OUT_USERS && row >= a.n_first) {
                if (out2) out2[(row - a.n_first) * ldo2 + col] = v;
            } else if (out) {
                out[row * ldo + col] = v;
            }
        }
    }
}

// out[row, col] = part[0][row, col] + part[1][row, col] + ..: the pieces in ascending order; a piece is piece_stride floats
__global__ __launch_bounds__(256) void softmax_full_add_pieces_kernel(const float *__restrict__ part, int n_pieces, int64_t piece_stride,
                                                                      int64_t n_rows, int D, float *__restrict__ out, int64_t ldo)
{
    const int64_t total = n_rows * D;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        float acc = part[i];
        for (int q = 1; q < n_pieces; ++q) acc += part[(int64_t)q * piece_stride + i];
        out[(i / D) * ldo + i % D] = acc;
    }
}

struct SoftmaxPlan {
    int64_t fwd_tiles, fwd_pieces, fwd_split;       // forward: user tiles of 64, column pieces
    int64_t du_tiles, du_pieces, du_split;          // dU: user tiles of 32, column pieces
    int64_t di_tiles, di_pieces, di_split;          // dI: column tiles of 32, user pieces
    int64_t slabs;                                  // column slabs of both gradients
};

SoftmaxPlan softmax_plan(int64_t B, int64_t n_items, int D)
{
    SoftmaxPlan p;
    p.fwd_tiles = (B + 63) / 64;
    const ItemSplit f = rank_item_split(p.fwd_tiles, n_items);
    p.fwd_pieces = f.splits;
    p.fwd_split = f.split_items;
    p.du_tiles = (B + kGT - 1) / kGT;
    const ItemSplit u = rank_item_split(p.du_tiles, n_items);
    p.du_pieces = u.splits;
    p.du_split = u.split_items;
    p.di_tiles = (n_items + kGT - 1) / kGT;
    const ItemSplit i = rank_item_split(p.di_tiles, B);
    p.di_pieces = i.splits;
    p.di_split = i.split_items;
    p.slabs = ((int64_t)D + kSlab - 1) / kSlab;
    return p;
}

// out = {forward pieces, 1, dU pieces, dU column slabs, dI pieces, dI column slabs}
void softmax_plan_out(const SoftmaxPlan &p, int64_t out[6])
{
    out[0] = p.fwd_pieces;
    out[1] = 1;                                         // the forward has no output columns
    out[2] = p.du_pieces;
    out[3] = p.slabs;
    out[4] = p.di_pieces;
    out[5] = p.slabs;
}

// workspace layout (256-byte aligned blocks): forward (max, sum) partials and the loss partials; the gradients' piece blocks
struct SoftmaxScratch {
    int64_t part_m, part_l, loss_part, du_part, di_part, total;
};

SoftmaxScratch softmax_scratch(const SoftmaxPlan &p, int64_t B, int64_t n_items, int D)
{
    SoftmaxScratch s;
    int64_t o = 256;                                    // room to align the caller's pointer
    s.part_m = o;
    o += align_up(p.fwd_pieces * B * 4, 256);
    s.part_l = o;
    o += align_up(p.fwd_pieces * B * 4, 256);
    s.loss_part = o;
    o += align_up(((B + 3) / 4) * 2 * 8, 256);
    s.du_part = o;
    if (p.du_pieces > 1) o += align_up(p.du_pieces * B * D * 4, 256);
    s.di_part = o;
    if (p.di_pieces > 1) o += align_up(p.di_pieces * n_items * D * 4, 256);
    s.total = o;
    return s;
}

// The three forward launches.  `who` names the entry point in the error texts.
template <bool INBATCH>
int softmax_launch_forward(const char *who, const SoftmaxSides &a, float inv_tau, float wd, float batch_size, float *loss, float *lse,
                           float *spos, int32_t *status, void *workspace, int64_t workspace_bytes, hipStream_t stream)
{
    const SoftmaxPlan p = softmax_plan(a.B, a.n_items, a.D);
    const SoftmaxScratch sc = softmax_scratch(p, a.B, a.n_items, a.D);
    if (!workspace || workspace_bytes < sc.total)
        return fail(NGCF_ERR_WORKSPACE, "%s: workspace %lld B < %lld B", who, (long long)workspace_bytes, (long long)sc.total);
    if (p.fwd_pieces > 65535) return fail(NGCF_ERR_ARG, "%s: too many item pieces", who);
    char *base = reinterpret_cast<char *>(align_up((int64_t)(uintptr_t)workspace, 256)) - 256;
    float *part_m = reinterpret_cast<float *>(base + sc.part_m), *part_l = reinterpret_cast<float *>(base + sc.part_l);
    double *loss_part = reinterpret_cast<double *>(base + sc.loss_part);
    softmax_full_fwd_kernel<INBATCH><<<dim3((unsigned)p.fwd_tiles, (unsigned)p.fwd_pieces), 256, 0, stream>>>(a, inv_tau, p.fwd_split, part_m,
                                                                                                        part_l, spos, status);
    LAUNCH_CHECK();
    const int64_t row_blocks = (a.B + 3) / 4;
    softmax_full_rows_kernel<INBATCH><<<dim3((unsigned)row_blocks), 256, 0, stream>>>(a, part_m, part_l, (int)p.fwd_pieces, lse, spos, loss_part);
    LAUNCH_CHECK();
    softmax_full_final_kernel<<<1, kFinalThreads, 0, stream>>>(loss_part, row_blocks, wd, batch_size, loss);
    LAUNCH_CHECK();
    return NGCF_OK;
}

// The gradient launches: dU into du (NULL: skipped); the columns' gradient into dcol (rows < n_first) and dcol2 (in-batch: the
// extras' rows), skipped when both are NULL.
template <bool INBATCH>
int softmax_launch_backward(const char *who, const SoftmaxSides &a, const float *lse, float inv_tau, float wd, float batch_size,
                            const float *grad_out, float *du, int64_t lddu, float *dcol, int64_t lddc, float *dcol2, int64_t lddc2,
                            void *workspace, int64_t workspace_bytes, hipStream_t stream)
{
    const int64_t B = a.B, C = a.n_items;
    const int D = a.D;
    const SoftmaxPlan p = softmax_plan(B, C, D);
    const SoftmaxScratch sc = softmax_scratch(p, B, C, D);
    if (!workspace || workspace_bytes < sc.total)
        return fail(NGCF_ERR_WORKSPACE, "%s: workspace %lld B < %lld B", who, (long long)workspace_bytes, (long long)sc.total);
    if (p.du_pieces > 65535 || p.di_pieces > 65535 || p.slabs > 65535) return fail(NGCF_ERR_ARG, "%s: too many pieces", who);
    char *base = reinterpret_cast<char *>(align_up((int64_t)(uintptr_t)workspace, 256)) - 256;
    if (du) {
        float *part = p.du_pieces > 1 ? reinterpret_cast<float *>(base + sc.du_part) : nullptr;
        softmax_full_grad_kernel<true, INBATCH><<<dim3((unsigned)p.du_tiles, (unsigned)p.du_pieces, (unsigned)p.slabs), 256, 0, stream>>>(
            a, lse, inv_tau, wd, batch_size, grad_out, p.du_split, du, lddu, nullptr, 0, part);
        LAUNCH_CHECK();
        if (part) {
            softmax_full_add_pieces_kernel<<<grid_for(B * D, 256), 256, 0, stream>>>(part, (int)p.du_pieces, B * D, B, D, du, lddu);
            LAUNCH_CHECK();
        }
    }
    if (dcol || dcol2) {
        float *part = p.di_pieces > 1 ? reinterpret_cast<float *>(base + sc.di_part) : nullptr;
        softmax_full_grad_kernel<false, INBATCH><<<dim3((unsigned)p.di_tiles, (unsigned)p.di_pieces, (unsigned)p.slabs), 256, 0, stream>>>(
            a, lse, inv_tau, wd, batch_size, grad_out, p.di_split, dcol, lddc, dcol2, lddc2, part);
        LAUNCH_CHECK();
        const int64_t n1 = INBATCH ? a.n_first : C;
        if (part && dcol) {
            softmax_full_add_pieces_kernel<<<grid_for(n1 * D, 256), 256, 0, stream>>>(part, (int)p.di_pieces, C * D, n1, D, dcol, lddc);
            LAUNCH_CHECK();
        }
        if (part && dcol2 && C > n1) {
            softmax_full_add_pieces_kernel<<<grid_for((C - n1) * D, 256), 256, 0, stream>>>(part + n1 * D, (int)p.di_pieces, C * D, C - n1, D,
                                                                                        dcol2, lddc2);
            LAUNCH_CHECK();
        }
    }
    return NGCF_OK;
}

}  // namespace

#endif  // NGCF_SOFTMAX_TILE_DEVICE_H
