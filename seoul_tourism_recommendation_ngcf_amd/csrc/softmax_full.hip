// softmax_full.hip - the softmax loss over the WHOLE catalogue, loss and both gradients, without the [B, n_items] score matrix
// (include/ngcf_hip.h, "Full-catalogue softmax").
//
// Forward.  rank_topk_kernel's score-tile walk (rank.hip: 64 users x 128 items a tile, K in chunks of 32 through LDS, one ascending-k
// fmaf chain per score), restated here as rank_position.hip restates it; instead of a selection every lane keeps a
// running (max, sum of exp) of its user over the 16 scores it holds of each tile, and picks the positive's score up when it passes.
// The eight (wave, lane half) holders of a user merge through LDS in ascending order, the item pieces in a second stage.
//
// Gradients.  One kernel, the roles swapped: a workgroup owns 32 OUTPUT rows (users for dU, items for dI) and a slab of <= 512 output
// columns, and walks the OTHER side in tiles of 128 rows.  Phase 1 recomputes the 128 x 32 score tile over the full D exactly as the
// forward does and writes g = gout/batch_size * inv_tau * (exp(s - lse) - [j == pos]) into LDS, transposed (rows of 129 floats);
// phase 2 is acc[32 x slab] += G[32 x 128] . W[128 x slab] with v_mfma_f32_32x32x2_f32, wave w owning the 32-column blocks
// w, w + 4, w + 8, w + 12 of the slab (64 accumulator registers a lane, kept for the whole walk).  No W element is used by two
// waves, so W goes from memory (L2) straight into the B operand, eight k steps of loads in flight: LDS would add a copy and no re-use.
// No atomics on floats, every sum in a fixed order: loss, lse, dU and dI are the same bits from run to run.
#include "rank_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSlab = 512;                      // output columns of a gradient workgroup: 4 waves x 4 blocks of 32
constexpr int kGT = 32;                         // output rows of a gradient workgroup
constexpr int kGLD = kRankIT + 1;               // row of the transposed g tile in LDS: 129 floats (the 33 of rank.hip, for 128)
constexpr int kFinalThreads = 256;

// (m, l) <- (m, l) merged with (mb, lb): M = max, l = l e^(m - M) + lb e^(mb - M); a maximum of -inf shifts by 0 (e^-inf = 0)
__device__ inline void lse_merge(float &m, float &l, float mb, float lb)
{
    const float M = fmaxf(m, mb);
    const float Ms = M == -INFINITY ? 0.f : M;
    l = l * expf(m - Ms) + lb * expf(mb - Ms);
    m = M;
}

__global__ __launch_bounds__(256) void softmax_full_fwd_kernel(const float *__restrict__ users, int64_t ldu, int64_t B,
                                                               const float *__restrict__ items, int64_t ldi, int64_t n_items, int D,
                                                               const int64_t *__restrict__ pos, float inv_tau, int64_t split_items,
                                                               float *__restrict__ part_m, float *__restrict__ part_l,
                                                               float *__restrict__ spos, int32_t *status)
{
    constexpr int UB = 2, UT = 32 * UB, IT = kRankIT, TK = kRankTK, SLD = TK + 1;
    constexpr int NI = IT * TK / 256, NU = UT * TK / 256;
    __shared__ float sI[IT * SLD];
    __shared__ float sU[UT * SLD];
    __shared__ float pm[8 * UT], pl[8 * UT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * UT;
    const int64_t i_begin = (int64_t)blockIdx.y * split_items;
    const int64_t i_end = i_begin + split_items < n_items ? i_begin + split_items : n_items;

    int64_t upos[UB];
    float m[UB], l[UB];
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) {
        const int64_t b = b0 + ub * 32 + (lane & 31);
        upos[ub] = b < B ? pos[b] : -1;
        m[ub] = -INFINITY;
        l[ub] = 0.f;
    }
    if (tid < UT && blockIdx.y == 0 && b0 + tid < B) {
        const int64_t p = pos[b0 + tid];
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
            pI[j] = (gi < i_end && k0 + kk < D) ? items[gi * ldi + k0 + kk] : 0.f;
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
        rank_f32x16 acc[UB];
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
                const float a = A[2 * s];
#pragma unroll
                for (int ub = 0; ub < UB; ++ub)
                    acc[ub] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bu[ub * 32 * SLD + 2 * s], acc[ub], 0, 0, 0);
            }
        }
        // lane holds user ub*32 + (lane&31), items 32*wave + (e&3) + 8*(e>>2) + 4*(lane>>5) of the tile: e ascending
#pragma unroll
        for (int ub = 0; ub < UB; ++ub) {
            const int64_t b = b0 + ub * 32 + (lane & 31);
            float sc[16];
            float tm = -INFINITY;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int64_t gi = i0 + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                sc[e] = acc[ub][e] * inv_tau;
                if (gi < i_end) {
                    tm = fmaxf(tm, sc[e]);
                    if (gi == upos[ub] && b < B) spos[b] = sc[e];
                }
            }
            const float M = fmaxf(m[ub], tm);
            const float Ms = M == -INFINITY ? 0.f : M;
            float ll = l[ub] * expf(m[ub] - Ms);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int64_t gi = i0 + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                if (gi < i_end) ll += expf(sc[e] - Ms);
            }
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

// One wave per batch row, four per workgroup: the item pieces merged in ascending order, lse = M + log(l), the row's term
// lse - s_pos and its squared norms in fp64; part[2 blk], part[2 blk + 1] = the workgroup's four rows, (r0 + r1) + (r2 + r3).
__global__ __launch_bounds__(256) void softmax_full_rows_kernel(const float *__restrict__ users, int64_t ldu, int64_t B,
                                                                const float *__restrict__ items, int64_t ldi, int64_t n_items, int D,
                                                                const int64_t *__restrict__ pos, const float *__restrict__ part_m,
                                                                const float *__restrict__ part_l, int n_pieces, float *__restrict__ lse,
                                                                float *__restrict__ spos, double *__restrict__ part)
{
    __shared__ double sh[8];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    double term = 0.0, sq = 0.0;
    if (b < B) {
        const int64_t p = pos[b];
        const bool has = p >= 0 && p < n_items;
        double uu = 0.0, pp = 0.0;
        for (int j = lane; j < D; j += 64) {
            const double a = (double)users[b * ldu + j];
            uu += a * a;
            if (has) {
                const double c = (double)items[p * ldi + j];
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
        double a = 0.0, q = 0.0;
        for (int i = 0; i < kFinalThreads; ++i) {
            a += st[i];
            q += ss[i];
        }
        *loss = (float)((a + (double)wd * q) / (double)batch_size);
    }
}

// OUT_USERS: output rows X = users (dU), walked rows Y = items; otherwise X = items (dI), Y = users.
template <bool OUT_USERS>
__global__ __launch_bounds__(256) void softmax_full_grad_kernel(const float *__restrict__ users, int64_t ldu, int64_t B,
                                                                const float *__restrict__ items, int64_t ldi, int64_t n_items, int D,
                                                                const int64_t *__restrict__ pos, const float *__restrict__ lse,
                                                                float inv_tau, float wd, float batch_size,
                                                                const float *__restrict__ gout, int64_t split_rows,
                                                                float *__restrict__ out, int64_t ldo, float *__restrict__ part)
{
    constexpr int IT = kRankIT, TK = kRankTK, SLD = TK + 1, GT = kGT, GLD = kGLD;
    constexpr int NI = IT * TK / 256, NU = GT * TK / 256;
    __shared__ float sI[IT * SLD];
    __shared__ float sU[GT * SLD];
    __shared__ float sG[GT * GLD];
    __shared__ float sLse[IT];
    __shared__ int64_t sPos[IT];
    __shared__ int sCnt[GT];

    const float *__restrict__ X = OUT_USERS ? users : items;
    const float *__restrict__ Y = OUT_USERS ? items : users;
    const int64_t ldx = OUT_USERS ? ldu : ldi, ldy = OUT_USERS ? ldi : ldu;
    const int64_t n_out = OUT_USERS ? B : n_items, n_walk = OUT_USERS ? n_items : B;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int64_t o0 = (int64_t)blockIdx.x * GT;
    const int64_t w_begin = (int64_t)blockIdx.y * split_rows;
    const int64_t w_end = w_begin + split_rows < n_walk ? w_begin + split_rows : n_walk;
    const int slab0 = (int)blockIdx.z * kSlab;
    const int slab_end = slab0 + kSlab < D ? slab0 + kSlab : D;

    const float g0 = gout[0] / batch_size;
    const float cg = g0 * inv_tau;
    const int64_t orow = o0 + (lane & 31);                  // the lane's output row in phase 1
    const bool orow_ok = orow < n_out;
    float lse_r = 0.f;
    int64_t pos_r = -1;
    if (OUT_USERS && orow_ok) {
        lse_r = lse[orow];
        pos_r = pos[orow];
    }
    if (tid < GT) sCnt[tid] = 0;
    int cnt_local = 0;

    rank_f32x16 out_acc[4];
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
            pI[j] = (gw < w_end && k0 + kk < D) ? Y[gw * ldy + k0 + kk] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int f = tid + 256 * j, r = f / TK, kk = f % TK;
            const int64_t go = o0 + r;
            pU[j] = (go < n_out && k0 + kk < D) ? X[go * ldx + k0 + kk] : 0.f;
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
        if (!OUT_USERS && tid < IT) {                       // the walked users' lse and positive (read after the K loop's barriers)
            const int64_t b = w0 + tid;
            sLse[tid] = b < w_end ? lse[b] : 0.f;
            sPos[tid] = b < w_end ? pos[b] : -1;
        }
        // phase 1: the score tile, as the forward computes it
        rank_f32x16 acc;
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
            const int64_t pb = OUT_USERS ? pos_r : sPos[il];
            const int64_t j = OUT_USERS ? gw : orow;
            const bool hit = j == pb;
            float g = 0.f;
            if (gw < w_end && orow_ok) {
                const float s = acc[e] * inv_tau;
                g = cg * (expf(s - lb) - (hit ? 1.f : 0.f));
                if (!OUT_USERS && hit) ++cnt_local;
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
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int col = slab0 + (q * 4 + wave) * 32 + (lane & 31);
                    bv[i][q] = (gw < w_end && col < slab_end) ? Y[gw * ldy + col] : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float a = Ga[2 * (s0 + i)];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (slab0 + (q * 4 + wave) * 32 < slab_end)           // wave-uniform
                        out_acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv[i][q], out_acc[q], 0, 0, 0);
            }
        }
    }
    // c_j of dI: positives of this piece's users that are the lane's item, counted in integers
    __syncthreads();
    if (!OUT_USERS && cnt_local) atomicAdd(&sCnt[lane & 31], cnt_local);
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
                if (blockIdx.y == 0) v = fmaf(two_wd_g, X[row * ldx + col], v);
            } else if (sCnt[r]) {
                v = fmaf(two_wd_g * (float)sCnt[r], X[row * ldx + col], v);
            }
            if (part)
                part[((int64_t)blockIdx.y * n_out + row) * D + col] = v;
            else
                out[row * ldo + col] = v;
        }
    }
}

// out[row, col] = part[0][row, col] + part[1][row, col] + ..: the pieces in ascending order
__global__ __launch_bounds__(256) void softmax_full_add_pieces_kernel(const float *__restrict__ part, int n_pieces, int64_t n_rows, int D,
                                                                      float *__restrict__ out, int64_t ldo)
{
    const int64_t total = n_rows * D;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        float a = part[i];
        for (int q = 1; q < n_pieces; ++q) a += part[(int64_t)q * total + i];
        out[(i / D) * ldo + i % D] = a;
    }
}

struct SoftmaxFullPlan {
    int64_t fwd_tiles, fwd_pieces, fwd_split;       // forward: user tiles of 64, item pieces
    int64_t du_tiles, du_pieces, du_split;          // dU: user tiles of 32, item pieces
    int64_t di_tiles, di_pieces, di_split;          // dI: item tiles of 32, user pieces
    int64_t slabs;                                  // column slabs of both gradients
};

SoftmaxFullPlan softmax_full_plan(int64_t B, int64_t n_items, int D)
{
    SoftmaxFullPlan p;
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

bool shape_ok(int64_t B, int64_t n_items, int D)
{
    return B >= 1 && n_items >= 1 && D >= 1 && B < ((int64_t)1 << 31) && n_items < ((int64_t)1 << 31);
}

// workspace layout (256-byte aligned blocks): forward (max, sum) partials and the loss partials; the gradients' piece blocks
struct SoftmaxFullScratch {
    int64_t part_m, part_l, loss_part, du_part, di_part, total;
};

SoftmaxFullScratch softmax_full_scratch(const SoftmaxFullPlan &p, int64_t B, int64_t n_items, int D)
{
    SoftmaxFullScratch s;
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

}  // namespace

extern "C" int ngcf_softmax_full_plan(int64_t B, int64_t n_items, int D, int64_t out[6])
{
    if (!out) return fail(NGCF_ERR_ARG, "softmax_full_plan: null argument");
    if (!shape_ok(B, n_items, D))
        return fail(NGCF_ERR_ARG, "softmax_full_plan: B=%lld, n_items=%lld, D=%d", (long long)B, (long long)n_items, D);
    const SoftmaxFullPlan p = softmax_full_plan(B, n_items, D);
    out[0] = p.fwd_pieces;
    out[1] = 1;                                         // the forward has no output columns
    out[2] = p.du_pieces;
    out[3] = p.slabs;
    out[4] = p.di_pieces;
    out[5] = p.slabs;
    return NGCF_OK;
}

extern "C" int64_t ngcf_softmax_full_workspace_bytes(int64_t B, int64_t n_items, int D)
{
    if (!shape_ok(B, n_items, D)) return -1;
    return softmax_full_scratch(softmax_full_plan(B, n_items, D), B, n_items, D).total;
}

static int softmax_full_check(const char *who, int64_t ldu, int64_t B, int64_t ldi, int64_t n_items, int D, float inv_tau,
                              float batch_size)
{
    if (!shape_ok(B, n_items, D))
        return fail(NGCF_ERR_ARG, "%s: B=%lld, n_items=%lld, D=%d", who, (long long)B, (long long)n_items, D);
    if (ldu < D || ldi < D) return fail(NGCF_ERR_ARG, "%s: leading dimensions %lld/%lld below D=%d", who, (long long)ldu, (long long)ldi, D);
    if (!(inv_tau > 0.f) || !(inv_tau < INFINITY)) return fail(NGCF_ERR_ARG, "%s: inv_tau=%g is not a positive finite number", who, inv_tau);
    if (!(batch_size > 0.f)) return fail(NGCF_ERR_ARG, "%s: batch_size=%g", who, batch_size);
    return NGCF_OK;
}

extern "C" int ngcf_softmax_full_f32(const float *users, int64_t ldu, int64_t B, const float *items, int64_t ldi, int64_t n_items, int D,
                                     const int64_t *pos, float inv_tau, float wd, float batch_size, float *loss, float *lse,
                                     float *spos, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!users || !items || !pos || !loss || !lse || !spos || !status) return fail(NGCF_ERR_ARG, "softmax_full: null argument");
    if (const int rc = softmax_full_check("softmax_full", ldu, B, ldi, n_items, D, inv_tau, batch_size)) return rc;
    const SoftmaxFullPlan p = softmax_full_plan(B, n_items, D);
    const SoftmaxFullScratch sc = softmax_full_scratch(p, B, n_items, D);
    if (!workspace || workspace_bytes < sc.total)
        return fail(NGCF_ERR_WORKSPACE, "softmax_full: workspace %lld B < %lld B", (long long)workspace_bytes, (long long)sc.total);
    if (p.fwd_pieces > 65535) return fail(NGCF_ERR_ARG, "softmax_full: too many item pieces");
    char *base = reinterpret_cast<char *>(align_up((int64_t)(uintptr_t)workspace, 256)) - 256;
    float *part_m = reinterpret_cast<float *>(base + sc.part_m), *part_l = reinterpret_cast<float *>(base + sc.part_l);
    double *loss_part = reinterpret_cast<double *>(base + sc.loss_part);
    softmax_full_fwd_kernel<<<dim3((unsigned)p.fwd_tiles, (unsigned)p.fwd_pieces), 256, 0, stream>>>(
        users, ldu, B, items, ldi, n_items, D, pos, inv_tau, p.fwd_split, part_m, part_l, spos, status);
    LAUNCH_CHECK();
    const int64_t row_blocks = (B + 3) / 4;
    softmax_full_rows_kernel<<<dim3((unsigned)row_blocks), 256, 0, stream>>>(users, ldu, B, items, ldi, n_items, D, pos, part_m, part_l,
                                                                            (int)p.fwd_pieces, lse, spos, loss_part);
    LAUNCH_CHECK();
    softmax_full_final_kernel<<<1, kFinalThreads, 0, stream>>>(loss_part, row_blocks, wd, batch_size, loss);
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_softmax_full_backward_f32(const float *users, int64_t ldu, int64_t B, const float *items, int64_t ldi,
                                              int64_t n_items, int D, const int64_t *pos, const float *lse, float inv_tau, float wd,
                                              float batch_size, const float *grad_out, float *du, int64_t lddu, float *ditems,
                                              int64_t lddi, void *workspace, int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!users || !items || !pos || !lse || !grad_out || (!du && !ditems)) return fail(NGCF_ERR_ARG, "softmax_full_backward: null argument");
    if (const int rc = softmax_full_check("softmax_full_backward", ldu, B, ldi, n_items, D, inv_tau, batch_size)) return rc;
    if ((du && lddu < D) || (ditems && lddi < D))
        return fail(NGCF_ERR_ARG, "softmax_full_backward: leading dimensions %lld/%lld below D=%d", (long long)lddu, (long long)lddi, D);
    const SoftmaxFullPlan p = softmax_full_plan(B, n_items, D);
    const SoftmaxFullScratch sc = softmax_full_scratch(p, B, n_items, D);
    if (!workspace || workspace_bytes < sc.total)
        return fail(NGCF_ERR_WORKSPACE, "softmax_full_backward: workspace %lld B < %lld B", (long long)workspace_bytes, (long long)sc.total);
    if (p.du_pieces > 65535 || p.di_pieces > 65535 || p.slabs > 65535) return fail(NGCF_ERR_ARG, "softmax_full_backward: too many pieces");
    char *base = reinterpret_cast<char *>(align_up((int64_t)(uintptr_t)workspace, 256)) - 256;
    if (du) {
        float *part = p.du_pieces > 1 ? reinterpret_cast<float *>(base + sc.du_part) : nullptr;
        softmax_full_grad_kernel<true><<<dim3((unsigned)p.du_tiles, (unsigned)p.du_pieces, (unsigned)p.slabs), 256, 0, stream>>>(
            users, ldu, B, items, ldi, n_items, D, pos, lse, inv_tau, wd, batch_size, grad_out, p.du_split, du, lddu, part);
        LAUNCH_CHECK();
        if (part) {
            softmax_full_add_pieces_kernel<<<grid_for(B * D, 256), 256, 0, stream>>>(part, (int)p.du_pieces, B, D, du, lddu);
            LAUNCH_CHECK();
        }
    }
    if (ditems) {
        float *part = p.di_pieces > 1 ? reinterpret_cast<float *>(base + sc.di_part) : nullptr;
        softmax_full_grad_kernel<false><<<dim3((unsigned)p.di_tiles, (unsigned)p.di_pieces, (unsigned)p.slabs), 256, 0, stream>>>(
            users, ldu, B, items, ldi, n_items, D, pos, lse, inv_tau, wd, batch_size, grad_out, p.di_split, ditems, lddi, part);
        LAUNCH_CHECK();
        if (part) {
            softmax_full_add_pieces_kernel<<<grid_for(n_items * D, 256), 256, 0, stream>>>(part, (int)p.di_pieces, n_items, D, ditems, lddi);
            LAUNCH_CHECK();
        }
    }
    return NGCF_OK;
}
