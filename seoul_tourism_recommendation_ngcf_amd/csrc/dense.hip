// dense.hip - the dense half of a layer on the matrix cores, and the fused layer entry point.
//
// Five forward kernels compute the same layer; ngcf_layer_dense_f32 picks one by shape:
//   layer_dense_kernel           staged: rows of LE / E and a chunk of weights through LDS, one barrier per chunk (any shape)
//   layer_dense_resident_kernel  persistent, fp32 weights resident in LDS (97-128 columns, many rows)
//   layer_dense_split_kernel     the same persistent loop on the bf16 matrix cores, exact three-way split (the default there)
//   layer_dense_direct_kernel    256 / 512 columns, at most one workgroup per CU: no operand in LDS
//   layer_dense_tall_kernel      256 / 512 columns, 96-row workgroups; row_scale_kernel normalises afterwards
// What they share is defined once:
//   tile_row()                     accumulator register -> row of the 32 x 32 tile (all five)
//   DenseAct                       LeakyReLU and the two dropout forms of one output element (resident, direct)
//   dense_epilogue<CW, NT, EVAL>   bias, DenseAct, row sums of squares, butterfly, cross-wave exchange, stores (resident, direct; the
//                                  staged and split kernels keep copies of it for their measured speed - see there)
//   fetch_pieces() / zero_tail()   a lane's clamped 16-byte reads of its row; columns past d_in zeroed at use (resident,
//                                  split, direct)
//   dense_persistent_tiles<SPLIT>  the persistent row-tile loop and its look-ahead (resident, split: only the operands differ)
//   pack_bias2()                   2*b1 + b2 (the three pack kernels)
// The fp32 kernels add the k-values of an output element in one order; the epilogue copies and row_scale_kernel (behind tall)
// repeat the summation order of dense_epilogue by hand: bit-identical results (tests/test_parity_gpu.py).
#include "common.h"
#include <type_traits>

// ---------------------------------------------------------------------------------------------
// Dense half of a layer (NGCF.py:131-146) on the fp32 matrix cores.
//
//   M = [LE+E | LE*E] . [W1^T ; W2^T] + (2*b1 + b2)
// The K dimension is walked in chunks of DC = 16 input columns: a chunk contributes 16 "sum" values
// and 16 "product" values per row (KC = 32 k-steps), so LE and E are read exactly once.  Weights are
// packed per call into that chunk order ([n_chunks*32][DOP], zero padded) by pack_weights_kernel.
// v_mfma_f32_32x32x2_f32: exact fp32 FMA chain per output element.
// A workgroup of 4 waves owns BM = 32*RW full rows; waves are arranged RW x CW, each wave NT 32x32 tiles,
// so a whole output row (<= 32*NT*CW columns) lives in one workgroup and the L2 row-normalisation is
// done in registers + one LDS exchange.
// ---------------------------------------------------------------------------------------------
#ifndef NGCF_DC
#define NGCF_DC 16
#endif
#define NGCF_KC (2 * NGCF_DC)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));   // native vector: stays in registers inside lambdas

// bias2[j] = 2*b1[j] + b2[j] for the DOP packed columns (b1 is added twice, NGCF.py:131,133); one workgroup of a pack kernel
__device__ __forceinline__ void pack_bias2(const float *__restrict__ b1, const float *__restrict__ b2, int d_out, int DOP,
                                           float *__restrict__ bias2)
{
    for (int j = threadIdx.x; j < DOP; j += 256) bias2[j] = j < d_out ? (b1[j] + b1[j]) + b2[j] : 0.f;
}

// Row of accumulator register r (0..15) in lane half lh (lane >> 5) of a 32 x 32 MFMA tile whose first row is `base` (the column is
// lane & 31).  The base is added HERE, first, so that the sum keeps one association everywhere (scalar parts first): as
// base + an int helper the staged and tall kernels compiled to different, slower code.
template <class T> __device__ __forceinline__ T tile_row(T base, int r, int lh) { return base + (r & 3) + 8 * (r >> 2) + 4 * lh; }

// What happens to one output element after the bias: LeakyReLU, then message dropout in one of its two forms.
struct DenseAct {
    float leaky, drop_p, keep_scale;
    uint32_t drop_thr;
    uint64_t drop_seed;            // resolved
    const float *drop_mask;        // "reference" mode: the noise tensor nn.Dropout drew on the host (0 or 1/(1-p)), NGCF.py:142
    int64_t ldm, n_rows;
    int d_out;
    __device__ __forceinline__ DenseAct(float leaky_, float drop_p_, uint64_t seed, const float *mask, int64_t ldm_, int64_t n_rows_,
                                        int d_out_)
        : leaky(leaky_), drop_p(drop_p_), keep_scale(drop_p_ > 0.f ? 1.f / (1.f - drop_p_) : 1.f), drop_thr(msg_drop_thr(drop_p_)),
          drop_seed(seed), drop_mask(mask), ldm(ldm_), n_rows(n_rows_), d_out(d_out_)
    {
    }
    __device__ __forceinline__ float operator()(float v, int64_t grow, int col) const
    {
        v = v >= 0.f ? v : leaky * v;
        if (drop_mask) v *= (grow < n_rows && col < d_out) ? drop_mask[grow * ldm + col] : 0.f;
        else if (drop_p > 0.f) v = msg_drop(v, drop_seed, grow, col, drop_thr, keep_scale);
        return v;
    }
};

// The end of a wave's NT 32 x 32 tiles of one row tile: bias, activation and dropout, the L2 norm of the complete output rows,
// and the stores of carry (un-normalised, feeds the next layer; may be null) and norm (the normalised all_E block).
// row0 is the first row of the tile and col0 = cw * NT * 32 the wave's first column; bias(t, col) is the bias of the wave's tile t, column
// col = col0 + t*32 + li (a load by col in the staged kernel, a register by t where it was read ahead).
// CW waves side by side share a row and exchange their partial sums through ssq ([32][CW] floats for this row tile; unused
// when CW == 1) - every wave of the workgroup must arrive.  `full`: every row and column of the tile lies inside the matrix
// (the caller decides for what unit), and the stores need no per-element tests.  EVAL_ARM: a second copy of the first loop
// without the per-element tests of the dropout form, taken in eval mode (the direct kernel has one loop).
// The order of every sum is part of the contract (the fp32 kernels and row_scale_kernel are bit-identical): the squares of a
// lane's columns as an fma chain from 0 in tile order (t outer, r inner), the xor butterfly 1, 2, 4, 8, 16 over the 32 lanes of
// a row, the waves in q order.
struct WaveTile {      // where a wave's NT tiles lie, and the lane in them
    int64_t row0;      // first row of the row tile
    int col0, cw;      // the wave's first column (cw * NT * 32) and its place among the CW waves that share the rows
    int li, lh;        // lane & 31 (column within a tile), lane >> 5 (see tile_row)
};
template <int CW, int NT, bool EVAL_ARM, class Bias>
__device__ __forceinline__ void dense_epilogue(f32x16 (&acc)[NT], Bias bias, const DenseAct &act, const WaveTile &w, float *ssq,
                                               bool full, float *carry, int64_t ldc, float *norm, int64_t ldn)
{
    const int64_t row0 = w.row0;
    const int col0 = w.col0, cw = w.cw, li = w.li, lh = w.lh;
    float rowss[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rowss[r] = 0.f;
    if (EVAL_ARM && !act.drop_mask && !(act.drop_p > 0.f)) {   // eval mode / no message dropout
        const float leaky = act.leaky;
        // the same loop without the per-element tests of the dropout form
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = col0 + t * 32 + li;
            const float bz = bias(t, col);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[t][r] + bz;
                v = v >= 0.f ? v : leaky * v;
                acc[t][r] = v;
                rowss[r] = fmaf(v, v, rowss[r]);
            }
        }
    } else {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = col0 + t * 32 + li;
            const float bz = bias(t, col);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = act(acc[t][r] + bz, tile_row(row0, r, lh), col);
                acc[t][r] = v;
                rowss[r] = fmaf(v, v, rowss[r]);
            }
        }
    }
    // reduce over the 32 lanes that share a row (lanes li = 0..31 within each half)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float s = rowss[r];
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        s += __shfl_xor(s, 8);
        s += __shfl_xor(s, 16);
        rowss[r] = s;
    }
    if constexpr (CW > 1) {
        if (li == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) ssq[tile_row(0, r, lh) * CW + cw] = rowss[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < CW; ++q) s += ssq[tile_row(0, r, lh) * CW + q];
            rowss[r] = s;
        }
    }
    if (full) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float inv = 1.f / fmaxf(sqrtf(rowss[r]), 1e-12f);   // F.normalize eps, NGCF.py:144
            float *nrow = norm + tile_row(row0, r, lh) * ldn + col0 + li;
#pragma unroll
            for (int t = 0; t < NT; ++t) nrow[t * 32] = acc[t][r] * inv;
        }
        if (carry) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float *crow = carry + tile_row(row0, r, lh) * ldc + col0 + li;
#pragma unroll
                for (int t = 0; t < NT; ++t) crow[t * 32] = acc[t][r];
            }
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t grow = tile_row(row0, r, lh);
        if (grow >= act.n_rows) continue;
        const float inv = 1.f / fmaxf(sqrtf(rowss[r]), 1e-12f);   // F.normalize eps, NGCF.py:144
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = col0 + t * 32 + li;
            if (col < act.d_out) {
                const float v = acc[t][r];
                if (carry) carry[grow * ldc + col] = v;
                norm[grow * ldn + col] = v * inv;
            }
        }
    }
}

// A lane's two 16-byte pieces of LE and of E at columns ca and cb of its row.  Columns past d_in (d4 = d_in rounded up to 4) are
// re-read from the row's last float4, so the loads are unconditional, and zero_tail() turns them into zeros at USE: zeroed here,
// the loads would be waited for right where they are issued.
__device__ __forceinline__ void fetch_pieces(const float *le_row, const float *e_row, int ca, int cb, int d4, f32x4 &la, f32x4 &lb,
                                             f32x4 &ea, f32x4 &eb)
{
    const int cca = ca < d4 ? ca : d4 - 4, ccb = cb < d4 ? cb : d4 - 4;
    la = *reinterpret_cast<const f32x4 *>(le_row + cca);
    ea = *reinterpret_cast<const f32x4 *>(e_row + cca);
    lb = *reinterpret_cast<const f32x4 *>(le_row + ccb);
    eb = *reinterpret_cast<const f32x4 *>(e_row + ccb);
}
__device__ __forceinline__ void zero_tail(int ca, int cb, int d_in, f32x4 &la, f32x4 &lb, f32x4 &ea, f32x4 &eb)   // ca < cb
{
    if (cb + 4 > d_in) {                          // only the last chunk of a width that is not a multiple of 16
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (ca + q >= d_in) la[q] = 0.f, ea[q] = 0.f;
            if (cb + q >= d_in) lb[q] = 0.f, eb[q] = 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void pack_weights_kernel(const float *__restrict__ W1, const float *__restrict__ b1,
                                                           const float *__restrict__ W2, const float *__restrict__ b2, int d_in,
                                                           int d_out, int n_chunks, int DOP, int NT, float *__restrict__ Wt,
                                                           float *__restrict__ bias2)
{
    // Wt[chunk][kl][cw][j][t] = weight of output column (cw*NT + t)*32 + j: a lane reads its NT tile values at once.
    // One workgroup per (chunk, 32 packed columns): the 16 input columns of the chunk are read along the rows of W1 / W2
    // (64-byte runs), turned in LDS, and leave as 128-byte runs of the packed row.
    __shared__ float tile[NGCF_KC][33];
    const int groups = DOP / 32;
    const int chunk = blockIdx.x / groups, g = blockIdx.x % groups;
    for (int idx = threadIdx.x; idx < 32 * NGCF_KC; idx += 256) {
        const int w = idx / NGCF_KC, kl = idx % NGCF_KC;
        const int within = g * 32 + w;
        const int t = within % NT, j = (within / NT) % 32, cw = within / (NT * 32);
        const int oc = (cw * NT + t) * 32 + j;
        const int col = chunk * NGCF_DC + (kl % NGCF_DC);
        float v = 0.f;
        if (oc < d_out && col < d_in) v = (kl < NGCF_DC ? W1 : W2)[(int64_t)oc * d_in + col];
        tile[kl][w] = v;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 32 * NGCF_KC; idx += 256) {
        const int kl = idx / 32, w = idx % 32;
        Wt[((int64_t)chunk * NGCF_KC + kl) * DOP + g * 32 + w] = tile[kl][w];
    }
    if (blockIdx.x == 0) pack_bias2(b1, b2, d_out, DOP, bias2);
}

#ifndef NGCF_DENSE_WAVES_PER_EU
#define NGCF_DENSE_WAVES_PER_EU 1
#endif
template <int RW, int CW, int NT, bool ALIGNED, bool FAST>
__global__ __launch_bounds__(256, NGCF_DENSE_WAVES_PER_EU) void layer_dense_kernel(const float *__restrict__ LE, int64_t ldLE,
                                                          const float *__restrict__ Es, int64_t ldE, int64_t n_rows,
                                                          int d_in, int d_out, const float *__restrict__ Wt,
                                                          const float *__restrict__ bias2, int n_chunks,
                                                          float leaky, float drop_p, uint64_t drop_seed_in,
                                                          const float *__restrict__ drop_mask, int64_t ldm,
                                                          float *__restrict__ carry, int64_t ldc,
                                                          float *__restrict__ norm, int64_t ldn)
{
    const uint64_t drop_seed = drop_p > 0.f ? resolve_seed(drop_seed_in) : drop_seed_in;
    constexpr int BM = 32 * RW;
    constexpr int WCOLS = 32 * NT * CW;      // == DOP
    constexpr int XLD = NGCF_KC + 4;         // 36: rows stay 16-B aligned and b128 column reads are conflict-free
    constexpr bool DB = WCOLS <= 128;        // double-buffered LDS (one barrier per chunk) where two blocks still fit a CU
    constexpr int NBUF = DB ? 2 : 1;
    constexpr int SQ = NGCF_DC / 4;          // lanes that cover the input columns of a chunk for one row
    constexpr int RPP = 256 / SQ;            // rows staged per pass of the workgroup
    constexpr int RR = (BM + RPP - 1) / RPP; // X rows staged per thread
    constexpr int WF4 = NGCF_KC * WCOLS / 4;           // float4s of a W chunk
    constexpr int WN = (WF4 + 255) / 256;              // W float4s staged per thread
    __shared__ float Xs[NBUF * BM * XLD];
    __shared__ float Ws[NBUF * NGCF_KC * WCOLS];
    __shared__ float ssq[BM * CW];

    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int rw = wave / CW, cw = wave % CW;
    const int li = lane & 31, lh = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * BM;

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // staging roles: 4 lanes x 4 columns cover the 16 input columns of a chunk for one row
    const int sq = tid % SQ;
    const int sr = tid / SQ;   // 0..RPP-1
    f32x4 xle[RR], xe[RR], wreg[WN];

    auto load_chunk = [&](int chunk) {       // global -> registers
        const int c0 = chunk * NGCF_DC + sq * 4;
        if constexpr (FAST) {   // 16-byte aligned rows padded to a multiple of 4 floats: one float4 per lane and operand
            // branch-free: rows past the end re-read the last row (never stored) and columns past d_in re-read the last
            // float4 of the row and are zeroed (the padding columns of LE hold no defined values), so the loads stay in
            // flight under the MFMAs of the current chunk instead of being waited for inside a conditional
            const int d4 = (d_in + 3) & ~3;
            const int cc = c0 < d4 ? c0 : d4 - 4;
            const bool k0 = c0 < d_in, k1 = c0 + 1 < d_in, k2 = c0 + 2 < d_in, k3 = c0 + 3 < d_in;
#pragma unroll
            for (int rr = 0; rr < RR; ++rr) {
                int64_t grow = row0 + (sr + rr * RPP) % BM;
                grow = grow < n_rows ? grow : n_rows - 1;
                f32x4 a = *reinterpret_cast<const f32x4 *>(LE + grow * ldLE + cc);
                f32x4 b = *reinterpret_cast<const f32x4 *>(Es + grow * ldE + cc);
                a.x = k0 ? a.x : 0.f; a.y = k1 ? a.y : 0.f; a.z = k2 ? a.z : 0.f; a.w = k3 ? a.w : 0.f;
                b.x = k0 ? b.x : 0.f; b.y = k1 ? b.y : 0.f; b.z = k2 ? b.z : 0.f; b.w = k3 ? b.w : 0.f;
                xle[rr] = a;
                xe[rr] = b;
            }
            const f32x4 *srcw = reinterpret_cast<const f32x4 *>(Wt + (int64_t)chunk * NGCF_KC * WCOLS);
#pragma unroll
            for (int i = 0; i < WN; ++i)
                if (WF4 % 256 == 0 || tid + i * 256 < WF4) wreg[i] = srcw[tid + i * 256];
            return;
        }
#pragma unroll
        for (int rr = 0; rr < RR; ++rr) {
            const int r = sr + rr * RPP;
            float le[4] = {0.f, 0.f, 0.f, 0.f}, e[4] = {0.f, 0.f, 0.f, 0.f};
            const int64_t grow = row0 + r;
            if (r < BM && grow < n_rows) {
                if (ALIGNED && c0 + 4 <= d_in) {
                    const float4 a = *reinterpret_cast<const float4 *>(LE + grow * ldLE + c0);
                    const float4 b = *reinterpret_cast<const float4 *>(Es + grow * ldE + c0);
                    le[0] = a.x; le[1] = a.y; le[2] = a.z; le[3] = a.w;
                    e[0] = b.x; e[1] = b.y; e[2] = b.z; e[3] = b.w;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (c0 + q < d_in) {
                            le[q] = LE[grow * ldLE + c0 + q];
                            e[q] = Es[grow * ldE + c0 + q];
                        }
                }
            }
            xle[rr] = f32x4{le[0], le[1], le[2], le[3]};
            xe[rr] = f32x4{e[0], e[1], e[2], e[3]};
        }
        const f32x4 *src = reinterpret_cast<const f32x4 *>(Wt + (int64_t)chunk * NGCF_KC * WCOLS);
#pragma unroll
        for (int i = 0; i < WN; ++i)
            if (WF4 % 256 == 0 || tid + i * 256 < WF4) wreg[i] = src[tid + i * 256];
    };
    auto store_chunk = [&](int buf) {        // registers -> LDS: (LE + E) feeds W1, (LE * E) feeds W2
        float *X = Xs + buf * (BM * XLD);
#pragma unroll
        for (int rr = 0; rr < RR; ++rr) {
            const int r = sr + rr * RPP;
            if (r < BM) {
                const f32x4 a = xle[rr], b = xe[rr];
                *reinterpret_cast<f32x4 *>(X + r * XLD + sq * 4) = a + b;
                *reinterpret_cast<f32x4 *>(X + r * XLD + NGCF_DC + sq * 4) = a * b;
            }
        }
        f32x4 *dst = reinterpret_cast<f32x4 *>(Ws + buf * (NGCF_KC * WCOLS));
#pragma unroll
        for (int i = 0; i < WN; ++i)
            if (WF4 % 256 == 0 || tid + i * 256 < WF4) dst[tid + i * 256] = wreg[i];
    };
    auto compute_chunk = [&](int buf) {      // 32 k-values: 4 blocks of (one b128 A read, 4 x NT-wide B reads, 4*NT MFMAs)
        const float *X = Xs + buf * (BM * XLD) + (rw * 32 + li) * XLD + lh * 4;
        const float *W = Ws + buf * (NGCF_KC * WCOLS) + cw * (32 * NT) + li * NT;
#pragma unroll
        for (int kb = 0; kb < NGCF_KC / 8; ++kb) {
            const f32x4 a4 = *reinterpret_cast<const f32x4 *>(X + kb * 8);
#define NGCF_KSTEP(sx, aval)                                                                                   \
    {                                                                                                          \
        const float *wk = W + (kb * 8 + lh * 4 + sx) * WCOLS;                                                  \
        float bv[NT];                                                                                          \
        _Pragma("unroll") for (int t = 0; t < NT; ++t) bv[t] = wk[t];                                          \
        _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                         \
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(aval, bv[t], acc[t], 0, 0, 0);                       \
    }
            NGCF_KSTEP(0, a4.x) NGCF_KSTEP(1, a4.y) NGCF_KSTEP(2, a4.z) NGCF_KSTEP(3, a4.w)
#undef NGCF_KSTEP
        }
    };

    if (DB) {
        load_chunk(0);
        store_chunk(0);
        __syncthreads();
        for (int chunk = 0; chunk < n_chunks; ++chunk) {
            const bool more = chunk + 1 < n_chunks;
            if (more) load_chunk(chunk + 1);        // global loads fly under the MFMAs
            compute_chunk(chunk & 1);
            if (more) store_chunk((chunk + 1) & 1);
            __syncthreads();
        }
    } else {
        // one LDS buffer (256 / 512 output columns: a chunk of W is 32 / 64 KB): the next chunk waits in registers while this
        // one is multiplied, so the global loads are hidden and only the LDS stores sit between the two barriers
        load_chunk(0);
        store_chunk(0);
        __syncthreads();
        for (int chunk = 0; chunk < n_chunks; ++chunk) {
            const bool more = chunk + 1 < n_chunks;
            if (more) load_chunk(chunk + 1);
            compute_chunk(0);
            __syncthreads();
            if (more) {
                store_chunk(0);
                __syncthreads();
            }
        }
    }

    // This kernel keeps its OWN COPY of dense_epilogue (same sums in the same order), which compiles to the parent's code.
    // Through the shared function, and with tile_row() still adding the base outside, the 32- and 64-column shapes at 1 M
    // rows measured 2.6 % and 2.4 % slower (122.2 against 119.1 us, 273.5 against 267.1 us, outside the spread:
    // profiles/r06_dense_shared_epilogue.txt); the shared function with the present tile_row() has not been timed here.
    // ---- epilogue: bias, LeakyReLU, dropout, row sum of squares
    const float keep_scale = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
    const uint32_t drop_thr = msg_drop_thr(drop_p);
    float rowss[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rowss[r] = 0.f;
    if (!drop_mask && !(drop_p > 0.f)) {
        // eval mode / no message dropout: the same loop without the two per-element tests of the dropout form
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = (cw * NT + t) * 32 + li;
            const float bz = bias2[col];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[t][r] + bz;
                v = v >= 0.f ? v : leaky * v;
                acc[t][r] = v;
                rowss[r] = fmaf(v, v, rowss[r]);
            }
        }
    } else {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = (cw * NT + t) * 32 + li;
            const float bz = bias2[col];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[t][r] + bz;
                v = v >= 0.f ? v : leaky * v;
                if (drop_mask) {       // "reference" mode: the noise tensor nn.Dropout drew on the host (0 or 1/(1-p)), NGCF.py:142
                    const int64_t grow = tile_row(row0 + rw * 32, r, lh);
                    v *= (grow < n_rows && col < d_out) ? drop_mask[grow * ldm + col] : 0.f;
                } else if (drop_p > 0.f) {
                    const int64_t grow = tile_row(row0 + rw * 32, r, lh);
                    v = msg_drop(v, drop_seed, grow, col, drop_thr, keep_scale);
                }
                acc[t][r] = v;
                rowss[r] = fmaf(v, v, rowss[r]);
            }
        }
    }
    // reduce over the 32 lanes that share a row (lanes li = 0..31 within each half)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float s = rowss[r];
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        s += __shfl_xor(s, 8);
        s += __shfl_xor(s, 16);
        rowss[r] = s;
    }
    if (CW > 1) {
        if (li == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = tile_row(rw * 32, r, lh);
                ssq[lr * CW + cw] = rowss[r];
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lr = tile_row(rw * 32, r, lh);
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < CW; ++q) s += ssq[lr * CW + q];
            rowss[r] = s;
        }
    }
    // ---- stores: carry (un-normalised, feeds the next layer) and the normalised all_E block.  A full tile (every row and
    // column inside the matrix: all but the last workgroup) stores without the per-element tests.
    if (row0 + BM <= n_rows && d_out == WCOLS) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t grow = tile_row(row0 + rw * 32, r, lh);
            const float inv = 1.f / fmaxf(sqrtf(rowss[r]), 1e-12f);   // F.normalize eps, NGCF.py:144
            float *nrow = norm + grow * ldn + cw * NT * 32 + li;
#pragma unroll
            for (int t = 0; t < NT; ++t) nrow[t * 32] = acc[t][r] * inv;
        }
        if (carry) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t grow = tile_row(row0 + rw * 32, r, lh);
                float *crow = carry + grow * ldc + cw * NT * 32 + li;
#pragma unroll
                for (int t = 0; t < NT; ++t) crow[t * 32] = acc[t][r];
            }
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t grow = tile_row(row0 + rw * 32, r, lh);
        if (grow >= n_rows) continue;
        const float nrm = fmaxf(sqrtf(rowss[r]), 1e-12f);   // F.normalize eps, NGCF.py:144
        const float inv = 1.f / nrm;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = (cw * NT + t) * 32 + li;
            if (col < d_out) {
                const float v = acc[t][r];
                if (carry) carry[grow * ldc + col] = v;
                norm[grow * ldn + col] = v * inv;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The same layer with the packed weights RESIDENT in LDS and no barrier in the main loop (r02).
// layer_dense_kernel stages the rows of LE / E through LDS, chunk by chunk, for the four waves of a workgroup: one barrier per
// chunk, and the matrix pipe is busy only 51 % of the time (profiles/r02_dense_lab.txt).  Here a wave owns its 32 rows outright:
// each lane reads the two 16-byte pieces of LE and of E it needs for a chunk straight from global memory into the MFMA A layout
// (lane (li, lh) holds input columns c*16 + lh*4 + {0..3} and c*16 + 8 + lh*4 + {0..3} of row li), one chunk ahead; the only shared
// operand is the weight matrix, and all of it (2 d_in x 128 floats <= 147 KB) sits in LDS for the lifetime of a persistent
// workgroup of 8 waves (one per CU).  No __syncthreads after the prologue: a wave in its epilogue or waiting for memory leaves
// the matrix pipe to the other wave of its SIMD.  For d_out in (96, 128], d_in <= 144, 16-byte aligned padded rows.
// ---------------------------------------------------------------------------------------------
constexpr int kResWaves = 8, kResWGs = 256;

// ---------------------------------------------------------------------------------------------
// The same layer on the bf16 matrix cores with an exact three-way split (r05, dense_resident = 4, the default).
// layer_dense_resident_kernel keeps the fp32 matrix pipe ~71 % busy and is bound by it: v_mfma_f32_32x32x2_f32 runs at 1/16 of
// the bf16 rate.  Every fp32 operand is split here as x = h + m + l (h = bf16(x), m = bf16(x - h), l = bf16(x - h - m); both
// residuals are exact in fp32 and the three parts carry the whole significand), and the product is accumulated in fp32 from the
// six terms that matter, smallest first: mm, lh, hl, mh, hm, hh (a bf16 x bf16 product is exact in fp32; the dropped ml, lm, ll
// are below 2^-24 relative).  6 v_mfma_f32_32x32x16_bf16 (32 cycles each) replace 8 v_mfma_f32_32x32x2_f32 (64 cycles each) per
// 16 k-values: 3/8 of the matrix time.  Not bit-identical to the fp32 kernels; error at fp32 level (tests/test_dense_split_gpu.py).
// Weights: pack_weights_split_kernel writes the three parts once per call in the B-fragment layout of 32x32x16 (lane (r, h)
// holds B[k = 8h + j][column r], j = 0..7: 16 contiguous bytes).  All three parts of a 256 x 128 panel are 192 KB and do not fit
// the 160 KB of LDS; h and m (2 x 8 KB per 16-column chunk: 128 KB at d_in = 128, 144 KB at 130 - the footprint of the fp32
// resident kernel) stay resident, and l (64 / 72 KB, L2 resident) is read straight from global memory into registers, one chunk
// ahead.  64-column output panels would fit as well, but a row would then be split over two workgroups and the row norm of the
// epilogue would need a second pass over the output.  A lane reads the 8 input columns c*16 + 8h .. +7 of its row for both
// k-steps of a chunk (k-step 0: the sums, against W1; k-step 1: the products, against W2) and splits them in registers.
// The row loop, look-ahead, epilogue and stores are those of layer_dense_resident_kernel: dense_persistent_tiles<SPLIT>.
// ---------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split3(f32x8 x, bf16x8 &h, bf16x8 &m, bf16x8 &l)
{
    h = __builtin_convertvector(x, bf16x8);                     // round to nearest even (v_cvt_pk_bf16_f32)
    const f32x8 r = x - __builtin_convertvector(h, f32x8);      // exact
    m = __builtin_convertvector(r, bf16x8);
    l = __builtin_convertvector(r - __builtin_convertvector(m, f32x8), bf16x8);
}

// One thread per B fragment (chunk c, k-step s, column tile t, lane): Whm[((c*2 + s)*4 + t)*2 + p][lane] holds part p (h, m), and
// Wl[(c*2 + s)*4 + t][lane] part l, of W_s[t*32 + lane%32][c*16 + 8*(lane/32) + j], j = 0..7 (W_0 = W1, W_1 = W2; zero outside).
__global__ __launch_bounds__(256) void pack_weights_split_kernel(const float *__restrict__ W1, const float *__restrict__ b1,
                                                                 const float *__restrict__ W2, const float *__restrict__ b2,
                                                                 int d_in, int d_out, int n_chunks, bf16x8 *__restrict__ Whm,
                                                                 bf16x8 *__restrict__ Wl, float *__restrict__ bias2)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < n_chunks * 512) {
        const int lane = idx & 63, frag = idx >> 6, t = frag & 3, s = (frag >> 2) & 1, c = frag >> 3;
        const int col = t * 32 + (lane & 31), in0 = c * NGCF_DC + 8 * (lane >> 5);
        const float *w = (s ? W2 : W1) + (int64_t)col * d_in;
        f32x8 x;
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (col < d_out && in0 + j < d_in) ? w[in0 + j] : 0.f;
        bf16x8 h, m, l;
        split3(x, h, m, l);
        Whm[(frag * 2 + 0) * 64 + lane] = h;
        Whm[(frag * 2 + 1) * 64 + lane] = m;
        Wl[idx] = l;
    }
    if (blockIdx.x == 0) pack_bias2(b1, b2, d_out, 128, bias2);
}

// ---------------------------------------------------------------------------------------------
// The persistent row-tile loop of layer_dense_resident_kernel (SPLIT = false) and layer_dense_split_kernel (SPLIT = true).
// Shared: the copy of the LDS-resident weights, row clamping, the two-set look-ahead, the paired chunk loop, the next-tile
// prefetch and the epilogue.  Per operand form: the lane's columns of a chunk, the A fragments, the MFMAs, and the split
// kernel's extra stream (part l of the weights, from global memory).
//   w_lds: what stays in LDS, n_chunks * 16 KB - fp32: [n_chunks * 32][128] floats, the layout of pack_weights_kernel;
//          split: parts h and m of every chunk, [n_chunks * 2 * 4 * 2][64] bf16x8
//   Wl:    split only, part l: fragment (k-step s, column tile t) of chunk c at (c*8 + s*4 + t) * 64 + lane
// ---------------------------------------------------------------------------------------------
template <bool SPLIT>
__device__ __forceinline__ void dense_persistent_tiles(const float *LE, int64_t ldLE, const float *Es, int64_t ldE, int64_t n_rows,
                                                       int d_in, int d_out, const f32x4 *w_lds, const bf16x8 *Wl, const float *bias2,
                                                       int n_chunks, float leaky, float drop_p, uint64_t drop_seed_in,
                                                       const float *drop_mask, int64_t ldm, float *carry, int64_t ldc, float *norm,
                                                       int64_t ldn)
{
    const uint64_t drop_seed = drop_p > 0.f ? resolve_seed(drop_seed_in) : drop_seed_in;
    constexpr int NT = 4, WCOLS = 128;
    // the lane's input columns of chunk c start at c*16 + lh*CA (pieces a) and CB further (pieces b).  fp32: lh*4 + {0..3} and
    // 8 + lh*4 + {0..3}, the MFMA A layout of 32x32x2; split: 8h + {0..3} and 8h + {4..7}, both k-steps of 32x32x16
    constexpr int CA = SPLIT ? 8 : 4, CB = SPLIT ? 4 : 8;
    using AFrag = std::conditional_t<SPLIT, bf16x8[2][3], f32x4[4]>;   // split: [k-step: sums, products][h, m, l]
    // part-l fragments per chunk.  fp32 has none: NL = 1 only gives bl0 / bl1 a legal size - they are never written or read
    // there (fetch_l is empty, chunk_mfma ignores them), which keeps the loop below one text for both forms
    constexpr int NL = SPLIT ? 8 : 1;
    extern __shared__ f32x4 Wres[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, lh = lane >> 5;
    for (int i = tid; i < n_chunks * 1024; i += kResWaves * 64) Wres[i] = w_lds[i];   // once per workgroup
    __syncthreads();
    const int64_t n_tiles = (n_rows + 31) / 32;
    const int d4 = (d_in + 3) & ~3;
    float bz[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bz[t] = bias2[t * 32 + li];
    // Stores and loads share one in-order counter (vmcnt), so a wave that stores its finished tile and THEN asks for the first
    // chunks of its next tile waits for all 256 stores to be acknowledged before its first MFMA: the per-tile cost that no
    // staggering of the waves could hide.  The first two chunks of the next tile are therefore requested BEFORE the epilogue of
    // the current one; by the time anything younger than the stores is waited for, two chunks of MFMAs have passed.
    const int last = n_chunks - 1;
    const int64_t tile_step = (int64_t)gridDim.x * kResWaves;
    auto row_of = [&](int64_t t) {                 // the lane's row of tile t (rows past the end re-read the last row, never stored)
        int64_t g = t * 32 + li;
        return g < n_rows ? g : n_rows - 1;
    };
    auto fetch = [&](const float *le_row, const float *e_row, int c, f32x4 &la, f32x4 &lb, f32x4 &ea, f32x4 &eb) {
        const int ca = c * NGCF_DC + lh * CA;
        fetch_pieces(le_row, e_row, ca, ca + CB, d4, la, lb, ea, eb);
    };
    auto fetch_l = [&](int c, bf16x8 (&bl)[NL]) {
        if constexpr (SPLIT) {
#pragma unroll
            for (int f = 0; f < 8; ++f) bl[f] = Wl[(c * 8 + f) * 64 + lane];
        }
    };
    // Two chunks of look-ahead in two fixed register sets (no rotation copies - a copy of a register that is still being
    // loaded is a wait): the A fragments of a chunk are formed first, which frees its set for the chunk after next.  Chunk c
    // uses set c & 1 of the raw operands (two chunks ahead) and, in the split kernel, of part l (one chunk ahead).
    // Every prefetch is UNCONDITIONAL (past the end the last chunk is read again and never used): behind a branch the
    // compiler cannot count the loads in flight and waits for all of them (s_waitcnt vmcnt(0)) at the next use - the
    // look-ahead then exists in the source only.  The odd last chunk is peeled off the loop for the same reason.
    f32x4 la0, lb0, ea0, eb0, la1, lb1, ea1, eb1;
    bf16x8 bl0[NL], bl1[NL];                         // part l of chunks 0, 2, 4, .. and 1, 3, 5, ..
    auto fetch_tile = [&](int64_t t) {               // the first two chunks of tile t (and its chunk 0 of part l)
        const int64_t g = row_of(t);
        fetch(LE + g * ldLE, Es + g * ldE, 0, la0, lb0, ea0, eb0);
        fetch(LE + g * ldLE, Es + g * ldE, last < 1 ? last : 1, la1, lb1, ea1, eb1);
    };
    fetch_l(0, bl0);
    int64_t tile = (int64_t)blockIdx.x * kResWaves + wave;
    fetch_tile(tile < n_tiles ? tile : 0);
    for (; tile < n_tiles; tile += tile_step) {
        const int64_t row0 = tile * 32;
        const int64_t grow_l = row_of(tile);
        const float *le_row = LE + grow_l * ldLE, *e_row = Es + grow_l * ldE;
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        // the A fragments of a chunk from its raw pieces (taken by value: the zeroing is of the copies)
        auto form = [&](int c, f32x4 la, f32x4 lb, f32x4 ea, f32x4 eb, AFrag &a) {
            const int ca = c * NGCF_DC + lh * CA;
            zero_tail(ca, ca + CB, d_in, la, lb, ea, eb);
            const f32x4 sa = la + ea, sb = lb + eb, pa = la * ea, pb = lb * eb;
            if constexpr (SPLIT) {       // sums (k-step 0) and products (k-step 1), each split into h, m, l
                split3(__builtin_shufflevector(sa, sb, 0, 1, 2, 3, 4, 5, 6, 7), a[0][0], a[0][1], a[0][2]);
                split3(__builtin_shufflevector(pa, pb, 0, 1, 2, 3, 4, 5, 6, 7), a[1][0], a[1][1], a[1][2]);
            } else {
                a[0] = sa, a[1] = sb, a[2] = pa, a[3] = pb;   // k-blocks: sum 0-7, sum 8-15, product 0-7, product 8-15
            }
        };
        auto chunk_mfma = [&](int c, const AFrag &a, const bf16x8 (&bl)[NL]) {
            if constexpr (SPLIT) {       // 48 MFMAs
                const bf16x8 *wc = reinterpret_cast<const bf16x8 *>(Wres) + c * 1024 + lane;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const bf16x8 &ah = a[s][0], &am = a[s][1], &al = a[s][2];
#pragma unroll
                    for (int t = 0; t < NT; ++t) {          // one accumulation chain per tile (32x32x16 needs no interleaving)
                        const bf16x8 bh = wc[((s * 4 + t) * 2 + 0) * 64], bm = wc[((s * 4 + t) * 2 + 1) * 64];
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[s * 4 + t], acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[t], 0, 0, 0);
                    }
                }
            } else {                     // 64 MFMAs
                const float *wc = reinterpret_cast<const float *>(Wres) + li * NT + (int64_t)c * NGCF_KC * WCOLS;
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
                    for (int sx = 0; sx < 4; ++sx) {
                        const f32x4 bv = *reinterpret_cast<const f32x4 *>(wc + (kb * 8 + lh * 4 + sx) * WCOLS);
                        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kb][sx], bv.x, acc[0], 0, 0, 0);
                        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kb][sx], bv.y, acc[1], 0, 0, 0);
                        acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kb][sx], bv.z, acc[2], 0, 0, 0);
                        acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kb][sx], bv.w, acc[3], 0, 0, 0);
                    }
                }
            }
        };
        int c = 0;
        for (; c + 1 < n_chunks; c += 2) {
            {
                AFrag a;
                form(c, la0, lb0, ea0, eb0, a);
                fetch(le_row, e_row, c + 2 < last ? c + 2 : last, la0, lb0, ea0, eb0);   // in flight under two chunks of MFMAs
                fetch_l(c + 1, bl1);
                __builtin_amdgcn_sched_barrier(0);      // (left alone the compiler sinks these loads to just before their use)
                chunk_mfma(c, a, bl0);
            }
            {
                AFrag a;
                form(c + 1, la1, lb1, ea1, eb1, a);
                fetch(le_row, e_row, c + 3 < last ? c + 3 : last, la1, lb1, ea1, eb1);
                fetch_l(c + 2 < last ? c + 2 : last, bl0);
                __builtin_amdgcn_sched_barrier(0);
                chunk_mfma(c + 1, a, bl1);
            }
        }
        if (c < n_chunks) {
            AFrag a;
            form(c, la0, lb0, ea0, eb0, a);
            chunk_mfma(c, a, bl0);
        }
        // the next tile's first two chunks, ahead of this tile's stores (the last tile of a wave re-reads its own)
        fetch_tile(tile + tile_step < n_tiles ? tile + tile_step : tile);
        fetch_l(0, bl0);
        __builtin_amdgcn_sched_barrier(0);
        // wave-local: a wave owns its 32 rows outright
        if constexpr (!SPLIT) {
            // DenseAct is built here, per tile, on purpose: built once above the loop, the split instantiation spilled 25
            // VGPRs instead of 24 (the compiler hoists the division by itself)
            const DenseAct act(leaky, drop_p, drop_seed, drop_mask, ldm, n_rows, d_out);
            const WaveTile w{row0, 0, 0, li, lh};
            const bool full = row0 + 32 <= n_rows && d_out == WCOLS;
            dense_epilogue<1, NT, true>(acc, [&](int t, int) { return bz[t]; }, act, w, nullptr, full, carry, ldc, norm, ldn);
        } else {
            // The split kernel keeps its OWN COPY of dense_epilogue<1, NT, true> (same sums in the same order).  Through the
            // shared function its schedule after the next-tile prefetch changed and the C3 forward (three layers on this kernel,
            // eval arm) was slower than the parent in 7 of 8 alternated runs, by 0.09 - 0.18 ms of 10.7 ms
            // (profiles/r06_dense_shared_epilogue.txt); with the text here the fp32 instantiation in turn spilled 2 VGPRs,
            // hence the two forms.
            const float keep_scale = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
            const uint32_t drop_thr = msg_drop_thr(drop_p);
            float rowss[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) rowss[r] = 0.f;
            const bool any_drop = drop_mask || drop_p > 0.f;
            if (!any_drop) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = acc[t][r] + bz[t];
                        v = v >= 0.f ? v : leaky * v;
                        acc[t][r] = v;
                        rowss[r] = fmaf(v, v, rowss[r]);
                    }
            } else {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int col = t * 32 + li;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = acc[t][r] + bz[t];
                        v = v >= 0.f ? v : leaky * v;
                        const int64_t grow = tile_row(row0, r, lh);
                        if (drop_mask) v *= (grow < n_rows && col < d_out) ? drop_mask[grow * ldm + col] : 0.f;
                        else v = msg_drop(v, drop_seed, grow, col, drop_thr, keep_scale);
                        acc[t][r] = v;
                        rowss[r] = fmaf(v, v, rowss[r]);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float s2 = rowss[r];
                s2 += __shfl_xor(s2, 1);
                s2 += __shfl_xor(s2, 2);
                s2 += __shfl_xor(s2, 4);
                s2 += __shfl_xor(s2, 8);
                s2 += __shfl_xor(s2, 16);
                rowss[r] = s2;
            }
            if (row0 + 32 <= n_rows && d_out == WCOLS) {          // full tile: no per-element tests
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t grow = tile_row(row0, r, lh);
                    const float inv = 1.f / fmaxf(sqrtf(rowss[r]), 1e-12f);   // F.normalize eps, NGCF.py:144
                    float *nrow = norm + grow * ldn + li;
#pragma unroll
                    for (int t = 0; t < NT; ++t) nrow[t * 32] = acc[t][r] * inv;
                }
                if (carry) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float *crow = carry + tile_row(row0, r, lh) * ldc + li;
#pragma unroll
                        for (int t = 0; t < NT; ++t) crow[t * 32] = acc[t][r];
                    }
                }
                continue;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t grow = tile_row(row0, r, lh);
                if (grow >= n_rows) continue;
                const float inv = 1.f / fmaxf(sqrtf(rowss[r]), 1e-12f);   // F.normalize eps, NGCF.py:144
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int col = t * 32 + li;
                    if (col < d_out) {
                        const float v = acc[t][r];
                        if (carry) carry[grow * ldc + col] = v;
                        norm[grow * ldn + col] = v * inv;
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(kResWaves * 64) void layer_dense_resident_kernel(
    const float *__restrict__ LE, int64_t ldLE, const float *__restrict__ Es, int64_t ldE, int64_t n_rows, int d_in, int d_out,
    const float *__restrict__ Wt, const float *__restrict__ bias2, int n_chunks, float leaky, float drop_p, uint64_t drop_seed_in,
    const float *__restrict__ drop_mask, int64_t ldm, float *__restrict__ carry, int64_t ldc, float *__restrict__ norm, int64_t ldn)
{
    dense_persistent_tiles<false>(LE, ldLE, Es, ldE, n_rows, d_in, d_out, reinterpret_cast<const f32x4 *>(Wt), nullptr, bias2,
                                  n_chunks, leaky, drop_p, drop_seed_in, drop_mask, ldm, carry, ldc, norm, ldn);
}

__global__ __launch_bounds__(kResWaves * 64) void layer_dense_split_kernel(
    const float *__restrict__ LE, int64_t ldLE, const float *__restrict__ Es, int64_t ldE, int64_t n_rows, int d_in, int d_out,
    const bf16x8 *__restrict__ Whm, const bf16x8 *__restrict__ Wl, const float *__restrict__ bias2, int n_chunks, float leaky,
    float drop_p, uint64_t drop_seed_in, const float *__restrict__ drop_mask, int64_t ldm, float *__restrict__ carry, int64_t ldc,
    float *__restrict__ norm, int64_t ldn)
{
    dense_persistent_tiles<true>(LE, ldLE, Es, ldE, n_rows, d_in, d_out, reinterpret_cast<const f32x4 *>(Whm), Wl, bias2, n_chunks,
                                 leaky, drop_p, drop_seed_in, drop_mask, ldm, carry, ldc, norm, ldn);
}

// Two resident variants (two row tiles per wave; stores under the next tile's K loop) were slower: profiles/r03_dense_il_lab.txt

// ---------------------------------------------------------------------------------------------
// 256 / 512 output columns with NO operand in LDS (r02).  At these widths a workgroup of layer_dense_kernel owns 32 (or 64) rows
// and each of its waves its own 128 output columns: the weights a wave multiplies by are shared with nobody, yet a 32 / 64 KB
// chunk of them goes through the one LDS buffer per chunk between two barriers, and with a few thousand rows (the Seoul graph:
// 186 workgroups, one wave per SIMD) nothing hides that.  Here a wave reads its B operands - the lane's four tile values of a
// k-pair are 16 contiguous bytes of the packed row - straight from the L2-resident packed matrix into registers, one chunk ahead
// in two fixed register sets, and its A operands like layer_dense_resident_kernel; the only LDS traffic is the exchange of the
// row sums of squares at the end.  Same k order per output element as the other two kernels: bit-identical results.
// ---------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int NT> struct TileVec;
template <> struct TileVec<4> { using type = f32x4; };
template <> struct TileVec<2> { using type = f32x2; };

template <int CW, int NT>
__global__ __launch_bounds__(CW * 64) void layer_dense_direct_kernel(
    const float *__restrict__ LE, int64_t ldLE, const float *__restrict__ Es, int64_t ldE, int64_t n_rows, int d_in, int d_out,
    const float *__restrict__ Wt, const float *__restrict__ bias2, int n_chunks, float leaky, float drop_p, uint64_t drop_seed_in,
    const float *__restrict__ drop_mask, int64_t ldm, float *__restrict__ carry, int64_t ldc, float *__restrict__ norm, int64_t ldn)
{
    const uint64_t drop_seed = drop_p > 0.f ? resolve_seed(drop_seed_in) : drop_seed_in;
    constexpr int WCOLS = 32 * NT * CW;            // weights packed with this NT: a lane's NT tile values are contiguous
    using BV = typename TileVec<NT>::type;
    __shared__ float ssq[32 * CW];
    const int tid = threadIdx.x, cw = tid >> 6, lane = tid & 63;
    const int li = lane & 31, lh = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * 32;
    int64_t grow_l = row0 + li;
    grow_l = grow_l < n_rows ? grow_l : n_rows - 1;              // rows past the end re-read the last row, never stored
    const float *le_row = LE + grow_l * ldLE, *e_row = Es + grow_l * ldE;
    const int d4 = (d_in + 3) & ~3;
    const float *Wl = Wt + (int64_t)lh * 4 * WCOLS + cw * (32 * NT) + li * NT;   // k-pair (kb, sx) of chunk c: + ((c*32 + kb*8 + sx) * WCOLS)
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    auto fetch_a = [&](int c, f32x4 &la, f32x4 &lb, f32x4 &ea, f32x4 &eb) {    // columns c*16 + lh*4 and 8 further, as the fp32 resident kernel
        const int ca = c * NGCF_DC + lh * 4;
        fetch_pieces(le_row, e_row, ca, ca + 8, d4, la, lb, ea, eb);
    };
    auto fetch_b = [&](int c, BV (&b)[16]) {
        const float *wc = Wl + (int64_t)c * NGCF_KC * WCOLS;
#pragma unroll
        for (int q = 0; q < 16; ++q) b[q] = *reinterpret_cast<const BV *>(wc + ((q >> 2) * 8 + (q & 3)) * WCOLS);
    };
    auto form = [&](int c, f32x4 la, f32x4 lb, f32x4 ea, f32x4 eb, f32x4 (&a4)[4]) {
        const int ca = c * NGCF_DC + lh * 4;
        zero_tail(ca, ca + 8, d_in, la, lb, ea, eb);
        a4[0] = la + ea, a4[1] = lb + eb, a4[2] = la * ea, a4[3] = lb * eb;
    };
    auto chunk_mfma = [&](const f32x4 (&a4)[4], const BV (&b)[16]) {
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int sx = 0; sx < 4; ++sx) {
                const BV bv = b[kb * 4 + sx];
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[kb][sx], bv[t], acc[t], 0, 0, 0);
            }
    };
    // every prefetch unconditional, the odd last chunk peeled off (see dense_persistent_tiles)
    const int last = n_chunks - 1;
    f32x4 la0, lb0, ea0, eb0, la1, lb1, ea1, eb1;
    BV b0[16], b1[16];
    fetch_a(0, la0, lb0, ea0, eb0);
    fetch_b(0, b0);
    fetch_a(last < 1 ? last : 1, la1, lb1, ea1, eb1);
    fetch_b(last < 1 ? last : 1, b1);
    int c = 0;
    for (; c + 1 < n_chunks; c += 2) {
        {
            f32x4 a4[4];
            form(c, la0, lb0, ea0, eb0, a4);
            fetch_a(c + 2 < last ? c + 2 : last, la0, lb0, ea0, eb0);
            __builtin_amdgcn_sched_barrier(0);
            chunk_mfma(a4, b0);
            fetch_b(c + 2 < last ? c + 2 : last, b0);          // in flight under the next chunk's MFMAs
            __builtin_amdgcn_sched_barrier(0);
        }
        {
            f32x4 a4[4];
            form(c + 1, la1, lb1, ea1, eb1, a4);
            fetch_a(c + 3 < last ? c + 3 : last, la1, lb1, ea1, eb1);
            __builtin_amdgcn_sched_barrier(0);
            chunk_mfma(a4, b1);
            fetch_b(c + 3 < last ? c + 3 : last, b1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (c < n_chunks) {
        f32x4 a4[4];
        form(c, la0, lb0, ea0, eb0, a4);
        chunk_mfma(a4, b0);
    }
    // one activation loop and no full-tile store path here, as this kernel always had
    const DenseAct act(leaky, drop_p, drop_seed, drop_mask, ldm, n_rows, d_out);
    float bz[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bz[t] = bias2[(cw * NT + t) * 32 + li];
    const WaveTile w{row0, cw * NT * 32, cw, li, lh};
    dense_epilogue<CW, NT, false>(acc, [&](int t, int) { return bz[t]; }, act, w, ssq, /*full=*/false, carry, ldc, norm, ldn);
}

// ---------------------------------------------------------------------------------------------
// 256 / 512 output columns on a FEW THOUSAND rows, balanced over the whole chip (r03; VERDICT r2 #7: the Seoul shape).
// layer_dense_direct_kernel gives a workgroup 32 complete rows: 5 940 rows are 186 workgroups on 256 CUs and every wave multiplies
// 32 rows x 128 columns x K - 2 060 MFMAs at 515 -> 512, 55 us before anything else.  What balances is three 32 x 32 tiles per
// SIMD: 186 x 16 tiles / 1 024 SIMDs = 2.9.  Here a workgroup owns 96 rows x 128 columns and each of its four waves THREE row
// tiles of ONE 32-column tile (62 x 4 = 248 workgroups, 1 545 MFMAs per wave = 41 us): the rows of LE / E go through LDS once per
// workgroup (sums and products formed on the way in, double-buffered, one barrier per chunk) and feed all four waves; a wave's
// weights come straight from the packed matrix (a lane's four k-values of a k-block are 16 contiguous bytes: pack_weights_tall_kernel),
// one chunk ahead.  A row is no longer complete inside a workgroup, so the kernel writes the activated values into BOTH outputs
// and row_scale_kernel turns the `norm` rows into unit rows in place - adding the squares in exactly the order the other dense
// kernels use (per 128-column panel: four columns 32 apart per lane, butterfly over 32 lanes; panels in order), so the results
// are bit-identical to theirs.
// ---------------------------------------------------------------------------------------------
constexpr int kTallRows = 96;

// Wp[chunk][ct][kb][lh][li][sx] = packed k-row kb*8 + lh*4 + sx (0..15: W1 column chunk*16 + kl, 16..31: W2 column chunk*16 + kl - 16)
// of output column ct*32 + li; zero outside the matrices
__global__ __launch_bounds__(256) void pack_weights_tall_kernel(const float *__restrict__ W1, const float *__restrict__ b1,
                                                                const float *__restrict__ W2, const float *__restrict__ b2, int d_in,
                                                                int d_out, int DOP, float *__restrict__ Wp, float *__restrict__ bias2)
{
    __shared__ float tile[NGCF_KC][33];
    const int n_ct = DOP / 32;
    const int chunk = blockIdx.x / n_ct, ct = blockIdx.x % n_ct;
    for (int idx = threadIdx.x; idx < 32 * NGCF_KC; idx += 256) {
        const int j = idx / NGCF_KC, kl = idx % NGCF_KC;          // consecutive threads: consecutive input columns of one output row
        const int oc = ct * 32 + j, col = chunk * NGCF_DC + (kl % NGCF_DC);
        float v = 0.f;
        if (oc < d_out && col < d_in) v = (kl < NGCF_DC ? W1 : W2)[(int64_t)oc * d_in + col];
        tile[kl][j] = v;
    }
    __syncthreads();
    float *dst = Wp + ((int64_t)chunk * n_ct + ct) * (32 * NGCF_KC);
    for (int idx = threadIdx.x; idx < 32 * NGCF_KC; idx += 256) {
        const int sx = idx & 3, li = (idx >> 2) & 31, lh = (idx >> 7) & 1, kb = idx >> 8;
        dst[idx] = tile[kb * 8 + lh * 4 + sx][li];
    }
    if (blockIdx.x == 0) pack_bias2(b1, b2, d_out, DOP, bias2);
}

__global__ __launch_bounds__(256) void layer_dense_tall_kernel(
    const float *__restrict__ LE, int64_t ldLE, const float *__restrict__ Es, int64_t ldE, int64_t n_rows, int d_in, int d_out,
    const float *__restrict__ Wp, const float *__restrict__ bias2, int n_chunks, int n_ct, float leaky, float drop_p,
    uint64_t drop_seed_in, const float *__restrict__ drop_mask, int64_t ldm, float *__restrict__ carry, int64_t ldc,
    float *__restrict__ norm, int64_t ldn)
{
    const uint64_t drop_seed = drop_p > 0.f ? resolve_seed(drop_seed_in) : drop_seed_in;
    constexpr int XLD = NGCF_KC + 4;               // 36: [16 sums | 16 products | pad], b128 reads of a column block conflict-free
    constexpr int MT = kTallRows / 32;             // row tiles per wave
    constexpr int XBUF = kTallRows * XLD;          // floats of one LDS buffer
    __shared__ float Xs[3 * XBUF];                 // THREE buffers: see the step comment below
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, lh = lane >> 5;
    const int n_cp = n_ct / 4;
    const int64_t row0 = (int64_t)(blockIdx.x / n_cp) * kTallRows;
    const int ct = (blockIdx.x % n_cp) * 4 + wave;                    // the wave's 32-column tile
    const int d4 = (d_in + 3) & ~3;
    // staging: 96 rows x 4 pieces of 16 bytes per operand and chunk = 384 pieces: thread t takes pieces t and t + 256 (< 384)
    const bool two = tid < 384 - 256;
    int64_t grow_a = row0 + (tid >> 2), grow_b = row0 + 64 + (tid >> 2);
    grow_a = grow_a < n_rows ? grow_a : n_rows - 1;                   // rows past the end re-read the last row, never stored
    grow_b = two ? (grow_b < n_rows ? grow_b : n_rows - 1) : grow_a;
    const int sq4 = (tid & 3) * 4;
    const float *le_a = LE + grow_a * ldLE + sq4, *e_a = Es + grow_a * ldE + sq4, *le_b = LE + grow_b * ldLE + sq4, *e_b = Es + grow_b * ldE + sq4;
    const int last = n_chunks - 1;
    const int cc_last = (last * NGCF_DC + sq4 < d4 ? last * NGCF_DC + sq4 : d4 - 4) - sq4;   // the last chunk may reach past the padded width
    struct XRegs { f32x4 al, ae, bl, be; };     // a thread's pieces of one chunk: rows tid / 4 and 64 + tid / 4
    XRegs x0, x1;                               // TWO chunks in flight: the rows come from beyond the L2 (12 MB each on the Seoul graph),
                                                // one chunk of MFMAs (1.3 us) does not cover that latency
    auto load_x = [&](int c, XRegs &x) {        // c <= last (callers clamp); every load unconditional (a load behind a branch cannot be counted)
        const int off = c < last ? c * NGCF_DC : cc_last;
        x.al = *reinterpret_cast<const f32x4 *>(le_a + off);
        x.ae = *reinterpret_cast<const f32x4 *>(e_a + off);
        x.bl = *reinterpret_cast<const f32x4 *>(le_b + off);
        x.be = *reinterpret_cast<const f32x4 *>(e_b + off);
    };
    float *xs_w = Xs + (tid >> 2) * XLD + sq4;
    auto store_x = [&](int c, int buf, XRegs x) {
        if (c == last) {                        // only the last chunk can hold columns past d_in: they contribute zeros
            const int c0 = c * NGCF_DC + sq4;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (c0 + q >= d_in) x.al[q] = 0.f, x.ae[q] = 0.f, x.bl[q] = 0.f, x.be[q] = 0.f;
        }
        float *xr = xs_w + buf * XBUF;
        *reinterpret_cast<f32x4 *>(xr) = x.al + x.ae;
        *reinterpret_cast<f32x4 *>(xr + NGCF_DC) = x.al * x.ae;
        if (two) {
            *reinterpret_cast<f32x4 *>(xr + 64 * XLD) = x.bl + x.be;
            *reinterpret_cast<f32x4 *>(xr + 64 * XLD + NGCF_DC) = x.bl * x.be;
        }
    };
    const float *wl = Wp + (int64_t)ct * (32 * NGCF_KC) + lane * 4;    // chunk c, k-block kb: + c * n_ct * 1024 + kb * 256
    const int64_t wstep = (int64_t)n_ct * (32 * NGCF_KC);
    f32x4 b0[4], b1[4];
    auto load_b = [&](int c, f32x4 (&b)[4]) {
        const float *w = wl + (int64_t)c * wstep;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) b[kb] = *reinterpret_cast<const f32x4 *>(w + kb * 256);
    };
    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
    const float *xs_r = Xs + li * XLD + lh * 4;
    auto read_a = [&](int buf, int kb, f32x4 (&a)[MT]) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
            a[m] = *reinterpret_cast<const f32x4 *>(xs_r + buf * XBUF + m * 32 * XLD + (kb >> 1) * NGCF_DC + (kb & 1) * 8);
    };
    // One wave per SIMD: nobody else covers a latency, so every operand is requested a step ahead.
    // At the top of step c: LDS buffers c % 3 and (c + 1) % 3 hold chunks c and c + 1; `an` holds the first k-block of chunk c
    // (read from LDS at the end of step c - 1); register set c & 1 holds the rows of chunk c + 2 and set (c + 1) & 1 those of
    // chunk c + 3 (in flight).  Step c: the MFMAs of chunk c (k-block kb + 1 read from LDS before the MFMAs of k-block kb);
    // chunk c + 2 goes into buffer (c + 2) % 3 (last read in step c - 1, a barrier ago); chunk c + 4 is requested; the first
    // k-block of chunk c + 1 is read; ONE barrier.  With three buffers the first LDS reads of a chunk are issued BEFORE the
    // barrier that ends the previous step, not after it.  Chunk indices past the end are clamped (re-read, never multiplied).
    auto cl = [&](int c) { return c < last ? c : last; };
    f32x4 an[MT];
    auto step = [&](int c, int buf, const f32x4 (&b)[4], XRegs &x) {
        f32x4 a0[MT], a1[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) a0[m] = an[m];
#pragma unroll
        for (int kb = 0; kb < 4; kb += 2) {
            read_a(buf, kb + 1, a1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int sx = 0; sx < 4; ++sx)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[m][sx], b[kb][sx], acc[m], 0, 0, 0);
            if (kb + 2 < 4) read_a(buf, kb + 2, a0);
            else {
                const int b2 = buf >= 1 ? buf - 1 : 2;                 // (c + 2) % 3
                store_x(cl(c + 2), b2, x);
                load_x(cl(c + 4), x);
                read_a(buf == 2 ? 0 : buf + 1, 0, an);                 // chunk c + 1, written a step ago
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int sx = 0; sx < 4; ++sx)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[m][sx], b[kb + 1][sx], acc[m], 0, 0, 0);
        }
    };
    load_x(0, x0);
    load_b(0, b0);
    load_x(cl(1), x1);
    load_b(cl(1), b1);
    store_x(0, 0, x0);
    load_x(cl(2), x0);
    store_x(cl(1), 1, x1);
    load_x(cl(3), x1);
    __syncthreads();
    read_a(0, 0, an);
    int buf = 0;
    int c = 0;
    for (; c + 1 < n_chunks; c += 2) {
        step(c, buf, b0, x0);
        load_b(cl(c + 2), b0);
        __syncthreads();
        buf = buf == 2 ? 0 : buf + 1;
        step(c + 1, buf, b1, x1);
        load_b(cl(c + 3), b1);
        __syncthreads();
        buf = buf == 2 ? 0 : buf + 1;
    }
    if (c < n_chunks) step(c, buf, b0, x0);
    // ---- epilogue: bias, LeakyReLU, dropout; the activated value goes to both outputs (row_scale_kernel finishes `norm`)
    // (its own text, not DenseAct, which compiles to the parent's code: with DenseAct and tile_row() adding the base outside,
    // 100 000 x 512 -> 512 measured 1 042.3 against 1 036.9 us, spread 1.8; DenseAct with the present tile_row() was not timed)
    const float keep_scale = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
    const uint32_t drop_thr = msg_drop_thr(drop_p);
    const int col = ct * 32 + li;
    const float bz = bias2[col];
    if (col >= d_out) return;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t grow = tile_row(row0 + m * 32, r, lh);
            if (grow >= n_rows) continue;
            float v = acc[m][r] + bz;
            v = v >= 0.f ? v : leaky * v;
            if (drop_mask) v *= drop_mask[grow * ldm + col];          // "reference" mode: the noise tensor nn.Dropout drew, NGCF.py:142
            else if (drop_p > 0.f) {
                v = msg_drop(v, drop_seed, grow, col, drop_thr, keep_scale);
            }
            if (carry) carry[grow * ldc + col] = v;
            norm[grow * ldn + col] = v;
        }
}

// norm[row, :] /= max(||norm[row, :]||, 1e-12) (F.normalize, NGCF.py:144), one wave per row.  The squares are added exactly as
// the dense kernels add them: per panel of 128 columns lane li takes columns li, 32 + li, 64 + li, 96 + li in that order (fma
// chain from 0), the 32 lanes are combined by the xor butterfly 1, 2, 4, 8, 16, and the panel sums are added in panel order.
template <int CW>      // panels: 2 (<= 256 columns) or 4
__global__ __launch_bounds__(256) void row_scale_kernel(float *__restrict__ norm, int64_t ldn, int64_t n_rows, int d_out)
{
    const int lane = threadIdx.x & 63, li = lane & 31, half = lane >> 5;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    float *x = norm + row * ldn;
    constexpr int PP = CW / 2;                     // panels per lane half: half h takes panels h, h + 2
    float v[PP][4], part[PP];
#pragma unroll
    for (int p = 0; p < PP; ++p) {
        const int cw = half + 2 * p;
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = cw * 128 + t * 32 + li;
            v[p][t] = col < d_out ? x[col] : 0.f;
            s = fmaf(v[p][t], v[p][t], s);
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        s += __shfl_xor(s, 8);
        s += __shfl_xor(s, 16);
        part[p] = s;
    }
    // panel order 0, 1, 2, 3: this half holds panels half, half + 2, the other one the rest
    float other[PP];
#pragma unroll
    for (int p = 0; p < PP; ++p) other[p] = __shfl_xor(part[p], 32);
    float ss = 0.f;
#pragma unroll
    for (int p = 0; p < PP; ++p) {
        const float even = half == 0 ? part[p] : other[p], odd = half == 0 ? other[p] : part[p];
        ss += even;
        ss += odd;
    }
    const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int p = 0; p < PP; ++p)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = (half + 2 * p) * 128 + t * 32 + li;
            if (col < d_out) x[col] = v[p][t] * inv;
        }
}

static int dense_dop(int d_out)
{
    if (d_out <= 32) return 32;
    if (d_out <= 64) return 64;
    if (d_out <= 96) return 96;
    if (d_out <= 128) return 128;
    if (d_out <= 256) return 256;
    if (d_out <= 512) return 512;
    return -1;
}

extern "C" int64_t ngcf_dense_workspace_bytes(int d_in, int d_out)
{
    int dop = dense_dop(d_out);
    if (dop < 0 || d_in <= 0) return -1;
    dop = std::max(dop, 128);                  // small matrices run narrow layers on 32-row x 128-column tiles
    const int64_t n_chunks = (d_in + NGCF_DC - 1) / NGCF_DC;
    const int64_t fp32_packed = (n_chunks * NGCF_KC * dop + dop) * (int64_t)sizeof(float);
    const int64_t split_packed = 128 * (int64_t)sizeof(float) + n_chunks * 3 * 8 * 1024;   // bias, parts h + m, part l
    return align_up(std::max(fp32_packed, split_packed), 256) + 256;
}

// The arguments every forward kernel takes, around the kernel's own weight arguments w... (the kernels keep plain parameter
// lists: a struct would change every kernel's argument loads).
struct DenseCall {
    const float *LE;
    int64_t ldLE;
    const float *Es;
    int64_t ldE, n_rows;
    int d_in, d_out;
    float leaky, drop_p;
    uint64_t drop_seed;
    const float *drop_mask;
    int64_t ldm;
    float *carry;
    int64_t ldc;
    float *norm;
    int64_t ldn;
    hipStream_t stream;
    template <class Kernel, class... W> void launch(Kernel kernel, int64_t grid, int block, size_t lds, W... w) const
    {
        kernel<<<dim3((unsigned)grid), block, lds, stream>>>(LE, ldLE, Es, ldE, n_rows, d_in, d_out, w..., leaky, drop_p, drop_seed, drop_mask,
                                                             ldm, carry, ldc, norm, ldn);
    }
};

template <int RW, int CW, int NT>   // the staged kernel; padded: 16-byte aligned rows padded to a multiple of 4 floats (any d_in)
static void launch_staged(const DenseCall &k, bool al, bool padded, const float *Wt, const float *bias2, int n_chunks)
{
    const int64_t blocks = (k.n_rows + 32 * RW - 1) / (32 * RW);
    if (padded) k.launch(layer_dense_kernel<RW, CW, NT, true, true>, blocks, 256, 0, Wt, bias2, n_chunks);
    else if (al) k.launch(layer_dense_kernel<RW, CW, NT, true, false>, blocks, 256, 0, Wt, bias2, n_chunks);
    else k.launch(layer_dense_kernel<RW, CW, NT, false, false>, blocks, 256, 0, Wt, bias2, n_chunks);
}

// Which forward kernel a call takes.  Every decision of the dispatch is made HERE, once: ngcf_layer_dense_f32 launches what this
// returns and ngcf_dense_path reports its name, so a test that names a kernel fails when the dispatch stops sending it there.
// Pure host code: the sizes, the alignment of the operands and the options (ngcf_opts()), nothing else.  d_out <= 512 (dop > 0).
enum DenseKernel { kDenseTall, kDenseSplit, kDenseResident, kDenseDirect, kDenseStaged };
struct DensePath {
    DenseKernel kernel;
    int dop;               // packed output columns: 32, 64, 96, 128, 256 or 512 (128 where small_rows)
    bool small_rows;       // up to 128 output columns on at most 16 384 rows: 32-row x 128-column tiles
    bool al;               // 16-byte aligned rows: ALIGNED of the staged kernel
    bool padded;           // and padded to a multiple of 4 floats: FAST of the staged kernel, and what every other kernel reads
    int tile;              // staged only: 0 = <1,4,1>, 1..4 = <4,1,1..4>, 5 = <2,2,4>, 6 = <1,4,4>
    const char *name;
};
static DensePath dense_path(int64_t n_rows, int d_in, int d_out, const float *LE, int64_t ldLE, const float *Es, int64_t ldEs)
{
    DensePath p{};
    p.dop = dense_dop(d_out);
    // Up to 128 output columns on a SMALL matrix (the Seoul graph: 5 940 rows): 128-row tiles are 47 workgroups on 256 CUs and the
    // 65 -> 65 layer of the reference's own configuration took 28-30 us; 32-row x 128-column tiles (four waves side by side, one
    // tile each) are 186 workgroups.  From 16 384 rows on (128 tiles of 128 rows) the tall tiles stay.
    p.small_rows = p.dop <= 128 && n_rows <= 16384 && ngcf_opts().dense_small_tiles;
    if (p.small_rows) p.dop = 128;
    const int dop = p.dop;
    p.al = (ldLE % 4 == 0) && (ldEs % 4 == 0) && aligned16(LE) && aligned16(Es);
    // 16-byte aligned rows padded to a multiple of 4 floats: what the tall, resident, split and direct kernels read
    p.padded = p.al && ldLE >= align_up(d_in, 4) && ldEs >= align_up(d_in, 4) && d_in >= 4;
    const int n_chunks = (d_in + NGCF_DC - 1) / NGCF_DC;

    // 256 / 512 output columns as 96-row x 128-column workgroups, three row tiles per wave, the row norm in a second kernel
    // (layer_dense_tall_kernel): 248 workgroups for the Seoul graph's 5 940 rows where the direct kernel has 186.  Measured
    // (tools/dense_wide_lab.py, profiles/r03_dense_wide_lab.txt; tall / direct / staged, us incl. pack and row scale):
    //   512 columns: 5 940 rows 84 / 92 / 109; 6 144: 84 / 93 / 109; 7 000: 127 / 89 / 107 (a second round of workgroups; the direct
    //   kernel still has one per CU up to 8 192 rows); 9 000: 132 / 267 / 165; 100 K: 956 / 1 384 / 1 078; 1.1 M: 10 129 / 12 114 / 10 858
    //   256 columns: 5 940 rows 47 / 47 / 58 (124 workgroups: no gain); 9 000: 48 / 78 / 59; 100 K: 290 / 418 / 310; 200 K: 569 / 735 / 552
    // dense_tall = 0: never; 2: wherever the shape allows; 1: by these numbers.
    const int tall_env = ngcf_opts().dense_tall;
    const bool tall_pays = dop == 512 ? (n_rows <= 6144 || n_rows > 8192) : (n_rows > 8192 && n_rows <= 131072);
    if (tall_env && dop >= 256 && p.padded && (tall_pays || tall_env == 2)) {
        p.kernel = kDenseTall;
        p.name = dop == 256 ? "tall256" : "tall512";
        return p;
    }

    // Weights resident in LDS, no barriers: large row counts at the 128-wide shapes, from two tiles per wave on.  dense_resident
    // = 4: the bf16 three-way split (layer_dense_split_kernel); 1 (any other non-zero value): the fp32 layer_dense_resident_kernel
    // (128 -> 128, resident / staged us: 65 536 rows 59 / 59, 98 304 rows 95 / 85, 131 072 rows 96 / 104, 262 144 rows 184 / 212,
    // C3's 1.1 M rows 633 / 780); 0: the staged kernel.
    const int resident = ngcf_opts().dense_resident;
    const int64_t lds_bytes = (int64_t)n_chunks * NGCF_KC * 128 * (int64_t)sizeof(float);
    const bool resident_fits = resident && dop == 128 && p.padded && lds_bytes <= 150 * 1024 &&
                               n_rows >= (int64_t)ngcf_opts().dense_resident_min_rows;
    if (resident_fits) {
        p.kernel = resident == 4 ? kDenseSplit : kDenseResident;
        p.name = resident == 4 ? "split" : "resident";
        return p;
    }

    // 256 / 512 output columns and at most ONE workgroup per CU (<= 8 192 rows - the Seoul graph has 5 940): operands straight
    // from global memory / L2, no staging (layer_dense_direct_kernel).  tools/dense_wide_lab.py: 94 vs 114 us at 5 940 x 515 -> 512,
    // 50 vs 57 us at 256 -> 256, 97 vs 117 us at 8 192 x 512 -> 512; as soon as a CU gets a second workgroup the staged kernel
    // (two workgroups share a CU's LDS and matrix pipe; the direct kernel runs one wave per SIMD) wins clearly: 170 vs 277 us at
    // 12 288 rows, 1.08 vs 1.40 ms at 100 K.  NGCF_DENSE_DIRECT=0 / 2: never / at any row count.
    const int direct_env = ngcf_opts().dense_direct;
    if (direct_env && dop >= 256 && p.padded && (n_rows <= 8192 || direct_env == 2)) {
        p.kernel = kDenseDirect;
        p.name = dop == 256 ? "direct<2,4>" : "direct<4,4>";
        return p;
    }

    // the staged kernel (layer_dense_kernel): the tile configuration by width, the row layout by alignment
#define NGCF_STAGED_NAMES(cfg) {"staged" cfg "/unaligned", "staged" cfg "/aligned", "staged" cfg "/padded"}
    static const char *const names[7][3] = {NGCF_STAGED_NAMES("<1,4,1>"), NGCF_STAGED_NAMES("<4,1,1>"), NGCF_STAGED_NAMES("<4,1,2>"),
                                            NGCF_STAGED_NAMES("<4,1,3>"), NGCF_STAGED_NAMES("<4,1,4>"), NGCF_STAGED_NAMES("<2,2,4>"),
                                            NGCF_STAGED_NAMES("<1,4,4>")};
#undef NGCF_STAGED_NAMES
    p.kernel = kDenseStaged;
    p.tile = p.small_rows ? 0 : dop <= 128 ? dop / 32 : dop == 256 ? 5 : 6;
    p.name = names[p.tile][p.padded ? 2 : p.al ? 1 : 0];
    return p;
}

extern "C" const char *ngcf_dense_path(int64_t n_rows, int d_in, int d_out, const float *LE, int64_t ldLE, const float *Es, int64_t ldEs)
{
    if (n_rows < 0 || d_in <= 0 || d_out <= 0 || dense_dop(d_out) < 0 || ldLE < d_in || ldEs < d_in) {
        fail(NGCF_ERR_ARG, "dense_path: bad sizes");
        return nullptr;
    }
    return dense_path(n_rows, d_in, d_out, LE, ldLE, Es, ldEs).name;
}

extern "C" int ngcf_layer_dense_f32(const float *LE, int64_t ldLE, const float *Es, int64_t ldEs, int64_t n_rows,
                                    int d_in, const float *W1, const float *b1, const float *W2, const float *b2,
                                    int d_out, float leaky, float drop_p, uint64_t drop_seed, const float *drop_mask,
                                    int64_t ld_mask, float *carry, int64_t ldc, float *norm, int64_t ldn, void *workspace,
                                    int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!LE || !Es || !W1 || !b1 || !W2 || !b2 || !norm) return fail(NGCF_ERR_ARG, "layer_dense: null argument");
    if (n_rows < 0 || d_in <= 0 || d_out <= 0) return fail(NGCF_ERR_ARG, "layer_dense: bad sizes");
    if (dense_dop(d_out) < 0) return fail(NGCF_ERR_ARG, "layer_dense: d_out=%d > 512 is not supported", d_out);
    if (!(drop_p >= 0.f && drop_p < 1.f)) return fail(NGCF_ERR_ARG, "layer_dense: drop_p=%f not in [0,1)", drop_p);
    if (ldLE < d_in || ldEs < d_in || ldn < d_out || (carry && ldc < d_out) || (drop_mask && ld_mask < d_out))
        return fail(NGCF_ERR_ARG, "layer_dense: leading dimension too small");
    const int64_t need = ngcf_dense_workspace_bytes(d_in, d_out);
    if (!workspace || workspace_bytes < need)
        return fail(NGCF_ERR_WORKSPACE, "layer_dense: workspace %lld B < %lld B", (long long)workspace_bytes, (long long)need);
    // Nothing to compute, and no kernel may run: the persistent kernels' row_of() would clamp to row -1 (dense_resident_min_rows
    // can be set to 0 or below).
    if (n_rows == 0) return NGCF_OK;
    const DensePath path = dense_path(n_rows, d_in, d_out, LE, ldLE, Es, ldEs);   // every decision: see there
    const int dop = path.dop;
    const int n_chunks = (d_in + NGCF_DC - 1) / NGCF_DC;
    float *Wt = reinterpret_cast<float *>(align_up((int64_t)(uintptr_t)workspace, 256));
    float *bias2 = Wt + (int64_t)n_chunks * NGCF_KC * dop;
    const DenseCall call{LE, ldLE, Es, ldEs, n_rows, d_in, d_out, leaky, drop_p, drop_seed, drop_mask, ld_mask, carry, ldc, norm, ldn, stream};

    if (path.kernel == kDenseTall) {
        const int n_ct = dop / 32;
        pack_weights_tall_kernel<<<dim3((unsigned)(n_chunks * n_ct)), 256, 0, stream>>>(W1, b1, W2, b2, d_in, d_out, dop, Wt, bias2);
        LAUNCH_CHECK();
        const int64_t groups = (n_rows + kTallRows - 1) / kTallRows;
        call.launch(layer_dense_tall_kernel, groups * (n_ct / 4), 256, 0, Wt, bias2, n_chunks, n_ct);
        LAUNCH_CHECK();
        if (dop == 256) row_scale_kernel<2><<<dim3((unsigned)((n_rows + 3) / 4)), 256, 0, stream>>>(norm, ldn, n_rows, d_out);
        else row_scale_kernel<4><<<dim3((unsigned)((n_rows + 3) / 4)), 256, 0, stream>>>(norm, ldn, n_rows, d_out);
        LAUNCH_CHECK();
        return NGCF_OK;
    }

    const int64_t lds_bytes = (int64_t)n_chunks * NGCF_KC * 128 * (int64_t)sizeof(float);
    auto pack_fp32 = [&](int nt) {  // the fp32 kernels' packed weights, nt tiles per wave (the split kernel packs its own)
        pack_weights_kernel<<<dim3((unsigned)(n_chunks * (dop / 32))), 256, 0, stream>>>(W1, b1, W2, b2, d_in, d_out, n_chunks, dop,
                                                                                        nt, Wt, bias2);
        return hipGetLastError();
    };
    if (path.kernel == kDenseSplit) {
        // bias at the start of the workspace, then parts h + m of every chunk (the LDS image), then part l
        HIP_TRY(allow_full_lds<layer_dense_split_kernel>());
        float *sbias = Wt;
        bf16x8 *whm = reinterpret_cast<bf16x8 *>(Wt + 128);
        bf16x8 *wl = whm + (int64_t)n_chunks * 1024;
        pack_weights_split_kernel<<<dim3((unsigned)(n_chunks * 2)), 256, 0, stream>>>(W1, b1, W2, b2, d_in, d_out, n_chunks,
                                                                                      whm, wl, sbias);
        LAUNCH_CHECK();
        call.launch(layer_dense_split_kernel, kResWGs, kResWaves * 64, (size_t)n_chunks * 16 * 1024, whm, wl, sbias, n_chunks);
        LAUNCH_CHECK();
        return NGCF_OK;
    }
    if (path.kernel == kDenseResident) {
        // four column tiles per lane, also where small_rows picked 32-row tiles for the staged kernel (a dense_resident_min_rows
        // at or below 16 384 rows)
        HIP_TRY(pack_fp32(4));
        HIP_TRY(allow_full_lds<layer_dense_resident_kernel>());
        call.launch(layer_dense_resident_kernel, kResWGs, kResWaves * 64, (size_t)lds_bytes, Wt, bias2, n_chunks);
        LAUNCH_CHECK();
        return NGCF_OK;
    }

    HIP_TRY(pack_fp32(path.small_rows ? 1 : dop <= 128 ? dop / 32 : 4));
    if (path.kernel == kDenseDirect) {
        const int64_t blocks = (n_rows + 31) / 32;
        if (dop == 256) call.launch(layer_dense_direct_kernel<2, 4>, blocks, 128, 0, Wt, bias2, n_chunks);
        else call.launch(layer_dense_direct_kernel<4, 4>, blocks, 256, 0, Wt, bias2, n_chunks);
        LAUNCH_CHECK();
        return NGCF_OK;
    }

    // the staged kernel (layer_dense_kernel)
#define NGCF_DENSE(RW, CW, NT) launch_staged<RW, CW, NT>(call, path.al, path.padded, Wt, bias2, n_chunks)
    switch (path.tile) {
    case 0: NGCF_DENSE(1, 4, 1); break;
    case 1: NGCF_DENSE(4, 1, 1); break;
    case 2: NGCF_DENSE(4, 1, 2); break;
    case 3: NGCF_DENSE(4, 1, 3); break;
    case 4: NGCF_DENSE(4, 1, 4); break;
    case 5: NGCF_DENSE(2, 2, 4); break;
    default: NGCF_DENSE(1, 4, 4);
    }
#undef NGCF_DENSE
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int64_t ngcf_layer_workspace_bytes(const ngcf_csr_t *c, int d_in, int d_out)
{
    if (!c) return -1;
    const int64_t a = ngcf_spmm_workspace_bytes(c, d_in);
    const int64_t b = ngcf_dense_workspace_bytes(d_in, d_out);
    if (a < 0 || b < 0) return -1;
    const int64_t le = align_up(c->n_rows * align_up(d_in, 32) * (int64_t)sizeof(float), 256);   // LE rows start on 128-byte lines
    return a + b + le + 256;
}

extern "C" int ngcf_layer_fused_f32(const ngcf_csr_t *c, const float *Eg, int64_t ldEg, const float *Es, int64_t ldEs,
                                    int d_in, const float *W1, const float *b1, const float *W2, const float *b2,
                                    int d_out, float leaky, float drop_p, uint64_t drop_seed, const float *drop_mask,
                                    int64_t ld_mask, float *carry, int64_t ldc, float *norm, int64_t ldn, void *workspace,
                                    int64_t workspace_bytes, void *stream)
{
    if (!c) return fail(NGCF_ERR_ARG, "layer_fused: null csr");
    const int64_t need = ngcf_layer_workspace_bytes(c, d_in, d_out);
    if (need < 0) return fail(NGCF_ERR_ARG, "layer_fused: unsupported widths d_in=%d d_out=%d", d_in, d_out);
    if (!workspace || workspace_bytes < need)
        return fail(NGCF_ERR_WORKSPACE, "layer_fused: workspace %lld B < %lld B", (long long)workspace_bytes, (long long)need);
    char *ws = reinterpret_cast<char *>(align_up((int64_t)(uintptr_t)workspace, 256));
    const int64_t ldLE = align_up(d_in, 32);
    float *LE = reinterpret_cast<float *>(ws);
    ws += align_up(c->n_rows * ldLE * (int64_t)sizeof(float), 256);
    const int64_t spmm_ws = ngcf_spmm_workspace_bytes(c, d_in);
    void *ws_spmm = ws;
    ws += spmm_ws;
    const int64_t dense_ws = ngcf_dense_workspace_bytes(d_in, d_out);
    void *ws_dense = ws;
    // Widths that are not a multiple of 4 (65, 130, 515: NGCF.py:39-43) on a SMALL matrix: the product is launch-bound, and the
    // main + tail panel split costs four extra launches (pack, tail product, fix-up, unpack: 23 of 141 us on the Seoul-shaped C1).
    // When the gathered rows are 16-byte aligned and padded, the columns up to the next multiple of 4 are simply multiplied along:
    // whatever they hold ends up in the padding columns of LE, which the dense half never reads (it selects zeros there).
    // (Reading them cannot fault: the 16-byte piece that holds the last column of a 16-byte aligned row is read whole.  The
    // mirror's engine.spmm asks the same function for the products of the training path, so both paths give the same bits.)
    const int d_sp = ngcf_spmm_product_width(c, Eg, ldEg, d_in);
    int rc = ngcf_spmm_csr_f32(c, Eg, ldEg, d_sp, LE, ldLE, ws_spmm, spmm_ws, stream);
    if (rc != NGCF_OK) return rc;
    return ngcf_layer_dense_f32(LE, ldLE, Es, ldEs, c->n_rows, d_in, W1, b1, W2, b2, d_out, leaky, drop_p, drop_seed,
                                drop_mask, ld_mask, carry, ldc, norm, ldn, ws_dense, dense_ws, stream);
}

