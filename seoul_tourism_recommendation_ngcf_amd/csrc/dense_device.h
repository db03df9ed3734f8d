// dense_device.h - what the forward dense kernels share (internal).  The dense half of a layer is five files:
//   dense.hip             host only: the dispatch (dense_path), the argument checks of ngcf_layer_dense_f32, the fused layer entry point
//   dense_staged.hip      layer_dense_kernel: rows of LE / E and a chunk of weights through LDS, one barrier per chunk (any shape);
//                         pack_weights_kernel, the fp32 pack that the resident and direct paths use too
//   dense_persistent.hip  layer_dense_resident_kernel: persistent, fp32 weights resident in LDS (97-128 columns, many rows);
//                         layer_dense_split_kernel: the same persistent loop on the bf16 matrix cores, exact three-way split (the default there)
//   dense_wide.hip        layer_dense_direct_kernel: 256 / 512 columns, at most one workgroup per CU, no operand in LDS;
//                         layer_dense_tall_kernel: 256 / 512 columns, 96-row workgroups; row_scale_kernel normalises afterwards
// All five kernels compute the same layer; dense_path (dense.hip) picks one by shape.  What they share is defined once, here:
//   tile_row()                     accumulator register -> row of the 32 x 32 tile (all five)
//   DenseAct                       LeakyReLU and the two dropout forms of one output element (resident, direct)
//   dense_epilogue<CW, NT, EVAL>   bias, DenseAct, row sums of squares, butterfly, cross-wave exchange, stores (resident, direct; the
//                                  staged and split kernels keep copies of it for their measured speed - see there)
//   fetch_pieces() / zero_tail()   a lane's clamped 16-byte reads of its row; columns past d_in zeroed at use (resident,
//                                  split, direct)
//   pack_bias2()                   2*b1 + b2 (the three pack kernels)
//   DenseCall / DensePath          a call's arguments and what the dispatch decided, handed to the launch function of each path
// and, in dense_persistent.hip, dense_persistent_tiles<SPLIT>: the persistent row-tile loop and its look-ahead (resident, split: only
// the operands differ).
// The fp32 kernels add the k-values of an output element in one order; the epilogue copies and row_scale_kernel (behind tall)
// repeat the summation order of dense_epilogue by hand: bit-identical results (tests/test_parity_gpu.py).
#ifndef NGCF_DENSE_DEVICE_H
#define NGCF_DENSE_DEVICE_H

#include "common.h"

// ---------------------------------------------------------------------------------------------
// Dense half of a layer (NGCF.py:131-146) on the fp32 matrix cores.
//
//   M = [LE+E | LE*E] . [W1^T ; W2^T] + (2*b1 + b2)
// The K dimension is walked in chunks of DC = 16 input columns: a chunk contributes 16 "sum" values
// and 16 "product" values per row (KC = 32 k-steps), so LE and E are read exactly once.  Weights are
// packed per call into that chunk order ([n_chunks*32][DOP], zero padded) by pack_weights_kernel.
// v_mfma_f32_32x32x2_f32: exact fp32 FMA chain per output element.
// ---------------------------------------------------------------------------------------------
#ifndef NGCF_DC
#define NGCF_DC 16
#endif
#define NGCF_KC (2 * NGCF_DC)

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
// (Written through a one-operand form, the resident, split and direct kernels compiled to different code, so
// layer_bwd_input_resident_kernel in bwd_dense.hip keeps its own copy of the clamp for dM: profiles/dense_files_split.txt.)
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

// Which forward kernel a call takes: what dense_path (dense.hip) returns.
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

// A call's weights, and the start of its workspace (256-byte aligned), where each path packs them its own way.
struct DenseWeights {
    const float *W1, *b1, *W2, *b2;
    float *Wt;
    int n_chunks;          // chunks of NGCF_DC input columns
    float *bias2(int dop) const { return Wt + (int64_t)n_chunks * NGCF_KC * dop; }   // behind the fp32 packs' [n_chunks * KC][dop]
};

// One launch function per DenseKernel value, each next to its kernels: the path's packs and launches in stream order; they
// return the library's codes.
int dense_pack_fp32(const DenseCall &k, const DenseWeights &w, int dop, int nt);                // dense_staged.hip: nt tiles per wave
int dense_launch_staged(const DenseCall &k, const DenseWeights &w, const DensePath &path);      // dense_staged.hip
int dense_launch_resident(const DenseCall &k, const DenseWeights &w);                           // dense_persistent.hip
int dense_launch_split(const DenseCall &k, const DenseWeights &w);                              // dense_persistent.hip
int dense_launch_direct(const DenseCall &k, const DenseWeights &w, int dop);                    // dense_wide.hip
int dense_launch_tall(const DenseCall &k, const DenseWeights &w, int dop);                      // dense_wide.hip

#endif  // NGCF_DENSE_DEVICE_H
