// dense_staged.hip - the staged forward dense kernel (layer_dense_kernel, any shape) and the fp32 weight pack that the resident
// and direct paths use too.  The shared parts and the map of the dense files: dense_device.h; the dispatch: dense.hip.
#include "dense_device.h"

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

// A workgroup of 4 waves owns BM = 32*RW full rows; waves are arranged RW x CW, each wave NT 32x32 tiles,
// so a whole output row (<= 32*NT*CW columns) lives in one workgroup and the L2 row-normalisation is
// done in registers + one LDS exchange.
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

// the fp32 kernels' packed weights, nt tiles per wave (the split and tall kernels pack their own)
int dense_pack_fp32(const DenseCall &k, const DenseWeights &w, int dop, int nt)
{
    pack_weights_kernel<<<dim3((unsigned)(w.n_chunks * (dop / 32))), 256, 0, k.stream>>>(w.W1, w.b1, w.W2, w.b2, k.d_in, k.d_out, w.n_chunks,
                                                                                        dop, nt, w.Wt, w.bias2(dop));
    LAUNCH_CHECK();
    return NGCF_OK;
}

template <int RW, int CW, int NT>   // the staged kernel; padded: 16-byte aligned rows padded to a multiple of 4 floats (any d_in)
static void launch_staged(const DenseCall &k, bool al, bool padded, const float *Wt, const float *bias2, int n_chunks)
{
    const int64_t blocks = (k.n_rows + 32 * RW - 1) / (32 * RW);
    if (padded) k.launch(layer_dense_kernel<RW, CW, NT, true, true>, blocks, 256, 0, Wt, bias2, n_chunks);
    else if (al) k.launch(layer_dense_kernel<RW, CW, NT, true, false>, blocks, 256, 0, Wt, bias2, n_chunks);
    else k.launch(layer_dense_kernel<RW, CW, NT, false, false>, blocks, 256, 0, Wt, bias2, n_chunks);
}

int dense_launch_staged(const DenseCall &call, const DenseWeights &w, const DensePath &path)
{
    const int dop = path.dop;
    if (const int rc = dense_pack_fp32(call, w, dop, path.small_rows ? 1 : dop <= 128 ? dop / 32 : 4)) return rc;
#define NGCF_DENSE(RW, CW, NT) launch_staged<RW, CW, NT>(call, path.al, path.padded, w.Wt, w.bias2(dop), w.n_chunks)
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
