// bwd_dense.hip - a layer's dense half in the backward pass: normalise / dropout / LeakyReLU backward, weight and bias gradients,
// input gradients (all on the fp32 matrix cores; see the banner of bwd_gather.hip).
#include "common.h"

// ---- normalise + dropout + LeakyReLU backward: (dN, dC, C) -> dM, one wave per row ------------
// forward: A = leaky(M); C = keep ? A/(1-p) : 0; N = C / max(|C|, eps)    (NGCF.py:140-144)
// VEC = 2 (r04): a lane owns the column pairs 2 lane, 2 lane + 128, .. (8-byte accesses: at d = 128 one load per operand and row
// instead of two; same arithmetic per element and the same order in the two row sums - lanes hold other columns, the wave sum is a
// sum over all of them either way - so only the association of those two sums differs from VEC = 1).
template <int VEC>
__global__ __launch_bounds__(256) void layer_bwd_pre_kernel(const float *__restrict__ dN, int64_t ldn,
                                                            const float *__restrict__ dC, int64_t ldc,
                                                            const float *__restrict__ C, int64_t ldC, int64_t n_rows,
                                                            int d, float leaky, float drop_p, uint64_t seed_in,
                                                            const float *__restrict__ drop_mask, int64_t ldk,
                                                            const int64_t *__restrict__ row_ids,
                                                            float *__restrict__ dM, int64_t ldm)
{
    const uint64_t seed = drop_p > 0.f ? resolve_seed(seed_in) : seed_in;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const int64_t r_hash = row_ids ? row_ids[r] : r;         // compacted rows: the hash stream is indexed by the row of the matrix
    const int lane = threadIdx.x & 63;
    const float *c = C + r * ldC, *g = dN ? dN + r * ldn : nullptr;   // dN == nullptr: no gradient through the normalised block
    float den = 1.f, ydot = 0.f;
    if (g) {
        float ss = 0.f, dot = 0.f;
        for (int j = lane * VEC; j < d; j += 64 * VEC) {
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                ss = fmaf(c[j + q], c[j + q], ss);
                dot = fmaf(c[j + q], g[j + q], dot);
            }
        }
        ss = wave_sum(ss);
        dot = wave_sum(dot);
        const float nrm = sqrtf(ss);
        const bool clamped = nrm < 1e-12f;                   // F.normalize's clamp_min: N = C / eps there
        den = clamped ? 1e-12f : nrm;
        ydot = clamped ? 0.f : dot / (den * den);            // (y.dy)/|x| with y = x/|x|
    }
    const float keep_scale = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
    const uint32_t thr = msg_drop_thr(drop_p);
    using V = typename VecT<VEC>::type;
    for (int j = lane * VEC; j < d; j += 64 * VEC) {
        float cv[VEC], gv[VEC], dc[VEC], mk[VEC], out[VEC];
        *reinterpret_cast<V *>(cv) = *reinterpret_cast<const V *>(c + j);
        if (g) *reinterpret_cast<V *>(gv) = *reinterpret_cast<const V *>(g + j);
        if (dC) *reinterpret_cast<V *>(dc) = *reinterpret_cast<const V *>(dC + r * ldc + j);
        if (drop_mask) *reinterpret_cast<V *>(mk) = *reinterpret_cast<const V *>(drop_mask + r * ldk + j);
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            float t = g ? gv[q] / den - cv[q] * (ydot / den) : 0.f;
            if (dC) t += dc[q];
            if (drop_mask) {
                t *= mk[q];                                   // the host-drawn noise tensor of the forward (0 or 1/(1-p))
            } else if (drop_p > 0.f) {
                t = msg_drop(t, seed, r_hash, j + q, thr, keep_scale);
            }
            out[q] = t * (cv[q] > 0.f ? 1.f : leaky);         // sign(C) == sign(M) wherever C was kept
        }
        *reinterpret_cast<V *>(dM + r * ldm + j) = *reinterpret_cast<const V *>(out);
    }
}

extern "C" int ngcf_layer_bwd_pre_f32(const float *dN, int64_t ldn, const float *dC, int64_t ldc, const float *C, int64_t ldC,
                                      int64_t n_rows, int d, float leaky, float drop_p, uint64_t seed, const float *drop_mask,
                                      int64_t ld_mask, const int64_t *row_ids, float *dM, int64_t ldm, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_rows == 0) return NGCF_OK;
    if ((!dN && !dC) || !C || !dM || d <= 0) return fail(NGCF_ERR_ARG, "layer_bwd_pre: bad argument");
    auto even = [](const float *p, int64_t ld) { return !p || (ld % 2 == 0 && ((uintptr_t)p & 7) == 0); };
    if (d % 2 == 0 && even(dN, ldn) && even(dC, ldc) && even(C, ldC) && even(drop_mask, ld_mask) && even(dM, ldm))
        layer_bwd_pre_kernel<2><<<dim3((unsigned)((n_rows + 3) / 4)), 256, 0, stream>>>(dN, ldn, dC, ldc, C, ldC, n_rows, d, leaky, drop_p,
                                                                                        seed, drop_mask, ld_mask, row_ids, dM, ldm);
    else
        layer_bwd_pre_kernel<1><<<dim3((unsigned)((n_rows + 3) / 4)), 256, 0, stream>>>(dN, ldn, dC, ldc, C, ldC, n_rows, d, leaky, drop_p,
                                                                                        seed, drop_mask, ld_mask, row_ids, dM, ldm);
    LAUNCH_CHECK();
    return NGCF_OK;
}


// out[r, :] += add[r, :]   (dE = dE_direct + L^T.dLE accumulation), VEC floats (of the row's dv = d / VEC pieces) to a thread.
// VEC = 4: 16-byte pieces (widths and leading dimensions that are multiples of 4, aligned rows: every padded matrix of the backward)
template <int VEC>
__global__ void add_rows_kernel(float *__restrict__ out, int64_t ldo, const float *__restrict__ add, int64_t lda, int64_t n_rows, int dv)
{
    using V = typename VecT<VEC>::type;
    const int64_t total = n_rows * dv;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / dv;
        const int j = (int)(i - r * dv) * VEC;
        V *o = reinterpret_cast<V *>(out + r * ldo + j);
        *o = vadd(*o, *reinterpret_cast<const V *>(add + r * lda + j));
    }
}

extern "C" int ngcf_add_rows_f32(float *out, int64_t ldo, const float *add, int64_t lda, int64_t n_rows, int d, void *stream_)
{
    if (n_rows == 0) return NGCF_OK;
    if (!out || !add || d <= 0 || n_rows < 0 || ldo < d || lda < d) return fail(NGCF_ERR_ARG, "add_rows: bad argument");
    if (d % 4 == 0 && ldo % 4 == 0 && lda % 4 == 0 && aligned16(out) && aligned16(add))
        add_rows_kernel<4><<<grid_for(n_rows * (d / 4), 256), 256, 0, (hipStream_t)stream_>>>(out, ldo, add, lda, n_rows, d / 4);
    else
        add_rows_kernel<1><<<grid_for(n_rows * d, 256), 256, 0, (hipStream_t)stream_>>>(out, ldo, add, lda, n_rows, d);
    LAUNCH_CHECK();
    return NGCF_OK;
}


// ---- weight gradients of a layer on the fp32 matrix cores --------------------------------------
//   gW[o][c]        = sum_rows dM[row][o] * (LE + E)[row][c]     (d loss / d W1, NGCF.py:131-133)
//   gW[o][d_in + c] = sum_rows dM[row][o] * (LE * E)[row][c]     (d loss / d W2, NGCF.py:135-136)
// A [d_out x 2 d_in] result with the 1.1 M rows as the reduction dimension: a library GEMM picks a 32x32 macro
// tile for this shape (2.3 ms at C3) and needs the [LE+E | LE*E] operand materialised (1.1 GB).  Here 256
// persistent workgroups stream blocks of 32 rows through LDS (the sum/product operand is formed on the way in),
// 8 waves each keep 4 of the 32 output tiles in registers (v_mfma_f32_32x32x2_f32: A = dM^T, B = [S|P], k = row),
// and write one partial result per workgroup; a second kernel adds the partials in workgroup order (fixed order,
// no atomics).  Widths up to 128 (padded to multiples of 32 inside LDS); wider layers use the library GEMM.
static constexpr int kBwRows = 32;        // rows per LDS block
static constexpr int kBwWGs = 256;
static constexpr int kBwM = 128, kBwN = 256;

template <bool ALIGNED>
__global__ __launch_bounds__(512) void bwd_weight_kernel(const float *__restrict__ dM, int64_t ldM,
                                                         const float *__restrict__ LE, int64_t ldLE,
                                                         const float *__restrict__ E, int64_t ldE, int64_t n_rows, int d_in,
                                                         int d_out, int P, float *__restrict__ partial,
                                                         float *__restrict__ partial_bias)
{
    __shared__ float As[2][kBwRows][kBwM];     // dM rows, columns >= d_out stay zero
    __shared__ float Bs[2][kBwRows][kBwN];     // [LE+E (P columns) | LE*E (P columns)], the rest stays zero
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
    for (int i = tid; i < 2 * kBwRows * kBwM; i += 512) (&As[0][0][0])[i] = 0.f;
    for (int i = tid; i < 2 * kBwRows * kBwN; i += 512) (&Bs[0][0][0])[i] = 0.f;
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float bsum = 0.f;
    // staging: 2 float4 slots per thread and operand: slot s -> row s / 32, columns 4 * (s % 32) ..
    f32x4 rm[2], rl[2], re[2];
    const int64_t n_blocks = (n_rows + kBwRows - 1) / kBwRows;
    auto load4 = [&](const float *base, int64_t ld, int64_t row, int c, int width) -> f32x4 {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < n_rows && c < width) {
            const float *p = base + row * ld + c;
            if (ALIGNED && c + 4 <= width) {
                v = *reinterpret_cast<const f32x4 *>(p);
            } else {
                v.x = p[0];
                if (c + 1 < width) v.y = p[1];
                if (c + 2 < width) v.z = p[2];
                if (c + 3 < width) v.w = p[3];
            }
        }
        return v;
    };
    auto load_block = [&](int64_t b) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const int s = tid + s2 * 512, r = s >> 5, c = (s & 31) * 4;
            const int64_t row = b * kBwRows + r;
            rm[s2] = load4(dM, ldM, row, c, d_out);
            rl[s2] = load4(LE, ldLE, row, c, d_in);
            re[s2] = load4(E, ldE, row, c, d_in);
        }
    };
    auto store_block = [&](int buf) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const int s = tid + s2 * 512, r = s >> 5, c = (s & 31) * 4;
            *reinterpret_cast<f32x4 *>(&As[buf][r][c]) = rm[s2];
            if (c < P) {
                *reinterpret_cast<f32x4 *>(&Bs[buf][r][c]) = rl[s2] + re[s2];
                *reinterpret_cast<f32x4 *>(&Bs[buf][r][P + c]) = rl[s2] * re[s2];
            }
        }
    };
    __syncthreads();                           // LDS zeroed
    int64_t b = blockIdx.x;
    if (b < n_blocks) {
        load_block(b);
        store_block(0);
    }
    __syncthreads();
    int buf = 0;
    for (; b < n_blocks; b += gridDim.x, buf ^= 1) {
        const bool more = b + gridDim.x < n_blocks;
        if (more) load_block(b + gridDim.x);   // the next block's global loads fly under the MFMAs
        // bias gradient = column sums of dM (NGCF.py:131-136: b1 enters twice, b2 once - the caller scales): thread (o, q)
        // adds rows 8 q .. 8 q + 7 of column o of the block that is in LDS anyway
#pragma unroll
        for (int r = 0; r < kBwRows / 4; ++r) bsum += As[buf][(tid >> 7) * (kBwRows / 4) + r][tid & (kBwM - 1)];
#pragma unroll
        for (int j = 0; j < kBwRows / 2; ++j) {
            const float bv = Bs[buf][2 * j + lh][wave * 32 + li];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(As[buf][2 * j + lh][t * 32 + li], bv, acc[t], 0, 0, 0);
        }
        if (more) store_block(buf ^ 1);
        __syncthreads();
    }
    // the partial leaves COMPACT: [d_out][2 d_in] contiguous per workgroup (r03: the padded [128][256] tile made the reduction
    // read a 4-byte word out of every 128 KB per workgroup and output element)
    float *out = partial + (int64_t)blockIdx.x * d_out * 2 * d_in;
    const int col = wave * 32 + li;                       // column of the [P | P] operand: sums in [0, P), products in [P, 2 P)
    const int cc = col < P ? col : d_in + (col - P);      // its place in [d_in | d_in]
    const bool col_ok = col < P ? col < d_in : (col - P) < d_in;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (col_ok && o < d_out) out[o * 2 * d_in + cc] = acc[t][r];
        }
    // the four row-quarters of a column, added in a fixed order (the last loop iteration ended with a barrier: As is free)
    float *bs = &As[0][0][0];
    bs[tid] = bsum;
    __syncthreads();
    if (tid < kBwM) partial_bias[(int64_t)blockIdx.x * kBwM + tid] = ((bs[tid] + bs[kBwM + tid]) + bs[2 * kBwM + tid]) + bs[3 * kBwM + tid];
}

// 64 output elements per workgroup; its four waves each add a quarter of the partials (eight independent load chains, combined in
// a fixed order), the quarters are added in wave order: the result does not depend on anything but n_wg.  (r03: one thread per
// element walking all partials - and one per bias element walking them as a single dependent chain - took 26 us of load latency
// on the Seoul graph's 93 partials.)
__global__ __launch_bounds__(256) void bwd_weight_reduce_kernel(const float *__restrict__ partial, const float *__restrict__ partial_bias,
                                                                int n_wg, int d_in, int d_out, float *__restrict__ gW1, int64_t ld1,
                                                                float *__restrict__ gW2, int64_t ld2, float *__restrict__ gb1,
                                                                float *__restrict__ gb2)
{
    __shared__ float quarter[4][64];
    const int e = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int n_w = d_out * 2 * d_in;
    const int i = blockIdx.x * 64 + e;
    const bool is_w = i < n_w, is_b = !is_w && (gb1 || gb2) && i - n_w < d_out;
    float r = 0.f;
    if (is_w || is_b) {
        const float *p = is_w ? partial + i : partial_bias + (i - n_w);
        const int64_t step = is_w ? (int64_t)n_w : (int64_t)kBwM;
        const int per = (n_wg + 3) / 4, w0 = q * per, w1 = min(n_wg, w0 + per);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f, s5 = 0.f, s6 = 0.f, s7 = 0.f;
        int w = w0;
        for (; w + 8 <= w1; w += 8) {
            s0 += p[(w + 0) * step];
            s1 += p[(w + 1) * step];
            s2 += p[(w + 2) * step];
            s3 += p[(w + 3) * step];
            s4 += p[(w + 4) * step];
            s5 += p[(w + 5) * step];
            s6 += p[(w + 6) * step];
            s7 += p[(w + 7) * step];
        }
        if (w + 0 < w1) s0 += p[(w + 0) * step];
        if (w + 1 < w1) s1 += p[(w + 1) * step];
        if (w + 2 < w1) s2 += p[(w + 2) * step];
        if (w + 3 < w1) s3 += p[(w + 3) * step];
        if (w + 4 < w1) s4 += p[(w + 4) * step];
        if (w + 5 < w1) s5 += p[(w + 5) * step];
        if (w + 6 < w1) s6 += p[(w + 6) * step];
        r = ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
    }
    quarter[q][e] = r;
    __syncthreads();
    if (q != 0) return;
    r = ((quarter[0][e] + quarter[1][e]) + quarter[2][e]) + quarter[3][e];
    if (is_w) {
        const int o = i / (2 * d_in), c = i % (2 * d_in);
        if (c < d_in) gW1[(int64_t)o * ld1 + c] = r;
        else gW2[(int64_t)o * ld2 + (c - d_in)] = r;
    } else if (is_b) {
        const int o = i - n_w;
        if (gb2) gb2[o] = r;
        if (gb1) gb1[o] = 2.0f * r;          // b1 enters the layer twice (NGCF.py:131,133)
    }
}

// A NARROW block of input columns (d_in <= 4: the 1..3 columns the reference's widths leave beyond a multiple of 128 - 130 -> 2,
// 515 -> 3; autograd._bwd_weight cuts the layer into blocks of 128 input columns).  The matrix-core kernel above multiplies the
// zero padding of such a block along at the full block's price (0.78 ms for the two last columns of C3's 130-wide first layer);
// this is a pass over dM with the 2 x d_in operand values of a row as scalars: thread o of a 128-thread group adds
// dM[row][o] * (LE + E)[row][c] and dM[row][o] * (LE * E)[row][c] over its workgroup's rows (coalesced rows of dM, a fixed order),
// two row groups per workgroup combined through LDS; the same compact per-workgroup partials, so the same reduction follows.
__global__ __launch_bounds__(256) void bwd_weight_narrow_kernel(const float *__restrict__ dM, int64_t ldM, const float *__restrict__ LE,
                                                                int64_t ldLE, const float *__restrict__ E, int64_t ldE, int64_t n_rows,
                                                                int d_in, int d_out, float *__restrict__ partial,
                                                                float *__restrict__ partial_bias)
{
    __shared__ float comb[9][kBwM];
    const int o = threadIdx.x & (kBwM - 1), half = threadIdx.x >> 7;
    float s[4] = {0.f, 0.f, 0.f, 0.f}, p[4] = {0.f, 0.f, 0.f, 0.f}, b = 0.f;
    const int64_t per = (n_rows + gridDim.x - 1) / gridDim.x;
    const int64_t r0 = (int64_t)blockIdx.x * per, r1 = r0 + per < n_rows ? r0 + per : n_rows;
    // eight rows per step and row group: eight independent loads of dM in flight per thread (rows past the end contribute zeros)
    for (int64_t row = r0 + 8 * half; row < r1; row += 16) {
        float m[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) m[q] = (o < d_out && row + q < r1) ? dM[(row + q) * ldM + o] : 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int64_t rq = row + q < r1 ? row + q : r1 - 1;                 // (clamped: m[q] is zero there)
            b += m[q];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < d_in) {
                    const float le = LE[rq * ldLE + c], e = E[rq * ldE + c];    // the same address in every lane: one broadcast load
                    s[c] = fmaf(m[q], le + e, s[c]);
                    p[c] = fmaf(m[q], le * e, p[c]);
                }
        }
    }
    if (half == 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) comb[c][o] = s[c], comb[4 + c][o] = p[c];
        comb[8][o] = b;
    }
    __syncthreads();
    if (half == 1 || o >= d_out) return;
    float *out = partial + (int64_t)blockIdx.x * d_out * 2 * d_in;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < d_in) {
            out[o * 2 * d_in + c] = s[c] + comb[c][o];
            out[o * 2 * d_in + d_in + c] = p[c] + comb[4 + c][o];
        }
    partial_bias[(int64_t)blockIdx.x * kBwM + o] = b + comb[8][o];
}

extern "C" int64_t ngcf_bwd_weight_workspace_bytes(void)
{
    return (int64_t)kBwWGs * kBwM * kBwN * sizeof(float) + (int64_t)kBwWGs * kBwM * sizeof(float) + 256;
}

// Which kernel a weight-gradient call takes and how many workgroups - partials for the reduction - it launches.  The decision is
// made HERE, once: ngcf_layer_bwd_weight_f32 launches what this returns and ngcf_layer_bwd_weight_path reports its name.  Pure host
// code: the sizes and the alignment of the operands, nothing else (no option enters).
enum BwdWeightKernel { kBwMfmaAligned, kBwMfmaUnaligned, kBwNarrow };
struct BwdWeightPath {
    BwdWeightKernel kernel;
    int n_wg;              // workgroups of the kernel = partials the reduction adds up
    const char *name;
};
static BwdWeightPath bwd_weight_path(int64_t n_rows, int d_in, const float *dM, int64_t ldM, const float *LE, int64_t ldLE,
                                     const float *E, int64_t ldE)
{
    if (d_in <= 4 && n_rows >= 65536)         // a narrow remainder block of a large matrix: no matrix cores for 2 x d_in columns
        return {kBwNarrow, kBwWGs * 8, "narrow"};                            // memory-bound: eight workgroups per CU
    // workgroups: one per CU on a large matrix; on a small one (the Seoul graph's 5 940 rows are 186 blocks, a compacted last
    // layer a few dozen) every workgroup should still see >= 2 blocks - each writes a 128 KB partial that the reduction reads
    // back (256 of them: 33 MB and 116 us for a 65 x 130 gradient)
    const int64_t n_blocks = (n_rows + kBwRows - 1) / kBwRows;
    const int n_wg = (int)std::min<int64_t>(kBwWGs, std::max<int64_t>(1, (n_blocks + 1) / 2));
    const bool al = ldM % 4 == 0 && ldLE % 4 == 0 && ldE % 4 == 0 && aligned16(dM) && aligned16(LE) && aligned16(E);
    return al ? BwdWeightPath{kBwMfmaAligned, n_wg, "mfma_aligned"} : BwdWeightPath{kBwMfmaUnaligned, n_wg, "mfma_unaligned"};
}

extern "C" const char *ngcf_layer_bwd_weight_path(int64_t n_rows, int d_in, int d_out, const float *dM, int64_t ldM, const float *LE,
                                                  int64_t ldLE, const float *E, int64_t ldE, int *n_workgroups)
{
    if (n_rows < 0 || d_in < 1 || d_out < 1 || d_in > 128 || d_out > 128 || ldM < d_out || ldLE < d_in || ldE < d_in) {
        fail(NGCF_ERR_ARG, "layer_bwd_weight_path: bad sizes");
        return nullptr;
    }
    const BwdWeightPath path = bwd_weight_path(n_rows, d_in, dM, ldM, LE, ldLE, E, ldE);
    if (n_workgroups) *n_workgroups = path.n_wg;
    return path.name;
}

extern "C" int ngcf_layer_bwd_weight_f32(const float *dM, int64_t ldM, const float *LE, int64_t ldLE, const float *E,
                                         int64_t ldE, int64_t n_rows, int d_in, int d_out, float *gW1, int64_t ld1, float *gW2,
                                         int64_t ld2, float *gb1, float *gb2, void *workspace, int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!gW1 || !gW2 || ld1 < d_in || ld2 < d_in || (n_rows > 0 && (!dM || !LE || !E)))
        return fail(NGCF_ERR_ARG, "layer_bwd_weight: null argument or leading dimension too small");
    if (n_rows < 0 || d_in < 1 || d_out < 1 || d_in > 128 || d_out > 128)
        return fail(NGCF_ERR_ARG, "layer_bwd_weight: widths d_in=%d d_out=%d not in 1..128", d_in, d_out);
    if (ldM < d_out || ldLE < d_in || ldE < d_in) return fail(NGCF_ERR_ARG, "layer_bwd_weight: leading dimension too small");
    if (!workspace || workspace_bytes < ngcf_bwd_weight_workspace_bytes())
        return fail(NGCF_ERR_WORKSPACE, "layer_bwd_weight: workspace %lld B < %lld B", (long long)workspace_bytes,
                    (long long)ngcf_bwd_weight_workspace_bytes());
    float *partial = reinterpret_cast<float *>(align_up((int64_t)(uintptr_t)workspace, 256));
    float *partial_bias = partial + (int64_t)kBwWGs * kBwM * kBwN;
    const int P = (int)align_up(d_in, 32);
    const BwdWeightPath path = bwd_weight_path(n_rows, d_in, dM, ldM, LE, ldLE, E, ldE);   // every decision: see there
    const int n_wg = path.n_wg;
    if (path.kernel == kBwNarrow) {
        partial_bias = partial + (int64_t)n_wg * d_out * 2 * d_in;           // (behind the weight partials: 2048 x 128 floats fit easily)
        bwd_weight_narrow_kernel<<<n_wg, 256, 0, stream>>>(dM, ldM, LE, ldLE, E, ldE, n_rows, d_in, d_out, partial, partial_bias);
    } else if (path.kernel == kBwMfmaAligned) {
        bwd_weight_kernel<true><<<n_wg, 512, 0, stream>>>(dM, ldM, LE, ldLE, E, ldE, n_rows, d_in, d_out, P, partial, partial_bias);
    } else {
        bwd_weight_kernel<false><<<n_wg, 512, 0, stream>>>(dM, ldM, LE, ldLE, E, ldE, n_rows, d_in, d_out, P, partial, partial_bias);
    }
    LAUNCH_CHECK();
    const int total = d_out * 2 * d_in + ((gb1 || gb2) ? d_out : 0);
    bwd_weight_reduce_kernel<<<(total + 63) / 64, 256, 0, stream>>>(partial, partial_bias, n_wg, d_in, d_out, gW1, ld1, gW2, ld2, gb1, gb2);
    LAUNCH_CHECK();
    return NGCF_OK;
}


// =============================================================================================
// Input gradients of a layer's dense half in one kernel (r02; replaces a library GEMM + the combine kernel and the
// [N, 2 d_in] intermediate between them):
//   dS = dM . W1,  dP = dM . W2                     ([n_rows, d_in] each; W1, W2 are nn.Linear weights [d_out, d_in])
//   dLE = dS + dP * E,   dE = dS + dP * LE          (NGCF.py:131-136 differentiated)
// Same structure as layer_dense_kernel (dense_staged.hip): a workgroup of 4 waves owns 128 rows, each wave a 32 x 128 output
// panel as four 32x32 tiles of v_mfma_f32_32x32x2_f32; K = d_out is walked in chunks of 32 through double-buffered LDS
// (A: rows of dM, B: the weight rows W[k, col0 .. col0+128), which need no transpose).  The K loop runs twice over the same
// rows of dM (second read from L2), once per weight matrix, so that both 64-register accumulators are live only in the
// epilogue, where a lane holds dS and dP of the same (row, column) and forms both outputs.
// =============================================================================================
static constexpr int kBiKC = 32, kBiRows = 128, kBiMaxCols = 160;

// One element of the epilogue, guarded: dLE = dS + dP * E, dE = dS + dP * LE at (row, col) inside the matrix.  (The full tiles of the
// weights-resident kernel run the same two fmaf without the tests, pipelined: see there.)
__device__ __forceinline__ void bwd_input_store(int64_t row, int col, float ds, float dp, int64_t n_rows, int d_in, const float *__restrict__ LE,
                                                int64_t ldLE, const float *__restrict__ E, int64_t ldE, float *__restrict__ dLE, int64_t ldd,
                                                float *__restrict__ dE, int64_t lde)
{
    if (row >= n_rows || col >= d_in) return;
    dLE[row * ldd + col] = fmaf(dp, E[row * ldE + col], ds);
    dE[row * lde + col] = fmaf(dp, LE[row * ldLE + col], ds);
}

// Wp[half][chunk][k][c] = W_half[chunk * 32 + k][col0 + c], c < wcols   (zero outside the matrix)
__global__ void bwd_input_pack_kernel(const float *__restrict__ W1, const float *__restrict__ W2, int d_out, int d_in, int col0,
                                      int wcols, int n_chunks, float *__restrict__ Wp)
{
    const int per_half = n_chunks * kBiKC * wcols;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * per_half; i += gridDim.x * blockDim.x) {
        const int half = i / per_half, x = i % per_half;
        const int c = x % wcols, k = x / wcols;
        const int col = col0 + c;
        Wp[i] = (k < d_out && col < d_in) ? (half ? W2 : W1)[(int64_t)k * d_in + col] : 0.f;
    }
}

// NT 32x32 tiles per wave: a panel of 32*NT input columns (NT = 4: 128; NT = 5: 160, which takes the reference's 130-wide
// first layer in one panel instead of two)
// SMALL (r03): a workgroup owns 32 rows and its four waves split the panel's columns (one 32x32 tile each at NT = 4) instead of
// 128 rows with a wave per 32 of them: on a matrix of a few thousand rows (the Seoul graph's 5 940: 47 workgroups of the tall shape
// on 256 CUs, 34 us) the panel is spread over 186 workgroups.
template <int NT, bool SMALL>
__global__ __launch_bounds__(256, 2) void layer_bwd_input_kernel(const float *__restrict__ dM, int64_t ldM, int64_t n_rows, int d_out,
                                                              const float *__restrict__ Wp, int n_chunks,
                                                              const float *__restrict__ LE, int64_t ldLE,
                                                              const float *__restrict__ E, int64_t ldE, int d_in, int col0,
                                                              float *__restrict__ dLE, int64_t ldd, float *__restrict__ dE, int64_t lde)
{
    constexpr int BM = SMALL ? 32 : kBiRows, WCOLS = 32 * NT, XLD = kBiKC + 4;
    constexpr int NTW = SMALL ? NT / 4 : NT;          // tiles per wave
    constexpr int XJ = BM * 8 / 256;                  // float4 of a dM chunk per thread
    static_assert(!SMALL || NT % 4 == 0, "the small shape splits the panel's tiles over four waves");
    __shared__ float Xs[2 * BM * XLD];
    __shared__ float Ws[2 * kBiKC * WCOLS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, lh = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * BM;
    const int d4 = (d_out + 3) & ~3;
    f32x16 acc[2][NTW];
    f32x4 xreg[XJ], wreg[NT];
    const int tile0 = SMALL ? wave * NTW : 0;         // first tile (32 columns) of this wave
    const int wrow = SMALL ? 0 : wave * 32;           // first row of this wave inside the workgroup's rows

    auto load_chunk = [&](int half, int chunk) {      // global -> registers (rows past the end re-read the last row, never stored)
#pragma unroll
        for (int j = 0; j < XJ; ++j) {
            const int f = tid + 256 * j;
            int64_t grow = row0 + f / 8;
            grow = grow < n_rows ? grow : n_rows - 1;
            const int c0 = chunk * kBiKC + (f % 8) * 4;
            const int cc = c0 < d4 ? c0 : d4 - 4;
            f32x4 a = *reinterpret_cast<const f32x4 *>(dM + grow * ldM + cc);
            a.x = c0 < d_out ? a.x : 0.f;
            a.y = c0 + 1 < d_out ? a.y : 0.f;
            a.z = c0 + 2 < d_out ? a.z : 0.f;
            a.w = c0 + 3 < d_out ? a.w : 0.f;
            xreg[j] = a;
        }
        const f32x4 *src = reinterpret_cast<const f32x4 *>(Wp + ((int64_t)half * n_chunks + chunk) * kBiKC * WCOLS);
#pragma unroll
        for (int j = 0; j < NT; ++j) wreg[j] = src[tid + 256 * j];       // 32 x WCOLS floats = NT float4 per thread
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int j = 0; j < XJ; ++j) {
            const int f = tid + 256 * j;
            *reinterpret_cast<f32x4 *>(Xs + buf * (BM * XLD) + (f / 8) * XLD + (f % 8) * 4) = xreg[j];
        }
        f32x4 *dst = reinterpret_cast<f32x4 *>(Ws + buf * (kBiKC * WCOLS));
#pragma unroll
        for (int j = 0; j < NT; ++j) dst[tid + 256 * j] = wreg[j];
    };
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int t = 0; t < NTW; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[half][t][r] = 0.f;
        load_chunk(half, 0);
        store_chunk(0);                                // (the previous half's loop ended with a barrier)
        __syncthreads();
        for (int chunk = 0; chunk < n_chunks; ++chunk) {
            const bool more = chunk + 1 < n_chunks;
            if (more) load_chunk(half, chunk + 1);      // global loads fly under the MFMAs
            const int buf = chunk & 1;
            const float *X = Xs + buf * (BM * XLD) + (wrow + li) * XLD + lh * 4;
            const float *W = Ws + buf * (kBiKC * WCOLS) + tile0 * 32 + li;
#pragma unroll
            for (int kb = 0; kb < kBiKC / 8; ++kb) {
                const f32x4 a4 = *reinterpret_cast<const f32x4 *>(X + kb * 8);
                const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                for (int sx = 0; sx < 4; ++sx) {
                    const float *wk = W + (kb * 8 + lh * 4 + sx) * WCOLS;
                    float bv[NTW];
#pragma unroll
                    for (int t = 0; t < NTW; ++t) bv[t] = wk[t * 32];
#pragma unroll
                    for (int t = 0; t < NTW; ++t) acc[half][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sx], bv[t], acc[half][t], 0, 0, 0);
                }
            }
            if (more) store_chunk((chunk + 1) & 1);
            __syncthreads();
        }
    }
    // epilogue: dLE = dS + dP * E, dE = dS + dP * LE
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t grow = row0 + wrow + (r & 3) + 8 * (r >> 2) + 4 * lh;
#pragma unroll
        for (int t = 0; t < NTW; ++t)
            bwd_input_store(grow, col0 + (tile0 + t) * 32 + li, acc[0][t][r], acc[1][t][r], n_rows, d_in, LE, ldLE, E, ldE, dLE, ldd, dE, lde);
    }
}


// ---- r04: the same product with the weights RESIDENT in LDS (the structure of layer_dense_resident_kernel, dense_persistent.hip) --------
// The staged kernel above runs at 37 % of the fp32 matrix peak at C3 (1.23 ms per 1.1 M-row layer): its two K loops over staged
// chunks (8 barriers per 128 rows, dM read twice, the W chunks re-staged by every workgroup) and its epilogue (2 loads + 2 stores per
// output element) run one after the other, so matrix time and memory time add up.  Here [W1 | W2] for one panel of 128 input
// columns - K x 256 floats, 128 KB at K = 128 - is loaded into LDS ONCE per persistent workgroup (8 waves, one workgroup per CU);
// a wave owns 32 rows outright: each lane reads the 16-byte pieces of ITS row of dM straight from global memory into the MFMA A
// layout, two chunks (of 16 k) ahead in two fixed register sets, and every k-pair feeds EIGHT accumulator tiles (dS and dP of the
// four 32-column tiles) - dM is read once, there is no barrier after the prologue, and the next tile's first chunks are requested
// before the epilogue of the current one.  The k order per output element is the staged kernel's (ascending k-pairs), so the
// results are bit-identical to it.
static constexpr int kBiResWaves = 8, kBiResWGs = 256, kBiResDC = 16;
static constexpr int kBiEpiDepth = 2;      // row groups of E / LE values in flight in the full-tile epilogue (4 and 6 measured no faster: profiles/r04_bwd_input_lab.txt)

// Wr[k][0..127] = W1[k][t * 32 + li] at [li * 4 + t], Wr[k][128..255] the same of W2 (zero outside the matrices): a lane's four
// tile values of one k are 16 contiguous bytes, a wave's reads of one k are 512 contiguous bytes (conflict-free ds_read_b128)
__global__ void bwd_input_pack_resident_kernel(const float *__restrict__ W1, const float *__restrict__ W2, int d_out, int d_in, int col0,
                                               int k_pad, float *__restrict__ Wr)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < k_pad * 256; i += gridDim.x * blockDim.x) {
        const int k = i >> 8, x = i & 255, half = x >> 7, y = x & 127;
        const int col = col0 + (y & 3) * 32 + (y >> 2);
        Wr[i] = (k < d_out && col < d_in) ? (half ? W2 : W1)[(int64_t)k * d_in + col] : 0.f;
    }
}

__global__ __launch_bounds__(kBiResWaves * 64) void layer_bwd_input_resident_kernel(
    const float *__restrict__ dM, int64_t ldM, int64_t n_rows, int d_out, const float *__restrict__ Wr, int n_chunks,
    const float *__restrict__ LE, int64_t ldLE, const float *__restrict__ E, int64_t ldE, int d_in, int col0, float *__restrict__ dLE,
    int64_t ldd, float *__restrict__ dE, int64_t lde)
{
    extern __shared__ float Wres[];                // [n_chunks * 16][256]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, lh = lane >> 5;
    {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(Wr);
        f32x4 *dst = reinterpret_cast<f32x4 *>(Wres);
        const int n4 = n_chunks * kBiResDC * 256 / 4;
        for (int i = tid; i < n4; i += kBiResWaves * 64) dst[i] = src[i];
    }
    __syncthreads();
    const int64_t n_tiles = (n_rows + 31) / 32;
    const int d4 = (d_out + 3) & ~3;
    const float *W = Wres + li * 4;
    const int last = n_chunks - 1;
    const int64_t tile_step = (int64_t)gridDim.x * kBiResWaves;
    auto row_of = [&](int64_t t) {                 // the lane's row of tile t (rows past the end re-read the last row, never stored)
        const int64_t g = t * 32 + li;
        return g < n_rows ? g : n_rows - 1;
    };
    // the lane's two 16-byte pieces of a chunk: dM at columns c*16 + lh*4 (a) and c*16 + 8 + lh*4 (b); columns past d_out are
    // re-read from the row's last float4 and zeroed at use
    auto fetch = [&](const float *row, int c, f32x4 &a, f32x4 &b) {
        const int ca = c * kBiResDC + lh * 4, cb = ca + 8;
        a = *reinterpret_cast<const f32x4 *>(row + (ca < d4 ? ca : d4 - 4));   // the clamp of fetch_pieces() (dense_device.h), for one operand
        b = *reinterpret_cast<const f32x4 *>(row + (cb < d4 ? cb : d4 - 4));
    };
    f32x4 a0, b0, a1, b1;                        // two chunks of look-ahead in two fixed register sets (every prefetch unconditional)
    int64_t tile = (int64_t)blockIdx.x * kBiResWaves + wave;
    {
        const float *r0 = dM + row_of(tile < n_tiles ? tile : 0) * ldM;
        fetch(r0, 0, a0, b0);
        fetch(r0, last < 1 ? last : 1, a1, b1);
    }
    for (; tile < n_tiles; tile += tile_step) {
        const int64_t row0 = tile * 32;
        const float *m_row = dM + row_of(tile) * ldM;
        f32x16 accS[4], accP[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) accS[t][r] = 0.f, accP[t][r] = 0.f;
        auto chunk_mfma = [&](int c, f32x4 a, f32x4 b) {
            const int ca = c * kBiResDC + lh * 4, cb = ca + 8;
            if (cb + 4 > d_out) {                   // only the last chunk of a width that is not a multiple of 16
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (ca + q >= d_out) a[q] = 0.f;
                    if (cb + q >= d_out) b[q] = 0.f;
                }
            }
            const float *wc = W + (int64_t)c * kBiResDC * 256;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const f32x4 av = kb ? b : a;
#pragma unroll
                for (int sx = 0; sx < 4; ++sx) {
                    const float *wk = wc + (kb * 8 + lh * 4 + sx) * 256;
                    const f32x4 v1 = *reinterpret_cast<const f32x4 *>(wk);
                    const f32x4 v2 = *reinterpret_cast<const f32x4 *>(wk + 128);
                    accS[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sx], v1.x, accS[0], 0, 0, 0);
                    accS[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sx], v1.y, accS[1], 0, 0, 0);
                    accS[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sx], v1.z, accS[2], 0, 0, 0);
                    accS[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sx], v1.w, accS[3], 0, 0, 0);
                    accP[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sx], v2.x, accP[0], 0, 0, 0);
                    accP[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sx], v2.y, accP[1], 0, 0, 0);
                    accP[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sx], v2.z, accP[2], 0, 0, 0);
                    accP[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sx], v2.w, accP[3], 0, 0, 0);
                }
            }
        };
        int c = 0;
        for (; c + 1 < n_chunks; c += 2) {
            {
                const f32x4 ua = a0, ub = b0;
                fetch(m_row, c + 2 < last ? c + 2 : last, a0, b0);          // in flight under two chunks of MFMAs
                __builtin_amdgcn_sched_barrier(0);
                chunk_mfma(c, ua, ub);
            }
            {
                const f32x4 ua = a1, ub = b1;
                fetch(m_row, c + 3 < last ? c + 3 : last, a1, b1);
                __builtin_amdgcn_sched_barrier(0);
                chunk_mfma(c + 1, ua, ub);
            }
        }
        if (c < n_chunks) chunk_mfma(c, a0, b0);
        {   // the next tile's first two chunks, ahead of this tile's epilogue (the last tile of a wave re-reads its own)
            const float *rn = dM + row_of(tile + tile_step < n_tiles ? tile + tile_step : tile) * ldM;
            fetch(rn, 0, a0, b0);
            fetch(rn, last < 1 ? last : 1, a1, b1);
            __builtin_amdgcn_sched_barrier(0);
        }
        // epilogue: dLE = dS + dP * E, dE = dS + dP * LE.  Full tiles take a path without per-element tests: behind a branch the
        // compiler cannot move a load ahead of the stores of the row before it, and an epilogue of 16 dependent load -> FMA -> store
        // rounds is 16 memory latencies per tile (the first version: 1.16 ms per layer, matrix pipe 43 % busy); here the E / LE values
        // of two row groups are in flight while the previous group is combined and stored.
        if (row0 + 32 <= n_rows && col0 + 128 <= d_in) {
            const int64_t rbase = row0 + 4 * lh;
            const float *pe = E + rbase * ldE + col0 + li, *pl = LE + rbase * ldLE + col0 + li;
            float *ple = dLE + rbase * ldd + col0 + li, *pde = dE + rbase * lde + col0 + li;
            constexpr int DEPTH = kBiEpiDepth;
            float ev[DEPTH][4], lv[DEPTH][4];
            auto ld_r = [&](int r, float (&e)[4], float (&l)[4]) {
                const int64_t ro = (r & 3) + 8 * (r >> 2);
#pragma unroll
                for (int t = 0; t < 4; ++t) e[t] = pe[ro * ldE + t * 32], l[t] = pl[ro * ldLE + t * 32];
            };
#pragma unroll
            for (int r = 0; r < DEPTH - 1; ++r) ld_r(r, ev[r], lv[r]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (r + DEPTH - 1 < 16) ld_r(r + DEPTH - 1, ev[(r + DEPTH - 1) % DEPTH], lv[(r + DEPTH - 1) % DEPTH]);
                const int64_t ro = (r & 3) + 8 * (r >> 2);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float ds = accS[t][r], dp = accP[t][r];
                    ple[ro * ldd + t * 32] = fmaf(dp, ev[r % DEPTH][t], ds);
                    pde[ro * lde + t * 32] = fmaf(dp, lv[r % DEPTH][t], ds);
                }
            }
            continue;
        }
        // (the edge tiles keep their own text: through bwd_input_store() this kernel - full-tile path included - compiles to other code,
        // 3 499 -> 3 450 instructions, and its text is pinned)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t grow = row0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (grow >= n_rows) continue;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int col = col0 + t * 32 + li;
                if (col < d_in) {
                    const float ds = accS[t][r], dp = accP[t][r];
                    dLE[grow * ldd + col] = fmaf(dp, E[grow * ldE + col], ds);
                    dE[grow * lde + col] = fmaf(dp, LE[grow * ldLE + col], ds);
                }
            }
        }
    }
}

// The 1..4 input columns a 130- / 515-wide first layer leaves beyond its panels of 128: per row the dot products of its dM row with
// columns c of W1 and W2 (K values each), one wave per four rows - lane l holds k = l and l + 64 of the weight columns in registers -
// and the same epilogue.  A pass over dM (0.56 GB at C3) instead of a 160-column panel of the staged kernel.
__global__ __launch_bounds__(256) void layer_bwd_input_narrow_kernel(const float *__restrict__ dM, int64_t ldM, int64_t n_rows, int d_out,
                                                                     const float *__restrict__ W1, const float *__restrict__ W2,
                                                                     const float *__restrict__ LE, int64_t ldLE, const float *__restrict__ E,
                                                                     int64_t ldE, int d_in, int col0, int ncols, float *__restrict__ dLE,
                                                                     int64_t ldd, float *__restrict__ dE, int64_t lde)
{
    const int lane = threadIdx.x & 63;
    float w1[2][4], w2[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = lane + 64 * h;
            const bool ok = k < d_out && c < ncols;
            w1[h][c] = ok ? W1[(int64_t)k * d_in + col0 + c] : 0.f;
            w2[h][c] = ok ? W2[(int64_t)k * d_in + col0 + c] : 0.f;
        }
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    // four rows per step: eight independent loads of dM in flight per lane (one row per step is one memory latency per row: 0.64 ms
    // at C3 for a pass that moves 0.56 GB)
    for (int64_t row4 = wave0 * 4; row4 < n_rows; row4 += n_waves * 4) {
        float m0[4], m1[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t row = row4 + q < n_rows ? row4 + q : n_rows - 1;
            m0[q] = lane < d_out ? dM[row * ldM + lane] : 0.f;
            m1[q] = lane + 64 < d_out ? dM[row * ldM + lane + 64] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t row = row4 + q;
            // v[0..3] = dS of columns 0..3, v[4..7] = dP: eight partial dot products per lane, reduced over the wave with a halving
            // butterfly - at every step a lane keeps half of its values and takes the partner's for those (10 exchanges, not 48)
            float v[8];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                v[c] = fmaf(m1[q], w1[1][c], m0[q] * w1[0][c]);
                v[4 + c] = fmaf(m1[q], w2[1][c], m0[q] * w2[0][c]);
            }
            float u[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {              // lanes with bit 5 clear keep v[0..3], the others v[4..7]
                const float mine = (lane & 32) ? v[4 + i] : v[i], theirs = (lane & 32) ? v[i] : v[4 + i];
                u[i] = mine + __shfl_xor(theirs, 32);
            }
            float t2[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {              // bit 4 clear: u[0..1], set: u[2..3]
                const float mine = (lane & 16) ? u[2 + i] : u[i], theirs = (lane & 16) ? u[i] : u[2 + i];
                t2[i] = mine + __shfl_xor(theirs, 16);
            }
            float x;
            {
                const float mine = (lane & 8) ? t2[1] : t2[0], theirs = (lane & 8) ? t2[0] : t2[1];
                x = mine + __shfl_xor(theirs, 8);
            }
            x += __shfl_xor(x, 4);
            x += __shfl_xor(x, 2);
            x += __shfl_xor(x, 1);
            // lane's value: index = (bit5 ? 4 : 0) + (bit4 ? 2 : 0) + (bit3 ? 1 : 0) of v; lanes 0, 8, 16, 24 hold dS of columns 0..3 and
            // lanes 32, 40, 48, 56 hold dP of the same columns: pair them up through one more exchange
            const float dp = __shfl(x, (lane & 31) + 32);
            const int c = ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1);
            if (lane < 32 && (lane & 7) == 0 && c < ncols) bwd_input_store(row, col0 + c, x, dp, n_rows, d_in, LE, ldLE, E, ldE, dLE, ldd, dE, lde);
        }
    }
}

extern "C" int64_t ngcf_layer_bwd_input_workspace_bytes(int d_out)
{
    if (d_out <= 0) return -1;
    const int64_t n_chunks = (d_out + kBiKC - 1) / kBiKC;
    return align_up(2 * n_chunks * kBiKC * kBiMaxCols * (int64_t)sizeof(float), 256) + 256;
}

// Which kernel the panel of input columns that starts at col0 takes, and the panel's width: the next panel starts at col0 + cols
// (the panel's columns past d_in do not exist and are never stored).  The decision is made HERE, once: ngcf_layer_bwd_input_f32
// walks the panels this returns and ngcf_layer_bwd_input_path reports their names.  Pure host code: the sizes and the option
// bwd_input_resident, nothing else.  col0 is a panel start: 0, or what the widths of the panels before it add up to.
enum BwdInputKernel { kBiStagedSmall, kBiStagedTall, kBiStagedWide, kBiResident, kBiNarrow };
struct BwdInputPanel {
    BwdInputKernel kernel;
    int cols;              // 128, 160 (staged_wide), or the 1..4 columns of the narrow kernel
    const char *name;
};
static bool bwd_input_rows_ok(int64_t n_rows) { return (n_rows + kBiRows - 1) / kBiRows < (int64_t)1 << 31; }
static BwdInputPanel bwd_input_panel(int64_t n_rows, int d_in, int d_out, int col0)
{
    const int left = d_in - col0;
    // r04: large matrices at K <= 128 - panels of 128 input columns on the weights-resident kernel, a remainder of 1..4 columns
    // (the reference's 130- / 515-wide first layers) on the narrow kernel
    const int k_chunks = (d_out + kBiResDC - 1) / kBiResDC;
    const bool resident = ngcf_opts().bwd_input_resident && d_out <= 128 && d_out >= 4 && n_rows >= 2 * 32 * kBiResWaves * kBiResWGs &&
                          ngcf_layer_bwd_input_workspace_bytes(d_out) >= (int64_t)k_chunks * kBiResDC * 256 * (int64_t)sizeof(float) + 256;
    if (resident) return left > 4 ? BwdInputPanel{kBiResident, 128, "resident"} : BwdInputPanel{kBiNarrow, left, "narrow"};
    // panels of 128 input columns, the last one up to 160
    if (left > 128 && left <= 160) return {kBiStagedWide, 160, "staged_wide"};
    // fewer than 128 tall tiles: 32-row tiles, the waves side by side (see the kernel)
    return n_rows <= 16384 ? BwdInputPanel{kBiStagedSmall, 128, "staged_small"} : BwdInputPanel{kBiStagedTall, 128, "staged_tall"};
}

extern "C" const char *ngcf_layer_bwd_input_path(int64_t n_rows, int d_in, int d_out, int col0, int *panel_cols)
{
    if (n_rows < 0 || d_in <= 0 || d_out < 1 || !bwd_input_rows_ok(n_rows)) {
        fail(NGCF_ERR_ARG, "layer_bwd_input_path: bad sizes");
        return nullptr;
    }
    int start = 0;                             // walk the panels as the entry point does
    while (start < col0 && start < d_in) start += bwd_input_panel(n_rows, d_in, d_out, start).cols;
    if (col0 < 0 || start != col0 || col0 >= d_in) {
        fail(NGCF_ERR_ARG, "layer_bwd_input_path: col0=%d is not the start of a panel of d_in=%d", col0, d_in);
        return nullptr;
    }
    const BwdInputPanel panel = bwd_input_panel(n_rows, d_in, d_out, col0);
    if (panel_cols) *panel_cols = panel.cols;
    return panel.name;
}

extern "C" int ngcf_layer_bwd_input_f32(const float *dM, int64_t ldM, int64_t n_rows, int d_out, const float *W1, const float *W2,
                                        int d_in, const float *LE, int64_t ldLE, const float *E, int64_t ldE, float *dLE,
                                        int64_t ldd, float *dE, int64_t lde, void *workspace, int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_rows == 0) return NGCF_OK;
    if (!dM || !W1 || !W2 || !LE || !E || !dLE || !dE || d_in <= 0 || d_out < 1 || ldM < d_out || ldLE < d_in || ldE < d_in ||
        ldd < d_in || lde < d_in)
        return fail(NGCF_ERR_ARG, "layer_bwd_input: bad argument");
    if (ldM % 4 != 0 || !aligned16(dM) || ldM < align_up(d_out, 4))
        return fail(NGCF_ERR_ARG, "layer_bwd_input: dM needs 16-byte aligned rows padded to a multiple of 4 floats");
    const int64_t need = ngcf_layer_bwd_input_workspace_bytes(d_out);
    if (!workspace || workspace_bytes < need)
        return fail(NGCF_ERR_WORKSPACE, "layer_bwd_input: workspace %lld B < %lld B", (long long)workspace_bytes, (long long)need);
    float *Wp = reinterpret_cast<float *>(align_up((int64_t)(uintptr_t)workspace, 256));
    const int n_chunks = (d_out + kBiKC - 1) / kBiKC;
    const int64_t blocks = (n_rows + kBiRows - 1) / kBiRows;
    if (!bwd_input_rows_ok(n_rows)) return fail(NGCF_ERR_ARG, "layer_bwd_input: too many rows");
    const int k_chunks = (d_out + kBiResDC - 1) / kBiResDC;
    // panel by panel, each on the kernel bwd_input_panel() names (stream-ordered re-use of Wp)
    for (int col0 = 0; col0 < d_in;) {
        const BwdInputPanel panel = bwd_input_panel(n_rows, d_in, d_out, col0);          // every decision: see there
        switch (panel.kernel) {
        case kBiResident:
            HIP_TRY(allow_full_lds<layer_bwd_input_resident_kernel>());
            bwd_input_pack_resident_kernel<<<64, 256, 0, stream>>>(W1, W2, d_out, d_in, col0, k_chunks * kBiResDC, Wp);
            LAUNCH_CHECK();
            layer_bwd_input_resident_kernel<<<dim3(kBiResWGs), kBiResWaves * 64, (size_t)k_chunks * kBiResDC * 256 * sizeof(float), stream>>>(
                dM, ldM, n_rows, d_out, Wp, k_chunks, LE, ldLE, E, ldE, d_in, col0, dLE, ldd, dE, lde);
            break;
        case kBiNarrow:
            layer_bwd_input_narrow_kernel<<<dim3(kBiResWGs * 8), 256, 0, stream>>>(dM, ldM, n_rows, d_out, W1, W2, LE, ldLE, E, ldE, d_in, col0,
                                                                                  panel.cols, dLE, ldd, dE, lde);
            break;
        case kBiStagedWide:
            bwd_input_pack_kernel<<<64, 256, 0, stream>>>(W1, W2, d_out, d_in, col0, panel.cols, n_chunks, Wp);
            LAUNCH_CHECK();
            layer_bwd_input_kernel<5, false><<<dim3((unsigned)blocks), 256, 0, stream>>>(dM, ldM, n_rows, d_out, Wp, n_chunks, LE, ldLE, E, ldE,
                                                                                         d_in, col0, dLE, ldd, dE, lde);
            break;
        case kBiStagedSmall:
            bwd_input_pack_kernel<<<64, 256, 0, stream>>>(W1, W2, d_out, d_in, col0, panel.cols, n_chunks, Wp);
            LAUNCH_CHECK();
            layer_bwd_input_kernel<4, true><<<dim3((unsigned)((n_rows + 31) / 32)), 256, 0, stream>>>(dM, ldM, n_rows, d_out, Wp, n_chunks, LE, ldLE,
                                                                                                    E, ldE, d_in, col0, dLE, ldd, dE, lde);
            break;
        case kBiStagedTall:
            bwd_input_pack_kernel<<<64, 256, 0, stream>>>(W1, W2, d_out, d_in, col0, panel.cols, n_chunks, Wp);
            LAUNCH_CHECK();
            layer_bwd_input_kernel<4, false><<<dim3((unsigned)blocks), 256, 0, stream>>>(dM, ldM, n_rows, d_out, Wp, n_chunks, LE, ldLE, E, ldE,
                                                                                         d_in, col0, dLE, ldd, dE, lde);
            break;
        }
        LAUNCH_CHECK();
        col0 += panel.cols;
    }
    return NGCF_OK;
}
