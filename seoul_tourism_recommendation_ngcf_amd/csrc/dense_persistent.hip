// dense_persistent.hip - the two persistent forward dense kernels with the weights resident in LDS (97-128 output columns, many
// rows): layer_dense_resident_kernel (fp32) and layer_dense_split_kernel (bf16, exact three-way split), one row-tile loop for both.
// The shared parts and the map of the dense files: dense_device.h; the dispatch: dense.hip.
#include "dense_device.h"
#include <type_traits>

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

int dense_launch_split(const DenseCall &call, const DenseWeights &w)
{
    // bias at the start of the workspace, then parts h + m of every chunk (the LDS image), then part l
    HIP_TRY(allow_full_lds<layer_dense_split_kernel>());
    float *sbias = w.Wt;
    bf16x8 *whm = reinterpret_cast<bf16x8 *>(w.Wt + 128);
    bf16x8 *wl = whm + (int64_t)w.n_chunks * 1024;
    pack_weights_split_kernel<<<dim3((unsigned)(w.n_chunks * 2)), 256, 0, call.stream>>>(w.W1, w.b1, w.W2, w.b2, call.d_in, call.d_out,
                                                                                       w.n_chunks, whm, wl, sbias);
    LAUNCH_CHECK();
    call.launch(layer_dense_split_kernel, kResWGs, kResWaves * 64, (size_t)w.n_chunks * 16 * 1024, whm, wl, sbias, w.n_chunks);
    LAUNCH_CHECK();
    return NGCF_OK;
}

int dense_launch_resident(const DenseCall &call, const DenseWeights &w)
{
    // four column tiles per lane, also where small_rows picked 32-row tiles for the staged kernel (a dense_resident_min_rows
    // at or below 16 384 rows)
    if (const int rc = dense_pack_fp32(call, w, 128, 4)) return rc;
    HIP_TRY(allow_full_lds<layer_dense_resident_kernel>());
    const int64_t lds_bytes = (int64_t)w.n_chunks * NGCF_KC * 128 * (int64_t)sizeof(float);
    call.launch(layer_dense_resident_kernel, kResWGs, kResWaves * 64, (size_t)lds_bytes, w.Wt, w.bias2(128), w.n_chunks);
    LAUNCH_CHECK();
    return NGCF_OK;
}
