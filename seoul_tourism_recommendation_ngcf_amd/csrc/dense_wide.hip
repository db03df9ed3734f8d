// dense_wide.hip - the two forward dense kernels for 256 / 512 output columns: layer_dense_direct_kernel (at most one workgroup
// per CU, no operand in LDS) and layer_dense_tall_kernel (96-row workgroups, with its own pack and row_scale_kernel behind it).
// The shared parts and the map of the dense files: dense_device.h; the dispatch: dense.hip.
#include "dense_device.h"

// ---------------------------------------------------------------------------------------------
// 256 / 512 output columns with NO operand in LDS (r02).  At these widths a workgroup of layer_dense_kernel owns 32 (or 64) rows
// and each of its waves its own 128 output columns: the weights a wave multiplies by are shared with nobody, yet a 32 / 64 KB
// chunk of them goes through the one LDS buffer per chunk between two barriers, and with a few thousand rows (the Seoul graph:
// 186 workgroups, one wave per SIMD) nothing hides that.  Here a wave reads its B operands - the lane's four tile values of a
// k-pair are 16 contiguous bytes of the packed row - straight from the L2-resident packed matrix into registers, one chunk ahead
// in two fixed register sets, and its A operands like layer_dense_resident_kernel; the only LDS traffic is the exchange of the
// row sums of squares at the end.  Same k order per output element as the other two kernels: bit-identical results.
// ---------------------------------------------------------------------------------------------
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

int dense_launch_direct(const DenseCall &call, const DenseWeights &w, int dop)
{
    if (const int rc = dense_pack_fp32(call, w, dop, 4)) return rc;
    const int64_t blocks = (call.n_rows + 31) / 32;
    if (dop == 256) call.launch(layer_dense_direct_kernel<2, 4>, blocks, 128, 0, w.Wt, w.bias2(dop), w.n_chunks);
    else call.launch(layer_dense_direct_kernel<4, 4>, blocks, 256, 0, w.Wt, w.bias2(dop), w.n_chunks);
    LAUNCH_CHECK();
    return NGCF_OK;
}

int dense_launch_tall(const DenseCall &call, const DenseWeights &w, int dop)
{
    const int n_ct = dop / 32;
    pack_weights_tall_kernel<<<dim3((unsigned)(w.n_chunks * n_ct)), 256, 0, call.stream>>>(w.W1, w.b1, w.W2, w.b2, call.d_in, call.d_out, dop,
                                                                                         w.Wt, w.bias2(dop));
    LAUNCH_CHECK();
    const int64_t groups = (call.n_rows + kTallRows - 1) / kTallRows;
    call.launch(layer_dense_tall_kernel, groups * (n_ct / 4), 256, 0, w.Wt, w.bias2(dop), w.n_chunks, n_ct);
    LAUNCH_CHECK();
    const unsigned scale_blocks = (unsigned)((call.n_rows + 3) / 4);
    if (dop == 256) row_scale_kernel<2><<<dim3(scale_blocks), 256, 0, call.stream>>>(call.norm, call.ldn, call.n_rows, call.d_out);
    else row_scale_kernel<4><<<dim3(scale_blocks), 256, 0, call.stream>>>(call.norm, call.ldn, call.n_rows, call.d_out);
    LAUNCH_CHECK();
    return NGCF_OK;
}
