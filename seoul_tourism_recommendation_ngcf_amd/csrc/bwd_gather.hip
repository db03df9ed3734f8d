// bwd_gather.hip - the loss and gather side of the backward pass: BPR gradient, the gathers' gradient rows summed per distinct row,
// the distinct rows of an index vector.  (The layer's dense half: bwd_dense.hip; L^T . dLE for a row-sparse dLE: spmm_t_rows.hip.)
#include "common.h"

// =============================================================================================
// Backward pass (`loss.backward()` in experiment.py:57).
// Everything the backward runs besides L^T . dLE on the SpMM kernels: BPR gradient, the gathers' gradient rows summed per
// distinct row, normalise/dropout/LeakyReLU backward, weight and input gradients on the fp32 matrix cores, and L^T . dLE for
// a row-sparse dLE.  No library GEMM, no atomics: every sum has a fixed order (bit-identical gradients from run to run).
// =============================================================================================

// ---- BPR backward (bprloss.py:15-22) ----------------------------------------------------------
// loss = (-sum logsig(|u.p| - |u.n|) + wd (|u|^2 + |p|^2 + |n|^2)) / bs ; one wave per row
// A row's share of both kernels below, which fill the rows and the broadcast sum of the SAME loss: x = |u.p| - |u.n| from the two
// dot products (summed over the wave), s = d(-logsigmoid(x))/dx and the two signs.
struct BprRow {
    float s, sp, sn;
};
__device__ __forceinline__ BprRow bpr_row(const float *__restrict__ ur, const float *__restrict__ pr, const float *__restrict__ nr, int D, int lane)
{
    float up = 0.f, un = 0.f;
    for (int j = lane; j < D; j += 64) {
        up = fmaf(ur[j], pr[j], up);
        un = fmaf(ur[j], nr[j], un);
    }
    up = wave_sum(up);
    un = wave_sum(un);
    const float x = fabsf(up) - fabsf(un);
    BprRow k;
    k.s = -1.f / (1.f + expf(x));                            // d(-logsigmoid(x))/dx = -sigmoid(-x)
    k.sp = up > 0.f ? 1.f : (up < 0.f ? -1.f : 0.f);          // d|t|/dt, 0 at 0 like torch.abs
    k.sn = un > 0.f ? 1.f : (un < 0.f ? -1.f : 0.f);
    return k;
}

__global__ __launch_bounds__(256) void bpr_backward_kernel(const float *__restrict__ u, int64_t Bu,
                                                           const float *__restrict__ p, int64_t Bp,
                                                           const float *__restrict__ n, int64_t Bn, int64_t R, int D,
                                                           float wd, float batch_size, const float *__restrict__ gout,
                                                           float *__restrict__ du, float *__restrict__ dp,
                                                           float *__restrict__ dn)
{
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int lane = threadIdx.x & 63;
    const float g = gout[0] / batch_size;
    const int64_t ru = Bu == 1 ? 0 : r, rp = Bp == 1 ? 0 : r, rn = Bn == 1 ? 0 : r;
    const float *ur = u + ru * D, *pr = p + rp * D, *nr = n + rn * D;
    const BprRow k = bpr_row(ur, pr, nr, D, lane);
    const float s = k.s, sp = k.sp, sn = k.sn, two_wd = 2.f * wd;
    for (int j = lane; j < D; j += 64) {
        const float a = ur[j], b = pr[j], c = nr[j];
        // the weight-decay term of a broadcast row is counted once (its own single row)
        const float gu = g * (s * (sp * b - sn * c) + ((Bu == 1 && r > 0) ? 0.f : two_wd * a));
        const float gp = g * (s * sp * a + ((Bp == 1 && r > 0) ? 0.f : two_wd * b));
        const float gn = g * (-s * sn * a + ((Bn == 1 && r > 0) ? 0.f : two_wd * c));
        if (Bu == R) du[ru * D + j] = gu;          // a broadcast operand's gradient is a sum over the rows: bpr_backward_bcast_kernel
        if (Bp == R) dp[rp * D + j] = gp;
        if (Bn == R) dn[rn * D + j] = gn;
    }
}

// The gradient of a BROADCAST operand (a [1, D] row against R > 1 rows: bprloss.py broadcasts like torch): the sum of the per-row
// terms in ROW ORDER, by one workgroup - the per-row coefficients of 256 rows at a time into LDS (a wave per row), then a thread
// per column adds them up.  (r04: this was three float atomicAdds per element - the last ones in the library; a rare path, R * D
// multiply-adds on one CU.)
__global__ __launch_bounds__(256) void bpr_backward_bcast_kernel(const float *__restrict__ u, int64_t Bu, const float *__restrict__ p,
                                                                 int64_t Bp, const float *__restrict__ n, int64_t Bn, int64_t R, int D,
                                                                 float wd, float batch_size, const float *__restrict__ gout,
                                                                 float *__restrict__ du, float *__restrict__ dp, float *__restrict__ dn)
{
    __shared__ float c_pos[256], c_neg[256];                   // s * sign(u.p), s * sign(u.n) of the rows of a chunk
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float g = gout[0] / batch_size, two_wd = 2.f * wd;
    for (int j0 = 0; j0 < D; j0 += 256) {
        const int j = j0 + threadIdx.x;
        float au = 0.f, ap = 0.f, an = 0.f;
        for (int64_t r0 = 0; r0 < R; r0 += 256) {
            const int cnt = (int)(R - r0 < 256 ? R - r0 : 256);
            __syncthreads();
            for (int rr = wave; rr < cnt; rr += 4) {
                const int64_t r = r0 + rr;
                const float *ur = u + (Bu == 1 ? 0 : r) * D, *pr = p + (Bp == 1 ? 0 : r) * D, *nr = n + (Bn == 1 ? 0 : r) * D;
                const BprRow k = bpr_row(ur, pr, nr, D, lane);
                if (lane == 0) c_pos[rr] = k.s * k.sp, c_neg[rr] = k.s * k.sn;
            }
            __syncthreads();
            if (j < D)
                for (int rr = 0; rr < cnt; ++rr) {
                    const int64_t r = r0 + rr;
                    const float a = u[(Bu == 1 ? 0 : r) * D + j], b = p[(Bp == 1 ? 0 : r) * D + j], c = n[(Bn == 1 ? 0 : r) * D + j];
                    au += c_pos[rr] * b - c_neg[rr] * c;
                    ap = fmaf(c_pos[rr], a, ap);
                    an = fmaf(-c_neg[rr], a, an);
                }
        }
        if (j < D) {                                           // the weight-decay term of a broadcast row is counted once
            if (Bu == 1) du[j] = g * (au + two_wd * u[j]);
            if (Bp == 1) dp[j] = g * (ap + two_wd * p[j]);
            if (Bn == 1) dn[j] = g * (an + two_wd * n[j]);
        }
    }
}

extern "C" int ngcf_bpr_backward_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn,
                                     int D, float wd, float batch_size, const float *grad_out, float *du, float *dp,
                                     float *dn, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!u || !p || !n || !grad_out || !du || !dp || !dn || D <= 0) return fail(NGCF_ERR_ARG, "bpr_backward: null argument");
    const int64_t R = std::max(Bu, std::max(Bp, Bn));
    if (R < 1 || (Bu != 1 && Bu != R) || (Bp != 1 && Bp != R) || (Bn != 1 && Bn != R))
        return fail(NGCF_ERR_ARG, "bpr_backward: row counts %lld/%lld/%lld do not broadcast", (long long)Bu, (long long)Bp, (long long)Bn);
    bpr_backward_kernel<<<dim3((unsigned)((R + 3) / 4)), 256, 0, stream>>>(u, Bu, p, Bp, n, Bn, R, D, wd, batch_size, grad_out,
                                                                            du, dp, dn);
    LAUNCH_CHECK();
    if (Bu != R || Bp != R || Bn != R) {                        // (only with R > 1: an operand of one row against several)
        bpr_backward_bcast_kernel<<<1, 256, 0, stream>>>(u, Bu, p, Bp, n, Bn, R, D, wd, batch_size, grad_out, du, dp, dn);
        LAUNCH_CHECK();
    }
    return NGCF_OK;
}

// ---- gather backward: the gradient rows of the (users, positive items, negative items) gathers (NGCF.py:151-155), summed per
// distinct row of all_E in a FIXED order: out[r, :] = sum over j in [segptr[r], segptr[r+1]) of g[order[j], :], in that order
// (the caller sorts the gathered positions by row, stable, so duplicates add up in batch order).  No atomics: two runs give
// the same bits.  One wave per output row.
__global__ __launch_bounds__(256) void segment_sum_rows_kernel(const float *__restrict__ g, int64_t ldg, int d,
                                                               const int64_t *__restrict__ order, const int64_t *__restrict__ segptr,
                                                               int64_t n_seg, const int64_t *__restrict__ dst_rows,
                                                               const int64_t *__restrict__ n_seg_dev, float *__restrict__ out, int64_t ldo,
                                                               int64_t n_out_rows)
{
    int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_seg || (n_seg_dev && r >= *n_seg_dev)) return;       // n_seg_dev: the number of segments lives on the device
    const int64_t j0 = segptr[r], j1 = segptr[r + 1];
    if (dst_rows) {                                                 // scatter form: segment r is row dst_rows[r] of a larger matrix
        r = dst_rows[r];
        if (r < 0 || r >= n_out_rows) return;                       // (an id the forward gather clamped and flagged: nothing to add, nothing written)
    }
    // four chains over the segment (positions j0 + 4 i + q; the last (j1 - j0) % 4 positions go to chain 0), combined as
    // (s0 + s1) + (s2 + s3): a fixed order.  r04: the positions `order[j]` of 64 entries are fetched by ONE load (a lane each) and
    // handed round with readlane, a lane keeps the sums of five column blocks and sixteen gradient rows are requested before the
    // first is added - the loads depend on nothing but that one load (before: order -> row -> next order, twice per group of four,
    // for every column block: a popular item is gathered 40 times in a batch of 1 024 on the Seoul graph's 100 items - 22 us).
    const int lane = threadIdx.x & 63;
    const int64_t n4 = (j1 - j0) / 4 * 4;                           // entries in full groups of four
    constexpr int kQ = 5;                                           // column blocks of 64 per pass (the Seoul model's 260 columns: one pass)
    for (int c0 = 0; c0 < d; c0 += 64 * kQ) {
        float s[kQ][4];
#pragma unroll
        for (int q = 0; q < kQ; ++q) s[q][0] = s[q][1] = s[q][2] = s[q][3] = 0.f;
        for (int64_t jb = j0; jb < j1; jb += 64) {                  // (jb - j0 is a multiple of 64: groups of four never straddle)
            const int cnt = (int)(j1 - jb < 64 ? j1 - jb : 64);
            const long long ord = order[jb + (lane < cnt ? lane : 0)];
            const int lo = (int)(ord & 0xffffffffll), hi = (int)(ord >> 32);
            const auto row_of = [&](int t) {
                return g + (((long long)__builtin_amdgcn_readlane(hi, t) << 32) | (unsigned)__builtin_amdgcn_readlane(lo, t)) * ldg + c0 + lane;
            };
            const auto add_rows = [&](auto n, int t) {                     // G rows (groups of four) requested together, added in group order
                constexpr int G = decltype(n)::value;
                float v[G][kQ];
#pragma unroll
                for (int u = 0; u < G; ++u) {
                    const float *gp = row_of(t + u);
#pragma unroll
                    for (int q = 0; q < kQ; ++q) v[u][q] = c0 + lane + 64 * q < d ? gp[64 * q] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < G; ++u)
#pragma unroll
                    for (int q = 0; q < kQ; ++q) s[q][u & 3] += v[u][q];
            };
            int t = 0;
            for (; t + 16 <= cnt && jb - j0 + t + 16 <= n4; t += 16) add_rows(std::integral_constant<int, 16>{}, t);   // sixteen rows in flight
            for (; t + 4 <= cnt && jb - j0 + t + 4 <= n4; t += 4) add_rows(std::integral_constant<int, 4>{}, t);
            for (; t < cnt; ++t) {
                const float *gp = row_of(t);
#pragma unroll
                for (int q = 0; q < kQ; ++q)
                    if (c0 + lane + 64 * q < d) s[q][0] += gp[64 * q];
            }
        }
#pragma unroll
        for (int q = 0; q < kQ; ++q)
            if (c0 + lane + 64 * q < d) out[r * ldo + c0 + lane + 64 * q] = (s[q][0] + s[q][1]) + (s[q][2] + s[q][3]);
    }
}

extern "C" int ngcf_segment_sum_rows_f32(const float *g, int64_t ldg, int d, const int64_t *order, const int64_t *segptr,
                                         int64_t n_seg, const int64_t *dst_rows, const int64_t *n_seg_dev, float *out, int64_t ldo,
                                         int64_t n_out_rows, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_seg == 0) return NGCF_OK;
    if (!g || !order || !segptr || !out || d <= 0 || ldg < d || ldo < d || n_seg < 0) return fail(NGCF_ERR_ARG, "segment_sum_rows: bad argument");
    if (dst_rows && n_out_rows <= 0) return fail(NGCF_ERR_ARG, "segment_sum_rows: the scatter form needs the row count of out");
    if ((n_seg + 3) / 4 >= (int64_t)1 << 31) return fail(NGCF_ERR_ARG, "segment_sum_rows: too many rows");
    segment_sum_rows_kernel<<<dim3((unsigned)((n_seg + 3) / 4)), 256, 0, stream>>>(g, ldg, d, order, segptr, n_seg, dst_rows, n_seg_dev, out, ldo,
                                                                                   n_out_rows);
    LAUNCH_CHECK();
    return NGCF_OK;
}


// =============================================================================================
// The distinct rows of a small index vector, in ONE launch (r03).  The gradient of all_E is non-zero on the rows the three
// gathers of a forward touched (NGCF.py:151-155): M = |u_id| + |pos_item| + |neg_item| <= 3 B positions, with duplicates.  The
// backward needs them sorted, distinct, and - for a summation in a fixed order - the gathered positions grouped by row in batch
// order.  torch.unique(return_inverse, return_counts) + a stable sort of the inverse + a cumsum are ~12 library launches of
// 5-40 us each on a launch-bound training step; for M <= 8 192 one workgroup does all of it in LDS: a bitonic sort of the 64-bit
// keys (row << 13 | position: equal rows keep their batch order), head flags, a scan.  Outputs: order[M] (positions, sorted by
// row), rows[<= M] (distinct, ascending), segptr[<= M + 1] (group bounds inside `order`), n_rows[1].
// =============================================================================================
static constexpr int kSortMax = 8192, kSortThreads = 1024;

template <typename K>     // key type: 32 bits when row << 13 | position fits (rows below 2^19: the Seoul graph), else 64
__global__ __launch_bounds__(kSortThreads) void rows_sort_unique_kernel(const int64_t *__restrict__ idx, int M, int64_t max_row,
                                                                        int64_t *__restrict__ order, int64_t *__restrict__ rows,
                                                                        int64_t *__restrict__ segptr, int64_t *__restrict__ n_rows)
{
    __shared__ K key[kSortMax];
    __shared__ int wsum[kSortThreads / 64];
    __shared__ int carry_s;
    const int tid = threadIdx.x;
    int P = 64;
    while (P < M) P <<= 1;                                          // power of two >= M
    // An id outside [0, max_row] (the forward gather clamped it and set the sticky status word; with deferred index checks the
    // backward may still run) becomes the one sentinel row max_row + 1: it sorts behind every valid row, forms the last segment
    // and is NOT counted in n_rows - nothing downstream ever indexes all_E with it.
    for (int i = tid; i < P; i += kSortThreads) {
        K k = (K)~(K)0;
        if (i < M) {
            int64_t r = idx[i];
            if (max_row >= 0 && (r < 0 || r > max_row)) r = max_row + 1;
            k = (K)(((K)r << 13) | (K)i);
        }
        key[i] = k;
    }
    __syncthreads();
    // one comparator per thread and pass: pair t exchanges i = (t with a zero bit inserted at log2 j) and i + j.  At j <= 64 the 64
    // pairs of a wave stay inside one 128-key block, so those passes need no workgroup barrier - a wave's LDS operations complete in
    // order - only the wait for its own outstanding ones (r03: 78 barriers for M = 3 072 before, 27 now).
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += kSortThreads) {
                const int i = 2 * t - (t & (j - 1)), l = i + j;
                const K a = key[i], b = key[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) {
                    key[i] = b;
                    key[l] = a;
                }
            }
            if (j > 64 || j == 1) __syncthreads();
            else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
    // head flags + exclusive scan (chunks of kSortThreads, running carry)
    if (tid == 0) carry_s = 0;
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int base = 0; base < M; base += kSortThreads) {
        const int i = base + tid;
        int head = 0;
        K kv = 0;
        if (i < M) {
            kv = key[i];
            order[i] = (int64_t)(kv & 8191u);
            head = i == 0 || (key[i - 1] >> 13) != (kv >> 13);
        }
        int incl = head;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = carry_s;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (head) {
            const int r = before + incl - 1;
            rows[r] = (int64_t)(kv >> 13);
            segptr[r] = i;
        }
        __syncthreads();
        if (tid == kSortThreads - 1) carry_s = before + incl;
        __syncthreads();
    }
    if (tid == 0) {
        segptr[carry_s] = M;
        const bool sentinel = max_row >= 0 && M > 0 && (int64_t)(key[M - 1] >> 13) == max_row + 1;
        n_rows[0] = carry_s - (sentinel ? 1 : 0);
    }
}

extern "C" int ngcf_rows_sort_unique(const int64_t *idx, int64_t M, int64_t max_row, int64_t *order, int64_t *rows, int64_t *segptr,
                                     int64_t *n_rows, void *stream)
{
    if (M < 0 || M > kSortMax) return fail(NGCF_ERR_ARG, "rows_sort_unique: M=%lld not in [0, %d]", (long long)M, kSortMax);
    if (!order || !rows || !segptr || !n_rows || (M > 0 && !idx)) return fail(NGCF_ERR_ARG, "rows_sort_unique: null argument");
    if (max_row >= ((int64_t)1 << 50)) return fail(NGCF_ERR_ARG, "rows_sort_unique: rows must be below 2^50");
    if (max_row >= 0 && max_row < ((int64_t)1 << 19) - 2)
        rows_sort_unique_kernel<unsigned><<<1, kSortThreads, 0, (hipStream_t)stream>>>(idx, (int)M, max_row, order, rows, segptr, n_rows);
    else
        rows_sort_unique_kernel<unsigned long long><<<1, kSortThreads, 0, (hipStream_t)stream>>>(idx, (int)M, max_row, order, rows, segptr, n_rows);
    LAUNCH_CHECK();
    return NGCF_OK;
}
