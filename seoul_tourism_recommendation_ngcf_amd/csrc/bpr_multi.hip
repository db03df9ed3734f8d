// bpr_multi.hip - BPR against m negatives per positive row, loss and gradient (include/ngcf_hip.h, "BPR, m negatives per positive").
//
// One wave per positive row b, four rows per workgroup.  The wave keeps its u row in registers (KU values per lane, D <= 64 KU),
// streams the m negative rows of the row once - R at a time, so that the loads of R rows are in flight together - and lane j keeps
// the score |u.n_j| of negative j, hence m <= 64.  The forward writes the two-float workgroup partials of bpr_rows_kernel (ops.hip)
// and ends in the same second stage (bpr_finish_block, common.h).  The backward recomputes the scores, as ngcf_bpr_backward_f32
// does, and walks the negatives a second time (cache hits), R rows at a time again: it writes dn_j on the way and keeps the lane's
// columns of du in registers.  (D > 2048, no registers for the row: column by column, the m rows below each.)  No atomics, every sum
// in a fixed order, no host synchronisation.
//
// With m = 1 and the mean reduction every value below goes through the operations of bpr_rows_kernel / bpr_backward_kernel in their
// order, which is why the products and sums that those kernels' expressions compile to are spelled out here (fmaf where the compiler
// fuses there, contraction off otherwise): tests/test_bpr_multi_gpu.py holds the two pairs equal bit for bit.
#include "common.h"

#pragma clang fp contract(off)

#include "loss_rows_device.h"          // URow, RowBatch, score_row, wave_max, lane_value, LOSS_ROWS_DISPATCH

namespace {

constexpr int kMeanReduction = 0, kSoftmaxReduction = 1;

__device__ inline float sign_of(float t) { return t > 0.f ? 1.f : (t < 0.f ? -1.f : 0.f); }      // d|t|/dt, 0 at 0 like torch.abs

// l_b of the row from the lanes' scores
__device__ __forceinline__ float row_loss(const Scores &s, int m, float inv_m, int reduction, int lane)
{
    const float sp = fabsf(s.up), sn = fabsf(s.un);
    if (reduction == kMeanReduction) {
        const float ls = lane < m ? log_sigmoid(sp - sn) : 0.f;                 // bprloss.py:16-19 per negative
        return -(inv_m * wave_sum(ls));
    }
    const float M = wave_max(lane < m ? sn : -INFINITY);
    const float e = lane < m ? expf(sn - M) : 0.f;
    const float lse = M + logf(wave_sum(e));
    return -log_sigmoid(sp - lse);
}

// s_j = dl_b/d(sn_j) negated, i.e. dl_b/dx_j for x_j = sp - sn_j, of the lane's negative (0 in the lanes from m on)
__device__ __forceinline__ float row_coefficient(const Scores &s, int m, float inv_m, int reduction, int lane)
{
    const float sp = fabsf(s.up), sn = fabsf(s.un);
    if (reduction == kMeanReduction) {
        const float c = -inv_m / (1.f + expf(sp - sn));                        // d(-logsigmoid(x))/dx = -sigmoid(-x), over m
        return lane < m ? c : 0.f;
    }
    const float M = fmaxf(sp, wave_max(lane < m ? sn : -INFINITY));
    const float e = lane < m ? expf(sn - M) : 0.f;
    const float den = expf(sp - M) + wave_sum(e);
    return -(e / den);
}

template <int KU>
__global__ __launch_bounds__(256) void bpr_multi_rows_kernel(const float *__restrict__ u, const float *__restrict__ p,
                                                             const float *__restrict__ n, int64_t B, int m, int D, int reduction,
                                                             float *__restrict__ part)
{
    __shared__ float sh[8];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    float nl = 0.f, sq = 0.f;
    if (b < B) {
        const float inv_m = 1.f / (float)m;
        const URow<KU> ur(u + b * D, D, lane);
        const Scores s = score_row<KU>(ur, p + b * D, n + b * m * D, m, D, lane);
        nl = row_loss(s, m, inv_m, reduction, lane);
        sq = s.uu + s.pp + inv_m * s.nn;
    }
    if (lane == 0) {
        sh[wave * 2] = nl;
        sh[wave * 2 + 1] = sq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[2 * (int64_t)blockIdx.x] = (sh[0] + sh[2]) + (sh[4] + sh[6]);
        part[2 * (int64_t)blockIdx.x + 1] = (sh[1] + sh[3]) + (sh[5] + sh[7]);
    }
}

__global__ __launch_bounds__(256) void bpr_multi_finish_kernel(const float *__restrict__ part, int64_t n_blocks, float wd,
                                                               float batch_size, float *__restrict__ loss)
{
    bpr_finish_block(part, n_blocks, wd, batch_size, loss);
}

template <int KU>
__global__ __launch_bounds__(256) void bpr_multi_backward_kernel(const float *__restrict__ u, const float *__restrict__ p,
                                                                 const float *__restrict__ n, int64_t B, int m, int D, int reduction,
                                                                 float wd, float batch_size, const float *__restrict__ gout,
                                                                 float *__restrict__ du, float *__restrict__ dp, float *__restrict__ dn)
{
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const float g = gout[0] / batch_size, inv_m = 1.f / (float)m;
    const float two_wd = 2.f * wd, two_wd_m = two_wd * inv_m;
    const float *__restrict__ pr = p + b * D, *__restrict__ nr = n + b * m * D;
    float *__restrict__ dur = du + b * D, *__restrict__ dpr = dp + b * D, *__restrict__ dnr = dn + b * m * D;
    const URow<KU> ur(u + b * D, D, lane);
    const Scores sc = score_row<KU>(ur, pr, nr, m, D, lane);
    const float s = row_coefficient(sc, m, inv_m, reduction, lane);           // lane j: s_j
    const float sgn_n = sign_of(sc.un);                                        // lane j: sgn_nj
    const float sgn_p = sign_of(sc.up);
    const float cp = wave_sum(s) * sgn_p;                                      // -A sgn_p
    // du/g = 2 wd u + sum_j s_j (sgn_p p - sgn_nj n_j) in four chains, as the gathers' backward sums its rows (bwd_gather.hip): chain q
    // takes the negatives j = q mod 4 in ascending order, one fma each, chain 0 starts from the weight-decay term, and the chains
    // combine as (c0 + c1) + (c2 + c3).  With m = 1 that is bpr_backward_kernel's fma(s, sgn_p p - sgn_n n, 2 wd u).
    if constexpr (KU > 0) {                 // second walk over the rows, R at a time; the lane's columns of du stay in registers
        float acc[4][KU], pb[KU];
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int col = lane + 64 * k;
            const float a = ur.v[k], bb = col < D ? pr[col] : 0.f;
            pb[k] = sgn_p * bb;
            acc[0][k] = two_wd * a;
            acc[1][k] = acc[2][k] = acc[3][k] = 0.f;
            if (col < D) dpr[col] = g * fmaf(cp, a, two_wd * bb);
        }
        constexpr int R = RowBatch<KU>::R;
        static_assert(4 % R == 0, "a batch of rows never straddles a group of four");
        for (int j0 = 0; j0 < m; j0 += 4) {
#pragma unroll
            for (int h = 0; h < 4; h += R) {
                if (j0 + h >= m) break;
                float c[R][KU];
#pragma unroll
                for (int r = 0; r < R; ++r) {   // (rows past m: row m - 1 again, dropped below)
                    const float *nj = nr + (int64_t)min(j0 + h + r, m - 1) * D;
#pragma unroll
                    for (int k = 0; k < KU; ++k) c[r][k] = lane + 64 * k < D ? nj[lane + 64 * k] : 0.f;
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int j = j0 + h + r;
                    if (j >= m) break;
                    const float sj = lane_value(s, j), gj = lane_value(sgn_n, j), cn = -sj * gj;
                    float *dnj = dnr + (int64_t)j * D;
#pragma unroll
                    for (int k = 0; k < KU; ++k) {
                        if (lane + 64 * k < D) dnj[lane + 64 * k] = g * fmaf(cn, ur.v[k], two_wd_m * c[r][k]);
                        acc[h + r][k] = fmaf(sj, pb[k] - gj * c[r][k], acc[h + r][k]);
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < KU; ++k)
            if (lane + 64 * k < D) dur[lane + 64 * k] = g * ((acc[0][k] + acc[1][k]) + (acc[2][k] + acc[3][k]));
    } else {                                // D > 2048: column by column, the m rows below each
        for (int col = lane; col < D; col += 64) {
            const float a = ur.row[col], bb = pr[col], pb = sgn_p * bb;
            float acc[4] = {two_wd * a, 0.f, 0.f, 0.f};
            for (int j0 = 0; j0 < m; j0 += 4) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = j0 + q;
                    if (j >= m) break;
                    const float c = nr[(int64_t)j * D + col];
                    const float sj = lane_value(s, j), gj = lane_value(sgn_n, j);
                    dnr[(int64_t)j * D + col] = g * fmaf(-sj * gj, a, two_wd_m * c);
                    acc[q] = fmaf(sj, pb - gj * c, acc[q]);
                }
            }
            dur[col] = g * ((acc[0] + acc[1]) + (acc[2] + acc[3]));
            dpr[col] = g * fmaf(cp, a, two_wd * bb);
        }
    }
}

template <int KU>
int launch_forward(const float *u, const float *p, const float *n, int64_t B, int m, int D, int reduction, float *part,
                   hipStream_t stream)
{
    bpr_multi_rows_kernel<KU><<<dim3((unsigned)((B + 3) / 4)), 256, 0, stream>>>(u, p, n, B, m, D, reduction, part);
    LAUNCH_CHECK();
    return NGCF_OK;
}

template <int KU>
int launch_backward(const float *u, const float *p, const float *n, int64_t B, int m, int D, int reduction, float wd,
                    float batch_size, const float *gout, float *du, float *dp, float *dn, hipStream_t stream)
{
    bpr_multi_backward_kernel<KU><<<dim3((unsigned)((B + 3) / 4)), 256, 0, stream>>>(u, p, n, B, m, D, reduction, wd, batch_size,
                                                                                    gout, du, dp, dn);
    LAUNCH_CHECK();
    return NGCF_OK;
}

int check_shapes(const char *what, int64_t Bu, int64_t Bp, int64_t Bn, int m, int D, int reduction)
{
    if (D <= 0) return fail(NGCF_ERR_ARG, "%s: D=%d", what, D);
    if (m < 1 || m > NGCF_BPR_MULTI_M_MAX) return fail(NGCF_ERR_ARG, "%s: m=%d outside [1, %d]", what, m, NGCF_BPR_MULTI_M_MAX);
    if (reduction != kMeanReduction && reduction != kSoftmaxReduction)
        return fail(NGCF_ERR_ARG, "%s: reduction=%d is neither NGCF_BPR_MULTI_MEAN nor NGCF_BPR_MULTI_SOFTMAX", what, reduction);
    if (Bu < 1 || Bu > ((int64_t)1 << 32) || Bp != Bu || Bn != Bu * m)
        return fail(NGCF_ERR_ARG, "%s: row counts %lld/%lld/%lld are not B/B/B*m with m=%d (no operand broadcasts)", what, (long long)Bu,
                    (long long)Bp, (long long)Bn, m);
    return NGCF_OK;
}

}  // namespace

extern "C" int64_t ngcf_bpr_multi_workspace_bytes(int64_t B)
{
    if (B < 0) return -1;
    return align_up(((B + 3) / 4) * 2 * (int64_t)sizeof(float), 256) + 256;
}

static int forward_kernel(const float *u, const float *p, const float *n, int64_t B, int m, int D, int reduction, float *part,
                          hipStream_t stream)
{
    LOSS_ROWS_DISPATCH(launch_forward, u, p, n, B, m, D, reduction, part, stream)
}

static int backward_kernel(const float *u, const float *p, const float *n, int64_t B, int m, int D, int reduction, float wd,
                           float batch_size, const float *gout, float *du, float *dp, float *dn, hipStream_t stream)
{
    LOSS_ROWS_DISPATCH(launch_backward, u, p, n, B, m, D, reduction, wd, batch_size, gout, du, dp, dn, stream)
}

extern "C" int ngcf_bpr_multi_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn, int m, int D,
                                  int reduction, float wd, float batch_size, float *loss, void *workspace, int64_t workspace_bytes,
                                  void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!u || !p || !n || !loss) return fail(NGCF_ERR_ARG, "bpr_multi: null argument");
    if (const int rc = check_shapes("bpr_multi", Bu, Bp, Bn, m, D, reduction)) return rc;
    const int64_t need = ngcf_bpr_multi_workspace_bytes(Bu);
    if (!workspace || workspace_bytes < need)
        return fail(NGCF_ERR_WORKSPACE, "bpr_multi: workspace %lld B < %lld B", (long long)workspace_bytes, (long long)need);
    float *part = reinterpret_cast<float *>(align_up((int64_t)(uintptr_t)workspace, 256));
    if (const int rc = forward_kernel(u, p, n, Bu, m, D, reduction, part, stream)) return rc;
    bpr_multi_finish_kernel<<<1, 256, 0, stream>>>(part, (Bu + 3) / 4, wd, batch_size, loss);
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_bpr_multi_backward_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn, int m,
                                           int D, int reduction, float wd, float batch_size, const float *grad_out, float *du,
                                           float *dp, float *dn, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!u || !p || !n || !grad_out || !du || !dp || !dn) return fail(NGCF_ERR_ARG, "bpr_multi_backward: null argument");
    if (const int rc = check_shapes("bpr_multi_backward", Bu, Bp, Bn, m, D, reduction)) return rc;
    return backward_kernel(u, p, n, Bu, m, D, reduction, wd, batch_size, grad_out, du, dp, dn, stream);
}
