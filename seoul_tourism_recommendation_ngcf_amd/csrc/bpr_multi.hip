// bpr_multi.hip - BPR against m negatives per positive row, loss and gradient (include/ngcf_hip.h, "BPR, m negatives per positive").
//
// One wave per positive row b, four rows per workgroup, on the row machinery of loss_rows_device.h: the score pass leaves u.n_j in
// lane j (hence m <= 64), the forward writes the two-float workgroup partials of bpr_rows_kernel (ops.hip) and ends in the same
// second stage, the backward recomputes the scores, as ngcf_bpr_backward_f32 does, and hands its coefficients and sign factors to
// the shared walk over the negatives.  What is here is the loss's own: |.| on the scores, the two reductions, the reduction's
// refusal.  No atomics, every sum in a fixed order, no host synchronisation.
//
// With m = 1 and the mean reduction every value goes through the operations of bpr_rows_kernel / bpr_backward_kernel in their
// order, which is why the products and sums that those kernels' expressions compile to are spelled out (fmaf where the compiler
// fuses there, contraction off otherwise): tests/test_bpr_multi_gpu.py holds the two pairs equal bit for bit.
#include "common.h"

#pragma clang fp contract(off)

#include "loss_rows_device.h"

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
    return -log_sigmoid(sp - lanes_lse(sn, m, lane));
}

// s_j = dl_b/d(sn_j) negated, i.e. dl_b/dx_j for x_j = sp - sn_j, of the lane's negative (0 in the lanes from m on)
__device__ __forceinline__ float row_coefficient(const Scores &s, int m, float inv_m, int reduction, int lane)
{
    const float sp = fabsf(s.up), sn = fabsf(s.un);
    if (reduction == kMeanReduction) {
        const float c = -inv_m / (1.f + expf(sp - sn));                        // d(-logsigmoid(x))/dx = -sigmoid(-x), over m
        return lane < m ? c : 0.f;
    }
    return -softmax_weight(sp, sn, m, lane);
}

template <int KU>
__global__ __launch_bounds__(256) void bpr_multi_rows_kernel(const float *__restrict__ u, const float *__restrict__ p,
                                                             const float *__restrict__ n, int64_t B, int m, int D, int reduction,
                                                             float *__restrict__ part)
{
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
    bpr_block_partials(wave, lane, nl, sq, part);
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
    const URow<KU> ur(u + b * D, D, lane);
    const Scores sc = score_row<KU>(ur, pr, nr, m, D, lane);
    const float s = row_coefficient(sc, m, inv_m, reduction, lane);           // lane j: s_j
    gradient_walk<KU>(ur, pr, nr, m, D, s, RowSigns{sign_of(sc.up), sign_of(sc.un)}, g, two_wd, two_wd_m, du + b * D, dp + b * D,
                      dn + b * m * D);
}

int check_shapes(const char *what, int64_t Bu, int64_t Bp, int64_t Bn, int m, int D, int reduction)
{
    if (const int rc = check_rows(what, Bu, Bp, Bn, m, D)) return rc;
    if (reduction != kMeanReduction && reduction != kSoftmaxReduction)
        return fail(NGCF_ERR_ARG, "%s: reduction=%d is neither NGCF_BPR_MULTI_MEAN nor NGCF_BPR_MULTI_SOFTMAX", what, reduction);
    return NGCF_OK;
}

}  // namespace

extern "C" int64_t ngcf_bpr_multi_workspace_bytes(int64_t B) { return partials_workspace_bytes(B); }

extern "C" int ngcf_bpr_multi_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn, int m, int D,
                                  int reduction, float wd, float batch_size, float *loss, void *workspace, int64_t workspace_bytes,
                                  void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!u || !p || !n || !loss) return fail(NGCF_ERR_ARG, "bpr_multi: null argument");
    if (const int rc = check_shapes("bpr_multi", Bu, Bp, Bn, m, D, reduction)) return rc;
    float *part;
    if (const int rc = partials_in("bpr_multi", workspace, workspace_bytes, Bu, &part)) return rc;
    LOSS_ROWS_LAUNCH(bpr_multi_rows_kernel, Bu, stream, u, p, n, Bu, m, D, reduction, part);
    return finish_loss(part, Bu, wd, batch_size, loss, stream);
}

extern "C" int ngcf_bpr_multi_backward_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn, int m,
                                           int D, int reduction, float wd, float batch_size, const float *grad_out, float *du,
                                           float *dp, float *dn, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!u || !p || !n || !grad_out || !du || !dp || !dn) return fail(NGCF_ERR_ARG, "bpr_multi_backward: null argument");
    if (const int rc = check_shapes("bpr_multi_backward", Bu, Bp, Bn, m, D, reduction)) return rc;
    LOSS_ROWS_LAUNCH(bpr_multi_backward_kernel, Bu, stream, u, p, n, Bu, m, D, reduction, wd, batch_size, grad_out, du, dp, dn);
    return NGCF_OK;
}
