// sampled_softmax.hip - the sampled softmax loss with the logQ correction and a temperature, loss and gradient (include/ngcf_hip.h,
// "Sampled softmax with logQ correction").
//
// The kernel shape is bpr_multi.hip's, on the same row machinery (loss_rows_device.h): one wave per positive row b, four rows per
// workgroup, lane j keeping the score of negative j - and its logq value, one coalesced load per wave.  The forward writes the
// two-float workgroup partials and ends in the shared second stage; the backward recomputes the scores and hands its coefficients
// to the shared walk over the negatives, without sign factors.  What is here is the loss's own: the corrected scores and the
// temperature's refusal.  No atomics, every sum in a fixed order, no host synchronisation.
//
// With inv_tau = 1, logq = 0, no pos_logq and positive dot products every value goes through the operations of bpr_multi.hip's
// softmax reduction in their order (x * 1 - 0 is x; its sign factors are exactly 1) - the log-sum-exp, the softmax weights and the
// walk are the same functions: tests/test_sampled_softmax_gpu.py holds the two equal bit for bit.
#include "common.h"

#pragma clang fp contract(off)

#include "loss_rows_device.h"

namespace {

// The corrected scores of a row: z0 (wave-uniform) and, per lane j < m, zj - one multiply and one subtract each (no fma).
struct Corrected {
    float z0, zj;
};

__device__ __forceinline__ Corrected correct(const Scores &s, float inv_tau, float c, float lq)
{
    Corrected z;
    z.z0 = s.up * inv_tau - c;
    z.zj = s.un * inv_tau - lq;
    return z;
}

// the lane's logq value (lane j: negative j of row b; 0 in the lanes from m on): one coalesced load per wave
__device__ __forceinline__ float lane_logq(const float *__restrict__ logq, int64_t b, int m, int lane)
{
    return lane < m ? logq[b * m + lane] : 0.f;
}

template <int KU>
__global__ __launch_bounds__(256) void sampled_softmax_rows_kernel(const float *__restrict__ u, const float *__restrict__ p,
                                                                   const float *__restrict__ n, const float *__restrict__ logq,
                                                                   const float *__restrict__ pos_logq, int64_t B, int m, int D,
                                                                   float inv_tau, float *__restrict__ part)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    float nl = 0.f, sq = 0.f;
    if (b < B) {
        const float inv_m = 1.f / (float)m;
        const float lq = lane_logq(logq, b, m, lane), c = pos_logq ? pos_logq[b] : 0.f;
        const URow<KU> ur(u + b * D, D, lane);
        const Scores s = score_row<KU>(ur, p + b * D, n + b * m * D, m, D, lane);
        const Corrected z = correct(s, inv_tau, c, lq);
        nl = -log_sigmoid(z.z0 - lanes_lse(z.zj, m, lane));                    // the lse runs over the negatives only
        sq = s.uu + s.pp + inv_m * s.nn;
    }
    bpr_block_partials(wave, lane, nl, sq, part);
}

template <int KU>
__global__ __launch_bounds__(256) void sampled_softmax_backward_kernel(const float *__restrict__ u, const float *__restrict__ p,
                                                                       const float *__restrict__ n, const float *__restrict__ logq,
                                                                       const float *__restrict__ pos_logq, int64_t B, int m, int D,
                                                                       float inv_tau, float wd, float batch_size,
                                                                       const float *__restrict__ gout, float *__restrict__ du,
                                                                       float *__restrict__ dp, float *__restrict__ dn)
{
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const float g = gout[0] / batch_size, inv_m = 1.f / (float)m;
    const float two_wd = 2.f * wd, two_wd_m = two_wd * inv_m;
    const float *__restrict__ pr = p + b * D, *__restrict__ nr = n + b * m * D;
    const float lq = lane_logq(logq, b, m, lane), c0 = pos_logq ? pos_logq[b] : 0.f;
    const URow<KU> ur(u + b * D, D, lane);
    const Scores sc = score_row<KU>(ur, pr, nr, m, D, lane);
    const Corrected z = correct(sc, inv_tau, c0, lq);
    const float s = -softmax_weight(z.z0, z.zj, m, lane) * inv_tau;            // lane j: -a_j inv_tau = -dl_b/d(u.n_j)
    gradient_walk<KU>(ur, pr, nr, m, D, s, NoSigns{}, g, two_wd, two_wd_m, du + b * D, dp + b * D, dn + b * m * D);
}

int check_shapes(const char *what, int64_t Bu, int64_t Bp, int64_t Bn, int m, int D, float inv_tau)
{
    if (const int rc = check_rows(what, Bu, Bp, Bn, m, D)) return rc;
    if (!(inv_tau > 0.f) || !(inv_tau < INFINITY))
        return fail(NGCF_ERR_ARG, "%s: inv_tau=%g is not a positive finite number", what, (double)inv_tau);
    return NGCF_OK;
}

}  // namespace

extern "C" int64_t ngcf_sampled_softmax_workspace_bytes(int64_t B) { return partials_workspace_bytes(B); }

extern "C" int ngcf_sampled_softmax_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn, int m, int D,
                                        const float *logq, const float *pos_logq, float inv_tau, float wd, float batch_size,
                                        float *loss, void *workspace, int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!u || !p || !n || !logq || !loss) return fail(NGCF_ERR_ARG, "sampled_softmax: null argument");
    if (const int rc = check_shapes("sampled_softmax", Bu, Bp, Bn, m, D, inv_tau)) return rc;
    float *part;
    if (const int rc = partials_in("sampled_softmax", workspace, workspace_bytes, Bu, &part)) return rc;
    LOSS_ROWS_LAUNCH(sampled_softmax_rows_kernel, Bu, stream, u, p, n, logq, pos_logq, Bu, m, D, inv_tau, part);
    return finish_loss(part, Bu, wd, batch_size, loss, stream);
}

extern "C" int ngcf_sampled_softmax_backward_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn,
                                                 int m, int D, const float *logq, const float *pos_logq, float inv_tau, float wd,
                                                 float batch_size, const float *grad_out, float *du, float *dp, float *dn,
                                                 void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!u || !p || !n || !logq || !grad_out || !du || !dp || !dn) return fail(NGCF_ERR_ARG, "sampled_softmax_backward: null argument");
    if (const int rc = check_shapes("sampled_softmax_backward", Bu, Bp, Bn, m, D, inv_tau)) return rc;
    LOSS_ROWS_LAUNCH(sampled_softmax_backward_kernel, Bu, stream, u, p, n, logq, pos_logq, Bu, m, D, inv_tau, wd, batch_size, grad_out, du,
                     dp, dn);
    return NGCF_OK;
}
