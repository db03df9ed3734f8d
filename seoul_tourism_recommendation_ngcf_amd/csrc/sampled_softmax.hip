// sampled_softmax.hip - the sampled softmax loss with the logQ correction and a temperature, loss and gradient (include/ngcf_hip.h,
// "Sampled softmax with logQ correction").
//
// The kernel shape is bpr_multi.hip's, on the same row machinery (loss_rows_device.h): one wave per positive row b, four rows per
// workgroup, the u row in KU registers per lane, the m negative rows streamed once, R at a time, lane j keeping the score of
// negative j - and its logq value, one coalesced load per wave.  The forward writes the two-float workgroup partials and ends in
// bpr_finish_block (common.h); the backward recomputes the scores and walks the negatives a second time (cache hits), writing dn_j
// on the way with the lane's columns of du in registers (D > 2048: column by column).  No atomics, every sum in a fixed order, no
// host synchronisation.
//
// With inv_tau = 1, logq = 0, no pos_logq and positive dot products every value below goes through the operations of bpr_multi.hip's
// softmax reduction in their order (x * 1 - 0 is x; its sign factors are exactly 1): tests/test_sampled_softmax_gpu.py holds the two
// equal bit for bit.
#include "common.h"

#pragma clang fp contract(off)

#include "loss_rows_device.h"          // URow, RowBatch, score_row, wave_max, lane_value, LOSS_ROWS_DISPATCH

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
    __shared__ float sh[8];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    float nl = 0.f, sq = 0.f;
    if (b < B) {
        const float inv_m = 1.f / (float)m;
        const float lq = lane_logq(logq, b, m, lane), c = pos_logq ? pos_logq[b] : 0.f;
        const URow<KU> ur(u + b * D, D, lane);
        const Scores s = score_row<KU>(ur, p + b * D, n + b * m * D, m, D, lane);
        const Corrected z = correct(s, inv_tau, c, lq);
        const float M = wave_max(lane < m ? z.zj : -INFINITY);                 // the lse runs over the negatives only
        const float e = lane < m ? expf(z.zj - M) : 0.f;
        const float lse = M + logf(wave_sum(e));
        nl = -log_sigmoid(z.z0 - lse);
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

__global__ __launch_bounds__(256) void sampled_softmax_finish_kernel(const float *__restrict__ part, int64_t n_blocks, float wd,
                                                                     float batch_size, float *__restrict__ loss)
{
    bpr_finish_block(part, n_blocks, wd, batch_size, loss);
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
    float *__restrict__ dur = du + b * D, *__restrict__ dpr = dp + b * D, *__restrict__ dnr = dn + b * m * D;
    const float lq = lane_logq(logq, b, m, lane), c0 = pos_logq ? pos_logq[b] : 0.f;
    const URow<KU> ur(u + b * D, D, lane);
    const Scores sc = score_row<KU>(ur, pr, nr, m, D, lane);
    const Corrected z = correct(sc, inv_tau, c0, lq);
    const float M = fmaxf(z.z0, wave_max(lane < m ? z.zj : -INFINITY));
    const float e = lane < m ? expf(z.zj - M) : 0.f;
    const float den = expf(z.z0 - M) + wave_sum(e);
    const float s = -(e / den) * inv_tau;                                      // lane j: -a_j inv_tau = -dl_b/d(u.n_j)
    const float cp = wave_sum(s);                                              // -A inv_tau = dl_b/d(u.p)
    // du/g = 2 wd u + sum_j s_j (p - n_j) in the four chains of bpr_multi.hip: chain q takes the negatives j = q mod 4 in ascending
    // order, one fma each, chain 0 starts from the weight-decay term, and the chains combine as (c0 + c1) + (c2 + c3).
    if constexpr (KU > 0) {                 // second walk over the rows, R at a time; the lane's columns of du stay in registers
        float acc[4][KU], pb[KU];
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int col = lane + 64 * k;
            const float a = ur.v[k], bb = col < D ? pr[col] : 0.f;
            pb[k] = bb;
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
                    const float sj = lane_value(s, j), cn = -sj;
                    float *dnj = dnr + (int64_t)j * D;
#pragma unroll
                    for (int k = 0; k < KU; ++k) {
                        if (lane + 64 * k < D) dnj[lane + 64 * k] = g * fmaf(cn, ur.v[k], two_wd_m * c[r][k]);
                        acc[h + r][k] = fmaf(sj, pb[k] - c[r][k], acc[h + r][k]);
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < KU; ++k)
            if (lane + 64 * k < D) dur[lane + 64 * k] = g * ((acc[0][k] + acc[1][k]) + (acc[2][k] + acc[3][k]));
    } else {                                // D > 2048: column by column, the m rows below each
        for (int col = lane; col < D; col += 64) {
            const float a = ur.row[col], bb = pr[col];
            float acc[4] = {two_wd * a, 0.f, 0.f, 0.f};
            for (int j0 = 0; j0 < m; j0 += 4) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = j0 + q;
                    if (j >= m) break;
                    const float c = nr[(int64_t)j * D + col];
                    const float sj = lane_value(s, j);
                    dnr[(int64_t)j * D + col] = g * fmaf(-sj, a, two_wd_m * c);
                    acc[q] = fmaf(sj, bb - c, acc[q]);
                }
            }
            dur[col] = g * ((acc[0] + acc[1]) + (acc[2] + acc[3]));
            dpr[col] = g * fmaf(cp, a, two_wd * bb);
        }
    }
}

template <int KU>
int launch_forward(const float *u, const float *p, const float *n, const float *logq, const float *pos_logq, int64_t B, int m, int D,
                   float inv_tau, float *part, hipStream_t stream)
{
    sampled_softmax_rows_kernel<KU><<<dim3((unsigned)((B + 3) / 4)), 256, 0, stream>>>(u, p, n, logq, pos_logq, B, m, D, inv_tau, part);
    LAUNCH_CHECK();
    return NGCF_OK;
}

template <int KU>
int launch_backward(const float *u, const float *p, const float *n, const float *logq, const float *pos_logq, int64_t B, int m, int D,
                    float inv_tau, float wd, float batch_size, const float *gout, float *du, float *dp, float *dn, hipStream_t stream)
{
    sampled_softmax_backward_kernel<KU><<<dim3((unsigned)((B + 3) / 4)), 256, 0, stream>>>(u, p, n, logq, pos_logq, B, m, D, inv_tau,
                                                                                          wd, batch_size, gout, du, dp, dn);
    LAUNCH_CHECK();
    return NGCF_OK;
}

int check_shapes(const char *what, int64_t Bu, int64_t Bp, int64_t Bn, int m, int D, float inv_tau)
{
    if (D <= 0) return fail(NGCF_ERR_ARG, "%s: D=%d", what, D);
    if (m < 1 || m > NGCF_SAMPLED_SOFTMAX_M_MAX)
        return fail(NGCF_ERR_ARG, "%s: m=%d outside [1, %d]", what, m, NGCF_SAMPLED_SOFTMAX_M_MAX);
    if (Bu < 1 || Bu > ((int64_t)1 << 32) || Bp != Bu || Bn != Bu * m)
        return fail(NGCF_ERR_ARG, "%s: row counts %lld/%lld/%lld are not B/B/B*m with m=%d (no operand broadcasts)", what, (long long)Bu,
                    (long long)Bp, (long long)Bn, m);
    if (!(inv_tau > 0.f) || !(inv_tau < INFINITY))
        return fail(NGCF_ERR_ARG, "%s: inv_tau=%g is not a positive finite number", what, (double)inv_tau);
    return NGCF_OK;
}

}  // namespace

extern "C" int64_t ngcf_sampled_softmax_workspace_bytes(int64_t B)
{
    if (B < 0) return -1;
    return align_up(((B + 3) / 4) * 2 * (int64_t)sizeof(float), 256) + 256;
}

static int forward_kernel(const float *u, const float *p, const float *n, const float *logq, const float *pos_logq, int64_t B, int m,
                          int D, float inv_tau, float *part, hipStream_t stream)
{
    LOSS_ROWS_DISPATCH(launch_forward, u, p, n, logq, pos_logq, B, m, D, inv_tau, part, stream)
}

static int backward_kernel(const float *u, const float *p, const float *n, const float *logq, const float *pos_logq, int64_t B, int m,
                           int D, float inv_tau, float wd, float batch_size, const float *gout, float *du, float *dp, float *dn,
                           hipStream_t stream)
{
    LOSS_ROWS_DISPATCH(launch_backward, u, p, n, logq, pos_logq, B, m, D, inv_tau, wd, batch_size, gout, du, dp, dn, stream)
}

extern "C" int ngcf_sampled_softmax_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn, int m, int D,
                                        const float *logq, const float *pos_logq, float inv_tau, float wd, float batch_size,
                                        float *loss, void *workspace, int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!u || !p || !n || !logq || !loss) return fail(NGCF_ERR_ARG, "sampled_softmax: null argument");
    if (const int rc = check_shapes("sampled_softmax", Bu, Bp, Bn, m, D, inv_tau)) return rc;
    const int64_t need = ngcf_sampled_softmax_workspace_bytes(Bu);
    if (!workspace || workspace_bytes < need)
        return fail(NGCF_ERR_WORKSPACE, "sampled_softmax: workspace %lld B < %lld B", (long long)workspace_bytes, (long long)need);
    float *part = reinterpret_cast<float *>(align_up((int64_t)(uintptr_t)workspace, 256));
    if (const int rc = forward_kernel(u, p, n, logq, pos_logq, Bu, m, D, inv_tau, part, stream)) return rc;
    sampled_softmax_finish_kernel<<<1, 256, 0, stream>>>(part, (Bu + 3) / 4, wd, batch_size, loss);
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_sampled_softmax_backward_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn,
                                                 int m, int D, const float *logq, const float *pos_logq, float inv_tau, float wd,
                                                 float batch_size, const float *grad_out, float *du, float *dp, float *dn,
                                                 void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!u || !p || !n || !logq || !grad_out || !du || !dp || !dn) return fail(NGCF_ERR_ARG, "sampled_softmax_backward: null argument");
    if (const int rc = check_shapes("sampled_softmax_backward", Bu, Bp, Bn, m, D, inv_tau)) return rc;
    return backward_kernel(u, p, n, logq, pos_logq, Bu, m, D, inv_tau, wd, batch_size, grad_out, du, dp, dn, stream);
}
