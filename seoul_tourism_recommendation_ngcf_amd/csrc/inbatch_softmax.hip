// inbatch_softmax.hip - the softmax loss with SHARED (in-batch) negatives: every row's positive is a negative of every other row,
// E extra rows are appended to the columns, with the logQ correction per column and the mask of false negatives; loss and the three
// gradients without the [B, B + E] score matrix (include/ngcf_hip.h, "In-batch softmax").  The kernels, the plan and
// the launches are those of softmax_tile_device.h with INBATCH = true (softmax_full.hip is the other instance): this file is the
// entry points and their argument checks.
#include "softmax_tile_device.h"

namespace {

bool inbatch_shape_ok(int64_t B, int64_t E, int D)
{
    return B >= 1 && E >= 0 && D >= 1 && B < ((int64_t)1 << 31) && E < ((int64_t)1 << 31) && B + E < ((int64_t)1 << 31);
}

// the forward's z_bb, kept between its kernels: one more block after the shared layout
int64_t inbatch_total(const SoftmaxScratch &sc, int64_t B)
{
    return sc.total + align_up(B * 4, 256);
}

int inbatch_check(const char *who, const float *u, int64_t ldu, int64_t B, const float *p, int64_t ldp, const float *x, int64_t ldx,
                  int64_t E, int D, const int64_t *ids, const int64_t *xids, float inv_tau, float batch_size)
{
    if (!inbatch_shape_ok(B, E, D)) return fail(NGCF_ERR_ARG, "%s: B=%lld, E=%lld, D=%d", who, (long long)B, (long long)E, D);
    if (!u || !p || (E > 0 && !x)) return fail(NGCF_ERR_ARG, "%s: null argument", who);
    if (ldu < D || ldp < D || (E > 0 && ldx < D))
        return fail(NGCF_ERR_ARG, "%s: leading dimensions %lld/%lld/%lld below D=%d", who, (long long)ldu, (long long)ldp, (long long)ldx, D);
    if (!(inv_tau > 0.f) || !(inv_tau < INFINITY)) return fail(NGCF_ERR_ARG, "%s: inv_tau=%g is not a positive finite number", who, inv_tau);
    if (!(batch_size > 0.f)) return fail(NGCF_ERR_ARG, "%s: batch_size=%g", who, batch_size);
    if (ids && E > 0 && !xids) return fail(NGCF_ERR_ARG, "%s: ids given, E=%lld extra rows and no xids", who, (long long)E);
    return NGCF_OK;
}

SoftmaxSides inbatch_sides(const float *u, int64_t ldu, int64_t B, const float *p, int64_t ldp, const float *x, int64_t ldx, int64_t E,
                           int D, const int64_t *ids, const int64_t *xids, const float *logq, const float *xlogq, const float *pos_logq)
{
    SoftmaxSides a = {};
    a.users = u, a.ldu = ldu, a.B = B;
    a.items = p, a.ldi = ldp, a.n_items = B + E, a.n_first = B;
    a.extra = x, a.ldx = ldx;
    a.D = D;
    a.ids = ids, a.xids = xids, a.logq = logq, a.xlogq = xlogq, a.pos_logq = pos_logq;
    return a;
}

}  // namespace

extern "C" int ngcf_inbatch_softmax_plan(int64_t B, int64_t E, int D, int64_t out[6])
{
    if (!out) return fail(NGCF_ERR_ARG, "inbatch_softmax_plan: null argument");
    if (!inbatch_shape_ok(B, E, D)) return fail(NGCF_ERR_ARG, "inbatch_softmax_plan: B=%lld, E=%lld, D=%d", (long long)B, (long long)E, D);
    softmax_plan_out(softmax_plan(B, B + E, D), out);
    return NGCF_OK;
}

extern "C" int64_t ngcf_inbatch_softmax_workspace_bytes(int64_t B, int64_t E, int D)
{
    if (!inbatch_shape_ok(B, E, D)) return -1;
    return inbatch_total(softmax_scratch(softmax_plan(B, B + E, D), B, B + E, D), B);
}

extern "C" int ngcf_inbatch_softmax_f32(const float *u, int64_t ldu, int64_t B, const float *p, int64_t ldp, const float *x, int64_t ldx,
                                        int64_t E, int D, const int64_t *ids, const int64_t *xids, const float *logq,
                                        const float *xlogq, const float *pos_logq, float inv_tau, float wd, float batch_size,
                                        float *loss, float *lse, void *workspace, int64_t workspace_bytes, void *stream_)
{
    if (const int rc = inbatch_check("inbatch_softmax", u, ldu, B, p, ldp, x, ldx, E, D, ids, xids, inv_tau, batch_size)) return rc;
    if (!loss || !lse) return fail(NGCF_ERR_ARG, "inbatch_softmax: null argument");
    const SoftmaxScratch sc = softmax_scratch(softmax_plan(B, B + E, D), B, B + E, D);
    if (!workspace || workspace_bytes < inbatch_total(sc, B))
        return fail(NGCF_ERR_WORKSPACE, "inbatch_softmax: workspace %lld B < %lld B", (long long)workspace_bytes,
                    (long long)inbatch_total(sc, B));
    char *base = reinterpret_cast<char *>(align_up((int64_t)(uintptr_t)workspace, 256)) - 256;
    float *zpos = reinterpret_cast<float *>(base + sc.total);
    return softmax_launch_forward<true>("inbatch_softmax", inbatch_sides(u, ldu, B, p, ldp, x, ldx, E, D, ids, xids, logq, xlogq, pos_logq),
                                        inv_tau, wd, batch_size, loss, lse, zpos, nullptr, workspace, workspace_bytes,
                                        (hipStream_t)stream_);
}

extern "C" int ngcf_inbatch_softmax_backward_f32(const float *u, int64_t ldu, int64_t B, const float *p, int64_t ldp, const float *x,
                                                 int64_t ldx, int64_t E, int D, const int64_t *ids, const int64_t *xids,
                                                 const float *logq, const float *xlogq, const float *pos_logq, const float *lse,
                                                 float inv_tau, float wd, float batch_size, const float *grad_out, float *du,
                                                 int64_t lddu, float *dp, int64_t lddp, float *dx, int64_t lddx, void *workspace,
                                                 int64_t workspace_bytes, void *stream_)
{
    if (const int rc = inbatch_check("inbatch_softmax_backward", u, ldu, B, p, ldp, x, ldx, E, D, ids, xids, inv_tau, batch_size)) return rc;
    if (E == 0) dx = nullptr;
    if (!lse || !grad_out || (!du && !dp && !dx)) return fail(NGCF_ERR_ARG, "inbatch_softmax_backward: null argument");
    if ((du && lddu < D) || (dp && lddp < D) || (dx && lddx < D))
        return fail(NGCF_ERR_ARG, "inbatch_softmax_backward: leading dimensions %lld/%lld/%lld below D=%d", (long long)lddu, (long long)lddp,
                    (long long)lddx, D);
    return softmax_launch_backward<true>("inbatch_softmax_backward",
                                         inbatch_sides(u, ldu, B, p, ldp, x, ldx, E, D, ids, xids, logq, xlogq, pos_logq), lse, inv_tau, wd,
                                         batch_size, grad_out, du, lddu, dp, lddp, dx, lddx, workspace, workspace_bytes,
                                         (hipStream_t)stream_);
}
