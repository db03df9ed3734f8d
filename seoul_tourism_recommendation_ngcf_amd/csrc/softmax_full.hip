// softmax_full.hip - the softmax loss over the WHOLE catalogue, loss and both gradients, without the [B, n_items] score matrix
// (include/ngcf_hip.h, "Full-catalogue softmax").  The kernels, the plan and the launches are those of
// softmax_tile_device.h with INBATCH = false (the in-batch loss of inbatch_softmax.hip is the other instance): this file is the
// entry points and their argument checks.
#include "softmax_tile_device.h"

namespace {

SoftmaxSides full_sides(const float *users, int64_t ldu, int64_t B, const float *items, int64_t ldi, int64_t n_items, int D,
                        const int64_t *pos)
{
    SoftmaxSides a = {};
    a.users = users, a.ldu = ldu, a.B = B;
    a.items = items, a.ldi = ldi, a.n_items = n_items, a.n_first = n_items;
    a.D = D, a.pos = pos;
    return a;
}

bool shape_ok(int64_t B, int64_t n_items, int D)
{
    return B >= 1 && n_items >= 1 && D >= 1 && B < ((int64_t)1 << 31) && n_items < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int ngcf_softmax_full_plan(int64_t B, int64_t n_items, int D, int64_t out[6])
{
    if (!out) return fail(NGCF_ERR_ARG, "softmax_full_plan: null argument");
    if (!shape_ok(B, n_items, D))
        return fail(NGCF_ERR_ARG, "softmax_full_plan: B=%lld, n_items=%lld, D=%d", (long long)B, (long long)n_items, D);
    softmax_plan_out(softmax_plan(B, n_items, D), out);
    return NGCF_OK;
}

extern "C" int64_t ngcf_softmax_full_workspace_bytes(int64_t B, int64_t n_items, int D)
{
    if (!shape_ok(B, n_items, D)) return -1;
    return softmax_scratch(softmax_plan(B, n_items, D), B, n_items, D).total;
}

static int softmax_full_check(const char *who, int64_t ldu, int64_t B, int64_t ldi, int64_t n_items, int D, float inv_tau,
                              float batch_size)
{
    if (!shape_ok(B, n_items, D))
        return fail(NGCF_ERR_ARG, "%s: B=%lld, n_items=%lld, D=%d", who, (long long)B, (long long)n_items, D);
    if (ldu < D || ldi < D) return fail(NGCF_ERR_ARG, "%s: leading dimensions %lld/%lld below D=%d", who, (long long)ldu, (long long)ldi, D);
    if (!(inv_tau > 0.f) || !(inv_tau < INFINITY)) return fail(NGCF_ERR_ARG, "%s: inv_tau=%g is not a positive finite number", who, inv_tau);
    if (!(batch_size > 0.f)) return fail(NGCF_ERR_ARG, "%s: batch_size=%g", who, batch_size);
    return NGCF_OK;
}

extern "C" int ngcf_softmax_full_f32(const float *users, int64_t ldu, int64_t B, const float *items, int64_t ldi, int64_t n_items, int D,
                                     const int64_t *pos, float inv_tau, float wd, float batch_size, float *loss, float *lse,
                                     float *spos, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream_)
{
    if (!users || !items || !pos || !loss || !lse || !spos || !status) return fail(NGCF_ERR_ARG, "softmax_full: null argument");
    if (const int rc = softmax_full_check("softmax_full", ldu, B, ldi, n_items, D, inv_tau, batch_size)) return rc;
    return softmax_launch_forward<false>("softmax_full", full_sides(users, ldu, B, items, ldi, n_items, D, pos), inv_tau, wd, batch_size,
                                         loss, lse, spos, status, workspace, workspace_bytes, (hipStream_t)stream_);
}

extern "C" int ngcf_softmax_full_backward_f32(const float *users, int64_t ldu, int64_t B, const float *items, int64_t ldi,
                                              int64_t n_items, int D, const int64_t *pos, const float *lse, float inv_tau, float wd,
                                              float batch_size, const float *grad_out, float *du, int64_t lddu, float *ditems,
                                              int64_t lddi, void *workspace, int64_t workspace_bytes, void *stream_)
{
    if (!users || !items || !pos || !lse || !grad_out || (!du && !ditems)) return fail(NGCF_ERR_ARG, "softmax_full_backward: null argument");
    if (const int rc = softmax_full_check("softmax_full_backward", ldu, B, ldi, n_items, D, inv_tau, batch_size)) return rc;
    if ((du && lddu < D) || (ditems && lddi < D))
        return fail(NGCF_ERR_ARG, "softmax_full_backward: leading dimensions %lld/%lld below D=%d", (long long)lddu, (long long)lddi, D);
    return softmax_launch_backward<false>("softmax_full_backward", full_sides(users, ldu, B, items, ldi, n_items, D, pos), lse, inv_tau, wd,
                                          batch_size, grad_out, du, lddu, ditems, lddi, nullptr, 0, workspace, workspace_bytes,
                                          (hipStream_t)stream_);
}
