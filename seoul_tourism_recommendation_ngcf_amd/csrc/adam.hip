// The optimizer step of the reference's training loop (experiment.py:58, `optimizer.step()` of the torch.optim.Adam that main.py:74
// builds): one launch updates p, m, v of up to 32 tensors and advances their step counters.  The recipe - every operation, its
// precision and its order - is in include/ngcf_hip.h (section "Adam step"); tests/adam_oracle.py restates it on the host and the
// kernel is pinned to that bit for bit.
#include "common.h"

// The lab's switch (tools/adam_lab.py builds this file alone, once per value): ONE operation of the per-element update contracted into
// a fused multiply-add, to measure which choice lies closest to torch's own kernels.  0 is the recipe of the header, and what the
// library is built with.
#ifndef NGCF_ADAM_VARIANT
#define NGCF_ADAM_VARIANT 0
#endif

namespace {

constexpr int kAdamTensors = NGCF_ADAM_MAX_TENSORS;     // tensors of one launch
constexpr int kAdamChunk = 4096;                       // elements of one workgroup
constexpr int kAdamBlock = 256;

struct AdamTensor {
    float *p;
    const float *g;
    float *m, *v;
    float *step;        // 0-dim float32: the steps taken so far
    int64_t n;
};

// The whole launch, by value in the kernel arguments: nothing is uploaded per step, and a captured launch carries it along.
struct AdamArgs {
    AdamTensor t[kAdamTensors];
    uint32_t chunk_begin[kAdamTensors + 1];     // tensor i owns the workgroups [chunk_begin[i], chunk_begin[i + 1])
    int n_tensors;
    int maximize;
    double lr, beta1, beta2, eps, wd;
    uint32_t *ticket;
};

struct AdamScalars {      // each rounded to fp32 once
    float step_size, bc2s, c1, beta2, c2, eps, wd;
    int maximize;
};

// beta^t in double-double, square-and-multiply on the integer t (the header spells the loop out).  A product's rounding error is
// recovered with Veltkamp's split, in IEEE operations only: nothing here may be contracted or re-associated.
struct AdamDD {
    double hi, lo;
};

__device__ inline AdamDD adam_dd_mul(AdamDD a, AdamDD b)
{
#pragma clang fp reassociate(off) contract(off)
    const double split = 134217729.0;       // 2^27 + 1
    const double p = a.hi * b.hi;
    double c = split * a.hi;
    const double ah = c - (c - a.hi), al = a.hi - ah;
    c = split * b.hi;
    const double bh = c - (c - b.hi), bl = b.hi - bh;
    double e = ((ah * bh - p) + ah * bl + al * bh) + al * bl;
    e = e + (a.hi * b.lo + a.lo * b.hi);
    AdamDD r;
    r.hi = p + e;
    r.lo = e - (r.hi - p);
    return r;
}

// beta1^t and beta2^t; one loop for both, so that the two dependent chains overlap (each is the header's loop, operation for operation)
__device__ inline void adam_pow2(double beta1, double beta2, int64_t t, double &pow1, double &pow2)
{
    AdamDD r1 = {1.0, 0.0}, b1 = {beta1, 0.0}, r2 = {1.0, 0.0}, b2 = {beta2, 0.0};
    for (int64_t e = t; e > 0;) {
        if (e & 1) {
            r1 = adam_dd_mul(r1, b1);
            r2 = adam_dd_mul(r2, b2);
        }
        e >>= 1;
        if (e > 0) {
            b1 = adam_dd_mul(b1, b1);
            b2 = adam_dd_mul(b2, b2);
        }
    }
    pow1 = r1.hi;
    pow2 = r2.hi;
}

// One element.  Both the 16-byte path and the scalar path go through this function, so they give the same bits.
__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, const AdamScalars &s)
{
#pragma clang fp reassociate(off) contract(off)
    if (s.maximize) g = -g;
#if NGCF_ADAM_VARIANT == 1
    if (s.wd != 0.f) g = fmaf(s.wd, p, g);
#else
    if (s.wd != 0.f) g = g + s.wd * p;
#endif
#if NGCF_ADAM_VARIANT == 2
    m = fmaf(s.c1, g - m, m);
#else
    m = m + s.c1 * (g - m);
#endif
#if NGCF_ADAM_VARIANT == 3
    v = fmaf(v, s.beta2, (s.c2 * g) * g);
#elif NGCF_ADAM_VARIANT == 4
    v = fmaf(s.c2 * g, g, v * s.beta2);
#else
    v = v * s.beta2 + (s.c2 * g) * g;
#endif
    const float d = sqrtf(v) / s.bc2s + s.eps;
#if NGCF_ADAM_VARIANT == 5
    p = fmaf(s.step_size, m / d, p);
#else
    p = p + s.step_size * (m / d);
#endif
}

__device__ __forceinline__ void adam_element4(float4 &p, const float4 &g, float4 &m, float4 &v, const AdamScalars &s)
{
    adam_element(p.x, g.x, m.x, v.x, s);
    adam_element(p.y, g.y, m.y, v.y, s);
    adam_element(p.z, g.z, m.z, v.z, s);
    adam_element(p.w, g.w, m.w, v.w, s);
}

__global__ void __launch_bounds__(kAdamBlock) adam_step_kernel(const AdamArgs a)
{
    __shared__ float sh_scalars[2];
    const int tid = threadIdx.x;
    // the workgroup's tensor: chunk_begin holds at most 33 wave-uniform entries
    int ti = 0;
    for (int i = 1; i < a.n_tensors; ++i) ti += blockIdx.x >= a.chunk_begin[i] ? 1 : 0;
    ti = __builtin_amdgcn_readfirstlane(ti);
    const AdamTensor &T = a.t[ti];
    const float step = *T.step;                  // before anything else: the last workgroup of the launch rewrites it
    const int64_t off = (int64_t)(blockIdx.x - a.chunk_begin[ti]) * kAdamChunk;
    const int64_t left = T.n - off;
    const int n = left < kAdamChunk ? (int)left : kAdamChunk;       // elements of this chunk, >= 1
    float *__restrict__ p = T.p + off;
    const float *__restrict__ g = T.g + off;
    float *__restrict__ m = T.m + off;
    float *__restrict__ v = T.v + off;
    // the 16-byte path loads its chunk first: the loads are in flight while the scalars are worked out
    constexpr int kVec = kAdamChunk / 4 / kAdamBlock;
    const bool vec = (((uintptr_t)T.p | (uintptr_t)T.g | (uintptr_t)T.m | (uintptr_t)T.v) & 15) == 0;      // (off is a multiple of 4 096 elements)
    const int n4 = vec ? n >> 2 : 0;
    float4 *p4 = reinterpret_cast<float4 *>(p), *m4 = reinterpret_cast<float4 *>(m), *v4 = reinterpret_cast<float4 *>(v);
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    float4 pp[kVec], gg[kVec], mm[kVec], vv[kVec];
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
        const int i = k * kAdamBlock + tid;
        if (i < n4) {
            pp[k] = p4[i];
            gg[k] = g4[i];
            mm[k] = m4[i];
            vv[k] = v4[i];
        }
    }
    if (tid < 64) {                              // one wave works the scalars out in fp64
#pragma clang fp reassociate(off) contract(off)
        const int64_t t = (int64_t)(step + 1.0f);
        double pow1, pow2;
        adam_pow2(a.beta1, a.beta2, t, pow1, pow2);
        const double bc1 = 1.0 - pow1;
        const double step_size = -(a.lr / bc1);
        const double bc2s = sqrt(1.0 - pow2);
        if (tid == 0) {
            sh_scalars[0] = (float)step_size;
            sh_scalars[1] = (float)bc2s;
        }
    }
    __syncthreads();
    AdamScalars s;
    s.step_size = sh_scalars[0];
    s.bc2s = sh_scalars[1];
    s.c1 = (float)(1.0 - a.beta1);
    s.beta2 = (float)a.beta2;
    s.c2 = (float)(1.0 - a.beta2);
    s.eps = (float)a.eps;
    s.wd = (float)a.wd;
    s.maximize = a.maximize;
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
        const int i = k * kAdamBlock + tid;
        if (i < n4) {
            adam_element4(pp[k], gg[k], mm[k], vv[k], s);
            p4[i] = pp[k];
            m4[i] = mm[k];
            v4[i] = vv[k];
        }
    }
    const int done = n4 << 2;                                       // elements the 16-byte path took
    for (int i = done + tid; i < n; i += kAdamBlock) {              // the tail, or a chunk whose pointers are not aligned
        float pp = p[i], mm = m[i], vv = v[i];
        adam_element(pp, g[i], mm, vv, s);
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
    }

    // the step counters: every workgroup has read its own before it takes a ticket; the one that takes the last ticket advances them all
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        const uint32_t total = a.chunk_begin[a.n_tensors];
        if (atomicAdd(a.ticket, 1u) == total - 1) {
            __threadfence();
            for (int i = 0; i < a.n_tensors; ++i) *a.t[i].step = *a.t[i].step + 1.0f;
            atomicExch(a.ticket, 0u);
        }
    }
}

}  // namespace

extern "C" int ngcf_adam_step_f32(int n_tensors, void *const *params, const void *const *grads, void *const *exp_avgs,
                                  void *const *exp_avg_sqs, void *const *steps, const int64_t *numel, uint32_t *ticket, double lr,
                                  double beta1, double beta2, double eps, double weight_decay, int maximize, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_tensors < 0) return fail(NGCF_ERR_ARG, "adam_step: n_tensors=%d is negative", n_tensors);
    if (n_tensors == 0) return NGCF_OK;
    if (!params || !grads || !exp_avgs || !exp_avg_sqs || !steps || !numel || !ticket) return fail(NGCF_ERR_ARG, "adam_step: null argument");
    if ((reinterpret_cast<uintptr_t>(ticket) & 3) != 0) return fail(NGCF_ERR_ARG, "adam_step: the ticket word is not 4-byte aligned");
    for (int i = 0; i < n_tensors; ++i) {           // everything is checked before the first launch
        if (numel[i] < 0) return fail(NGCF_ERR_ARG, "adam_step: tensor %d has %lld elements", i, (long long)numel[i]);
        if (numel[i] == 0) continue;
        if (!params[i] || !grads[i] || !exp_avgs[i] || !exp_avg_sqs[i] || !steps[i])
            return fail(NGCF_ERR_ARG, "adam_step: tensor %d has a null pointer", i);
        const uintptr_t bits = reinterpret_cast<uintptr_t>(params[i]) | reinterpret_cast<uintptr_t>(grads[i]) |
                               reinterpret_cast<uintptr_t>(exp_avgs[i]) | reinterpret_cast<uintptr_t>(exp_avg_sqs[i]) |
                               reinterpret_cast<uintptr_t>(steps[i]);
        if (bits & 3) return fail(NGCF_ERR_ARG, "adam_step: tensor %d has a pointer that is not 4-byte aligned", i);
        if ((numel[i] + kAdamChunk - 1) / kAdamChunk > 0x7fffffffll / kAdamTensors)
            return fail(NGCF_ERR_ARG, "adam_step: tensor %d has %lld elements, too many for one launch", i, (long long)numel[i]);
    }
    AdamArgs a;
    memset(&a, 0, sizeof(a));
    a.maximize = maximize ? 1 : 0;
    a.lr = lr;
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.eps = eps;
    a.wd = weight_decay;
    a.ticket = ticket;
    int k = 0;
    for (int i = 0; i <= n_tensors; ++i) {
        if (i < n_tensors && numel[i] > 0) {
            a.t[k] = AdamTensor{(float *)params[i], (const float *)grads[i], (float *)exp_avgs[i], (float *)exp_avg_sqs[i], (float *)steps[i],
                                numel[i]};
            a.chunk_begin[k + 1] = a.chunk_begin[k] + (uint32_t)((numel[i] + kAdamChunk - 1) / kAdamChunk);
            ++k;
        }
        if (k == kAdamTensors || (i == n_tensors && k > 0)) {
            a.n_tensors = k;
            adam_step_kernel<<<a.chunk_begin[k], kAdamBlock, 0, stream>>>(a);
            LAUNCH_CHECK();
            k = 0;
        }
    }
    return NGCF_OK;
}
