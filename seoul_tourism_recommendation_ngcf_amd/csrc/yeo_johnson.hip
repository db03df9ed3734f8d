// Yeo-Johnson power transform, the numeric core of sklearn's PowerTransformer() that the reference's Preprocess.scale_implicit runs
// with args.scaler == 'power' (utils.py:107-112): the elementwise transform psi(x, lambda), and the fused pass of one
// evaluation of the likelihood that fits lambda - count, mean and centred sum of squares of psi over the non-NaN rows, and the
// lambda-free term sum sign(x) log1p|x|.  All arithmetic is fp64 and every operation of psi rounds once, as numpy's does.
#include "common.h"

// ---------------------------------------------------------------------------------------------
// The moments of one evaluation are a reduction over the whole column.  Each thread walks a grid-stride slice with Welford's
// running (n, mean, M2); partials are merged with Chan's formula in a FIXED tree: lane i takes lane i + s for s = 32 .. 1, wave w
// takes wave w + s for s = 2, 1, and the workgroup's partial goes to the workspace.  A second launch of one workgroup reads the
// partials (thread t takes t, t + 256, ... in ascending order) and merges them through the same tree.  No floating-point atomics;
// the grid is a function of T alone, so the four doubles are bit-identical from run to run.
// ---------------------------------------------------------------------------------------------
#define NGCF_YJ_THREADS 256
#define NGCF_YJ_MAX_BLOCKS 1024

namespace {

constexpr double kYjEps = 2.220446049250313e-16;       // 2^-52, numpy's spacing(1.0)

// sklearn 1.7's _yeo_johnson_transform, operation for operation; no contraction into an FMA (numpy has none)
__device__ inline double yeo_johnson_psi(double x, double lambda)
{
#pragma clang fp contract(off)
    if (x != x) return x;
    if (x >= 0.0) {                                     // -0.0 too
        if (fabs(lambda) < kYjEps) return log1p(x);
        const double b = x + 1.0;
        const double p = pow(b, lambda);
        const double m = p - 1.0;
        return m / lambda;
    }
    const double l2 = lambda - 2.0;
    if (!(fabs(l2) > kYjEps)) return -log1p(-x);
    const double e = 2.0 - lambda;
    const double b = -x + 1.0;
    const double p = pow(b, e);
    const double m = p - 1.0;
    return -m / e;
}

struct YjMoments {
    double n, mean, m2, c;                              // counts are integers below 2^53: exact in a double
};

// Chan, Golub & LeVeque: the moments of the union of two disjoint sets.  An empty side leaves the other as it is.
__device__ inline YjMoments yj_merge(const YjMoments &a, const YjMoments &b)
{
    if (b.n == 0.0) return YjMoments{a.n, a.mean, a.m2, a.c + b.c};
    if (a.n == 0.0) return YjMoments{b.n, b.mean, b.m2, a.c + b.c};
    const double n = a.n + b.n, delta = b.mean - a.mean, w = b.n / n;
    return YjMoments{n, a.mean + delta * w, a.m2 + b.m2 + delta * delta * a.n * w, a.c + b.c};
}

__device__ inline YjMoments yj_shfl_down(const YjMoments &v, int s)
{
    return YjMoments{__shfl_down(v.n, s), __shfl_down(v.mean, s), __shfl_down(v.m2, s), __shfl_down(v.c, s)};
}

// the workgroup's merged moments, valid in thread 0
__device__ inline YjMoments yj_block_merge(YjMoments v)
{
    __shared__ YjMoments s_wave[NGCF_YJ_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const YjMoments o = yj_shfl_down(v, s);
        if (lane < s) v = yj_merge(v, o);
    }
    if (lane == 0) s_wave[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int s = NGCF_YJ_THREADS / 128; s >= 1; s >>= 1)
            for (int w = 0; w < s; ++w) s_wave[w] = yj_merge(s_wave[w], s_wave[w + s]);
        v = s_wave[0];
    }
    return v;
}

__global__ __launch_bounds__(NGCF_YJ_THREADS) void yeo_johnson_kernel(const double *x, int64_t T, double lambda, double *out)
{
    for (int64_t t = (int64_t)blockIdx.x * NGCF_YJ_THREADS + threadIdx.x; t < T; t += (int64_t)gridDim.x * NGCF_YJ_THREADS)
        out[t] = yeo_johnson_psi(x[t], lambda);
}

__global__ __launch_bounds__(NGCF_YJ_THREADS) void yeo_johnson_moments_kernel(const double *__restrict__ x, int64_t T, double lambda,
                                                                              YjMoments *__restrict__ partial)
{
    YjMoments v{0.0, 0.0, 0.0, 0.0};
    for (int64_t t = (int64_t)blockIdx.x * NGCF_YJ_THREADS + threadIdx.x; t < T; t += (int64_t)gridDim.x * NGCF_YJ_THREADS) {
        const double xt = x[t];
        if (xt != xt) continue;                         // sklearn drops NaNs before the fit
        const double y = yeo_johnson_psi(xt, lambda);
        v.n += 1.0;
        const double d = y - v.mean;
        v.mean += d / v.n;
        v.m2 += d * (y - v.mean);
        v.c += copysign(log1p(fabs(xt)), xt);
    }
    v = yj_block_merge(v);
    if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

__global__ __launch_bounds__(NGCF_YJ_THREADS) void yeo_johnson_moments_final_kernel(const YjMoments *__restrict__ partial, int n_partial,
                                                                                    double *__restrict__ result)
{
    YjMoments v{0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n_partial; i += NGCF_YJ_THREADS) v = yj_merge(v, partial[i]);
    v = yj_block_merge(v);
    if (threadIdx.x == 0) {
        result[0] = v.n;
        result[1] = v.mean;
        result[2] = v.m2;
        result[3] = v.c;
    }
}

inline int yj_blocks(int64_t T)
{
    return (int)std::min<int64_t>((T + NGCF_YJ_THREADS - 1) / NGCF_YJ_THREADS, NGCF_YJ_MAX_BLOCKS);
}

}  // namespace

extern "C" int ngcf_yeo_johnson_f64(const double *x, int64_t T, double lambda, double *out, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (T < 0) return fail(NGCF_ERR_ARG, "yeo_johnson: negative count (T=%lld)", (long long)T);
    if (lambda != lambda) return fail(NGCF_ERR_ARG, "yeo_johnson: lambda is NaN");
    if (T == 0) return NGCF_OK;
    if (!x || !out) return fail(NGCF_ERR_ARG, "yeo_johnson: null argument");
    yeo_johnson_kernel<<<dim3((unsigned)grid_for(T, NGCF_YJ_THREADS)), NGCF_YJ_THREADS, 0, stream>>>(x, T, lambda, out);
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_yeo_johnson_moments_launch(int64_t T, int *blocks, int *threads, int *max_blocks)
{
    if (T < 0) return fail(NGCF_ERR_ARG, "yeo_johnson_moments: negative count (T=%lld)", (long long)T);
    if (blocks) *blocks = yj_blocks(T);
    if (threads) *threads = NGCF_YJ_THREADS;
    if (max_blocks) *max_blocks = NGCF_YJ_MAX_BLOCKS;
    return NGCF_OK;
}

extern "C" int64_t ngcf_yeo_johnson_workspace_bytes(int64_t T)
{
    return T < 0 ? -1 : (int64_t)yj_blocks(T) * (int64_t)sizeof(YjMoments);
}

extern "C" int ngcf_yeo_johnson_moments_f64(const double *x, int64_t T, double lambda, double *result, void *workspace,
                                            int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (T < 0) return fail(NGCF_ERR_ARG, "yeo_johnson_moments: negative count (T=%lld)", (long long)T);
    if (lambda != lambda) return fail(NGCF_ERR_ARG, "yeo_johnson_moments: lambda is NaN");
    if (!result || (T > 0 && (!x || !workspace))) return fail(NGCF_ERR_ARG, "yeo_johnson_moments: null argument");
    const int64_t need = ngcf_yeo_johnson_workspace_bytes(T);
    if (workspace_bytes < need)
        return fail(NGCF_ERR_WORKSPACE, "yeo_johnson_moments: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                    (long long)need);
    if (T > 0 && (reinterpret_cast<uintptr_t>(workspace) & 7))
        return fail(NGCF_ERR_ARG, "yeo_johnson_moments: workspace is not 8-byte aligned");
    const int blocks = yj_blocks(T);
    YjMoments *partial = static_cast<YjMoments *>(workspace);
    if (blocks) {
        yeo_johnson_moments_kernel<<<dim3((unsigned)blocks), NGCF_YJ_THREADS, 0, stream>>>(x, T, lambda, partial);
        LAUNCH_CHECK();
    }
    yeo_johnson_moments_final_kernel<<<dim3(1), NGCF_YJ_THREADS, 0, stream>>>(partial, blocks, result);    // T == 0: n = 0
    LAUNCH_CHECK();
    return NGCF_OK;
}
