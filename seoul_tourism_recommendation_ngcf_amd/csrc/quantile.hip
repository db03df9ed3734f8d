// Per-segment quantile floor, the numeric core of the reference's Preprocess.scale_implicit (utils.py:103-122) for every user in one
// call: z = ((x - mean) / scale) + shift, the segment's q4/4 quantile of z the way pandas / numpy (method="linear") compute it, and
// every z below it set to 0.  All arithmetic is fp64 and every operation rounds once, as numpy's does.
#include "common.h"

// ---------------------------------------------------------------------------------------------
// The quantile of n values is a blend of the two order statistics s[lo] and s[lo + 1].  z is non-decreasing in x, so both are
// SELECTED on the raw values and only they, and the values written, are transformed: z(s[lo]) is the lo-th smallest z.
//
// Wave tier (n <= wave_max <= 64): a wave per segment, a value per lane; every lane counts the values that sort before its own
// (ties broken by lane), which gives each a unique rank, and the lanes of rank lo and lo + 1 hold a and b.
//
// Workgroup tier (any n): 256 threads per segment, a radix select on the order-preserving 64-bit key of the value: 8 passes from
// the most significant byte, each a 256-bin histogram in LDS (integer atomics) of the values that match the prefix found so far;
// the bin that holds rank lo extends the prefix.  One more pass counts c = #{x <= a} and finds m = min{x > a}: b = a if c >= lo + 2,
// else m.  A segment of up to kQResident values keeps its keys and positions in LDS, so `order` and x are read once; a longer one
// is read again from memory in every pass.
//
// Both tiers read all of a segment before they write any of it (out may alias x), and both put -0.0 as +0.0, so they agree bit
// for bit.
// ---------------------------------------------------------------------------------------------
#define NGCF_QUANTILE_WAVES 4

namespace {

constexpr int kQResident = 2048;          // values of a segment held in LDS by the workgroup tier: 16 KiB of keys + 16 KiB of positions
constexpr uint64_t kQSign = 0x8000000000000000ull;

struct QTransform {
    double mean, scale, shift;
};

// Every operation of the transform and of the blend rounds once: no contraction into an FMA (numpy has none).
__device__ inline double quantile_z(double v, const QTransform &tr)
{
#pragma clang fp contract(off)
    const double c = v - tr.mean;
    const double s = c / tr.scale;
    return s + tr.shift;
}

// numpy's _lerp: a + (b - a) * t below t = 0.5, b - (b - a) * (1 - t) from there; r = (n - 1) * q4, t = (r % 4) / 4
__device__ inline double quantile_blend(double a, double b, int r4)
{
#pragma clang fp contract(off)
    const double t = (double)r4 * 0.25;
    const double d = b - a;
    if (r4 < 2) {
        const double dt = d * t;
        return a + dt;
    }
    const double u = 1.0 - t;
    const double du = d * u;
    return b - du;
}

__device__ inline double quantile_canon(double v) { return v == 0.0 ? 0.0 : v; }          // -0.0 -> +0.0; a NaN stays

// monotone map double -> uint64 (larger value = larger key) of a canonical non-NaN value, and back
__device__ inline uint64_t quantile_key(double v)
{
    const uint64_t u = (uint64_t)__double_as_longlong(quantile_canon(v));
    return (u & kQSign) ? ~u : (u | kQSign);
}
__device__ inline double quantile_unkey(uint64_t k)
{
    return __longlong_as_double((long long)((k & kQSign) ? (k & ~kQSign) : ~k));
}

__device__ inline double quantile_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

__device__ inline double readlane_f64(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// a segment's bounds; false: the row pointers decrease or leave [0, T]
__device__ inline bool quantile_segment(const int64_t *__restrict__ rowptr, int64_t u, int64_t T, int64_t &lo, int64_t &n)
{
    lo = rowptr[u];
    const int64_t hi = rowptr[u + 1];
    n = hi - lo;
    return lo >= 0 && hi >= lo && hi <= T;
}

__global__ __launch_bounds__(64 * NGCF_QUANTILE_WAVES) void segment_quantile_wave_kernel(
    const int64_t *__restrict__ rowptr, int64_t n_rows, const int64_t *__restrict__ order, const double *x, int64_t T, QTransform tr,
    int q4, int wmax, double *__restrict__ quant, double *out, int32_t *status)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t u = (int64_t)blockIdx.x * NGCF_QUANTILE_WAVES + wave; u < n_rows; u += (int64_t)gridDim.x * NGCF_QUANTILE_WAVES) {
        int64_t lo, n64;
        if (!quantile_segment(rowptr, u, T, lo, n64)) {                 // reported here, whatever its length
            if (lane == 0) {
                atomicOr(status, 1);
                quant[u] = quantile_nan();
            }
            continue;
        }
        if (n64 > wmax) continue;                                       // the workgroup tier's
        const int n = (int)n64;
        if (n == 0) {
            if (lane == 0) quant[u] = quantile_nan();
            continue;
        }
        const bool mine = lane < n;
        int64_t p = 0;
        if (mine) p = order ? order[lo + lane] : lo + lane;
        const bool inside = p >= 0 && p < T;
        if (__any(mine && !inside)) {
            if (lane == 0) {
                atomicOr(status, 1);
                quant[u] = quantile_nan();
            }
            continue;
        }
        const double xi = mine ? quantile_canon(x[p]) : 0.0;
        const double zi = quantile_z(xi, tr);
        if (__any(mine && xi != xi)) {                                  // a NaN: the segment passes through
            if (lane == 0) {
                atomicOr(status, 2);
                quant[u] = quantile_nan();
            }
            if (mine) out[p] = zi;
            continue;
        }
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double xj = readlane_f64(xi, j);
            rank += (xj < xi || (xj == xi && j < lane)) ? 1 : 0;
        }
        const int r = (n - 1) * q4, k = r >> 2;
        const uint64_t ma = __ballot(mine && rank == k), mb = __ballot(mine && rank == min(k + 1, n - 1));
        const double a = readlane_f64(zi, __ffsll((unsigned long long)ma) - 1), b = readlane_f64(zi, __ffsll((unsigned long long)mb) - 1);
        const double qv = quantile_blend(a, b, r & 3);
        if (lane == 0) quant[u] = qv;
        if (mine) out[p] = zi < qv ? 0.0 : zi;
    }
}

__device__ inline unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}
__device__ inline unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = __shfl_xor(v, s);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void segment_quantile_block_kernel(
    const int64_t *__restrict__ rowptr, int64_t n_rows, const int64_t *__restrict__ order, const double *x, int64_t T, QTransform tr,
    int q4, int wmax, double *__restrict__ quant, double *out, int32_t *status)
{
    __shared__ unsigned long long s_key[kQResident];
    __shared__ long long s_pos[kQResident];
    __shared__ unsigned long long s_hist[256];
    __shared__ unsigned long long s_k, s_cnt, s_min;
    __shared__ int s_bin, s_flags;
    const int tid = threadIdx.x, lane = tid & 63;

    for (int64_t u = blockIdx.x; u < n_rows; u += gridDim.x) {
        int64_t lo, n;
        if (!quantile_segment(rowptr, u, T, lo, n) || n <= wmax) continue;        // the wave tier's (it reports bad row pointers)
        const bool resident = n <= kQResident;
        if (tid == 0) {
            s_flags = 0;
            s_cnt = 0;
            s_min = ~0ull;
        }
        s_hist[tid] = 0;
        __syncthreads();

        // pass 0: every position checked before it is read through, NaNs found, the histogram of the top byte
        int flags = 0;
        for (int64_t i = tid; i < n; i += 256) {
            const int64_t p = order ? order[lo + i] : lo + i;
            if (p < 0 || p >= T) {
                flags |= 1;
                continue;
            }
            const double v = x[p];
            if (v != v) {
                flags |= 2;
                continue;
            }
            const unsigned long long key = quantile_key(v);
            if (resident) {
                s_key[i] = key;
                s_pos[i] = p;
            }
            atomicAdd(&s_hist[key >> 56], 1ull);
        }
        if (flags) atomicOr(&s_flags, flags);
        __syncthreads();
        flags = s_flags;
        if (flags) {
            if (tid == 0) {
                atomicOr(status, (flags & 1) ? 1 : 2);
                quant[u] = quantile_nan();
            }
            if (!(flags & 1))                                            // a NaN: the segment passes through
                for (int64_t i = tid; i < n; i += 256) {
                    const int64_t p = order ? order[lo + i] : lo + i;
                    out[p] = quantile_z(quantile_canon(x[p]), tr);
                }
            __syncthreads();
            continue;
        }

        const int64_t r = (n - 1) * q4, rank_a = r >> 2;
        unsigned long long prefix = 0, k = (unsigned long long)rank_a;
        for (int byte = 7; byte >= 0; --byte) {
            const int sh = 8 * byte;
            if (byte < 7) {
                for (int64_t i = tid; i < n; i += 256) {
                    const unsigned long long key = resident ? s_key[i] : quantile_key(x[order ? order[lo + i] : lo + i]);
                    if (((key ^ prefix) >> sh >> 8) == 0) atomicAdd(&s_hist[(key >> sh) & 255], 1ull);
                }
                __syncthreads();
            }
            if (tid < 64) {                                              // the bin that holds rank k: 4 bins per lane of one wave
                unsigned long long h[4], s = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) s += h[q] = s_hist[4 * lane + q];
                unsigned long long inc = s;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned long long o = __shfl_up(inc, d);
                    if (lane >= d) inc += o;
                }
                unsigned long long kk = k - (inc - s);                   // wraps below the lane's first bin: then kk >= s too
                if (inc - s <= k && k < inc) {
                    int bin = 4 * lane;
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        if (bin == 4 * lane + q && kk >= h[q]) {
                            kk -= h[q];
                            ++bin;
                        }
                    s_bin = bin;
                    s_k = kk;
                }
            }
            __syncthreads();
            prefix |= (unsigned long long)s_bin << sh;
            k = s_k;
            s_hist[tid] = 0;
            __syncthreads();
        }

        // a = the value of key `prefix`; c = #{x <= a}, m = min{x > a}
        unsigned long long c = 0, m = ~0ull;
        for (int64_t i = tid; i < n; i += 256) {
            const unsigned long long key = resident ? s_key[i] : quantile_key(x[order ? order[lo + i] : lo + i]);
            if (key <= prefix) ++c;
            else m = key < m ? key : m;
        }
        c = wave_sum_u64(c);
        m = wave_min_u64(m);
        if (lane == 0) {
            atomicAdd(&s_cnt, c);
            atomicMin(&s_min, m);
        }
        __syncthreads();
        const unsigned long long key_b = (s_cnt >= (unsigned long long)rank_a + 2 || rank_a + 1 >= n) ? prefix : s_min;
        const double qv = quantile_blend(quantile_z(quantile_unkey(prefix), tr), quantile_z(quantile_unkey(key_b), tr), (int)(r & 3));
        if (tid == 0) quant[u] = qv;
        for (int64_t i = tid; i < n; i += 256) {
            const int64_t p = resident ? (int64_t)s_pos[i] : (order ? order[lo + i] : lo + i);
            const double zi = quantile_z(resident ? quantile_unkey(s_key[i]) : quantile_canon(x[p]), tr);
            out[p] = zi < qv ? 0.0 : zi;
        }
        __syncthreads();                                                 // the next segment overwrites the shared state
    }
}

}  // namespace

extern "C" int ngcf_segment_quantile_floor_f64(const int64_t *rowptr, int64_t n_rows, const int64_t *order, const double *x, int64_t T,
                                               double mean, double scale, double shift, int q4, int wave_max, double *quant,
                                               double *out, int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (q4 < 1 || q4 > 3) return fail(NGCF_ERR_ARG, "segment_quantile_floor: q4=%d outside [1, 3]", q4);
    if (wave_max < 0 || wave_max > 64) return fail(NGCF_ERR_ARG, "segment_quantile_floor: wave_max=%d outside [0, 64]", wave_max);
    if (!(scale > 0.0) || scale > 1.7976931348623157e308)
        return fail(NGCF_ERR_ARG, "segment_quantile_floor: scale=%g is not a finite positive number", scale);
    if (T < 0 || n_rows < 0)
        return fail(NGCF_ERR_ARG, "segment_quantile_floor: negative count (n_rows=%lld, T=%lld)", (long long)n_rows, (long long)T);
    if (T == 0 || n_rows == 0) return NGCF_OK;
    if (!rowptr || !x || !quant || !out || !status) return fail(NGCF_ERR_ARG, "segment_quantile_floor: null argument");

    const QTransform tr{mean, scale, shift};
    const int wmax = wave_max ? wave_max : 64;
    const int64_t wave_blocks = std::min<int64_t>((n_rows + NGCF_QUANTILE_WAVES - 1) / NGCF_QUANTILE_WAVES, 256 * 16);
    segment_quantile_wave_kernel<<<dim3((unsigned)wave_blocks), 64 * NGCF_QUANTILE_WAVES, 0, stream>>>(
        rowptr, n_rows, order, x, T, tr, q4, wmax, quant, out, status);
    LAUNCH_CHECK();
    if (T > wmax) {                                                      // else no segment can be longer than the wave tier's limit
        const int64_t blocks = std::min<int64_t>(n_rows, 256 * 8);
        segment_quantile_block_kernel<<<dim3((unsigned)blocks), 256, 0, stream>>>(rowptr, n_rows, order, x, T, tr, q4, wmax, quant,
                                                                                  out, status);
        LAUNCH_CHECK();
    }
    return NGCF_OK;
}
