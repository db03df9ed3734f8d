// Trip context of a recommendation request, what the reference's demo.py builds in pandas before its blend: the float group sum of
// the congestion pivot (demo.py:99-102, pandas' compensated group_sum bit for bit) and the table of great-circle distances between
// departure points and destinations (demo.py:241-248, the `haversine` package's formula operation for operation).  All fp64.
#include "common.h"
#include "dd_math.h"

// ---------------------------------------------------------------------------------------------
// Segment Kahan sum.  pandas' group_sum keeps (s, c) per group and takes the rows in their order:
//   v a NaN: skipped;  y = v - c;  t = s + y;  c = (t - s) - y;  c a NaN: c = 0;  s = t
// The chain is sequential by definition - its bits are the order's - so the parallelism is across segments and in the loads.
//
// Lane tier (n < wave_min): a lane per segment walks its rows.
// Wave tier (n >= wave_min): a wave per segment; the lanes fetch 64 rows at a time, coalesced through `order`, the next 64 while
// the chain of the current ones runs, and the chain takes value j from lane j with a cross-lane read: (s, c) are wave-uniform, every
// lane computes the same step.  No dependent load sits inside the chain.
//
// Both tiers run kahan_step on the same values in the same order: they agree bit for bit.  No atomics touch a sum.
// ---------------------------------------------------------------------------------------------
#define NGCF_KAHAN_WAVES 4
#define NGCF_KAHAN_MAX_VALUES 4

namespace {

constexpr int kKahanWaveMin = 128;        // the default `wave_min`: a placeholder; profiles/context_lab.txt records the run that sets it (none yet)

struct KahanCols {
    const double *x[NGCF_KAHAN_MAX_VALUES];
    double *sum[NGCF_KAHAN_MAX_VALUES];
};

__device__ inline double context_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ inline double context_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// One row of pandas' recurrence.  Re-association would fold (t - s) - y to 0: it is off here whatever the command line says.
__device__ inline void kahan_step(double v, double &s, double &c)
{
#pragma clang fp reassociate(off) contract(off)
    if (v != v) return;
    const double y = v - c;
    const double t = s + y;
    c = (t - s) - y;
    if (c != c) c = 0.0;
    s = t;
}

__device__ inline double kahan_readlane(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// a segment's bounds; false: the row pointers decrease or leave [0, T]
__device__ inline bool kahan_segment(const int64_t *__restrict__ rowptr, int64_t u, int64_t T, int64_t &lo, int64_t &n)
{
    lo = rowptr[u];
    const int64_t hi = rowptr[u + 1];
    n = hi - lo;
    return lo >= 0 && hi >= lo && hi <= T;
}

template <int V>
__global__ __launch_bounds__(256) void segment_kahan_lane_kernel(const int64_t *__restrict__ rowptr, int64_t n_rows,
                                                                 const int64_t *__restrict__ order, KahanCols cols, int64_t T,
                                                                 int64_t wave_min, int32_t *status)
{
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < n_rows; u += (int64_t)gridDim.x * 256) {
        int64_t lo, n;
        bool good = kahan_segment(rowptr, u, T, lo, n);                 // bad row pointers are reported here, whatever the length
        if (good && n >= wave_min) continue;                            // the wave tier's
        double s[V], c[V];
#pragma unroll
        for (int k = 0; k < V; ++k) s[k] = c[k] = 0.0;
        for (int64_t i = 0; good && i < n; ++i) {
            const int64_t p = order ? order[lo + i] : lo + i;
            if (p < 0 || p >= T) {                                      // never read through
                good = false;
                break;
            }
#pragma unroll
            for (int k = 0; k < V; ++k) kahan_step(cols.x[k][p], s[k], c[k]);
        }
        if (!good) atomicOr(status, 1);
#pragma unroll
        for (int k = 0; k < V; ++k) cols.sum[k][u] = good ? s[k] : context_nan();
    }
}

// the wave's next 64 rows of a segment, one per lane (lanes past the end hold a NaN, which the chain skips); true: an order entry
// of these rows lies outside [0, T) - no lane has read through it
template <int V>
__device__ inline bool kahan_fetch(const KahanCols &cols, const int64_t *__restrict__ order, int64_t lo, int64_t base, int64_t n,
                                   int64_t T, int lane, double (&v)[V])
{
    const int64_t i = base + lane;
    const bool mine = i < n;
    int64_t p = 0;
    if (mine) p = order ? order[lo + i] : lo + i;
    const bool inside = p >= 0 && p < T;
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = (mine && inside) ? cols.x[k][p] : context_nan();
    return __any(mine && !inside);
}

template <int V>
__global__ __launch_bounds__(64 * NGCF_KAHAN_WAVES) void segment_kahan_wave_kernel(const int64_t *__restrict__ rowptr, int64_t n_rows,
                                                                                  const int64_t *__restrict__ order, KahanCols cols,
                                                                                  int64_t T, int64_t wave_min, int32_t *status)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t u = (int64_t)blockIdx.x * NGCF_KAHAN_WAVES + wave; u < n_rows; u += (int64_t)gridDim.x * NGCF_KAHAN_WAVES) {
        int64_t lo, n;
        if (!kahan_segment(rowptr, u, T, lo, n) || n < wave_min) continue;        // the lane tier's (it reports bad row pointers)
        double s[V], c[V], v[V], next[V];
#pragma unroll
        for (int k = 0; k < V; ++k) s[k] = c[k] = next[k] = 0.0;
        bool bad = kahan_fetch<V>(cols, order, lo, 0, n, T, lane, v);
        for (int64_t base = 0; base < n && !bad; base += 64) {
            const int cnt = (int)(n - base < 64 ? n - base : 64);
            bool bad_next = false;
            if (base + 64 < n) bad_next = kahan_fetch<V>(cols, order, lo, base + 64, n, T, lane, next);
            for (int j = 0; j < cnt; ++j) {
#pragma unroll
                for (int k = 0; k < V; ++k) kahan_step(kahan_readlane(v[k], j), s[k], c[k]);
            }
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = next[k];
            bad = bad_next;
        }
        if (lane == 0) {
            if (bad) atomicOr(status, 1);
#pragma unroll
            for (int k = 0; k < V; ++k) cols.sum[k][u] = bad ? context_nan() : s[k];
        }
    }
}

template <int V>
int launch_kahan(const int64_t *rowptr, int64_t n_rows, const int64_t *order, const KahanCols &cols, int64_t T, int64_t wave_min,
                 int32_t *status, hipStream_t stream)
{
    segment_kahan_lane_kernel<V><<<dim3((unsigned)grid_for(n_rows, 256)), 256, 0, stream>>>(rowptr, n_rows, order, cols, T, wave_min, status);
    LAUNCH_CHECK();
    if (T >= wave_min) {                                                 // else no segment is long enough for the wave tier
        const int64_t blocks = std::min<int64_t>((n_rows + NGCF_KAHAN_WAVES - 1) / NGCF_KAHAN_WAVES, 256 * 16);
        segment_kahan_wave_kernel<V><<<dim3((unsigned)blocks), 64 * NGCF_KAHAN_WAVES, 0, stream>>>(rowptr, n_rows, order, cols, T, wave_min,
                                                                                                 status);
        LAUNCH_CHECK();
    }
    return NGCF_OK;
}

}  // namespace

extern "C" int ngcf_segment_kahan_sum_f64(const int64_t *rowptr, int64_t n_rows, const int64_t *order, const double *const *values,
                                          int n_values, int64_t T, int wave_min, double *const *sums, int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_values < 1 || n_values > NGCF_KAHAN_MAX_VALUES)
        return fail(NGCF_ERR_ARG, "segment_kahan_sum: %d value columns, outside [1, %d]", n_values, NGCF_KAHAN_MAX_VALUES);
    if (wave_min < 0) return fail(NGCF_ERR_ARG, "segment_kahan_sum: wave_min=%d is negative", wave_min);
    if (T < 0 || n_rows < 0)
        return fail(NGCF_ERR_ARG, "segment_kahan_sum: negative count (n_rows=%lld, T=%lld)", (long long)n_rows, (long long)T);
    if (n_rows == 0) return NGCF_OK;
    if (!rowptr || !values || !sums || !status) return fail(NGCF_ERR_ARG, "segment_kahan_sum: null argument");
    KahanCols cols = {};
    for (int k = 0; k < n_values; ++k) {
        if ((!values[k] && T > 0) || !sums[k]) return fail(NGCF_ERR_ARG, "segment_kahan_sum: null argument (column %d)", k);
        cols.x[k] = values[k];
        cols.sum[k] = sums[k];
    }
    const int64_t wmin = wave_min ? wave_min : kKahanWaveMin;
    switch (n_values) {
    case 1: return launch_kahan<1>(rowptr, n_rows, order, cols, T, wmin, status, stream);
    case 2: return launch_kahan<2>(rowptr, n_rows, order, cols, T, wmin, status, stream);
    case 3: return launch_kahan<3>(rowptr, n_rows, order, cols, T, wmin, status, stream);
    default: return launch_kahan<4>(rowptr, n_rows, order, cols, T, wmin, status, stream);
    }
}

// ---------------------------------------------------------------------------------------------
// Haversine table.  A workgroup takes 256 items and kHavRows departure points: a thread converts its item once (lat2, lng2,
// cos(lat2)), the first kHavRows threads convert a departure point each into LDS (lat1, lng1, cos(lat1): once per row and
// workgroup), then every thread walks the rows - two sines, a square root and an arc sine per output, stores coalesced along the
// items.  Every product and sum rounds once, as CPython's floats do, and sin, cos and asin are dd_math.h's: correctly rounded, so
// the table has the bits of a host whose libm rounds correctly instead of differing from it in the last place here and there.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr int kHavRows = 16;
constexpr double kDegToRad = 3.14159265358979323846 / 180.0;           // CPython's math.radians: x * (pi / 180)

__global__ __launch_bounds__(256) void haversine_table_kernel(const double *__restrict__ dep, int64_t S, const double *__restrict__ item,
                                                              int64_t n_item, double two_r, double *__restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ double s_lat[kHavRows], s_lng[kHavRows], s_cos[kHavRows];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    double lat2 = 0.0, lng2 = 0.0, cos2 = 0.0;
    if (i < n_item) {
        lat2 = item[2 * i] * kDegToRad;
        lng2 = item[2 * i + 1] * kDegToRad;
        cos2 = ddm::cos_cr(lat2);
    }
    for (int64_t s0 = (int64_t)blockIdx.y * kHavRows; s0 < S; s0 += (int64_t)gridDim.y * kHavRows) {
        const int rows = (int)(S - s0 < kHavRows ? S - s0 : kHavRows);
        __syncthreads();                                                // the previous chunk's rows have been read
        if (tid < rows) {
            const double lat1 = dep[2 * (s0 + tid)] * kDegToRad;
            s_lat[tid] = lat1;
            s_lng[tid] = dep[2 * (s0 + tid) + 1] * kDegToRad;
            s_cos[tid] = ddm::cos_cr(lat1);
        }
        __syncthreads();
        if (i >= n_item) continue;
        for (int r = 0; r < rows; ++r) {
            const double dlat = lat2 - s_lat[r], dlng = lng2 - s_lng[r];
            const double a = ddm::sin_cr(dlat * 0.5), b = ddm::sin_cr(dlng * 0.5);
            const double aa = a * a, bb = b * b;
            const double cc = s_cos[r] * cos2;
            const double ccbb = cc * bb;
            const double d = aa + ccbb;
            const double km = two_r * ddm::asin_cr(sqrt(d));
            const double m = km * 1000.0;
            out[(s0 + r) * n_item + i] = m != m ? context_inf() : m;    // a NaN coordinate: missing, sorts last
        }
    }
}

}  // namespace

extern "C" int ngcf_haversine_table_f64(const double *dep, int64_t S, const double *item, int64_t n_item, double *out, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (S < 0 || n_item < 0)
        return fail(NGCF_ERR_ARG, "haversine_table: negative count (S=%lld, n_item=%lld)", (long long)S, (long long)n_item);
    if (S == 0 || n_item == 0) return NGCF_OK;
    if (!dep || !item || !out) return fail(NGCF_ERR_ARG, "haversine_table: null argument");
    const int64_t bx = (n_item + 255) / 256;
    if (bx > 0x7fffffffll) return fail(NGCF_ERR_ARG, "haversine_table: n_item=%lld does not fit a grid", (long long)n_item);
    const int64_t by = std::min<int64_t>((S + kHavRows - 1) / kHavRows, 4096);
    const double two_r = 2 * 6371.0088;                                 // the package's mean earth radius in km, doubled on the host
    haversine_table_kernel<<<dim3((unsigned)bx, (unsigned)by), 256, 0, stream>>>(dep, S, item, n_item, two_r, out);
    LAUNCH_CHECK();
    return NGCF_OK;
}
