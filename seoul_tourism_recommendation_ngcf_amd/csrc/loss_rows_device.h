// loss_rows_device.h - the row machinery of the losses that score one positive row against m <= 64 negative rows (bpr_multi.hip,
// sampled_softmax.hip): one wave per positive row b, the wave's u row in KU registers per lane (D <= 64 KU; none beyond 2048), the m
// negative rows streamed once, R at a time, and lane j keeping the score u.n_j of negative j.  Defined once: both files' dot products
// and squared norms are the same operations in the same order (fmaf over a lane's columns, stride 64, then the xor butterfly), which
// is what holds the two losses equal bit for bit where their definitions meet (include/ngcf_hip.h).
#ifndef NGCF_LOSS_ROWS_DEVICE_H
#define NGCF_LOSS_ROWS_DEVICE_H

#include "common.h"

#pragma clang fp contract(off)

namespace {

__device__ inline float wave_max(float x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = fmaxf(x, __shfl_xor(x, m));
    return x;
}

// lane `j` (wave-uniform) of x
__device__ inline float lane_value(float x, int j)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j));
}

// The u row of a wave: KU registers per lane, column lane + 64 k in register k; KU = 0 reads the row from memory every time
// (D > 2048: the row is a cache hit after its first use).
template <int KU>
struct URow {
    float v[KU > 0 ? KU : 1];
    const float *row;
    int D, lane;

    __device__ URow(const float *__restrict__ ur, int D_, int lane_) : row(ur), D(D_), lane(lane_)
    {
        if (KU > 0) {
#pragma unroll
            for (int k = 0; k < KU; ++k) {
                const int j = lane + 64 * k;
                v[k] = j < D ? ur[j] : 0.f;
            }
        }
    }

    // f(column, u value) for the lane's columns in ascending order
    template <class F>
    __device__ __forceinline__ void for_columns(F &&f) const
    {
        if (KU > 0) {
#pragma unroll
            for (int k = 0; k < KU; ++k) {
                const int j = lane + 64 * k;
                if (j < D) f(j, v[k]);
            }
        } else {
            for (int j = lane; j < D; j += 64) f(j, row[j]);
        }
    }
};

// What a wave knows of its row after the score pass.  Wave-uniform: up = u.p, the squared norms uu, pp and nn = sum_j |n_j|^2
// (j ascending).  Per lane j < m: un = u.n_j (0 in the lanes from m on).
struct Scores {
    float up, uu, pp, nn, un;
};

// rows per batch of the score pass: R x KU loads in flight per lane
template <int KU>
struct RowBatch {
    static constexpr int R = KU == 0 ? 2 : (KU <= 8 ? 4 : (KU <= 16 ? 2 : 1));
};

template <int KU>
__device__ __forceinline__ Scores score_row(const URow<KU> &u, const float *__restrict__ pr, const float *__restrict__ nr, int m, int D,
                                            int lane)
{
    Scores s;
    float up = 0.f, uu = 0.f, pp = 0.f;
    u.for_columns([&](int j, float a) {
        const float b = pr[j];
        up = fmaf(a, b, up);
        uu = fmaf(a, a, uu);
        pp = fmaf(b, b, pp);
    });
    s.up = wave_sum(up);
    s.uu = wave_sum(uu);
    s.pp = wave_sum(pp);
    s.nn = 0.f;
    s.un = 0.f;
    constexpr int R = RowBatch<KU>::R;
    for (int j0 = 0; j0 < m; j0 += R) {
        float un[R], nn[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {       // a batch's rows past m read row m - 1 again (no branch between the rows' loads) and are dropped below
            const float *nj = nr + (int64_t)min(j0 + r, m - 1) * D;
            float d = 0.f, q = 0.f;
            u.for_columns([&](int j, float a) {
                const float c = nj[j];
                d = fmaf(a, c, d);
                q = fmaf(c, c, q);
            });
            un[r] = d;
            nn[r] = q;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float d = wave_sum(un[r]), q = wave_sum(nn[r]);
            if (j0 + r < m) {
                if (lane == j0 + r) s.un = d;
                s.nn += q;
            }
        }
    }
    return s;
}

// the u row's registers per lane for a width: the next power of two of ceil(D / 64) up to 32, 0 (memory) beyond
inline int registers_for(int D)
{
    for (int ku = 1; ku <= 32; ku *= 2)
        if (D <= 64 * ku) return ku;
    return 0;
}

}  // namespace

// fn<KU>(...) for the KU of the width `D` in scope
#define LOSS_ROWS_DISPATCH(fn, ...)                          \
    switch (registers_for(D)) {                              \
    case 1: return fn<1>(__VA_ARGS__);                       \
    case 2: return fn<2>(__VA_ARGS__);                       \
    case 4: return fn<4>(__VA_ARGS__);                       \
    case 8: return fn<8>(__VA_ARGS__);                       \
    case 16: return fn<16>(__VA_ARGS__);                     \
    case 32: return fn<32>(__VA_ARGS__);                     \
    default: return fn<0>(__VA_ARGS__);                      \
    }

#endif  // NGCF_LOSS_ROWS_DEVICE_H
