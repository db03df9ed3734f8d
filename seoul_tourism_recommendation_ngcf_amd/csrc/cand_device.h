// Device-side building blocks of a candidate score (shared by eval_candidates.hip and sample_hard.hip): the "Score bits" of
// eval_candidates.hip, defined once so that every kernel that scores a (user row, item row) pair gives the same bits.
#ifndef NGCF_CAND_DEVICE_H
#define NGCF_CAND_DEVICE_H

#include "common.h"

// ---------------------------------------------------------------------------------------------
// Score bits.  s = <u, item> is: per lane of a 16-lane group one ascending fmaf chain from 0 over the lane's quads q = s, s + 16, ..
// (quad q = elements 4q..4q+3; elements past D enter as 0 in both load forms), then an xor butterfly (8, 4, 2, 1) over the 16 lanes.
// Which lane adds what depends on D alone.  The user row comes out of the wave's LDS (whole quads, zero-padded) when it fits
// NGCF_CAND_LDS_FLOATS, out of global memory through cand_quad<false> when not: the same values, the same bits.
// ---------------------------------------------------------------------------------------------
#define NGCF_CAND_LDS_FLOATS 4096          // per wave: a user row that (with what else the wave keeps there) exceeds this is read from global memory instead

namespace {

// quad q of a row of D floats, elements past D as 0
template <bool VEC> __device__ inline float4 cand_quad(const float *row, int q, int D)
{
    const int e = 4 * q;
    if (VEC && e + 3 < D) return *reinterpret_cast<const float4 *>(row + e);
    float4 v;
    v.x = row[e];                           // callers pass e < D
    v.y = e + 1 < D ? row[e + 1] : 0.f;
    v.z = e + 2 < D ? row[e + 2] : 0.f;
    v.w = e + 3 < D ? row[e + 3] : 0.f;
    return v;
}

// one quad's four steps of a lane's chain
__device__ inline float cand_fma4(float4 u, float4 x, float s)
{
    s = fmaf(u.x, x.x, s);
    s = fmaf(u.y, x.y, s);
    s = fmaf(u.z, x.z, s);
    s = fmaf(u.w, x.w, s);
    return s;
}

__device__ inline float group16_sum(float x)
{
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

}  // namespace

#endif  // NGCF_CAND_DEVICE_H
