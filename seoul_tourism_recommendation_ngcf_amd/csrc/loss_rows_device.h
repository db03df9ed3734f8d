// loss_rows_device.h - the row machinery of the losses that score one positive row against m <= 64 negative rows (bpr_multi.hip,
// sampled_softmax.hip): one wave per positive row b, four rows per workgroup, the wave's u row in KU registers per lane (D <= 64 KU;
// none beyond 2048), the m negative rows streamed once, R at a time, and lane j keeping the score u.n_j of negative j.  Everything
// that the two losses do alike stands here once, in the same operations in the same order - which is what holds them equal bit for
// bit where their definitions meet (include/ngcf_hip.h):
//   device  URow, RowBatch, score_row (the score pass: fmaf over a lane's columns, stride 64, then the xor butterfly); lanes_lse and
//           softmax_weight (the softmax over the lanes' negatives); gradient_walk (the backward's second walk over the negatives,
//           with or without sign factors); the forward's tail is bpr_block_partials / bpr_finish_block (common.h)
//   host    check_rows, partials_workspace_bytes, partials_in, finish_loss and the width dispatch LOSS_ROWS_LAUNCH
// A loss file keeps its row's recipe: the loss and the coefficients s_j from the scores, its two kernels as compositions of the
// above, and the refusals of its own arguments.
#ifndef NGCF_LOSS_ROWS_DEVICE_H
#define NGCF_LOSS_ROWS_DEVICE_H

#include "common.h"

#pragma clang fp contract(off)

static_assert(NGCF_BPR_MULTI_M_MAX == 64 && NGCF_SAMPLED_SOFTMAX_M_MAX == 64, "lane j of a row's wave keeps negative j");

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

// log sum_j exp(x_j) over the lanes j < m of their values x: exp only ever sees differences to the maximum
__device__ __forceinline__ float lanes_lse(float x, int m, int lane)
{
    const float M = wave_max(lane < m ? x : -INFINITY);
    const float e = lane < m ? expf(x - M) : 0.f;
    return M + logf(wave_sum(e));
}

// lane j < m: exp(x_j) / (exp(x0) + sum_j exp(x_j)), the softmax weight of its value among x0 (wave-uniform, the positive's: it
// takes part in the maximum) and the lanes' values; 0 in the lanes from m on
__device__ __forceinline__ float softmax_weight(float x0, float x, int m, int lane)
{
    const float M = fmaxf(x0, wave_max(lane < m ? x : -INFINITY));
    const float e = lane < m ? expf(x - M) : 0.f;
    const float den = expf(x0 - M) + wave_sum(e);
    return e / den;
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

// The sign factors of a loss that scores |u.p| and |u.n_j|: p = sgn(u.p) (wave-uniform), n = sgn(u.n_j) in lane j.  NoSigns: plain
// scores - the walk below then has no multiply by them at all.
struct RowSigns {
    float p, n;
};
struct NoSigns {};

// The backward after the coefficients: with s_j = dl_b/d(u.n_j) up to the sign factor in lane j (0 from lane m on) and g, the
// upstream gradient over the batch size, a second walk over the row's negatives (cache hits), R rows at a time as the score pass,
//   dp = g fma(cp, u, 2 wd p),  cp = sgn_p sum_j s_j;   dn_j = g fma(-s_j sgn_nj, u, (2 wd / m) n_j);
//   du / g = 2 wd u + sum_j s_j (sgn_p p - sgn_nj n_j)
// in four chains, as the gathers' backward sums its rows (bwd_gather.hip): chain q takes the negatives j = q mod 4 in ascending
// order, one fma each, chain 0 starts from the weight-decay term, and the chains combine as (c0 + c1) + (c2 + c3).  With m = 1 and
// signs that is bpr_backward_kernel's fma(s, sgn_p p - sgn_n n, 2 wd u).  The lane's columns of du stay in registers; D > 2048 (no
// registers for the row): column by column, the m rows below each.
template <int KU, class Signs>
__device__ __forceinline__ void gradient_walk(const URow<KU> &ur, const float *__restrict__ pr, const float *__restrict__ nr, int m,
                                              int D, float s, const Signs sg, float g, float two_wd, float two_wd_m,
                                              float *__restrict__ dur, float *__restrict__ dpr, float *__restrict__ dnr)
{
    constexpr bool kSigned = std::is_same<Signs, RowSigns>::value;
    static_assert(kSigned || std::is_same<Signs, NoSigns>::value, "RowSigns or NoSigns");
    const int lane = ur.lane;
    float cp = wave_sum(s);
    if constexpr (kSigned) cp = cp * sg.p;
    const auto signed_p = [&](float bb) {                                     // sgn_p p
        if constexpr (kSigned) return sg.p * bb;
        else return bb;
    };
    const auto sign_n = [&](int j) {                                          // sgn_nj
        if constexpr (kSigned) return lane_value(sg.n, j);
        else return 0.f;                                                      // (never read)
    };
    const auto dn_coefficient = [&](float sj, float gj) {                     // -s_j sgn_nj
        if constexpr (kSigned) return -sj * gj;
        else return -sj;
    };
    const auto difference = [&](float pb, float gj, float c) {                // sgn_p p - sgn_nj n_j
        if constexpr (kSigned) return pb - gj * c;
        else return pb - c;
    };
    if constexpr (KU > 0) {
        float acc[4][KU], pb[KU];
#pragma unroll
        for (int k = 0; k < KU; ++k) {
            const int col = lane + 64 * k;
            const float a = ur.v[k], bb = col < D ? pr[col] : 0.f;
            pb[k] = signed_p(bb);
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
                    const float sj = lane_value(s, j), gj = sign_n(j), cn = dn_coefficient(sj, gj);
                    float *dnj = dnr + (int64_t)j * D;
#pragma unroll
                    for (int k = 0; k < KU; ++k) {
                        if (lane + 64 * k < D) dnj[lane + 64 * k] = g * fmaf(cn, ur.v[k], two_wd_m * c[r][k]);
                        acc[h + r][k] = fmaf(sj, difference(pb[k], gj, c[r][k]), acc[h + r][k]);
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < KU; ++k)
            if (lane + 64 * k < D) dur[lane + 64 * k] = g * ((acc[0][k] + acc[1][k]) + (acc[2][k] + acc[3][k]));
    } else {
        for (int col = lane; col < D; col += 64) {
            const float a = ur.row[col], bb = pr[col], pb = signed_p(bb);
            float acc[4] = {two_wd * a, 0.f, 0.f, 0.f};
            for (int j0 = 0; j0 < m; j0 += 4) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = j0 + q;
                    if (j >= m) break;
                    const float c = nr[(int64_t)j * D + col];
                    const float sj = lane_value(s, j), gj = sign_n(j);
                    dnr[(int64_t)j * D + col] = g * fmaf(dn_coefficient(sj, gj), a, two_wd_m * c);
                    acc[q] = fmaf(sj, difference(pb, gj, c), acc[q]);
                }
            }
            dur[col] = g * ((acc[0] + acc[1]) + (acc[2] + acc[3]));
            dpr[col] = g * fmaf(cp, a, two_wd * bb);
        }
    }
}

// The second stage of the forward: the workgroups' partials -> *loss
__global__ __launch_bounds__(256) void loss_rows_finish_kernel(const float *__restrict__ part, int64_t n_blocks, float wd,
                                                               float batch_size, float *__restrict__ loss)
{
    bpr_finish_block(part, n_blocks, wd, batch_size, loss);
}

inline int finish_loss(const float *part, int64_t B, float wd, float batch_size, float *loss, hipStream_t stream)
{
    loss_rows_finish_kernel<<<1, 256, 0, stream>>>(part, (B + 3) / 4, wd, batch_size, loss);
    LAUNCH_CHECK();
    return NGCF_OK;
}

// the u row's registers per lane for a width: the next power of two of ceil(D / 64) up to 32, 0 (memory) beyond
inline int registers_for(int D)
{
    for (int ku = 1; ku <= 32; ku *= 2)
        if (D <= 64 * ku) return ku;
    return 0;
}

// the refusals of both directions of both losses: the width, m, and row counts that are B / B / B m (`what`: the entry's name)
inline int check_rows(const char *what, int64_t Bu, int64_t Bp, int64_t Bn, int m, int D)
{
    if (D <= 0) return fail(NGCF_ERR_ARG, "%s: D=%d", what, D);
    if (m < 1 || m > 64) return fail(NGCF_ERR_ARG, "%s: m=%d outside [1, %d]", what, m, 64);
    if (Bu < 1 || Bu > ((int64_t)1 << 32) || Bp != Bu || Bn != Bu * m)
        return fail(NGCF_ERR_ARG, "%s: row counts %lld/%lld/%lld are not B/B/B*m with m=%d (no operand broadcasts)", what, (long long)Bu,
                    (long long)Bp, (long long)Bn, m);
    return NGCF_OK;
}

// the forward's workspace: two floats per workgroup of four rows, and room to align them
inline int64_t partials_workspace_bytes(int64_t B)
{
    if (B < 0) return -1;
    return align_up(((B + 3) / 4) * 2 * (int64_t)sizeof(float), 256) + 256;
}

// *part: the partials, 256-byte aligned in the caller's workspace - or the refusal of a workspace that cannot hold them
inline int partials_in(const char *what, void *workspace, int64_t workspace_bytes, int64_t B, float **part)
{
    const int64_t need = partials_workspace_bytes(B);
    if (!workspace || workspace_bytes < need)
        return fail(NGCF_ERR_WORKSPACE, "%s: workspace %lld B < %lld B", what, (long long)workspace_bytes, (long long)need);
    *part = reinterpret_cast<float *>(align_up((int64_t)(uintptr_t)workspace, 256));
    return NGCF_OK;
}

}  // namespace

// kernel<KU><<<a workgroup per four of the B rows, on stream>>>(...) for the KU of the width `D` in scope; returns on a failed launch
#define LOSS_ROWS_LAUNCH(kernel, B, stream, ...)                                     \
    do {                                                                             \
        const dim3 grid_((unsigned)(((B) + 3) / 4));                                 \
        switch (registers_for(D)) {                                                  \
        case 1: kernel<1><<<grid_, 256, 0, stream>>>(__VA_ARGS__); break;            \
        case 2: kernel<2><<<grid_, 256, 0, stream>>>(__VA_ARGS__); break;            \
        case 4: kernel<4><<<grid_, 256, 0, stream>>>(__VA_ARGS__); break;            \
        case 8: kernel<8><<<grid_, 256, 0, stream>>>(__VA_ARGS__); break;            \
        case 16: kernel<16><<<grid_, 256, 0, stream>>>(__VA_ARGS__); break;          \
        case 32: kernel<32><<<grid_, 256, 0, stream>>>(__VA_ARGS__); break;          \
        default: kernel<0><<<grid_, 256, 0, stream>>>(__VA_ARGS__); break;           \
        }                                                                            \
        LAUNCH_CHECK();                                                              \
    } while (0)

#endif  // NGCF_LOSS_ROWS_DEVICE_H
