// Diversified top lists: greedy Maximal Marginal Relevance over a pool of candidates per request.  The definitions
// and operation orders are in include/ngcf_hip.h, section "diversified top lists".
//
// The gather / Gram stage below is list_diversity_kernel's (list_quality.hip), restated here on purpose: a test reads that file's
// text expression by expression, so its staging code cannot move into a shared header without changing that test.  One definition
// for both files is a later change.
#include "rank_device.h"

// ---------------------------------------------------------------------------------------------
// One wave per pool, a workgroup = 4 independent waves (no workgroup barrier at all).  The wave gathers its pool's item rows a
// 32-float chunk of D at a time into its own LDS region (rows padded to 33 floats; the next chunk's global loads sit in registers
// while the MFMAs run) and accumulates the pool's Gram matrix with v_mfma_f32_32x32x2_f32, A = B = the pool's rows: step s takes
// k = 2s (lanes 0-31) then 2s + 1 (lanes 32-63) into one accumulator, so G_ab is the ascending-k fmaf chain from 0 of
// ngcf_rank_topk_f32.  n <= 32: one 32x32 tile; n <= 64: the tiles (0,0), (0,1), (1,1).
//
// The finished tiles go back into the same LDS region, which the staging no longer needs.  G is symmetric bit for bit, so only
// G[a][b] with a <= b is ever read and the tile (1,0) is not kept: rows 0..31 have a pitch of 65 floats (33 for n <= 32), rows
// 32..63 hold their columns 32..63 at a pitch of 33.  With lane = slot a and the pick s, lane a reads G[min(a, s)][max(a, s)]: its
// bank is (a + s) mod 32 whichever side of s it is on (both pitches are 1 mod 32), distinct within each 32-lane half.
//
// LDS per workgroup: 4 x (32 x 65 + 32 x 33) x 4 B = 50 176 B of tiles and 4 x 64 x 4 B = 1 024 B of ids = 51 200 B: three
// workgroups share a CU's 160 KiB (n <= 32: 4 x 32 x 33 x 4 B + 1 024 B = 17 920 B).
//
// The greedy loop keeps lane = slot: relevance, G_aa, m_a and the candidate flag in registers; a step is one 6-round butterfly over
// (key, slot), one broadcast of the winner's key, two LDS reads and the fp64 cosine.  Nothing of size [n, D] or [n, n] goes to memory.
// ---------------------------------------------------------------------------------------------
namespace {

// where G[a][b], a <= b, sits in a wave's region
template <int NB> __device__ inline int mmr_gidx(int a, int b)
{
    if constexpr (NB == 1) return a * 33 + b;
    return a < 32 ? a * 65 + b : 32 * 65 + (a - 32) * 33 + (b - 32);
}

// Greater key wins, a NaN key is below every other, a slot that is not a candidate below that; +0.0 and -0.0 are one key.
__device__ inline unsigned long long mmr_order_key(double key, bool cand)
{
    if (!cand) return 0ull;
    if (key != key) return 1ull;
    unsigned long long u = key == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(key);
    return (u >> 63) ? ~u : (u | (1ull << 63));                 // -inf maps to 0x000fffffffffffff, above the two marks
}

template <int NB, bool VEC, bool F64>
__global__ __launch_bounds__(256) void list_mmr_kernel(const int64_t *__restrict__ pool, int64_t ld, const void *__restrict__ rel_,
                                                       int64_t ldr, int64_t B, int n, int top, const float *__restrict__ items,
                                                       int64_t ldi, int64_t n_items, int D, double lam, int normalize,
                                                       int64_t rows_per_wave, int64_t *__restrict__ out_items,
                                                       int32_t *__restrict__ out_slots, double *__restrict__ out_keys, int32_t *status)
{
#pragma clang fp contract(off) reassociate(off)
    constexpr int R = 32 * NB, TK = 32, SLD = TK + 1;
    constexpr int NP = VEC ? R / 8 : R / 2;                      // load passes per chunk: a float4 or a float per lane and pass
    constexpr int REGION = NB == 1 ? 32 * 33 : 32 * 65 + 32 * 33;
    static_assert(REGION >= R * SLD, "the staging rows fit in the Gram region");
    __shared__ float sE_[4][REGION];
    __shared__ int32_t sid_[4][64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
    float *sE = sE_[wave];
    int32_t *sid = sid_[wave];
    bool bad = false;
    const double oml = 1.0 - lam;
    const double kNaN = __longlong_as_double(0x7ff8000000000000ll), kInf = __longlong_as_double(0x7ff0000000000000ll);

    const int n_chunks = (D + TK - 1) / TK;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * rows_per_wave;
    const int64_t r1 = r0 + rows_per_wave < B ? r0 + rows_per_wave : B;
    for (int64_t r = r0; r < r1; ++r) {
        wave_lds_sync();                                         // the previous pool's readers are done
        int32_t id = -1;
        double v = 0.0;
        if (lane < n) {
            const int64_t e = pool[r * ld + lane];
            if (e >= n_items)
                bad = true;                                      // flagged, never an index: an empty slot from here on
            else if (e >= 0)
                id = (int32_t)e;
            if constexpr (F64)
                v = static_cast<const double *>(rel_)[r * ldr + lane];
            else
                v = (double)static_cast<const float *>(rel_)[r * ldr + lane];
        }
        sid[lane] = id;
        wave_lds_sync();

        float pf[NP * (VEC ? 4 : 1)];
        auto load = [&](int c) {
            const int k0 = c * TK;
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int f = lane + 64 * j;
                if constexpr (VEC) {
                    const int row = f >> 3, kk = k0 + 4 * (f & 7);
                    const int32_t it = sid[row];
                    float4 x = vzero4();
                    if (it >= 0 && kk < D) {
                        const float *p = items + (int64_t)it * ldi + kk;
                        if (kk + 3 < D) {
                            x = *reinterpret_cast<const float4 *>(p);
                        } else {
                            x.x = p[0];
                            if (kk + 1 < D) x.y = p[1];
                            if (kk + 2 < D) x.z = p[2];
                        }
                    }
                    pf[4 * j] = x.x, pf[4 * j + 1] = x.y, pf[4 * j + 2] = x.z, pf[4 * j + 3] = x.w;
                } else {
                    const int row = f >> 5, kk = k0 + (f & 31);
                    const int32_t it = sid[row];
                    pf[j] = (it >= 0 && kk < D) ? items[(int64_t)it * ldi + kk] : 0.f;
                }
            }
        };
        auto store = [&]() {
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int f = lane + 64 * j;
                if constexpr (VEC) {
                    float *q = sE + (f >> 3) * SLD + 4 * (f & 7);
                    q[0] = pf[4 * j], q[1] = pf[4 * j + 1], q[2] = pf[4 * j + 2], q[3] = pf[4 * j + 3];
                } else {
                    sE[(f >> 5) * SLD + (f & 31)] = pf[j];
                }
            }
        };

        f32x16 acc00, acc01, acc11;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc00[e] = acc01[e] = acc11[e] = 0.f;
        load(0);
        for (int c = 0; c < n_chunks; ++c) {
            wave_lds_sync();                                     // the previous chunk's operands are read
            store();
            wave_lds_sync();
            if (c + 1 < n_chunks) load(c + 1);                   // flies under the MFMAs
            const float *A0 = sE + col * SLD + half;
#pragma unroll
            for (int s = 0; s < TK / 2; ++s) {
                const float a0 = A0[2 * s];
                acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, a0, acc00, 0, 0, 0);
                if constexpr (NB == 2) {
                    const float a1 = A0[32 * SLD + 2 * s];
                    acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, a1, acc01, 0, 0, 0);
                    acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, a1, acc11, 0, 0, 0);
                }
            }
        }

        // the tiles into the region: a lane holds column `col` and the rows a = (e & 3) + 8 (e >> 2) + 4 half of a tile
        wave_lds_sync();                                         // the last chunk's operands are read
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int a = (e & 3) + 8 * (e >> 2) + 4 * half;
            if constexpr (NB == 1) {
                sE[a * 33 + col] = acc00[e];
            } else {
                sE[a * 65 + col] = acc00[e];
                sE[a * 65 + 32 + col] = acc01[e];
                sE[32 * 65 + a * 33 + col] = acc11[e];
            }
        }
        wave_lds_sync();

        // ---- relevance
        const bool valid = id >= 0;
        double rr = v;
        if (normalize) {
            const bool fin = valid && v - v == 0.0;              // finite: neither an infinity nor a NaN
            double lo = fin ? v + 0.0 : kInf, hi = fin ? v + 0.0 : -kInf;      // a zero of either sign enters as +0.0
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double ol = shfl_xor_f64(lo, m), oh = shfl_xor_f64(hi, m);
                lo = ol < lo ? ol : lo;
                hi = oh > hi ? oh : hi;
            }
            if (v - v == 0.0) {
                if (hi > lo) {
                    const double num = v - lo, den = hi - lo;
                    rr = num / den;
                } else {
                    rr = 0.0;
                }
            }
        }
        const double lr = lam * rr;

        // ---- the greedy loop, lane = slot
        const int V = __popcll(__ballot(valid));
        const int steps = top < V ? top : V;
        const double gaa = lane < R ? (double)sE[mmr_gidx<NB>(lane, lane)] : 0.0;
        bool cand = valid;
        double m_a = 0.0;
        int32_t res_slot = -1;
        int64_t res_item = -1;
        double res_key = -kInf;
        for (int t = 0; t < steps; ++t) {
            double key = lr;
            if (t > 0) {
                const double pen = oml * m_a;
                key = lr - pen;
            }
            unsigned long long ck = mmr_order_key(key, cand);
            int slot = lane;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const unsigned long long ok = shfl_xor_u64(ck, m);
                const int os = __shfl_xor(slot, m);
                if (ok > ck || (ok == ck && os < slot)) {
                    ck = ok;
                    slot = os;
                }
            }
            const int s = __builtin_amdgcn_readfirstlane(slot);  // a candidate: t < V
            const double wkey = __longlong_as_double(shfl_i64(__double_as_longlong(key), s));
            if (lane == t) {
                res_slot = s;
                res_item = (int64_t)sid[s];
                res_key = wkey != wkey ? kNaN : wkey;
            }
            if (lane == s) cand = false;
            if (t + 1 < steps) {
                const int lo_i = lane < s ? lane : s, hi_i = lane < s ? s : lane;
                const double g = lane < R ? (double)sE[mmr_gidx<NB>(lo_i, hi_i)] : 0.0;
                const double gss = (double)sE[mmr_gidx<NB>(s, s)];
                const double p = gaa * gss;
                double c = 0.0;
                if (!(p == 0.0)) {
                    const double root = sqrt(p);
                    c = g / root;
                }
                if (t == 0)
                    m_a = c;
                else if (m_a != m_a || c != c)
                    m_a = kNaN;
                else if (c > m_a)
                    m_a = c;
            }
        }
        if (lane < top) {
            out_items[r * top + lane] = res_item;
            if (out_slots) out_slots[r * top + lane] = res_slot;
            if (out_keys) out_keys[r * top + lane] = res_key;
        }
    }
    if (bad) atomicOr(status, 1);
}

}  // namespace

extern "C" int ngcf_list_mmr_f32(const int64_t *pool_idx, int64_t ld, const void *rel, int rel_f64, int64_t ldr, int64_t B, int n,
                                 int top, const float *items, int64_t ldi, int64_t n_items, int D, double lam, int normalize,
                                 int64_t *out_items, int32_t *out_slots, double *out_keys, int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 1 || n > NGCF_LIST_MMR_POOL_MAX) return fail(NGCF_ERR_ARG, "list_mmr: pool size n=%d outside [1, %d]", n, NGCF_LIST_MMR_POOL_MAX);
    if (top < 1 || top > n) return fail(NGCF_ERR_ARG, "list_mmr: top=%d outside [1, n=%d]", top, n);
    if (!(lam >= 0.0 && lam <= 1.0)) return fail(NGCF_ERR_ARG, "list_mmr: lam=%g outside [0, 1]", lam);
    if (D < 1 || ldi < D) return fail(NGCF_ERR_ARG, "list_mmr: D=%d, item row pitch %lld", D, (long long)ldi);
    if (n_items < 1 || n_items >= (int64_t)1 << 31) return fail(NGCF_ERR_ARG, "list_mmr: n_items=%lld outside [1, 2^31)", (long long)n_items);
    if (B < 0 || ld < n || ldr < n) return fail(NGCF_ERR_ARG, "list_mmr: bad argument (B, or a row pitch below n)");
    if (!pool_idx || !rel || !items || !out_items || !status) return fail(NGCF_ERR_ARG, "list_mmr: a null pointer");
    if (B == 0) return NGCF_OK;
    // the launch shape is a function of B alone: up to 2 048 workgroups of 4 waves, a wave takes a run of consecutive pools
    const int64_t blocks_want = std::min<int64_t>((B + 3) / 4, 2048);
    const int64_t rows_per_wave = (B + blocks_want * 4 - 1) / (blocks_want * 4);
    const int64_t blocks = (B + rows_per_wave * 4 - 1) / (rows_per_wave * 4);
    const bool vec = aligned16(items) && ldi % 4 == 0;
#define NGCF_LIST_MMR_LAUNCH(NB_, VEC_, F64_)                                                                                     \
    list_mmr_kernel<NB_, VEC_, F64_><<<dim3((unsigned)blocks), 256, 0, stream>>>(pool_idx, ld, rel, ldr, B, n, top, items, ldi, n_items, D, \
                                                                                lam, normalize != 0, rows_per_wave, out_items,   \
                                                                                out_slots, out_keys, status)
#define NGCF_LIST_MMR_BY_REL(NB_, VEC_)                                                                                           \
    do {                                                                                                                           \
        if (rel_f64) NGCF_LIST_MMR_LAUNCH(NB_, VEC_, true); else NGCF_LIST_MMR_LAUNCH(NB_, VEC_, false);                          \
    } while (0)
    if (n <= 32) {
        if (vec) NGCF_LIST_MMR_BY_REL(1, true); else NGCF_LIST_MMR_BY_REL(1, false);
    } else {
        if (vec) NGCF_LIST_MMR_BY_REL(2, true); else NGCF_LIST_MMR_BY_REL(2, false);
    }
#undef NGCF_LIST_MMR_BY_REL
#undef NGCF_LIST_MMR_LAUNCH
    LAUNCH_CHECK();
    return NGCF_OK;
}
