// Beyond-accuracy figures of top lists: how often every item is shown (exposure counts), what the exposure histogram
// looks like (coverage, Gini, entropy, novelty from five reduced numbers) and how different the items within one list are
// (intra-list diversity from the lists' Gram matrices).  The definitions and operation orders are in include/ngcf_hip.h.
#include "rank_device.h"
#include "dd_log2.h"

// ---------------------------------------------------------------------------------------------
// Exposure.  Up to NGCF_EXPOSURE_LDS_ITEMS items a workgroup folds its slice of the entries into an int32 table in LDS and flushes
// the non-zero slots with one 64-bit atomic each: a catalogue of 100 destinations would otherwise send every entry of every list to
// the same 100 words in memory (the reason groupby.hip keeps its small tables in LDS).  16 384 slots = 64 KiB: two workgroups of the
// largest table share a CU's 160 KiB, and a smaller catalogue asks for less (the table is dynamic LDS of n_items slots).  A slice
// holds at most 2^30 entries, so a slot cannot overflow.  Above the constant: 64-bit atomics in memory.
// ---------------------------------------------------------------------------------------------
#define NGCF_EXPOSURE_LDS_ITEMS 16384
#define NGCF_EXPOSURE_SLICE_MAX (1ll << 30)

namespace {

template <bool LDS>
__global__ __launch_bounds__(256) void list_exposure_kernel(const int64_t *__restrict__ top, int64_t ld, int64_t total, int k,
                                                            int64_t n_items, int64_t slice, unsigned long long *__restrict__ counts,
                                                            int32_t *status)
{
    extern __shared__ int32_t expo_tab[];
    const int tid = threadIdx.x;
    if (LDS) {
        for (int64_t i = tid; i < n_items; i += 256) expo_tab[i] = 0;
        __syncthreads();
    }
    const int64_t e0 = (int64_t)blockIdx.x * slice;
    const int64_t e1 = e0 + slice < total ? e0 + slice : total;
    bool bad = false;
    for (int64_t e = e0 + tid; e < e1; e += 256) {
        const int64_t id = ld == k ? top[e] : top[(e / k) * ld + e % k];
        if (id < 0) continue;
        if (id >= n_items) {                                    // flagged, never an index
            bad = true;
            continue;
        }
        if (LDS)
            atomicAdd(&expo_tab[id], 1);
        else
            atomicAdd(&counts[id], 1ull);
    }
    if (bad) atomicOr(status, 1);
    if (LDS) {
        __syncthreads();
        for (int64_t i = tid; i < n_items; i += 256) {
            const int32_t v = expo_tab[i];
            if (v) atomicAdd(&counts[i], (unsigned long long)v);
        }
    }
}

}  // namespace

extern "C" int ngcf_list_exposure(const int64_t *top_idx, int64_t ld, int64_t B, int k, int64_t n_items, int64_t *counts,
                                  int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (B < 0 || k < 1 || ld < k || n_items < 1 || n_items >= (int64_t)1 << 31) return fail(NGCF_ERR_ARG, "list_exposure: bad argument");
    if (B == 0) return NGCF_OK;
    if (!top_idx || !counts || !status) return fail(NGCF_ERR_ARG, "list_exposure: bad argument");
    if (B > ((int64_t)1 << 40) / k) return fail(NGCF_ERR_ARG, "list_exposure: batch too large");
    const int64_t total = B * k;
    int64_t slice = align_up((total + 1023) / 1024, 256);
    slice = std::min<int64_t>(std::max<int64_t>(slice, 4096), NGCF_EXPOSURE_SLICE_MAX);
    const int64_t blocks = (total + slice - 1) / slice;
    unsigned long long *c = reinterpret_cast<unsigned long long *>(counts);
    if (n_items <= NGCF_EXPOSURE_LDS_ITEMS)
        list_exposure_kernel<true><<<dim3((unsigned)blocks), 256, (size_t)n_items * 4, stream>>>(top_idx, ld, total, k, n_items, slice, c,
                                                                                                  status);
    else
        list_exposure_kernel<false><<<dim3((unsigned)blocks), 256, 0, stream>>>(top_idx, ld, total, k, n_items, slice, c, status);
    LAUNCH_CHECK();
    return NGCF_OK;
}

// ---------------------------------------------------------------------------------------------
// Summary of an exposure histogram: three exact integers and two fp64 sums in a fixed tree - a thread its strided elements in
// ascending order, a wave by xor-shuffles (32, 16, .., 1), a workgroup its four waves in order, one workgroup the blocks the same way.
// ---------------------------------------------------------------------------------------------
#define NGCF_SUMMARY_BLOCKS_MAX 1024

namespace {

struct SummaryAcc {
    unsigned long long covered, total, weighted, bad;
    double clog, nov;
};

// wave, then workgroup: the result in thread 0
__device__ inline SummaryAcc summary_block_reduce(SummaryAcc a)
{
#pragma clang fp contract(off) reassociate(off)
    __shared__ SummaryAcc sh[4];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        a.covered += shfl_xor_u64(a.covered, m);
        a.total += shfl_xor_u64(a.total, m);
        a.weighted += shfl_xor_u64(a.weighted, m);
        a.bad |= shfl_xor_u64(a.bad, m);
        a.clog += shfl_xor_f64(a.clog, m);
        a.nov += shfl_xor_f64(a.nov, m);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        a = sh[0];
        for (int w = 1; w < 4; ++w) {
            a.covered += sh[w].covered;
            a.total += sh[w].total;
            a.weighted += sh[w].weighted;
            a.bad |= sh[w].bad;
            a.clog += sh[w].clog;
            a.nov += sh[w].nov;
        }
    }
    return a;
}

__global__ __launch_bounds__(256) void exposure_summary_kernel(const int64_t *__restrict__ sorted, const int64_t *__restrict__ counts,
                                                               const int64_t *__restrict__ pop, int64_t n_items, int64_t n_user,
                                                               SummaryAcc *__restrict__ part)
{
#pragma clang fp contract(off) reassociate(off)
    SummaryAcc a = {0, 0, 0, 0, 0.0, 0.0};
    const double log_users = pop ? ddm::log2_cr((double)n_user) : 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_items; i += stride) {
        const int64_t c = sorted[i];
        if (c < 0) a.bad = 1;
        if (c > 0) {
            a.covered += 1;
            a.total += (unsigned long long)c;
            a.weighted += (unsigned long long)(i + 1) * (unsigned long long)c;     // wraps only where the finish drops it
            const double cd = (double)c;
            a.clog += cd * ddm::log2_cr(cd);
        }
        if (pop) {
            const int64_t u = counts[i];
            if (u > 0) {
                const int64_t p = pop[i] > 1 ? pop[i] : 1;
                const double surprise = log_users - ddm::log2_cr((double)p);
                a.nov += (double)u * surprise;
            }
        }
    }
    a = summary_block_reduce(a);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

__global__ __launch_bounds__(256) void exposure_summary_finish_kernel(const SummaryAcc *__restrict__ part, int n_blocks, int64_t n_items,
                                                                      int64_t *__restrict__ out)
{
#pragma clang fp contract(off) reassociate(off)
    SummaryAcc a = {0, 0, 0, 0, 0.0, 0.0};
    for (int b = threadIdx.x; b < n_blocks; b += 256) {
        const SummaryAcc p = part[b];
        a.covered += p.covered;
        a.total += p.total;
        a.weighted += p.weighted;
        a.bad |= p.bad;
        a.clog += p.clog;
        a.nov += p.nov;
    }
    a = summary_block_reduce(a);
    if (threadIdx.x == 0) {
        int64_t word = a.bad ? 2 : 0;
        // n_items * total >= 2^62 (n_items < 2^31): the weighted sum may not fit, it is not reported
        const unsigned long long hi = __umul64hi((unsigned long long)n_items, a.total), lo = (unsigned long long)n_items * a.total;
        if (hi != 0 || lo >> 62) {
            word |= 1;
            a.weighted = 0;
        }
        out[0] = (int64_t)a.covered;
        out[1] = (int64_t)a.total;
        out[2] = (int64_t)a.weighted;
        out[3] = word;
        out[4] = __double_as_longlong(a.clog);
        out[5] = __double_as_longlong(a.nov);
    }
}

}  // namespace

extern "C" int ngcf_exposure_summary(const int64_t *sorted_counts, const int64_t *counts, const int64_t *popularity, int64_t n_items,
                                     int64_t n_user, int64_t *out, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_items < 1 || n_items >= (int64_t)1 << 31 || !sorted_counts || !out) return fail(NGCF_ERR_ARG, "exposure_summary: bad argument");
    if (popularity && (!counts || n_user < 1))
        return fail(NGCF_ERR_ARG, "exposure_summary: popularity needs the unsorted counts and n_user >= 1");
    const int blocks = (int)std::min<int64_t>((n_items + 255) / 256, NGCF_SUMMARY_BLOCKS_MAX);
    void *part = nullptr;
    HIP_TRY(hipMallocAsync(&part, sizeof(SummaryAcc) * (size_t)blocks, stream));
    exposure_summary_kernel<<<dim3((unsigned)blocks), 256, 0, stream>>>(sorted_counts, counts, popularity, n_items, n_user,
                                                                        static_cast<SummaryAcc *>(part));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        exposure_summary_finish_kernel<<<1, 256, 0, stream>>>(static_cast<SummaryAcc *>(part), blocks, n_items, out);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(part, stream);
    if (e != hipSuccess) return fail(NGCF_ERR_HIP, "exposure_summary: kernel launch failed: %s", hipGetErrorString(e));
    return NGCF_OK;
}

// ---------------------------------------------------------------------------------------------
// Intra-list diversity.  One wave per list, a workgroup = 4 independent waves (no workgroup barrier until the final sums).  The wave
// gathers its list's item rows a 32-float chunk of D at a time into its own LDS region (rows padded to 33 floats; the next chunk's
// global loads sit in registers while the MFMAs run) and accumulates the list's Gram matrix with v_mfma_f32_32x32x2_f32, A = B = the
// list's rows: step s takes k = 2s (lanes 0-31) then 2s + 1 (lanes 32-63) into one accumulator, so G_ab is the ascending-k fmaf
// chain from 0 of ngcf_rank_topk_f32.  Columns past D and the rows of empty slots are zeros in LDS (a zero product leaves the chain's
// value as it is); no row of an empty slot is ever loaded.  k <= 32: one 32x32 tile; k <= 64: the tiles (0,0), (0,1), (1,1) - only
// pairs a < b and the diagonal are needed.  A lane then holds column b = lane & 31 of a tile and 16 of its rows,
// a = (e & 3) + 8 (e >> 2) + 4 (lane >> 5): the fp64 chain s_b over ascending a alternates between the two half-waves, four terms
// at a time, the running value handed over by a shuffle.  Nothing of size [k, D] or [k, k] goes to memory.
// ---------------------------------------------------------------------------------------------
#define NGCF_LIST_DIV_KS_MAX 8

namespace {

struct ListDivKs {
    int v[NGCF_LIST_DIV_KS_MAX];
};

__device__ inline double list_pair_distance(double g, double gaa, double gbb)
{
#pragma clang fp contract(off) reassociate(off)
    const double p = gaa * gbb;
    const double c = p == 0.0 ? 0.0 : g / sqrt(p);
    return 1.0 - c;
}

// this lane's column b of one tile whose rows are a_base + 0..31: s += d_ab over the valid a < b, ascending a
__device__ inline double list_div_chain(const f32x16 &acc, int a_base, int b, double s, const int32_t *sid, const float *sdiag,
                                        int half)
{
#pragma clang fp contract(off) reassociate(off)
    const bool b_valid = sid[b] >= 0;
    const double gbb = (double)sdiag[b];
#pragma unroll
    for (int t = 0; t < 8; ++t) {                                // rows a_base + 4t .. 4t + 3 live in half-wave t & 1
        if (half == (t & 1)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int a = a_base + 4 * t + j;
                if (b_valid && a < b && sid[a] >= 0) s += list_pair_distance((double)acc[4 * (t >> 1) + j], (double)sdiag[a], gbb);
            }
        }
        const double o = shfl_xor_f64(s, 32);
        if (half != (t & 1)) s = o;
    }
    return s;
}

// G_cc of a diagonal tile: row c sits in half-wave (c >> 2) & 1, element 4 (c >> 3) + (c & 3)
__device__ inline void list_div_diag(const f32x16 &acc, int col, int half, float *sdiag)
{
    const int want = 4 * (col >> 3) + (col & 3);
    float g = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e)
        if (e == want) g = acc[e];
    if (half == ((col >> 2) & 1)) sdiag[col] = g;
}

template <int NB, bool VEC>
__global__ __launch_bounds__(256) void list_diversity_kernel(const int64_t *__restrict__ top, int64_t ld, int64_t B, int k,
                                                             const float *__restrict__ items, int64_t ldi, int64_t n_items, int D,
                                                             int n_ks, ListDivKs ks, int64_t rows_per_wave, double *__restrict__ per_user,
                                                             double *__restrict__ part, int32_t *status)
{
#pragma clang fp contract(off) reassociate(off)
    constexpr int R = 32 * NB, TK = 32, SLD = TK + 1;
    constexpr int NP = VEC ? R / 8 : R / 2;                      // load passes per chunk: a float4 or a float per lane and pass
    __shared__ float sE_[4][R * SLD];
    __shared__ int32_t sid_[4][64];
    __shared__ float sdiag_[4][64];
    __shared__ double ssb_[4][64];
    __shared__ double swg[4][2 * NGCF_LIST_DIV_KS_MAX];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
    float *sE = sE_[wave];
    int32_t *sid = sid_[wave];
    float *sdiag = sdiag_[wave];
    double *ssb = ssb_[wave];

    int my_k = 0;                                                // lane q < n_ks evaluates cut-off q
#pragma unroll
    for (int q = 0; q < NGCF_LIST_DIV_KS_MAX; ++q)
        if (lane == q && q < n_ks) my_k = ks.v[q];
    double sum_ild = 0.0, sum_rows = 0.0;
    bool bad = false;

    const int n_chunks = (D + TK - 1) / TK;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * rows_per_wave;
    const int64_t r1 = r0 + rows_per_wave < B ? r0 + rows_per_wave : B;
    for (int64_t r = r0; r < r1; ++r) {
        wave_lds_sync();                                         // the previous list's readers are done
        int32_t id = -1;
        if (lane < k) {
            const int64_t v = top[r * ld + lane];
            if (v >= n_items)
                bad = true;                                      // flagged, never an index: an empty slot from here on
            else if (v >= 0)
                id = (int32_t)v;
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
                    float4 v = vzero4();
                    if (it >= 0 && kk < D) {
                        const float *p = items + (int64_t)it * ldi + kk;
                        if (kk + 3 < D) {
                            v = *reinterpret_cast<const float4 *>(p);
                        } else {
                            v.x = p[0];
                            if (kk + 1 < D) v.y = p[1];
                            if (kk + 2 < D) v.z = p[2];
                        }
                    }
                    pf[4 * j] = v.x, pf[4 * j + 1] = v.y, pf[4 * j + 2] = v.z, pf[4 * j + 3] = v.w;
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

        list_div_diag(acc00, col, half, sdiag);
        if constexpr (NB == 2) list_div_diag(acc11, col, half, sdiag + 32);
        wave_lds_sync();
        const double s0 = list_div_chain(acc00, 0, col, 0.0, sid, sdiag, half);
        if (half == 0) ssb[col] = s0;
        if constexpr (NB == 2) {
            double s1 = list_div_chain(acc01, 0, 32 + col, 0.0, sid, sdiag, half);
            s1 = list_div_chain(acc11, 32, 32 + col, s1, sid, sdiag, half);
            if (half == 0) ssb[32 + col] = s1;
        }
        wave_lds_sync();

        if (lane < n_ks) {
            double S = 0.0;
            int V = 0;
            for (int b = 0; b < my_k; ++b) {
                if (sid[b] >= 0) {
                    S += ssb[b];
                    ++V;
                }
            }
            double ild = 0.0;
            if (V >= 2) {
                ild = S / (double)(V * (V - 1) / 2);
                sum_ild += ild;
                sum_rows += 1.0;
            }
            if (per_user) per_user[r * n_ks + lane] = ild;
        }
    }
    if (bad) atomicOr(status, 1);

    // this workgroup's waves in order, slot by slot
    if (lane < n_ks) {
        swg[wave][lane] = sum_ild;
        swg[wave][n_ks + lane] = sum_rows;
    }
    __syncthreads();
    if (tid < 2 * n_ks) {
        double a = 0.0;
        for (int w = 0; w < 4; ++w) a += swg[w][tid];
        part[(int64_t)blockIdx.x * (2 * n_ks) + tid] = a;
    }
}

}  // namespace

extern "C" int ngcf_list_diversity_f32(const int64_t *top_idx, int64_t ld, int64_t B, int k, const float *items, int64_t ldi,
                                       int64_t n_items, int D, const int32_t *ks_host, int n_ks, double *per_user, double *sums,
                                       int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_ks < 1 || n_ks > NGCF_LIST_DIV_KS_MAX || !ks_host)
        return fail(NGCF_ERR_ARG, "list_diversity: between 1 and %d cut-offs", NGCF_LIST_DIV_KS_MAX);
    if (k < 2 || ld < k) return fail(NGCF_ERR_ARG, "list_diversity: k=%d, row pitch %lld", k, (long long)ld);
    ListDivKs ks = {{0, 0, 0, 0, 0, 0, 0, 0}};
    int k_used = 0;
    for (int q = 0; q < n_ks; ++q) {
        if (ks_host[q] < 2 || ks_host[q] > k || ks_host[q] > NGCF_LIST_DIV_K_MAX)
            return fail(NGCF_ERR_ARG, "list_diversity: cut-off K=%d outside [2, min(k=%d, %d)]", ks_host[q], k, NGCF_LIST_DIV_K_MAX);
        ks.v[q] = ks_host[q];
        k_used = std::max(k_used, ks_host[q]);
    }
    if (B < 0 || n_items < 1 || n_items >= (int64_t)1 << 31 || D < 1 || ldi < D) return fail(NGCF_ERR_ARG, "list_diversity: bad argument");
    if (B == 0) return NGCF_OK;
    if (!top_idx || !items || !sums || !status) return fail(NGCF_ERR_ARG, "list_diversity: bad argument");
    // the launch shape is a function of B alone: up to 2 048 workgroups of 4 waves, a wave takes a run of consecutive lists
    const int64_t blocks_want = std::min<int64_t>((B + 3) / 4, 2048);
    const int64_t rows_per_wave = (B + blocks_want * 4 - 1) / (blocks_want * 4);
    const int64_t blocks = (B + rows_per_wave * 4 - 1) / (rows_per_wave * 4);
    const int n_slots = 2 * n_ks;
    const bool vec = aligned16(items) && ldi % 4 == 0;
    return launch_with_partial_sums("list_diversity", blocks, n_slots, sums, stream, [&](double *part) {
#define NGCF_LIST_DIV_LAUNCH(NB_, VEC_)                                                                                           \
    list_diversity_kernel<NB_, VEC_><<<dim3((unsigned)blocks), 256, 0, stream>>>(top_idx, ld, B, k_used, items, ldi, n_items, D, n_ks, ks, \
                                                                                rows_per_wave, per_user, part, status)
        if (k_used <= 32) {
            if (vec) NGCF_LIST_DIV_LAUNCH(1, true); else NGCF_LIST_DIV_LAUNCH(1, false);
        } else {
            if (vec) NGCF_LIST_DIV_LAUNCH(2, true); else NGCF_LIST_DIV_LAUNCH(2, false);
        }
#undef NGCF_LIST_DIV_LAUNCH
    });
}
