// Candidate-list evaluation, the reference's test protocol (experiment.py:66-119) for T cases x C candidates in one launch: the
// scores of one user against its C candidate items, the position of the held-out item (column 0) among them, and from these
// HR@hit_k, NDCG@ks, the Test-BPR of bprloss.py:15-22 and |s_0 - rating| - no forward, no mm, no topk, no read-back per case
// (DESIGN 4.3).
#include "cand_device.h"

// ---------------------------------------------------------------------------------------------
// Mapping.  A wave owns a case; a workgroup = 4 waves with nothing shared but the final partial sums.  The wave stages the user
// row in LDS once (zero-padded to whole quads), then takes 8 candidates per step: each 16-lane group two of them, lane s of the
// group the quads q = s, s + 16, ... of the row (quad q = elements 4q..4q+3), a float4 load where the item rows are 16-byte
// aligned, four dword loads (or fewer, at the row's end) where not - the swept SpMM's lanes-per-entry shape.  The kernel is bound
// by these gathers: T x C rows of D floats against 5 VALU ops per loaded float.
//
// Score bits.  s = <u, item> is: per lane one ascending fmaf chain from 0 over the lane's quads (elements past D enter as 0 in
// both load forms), then an xor butterfly (8, 4, 2, 1) over the 16 lanes.  Which lane adds what depends on D alone, so a (user
// row, item row) pair gives the same bits in every case, column, launch shape and alignment; duplicated candidates tie exactly.
// The quad loads, the chain and the butterfly are cand_device.h's, which sample_hard.hip shares.
//
// Per case, from the C scores and squared item norms in LDS: position = number of columns j >= 1 whose key (float_key: NaN above
// +inf) is above column 0's - column 0 is the lowest column, so it wins every tie (the order of ngcf_topk_rows_f32); the BPR terms
// in column order.  Every id of a case is checked before any row of it is loaded; a case with a bad id sets *status, adds nothing
// and gets position -1 (its score row: NaN).
//
// Sums.  A wave adds its cases (t = wave, wave + n_waves, ...) in fp64 in that order (lane 0, into the wave's 12 LDS words); the 4 waves of a workgroup are
// added in wave order into the workgroup's partial; one workgroup adds the partials in order into `sums`.  No float atomics: the
// same call gives the same bits every time.  The grid depends on T, so a case set evaluated in chunks groups its additions
// differently: hits and cases are integers and exact either way, NDCG / BPR / |err| agree to fp64 rounding (1e-12 relative).
// ---------------------------------------------------------------------------------------------
#define NGCF_CAND_CMAX 1024
#define NGCF_CAND_KS 8
#define NGCF_CAND_WAVES 4
#define NGCF_CAND_SLOTS (NGCF_CAND_KS + 4)
// NGCF_CAND_LDS_FLOATS (cand_device.h), per wave: a user row that with 2 C floats exceeds it is read from global memory instead

namespace {

struct CandParams {                         // by value: stays in the kernarg segment
    int n_ks, hit_k, user_repeat;
    int ks[NGCF_CAND_KS];
    float weight_decay, batch_size;
};

// LDS floats of one wave: the user row (whole quads), C scores, C squared norms; a multiple of 4, so every wave's row is 16-byte aligned
__host__ __device__ inline int cand_wave_floats(int Dp, int C) { return Dp + ((2 * C + 3) & ~3); }

template <bool VEC, bool ULDS>
__global__ __launch_bounds__(64 * NGCF_CAND_WAVES, 4) void eval_candidates_kernel(
    const float *__restrict__ users, int64_t ldu, int64_t n_user_rows, const float *__restrict__ items, int64_t ldi, int64_t n_items,
    int D, const int64_t *__restrict__ user_ids, const int64_t *__restrict__ cand, int64_t ldc, int64_t T, int C,
    const float *__restrict__ ratings, CandParams prm, float *__restrict__ scores, int32_t *__restrict__ position,
    double *__restrict__ part, int32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) float cand_lds[];
    __shared__ double sh[NGCF_CAND_WAVES][NGCF_CAND_SLOTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & 15, grp = lane >> 4;
    const int Dp = (D + 3) & ~3, n_quads = Dp >> 2;
    float *my = cand_lds + (size_t)wave * cand_wave_floats(ULDS ? Dp : 0, C);
    float *su = my;                                              // [Dp] the user row (ULDS)
    float *sc = my + (ULDS ? Dp : 0);                            // [C] scores
    float *sn = sc + C;                                          // [C] squared item norms

    double *acc = sh[wave];                                      // the wave's running sums; lane 0 alone touches them (no registers held)
    if (lane < NGCF_CAND_SLOTS) acc[lane] = 0.0;
    wave_lds_sync();

    const int64_t n_waves = (int64_t)gridDim.x * NGCF_CAND_WAVES;
    for (int64_t t = (int64_t)blockIdx.x * NGCF_CAND_WAVES + wave; t < T; t += n_waves) {
        // every id of the case, before any row is loaded
        const int64_t r = user_ids[t];
        const int64_t *cl = cand + t * ldc;
        bool bad = r < 0 || r >= n_user_rows;
        for (int j = lane; j < C; j += 64) {
            const int64_t id = cl[j];
            bad = bad || id < 0 || id >= n_items;
        }
        if (__any(bad)) {                                        // wave-uniform
            if (lane == 0) {
                atomicOr(status, 1);
                if (position) position[t] = -1;
            }
            if (scores)
                for (int j = lane; j < C; j += 64) scores[t * C + j] = __int_as_float(0x7fc00000);
            continue;
        }
        const float *urow = users + r * ldu;
        float uu = 0.f;
        for (int e = lane; e < Dp; e += 64) {
            const float v = e < D ? urow[e] : 0.f;
            if (ULDS) su[e] = v;
            uu = fmaf(v, v, uu);
        }
        uu = wave_sum(uu);
        wave_lds_sync();

        for (int c0 = 0; c0 < C; c0 += 8) {
            const int ca = c0 + grp, cb = c0 + 4 + grp;
            const float *ra = items + (ca < C ? cl[ca] : cl[0]) * ldi;      // a group past C works on column 0 and drops the result
            const float *rb = items + (cb < C ? cl[cb] : cl[0]) * ldi;
            float sa = 0.f, sb = 0.f, na = 0.f, nb = 0.f;
#pragma unroll 2
            for (int q = sub; q < n_quads; q += 16) {
                const float4 x = cand_quad<VEC>(ra, q, D), y = cand_quad<VEC>(rb, q, D);
                const float4 u = ULDS ? *reinterpret_cast<const float4 *>(su + 4 * q) : cand_quad<false>(urow, q, D);
                sa = cand_fma4(u, x, sa); sb = cand_fma4(u, y, sb);
                na = cand_fma4(x, x, na); nb = cand_fma4(y, y, nb);
            }
            sa = group16_sum(sa); sb = group16_sum(sb);
            na = group16_sum(na); nb = group16_sum(nb);
            if (sub == 0) {
                if (ca < C) {
                    sc[ca] = sa; sn[ca] = na;
                    if (scores) scores[t * C + ca] = sa;
                }
                if (cb < C) {
                    sc[cb] = sb; sn[cb] = nb;
                    if (scores) scores[t * C + cb] = sb;
                }
            }
        }

        wave_lds_sync();
        // position of column 0 and the BPR terms of bprloss.py:15-22 on (u x user_repeat, item[cand_0], item[cand_1.., cand_1])
        const float s0 = sc[0];
        const uint32_t k0 = float_key(s0);
        int above = 0;
        double nl = 0.0, sq = 0.0;
        for (int j = lane; j < C; j += 64) {
            if (j >= 1 && float_key(sc[j]) > k0) ++above;
            if (C >= 2) {
                const int n = j + 1 < C ? j + 1 : 1;             // experiment.py:96-97: cat(pos[1:], pos[1:][:1])
                nl -= (double)log_sigmoid(fabsf(s0) - fabsf(sc[n]));
                sq += (double)sn[n];
            }
        }
        above = wave_sum(above);
        nl = wave_sum(nl);
        sq = wave_sum(sq) + (double)prm.user_repeat * (double)uu + (double)sn[0];
        if (lane == 0) {
            if (position) position[t] = above;
            if (above < prm.hit_k) acc[0] += 1.0;
            const double gain = 1.0 / log2((double)above + 2.0);
#pragma unroll
            for (int q = 0; q < NGCF_CAND_KS; ++q)
                if (q < prm.n_ks && above < prm.ks[q]) acc[1 + q] += gain;
            acc[NGCF_CAND_KS + 1] += (nl + (double)prm.weight_decay * sq) / (double)prm.batch_size;
            if (ratings) acc[NGCF_CAND_KS + 2] += fabs((double)s0 - (double)ratings[t]);
            acc[NGCF_CAND_KS + 3] += 1.0;
        }
        wave_lds_sync();                                        // the next case overwrites the region
    }
    __syncthreads();
    if (threadIdx.x < NGCF_CAND_SLOTS) {
        double a = 0.0;
        for (int w = 0; w < NGCF_CAND_WAVES; ++w) a += sh[w][threadIdx.x];
        part[(int64_t)blockIdx.x * NGCF_CAND_SLOTS + threadIdx.x] = a;
    }
}

// sums = [hits, ndcg@ks[0..n_ks), bpr, |err|, cases] += the workgroups' partials (slots [hits, ndcg x 8, bpr, |err|, cases]) in order
__global__ __launch_bounds__(64) void eval_candidates_finish_kernel(const double *__restrict__ part, int n_blocks, int n_ks,
                                                                    double *__restrict__ sums)
{
    const int s = threadIdx.x;
    if (s >= n_ks + 4) return;
    const int slot = s <= n_ks ? s : s + (NGCF_CAND_KS - n_ks);
    double a = 0.0;
    for (int b = 0; b < n_blocks; ++b) a += part[(int64_t)b * NGCF_CAND_SLOTS + slot];
    sums[s] += a;
}

}  // namespace

extern "C" int ngcf_eval_candidates_f32(const float *users, int64_t ldu, int64_t n_user_rows, const float *items, int64_t ldi,
                                        int64_t n_items, int D, const int64_t *user_ids, const int64_t *cand, int64_t ldc, int64_t T,
                                        int C, const float *ratings, const int32_t *ks_host, int n_ks, int hit_k, float weight_decay,
                                        float batch_size, int user_repeat, float *scores, int32_t *position, double *sums,
                                        int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (C < 1 || C > NGCF_CAND_CMAX) return fail(NGCF_ERR_ARG, "eval_candidates: C=%d candidates outside [1, %d]", C, NGCF_CAND_CMAX);
    if (n_ks < 0 || n_ks > NGCF_CAND_KS || (n_ks > 0 && !ks_host))
        return fail(NGCF_ERR_ARG, "eval_candidates: between 0 and %d cut-offs", NGCF_CAND_KS);
    if (hit_k < 1 || hit_k > C)
        return fail(NGCF_ERR_ARG, "selected index k out of range (hit_k=%d, row length %d)", hit_k, C);
    CandParams prm = {};
    for (int q = 0; q < n_ks; ++q) {
        if (ks_host[q] < 1 || ks_host[q] > C)
            return fail(NGCF_ERR_ARG, "selected index k out of range (k=%d, row length %d)", ks_host[q], C);
        prm.ks[q] = ks_host[q];
    }
    if (user_repeat != 1 && user_repeat != C)
        return fail(NGCF_ERR_ARG, "eval_candidates: user_repeat=%d is neither 1 nor C=%d", user_repeat, C);
    if (T < 0 || n_user_rows < 0 || n_items < 0 || D < 1 || ldu < D || ldi < D || ldc < C || !(batch_size != 0.f))
        return fail(NGCF_ERR_ARG, "eval_candidates: bad argument");
    if (T == 0) return NGCF_OK;
    if (!users || !items || !user_ids || !cand || !sums || !status) return fail(NGCF_ERR_ARG, "eval_candidates: null argument");
    prm.n_ks = n_ks;
    prm.hit_k = hit_k;
    prm.user_repeat = user_repeat;
    prm.weight_decay = weight_decay;
    prm.batch_size = batch_size;

    const int Dp = (D + 3) & ~3;
    const bool ulds = (int64_t)Dp + 2 * C <= NGCF_CAND_LDS_FLOATS;
    const bool vec = aligned16(items) && ldi % 4 == 0;
    const size_t lds = (size_t)NGCF_CAND_WAVES * cand_wave_floats(ulds ? Dp : 0, C) * sizeof(float);
    // as many workgroups as stay resident (4 waves per SIMD by the kernel's registers, or the LDS of a CU), the cases strided over them
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(16 / NGCF_CAND_WAVES, (160 * 1024) / (int64_t)(lds + 512)));
    const int blocks = (int)std::min<int64_t>((T + NGCF_CAND_WAVES - 1) / NGCF_CAND_WAVES, 256 * per_cu);
    void *part = nullptr;
    HIP_TRY(hipMallocAsync(&part, sizeof(double) * (size_t)blocks * NGCF_CAND_SLOTS, stream));
#define NGCF_CAND_LAUNCH(VEC_, ULDS_)                                                                                             \
    eval_candidates_kernel<VEC_, ULDS_><<<dim3((unsigned)blocks), 64 * NGCF_CAND_WAVES, lds, stream>>>(                           \
        users, ldu, n_user_rows, items, ldi, n_items, D, user_ids, cand, ldc, T, C, ratings, prm, scores, position,               \
        static_cast<double *>(part), status)
    if (vec && ulds) NGCF_CAND_LAUNCH(true, true);
    else if (vec) NGCF_CAND_LAUNCH(true, false);
    else if (ulds) NGCF_CAND_LAUNCH(false, true);
    else NGCF_CAND_LAUNCH(false, false);
#undef NGCF_CAND_LAUNCH
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        eval_candidates_finish_kernel<<<1, 64, 0, stream>>>(static_cast<double *>(part), blocks, n_ks, sums);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(part, stream);
    if (e != hipSuccess) return fail(NGCF_ERR_HIP, "eval_candidates: kernel launch failed: %s", hipGetErrorString(e));
    return NGCF_OK;
}
