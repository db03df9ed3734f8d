// Hard negatives, dynamic negative sampling for BPR training: for T cases in one launch, draw m items the case's user has no
// stored interaction with (the draw of ngcf_sample_unseen), score them against the user's row (the score bits of
// ngcf_eval_candidates_f32) and keep the best-scoring one.  One item per case is written; the m candidates and their scores live
// in registers.  The composition sample_unseen -> eval_candidates(scores) -> argmax gives the same bits and is the tests' oracle.
#include "cand_device.h"
#include "sample_device.h"

// ---------------------------------------------------------------------------------------------
// Mapping.  A wave owns a case; a workgroup = 4 waves that share nothing; the cases are strided over a capped grid.
//
// Draw.  m <= 64 is one chunk of sample_device.h's map: lane j ends up with candidate c_j, the map's entries stay in the lanes, no
// LDS history.  A seen row of up to 64 ids is held in the lanes, a longer one is searched where it lies.
//
// Score.  The wave stages the user row in its LDS region once (zero-padded to whole quads; a row longer than
// NGCF_CAND_LDS_FLOATS is read from global memory instead), then takes 8 candidates per step, each 16-lane group two of them,
// with cand_device.h's quads, chain and butterfly: T x m row gathers of D floats bound the kernel, as they do the candidate
// evaluation.  A group past m works on candidate 0 and drops the result.
//
// Select.  Every lane keeps the best (float_key(score) + 1) << 6 | (63 - slot) of its group's candidates as one unsigned 64-bit
// word - 0: none yet -, so the largest word is the largest score under float_key (NaN above +inf) and, among equal keys, the lowest
// slot; the four groups are combined with an xor butterfly (16, 32).  float_key is a bijection on the bits, so the winning
// score's bits come back out of the word.
// ---------------------------------------------------------------------------------------------
#define NGCF_SAMPLE_HARD_WAVES 4

namespace {

__device__ inline uint64_t hard_word(float score, int slot) { return (((uint64_t)float_key(score) + 1) << 6) | (uint64_t)(63 - slot); }

__device__ inline uint64_t hard_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

template <bool VEC, bool ULDS>
__global__ __launch_bounds__(64 * NGCF_SAMPLE_HARD_WAVES) void sample_hard_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int64_t col_offset, int64_t n_rows, int64_t n_items,
    const float *__restrict__ users, int64_t ldu, const float *__restrict__ items, int64_t ldi, int D,
    const int64_t *__restrict__ user_ids, int64_t T, int64_t case_offset, int m, uint64_t seed, int64_t *__restrict__ neg,
    float *__restrict__ score, int32_t *__restrict__ slot, int32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) float hard_lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), sub = lane & 15, grp = lane >> 4;
    const int Dp = (D + 3) & ~3, n_quads = Dp >> 2;
    float *su = hard_lds + (size_t)wave * (ULDS ? Dp : 0);       // [Dp] the user row (ULDS)

    const int64_t n_waves = (int64_t)gridDim.x * NGCF_SAMPLE_HARD_WAVES;
    for (int64_t t = (int64_t)blockIdx.x * NGCF_SAMPLE_HARD_WAVES + wave; t < T; t += n_waves) {
        // the user id is checked before any row is loaded; the drawn items lie in [0, n_items) by construction
        const int64_t u = user_ids[t];
        int64_t lo, len, n;
        const int bad = sample_row(rowptr, n_rows, n_items, u, m, lo, len, n);     // the same in every lane
        if (bad) {
            if (lane == 0) {
                atomicOr(status, bad);
                neg[t] = -1;
                if (score) score[t] = __int_as_float(0x7fc00000);
                if (slot) slot[t] = -1;
            }
            continue;
        }
        const int32_t *seen = colidx + lo;
        int K, V;
        const int item = sample_chunk(sample_case_key(seed, case_offset + t), n, 0, m, lane, seen, len, col_offset,
                                      sample_seen_lanes(seen, len, col_offset, lane), nullptr, nullptr, K, V);   // lane j < m: c_j

        const float *urow = users + u * ldu;
        if (ULDS) {
            for (int e = lane; e < Dp; e += 64) su[e] = e < D ? urow[e] : 0.f;
            wave_lds_sync();
        }

        uint64_t best = 0;
        for (int c0 = 0; c0 < m; c0 += 8) {
            const int ca = c0 + grp, cb = c0 + 4 + grp;
            const float *ra = items + (int64_t)__shfl(item, ca < m ? ca : 0) * ldi;
            const float *rb = items + (int64_t)__shfl(item, cb < m ? cb : 0) * ldi;
            float sa = 0.f, sb = 0.f;
#pragma unroll 2
            for (int q = sub; q < n_quads; q += 16) {
                const float4 x = cand_quad<VEC>(ra, q, D), y = cand_quad<VEC>(rb, q, D);
                const float4 uq = ULDS ? *reinterpret_cast<const float4 *>(su + 4 * q) : cand_quad<false>(urow, q, D);
                sa = cand_fma4(uq, x, sa);
                sb = cand_fma4(uq, y, sb);
            }
            sa = group16_sum(sa);
            sb = group16_sum(sb);
            if (ca < m) best = hard_max(best, hard_word(sa, ca));
            if (cb < m) best = hard_max(best, hard_word(sb, cb));
        }
        best = hard_max(best, __shfl_xor(best, 16));
        best = hard_max(best, __shfl_xor(best, 32));

        const int win = 63 - (int)(best & 63);                    // slot 0 always runs, so best != 0
        const int64_t win_item = __shfl(item, win);
        if (lane == 0) {
            const uint32_t key = (uint32_t)((best >> 6) - 1);
            neg[t] = win_item;
            if (score) score[t] = __uint_as_float((key & 0x80000000u) ? key ^ 0x80000000u : ~key);
            if (slot) slot[t] = win;
        }
        if (ULDS) wave_lds_sync();                               // the next case overwrites the region
    }
}

}  // namespace

extern "C" int ngcf_sample_hard_f32(const int64_t *seen_rowptr, const int32_t *seen_colidx, int64_t col_offset, int64_t n_rows,
                                    int64_t n_items, const float *users, int64_t ldu, int64_t n_user_rows, const float *items,
                                    int64_t ldi, int64_t n_item_rows, int D, const int64_t *user_ids, int64_t T, int64_t case_offset,
                                    int m, uint64_t seed, int64_t *neg, float *score, int32_t *slot, int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (m < 1 || m > NGCF_SAMPLE_HARD_M_MAX) return fail(NGCF_ERR_ARG, "sample_hard: m=%d outside [1, %d]", m, NGCF_SAMPLE_HARD_M_MAX);
    if (int e = sample_check_items("sample_hard", n_items)) return e;
    if (n_item_rows < n_items)
        return fail(NGCF_ERR_ARG, "sample_hard: %lld item rows for n_items=%lld", (long long)n_item_rows, (long long)n_items);
    if (n_rows < 0 || n_user_rows < n_rows)
        return fail(NGCF_ERR_ARG, "sample_hard: %lld user rows for n_rows=%lld seen rows", (long long)n_user_rows, (long long)n_rows);
    if (D < 1) return fail(NGCF_ERR_ARG, "sample_hard: D=%d below 1", D);
    if (T < 0 || ldu < D || ldi < D) return fail(NGCF_ERR_ARG, "sample_hard: bad argument");
    if (T == 0) return NGCF_OK;
    if (int e = sample_check_pointers("sample_hard", {seen_rowptr, seen_colidx, users, items, user_ids, neg, status})) return e;

    const int Dp = (D + 3) & ~3;
    const bool ulds = Dp <= NGCF_CAND_LDS_FLOATS;
    const bool vec = aligned16(items) && ldi % 4 == 0;
    const size_t lds = ulds ? (size_t)NGCF_SAMPLE_HARD_WAVES * Dp * sizeof(float) : 0;      // at most 64 KiB
    const int blocks = sample_blocks(T, NGCF_SAMPLE_HARD_WAVES);
#define NGCF_HARD_LAUNCH(VEC_, ULDS_)                                                                                              \
    sample_hard_kernel<VEC_, ULDS_><<<dim3((unsigned)blocks), 64 * NGCF_SAMPLE_HARD_WAVES, lds, stream>>>(                         \
        seen_rowptr, seen_colidx, col_offset, n_rows, n_items, users, ldu, items, ldi, D, user_ids, T, case_offset, m, seed, neg,  \
        score, slot, status)
    if (vec && ulds) NGCF_HARD_LAUNCH(true, true);
    else if (vec) NGCF_HARD_LAUNCH(true, false);
    else if (ulds) NGCF_HARD_LAUNCH(false, true);
    else NGCF_HARD_LAUNCH(false, false);
#undef NGCF_HARD_LAUNCH
    LAUNCH_CHECK();
    return NGCF_OK;
}
