// Exact held-out positions over the full catalogue: the 0-based index of every held-out item in its user's full
// sorted list of eligible items, and MRR / MAP / AUC / NDCG / Recall@K for any K from those positions.  The scoring pass is
// rank_topk_kernel's (rank.hip): fp32 MFMA tiles, no score is ever stored.  The streaming selection is replaced by a streaming
// count: per user the held-out (key, item) pairs lie sorted in LDS, every computed score finds its gap among them by binary search
// and bumps an integer counter, and a prefix sum over the gaps gives the positions.  The (key, item) order, the padding pair,
// the item split, the row search and the fixed-order sums are rank_topk's by construction (rank_device.h); the score-tile walk of
// pos_scan_kernel is restated from rank_topk_kernel and held to it bit for bit by the tests (DESIGN 4.3.15 has the reason).
#include "rank_device.h"
#include "dd_log2.h"

// ---------------------------------------------------------------------------------------------
// Launches of ngcf_rank_positions_f32 (all on the caller's stream, nothing is read back):
//   pos_prep_kernel    one workgroup: batch rows with a non-empty truth row become VIRTUAL ROWS of at most CAP = NGCF_POS_CAP held-out
//                      entries each (a longer truth row is cut into chunks; each chunk is ranked against the whole catalogue, so
//                      its positions are already global).  Users with an empty truth row get no virtual row and cost no scoring.
//   pos_truth_kernel   a wave per virtual row, a lane per entry: range check, exclusion check (binary search in the user's
//                      exclusion row), the entry's own score as one ascending-k fmaf chain from 0 on the VALU - the bits of the MFMA
//                      tile, as recommend_topk_kernel (ops.hip) shows -, then the wave sorts its (key, item, source) triples by
//                      counting across lanes.  Entries that are out of range or excluded sort last as padding.
//   pos_scan_kernel    rank_topk_kernel's tiling (UT = 64 virtual rows x IT = 128 items per tile, K through LDS in chunks of 32, wave w
//                      = items [32w, 32w+32) of the tile).  A score that sorts after the row's last valid entry changes no position
//                      and is dropped after one compare (rank_topk's threshold test); any other one is a lower-bound search in the
//                      row's sorted pairs (LDS rows of CAP + 1 words: lanes of different users hit different banks) and one
//                      integer LDS atomic on the gap it falls into.  The workgroup adds its gap counts into global memory with integer
//                      atomics, so item splits (blockIdx.y) simply add up.
//   pos_finish_kernel  a wave per virtual row: inclusive prefix sum of the gaps across lanes; the held-out item itself lands in
//                      its own gap, hence position = prefix - 1.  Padding entries get -1.
// LDS of the scan: 25 KiB of tiles + 3 x 64 x 65 words = 49 KiB of pairs and counters: two workgroups per CU (160 KiB).
// ---------------------------------------------------------------------------------------------
#define NGCF_POS_CAP NGCF_RANK_POS_CAP
#define NGCF_POS_KS 8

namespace {

__device__ inline int64_t pos_clamp(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

struct PosWs {                 // the workspace, cut up on the host
    int32_t *n_vrows;          // [1] virtual rows of this call (<= vcap)
    int64_t *v_row, *v_e0;     // [vcap] user row, first truth entry
    int32_t *v_len, *v_nval;   // [vcap] entries of the chunk, valid ones among them
    uint32_t *s_key;           // [vcap][CAP] sorted keys
    int32_t *s_idx, *s_src;    // [vcap][CAP] sorted items, and which entry of the chunk each one is
    uint32_t *gap;             // [vcap][CAP] eligible items that fall right before sorted entry j
};

__global__ __launch_bounds__(1024) void pos_prep_kernel(const int64_t *__restrict__ user_ids, int64_t n_user_rows, int64_t B,
                                                        const int64_t *__restrict__ t_rowptr, int64_t n_truth, int64_t vcap, PosWs ws,
                                                        int32_t *status)
{
    constexpr int CAP = NGCF_POS_CAP;
    __shared__ int64_t ssum[1024];
    const int tid = threadIdx.x;
    const int64_t per = (B + 1023) / 1024;
    const int64_t b_lo = tid * per < B ? tid * per : B, b_hi = b_lo + per < B ? b_lo + per : B;
    int64_t cnt = 0;
    for (int64_t b = b_lo; b < b_hi; ++b) {
        const int64_t r = user_ids ? user_ids[b] : b;
        if (r < 0 || r >= n_user_rows) {
            atomicOr(status, 1);
            continue;
        }
        const int64_t e0 = pos_clamp(t_rowptr[r], 0, n_truth), e1 = pos_clamp(t_rowptr[r + 1], e0, n_truth);
        cnt += (e1 - e0 + CAP - 1) / CAP;
    }
    ssum[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int64_t t = tid >= off ? ssum[tid - off] : 0;
        __syncthreads();
        ssum[tid] += t;
        __syncthreads();
    }
    int64_t v = ssum[tid] - cnt;
    const int64_t total = ssum[1023];
    if (tid == 0) {
        *ws.n_vrows = (int32_t)(total < vcap ? total : vcap);
        if (total > vcap) atomicOr(status, 4);
    }
    for (int64_t b = b_lo; b < b_hi; ++b) {
        const int64_t r = user_ids ? user_ids[b] : b;
        if (r < 0 || r >= n_user_rows) continue;
        const int64_t e0 = pos_clamp(t_rowptr[r], 0, n_truth), e1 = pos_clamp(t_rowptr[r + 1], e0, n_truth);
        for (int64_t e = e0; e < e1 && v < vcap; e += CAP, ++v) {
            ws.v_row[v] = r;
            ws.v_e0[v] = e;
            ws.v_len[v] = (int32_t)(e1 - e < CAP ? e1 - e : CAP);
        }
    }
}

__global__ __launch_bounds__(256) void pos_truth_kernel(const float *__restrict__ users, int64_t ldu, const float *__restrict__ items,
                                                        int64_t ldi, int64_t n_items, int D, const int32_t *__restrict__ t_colidx,
                                                        int64_t t_off, const int64_t *__restrict__ x_rowptr,
                                                        const int32_t *__restrict__ x_colidx, int64_t x_off, int vec_items, PosWs ws, int32_t *status)
{
    constexpr int CAP = NGCF_POS_CAP;
    static_assert(CAP == 64, "one lane per entry of a virtual row");
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= *ws.n_vrows) return;                               // the whole wave
    const int64_t r = ws.v_row[v], e0 = ws.v_e0[v];
    const int len = ws.v_len[v];
    bool valid = false;
    uint32_t key = kPadKey;
    int32_t idx = kPadIdx;
    if (lane < len) {
        const int64_t c = (int64_t)t_colidx[e0 + lane] - t_off;
        if (c < 0 || c >= n_items) {
            atomicOr(status, 2);                                  // never used as an index
        } else {
            const bool excluded = x_rowptr && row_has(x_colidx, x_rowptr[r], x_rowptr[r + 1], x_off, c);
            if (!excluded) {
                const float *ur = users + r * ldu, *ir = items + c * ldi;
                float acc = 0.f;
                int k = 0;
                if (vec_items) {                                  // 16-byte item rows: the chain is the same, the loads are wider
                    for (; k + 4 <= D; k += 4) {
                        const float4 x = *reinterpret_cast<const float4 *>(ir + k);
                        acc = fmaf(x.x, ur[k], acc);
                        acc = fmaf(x.y, ur[k + 1], acc);
                        acc = fmaf(x.z, ur[k + 2], acc);
                        acc = fmaf(x.w, ur[k + 3], acc);
                    }
                }
                for (; k < D; ++k) acc = fmaf(ir[k], ur[k], acc);
                valid = true;
                key = float_key(acc);
                idx = (int32_t)c;
            }
        }
    }
    int rank = 0;                                               // triples before this lane's: (key desc, item asc, lane asc) is a total order
    for (int j = 0; j < 64; ++j) {
        const uint32_t kj = (uint32_t)__shfl((int)key, j);
        const int32_t ij = __shfl(idx, j);
        rank += pair_before(kj, ij, key, idx) || (kj == key && ij == idx && j < lane);
    }
    ws.s_key[v * CAP + rank] = key;
    ws.s_idx[v * CAP + rank] = idx;
    ws.s_src[v * CAP + rank] = lane;
    ws.gap[v * CAP + lane] = 0u;
    const int nval = __popcll(__ballot(valid));
    if (lane == 0) ws.v_nval[v] = nval;
}

__global__ __launch_bounds__(256) void pos_scan_kernel(const float *__restrict__ users, int64_t ldu, const float *__restrict__ items,
                                                       int64_t ldi, int64_t n_items, int D, int64_t split_items,
                                                       const int64_t *__restrict__ x_rowptr, const int32_t *__restrict__ x_colidx,
                                                       int64_t x_off, PosWs ws)
{
    constexpr int UB = 2, UT = 32 * UB, IT = kRankIT, TK = kRankTK, SLD = TK + 1, CAP = NGCF_POS_CAP, TLD = CAP + 1;
    constexpr int NI = IT * TK / 256, NU = UT * TK / 256;
    __shared__ float sI[IT * SLD];
    __shared__ float sU[UT * SLD];
    __shared__ uint32_t thk[UT], exm[UT * (IT / 32)];
    __shared__ int32_t thi[UT], nv[UT];
    __shared__ int64_t srow[UT];
    extern __shared__ uint32_t pos_dyn[];
    uint32_t *tk = pos_dyn;                                              // [UT][TLD] sorted keys
    int32_t *ti = reinterpret_cast<int32_t *>(pos_dyn + UT * TLD);       // [UT][TLD] sorted items
    uint32_t *gp = pos_dyn + 2 * UT * TLD;                               // [UT][TLD] gap counters

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n_v = *ws.n_vrows;
    const int64_t v0 = (int64_t)blockIdx.x * UT;
    if (v0 >= n_v) return;                                               // the whole workgroup
    const int64_t i_begin = (int64_t)blockIdx.y * split_items;
    const int64_t i_end = i_begin + split_items < n_items ? i_begin + split_items : n_items;

    for (int p = tid; p < UT * CAP; p += 256) {
        const int u = p / CAP, j = p % CAP;
        const bool ok = v0 + u < n_v;
        tk[u * TLD + j] = ok ? ws.s_key[(v0 + u) * CAP + j] : kPadKey;
        ti[u * TLD + j] = ok ? ws.s_idx[(v0 + u) * CAP + j] : kPadIdx;
        gp[u * TLD + j] = 0u;
    }
    int64_t cur = 0, cur_end = 0;                                        // exclusion cursor of virtual row `tid` (threads tid < UT)
    if (tid < UT) {
        const int64_t v = v0 + tid;
        const int n = v < n_v ? ws.v_nval[v] : 0;
        const int64_t r = n > 0 ? ws.v_row[v] : -1;                       // a row with no valid entry has nothing to count
        srow[tid] = r;
        nv[tid] = n;
        thk[tid] = n > 0 ? ws.s_key[v * CAP + n - 1] : kPadKey;
        thi[tid] = n > 0 ? ws.s_idx[v * CAP + n - 1] : kPadIdx;
        if (r >= 0 && x_rowptr) {
            cur = x_rowptr[r];
            cur_end = x_rowptr[r + 1];
        }
    }
    __syncthreads();

    const int n_chunks = (D + TK - 1) / TK;
    const int64_t n_tiles = (i_end - i_begin + IT - 1) / IT;
    const int64_t n_steps = n_tiles * n_chunks;
    float pI[NI], pU[NU];
    auto load = [&](int64_t s) {
        const int64_t i0 = i_begin + (s / n_chunks) * IT;
        const int k0 = (int)(s % n_chunks) * TK;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int f = tid + 256 * j, it = f / TK, kk = f % TK;
            const int64_t gi = i0 + it;
            pI[j] = (gi < i_end && k0 + kk < D) ? items[gi * ldi + k0 + kk] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int f = tid + 256 * j, ur = f / TK, kk = f % TK;
            const int64_t r = srow[ur];
            pU[j] = (r >= 0 && k0 + kk < D) ? users[r * ldu + k0 + kk] : 0.f;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int f = tid + 256 * j;
            sI[(f / TK) * SLD + f % TK] = pI[j];
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int f = tid + 256 * j;
            sU[(f / TK) * SLD + f % TK] = pU[j];
        }
    };

    if (n_steps > 0) load(0);
    int64_t step = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t i0 = i_begin + t * IT;
        // this tile's exclusion masks (the previous tile's counting is past the barrier that ended it)
        if (tid < UT) {
            uint32_t m[IT / 32] = {};
            while (cur < cur_end) {
                const int64_t c = (int64_t)x_colidx[cur] - x_off;
                if (c >= i0 + IT) break;
                if (c >= i0) m[(c - i0) >> 5] |= 1u << ((c - i0) & 31);
                ++cur;
            }
#pragma unroll
            for (int w = 0; w < IT / 32; ++w) exm[tid * (IT / 32) + w] = m[w];
        }
        f32x16 acc[UB];
#pragma unroll
        for (int ub = 0; ub < UB; ++ub)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ub][e] = 0.f;
        for (int c = 0; c < n_chunks; ++c, ++step) {
            __syncthreads();
            store();
            __syncthreads();
            if (step + 1 < n_steps) load(step + 1);          // next chunk (next tile's first one too) flies under the MFMAs
            const float *A = sI + (wave * 32 + (lane & 31)) * SLD + (lane >> 5);
            const float *Bu = sU + (lane & 31) * SLD + (lane >> 5);
#pragma unroll
            for (int s = 0; s < TK / 2; ++s) {
                const float a = A[2 * s];
#pragma unroll
                for (int ub = 0; ub < UB; ++ub)
                    acc[ub] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bu[ub * 32 * SLD + 2 * s], acc[ub], 0, 0, 0);
            }
        }
        __syncthreads();                                      // exclusion masks written
        // count: lane holds virtual row ub*32 + (lane&31), items 32*wave + (e&3) + 8*(e>>2) + 4*(lane>>5) of the tile
#pragma unroll
        for (int ub = 0; ub < UB; ++ub) {
            const int u = ub * 32 + (lane & 31);
            if (srow[u] < 0) continue;
            const uint32_t lk = thk[u];
            const int32_t li = thi[u];
            const int n = nv[u];
            const uint32_t *K = tk + u * TLD;
            const int32_t *I = ti + u * TLD;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int il = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                const int64_t gi = i0 + il;
                if (gi >= i_end || ((exm[u * (IT / 32) + (il >> 5)] >> (il & 31)) & 1u)) continue;
                const uint32_t key = float_key(acc[ub][e]);
                if (pair_before(lk, li, key, (int32_t)gi)) continue;      // after the last valid entry: no position changes
                int lo = 0, hi = n - 1;                                   // entries strictly before the item: at most n - 1 now
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (pair_before(K[mid], I[mid], key, (int32_t)gi)) lo = mid + 1; else hi = mid;
                }
                atomicAdd(&gp[u * TLD + lo], 1u);
            }
        }
        __syncthreads();                                      // the masks are rewritten by the next tile
    }

    for (int p = tid; p < UT * CAP; p += 256) {
        const int u = p / CAP, j = p % CAP;
        const uint32_t c = gp[u * TLD + j];
        if (c != 0u && v0 + u < n_v) atomicAdd(&ws.gap[(v0 + u) * CAP + j], c);
    }
}

__global__ __launch_bounds__(256) void pos_finish_kernel(PosWs ws, int64_t n_truth, int32_t *__restrict__ position)
{
    constexpr int CAP = NGCF_POS_CAP;
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= *ws.n_vrows) return;                               // the whole wave
    const int64_t e0 = ws.v_e0[v];
    const int len = ws.v_len[v], nval = ws.v_nval[v];
    uint32_t g = ws.gap[v * CAP + lane];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)g, off);
        if (lane >= off) g += t;
    }
    const int src = ws.s_src[v * CAP + lane];
    if (src >= 0 && src < len && e0 + src < n_truth) position[e0 + src] = lane < nval ? (int32_t)g - 1 : -1;
}

int64_t pos_vcap(int64_t B, int64_t n_truth) { return B + n_truth / NGCF_POS_CAP; }

int64_t pos_carve(PosWs *ws, char *base, int64_t vcap)
{
    constexpr int CAP = NGCF_POS_CAP;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        char *p = base ? base + o : nullptr;
        o += align_up(bytes, 256);
        return p;
    };
    char *p[9] = {take(4), take(vcap * 8), take(vcap * 8), take(vcap * 4), take(vcap * 4), take(vcap * CAP * 4), take(vcap * CAP * 4),
                  take(vcap * CAP * 4), take(vcap * CAP * 4)};
    if (ws) {
        ws->n_vrows = reinterpret_cast<int32_t *>(p[0]);
        ws->v_row = reinterpret_cast<int64_t *>(p[1]);
        ws->v_e0 = reinterpret_cast<int64_t *>(p[2]);
        ws->v_len = reinterpret_cast<int32_t *>(p[3]);
        ws->v_nval = reinterpret_cast<int32_t *>(p[4]);
        ws->s_key = reinterpret_cast<uint32_t *>(p[5]);
        ws->s_idx = reinterpret_cast<int32_t *>(p[6]);
        ws->s_src = reinterpret_cast<int32_t *>(p[7]);
        ws->gap = reinterpret_cast<uint32_t *>(p[8]);
    }
    return o;
}

}  // namespace

extern "C" int64_t ngcf_rank_positions_workspace_bytes(int64_t B, int64_t n_items, int D, int64_t n_truth)
{
    if (B < 0 || n_items < 1 || n_items >= ((int64_t)1 << 31) || D < 1 || n_truth < 0) return -1;
    if (B == 0) return 0;
    return pos_carve(nullptr, nullptr, pos_vcap(B, n_truth));
}

extern "C" int ngcf_rank_positions_f32(const float *users, int64_t ldu, const int64_t *user_ids, int64_t n_user_rows, int64_t B,
                                       const float *items, int64_t ldi, int64_t n_items, int D, const int64_t *truth_rowptr,
                                       const int32_t *truth_colidx, int64_t truth_col_offset, int64_t n_truth,
                                       const int64_t *excl_rowptr, const int32_t *excl_colidx, int64_t excl_col_offset,
                                       int32_t *position, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    constexpr int UT = 64, CAP = NGCF_POS_CAP;
    if (n_items < 1 || n_items >= ((int64_t)1 << 31)) return fail(NGCF_ERR_ARG, "rank_positions: n_items=%lld outside [1, 2^31)", (long long)n_items);
    if (B < 0 || n_user_rows < 0 || n_truth < 0 || D < 1) return fail(NGCF_ERR_ARG, "rank_positions: bad argument");
    if (B == 0) return NGCF_OK;
    if (!users || !items || !truth_rowptr || !position || !status || (n_truth > 0 && !truth_colidx) || ldu < D || ldi < D ||
        (excl_rowptr && !excl_colidx))
        return fail(NGCF_ERR_ARG, "rank_positions: bad argument");
    const int64_t vcap = pos_vcap(B, n_truth);
    const int64_t need = ngcf_rank_positions_workspace_bytes(B, n_items, D, n_truth);
    if (!workspace || workspace_bytes < need)
        return fail(NGCF_ERR_WORKSPACE, "rank_positions: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    // the item range is split when the batch alone cannot fill the chip: rank_topk's rule
    const int64_t user_tiles = (B + UT - 1) / UT, v_tiles = (vcap + UT - 1) / UT;
    const ItemSplit sp = rank_item_split(user_tiles, n_items);
    const int64_t splits = sp.splits, split_items = sp.split_items;
    if (vcap >= ((int64_t)1 << 31) || splits > 65535)
        return fail(NGCF_ERR_ARG, "rank_positions: batch too large");
    PosWs ws;
    pos_carve(&ws, static_cast<char *>(workspace), vcap);
    pos_prep_kernel<<<1, 1024, 0, stream>>>(user_ids, n_user_rows, B, truth_rowptr, n_truth, vcap, ws, status);
    LAUNCH_CHECK();
    const unsigned wave_blocks = (unsigned)((vcap + 3) / 4);
    pos_truth_kernel<<<wave_blocks, 256, 0, stream>>>(users, ldu, items, ldi, n_items, D, truth_colidx, truth_col_offset, excl_rowptr,
                                                      excl_colidx, excl_col_offset, (ldi & 3) == 0 && aligned16(items), ws, status);
    LAUNCH_CHECK();
    const int dyn = 3 * UT * (CAP + 1) * 4;
    HIP_TRY(allow_full_lds<pos_scan_kernel>(dyn));
    pos_scan_kernel<<<dim3((unsigned)v_tiles, (unsigned)splits), 256, dyn, stream>>>(users, ldu, items, ldi, n_items, D, split_items,
                                                                                    excl_rowptr, excl_colidx, excl_col_offset, ws);
    LAUNCH_CHECK();
    pos_finish_kernel<<<wave_blocks, 256, 0, stream>>>(ws, n_truth, position);
    LAUNCH_CHECK();
    return NGCF_OK;
}

// ---------------------------------------------------------------------------------------------
// Metrics from positions.  A workgroup covers 256 batch rows, wave w rows [64w, 64w + 64) one after the other; all lanes carry the
// same fp64 values.  The valid positions of a row are visited in ascending order by repeated selection of the smallest position above
// the previous one (a wave-wide minimum): rows of up to NGCF_RANK_POS_WAVE_ROW = 64 entries sit in registers, one per lane, longer
// rows re-read the entries past the 64th every round.  Duplicate ids of a truth row have equal positions and are visited once; -1
// (not eligible) and -2 (not ranked) are never selected: misses.  Sums: a wave adds its users in order, the workgroup its four waves
// in order, one workgroup the blocks in order (rank_metrics' scheme): bit-identical from run to run.  The 1/log2(rank + 2) terms take
// their log2 from dd_log2.h: correctly rounded, so a host oracle adding the same terms in the same order gets the same fp64 bits.
// ---------------------------------------------------------------------------------------------
namespace {

__global__ __launch_bounds__(256) void pos_metrics_kernel(const int32_t *__restrict__ position, int64_t B,
                                                          const int64_t *__restrict__ user_ids, int64_t n_user_rows,
                                                          const int64_t *__restrict__ t_rowptr, const int32_t *__restrict__ t_colidx,
                                                          int64_t n_truth, const int64_t *__restrict__ x_rowptr, int64_t n_items, int n_ks,
                                                          int ks0, int ks1, int ks2, int ks3, int ks4, int ks5, int ks6, int ks7,
                                                          double *__restrict__ per_user, double *__restrict__ part, int32_t *status)
{
    constexpr int NK = NGCF_POS_KS, NS = 4 + 4 * NK + 2;
    __shared__ double sh[4][NS];
    const int ks[NK] = {ks0, ks1, ks2, ks3, ks4, ks5, ks6, ks7};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b_base = (int64_t)blockIdx.x * 256 + wave * 64;
    const int n_out = 4 + 4 * n_ks;
    int64_t my_e0 = 0, my_e1 = 0, my_xl = 0;                    // lane i: the row of batch row b_base + i
    if (b_base + lane < B) {
        const int64_t r = user_ids ? user_ids[b_base + lane] : b_base + lane;
        if (r < 0 || r >= n_user_rows) {
            atomicOr(status, 1);
        } else {
            my_e0 = pos_clamp(t_rowptr[r], 0, n_truth);
            my_e1 = pos_clamp(t_rowptr[r + 1], my_e0, n_truth);
            my_xl = x_rowptr ? x_rowptr[r + 1] - x_rowptr[r] : 0;
        }
    }
    double acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0.0;
    for (int i = 0; i < 64; ++i) {
        const int64_t b = b_base + i;
        if (b >= B) break;                                      // the whole wave
        const int64_t e0 = shfl_i64(my_e0, i), e1 = shfl_i64(my_e1, i), xl = shfl_i64(my_xl, i);
        double v[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) v[s] = 0.0;
        if (e1 > e0) {
            int distinct = 0;                                   // |T|: the row is ascending
            for (int64_t e = e0 + lane; e < e1; e += 64) distinct += e == e0 || t_colidx[e] != t_colidx[e - 1];
            const int nt = wave_sum(distinct);
            const int32_t mine = e0 + lane < e1 ? position[e0 + lane] : -1;
            const double neg = (double)(n_items - xl - nt);     // E - T
            double rr = 0.0, ap = 0.0, dcg = 0.0, below = 0.0, dcg_k[NK] = {};
            int hits[NK] = {};
            int prev = -1, j = 0;
            for (;;) {
                int m = 0x7fffffff;
                if (mine > prev) m = mine;
                for (int64_t e = e0 + 64 + lane; e < e1; e += 64) {
                    const int32_t p = position[e];
                    if (p > prev && p < m) m = p;
                }
                m = wave_min(m);
                if (m == 0x7fffffff) break;
                const double g = 1.0 / ddm::log2_cr((double)m + 2.0);
                if (j == 0) rr = 1.0 / ((double)m + 1.0);
                ap += (double)(j + 1) / ((double)m + 1.0);
                dcg += g;
                below += neg - (double)(m - j);
#pragma unroll
                for (int q = 0; q < NK; ++q) {
                    if (q < n_ks && m < ks[q]) { hits[q] += 1; dcg_k[q] += g; }
                }
                prev = m;
                ++j;
            }
            double idcg = 0.0, idcg_k[NK] = {};
            for (int jj = 0; jj < nt; ++jj) {
                const double g = 1.0 / ddm::log2_cr((double)jj + 2.0);
                idcg += g;
#pragma unroll
                for (int q = 0; q < NK; ++q)
                    if (q < n_ks && jj < ks[q]) idcg_k[q] += g;
            }
            v[0] = rr;
            v[1] = ap / (double)nt;
            v[2] = dcg / idcg;
            if (neg > 0.0) {
                v[3] = below / ((double)nt * neg);
                v[NS - 1] = 1.0;
            }
#pragma unroll
            for (int q = 0; q < NK; ++q) {
                if (q < n_ks) {
                    v[4 + 4 * q + 0] = (double)hits[q] / (double)nt;
                    v[4 + 4 * q + 1] = dcg_k[q] / idcg_k[q];
                    v[4 + 4 * q + 2] = (double)hits[q] / (double)ks[q];
                    v[4 + 4 * q + 3] = hits[q] > 0 ? 1.0 : 0.0;
                }
            }
            v[NS - 2] = 1.0;
        }
        if (per_user && lane == 0) {
#pragma unroll
            for (int s = 0; s < NS - 2; ++s)
                if (s < n_out) per_user[b * n_out + s] = v[s];
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[s] += v[s];
    }
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) sh[wave][s] = acc[s];
    }
    __syncthreads();
    if (tid < NS) {
        const int slot = tid >= NS - 2 ? n_out + (tid - (NS - 2)) : tid;
        if (tid >= NS - 2 || tid < n_out) part[(int64_t)blockIdx.x * (n_out + 2) + slot] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
    }
}

}  // namespace

extern "C" int ngcf_rank_position_metrics(const int32_t *position, int64_t B, const int64_t *user_ids, int64_t n_user_rows,
                                          const int64_t *truth_rowptr, const int32_t *truth_colidx, int64_t n_truth,
                                          const int64_t *excl_rowptr, int64_t n_items, const int32_t *ks_host, int n_ks,
                                          double *per_user, double *sums, int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_ks < 0 || n_ks > NGCF_POS_KS || (n_ks > 0 && !ks_host))
        return fail(NGCF_ERR_ARG, "rank_position_metrics: between 0 and %d cut-offs", NGCF_POS_KS);
    if (n_items < 1 || n_items >= ((int64_t)1 << 31))
        return fail(NGCF_ERR_ARG, "rank_position_metrics: n_items=%lld outside [1, 2^31)", (long long)n_items);
    int ks[NGCF_POS_KS] = {1, 1, 1, 1, 1, 1, 1, 1};
    for (int q = 0; q < n_ks; ++q) {
        if (ks_host[q] < 1 || ks_host[q] > n_items)
            return fail(NGCF_ERR_ARG, "rank_position_metrics: cut-off K=%d outside [1, n_items=%lld]", ks_host[q], (long long)n_items);
        ks[q] = ks_host[q];
    }
    if (B < 0 || n_user_rows < 0 || n_truth < 0) return fail(NGCF_ERR_ARG, "rank_position_metrics: bad argument");
    if (B == 0) return NGCF_OK;
    if (!truth_rowptr || !sums || !status || (n_truth > 0 && (!position || !truth_colidx)))
        return fail(NGCF_ERR_ARG, "rank_position_metrics: bad argument");
    const int n_slots = 4 + 4 * n_ks + 2;
    const int64_t blocks = (B + 255) / 256;
    if (blocks >= ((int64_t)1 << 31)) return fail(NGCF_ERR_ARG, "rank_position_metrics: batch too large");
    return launch_with_partial_sums("rank_position_metrics", blocks, n_slots, sums, stream, [&](double *part) {
        pos_metrics_kernel<<<dim3((unsigned)blocks), 256, 0, stream>>>(position, B, user_ids, n_user_rows, truth_rowptr, truth_colidx,
                                                                      n_truth, excl_rowptr, n_items, n_ks, ks[0], ks[1], ks[2], ks[3],
                                                                      ks[4], ks[5], ks[6], ks[7], per_user, part, status);
    });
}
