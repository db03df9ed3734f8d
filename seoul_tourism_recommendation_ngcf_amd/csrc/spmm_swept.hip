// spmm_swept.hip - the L2-swept SpMM for long-lived matrices: the persistent kernel, its launch, and the host plan (swept_plan.h) on the device.
//
// Same product LE = L.E (NGCF.py:130).  Why: on a graph without locality the row-wise kernels miss L2 on most
// gathered rows and run at the chip's L2-miss rate (~8 TB/s of gathered bytes); rows served from L2 arrive 2-3x
// faster (profiles/r01_window_lab.txt).  Here the gathered table is swept in column windows of a few MiB while
// every CU works on the same window, so a table row is fetched from memory once per XCD and re-used from that
// XCD's L2 by the other output rows that need it.
//
// How: a persistent grid of 256 workgroups (one per CU).  Every wave owns up to RW output rows ("wave task") whose
// accumulators - one 64-float slice each - stay in LDS for a whole sweep, so the chip's LDS holds 147 K row slices
// at once; d is walked slice by slice, the rows in "row passes" when they do not fit at once.  The host plan deals
// rows (long rows in strided pieces) to the wave tasks so that all tasks carry the same number of entries, and
// lays each task's entries out window by window (8 MiB of table slice), inside a window in ascending column order:
// waves that enter a window together walk the table left to right together.  A round = one wave instruction = four
// entries (16 lanes x 16 B each).  The contribution of an entry is added to its LDS row with a plain
// read-modify-write (LDS float atomics were measured 15x slower), so the four entries of a round must belong to four
// different rows: the rounds are filled greedily in column order, an entry whose row is already in the round waits
// for the next one; slots that stay empty (~1 % on C3) point at a spare LDS row.  A wave touches nothing but its own
// LDS rows and adds in list order: the result is deterministic.
// The sweep is kept together per XCD (HW_REG_XCC_ID) by counters: a wave may enter window s once every workgroup
// of its XCD has left window s-1-lead behind.  The spin is bounded and only serves speed - a grid that is not
// resident together loses the L2 re-use, it never hangs and never changes the result.
// Rows cut into pieces leave partial sums in the workspace; spmm_fixup_kernel adds them in piece order.
// Measured on C3 (1x MI355X, d=128): item rows 1.83-1.93 ms vs 3.5 ms row-wise, user rows 1.84-1.94 vs 2.46 ms d-sliced.
#include "spmm_device.h"
#include "swept_plan.h"      // the host plan and the geometry constants of a part

using namespace swept_plan;

namespace {
constexpr int kRing = 8;                  // rotating sweep counters per XCD

void free_part(ngcf_csr::Swept::Part &p)
{
    if (p.tptr) (void)hipFree(p.tptr);
    if (p.e_pack) (void)hipFree(p.e_pack);
    if (p.e_val) (void)hipFree(p.e_val);
    if (p.dst) (void)hipFree(p.dst);
    if (p.prow) (void)hipFree(p.prow);
    if (p.heavy_row) (void)hipFree(p.heavy_row);
    if (p.heavy_seg_ptr) (void)hipFree(p.heavy_seg_ptr);
    p = ngcf_csr::Swept::Part();
}

// Plan of the rows of one group (swept_plan.h: plan_part) on the device.  Leaves part.waves == 0 when the part is not worth
// it (mode 3) or the shape does not fit the entry encoding.
int build_part(const ngcf_csr *c, const ngcf_csr::RowGroup &grp, bool force, hipStream_t stream, ngcf_csr::Swept::Part &part, int LPE)
{
    const NgcfOptions &o = ngcf_opts();
    Params prm;
    prm.lpe = LPE;
    prm.cut = o.swept_cut;
    prm.moments = !o.swept_no_moments;
    prm.order_rows = o.swept_order_rows != 0;
    prm.window_kb = o.swept_window_kb;
    prm.force = force;
    prm.debug = o.swept_debug != 0;
    const int64_t n = grp.end - grp.begin;
    if (n <= 0 || grp.col_hi < grp.col_lo) return NGCF_OK;           // no rows, no entries
    std::vector<int64_t> rp((size_t)n + 1);
    HIP_TRY(hipMemcpyAsync(rp.data(), c->rowptr + grp.begin, sizeof(int64_t) * rp.size(), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const int64_t e0 = rp[0], nnz = rp[(size_t)n] - e0;
    if (declined(n, nnz, grp.col_lo, grp.col_hi, prm)) return NGCF_OK;
    std::vector<int32_t> col((size_t)nnz);    // only now the entries come to the host
    std::vector<float> val((size_t)nnz);
    HIP_TRY(hipMemcpyAsync(col.data(), c->colidx + e0, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(val.data(), c->vals + e0, sizeof(float) * (size_t)nnz, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (auto &x : rp) x -= e0;
    const PartPlan plan = plan_part(rp.data(), n, col.data(), val.data(), grp.begin, grp.col_lo, grp.col_hi, prm);
    if (!plan.error.empty()) return fail(NGCF_ERR_ARG, "%s", plan.error.c_str());
    part.row_lo = grp.begin;
    part.row_hi = grp.end;
    part.rows_per_wave = plan.rows_per_wave;
    part.lpe = LPE;
    part.n_rowpass = plan.n_rowpass;
    part.n_win = plan.n_win;
    part.win_cols = plan.win_cols;
    part.col_lo = grp.col_lo;
    part.col_hi = grp.col_hi;
    part.n_slots = plan.n_slots;
    part.n_partial = plan.n_partial;
    part.n_heavy = (int64_t)plan.heavy_row.size();
    int rc = upload(&part.tptr, plan.tptr, stream);
    if (rc == NGCF_OK) rc = upload(&part.e_pack, plan.e_pack, stream);
    if (rc == NGCF_OK) rc = upload(&part.e_val, plan.e_val, stream);
    if (rc == NGCF_OK) rc = upload(&part.dst, plan.dst, stream);
    if (rc == NGCF_OK) rc = upload(&part.prow, plan.prow, stream);
    if (rc == NGCF_OK && part.n_heavy > 0) rc = upload(&part.heavy_row, plan.heavy_row, stream);
    if (rc == NGCF_OK && part.n_heavy > 0) rc = upload(&part.heavy_seg_ptr, plan.heavy_ptr, stream);
    if (rc == NGCF_OK && hipStreamSynchronize(stream) != hipSuccess) rc = fail(NGCF_ERR_HIP, "swept plan: upload failed");
    if (rc != NGCF_OK) {
        free_part(part);
        return rc;
    }
    part.waves = plan.waves;
    return NGCF_OK;
}
}  // namespace

void free_swept(ngcf_csr *c)
{
    ngcf_csr::Swept &w = c->swept;
    for (auto &p : w.parts) free_part(p);
    free_segset(w.out);
    if (w.barrier) (void)hipFree(w.barrier);
    w = ngcf_csr::Swept();
}

// Builds the parts for c->mode (2: every row group whose shape allows it, 3: the groups where re-use is expected) and
// the segment set of the cut rows that stay with the row-wise kernels.  Workspace rows: [those segments][part 0's
// partial rows][part 1's]...
int build_swept_plan(ngcf_csr *c, hipStream_t stream)
{
    free_swept(c);
    ngcf_csr::Swept &w = c->swept;
    w.built_mode = c->mode;
    w.lpe = ngcf_opts().swept_lpe == 32 ? 32 : 16;
    if (c->mode < 2 || c->n_rows == 0 || c->nnz == 0) return NGCF_OK;
    // the plan is laid out for one resident workgroup on each of 256 CUs in 8 XCDs (an MI355X in SPX mode); on any
    // other partitioning the grid would not be resident together, so the products stay on the row-wise kernels
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus != kSweptWGs) {
        static bool warned = false;
        if (!warned) {
            warned = true;
            fprintf(stderr, "[ngcf] note: this device reports %d CUs, not %d (an MI355X in SPX mode): the L2-swept SpMM plan is not built and the "
                            "products run on the row-wise kernels (about half the speed on large graphs); ngcf_csr_swept_rows() returns 0\n",
                    cus, kSweptWGs);
        }
        return NGCF_OK;
    }
    w.group_swept.assign(c->groups.size(), 0);
    for (size_t g = 0; g < c->groups.size(); ++g) {
        ngcf_csr::Swept::Part p;
        const int rc = build_part(c, c->groups[g], c->mode == 2, stream, p, w.lpe);
        if (rc != NGCF_OK) {
            free_swept(c);
            return rc;
        }
        if (p.waves == 0) continue;
        w.group_swept[g] = 1;
        w.parts.push_back(p);
    }
    if (w.parts.empty()) return NGCF_OK;
    std::vector<int64_t> rp((size_t)c->n_rows + 1);
    HIP_TRY(hipMemcpyAsync(rp.data(), c->rowptr, sizeof(int64_t) * rp.size(), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    std::vector<std::pair<int64_t, int64_t>> rest;     // the groups no part covers
    for (size_t g = 0; g < c->groups.size(); ++g)
        if (!w.group_swept[g]) rest.push_back({c->groups[g].begin, c->groups[g].end});
    const HostSegs segs = cut_rows(rp, rest, c->seg_len);     // (alive until the stream is synchronised below)
    int rc = upload_segset(w.out, segs, stream);
    int64_t base = w.out.n_seg;
    for (auto &p : w.parts) {
        p.partial_base = base;
        base += p.n_partial;
        w.n_partial += p.n_partial;
    }
    if (rc == NGCF_OK && (hipMalloc(&w.barrier, sizeof(uint32_t) * 32 * 8 * 4) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess))
        rc = fail(NGCF_ERR_HIP, "swept plan: allocation failed");
    if (rc != NGCF_OK) free_swept(c);
    return rc;
}

// The parts gather with 32-bit byte offsets: the gathered rows must lie within 4 GiB of the table base
bool swept_usable(const ngcf_csr *c, int64_t ldE, int d)
{
    const ngcf_csr::Swept &w = c->swept;
    if (w.parts.empty() || c->mode < 2 || d % (w.lpe * 4) != 0) return false;
    for (const auto &p : w.parts)
        if (((int64_t)p.col_hi + 1) * ldE * 4 > (int64_t)UINT32_MAX) return false;
    return true;
}

#ifndef NGCF_SWEPT_LABW
#define NGCF_SWEPT_LABW 2      // loads allowed in flight when the adds of a half-chunk begin (see load_entries below)
#endif

// RW accumulator rows per wave, NW waves per workgroup (NW*RW*256 B of LDS)
// The kernel can take up to kMaxLaunchParts parts (row groups) of a product one after the other: a workgroup that has finished
// its share of the first goes straight on to the second, so the end-of-part stragglers (the last waves finish 5-8 % after the
// first, profiles/r02_swept_trace.txt) would cost once per product instead of once per part; the sweep steps are numbered
// through, so the XCD counters need no reset in between.  launch_swept passes one part per launch (merging measured slower).
constexpr int kMaxLaunchParts = 4;
struct SweptPartArgs {
    const int64_t *tptr;
    const int32_t *e_pack;
    const float *e_val;
    const int32_t *dst;
    const int32_t *prow;
    float *partial;
    int n_rowpass, n_win, lead;
};
struct SweptLaunch {
    SweptPartArgs part[kMaxLaunchParts];
    int n_parts;
};

// DROP: device-mode node dropout (common.h, EdgeDrop): a lane tests the entry it holds when it loads it - row from the wave's
// table of matrix rows (one ds_bpermute), column from the packed entry - and zeroes the value of a dropped entry; the gather of
// a dropped entry still happens (the round structure is fixed by the plan), its product is 0.
template <int LPE, int RW, int NW, bool DROP>
__global__ __launch_bounds__(NW * 64) void spmm_swept_kernel(SweptLaunch L, int n_slices, const float *__restrict__ E,
                                                             int64_t ldE, float *__restrict__ out, int64_t ldo, int dp, unsigned *bar,
                                                             int max_spin, int sync_k, unsigned prio_cols, int prio_graded,
                                                             EdgeDrop dr_in)
{
    const EdgeDropR dr = resolve_drop(dr_in);
    constexpr int kSW = LPE * 4, kEPR = 64 / LPE, kCH = 16 * kEPR;
    __shared__ float acc_lds[NW * (RW + 1) * kSW];   // per wave: RW accumulator rows + the spare row of the empty slots
    __shared__ unsigned wg_cnt[kRing];
    __shared__ int perm_lds;                    // highest sweep step this workgroup knows to be permitted
    __shared__ unsigned xcc_id;
    __shared__ unsigned wg_front;               // furthest (sweep, column) any wave of this workgroup has reached
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane / LPE, p = lane % LPE;   // entry slot in the round, position in the slice
    // chunk entry this lane keeps: round u = lane u of every 16-lane DPP row (LPE = 32: the two DPP rows of an entry's lanes hold it twice)
    const int held = (lane & 15) * kEPR + g;
    float *wacc = acc_lds + wave * ((RW + 1) * kSW);
    if (threadIdx.x < kRing) wg_cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        xcc_id = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u;   // HW_REG_XCC_ID
        perm_lds = L.part[0].lead;              // steps 0..lead wait for nobody
        wg_front = 0;
    }
    __syncthreads();
    unsigned *ctr = bar + xcc_id * 32;
    const unsigned members = gridDim.x / 8;
    int perm = L.part[0].lead;                  // this wave's copy of perm_lds
    int step0 = 0;                              // sweep steps of the passes before this one
    const unsigned ld_bytes = (unsigned)ldE * 4u;
    int sweep_no = 0;                           // sweeps (row pass x slice) so far, over all parts
    for (int pi = 0; pi < L.n_parts; ++pi) {
    const int64_t *__restrict__ tptr = L.part[pi].tptr;
    const int32_t *__restrict__ e_pack = L.part[pi].e_pack;
    const float *__restrict__ e_val = L.part[pi].e_val;
    const int32_t *__restrict__ dst = L.part[pi].dst;
    float *__restrict__ partial = L.part[pi].partial;
    const int n_rowpass = L.part[pi].n_rowpass, n_win = L.part[pi].n_win, lead = L.part[pi].lead;
    const bool sync = lead >= 0;
    for (int rp = 0; rp < n_rowpass; ++rp) {
        const int64_t task = ((int64_t)rp * gridDim.x + blockIdx.x) * NW + wave;
        const int64_t *tp = tptr + task * n_win;
        const int64_t beg = tp[0], end = tp[n_win];
        int my_row = 0, my_row_hi = 0;           // lane lr (and lr - 64): the matrix row behind accumulator row lr of this task
        if (DROP && lane < RW) my_row = L.part[pi].prow[task * RW + lane];
        if (DROP && RW > 64 && lane + 64 < RW) my_row_hi = L.part[pi].prow[task * RW + 64 + lane];
        for (int slice = 0; slice < n_slices; ++slice, ++sweep_no, step0 += (n_win + sync_k - 1) / sync_k) {   // sweep step = sync_k windows
            const char *Eb = reinterpret_cast<const char *>(E + slice * kSW);   // uniform base + 32-bit lane offsets
            for (int i = lane; i < (RW + 1) * kSW; i += 64) wacc[i] = 0.f;
            int b = 0;
            int64_t wend = tp[1], wend_next = n_win > 1 ? tp[2] : end;
            auto arrive = [&](int s) {           // this wave has left sweep step s behind
                if (sync && lane == 0) {
                    const unsigned old = atomicAdd(&wg_cnt[s % kRing], 1u);
                    if ((old + 1) % NW == 0)
                        __hip_atomic_fetch_add(ctr + (s % kRing), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            };
            // windows left behind by a wave whose next slot is `pos`; then the permission to enter the new one
            auto cross = [&](int64_t pos, bool crossed) {
                while (b < n_win - 1 && pos >= wend) {
                    if ((b + 1) % sync_k == 0) arrive(step0 + b / sync_k);
                    ++b;
                    wend = wend_next;
                    wend_next = b + 2 <= n_win ? tp[b + 2] : end;
                    crossed = true;
                }
                const int s = step0 + b / sync_k;   // the step being entered needs step s-1-lead finished by the whole XCD
                if (crossed && sync && max_spin > 0 && perm < s) {
                    perm = __hip_atomic_load(&perm_lds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    int spins = 0;
                    while (perm < s) {
                        // lanes 0..kRing-1 read the ring; step t is finished when its slot reached members*(t/kRing+1)
                        const unsigned mine = lane < kRing ? __hip_atomic_load(ctr + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
                        int t = perm - lead;     // first step not yet known to be finished
                        for (int k = 0; k < kRing - 2 - lead; ++k, ++t) {
                            const unsigned have = __builtin_amdgcn_readlane(mine, t % kRing);
                            if (have < members * (unsigned)(t / kRing + 1)) break;
                        }
                        perm = t + lead;         // steps <= perm may start
                        if (perm >= s) break;
                        if (++spins >= max_spin) {
                            max_spin = 0;        // the XCD's workgroups are not resident together: stop waiting for good
                            break;
                        }
                        __builtin_amdgcn_s_sleep(2);
                    }
                    if (lane == 0) atomicMax(&perm_lds, perm);
                }
            };
            const int idle_pk = end > beg ? (RW << kRowBits) | (e_pack[beg] & kColMask) : 0;   // past the end: like an empty slot
            // Every load of the main loop is UNCONDITIONAL (slots past the end of the list read the list's last entry again and
            // are turned into idle slots afterwards): behind a branch the compiler cannot count a load and waits for everything
            // in flight instead - which is what r01/r02 ran with unknowingly (s_waitcnt vmcnt(7..0) in front of the adds of a
            // half: at most the other half's eight gathers in flight).  With exact counts (vmcnt(15..8): both halves in flight)
            // the product is SLOWER - 3.16 vs 2.96-2.99 ms per L.E on C3 - because waves that run further ahead of their
            // data spread the sweep; so the depth is now stated: all but NGCF_SWEPT_LABW loads have arrived before the adds
            // of a half begin.  C3, ms per L.E, same box: 0 -> 2.99-3.00, 2 -> 2.94, 3 -> 2.95, 4 -> 2.95 (3.05 once), 5 -> 2.96,
            // 6 -> 2.97, 8 -> 3.16, 12 -> 3.13, no explicit wait -> 3.16-3.18 (0..6 are within run-to-run noise of each other: +-0.04).
            auto load_entries = [&](int64_t pos, int &pk, float &v) {
                const int64_t idx = pos + held;
                const int64_t idc = idx < end ? idx : end - 1;
                const int pk_l = e_pack[idc];
                const float v_l = e_val[idc];
                pk = idx < end ? pk_l : idle_pk;
                v = idx < end ? v_l : 0.f;
                if (DROP) {
                    const int lr = (pk >> kRowBits) & 0x7f;                      // RW (the spare row) for idle slots: any row will do
                    int grow = __shfl(my_row, lr < RW ? lr & 63 : 0);
                    if (RW > 64) {
                        const int hi = __shfl(my_row_hi, lr & 63);
                        grow = lr >= 64 && lr < RW ? hi : grow;
                    }
                    v = edge_keep(dr, grow, pk & kColMask) ? v : 0.f;
                }
            };
            if (end > beg) {
                int pkA, pkB;
                float vA, vB;
                f32x4 xa[8], xb[8];
                unsigned offA;
                const unsigned lane_off = p * 16;
#define NGCF_GATHER(buf, u, j) buf[j] = *reinterpret_cast<const f32x4 *>(Eb + ((unsigned)row_bcast<u>((int)offA) + lane_off));
#define NGCF_GATHER_LO(x) NGCF_GATHER(x, 0, 0) NGCF_GATHER(x, 1, 1) NGCF_GATHER(x, 2, 2) NGCF_GATHER(x, 3, 3) NGCF_GATHER(x, 4, 4) NGCF_GATHER(x, 5, 5) NGCF_GATHER(x, 6, 6) NGCF_GATHER(x, 7, 7)
#define NGCF_GATHER_HI(x) NGCF_GATHER(x, 8, 0) NGCF_GATHER(x, 9, 1) NGCF_GATHER(x, 10, 2) NGCF_GATHER(x, 11, 3) NGCF_GATHER(x, 12, 4) NGCF_GATHER(x, 13, 5) NGCF_GATHER(x, 14, 6) NGCF_GATHER(x, 15, 7)
#define NGCF_ACC(buf, u, j)                                                                        \
    {                                                                                             \
        const int pku = row_bcast<u>(pkA);                                                        \
        const float vu = row_bcast<u>(vA);                                                        \
        if (pku >= 0) {                                                                           \
            f32x4 *a = reinterpret_cast<f32x4 *>(wacc + (pku >> kRowBits) * kSW + p * 4);         \
            f32x4 t = *a;                                                                         \
            t.x = fmaf(vu, buf[j].x, t.x);                                                          \
            t.y = fmaf(vu, buf[j].y, t.y);                                                          \
            t.z = fmaf(vu, buf[j].z, t.z);                                                          \
            t.w = fmaf(vu, buf[j].w, t.w);                                                          \
            *a = t;                                                                               \
        }                                                                                         \
    }
#define NGCF_ACC_LO(x) NGCF_ACC(x, 0, 0) NGCF_ACC(x, 1, 1) NGCF_ACC(x, 2, 2) NGCF_ACC(x, 3, 3) NGCF_ACC(x, 4, 4) NGCF_ACC(x, 5, 5) NGCF_ACC(x, 6, 6) NGCF_ACC(x, 7, 7)
#define NGCF_ACC_HI(x) NGCF_ACC(x, 8, 0) NGCF_ACC(x, 9, 1) NGCF_ACC(x, 10, 2) NGCF_ACC(x, 11, 3) NGCF_ACC(x, 12, 4) NGCF_ACC(x, 13, 5) NGCF_ACC(x, 14, 6) NGCF_ACC(x, 15, 7)
                load_entries(beg, pkA, vA);
                cross(beg, true);
                offA = (unsigned)(pkA & kColMask) * ld_bytes;
                NGCF_GATHER_LO(xa)
                const unsigned sweep_tag = (unsigned)(sweep_no & 0xff) << kRowBits;
                for (int64_t pos = beg; pos < end; pos += kCH) {
                    if (prio_cols) {
                        // Inside a workgroup the same few waves fall behind and stay behind (the instruction arbiter serves the
                        // older wave of a SIMD first), up to 4.5 MiB of table on the C3 item rows while the workgroups themselves
                        // stay within 0.3 MiB of each other (profiles/r02_swept_trace.txt): a wave that is more than prio_cols
                        // columns behind the front of its workgroup raises its priority, the others run at 0.
                        const unsigned mine = sweep_tag | (unsigned)(__builtin_amdgcn_readfirstlane(pkA) & kColMask);
                        unsigned front = 0;
                        if (lane == 0) front = atomicMax(&wg_front, mine);
                        front = (unsigned)__builtin_amdgcn_readfirstlane((int)front);
                        const unsigned lag = front > mine ? front - mine : 0u;
                        if (prio_graded) {
                            if (lag > 4 * prio_cols) __builtin_amdgcn_s_setprio(3);
                            else if (lag > 2 * prio_cols) __builtin_amdgcn_s_setprio(2);
                            else if (lag > prio_cols) __builtin_amdgcn_s_setprio(1);
                            else __builtin_amdgcn_s_setprio(0);
                        } else {
                            if (lag > prio_cols) __builtin_amdgcn_s_setprio(3);
                            else __builtin_amdgcn_s_setprio(0);
                        }
                    }
                    load_entries(pos + kCH, pkB, vB);                // the next chunk's entries, two gathers ahead
                    if (pos + 8 * kEPR < end) cross(pos + 8 * kEPR, false);   // no gather is issued into a window before its permission
                    NGCF_GATHER_HI(xb)                               // (past the end: idle slots, the column of the task's first entry)
                    __builtin_amdgcn_s_waitcnt(0xF70 | (NGCF_SWEPT_LABW & 0xf));   // s_waitcnt vmcnt(NGCF_SWEPT_LABW)
                    NGCF_ACC_LO(xa)
                    if (pos + kCH < end) cross(pos + kCH, false);
                    offA = (unsigned)(pkB & kColMask) * ld_bytes;
                    NGCF_GATHER_LO(xa)                               // first half of the next chunk, in flight during the adds below
                    __builtin_amdgcn_s_waitcnt(0xF70 | (NGCF_SWEPT_LABW & 0xf));
                    NGCF_ACC_HI(xb)
                    pkA = pkB;
                    vA = vB;
                }
#undef NGCF_GATHER
#undef NGCF_GATHER_LO
#undef NGCF_GATHER_HI
#undef NGCF_ACC
#undef NGCF_ACC_LO
#undef NGCF_ACC_HI
            }
            cross(INT64_MAX - 1, false);         // leave the remaining windows (b ends at n_win-1) ...
            arrive(step0 + (n_win - 1) / sync_k);   // ... and the last step
            // write this wave's rows (its own LDS rows; a wave's LDS operations complete in order)
            for (int r0 = 0; r0 < RW; r0 += kEPR) {
                const int r = r0 + g;
                if (r < RW) {
                    const int drow = dst[task * RW + r];
                    if (drow != -1) {
                        float *o = drow >= 0 ? out + (int64_t)drow * ldo : partial + (int64_t)(-2 - drow) * dp;
                        *reinterpret_cast<f32x4 *>(o + slice * kSW + p * 4) = *reinterpret_cast<const f32x4 *>(wacc + r * kSW + p * 4);
                    }
                }
            }
        }
    }
    }   // parts
}

// kernels + fix-ups of every part; `partial` = workspace base (rows of dp floats)
int launch_swept(const ngcf_csr *c, const float *E, int64_t ldE, int d, float *out, int64_t ldo, float *partial, int dp,
                 hipStream_t stream, const EdgeDrop &dr)
{
    const ngcf_csr::Swept &w = c->swept;
    const NgcfOptions &o = ngcf_opts();
    const int max_spin = o.swept_spin;                       // polls before a wave stops waiting for good
    // Inside a window a wave's entries are in ascending column order (plan, "cols" layout), so waves that enter a window
    // together walk the table left to right together and the live set is a few hundred KiB; the XCD-wide counters tick
    // once per 8 MiB window and a wave may be one window ahead - they only bound the drift.  bench.py on C3, same process:
    // row-wise layout inside 4 MiB windows 15.1 ms/step (SpMM 4.16 ms), inside 2 MiB windows with a tick every third
    // 14.3-14.4 (3.9); column order inside 8 MiB windows 13.65-13.7 (3.68-3.71), 6 MiB 13.8, 12 MiB 13.9, 16 MiB 14.3,
    // 4 MiB 14.4; lead 0: 14.9, lead 2: 14.5.
    // r02, with the graded wave priorities below (profiles/r02_swept_lab.txt, grid of window x lead x threshold): a table of
    // many windows wants lead 2 (C3 item rows, 16 windows: 1.50 vs 1.53 ms), a table of a few windows lead 1 (C3 user rows, 4
    // windows: 1.44 vs 1.46 ms); NGCF_SWEPT_LEAD overrides both (-1: no synchronisation at all)
    const int lead_env = o.swept_lead;
    const int sync_k = std::max(1, o.swept_sync_every);       // windows per sweep step (lab knob)
    // lag (KiB of table slice) behind the front of its workgroup beyond which a wave raises its priority; 0 = off
    const int kSW = w.lpe * 4;
    const unsigned prio_cols = (unsigned)std::max(0, o.swept_prio_kb) * 1024u / (kSW * 4);
    // graded: priority 1 / 2 / 3 beyond 1x / 2x / 4x the threshold (C3 item rows 1.50 vs 1.61 ms against one step to 3)
    const int prio_graded = o.swept_prio_graded;
    // one launch per part: taking both halves of C3 in one launch was measured SLOWER (3.01-3.11 vs 2.96-2.98 ms per product,
    // same box) - the workgroups that start the second part early gather from another table and take L2 away from the
    // stragglers of the first
    for (const auto &p : w.parts) {
        SweptLaunch L{};
        // sweep steps a wave may run ahead: by the size of the part's table
        const int lead = std::min(lead_env != -2 ? lead_env : (p.n_win >= 8 ? 2 : 1), kRing - 4);
        L.part[L.n_parts++] = SweptPartArgs{p.tptr, p.e_pack, p.e_val, p.dst, p.prow, partial ? partial + p.partial_base * (int64_t)dp : nullptr,
                                            p.n_rowpass, p.n_win, lead};
        // this stream's block of sweep counters (up to four streams per CSR get one of their own; a fifth shares the last)
        int bi = 0;
        for (; bi < w.barrier_used && w.barrier_owner[bi] != stream; ++bi) {}
        if (bi == w.barrier_used) {
            if (w.barrier_used < 4) w.barrier_owner[w.barrier_used++] = stream;
            else bi = 3;
        }
        unsigned *bar_blk = w.barrier + (size_t)bi * 32 * 8;
        HIP_TRY(hipMemsetAsync(bar_blk, 0, sizeof(uint32_t) * 32 * 8, stream));
#define NGCF_SWEPT_LAUNCH(LPE_, RW_, NW_, DROP_)                                                                                    \
    spmm_swept_kernel<LPE_, RW_, NW_, DROP_><<<dim3(kSweptWGs), NW_ * 64, 0, stream>>>(L, d / kSW, E, ldE, out, ldo, dp, bar_blk, \
                                                                                max_spin, sync_k, prio_cols, prio_graded, dr)
        if (w.lpe == 32 && dr.n > 0) NGCF_SWEPT_LAUNCH(32, 18, 16, true);
        else if (w.lpe == 32) NGCF_SWEPT_LAUNCH(32, 18, 16, false);
        else if (dr.n > 0) NGCF_SWEPT_LAUNCH(16, 36, 16, true);
        else NGCF_SWEPT_LAUNCH(16, 36, 16, false);
#undef NGCF_SWEPT_LAUNCH
        LAUNCH_CHECK();
    }
    for (const auto &p : w.parts) {
        if (p.n_heavy == 0) continue;
        spmm_fixup_kernel<4><<<dim3((unsigned)((p.n_heavy + 3) / 4)), 256, 0, stream>>>(
            p.heavy_row, p.heavy_seg_ptr, p.n_heavy, partial + p.partial_base * (int64_t)dp, dp, d, out, ldo);
        LAUNCH_CHECK();
    }
    return NGCF_OK;
}
