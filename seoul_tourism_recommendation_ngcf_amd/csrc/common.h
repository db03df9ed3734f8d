// Shared host/device declarations of libngcf_hip.so (internal; the public C ABI is include/ngcf_hip.h).
#ifndef NGCF_COMMON_H
#define NGCF_COMMON_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/ngcf_hip.h"

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
inline thread_local char g_err[512] = "";

inline int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(NGCF_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                        __FILE__, __LINE__);                                                   \
    } while (0)

#define LAUNCH_CHECK()                                                                         \
    do {                                                                                       \
        hipError_t e_ = hipGetLastError();                                                     \
        if (e_ != hipSuccess)                                                                  \
            return fail(NGCF_ERR_HIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                   \
    } while (0)


// ---------------------------------------------------------------------------------------------
// options: every tunable of the dispatch code in ONE struct.  library.hip fills it once per process (the only getenv() of the
// library is in ngcf_options_from_env there: launches never touch the environment) and ngcf_set_option changes single
// fields at run time (tests, tools/).
// ---------------------------------------------------------------------------------------------
struct NgcfOptions {
    // spmm.hip
    int no_fork = 0;               // NGCF_NO_FORK: never record the two halves of a row-wise product as parallel graph branches
    int no_slicing = 0;            // NGCF_NO_SLICING: no d-sliced launches of the sliceable row groups
    int no_ldstab = 0;             // NGCF_NO_LDSTAB: no table-in-LDS kernel
    int no_panel_split = 0;        // NGCF_NO_PANEL_SPLIT: odd widths in one piece on the scalar kernels
    int no_tail_table = 0;         // NGCF_NO_TAIL_TABLE: tail columns gathered out of the strided table
    int no_pad_product = 0;        // NGCF_NO_PAD_PRODUCT: small matrices: do not multiply the padding columns along
    int64_t fork_min = 200000000;  // NGCF_FORK_MIN: entry-columns from which the halves are forked under capture
    // dense.hip (dense_path)
    int dense_direct = 1;          // NGCF_DENSE_DIRECT: 0 never, 1 up to 8 192 rows, 2 at any row count
    int dense_resident = 4;        // NGCF_DENSE_RESIDENT: 4 the bf16 three-way split kernel; 1 the fp32 weights-resident kernel; 0 keeps the staged kernel
    int dense_resident_min_rows = 106496;  // NGCF_DENSE_RESIDENT_MIN_ROWS: rows from which the weights-resident kernel runs (65 536 = one round of its 2 048 waves; measured cross-over, profiles/r04_dense_rows_lab.txt)
    int dense_small_tiles = 1;     // NGCF_DENSE_SMALL_TILES: 32-row tiles for <= 128 output columns on <= 16 384 rows
    int dense_tall = 1;            // NGCF_DENSE_TALL: 256 / 512 output columns as 96-row x 128-column workgroups: 0 never, 1 where measured faster, 2 always
    // spmm_t_rows.hip, bwd_dense.hip
    int t_rows_bitmap = 1;         // NGCF_T_ROWS_BITMAP: the bitmap-in-LDS kernel of the row-sparse transposed product: 0 never (the slot-table kernel at every size), 1 from 2^22 stored entries, 2 at any number of stored entries (every other condition stays)
    int bwd_input_resident = 1;    // NGCF_BWD_INPUT_RESIDENT: 0 keeps the staged input-gradient kernel at every size
    // select.hip
    int select_no_lds = 0;         // NGCF_SELECT_NO_LDS: the per-group select counts in memory at every group count
    // csr.hip
    int slice_max_mb = 48;         // NGCF_SLICE_MAX_MB: largest table slice a d-sliced group may gather from
    // spmm_swept.hip (plan)
    int swept_lpe = 16;            // NGCF_SWEPT_LPE: lanes per entry of the swept plan: 16 = 64-float slices, 32 = 128-float slices
    int swept_cut = 4;             // NGCF_SWEPT_CUT: rows are cut at 1/cut of a wave task's share
    int swept_no_moments = 0;      // NGCF_SWEPT_NO_MOMENTS
    int swept_order_rows = 0;      // NGCF_SWEPT_ORDER=rows
    int swept_debug = 0;           // NGCF_SWEPT_DEBUG: print the plan
    int swept_window_kb = 0;       // NGCF_SWEPT_WINDOW_KB: 0 = by table size
    // spmm_swept.hip (launch)
    int swept_spin = 500;          // NGCF_SWEPT_SPIN
    int swept_lead = -2;           // NGCF_SWEPT_LEAD: -2 = by table size, -1 = no synchronisation
    int swept_sync_every = 1;      // NGCF_SWEPT_SYNC_EVERY
    int swept_prio_kb = 256;       // NGCF_SWEPT_PRIO_KB
    int swept_prio_graded = 1;     // NGCF_SWEPT_PRIO_GRADED
};
extern NgcfOptions g_opts;                      // library.hip
const NgcfOptions &ngcf_opts();                 // library.hip: reads the environment on first use


// per-device state (function attributes, side streams) lives in small arrays indexed by the current device
constexpr int kMaxDevices = 64;
inline int current_device_slot()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    return dev % kMaxDevices;
}

// A kernel that keeps up to 160 KiB (all of a CU's LDS) in dynamic LDS: the attribute is per kernel and device, set once.
template <auto kernel> static hipError_t allow_full_lds(int bytes = 160 * 1024)
{
    static bool set[kMaxDevices] = {};
    const int dev_i = current_device_slot();
    if (set[dev_i]) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    set[dev_i] = e == hipSuccess;
    return e;
}

inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }


inline int grid_for(int64_t n, int block)

{
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > 256 * 16) g = 256 * 16;
    return (int)g;
}



// ---------------------------------------------------------------------------------------------
// CSR object (csr.hip owns its lifetime; spmm*.hip read it)
// ---------------------------------------------------------------------------------------------
struct ngcf_csr {
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    int64_t max_row_len = 0;     // stored entries of the longest row (set by the segmentation plan)
    int64_t *rowptr = nullptr;   // device [n_rows+1]
    int32_t *colidx = nullptr;   // device [nnz]
    float *vals = nullptr;       // device [nnz]
    bool owns = false;
    // a thinned copy made by ngcf_csr_filter (csr_filter.hip): capacity of colidx / vals, the exclusive scan of the keep flags over
    // the source's entries (pos[e] = kept entries before e, pos[src nnz] = kept in all), scan scratch; seg.seg_row / heavy_row /
    // heavy_seg_ptr are then BORROWED from the source (same segment structure, own seg_begin) and nnz may be an upper bound
    int64_t cap = 0, pos_len = 0;
    int32_t *pos = nullptr;
    int32_t *scan_blk = nullptr;
    bool borrows_plan = false;
    const struct ngcf_csr *filter_src = nullptr;
    // row segmentation: rows with > seg_len entries are cut into segments
    struct SegSet {
        int64_t n_seg = 0, n_heavy = 0;
        int32_t *seg_row = nullptr;        // device [n_seg]   row of each segment
        int64_t *seg_begin = nullptr;      // device [n_seg]   first entry of each segment
        int32_t *heavy_row = nullptr;      // device [n_heavy] rows that were cut
        int64_t *heavy_seg_ptr = nullptr;  // device [n_heavy+1] their segment ranges
    };
    int32_t seg_len = 0;
    SegSet seg;                        // the cut rows of the whole matrix
    // row groups: maximal runs of rows whose gathered column range is small enough that d-slicing pays
    struct RowGroup {                   // col_hi < col_lo: no entries
        int64_t begin, end;
        bool sliceable;
        int32_t col_lo, col_hi;
        bool lds_table = false;        // the rows gather from <= kLdsTableRows table rows: spmm_ldstab_kernel
    };
    std::vector<RowGroup> groups;
    // L2-swept plan (spmm_swept.hip): built on request (mode 2/3) for long-lived matrices
    int mode = 0;                      // 0 row-wise (+ d-sliced groups), 1 row-wise only, 2 swept wherever the shape
                                       // allows, 3 swept on the row groups where the plan expects L2 re-use to pay
    struct Swept {
        struct Part {                      // one row group handled by the swept kernel
            int64_t row_lo = 0, row_hi = 0;
            int waves = 0, rows_per_wave = 0;          // workgroup shape the entry lists were laid out for
            int lpe = 16;                              // lanes per entry (16: 64-float slices, 32: 128-float slices)
            int32_t n_rowpass = 0, n_win = 0, win_cols = 0, col_lo = 0, col_hi = 0;
            int64_t n_slots = 0, n_partial = 0, n_heavy = 0, partial_base = 0;   // partial rows: workspace rows base..base+n
            int64_t *tptr = nullptr;           // device [n_tasks*n_win+1] slot range of every (wave task, column window)
            int32_t *e_pack = nullptr;         // device [n_slots] (local row << 25) | column; negative: empty slot
            float *e_val = nullptr;            // device [n_slots]
            int32_t *dst = nullptr;            // device [n_tasks*rows_per_wave] >=0 output row, <=-2 the part's partial row -2-p, -1 unused
            int32_t *prow = nullptr;           // device [n_tasks*rows_per_wave] the matrix row behind every accumulator row (cut rows too)
            int32_t *heavy_row = nullptr;      // device [n_heavy]   rows cut into pieces
            int64_t *heavy_seg_ptr = nullptr;  // device [n_heavy+1] their ranges of the part's partial rows
        };
        std::vector<Part> parts;
        std::vector<char> group_swept;     // per entry of `groups`: handled by a part
        SegSet out;                        // segments of the cut rows that no part covers
        int64_t n_partial = 0;             // partial rows of all parts (they follow out.n_seg in the workspace)
        // device [kSweptStreams][8*32] per-XCD sweep counters (zeroed before each launch): one block per stream that has
        // launched products of this CSR, so two streams multiplying the same matrix at once do not pace each other's sweep
        uint32_t *barrier = nullptr;
        mutable hipStream_t barrier_owner[4] = {nullptr, nullptr, nullptr, nullptr};
        mutable int barrier_used = 0;
        int built_mode = 0;
        int lpe = 16;                      // geometry of the parts (spmm_swept.hip): lanes per entry
    } swept;
};


static const int32_t kLdsTableRows = 512;      // x 256 B (one 64-float slice) = 128 KiB of LDS
static const int32_t kDefaultSegLen = 2048;   // measured on C3: 512 -> 20.9 ms/step, 2048 -> 20.6, 4096 -> 20.5
// Default segment length of a matrix with `nnz` stored entries.  A wave walks its segment 8 gathers at a time, so a small matrix
// with a few very long rows (the Seoul graph: 100 item rows of ~4 400 entries) is latency-bound on a few hundred waves at 2048;
// aim at >= 4 096 segments instead.  Seoul-shaped C2 / C1 (876 K entries, whole forward as a hipGraph): 2048 -> 0.967 / 0.232 ms,
// 512 -> 0.607 / 0.145, 256 -> 0.577 / 0.139, 128 -> 0.621 / 0.149, 64 -> 0.652 / 0.169.
static inline int32_t default_seg_len(int64_t nnz)
{
    int32_t s = 64;
    while (s < kDefaultSegLen && (int64_t)s * 4096 < nnz) s *= 2;
    return s;
}

// device copy of a host array (an empty one still gets an allocation: a non-null pointer)
template <typename T>
int upload(T **dptr, const std::vector<T> &h, hipStream_t stream)
{
    HIP_TRY(hipMalloc(dptr, sizeof(T) * std::max<size_t>(h.size(), 1)));
    if (!h.empty()) HIP_TRY(hipMemcpyAsync(*dptr, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, stream));
    return NGCF_OK;
}

// the segment plan on the host (csr.hip): the rows of `ranges` longer than seg_len, cut at seg_len
struct HostSegs {
    std::vector<int32_t> seg_row, heavy_row;
    std::vector<int64_t> seg_begin, heavy_ptr;
};
HostSegs cut_rows(const std::vector<int64_t> &rowptr, const std::vector<std::pair<int64_t, int64_t>> &ranges, int32_t seg_len);
int upload_segset(ngcf_csr::SegSet &s, const HostSegs &h, hipStream_t stream);   // no cut rows: no allocation, null pointers
void free_segset(ngcf_csr::SegSet &s, bool borrowed = false);  // borrowed (a filtered copy): only seg_begin is its own

void free_swept(ngcf_csr *c);                                  // spmm_swept.hip
int build_swept_plan(ngcf_csr *c, hipStream_t stream);         // spmm_swept.hip (reads c->mode)
bool swept_usable(const ngcf_csr *c, int64_t ldE, int d);       // spmm_swept.hip: can this call use the parts?
void prof_mark(hipStream_t stream, int which);                 // library.hip: hipEvent around the SpMM launches

// counter-based hash: the keep masks of node and message dropout and the draws of sample.hip are pure functions of (seed, index)
__host__ __device__ inline uint64_t fmix64(uint64_t x)
{
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}
__device__ inline uint32_t mix32(uint64_t x) { return (uint32_t)fmix64(x); }

// Device-side message dropout (nn.Dropout on a layer's activated output, NGCF.py:142): element (row, col) is dropped iff its
// hash is below msg_drop_thr(p); a kept one is scaled by keep_scale = 1/(1-p).  The forward dense kernels and the backward's
// layer_bwd_pre_kernel must draw the same mask bit for bit: all of them go through these two functions.
__device__ __forceinline__ uint32_t msg_drop_thr(float drop_p)
{
    return drop_p > 0.f ? (uint32_t)((double)drop_p * 4294967296.0) : 0u;
}
__device__ __forceinline__ float msg_drop(float v, uint64_t seed, int64_t row, int col, uint32_t thr, float keep_scale)
{
    const uint32_t h = mix32(seed ^ ((uint64_t)row * 0x9E3779B97F4A7C15ULL + (uint64_t)col));
    return h < thr ? 0.f : v * keep_scale;
}

// Device-side node dropout (NGCF.py:93-100 semantics: keep each stored entry w.p. 1-p, values NOT rescaled,
// cumulative over layers): the entry (i, j) of L survives layer k iff mix32(seed_q ^ key(i, j)) >= thr for every q <= k.
// The key is the entry's (row, column) in L - not its position in some storage order - so every kernel that walks L in
// whatever layout (row-wise CSR, the L2-swept plan, the rows of L^T, a scatter over selected rows) thins it the same way
// without a map between layouts; `transposed` says that the CSR being walked is L^T (its rows are L's columns).
// A 64-bit dropout seed is either a value or - top 16 bits == kSeedPtrTag - the device address (low 48 bits) of a uint64_t that
// holds the value: a captured hipGraph bakes its kernel arguments in, and with the seeds behind a pointer every replay still draws
// new masks (the mirror advances the words on the device).  Values handed over by the mirror are below 2^62, so they never
// carry the tag.  Kernels resolve a seed ONCE, at their start.
constexpr uint64_t kSeedPtrTag = 0xD5EDull;
__device__ inline uint64_t resolve_seed(uint64_t s)
{
    if ((s >> 48) == kSeedPtrTag) s = *reinterpret_cast<const uint64_t *>(s & 0xFFFFFFFFFFFFull);
    // the same in every lane by construction: say so, and the value stays in scalar registers (as a by-value kernel argument would)
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)s), hi = __builtin_amdgcn_readfirstlane((uint32_t)(s >> 32));
    return ((uint64_t)hi << 32) | lo;
}

struct EdgeDrop {
    int n;                  // number of seeds (0 = no dropout)
    uint32_t thr;           // p * 2^32
    uint64_t seed[4];
    int transposed;
};

// The kernel-side form: the seeds resolved (tagged addresses read once, at kernel start) into NAMED scalars - an array indexed by
// a loop counter in a local copy of the argument would live in scratch memory (measured: spmm_kernel 12.6 -> 28.7 us on the Seoul
// graph); the argument struct itself stays in the kernarg segment.
struct EdgeDropR {
    int n;
    uint32_t thr;
    uint64_t s0, s1, s2, s3;
    int transposed;
};

__device__ inline EdgeDropR resolve_drop(const EdgeDrop &dr)
{
    EdgeDropR r;
    r.n = dr.n;
    r.thr = dr.thr;
    r.transposed = dr.transposed;
    r.s0 = dr.n > 0 ? resolve_seed(dr.seed[0]) : 0;
    r.s1 = dr.n > 1 ? resolve_seed(dr.seed[1]) : 0;
    r.s2 = dr.n > 2 ? resolve_seed(dr.seed[2]) : 0;
    r.s3 = dr.n > 3 ? resolve_seed(dr.seed[3]) : 0;
    return r;
}

__device__ inline bool edge_keep(const EdgeDropR &dr, int64_t row, int64_t col)   // row, col of the CSR being walked
{
    const uint64_t i = (uint64_t)(dr.transposed ? col : row), j = (uint64_t)(dr.transposed ? row : col);
    const uint64_t e = ((i << 32) | (j & 0xffffffffull)) * 0x9E3779B97F4A7C15ULL;
    bool keep = true;
    if (dr.n > 0) keep = mix32(dr.s0 ^ e) >= dr.thr;
    if (dr.n > 1) keep = keep && mix32(dr.s1 ^ e) >= dr.thr;
    if (dr.n > 2) keep = keep && mix32(dr.s2 ^ e) >= dr.thr;
    if (dr.n > 3) keep = keep && mix32(dr.s3 ^ e) >= dr.thr;
    return keep;
}


int spmm_dispatch(const ngcf_csr *c, const float *E, int64_t ldE, int d, float *out, int64_t ldo, void *workspace,
                  int64_t workspace_bytes, hipStream_t stream, const EdgeDrop &dr = EdgeDrop{0, 0, {0, 0, 0, 0}, 0});
// swept parts (spmm_swept.hip): kernels + fix-ups of every part; `partial` is the workspace base (rows of dp floats)
int launch_swept(const ngcf_csr *c, const float *E, int64_t ldE, int d, float *out, int64_t ldo, float *partial, int dp,
                 hipStream_t stream, const EdgeDrop &dr);

// ---------------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------------
// value of lane U of this lane's 16-lane row (DPP row_newbcast: one VALU op, no LDS round trip)
template <int U> __device__ inline int row_bcast(int x)
{
    return __builtin_amdgcn_update_dpp(0, x, 0x150 + U, 0xf, 0xf, false);
}
template <int U> __device__ inline float row_bcast(float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x150 + U, 0xf, 0xf, false));
}

template <int VEC> struct VecT;
template <> struct VecT<4> { using type = float4; };
template <> struct VecT<2> { using type = float2; };
template <> struct VecT<1> { using type = float; };

// The register vocabulary of the matrix-core kernels (dense*.hip, bwd_dense.hip, rank*.hip, softmax_tile_device.h, list_*.hip):
// an MFMA 32 x 32 accumulator tile, a lane's 16-byte pieces and the bf16 fragments of 32x32x16.
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));   // native vector: stays in registers inside lambdas
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ inline float4 vfma(float s, float4 x, float4 a)
{
    a.x = fmaf(s, x.x, a.x);
    a.y = fmaf(s, x.y, a.y);
    a.z = fmaf(s, x.z, a.z);
    a.w = fmaf(s, x.w, a.w);
    return a;
}
__device__ inline float vfma(float s, float x, float a) { return fmaf(s, x, a); }
__device__ inline float2 vfma(float s, float2 x, float2 a)
{
    a.x = fmaf(s, x.x, a.x);
    a.y = fmaf(s, x.y, a.y);
    return a;
}
__device__ inline float2 vadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ inline float2 vshfl_xor(float2 a, int m)
{
    a.x = __shfl_xor(a.x, m);
    a.y = __shfl_xor(a.y, m);
    return a;
}
__device__ inline float4 vsel(bool p, float4 a, float4 b) { return p ? a : b; }
__device__ inline float vsel(bool p, float a, float b) { return p ? a : b; }
__device__ inline float4 vzero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
template <int VEC> __device__ inline typename VecT<VEC>::type vzero();
template <> __device__ inline float4 vzero<4>() { return vzero4(); }
template <> __device__ inline float vzero<1>() { return 0.f; }
template <> __device__ inline float2 vzero<2>() { return make_float2(0.f, 0.f); }
__device__ inline float4 vshfl_xor(float4 a, int m)
{
    a.x = __shfl_xor(a.x, m);
    a.y = __shfl_xor(a.y, m);
    a.z = __shfl_xor(a.z, m);
    a.w = __shfl_xor(a.w, m);
    return a;
}
__device__ inline float vshfl_xor(float a, int m) { return __shfl_xor(a, m); }
__device__ inline float4 vadd(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ inline float vadd(float a, float b) { return a + b; }

// A wave's LDS region is its own and its ds operations complete in order: between a phase whose lanes write and one whose other
// lanes read, only the compiler has to be held back.
__device__ inline void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ inline float wave_sum(float x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

// the same xor butterfly (32, 16, .., 1) for the other types the evaluation kernels reduce; every lane ends with the result
__device__ inline int wave_sum(int x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

__device__ inline double wave_sum(double x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

__device__ inline int wave_min(int x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int y = __shfl_xor(x, m);
        x = y < x ? y : x;
    }
    return x;
}

// 64-bit values across lanes, as two 32-bit shuffles: from lane `src`, and from lane (own ^ m)
__device__ inline int64_t shfl_i64(int64_t x, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, src), hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)x >> 32), src);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ inline unsigned long long shfl_xor_u64(unsigned long long x, int m)
{
    const uint32_t lo = __shfl_xor((uint32_t)x, m), hi = __shfl_xor((uint32_t)(x >> 32), m);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ inline double shfl_xor_f64(double x, int m)
{
    return __longlong_as_double((long long)shfl_xor_u64((unsigned long long)__double_as_longlong(x), m));
}

__device__ inline float log_sigmoid(float x)      // F.logsigmoid (bprloss.py:19)
{
    return fminf(x, 0.f) - log1pf(expf(-fabsf(x)));
}

// The first stage's tail in the row losses (ops.hip, loss_rows_device.h), a wave per row and four waves per workgroup: the waves'
// (nl, sq) = (the row's loss, its sum of squares; 0 in a wave without a row) -> the workgroup's two partials part[2*block + 0 / 1].
// (wave, lane: the thread's, which every caller has at hand.)
__device__ inline void bpr_block_partials(int wave, int lane, float nl, float sq, float *__restrict__ part)
{
    __shared__ float sh[8];
    if (lane == 0) {
        sh[wave * 2] = nl;
        sh[wave * 2 + 1] = sq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[2 * (int64_t)blockIdx.x] = (sh[0] + sh[2]) + (sh[4] + sh[6]);
        part[2 * (int64_t)blockIdx.x + 1] = (sh[1] + sh[3]) + (sh[5] + sh[7]);
    }
}

// The second stage of the row losses (ops.hip, loss_rows_device.h), one workgroup of 256: the workgroups' partials
// part[2*i] = -sum logsigmoid, part[2*i + 1] = sum of squares in a fixed order -> *loss (bprloss.py:20-22).
__device__ inline void bpr_finish_block(const float *__restrict__ part, int64_t n_blocks, float wd, float batch_size,
                                        float *__restrict__ loss)
{
    __shared__ float sh[8];
    float nl = 0.f, sq = 0.f;
    for (int64_t i = threadIdx.x; i < n_blocks; i += 256) {
        nl += part[2 * i];
        sq += part[2 * i + 1];
    }
    nl = wave_sum(nl);
    sq = wave_sum(sq);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        sh[wave * 2] = nl;
        sh[wave * 2 + 1] = sq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float a = (sh[0] + sh[2]) + (sh[4] + sh[6]);
        const float b = (sh[1] + sh[3]) + (sh[5] + sh[7]);
        *loss = (a + wd * b) / batch_size;                          // bprloss.py:20-22
    }
}

__device__ inline uint32_t float_key(float x)     // monotone map float -> uint32 (larger float = larger key, NaN above +inf)
{
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}


#endif  // NGCF_COMMON_H
