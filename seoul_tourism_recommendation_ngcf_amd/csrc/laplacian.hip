// The year-slice Laplacians of model/matrix.py:12-83, built on the device straight into CSR.  The state of R between
// years is a user-sorted CSR (rowptr int64 [n_user + 1], item int32, rating fp32); one year is
//   1. bucket    histogram the year's records by user (integer atomics), exclusive scan, scatter (item, sequence number, rating)
//                into per-user buckets; the order inside a bucket is arbitrary, the sequence number decides "the last record wins";
//   2. resolve   per user with new records: the sorted state row and the bucket, ordered by (item, sequence); the last of every
//                item is kept, a rating == 0 (either sign) deletes; the row goes to a scratch row at state offset + bucket offset.
//                Three classes by candidate count (old + new): a wave per row that ranks in registers with cross-lane reads (up to
//                NGCF_LAP_WAVE_LIMIT), a workgroup with a bitonic sort in LDS (up to NGCF_LAP_WG_LIMIT), and above that a workgroup
//                with a per-item table in memory, which is right for any length (a bucket that repeats pairs may exceed n_item);
//   3. degrees   users from the resolved counts, items from an integer histogram; one scan over all N counts is the slice's rowptr;
//   4. emit      after the host's d^-1/2 (numpy's float32 power, not reproducible on the device): the new state, and per entry the
//                two separately rounded fp64 products cast to fp32 - the user row's value and the item row's;
//   5. item rows gathered through the stable order of the int32 item ids (a library sort, the caller's).
// Entries whose fp32 value is 0 stay in the state and in the degrees; they are counted, and only a slice that has some is compacted
// (ngcf_laplacian_drop_zeros).  No floating-point atomics: the same input gives the same bytes.
#include "common.h"

#define NGCF_LAP_WAVE_LIMIT 64
#define NGCF_LAP_WG_LIMIT 2048

namespace {

constexpr int kLapThreads = 256;
constexpr int kLapWaves = kLapThreads / 64;
constexpr int kScanPer = 8, kScanTile = kLapThreads * kScanPer;
constexpr uint32_t kLapOld = 0xffffffffu;           // table mark of the long-row class: the state's entry stands

static_assert(NGCF_LAP_WAVE_LIMIT == 64, "the wave class holds one candidate per lane");
static_assert((NGCF_LAP_WG_LIMIT & (NGCF_LAP_WG_LIMIT - 1)) == 0 && NGCF_LAP_WG_LIMIT >= 2 * kLapThreads, "bitonic sort of a power of two");

// ---- exclusive scan of int32 counts into int64 offsets -------------------------------------------------------------------------
// exclusive prefix of v over the workgroup's 256 threads; total: the sum over all of them
__device__ inline long long block_exscan(long long v, long long *s_wave, long long &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();                                 // the previous call's sums have been read
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    long long off = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kLapWaves; ++w) {
        const long long s = s_wave[w];
        off += w < wave ? s : 0;
        total += s;
    }
    return off + inc - v;
}

__global__ __launch_bounds__(kLapThreads) void lap_scan_sums_kernel(const int32_t *__restrict__ in, int64_t n, long long *__restrict__ sums)
{
    __shared__ long long s_wave[kLapWaves];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
    long long v = 0;
#pragma unroll
    for (int q = 0; q < kScanPer; ++q)
        if (base + q < n) v += in[base + q];
    long long total;
    block_exscan(v, s_wave, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kLapThreads) void lap_scan_tiles_kernel(long long *sums, int64_t n_tiles)
{
    __shared__ long long s_wave[kLapWaves];
    long long running = 0;
    for (int64_t base = 0; base < n_tiles; base += kLapThreads) {
        const int64_t t = base + threadIdx.x;
        const long long v = t < n_tiles ? sums[t] : 0;
        long long total;
        const long long ex = block_exscan(v, s_wave, total);
        if (t < n_tiles) sums[t] = running + ex;
        running += total;
    }
}

// out[i] = offset + sum of in[0 .. i), i in [0, n]
__global__ __launch_bounds__(kLapThreads) void lap_scan_write_kernel(const int32_t *__restrict__ in, int64_t n, const long long *__restrict__ sums,
                                                                     int64_t *__restrict__ out)
{
    __shared__ long long s_wave[kLapWaves];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
    int32_t c[kScanPer];
    long long v = 0;
#pragma unroll
    for (int q = 0; q < kScanPer; ++q) {
        c[q] = base + q < n ? in[base + q] : 0;
        v += c[q];
    }
    long long total;
    long long at = sums[blockIdx.x] + block_exscan(v, s_wave, total);
#pragma unroll
    for (int q = 0; q < kScanPer; ++q) {
        if (base + q <= n) out[base + q] = at;           // i == n: the grand total (its tile exists: the grid covers n + 1 offsets)
        at += c[q];
    }
}

int64_t scan_tiles(int64_t n) { return (n + 1 + kScanTile - 1) / kScanTile; }

int scan_counts(const int32_t *in, int64_t n, int64_t *out, void *workspace, hipStream_t stream)
{
    long long *sums = (long long *)workspace;
    const int64_t tiles = scan_tiles(n);
    lap_scan_sums_kernel<<<dim3((unsigned)tiles), kLapThreads, 0, stream>>>(in, n, sums);
    LAUNCH_CHECK();
    lap_scan_tiles_kernel<<<dim3(1), kLapThreads, 0, stream>>>(sums, tiles);
    LAUNCH_CHECK();
    lap_scan_write_kernel<<<dim3((unsigned)tiles), kLapThreads, 0, stream>>>(in, n, sums, out);
    LAUNCH_CHECK();
    return NGCF_OK;
}

// ---- 1. bucket --------------------------------------------------------------------------------------------------------------------
__device__ inline bool lap_valid(int64_t u, int64_t i, int64_t n_user, int64_t n_item) { return u >= 0 && u < n_user && i >= 0 && i < n_item; }

// A record with an id outside its range is reported and left out by BOTH kernels, so counts and cursors agree.
__global__ __launch_bounds__(kLapThreads) void lap_bucket_count_kernel(const int64_t *__restrict__ userid, const int64_t *__restrict__ itemid,
                                                                       int64_t T, int64_t n_user, int64_t n_item, int32_t *cnt, int32_t *info)
{
    bool bad = false;
    for (int64_t t = (int64_t)blockIdx.x * kLapThreads + threadIdx.x; t < T; t += (int64_t)gridDim.x * kLapThreads) {
        const int64_t u = userid[t];
        if (lap_valid(u, itemid[t], n_user, n_item)) atomicAdd(&cnt[u], 1);
        else bad = true;
    }
    if (bad) atomicOr(&info[0], 1);
}

// cnt[u] counts down to 0: the bucket fills from its end, in whatever order the records arrive
__global__ __launch_bounds__(kLapThreads) void lap_bucket_scatter_kernel(
    const int64_t *__restrict__ userid, const int64_t *__restrict__ itemid, const float *__restrict__ rating, int64_t T, int64_t n_user,
    int64_t n_item, const int64_t *__restrict__ bptr, int32_t *cnt, int32_t *__restrict__ b_item, int32_t *__restrict__ b_seq,
    float *__restrict__ b_rating)
{
    for (int64_t t = (int64_t)blockIdx.x * kLapThreads + threadIdx.x; t < T; t += (int64_t)gridDim.x * kLapThreads) {
        const int64_t u = userid[t], i = itemid[t];
        if (!lap_valid(u, i, n_user, n_item)) continue;
        const int32_t left = atomicSub(&cnt[u], 1);
        const int64_t lo = bptr[u], pos = lo + left - 1;
        if (left < 1 || pos >= T) continue;              // cannot happen while the input stays as the count kernel saw it
        b_item[pos] = (int32_t)i;
        b_seq[pos] = (int32_t)t;
        b_rating[pos] = rating[t];
    }
}

// rows of the workgroup class and of the long-row class: they size the launches and the long-row tables
__global__ __launch_bounds__(kLapThreads) void lap_classify_kernel(const int64_t *__restrict__ old_rowptr, const int64_t *__restrict__ bptr,
                                                                   int64_t n_user, int32_t *info)
{
    for (int64_t u = (int64_t)blockIdx.x * kLapThreads + threadIdx.x; u < n_user; u += (int64_t)gridDim.x * kLapThreads) {
        const int64_t n_new = bptr[u + 1] - bptr[u], c = n_new + (old_rowptr[u + 1] - old_rowptr[u]);
        if (n_new > 0 && c > NGCF_LAP_WG_LIMIT) atomicAdd(&info[2], 1);
        else if (n_new > 0 && c > NGCF_LAP_WAVE_LIMIT) atomicAdd(&info[1], 1);
    }
}

// ---- 2. resolve rows ----------------------------------------------------------------------------------------------------------------
struct LapState {                        // the state of R before this year, and the year's buckets
    const int64_t *rowptr;
    const int32_t *item;
    const float *rating;
    int64_t nnz;
    const int64_t *bptr;
    int64_t T;
    int64_t n_user, n_item;
};

struct LapRow {
    int64_t o_lo, b_lo, t_lo;            // first entry in the state, in the buckets, in the scratch rows (o_lo + b_lo)
    int64_t n_old, n_new;
};

// false: the row pointers decrease or leave their arrays (then the row counts as empty, so nothing is read through them)
__device__ inline bool lap_row(const LapState &s, int64_t u, LapRow &r)
{
    const int64_t o_lo = s.rowptr[u], o_hi = s.rowptr[u + 1], b_lo = s.bptr[u], b_hi = s.bptr[u + 1];
    const bool ok = o_lo >= 0 && o_hi >= o_lo && o_hi <= s.nnz && o_hi - o_lo <= s.n_item && b_lo >= 0 && b_hi >= b_lo && b_hi <= s.T;
    r.o_lo = o_lo;
    r.b_lo = b_lo;
    r.t_lo = o_lo + b_lo;
    r.n_old = ok ? o_hi - o_lo : 0;
    r.n_new = ok ? b_hi - b_lo : 0;
    return ok;
}

// (item, sequence + 1) as one key; the state's entry has sequence part 0, so every record of the year sorts behind it
__device__ inline unsigned long long lap_key(int32_t item, uint32_t seq1) { return ((unsigned long long)(uint32_t)item << 32) | seq1; }
__device__ inline bool lap_nonzero(float r) { return (__float_as_uint(r) << 1) != 0; }          // != 0 for either sign of zero, whatever the denormal mode

__device__ inline unsigned long long readlane_u64(unsigned long long v, int l)
{
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, l), hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

// Wave class: a candidate per lane.  This kernel visits every user: it also writes the count of a row without new records (which is
// copied through later) and reports bad row pointers.
__global__ __launch_bounds__(kLapThreads) void lap_resolve_wave_kernel(
    LapState s, const int32_t *__restrict__ b_item, const int32_t *__restrict__ b_seq, const float *__restrict__ b_rating,
    int32_t *__restrict__ t_item, float *__restrict__ t_rating, int32_t *__restrict__ deg, int32_t *status)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t u = (int64_t)blockIdx.x * kLapWaves + wave; u < s.n_user; u += (int64_t)gridDim.x * kLapWaves) {
        LapRow r;
        if (!lap_row(s, u, r)) {
            if (lane == 0) {
                atomicOr(status, 2);
                deg[u] = 0;
            }
            continue;
        }
        if (r.n_new == 0) {
            if (lane == 0) deg[u] = (int32_t)r.n_old;
            continue;
        }
        const int64_t c64 = r.n_old + r.n_new;
        if (c64 > NGCF_LAP_WAVE_LIMIT) continue;                          // the other classes'
        const int c = (int)c64, n_old = (int)r.n_old;
        const bool mine = lane < c;
        int32_t item = 0;
        uint32_t seq1 = 0;
        float rat = 0.f;
        if (mine) {
            if (lane < n_old) {
                item = s.item[r.o_lo + lane];
                rat = s.rating[r.o_lo + lane];
            } else {
                const int64_t p = r.b_lo + (lane - n_old);
                item = b_item[p];
                seq1 = (uint32_t)b_seq[p] + 1u;
                rat = b_rating[p];
            }
        }
        const unsigned long long key = lap_key(item, seq1);
        bool later = false;                                               // a later candidate has the same item
        for (int j = 0; j < c; ++j) {
            const unsigned long long kj = readlane_u64(key, j);
            later |= (uint32_t)(kj >> 32) == (uint32_t)item && kj > key;
        }
        const bool keep = mine && !later && lap_nonzero(rat);
        const unsigned long long kept = __ballot(keep);
        int pos = 0;                                                      // kept items are distinct: the rank among them
        for (unsigned long long m = kept; m; m &= m - 1) {
            const int j = __ffsll(m) - 1;
            pos += (uint32_t)__builtin_amdgcn_readlane(item, j) < (uint32_t)item ? 1 : 0;
        }
        if (keep) {
            t_item[r.t_lo + pos] = item;
            t_rating[r.t_lo + pos] = rat;
        }
        if (lane == 0) deg[u] = __popcll(kept);
    }
}

// Workgroup class: the candidates sorted in LDS (bitonic, padded to a power of two with keys above every real one), the last of
// every item flagged, the survivors written in order.
__global__ __launch_bounds__(kLapThreads) void lap_resolve_block_kernel(
    LapState s, const int32_t *__restrict__ b_item, const int32_t *__restrict__ b_seq, const float *__restrict__ b_rating,
    int32_t *__restrict__ t_item, float *__restrict__ t_rating, int32_t *__restrict__ deg)
{
    __shared__ unsigned long long s_key[NGCF_LAP_WG_LIMIT];
    __shared__ float s_rat[NGCF_LAP_WG_LIMIT];
    __shared__ long long s_wave[kLapWaves];
    const int tid = threadIdx.x;
    for (int64_t u = blockIdx.x; u < s.n_user; u += gridDim.x) {
        LapRow r;
        const bool ok = lap_row(s, u, r);
        const int64_t c64 = r.n_old + r.n_new;
        if (!ok || r.n_new == 0 || c64 <= NGCF_LAP_WAVE_LIMIT || c64 > NGCF_LAP_WG_LIMIT) continue;       // the same in every thread
        const int c = (int)c64, n_old = (int)r.n_old;
        int P = 2 * NGCF_LAP_WAVE_LIMIT;
        while (P < c) P <<= 1;
        for (int k = tid; k < P; k += kLapThreads) {
            unsigned long long key = ~0ull;
            float rat = 0.f;
            if (k < n_old) {
                key = lap_key(s.item[r.o_lo + k], 0u);
                rat = s.rating[r.o_lo + k];
            } else if (k < c) {
                const int64_t p = r.b_lo + (k - n_old);
                key = lap_key(b_item[p], (uint32_t)b_seq[p] + 1u);
                rat = b_rating[p];
            }
            s_key[k] = key;
            s_rat[k] = rat;
        }
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < P / 2; t += kLapThreads) {
                    const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                    const unsigned long long ka = s_key[a], kb = s_key[b];
                    if ((ka > kb) == ((a & k) == 0)) {
                        s_key[a] = kb;
                        s_key[b] = ka;
                        const float ra = s_rat[a];
                        s_rat[a] = s_rat[b];
                        s_rat[b] = ra;
                    }
                }
                __syncthreads();
            }
        long long running = 0;
        for (int base = 0; base < c; base += kLapThreads) {
            const int k = base + tid;
            bool keep = false;
            int32_t item = 0;
            float rat = 0.f;
            if (k < c) {
                item = (int32_t)(s_key[k] >> 32);
                rat = s_rat[k];
                const bool last = k + 1 == c || (int32_t)(s_key[k + 1] >> 32) != item;
                keep = last && lap_nonzero(rat);
            }
            long long total;
            const long long pos = running + block_exscan(keep ? 1 : 0, s_wave, total);
            if (keep) {
                t_item[r.t_lo + pos] = item;
                t_rating[r.t_lo + pos] = rat;
            }
            running += total;
        }
        if (tid == 0) deg[u] = (int32_t)running;
        __syncthreads();                                                  // the next row overwrites the keys
    }
}

// The table of a long-row workgroup lives in memory and is shared by the workgroup's waves between barriers: every access goes to
// the device's coherent level, past the CU's cache.
__device__ inline uint32_t tab_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void tab_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Long-row class, any length: tab_seq[item] = the largest sequence + 1 among the year's records of the item (integer max: order
// free), or kLapOld where only the state has the item; tab_rat[item] = the winner's rating bits; then one ordered sweep of the items.
__global__ __launch_bounds__(kLapThreads) void lap_resolve_long_kernel(
    LapState s, const int32_t *__restrict__ b_item, const int32_t *__restrict__ b_seq, const float *__restrict__ b_rating,
    int32_t *__restrict__ t_item, float *__restrict__ t_rating, int32_t *__restrict__ deg, uint32_t *tables, int64_t n_tables, int32_t *status)
{
    __shared__ long long s_wave[kLapWaves];
    const int tid = threadIdx.x;
    uint32_t *tab_seq = tables ? tables + (int64_t)blockIdx.x * 2 * s.n_item : nullptr, *tab_rat = tables ? tab_seq + s.n_item : nullptr;
    for (int64_t u = blockIdx.x; u < s.n_user; u += gridDim.x) {
        LapRow r;
        const bool ok = lap_row(s, u, r);
        if (!ok || r.n_new == 0 || r.n_old + r.n_new <= NGCF_LAP_WG_LIMIT) continue;                    // the same in every thread
        if (!tables || (int64_t)blockIdx.x >= n_tables) {                    // no table was handed over for a row that needs one
            if (tid == 0) {
                atomicOr(status, 4);
                deg[u] = 0;
            }
            continue;
        }
        for (int64_t i = tid; i < s.n_item; i += kLapThreads) tab_store(&tab_seq[i], 0u);
        __syncthreads();
        bool bad = false;
        for (int64_t j = tid; j < r.n_new; j += kLapThreads) {
            const int32_t item = b_item[r.b_lo + j];
            if (item >= 0 && item < s.n_item) atomicMax(&tab_seq[item], (uint32_t)b_seq[r.b_lo + j] + 1u);
            else bad = true;                                              // the scatter wrote checked ids only: never, unless overwritten
        }
        __syncthreads();
        for (int64_t j = tid; j < r.n_new; j += kLapThreads) {
            const int32_t item = b_item[r.b_lo + j];
            if (item < 0 || item >= s.n_item) continue;
            if (tab_load(&tab_seq[item]) == (uint32_t)b_seq[r.b_lo + j] + 1u) tab_store(&tab_rat[item], __float_as_uint(b_rating[r.b_lo + j]));
        }
        for (int64_t k = tid; k < r.n_old; k += kLapThreads) {
            const int32_t item = s.item[r.o_lo + k];
            if (item < 0 || item >= s.n_item) {
                bad = true;
                continue;
            }
            if (tab_load(&tab_seq[item]) == 0u) {                         // no record of the year names it (they left a value >= 1)
                tab_store(&tab_seq[item], kLapOld);
                tab_store(&tab_rat[item], __float_as_uint(s.rating[r.o_lo + k]));
            }
        }
        if (bad) atomicOr(status, 2);
        __syncthreads();
        long long running = 0;
        for (int64_t base = 0; base < s.n_item; base += kLapThreads) {
            const int64_t i = base + tid;
            bool keep = false;
            float rat = 0.f;
            if (i < s.n_item && tab_load(&tab_seq[i]) != 0u) {
                rat = __uint_as_float(tab_load(&tab_rat[i]));
                keep = lap_nonzero(rat);
            }
            long long total;
            const long long pos = running + block_exscan(keep ? 1 : 0, s_wave, total);
            if (keep) {
                t_item[r.t_lo + pos] = (int32_t)i;
                t_rating[r.t_lo + pos] = rat;
            }
            running += total;
        }
        if (tid == 0) deg[u] = (int32_t)running;
        __syncthreads();                                                  // the next row clears the table
    }
}

// where the resolved row of user u lies: the scratch row if the year touched it, else the state's own
__device__ inline void lap_source(const LapState &s, const int32_t *t_item, const float *t_rating, int64_t u, const int32_t *&item,
                                  const float *&rating)
{
    LapRow r;
    const bool ok = lap_row(s, u, r);
    const bool fresh = ok && r.n_new > 0;
    item = fresh ? t_item + r.t_lo : s.item + (ok ? r.o_lo : 0);
    rating = fresh ? t_rating + r.t_lo : s.rating + (ok ? r.o_lo : 0);
}

// ---- 3. item degrees ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLapThreads) void lap_item_degree_kernel(LapState s, const int32_t *__restrict__ t_item, const float *__restrict__ t_rating,
                                                                      int32_t *deg, int32_t *status)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    bool bad = false;
    for (int64_t u = (int64_t)blockIdx.x * kLapWaves + wave; u < s.n_user; u += (int64_t)gridDim.x * kLapWaves) {
        const int32_t *item;
        const float *rating;
        lap_source(s, t_item, t_rating, u, item, rating);
        const int n = deg[u];                                             // <= the row's candidates, by construction
        for (int k = lane; k < n; k += 64) {
            const int32_t i = item[k];
            if (i >= 0 && i < s.n_item) atomicAdd(&deg[s.n_user + i], 1);
            else bad = true;
        }
    }
    if (bad) atomicOr(status, 2);
}

// ---- 4. normalise and emit ------------------------------------------------------------------------------------------------------------
// the reference's (d_i * a_ij) * d_j in float64, cast to float32 (matrix.py:62): two roundings in fp64, one to fp32, no FMA
__device__ inline float lap_value(float da, float w, float db)
{
#pragma clang fp contract(off)
    const double p = (double)da * (double)w;
    const double q = p * (double)db;
    return (float)q;
}

__global__ __launch_bounds__(kLapThreads) void lap_emit_kernel(
    LapState s, const int32_t *__restrict__ t_item, const float *__restrict__ t_rating, const int32_t *__restrict__ deg,
    const int64_t *__restrict__ rowptr, const float *__restrict__ ds, int64_t nnz, int32_t *__restrict__ s_item, float *__restrict__ s_rating,
    int32_t *__restrict__ s_user, int32_t *__restrict__ colidx, float *__restrict__ vals, float *__restrict__ vals_item,
    unsigned long long *zeros, int32_t *status)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned long long n_zero = 0;
    bool bad = false;
    for (int64_t u = (int64_t)blockIdx.x * kLapWaves + wave; u < s.n_user; u += (int64_t)gridDim.x * kLapWaves) {
        const int32_t *item;
        const float *rating;
        lap_source(s, t_item, t_rating, u, item, rating);
        const int64_t lo = rowptr[u];
        const int n = deg[u];
        if (lo < 0 || n < 0 || lo + n > nnz) {                            // rowptr is this library's own scan of deg: never, unless overwritten
            bad = true;
            continue;
        }
        const float du = ds[u];
        for (int k = lane; k < n; k += 64) {
            const int32_t i = item[k];
            const float w = rating[k];
            const bool in = i >= 0 && i < s.n_item;
            const float di = in ? ds[s.n_user + i] : 0.f;
            const float vu = lap_value(du, w, di), vi = lap_value(di, w, du);
            bad |= !in;
            s_item[lo + k] = i;
            s_rating[lo + k] = w;
            s_user[lo + k] = (int32_t)u;
            colidx[lo + k] = (int32_t)(s.n_user + i);
            vals[lo + k] = vu;
            vals_item[lo + k] = vi;
            n_zero += (lap_nonzero(vu) ? 0 : 1) + (lap_nonzero(vi) ? 0 : 1);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n_zero += __shfl_xor(n_zero, d);
    if (lane == 0 && n_zero) atomicAdd(zeros, n_zero);
    if (bad) atomicOr(status, 2);
}

// ---- 5. item rows ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLapThreads) void lap_item_rows_kernel(const int64_t *__restrict__ order, const int32_t *__restrict__ s_user,
                                                                    const float *__restrict__ vals_item, int64_t nnz, int32_t *__restrict__ colidx,
                                                                    float *__restrict__ vals, int32_t *status)
{
    bool bad = false;
    for (int64_t e = (int64_t)blockIdx.x * kLapThreads + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kLapThreads) {
        const int64_t p = order[e];
        const bool in = p >= 0 && p < nnz;
        colidx[e] = in ? s_user[p] : 0;
        vals[e] = in ? vals_item[p] : 0.f;
        bad |= !in;
    }
    if (bad) atomicOr(status, 1);
}

// ---- zeros out of a finished slice ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLapThreads) void lap_count_nonzero_kernel(const int64_t *__restrict__ rowptr, const float *__restrict__ vals, int64_t n_rows,
                                                                        int64_t nnz, int32_t *__restrict__ cnt)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * kLapWaves + wave; r < n_rows; r += (int64_t)gridDim.x * kLapWaves) {
        const int64_t lo = rowptr[r], hi = rowptr[r + 1];
        int n = 0;
        if (lo >= 0 && hi <= nnz)
            for (int64_t k = lo + lane; k < hi; k += 64) n += lap_nonzero(vals[k]) ? 1 : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
        if (lane == 0) cnt[r] = n;
    }
}

__global__ __launch_bounds__(kLapThreads) void lap_drop_zeros_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const float *__restrict__ vals, int64_t n_rows, int64_t nnz,
    const int64_t *__restrict__ out_rowptr, int32_t *__restrict__ out_colidx, float *__restrict__ out_vals, int64_t out_cap)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * kLapWaves + wave; r < n_rows; r += (int64_t)gridDim.x * kLapWaves) {
        const int64_t lo = rowptr[r], hi = rowptr[r + 1];
        if (lo < 0 || hi > nnz) continue;
        int64_t at = out_rowptr[r];
        for (int64_t base = lo; base < hi; base += 64) {
            const int64_t k = base + lane;
            const float v = k < hi ? vals[k] : 0.f;
            const bool keep = k < hi && lap_nonzero(v);
            const unsigned long long m = __ballot(keep);
            const int64_t pos = at + __popcll(m & ((1ull << lane) - 1ull));
            if (keep && pos >= 0 && pos < out_cap) {
                out_colidx[pos] = colidx[k];
                out_vals[pos] = v;
            }
            at += __popcll(m);
        }
    }
}

int lap_sizes(const char *fn, int64_t n_user, int64_t n_item, int64_t T)
{
    if (n_user < 0 || n_item < 0 || T < 0)
        return fail(NGCF_ERR_ARG, "laplacian: %s: negative count (n_user=%lld, n_item=%lld, records=%lld)", fn, (long long)n_user,
                    (long long)n_item, (long long)T);
    if (n_user >= (1ll << 31) || n_item >= (1ll << 31) || n_user + n_item >= (1ll << 31))
        return fail(NGCF_ERR_ARG, "laplacian: %s: n_user + n_item = %lld does not fit 31 bits", fn, (long long)n_user + (long long)n_item);
    if (T > (1ll << 31) - 1)
        return fail(NGCF_ERR_ARG, "laplacian: %s: %lld records in one year, more than 2^31 - 1", fn, (long long)T);
    return NGCF_OK;
}

int wave_rows_grid(int64_t n_rows) { return grid_for(n_rows, kLapWaves); }

}  // namespace

extern "C" int ngcf_laplacian_limits(int *wave_limit, int *workgroup_limit)
{
    if (wave_limit) *wave_limit = NGCF_LAP_WAVE_LIMIT;
    if (workgroup_limit) *workgroup_limit = NGCF_LAP_WG_LIMIT;
    return NGCF_OK;
}

extern "C" int64_t ngcf_laplacian_workspace_bytes(int64_t n_user, int64_t n_item)
{
    if (n_user < 0 || n_item < 0 || n_user + n_item >= (1ll << 31)) return -1;
    return scan_tiles(n_user + n_item) * (int64_t)sizeof(long long);
}

extern "C" int ngcf_laplacian_bucket(const int64_t *userid, const int64_t *itemid, const float *rating, int64_t T, int64_t n_user,
                                     int64_t n_item, const int64_t *old_rowptr, int32_t *count, int64_t *bptr, int32_t *b_item,
                                     int32_t *b_seq, float *b_rating, int32_t *info, void *workspace, int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = lap_sizes("bucket", n_user, n_item, T)) return rc;
    if (!old_rowptr || !count || !bptr || !info || !workspace || (T > 0 && (!userid || !itemid || !rating || !b_item || !b_seq || !b_rating)))
        return fail(NGCF_ERR_ARG, "laplacian: bucket: null argument");
    if (workspace_bytes < ngcf_laplacian_workspace_bytes(n_user, n_item))
        return fail(NGCF_ERR_WORKSPACE, "laplacian: bucket: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                    (long long)ngcf_laplacian_workspace_bytes(n_user, n_item));
    HIP_TRY(hipMemsetAsync(info, 0, 4 * sizeof(int32_t), stream));
    if (n_user > 0) HIP_TRY(hipMemsetAsync(count, 0, (size_t)n_user * sizeof(int32_t), stream));
    if (T > 0) {
        lap_bucket_count_kernel<<<dim3(grid_for(T, kLapThreads)), kLapThreads, 0, stream>>>(userid, itemid, T, n_user, n_item, count, info);
        LAUNCH_CHECK();
    }
    if (int rc = scan_counts(count, n_user, bptr, workspace, stream)) return rc;
    if (T > 0) {
        lap_bucket_scatter_kernel<<<dim3(grid_for(T, kLapThreads)), kLapThreads, 0, stream>>>(userid, itemid, rating, T, n_user, n_item, bptr,
                                                                                                 count, b_item, b_seq, b_rating);
        LAUNCH_CHECK();
    }
    lap_classify_kernel<<<dim3(grid_for(n_user, kLapThreads)), kLapThreads, 0, stream>>>(old_rowptr, bptr, n_user, info);
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_laplacian_resolve(const int64_t *old_rowptr, const int32_t *old_item, const float *old_rating, int64_t old_nnz,
                                      const int64_t *bptr, const int32_t *b_item, const int32_t *b_seq, const float *b_rating, int64_t T,
                                      int64_t n_user, int64_t n_item, int64_t n_block_rows, int64_t n_long_rows, int32_t *t_item,
                                      float *t_rating, int32_t *deg, int64_t *rowptr, uint32_t *long_tables, int64_t n_tables,
                                      int32_t *status, void *workspace, int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = lap_sizes("resolve", n_user, n_item, T)) return rc;
    if (old_nnz < 0 || n_block_rows < 0 || n_long_rows < 0 || n_tables < 0)
        return fail(NGCF_ERR_ARG, "laplacian: resolve: negative count (old_nnz=%lld, rows of the classes %lld / %lld, tables=%lld)",
                    (long long)old_nnz, (long long)n_block_rows, (long long)n_long_rows, (long long)n_tables);
    if (!old_rowptr || !bptr || !deg || !rowptr || !status || !workspace || (old_nnz > 0 && (!old_item || !old_rating)) ||
        (T > 0 && (!b_item || !b_seq || !b_rating)) || (old_nnz + T > 0 && (!t_item || !t_rating)) || (n_tables > 0 && !long_tables))
        return fail(NGCF_ERR_ARG, "laplacian: resolve: null argument");
    if (n_long_rows > 0 && n_tables == 0) return fail(NGCF_ERR_ARG, "laplacian: resolve: %lld long rows and no table", (long long)n_long_rows);
    if (workspace_bytes < ngcf_laplacian_workspace_bytes(n_user, n_item))
        return fail(NGCF_ERR_WORKSPACE, "laplacian: resolve: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                    (long long)ngcf_laplacian_workspace_bytes(n_user, n_item));
    const LapState s{old_rowptr, old_item, old_rating, old_nnz, bptr, T, n_user, n_item};
    if (n_item > 0) HIP_TRY(hipMemsetAsync(deg + n_user, 0, (size_t)n_item * sizeof(int32_t), stream));
    if (n_user > 0) {
        lap_resolve_wave_kernel<<<dim3(wave_rows_grid(n_user)), kLapThreads, 0, stream>>>(s, b_item, b_seq, b_rating, t_item, t_rating, deg,
                                                                                           status);
        LAUNCH_CHECK();
        if (n_block_rows > 0) {
            const int64_t blocks = std::min<int64_t>(n_user, 256 * 8);
            lap_resolve_block_kernel<<<dim3((unsigned)blocks), kLapThreads, 0, stream>>>(s, b_item, b_seq, b_rating, t_item, t_rating, deg);
            LAUNCH_CHECK();
        }
        if (n_long_rows > 0) {
            const int64_t blocks = std::min<int64_t>(n_tables, n_user);
            lap_resolve_long_kernel<<<dim3((unsigned)blocks), kLapThreads, 0, stream>>>(s, b_item, b_seq, b_rating, t_item, t_rating, deg,
                                                                                         long_tables, n_tables, status);
            LAUNCH_CHECK();
        }
        lap_item_degree_kernel<<<dim3(wave_rows_grid(n_user)), kLapThreads, 0, stream>>>(s, t_item, t_rating, deg, status);
        LAUNCH_CHECK();
    }
    return scan_counts(deg, n_user + n_item, rowptr, workspace, stream);
}

extern "C" int ngcf_laplacian_emit(const int64_t *old_rowptr, const int32_t *old_item, const float *old_rating, int64_t old_nnz,
                                   const int64_t *bptr, int64_t T, const int32_t *t_item, const float *t_rating, int64_t n_user,
                                   int64_t n_item, const int32_t *deg, const int64_t *rowptr, const float *ds, int64_t nnz, int32_t *s_item,
                                   float *s_rating, int32_t *s_user, int32_t *colidx, float *vals, float *vals_item, uint64_t *zeros,
                                   int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = lap_sizes("emit", n_user, n_item, T)) return rc;
    if (old_nnz < 0 || nnz < 0) return fail(NGCF_ERR_ARG, "laplacian: emit: negative count (old_nnz=%lld, nnz=%lld)", (long long)old_nnz, (long long)nnz);
    if (!old_rowptr || !bptr || !deg || !rowptr || !ds || !zeros || !status || (old_nnz > 0 && (!old_item || !old_rating)) ||
        (old_nnz + T > 0 && (!t_item || !t_rating)) || (nnz > 0 && (!s_item || !s_rating || !s_user || !colidx || !vals || !vals_item)))
        return fail(NGCF_ERR_ARG, "laplacian: emit: null argument");
    HIP_TRY(hipMemsetAsync(zeros, 0, sizeof(uint64_t), stream));
    if (n_user == 0 || nnz == 0) return NGCF_OK;
    const LapState s{old_rowptr, old_item, old_rating, old_nnz, bptr, T, n_user, n_item};
    lap_emit_kernel<<<dim3(wave_rows_grid(n_user)), kLapThreads, 0, stream>>>(s, t_item, t_rating, deg, rowptr, ds, nnz, s_item, s_rating, s_user,
                                                                               colidx, vals, vals_item, (unsigned long long *)zeros, status);
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_laplacian_item_rows(const int64_t *order, const int32_t *s_user, const float *vals_item, int64_t nnz, int32_t *colidx,
                                        float *vals, int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (nnz < 0) return fail(NGCF_ERR_ARG, "laplacian: item_rows: negative count (nnz=%lld)", (long long)nnz);
    if (!status || (nnz > 0 && (!order || !s_user || !vals_item || !colidx || !vals))) return fail(NGCF_ERR_ARG, "laplacian: item_rows: null argument");
    if (nnz == 0) return NGCF_OK;
    lap_item_rows_kernel<<<dim3(grid_for(nnz, kLapThreads)), kLapThreads, 0, stream>>>(order, s_user, vals_item, nnz, colidx, vals, status);
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_laplacian_drop_zeros(const int64_t *rowptr, const int32_t *colidx, const float *vals, int64_t n_rows, int64_t nnz,
                                         int32_t *count, int64_t *out_rowptr, int32_t *out_colidx, float *out_vals, int64_t out_nnz,
                                         void *workspace, int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_rows < 0 || nnz < 0 || out_nnz < 0)
        return fail(NGCF_ERR_ARG, "laplacian: drop_zeros: negative count (n_rows=%lld, nnz=%lld, out_nnz=%lld)", (long long)n_rows, (long long)nnz,
                    (long long)out_nnz);
    if (n_rows >= (1ll << 31)) return fail(NGCF_ERR_ARG, "laplacian: drop_zeros: n_rows = %lld does not fit 31 bits", (long long)n_rows);
    if (!rowptr || !count || !out_rowptr || !workspace || (nnz > 0 && (!colidx || !vals)) || (out_nnz > 0 && (!out_colidx || !out_vals)))
        return fail(NGCF_ERR_ARG, "laplacian: drop_zeros: null argument");
    if (workspace_bytes < scan_tiles(n_rows) * (int64_t)sizeof(long long))
        return fail(NGCF_ERR_WORKSPACE, "laplacian: drop_zeros: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                    (long long)(scan_tiles(n_rows) * (int64_t)sizeof(long long)));
    if (n_rows > 0) {
        lap_count_nonzero_kernel<<<dim3(wave_rows_grid(n_rows)), kLapThreads, 0, stream>>>(rowptr, vals, n_rows, nnz, count);
        LAUNCH_CHECK();
    }
    if (int rc = scan_counts(count, n_rows, out_rowptr, workspace, stream)) return rc;
    if (n_rows > 0 && out_nnz > 0) {
        lap_drop_zeros_kernel<<<dim3(wave_rows_grid(n_rows)), kLapThreads, 0, stream>>>(rowptr, colidx, vals, n_rows, nnz, out_rowptr, out_colidx,
                                                                                         out_vals, out_nnz);
        LAUNCH_CHECK();
    }
    return NGCF_OK;
}
