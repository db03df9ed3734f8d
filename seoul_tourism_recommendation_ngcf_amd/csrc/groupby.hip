// Group-by-sum on packed integer keys, and the decimal string code of the reference's user key: what pandas'
// pivot_table(aggfunc='sum') and the np.sort(unique) of utils.py:46-48, 70-74 compute, in single passes over integer columns.
//   insert   every row's K key columns are packed into one word of <= 63 bits (first column most significant, so the word's order
//            is the lexicographic order of the columns; all ones stays free to mean "empty slot") and inserted into an
//            open-addressing table in memory: home slot fmix64(key) & (capacity - 1), linear probing, the slot claimed by a 64-bit
//            compare-and-swap at agent scope.  A slot only ever goes from empty to one key, so a stale "empty" is harmless: the swap
//            returns what is there.  The V sums are int64 integer atomic adds into the slot's accumulators: associative, so the
//            result does not depend on arrival order.  No floating-point atomics.  The packed keys are never written out per row.
//            Before that a workgroup folds its rows into a table in LDS (keys + V sums, 64-bit LDS atomics, kGbLdsProbes probes at
//            most); a row that finds no place there goes straight to memory, and the workgroup flushes its LDS entries at its end:
//            with few groups the chip's atomics would otherwise all land on a handful of addresses.
//   count    occupied slots per tile, a scan of the tile counts, the number of groups G (the caller reads it back: outputs are sized)
//   compact  the G keys with their slot numbers, in slot order          (caller: one library sort of the G keys)
//   unpack   the sorted keys taken apart into K int64 columns, the V sums gathered through the slot numbers, and - for the
//            inverse - each group's rank in sorted order written into a table beside its slot ("assign")
//   lookup   one probe sequence per row through the same table: inverse[t] = the rank of row t's group
// Status word (sticky, OR-ed): 1 the table cannot hold the groups, 2 a value outside the offset / range it was packed with (the row
// is left out, nothing is read or written through it), 4 the arrays handed over do not belong together.
#include "common.h"

namespace {

constexpr int kGbThreads = 256;
constexpr int kGbWaves = kGbThreads / 64;
constexpr int kGbRowsPerThread = 16;
constexpr int kGbChunk = kGbThreads * kGbRowsPerThread;      // rows of one workgroup pass
constexpr int kGbLdsProbes = 8;
constexpr int kGbMaxLdsSlots = 2048;                          // x 8 B x (1 + 4 sums) = 80 KiB
constexpr int kGbMinLdsSlots = 16;
constexpr int kGbTilePer = 8, kGbTile = kGbThreads * kGbTilePer;
constexpr int64_t kGbMaxCapacity = 1ll << 36;
constexpr unsigned long long kGbEmpty = ~0ull;
constexpr int kDecMaxChars = 18;                              // 11^18 < 2^63

typedef ngcf_groupby_cols_t GbCols;

struct GbOut {
    int64_t *key[NGCF_GROUPBY_MAX_KEYS];
    int64_t *sum[NGCF_GROUPBY_MAX_VALUES];
};

struct DecCols {
    const void *col[NGCF_GROUPBY_MAX_KEYS];
    int32_t is64[NGCF_GROUPBY_MAX_KEYS];
    int32_t width[NGCF_GROUPBY_MAX_KEYS];
    int32_t n;
};

__device__ inline int64_t gb_load(const void *p, int is64, int64_t t)
{
    return is64 ? static_cast<const int64_t *>(p)[t] : (int64_t) static_cast<const int32_t *>(p)[t];
}

// false: a value outside [offset, offset + range] of its column.  The loops are unrolled over constant indices so that the
// argument struct stays in the kernarg segment (an index that is a loop counter would copy it to scratch memory).
__device__ inline bool gb_pack(const GbCols &c, int64_t t, unsigned long long &key)
{
    bool ok = true;
    key = 0;
#pragma unroll
    for (int k = 0; k < NGCF_GROUPBY_MAX_KEYS; ++k)
        if (k < c.n_keys) {
            const unsigned long long d = (unsigned long long)gb_load(c.key[k], c.key_is64[k], t) - (unsigned long long)c.key_offset[k];
            ok &= d <= c.key_range[k];
            key |= d << c.key_shift[k];
        }
    return ok;
}

struct GbVals {
    unsigned long long v0, v1, v2, v3;
};

__device__ inline GbVals gb_values(const GbCols &c, int64_t t)
{
    GbVals r{0, 0, 0, 0};
    if (c.n_values > 0) r.v0 = (unsigned long long)gb_load(c.value[0], c.value_is64[0], t);
    if (c.n_values > 1) r.v1 = (unsigned long long)gb_load(c.value[1], c.value_is64[1], t);
    if (c.n_values > 2) r.v2 = (unsigned long long)gb_load(c.value[2], c.value_is64[2], t);
    if (c.n_values > 3) r.v3 = (unsigned long long)gb_load(c.value[3], c.value_is64[3], t);
    return r;
}

// sums[v * stride + slot] += the row's v-th value (two's complement: a sum past 2^63 wraps, as numpy's int64 does)
template <int SCOPE> __device__ inline void gb_add(unsigned long long *sums, int64_t stride, int64_t slot, int nv, const GbVals &x)
{
    if (nv > 0 && x.v0) __hip_atomic_fetch_add(&sums[slot], x.v0, __ATOMIC_RELAXED, SCOPE);
    if (nv > 1 && x.v1) __hip_atomic_fetch_add(&sums[stride + slot], x.v1, __ATOMIC_RELAXED, SCOPE);
    if (nv > 2 && x.v2) __hip_atomic_fetch_add(&sums[2 * stride + slot], x.v2, __ATOMIC_RELAXED, SCOPE);
    if (nv > 3 && x.v3) __hip_atomic_fetch_add(&sums[3 * stride + slot], x.v3, __ATOMIC_RELAXED, SCOPE);
}

// the key that owns `slot` after this call: `key` if the slot was empty (now claimed) or already its own, else the other key.
// The load before the swap is an atomic one: a plain load may be hoisted out of the probe loop.
template <int SCOPE> __device__ inline unsigned long long gb_claim(unsigned long long *slot, unsigned long long key)
{
    unsigned long long cur = __hip_atomic_load(slot, __ATOMIC_RELAXED, SCOPE);
    if (cur == kGbEmpty) {
        unsigned long long expected = kGbEmpty;
        cur = __hip_atomic_compare_exchange_strong(slot, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE) ? key : expected;
    }
    return cur;
}

// false: every slot holds another key (or another row found that out: the status word is looked at every 64 probes, which bounds
// the work of a launch whose table is too small)
__device__ inline bool gb_insert_global(unsigned long long key, uint64_t h, const GbVals &x, int nv, unsigned long long *keys,
                                        unsigned long long *sums, int64_t cap, int32_t *status)
{
    const uint64_t mask = (uint64_t)cap - 1;
    uint64_t slot = h & mask;
    for (int64_t p = 0; p < cap; ++p) {
        if (gb_claim<__HIP_MEMORY_SCOPE_AGENT>(&keys[slot], key) == key) {
            gb_add<__HIP_MEMORY_SCOPE_AGENT>(sums, cap, (int64_t)slot, nv, x);
            return true;
        }
        slot = (slot + 1) & mask;
        if ((p & 63) == 63 && (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & NGCF_GROUPBY_FULL)) return false;
    }
    return false;
}

__device__ inline bool gb_insert_lds(unsigned long long key, uint64_t h, const GbVals &x, int nv, unsigned long long *s_keys,
                                     unsigned long long *s_sums, int S)
{
    uint32_t slot = (uint32_t)(h >> 32) & (uint32_t)(S - 1);            // the hash's upper half: independent of the memory table's home
#pragma unroll 1
    for (int p = 0; p < kGbLdsProbes; ++p) {
        if (gb_claim<__HIP_MEMORY_SCOPE_WORKGROUP>(&s_keys[slot], key) == key) {
            gb_add<__HIP_MEMORY_SCOPE_WORKGROUP>(s_sums, S, (int64_t)slot, nv, x);
            return true;
        }
        slot = (slot + 1) & (uint32_t)(S - 1);
    }
    return false;
}

// A workgroup takes the chunks blockIdx.x, blockIdx.x + gridDim.x, ... of kGbChunk rows each.
__global__ __launch_bounds__(kGbThreads) void groupby_insert_kernel(GbCols c, int64_t T, unsigned long long *keys, unsigned long long *sums,
                                                                    int64_t cap, int lds_slots, int32_t *status)
{
    extern __shared__ unsigned long long s_tab[];                       // lds_slots keys, then n_values x lds_slots sums
    const int tid = threadIdx.x, nv = c.n_values;
    unsigned long long *s_keys = s_tab, *s_sums = s_tab + lds_slots;
    if (lds_slots > 0) {
        for (int i = tid; i < lds_slots; i += kGbThreads) s_keys[i] = kGbEmpty;
        for (int i = tid; i < lds_slots * nv; i += kGbThreads) s_sums[i] = 0;
        __syncthreads();
    }
    bool bad = false, full = false;
    const int64_t n_chunks = (T + kGbChunk - 1) / kGbChunk;
    for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const int64_t base = ch * kGbChunk;
#pragma unroll 1
        for (int q = 0; q < kGbRowsPerThread; ++q) {
            const int64_t t = base + (int64_t)q * kGbThreads + tid;
            if (t >= T) break;
            unsigned long long key;
            if (!gb_pack(c, t, key)) {
                bad = true;
                continue;
            }
            const GbVals x = gb_values(c, t);
            const uint64_t h = fmix64(key);
            if (lds_slots > 0 && gb_insert_lds(key, h, x, nv, s_keys, s_sums, lds_slots)) continue;
            full |= !gb_insert_global(key, h, x, nv, keys, sums, cap, status);
        }
    }
    if (lds_slots > 0) {
        __syncthreads();
        for (int i = tid; i < lds_slots; i += kGbThreads) {
            const unsigned long long key = s_keys[i];
            if (key == kGbEmpty) continue;
            GbVals x{0, 0, 0, 0};
            if (nv > 0) x.v0 = s_sums[i];
            if (nv > 1) x.v1 = s_sums[lds_slots + i];
            if (nv > 2) x.v2 = s_sums[2 * lds_slots + i];
            if (nv > 3) x.v3 = s_sums[3 * lds_slots + i];
            full |= !gb_insert_global(key, fmix64(key), x, nv, keys, sums, cap, status);
        }
    }
    if (bad) atomicOr(status, NGCF_GROUPBY_RANGE);
    if (full) atomicOr(status, NGCF_GROUPBY_FULL);
}

// exclusive prefix of v over the workgroup's 256 threads; total: the sum over all of them
__device__ inline long long gb_block_exscan(long long v, long long *s_wave, long long &total)
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
    for (int w = 0; w < kGbWaves; ++w) {
        const long long s = s_wave[w];
        off += w < wave ? s : 0;
        total += s;
    }
    return off + inc - v;
}

__global__ __launch_bounds__(kGbThreads) void groupby_count_kernel(const unsigned long long *__restrict__ keys, int64_t cap, long long *__restrict__ tile_cnt)
{
    __shared__ long long s_wave[kGbWaves];
    const int64_t base = (int64_t)blockIdx.x * kGbTile + (int64_t)threadIdx.x * kGbTilePer;
    long long v = 0;
#pragma unroll
    for (int q = 0; q < kGbTilePer; ++q)
        if (base + q < cap) v += keys[base + q] != kGbEmpty ? 1 : 0;
    long long total;
    gb_block_exscan(v, s_wave, total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// tile counts -> exclusive offsets in place; *n_groups = their sum
__global__ __launch_bounds__(kGbThreads) void groupby_scan_tiles_kernel(long long *tile_cnt, int64_t n_tiles, int64_t *n_groups)
{
    __shared__ long long s_wave[kGbWaves];
    long long running = 0;
    for (int64_t base = 0; base < n_tiles; base += kGbThreads) {
        const int64_t t = base + threadIdx.x;
        const long long v = t < n_tiles ? tile_cnt[t] : 0;
        long long total;
        const long long ex = gb_block_exscan(v, s_wave, total);
        if (t < n_tiles) tile_cnt[t] = running + ex;
        running += total;
    }
    if (threadIdx.x == 0) *n_groups = running;
}

__global__ __launch_bounds__(kGbThreads) void groupby_compact_kernel(const unsigned long long *__restrict__ keys, int64_t cap,
                                                                     const long long *__restrict__ tile_off, int64_t G, int64_t *__restrict__ out_key,
                                                                     int64_t *__restrict__ out_slot, int32_t *status)
{
    __shared__ long long s_wave[kGbWaves];
    const int64_t base = (int64_t)blockIdx.x * kGbTile + (int64_t)threadIdx.x * kGbTilePer;
    unsigned long long k[kGbTilePer];
    long long v = 0;
#pragma unroll
    for (int q = 0; q < kGbTilePer; ++q) {
        k[q] = base + q < cap ? keys[base + q] : kGbEmpty;
        v += k[q] != kGbEmpty ? 1 : 0;
    }
    long long total;
    long long at = tile_off[blockIdx.x] + gb_block_exscan(v, s_wave, total);
    bool bad = false;
#pragma unroll
    for (int q = 0; q < kGbTilePer; ++q) {
        if (k[q] == kGbEmpty) continue;
        if (at >= 0 && at < G) {
            out_key[at] = (int64_t)k[q];
            out_slot[at] = base + q;
        } else {
            bad = true;                                                   // the table changed since it was counted
        }
        ++at;
    }
    if (bad) atomicOr(status, NGCF_GROUPBY_LOST);
}

__global__ __launch_bounds__(kGbThreads) void groupby_unpack_kernel(GbCols c, GbOut o, const int64_t *__restrict__ sorted_key, const int64_t *__restrict__ order,
                                                                    const int64_t *__restrict__ slots, const unsigned long long *__restrict__ sums,
                                                                    int64_t cap, int64_t G, int64_t *__restrict__ rank, int32_t *status)
{
    bool bad = false;
    for (int64_t g = (int64_t)blockIdx.x * kGbThreads + threadIdx.x; g < G; g += (int64_t)gridDim.x * kGbThreads) {
        const unsigned long long key = (unsigned long long)sorted_key[g];
#pragma unroll
        for (int k = 0; k < NGCF_GROUPBY_MAX_KEYS; ++k)
            if (k < c.n_keys) {
                const unsigned long long field = c.key_bits[k] ? (key >> c.key_shift[k]) & ((1ull << c.key_bits[k]) - 1ull) : 0ull;
                o.key[k][g] = (int64_t)(field + (unsigned long long)c.key_offset[k]);
            }
        const int64_t p = order[g];
        const int64_t slot = p >= 0 && p < G ? slots[p] : -1;
        const bool in = slot >= 0 && slot < cap;
        bad |= !in;
#pragma unroll
        for (int v = 0; v < NGCF_GROUPBY_MAX_VALUES; ++v)
            if (v < c.n_values) o.sum[v][g] = in ? (int64_t)sums[(int64_t)v * cap + slot] : 0;
        if (rank && in) rank[slot] = g;
    }
    if (bad) atomicOr(status, NGCF_GROUPBY_LOST);
}

// The table is read-only here: plain loads.
__global__ __launch_bounds__(kGbThreads) void groupby_lookup_kernel(GbCols c, int64_t T, const unsigned long long *__restrict__ keys,
                                                                    const int64_t *__restrict__ rank, int64_t cap, int64_t *__restrict__ inverse, int32_t *status)
{
    const uint64_t mask = (uint64_t)cap - 1;
    int flags = 0;
    for (int64_t t = (int64_t)blockIdx.x * kGbThreads + threadIdx.x; t < T; t += (int64_t)gridDim.x * kGbThreads) {
        unsigned long long key;
        int64_t r = -1;
        if (!gb_pack(c, t, key)) {
            flags |= NGCF_GROUPBY_RANGE;
        } else {
            uint64_t slot = fmix64(key) & mask;
            for (int64_t p = 0; p < cap; ++p) {
                const unsigned long long cur = keys[slot];
                if (cur == key) {
                    r = rank[slot];
                    break;
                }
                if (cur == kGbEmpty) break;
                slot = (slot + 1) & mask;
                if ((p & 63) == 63 && (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & NGCF_GROUPBY_LOST)) break;
            }
            if (r < 0) {
                flags |= NGCF_GROUPBY_LOST;                              // a row whose group is not in the table
                atomicOr(status, NGCF_GROUPBY_LOST);
            }
        }
        inverse[t] = r;
    }
    if (flags) atomicOr(status, flags);
}

// ---- the decimal string code ---------------------------------------------------------------------------------------------------------
// The characters of the columns' decimal strings, concatenated: character '0' + d is the base-11 digit d + 1, the string is a
// left-aligned number of kDecMaxChars places, padding 0.  Status: 1 a negative value, 2 more digits than the column's fixed width,
// 4 more than kDecMaxChars characters; such a row's code is -1.
__global__ __launch_bounds__(kGbThreads) void decimal_code_kernel(DecCols c, int64_t T, int64_t *__restrict__ out, int32_t *status)
{
    int flags = 0;
    for (int64_t t = (int64_t)blockIdx.x * kGbThreads + threadIdx.x; t < T; t += (int64_t)gridDim.x * kGbThreads) {
        unsigned long long acc = 0;
        int n = 0, bad = 0;
#pragma unroll
        for (int k = 0; k < NGCF_GROUPBY_MAX_KEYS; ++k)
            if (k < c.n) {
                const int64_t sv = gb_load(c.col[k], c.is64[k], t);
                if (sv < 0) bad |= 1;
                unsigned long long v = sv < 0 ? 0ull : (unsigned long long)sv, code = 0, p = 1;
                int L = 0;
                do {                                                      // least significant digit first: the column's own number
                    code += (v % 10ull + 1ull) * p;
                    p *= 11ull;
                    v /= 10ull;
                    ++L;
                } while (v > 0 && L < 20);
                const int w = c.width[k];
                if (w > 0 && L > w) bad |= 2;
                for (; L < w && L < 20; ++L) {                            // zero-padded on the left: '0' is digit 1
                    code += p;
                    p *= 11ull;
                }
                n += L;
                if (n > kDecMaxChars) bad |= 4;
                else acc = acc * p + code;                                // < 11^n: no overflow while n <= 18
            }
        for (; n < kDecMaxChars; ++n) acc *= 11ull;
        out[t] = bad ? -1 : (int64_t)acc;
        flags |= bad;
    }
    if (flags) atomicOr(status, flags);
}

int64_t gb_tiles(int64_t cap) { return (cap + kGbTile - 1) / kGbTile; }

bool gb_pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

int gb_check_capacity(const char *fn, int64_t cap)
{
    if (!gb_pow2(cap) || cap > kGbMaxCapacity)
        return fail(NGCF_ERR_ARG, "groupby: %s: capacity=%lld is not a power of two in [1, 2^36]", fn, (long long)cap);
    return NGCF_OK;
}

// the packing must be consistent in itself: the kernels shift and mask by it
int gb_check_cols(const char *fn, const GbCols *c, int64_t T, bool with_values)
{
    if (!c) return fail(NGCF_ERR_ARG, "groupby: %s: null argument", fn);
    if (T < 0) return fail(NGCF_ERR_ARG, "groupby: %s: negative count (T=%lld)", fn, (long long)T);
    if (c->n_keys < 1 || c->n_keys > NGCF_GROUPBY_MAX_KEYS || c->n_values < 0 || c->n_values > NGCF_GROUPBY_MAX_VALUES)
        return fail(NGCF_ERR_ARG, "groupby: %s: %d key columns and %d value columns, outside [1, %d] and [0, %d]", fn, c->n_keys, c->n_values,
                    NGCF_GROUPBY_MAX_KEYS, NGCF_GROUPBY_MAX_VALUES);
    int shift = 0;
    for (int k = c->n_keys - 1; k >= 0; --k) {
        const int bits = c->key_bits[k];
        if (bits < 0 || bits > 63 || c->key_shift[k] != shift || (bits < 63 && (c->key_range[k] >> bits) != 0) || (bits == 63 && (c->key_range[k] >> 63) != 0))
            return fail(NGCF_ERR_ARG, "groupby: %s: key column %d: bits=%d, shift=%d and range do not fit together", fn, k, bits, c->key_shift[k]);
        shift += bits;
        if (shift > 63) return fail(NGCF_ERR_ARG, "groupby: %s: the packed key has %d bits or more, above 63", fn, shift);
        if (T > 0 && !c->key[k]) return fail(NGCF_ERR_ARG, "groupby: %s: null argument", fn);
    }
    if (with_values)
        for (int v = 0; v < c->n_values; ++v)
            if (T > 0 && !c->value[v]) return fail(NGCF_ERR_ARG, "groupby: %s: null argument", fn);
    return NGCF_OK;
}

}  // namespace

extern "C" uint64_t ngcf_groupby_hash(uint64_t packed_key) { return fmix64(packed_key); }

extern "C" int ngcf_groupby_limits(int *chunk_rows, int *lds_probes, int *max_lds_slots)
{
    if (chunk_rows) *chunk_rows = kGbChunk;
    if (lds_probes) *lds_probes = kGbLdsProbes;
    if (max_lds_slots) *max_lds_slots = kGbMaxLdsSlots;
    return NGCF_OK;
}

extern "C" int64_t ngcf_groupby_workspace_bytes(int64_t capacity)
{
    if (!gb_pow2(capacity) || capacity > kGbMaxCapacity) return -1;
    return gb_tiles(capacity) * (int64_t)sizeof(long long);
}

extern "C" int ngcf_groupby_insert(const ngcf_groupby_cols_t *cols, int64_t T, uint64_t *table_keys, int64_t *table_sums, int64_t capacity,
                                   int lds_slots, int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gb_check_cols("insert", cols, T, true)) return rc;
    if (int rc = gb_check_capacity("insert", capacity)) return rc;
    if (lds_slots != 0 && (!gb_pow2(lds_slots) || lds_slots < kGbMinLdsSlots || lds_slots > kGbMaxLdsSlots))
        return fail(NGCF_ERR_ARG, "groupby: insert: lds_slots=%d is neither 0 nor a power of two in [%d, %d]", lds_slots, kGbMinLdsSlots, kGbMaxLdsSlots);
    if (!table_keys || !status || (cols->n_values > 0 && !table_sums)) return fail(NGCF_ERR_ARG, "groupby: insert: null argument");
    HIP_TRY(hipMemsetAsync(table_keys, 0xff, (size_t)capacity * sizeof(uint64_t), stream));
    if (cols->n_values > 0) HIP_TRY(hipMemsetAsync(table_sums, 0, (size_t)capacity * cols->n_values * sizeof(int64_t), stream));
    if (T == 0) return NGCF_OK;
    const size_t lds = (size_t)lds_slots * sizeof(unsigned long long) * (1 + cols->n_values);
    if (lds > 0) HIP_TRY(allow_full_lds<groupby_insert_kernel>());
    const int64_t n_chunks = (T + kGbChunk - 1) / kGbChunk;
    groupby_insert_kernel<<<dim3((unsigned)std::min<int64_t>(n_chunks, 256 * 8)), kGbThreads, lds, stream>>>(
        *cols, T, (unsigned long long *)table_keys, (unsigned long long *)table_sums, capacity, lds_slots, status);
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_groupby_count(const uint64_t *table_keys, int64_t capacity, int64_t *n_groups, void *workspace, int64_t workspace_bytes,
                                  void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gb_check_capacity("count", capacity)) return rc;
    if (!table_keys || !n_groups || !workspace) return fail(NGCF_ERR_ARG, "groupby: count: null argument");
    if (workspace_bytes < ngcf_groupby_workspace_bytes(capacity))
        return fail(NGCF_ERR_WORKSPACE, "groupby: count: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                    (long long)ngcf_groupby_workspace_bytes(capacity));
    const int64_t tiles = gb_tiles(capacity);
    groupby_count_kernel<<<dim3((unsigned)tiles), kGbThreads, 0, stream>>>((const unsigned long long *)table_keys, capacity, (long long *)workspace);
    LAUNCH_CHECK();
    groupby_scan_tiles_kernel<<<dim3(1), kGbThreads, 0, stream>>>((long long *)workspace, tiles, n_groups);
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_groupby_compact(const uint64_t *table_keys, int64_t capacity, int64_t n_groups, int64_t *keys, int64_t *slots,
                                    const void *workspace, int64_t workspace_bytes, int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gb_check_capacity("compact", capacity)) return rc;
    if (n_groups < 0 || n_groups > capacity)
        return fail(NGCF_ERR_ARG, "groupby: compact: n_groups=%lld outside [0, capacity=%lld]", (long long)n_groups, (long long)capacity);
    if (!table_keys || !workspace || !status || (n_groups > 0 && (!keys || !slots))) return fail(NGCF_ERR_ARG, "groupby: compact: null argument");
    if (workspace_bytes < ngcf_groupby_workspace_bytes(capacity))
        return fail(NGCF_ERR_WORKSPACE, "groupby: compact: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                    (long long)ngcf_groupby_workspace_bytes(capacity));
    if (n_groups == 0) return NGCF_OK;
    groupby_compact_kernel<<<dim3((unsigned)gb_tiles(capacity)), kGbThreads, 0, stream>>>((const unsigned long long *)table_keys, capacity,
                                                                                          (const long long *)workspace, n_groups, keys, slots, status);
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_groupby_unpack(const ngcf_groupby_cols_t *cols, const int64_t *sorted_keys, const int64_t *order, const int64_t *slots,
                                   const int64_t *table_sums, int64_t capacity, int64_t n_groups, int64_t *const *key_out,
                                   int64_t *const *sum_out, int64_t *table_rank, int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gb_check_cols("unpack", cols, 0, false)) return rc;
    if (int rc = gb_check_capacity("unpack", capacity)) return rc;
    if (n_groups < 0 || n_groups > capacity)
        return fail(NGCF_ERR_ARG, "groupby: unpack: n_groups=%lld outside [0, capacity=%lld]", (long long)n_groups, (long long)capacity);
    if (!status || !key_out || (cols->n_values > 0 && !sum_out)) return fail(NGCF_ERR_ARG, "groupby: unpack: null argument");
    if (n_groups == 0) return NGCF_OK;
    if (!sorted_keys || !order || !slots || (cols->n_values > 0 && !table_sums)) return fail(NGCF_ERR_ARG, "groupby: unpack: null argument");
    GbOut o{};
    for (int k = 0; k < cols->n_keys; ++k)
        if (!(o.key[k] = key_out[k])) return fail(NGCF_ERR_ARG, "groupby: unpack: null argument");
    for (int v = 0; v < cols->n_values; ++v)
        if (!(o.sum[v] = sum_out[v])) return fail(NGCF_ERR_ARG, "groupby: unpack: null argument");
    groupby_unpack_kernel<<<dim3(grid_for(n_groups, kGbThreads)), kGbThreads, 0, stream>>>(
        *cols, o, sorted_keys, order, slots, (const unsigned long long *)table_sums, capacity, n_groups, table_rank, status);
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_groupby_lookup(const ngcf_groupby_cols_t *cols, int64_t T, const uint64_t *table_keys, const int64_t *table_rank,
                                   int64_t capacity, int64_t *inverse, int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = gb_check_cols("lookup", cols, T, false)) return rc;
    if (int rc = gb_check_capacity("lookup", capacity)) return rc;
    if (!table_keys || !table_rank || !status || (T > 0 && !inverse)) return fail(NGCF_ERR_ARG, "groupby: lookup: null argument");
    if (T == 0) return NGCF_OK;
    groupby_lookup_kernel<<<dim3(grid_for(T, kGbThreads)), kGbThreads, 0, stream>>>(*cols, T, (const unsigned long long *)table_keys, table_rank,
                                                                                    capacity, inverse, status);
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_decimal_code(const void *const *columns, const int32_t *is64, const int32_t *widths, int n_columns, int64_t T, int64_t *out,
                                 int32_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (T < 0) return fail(NGCF_ERR_ARG, "decimal_code: negative count (T=%lld)", (long long)T);
    if (n_columns < 1 || n_columns > NGCF_GROUPBY_MAX_KEYS)
        return fail(NGCF_ERR_ARG, "decimal_code: %d columns, outside [1, %d]", n_columns, NGCF_GROUPBY_MAX_KEYS);
    if (!columns || !is64 || !widths || !status || (T > 0 && !out)) return fail(NGCF_ERR_ARG, "decimal_code: null argument");
    DecCols c{};
    c.n = n_columns;
    int fixed = 0;
    for (int k = 0; k < n_columns; ++k) {
        if (widths[k] < 0 || widths[k] > kDecMaxChars)
            return fail(NGCF_ERR_ARG, "decimal_code: width %d of column %d outside [0, %d]", widths[k], k, kDecMaxChars);
        if (T > 0 && !columns[k]) return fail(NGCF_ERR_ARG, "decimal_code: null argument");
        c.col[k] = columns[k];
        c.is64[k] = is64[k];
        c.width[k] = widths[k];
        fixed += widths[k] > 0 ? widths[k] : 1;
    }
    if (fixed > kDecMaxChars) return fail(NGCF_ERR_ARG, "decimal_code: the columns make at least %d characters, more than %d", fixed, kDecMaxChars);
    if (T == 0) return NGCF_OK;
    decimal_code_kernel<<<dim3(grid_for(T, kGbThreads)), kGbThreads, 0, stream>>>(c, T, out, status);
    LAUNCH_CHECK();
    return NGCF_OK;
}
