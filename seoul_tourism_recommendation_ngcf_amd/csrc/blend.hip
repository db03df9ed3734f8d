// Rank-point blending, the part of the reference's recommender after its topk (demo.py:285-292, 315-334, 378-398) for any number
// of request rows, columns and items in one launch: three orderings of the catalogue per request row (preference,
// congestion, distance) become points P - position, the points of a column's rows are summed per item, blended with the
// traveller's weights, filtered by the genre mask, and the best `top` items of every column come out - no score matrix, no
// dense [columns, items] table, no read-back.
#include "common.h"

// rating = (sp * w_pref + sc * w_con) + sd * w_dis with every product and sum rounded on its own (numpy's result bit for bit): the
// __dmul_rn / __dadd_rn of this toolchain are plain operators that the device default (-ffp-contract=fast) would fuse.
#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// Mapping.  One workgroup (4 waves) per (column, item tile).  The tile's three int32 point sums live in LDS (3 x tile_items x 4 B;
// 48 KiB at the default tile of 4 096 items, so two workgroups share a CU's 160 KiB).  The workgroup walks the lists of the
// column's rows, entry by entry across its lanes, and adds the points of the entries that fall into its tile with LDS integer
// atomics: integer sums, so the order of rows, lanes and workgroups does not matter.  Every id is checked before it is used as an
// index: a row index outside [0, R), a slot outside its table or a list entry outside [0, n_items) other than -1 sets *status and
// adds nothing (ngcf_gather_rows_f32's rule); every tile sees and flags the same ids.
//
// Selection.  The order is total: rating descending (as a monotone 64-bit key, -0.0 = +0.0), equal ratings lowest item first.  The
// `top` best of n candidates: an 8 x 8-bit radix select on the key (LDS histogram, integer atomics) finds the key K of the last
// place; everything above K is taken, and of the candidates equal to K the first ones in candidate order - which is item order, in
// a tile and in the merge alike (tiles ascend, a tile's list is sorted) - by a block scan; the <= 256 taken are ordered by counting.
// A tile does not keep its ratings: each pass forms them again from the three sums (3 LDS reads, 5 fp64 operations).
// One tile: the list is the result.  Several: the tiles' lists go to the workspace ([G, tiles, top] items and ratings) and a second
// kernel, one workgroup per column, selects among them with the same code.  Nothing depends on the tile size but the grouping.
// ---------------------------------------------------------------------------------------------
#define NGCF_BLEND_THREADS 256
#define NGCF_BLEND_TOP_MAX 256
#define NGCF_BLEND_P_MAX 1024
#define NGCF_BLEND_TILE_MAX 4096           // 3 int32 sums per item: 48 KiB, two workgroups per CU with the selection's 7 KiB

namespace {

struct SelectShared {
    int hist[256];
    int wave_total[NGCF_BLEND_THREADS / 64];
    int n_valid, n_above, digit, remaining;
    uint64_t key[NGCF_BLEND_TOP_MAX];
    int64_t item[NGCF_BLEND_TOP_MAX];
    double rating[NGCF_BLEND_TOP_MAX];
};

__device__ inline double blend_rating(int32_t sp, int32_t sc, int32_t sd, double wp, double wc, double wd)
{
    const double a = (double)sp * wp;
    const double b = (double)sc * wc;
    const double c = (double)sd * wd;
    const double ab = a + b;
    return ab + c;
}

// monotone map double -> uint64 (larger rating = larger key); -0.0 and +0.0 share a key
__device__ inline uint64_t rating_key(double r)
{
    if (r == 0.0) r = 0.0;
    const uint64_t u = (uint64_t)__double_as_longlong(r);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// inclusive scan of one int per thread over the workgroup, in thread order
__device__ inline int block_scan_incl(int v, int *wave_total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) wave_total[wave] = x;
    __syncthreads();
    for (int w = 0; w < wave; ++w) x += wave_total[w];
    __syncthreads();                                             // the totals are free again
    return x;
}

// The items of one tile: candidate i is item lo + i; its sums are in LDS, sp < 0 marks an item the mask leaves out.
struct TileSource {
    const int32_t *sp, *sc, *sd;
    int64_t lo;
    double wp, wc, wd;
    __device__ bool get(int64_t i, double &rating, int64_t &item) const
    {
        const int32_t p = sp[i];
        if (p < 0) return false;
        rating = blend_rating(p, sc[i], sd[i], wp, wc, wd);
        item = lo + i;
        return true;
    }
};

// The tiles' lists of one column, tile after tile; an item of -1 is an empty slot.
struct ListSource {
    const int64_t *items;
    const double *ratings;
    __device__ bool get(int64_t i, double &rating, int64_t &item) const
    {
        item = items[i];
        if (item < 0) return false;
        rating = ratings[i];
        return true;
    }
};

// out_items / out_rating [top] = the best `top` of the source's n candidates (rating descending, equal ratings in candidate
// order), the slots past them (-1, -inf).  Called by the whole workgroup.
template <class Source>
__device__ void select_top(const Source &src, int64_t n, int top, SelectShared &sh, int64_t *out_items, double *out_rating)
{
    const int tid = threadIdx.x;
    if (tid == 0) sh.n_valid = sh.n_above = 0;
    __syncthreads();
    {
        int mine = 0;
        double r;
        int64_t it;
        for (int64_t i = tid; i < n; i += NGCF_BLEND_THREADS) mine += src.get(i, r, it) ? 1 : 0;
        if (mine) atomicAdd(&sh.n_valid, mine);
    }
    __syncthreads();
    const int take = sh.n_valid < top ? sh.n_valid : top;
    for (int s = tid + take; s < top; s += NGCF_BLEND_THREADS) {
        out_items[s] = -1;
        out_rating[s] = -__builtin_inf();
    }
    if (take == 0) return;                                       // uniform

    // the key of place take - 1, eight bits at a time from the top
    uint64_t prefix = 0;
    int remaining = take;
    for (int shift = 56; shift >= 0; shift -= 8) {
        sh.hist[tid] = 0;
        __syncthreads();
        for (int64_t i = tid; i < n; i += NGCF_BLEND_THREADS) {
            double r;
            int64_t it;
            if (!src.get(i, r, it)) continue;
            const uint64_t k = rating_key(r);
            if (shift == 56 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&sh.hist[(k >> shift) & 255], 1);
        }
        __syncthreads();
        const int bin = 255 - tid;                               // scan from the largest digit down
        const int own = sh.hist[bin];
        const int incl = block_scan_incl(own, sh.wave_total);
        if (incl >= remaining && incl - own < remaining) {       // exactly one thread: remaining <= the candidates under the prefix
            sh.digit = bin;
            sh.remaining = remaining - (incl - own);
        }
        __syncthreads();
        prefix |= (uint64_t)sh.digit << shift;
        remaining = sh.remaining;
    }
    // `remaining` candidates equal to the key `prefix` are taken, the first ones in candidate order, behind the take - remaining above it
    const int n_above = take - remaining;
    const int64_t per = (n + NGCF_BLEND_THREADS - 1) / NGCF_BLEND_THREADS;
    const int64_t i0 = per * tid, i1 = i0 + per < n ? i0 + per : n;
    int equal = 0;
    for (int64_t i = i0; i < i1; ++i) {
        double r;
        int64_t it;
        if (!src.get(i, r, it)) continue;
        const uint64_t k = rating_key(r);
        if (k > prefix) {
            const int s = atomicAdd(&sh.n_above, 1);             // any slot: the counting sort below orders them
            if (s < n_above) sh.key[s] = k, sh.item[s] = it, sh.rating[s] = r;   // (always: the select counted them)
        } else if (k == prefix) {
            ++equal;
        }
    }
    equal = equal < remaining ? equal : remaining;               // (keeps the scan below 2^31 whatever n)
    int before = block_scan_incl(equal, sh.wave_total) - equal;
    for (int64_t i = i0; i < i1 && before < remaining; ++i) {
        double r;
        int64_t it;
        if (!src.get(i, r, it)) continue;
        const uint64_t k = rating_key(r);
        if (k != prefix) continue;
        const int s = n_above + before++;
        sh.key[s] = k, sh.item[s] = it, sh.rating[s] = r;
    }
    __syncthreads();
    if (tid < take) {
        const uint64_t k = sh.key[tid];
        const int64_t it = sh.item[tid];
        int place = 0;
        for (int j = 0; j < take; ++j) place += (sh.key[j] > k || (sh.key[j] == k && sh.item[j] < it)) ? 1 : 0;
        out_items[place] = it;
        out_rating[place] = sh.rating[tid];
    }
}

struct BlendLists {                         // one kind of points: lists [S, Pl] (ld), slot[R] (NULL: the list of row r is row r)
    const int64_t *lists;
    int64_t ld, n_lists;
    const int64_t *slot;
};

struct BlendParams {                        // by value: stays in the kernarg segment
    BlendLists kind[3];                     // preference, congestion, distance; lists == NULL: no points of that kind
    const int64_t *col_rowptr, *col_rows;
    int64_t n_col_rows, R, n_items;
    int Pl, P, top, tile, tiles;
    double w[3];
    const uint8_t *mask;
};

__global__ __launch_bounds__(NGCF_BLEND_THREADS) void blend_points_kernel(BlendParams prm, int64_t *__restrict__ out_items,
                                                                          double *__restrict__ out_rating,
                                                                          double *__restrict__ table, int32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) int32_t blend_lds[];
    __shared__ SelectShared sh;
    const int tid = threadIdx.x, tile = prm.tile;
    const int64_t g = blockIdx.x / prm.tiles, t = blockIdx.x % prm.tiles;
    const int64_t lo = t * tile;
    const int n_here = (int)(prm.n_items - lo < tile ? prm.n_items - lo : tile);
    int32_t *acc = blend_lds;                                    // [3][tile]
    for (int i = tid; i < 3 * tile; i += NGCF_BLEND_THREADS) acc[i] = 0;
    __syncthreads();

    int64_t rb = prm.col_rowptr[g], re = prm.col_rowptr[g + 1];
    bool bad = false;
    if (rb < 0 || re < rb || re > prm.n_col_rows) {
        bad = true;
        re = rb = 0;
    }
    const int Pl = prm.Pl;
    const int64_t n_entries = (re - rb) * Pl;
    for (int64_t e = tid; e < n_entries; e += NGCF_BLEND_THREADS) {
        const int64_t rr = e / Pl;
        const int j = (int)(e - rr * Pl);
        const int64_t r = prm.col_rows[rb + rr];
        if (r < 0 || r >= prm.R) {
            bad = true;
            continue;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const BlendLists &L = prm.kind[q];
            if (!L.lists) continue;
            int64_t s = r;
            if (L.slot) {
                s = L.slot[r];
                if (s < 0 || s >= L.n_lists) {
                    bad = true;
                    continue;
                }
            }
            const int64_t id = L.lists[s * L.ld + j];
            if (id == -1) continue;
            if (id < 0 || id >= prm.n_items) {
                bad = true;
                continue;
            }
            if (id >= lo && id < lo + n_here) atomicAdd(&acc[q * tile + (int)(id - lo)], prm.P - j);
        }
    }
    if (bad) atomicOr(status, 1);
    __syncthreads();

    if (table || prm.mask) {
        for (int i = tid; i < n_here; i += NGCF_BLEND_THREADS) {
            if (table) table[g * prm.n_items + lo + i] = blend_rating(acc[i], acc[tile + i], acc[2 * tile + i], prm.w[0], prm.w[1], prm.w[2]);
            if (prm.mask && !prm.mask[lo + i]) acc[i] = -1;      // the sums are >= 0: below 0 = not eligible
        }
        __syncthreads();
    }
    TileSource src = {acc, acc + tile, acc + 2 * tile, lo, prm.w[0], prm.w[1], prm.w[2]};
    const int64_t o = ((int64_t)blockIdx.x) * prm.top;           // [G, tiles, top]; with one tile that is [G, top]
    select_top(src, n_here, prm.top, sh, out_items + o, out_rating + o);
}

__global__ __launch_bounds__(NGCF_BLEND_THREADS) void blend_merge_kernel(const int64_t *__restrict__ tile_items,
                                                                         const double *__restrict__ tile_rating, int tiles, int top,
                                                                         int64_t *__restrict__ out_items,
                                                                         double *__restrict__ out_rating)
{
    __shared__ SelectShared sh;
    const int64_t g = blockIdx.x, n = (int64_t)tiles * top;
    ListSource src = {tile_items + g * n, tile_rating + g * n};
    select_top(src, n, top, sh, out_items + g * top, out_rating + g * top);
}

// 0: the default, enough items for the whole catalogue in one tile where it fits
int blend_tile(int64_t n_items, int tile_items)
{
    if (tile_items > 0) return tile_items;
    return (int)std::min<int64_t>(NGCF_BLEND_TILE_MAX, align_up(std::max<int64_t>(n_items, 1), 64));
}

const char *blend_limits(int64_t G, int64_t n_items, int top, int tile_items, int64_t *tiles_out)
{
    if (top < 1 || top > NGCF_BLEND_TOP_MAX) return "top outside [1, 256]";
    if (tile_items < 0 || tile_items > NGCF_BLEND_TILE_MAX) return "tile_items outside [0, 4096]";
    if (G < 0 || n_items < 1 || n_items >= (int64_t)1 << 31) return "n_items outside [1, 2^31) or a negative column count";
    const int64_t tiles = (n_items + blend_tile(n_items, tile_items) - 1) / blend_tile(n_items, tile_items);
    if (tiles * top >= (int64_t)1 << 31 || (G > 0 && tiles > (((int64_t)1 << 31) - 1) / G))
        return "more than 2^31 - 1 workgroups or tile candidates: raise tile_items";
    *tiles_out = tiles;
    return nullptr;
}

}  // namespace

extern "C" int64_t ngcf_blend_workspace_bytes(int64_t G, int64_t n_items, int top, int tile_items)
{
    int64_t tiles = 0;
    if (blend_limits(G, n_items, top, tile_items, &tiles)) return -1;
    return tiles <= 1 ? 0 : G * tiles * top * (int64_t)(sizeof(int64_t) + sizeof(double));
}

extern "C" int ngcf_blend_points(const int64_t *pref, int64_t ld_pref, int64_t R, int Pl, const int64_t *con, int64_t ld_con,
                                 int64_t S_con, const int64_t *con_slot, const int64_t *dis, int64_t ld_dis, int64_t S_dis,
                                 const int64_t *dis_slot, const int64_t *col_rowptr, const int64_t *col_rows, int64_t n_col_rows,
                                 int64_t G, int P, int64_t n_items, double w_pref, double w_con, double w_dis,
                                 const uint8_t *item_mask, int top, int tile_items, int64_t *out_items, double *out_rating,
                                 double *table, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 1 || P > NGCF_BLEND_P_MAX) return fail(NGCF_ERR_ARG, "blend_points: P=%d point ranks outside [1, %d]", P, NGCF_BLEND_P_MAX);
    int64_t tiles = 0;
    if (const char *why = blend_limits(G, n_items, top, tile_items, &tiles))
        return fail(NGCF_ERR_ARG, "blend_points: %s (top=%d, tile_items=%d, n_items=%lld, G=%lld)", why, top, tile_items,
                    (long long)n_items, (long long)G);
    if (R < 0 || R >= (((int64_t)1 << 31) + P - 1) / P)
        return fail(NGCF_ERR_ARG, "blend_points: R * P = %lld * %d >= 2^31: the int32 point sums could overflow", (long long)R, P);
    if (Pl < 1 || Pl > P || ld_pref < Pl || n_col_rows < 0 || S_con < 0 || S_dis < 0 || (con && ld_con < Pl) || (dis && ld_dis < Pl))
        return fail(NGCF_ERR_ARG, "blend_points: bad argument (lists of Pl=%d entries, 1 <= Pl <= P=%d, leading dimensions >= Pl)", Pl, P);
    if (G == 0) return NGCF_OK;
    if (!pref || !col_rowptr || (n_col_rows > 0 && !col_rows) || !out_items || !out_rating || !status)
        return fail(NGCF_ERR_ARG, "blend_points: null argument");
    const int64_t need = tiles <= 1 ? 0 : G * tiles * top * (int64_t)(sizeof(int64_t) + sizeof(double));
    if (need > 0 && (!workspace || workspace_bytes < need))
        return fail(NGCF_ERR_WORKSPACE, "blend_points: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);

    BlendParams prm = {};
    prm.kind[0] = {pref, ld_pref, R, nullptr};
    // a kind without its table or without its slots gives no points
    prm.kind[1] = {con && con_slot ? con : nullptr, ld_con, S_con, con_slot};
    prm.kind[2] = {dis && dis_slot ? dis : nullptr, ld_dis, S_dis, dis_slot};
    prm.col_rowptr = col_rowptr;
    prm.col_rows = col_rows;
    prm.n_col_rows = n_col_rows;
    prm.R = R;
    prm.n_items = n_items;
    prm.Pl = Pl;
    prm.P = P;
    prm.top = top;
    prm.tile = blend_tile(n_items, tile_items);
    prm.tiles = (int)tiles;
    prm.w[0] = w_pref, prm.w[1] = w_con, prm.w[2] = w_dis;
    prm.mask = item_mask;
    int64_t *tile_items_out = tiles <= 1 ? out_items : static_cast<int64_t *>(workspace);
    double *tile_rating_out = tiles <= 1 ? out_rating : reinterpret_cast<double *>(tile_items_out + G * tiles * top);
    const size_t lds = (size_t)3 * prm.tile * sizeof(int32_t);
    blend_points_kernel<<<dim3((unsigned)(G * tiles)), NGCF_BLEND_THREADS, lds, stream>>>(prm, tile_items_out, tile_rating_out, table,
                                                                                        status);
    LAUNCH_CHECK();
    if (tiles > 1) {
        blend_merge_kernel<<<dim3((unsigned)G), NGCF_BLEND_THREADS, 0, stream>>>(tile_items_out, tile_rating_out, (int)tiles, top,
                                                                                out_items, out_rating);
        LAUNCH_CHECK();
    }
    return NGCF_OK;
}
