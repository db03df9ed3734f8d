// swept_plan.h - the host plan of the L2-swept SpMM (spmm_swept.hip) as plain C++: a function of host arrays, no HIP.
//
// plan_part() takes the CSR entries of one row group and returns the arrays the kernel walks: rows are cut into pieces, the
// pieces dealt to wave tasks of equal load, and every task's entries laid out column window by column window in rounds of
// 64 / lpe slots whose entries belong to different accumulator rows.  tests/test_swept_plan.py builds this header with the host
// compiler and replays the plan on the CPU.
#ifndef NGCF_SWEPT_PLAN_H
#define NGCF_SWEPT_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

namespace swept_plan {
// Geometry of a part: LPE lanes share one entry, i.e. a slice of SW = 4 LPE floats of the gathered row per wave instruction;
// EPR = 64 / LPE entries per round, 16 rounds per chunk.  LPE = 16: 64-float (256-byte) slices, four entries per round, 576
// accumulator rows per workgroup.  LPE = 32 (r03): 128-float (512-byte) slices - at d = 128 the whole row in ONE sweep, two entries
// per round, 288 accumulator rows per workgroup: twice the row passes, half the slices, every stored entry read once instead of
// twice, four consecutive 128-byte lines per gather instead of two.
constexpr int kLdsBytes = 36 * 16 * 256;  // accumulator bytes per workgroup (144 KiB of LDS, + one spare row per wave)
constexpr int kSweptWGs = 256;            // one workgroup per CU
constexpr int kRowBits = 24;              // e_pack: column in bits 0..23, local row in bits 24..30
constexpr int kColMask = (1 << kRowBits) - 1;
// workgroup shape: 16 waves x 36 rows.  (Round 1 ran the parts that need three or more row passes as 8 x 72: fewer,
// longer wave tasks fetched 30 % less.  With the lag-driven wave priorities of the kernel 16 waves are faster there
// too - C3 user rows 1.60 vs 1.93 ms, profiles/r02_swept_lab.txt.)
constexpr int kWaves = 16;

template <typename F>
void parallel_for(int64_t n, F &&fn, int64_t min_parallel = 64)
{
    unsigned nt = std::thread::hardware_concurrency();
    if (nt > 16) nt = 16;
    if (nt < 1) nt = 1;
    if ((int64_t)nt > n) nt = (unsigned)std::max<int64_t>(n, 1);
    if (n < min_parallel || nt == 1) {
        fn(0, n);
        return;
    }
    std::vector<std::thread> th;
    const int64_t chunk = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; ++t) {
        const int64_t lo = t * chunk, hi = std::min<int64_t>(n, lo + chunk);
        if (lo >= hi) break;
        th.emplace_back([&fn, lo, hi]() { fn(lo, hi); });
    }
    for (auto &t : th) t.join();
}

// entries begin+off, begin+off+step, ... < end of one row.  A long row is dealt out to its pieces round-robin so
// that every piece covers the whole column range evenly (a contiguous cut would pile a piece's work into a few windows)
struct Piece {
    int64_t row;            // >= 0 row of the part, < 0 partial row -1-p of the part
    int64_t begin, end, count;
    int32_t off, step;
    int64_t src;            // the row of the part its entries come from (== row when the row is not cut)
};

struct Params {             // the caller's copy of the swept_* plan options
    int lpe = 16;           // lanes per entry: 16 or 32
    int cut = 4;            // rows are cut at 1/cut of a wave task's share
    bool moments = true;    // balance the column moments of the tasks when dealing
    bool order_rows = false;   // bucket layout "rows" instead of "cols"
    int window_kb = 0;      // 0 = by table size
    bool force = false;     // plan whatever the expected re-use (mode 2)
    bool debug = false;     // print the plan
};

struct PartPlan {
    std::vector<int64_t> tptr;        // [n_tasks*n_win+1] slot range of every (wave task, column window)
    std::vector<int32_t> e_pack;      // [n_slots] (local row << kRowBits) | column
    std::vector<float> e_val;         // [n_slots]
    std::vector<int32_t> dst, prow;   // [n_tasks*rows_per_wave] output row (>= 0), partial row -2-p, -1 unused; source row
    std::vector<int32_t> heavy_row;   // rows cut into pieces ...
    std::vector<int64_t> heavy_ptr;   // ... and their ranges of partial rows
    int waves = 0;                    // 0: the part is declined
    int rows_per_wave = 0;
    int32_t n_rowpass = 0, n_win = 0, win_cols = 0;
    int64_t n_slots = 0, n_partial = 0;
    std::string error;                // set when the shape is too large to plan
};

// Is a part of `n` rows with `nnz` entries in columns [col_lo, col_hi] not worth planning (or impossible to encode)?
inline bool declined(int64_t n, int64_t nnz, int32_t col_lo, int32_t col_hi, const Params &p)
{
    if (n <= 0 || col_hi < col_lo || nnz <= 0) return true;
    if (col_hi > kColMask) return true;                              // column does not fit the packed entry
    if (p.force) return false;
    if (nnz < ((int64_t)1 << 22)) return true;                       // small products are launch-bound, not L2-bound
    // expected uses of a fetched table row inside one XCD during one sweep: its column degree times the share
    // of the output rows that the XCD holds in LDS.  Below ~3 the sweep costs more than the misses it saves;
    // a table slice that fits the L2s anyway needs no sweep either.
    const int kSW = p.lpe * 4;
    const int64_t cap = (int64_t)kSweptWGs * (kLdsBytes / (kSW * 4));   // output rows resident in LDS at a time
    const double span = (double)col_hi - col_lo + 1;
    const double reuse = (double)nnz / span * std::min(1.0, (double)(cap / 8) / (double)n);
    return reuse < 3.0 || span * kSW * 4 < (double)(8 << 20);
}

namespace detail {
constexpr int kDealK = 8, kDealBucket = 256;

struct Cut {
    std::vector<Piece> pieces;
    int64_t n_rowpass = 0, n_tasks = 0, T = 0, n_partial = 0;
};

// 1) pieces and wave tasks: all tasks get the same number of entries and at most RW rows; row passes are added until the
// pieces fit.  False: they cannot be placed.
inline bool cut_pieces(const int64_t *rp, int64_t n, int64_t row_lo, int RW, int cut, int64_t cap, PartPlan &plan, Cut &c)
{
    const int64_t nnz = rp[n], n_wave_slots = (int64_t)kSweptWGs * kWaves;
    for (c.n_rowpass = std::max<int64_t>(1, (n + cap - 1) / cap);; ++c.n_rowpass) {
        c.n_tasks = c.n_rowpass * n_wave_slots;
        c.T = std::max<int64_t>(64, (nnz + c.n_tasks - 1) / c.n_tasks);
        const int64_t Tp = std::max<int64_t>(64, c.T / std::max(2, cut));   // rows are cut well below a task's share
        c.pieces.clear();
        plan.heavy_row.clear();
        plan.heavy_ptr.assign(1, 0);
        c.n_partial = 0;
        for (int64_t r = 0; r < n; ++r) {
            const int64_t b = rp[r], e = rp[r + 1], len = e - b;
            if (len <= Tp) {
                c.pieces.push_back({r, b, e, len, 0, 1, r});
            } else {
                const int64_t k = (len + Tp - 1) / Tp;
                plan.heavy_row.push_back((int32_t)(row_lo + r));
                for (int64_t j = 0; j < k; ++j) c.pieces.push_back({-1 - c.n_partial++, b, e, (len - j + k - 1) / k, (int32_t)j, (int32_t)k, r});
                plan.heavy_ptr.push_back(c.n_partial);
            }
        }
        if ((int64_t)c.pieces.size() <= c.n_tasks * RW) return true;
        if (c.n_rowpass > (int64_t)1 << 20) return false;
    }
}

// m_k = sum over a piece's entries of cos(k pi x), k = 1..kDealK, x = share of all entries left of the entry's column
inline std::vector<float> piece_moments(const std::vector<Piece> &pieces, const int32_t *col, int64_t nnz, int32_t col_lo, int32_t col_hi)
{
    const int64_t span = (int64_t)col_hi - col_lo + 1;
    std::vector<int64_t> ccnt((size_t)span + 1, 0);
    for (int64_t x = 0; x < nnz; ++x) ccnt[(size_t)(col[x] - col_lo) + 1]++;
    for (int64_t c = 0; c < span; ++c) ccnt[(size_t)c + 1] += ccnt[(size_t)c];
    std::vector<float> ctab((size_t)span * kDealK);
    parallel_for(span, [&](int64_t lo, int64_t hi) {
        for (int64_t c = lo; c < hi; ++c) {
            const double xpos = (0.5 * (double)(ccnt[(size_t)c] + ccnt[(size_t)c + 1])) / (double)nnz;
            for (int k = 0; k < kDealK; ++k) ctab[(size_t)c * kDealK + k] = (float)cos((k + 1) * 3.14159265358979323846 * xpos);
        }
    });
    std::vector<float> mom(pieces.size() * kDealK, 0.f);             // [piece][kDealK]
    parallel_for((int64_t)pieces.size(), [&](int64_t lo, int64_t hi) {
        for (int64_t pi = lo; pi < hi; ++pi) {
            const Piece &pc = pieces[(size_t)pi];
            float acc[kDealK] = {0};
            for (int64_t x = pc.begin + pc.off; x < pc.end; x += pc.step) {
                const float *t = &ctab[(size_t)(col[x] - col_lo) * kDealK];
                for (int k = 0; k < kDealK; ++k) acc[k] += t[k];
            }
            for (int k = 0; k < kDealK; ++k) mom[(size_t)pi * kDealK + k] = acc[k];
        }
    });
    return mom;
}

// Dealing.  Level by level, heaviest piece -> lightest task (every task gets at most one piece per level): all tasks end
// within +-2 % of the same entry count.  That alone leaves WHERE in the table a task's entries lie to chance, and the
// sweep pays for it: a wave whose rows happen to hold few entries in the first half of the table runs ahead of the
// others by (missing entries) / (entries per column) - on the C3 item rows sigma = 1.1 MiB of table slice, 4 096 waves
// spread over ~10 MiB against a 4 MiB L2 (measured: profiles/r02_swept_trace.txt; a table
// row is then fetched again for the late waves).  So inside buckets of kDealBucket neighbouring (task, piece) pairs of a
// level - equal loads to within a fraction of a percent - the pairing is chosen to cancel the low-order cosine moments
// of every task's entry positions (position = share of all entries left of the column, so that a uniform sweep is the
// target whatever the column popularity): m_k = sum over entries of cos(k pi x), k = 1..kDealK, are the sine-series
// coefficients of the task's cumulative-count deviation; the greedy gives each piece to the task of its bucket whose
// moments it cancels best.  Simulated on the C3 item rows: spread (p5..p95) 2.9 -> 0.9 MiB, worst wave 4.6 -> 2.0 MiB.
// `mom` empty: no moment balancing.  Returns [task][local row] -> piece, -1 = unused.
inline std::vector<int64_t> deal(const std::vector<Piece> &pieces, const std::vector<float> &mom, int64_t n_tasks, int RW)
{
    const bool balance_moments = !mom.empty();
    std::vector<int64_t> order(pieces.size());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return pieces[(size_t)a].count > pieces[(size_t)b].count; });
    std::vector<int64_t> load((size_t)n_tasks, 0), by_load((size_t)n_tasks);
    std::vector<float> tmom(balance_moments ? (size_t)n_tasks * kDealK : 0, 0.f);   // moments of every task so far
    std::vector<int64_t> task_piece((size_t)(n_tasks * RW), -1);
    for (int64_t lvl = 0; lvl * n_tasks < (int64_t)pieces.size(); ++lvl) {
        std::iota(by_load.begin(), by_load.end(), 0);
        std::stable_sort(by_load.begin(), by_load.end(), [&](int64_t a, int64_t b) { return load[(size_t)a] < load[(size_t)b]; });
        const int64_t lo = lvl * n_tasks, hi = std::min<int64_t>((int64_t)pieces.size(), lo + n_tasks);
        if (!balance_moments) {
            for (int64_t i = lo; i < hi; ++i) {
                const int64_t t = by_load[(size_t)(i - lo)];
                task_piece[(size_t)(t * RW + lvl)] = order[(size_t)i];
                load[(size_t)t] += pieces[(size_t)order[(size_t)i]].count;
            }
            continue;
        }
        const int64_t n_buckets = (hi - lo + kDealBucket - 1) / kDealBucket;
        parallel_for(n_buckets, [&](int64_t b_lo, int64_t b_hi) {
            std::vector<int64_t> ps, ts;
            for (int64_t b = b_lo; b < b_hi; ++b) {
                const int64_t i0 = lo + b * kDealBucket, i1 = std::min(hi, i0 + kDealBucket);
                ps.assign(order.begin() + i0, order.begin() + i1);                      // pieces of the bucket ...
                ts.assign(by_load.begin() + (i0 - lo), by_load.begin() + (i1 - lo));   // ... and its tasks
                // pieces with the largest moments choose first
                std::stable_sort(ps.begin(), ps.end(), [&](int64_t a, int64_t c) {
                    float na = 0.f, nc = 0.f;
                    for (int k = 0; k < kDealK; ++k) {
                        na += fabsf(mom[(size_t)a * kDealK + k]);
                        nc += fabsf(mom[(size_t)c * kDealK + k]);
                    }
                    return na > nc;
                });
                for (const int64_t pi : ps) {
                    const float *pm = &mom[(size_t)pi * kDealK];
                    size_t best = 0;
                    float best_cost = 3.4e38f;
                    for (size_t j = 0; j < ts.size(); ++j) {
                        const float *tm = &tmom[(size_t)ts[j] * kDealK];
                        float cost = 0.f;
                        for (int k = 0; k < kDealK; ++k) cost += (tm[k] + pm[k]) * (tm[k] + pm[k]);
                        if (cost < best_cost) {
                            best_cost = cost;
                            best = j;
                        }
                    }
                    const int64_t t = ts[best];
                    ts[best] = ts.back();
                    ts.pop_back();
                    task_piece[(size_t)(t * RW + lvl)] = pi;
                    load[(size_t)t] += pieces[(size_t)pi].count;
                    for (int k = 0; k < kDealK; ++k) tmom[(size_t)t * kDealK + k] += pm[k];
                }
            }
        }, 2);
    }
    return task_piece;
}

// Layout of a (task, window) bucket, two ways (NGCF_SWEPT_ORDER): its slot list (index into `ents`, -1 = empty), a multiple of
// kEPR long, slot 0 never empty.  Either way the entries of one row never share a round (they are read-modify-written in LDS
// without atomics).
struct Ent { int32_t col, lr; float v; };

//  "cols"  : entries sorted by column, rounds filled greedily in that order with entries of distinct rows (an entry
//            whose row is already in the round waits for the next one): the wave walks the window left to right
inline void schedule_cols(std::vector<Ent> &ents, int kEPR, std::vector<int32_t> &slots, std::vector<char> &done)
{
    std::sort(ents.begin(), ents.end(), [](const Ent &x, const Ent &y) { return x.col != y.col ? x.col < y.col : x.lr < y.lr; });
    slots.clear();
    done.assign(ents.size(), 0);
    size_t first = 0, left = ents.size();
    while (left > 0) {
        uint64_t in_round[2] = {0, 0};
        int taken = 0;
        while (first < ents.size() && done[first]) ++first;
        for (size_t i = first; i < ents.size() && taken < kEPR && i < first + 512; ++i) {
            if (done[i]) continue;
            const int lr = ents[i].lr;
            if (in_round[lr >> 6] >> (lr & 63) & 1) continue;
            in_round[lr >> 6] |= (uint64_t)1 << (lr & 63);
            done[i] = 1;
            slots.push_back((int32_t)i);
            ++taken;
            --left;
        }
        for (; taken < kEPR; ++taken) slots.push_back(-1);
    }
}

//  "rows"  : R = max(longest row, ceil(entries / kEPR)) rounds; row after row (`ents` comes row by row) is laid down the
//            rounds, wrapping round: the k-th entry sits in round k % R, and a row has at most R entries
inline void schedule_rows(const std::vector<Ent> &ents, int kEPR, std::vector<int32_t> &slots)
{
    int64_t longest = 0, run = 0;
    for (size_t i = 0; i < ents.size(); ++i) {
        run = i > 0 && ents[i].lr == ents[i - 1].lr ? run + 1 : 1;
        longest = std::max(longest, run);
    }
    const int64_t R = std::max(longest, ((int64_t)ents.size() + kEPR - 1) / kEPR);
    slots.assign((size_t)(R * kEPR), -1);
    for (int64_t k = 0; k < (int64_t)ents.size(); ++k) slots[(size_t)((k % R) * kEPR + k / R)] = (int32_t)k;
}

// The buckets of the tasks [t_lo, t_hi): fn(task, window, entries, slot list) for each, in task and window order.  The count
// pass and the fill pass both walk through here, so they see the same slot lists.
template <typename F>
void for_each_bucket(int64_t t_lo, int64_t t_hi, const std::vector<Piece> &pieces, const std::vector<int64_t> &task_piece, int RW,
                     const int32_t *col, const float *val, int32_t col_lo, int32_t win_cols, int64_t n_win, int kEPR, bool by_cols, F &&fn)
{
    std::vector<std::vector<Ent>> per_win((size_t)n_win);
    std::vector<int32_t> slots;
    std::vector<char> done;
    for (int64_t t = t_lo; t < t_hi; ++t) {
        for (auto &v : per_win) v.clear();
        for (int lr = 0; lr < RW; ++lr) {
            const int64_t pi = task_piece[(size_t)(t * RW + lr)];
            if (pi < 0) continue;
            const Piece &pc = pieces[(size_t)pi];
            for (int64_t x = pc.begin + pc.off; x < pc.end; x += pc.step)
                per_win[(size_t)((col[x] - col_lo) / win_cols)].push_back({col[x], lr, val[x]});
        }
        for (int64_t w = 0; w < n_win; ++w) {
            if (by_cols) schedule_cols(per_win[(size_t)w], kEPR, slots, done);
            else schedule_rows(per_win[(size_t)w], kEPR, slots);
            fn(t, w, per_win[(size_t)w], slots);
        }
    }
}
}  // namespace detail

// Plan of the rows [row_lo, row_lo + n) of a matrix: `rp` [n + 1] is their row pointer rebased to 0, `col` / `val` their
// rp[n] entries, [col_lo, col_hi] the column range they gather from.  plan.waves == 0 when the part is declined.
inline PartPlan plan_part(const int64_t *rp, int64_t n, const int32_t *col, const float *val, int64_t row_lo, int32_t col_lo,
                          int32_t col_hi, const Params &p)
{
    using namespace detail;
    PartPlan plan;
    const int64_t nnz = n > 0 ? rp[n] : 0;
    if (declined(n, nnz, col_lo, col_hi, p)) return plan;
    const int kSW = p.lpe * 4, kEPR = 64 / p.lpe, kLdsRows = kLdsBytes / (kSW * 4);    // the part's geometry (see the top of the file)
    const int RW = kLdsRows / kWaves;
    Cut c;
    if (!cut_pieces(rp, n, row_lo, RW, p.cut, (int64_t)kSweptWGs * kLdsRows, plan, c)) {
        plan.error = "swept plan: cannot place " + std::to_string(c.pieces.size()) + " pieces";
        return plan;
    }
    const std::vector<Piece> &pieces = c.pieces;
    const int64_t n_tasks = c.n_tasks;
    if (n_tasks * RW >= (int64_t)1 << 31 || c.n_partial >= ((int64_t)1 << 31) - 2) {
        plan.error = "swept plan: matrix too large";
        return plan;
    }
    const std::vector<int64_t> task_piece =
        deal(pieces, p.moments ? piece_moments(pieces, col, nnz, col_lo, col_hi) : std::vector<float>(), n_tasks, RW);
    // 2) column windows and the slot layout of every (task, window) bucket
    // 8 MiB windows; 16 MiB when the table slice is 128 MiB or more (C3 item rows, lead 2: 1.58 vs 1.61 ms; on the 25 MiB
    // table of the user rows 8 MiB: 1.53 vs 1.84 ms)
    int64_t win_kb = p.window_kb > 0 ? p.window_kb : (((int64_t)col_hi - col_lo + 1) * kSW * 4 >= ((int64_t)128 << 20) ? 16384 : 8192);
    if (win_kb < 16) win_kb = 16;
    const int32_t win_cols = (int32_t)std::max<int64_t>(64, win_kb * 1024 / (kSW * 4));
    const int64_t n_win = ((int64_t)col_hi - col_lo) / win_cols + 1;
    if (n_tasks * n_win >= (int64_t)1 << 31) {
        plan.error = "swept plan: too many windows";
        return plan;
    }
    std::vector<int64_t> &tptr = plan.tptr;
    tptr.assign((size_t)(n_tasks * n_win) + 1, 0);
    auto buckets = [&](int64_t lo, int64_t hi, auto &&fn) {
        for_each_bucket(lo, hi, pieces, task_piece, RW, col, val, col_lo, win_cols, n_win, kEPR, !p.order_rows, fn);
    };
    parallel_for(n_tasks, [&](int64_t lo, int64_t hi) {
        buckets(lo, hi, [&](int64_t t, int64_t w, const std::vector<Ent> &, const std::vector<int32_t> &slots) {
            tptr[(size_t)(t * n_win + w) + 1] = (int64_t)slots.size();
        });
    });
    for (size_t i = 1; i < tptr.size(); ++i) tptr[i] += tptr[i - 1];
    const int64_t n_slots = tptr.back();
    // empty slots add 0 x (a row of their own window, an L2 hit) to the wave's spare accumulator row RW: "cols" names the
    // row just gathered, "rows" the row of the bucket's first slot
    plan.e_pack.assign((size_t)std::max<int64_t>(n_slots, 1), -1);
    plan.e_val.assign((size_t)std::max<int64_t>(n_slots, 1), 0.f);
    parallel_for(n_tasks, [&](int64_t lo, int64_t hi) {
        buckets(lo, hi, [&](int64_t t, int64_t w, const std::vector<Ent> &ents, const std::vector<int32_t> &slots) {
            const int64_t b0 = tptr[(size_t)(t * n_win + w)];
            int32_t near_col = ents.empty() ? 0 : ents[(size_t)slots[0]].col;
            for (size_t i = 0; i < slots.size(); ++i) {
                if (slots[i] >= 0) {
                    const Ent &e = ents[(size_t)slots[i]];
                    if (!p.order_rows) near_col = e.col;
                    plan.e_pack[(size_t)b0 + i] = (int32_t)((uint32_t)e.lr << kRowBits) | e.col;
                    plan.e_val[(size_t)b0 + i] = e.v;
                } else {
                    plan.e_pack[(size_t)b0 + i] = (int32_t)((uint32_t)RW << kRowBits) | near_col;
                }
            }
        });
    });
    // 3) where every accumulator row goes, and the matrix row behind it (edge dropout key)
    plan.dst.assign((size_t)(n_tasks * RW), -1);
    plan.prow.assign((size_t)(n_tasks * RW), 0);
    for (size_t i = 0; i < plan.dst.size(); ++i) {
        if (task_piece[i] < 0) continue;
        const int64_t r = pieces[(size_t)task_piece[i]].row;
        plan.dst[i] = r >= 0 ? (int32_t)(row_lo + r) : (int32_t)(-2 - (-1 - r));
        plan.prow[i] = (int32_t)(row_lo + pieces[(size_t)task_piece[i]].src);
    }
    if (p.debug) {
        int64_t mx = 0, mn = INT64_MAX;
        for (int64_t t = 0; t < n_tasks; ++t) {
            const int64_t s = tptr[(size_t)((t + 1) * n_win)] - tptr[(size_t)(t * n_win)];
            mx = std::max(mx, s);
            mn = std::min(mn, s);
        }
        fprintf(stderr, "[swept plan] rows [%lld, %lld) nnz %lld cols [%d, %d]: %d waves x %d rows, %lld row passes, %lld windows x %d "
                        "cols, T %lld, pieces %zu (partial %lld), slots %lld (+%.1f%%), per task %lld..%lld\n",
                (long long)row_lo, (long long)(row_lo + n), (long long)nnz, col_lo, col_hi, kWaves, RW, (long long)c.n_rowpass, (long long)n_win,
                win_cols, (long long)c.T, pieces.size(), (long long)c.n_partial, (long long)n_slots,
                100.0 * (double)(n_slots - nnz) / (double)nnz, (long long)mn, (long long)mx);
    }
    plan.waves = kWaves;
    plan.rows_per_wave = RW;
    plan.n_rowpass = (int32_t)c.n_rowpass;
    plan.n_win = (int32_t)n_win;
    plan.win_cols = win_cols;
    plan.n_slots = n_slots;
    plan.n_partial = c.n_partial;
    return plan;
}
}  // namespace swept_plan

#endif  // NGCF_SWEPT_PLAN_H
