// Delimited text on the device: the first line of Preprocess.load_preprocess_data, `pd.read_csv(path, sep='|')` (utils.py:38-39), for
// integer and float columns.  The buffer is uint8 [n]; the grammar, the error kinds and the status block are in include/ngcf_hip.h,
// section "delimited text".
//   count   a workgroup per block of kTextCountBlock bytes, a 16-byte load per lane and step: the bytes that start a row, counted.
//           (The caller scans the block counts.)
//   starts  the same walk again; a workgroup scan puts every row start at its rank: starts[r], ascending, and starts[n_rows] = n.
//   parse   a lane per row, a workgroup per run of kTextRows rows.  The run's bytes come into LDS with coalesced 16-byte loads
//           (LDS tier); a row that does not lie inside the staged window is walked from memory by its lane (memory tier).  Both
//           tiers run the same code through a flat pointer, so they agree bit for bit.
// Integer atomics only (status bits, the first error, the slow-field counter); every value is written with ordinary vector stores,
// and a slow field's patch does not depend on the order of the list: two runs give the same bytes.
#include "common.h"

namespace {

constexpr int kTextThreads = 256;
constexpr int kTextCountSteps = 4;
constexpr int kTextCountBlock = kTextThreads * 16 * kTextCountSteps;      // bytes of one counting block
constexpr int kTextRows = kTextThreads;                                    // rows of one workgroup of the parse
// LDS budget of a parse workgroup.  160 KiB per CU and workgroups of four waves: 30 KiB (and the 16 bytes of alignment slack and the
// column tables beside it) keeps five workgroups, 20 waves, on a CU and holds runs of rows of up to 120 bytes on average (the Seoul
// log's are about 50).  A placeholder: profiles/text_lab.txt records the run that settles it (none yet).
constexpr int kTextLdsBytes = 30 * 1024;
constexpr int kTextMaxFields = NGCF_TEXT_MAX_FIELDS;
constexpr int kTextMaxColumns = NGCF_TEXT_MAX_COLUMNS;

struct TextCols {
    int32_t n_columns, n_fields;
    int8_t slot_of_field[kTextMaxFields];       // -1: the field is not selected
    uint8_t field[kTextMaxColumns];
    uint8_t kind[kTextMaxColumns];              // 0 int64, 1 float64
    void *out[kTextMaxColumns];
};

// 10^0 .. 10^22: every one a double without rounding (5^22 < 2^53)
__device__ const double kTextPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                          1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

__device__ inline double text_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ inline double text_inf(bool neg) { return __longlong_as_double(neg ? (long long)0xfff0000000000000ull : 0x7ff0000000000000ll); }
__device__ inline bool text_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// ---------------------------------------------------------------------------------------------
// line starts
// ---------------------------------------------------------------------------------------------
// Bit j of the result: byte 16 * chunk + j starts a row.  `quote`: one of the chunk's bytes is a '"'.
__device__ inline uint32_t text_chunk_mask(const uint8_t *__restrict__ data, int64_t n, int64_t chunk, bool &quote)
{
    const int64_t base = chunk * 16;
    if (base >= n) return 0;
    uint8_t b[18];                                                      // b[0] the byte before the chunk, b[17] the one after
    if (base + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(data + base);  // data is 16-byte aligned
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) b[1 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) b[1 + j] = base + j < n ? data[base + j] : (uint8_t)0;
    }
    b[0] = base > 0 ? data[base - 1] : (uint8_t)'\n';
    b[17] = base + 16 < n ? data[base + 16] : (uint8_t)0;
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int64_t p = base + j;
        const uint8_t c = b[1 + j];
        if (p < n && c == '"') quote = true;
        const bool blank = c == '\n' || (c == '\r' && (p + 1 == n || b[2 + j] == '\n'));
        if (p < n && b[j] == '\n' && !blank) mask |= 1u << j;
    }
    return mask;
}

__global__ __launch_bounds__(kTextThreads) void text_count_kernel(const uint8_t *__restrict__ data, int64_t n, int64_t *__restrict__ block_counts,
                                                                  unsigned long long *status)
{
    __shared__ int s_wave[kTextThreads / 64];
    const int tid = threadIdx.x;
    const int64_t chunk0 = (int64_t)blockIdx.x * (kTextCountBlock / 16);
    bool quote = false;
    int count = 0;
#pragma unroll
    for (int s = 0; s < kTextCountSteps; ++s) count += __popc(text_chunk_mask(data, n, chunk0 + s * kTextThreads + tid, quote));
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) count += __shfl_xor(count, m);
    if ((tid & 63) == 0) s_wave[tid >> 6] = count;
    if (__any(quote) && (tid & 63) == 0) atomicOr(status, (unsigned long long)NGCF_TEXT_QUOTE);
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < kTextThreads / 64; ++w) total += s_wave[w];
        block_counts[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(kTextThreads) void text_starts_kernel(const uint8_t *__restrict__ data, int64_t n, const int64_t *__restrict__ block_offsets,
                                                                   int64_t n_rows, int64_t *__restrict__ starts, unsigned long long *status)
{
    __shared__ int s_wave[kTextThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t chunk0 = (int64_t)blockIdx.x * (kTextCountBlock / 16);
    int64_t rank = block_offsets[blockIdx.x];                            // rows before this block
    bool lost = false, quote = false;
    if (blockIdx.x == 0 && tid == 0) starts[n_rows] = n;
    for (int s = 0; s < kTextCountSteps; ++s) {
        const int64_t chunk = chunk0 + s * kTextThreads + tid;
        uint32_t mask = text_chunk_mask(data, n, chunk, quote);
        const int mine = __popc(mask);
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        __syncthreads();                                                // the previous step's sums have been read
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = incl - mine, total = 0;
#pragma unroll
        for (int w = 0; w < kTextThreads / 64; ++w) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        int64_t r = rank + before;
        while (mask) {
            const int j = __ffs(mask) - 1;
            mask &= mask - 1;
            if (r >= 0 && r < n_rows) starts[r] = chunk * 16 + j;
            else lost = true;                                           // the buffer changed since the count: nothing is written out of bounds
            ++r;
        }
        rank += total;
    }
    if (lost) atomicOr(status, (unsigned long long)NGCF_TEXT_LOST);
}

// ---------------------------------------------------------------------------------------------
// fields.  `p` is a flat pointer (LDS or memory), `len` the field's bytes; both parsers strip spaces and tabs first.
// Return value: 0, or the error kind.
// ---------------------------------------------------------------------------------------------
__device__ inline void text_strip(const uint8_t *&p, int64_t &len)
{
    while (len > 0 && (p[0] == ' ' || p[0] == '\t')) {
        ++p;
        --len;
    }
    while (len > 0 && (p[len - 1] == ' ' || p[len - 1] == '\t')) --len;
}

// [+-]?[0-9]+ inside int64, the overflow found exactly
__device__ inline int text_parse_int(const uint8_t *p, int64_t len, int64_t &value)
{
    value = 0;
    text_strip(p, len);
    if (len == 0) return NGCF_TEXT_KIND_EMPTY;
    int64_t i = 0;
    bool neg = false;
    if (p[0] == '+' || p[0] == '-') {
        neg = p[0] == '-';
        i = 1;
    }
    if (i == len) return NGCF_TEXT_KIND_BYTE;
    const uint64_t limit = neg ? 0x8000000000000000ull : 0x7fffffffffffffffull;
    uint64_t acc = 0;
    bool over = false;
    for (; i < len; ++i) {
        const uint8_t c = p[i];
        if (!text_digit(c)) return NGCF_TEXT_KIND_BYTE;                 // a bad byte comes before an overflow, as in int()
        const uint64_t d = c - '0';
        if (acc > (limit - d) / 10) over = true;
        else acc = acc * 10 + d;
    }
    if (over) return NGCF_TEXT_KIND_OVERFLOW;
    value = neg ? (int64_t)(0 - acc) : (int64_t)acc;
    return 0;
}

__device__ inline bool text_is(const uint8_t *p, int64_t len, const char *word, int n)
{
    if (len != n) return false;
    for (int k = 0; k < n; ++k)
        if (p[k] != (uint8_t)word[k]) return false;
    return true;
}

// [+-]?(digits[.digits?]|.digits)([eE][+-]?digits)? and the spellings of NaN and the infinities.  `slow`: the field is a number
// outside the fast path; value is then NaN and the caller appends the field to the slow list.
__device__ inline int text_parse_float(const uint8_t *p, int64_t len, double &value, bool &slow)
{
#pragma clang fp contract(off)
    value = text_nan();
    slow = false;
    text_strip(p, len);
    if (len == 0) return 0;                                             // an empty field is a NaN
    if (text_is(p, len, "nan", 3) || text_is(p, len, "NaN", 3) || text_is(p, len, "NA", 2)) return 0;
    int64_t i = 0;
    bool neg = false;
    if (p[0] == '+' || p[0] == '-') {
        neg = p[0] == '-';
        i = 1;
    }
    if (text_is(p + i, len - i, "inf", 3) || text_is(p + i, len - i, "Infinity", 8)) {
        value = text_inf(neg);
        return 0;
    }
    uint64_t m = 0;                 // the significand's digits, leading zeros stripped, at most 19 of them
    int nd = 0;
    int64_t e10 = 0;                // value = m * 10^e10
    bool any = false, many = false;
    for (; i < len && text_digit(p[i]); ++i) {
        const uint64_t d = p[i] - '0';
        any = true;
        if (m == 0 && d == 0) continue;
        if (nd < 19) {
            m = m * 10 + d;
            ++nd;
        } else {
            many = true;
        }
    }
    if (i < len && p[i] == '.') {
        for (++i; i < len && text_digit(p[i]); ++i) {
            const uint64_t d = p[i] - '0';
            any = true;
            if (m == 0 && d == 0) {
                --e10;
                continue;
            }
            if (nd < 19) {
                m = m * 10 + d;
                ++nd;
                --e10;
            } else {
                many = true;
            }
        }
    }
    if (!any) return NGCF_TEXT_KIND_BYTE;
    if (i < len && (p[i] == 'e' || p[i] == 'E')) {
        ++i;
        bool eneg = false;
        if (i < len && (p[i] == '+' || p[i] == '-')) {
            eneg = p[i] == '-';
            ++i;
        }
        if (i == len || !text_digit(p[i])) return NGCF_TEXT_KIND_BYTE;
        int64_t ex = 0;
        for (; i < len && text_digit(p[i]); ++i) ex = ex < 100000 ? ex * 10 + (p[i] - '0') : ex;      // beyond any double either way
        e10 += eneg ? -ex : ex;
    }
    if (i != len) return NGCF_TEXT_KIND_BYTE;
    if (many) {
        slow = true;
        return 0;
    }
    if (m == 0) {
        value = neg ? -0.0 : 0.0;
        return 0;
    }
    if (m > (1ull << 53) || e10 > 22 || e10 < -22) {
        slow = true;
        return 0;
    }
    // ONE correctly rounded IEEE operation on two exact operands: the bits of strtod
    const double md = (double)(long long)m;
    const double v = e10 >= 0 ? md * kTextPow10[e10] : md / kTextPow10[-e10];
    value = neg ? -v : v;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// parse
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTextThreads) void text_parse_kernel(const uint8_t *__restrict__ data, int64_t n, const int64_t *__restrict__ starts,
                                                                  int64_t n_rows, int64_t skip_rows, TextCols cols, uint8_t delim,
                                                                  int64_t *__restrict__ slow_list, int64_t slow_capacity, int tier,
                                                                  unsigned long long *status)
{
    __shared__ uint4 s_stage[kTextLdsBytes / 16 + 1];                   // the window starts at a 16-byte boundary at or below the run
    __shared__ int8_t s_slot[kTextMaxFields];
    __shared__ uint8_t s_field[kTextMaxColumns], s_kind[kTextMaxColumns];
    __shared__ void *s_out[kTextMaxColumns];
    const int tid = threadIdx.x;
    if (tid < kTextMaxFields) s_slot[tid] = cols.slot_of_field[tid];
    if (tid < kTextMaxColumns) {
        s_field[tid] = cols.field[tid];
        s_kind[tid] = cols.kind[tid];
        s_out[tid] = cols.out[tid];
    }
    const int64_t n_data = n_rows - skip_rows;
    const int64_t d0 = (int64_t)blockIdx.x * kTextRows;                 // the run's first data row
    const int64_t d1 = d0 + kTextRows < n_data ? d0 + kTextRows : n_data;
    // the staged window [w_lo, w_hi): the run's bytes, cut at the budget
    int64_t w_lo = starts[skip_rows + d0], w_hi = starts[skip_rows + d1];
    if (tier == 1 || w_lo < 0 || w_hi < w_lo || w_hi > n) w_hi = w_lo = 0;
    if (w_hi - w_lo > kTextLdsBytes) w_hi = w_lo + kTextLdsBytes;
    const int64_t a0 = w_lo & ~(int64_t)15;
    const int n_chunks = (int)((w_hi - a0 + 15) >> 4);                  // <= kTextLdsBytes / 16 + 1
    for (int k = tid; k < n_chunks; k += kTextThreads) {
        const int64_t g = a0 + 16 * (int64_t)k;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (g + 16 <= n) {
            v = *reinterpret_cast<const uint4 *>(data + g);             // data is 16-byte aligned
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (int j = 0; g + j < n; ++j) w[j >> 2] |= (uint32_t)data[g + j] << (8 * (j & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        s_stage[k] = v;
    }
    __syncthreads();
    const int64_t d = d0 + tid;
    if (d >= d1) return;
    const int n_columns = cols.n_columns, n_fields = cols.n_fields;
    const int64_t r0 = starts[skip_rows + d], r1 = starts[skip_rows + d + 1];
    uint32_t bits = 0, first = 0xffffffffu;                             // this row's status bits and its first (field, kind)
    auto report = [&](int field, int kind) {
        bits |= 1u << (kind - 1);
        const uint32_t key = ((uint32_t)field << 8) | (uint32_t)kind;
        first = key < first ? key : first;
    };
    int nf = 0;
    if (r0 < 0 || r1 <= r0 || r1 > n) {
        bits |= NGCF_TEXT_LOST;                                         // row pointers that do not belong to the buffer: never read through
    } else {
        const bool staged = r0 >= w_lo && r1 <= w_hi;
        if (!staged && tier == 2) bits |= NGCF_TEXT_TIER;
        const uint8_t *row = staged ? reinterpret_cast<const uint8_t *>(s_stage) + (r0 - a0) : data + r0;
        int64_t len = 0;                                                // the row's text: up to its '\n', less a '\r' in front of that
        while (len < r1 - r0 && row[len] != '\n') ++len;
        if (len > 0 && row[len - 1] == '\r' && (len < r1 - r0 || r1 == n)) --len;
        int64_t fs = 0;
        bool quoted = false;                                            // this field holds a '"': that is its error, whatever else it holds
        for (int64_t i = 0; i <= len; ++i) {
            const uint8_t c = i < len ? row[i] : delim;
            if (c == '"') {
                quoted = true;
                report(nf < 255 ? nf : 255, NGCF_TEXT_KIND_QUOTE);
            }
            if (c != delim) continue;
            const int slot = nf < kTextMaxFields ? s_slot[nf] : -1;
            if (slot >= 0) {
                if (s_kind[slot] == 0) {
                    int64_t v;
                    const int err = text_parse_int(row + fs, i - fs, v);
                    if (err && !quoted) report(nf, err);
                    static_cast<int64_t *>(s_out[slot])[d] = v;
                } else {
                    double v;
                    bool slow;
                    const int err = text_parse_float(row + fs, i - fs, v, slow);
                    if (err && !quoted) report(nf, err);
                    static_cast<double *>(s_out[slot])[d] = v;
                    if (slow) {
                        const unsigned long long at = atomicAdd(status + 2, 1ull);
                        if ((int64_t)at < slow_capacity) slow_list[at] = (d << 8) | slot;
                    }
                }
            }
            if (nf < 0x7fffffff) ++nf;
            fs = i + 1;
            quoted = false;
        }
        if (nf != n_fields) report(0, NGCF_TEXT_KIND_FIELDS);
    }
    for (int s = 0; s < n_columns; ++s) {                               // the selected fields the row does not have
        if (s_field[s] < nf) continue;
        if (s_kind[s] == 0) static_cast<int64_t *>(s_out[s])[d] = 0;
        else static_cast<double *>(s_out[s])[d] = text_nan();
    }
    if (bits) atomicOr(status, (unsigned long long)bits);
    if (first != 0xffffffffu) atomicMin(status + 1, ((unsigned long long)d << 16) | first);
}

bool text_delimiter_ok(int c)
{
    if (c < 1 || c >= 0x80) return false;
    if (c >= '0' && c <= '9') return false;
    return !strchr("+-.eE \t\r\n\"", c);
}

}  // namespace

extern "C" int ngcf_text_limits(int *rows_per_workgroup, int *lds_bytes, int *count_block_bytes)
{
    if (rows_per_workgroup) *rows_per_workgroup = kTextRows;
    if (lds_bytes) *lds_bytes = kTextLdsBytes;
    if (count_block_bytes) *count_block_bytes = kTextCountBlock;
    return NGCF_OK;
}

static int text_check_buffer(const char *fn, const uint8_t *data, int64_t n, const void *status, int64_t &n_blocks)
{
    if (n < 0) return fail(NGCF_ERR_ARG, "%s: negative count (n=%lld)", fn, (long long)n);
    if (!status || (n > 0 && !data)) return fail(NGCF_ERR_ARG, "%s: null argument", fn);
    if (!aligned16(data)) return fail(NGCF_ERR_ARG, "%s: the buffer is not 16-byte aligned", fn);
    if (reinterpret_cast<uintptr_t>(status) & 7) return fail(NGCF_ERR_ARG, "%s: the status block is not 8-byte aligned", fn);
    n_blocks = (n + kTextCountBlock - 1) / kTextCountBlock;
    if (n_blocks > 0x7fffffffll) return fail(NGCF_ERR_ARG, "%s: n=%lld does not fit a grid", fn, (long long)n);
    return NGCF_OK;
}

extern "C" int ngcf_text_count_rows(const uint8_t *data, int64_t n, int64_t *block_counts, int64_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    int64_t n_blocks = 0;
    if (const int rc = text_check_buffer("text_count_rows", data, n, status, n_blocks)) return rc;
    if (n == 0) return NGCF_OK;
    if (!block_counts) return fail(NGCF_ERR_ARG, "text_count_rows: null argument");
    text_count_kernel<<<dim3((unsigned)n_blocks), kTextThreads, 0, stream>>>(data, n, block_counts, reinterpret_cast<unsigned long long *>(status));
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_text_row_starts(const uint8_t *data, int64_t n, const int64_t *block_offsets, int64_t n_rows, int64_t *starts,
                                    int64_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    int64_t n_blocks = 0;
    if (const int rc = text_check_buffer("text_row_starts", data, n, status, n_blocks)) return rc;
    if (n_rows < 0 || n_rows > n) return fail(NGCF_ERR_ARG, "text_row_starts: n_rows=%lld outside [0, n = %lld]", (long long)n_rows, (long long)n);
    if (!starts) return fail(NGCF_ERR_ARG, "text_row_starts: null argument");
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(starts, 0, sizeof(int64_t), stream));    // starts[0] = n = 0
        return NGCF_OK;
    }
    if (!block_offsets) return fail(NGCF_ERR_ARG, "text_row_starts: null argument");
    text_starts_kernel<<<dim3((unsigned)n_blocks), kTextThreads, 0, stream>>>(data, n, block_offsets, n_rows, starts,
                                                                            reinterpret_cast<unsigned long long *>(status));
    LAUNCH_CHECK();
    return NGCF_OK;
}

extern "C" int ngcf_text_parse_columns(const uint8_t *data, int64_t n, const int64_t *starts, int64_t n_rows, int64_t skip_rows, int n_fields,
                                       int delimiter, const int32_t *fields, const int32_t *kinds, int n_columns, void *const *out,
                                       int64_t *slow_list, int64_t slow_capacity, int tier, int64_t *status, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *fn = "text_parse_columns";
    int64_t n_blocks = 0;
    if (const int rc = text_check_buffer(fn, data, n, status, n_blocks)) return rc;
    if (!text_delimiter_ok(delimiter))
        return fail(NGCF_ERR_ARG, "%s: delimiter %d is not a single byte below 0x80 outside digits, '+-.eE', blanks, line ends and '\"'", fn, delimiter);
    if (n_fields < 1 || n_fields > kTextMaxFields) return fail(NGCF_ERR_ARG, "%s: %d fields, outside [1, %d]", fn, n_fields, kTextMaxFields);
    if (n_columns < 1 || n_columns > kTextMaxColumns)
        return fail(NGCF_ERR_ARG, "%s: %d selected columns, outside [1, %d]", fn, n_columns, kTextMaxColumns);
    if (n_rows < 0 || skip_rows < 0 || skip_rows > n_rows || n_rows > n)
        return fail(NGCF_ERR_ARG, "%s: bad row counts (n_rows=%lld, skip_rows=%lld, n=%lld)", fn, (long long)n_rows, (long long)skip_rows, (long long)n);
    if (slow_capacity < 0 || tier < 0 || tier > 2) return fail(NGCF_ERR_ARG, "%s: slow_capacity=%lld or tier=%d out of range", fn, (long long)slow_capacity, tier);
    if (!fields || !kinds || !out || !starts || (slow_capacity > 0 && !slow_list)) return fail(NGCF_ERR_ARG, "%s: null argument", fn);
    TextCols cols = {};
    cols.n_columns = n_columns;
    cols.n_fields = n_fields;
    memset(cols.slot_of_field, -1, sizeof(cols.slot_of_field));
    for (int s = 0; s < n_columns; ++s) {
        if (fields[s] < 0 || fields[s] >= n_fields) return fail(NGCF_ERR_ARG, "%s: column %d selects field %d of %d", fn, s, fields[s], n_fields);
        if (kinds[s] != 0 && kinds[s] != 1) return fail(NGCF_ERR_ARG, "%s: column %d has kind %d, neither 0 (int64) nor 1 (float64)", fn, s, kinds[s]);
        if (cols.slot_of_field[fields[s]] >= 0) return fail(NGCF_ERR_ARG, "%s: field %d is selected twice", fn, fields[s]);
        if (!out[s] && n_rows > skip_rows) return fail(NGCF_ERR_ARG, "%s: null argument (column %d)", fn, s);
        cols.slot_of_field[fields[s]] = (int8_t)s;
        cols.field[s] = (uint8_t)fields[s];
        cols.kind[s] = (uint8_t)kinds[s];
        cols.out[s] = out[s];
    }
    const int64_t n_data = n_rows - skip_rows;
    if (n_data == 0) return NGCF_OK;
    if (n_data >= (1ll << 40)) return fail(NGCF_ERR_ARG, "%s: %lld rows, beyond the 2^40 of the error word", fn, (long long)n_data);
    const int64_t grid = (n_data + kTextRows - 1) / kTextRows;
    text_parse_kernel<<<dim3((unsigned)grid), kTextThreads, 0, stream>>>(data, n, starts, n_rows, skip_rows, cols, (uint8_t)delimiter, slow_list,
                                                                      slow_capacity, tier, reinterpret_cast<unsigned long long *>(status));
    LAUNCH_CHECK();
    return NGCF_OK;
}
