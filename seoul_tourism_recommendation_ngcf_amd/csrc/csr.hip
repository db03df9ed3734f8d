// csr.hip - the Laplacian CSR object: construction from COO triplets or CSR arrays, its row-segment plan, its row groups and
// the kernel mode (ngcf_csr_set_mode).
#include "common.h"

// ---------------------------------------------------------------------------------------------
// segment sets: the rows longer than seg_len, cut into segments (the CSR's own plan, and the swept plan's `out`)
// ---------------------------------------------------------------------------------------------
HostSegs cut_rows(const std::vector<int64_t> &rp, const std::vector<std::pair<int64_t, int64_t>> &ranges, int32_t seg_len)
{
    HostSegs h;
    h.heavy_ptr.push_back(0);
    for (const auto &range : ranges)
        for (int64_t r = range.first; r < range.second; ++r) {
            if (rp[(size_t)r + 1] - rp[(size_t)r] <= seg_len) continue;
            h.heavy_row.push_back((int32_t)r);
            for (int64_t b = rp[(size_t)r]; b < rp[(size_t)r + 1]; b += seg_len) {
                h.seg_row.push_back((int32_t)r);
                h.seg_begin.push_back(b);
            }
            h.heavy_ptr.push_back((int64_t)h.seg_row.size());
        }
    return h;
}

int upload_segset(ngcf_csr::SegSet &s, const HostSegs &h, hipStream_t stream)
{
    s.n_seg = (int64_t)h.seg_row.size();
    s.n_heavy = (int64_t)h.heavy_row.size();
    if (s.n_seg == 0) return NGCF_OK;
    int rc = upload(&s.seg_row, h.seg_row, stream);
    if (rc == NGCF_OK) rc = upload(&s.seg_begin, h.seg_begin, stream);
    if (rc == NGCF_OK) rc = upload(&s.heavy_row, h.heavy_row, stream);
    if (rc == NGCF_OK) rc = upload(&s.heavy_seg_ptr, h.heavy_ptr, stream);
    return rc;
}

void free_segset(ngcf_csr::SegSet &s, bool borrowed)
{
    if (s.seg_begin) (void)hipFree(s.seg_begin);
    if (!borrowed) {                   // a filtered copy shares its source's segment lists (it owns seg_begin only)
        if (s.seg_row) (void)hipFree(s.seg_row);
        if (s.heavy_row) (void)hipFree(s.heavy_row);
        if (s.heavy_seg_ptr) (void)hipFree(s.heavy_seg_ptr);
    }
    s = ngcf_csr::SegSet();
}

extern "C" void ngcf_csr_free(ngcf_csr_t *c)
{
    if (!c) return;
    free_segset(c->seg, c->borrows_plan);
    free_swept(c);
    if (c->owns) {
        if (c->rowptr) (void)hipFree(c->rowptr);
        if (c->colidx) (void)hipFree(c->colidx);
        if (c->vals) (void)hipFree(c->vals);
    }
    if (c->pos) (void)hipFree(c->pos);
    if (c->scan_blk) (void)hipFree(c->scan_blk);
    delete c;
}

extern "C" int64_t ngcf_csr_nnz(const ngcf_csr_t *c) { return c ? c->nnz : -1; }
extern "C" int64_t ngcf_csr_n_rows(const ngcf_csr_t *c) { return c ? c->n_rows : -1; }
extern "C" int64_t ngcf_csr_n_cols(const ngcf_csr_t *c) { return c ? c->n_cols : -1; }
extern "C" int64_t ngcf_csr_n_segments(const ngcf_csr_t *c) { return c ? c->seg.n_seg : -1; }
extern "C" int64_t ngcf_csr_max_row_len(const ngcf_csr_t *c) { return c ? c->max_row_len : -1; }
extern "C" int64_t ngcf_csr_swept_rows(const ngcf_csr_t *c)
{
    if (!c) return -1;
    int64_t n = 0;
    for (const auto &p : c->swept.parts) n += p.row_hi - p.row_lo;
    return n;
}
extern "C" int64_t ngcf_csr_n_groups(const ngcf_csr_t *c) { return c ? (int64_t)c->groups.size() : -1; }
extern "C" int ngcf_csr_group(const ngcf_csr_t *c, int64_t g, int64_t *begin, int64_t *end, int *sliceable, int *lds_table,
                              int32_t *col_lo, int32_t *col_hi)
{
    if (!c || g < 0 || g >= (int64_t)c->groups.size()) return fail(NGCF_ERR_ARG, "ngcf_csr_group: no such row group");
    const ngcf_csr::RowGroup &grp = c->groups[(size_t)g];
    if (begin) *begin = grp.begin;
    if (end) *end = grp.end;
    if (sliceable) *sliceable = grp.sliceable ? 1 : 0;
    if (lds_table) *lds_table = grp.lds_table ? 1 : 0;
    if (col_lo) *col_lo = grp.col_lo;
    if (col_hi) *col_hi = grp.col_hi;
    return NGCF_OK;
}
extern "C" const int64_t *ngcf_csr_rowptr(const ngcf_csr_t *c) { return c ? c->rowptr : nullptr; }
extern "C" const int32_t *ngcf_csr_colidx(const ngcf_csr_t *c) { return c ? c->colidx : nullptr; }
extern "C" const float *ngcf_csr_vals(const ngcf_csr_t *c) { return c ? c->vals : nullptr; }

// flags[0] |= 1 when rows are not non-decreasing; flags[1] |= 1 when an id is out of range
__global__ void coo_check_kernel(const int64_t *__restrict__ rows, const int64_t *__restrict__ cols,
                                 int64_t nnz, int64_t n_rows, int64_t n_cols, int32_t *flags)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool unsorted = false, bad = false;
    for (; i < nnz; i += stride) {
        const int64_t r = rows[i], c = cols[i];
        bad |= (r < 0) | (r >= n_rows) | (c < 0) | (c >= n_cols);
        if (i + 1 < nnz) unsorted |= rows[i + 1] < r;
    }
    if (unsorted) atomicOr(&flags[0], 1);
    if (bad) atomicOr(&flags[1], 1);
}

// rowptr[r] = first entry whose row id is >= r (rows sorted); one thread per r in [0, n_rows]
__global__ void coo_rowptr_kernel(const int64_t *__restrict__ rows, int64_t nnz, int64_t n_rows,
                                  int64_t *__restrict__ rowptr)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rows) return;
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (rows[mid] < r)
            lo = mid + 1;
        else
            hi = mid;
    }
    rowptr[r] = lo;
}

__global__ void coo_copy_kernel(const int64_t *__restrict__ cols, const float *__restrict__ vals, int64_t nnz,
                                int32_t *__restrict__ colidx, float *__restrict__ out_vals)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < nnz; i += stride) {
        colidx[i] = (int32_t)cols[i];
        out_vals[i] = vals[i];
    }
}


// per block of `group_rows` rows: smallest and largest column any of its rows gathers (one-time, plan only)
__global__ void row_colrange_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                    int64_t n_rows, int group_rows, int32_t *__restrict__ blk_min, int32_t *__restrict__ blk_max)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    int32_t lo = INT32_MAX, hi = -1;
    for (int64_t e = rowptr[row]; e < rowptr[row + 1]; ++e) {
        const int32_t c = colidx[e];
        lo = c < lo ? c : lo;
        hi = c > hi ? c : hi;
    }
    if (hi >= 0) {
        atomicMin(&blk_min[row / group_rows], lo);
        atomicMax(&blk_max[row / group_rows], hi);
    }
}

// A row block is "sliceable" when one 32-float slice (128 B) of every row it gathers is at most 48 MiB: then the
// hot part of the table slice lives in the XCD L2s while a slice-major launch walks it (measured on the user half
// of C3: 2.33 ms sliced vs 2.98 ms unsliced; the 1 M-row user table gets slower sliced: 3.8 vs 3.46 ms).
static int64_t slice_footprint_rows()   // slice_max_mb: lab knob (C5-sized tables: slices that fit the 256 MiB Infinity Cache)
{
    return ((int64_t)ngcf_opts().slice_max_mb << 20) / 128;
}
#define kSliceFootprintRows slice_footprint_rows()

static int build_row_groups(ngcf_csr *c, hipStream_t stream)
{
    c->groups.clear();
    if (c->n_rows == 0) return NGCF_OK;
    // blocks of 1024 rows; 64 on a small matrix, where the border between the user rows and the item rows of a Seoul-sized
    // graph (5 840 + 100 rows) would otherwise put an eighth of the user rows into a mixed block
    const int64_t NGCF_GROUP_ROWS = c->n_rows <= 65536 ? 64 : 1024;
    const int64_t nb = (c->n_rows + NGCF_GROUP_ROWS - 1) / NGCF_GROUP_ROWS;
    int32_t *d_min = nullptr, *d_max = nullptr;
    std::vector<int32_t> h_min((size_t)nb), h_max((size_t)nb);
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&d_min, sizeof(int32_t) * (size_t)nb));
        HIP_TRY(hipMalloc(&d_max, sizeof(int32_t) * (size_t)nb));
        HIP_TRY(hipMemsetAsync(d_min, 0x7f, sizeof(int32_t) * (size_t)nb, stream));   // 0x7f7f7f7f: large
        HIP_TRY(hipMemsetAsync(d_max, 0xff, sizeof(int32_t) * (size_t)nb, stream));   // -1
        row_colrange_kernel<<<(int)((c->n_rows + 255) / 256), 256, 0, stream>>>(c->rowptr, c->colidx, c->n_rows, (int)NGCF_GROUP_ROWS, d_min, d_max);
        LAUNCH_CHECK();
        HIP_TRY(hipMemcpyAsync(h_min.data(), d_min, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(h_max.data(), d_max, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return NGCF_OK;
    };
    const int rc = body();
    if (d_min) (void)hipFree(d_min);
    if (d_max) (void)hipFree(d_max);
    if (rc != NGCF_OK) return rc;
    // class of a row block: 2 = its rows gather from at most kLdsTableRows table rows (the user rows of a graph with a
    // few hundred items - the Seoul data has ~100: the table slice is staged in LDS), 1 = sliceable, 0 = neither
    auto block_class = [&](int64_t b) {
        if (h_max[(size_t)b] < 0) return 1;
        const int64_t range = (int64_t)h_max[(size_t)b] - h_min[(size_t)b] + 1;
        return range <= kLdsTableRows ? 2 : range <= kSliceFootprintRows ? 1 : 0;
    };
    std::vector<int> cls;
    for (int64_t b = 0; b < nb; ++b) {
        const int k = block_class(b);
        const int64_t lo = b * NGCF_GROUP_ROWS, hi = std::min<int64_t>(c->n_rows, lo + NGCF_GROUP_ROWS);
        if (!c->groups.empty() && cls.back() == k) {
            c->groups.back().end = hi;
        } else {
            c->groups.push_back({lo, hi, k >= 1, INT32_MAX, -1, k == 2});
            cls.push_back(k);
        }
    }
    // an LDS-table group must gather from ONE small range as a whole, not only block by block
    for (size_t i = 0; i < c->groups.size(); ++i) {
        if (!c->groups[i].lds_table) continue;
        int32_t lo = INT32_MAX, hi = -1;
        for (int64_t b = c->groups[i].begin / NGCF_GROUP_ROWS; b * NGCF_GROUP_ROWS < c->groups[i].end; ++b)
            if (h_max[(size_t)b] >= 0) lo = std::min(lo, h_min[(size_t)b]), hi = std::max(hi, h_max[(size_t)b]);
        if (hi >= 0 && (int64_t)hi - lo + 1 > kLdsTableRows) c->groups[i].lds_table = false;
    }
    // a group of a few blocks is not worth its own launch: give it its neighbour's class, then fuse equal neighbours
    // (LDS-table groups keep to themselves: on a Seoul-shaped graph they are most of the rows of a six-block matrix)
    auto same = [&](size_t a, size_t b) {
        return c->groups[a].sliceable == c->groups[b].sliceable && !c->groups[a].lds_table && !c->groups[b].lds_table;
    };
    for (size_t i = 0; i < c->groups.size(); ++i) {
        if (c->groups[i].lds_table || c->groups.size() == 1 || c->groups[i].end - c->groups[i].begin >= 16 * NGCF_GROUP_ROWS) continue;
        const size_t nb_i = i > 0 ? i - 1 : i + 1;
        if (!c->groups[nb_i].lds_table) c->groups[i].sliceable = c->groups[nb_i].sliceable;
    }
    for (size_t k = 1; k < c->groups.size();) {
        if (same(k, k - 1)) {
            c->groups[k - 1].end = c->groups[k].end;
            c->groups.erase(c->groups.begin() + (long)k);
        } else {
            ++k;
        }
    }
    for (auto &g : c->groups)                  // column range every group gathers from (the swept plan's first question)
        for (int64_t b = g.begin / NGCF_GROUP_ROWS; b * NGCF_GROUP_ROWS < g.end; ++b)
            if (h_max[(size_t)b] >= 0) {
                g.col_lo = std::min(g.col_lo, h_min[(size_t)b]);
                g.col_hi = std::max(g.col_hi, h_max[(size_t)b]);
            }
    return NGCF_OK;
}


extern "C" int ngcf_csr_plan(ngcf_csr_t *c, int32_t seg_len, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!c) return fail(NGCF_ERR_ARG, "ngcf_csr_plan: null csr");
    if (seg_len < 64) return fail(NGCF_ERR_ARG, "ngcf_csr_plan: seg_len must be >= 64 (got %d)", seg_len);
    free_segset(c->seg, c->borrows_plan);
    c->borrows_plan = false;
    c->seg_len = seg_len;
    std::vector<int64_t> rp((size_t)c->n_rows + 1);
    HIP_TRY(hipMemcpyAsync(rp.data(), c->rowptr, sizeof(int64_t) * rp.size(), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    c->max_row_len = 0;
    for (int64_t r = 0; r < c->n_rows; ++r) c->max_row_len = std::max(c->max_row_len, rp[(size_t)r + 1] - rp[(size_t)r]);
    {
        const HostSegs segs = cut_rows(rp, {{0, c->n_rows}}, seg_len);
        const int rc = upload_segset(c->seg, segs, stream);
        if (rc != NGCF_OK) return rc;
        if (c->seg.n_seg > 0) HIP_TRY(hipStreamSynchronize(stream));
    }
    {
        const int rc = build_row_groups(c, stream);
        if (rc != NGCF_OK) return rc;
    }
    if (c->mode >= 2) return build_swept_plan(c, stream);          // the parts follow the row groups and seg_len
    free_swept(c);
    return NGCF_OK;
}

extern "C" int ngcf_csr_set_mode(ngcf_csr_t *c, int mode, void *stream)
{
    if (!c || mode < 0 || mode > 3) return fail(NGCF_ERR_ARG, "ngcf_csr_set_mode: bad argument");
    c->mode = mode;
    if (mode < 2) {
        free_swept(c);
        return NGCF_OK;
    }
    if (c->swept.built_mode != mode) return build_swept_plan(c, (hipStream_t)stream);
    return NGCF_OK;
}

extern "C" int ngcf_csr_from_arrays(const int64_t *rowptr, const int32_t *colidx, const float *vals,
                                    int64_t n_rows, int64_t n_cols, int64_t nnz, ngcf_csr_t **out, void *stream)
{
    if (!out) return fail(NGCF_ERR_ARG, "ngcf_csr_from_arrays: null out");
    *out = nullptr;
    if (!rowptr || (nnz > 0 && (!colidx || !vals)))
        return fail(NGCF_ERR_ARG, "ngcf_csr_from_arrays: null array");
    if (n_rows < 0 || n_cols < 0 || nnz < 0 || n_cols >= (int64_t)1 << 31 || n_rows >= (int64_t)1 << 31)
        return fail(NGCF_ERR_ARG, "ngcf_csr_from_arrays: bad shape %lld x %lld nnz %lld", (long long)n_rows,
                    (long long)n_cols, (long long)nnz);
    ngcf_csr *c = new ngcf_csr();
    c->n_rows = n_rows;
    c->n_cols = n_cols;
    c->nnz = nnz;
    c->rowptr = const_cast<int64_t *>(rowptr);
    c->colidx = const_cast<int32_t *>(colidx);
    c->vals = const_cast<float *>(vals);
    c->owns = false;
    const int rc = ngcf_csr_plan(c, default_seg_len(c->nnz), stream);
    if (rc != NGCF_OK) {
        ngcf_csr_free(c);
        return rc;
    }
    *out = c;
    return NGCF_OK;
}

extern "C" int ngcf_csr_from_coo(const int64_t *rows, const int64_t *cols, const float *vals, int64_t nnz,
                                 int64_t n_rows, int64_t n_cols, ngcf_csr_t **out, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!out) return fail(NGCF_ERR_ARG, "ngcf_csr_from_coo: null out");
    *out = nullptr;
    if (nnz < 0 || n_rows < 0 || n_cols < 0 || n_cols >= (int64_t)1 << 31 || n_rows >= (int64_t)1 << 31)
        return fail(NGCF_ERR_ARG, "ngcf_csr_from_coo: bad shape %lld x %lld nnz %lld", (long long)n_rows,
                    (long long)n_cols, (long long)nnz);
    if (nnz > 0 && (!rows || !cols || !vals)) return fail(NGCF_ERR_ARG, "ngcf_csr_from_coo: null array");

    ngcf_csr *c = new ngcf_csr();
    c->n_rows = n_rows;
    c->n_cols = n_cols;
    c->nnz = nnz;
    c->owns = true;
    int32_t *flags = nullptr;
    int rc = NGCF_OK;
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&c->rowptr, sizeof(int64_t) * (size_t)(n_rows + 1)));
        HIP_TRY(hipMalloc(&c->colidx, sizeof(int32_t) * (size_t)std::max<int64_t>(nnz, 1)));
        HIP_TRY(hipMalloc(&c->vals, sizeof(float) * (size_t)std::max<int64_t>(nnz, 1)));
        HIP_TRY(hipMalloc(&flags, 2 * sizeof(int32_t)));
        HIP_TRY(hipMemsetAsync(flags, 0, 2 * sizeof(int32_t), stream));
        int32_t h_flags[2] = {0, 0};
        if (nnz > 0) {
            coo_check_kernel<<<grid_for(nnz, 256), 256, 0, stream>>>(rows, cols, nnz, n_rows, n_cols, flags);
            LAUNCH_CHECK();
        }
        HIP_TRY(hipMemcpyAsync(h_flags, flags, sizeof(h_flags), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (h_flags[1])
            return fail(NGCF_ERR_INDEX, "ngcf_csr_from_coo: index out of range for a %lld x %lld matrix",
                        (long long)n_rows, (long long)n_cols);
        if (!h_flags[0]) {
            // rows already sorted (what matrix.py:79-83 emits): convert on the device
            coo_rowptr_kernel<<<(int)((n_rows + 1 + 255) / 256), 256, 0, stream>>>(rows, nnz, n_rows, c->rowptr);
            LAUNCH_CHECK();
            if (nnz > 0) {
                coo_copy_kernel<<<grid_for(nnz, 256), 256, 0, stream>>>(cols, vals, nnz, c->colidx, c->vals);
                LAUNCH_CHECK();
            }
        } else {
            // unsorted input: stable sort by row on the host (one-time set-up path)
            std::vector<int64_t> hr((size_t)nnz), hc((size_t)nnz);
            std::vector<float> hv((size_t)nnz);
            HIP_TRY(hipMemcpyAsync(hr.data(), rows, sizeof(int64_t) * (size_t)nnz, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipMemcpyAsync(hc.data(), cols, sizeof(int64_t) * (size_t)nnz, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipMemcpyAsync(hv.data(), vals, sizeof(float) * (size_t)nnz, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            std::vector<int64_t> rp((size_t)n_rows + 1, 0);
            for (int64_t i = 0; i < nnz; ++i) rp[(size_t)hr[i] + 1]++;
            for (int64_t r = 0; r < n_rows; ++r) rp[(size_t)r + 1] += rp[(size_t)r];
            std::vector<int64_t> cur(rp.begin(), rp.end() - 1);
            std::vector<int32_t> oc((size_t)nnz);
            std::vector<float> ov((size_t)nnz);
            for (int64_t i = 0; i < nnz; ++i) {   // counting sort = stable
                const int64_t dst = cur[(size_t)hr[i]]++;
                oc[(size_t)dst] = (int32_t)hc[i];
                ov[(size_t)dst] = hv[i];
            }
            HIP_TRY(hipMemcpyAsync(c->rowptr, rp.data(), sizeof(int64_t) * rp.size(), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(c->colidx, oc.data(), sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(c->vals, ov.data(), sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        return ngcf_csr_plan(c, default_seg_len(c->nnz), stream);
    };
    rc = body();
    if (flags) (void)hipFree(flags);
    if (rc != NGCF_OK) {
        ngcf_csr_free(c);
        return rc;
    }
    *out = c;
    return NGCF_OK;
}



