// dense.hip - the dense half of a layer on the matrix cores, host side: the dispatch, ngcf_layer_dense_f32 and the fused layer entry
// point.  No kernel lives here.  Five forward kernels compute the same layer; dense_path() below picks one by shape and
// ngcf_layer_dense_f32 calls that path's launch function:
//   dense_staged.hip      layer_dense_kernel (any shape), pack_weights_kernel       dense_pack_fp32, dense_launch_staged
//   dense_persistent.hip  layer_dense_resident_kernel, layer_dense_split_kernel     dense_launch_resident, dense_launch_split
//   dense_wide.hip        layer_dense_direct_kernel, layer_dense_tall_kernel        dense_launch_direct, dense_launch_tall
//   dense_device.h        what more than one of them needs, each defined once (the list is at its top)
#include "dense_device.h"

static int dense_dop(int d_out)
{
    if (d_out <= 32) return 32;
    if (d_out <= 64) return 64;
    if (d_out <= 96) return 96;
    if (d_out <= 128) return 128;
    if (d_out <= 256) return 256;
    if (d_out <= 512) return 512;
    return -1;
}

extern "C" int64_t ngcf_dense_workspace_bytes(int d_in, int d_out)
{
    int dop = dense_dop(d_out);
    if (dop < 0 || d_in <= 0) return -1;
    dop = std::max(dop, 128);                  // small matrices run narrow layers on 32-row x 128-column tiles
    const int64_t n_chunks = (d_in + NGCF_DC - 1) / NGCF_DC;
    const int64_t fp32_packed = (n_chunks * NGCF_KC * dop + dop) * (int64_t)sizeof(float);
    const int64_t split_packed = 128 * (int64_t)sizeof(float) + n_chunks * 3 * 8 * 1024;   // bias, parts h + m, part l
    return align_up(std::max(fp32_packed, split_packed), 256) + 256;
}

// Which forward kernel a call takes.  Every decision of the dispatch is made HERE, once: ngcf_layer_dense_f32 launches what this
// returns and ngcf_dense_path reports its name, so a test that names a kernel fails when the dispatch stops sending it there.
// Pure host code: the sizes, the alignment of the operands and the options (ngcf_opts()), nothing else.  d_out <= 512 (dop > 0).
static DensePath dense_path(int64_t n_rows, int d_in, int d_out, const float *LE, int64_t ldLE, const float *Es, int64_t ldEs)
{
    DensePath p{};
    p.dop = dense_dop(d_out);
    // Up to 128 output columns on a SMALL matrix (the Seoul graph: 5 940 rows): 128-row tiles are 47 workgroups on 256 CUs and the
    // 65 -> 65 layer of the reference's own configuration took 28-30 us; 32-row x 128-column tiles (four waves side by side, one
    // tile each) are 186 workgroups.  From 16 384 rows on (128 tiles of 128 rows) the tall tiles stay.
    p.small_rows = p.dop <= 128 && n_rows <= 16384 && ngcf_opts().dense_small_tiles;
    if (p.small_rows) p.dop = 128;
    const int dop = p.dop;
    p.al = (ldLE % 4 == 0) && (ldEs % 4 == 0) && aligned16(LE) && aligned16(Es);
    // 16-byte aligned rows padded to a multiple of 4 floats: what the tall, resident, split and direct kernels read
    p.padded = p.al && ldLE >= align_up(d_in, 4) && ldEs >= align_up(d_in, 4) && d_in >= 4;
    const int n_chunks = (d_in + NGCF_DC - 1) / NGCF_DC;

    // 256 / 512 output columns as 96-row x 128-column workgroups, three row tiles per wave, the row norm in a second kernel
    // (layer_dense_tall_kernel): 248 workgroups for the Seoul graph's 5 940 rows where the direct kernel has 186.  Measured
    // (tools/dense_wide_lab.py, profiles/r03_dense_wide_lab.txt; tall / direct / staged, us incl. pack and row scale):
    //   512 columns: 5 940 rows 84 / 92 / 109; 6 144: 84 / 93 / 109; 7 000: 127 / 89 / 107 (a second round of workgroups; the direct
    //   kernel still has one per CU up to 8 192 rows); 9 000: 132 / 267 / 165; 100 K: 956 / 1 384 / 1 078; 1.1 M: 10 129 / 12 114 / 10 858
    //   256 columns: 5 940 rows 47 / 47 / 58 (124 workgroups: no gain); 9 000: 48 / 78 / 59; 100 K: 290 / 418 / 310; 200 K: 569 / 735 / 552
    // dense_tall = 0: never; 2: wherever the shape allows; 1: by these numbers.
    const int tall_env = ngcf_opts().dense_tall;
    const bool tall_pays = dop == 512 ? (n_rows <= 6144 || n_rows > 8192) : (n_rows > 8192 && n_rows <= 131072);
    if (tall_env && dop >= 256 && p.padded && (tall_pays || tall_env == 2)) {
        p.kernel = kDenseTall;
        p.name = dop == 256 ? "tall256" : "tall512";
        return p;
    }

    // Weights resident in LDS, no barriers: large row counts at the 128-wide shapes, from two tiles per wave on.  dense_resident
    // = 4: the bf16 three-way split (layer_dense_split_kernel); 1 (any other non-zero value): the fp32 layer_dense_resident_kernel
    // (128 -> 128, resident / staged us: 65 536 rows 59 / 59, 98 304 rows 95 / 85, 131 072 rows 96 / 104, 262 144 rows 184 / 212,
    // C3's 1.1 M rows 633 / 780); 0: the staged kernel.
    const int resident = ngcf_opts().dense_resident;
    const int64_t lds_bytes = (int64_t)n_chunks * NGCF_KC * 128 * (int64_t)sizeof(float);
    const bool resident_fits = resident && dop == 128 && p.padded && lds_bytes <= 150 * 1024 &&
                               n_rows >= (int64_t)ngcf_opts().dense_resident_min_rows;
    if (resident_fits) {
        p.kernel = resident == 4 ? kDenseSplit : kDenseResident;
        p.name = resident == 4 ? "split" : "resident";
        return p;
    }

    // 256 / 512 output columns and at most ONE workgroup per CU (<= 8 192 rows - the Seoul graph has 5 940): operands straight
    // from global memory / L2, no staging (layer_dense_direct_kernel).  tools/dense_wide_lab.py: 94 vs 114 us at 5 940 x 515 -> 512,
    // 50 vs 57 us at 256 -> 256, 97 vs 117 us at 8 192 x 512 -> 512; as soon as a CU gets a second workgroup the staged kernel
    // (two workgroups share a CU's LDS and matrix pipe; the direct kernel runs one wave per SIMD) wins clearly: 170 vs 277 us at
    // 12 288 rows, 1.08 vs 1.40 ms at 100 K.  NGCF_DENSE_DIRECT=0 / 2: never / at any row count.
    const int direct_env = ngcf_opts().dense_direct;
    if (direct_env && dop >= 256 && p.padded && (n_rows <= 8192 || direct_env == 2)) {
        p.kernel = kDenseDirect;
        p.name = dop == 256 ? "direct<2,4>" : "direct<4,4>";
        return p;
    }

    // the staged kernel (layer_dense_kernel): the tile configuration by width, the row layout by alignment
#define NGCF_STAGED_NAMES(cfg) {"staged" cfg "/unaligned", "staged" cfg "/aligned", "staged" cfg "/padded"}
    static const char *const names[7][3] = {NGCF_STAGED_NAMES("<1,4,1>"), NGCF_STAGED_NAMES("<4,1,1>"), NGCF_STAGED_NAMES("<4,1,2>"),
                                            NGCF_STAGED_NAMES("<4,1,3>"), NGCF_STAGED_NAMES("<4,1,4>"), NGCF_STAGED_NAMES("<2,2,4>"),
                                            NGCF_STAGED_NAMES("<1,4,4>")};
#undef NGCF_STAGED_NAMES
    p.kernel = kDenseStaged;
    p.tile = p.small_rows ? 0 : dop <= 128 ? dop / 32 : dop == 256 ? 5 : 6;
    p.name = names[p.tile][p.padded ? 2 : p.al ? 1 : 0];
    return p;
}

extern "C" const char *ngcf_dense_path(int64_t n_rows, int d_in, int d_out, const float *LE, int64_t ldLE, const float *Es, int64_t ldEs)
{
    if (n_rows < 0 || d_in <= 0 || d_out <= 0 || dense_dop(d_out) < 0 || ldLE < d_in || ldEs < d_in) {
        fail(NGCF_ERR_ARG, "dense_path: bad sizes");
        return nullptr;
    }
    return dense_path(n_rows, d_in, d_out, LE, ldLE, Es, ldEs).name;
}

extern "C" int ngcf_layer_dense_f32(const float *LE, int64_t ldLE, const float *Es, int64_t ldEs, int64_t n_rows,
                                    int d_in, const float *W1, const float *b1, const float *W2, const float *b2,
                                    int d_out, float leaky, float drop_p, uint64_t drop_seed, const float *drop_mask,
                                    int64_t ld_mask, float *carry, int64_t ldc, float *norm, int64_t ldn, void *workspace,
                                    int64_t workspace_bytes, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!LE || !Es || !W1 || !b1 || !W2 || !b2 || !norm) return fail(NGCF_ERR_ARG, "layer_dense: null argument");
    if (n_rows < 0 || d_in <= 0 || d_out <= 0) return fail(NGCF_ERR_ARG, "layer_dense: bad sizes");
    if (dense_dop(d_out) < 0) return fail(NGCF_ERR_ARG, "layer_dense: d_out=%d > 512 is not supported", d_out);
    if (!(drop_p >= 0.f && drop_p < 1.f)) return fail(NGCF_ERR_ARG, "layer_dense: drop_p=%f not in [0,1)", drop_p);
    if (ldLE < d_in || ldEs < d_in || ldn < d_out || (carry && ldc < d_out) || (drop_mask && ld_mask < d_out))
        return fail(NGCF_ERR_ARG, "layer_dense: leading dimension too small");
    const int64_t need = ngcf_dense_workspace_bytes(d_in, d_out);
    if (!workspace || workspace_bytes < need)
        return fail(NGCF_ERR_WORKSPACE, "layer_dense: workspace %lld B < %lld B", (long long)workspace_bytes, (long long)need);
    // Nothing to compute, and no kernel may run: the persistent kernels' row_of() would clamp to row -1 (dense_resident_min_rows
    // can be set to 0 or below).
    if (n_rows == 0) return NGCF_OK;
    const DensePath path = dense_path(n_rows, d_in, d_out, LE, ldLE, Es, ldEs);   // every decision: see there
    const DenseCall call{LE, ldLE, Es, ldEs, n_rows, d_in, d_out, leaky, drop_p, drop_seed, drop_mask, ld_mask, carry, ldc, norm, ldn, stream};
    const DenseWeights w{W1, b1, W2, b2, reinterpret_cast<float *>(align_up((int64_t)(uintptr_t)workspace, 256)),
                         (d_in + NGCF_DC - 1) / NGCF_DC};
    switch (path.kernel) {
    case kDenseTall: return dense_launch_tall(call, w, path.dop);
    case kDenseSplit: return dense_launch_split(call, w);
    case kDenseResident: return dense_launch_resident(call, w);
    case kDenseDirect: return dense_launch_direct(call, w, path.dop);
    default: return dense_launch_staged(call, w, path);
    }
}

extern "C" int64_t ngcf_layer_workspace_bytes(const ngcf_csr_t *c, int d_in, int d_out)
{
    if (!c) return -1;
    const int64_t a = ngcf_spmm_workspace_bytes(c, d_in);
    const int64_t b = ngcf_dense_workspace_bytes(d_in, d_out);
    if (a < 0 || b < 0) return -1;
    const int64_t le = align_up(c->n_rows * align_up(d_in, 32) * (int64_t)sizeof(float), 256);   // LE rows start on 128-byte lines
    return a + b + le + 256;
}

extern "C" int ngcf_layer_fused_f32(const ngcf_csr_t *c, const float *Eg, int64_t ldEg, const float *Es, int64_t ldEs,
                                    int d_in, const float *W1, const float *b1, const float *W2, const float *b2,
                                    int d_out, float leaky, float drop_p, uint64_t drop_seed, const float *drop_mask,
                                    int64_t ld_mask, float *carry, int64_t ldc, float *norm, int64_t ldn, void *workspace,
                                    int64_t workspace_bytes, void *stream)
{
    if (!c) return fail(NGCF_ERR_ARG, "layer_fused: null csr");
    const int64_t need = ngcf_layer_workspace_bytes(c, d_in, d_out);
    if (need < 0) return fail(NGCF_ERR_ARG, "layer_fused: unsupported widths d_in=%d d_out=%d", d_in, d_out);
    if (!workspace || workspace_bytes < need)
        return fail(NGCF_ERR_WORKSPACE, "layer_fused: workspace %lld B < %lld B", (long long)workspace_bytes, (long long)need);
    char *ws = reinterpret_cast<char *>(align_up((int64_t)(uintptr_t)workspace, 256));
    const int64_t ldLE = align_up(d_in, 32);
    float *LE = reinterpret_cast<float *>(ws);
    ws += align_up(c->n_rows * ldLE * (int64_t)sizeof(float), 256);
    const int64_t spmm_ws = ngcf_spmm_workspace_bytes(c, d_in);
    void *ws_spmm = ws;
    ws += spmm_ws;
    const int64_t dense_ws = ngcf_dense_workspace_bytes(d_in, d_out);
    void *ws_dense = ws;
    // Widths that are not a multiple of 4 (65, 130, 515: NGCF.py:39-43) on a SMALL matrix: the product is launch-bound, and the
    // main + tail panel split costs four extra launches (pack, tail product, fix-up, unpack: 23 of 141 us on the Seoul-shaped C1).
    // When the gathered rows are 16-byte aligned and padded, the columns up to the next multiple of 4 are simply multiplied along:
    // whatever they hold ends up in the padding columns of LE, which the dense half never reads (it selects zeros there).
    // (Reading them cannot fault: the 16-byte piece that holds the last column of a 16-byte aligned row is read whole.  The
    // mirror's engine.spmm asks the same function for the products of the training path, so both paths give the same bits.)
    const int d_sp = ngcf_spmm_product_width(c, Eg, ldEg, d_in);
    int rc = ngcf_spmm_csr_f32(c, Eg, ldEg, d_sp, LE, ldLE, ws_spmm, spmm_ws, stream);
    if (rc != NGCF_OK) return rc;
    return ngcf_layer_dense_f32(LE, ldLE, Es, ldEs, c->n_rows, d_in, W1, b1, W2, b2, d_out, leaky, drop_p, drop_seed,
                                drop_mask, ld_mask, carry, ldc, norm, ldn, ws_dense, dense_ws, stream);
}
