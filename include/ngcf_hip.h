/*
 * ngcf_hip.h - C ABI of libngcf_hip.so, the MI355X (gfx950) NGCF embedding-propagation engine.
 *
 * This is the drop-in boundary for ONE path of haesungpyun/seoul_tourism_recommendation_NGCF:
 * the body of `NGCF.forward` (model/NGCF.py:102-156) and `BPR.forward` (model/bprloss.py:15-22).
 * The reference is pure Python on top of PyTorch, so "what its FFI would bind" is the set of
 * tensor ops it issues on that path; each entry point below names the reference lines it replaces.
 * The Python mirror of the reference's nn.Module surface (seoul_tourism_recommendation_ngcf_amd/
 * NGCF.py, bprloss.py) calls these through ctypes with `tensor.data_ptr()` and
 * `torch.cuda.current_stream().cuda_stream`; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types.
 *   - every `const float*` / `float*` / index pointer is a DEVICE pointer owned by the caller
 *     unless a comment says "host".  The library allocates only ngcf_csr_t objects.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Compute entry points
 *     are asynchronous on that stream; ngcf_csr_* builders synchronise it once (one-time set-up).
 *   - return 0 on success, non-zero on error; ngcf_last_error() gives the message (thread-local).
 *     The Python mirror raises RuntimeError (IndexError for NGCF_ERR_INDEX), like torch does
 *     at the same call sites in the reference.
 *   - row-major fp32 matrices with an explicit leading dimension `ld*` in elements.
 */
#ifndef NGCF_HIP_H
#define NGCF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGCF_OK            0
#define NGCF_ERR_ARG       1   /* bad argument (null pointer, negative size, unsupported width) */
#define NGCF_ERR_HIP       2   /* a HIP runtime call failed */
#define NGCF_ERR_INDEX     3   /* an index is out of range (IndexError in the Python mirror) */
#define NGCF_ERR_WORKSPACE 4   /* caller's workspace is too small */

typedef struct ngcf_csr ngcf_csr_t;

/* ---- library ------------------------------------------------------------------------- */
const char *ngcf_last_error(void);
/* "gfx950" - the only architecture the code objects are built for. */
const char *ngcf_target_arch(void);
/* ABI version of this header.  ngcf_version() returns the value the library was built with; the Python mirror refuses to bind
 * a library whose version differs (a stale .so would otherwise receive shifted arguments). */
#define NGCF_ABI_VERSION 11
int ngcf_version(void);

/* Tunables of the kernel dispatch (thresholds, switches).  The library reads its NGCF_* environment variables ONCE, in
 * ngcf_options_from_env() on first use (no launch path touches the environment); call it again to re-read them, or set single
 * options by name (the variable's name without the NGCF_ prefix, lower case: "dense_resident", "swept_lead", ...; the table
 * is NgcfOptions in csrc/common.h).  Unknown names are an error.  Not thread-safe against concurrent launches. */
int ngcf_options_from_env(void);
int ngcf_set_option(const char *name, int64_t value);

/* Timing of the dominant kernel for bench.py's roofline line: while enabled, every SpMM kernel launch is
 * bracketed by a hipEvent pair on its own stream.  ngcf_prof_collect waits for them and returns the number
 * of timed launches and their summed duration (ms), then resets the recorder.  Not thread-safe. */
int ngcf_prof_enable(int on);
int ngcf_prof_collect(int64_t *n_launches, double *total_ms);

/* ---- Laplacian: COO (the layout of `lap_list[k]`, matrix.py:79-83) -> CSR -------------- */
/*
 * Replaces the per-call `self.lap_list[year_idx].to(device)` + COO SpMM set-up (NGCF.py:118,130):
 * built once per year slice.  `rows/cols` are int64[nnz] (the two rows of `_indices()`), `vals`
 * fp32[nnz] (`_values()`), all on the device.  Entries need not be coalesced; duplicates are kept
 * as separate entries, like the reference's CPU `torch.mm` which FMAs each stored entry.
 * Row-sorted input (what matrix.py emits) is converted on the device; anything else is stably
 * sorted by row on the host.  `n_rows` x `n_cols` is the shape of this slab: a full Laplacian has
 * n_rows == n_cols == N; a row slab of a row-partitioned graph has n_rows < n_cols and row ids
 * relative to the slab.  Columns are stored as int32 (n_cols < 2^31).
 * Fails with NGCF_ERR_INDEX when a row/col id is out of range.
 */
int ngcf_csr_from_coo(const int64_t *rows, const int64_t *cols, const float *vals, int64_t nnz,
                      int64_t n_rows, int64_t n_cols, ngcf_csr_t **out, void *stream);
/* Adopt device CSR arrays (rowptr int64[n_rows+1], colidx int32[nnz], vals fp32[nnz]); they are
 * borrowed and must outlive the handle. */
int ngcf_csr_from_arrays(const int64_t *rowptr, const int32_t *colidx, const float *vals,
                         int64_t n_rows, int64_t n_cols, int64_t nnz, ngcf_csr_t **out, void *stream);
/* Re-plan the row segmentation: rows with more than `seg_len` stored entries are cut into
 * segments of `seg_len` entries whose partial sums are combined in a fixed order (no atomics).
 * The constructors plan with a default that grows with the matrix: the power of two in [64, 2048]
 * that gives about 4 096 segments or more (2048 from 4 M stored entries up). */
int ngcf_csr_plan(ngcf_csr_t *csr, int32_t seg_len, void *stream);
/* SpMM kernel choice.  0 = row-wise gather kernels, d-sliced on the row groups whose gathered table is small
 * (default: right for matrices that live for one product, e.g. the per-layer node-dropout matrices); 1 = row-wise
 * kernels without d-slicing; 2 = L2-swept kernel (csrc/spmm_swept.hip) on every row group whose shape allows it
 * (tests); 3 = L2-swept kernel on the row groups where its host-side plan expects enough L2 re-use to pay, the
 * row-wise kernels on the rest - meant for long-lived matrices (the Laplacians of `lap_list`): building the plan
 * costs a host pass over the entries and as much device memory again as the CSR.  Calls whose width is not a
 * multiple of 64, that use edge dropout, or whose table spans more than 4 GiB use the row-wise kernels anyway.
 * A CSR with swept parts keeps a block of sweep counters per launching stream (up to four): products of the same CSR may run
 * concurrently on different streams (beyond four streams the extra ones share a block: results stay correct - the counters
 * only pace the sweep - but those products lose L2 re-use).  The stream registry is not thread-safe: launch a given CSR from one
 * host thread. */
int ngcf_csr_set_mode(ngcf_csr_t *csr, int mode, void *stream);
/*
 * Thinned copy of a CSR, made on the device: *dst keeps, in src's order, every stored entry e of `src` with
 * keep[map ? map[e] : e] != 0 (`keep`: device uint8, one flag per entry of the matrix the flags were drawn for; `map`: device
 * int32[src nnz] or NULL = identity).  This is the reference's per-layer `sparse_dropout` (NGCF.py:93-100,124-126: a COO tensor
 * rebuilt from `indices[:, mask]`, values not rescaled) as one stream compaction: no host round trip, no synchronisation, and
 * no allocation after the first call - pass the previous step's object back in *dst and its buffers are re-used (*dst == NULL:
 * a new object, sized for all of src's entries).  `nnz_kept`: the number of set flags if the caller knows it (it drew the
 * mask), else -1: ngcf_csr_nnz(*dst) is then an upper bound.  The copy runs on the row-wise kernels (mode 0) with src's
 * segment structure and row groups and BORROWS them: `src` must outlive `*dst`.
 * ngcf_csr_filter_pos(dst): device int32[src nnz + 1], pos[e] = kept entries before e (the new position of a kept entry).
 */
int ngcf_csr_filter(const ngcf_csr_t *src, const uint8_t *keep, const int32_t *map, int64_t nnz_kept, ngcf_csr_t **dst,
                    void *stream);
const int32_t *ngcf_csr_filter_pos(const ngcf_csr_t *dst);
/*
 * Entry map of a thinned transpose.  L^T is thinned with the flags drawn for L through map[j] = position in L of entry j of
 * L^T; after both were filtered, the next layer needs the same map between the two thinned matrices:
 * map_out[pos_t[j]] = pos_l[map[j]] for every kept j, with pos_t = ngcf_csr_filter_pos(dst_t), pos_l = that of the thinned L.
 * n_src_entries: entries of the transpose that was filtered into dst_t.
 */
int ngcf_csr_filter_remap(const ngcf_csr_t *dst_t, const uint8_t *keep, const int32_t *map, int64_t n_src_entries,
                          const int32_t *pos_l, int32_t *map_out, void *stream);
void ngcf_csr_free(ngcf_csr_t *csr);
int64_t ngcf_csr_nnz(const ngcf_csr_t *csr);
int64_t ngcf_csr_n_rows(const ngcf_csr_t *csr);
int64_t ngcf_csr_n_cols(const ngcf_csr_t *csr);
int64_t ngcf_csr_n_segments(const ngcf_csr_t *csr);
int64_t ngcf_csr_max_row_len(const ngcf_csr_t *csr);        /* stored entries of the longest row */
/* rows currently covered by L2-swept parts (0: every product of this CSR runs on the row-wise kernels: mode 0/1, a shape the
 * plan declines - too small, expected re-use below 3, table beyond 32-bit offsets - or a device that does not report 256 CUs,
 * for which one note is printed on stderr) */
int64_t ngcf_csr_swept_rows(const ngcf_csr_t *csr);
/* the row groups of the current plan (for tests and tools; read-only): group g covers rows [begin, end); `sliceable`: its rows
 * gather from a table slice small enough for the d-sliced kernel; `lds_table`: from at most 512 table rows (table-in-LDS
 * kernel); [col_lo, col_hi]: the columns its rows gather from (col_hi < col_lo: no entries).  Any out pointer may be NULL.
 * A thinned copy reports its source's groups. */
int64_t ngcf_csr_n_groups(const ngcf_csr_t *csr);
int ngcf_csr_group(const ngcf_csr_t *csr, int64_t g, int64_t *begin, int64_t *end, int *sliceable, int *lds_table,
                   int32_t *col_lo, int32_t *col_hi);
/* device pointers of the CSR arrays (for tests / the transposed view) */
const int64_t *ngcf_csr_rowptr(const ngcf_csr_t *csr);
const int32_t *ngcf_csr_colidx(const ngcf_csr_t *csr);
const float *ngcf_csr_vals(const ngcf_csr_t *csr);

/* ---- propagation ----------------------------------------------------------------------- */
/* Bytes of workspace ngcf_spmm_csr_f32 / ngcf_layer_fused_f32 need for this CSR at width d_in
 * (segment partial sums; for the fused layer also the L.E tile and the packed weights). */
int64_t ngcf_spmm_workspace_bytes(const ngcf_csr_t *csr, int d);
int64_t ngcf_layer_workspace_bytes(const ngcf_csr_t *csr, int d_in, int d_out);

/*
 * LE = L.E  (NGCF.py:130, `torch.mm(L, E)`).
 * E: [n_cols, d] with leading dimension ldE; LE: [n_rows, d] with ldLE.  fp32 FMA accumulation;
 * the summation order inside a row differs from the reference's sequential order (tolerance in
 * tests/test_parity_gpu.py).
 */
int ngcf_spmm_csr_f32(const ngcf_csr_t *csr, const float *E, int64_t ldE, int d, float *LE,
                      int64_t ldLE, void *workspace, int64_t workspace_bytes, void *stream);

/* Width to run a product at when LE has padded rows (leading dimension a multiple of 4 >= d rounded up): a width that is not
 * a multiple of 4 on a small (launch-bound) matrix is multiplied up to the next multiple of 4 when the gathered rows are
 * 16-byte aligned and padded - the extra columns land in the padding of LE.  ngcf_layer_fused_f32 applies this rule itself;
 * callers that run the SpMM on its own (the training path) ask here so that both paths produce the same bits. */
int ngcf_spmm_product_width(const ngcf_csr_t *csr, const float *E, int64_t ldE, int d);

/*
 * LE = drop(L).E with node dropout on the device (NGCF.py:93-100,124-126 semantics: every stored entry is kept
 * with probability 1-p, values are NOT rescaled, and the thinning is cumulative over layers): the entry (i, j) of L
 * survives iff hash(seeds[q], i, j) passes for every q < n_seeds (layer k passes its own and all earlier layers' seeds,
 * n_seeds <= 4, host array).  No CSR is rebuilt.  The hash is keyed by the entry's row and column in L, so any layout of
 * L is thinned the same way: pass `transposed` != 0 when `csr` holds L^T (the backward pass), and L^T loses exactly the
 * entries L lost.  (Entries stored twice at the same (i, j) share their fate.)  The mask is a counter-based hash, not
 * torch's generator: same distribution as the reference, different stream.
 * The threshold: `drop_p` is taken as a FLOAT (a caller's double is rounded to float first: 0.3 arrives as 0.300000011920929),
 * and an entry is kept iff every one of its 32-bit hashes is >= (uint32_t)((double)drop_p * 2^32) - for 0.3 that is
 * 1288490240, not the 1288490188 of the double 0.3.  A host mask must use the same number (tests/dropout_oracle.py).
 */
int ngcf_spmm_csr_dropout_f32(const ngcf_csr_t *csr, const float *E, int64_t ldE, int d, float *LE, int64_t ldLE,
                              float drop_p, const uint64_t *seeds, int n_seeds, int transposed,
                              void *workspace, int64_t workspace_bytes, void *stream);

/*
 * One whole propagation layer (NGCF.py:130-146) for the rows of `csr`:
 *   LE    = L.E_gather                                              NGCF.py:130
 *   M     = (LE+E_self).W1^T + (LE*E_self).W2^T + (2*b1 + b2)       NGCF.py:131-138 (b1 twice)
 *   carry = dropout_p(leaky_relu(M, slope))                         NGCF.py:140-142
 *   norm  = carry / max(||carry||_2, 1e-12)                         NGCF.py:144
 * E_gather: [n_cols, d_in] table the neighbours are read from; E_self: [n_rows, d_in], the same
 * rows as the output (E_gather + row_start*ld for a row slab).  W1, W2: [d_out, d_in] row-major
 * (nn.Linear.weight), b1, b2: [d_out].  `carry` ([n_rows, d_out], may be NULL for the last
 * layer) feeds the next layer; `norm` is written straight into its column block of all_E
 * (pointer already offset by the block's first column, leading dimension ldn = ld of all_E),
 * which removes the reference's `torch.cat` (NGCF.py:147).  drop_p == 0 -> no dropout (eval).
 * Message dropout (NGCF.py:142), two forms: `drop_mask` != NULL ([n_rows, d_out], leading dimension ld_mask) is the
 * noise tensor nn.Dropout multiplies by (0 or 1/(1-p)), drawn by the caller - the mirror draws it from torch's CPU
 * generator exactly where the reference does, so the zero pattern is bit-identical ("reference" mode); drop_mask == NULL
 * and drop_p > 0: keep mask = counter-based hash of (drop_seed, row, column) evaluated in the epilogue ("device" mode).
 * One call, two phases on the stream: the SpMM writes LE [n_rows, d_in] into the workspace and the dense phase (everything from
 * the nn.Linear contractions to both outputs in one kernel) reads it back; what is fused is the dense half and its epilogue, not
 * the SpMM into it (DESIGN.md 4.2 says why).
 */
int ngcf_layer_fused_f32(const ngcf_csr_t *csr, const float *E_gather, int64_t ldEg,
                         const float *E_self, int64_t ldEs, int d_in,
                         const float *W1, const float *b1, const float *W2, const float *b2, int d_out,
                         float leaky_slope, float drop_p, uint64_t drop_seed,
                         const float *drop_mask, int64_t ld_mask,
                         float *carry, int64_t ldc, float *norm, int64_t ldn,
                         void *workspace, int64_t workspace_bytes, void *stream);

/* The dense half alone (NGCF.py:131-146) on an already computed LE; same arguments as above.
 * Needs ngcf_dense_workspace_bytes(d_in, d_out) bytes of workspace (packed weights). */
int64_t ngcf_dense_workspace_bytes(int d_in, int d_out);
int ngcf_layer_dense_f32(const float *LE, int64_t ldLE, const float *E_self, int64_t ldEs,
                         int64_t n_rows, int d_in,
                         const float *W1, const float *b1, const float *W2, const float *b2, int d_out,
                         float leaky_slope, float drop_p, uint64_t drop_seed,
                         const float *drop_mask, int64_t ld_mask,
                         float *carry, int64_t ldc, float *norm, int64_t ldn,
                         void *workspace, int64_t workspace_bytes, void *stream);
/* Which forward kernel ngcf_layer_dense_f32 would launch for these sizes and operands under the current options: a read-only
 * query answered by the host function the entry point itself dispatches through (nothing is launched, LE / E_self are not
 * dereferenced - only their alignment counts).  A short static name: "staged<RW,CW,NT>/padded", ".../aligned" or ".../unaligned"
 * (the tile configuration of layer_dense_kernel and its row layout: 16-byte aligned rows padded to a multiple of 4 floats,
 * aligned rows of fewer than 4 columns, anything else), "direct<2,4>", "direct<4,4>", "tall256", "tall512", "resident" or
 * "split".  NULL (and ngcf_last_error) for sizes ngcf_layer_dense_f32 rejects.  For tests and tools. */
const char *ngcf_dense_path(int64_t n_rows, int d_in, int d_out, const float *LE, int64_t ldLE, const float *E_self, int64_t ldEs);

/* dst[r, 0:d] = src[r, 0:d] for r < n_rows (strided copy; writes E0 into its block of all_E,
 * NGCF.py:120-121 + 147). */
int ngcf_copy_rows_f32(const float *src, int64_t lds, float *dst, int64_t ldd, int64_t n_rows, int d,
                       void *stream);
/* The same with two destinations (the source rows are read once): E0 goes to its block of all_E and, when the rows of
 * all_E are not 16-byte aligned (embed_size 65 / 130 / 515, NGCF.py:39-43), to the aligned copy the first layer gathers from. */
int ngcf_copy_rows2_f32(const float *src, int64_t lds, float *dst, int64_t ldd, float *dst2, int64_t ldd2,
                        int64_t n_rows, int d, void *stream);

/* dst[idx[b], 0:d] = src[idx[b], 0:d] for b < n_idx, ids outside [0, n_rows) skipped (r04): block 0 of a retained all_E follows
 * the rows the feature injection rewrote (NGCF.py:114-115) without the whole table being copied again.  idx: int64, device. */
int ngcf_copy_rows_indexed_f32(const float *src, int64_t lds, float *dst, int64_t ldd, const int64_t *idx, int64_t n_idx,
                               int64_t n_rows, int d, void *stream);

/* HOST routine (r04): n draws of torch's CPU `bernoulli_(keep)` - what `nn.Dropout` draws on a CPU tensor, NGCF.py:93-100,142 -
 * from the generator whose state bytes (`torch.get_rng_state()`, >= 5016 bytes, legacy mt19937 layout) are `rng_state`; the bytes
 * are advanced in place exactly as torch advances its generator (two 32-bit outputs per element).  flags[i] (uint8, may be NULL) =
 * kept, noise[i] (float, may be NULL) = kept ? scale : 0, *n_kept = count.  Host pointers.  Bit-identical to torch's own serial
 * kernel (checked against it by the caller once per process), several times faster (vector loops, no lock per element). */
int ngcf_torch_cpu_bernoulli(uint8_t *rng_state, int64_t state_bytes, int64_t n, double keep, uint8_t *flags, float *noise,
                             float scale, int64_t *n_kept);

/* The draws of a whole forward in ONE call (r04; a helper thread draws the next forward's masks ahead and must not need the
 * interpreter between two draws): draw i is ngcf_torch_cpu_bernoulli(n[i], keep[i], flags[i], noise[i], scale[i]) -> n_kept[i], one
 * after the other on the same state bytes; n[i] = -1 stands for "as many as the latest earlier draw WITH flags kept" (the node
 * mask of a layer has one flag per entry the earlier layers kept, NGCF.py:126: its buffer must hold the first such draw's n). */
int ngcf_torch_cpu_bernoulli_seq(uint8_t *rng_state, int64_t state_bytes, int n_draws, const int64_t *n, const double *keep,
                                 uint8_t *const *flags, float *const *noise, const float *scale, int64_t *n_kept);

/* ---- feature injection (NGCF.py:103-115) ---------------------------------------------- */
/*
 * user_w[u_id[b], :] = user_w[u_id[b], :]*(1-r) + cat(age,sex,month,day,dow rows)[b, :]*r.
 * tables[5]: device pointers of the five [card, fw] tables in the concat order age, sex, month,
 * day, dow (NGCF.py:110); idx[5]: the five int64[B] index vectors in the same order; cards[5] their
 * cardinalities (host).  5*fw must equal d0 (the reference raises RuntimeError otherwise).
 * Duplicate u_id: the LAST occurrence in the batch wins (what the CPU index_put_ of the reference
 * does).  `scratch` is int32[n_user], all -1 on entry and on exit.
 * `status` is a device int32: set non-zero when an index is out of range (rows skipped).
 */
int ngcf_feature_inject_f32(float *user_w, int64_t ldu, int64_t n_user, int d0,
                            const float *const *tables, const int64_t *const *idx, const int64_t *cards,
                            int fw, const int64_t *u_id, int64_t B, double emb_ratio,
                            int32_t *scratch, int32_t *status, void *stream);

/* ---- dropout seeds on the device ---------------------------------------------------------- */
/* Every 64-bit dropout seed of this interface (drop_seed of the layer entry points, the `seeds` of the node-dropout products) is
 * either a value below 2^62 or a TAGGED DEVICE ADDRESS: top 16 bits 0xD5ED, low 48 bits the address of a uint64_t that holds the
 * value - read by the kernels when they run.  A captured hipGraph bakes kernel arguments in; with its seeds behind addresses every
 * replay still draws new masks.  ngcf_seeds_advance steps n such words to their next values (a splitmix64 chain, results below
 * 2^62), asynchronously on `stream`. */
#define NGCF_SEED_PTR_TAG 0xD5EDull
int ngcf_seeds_advance(uint64_t *seeds_device, int n, void *stream);

/* ---- gathers (NGCF.py:151-155) ---------------------------------------------------------- */
/* out[b, 0:d] = table[(row_off + idx[b]), 0:d], bit-exact copies.  idx must lie in [0, n_idx_rows);
 * offenders are skipped and *status (device int32) is set non-zero. */
int ngcf_gather_rows_f32(const float *table, int64_t ld, int d, const int64_t *idx, int64_t B,
                         int64_t row_off, int64_t n_idx_rows, float *out, int64_t ldo,
                         int32_t *status, void *stream);

/* The three gathers of NGCF.forward (NGCF.py:151-155: users, positive items, negative items) from one table in ONE launch:
 * out_k[b, 0:d] = table[(row_off_k + idx_k[b]), 0:d] for k = 0, 1, 2; a set with B_k == 0 is skipped (no negative items:
 * NGCF.py:153).  Same bounds rule and status word as ngcf_gather_rows_f32; the three outputs share the leading dimension. */
int ngcf_gather_rows3_f32(const float *table, int64_t ld, int d,
                          const int64_t *idx0, int64_t B0, int64_t row_off0, int64_t n_idx_rows0, float *out0,
                          const int64_t *idx1, int64_t B1, int64_t row_off1, int64_t n_idx_rows1, float *out1,
                          const int64_t *idx2, int64_t B2, int64_t row_off2, int64_t n_idx_rows2, float *out2,
                          int64_t ldo, int32_t *status, void *stream);

/* ---- BPR (bprloss.py:15-22) ------------------------------------------------------------- */
/*
 * loss = (-sum_r logsigmoid(|u_r.p_r| - |u_r.n_r|) + wd*(sum|u|^2 + sum|p|^2 + sum|n|^2)) / batch_size
 * u: [Bu, D], p: [Bp, D], n: [Bn, D] contiguous; each row count is 1 (broadcast) or R = max.
 * The squared norms run over each tensor's own rows.  `loss` is one device float.
 * workspace: ngcf_bpr_workspace_bytes(R) bytes.  Deterministic (fixed-order two-stage reduction).
 */
int64_t ngcf_bpr_workspace_bytes(int64_t R);
int ngcf_bpr_fused_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn,
                       int D, float weight_decay, float batch_size, float *loss,
                       void *workspace, int64_t workspace_bytes, void *stream);

/* ---- BPR, m negatives per positive (csrc/bpr_multi.hip) -------------------------------------- */
/*
 * The loss of a batch whose every positive row is scored against m negatives, without expanding the batch to B*m triplets.
 * u: [B, D], p: [B, D], n: [B*m, D], fp32 and contiguous; rows b*m .. b*m + m - 1 of n are the negatives of row b.  Nothing
 * broadcasts: Bu == Bp == B >= 1, Bn == B*m, 1 <= m <= NGCF_BPR_MULTI_M_MAX, D >= 1; anything else is NGCF_ERR_ARG before any
 * launch.  Per row, with the reference's abs around both scores (bprloss.py:18):
 *   sp = |u_b.p_b|,  sn_j = |u_b.n_bj|
 *   reduction NGCF_BPR_MULTI_MEAN     l_b = -(1/m) sum_j logsigmoid(sp - sn_j)
 *   reduction NGCF_BPR_MULTI_SOFTMAX  l_b = -logsigmoid(sp - lse_b),  lse_b = M + log(sum_j exp(sn_j - M)),  M = max_j sn_j
 *                                     (= -log(e^sp / (e^sp + sum_j e^sn_j)), finite for scores of several hundred)
 *   loss = (sum_b l_b + wd*(sum|u|^2 + sum|p|^2 + (1/m) sum|n|^2)) / batch_size
 * Two identities fix the choices.  (a) With m = 1, MEAN is ngcf_bpr_fused_f32 / ngcf_bpr_backward_f32 bit for bit, loss and all
 * three gradients: the dot products are fmaf over the lanes' columns (stride 64) and a wave sum, a row's term is
 * -logsigmoid(|u.p| - |u.n|), four rows make a workgroup partial (sh[0]+sh[2])+(sh[4]+sh[6]) and the second stage is the same code.
 * (b) MEAN at any m is, mathematically, ngcf_bpr_fused_f32 over the B*m expanded triplets (u and p rows repeated m times) with
 * batch_size*m; only the order of the sums differs.
 * Gradients, times *grad_out / batch_size, with sgn(0) = 0 like torch.abs:
 *   a_j = dl_b/dsn_j   MEAN     (1/m) / (1 + exp(sp - sn_j))
 *                      SOFTMAX  exp(sn_j - M') / (exp(sp - M') + sum_k exp(sn_k - M')),  M' = max(sp, M)
 *   A   = sum_j a_j
 *   du_b  = 2 wd u_b + sum_j a_j (sgn_nj n_bj - sgn_p p_b)      (four chains like ngcf_segment_sum_rows_f32: chain q takes the
 *                                                               negatives j = q mod 4 ascending, one fma each, chain 0 starts from
 *                                                               the weight-decay term; combined (c0 + c1) + (c2 + c3))
 *   dp_b  = -A sgn_p u_b + 2 wd p_b
 *   dn_bj = a_j sgn_nj u_b + (2 wd / m) n_bj
 * One wave per positive row, four per workgroup; lane j keeps sn_j and a_j (hence m <= 64); the backward recomputes the scores.
 * No atomics and no host synchronisation: results are identical from run to run and both calls can be captured in a hipGraph.
 * `loss` is one device float; workspace: ngcf_bpr_multi_workspace_bytes(B) bytes (NGCF_ERR_WORKSPACE when shorter).
 */
#define NGCF_BPR_MULTI_M_MAX 64
#define NGCF_BPR_MULTI_MEAN 0
#define NGCF_BPR_MULTI_SOFTMAX 1
int64_t ngcf_bpr_multi_workspace_bytes(int64_t B);
int ngcf_bpr_multi_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn, int m, int D,
                       int reduction, float weight_decay, float batch_size, float *loss, void *workspace,
                       int64_t workspace_bytes, void *stream);
int ngcf_bpr_multi_backward_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn, int m, int D,
                                int reduction, float weight_decay, float batch_size, const float *grad_out, float *du,
                                float *dp, float *dn, void *stream);

/* ---- Sampled softmax with logQ correction (csrc/sampled_softmax.hip) --------------------------- */
/*
 * The softmax of a positive among its m sampled negatives, every score corrected by the log of the probability with which its item
 * was proposed, at a temperature.  Operands as in ngcf_bpr_multi_f32: u: [B, D], p: [B, D], n: [B*m, D], fp32 and contiguous, rows
 * b*m .. b*m + m - 1 of n the negatives of row b; logq: fp32 [B*m], logq[b*m + j - 1] belongs to negative j = 1..m of row b;
 * pos_logq: fp32 [B] or NULL (then c_b is exactly 0).  Nothing broadcasts: Bu == Bp == B >= 1, Bn == B*m,
 * 1 <= m <= NGCF_SAMPLED_SOFTMAX_M_MAX, D >= 1, inv_tau > 0 and finite; anything else is NGCF_ERR_ARG before any launch.  Scores
 * are plain (no abs, as in the full-catalogue softmax below).  logq and pos_logq are data: they get no gradient, and non-finite
 * values in them are undefined and not checked.
 *   z_0 = (u_b.p_b) * inv_tau - c_b          z_j = (u_b.n_bj) * inv_tau - logq[b*m + j - 1]
 *   l_b = logsumexp(z_0, .., z_m) - z_0
 *   loss = (sum_b l_b + wd*(sum|u|^2 + sum|p|^2 + (1/m) sum|n|^2)) / batch_size            (regulariser and divisor: ngcf_bpr_multi_f32's)
 * The recipe, operation by operation where it decides bits (fp32, no contraction but the fmaf named):
 *   dots     u.p, u.n_j, |u|^2, |p|^2, |n_j|^2 are those of ngcf_bpr_multi_f32: fmaf over a lane's columns (stride 64, ascending),
 *            then the xor butterfly 32, 16, .., 1 over the wave; sum_j |n_j|^2 with j ascending.
 *   z        one multiply and one subtract each, rounded twice (no fma).
 *   forward  M = max_{j>=1} z_j;  lse = M + logf(sum_{j>=1} expf(z_j - M))  (butterfly sums; over the negatives only);
 *            l_b = -logsigmoid(z_0 - lse),  logsigmoid(x) = fminf(x, 0) - log1pf(expf(-|x|)).  Four rows make a workgroup partial
 *            (r0 + r1) + (r2 + r3), the second stage is the BPR losses' (thread t adds the partials t, t + 256, ..).
 *   backward M' = max(z_0, M);  den = expf(z_0 - M') + sum_{j>=1} expf(z_j - M');  s_j = -(expf(z_j - M') / den) * inv_tau;
 *            S = sum_j s_j (butterfly);  with g = *grad_out / batch_size:
 *            dp_b  = g * fmaf(S, u_b, 2 wd p_b)
 *            dn_bj = g * fmaf(-s_j, u_b, (2 wd / m) n_bj)
 *            du_b  = g * ((c0 + c1) + (c2 + c3)): chain q takes the negatives j = q mod 4 in ascending order, one
 *                    fmaf(s_j, p_b - n_bj, chain) each, chain 0 starts from 2 wd u_b (the four chains of ngcf_bpr_multi_backward_f32).
 *            That is dl_b/d(u.n_j) = a_j inv_tau and dl_b/d(u.p) = -A inv_tau with a_j = exp(z_j) / sum_{k>=0} exp(z_k), A = sum_j a_j.
 *            The scores are recomputed; nothing of the forward is kept.
 * The identity that fixes the recipe: with inv_tau = 1, logq all zero, pos_logq NULL and inputs whose dot products are all positive,
 * the loss and the three gradients are those of ngcf_bpr_multi_f32 / ngcf_bpr_multi_backward_f32 under NGCF_BPR_MULTI_SOFTMAX bit
 * for bit (x * 1 - 0 is x, and the sign factors there are exactly 1).
 * What logq is: the LOG OF THE PROPOSAL PROBABILITY OF THE SLOT AS THE SAMPLER DREW IT - for ngcf_sample_weighted's successive
 * sampling the conditional probability log(w_j / U_j) given the slots before it, not the marginal probability that the item is
 * among the m.  No unbiasedness of the resulting estimator of the full softmax is claimed.  Adding one constant to a row's logq and
 * pos_logq changes nothing mathematically.
 * One wave per positive row, four per workgroup; lane j keeps z_j, its logq value (loaded once, coalesced across the wave) and s_j,
 * hence m <= 64.  No atomics and no host synchronisation: results are identical from run to run and both calls can be captured.
 * `loss` is one device float; workspace: ngcf_sampled_softmax_workspace_bytes(B) bytes (NGCF_ERR_WORKSPACE when shorter; -1 for B < 0).
 */
#define NGCF_SAMPLED_SOFTMAX_M_MAX 64
int64_t ngcf_sampled_softmax_workspace_bytes(int64_t B);
int ngcf_sampled_softmax_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn, int m, int D,
                             const float *logq, const float *pos_logq, float inv_tau, float weight_decay, float batch_size,
                             float *loss, void *workspace, int64_t workspace_bytes, void *stream);
int ngcf_sampled_softmax_backward_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn, int m,
                                      int D, const float *logq, const float *pos_logq, float inv_tau, float weight_decay,
                                      float batch_size, const float *grad_out, float *du, float *dp, float *dn, void *stream);

/* ---- Full-catalogue softmax (csrc/softmax_full.hip) ------------------------------------------- */
/*
 * The softmax loss over the whole catalogue, the limit of the sampled losses above, without a [B, n_items] matrix in memory:
 *   s_bj = <u_b, i_j> * inv_tau          L_b = lse_j s_bj - s_b,pos_b
 *   loss = (sum_b L_b + wd * (sum_b |u_b|^2 + sum_b |i_pos_b|^2)) / batch_size
 * users: [B, D] fp32 rows, leading dimension ldu; items: [n_items, D] fp32 rows, leading dimension ldi (a row block of all_E);
 * pos: [B] int64 item ids.  Scores are plain (no abs: rank_topk ranks by the plain score; the abs is the reference's BPR's).
 * An id outside [0, n_items) is never used as an index: the row has no positive term (s_b,pos = 0, no |i_pos|^2, no -1 in the
 * gradient) and bit 0 of *status (device int32) is set with an integer atomic.  1 <= B, n_items < 2^31, D >= 1, inv_tau > 0 and
 * finite, batch_size > 0; anything else is NGCF_ERR_ARG before any launch.
 *
 * The recipe, operation by operation where it decides bits (fp32 unless fp64 is said; no contraction but the fmaf named):
 *   score    the fp32 score of ngcf_rank_topk_f32: ONE chain acc = fmaf(u_bk, i_jk, acc), k ascending from acc = 0 (the MFMA step
 *            order of rank.hip, K zero-padded to a multiple of 32); s_bj = acc * inv_tau, rounded once.  With inv_tau = 1, spos[b]
 *            has the bits rank_topk returns for (b, pos_b).
 *   forward  a workgroup owns 64 users and one item piece (rank_item_split of the 64-user tiles: whole tiles of 128 items) and
 *            walks the piece in tiles of 128 items.  A lane holds one user and 16 items of a tile: wave w (0..3), lane half h,
 *            register e -> item 32 w + (e & 3) + 8 (e >> 2) + 4 h of the tile.  Per lane a running pair (m, l), from (-inf, 0):
 *              tm = max over the lane's valid scores of the tile (fmaxf, e ascending);  M = fmaxf(m, tm);  Ms = M, or 0 if M = -inf
 *              l = l * expf(m - Ms);  then for e ascending: l = l + expf(s_e - Ms);  m = M
 *            The positive's score is the s_e of the lane that holds item pos_b when its tile passes: spos[b] <= m in the bits.
 *   merge    (m, l) <- (ma, la) + (mb, lb):  M = fmaxf(ma, mb);  Ms = M or 0 as above;  l = la * expf(ma - Ms) + lb * expf(mb - Ms).
 *            The eight holders of a user merge as a left fold in the order h' = 2 w + h = 0..7; the item pieces as a left fold in
 *            ascending piece order; then lse_b = m + logf(l).
 *   sums     L_b = (double)lse_b - (double)spos_b;  |u_b|^2 and |i_pos_b|^2 in fp64: lane t of the row's wave adds the exact fp64
 *            squares of columns t, t + 64, .. ascending, the lanes combine by the xor butterfly 32, 16, .., 1, the two norms add.
 *            Four rows a workgroup: (r0 + r1) + (r2 + r3) in fp64, for the L's and for the norms.  Last stage, one workgroup of
 *            256: thread t adds the workgroups t, t + 256, .. ascending, thread 0 adds the 256 results ascending;
 *            loss = (float)((sumL + (double)wd * sumsq) / (double)batch_size).
 *   A maximum of -inf, an infinite score or a NaN faults nothing: a NaN input gives a NaN loss (fmaxf drops the NaN, expf keeps it).
 *
 * Gradients, times *grad_out (one device float):
 *   c    = grad_out / batch_size * inv_tau            (in that order)
 *   g_bj = c * (expf(s_bj - lse_b) - [j == pos_b])     s_bj recomputed by the recipe above
 *   dU_b = sum_j g_bj i_j + (2 wd * (grad_out / batch_size)) u_b
 *   dI_j = sum_b g_bj u_b + (2 wd * (grad_out / batch_size) * c_j) i_j,   c_j = the batch rows whose positive is j, counted in integers
 * One kernel with the roles swapped: a workgroup owns 32 output rows and a slab of <= 512 output columns and walks the other side in
 * tiles of 128 rows; each output element is ONE chain acc = fmaf(g, w, acc) over the walked rows in ascending order from 0
 * (v_mfma_f32_32x32x2_f32), the weight-decay term joins last as fmaf(coefficient, x, acc).  A width above 512 takes ceil(D / 512)
 * slabs, each of which recomputes the scores over the full D: at D = 1 539 the score work is done four times.  When the output
 * tiles are few the walked side is cut by rank_item_split into pieces; each piece writes a partial [rows, D] block (for dI with its own
 * share of c_j, for dU the weight-decay term in piece 0) and one pass adds the pieces in ascending order; one piece stores directly.
 * du / ditems may be NULL (not both): that gradient is not computed.  Nothing of size B x n_items is in memory; no float atomics;
 * loss, lse, spos, dU and dI are bit-identical from run to run; no host synchronisation, so both calls can be captured.
 *
 * ngcf_softmax_full_plan (host only): out = {forward pieces, 1, dU pieces, dU column slabs, dI pieces, dI column slabs}.
 * Workspace for both calls: ngcf_softmax_full_workspace_bytes(B, n_items, D) = the (max, sum) partials (2 x pieces x B floats), the
 * loss partials and, where a gradient is cut, pieces x rows x D floats (NGCF_ERR_WORKSPACE when shorter; -1 for a bad shape).
 */
int ngcf_softmax_full_plan(int64_t B, int64_t n_items, int D, int64_t out[6]);
int64_t ngcf_softmax_full_workspace_bytes(int64_t B, int64_t n_items, int D);
int ngcf_softmax_full_f32(const float *users, int64_t ldu, int64_t B, const float *items, int64_t ldi, int64_t n_items, int D,
                          const int64_t *pos, float inv_tau, float weight_decay, float batch_size, float *loss, float *lse,
                          float *spos, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);
int ngcf_softmax_full_backward_f32(const float *users, int64_t ldu, int64_t B, const float *items, int64_t ldi, int64_t n_items,
                                   int D, const int64_t *pos, const float *lse, float inv_tau, float weight_decay,
                                   float batch_size, const float *grad_out, float *du, int64_t lddu, float *ditems, int64_t lddi,
                                   void *workspace, int64_t workspace_bytes, void *stream);

/* ---- In-batch softmax (csrc/inbatch_softmax.hip) ----------------------------------------------- */
/*
 * The softmax loss with SHARED negatives: every row's positive is a negative of every other row, E extra rows are appended to the
 * columns; per-column logQ corrections and a mask of false negatives; without a [B, B + E] matrix in memory.
 *   u: [B, D] fp32 rows (ldu), p: [B, D] the positives' rows (ldp), x: [E, D] extra rows (ldx; NULL when E = 0)
 *   columns c_j = p_j (j < B), x_(j-B) (B <= j < C = B + E);  ids cid_j = ids[j] / xids[j - B] (int64);  q_j = logq[j] / xlogq[j - B]
 *   ids, xids, logq, xlogq, pos_logq may be NULL: no mask / a correction of exactly 0
 *   s_bj = <u_b, c_j> * inv_tau                       plain score, as in the full-catalogue section
 *   z_bb = s_bb - pos_logq[b]         z_bj = s_bj - q_j  (j != b)          one fp32 subtraction, rounded once
 *   masked(b, j) = ids given and j != b and cid_j == ids[b]                 out of the softmax, zero gradient; never the diagonal
 *   L_b  = lse over unmasked j of z_bj  -  z_bb
 *   loss = (sum_b L_b + wd * (sum_b |u_b|^2 + sum_b |p_b|^2)) / batch_size    the extras are not regularised
 * Ids are only compared, never an index: no range check and no status word.  B >= 1, E >= 0, C < 2^31, D >= 1, inv_tau > 0 and
 * finite, batch_size > 0, xids given whenever ids are and E > 0; anything else is NGCF_ERR_ARG before any launch.
 *
 * The recipe is the full-catalogue section's with n_items = C, operation by operation (the kernels are the same templates,
 * csrc/softmax_tile_device.h), with these differences:
 *   score    the same chain and s_bj = acc * inv_tau; then z = s - q, q as above (0.f for a NULL array).
 *   forward  a score enters the lane's (tm, l) only if unmasked; the positive's score is z_bb, picked up by the lane that holds
 *            column b (workspace, not exported).
 *   sums     L_b = (double)lse_b - (double)z_bb;  |u_b|^2 and |p_b|^2 as there.
 *   Without ids and corrections loss, lse, dU and dp over dx have the bits of ngcf_softmax_full_* on the rows p over x with
 *   pos[b] = b; all-zero corrections have the bits of NULL ones.
 *
 * Gradients, times *grad_out (one device float):  g0 = grad_out / batch_size,  c = g0 * inv_tau  (in that order)
 *   g_bj = masked ? 0 : c * (expf(z_bj - lse_b) - [j == b])          z_bj recomputed by the recipe above
 *   dU_b = sum_j g_bj c_j + (2 wd g0) u_b
 *   dC_j = sum_b g_bj u_b + [j < B] (2 wd g0) p_j          rows j < B to dp, the others to dx
 * by the role-swapped kernel of the full-catalogue section: one chain fmaf(g, w, acc) per output element over the walked rows
 * ascending, the weight-decay term last as fmaf(2 wd g0, x, acc) - for dU in piece 0, for dC in the piece that walks user j.
 * Any of du / dp / dx may be NULL (not all; dx is ignored when E = 0): that gradient is not stored, the others keep their bits.
 * No float atomics; loss, lse, dU, dp and dx are bit-identical from run to run; no host synchronisation, so both calls can be
 * captured.
 *
 * ngcf_inbatch_softmax_plan (host only): out = {forward pieces, 1, dU pieces, dU column slabs, dC pieces, dC column slabs} - that of
 * ngcf_softmax_full_plan(B, B + E, D).  Workspace for both calls: ngcf_inbatch_softmax_workspace_bytes(B, E, D) = that of the full
 * catalogue at (B, B + E, D) plus B floats (NGCF_ERR_WORKSPACE when shorter; -1 for a bad shape).
 */
int ngcf_inbatch_softmax_plan(int64_t B, int64_t E, int D, int64_t out[6]);
int64_t ngcf_inbatch_softmax_workspace_bytes(int64_t B, int64_t E, int D);
int ngcf_inbatch_softmax_f32(const float *u, int64_t ldu, int64_t B, const float *p, int64_t ldp, const float *x, int64_t ldx,
                             int64_t E, int D, const int64_t *ids, const int64_t *xids, const float *logq, const float *xlogq,
                             const float *pos_logq, float inv_tau, float weight_decay, float batch_size, float *loss, float *lse,
                             void *workspace, int64_t workspace_bytes, void *stream);
int ngcf_inbatch_softmax_backward_f32(const float *u, int64_t ldu, int64_t B, const float *p, int64_t ldp, const float *x,
                                      int64_t ldx, int64_t E, int D, const int64_t *ids, const int64_t *xids, const float *logq,
                                      const float *xlogq, const float *pos_logq, const float *lse, float inv_tau,
                                      float weight_decay, float batch_size, const float *grad_out, float *du, int64_t lddu,
                                      float *dp, int64_t lddp, float *dx, int64_t lddx, void *workspace, int64_t workspace_bytes,
                                      void *stream);

/* ---- backward pass (`loss.backward()` of experiment.py:57; driven by autograd.py) -------------- */
/* Everything `loss.backward()` runs: no library GEMM at any width.  L^T.dLE re-uses ngcf_spmm_csr_f32 on the CSR of L^T. */
/* du/dp/dn of the BPR loss (bprloss.py:15-22) times the upstream scalar *grad_out (device). */
int ngcf_bpr_backward_f32(const float *u, int64_t Bu, const float *p, int64_t Bp, const float *n, int64_t Bn, int D,
                          float weight_decay, float batch_size, const float *grad_out, float *du, float *dp,
                          float *dn, void *stream);
/* Backward of the row gathers (NGCF.py:151-155): the gradient rows g [M, d] of the gathered positions, summed per distinct row
 * of all_E in a fixed order: out[r, :] = sum of g[order[j], :] for j in [segptr[r], segptr[r+1]), in that order (`order`: the
 * gathered positions sorted by row, stable - duplicates add up in batch order; int64 device arrays).  No atomics. */
int ngcf_segment_sum_rows_f32(const float *g, int64_t ldg, int d, const int64_t *order, const int64_t *segptr, int64_t n_seg,
                              const int64_t *dst_rows, const int64_t *n_seg_dev, float *out, int64_t ldo, int64_t n_out_rows,
                              void *stream);
/* (dst_rows != NULL: the sum of segment r goes to row dst_rows[r] of `out` - the scatter into a dense, zero-filled gradient of
 * all_E with n_out_rows rows; a segment whose destination lies outside [0, n_out_rows) is skipped (r04: memory-safe whatever the
 * caller's index-check cadence); n_seg_dev != NULL: only the first *n_seg_dev segments exist (the count ngcf_rows_sort_unique left on the device: no
 * host round trip between the two launches), n_seg is then an upper bound that sizes the grid) */
/* The distinct rows among M <= 8 192 gathered positions, in one launch: idx int64[M] (rows of all_E, each < 2^50) ->
 * order int64[M] (the positions 0..M-1 sorted by row, equal rows in batch order), rows int64[<= M] (distinct, ascending),
 * segptr int64[<= M + 1] (group bounds inside `order`), n_rows int64[1].  All device arrays sized for M (segptr M + 1).
 * Feeds ngcf_segment_sum_rows_f32; replaces torch.unique + sort + cumsum (a dozen library launches) on the training step. */
int ngcf_rows_sort_unique(const int64_t *idx, int64_t M, int64_t max_row, int64_t *order, int64_t *rows, int64_t *segptr,
                          int64_t *n_rows, void *stream);
/* (max_row: the largest valid row, or -1 = unknown / unchecked: below 2^19 the sort runs on 32-bit keys.  r04: with max_row >= 0 an id
 * outside [0, max_row] - which the forward gather clamped and flagged in its status word - is sorted as ONE sentinel row
 * max_row + 1 behind the valid ones, forms the last segment of `order` and is not counted in n_rows.) */
/* Backward of normalise + dropout + LeakyReLU (NGCF.py:140-144): dM from dN (gradient of the all_E block; NULL = zero:
 * the rows no gather touched), dC (gradient of the carry from the next layer, may be NULL; not both) and the saved carry C. */
int ngcf_layer_bwd_pre_f32(const float *dN, int64_t ldn, const float *dC, int64_t ldc, const float *C, int64_t ldC,
                           int64_t n_rows, int d, float leaky_slope, float drop_p, uint64_t drop_seed,
                           const float *drop_mask, int64_t ld_mask, const int64_t *row_ids, float *dM, int64_t ldm, void *stream);
/* (row_ids: NULL, or the matrix rows the n_rows compacted rows stand for - they index the hash stream of device-mode dropout) */
/* out = init + L^T . X for a ROW-SPARSE X (the last layer's backward: dLE is non-zero on the <= 3 B gathered rows only).
 * csr_t: the CSR of L^T ([N, N]); slot: device int32[N], slot[r] = row of the compact X [R, d] that holds matrix row r, or -1
 * (zero row); init: compact [R, d] or NULL, added to the rows with slot >= 0 (the direct part of the gradient).
 * out[c, :] = (slot[c] >= 0 ? init[slot[c], :] : 0) + sum over the stored entries (c, r, v) of csr_t with slot[r] >= 0 of
 * v * X[slot[r], :], in entry order: a fixed summation order, no atomics; every row of out [N, d] is written.
 * drop_p / seeds: device-side node dropout as in ngcf_spmm_csr_dropout_f32 (csr_t is walked as the transpose): drop_p is taken
 * as a float, and an entry is kept iff every one of its hashes is >= (uint32_t)((double)drop_p * 2^32).
 * workspace: ngcf_spmm_workspace_bytes(csr_t, min(d, 512)) bytes (partial sums of the cut rows). */
int ngcf_spmm_t_rows_f32(const ngcf_csr_t *csr_t, const int32_t *slot, const float *X, int64_t ldx, int d, const float *init,
                         int64_t ldi, float *out, int64_t ldo, float drop_p, const uint64_t *seeds, int n_seeds,
                         void *workspace, int64_t workspace_bytes, void *stream);
/* Which of its two kernels ngcf_spmm_t_rows_f32 would launch for this CSR, width and workspace size under the current options:
 * a read-only query answered by the host function the entry point itself dispatches through (nothing is launched).  "bitmap":
 * 16 rows to a wave, the membership of a column in the R rows tested on a bitmap in LDS - a square matrix whose bitmap fits
 * 160 KiB of LDS beside the hit lists (N <= 1 138 560), d <= 4096, at least 2^22 stored entries (option t_rows_bitmap = 2: any
 * number; 0: never) and a workspace with room for the bitmap behind the partial sums (their bytes + N / 8 + 1 KiB: the size
 * ngcf_spmm_workspace_bytes gives has it from 17 rows on); "slot": one wave per row on the slot table, everywhere else.  Both
 * form every sum in entry order with the same fmaf: the same bits.  NULL (and ngcf_last_error) for a NULL csr, d <= 0 or a
 * negative size.  For tests and tools. */
const char *ngcf_spmm_t_rows_path(const ngcf_csr_t *csr_t, int d, int64_t workspace_bytes);
/* Input gradients of a layer's dense half in one MFMA kernel: dS = dM.W1, dP = dM.W2 (never stored), dLE = dS + dP*E,
 * dE_direct = dS + dP*LE (NGCF.py:131-136 differentiated).  dM: [n_rows, d_out], any d_out >= 1 (65 in the reference's own
 * configuration), with 16-byte aligned rows padded to a multiple of 4 floats (the padding is never used); W1, W2: [d_out, d_in] row-major (nn.Linear.weight); LE, E, dLE, dE: [n_rows, d_in]. */
int64_t ngcf_layer_bwd_input_workspace_bytes(int d_out);
int ngcf_layer_bwd_input_f32(const float *dM, int64_t ldM, int64_t n_rows, int d_out, const float *W1, const float *W2,
                             int d_in, const float *LE, int64_t ldLE, const float *E, int64_t ldE, float *dLE, int64_t ldd,
                             float *dE, int64_t lde, void *workspace, int64_t workspace_bytes, void *stream);
/* Which kernel ngcf_layer_bwd_input_f32 runs for the panel of input columns that starts at col0, and the panel's width in
 * *panel_cols (may be NULL): the next panel starts at col0 + *panel_cols; a panel's columns past d_in do not exist.  A read-only
 * query answered by the host function the entry point itself walks its panels with (nothing is launched); the sizes and the
 * option bwd_input_resident decide, nothing else.  The rules, in this order:
 *   bwd_input_resident != 0, 4 <= d_out <= 128 and n_rows >= 131 072 (two 32-row tiles for each of the 8 waves of 256 persistent
 *   workgroups): panels of 128 columns on "resident" (layer_bwd_input_resident_kernel) while more than 4 columns are left, the
 *   last 1..4 columns on "narrow" (layer_bwd_input_narrow_kernel; d_in <= 4: the whole product);
 *   otherwise 129..160 columns left: "staged_wide" (layer_bwd_input_kernel<5,false>, one panel of 160);
 *   otherwise a panel of 128: "staged_small" (<4,true>, 32-row tiles) up to 16 384 rows, "staged_tall" (<4,false>, 128-row
 *   tiles) above.
 * NULL (and ngcf_last_error) for sizes the entry point rejects and for a col0 that is not the start of a panel.  For tests and tools. */
const char *ngcf_layer_bwd_input_path(int64_t n_rows, int d_in, int d_out, int col0, int *panel_cols);
/* weight gradients of one layer on the fp32 matrix cores: gW1 [d_out, d_in] = dM^T . (LE + E) (the gradient of W1,
 * NGCF.py:131-133), gW2 [d_out, d_in] = dM^T . (LE * E) (W2, NGCF.py:135-136), each row-major with its own leading dimension
 * (so a caller tiling a wide layer passes sub-blocks of the full gradients); d_in, d_out <= 128 per call.  Fixed summation
 * order (per-workgroup partials in the workspace, added in workgroup order).  gb2 / gb1 (may be NULL): [d_out] column sums of dM
 * from the same pass and twice that - the gradients of W2's and W1's bias (b1 enters the layer twice, NGCF.py:131,133). */
int64_t ngcf_bwd_weight_workspace_bytes(void);
int ngcf_layer_bwd_weight_f32(const float *dM, int64_t ldM, const float *LE, int64_t ldLE, const float *E, int64_t ldE,
                              int64_t n_rows, int d_in, int d_out, float *gW1, int64_t ld1, float *gW2, int64_t ld2,
                              float *gb1, float *gb2, void *workspace, int64_t workspace_bytes, void *stream);
/* Which kernel ngcf_layer_bwd_weight_f32 would launch for these sizes and operands, and in *n_workgroups (may be NULL) how many
 * workgroups - one partial result each, which bwd_weight_reduce_kernel adds in workgroup order.  A read-only query answered by
 * the host function the entry point itself dispatches through (nothing is launched, the operands are not dereferenced - only
 * their alignment counts; no option enters).  The rules, in this order:
 *   d_in <= 4 and n_rows >= 65 536: "narrow" (bwd_weight_narrow_kernel), 2 048 workgroups of ceil(n_rows / 2 048) rows;
 *   otherwise the matrix-core kernel on min(256, max(1, (ceil(n_rows / 32) + 1) / 2)) workgroups, which take the 32-row blocks
 *   round robin: "mfma_aligned" (bwd_weight_kernel<true>) when dM, LE and E are 16-byte aligned and their leading dimensions
 *   multiples of 4, "mfma_unaligned" (<false>) otherwise.
 * NULL (and ngcf_last_error) for sizes ngcf_layer_bwd_weight_f32 rejects.  For tests and tools. */
const char *ngcf_layer_bwd_weight_path(int64_t n_rows, int d_in, int d_out, const float *dM, int64_t ldM, const float *LE,
                                       int64_t ldLE, const float *E, int64_t ldE, int *n_workgroups);
/* out[r, 0:d] += add[r, 0:d] */
int ngcf_add_rows_f32(float *out, int64_t ldo, const float *add, int64_t lda, int64_t n_rows, int d, void *stream);

/* ---- top-k of score rows (experiment.py:104-111, demo.py:234-235: `torch.topk(torch.mm(u, items.T), k)`) ---- */
/* out_val/out_idx [n_rows, k]: the k largest entries of every row of `scores` [n_rows, n_cols] in descending
 * order (equal values: lowest column first; NaN sorts above +inf like torch.topk).  1 <= k <= min(n_cols, 1024).
 * The score matrix is a plain GEMM and is left to the caller. */
int ngcf_topk_rows_f32(const float *scores, int64_t ld, int64_t n_rows, int64_t n_cols, int k, float *out_val,
                       int64_t *out_idx, void *stream);
/* Score-and-select in one launch (experiment.py:93,104-109; demo.py:233-235): scores[b, i] = u[b, :] . items[i, :] for every
 * item, then top-k per user row (values descending, ties lowest item first), without a library GEMM.  u: [B, D] (ldu),
 * items: [n_items, D] (ldi; e.g. all_items_emb, a row range of all_E), scratch: [B, ld_scratch >= n_items] floats of caller
 * memory that receives the score matrix (it is what `torch.mm` would have returned), out_val [B, k], out_idx [B, k] int64. */
int ngcf_recommend_topk_f32(const float *u, int64_t ldu, int64_t B, const float *items, int64_t ldi, int64_t n_items,
                            int D, int k, float *scratch, int64_t ld_scratch, float *out_val, int64_t *out_idx, void *stream);

/* ---- full-catalogue ranking and held-out metrics (the NGCF evaluation protocol) ---- */
/* Score-and-select with no score matrix: batch row b ranks user r = user_ids ? user_ids[b] : b (embedding users[r*ldu + 0..D))
 * against every item, score(b, i) = sum_k users[r,k]*items[i,k] as one ascending-k fmaf chain from 0 (fp32 MFMA; the same bits as
 * ngcf_recommend_topk_f32), and writes the k best: values descending, equal values lowest item first, NaN above +inf.
 * Exclusion (excl_rowptr may be NULL): items excl_colidx[excl_rowptr[r] .. excl_rowptr[r+1]) - excl_col_offset never appear;
 * ids ascending within a row, duplicates allowed, ids outside [0, n_items) ignored.  With excl_col_offset = n_user the user rows
 * of the model's Laplacian CSR serve as the exclusion set.  Fewer than k eligible items: the trailing slots are (-inf, -1).
 * An r outside [0, n_user_rows) sets *status and leaves its output row untouched (ngcf_gather_rows_f32's rule).
 * 1 <= k <= min(n_items, 256) (larger k: ngcf_recommend_topk_f32); any D >= 1; n_items < 2^31.  Deterministic, no float atomics:
 * the row of a user does not depend on B, on the batch order or on the item split.  The workspace (ngcf_rank_workspace_bytes,
 * 0 when none is needed) holds the per-split lists when the batch is too small to fill the chip on its own. */
int64_t ngcf_rank_workspace_bytes(int64_t B, int64_t n_items, int D, int k);
int ngcf_rank_topk_f32(const float *users, int64_t ldu, const int64_t *user_ids, int64_t n_user_rows, int64_t B,
                       const float *items, int64_t ldi, int64_t n_items, int D, int k,
                       const int64_t *excl_rowptr, const int32_t *excl_colidx, int64_t excl_col_offset,
                       float *out_val, int64_t *out_idx, int32_t *status,
                       void *workspace, int64_t workspace_bytes, void *stream);
/* Held-out metrics of top lists top_idx [B, k] (entries of -1 ignored) against truth rows (ascending, like the exclusion rows;
 * T = the distinct ids >= 0 after truth_col_offset).  For each cut-off K of ks_host[0..n_ks) (1 <= n_ks <= 8, K <= k), slots
 * 4q..4q+3 are recall = hits/|T|, ndcg = sum over hit ranks j of 1/log2(j+2) / sum_{j < min(K,|T|)} 1/log2(j+2),
 * precision = hits/K, hr = hits > 0; slot 4*n_ks counts the users with non-empty T (users with empty T add nothing).
 * per_user [B, 4*n_ks] (may be NULL) gets the per-row values; sums (device, [4*n_ks + 1]) is ADDED to, in a fixed order
 * (per-block partials, then one workgroup): bit-identical from run to run, and a user set can be ranked in chunks. */
int ngcf_rank_metrics(const int64_t *top_idx, int64_t B, int k, const int64_t *user_ids, int64_t n_user_rows,
                      const int64_t *truth_rowptr, const int32_t *truth_colidx, int64_t truth_col_offset,
                      const int32_t *ks_host, int n_ks, float *per_user, double *sums, int32_t *status, void *stream);

/* ---- certified two-stage ranking: bf16 shortlist, exact fp32 re-score (csrc/rank_prefilter.hip) ---- */
/* ngcf_rank_topk_f32's answer for less fp32 matrix work: every (user, item) pair is scored with bf16 MFMA, the approximate score is
 * turned into an UPPER BOUND of the exact one, the `pool` items with the largest bounds are re-scored exactly, and a per-user
 * certificate says whether the pool's top-k is provably the catalogue's.  A certified row has ngcf_rank_topk_f32's bits; an
 * uncertified one has to be ranked again by ngcf_rank_topk_f32 (engine/shortlist.py does).
 *
 * The bound.  For fp32 rows u, i of width D let u^, i^ be their bf16 images (round to nearest even, 8 significant bits:
 * |x^ - x| <= 2^-8 |x|), s the score of ngcf_rank_topk_f32 (one ascending-k fmaf chain from 0) and s~ the bf16 MFMA score of u^, i^
 * (products exact in fp32, every partial sum within one fp32 ulp of exact, whether the unit truncates or rounds).  Then
 *     |s - s~| <= (beta - 2^-23) |u| |i|,    beta = 2^-7 + 2^-16 + (4 D + 2) 2^-24    (|.| the Euclidean norm)
 * - 2^-7 + 2^-16 for the two operand roundings, 4 D 2^-24 for the two accumulation chains (D 2^-24 + 2 D 2^-24 and their second-order
 * terms, D <= NGCF_RANK_PREFILTER_DMAX), and the last 2^-23 pays for the one rounding of the bound's own evaluation
 *     ub = fmaf(bu, ni, s~),    ni >= |i| and bu >= beta |u| fp32 values rounded UP (the norm in fp64, its nearest fp32, one ulp up),
 * so ub >= s for every pair.  The model needs no underflow and no overflow: a row is REGULAR when every element is 0 or has a
 * magnitude in [2^-40, 2^40] (DESIGN 4.3.22 says why not 2^-60).  An irregular user is never certified; one irregular item in the
 * table and no user is.
 *
 * ngcf_rank_pack_items: the fp32 item table (rows of pitch ldi >= D, as ngcf_rank_topk_f32 takes them) -> out_bf16
 * [n_items, Dp] bf16 (Dp = D rounded up to NGCF_RANK_PREFILTER_KSTEP, the padding zero; 16-byte aligned), norm_up [n_items] = ni,
 * flags[0] = 1 iff an item is irregular (else 0).  One pass, reusable while the table is unchanged.
 *
 * ngcf_rank_shortlist_bf16: batch rows, user_ids, exclusion sets and *status as in ngcf_rank_topk_f32.  Per batch row the `pool`
 * (1 <= pool <= NGCF_RANK_POOL_MAX) eligible items with the largest (float_key(ub), item) pairs in ngcf_rank_topk_f32's order (key
 * descending, item ascending): pool_idx [B, pool] int32, -1 past the eligible items; pool_thr [B] = the pool-th ub, -inf when the
 * pool is not full; user_flags [B] = 1 for an irregular user row (and for an r outside [0, n_user_rows), whose pool_idx row is
 * left untouched).  debug_scores (NULL, or float [2, B, n_items]: tests and the lab) receives s~ and ub of every pair.  The
 * workspace (ngcf_rank_prefilter_workspace_bytes) holds bu and, when the item range is split, the per-split lists.
 *
 * ngcf_rank_rescore: per batch row the pool's fp32 item rows are gathered through LDS (no [B, pool, D] buffer), scored with
 * ngcf_rank_topk_f32's chain (the same bits), sorted in that order, and the best k (1 <= k <= pool) written as ngcf_rank_topk_f32
 * writes them ((-inf, -1) past the eligible items).  certified[b] = 1 iff the user row and the table are regular AND (the pool is
 * not full - it then holds every eligible item - OR the k-th exact score is strictly greater than pool_thr[b]); else 0.
 *
 * Integer atomics in LDS only (the status word's bit, set for a bad id alone, is the exception all entry points share), no float
 * atomics: identical from run to run, and a row does not depend on B, the batch order or the item split. */
#define NGCF_RANK_PREFILTER_KSTEP 16
#define NGCF_RANK_POOL_MAX 256
#define NGCF_RANK_PREFILTER_DMAX 4096
int ngcf_rank_pack_items(const float *items, int64_t ldi, int64_t n_items, int D, void *out_bf16, float *norm_up, int32_t *flags,
                         void *stream);
int64_t ngcf_rank_prefilter_workspace_bytes(int64_t B, int64_t n_items, int D, int pool);
int ngcf_rank_shortlist_bf16(const float *users, int64_t ldu, const int64_t *user_ids, int64_t n_user_rows, int64_t B,
                             const void *packed_bf16, const float *norm_up, int64_t n_items, int D, int pool,
                             const int64_t *excl_rowptr, const int32_t *excl_colidx, int64_t excl_col_offset,
                             int32_t *pool_idx, float *pool_thr, int32_t *user_flags, float *debug_scores, int32_t *status,
                             void *workspace, int64_t workspace_bytes, void *stream);
int ngcf_rank_rescore(const float *users, int64_t ldu, const int64_t *user_ids, int64_t n_user_rows, int64_t B,
                      const float *items, int64_t ldi, int64_t n_items, int D, int k, int pool, const int32_t *pool_idx,
                      const float *pool_thr, const int32_t *user_flags, const int32_t *item_flags, float *out_val, int64_t *out_idx,
                      uint8_t *certified, void *stream);

/* ---- exact held-out positions (csrc/rank_position.hip) ---- */
/* The exact rank of every held-out item among its user's eligible items, with no score matrix and no top list.  Batch row b is user
 * r = user_ids ? user_ids[b] : b; the truth set and the optional exclusion set are item sets as above (rowptr int64, colidx int32
 * ascending within a row, stored id - column offset = item id).  position is int32[n_truth], aligned with truth_colidx: entry e of
 * truth row r, held-out item t, gets
 *     position[e] = #{ eligible i != t : rank_before(key(s_i), i, key(s_t), t) }
 * where eligible means 0 <= i < n_items and i not in the user's exclusion row (the user's other held-out items are eligible and
 * count), s_i is the score of ngcf_rank_topk_f32 (one ascending-k fmaf chain from 0: the same bits), key is the monotone map float
 * -> uint32 under which NaN sorts above +inf, and rank_before(ka, a, kb, b) = ka > kb || (ka == kb && a < b).  So position[e] is the
 * 0-based index of t in the user's full sorted eligible list; wherever it is below 256 it is the column at which
 * ngcf_rank_topk_f32 returns t.
 *   - a held-out item that is in the user's exclusion row: -1
 *   - a held-out id outside [0, n_items) after the offset: -1, and bit 1 (value 2) of *status; it is never used as an index
 *   - r outside [0, n_user_rows): bit 0 (value 1) of *status, nothing is written for that batch row
 *   - entries of users that are not in the batch are left untouched: chunked calls fill one buffer
 *   - a user that occurs twice in user_ids has the same values written twice; duplicate ids within a truth row get equal positions
 * All counts are integers and every atomic is an integer atomic: the result is identical from run to run and does not depend on
 * B, the batch order or the item split.  Tiers: truth rows are ranked NGCF_RANK_POS_CAP entries at a time (the sorted pairs of 64
 * such chunks sit in LDS beside the MFMA tiles); a longer row is cut into chunks that are scored as separate rows of the same user.
 * Users with an empty truth row cost no scoring work.  The workspace (ngcf_rank_positions_workspace_bytes(B, n_items, D, n_truth),
 * n_truth = entries of truth_colidx) holds B + n_truth / NGCF_RANK_POS_CAP chunks - enough for any batch of distinct users; a batch
 * that repeats users with long rows past that sets bit 2 (value 4) of *status and leaves the chunks that did not fit untouched.
 * Any D >= 1, n_items < 2^31. */
#define NGCF_RANK_POS_CAP 64
int64_t ngcf_rank_positions_workspace_bytes(int64_t B, int64_t n_items, int D, int64_t n_truth);
int ngcf_rank_positions_f32(const float *users, int64_t ldu, const int64_t *user_ids, int64_t n_user_rows, int64_t B,
                            const float *items, int64_t ldi, int64_t n_items, int D,
                            const int64_t *truth_rowptr, const int32_t *truth_colidx, int64_t truth_col_offset, int64_t n_truth,
                            const int64_t *excl_rowptr, const int32_t *excl_colidx, int64_t excl_col_offset,
                            int32_t *position, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);
/* Metrics from positions.  Per batch row: T = the distinct ids of the user's truth row, E = n_items - the length of its exclusion
 * row (excl_rowptr may be NULL: E = n_items); a user with T = 0 is not evaluated.  Entries with a negative position (-1 not
 * eligible, -2 never ranked) stay in T and in every denominator and count as misses.  With the valid positions ascending,
 * p_0 < p_1 < .. < p_{V-1} (duplicate ids once), all in fp64:
 *   rr   = 1/(p_0 + 1), 0 if V = 0            ap  = (sum_j (j + 1)/(p_j + 1)) / T
 *   ndcg = sum_j 1/log2(p_j + 2) / sum_{j<T} 1/log2(j + 2)
 *   auc  = sum_j ((E - T) - (p_j - j)) / (T * (E - T)): the share of (held-out, negative) pairs in the right order, a miss counting
 *          as ranked below every negative; a user with E - T <= 0 is left out of the AUC sum and of its counter
 *   per cut-off K of ks_host[0..n_ks) (HOST int32, 0 <= n_ks <= 8, 1 <= K <= n_items): recall = hits/T, ndcg = DCG@K/IDCG@K
 *   (terms added in ascending position; IDCG over j < min(T, K)), precision = hits/K, hr = hits > 0, hits = #{p_j < K}: the
 *   arithmetic and summation order of ngcf_rank_metrics, so for K <= 256 the per-user values, written as float32 as that function
 *   writes them, equal its output bit for bit.  One operation differs below that: log2 is the correctly rounded one of
 *   csrc/dd_log2.h, not the maths library's (good to an ulp, and which ulp differs from a host library's: at 3, for one), so that a
 *   host oracle with the same operation order reproduces every per-user fp64 value.
 * sums (device, float64 [4 + 4*n_ks + 2]) = [rr, ap, ndcg, auc, (recall, ndcg, precision, hr) per K, users, auc_users] is ADDED to
 * in a fixed order (a wave its users in order, a workgroup its waves, one workgroup the blocks): bit-identical from run to run.
 * per_user (float64 [B, 4 + 4*n_ks], may be NULL) gets the per-row values, 0 where a user or its AUC is not evaluated.  Rows of up
 * to NGCF_RANK_POS_WAVE_ROW entries are visited in ascending position out of registers (one entry per lane, a wave-wide minimum per
 * step); longer rows re-read the entries past that boundary every step.  An r outside [0, n_user_rows) sets bit 0 of *status. */
#define NGCF_RANK_POS_WAVE_ROW 64
int ngcf_rank_position_metrics(const int32_t *position, int64_t B, const int64_t *user_ids, int64_t n_user_rows,
                               const int64_t *truth_rowptr, const int32_t *truth_colidx, int64_t n_truth,
                               const int64_t *excl_rowptr, int64_t n_items, const int32_t *ks_host, int n_ks,
                               double *per_user, double *sums, int32_t *status, void *stream);

/* Candidate-list evaluation, the reference's own test protocol (experiment.py:66-119) for T cases x C candidates in one launch
 * (DESIGN 4.3).  Case t scores user r = user_ids[t] (users[r*ldu + 0..D)) against the items cand[t*ldc + 0..C) (rows of `items`,
 * ldi); column 0 is the held-out item.  s_j = <u, item[cand_j]> in fp32 in a summation order that depends on D alone: the same
 * (user row, item row) pair gives the same bits whatever T, C, the case order, the column or the tables' alignment, so duplicated
 * candidates tie exactly.  position[t] = the number of columns that sort above column 0 in the order of ngcf_topk_rows_f32 (value
 * descending, equal values lowest column first - column 0 wins every tie -, NaN above +inf).  Per case, added into sums
 * (device, [n_ks + 4]) = [hits, ndcg@ks[0..n_ks), bpr, abs_err, cases]:
 *   hits    position < hit_k                                      (experiment.py:104-106; the reference's hit_k is 3)
 *   ndcg@K  position < K ? 1/log2(position + 2) : 0               (experiment.py:109-111,121-128)
 *   bpr     BPR.forward (bprloss.py:15-22, the abs included) on u repeated user_repeat times (1 or C: only the weight of |u|^2 in
 *           the regulariser), pos = item[cand_0], neg = item[cand_1.., cand_{C-1}, cand_1] (experiment.py:96-100; C rows for
 *           C >= 2, none for C = 1), divided by batch_size
 *   abs_err |s_0 - ratings[t]| (what the reference's sqrt(MSE) of two scalars is, experiment.py:114-116); 0 when ratings is NULL
 *   cases   1
 * in a fixed order (per-workgroup partials, then one workgroup; no float atomics): bit-identical from run to run, and a case set
 * can be evaluated in chunks and across years into one `sums` (the grouping then differs: equal to fp64 rounding).
 * scores [T, C] and position int32[T] may be NULL.  Every id of a case is checked before any of its rows is loaded: a case with a
 * user id outside [0, n_user_rows) or a candidate outside [0, n_items) sets *status, adds nothing to sums and gets position -1
 * (its row of scores: NaN).  ks_host: HOST int32[n_ks], 0 <= n_ks <= 8; 1 <= hit_k, ks[i] <= C <= 1024 (a k above C is an error,
 * as torch.topk raises there); any D >= 1, any alignment (float4 loads where `items` and ldi allow them). */
int ngcf_eval_candidates_f32(const float *users, int64_t ldu, int64_t n_user_rows, const float *items, int64_t ldi,
                             int64_t n_items, int D, const int64_t *user_ids, const int64_t *cand, int64_t ldc, int64_t T, int C,
                             const float *ratings, const int32_t *ks_host, int n_ks, int hit_k, float weight_decay,
                             float batch_size, int user_repeat, float *scores, int32_t *position, double *sums, int32_t *status,
                             void *stream);

/* Rank-point blending, the reference's recommender after its topk (demo.py:285-292, 315-334, 378-398) for R request
 * rows in G columns in one launch.  Request row r has up to three lists of Pl <= P items each, best first: its preference list
 * pref[r*ld_pref + 0..Pl) (a top list of ngcf_rank_topk_f32), the congestion list con[con_slot[r]*ld_con + ..) of its day and the
 * distance list dis[dis_slot[r]*ld_dis + ..) of its departure point (top lists of ngcf_topk_rows_f32 over the negated values; con
 * or con_slot NULL: no congestion points, the same for distance).  The item at position j of a list gets P - j points of that
 * kind, every other item 0; an entry of -1 is an empty slot; the items of a list are distinct.  Column g is the set of rows
 * col_rows[col_rowptr[g] .. col_rowptr[g+1]) (a row may be in several columns, at most once in each); with sp, sc, sd the exact
 * int32 sums of the three kinds over the column's rows,
 *   rating[g, i] = ((double)sp * w_pref + (double)sc * w_con) + (double)sd * w_dis
 * in fp64, left to right, every operation rounded on its own (no FMA): numpy's result bit for bit, independent of the order of rows,
 * columns and workgroups.  out_items / out_rating [G, top]: the `top` items with item_mask[i] != 0 (uint8 [n_items]; NULL: all),
 * rating descending, equal ratings (-0.0 = +0.0) lowest item first; slots past the eligible items are (-1, -inf); a column without
 * rows rates every item 0.0.  table (may be NULL; tests and small catalogues): [G, n_items] the ratings of all items, masked or not.
 * One workgroup per (column, tile of tile_items items; 0 = the default, at most 4096), the tile's sums in LDS; with more than one
 * tile the tiles' lists pass through the workspace (ngcf_blend_workspace_bytes; 0 for one tile, -1 for arguments out of range) and a
 * second kernel merges them per column: the result does not depend on tile_items.  No float atomics.  Every id is checked before
 * use: a row index outside [0, R), a slot outside [0, S_con) / [0, S_dis), a list entry outside [0, n_items) other than -1 or a
 * column range outside col_rows (n_col_rows entries) sets *status and contributes nothing (ngcf_gather_rows_f32's rule).
 * Argument errors, before any launch: top outside [1, 256], P outside [1, 1024], Pl outside [1, P], R * P >= 2^31 (the bound that
 * keeps the int32 sums exact), n_items outside [1, 2^31). */
int64_t ngcf_blend_workspace_bytes(int64_t G, int64_t n_items, int top, int tile_items);
int ngcf_blend_points(const int64_t *pref, int64_t ld_pref, int64_t R, int Pl, const int64_t *con, int64_t ld_con, int64_t S_con,
                      const int64_t *con_slot, const int64_t *dis, int64_t ld_dis, int64_t S_dis, const int64_t *dis_slot,
                      const int64_t *col_rowptr, const int64_t *col_rows, int64_t n_col_rows, int64_t G, int P, int64_t n_items,
                      double w_pref, double w_con, double w_dis, const uint8_t *item_mask, int top, int tile_items,
                      int64_t *out_items, double *out_rating, double *table, int32_t *status, void *workspace,
                      int64_t workspace_bytes, void *stream);

/* Unseen items per case, the reference's TourDataset._negative_sampling (utils.py:213-275) for T cases in one launch.
 * Case `row` belongs to user user_ids[row], whose seen items are seen_colidx[seen_rowptr[u] .. seen_rowptr[u+1]) - col_offset,
 * ascending and distinct, in [0, n_items) (the arrays of ngcf_rank_topk_f32's exclusion sets).  The case draws m of the user's
 * n = n_items - (length of that row) unseen items, uniformly and without replacement, as a pure function of (seed, t = case_offset +
 * row, the seen row), all arithmetic unsigned 64-bit:
 *   fmix(x): x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33
 *   a = fmix(seed ^ (t * 0x9E3779B97F4A7C15))
 *   for j in 0 .. m-1:  x = j + mulhi64(fmix(a + (j + 1) * 0xD1B54A32D192ED03), n - j)
 *                       r_j = map(x); map(x) = map(j)           (map: the identity at j = 0 - a partial Fisher-Yates shuffle)
 * and slot j gets the r_j-th unseen item in ascending order, r_j + #{k : c_k - k <= r_j} for the seen row c_0 < c_1 < ...  A case
 * set drawn in chunks with case_offset = the chunk's first case equals the set drawn at once.  out[row*ld_out + ..]: first[row]
 * (when `first` is given: the held-out item of a candidate list), then the m items; ld_out >= m + (first != NULL).  *status is
 * OR-ed into, never cleared: 1 = a user id outside [0, n_rows), 2 = a user with fewer than m unseen items (np.random.choice raises
 * there); the drawn slots of such a case are -1, its first[row] is still written.  Argument errors, before any launch: m outside
 * [1, 1023] (m + 1 <= 1024, the limit of ngcf_eval_candidates_f32), n_items outside [1, 2^31), ld_out too small, a null pointer
 * (`first` may be NULL); T == 0 is not an error. */
int ngcf_sample_unseen(const int64_t *seen_rowptr, const int32_t *seen_colidx, int64_t col_offset, int64_t n_rows, int64_t n_items,
                       const int64_t *user_ids, int64_t T, int64_t case_offset, int m, uint64_t seed, const int64_t *first,
                       int64_t *out, int64_t ld_out, int32_t *status, void *stream);

/* Hard negatives, dynamic negative sampling for BPR training, for T cases in one launch: of m unseen draws per case, the one the
 * current embeddings score highest.  Case `row` of user u = user_ids[row]:
 *   draw    c_0 .. c_{m-1} = exactly the m items of ngcf_sample_unseen for (seed, t = case_offset + row, the seen row of u, m): the
 *           same case key, positions, partial Fisher-Yates map and rank-to-item conversion, 1 <= m <= NGCF_SAMPLE_HARD_M_MAX
 *   score   s_j = <users[u*ldu + 0..D), items[c_j*ldi + 0..D)> with exactly the score bits of ngcf_eval_candidates_f32 (a summation
 *           order that depends on D alone, whatever the tables' alignment)
 *   select  the largest s_j in the order of ngcf_topk_rows_f32 on the scores' bits (NaN above +inf - a NaN whose sign bit is set,
 *           as gfx950 makes of inf - inf, below -inf -, -0.0 below +0.0); equal bits: the lowest slot j
 * and neg[row] = c_j, score[row] = s_j (fp32, may be NULL), slot[row] = j (int32, may be NULL): what ngcf_sample_unseen, then
 * ngcf_eval_candidates_f32 with `scores`, then an argmax over each row would give, bit for bit, with nothing of size T x m written
 * to memory.  A case set drawn in chunks with case_offset = the chunk's first case equals the set drawn at once.  *status is OR-ed
 * into, never cleared: 1 = a user id outside [0, n_rows), 2 = a user with fewer than m unseen items; such a case writes neg = -1,
 * slot = -1 and a NaN score and loads no embedding row (the user id is checked before any row is loaded; the drawn items lie in
 * [0, n_items)).  Argument errors, before any launch: m outside [1, 64], n_items outside [1, 2^31), n_item_rows < n_items (the item
 * table is shorter than the catalogue the sets index), n_user_rows < n_rows, D < 1, ldu or ldi below D, a null pointer; T == 0 is
 * not an error.  Any D, any alignment (float4 loads where `items` and ldi allow them). */
#define NGCF_SAMPLE_HARD_M_MAX 64
int ngcf_sample_hard_f32(const int64_t *seen_rowptr, const int32_t *seen_colidx, int64_t col_offset, int64_t n_rows, int64_t n_items,
                         const float *users, int64_t ldu, int64_t n_user_rows, const float *items, int64_t ldi, int64_t n_item_rows,
                         int D, const int64_t *user_ids, int64_t T, int64_t case_offset, int m, uint64_t seed, int64_t *neg,
                         float *score, int32_t *slot, int32_t *status, void *stream);

/* Popularity-weighted negatives for T cases in one launch: m distinct items the case's user has no stored interaction with, drawn in
 * proportion to an integer weight w_i per item.  The seen sets are those of ngcf_sample_unseen; w_i in [0, 2^40],
 * n_items in [1, 2^31), W = sum of all w_i in [1, 2^62).  The law is successive sampling, np.random.choice(p = w / sum, replace =
 * False): slot 0 is item i with probability w_i / U over the user's unseen items, U their weight; slot j is item i with probability
 * w_i / U_j over the unseen items not drawn yet, U_j = U - (w of slots 0 .. j-1).  An item of weight 0 is never drawn.  Integer
 * weights make every comparison exact and the result recomputable on the host.
 *
 * Prepared arrays, once per (seen sets, weights):
 *   cdf  int64 [n_items + 1]   cdf[i] = sum of w_i' over i' < i, so cdf[0] = 0, cdf[n_items] = W and w_i = cdf[i+1] - cdf[i]; the
 *                              caller's (an int64 prefix sum is exact)
 *   gap  int64, one per stored entry of the seen sets, at the entry's position in seen_colidx: for the k-th seen item c_k of a row,
 *                              gap_k = cdf[c_k] - S_k with S_k = sum of w[c_k'] over k' < k - the unseen weight below c_k; it
 *                              does not decrease with k
 *   mass int64 [n_rows]        U = W - S_len, the user's unseen weight
 * ngcf_weighted_prepare fills gap and mass from cdf, one wave per seen row, integer adds only (identical from run to run); S_K is
 * recovered as cdf[c_K] - gap_K for K < len and as W - mass[u] for K = len.  Its *status is OR-ed into, never cleared: 4 = a stored
 * id outside [0, n_items) (it counts as weight 0; arrays prepared from such sets are not to be drawn from).
 *
 * The draw of case `row`, user u = user_ids[row], is a pure function of (seed, t = case_offset + row, the seen row, the weights), with
 * no rejection loop, all arithmetic unsigned 64-bit; fmix, the case key and the step constant are ngcf_sample_unseen's:
 *   a = fmix(seed ^ (t * 0x9E3779B97F4A7C15))
 *   for j in 0 .. m-1:
 *     r'  = mulhi64(fmix(a + (j + 1) * 0xD1B54A32D192ED03), U_j)                  a point in [0, U_j)
 *     step over the drawn intervals (q_i, w_i), i < j, of the user's unseen coordinate:
 *           e_i = q_i - sum of w_i' over the i' with q_i' < q_i ;  r = r' + sum of w_i over the i with e_i <= r'
 *     K   = #{k : gap_k <= r}                                                     a search of the user's gap row
 *     tgt = r + S_K
 *     c_j = the largest i with cdf[i] <= tgt                                      a search of cdf; w[c_j] > 0 and c_j is unseen
 *     q_j = cdf[c_j] - S_K ;  U_{j+1} = U_j - w[c_j]
 * mulhi64 without rejection gives every point of [0, U_j) floor(2^64 / U_j) hash values or one more: a relative bias of at most
 * U_j / 2^64 per point (< 2^-2 at the largest admissible U, 2^-34 at U = 2^30), the trade ngcf_sample_unseen makes.  A case set drawn in chunks with case_offset = the
 * chunk's first case equals the set drawn at once, and slot 0 of a draw of m items is the draw of one item.
 * out[row*ld_out + 0..m): the items; draw_weight[row*ld_weight + 0..m) (may be NULL): w of each; case_mass[row] (may be NULL): U -
 * so slot j's proposal probability is exactly draw_weight_j / (case_mass - sum of draw_weight over the slots before j).  *status is
 * OR-ed into, never cleared: 1 = a user id outside [0, n_rows) (no id is used as an index before it is checked; its case_mass is
 * 0), 2 = a user with fewer than m positive-weight unseen items (U_j = 0 at some step); all slots of such a case are -1 and its
 * weights 0.  Argument errors, before any launch: m outside [1, NGCF_SAMPLE_WEIGHTED_M_MAX], n_items outside [1, 2^31), ld_out (or,
 * with draw_weight, ld_weight) < m, a null pointer; T == 0 (n_rows == 0 for the preparation) is not an error. */
#define NGCF_SAMPLE_WEIGHTED_M_MAX 64
int ngcf_weighted_prepare(const int64_t *seen_rowptr, const int32_t *seen_colidx, int64_t col_offset, int64_t n_rows, int64_t n_items,
                          const int64_t *cdf, int64_t *gap, int64_t *mass, int32_t *status, void *stream);
int ngcf_sample_weighted(const int64_t *seen_rowptr, const int32_t *seen_colidx, int64_t col_offset, int64_t n_rows, int64_t n_items,
                         const int64_t *cdf, const int64_t *gap, const int64_t *mass, const int64_t *user_ids, int64_t T,
                         int64_t case_offset, int m, uint64_t seed, int64_t *out, int64_t ld_out, int64_t *draw_weight,
                         int64_t ld_weight, int64_t *case_mass, int32_t *status, void *stream);

/* Per-segment quantile floor, the numeric core of the reference's Preprocess.scale_implicit (utils.py:103-122) for every
 * user in one call.  Segment u is the entries order[rowptr[u] .. rowptr[u+1]), positions into x and out (both double [T]); order ==
 * NULL is the identity: x is already grouped.  With z(v) = ((v - mean) / scale) + shift (0, 1, 0: the identity) and, for the n values
 * of the segment sorted ascending s[0 .. n-1],
 *   lo = ((n-1)*q4) / 4;  t = (((n-1)*q4) % 4) * 0.25;  a = z(s[lo]);  b = z(s[min(lo+1, n-1)]);  d = b - a
 *   quant[u] = t < 0.5 ? a + d*t : b - d*(1-t)            (numpy's percentile(method="linear"), pandas' quantile(q4/4))
 *   out[p]   = z(x[p]) < quant[u] ? 0.0 : z(x[p])
 * every operation an individually rounded fp64 one (no FMA), so the result is bit-equal to numpy's; the sign of a zero is not part
 * of the contract.  quant[u] of an empty segment is NaN.  out may alias x: a segment is read completely before any of it is written,
 * and segments are disjoint.  q4 in {1, 2, 3}.  Segments of up to wave_max values (0: the default, 64; [0, 64]) are ranked by one
 * wave, longer ones by a radix select of one workgroup; the result does not depend on it.  *status is OR-ed into, never cleared:
 * 1 = a rowptr that decreases or leaves [0, T], or an order entry outside [0, T): that segment writes nothing to out, its quant is NaN;
 * 2 = a NaN in a segment: its quant is NaN and its values pass through as z(x), unfloored (a comparison with NaN is false).
 * Argument errors, before any launch: q4 outside [1, 3], wave_max outside [0, 64], scale not > 0 or not finite, a negative count,
 * a null pointer (`order` may be NULL); T == 0 or n_rows == 0 is not an error and writes nothing. */
int ngcf_segment_quantile_floor_f64(const int64_t *rowptr, int64_t n_rows, const int64_t *order, const double *x, int64_t T,
                                    double mean, double scale, double shift, int q4, int wave_max,
                                    double *quant, double *out, int32_t *status, void *stream);

/* Yeo-Johnson power transform, the numeric core of sklearn's PowerTransformer() that the reference's Preprocess.scale_implicit runs with
 * args.scaler == 'power' (utils.py:107-112).  With eps = 2^-52,
 *   psi(x, l) = log1p(x)                            x >= 0 (-0.0 included), |l| < eps
 *             = (pow(x + 1, l) - 1) / l             x >= 0, otherwise
 *             = -log1p(-x)                          x <  0, |l - 2| <= eps
 *             = -(pow(-x + 1, 2 - l) - 1) / (2 - l) x <  0, otherwise
 *             = x                                   x a NaN
 * sklearn 1.7's _yeo_johnson_transform operation for operation: x + 1, pow, - 1, / l (and 2 - l, -x + 1, the final negation) are
 * each an individually rounded fp64 operation (no FMA); what differs from numpy's result is the last bits of pow and log1p
 * themselves, the device's libm against the host's.
 * ngcf_yeo_johnson_f64: out[t] = psi(x[t], lambda) for t in [0, T); out may alias x.
 * ngcf_yeo_johnson_moments_f64: one evaluation of the likelihood that fits lambda, over the rows whose x is not a NaN (sklearn drops
 * NaNs before the fit), result[0..3] on the device:
 *   n    = the number of such rows
 *   mean = (sum psi(x, lambda)) / n
 *   M2   = sum (psi(x, lambda) - mean)^2
 *   c    = sum sign(x) * log1p(|x|)                 (it does not depend on lambda)
 * so that the negative log-likelihood is n/2 * log(M2 / n) - (lambda - 1) * c.  Each thread keeps a running (n, mean, M2) in
 * Welford's form over a grid-stride slice; partials are merged with Chan's formula in a fixed tree (wave, workgroup, one partial
 * per workgroup in the workspace, a second launch of one workgroup for the rest): no floating-point atomics, and a grid that depends
 * on T alone, so the four doubles are bit-identical from run to run.  ngcf_yeo_johnson_moments_launch reports that grid: the
 * workgroups of the first launch for T rows, the threads of a workgroup, and the cap on the workgroups (any pointer may be NULL).
 * workspace: ngcf_yeo_johnson_workspace_bytes(T) bytes, 8-byte aligned (-1 for T < 0).  Argument errors, before any launch: negative
 * T, a NaN lambda, a null pointer, a workspace that is too small (NGCF_ERR_WORKSPACE).  T == 0 is not an error: the transform writes
 * nothing, the moments are n = 0, mean = M2 = c = 0, and x and workspace may be NULL. */
int ngcf_yeo_johnson_f64(const double *x, int64_t T, double lambda, double *out, void *stream);
int64_t ngcf_yeo_johnson_workspace_bytes(int64_t T);
int ngcf_yeo_johnson_moments_launch(int64_t T, int *blocks, int *threads, int *max_blocks);
int ngcf_yeo_johnson_moments_f64(const double *x, int64_t T, double lambda, double *result, void *workspace, int64_t workspace_bytes,
                                 void *stream);

/* ---- beyond-accuracy figures of top lists (csrc/list_quality.hip) ----
 * What the lists are made of, next to how accurate they are.  A list is a row of top_idx (int64, row pitch ld >= k: a column slice of
 * a wider tensor works), its first k columns best first - ngcf_rank_topk_f32's out_idx, ngcf_blend_points' out_items.  A negative
 * entry is an empty slot wherever it stands.  An entry >= n_items sets bit 0 (value 1) of *status; it is compared before anything
 * else is done with it and is never used as an index (the slot then counts as empty).  n_items < 2^31.
 *
 * Exposure: counts[i] += the number of entries equal to i in columns [0, k) of all B rows (counts: int64[n_items], ADDED to, so a
 * user set can be counted in chunks).  Integer atomics only: identical from run to run.  Up to NGCF_EXPOSURE_LDS_ITEMS items (a
 * constant of the source file) every workgroup folds its slice of at most 2^30 entries into an int32 table in LDS and adds the
 * non-zero slots with one 64-bit atomic each; above it every entry is one 64-bit atomic in memory.  Same counts either way.
 * B * k <= 2^40. */
int ngcf_list_exposure(const int64_t *top_idx, int64_t ld, int64_t B, int k, int64_t n_items, int64_t *counts, int32_t *status,
                       void *stream);
/* Summary of an exposure histogram.  sorted_counts: the n_items counts in ascending order c_(1) <= .. <= c_(n) (the caller sorts);
 * counts, popularity (int64[n_items], both or neither; with them n_user >= 1): the same counts in item order and the items'
 * popularity.  out (device, int64[6]):
 *   out[0] covered  = #{c_i > 0}                     out[1] total = sum c_i               out[2] weighted = sum_{i=1..n} i * c_(i)
 *   out[3] status   : bit 0 (value 1) n_items * total >= 2^62, weighted is then not computed (0); bit 1 (value 2) a negative count
 *   out[4] the bits of the double clog = sum c_i * log2(c_i), a term with c_i = 0 being 0
 *   out[5] the bits of the double nov  = sum c_i * (log2(n_user) - log2(max(pop_i, 1))), 0 without popularity
 * The integers are exact.  In the two doubles log2 is the correctly rounded one of csrc/dd_log2.h, every operation is rounded on its
 * own (no FMA), and the terms are added in a fixed tree - a thread its strided elements in ascending order, a wave, a workgroup, one
 * workgroup the blocks; no float atomics - on a grid that depends on n_items alone: bit-identical from run to run.  From these:
 * coverage = covered / n, gini = 2 weighted / (n total) - (n + 1) / n, entropy = log2(total) - clog / total, novelty = nov / total. */
int ngcf_exposure_summary(const int64_t *sorted_counts, const int64_t *counts, const int64_t *popularity, int64_t n_items,
                          int64_t n_user, int64_t *out, void *stream);
/* Intra-list diversity: the mean cosine distance of the item pairs of a list, at up to 8 cut-offs ks_host[0..n_ks) (HOST int32,
 * 2 <= K <= min(k, NGCF_LIST_DIV_K_MAX)) from one pass.  items [n_items, D] fp32, row pitch ldi >= D (a row range of all_E, unaligned
 * rows: 16-byte loads where the pointer and the pitch allow them, dword loads elsewhere, the same bits either way); any D >= 1.
 * Per row, with e_a the item row of column a:
 *   G_ab   = sum_k e_a[k] * e_b[k] in fp32 as ONE ascending-k fmaf chain from 0 (the score of ngcf_rank_topk_f32; fp32 MFMA), so its
 *            bits do not depend on the tiling, on B or on the row order, and G_ab = G_ba
 *   cos_ab = (double)G_ab / sqrt((double)G_aa * (double)G_bb), every fp64 operation rounded once, no FMA; 0 where the product under the
 *            root is 0; a NaN propagates.  d_ab = 1.0 - cos_ab
 *   s_b    = sum_{a < b} d_ab over the a whose slot and b's are not empty, added in ascending a from 0.0
 *   S_K    = sum_{b < K} s_b over the b whose slot is not empty, added in ascending b from 0.0 - every cut-off is a prefix of one chain
 *   V_K    = the number of non-empty slots in columns [0, K);   ild@K = S_K / (double)(V_K (V_K - 1) / 2)
 * A row with V_K < 2 is not evaluated at K: its value is 0 and it is not counted.  per_user (float64 [B, n_ks], may be NULL) gets the
 * per-row values; sums (device, float64 [2 n_ks]) = [sum of ild@K per K, rows counted at K per K] is ADDED to in a fixed order (a wave
 * its run of consecutive rows in order, a workgroup its four waves, one workgroup the blocks, on a launch shape that depends on B
 * alone): bit-identical from run to run.  Nothing of size [B, k, D] or [B, k, k] is written to memory. */
#define NGCF_LIST_DIV_K_MAX 64
int ngcf_list_diversity_f32(const int64_t *top_idx, int64_t ld, int64_t B, int k, const float *items, int64_t ldi, int64_t n_items,
                            int D, const int32_t *ks_host, int n_ks, double *per_user, double *sums, int32_t *status, void *stream);

/* ---- diversified top lists (csrc/list_rerank.hip) ----
 * Greedy Maximal Marginal Relevance: from a pool of n candidates per request pick `top` of them one by one, each pick trading its
 * relevance against its similarity to what is already picked.  One launch; nothing of size [B, n, D] or [B, n, n] goes to memory.
 *
 * Pool: row b of pool_idx (int64, row pitch ld >= n), columns [0, n), 1 <= n <= NGCF_LIST_MMR_POOL_MAX, 1 <= top <= n -
 * ngcf_rank_topk_f32's out_idx, ngcf_blend_points' out_items.  A negative entry is an empty slot wherever it stands.  An entry
 * >= n_items sets bit 0 (value 1) of *status; it is compared before anything else is done with it and is never used as an index
 * (the slot then counts as empty).  n_items < 2^31.
 * Relevance: rel [B, n], row pitch ldr >= n, fp32 (rel_f64 = 0: ngcf_rank_topk_f32's values) or fp64 (rel_f64 = 1:
 * ngcf_blend_points' ratings), widened to double on load: v_a.  The relevance of an empty slot is not used.
 * items [n_items, D] fp32, row pitch ldi >= D (a row range of all_E, unaligned rows: 16-byte loads where the pointer and the pitch
 * allow them, dword loads elsewhere, the same bits either way); any D >= 1.  Per row, with e_a the item row of slot a:
 *   G_ab   = sum_k e_a[k] * e_b[k] in fp32 as ONE ascending-k fmaf chain from 0 (the bits of ngcf_list_diversity_f32 and
 *            ngcf_rank_topk_f32; fp32 MFMA): G_ab = G_ba
 *   cos_ab = (double)G_ab / sqrt((double)G_aa * (double)G_bb), every fp64 operation rounded once, no FMA; 0.0 where the product under
 *            the root is 0; a NaN propagates
 *   r_a    normalize = 0: v_a.  normalize = 1: with vmin and vmax the smallest and the largest FINITE v_a of the non-empty slots (a
 *            zero of either sign enters both as +0.0), r_a = (v_a - vmin) / (vmax - vmin) - a subtraction, a subtraction, a
 *            division, each rounded once - for a finite v_a; r_a = 0.0 for every finite v_a when vmax == vmin or when no value is
 *            finite; a v_a that is not finite (an infinity, a NaN) stays as it is
 *   step 0:      key_a = lam * r_a
 *   step t >= 1: key_a = lam * r_a - (1.0 - lam) * m_a; 1.0 - lam is formed once; two products and one subtraction, each rounded
 *            once, no FMA.  m_a = cos_as of the first pick s; with every further pick s it becomes a NaN if it or cos_as is a NaN,
 *            cos_as if cos_as > m_a, and stays otherwise: the largest cosine to the slots picked so far, a NaN once any of them is
 *   pick:    the non-empty slot not picked so far with the greatest key.  A NaN key ranks below every other key, -inf included; +0.0
 *            and -0.0 are equal; among equal keys, and among NaN keys, the lowest slot wins
 * The loop runs min(top, V) steps, V = the number of non-empty slots.  Step t writes out_items[b, t] = the picked item id,
 * out_slots[b, t] = its pool column (int32, may be NULL) and out_keys[b, t] = the key it was picked with (float64, may be NULL; a
 * NaN key is written as the quiet NaN 0x7ff8000000000000); the columns t >= V hold (-1, -1, -inf).  The outputs are [B, top],
 * contiguous.  A row's result depends on that row alone - not on B, the row order or the launch shape - and there are no atomics
 * but the status bit: identical from run to run.
 * Argument errors, before any launch (NGCF_ERR_ARG, message "list_mmr: ..."): a null pointer (out_slots and out_keys may be NULL),
 * n outside [1, NGCF_LIST_MMR_POOL_MAX], top outside [1, n], lam a NaN or outside [0, 1], D < 1, n_items outside [1, 2^31), a
 * negative B, a row pitch below its row.  B == 0 launches nothing. */
#define NGCF_LIST_MMR_POOL_MAX 64
int ngcf_list_mmr_f32(const int64_t *pool_idx, int64_t ld, const void *rel, int rel_f64, int64_t ldr, int64_t B, int n, int top,
                      const float *items, int64_t ldi, int64_t n_items, int D, double lam, int normalize, int64_t *out_items,
                      int32_t *out_slots, double *out_keys, int32_t *status, void *stream);

/* ---- year-slice Laplacians straight into CSR (csrc/laplacian.hip; the reference's Matrix.create_matrix, matrix.py:12-83) ----
 * What matrix.laplacian_slices computes, with the state of R kept between years as a user-sorted CSR (rowptr int64[n_user + 1],
 * item int32, rating fp32) instead of a sorted key list.  Years are taken in order of first appearance; within a year the last
 * record of a (user, item) in input order wins, a newer year overrides an older one, a rating that compares == 0 (-0.0 too)
 * deletes the edge, carried over or not; the degree of a node is the count of its state entries.  One year is five calls:
 *   1. ngcf_laplacian_bucket   histogram of the year's T records by user (integer atomics: counts are order-free), exclusive scan
 *        -> bptr int64[n_user + 1], scatter of (item, sequence number = position in the year's input, rating) into per-user buckets
 *        b_item / b_seq / b_rating [T].  The order inside a bucket is arbitrary; the sequence number is what makes "last wins"
 *        deterministic.  info int32[4]: [0] status (bit 1: an id outside [0, n_user) / [0, n_item): the record is left out of the
 *        buckets, never read through - NGCF_ERR_INDEX is the caller's to raise after reading the word back), [1] rows of the
 *        workgroup class, [2] rows of the long-row class (they size step 2's launches and tables).  count: int32[n_user] scratch.
 *   2. ngcf_laplacian_resolve  per user with new records: the sorted state row merged with the bucket by (item, sequence), the last
 *        of every item kept, == 0 dropped, written to the scratch row t_item / t_rating [old_nnz + T] at old_rowptr[u] + bptr[u];
 *        users without records are copied through in step 3.  Three classes by candidate count (old + new), limits from
 *        ngcf_laplacian_limits: up to the wave limit a wave per row ranks the candidates in registers with cross-lane reads; up
 *        to the workgroup limit a workgroup sorts them in LDS (bitonic); above it a workgroup uses a table of 2 * n_item words in
 *        long_tables (n_tables of them, one per workgroup: an integer max of the sequence numbers per item, the winners' ratings,
 *        an ordered sweep) - right for any length, also a bucket longer than n_item.  Then deg int32[N]: users = resolved counts,
 *        items = an integer histogram; rowptr int64[N + 1] = its exclusive scan: the slice's row pointers, and rowptr[0 .. n_user]
 *        the new state's.  status bit 2: a state row pointer or item out of range; bit 4: a long row and no table for it.
 *      (host: ds = float32 d^-1/2 of deg with inf -> 0, by numpy's float32 power - that routine is not correctly rounded, so its
 *       bits cannot be reproduced here; this N-sized vector is the one read-back of a year besides the counts that size arrays.)
 *   3. ngcf_laplacian_emit     the new state s_item / s_rating [nnz] and its users s_user [nnz]; the user rows of the slice:
 *        colidx = n_user + item, vals = float((double(ds[u]) * double(w)) * double(ds[n_user + i])); and vals_item, the item
 *        row's own float((double(ds[n_user + i]) * double(w)) * double(ds[u])) - two separately rounded products, no FMA.
 *        *zeros: how many of the 2 * nnz values are 0 (a device count: the common case has none and pays no pass for them).
 *   4. (caller: the stable order of the int32 s_item - one library sort of 32-bit keys.)
 *      ngcf_laplacian_item_rows  colidx[e] = s_user[order[e]], vals[e] = vals_item[order[e]]: the item rows, by (item, user).
 *   5. ngcf_laplacian_drop_zeros  only when *zeros != 0: the slice without its zero values (they stay in the state and in the
 *        degrees): count int32[n_rows] scratch, out_rowptr int64[n_rows + 1], out_colidx / out_vals [out_nnz = nnz - zeros].
 * The result per slice is one [N, N] CSR: rowptr int64[N + 1], colidx int32, vals fp32, the user rows followed by the item rows.
 * workspace: ngcf_laplacian_workspace_bytes(n_user, n_item) bytes, 8-byte aligned (-1 for sizes that do not fit).  NaN ratings are
 * undefined (a NaN is kept as an edge; nothing is read out of bounds).  No floating-point atomics: two builds give the same bytes.
 * Argument errors, before any launch (NGCF_ERR_ARG, message "laplacian: ..."): a null pointer, a negative count,
 * n_user + n_item >= 2^31, more than 2^31 - 1 records in one year; NGCF_ERR_WORKSPACE for a workspace that is too small.
 */
int ngcf_laplacian_limits(int *wave_limit, int *workgroup_limit);
int64_t ngcf_laplacian_workspace_bytes(int64_t n_user, int64_t n_item);
int ngcf_laplacian_bucket(const int64_t *userid, const int64_t *itemid, const float *rating, int64_t T, int64_t n_user, int64_t n_item,
                          const int64_t *old_rowptr, int32_t *count, int64_t *bptr, int32_t *b_item, int32_t *b_seq, float *b_rating,
                          int32_t *info, void *workspace, int64_t workspace_bytes, void *stream);
int ngcf_laplacian_resolve(const int64_t *old_rowptr, const int32_t *old_item, const float *old_rating, int64_t old_nnz,
                           const int64_t *bptr, const int32_t *b_item, const int32_t *b_seq, const float *b_rating, int64_t T,
                           int64_t n_user, int64_t n_item, int64_t n_block_rows, int64_t n_long_rows, int32_t *t_item, float *t_rating,
                           int32_t *deg, int64_t *rowptr, uint32_t *long_tables, int64_t n_tables, int32_t *status, void *workspace,
                           int64_t workspace_bytes, void *stream);
int ngcf_laplacian_emit(const int64_t *old_rowptr, const int32_t *old_item, const float *old_rating, int64_t old_nnz,
                        const int64_t *bptr, int64_t T, const int32_t *t_item, const float *t_rating, int64_t n_user, int64_t n_item,
                        const int32_t *deg, const int64_t *rowptr, const float *ds, int64_t nnz, int32_t *s_item, float *s_rating,
                        int32_t *s_user, int32_t *colidx, float *vals, float *vals_item, uint64_t *zeros, int32_t *status, void *stream);
int ngcf_laplacian_item_rows(const int64_t *order, const int32_t *s_user, const float *vals_item, int64_t nnz, int32_t *colidx,
                             float *vals, int32_t *status, void *stream);
int ngcf_laplacian_drop_zeros(const int64_t *rowptr, const int32_t *colidx, const float *vals, int64_t n_rows, int64_t nnz,
                              int32_t *count, int64_t *out_rowptr, int32_t *out_colidx, float *out_vals, int64_t out_nnz,
                              void *workspace, int64_t workspace_bytes, void *stream);

/* ---- group-by-sum on packed integer keys, and the decimal string code (csrc/groupby.hip; the reference's pivot_table and
 * map_ids, utils.py:46-48, 59-97) ----
 * K <= 8 integer key columns (int32 or int64, length T) and V in 0..4 integer value columns, described by ngcf_groupby_cols_t (a
 * HOST struct; the kernels take it by value and read the columns themselves - no packed key array of length T exists anywhere).
 * Column k has an offset (its minimum), a range (maximum - minimum) and a field of key_bits[k] = bit length of the range (0 for a
 * single-valued column) at key_shift[k]; the fields are concatenated with column 0 most significant and the last column at shift 0,
 * so the unsigned order of the packed key is the lexicographic order of the columns.  The fields together have at most 63 bits: the
 * all-ones word means "empty slot".  A shift / bits / range triple that does not fit together is NGCF_ERR_ARG.
 *   ngcf_groupby_insert   clears the table (table_keys uint64[capacity] to all ones, table_sums int64[V x capacity] to 0, sum v of
 *        slot s at [v * capacity + s]) and inserts every row: home slot ngcf_groupby_hash(key) & (capacity - 1) - the 64-bit
 *        finaliser of MurmurHash3 (fmix64) - then linear probing with wrap-around; an empty slot is claimed by a 64-bit
 *        compare-and-swap at agent scope; the V values are added with int64 integer atomics (associative: the sums do not depend
 *        on arrival order; they wrap modulo 2^64 as int64 arithmetic does).  capacity is a power of two <= 2^36.  With
 *        lds_slots != 0 (a power of two in [16, max_lds_slots]) every workgroup first folds its rows - chunks of chunk_rows rows,
 *        chunk c to workgroup c mod grid - into a table of lds_slots keys and V sums in LDS (slot: bits 32.. of the same hash, at
 *        most lds_probes probes, 64-bit LDS atomics); a row that finds no place there goes straight to the table in memory, and
 *        the workgroup's LDS entries are inserted at its end.  The result does not depend on lds_slots.  ngcf_groupby_limits
 *        reports chunk_rows, lds_probes and max_lds_slots (any pointer may be NULL).
 *   ngcf_groupby_count    occupied slots per tile, their scan into the workspace, *n_groups (device int64) = G.
 *   ngcf_groupby_compact  keys[G] (the packed keys, as int64: they are < 2^63) and slots[G], in slot order; the workspace is the
 *        one ngcf_groupby_count filled.
 *      (caller: one library sort of the G keys -> sorted_keys, order.)
 *   ngcf_groupby_unpack   key_out[k][g] = column k of sorted_keys[g] (HOST arrays of K and V device pointers, int64[G] each),
 *        sum_out[v][g] = table_sums[v * capacity + slots[order[g]]], and, when table_rank (int64[capacity]) is not NULL,
 *        table_rank[slots[order[g]]] = g: the group's rank in ascending (column 0, column 1, ...) order beside its slot.
 *   ngcf_groupby_lookup   inverse[t] = table_rank[slot of row t's key], one probe sequence per row: numpy's
 *        unique(return_inverse=True).  The table is the dictionary; there is no search per row.
 * status (int32, sticky: bits are OR-ed in; zero it before ngcf_groupby_insert and ngcf_groupby_lookup, whose probe loops give up
 * once their bit is set):
 *   NGCF_GROUPBY_FULL   the table cannot hold the groups (run again with a larger capacity: a capacity >= 2 x groups never fails)
 *   NGCF_GROUPBY_RANGE  a value outside [offset, offset + range] of its column: the row is left out (inverse -1)
 *   NGCF_GROUPBY_LOST   arrays that do not belong together: a table changed between two calls, an order entry or slot out of range,
 *                       a row whose key is not in the table (inverse -1).  Nothing is read or written out of bounds.
 * workspace: ngcf_groupby_workspace_bytes(capacity) bytes, 8-byte aligned (-1 for a capacity that is no power of two <= 2^36).
 * Argument errors, before any launch (NGCF_ERR_ARG, message "groupby: ..."): a null pointer, a negative T, K or V out of range, a
 * bad capacity or lds_slots, n_groups outside [0, capacity]; NGCF_ERR_WORKSPACE for a workspace that is too small.
 *
 * ngcf_decimal_code: out[t] (int64) = the code of the string made of the decimal strings of row t's n_columns <= 8 columns (HOST
 * arrays: device pointers, is64 flags, widths), concatenated; widths[k] = 0: the value's natural length, w > 0: zero-padded on the
 * left to w characters.  Character c is the base-11 digit (c - '0') + 1, and the string is read as a left-aligned number of 18
 * places with padding 0, so the code's numeric order is the strings' lexicographic order (11^18 < 2^63).  status bits: 1 a
 * negative value, 2 a value with more digits than its fixed width, 4 more than 18 characters; such a row's code is -1.
 */
#define NGCF_GROUPBY_MAX_KEYS 8
#define NGCF_GROUPBY_MAX_VALUES 4
#define NGCF_GROUPBY_FULL 1
#define NGCF_GROUPBY_RANGE 2
#define NGCF_GROUPBY_LOST 4
typedef struct ngcf_groupby_cols {
    int32_t n_keys, n_values;
    const void *key[NGCF_GROUPBY_MAX_KEYS];        /* device, int32 or int64 [T] */
    const void *value[NGCF_GROUPBY_MAX_VALUES];    /* device, int32 or int64 [T] */
    int64_t key_offset[NGCF_GROUPBY_MAX_KEYS];
    uint64_t key_range[NGCF_GROUPBY_MAX_KEYS];
    int32_t key_is64[NGCF_GROUPBY_MAX_KEYS];
    int32_t key_bits[NGCF_GROUPBY_MAX_KEYS];
    int32_t key_shift[NGCF_GROUPBY_MAX_KEYS];
    int32_t value_is64[NGCF_GROUPBY_MAX_VALUES];
} ngcf_groupby_cols_t;
uint64_t ngcf_groupby_hash(uint64_t packed_key);
int ngcf_groupby_limits(int *chunk_rows, int *lds_probes, int *max_lds_slots);
int64_t ngcf_groupby_workspace_bytes(int64_t capacity);
int ngcf_groupby_insert(const ngcf_groupby_cols_t *cols, int64_t T, uint64_t *table_keys, int64_t *table_sums, int64_t capacity,
                        int lds_slots, int32_t *status, void *stream);
int ngcf_groupby_count(const uint64_t *table_keys, int64_t capacity, int64_t *n_groups, void *workspace, int64_t workspace_bytes,
                       void *stream);
int ngcf_groupby_compact(const uint64_t *table_keys, int64_t capacity, int64_t n_groups, int64_t *keys, int64_t *slots,
                         const void *workspace, int64_t workspace_bytes, int32_t *status, void *stream);
int ngcf_groupby_unpack(const ngcf_groupby_cols_t *cols, const int64_t *sorted_keys, const int64_t *order, const int64_t *slots,
                        const int64_t *table_sums, int64_t capacity, int64_t n_groups, int64_t *const *key_out, int64_t *const *sum_out,
                        int64_t *table_rank, int32_t *status, void *stream);
int ngcf_groupby_lookup(const ngcf_groupby_cols_t *cols, int64_t T, const uint64_t *table_keys, const int64_t *table_rank,
                        int64_t capacity, int64_t *inverse, int32_t *status, void *stream);
int ngcf_decimal_code(const void *const *columns, const int32_t *is64, const int32_t *widths, int n_columns, int64_t T, int64_t *out,
                      int32_t *status, void *stream);

/* ---- trip context (csrc/context.hip; the reference's congestion pivot and distance loop, demo.py:99-102, 241-248) ----
 * ngcf_segment_kahan_sum_f64: per segment u = order[rowptr[u] .. rowptr[u+1]) (positions into the value columns; order == NULL is
 * the identity: the rows are already grouped) and per value column k < n_values <= 4 (HOST arrays of device pointers: values[k]
 * double [T], sums[k] double [n_rows]) the compensated sum of pandas' group_sum, its recurrence in ascending position order:
 *   s = 0; c = 0
 *   for each v of the segment that is not a NaN:  y = v - c;  t = s + y;  c = (t - s) - y;  if c is a NaN: c = 0;  s = t
 *   sums[k][u] = s                                          (an empty or all-NaN segment: 0.0)
 * every operation an individually rounded fp64 one, never re-associated: the bits are pandas' (`pivot_table(aggfunc='sum')`,
 * `groupby().sum()`) when the positions of a segment are in row order.  Segments of fewer than wave_min rows (0: the default; any
 * positive value) are walked by one lane each; longer ones by one wave each, which fetches 64 rows at a time, coalesced through
 * `order`, and runs the chain on wave-uniform values read across the lanes.  Both tiers perform the same operations in the same
 * order: the result does not depend on wave_min, and, as no sum is touched by an atomic, not on the run.  *status is OR-ed into,
 * never cleared: 1 = a rowptr that decreases or leaves [0, T], or an order entry outside [0, T): never read through, that
 * segment's sums are NaN.  Argument errors, before any launch: n_values outside [1, 4], a negative wave_min or count, a null
 * pointer (`order` may be NULL; values[k] may be NULL when T == 0); n_rows == 0 is not an error.
 *
 * ngcf_haversine_table_f64: out[s * n_item + i] = the great-circle distance in metres between departure point s (dep double [S, 2])
 * and item i (item double [n_item, 2]), coordinates in degrees, the FIRST one taken as the latitude - the `haversine` package's
 * formula on the tuples the demo hands it, operation for operation:
 *   lat1, lng1, lat2, lng2 = x * (pi / 180)                 (CPython's math.radians)
 *   d   = sin((lat2 - lat1) * 0.5)^2 + (cos(lat1) * cos(lat2)) * sin((lng2 - lng1) * 0.5)^2
 *   out = ((2 * 6371.0088) * asin(sqrt(d))) * 1000          (2 * 6371.0088 folded on the host)
 * every product, sum and difference an individually rounded fp64 operation (no FMA), and sin, cos and asin the correctly rounded
 * ones (csrc/dd_math.h: double-double arithmetic out of IEEE add, multiply, fma, divide and sqrt, the same text on host and
 * device), so the table has the bits of a host whose maths library rounds these calls correctly - glibc does on all but a few
 * arguments in a thousand.  A result that is a NaN (a NaN coordinate; a d
 * that rounds above 1 at exact antipodes) is written as +inf: "missing, sorts last" to ngcf_topk_rows_f32 on the negated table.
 * One thread per output, items fastest; lat1 and cos(lat1) once per row and workgroup, cos(lat2) once per thread.  Argument
 * errors, before any launch: a negative count, a null pointer; S == 0 or n_item == 0 is not an error and writes nothing. */
int ngcf_segment_kahan_sum_f64(const int64_t *rowptr, int64_t n_rows, const int64_t *order, const double *const *values, int n_values,
                               int64_t T, int wave_min, double *const *sums, int32_t *status, void *stream);
int ngcf_haversine_table_f64(const double *dep, int64_t S, const double *item, int64_t n_item, double *out, void *stream);

/* ---- delimited text (csrc/text.hip; the reference's `pd.read_csv(path, sep='|')`, utils.py:38-39, for int and float columns) ----
 * The input is a uint8 [n] DEVICE buffer, 16-byte aligned.  The delimiter is one byte below 0x80 that is no digit, '+', '-', '.',
 * 'e', 'E', space, tab, CR, LF or '"'.  Quoting, comments, strings and dates are not supported.
 *
 * Rows.  Position p < n starts a row if (p == 0 or byte[p-1] == '\n') and the line is not blank; a line is blank if byte[p] == '\n',
 * or byte[p] == '\r' followed by '\n', or byte[p] == '\r' with p + 1 == n (pandas' skip_blank_lines).  A final line without a
 * newline is a row.  A row's text ends before its '\n' and before a '\r' directly in front of that - or, on a final line without a
 * newline, directly in front of the end of the buffer, the case the blank rule names.
 *   ngcf_text_count_rows  block_counts[b] (int64 [ceil(n / count_block_bytes)]) = the row starts among the bytes of block b; one
 *                         16-byte load per lane and step.  A '"' anywhere sets NGCF_TEXT_QUOTE.  (The caller scans the counts.)
 *   ngcf_text_row_starts  given block_offsets[b] = the rows before block b (the exclusive scan) and their total n_rows, writes
 *                         starts int64 [n_rows + 1]: the row starts in ascending order and starts[n_rows] = n.  A start whose rank is
 *                         not below n_rows (the buffer changed between the passes) is not written: NGCF_TEXT_LOST.
 *
 * ngcf_text_parse_columns: of the rows skip_rows .. n_rows - 1 of `starts` (the leading ones skipped are the header) and of the
 * n_fields <= 64 fields of every row, n_columns <= 16 are parsed: column s is field fields[s] of kind kinds[s] (0 int64, 1 float64;
 * HOST arrays; a field is selected at most once) and goes to out[s] (HOST array of device pointers, int64 or double
 * [n_rows - skip_rows]), one value per data row, written with ordinary stores.  One lane per row, a workgroup per run of
 * rows_per_workgroup rows: the run's bytes, up to lds_bytes of them, are brought into LDS with coalesced 16-byte loads, and a row
 * that does not end inside that window is walked straight from memory by its lane - the same code through a flat pointer, the same
 * results.  tier: 0 as described, 1 every row from memory, 2 as 0 and a row walked from memory sets NGCF_TEXT_TIER (tests, tools).
 * Spaces and tabs around a field are skipped.
 *   int64    [+-]?[0-9]+ ; an empty field, any other byte or a value outside int64 is an error, the overflow found exactly
 *            (-9223372036854775808 is a value).
 *   float64  [+-]?(digits[.digits?]|.digits)([eE][+-]?digits)? ; an empty field, nan, NaN and NA give NaN; [+-]?inf and
 *            [+-]?Infinity the infinities; any other byte is an error.  The decimal significand is gathered as an unsigned integer m
 *            (leading zeros stripped, at most 19 digits) with a decimal exponent e, so that the field is m * 10^e:
 *              m == 0                        a signed zero
 *              m <= 2^53 and |e| <= 22       m * 10^e (e >= 0) or m / 10^-e: ONE IEEE fp64 operation on two operands that are exact
 *                                            (a table of the powers), never contracted and never a reciprocal multiply, hence
 *                                            correctly rounded: the bits of strtod and of Python's float()
 *              anything else                 a SLOW field: NaN is written and (data row << 8) | column appended to slow_list
 *                                            (int64 [slow_capacity]) at the position an integer atomic counter hands out; the counter
 *                                            (status[2]) goes on counting past the capacity, so that the caller can size a second run.
 * status: int64 [4], 8-byte aligned, set by the caller to {0, -1, 0, 0} before the first of the three calls:
 *   status[0]  sticky bits, OR-ed in: NGCF_TEXT_FIELDS a row with fewer or more than n_fields fields (pandas pads the first case;
 *              both are refused here), NGCF_TEXT_BYTE a byte outside the grammar, NGCF_TEXT_EMPTY an empty int field,
 *              NGCF_TEXT_OVERFLOW an int outside int64, NGCF_TEXT_QUOTE a '"', NGCF_TEXT_LOST row starts that do not belong to
 *              the buffer (never read through: the row's columns are 0 / NaN), NGCF_TEXT_TIER (see tier)
 *   status[1]  the FIRST offending field as an unsigned word, (data row << 16) | (field << 8) | kind (NGCF_TEXT_KIND_*; a wrong
 *              field count has field 0; a field that holds a '"' reports that and nothing else), kept with an atomic minimum: the
 *              same on every run
 *   status[2]  the number of slow fields
 * A row with an error still has every selected column written (0 or NaN where there is nothing to parse).
 * Argument errors, before any launch (NGCF_ERR_ARG, message "text_...: ..."): a negative n, a null pointer, a buffer that is not
 * 16-byte aligned, a bad delimiter, n_fields outside [1, 64], n_columns outside [1, 16], a field index outside [0, n_fields) or
 * selected twice, a kind other than 0 and 1, skip_rows outside [0, n_rows], a tier outside [0, 2].  n == 0 is not an error.
 * ngcf_text_limits: rows_per_workgroup and lds_bytes of the parse, count_block_bytes of the two row passes. */
#define NGCF_TEXT_MAX_FIELDS 64
#define NGCF_TEXT_MAX_COLUMNS 16
#define NGCF_TEXT_KIND_FIELDS 1
#define NGCF_TEXT_KIND_BYTE 2
#define NGCF_TEXT_KIND_EMPTY 3
#define NGCF_TEXT_KIND_OVERFLOW 4
#define NGCF_TEXT_KIND_QUOTE 5
#define NGCF_TEXT_FIELDS 1
#define NGCF_TEXT_BYTE 2
#define NGCF_TEXT_EMPTY 4
#define NGCF_TEXT_OVERFLOW 8
#define NGCF_TEXT_QUOTE 16
#define NGCF_TEXT_LOST 32
#define NGCF_TEXT_TIER 64
int ngcf_text_limits(int *rows_per_workgroup, int *lds_bytes, int *count_block_bytes);
int ngcf_text_count_rows(const uint8_t *data, int64_t n, int64_t *block_counts, int64_t *status, void *stream);
int ngcf_text_row_starts(const uint8_t *data, int64_t n, const int64_t *block_offsets, int64_t n_rows, int64_t *starts, int64_t *status,
                         void *stream);
int ngcf_text_parse_columns(const uint8_t *data, int64_t n, const int64_t *starts, int64_t n_rows, int64_t skip_rows, int n_fields,
                            int delimiter, const int32_t *fields, const int32_t *kinds, int n_columns, void *const *out, int64_t *slow_list,
                            int64_t slow_capacity, int tier, int64_t *status, void *stream);

/* ---- exact per-group sampling (csrc/select.hip; the reference's Preprocess.split_train_test, utils.py:126-148) ----
 * From every group g of the T rows exactly quota[g] rows are marked, uniformly among all subsets of that size: pandas'
 * `sample(frac=, replace=False)` of a part of a frame (one group) and the per-class draws of sklearn's stratified split (one group
 * per class) - the reference's distribution, not numpy's stream.  Row t belongs to group group[t] (int32 [T], ids in [0, G); group ==
 * NULL: all rows in group 0, G must be 1); the groups need not be contiguous.  All arithmetic unsigned 64-bit:
 *   fmix(x): x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33      (as for ngcf_sample_unseen)
 *   k_t   = fmix(seed ^ (t * 0x9E3779B97F4A7C15))                                            (ngcf_select_key, a host call)
 *   tau_g = the quota[g]-th smallest k_t among the rows of group g                            (quota[g] > 0)
 *   mask[t] = quota[g] > 0 && k_t <= tau_g                                                    (uint8: 0 or 1)
 * Multiplying by an odd constant, xor with a constant and fmix are bijections on 64-bit words: the keys of distinct rows are
 * distinct, exactly quota[g] rows of group g qualify, and there is no tie to break.  Equal (seed, group, quota) give equal masks on
 * every run: the keys are recomputed from t in each pass and never stored, and the only atomics are integer counts.
 * tau is found by a radix select: eight passes from the most significant byte; in a pass every row whose key agrees with its
 * group's prefix so far counts into hist[g][next byte], and per group the bin that holds the remaining rank extends the prefix.
 * Up to lds_groups groups (ngcf_select_limits: the 160 KiB of a CU's LDS / 1 KiB per group) the G x 256 int32 table is kept in each
 * workgroup's LDS and flushed once per pass; above, the rows add straight into the table in memory.  The mask does not depend on the
 * tier (option "select_no_lds": the memory tier at every G; tests and tools).
 * thresholds (may be NULL): uint64 [G], tau_g, or 0 for a group with nothing marked.  quota: DEVICE int64 [G]; a quota <= 0 marks
 * nothing.  *status is OR-ed into, never cleared - zero it before the call, the marking pass looks at it:
 *   NGCF_SELECT_GROUP  a group id outside [0, G): the row counts nowhere, and the call marks no row at all
 *   NGCF_SELECT_QUOTA  quota[g] above the row count of group g (pandas and numpy raise there): no row of that group is marked
 *   NGCF_SELECT_LOST   the rows changed between two passes; nothing is read or written out of bounds
 * workspace: 16-byte aligned, workspace_bytes of ngcf_select_limits(G) - the G x 256 int32 table and 16 bytes of state per group,
 * 1 KiB + 16 B per group in both tiers (-1 for a G outside [1, 2^31)).  Argument errors, before any launch (NGCF_ERR_ARG, message
 * "select: ..."): T outside [0, 2^31) (the bins are int32), G outside [1, 2^31), group == NULL with G != 1 and T > 0, a null pointer (mask
 * may be NULL when T == 0), a misaligned workspace; NGCF_ERR_WORKSPACE for one that is too small.  T == 0 is not an error: a positive quota
 * then sets NGCF_SELECT_QUOTA. */
#define NGCF_SELECT_GROUP 1
#define NGCF_SELECT_QUOTA 2
#define NGCF_SELECT_LOST 4
int ngcf_select_limits(int64_t G, int *lds_groups, int64_t *workspace_bytes);
uint64_t ngcf_select_key(uint64_t seed, int64_t t);
int ngcf_select_per_group(const int32_t *group, int64_t T, int64_t G, const int64_t *quota, uint64_t seed, uint8_t *mask,
                          uint64_t *thresholds, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- Adam step (csrc/adam.hip; the reference's `optimizer.step()`, experiment.py:58, of main.py:74's torch.optim.Adam) ----
 * One launch per 32 tensors (NGCF_ADAM_MAX_TENSORS; more tensors, more launches of the same kernel) updates p, m = exp_avg,
 * v = exp_avg_sq in place from g and advances the tensors' step counters.  params, grads, exp_avgs, exp_avg_sqs, steps: HOST arrays
 * of n_tensors device pointers, numel a HOST array of element counts (int64; a tensor of 0 elements is skipped, its pointers not
 * looked at).  p, g, m, v are contiguous fp32 [numel[i]]; steps[i] is a float32 word, the steps taken so far - torch's capturable
 * format (`state["step"]`, a 0-dim float32 tensor on the device), exact up to 2^24 as there, and not guarded beyond.  The step words
 * of one call must be distinct.  The descriptors travel by value in the kernel arguments: no table in memory, no upload per step; a
 * captured launch is replayed as it stands, with lr, betas, eps and weight_decay baked in.
 * A workgroup of 256 threads takes one chunk of 4 096 elements of one tensor.  It reads its tensor's step word first, t = step + 1.
 * Scalars, once per workgroup, in fp64 with IEEE operations only (no pow):
 *   beta^t, in double-double (hi, lo), square-and-multiply on the integer t:
 *       r = (1, 0); b = (beta, 0); e = t
 *       while e > 0:  if e odd: r = mul(r, b);   e = e >> 1;   if e > 0: b = mul(b, b)
 *       beta^t = r.hi
 *     mul((a, al_), (b, bl_)), every operation rounded once, none contracted, S = 2^27 + 1:
 *       p = a * b;   c = S * a;  ah = c - (c - a);  al = a - ah;   c = S * b;  bh = c - (c - b);  bl = b - bh
 *       e = (((ah * bh - p) + ah * bl) + al * bh) + al * bl;       e = e + (a * bl_ + al_ * b)
 *       hi = p + e;   lo = e - (hi - p)
 *     (a plain fp64 chain of squarings doubles its relative error at every squaring: about t * 2^-53 at the end)
 *   bc1 = 1 - beta1^t;   step_size = -(lr / bc1);   bc2s = sqrt(1 - beta2^t)
 * step_size, bc2s, c1 = 1 - beta1, beta2, c2 = 1 - beta2, eps and wd = weight_decay are each rounded to fp32 once.
 * Per element, in fp32, every operation rounded once, none contracted, division and sqrt correctly rounded, denormals kept:
 *   g = maximize ? -g : g;          if (wd != 0) g = g + wd * p
 *   m = m + c1 * (g - m)
 *   v = v * beta2 + (c2 * g) * g
 *   d = sqrt(v) / bc2s + eps
 *   p = p + step_size * (m / d)
 * 16-byte loads and stores where p, g, m and v of a tensor are all 16-byte aligned, element by element otherwise and for the last
 * numel % 4 elements - through the same per-element function, the same bits.  tests/adam_oracle.py restates all of this on the host.
 * After its stores a workgroup takes a ticket from *ticket (a uint32 device word of the caller's, 0 before the first call) with an
 * integer atomic add; the workgroup that takes the launch's last ticket writes step + 1 to every tensor's step word and sets *ticket
 * back to 0.  Stream order shows the next launch the new steps.  No float atomics: equal inputs give equal bits on every run.
 * Argument errors, before any launch (NGCF_ERR_ARG, message "adam_step: ..."): a negative count, a null pointer, a pointer that is
 * not 4-byte aligned, a tensor of more than 2^31 / 32 chunks.  n_tensors == 0 is not an error. */
#define NGCF_ADAM_MAX_TENSORS 32
int ngcf_adam_step_f32(int n_tensors, void *const *params, const void *const *grads, void *const *exp_avgs, void *const *exp_avg_sqs,
                       void *const *steps, const int64_t *numel, uint32_t *ticket, double lr, double beta1, double beta2, double eps,
                       double weight_decay, int maximize, void *stream);

/* ---- multi-GPU row partition (new design; host-only helper) --------------- */
/*
 * Cut rows [row_begin, row_end) into `world` contiguous ranges of roughly equal stored-entry
 * count.  rowptr is a HOST int64[n_rows+1].  bounds is a HOST int64[world+1].
 */
int ngcf_shard_plan(const int64_t *rowptr_host, int64_t row_begin, int64_t row_end, int world,
                    int64_t *bounds_host);

/*
 * The exchange step between two layers of the row-partitioned engine (the reference is
 * single-device, NGCF.py has no counterpart): recv[q*rows_per_rank + k, :] = rank q's send[k, :] for every rank q of
 * the communicator - one ncclAllGather (RCCL over xGMI) of rows_per_rank*d floats per rank, asynchronous on `stream`.
 * `nccl_comm` is an ncclComm_t passed as void* (the Python mirror hands over its process group's communicator);
 * send: [rows_per_rank, d] contiguous, recv: [n_ranks*rows_per_rank, d] contiguous, both device pointers.  With the
 * padded rank-major numbering of dist.ShardLayout the received block IS the replica the next layer gathers from.
 * The library binds to the librccl already loaded in the process (it does not link one).
 */
int ngcf_allgather_rows(void *nccl_comm, const float *send, float *recv, int64_t rows_per_rank, int d, void *stream);
/* number of ranks of the communicator (host call) */
int ngcf_comm_size(void *nccl_comm, int *n_ranks);

/*
 * CU-free exchange between the ranks of one node (r03): copy engines move the bytes, host threads do the waiting, no kernel of
 * the exchange ever occupies a CU - the L2-swept SpMM keeps the chip to itself while the previous step's rows travel.
 * Every rank owns one exchange buffer; its producers write the rows the others need into it; the others PULL:
 *   ngcf_p2p_create   allocate the buffer (current device) and map the node's shared sequence words (POSIX shm `shm_name`, the
 *                     same name on every rank, unique per job)
 *   ngcf_p2p_handle   64-byte IPC handle of the buffer; the caller all-gathers the handles (host, any transport)
 *   ngcf_p2p_connect  open the peers' buffers (handles: world x 64 bytes, rank-major)
 *   ngcf_p2p_publish  on `stream`: everything enqueued so far is finished and visible to other devices when peers see `seq`
 *   ngcf_p2p_pull     host-wait (bounded) for rank `peer`'s `seq` in `slot`, then enqueue dst <- peer buffer[src_off, +bytes)
 *                     on this rank's copy stream for that peer (device-to-device: an SDMA engine across xGMI)
 *   ngcf_p2p_ack / ngcf_p2p_wait_acks   the reverse notice: a producer overwrites a region only after all peers have read it
 *   ngcf_p2p_fence    later copies start only after what `stream` holds now (the last readers of their destinations)
 *   ngcf_p2p_join     `stream` waits (stream dependency, no kernel) for every copy enqueued since the last join
 *   ngcf_p2p_stats    host time spent inside those waits so far, number of waits, number that found their word missing
 * `seq` must grow from call to call per slot (64 slots).  A wait that exceeds timeout_ms fails with NGCF_ERR_HIP.
 * Why the waiting is done by host threads and the publishing by a non-blocking host function (r04, tools/memops_lab.hip,
 * profiles/r04_memops_lab.txt): on this runtime hipStreamWriteValue64 / hipStreamWaitValue64 on host-registered memory, 8-byte
 * copies and event-less flag kernels are all SHADER work - beside a kernel that holds every CU (the L2-swept SpMM) none of them
 * starts before it ends (2.6 ms late beside a 2.65 ms kernel; a host function: 24 us), and a pending wait-value occupies a CU
 * (a one-workgroup-per-CU kernel launched behind it takes twice as long); a BLOCKING host function on a copy stream would take
 * the host out of the path, but the runtime runs every stream's host functions on one thread: a blocked one holds the
 * publishing ones of the same process (released only by its time-out).
 * ngcf_sum_slots_f32: out = slots[0] + slots[1] + ... (fixed order): the owner's side of a reduce-scatter done with pulls.
 */
typedef struct ngcf_p2p ngcf_p2p_t;
int ngcf_p2p_create(int rank, int world, int64_t bytes, const char *shm_name, ngcf_p2p_t **out);
void ngcf_p2p_destroy(ngcf_p2p_t *p2p);
int ngcf_p2p_handle(ngcf_p2p_t *p2p, void *handle64_host);
int ngcf_p2p_connect(ngcf_p2p_t *p2p, const void *handles_host);
void *ngcf_p2p_local(ngcf_p2p_t *p2p);
int64_t ngcf_p2p_bytes(const ngcf_p2p_t *p2p);
int ngcf_p2p_publish(ngcf_p2p_t *p2p, int slot, uint64_t seq, void *stream);
int ngcf_p2p_pull(ngcf_p2p_t *p2p, int peer, int slot, uint64_t seq, int64_t src_off, void *dst, int64_t bytes, double timeout_ms);
int ngcf_p2p_ack(ngcf_p2p_t *p2p, int peer, int slot, uint64_t seq);
int ngcf_p2p_wait_acks(ngcf_p2p_t *p2p, int slot, uint64_t seq, double timeout_ms);
int ngcf_p2p_fence(ngcf_p2p_t *p2p, void *stream);
int ngcf_p2p_join(ngcf_p2p_t *p2p, void *stream);
int ngcf_p2p_stats(ngcf_p2p_t *p2p, double *blocked_ms, int64_t *waits, int64_t *waits_blocked, int reset);
int ngcf_sum_slots_f32(const float *slots, int64_t slot_stride, int n_slots, int64_t n, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NGCF_HIP_H */
