"""The surface of the `engine` package: the names it exports, its constants and every public signature, pinned from the last commit
in which `engine` was one module, so that splitting or regrouping its wrappers cannot change what callers see."""
import ctypes
import inspect
import types

from seoul_tourism_recommendation_ngcf_amd import engine

PACKAGE = "seoul_tourism_recommendation_ngcf_amd"

CONSTANTS = {'BLEND_POINTS_MAX': 1024,
 'BLEND_TOP_MAX': 256,
 'CAND_MAX': 1024,
 'DECIMAL_MAX_CHARS': 18,
 'GROUPBY_FULL': 1,
 'GROUPBY_LDS_SLOTS': 1024,
 'GROUPBY_LOST': 4,
 'GROUPBY_MAX_KEYS': 8,
 'GROUPBY_MAX_VALUES': 4,
 'GROUPBY_MIN_CAPACITY': 64,
 'GROUPBY_RANGE': 2,
 'LAPLACIAN_LONG_TABLES': 16,
 'LEAKY_SLOPE': 0.2,
 'QUANTILE_WAVE_MAX': 64,
 'RANK_K_MAX': 256,
 'SAMPLE_M_MAX': 1023,
 'SELECT_GOLDEN': 11400714819323198485,
 'SELECT_GROUP': 1,
 'SELECT_LOST': 4,
 'SELECT_QUOTA': 2}

PUBLIC = CONSTANTS.keys() | {
    "Groups", "ItemSets", "LaplacianCSR", "Workspace", "blend_points", "bpr_loss", "build_laplacian_year", "candidate_metrics_from_sums",
    "copy_rows", "copy_rows_indexed", "decimal_code", "decimal_string", "empty_laplacian_state", "eval_candidates", "feature_inject",
    "gather_rows", "gather_rows3", "group_by", "groupby_hash", "groupby_limits", "groupby_packing", "inverse_sqrt_degree",
    "laplacian_limits", "layer_dense", "layer_fused", "metrics_from_sums", "rank_topk", "ranking_metrics", "recommend_topk",
    "sample_unseen", "segment_quantile_floor", "segments_from_ids", "select_key", "select_limits", "select_per_group", "shard_plan", "spmm",
    "spmm_t_rows", "spmm_t_rows_path", "topk_rows", "yeo_johnson", "yeo_johnson_launch", "yeo_johnson_moments",
}

# private names that the rest of the package, the tools and other tests reach as `engine.<name>`
PRIVATE = {"_GroupbyCols", "_device_view", "_f32c", "_lib", "_on", "_ptr", "_require_device", "_row_major_ld", "_stream"}

GROUPS_FIELDS = ('keys', 'sums', 'inverse')

# str(inspect.signature(f)) of every public function and of the methods of LaplacianCSR, ItemSets and Workspace ("property" for a property)
SIGNATURES = {'ItemSets.__init__': "(self, rowptr: 'torch.Tensor', colidx: 'torch.Tensor', col_offset: 'int', n_items: 'int', keep_alive=())",
 'ItemSets.from_laplacian': '(cls, csr: \'LaplacianCSR\', n_user: \'int\') -> "\'ItemSets\'"',
 'ItemSets.from_pairs': '(cls, users: \'torch.Tensor\', items: \'torch.Tensor\', n_user: \'int\', n_item: \'int\') -> "\'ItemSets\'"',
 'LaplacianCSR.__init__': "(self, handle: 'int', keep_alive=())",
 'LaplacianCSR.close': '(self)',
 'LaplacianCSR.filter_pos': 'property',
 'LaplacianCSR.filtered': "(self, keep: 'torch.Tensor', entry_map: 'Optional[torch.Tensor]' = None, nnz_kept: 'int' = -1, reuse: "
                          '"Optional[\'LaplacianCSR\']" = None) -> "\'LaplacianCSR\'"',
 'LaplacianCSR.from_coo': "(cls, rows: 'torch.Tensor', cols: 'torch.Tensor', vals: 'torch.Tensor', n_rows: 'int', n_cols: 'int')",
 'LaplacianCSR.from_csr_arrays': "(cls, rowptr: 'torch.Tensor', colidx: 'torch.Tensor', vals: 'torch.Tensor', n_cols: 'int')",
 'LaplacianCSR.from_sparse_coo': "(cls, L: 'torch.Tensor', device, row_range=None)",
 'LaplacianCSR.groups': "(self) -> 'list'",
 'LaplacianCSR.layer_workspace_bytes': "(self, d_in: 'int', d_out: 'int') -> 'int'",
 'LaplacianCSR.max_row_len': 'property',
 'LaplacianCSR.n_segments': 'property',
 'LaplacianCSR.plan': "(self, seg_len: 'int')",
 'LaplacianCSR.set_mode': "(self, mode: 'int')",
 'LaplacianCSR.spmm_workspace_bytes': "(self, d: 'int') -> 'int'",
 'LaplacianCSR.swept_rows': 'property',
 'Workspace.__init__': '(self)',
 'Workspace.get': "(self, nbytes: 'int', device) -> 'torch.Tensor'",
 'blend_points': "(pref: 'torch.Tensor', col_rowptr: 'torch.Tensor', col_rows: 'torch.Tensor', n_items: 'int', *, points: 'int' = 100, weights: "
                 "'Sequence[float]' = (1.0, 0.0, 0.0), con: 'Optional[torch.Tensor]' = None, con_slot: 'Optional[torch.Tensor]' = None, dis: "
                 "'Optional[torch.Tensor]' = None, dis_slot: 'Optional[torch.Tensor]' = None, item_mask: 'Optional[torch.Tensor]' = None, top: 'int' "
                 "= 10, tile_items: 'int' = 0, return_table: 'bool' = False, status: 'Optional[torch.Tensor]' = None)",
 'bpr_loss': "(u: 'torch.Tensor', p: 'torch.Tensor', n: 'torch.Tensor', weight_decay: 'float', batch_size: 'float', ws: 'Workspace') -> "
             "'torch.Tensor'",
 'build_laplacian_year': "(state, userid: 'torch.Tensor', itemid: 'torch.Tensor', rating: 'torch.Tensor', n_user: 'int', n_item: 'int')",
 'candidate_metrics_from_sums': "(sums, ks: 'Sequence[int]', hit_k: 'int' = 3) -> 'dict'",
 'copy_rows': "(src: 'torch.Tensor', dst: 'torch.Tensor', dst2: 'Optional[torch.Tensor]' = None)",
 'copy_rows_indexed': "(src: 'torch.Tensor', dst: 'torch.Tensor', idx: 'torch.Tensor')",
 'decimal_code': "(columns: 'Sequence[torch.Tensor]', widths: 'Sequence[int]') -> 'torch.Tensor'",
 'decimal_string': "(code: 'int') -> 'str'",
 'empty_laplacian_state': "(n_user: 'int', device)",
 'eval_candidates': "(user_emb: 'torch.Tensor', item_emb: 'torch.Tensor', user_ids: 'torch.Tensor', candidates: 'torch.Tensor', ratings: "
                    "'Optional[torch.Tensor]' = None, ks: 'Sequence[int]' = (10,), hit_k: 'int' = 3, weight_decay: 'float' = 0.0, batch_size: "
                    "'float' = 1.0, user_repeat: 'Optional[int]' = None, sums: 'Optional[torch.Tensor]' = None, status: 'Optional[torch.Tensor]' = "
                    "None, return_scores: 'bool' = False, return_position: 'bool' = True)",
 'feature_inject': "(user_w: 'torch.Tensor', tables: 'Sequence[torch.Tensor]', idx: 'Sequence[torch.Tensor]', u_id: 'torch.Tensor', emb_ratio: "
                   "'float', scratch: 'torch.Tensor', status: 'torch.Tensor')",
 'gather_rows': "(table: 'torch.Tensor', idx: 'torch.Tensor', status: 'torch.Tensor', row_off: 'int' = 0, n_idx_rows: 'Optional[int]' = None) -> "
                "'torch.Tensor'",
 'gather_rows3': "(table: 'torch.Tensor', sets, status: 'torch.Tensor')",
 'group_by': "(columns: 'Sequence[torch.Tensor]', values: 'Sequence[torch.Tensor]' = (), *, inverse: 'bool' = False, capacity: 'Optional[int]' = "
             "None, lds_slots: 'Optional[int]' = None, bounds: 'Optional[Sequence[Tuple[int, int]]]' = None) -> 'Groups'",
 'groupby_hash': "(key: 'int') -> 'int'",
 'groupby_limits': '()',
 'groupby_packing': "(bounds: 'Sequence[Tuple[int, int]]')",
 'inverse_sqrt_degree': "(deg: 'np.ndarray') -> 'np.ndarray'",
 'laplacian_limits': '()',
 'layer_dense': "(LE: 'torch.Tensor', E_self: 'torch.Tensor', W1, b1, W2, b2, carry, norm, ws: 'Workspace', drop_p: 'float' = 0.0, drop_seed: 'int' "
                "= 0, drop_mask: 'Optional[torch.Tensor]' = None)",
 'layer_fused': "(csr: 'LaplacianCSR', E_gather: 'torch.Tensor', E_self: 'torch.Tensor', W1, b1, W2, b2, carry: 'Optional[torch.Tensor]', norm: "
                "'torch.Tensor', ws: 'Workspace', drop_p: 'float' = 0.0, drop_seed: 'int' = 0, drop_mask: 'Optional[torch.Tensor]' = None)",
 'metrics_from_sums': "(sums: 'torch.Tensor', ks: 'Sequence[int]') -> 'dict'",
 'rank_topk': "(user_emb: 'torch.Tensor', item_emb: 'torch.Tensor', k: 'int', user_ids: 'Optional[torch.Tensor]' = None, exclude: "
              "'Optional[ItemSets]' = None, status: 'Optional[torch.Tensor]' = None)",
 'ranking_metrics': "(top_idx: 'torch.Tensor', truth: 'ItemSets', ks: 'Sequence[int]', user_ids: 'Optional[torch.Tensor]' = None, sums: "
                    "'Optional[torch.Tensor]' = None, per_user: 'bool' = False, status: 'Optional[torch.Tensor]' = None)",
 'recommend_topk': "(u_emb: 'torch.Tensor', item_emb: 'torch.Tensor', k: 'int', return_scores: 'bool' = False)",
 'sample_unseen': "(seen: 'ItemSets', user_ids: 'torch.Tensor', m: 'int', seed: 'int', *, first: 'Optional[torch.Tensor]' = None, case_offset: 'int' "
                  "= 0, out: 'Optional[torch.Tensor]' = None, status: 'Optional[torch.Tensor]' = None) -> 'torch.Tensor'",
 'segment_quantile_floor': "(rowptr: 'torch.Tensor', x: 'torch.Tensor', *, order: 'Optional[torch.Tensor]' = None, mean: 'float' = 0.0, scale: "
                           "'float' = 1.0, shift: 'float' = 0.0, q: 'float' = 0.25, wave_max: 'int' = 0, out: 'Optional[torch.Tensor]' = None, "
                           "quant: 'Optional[torch.Tensor]' = None, status: 'Optional[torch.Tensor]' = None)",
 'segments_from_ids': "(ids: 'torch.Tensor', n_rows: 'int')",
 'select_key': "(seed: 'int', t: 'int') -> 'int'",
 'select_limits': "(n_groups: 'int' = 1)",
 'select_per_group': "(group: 'Optional[torch.Tensor]', quota, *, seed: 'int', n_rows: 'Optional[int]' = None, return_thresholds: 'bool' = False, "
                     "out: 'Optional[torch.Tensor]' = None, device=None)",
 'shard_plan': "(rowptr_host: 'torch.Tensor', row_begin: 'int', row_end: 'int', world: 'int')",
 'spmm': "(csr: 'LaplacianCSR', E: 'torch.Tensor', out: 'Optional[torch.Tensor]' = None, ws: 'Optional[Workspace]' = None, edge_drop=None)",
 'spmm_t_rows': "(csr_t: 'LaplacianCSR', slot: 'torch.Tensor', X: 'torch.Tensor', init: 'Optional[torch.Tensor]', out: 'torch.Tensor', ws: "
                "'Workspace', edge_drop=None)",
 'spmm_t_rows_path': "(csr_t: 'LaplacianCSR', d: 'int', ws: 'Workspace', device) -> 'str'",
 'topk_rows': "(scores: 'torch.Tensor', k: 'int')",
 'yeo_johnson': "(x: 'torch.Tensor', lam: 'float', out: 'Optional[torch.Tensor]' = None) -> 'torch.Tensor'",
 'yeo_johnson_launch': "(T: 'int')",
 'yeo_johnson_moments': "(x: 'torch.Tensor', lam: 'float') -> 'torch.Tensor'"}


def _public_names():
    """What `engine` itself defines: no module, nothing imported from outside the package, no private name."""
    found = set()
    for name, value in vars(engine).items():
        if name.startswith("_") or isinstance(value, types.ModuleType):
            continue
        if isinstance(value, (int, float)) or str(getattr(value, "__module__", "")).startswith(PACKAGE):
            found.add(name)
    return found


def _signature(qualname):
    owner, _, attr = qualname.rpartition(".")
    if not owner:
        return str(inspect.signature(getattr(engine, attr)))
    member = vars(getattr(engine, owner))[attr]
    if isinstance(member, property):
        return "property"
    return str(inspect.signature(member.__func__ if isinstance(member, classmethod) else member))


def test_engine_exports_the_pinned_names_constants_and_signatures():
    assert _public_names() == set(PUBLIC)
    assert {name for name in PRIVATE if not hasattr(engine, name)} == set()
    assert {name: getattr(engine, name) for name in CONSTANTS} == CONSTANTS
    assert engine.Groups._fields == GROUPS_FIELDS
    assert engine._lib.__name__ == PACKAGE + "._lib" and engine.C is ctypes          # NGCF.py reaches ctypes as `engine.C`
    functions = {n for n in PUBLIC - CONSTANTS.keys() if not inspect.isclass(getattr(engine, n))}
    assert functions == {q for q in SIGNATURES if "." not in q}
    for cls in ("LaplacianCSR", "ItemSets", "Workspace"):
        members = {f"{cls}.{m}" for m, f in vars(getattr(engine, cls)).items()
                   if m == "__init__" or (not m.startswith("__") and (callable(f) or isinstance(f, (property, classmethod))))}
        assert members == {q for q in SIGNATURES if q.startswith(cls + ".")}
    assert {q: _signature(q) for q in SIGNATURES} == SIGNATURES
