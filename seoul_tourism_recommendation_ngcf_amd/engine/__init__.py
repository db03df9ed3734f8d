"""Host side of the propagation engine: thin, typed wrappers over the C ABI (include/ngcf_hip.h), one module per kernel family.

Everything here hands `tensor.data_ptr()` + the current HIP stream to libngcf_hip.so.  torch is used for device memory and
streams only; no tensor arithmetic of the hot path happens in torch.  Importing the package neither loads the library nor touches
the device: `_lib.load()` runs inside the calls.  Callers reach every name below, the private ones included, as `engine.<name>`;
the backward pass (csrc/bwd_dense.hip, csrc/bwd_gather.hip: `engine.backward.<name>`, and `engine.layers.bpr_backward` next to `bpr_loss`),
the trip-context family (csrc/context.hip), the delimited-text family (csrc/text.hip), the optimizer step (csrc/adam.hip), the exact
held-out positions (csrc/rank_position.hip), the hard and the popularity-weighted negatives (csrc/sample_hard.hip, csrc/sample_weighted.hip), the loss against m negatives per positive
(csrc/bpr_multi.hip), the beyond-accuracy list figures with the diversifying re-rank (csrc/list_quality.hip, csrc/list_rerank.hip) and the certified
two-stage ranking (csrc/rank_prefilter.hip) keep their modules' names: `engine.context.<name>`,
`engine.text.<name>`, `engine.optim.<name>`, `engine.ranks.<name>`, `engine.negatives.<name>`, `engine.losses.<name>`,
`engine.lists.<name>`, `engine.shortlist.<name>`.
"""
import ctypes as C  # noqa: F401  (NGCF.py builds its pointers with `engine.C`)

from .. import _lib  # noqa: F401
from . import backward, context, layers, lists, losses, negatives, optim, ranks, shortlist, text  # noqa: F401
from ._plumbing import Workspace, _device_view, _f32c, _on, _ptr, _require_device, _row_major_ld, _stream
from .csr import LaplacianCSR, shard_plan
from .groupby import (DECIMAL_MAX_CHARS, GROUPBY_FULL, GROUPBY_LDS_SLOTS, GROUPBY_LOST, GROUPBY_MAX_KEYS, GROUPBY_MAX_VALUES,
                      GROUPBY_MIN_CAPACITY, GROUPBY_RANGE, Groups, _GroupbyCols, decimal_code, decimal_string, group_by, groupby_hash,
                      groupby_limits, groupby_packing)
from .laplacian import LAPLACIAN_LONG_TABLES, build_laplacian_year, empty_laplacian_state, inverse_sqrt_degree, laplacian_limits
from .layers import (LEAKY_SLOPE, bpr_loss, copy_rows, copy_rows_indexed, feature_inject, gather_rows, gather_rows3, layer_dense,
                     layer_fused, spmm, spmm_t_rows, spmm_t_rows_path)
from .ranking import (BLEND_POINTS_MAX, BLEND_TOP_MAX, CAND_MAX, RANK_K_MAX, ItemSets, blend_points, candidate_metrics_from_sums,
                      eval_candidates, metrics_from_sums, rank_topk, ranking_metrics, recommend_topk, topk_rows)
from .scaling import (QUANTILE_WAVE_MAX, segment_quantile_floor, segments_from_ids, yeo_johnson, yeo_johnson_launch,
                      yeo_johnson_moments)
from .selection import (SAMPLE_M_MAX, SELECT_GOLDEN, SELECT_GROUP, SELECT_LOST, SELECT_QUOTA, sample_unseen, select_key, select_limits,
                        select_per_group)
