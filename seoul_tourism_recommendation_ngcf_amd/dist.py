"""Multi-GPU propagation: one process per GPU, `torch.distributed` (backend "nccl" = RCCL over xGMI).

The reference is single-device; this is new design.  Rows of `L`, `E` and
`all_E` are independent given the previous layer's `E`, so the graph is row-partitioned and one exchange
step per layer moves embeddings between ranks.  Two exchange schemes share the same partition helpers:

``allgather`` (the north-star scheme, BASELINE config 4)
    Every rank owns a contiguous user range and a contiguous item range, both cut so that stored entries
    are balanced (`ngcf_shard_plan`).  The user range is cut again into `chunks` row chunks (balanced the same
    way).  Nodes are renumbered into a padded chunk-major / rank-major space (``ShardLayout``) so that ONE
    `all_gather_into_tensor` per chunk drops every rank's freshly computed carry rows straight into the replica
    the next layer gathers from - no unpack copies.  The layer is pipelined: chunk j's kernels are followed at once
    by chunk j's asynchronous all-gather, which runs on RCCL's stream while chunk j+1 computes; the layer waits
    only before the next layer's first read.  Bytes received per rank and layer: (W-1)/W * N * d * 4.

``bipartite`` (~10x fewer exchanged bytes; the default of bench.py at N > 1)
    `L = [[0, R], [R^T, 0]]` (matrix.py:49-52): user rows only read item embeddings and vice versa.
    Users are partitioned (by stored entries), the (small) item carry is replicated.  User rows are then fully local; item
    rows are partial sums over the local users, REDUCE-SCATTERED to the rank that owns the item, whose dense half runs
    there only, followed by an ALL-GATHER of the owned items' carry rows into every rank's item replica - the
    neighbour embeddings of the next layer's user rows.  Both exchanges overlap with SpMM kernels.  fp32 summation order
    differs from the single-GPU engine (tolerance, not bit-exact).

A rank never holds more of the graph than its own slabs: they are cut from the interaction triplets (host or
device tensors, `ShardedPropagation.from_interactions`) or from a row-sorted COO (`from_coo`).

Transport (`NGCF_DIST_COLLECTIVES`): "p2p" (default on device tensors) - the CU-free exchange of include/ngcf_hip.h
(`ngcf_p2p_*`: every rank's producers write into its own IPC-exported exchange buffer, the peers pull with device-to-device
copies on copy-engine streams, host threads wait on shared sequence words), which leaves every CU to the L2-swept SpMM;
"torch" - torch.distributed collectives (RCCL under "nccl"); "cabi" - `ngcf_allgather_rows` on the group's communicator.

Compute is always the HIP engine (the `engine` package); nothing here has a CPU path.  The layout/exchange helpers
are backend-agnostic tensor plumbing, which is what the world_size-2 `gloo` tests exercise on CPU tensors.

This module is the import path and holds no logic: the code lives in the package `multigpu`, one module per concern.  Callers reach
every name below as `dist.<name>`; `p2p` is imported here because `P2PExchange.TIMEOUT_MS` reads NGCF_P2P_TIMEOUT_MS when the
class is defined: when this module is first imported.
"""
from .multigpu.functions import (AllGatherRows, DenseLayerFn, OwnerRowsSum, ReduceScatterRows, SpmmFn, _SumGrads,  # noqa: F401
                                 allgather_rows, owner_rows_sum)
from .multigpu.p2p import P2PCollectives, P2PExchange  # noqa: F401
from .multigpu.partition import (ShardLayout, balanced_bounds, chunk_bounds, cut_slabs, even_bounds, laplacian_values,  # noqa: F401
                                 padded_item_pos, row_counts, slab_coo)
from .multigpu.sharded import SCHEME_NOTES, ShardedPropagation  # noqa: F401
