"""Host side of the exact held-out positions: where the names live, argument checks before any launch, the C entry points' own
checks, the header, the slot vector's means."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sets(n_rows, n_items, pairs=((0, 1), (1, 0), (1, 2))):
    from seoul_tourism_recommendation_ngcf_amd import engine
    u = torch.tensor([p[0] for p in pairs])
    i = torch.tensor([p[1] for p in pairs])
    return engine.ItemSets.from_pairs(u, i, n_rows, n_items)


def test_ranks_is_a_module_of_engine_and_adds_no_flat_name():
    from seoul_tourism_recommendation_ngcf_amd import engine
    from seoul_tourism_recommendation_ngcf_amd.engine import ranks
    assert engine.ranks is ranks
    for name in ("rank_positions", "position_metrics", "position_metrics_from_sums"):
        assert callable(getattr(ranks, name)) and not hasattr(engine, name)
    assert ranks.POSITION_CAP == 64 and ranks.POSITION_WAVE_ROW == 64 and ranks.NOT_RANKED == -2
    header = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    assert re.search(r"#define NGCF_RANK_POS_CAP %d\b" % ranks.POSITION_CAP, header)
    assert re.search(r"#define NGCF_RANK_POS_WAVE_ROW %d\b" % ranks.POSITION_WAVE_ROW, header)


def test_header_declares_the_three_functions_and_keeps_version_11():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    assert "exact held-out positions" in header and "#define NGCF_ABI_VERSION 11" in header
    lib = _lib.load()
    for name, n_args in (("ngcf_rank_positions_workspace_bytes", 4), ("ngcf_rank_positions_f32", 21), ("ngcf_rank_position_metrics", 15)):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert hasattr(lib, name) and len(_lib.PROTOTYPES[name][1]) == n_args
    assert _lib.ABI_VERSION == 11 and lib.ngcf_version() == 11
    assert any(p.endswith("rank_position.hip") for p in _build.SOURCES)


def test_the_ranking_kernels_share_one_definition_of_order_split_and_sums():
    """By reading the sources: the pair order, the item split, the row search and the fixed-order sums stand once, in rank_device.h
    (the key map in common.h), and the header is part of the source hash."""
    from seoul_tourism_recommendation_ngcf_amd import _build
    csrc = os.path.join(ROOT, "seoul_tourism_recommendation_ngcf_amd", "csrc")
    assert any(p.endswith("rank_device.h") for p in _build.HEADERS)
    text = {f: open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".hip", ".h"))}
    sites = lambda words: sorted(f for f, t in text.items() for _ in range(t.count(words)))  # noqa: E731
    assert sites("n_items / (16 * ") == ["rank_device.h"]
    assert sites("(u & 0x80000000u) ? ~u") == ["common.h"]
    assert sites("void sum_partials_kernel(") == ["rank_device.h"]
    for f in ("rank.hip", "rank_position.hip"):
        assert '#include "rank_device.h"' in text[f] and "rank_item_split(" in text[f]
        assert "pair_before(" in text[f] and "row_has(" in text[f] and "launch_with_partial_sums(" in text[f]
    # ops.hip's recommend_topk_kernel, which the MFMA kernels are pinned against, keeps its own statement of the order on purpose
    assert sites("ka > kb || (ka == kb && ") == ["ops.hip", "rank_device.h"]
    for gone in ("rank_metrics_finish_kernel", "pos_metrics_finish_kernel", "list_diversity_finish_kernel", "rank_key(", "pos_key(",
                 "rank_before(", "pos_before(", "kPosPadKey"):
        assert not sites(gone), gone


def test_argument_errors_come_before_any_launch():
    from seoul_tourism_recommendation_ngcf_amd.engine import ranks
    truth = _sets(2, 5)
    u, items = torch.zeros(2, 4), torch.zeros(5, 4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ranks.rank_positions(u, items, truth)
    with pytest.raises(RuntimeError, match="cannot be multiplied"):
        ranks.rank_positions(u, items[:, :3], truth)
    with pytest.raises(RuntimeError, match="float32"):
        ranks.rank_positions(u.double(), items.double(), truth)
    with pytest.raises(TypeError, match="int64"):
        ranks.rank_positions(u, items, truth, user_ids=torch.tensor([0], dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        ranks.rank_positions(u, items, truth, out=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="3 entries"):
        ranks.rank_positions(u, items, truth, out=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="index 6 items"):
        ranks.rank_positions(u, items, _sets(2, 6))
    with pytest.raises(TypeError, match="ItemSets"):
        ranks.rank_positions(u, items, (torch.tensor([0]), torch.tensor([1])))
    pos = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ranks.position_metrics(pos, truth, [2], 5)
    with pytest.raises(TypeError, match="int32"):
        ranks.position_metrics(pos.long(), truth, [2], 5)
    with pytest.raises(ValueError, match="truth nnz"):
        ranks.position_metrics(pos[:2], truth, [2], 5)
    with pytest.raises(ValueError, match="at most 8"):
        ranks.position_metrics(pos, truth, list(range(1, 10)), 50)
    for bad in (0, 6):
        with pytest.raises(ValueError, match="outside"):
            ranks.position_metrics(pos, truth, [1, bad], 5)
    with pytest.raises(TypeError, match="int64"):
        ranks.position_metrics(pos, truth, [2], 5, user_ids=torch.tensor([0], dtype=torch.int32))


def test_c_entry_points_refuse_bad_arguments_with_a_message():
    from seoul_tourism_recommendation_ngcf_amd import _lib
    lib = _lib.load()
    assert lib.ngcf_rank_positions_workspace_bytes(4, 100, 8, 10) > 0
    assert lib.ngcf_rank_positions_workspace_bytes(0, 100, 8, 10) == 0
    bigger = lib.ngcf_rank_positions_workspace_bytes(4, 100, 8, 64 * 1000)
    assert bigger > lib.ngcf_rank_positions_workspace_bytes(4, 100, 8, 10)            # long rows are cut into more chunks
    for bad in ((-1, 100, 8, 10), (4, 0, 8, 10), (4, 2 ** 31, 8, 10), (4, 100, 0, 10), (4, 100, 8, -1)):
        assert lib.ngcf_rank_positions_workspace_bytes(*bad) == -1
    null = [None, 8, None, 4, 4, None, 8, 100, 8, None, None, 0, 10, None, None, 0, None, None, None, 0, None]
    assert lib.ngcf_rank_positions_f32(*null) == _lib.ERR_ARG and "rank_positions" in _lib.last_error()
    bad_items = list(null)
    bad_items[7] = 0
    assert lib.ngcf_rank_positions_f32(*bad_items) == _lib.ERR_ARG and "n_items" in _lib.last_error()
    ks = (C.c_int32 * 9)(*range(1, 10))
    assert lib.ngcf_rank_position_metrics(None, 4, None, 4, None, None, 3, None, 100, ks, 9, None, None, None, None) == _lib.ERR_ARG
    assert "cut-offs" in _lib.last_error()
    ks = (C.c_int32 * 1)(101)
    assert lib.ngcf_rank_position_metrics(None, 4, None, 4, None, None, 3, None, 100, ks, 1, None, None, None, None) == _lib.ERR_ARG
    assert "cut-off K=101" in _lib.last_error()
    ks = (C.c_int32 * 1)(20)
    assert lib.ngcf_rank_position_metrics(None, 4, None, 4, None, None, 3, None, 100, ks, 1, None, None, None, None) == _lib.ERR_ARG
    assert "bad argument" in _lib.last_error()


def test_position_metrics_from_sums_on_a_hand_made_vector():
    from seoul_tourism_recommendation_ngcf_amd.engine import ranks
    #        rr   ap   ndcg auc  | @5: recall ndcg prec hr | @70000                | users auc_users
    sums = [2.0, 1.0, 3.0, 1.5, 2.0, 1.0, 0.8, 4.0, 4.0, 3.0, 0.5, 4.0, 4.0, 3.0]
    got = ranks.position_metrics_from_sums(torch.tensor(sums, dtype=torch.float64), (5, 70000))
    assert got == {"mrr": 0.5, "map": 0.25, "ndcg": 0.75, "auc": 0.5, "recall@5": 0.5, "ndcg@5": 0.25, "precision@5": 0.2, "hr@5": 1.0,
                   "recall@70000": 1.0, "ndcg@70000": 0.75, "precision@70000": 0.125, "hr@70000": 1.0, "users": 4, "auc_users": 3}
    empty = ranks.position_metrics_from_sums([0.0] * 6, ())
    assert empty == {"mrr": 0.0, "map": 0.0, "ndcg": 0.0, "auc": 0.0, "users": 0, "auc_users": 0}
    with pytest.raises(ValueError, match="slots"):
        ranks.position_metrics_from_sums(sums, (5,))


def test_full_ranks_is_exported_beside_full_ranking():
    import inspect

    import seoul_tourism_recommendation_ngcf_amd as pkg
    assert callable(pkg.evaluate.full_ranks) and callable(pkg.evaluate.full_ranking)
    sig = inspect.signature(pkg.evaluate.full_ranks)
    assert list(sig.parameters) == ["model", "train", "test", "ks", "year_idx", "users", "user_chunk", "return_positions"]
    assert sig.parameters["ks"].default == (20,) and sig.parameters["user_chunk"].default == 65536
    assert sig.parameters["return_positions"].default is False
