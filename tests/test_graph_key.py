"""`graphed._param_ptrs`: the parameter addresses in the graph keys are read from the module as it is NOW (no GPU needed: the
addresses of CPU tensors serve as well)."""
import copy

import torch

import seoul_tourism_recommendation_ngcf_amd as pkg
from seoul_tourism_recommendation_ngcf_amd import graphed

NUM = {"user": 40, "item": 9, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}


def _model():
    lap = torch.sparse_coo_tensor(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0), (49, 49))
    torch.manual_seed(2)
    return pkg.NGCF(65, [65, 64], 0.3, [0.1, 0.1], 1.0, [lap], NUM, 8, "cpu")


def _walk(m):
    return tuple(p.data_ptr() for p in m.parameters())


def test_the_addresses_are_those_of_a_tree_walk_after_every_kind_of_replacement():
    m = _model()
    seen = [graphed._param_ptrs(m)]
    assert seen[-1] == _walk(m) and len(seen[-1]) == 15
    cache = m._plist
    old = m.item_embedding.weight                                       # (kept alive: its address cannot come back)
    m.item_embedding.weight = torch.nn.Parameter(old.detach() + 0.25)   # a Parameter: seen through the cached dicts
    seen.append(graphed._param_ptrs(m))
    assert m._plist is cache and seen[-1] == _walk(m) and seen[-1] != seen[-2]
    keep = [m.w1_list[1], m.user_embedding]
    m.w1_list[1] = torch.nn.Linear(65, 64)                              # a submodule inside a container: the cache is rebuilt
    seen.append(graphed._param_ptrs(m))
    assert m._plist is not cache and seen[-1] == _walk(m) and seen[-1] != seen[-2]
    cache = m._plist
    m.user_embedding = torch.nn.Embedding(40, 65)                       # a submodule of the model itself
    seen.append(graphed._param_ptrs(m))
    assert m._plist is not cache and seen[-1] == _walk(m) and seen[-1] != seen[-2]
    m.w2_list[0] = torch.nn.Linear(65, 65, bias=False)                  # a None entry among the parameters
    seen.append(graphed._param_ptrs(m))
    assert seen[-1] == _walk(m) and len(seen[-1]) == 14
    cache = m._plist
    assert graphed._param_ptrs(m) == seen[-1] and m._plist is cache     # nothing changed: nothing rebuilt
    twin = copy.deepcopy(m)                                             # a copy reads ITS parameters
    assert graphed._param_ptrs(twin) == _walk(twin) != seen[-1] and graphed._param_ptrs(m) == seen[-1]
    assert keep and old is not None


def test_train_eval_and_load_state_dict_drop_the_cache():
    m = _model()
    graphed._param_ptrs(m)
    for act in (m.eval, m.train, lambda: m.load_state_dict(m.state_dict()), lambda: m.to("cpu")):
        assert m._plist is not None
        act()
        assert m._plist is None
        assert graphed._param_ptrs(m) == _walk(m)
