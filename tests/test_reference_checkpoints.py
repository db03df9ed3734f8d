"""The 23 checkpoints shipped with the reference load into the mirror module with strict=True.
Their structure (state-dict names in order, shapes, dtypes, the last layer's w2 bias) is stored in
tests/golden/reference_checkpoints.npz (oracle/make_golden.py); the weights are seeded stand-ins of those shapes."""
import numpy as np
import torch

from conftest import load_golden


def _state_dicts():
    g = load_golden("reference_checkpoints")
    gen = torch.Generator().manual_seed(0)
    for i, path in enumerate(g["files"]):
        sd = {}
        for name, shape, dtype in zip(g[f"c{i}_names"], g[f"c{i}_shapes"], g[f"c{i}_dtypes"]):
            sd[str(name)] = torch.randn(tuple(int(s) for s in shape if s >= 0), generator=gen).to(getattr(torch, str(dtype)))
        n_layer = sum(1 for k in sd if k.startswith("w1_list.") and k.endswith(".weight"))
        sd[f"w2_list.{n_layer - 1}.bias"] = torch.from_numpy(np.array(g[f"c{i}_last_bias"]))
        yield str(path), sd


def test_all_reference_checkpoints_load_strict():
    from seoul_tourism_recommendation_ngcf_amd import NGCF
    ckpts = list(_state_dicts())
    assert len(ckpts) == 23
    num_dict = {"user": 5840, "item": 100, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}   # num_dict.pkl
    sigs = set()
    for path, sd in ckpts:
        n_layer = sum(1 for k in sd if k.startswith("w1_list.") and k.endswith(".weight"))
        layers = [int(sd[f"w1_list.{k}.weight"].shape[0]) for k in range(n_layer)]
        embed = int(sd["user_embedding.weight"].shape[1])
        model = NGCF(embed, layers, 0.3, [0.1] * n_layer, 1.0, [], num_dict, 512, torch.device("cpu"))
        assert list(model.state_dict().keys()) == list(sd.keys()), path
        model.load_state_dict(sd, strict=True)
        assert torch.equal(model.w2_list[n_layer - 1].bias, sd[f"w2_list.{n_layer - 1}.bias"])
        sigs.add((n_layer, tuple(layers)))
    assert sigs == {(2, (65, 65)), (3, (65, 65, 65)), (3, (64, 64, 64))}          # Sig-A, Sig-B, Sig-C
