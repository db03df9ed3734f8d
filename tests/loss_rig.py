"""What the GPU tests of the loss family (test_bpr_multi_gpu, test_sampled_softmax_gpu, test_softmax_full_gpu, test_inbatch_softmax_gpu)
share: the package, the device, the tolerance rule `held`, and the stand-in model of their "through the model" sections.  A plain
module: the files import the fixtures `dev` and `lap` by name.  tests/test_loss_rig.py makes `held` prove that it can fail."""
import numpy as np
import pytest
import torch

import ngcf_oracle as model_orc


def pkg():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def held(name, fused, other, want, ratios):
    """The measured tolerance for one tensor (or the loss): against the float64 oracle `want`, the fused kernels' largest absolute
    error may be twice that of the comparator `other` - the same float32 inputs through another order of sums - plus 4 ulp of
    float32 at the oracle's largest magnitude, which cover a comparator that happens to be exact:
        max |fused - want|  <=  2 * max |other - want|  +  4 ulp32(max |want|)
    -> None when it holds, else the message to fail with; `ratios[name]` keeps the largest error / bound seen.  `fused` must be
    finite and the three of one shape; an empty tensor (a gradient without rows) holds."""
    fused, other, want = (np.asarray(x, dtype=np.float64) for x in (fused, other, want))
    assert fused.shape == other.shape == want.shape, name
    assert np.isfinite(fused).all(), name
    if want.size == 0:
        return None
    e_f, e_x = np.abs(fused - want).max(), np.abs(other - want).max()
    bound = 2 * e_x + 4 * ulp32(np.abs(want).max())
    ratios[name] = max(ratios.get(name, 0.0), e_f / bound)
    return None if e_f <= bound else f"{name}: fused error {e_f:.3e}, comparator error {e_x:.3e}, bound {bound:.3e}"


# ---- the stand-in of the sections "through the model": 600 users, 30 items, three 65-wide layers, no dropout ---------------------
U, I = 600, 30
NUM = {"user": U, "item": I, "sex": 2, "age": 76, "month": 13, "day": 32, "dayofweek": 7}


@pytest.fixture(scope="module")
def lap(dev):
    return [pkg().graphs.to_sparse_coo(s) for s in pkg().graphs.seoul_standin(dev, seed=6, n_user=U, n_item=I)]


def batch(g, B, dev, m=None):
    """The model's inputs for B distinct users drawn from `g`; with `m` also `[B, m]` negative ids, drawn after them."""
    r = lambda hi, k=B: torch.randint(0, hi, (k,), generator=g).to(dev)  # noqa: E731
    b = dict(year=torch.full((B,), 18, device=dev), u_id=torch.randperm(U, generator=g)[:B].to(dev), age=r(76), sex=r(2),
             month=r(13), day=r(32), dow=r(7), pos_item=r(I))
    return b if m is None else (b, torch.randint(0, I, (B, m), generator=g).to(dev))


def model(pkg, lap, dev, B, auto):
    """A freshly seeded model in train mode with device-drawn dropouts; `auto` None leaves `auto_train_graph` at its default."""
    torch.manual_seed(4)
    model = pkg.NGCF(65, [65, 65, 65], 0.0, [0.0, 0.0, 0.0], 1.0, lap, NUM, B, dev).to(dev)
    model.node_dropout_mode = model.mess_dropout_mode = "device"
    if auto is not None:
        model.auto_train_graph = auto
    model.train()
    return model


def step_grads(model, forward_and_loss):
    """(loss, parameter gradients) of one step from cleared gradients; `forward_and_loss(model)` runs the forward and returns the loss."""
    model.zero_grad(set_to_none=True)
    loss = forward_and_loss(model)
    loss.backward()
    return loss.detach().clone(), {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}


def float64_leaves(model, lap):
    """(leaves, all_E): the model's tables and layer weights as float64 leaves on the host - read after a forward, so with the
    injected user rows - and the oracle's propagation of them; a file's `_model_oracle` puts its loss on top and calls `finish`."""
    sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith(("w1_list", "w2_list", "item_emb", "user_emb"))}
    w1, b1, w2, b2 = ([leaves[f"{w}_list.{k}.{x}"] for k in range(3)]
                      for w, x in (("w1", "weight"), ("w1", "bias"), ("w2", "weight"), ("w2", "bias")))
    L = lap[0].cpu().double().coalesce()
    return leaves, model_orc.propagate_torch(L, leaves["user_embedding.weight"], leaves["item_embedding.weight"], w1, b1, w2, b2)


def finish(loss, leaves):
    """(loss as a float, the float64 gradient of every leaf) after the oracle's backward."""
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in leaves.items()}
