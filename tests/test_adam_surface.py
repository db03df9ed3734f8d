"""CPU tests of the Adam step's surface: the C ABI, `engine.optim`, `optim.Adam`'s groups, refusals and state_dict exchange with
torch.optim.Adam.  Nothing here launches a kernel."""
import io
import os
import re

import pytest
import torch

from conftest import ROOT

TORCH_GROUP_KEYS = {"params", "lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused",
                    "decoupled_weight_decay"}


def _pkg():
    import seoul_tourism_recommendation_ngcf_amd as pkg
    return pkg


def _param(n=5, **kw):
    return torch.nn.Parameter(torch.arange(n, dtype=torch.float32), **kw)


def test_header_declares_the_step_and_the_abi_version_stays():
    from seoul_tourism_recommendation_ngcf_amd import _build, _lib
    text = open(os.path.join(ROOT, "include", "ngcf_hip.h")).read()
    assert re.search(r"\bint ngcf_adam_step_f32\(", text) and "#define NGCF_ABI_VERSION 11\n" in text
    assert "#define NGCF_ADAM_MAX_TENSORS 32\n" in text
    assert any(p.endswith("adam.hip") for p in _build.SOURCES)
    assert "ngcf_adam_step_f32" in _lib.PROTOTYPES and _lib.ABI_VERSION == 11
    lib = _lib.load()
    assert lib.ngcf_version() == 11 and hasattr(lib, "ngcf_adam_step_f32")
    # argument errors come back before any launch (no device is touched)
    assert lib.ngcf_adam_step_f32(0, None, None, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None) == _lib.OK
    assert lib.ngcf_adam_step_f32(-1, None, None, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None) == _lib.ERR_ARG
    assert lib.ngcf_adam_step_f32(1, None, None, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None) == _lib.ERR_ARG
    assert "adam_step" in _lib.last_error()


def test_engine_optim_is_a_module_of_its_own():
    pkg = _pkg()
    eng = pkg.engine
    assert eng.optim.__name__.endswith("engine.optim") and callable(eng.optim.adam_step) and eng.optim.ADAM_MAX_TENSORS == 32
    assert not hasattr(eng, "adam_step") and not hasattr(eng, "ADAM_MAX_TENSORS")
    assert "optim" in pkg.__all__ and issubclass(pkg.optim.Adam, torch.optim.Optimizer)


def test_engine_adam_step_checks_its_arguments_before_the_device():
    step = _pkg().engine.optim.adam_step
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False)
    f = lambda n=4, dtype=torch.float32: torch.zeros(n, dtype=dtype)  # noqa: E731
    ticket = torch.zeros(1, dtype=torch.int32)
    step([], [], [], [], [], ticket, **kw)                                        # nothing to do, nothing loaded
    with pytest.raises(ValueError, match="grads"):
        step([f()], [], [f()], [f()], [f(1)], ticket, **kw)
    with pytest.raises(TypeError, match="ticket"):
        step([f()], [f()], [f()], [f()], [f(1)], torch.zeros(1), **kw)
    with pytest.raises(TypeError, match="float32"):
        step([f()], [f(dtype=torch.float64)], [f()], [f()], [f(1)], ticket, **kw)
    with pytest.raises(TypeError, match="lr"):
        step([f()], [f()], [f()], [f()], [f(1)], ticket, **dict(kw, lr=torch.tensor(1e-3)))
    with pytest.raises(RuntimeError, match="ROCm device only"):                   # the engine has no CPU path
        step([f()], [f()], [f()], [f()], [f(1)], ticket, **kw)


def test_param_groups_carry_torchs_keys_and_say_capturable():
    pkg = _pkg()
    a, b = _param(), _param(3)
    opt = pkg.optim.Adam([{"params": [a]}, {"params": [b], "lr": 0.5, "weight_decay": 0.01}], lr=1e-2, maximize=True)
    ref = torch.optim.Adam([_param()], capturable=True)
    for g in opt.param_groups:
        assert set(g) == TORCH_GROUP_KEYS == set(ref.param_groups[0])
        assert g["capturable"] is True and g["foreach"] is None and g["fused"] is None and g["maximize"] is True
        assert g["amsgrad"] is False and g["differentiable"] is False and g["decoupled_weight_decay"] is False
    assert opt.param_groups[0]["lr"] == 1e-2 and opt.param_groups[1]["lr"] == 0.5 and opt.param_groups[1]["weight_decay"] == 0.01
    assert opt.defaults["betas"] == (0.9, 0.999) and opt.defaults["eps"] == 1e-8 and opt.defaults["lr"] == 1e-2
    assert len(opt.state) == 0                                                    # state is created on a parameter's first step
    with pytest.raises(ValueError, match="learning rate"):
        pkg.optim.Adam([_param()], lr=-1.0)
    with pytest.raises(ValueError, match="beta"):
        pkg.optim.Adam([_param()], betas=(0.9, 1.0))


def test_every_refusal_names_its_option():
    Adam = _pkg().optim.Adam
    refused = (NotImplementedError, TypeError)
    # visible at construction
    for opt_name in ("amsgrad", "decoupled_weight_decay", "differentiable"):
        with pytest.raises(refused, match=opt_name):
            Adam([_param()], **{opt_name: True})
        with pytest.raises(refused, match=opt_name):
            Adam([{"params": [_param()], opt_name: True}])
    with pytest.raises(refused, match="lr"):
        Adam([_param()], lr=torch.tensor(1e-3))
    with pytest.raises(refused, match="lr"):
        Adam([{"params": [_param()], "lr": torch.tensor(1e-3)}])
    for dtype in (torch.float64, torch.float16, torch.bfloat16, torch.complex64):
        with pytest.raises(refused, match=str(dtype)):
            Adam([torch.nn.Parameter(torch.zeros(3, dtype=dtype))])
    # a refused group leaves the optimizer as it was
    opt = Adam([_param()])
    with pytest.raises(refused, match="amsgrad"):
        opt.add_param_group({"params": [_param()], "amsgrad": True})
    assert len(opt.param_groups) == 1
    # visible at step()
    p = _param()
    opt = Adam([p])
    p.grad = torch.ones(5).to_sparse()
    with pytest.raises(refused, match="sparse"):
        opt.step()
    p.grad = torch.ones(5)
    with pytest.raises(refused, match="cpu"):                                     # a dense gradient of a CPU parameter
        opt.step()
    opt.found_inf = torch.zeros(())
    with pytest.raises(refused, match="found_inf"):
        opt.step()
    del opt.found_inf
    opt.param_groups[0]["amsgrad"] = True                                         # set behind the constructor's back
    with pytest.raises(refused, match="amsgrad"):
        opt.step()
    assert len(opt.state) == 0 and torch.equal(p.detach(), torch.arange(5.0))     # nothing was touched
    # a parameter without a gradient is not looked at: nothing to do, no device needed
    q = _param()
    assert Adam([q]).step() is None and Adam([q]).step(lambda: 3.5) == 3.5


def test_state_dict_key_sets_go_both_ways():
    """The key sets of `state_dict()` are torch's, and each class loads the other's (through torch.save / torch.load); a step counter
    that torch kept on the host arrives as a 0-dim float32 tensor, and the loaded groups say capturable again."""
    Adam = _pkg().optim.Adam
    p, q = _param(), _param()
    ref = torch.optim.Adam([p], lr=3e-3, weight_decay=0.01)
    p.grad = torch.ones(5)
    ref.step()
    ref.step()
    ours = Adam([q])
    assert set(ours.state_dict()) == set(ref.state_dict()) == {"state", "param_groups"}
    assert set(ours.state_dict()["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])
    buf = io.BytesIO()
    torch.save(ref.state_dict(), buf)
    buf.seek(0)
    ours.load_state_dict(torch.load(buf))
    st = ours.state[q]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} == set(ref.state[p])
    assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 2.0
    assert torch.equal(st["exp_avg"], ref.state[p]["exp_avg"]) and torch.equal(st["exp_avg_sq"], ref.state[p]["exp_avg_sq"])
    g = ours.param_groups[0]
    assert g["capturable"] is True and g["lr"] == 3e-3 and g["weight_decay"] == 0.01 and set(g) == TORCH_GROUP_KEYS
    # and back: a torch Adam built with capturable=True takes ours
    buf = io.BytesIO()
    torch.save(ours.state_dict(), buf)
    buf.seek(0)
    back = torch.optim.Adam([_param()], capturable=True)
    back.load_state_dict(torch.load(buf))
    r = back.param_groups[0]["params"][0]
    assert set(back.state[r]) == {"step", "exp_avg", "exp_avg_sq"} and float(back.state[r]["step"]) == 2.0
    assert torch.equal(back.state[r]["exp_avg"], st["exp_avg"]) and back.param_groups[0]["capturable"] is True
