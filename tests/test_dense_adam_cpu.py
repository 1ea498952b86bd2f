"""CPU: the dense Adam entry point (grut_adam_update / GrutDenseAdamGroup), its argument checks, and the Python class around it -
FusedAdam on host tensors takes torch's path with torch's state, interchanges state_dicts with torch.optim.Adam, adopts an existing
optimizer, and install_fused_adam() switches the reference model's optimizer (imported as tests/test_reference_seam_cpu.py does)."""
import copy
import ctypes as C
import importlib
import os
import subprocess
import sys
from unittest.mock import MagicMock

import numpy as np
import pytest
import torch

from test_reference_seam_cpu import REFERENCE, _REAL, _conf, _DictConfig, _GutRecorder, reference  # noqa: F401  (the reference fixture, its stubs and its ctypes fake)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
abi = importlib.import_module("3dgrut_amd._abi")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "threedgrut")),
                                     reason="the reference checkout is only present in the build container")
WIDTHS = (3, 1, 4, 3, 3, 45)


def _opt_mod():
    return importlib.import_module("3dgrut_amd.optimizers")


def test_entry_point_is_declared_and_exported(grut_lib):
    assert "grut_adam_update" in abi.EXPORTED_SYMBOLS and hasattr(grut_lib, "grut_adam_update")
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    assert "GrutDenseAdamGroup" in header and "grut_adam_update(" in header


def test_struct_mirror_matches_the_header(tmp_path):
    fields = [name for name, _ in abi.GrutDenseAdamGroup._fields_]
    assert fields == ["param", "grad", "exp_avg", "exp_avg_sq", "step", "numel", "lr", "beta1", "beta2", "eps", "weight_decay"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "grut_amd.h"\nint main(){printf("%zu", sizeof(GrutDenseAdamGroup));\n'
                   + "".join(f'printf(" %zu", offsetof(GrutDenseAdamGroup, {f}));\n' for f in fields) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.GrutDenseAdamGroup)] + [getattr(abi.GrutDenseAdamGroup, f).offset for f in fields]


def _group(**over):
    g = abi.GrutDenseAdamGroup()
    g.param, g.grad, g.exp_avg, g.exp_avg_sq, g.step = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000   # never dereferenced: every case is refused
    g.numel, g.lr, g.beta1, g.beta2, g.eps, g.weight_decay = 16, 1e-3, 0.9, 0.999, 1e-8, 0.0
    for k, v in over.items():
        setattr(g, k, v)
    return g


@pytest.mark.parametrize("case, word", [
    ("null_groups", "groups"), ("negative", "num_groups"), ("null_scratch", "scratch"),
    ("param", "param"), ("grad", "grad"), ("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq"), ("step", "step"),
    ("align_param", "param"), ("align_grad", "grad"), ("align_exp_avg", "exp_avg"), ("align_exp_avg_sq", "exp_avg_sq"),
])
def test_bad_input_is_refused_before_any_device_call(grut_lib, case, word):
    scratch = C.c_void_p(0x6000)
    ok = (abi.GrutDenseAdamGroup * 2)(_group(), _group())
    if case == "null_groups":
        status = grut_lib.grut_adam_update(None, None, 2, scratch)
    elif case == "negative":
        status = grut_lib.grut_adam_update(None, ok, -1, scratch)
    elif case == "null_scratch":
        status = grut_lib.grut_adam_update(None, ok, 2, None)
    elif case.startswith("align_"):
        field = case[len("align_"):]
        status = grut_lib.grut_adam_update(None, (abi.GrutDenseAdamGroup * 2)(_group(), _group(**{field: 0x1004})), 2, scratch)
    else:   # a NULL pointer in the SECOND group: nothing may have been launched for the first
        status = grut_lib.grut_adam_update(None, (abi.GrutDenseAdamGroup * 2)(_group(), _group(**{case: None})), 2, scratch)
    assert abi.STATUS_NAMES[status] == "BAD_INPUT"
    message = grut_lib.grut_last_error().decode()
    assert "grut_adam_update" in message and word in message, message
    if case.startswith("align_") or case in ("param", "grad", "exp_avg", "exp_avg_sq", "step"):
        assert "group 1" in message, message


def test_empty_groups_and_no_groups_are_accepted_without_a_device(grut_lib):
    scratch = C.c_void_p(0x6000)
    assert grut_lib.grut_adam_update(None, None, 0, scratch) == abi.GRUT_OK
    empty = (abi.GrutDenseAdamGroup * 1)(_group(numel=0, param=None, grad=None, exp_avg=None, exp_avg_sq=None, step=None))
    assert grut_lib.grut_adam_update(None, empty, 1, scratch) == abi.GRUT_OK   # skipped: nothing to launch


def _host_params(seed=0, n=37):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn((n, w), generator=g)) for w in WIDTHS]


def _groups(params):
    return [{"params": [p], "lr": 1e-3 * (i + 1), "name": f"g{i}"} for i, p in enumerate(params)]


def _set_grads(params, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)


def test_host_tensors_take_torchs_path_bit_for_bit():
    mod = _opt_mod()
    mine, theirs = _host_params(), _host_params()
    a = mod.FusedAdam(_groups(mine), lr=0.0, eps=1e-15, fused=True)    # the call of model.py:808-810
    b = torch.optim.Adam(_groups(theirs), lr=0.0, eps=1e-15, fused=True)
    before = dict(mod.stats)
    for s in range(5):
        _set_grads(mine, s)
        _set_grads(theirs, s)
        a.step()
        b.step()
    assert mod.stats["torch_steps"] == before["torch_steps"] + 5 and mod.stats["hip_steps"] == before["hip_steps"]
    for p, q in zip(mine, theirs):
        assert torch.equal(p, q)
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a.state[p][key], b.state[q][key]) and a.state[p][key].dtype == b.state[q][key].dtype
        assert a.state[p]["step"].dim() == 0 and a.state[p]["step"].dtype == torch.float32


def test_constructor_accepts_what_adam_accepts():
    mod = _opt_mod()
    p = torch.nn.Parameter(torch.zeros(4))
    opt = mod.FusedAdam([p], 1e-2, (0.8, 0.9), 1e-6, 0.01, False, maximize=False, capturable=False, differentiable=False, fused=None)
    assert isinstance(opt, torch.optim.Adam) and opt.defaults["fused"] is True and opt.param_groups[0]["betas"] == (0.8, 0.9)
    assert opt.param_groups[0]["weight_decay"] == 0.01 and opt.param_groups[0]["eps"] == 1e-6


def _same_state_dict(x, y):
    assert x["param_groups"] == y["param_groups"]
    assert x["state"].keys() == y["state"].keys()
    for k in x["state"]:
        assert x["state"][k].keys() == y["state"][k].keys()
        for name in x["state"][k]:
            s, t = x["state"][k][name], y["state"][k][name]
            assert s.shape == t.shape and s.dtype == t.dtype and s.device == t.device and torch.equal(s, t), (k, name)


@pytest.mark.parametrize("direction", ["torch_to_fused", "fused_to_torch"])
def test_state_dict_round_trips_with_torch_adam(direction):
    mod = _opt_mod()
    make = {"torch": lambda ps: torch.optim.Adam(_groups(ps), lr=0.0, eps=1e-15, fused=True),
            "fused": lambda ps: mod.FusedAdam(_groups(ps), lr=0.0, eps=1e-15)}
    src_kind, dst_kind = ("torch", "fused") if direction == "torch_to_fused" else ("fused", "torch")
    src_params, dst_params = _host_params(), _host_params()
    src, dst = make[src_kind](src_params), make[dst_kind](dst_params)
    for s in range(2):
        _set_grads(src_params, s)
        src.step()
    sd = copy.deepcopy(src.state_dict())
    dst.load_state_dict(sd)
    _same_state_dict(dst.state_dict(), src.state_dict())
    with torch.no_grad():
        for p, q in zip(dst_params, src_params):
            p.copy_(q)
    _set_grads(src_params, 7)
    _set_grads(dst_params, 7)
    src.step()
    dst.step()
    for p, q in zip(dst_params, src_params):
        assert torch.equal(p, q)
    _same_state_dict(dst.state_dict(), src.state_dict())


@pytest.mark.parametrize("flavour", [{}, {"foreach": True}, {"fused": True}])
def test_adopt_keeps_groups_and_state_and_moves_a_host_step(flavour):
    mod = _opt_mod()
    params, twin = _host_params(), _host_params()
    old = torch.optim.Adam(_groups(params), lr=0.0, eps=1e-15, **flavour)
    check = torch.optim.Adam(_groups(twin), lr=0.0, eps=1e-15, **flavour)
    _set_grads(params, 0)
    _set_grads(twin, 0)
    old.step()
    check.step()
    group_ids, state_ids = [id(g) for g in old.param_groups], {id(p): id(old.state[p]["exp_avg"]) for p in params}
    new = mod.FusedAdam.adopt(old)
    assert type(new) is mod.FusedAdam and mod.FusedAdam.adopt(new) is new
    assert new.param_groups is old.param_groups and [id(g) for g in new.param_groups] == group_ids
    assert new.state is old.state and {id(p): id(new.state[p]["exp_avg"]) for p in params} == state_ids
    for g in new.param_groups:
        assert g["fused"] is True and g["foreach"] is None
    for p in params:
        step = new.state[p]["step"]
        assert torch.is_tensor(step) and step.dtype == torch.float32 and step.dim() == 0 and step.device == p.device and float(step) == 1.0
    for s in range(1, 4):   # the adopted optimizer goes on where the old one stood (the moments agree to the flavours' rounding)
        _set_grads(params, s)
        _set_grads(twin, s)
        new.step()
        check.step()
    for p, q in zip(params, twin):
        assert float(new.state[p]["step"]) == 4.0
        torch.testing.assert_close(p, q, rtol=1e-5, atol=1e-6)
    with pytest.raises(TypeError):
        mod.FusedAdam.adopt(torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=0.1))


@pytest.mark.parametrize("scheduler", ["exponential", "cosine"])
def test_adopt_after_an_lr_scheduler_was_attached(scheduler):
    """trainer.py:573-590 builds the decoder's Adam and its ExponentialLR / CosineAnnealingLR in one function, so a user adopts an
    optimizer whose instance already carries the scheduler's `step`.  The adopted optimizer must run ITS step (a stats counter
    moves), advance the shared state, see the scheduler's rates, and keep the scheduler's order-of-calls warning quiet - also once
    the old optimizer object is gone."""
    import gc
    import warnings
    mod = _opt_mod()
    params = _host_params()
    old = torch.optim.Adam(_groups(params), lr=0.0, eps=1e-15)
    sched = (torch.optim.lr_scheduler.ExponentialLR(old, gamma=0.5) if scheduler == "exponential"
             else torch.optim.lr_scheduler.CosineAnnealingLR(old, T_max=4, eta_min=0.0))
    assert "step" in old.__dict__   # what the scheduler installed
    _set_grads(params, 0)
    old.step()
    new = mod.FusedAdam.adopt(old)
    assert getattr(new.step, "_wrapped_by_lr_sched", False) and new.step is not old.__dict__["step"]
    before, start = dict(mod.stats), [p.detach().clone() for p in params]
    _set_grads(params, 1)
    new.step()
    assert mod.stats["torch_steps"] + mod.stats["hip_steps"] == before["torch_steps"] + before["hip_steps"] + 1
    assert all(float(new.state[p]["step"]) == 2.0 for p in params)
    assert all(not torch.equal(p, q) for p, q in zip(params, start))
    rates = [g["lr"] for g in new.param_groups]
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # "lr_scheduler.step() before optimizer.step()" would be raised here
        sched.step()
    assert [g["lr"] for g in new.param_groups] != rates and [g["lr"] for g in new.param_groups] == sched.get_last_lr()
    # the rate the next step uses is the scheduler's: a twin with those rates written by hand lands on the same bits
    twin = [torch.nn.Parameter(p.detach().clone()) for p in params]
    check = mod.FusedAdam(_groups(twin), lr=0.0, eps=1e-15)
    sd = copy.deepcopy(new.state_dict())
    check.load_state_dict(sd)
    for g, lr in zip(check.param_groups, sched.get_last_lr()):
        g["lr"] = lr
    _set_grads(params, 2)
    _set_grads(twin, 2)
    new.step()
    check.step()
    for p, q in zip(params, twin):
        assert torch.equal(p, q)
    del old, sched
    gc.collect()
    _set_grads(params, 3)
    new.step()   # no reference to the adopted-from object is needed any more
    assert all(float(new.state[p]["step"]) == 4.0 for p in params)


def test_adopt_without_a_scheduler_puts_no_step_on_the_instance():
    mod = _opt_mod()
    old = torch.optim.Adam(_groups(_host_params()), lr=1e-3)
    assert "step" not in mod.FusedAdam.adopt(old).__dict__


def test_step_hooks_run_once_per_step_on_torchs_path():
    mod = _opt_mod()
    torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))])   # makes torch wrap Adam.step with its hook runner
    p = torch.nn.Parameter(torch.ones(3))
    opt = mod.FusedAdam([p], lr=1e-2)
    calls = []
    opt.register_step_pre_hook(lambda *a: calls.append("pre"))
    opt.register_step_post_hook(lambda *a: calls.append("post"))
    p.grad = torch.ones(3)
    loss = opt.step(lambda: torch.tensor(2.0))
    assert calls == ["pre", "post"] and float(loss) == 2.0


# ---- the reference's model ------------------------------------------------------------------------------------------------------
LRS = {"positions": 0.00016, "density": 0.05, "features_albedo": 0.0025, "features_specular": 0.0025 / 20, "rotation": 0.001, "scale": 0.005}


def _model(monkeypatch, optimizer_type, scene_extent=2.5):
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    _REAL.update(gut=gt._GutNative)
    monkeypatch.setattr(gt, "_GutNative", _GutRecorder)
    model_mod = importlib.import_module("threedgrut.model.model")
    conf = _conf("3dgut")
    conf["optimizer"] = {"type": optimizer_type, "lr": 0.0, "eps": 1e-15,
                         "params": {**{k: {"lr": v} for k, v in LRS.items()}, "features": {"lr": 0.015}}}   # configs/base_gs.yaml:134-152
    conf["scheduler"] = {"positions": _DictConfig({"type": "exp", "lr_init": 0.00016, "lr_final": 0.0000016, "max_steps": 30000}),
                         "density": _DictConfig({"type": "skip"})}
    mog = model_mod.MixtureOfGaussians(conf, scene_extent=scene_extent)
    g = torch.Generator().manual_seed(0)
    P, n = torch.nn.Parameter, 23
    mog.positions, mog.rotation = P(torch.randn((n, 3), generator=g)), P(torch.randn((n, 4), generator=g))
    mog.scale, mog.density = P(torch.randn((n, 3), generator=g) - 3), P(torch.randn((n, 1), generator=g))
    mog.features_albedo, mog.features_specular = P(torch.rand((n, 3), generator=g)), P(torch.zeros((n, 45)))
    return model_mod, mog


@needs_reference
def test_install_switches_the_reference_models_adam(reference, monkeypatch):
    mod = _opt_mod()
    model_mod, mog = _model(monkeypatch, "adam")
    original = model_mod.MixtureOfGaussians.setup_optimizer
    mog.setup_optimizer()
    assert type(mog.optimizer) is torch.optim.Adam            # nothing changes unless the installer is called
    replaced = mod.install_fused_adam()
    assert replaced is original
    wrapped = model_mod.MixtureOfGaussians.setup_optimizer
    assert wrapped is not original
    assert mod.install_fused_adam() is original and model_mod.MixtureOfGaussians.setup_optimizer is wrapped   # idempotent

    mog.setup_optimizer()
    opt = mog.optimizer
    assert type(opt) is mod.FusedAdam
    assert [g["name"] for g in opt.param_groups] == list(LRS)
    for g in opt.param_groups:
        assert g["lr"] == pytest.approx(LRS[g["name"]] * (2.5 if g["name"] == "positions" else 1.0), rel=1e-12)
        assert g["eps"] == 1e-15 and g["fused"] is True and g["params"][0] is getattr(mog, g["name"])
    assert set(mog.schedulers) == {"positions", "density"}

    # a step moves positions by the scheduled rate: Adam's first step is lr * sign(grad) up to eps
    mog.scheduler_step(15000)
    lr_now = {g["name"]: g["lr"] for g in opt.param_groups}["positions"]
    assert lr_now == pytest.approx(2.5 * np.sqrt(0.00016 * 0.0000016), rel=1e-9)
    before = mog.positions.detach().clone()
    for name in LRS:
        getattr(mog, name).grad = torch.ones_like(getattr(mog, name))
    count = mod.stats["torch_steps"]
    opt.step()
    assert mod.stats["torch_steps"] == count + 1              # host tensors: torch's path
    moved = (before - mog.positions.detach()).numpy()   # each difference carries the rounding of its two fp32 positions
    np.testing.assert_allclose(moved, lr_now, rtol=1e-5, atol=float(np.spacing(np.abs(before.numpy()).max())))

    # a checkpoint's optimizer state goes through the reference's own load_state_dict and is adopted with it
    sd = copy.deepcopy(opt.state_dict())
    mog.setup_optimizer(state_dict=sd)
    assert type(mog.optimizer) is mod.FusedAdam and mog.optimizer is not opt
    step = mog.optimizer.state[mog.positions]["step"]
    assert float(step) == 1.0 and step.dtype == torch.float32
    assert torch.equal(mog.optimizer.state[mog.features_specular]["exp_avg"], opt.state[mog.features_specular]["exp_avg"])


@needs_reference
def test_install_leaves_selective_adam_configs_alone(reference, monkeypatch):
    mod = _opt_mod()
    monkeypatch.setitem(sys.modules, "threedgrut.optimizers.lib_optimizers_cc", MagicMock())   # the reference's CUDA plugin, loaded by its constructor
    model_mod, mog = _model(monkeypatch, "selective_adam")
    mod.install_fused_adam()
    mog.setup_optimizer()
    assert type(mog.optimizer) is model_mod.SelectiveAdam and not isinstance(mog.optimizer, mod.FusedAdam)
    assert [g["name"] for g in mog.optimizer.param_groups] == list(LRS)
