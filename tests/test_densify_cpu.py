"""CPU: the default strategy's five C-ABI entry points are declared, mirrored and exported, the Python surface rejects host tensors
before anything is launched, and the seam with the reference's own `threedgrut.strategy.gs` holds: `install_fused_gs_strategy()`
swaps in a subclass that hands the model's own tensors to the three device functions and leaves the model, the optimizer and the
densification buffers exactly as the unmodified reference class leaves them.  What the kernels compute is covered by
tests/test_densify_gpu.py."""
import copy
import importlib
import os
import re
import sys

import pytest
import torch

import densify_reference as restated
from test_reference_seam_cpu import REFERENCE, _REAL, _conf, _DictConfig, _GutRecorder, reference  # noqa: F401  (the reference fixture, its stubs and its ctypes fake)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("grut_densify_accumulate", "grut_relayout_scan", "grut_relayout_rows", "grut_split_tail")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "threedgrut")),
                                     reason="the reference checkout is only present in the build container")


def test_densify_symbols_are_declared_mirrored_and_exported(grut_lib):
    abi = importlib.import_module("3dgrut_amd._abi")
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(void\* stream, uint32_t n,", header), name
    assert re.search(r"\buint64_t grut_relayout_scratch_bytes\(uint32_t n\);", header)
    for name in NEW_SYMBOLS + ("grut_relayout_scratch_bytes",):
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(grut_lib, name) and getattr(grut_lib, name).argtypes, name
    assert re.search(r"GRUT_APPEND_COPY\s*=\s*0", header) and re.search(r"GRUT_APPEND_ZERO\s*=\s*1", header)
    densify = importlib.import_module("3dgrut_amd.densify")
    assert (densify.APPEND_COPY, densify.APPEND_ZERO) == (0, 1)
    assert "densify.hip" in importlib.import_module("3dgrut_amd.build").SOURCES
    assert abi.ABI_VERSION == 5 and grut_lib.grut_abi_version() == 5
    # two flag arrays and the scan's block sums: grows with n, never below the scan's own need
    assert grut_lib.grut_relayout_scratch_bytes(100_003) >= 2 * 4 * 100_003 + grut_lib.grut_scan_scratch_bytes(100_003)
    assert grut_lib.grut_relayout_scratch_bytes(1) >= 8


def test_input_checks_reject_host_tensors_before_any_launch():
    densify = importlib.import_module("3dgrut_amd.densify")
    n = 8
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        densify.accumulate_grad_stats_(torch.zeros(n, 1), torch.zeros((n, 1), dtype=torch.int32), torch.ones(n, 3), torch.ones(n, 3), torch.zeros(3))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        densify.relayout([torch.zeros(n, 3)], keep=torch.ones(n, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        densify.split_tail_(torch.zeros(n, 3), torch.zeros(n, 3), torch.ones(n, 4), torch.zeros(4, 3), 4, 2)
    with pytest.raises(RuntimeError, match="at least one tensor"):
        densify.relayout([])


def test_the_module_imports_nothing_of_threedgrut():
    before = {k for k in sys.modules if k.split(".")[0] == "threedgrut"}
    importlib.import_module("3dgrut_amd.densify")
    assert {k for k in sys.modules if k.split(".")[0] == "threedgrut"} == before


# ---- the seam with the reference's own classes -------------------------------------------------------------------------------------------
N0 = 60
NAMES = restated.DuckModel.NAMES


def _strategy_conf():
    return _DictConfig({"strategy": {"print_stats": True,
                                     "densify": {"split": {"n_gaussians": 2}, "relative_size_threshold": 0.01, "clone_grad_threshold": 2e-4,
                                                 "split_grad_threshold": 2e-4},
                                     "prune": {"density_threshold": 0.3}, "prune_weight": {"weight_threshold": 0.4},
                                     "prune_scale": {"threshold": 0.5}, "reset_density": {"new_max_density": 0.01}}})


def _reference_model(model_mod, optimizer_cls=torch.optim.Adam):
    """The reference's own MixtureOfGaussians on the host, with the six parameter groups of a trained model and Adam state."""
    mog = model_mod.MixtureOfGaussians(_conf("3dgut"), scene_extent=1.0)
    mog.device = "cpu"
    duck = restated.DuckModel(N0, "cpu", seed=2)
    for name, _ in NAMES:
        setattr(mog, name, torch.nn.Parameter(getattr(duck, name).data.clone()))
    mog.features_albedo.requires_grad_(False)                      # requires_grad must survive the relayout
    mog.optimizer = optimizer_cls([{"params": [getattr(mog, name)], "name": name, "lr": 1e-3} for name, _ in NAMES], lr=1e-3, eps=1e-15)
    g = torch.Generator().manual_seed(4)
    for name, _ in NAMES:
        p = getattr(mog, name)
        mog.optimizer.state[p] = {"step": torch.tensor(7.0), "exp_avg": torch.randn(p.shape, generator=g), "exp_avg_sq": torch.rand(p.shape, generator=g)}
    mog.rolling_weight_contrib = torch.rand((N0, 1), generator=g)
    return mog


class _HostRecorders:
    """The three device functions (and the plan that relayout shares between tensors), on the host with torch indexing; every call is
    recorded."""

    def __init__(self):
        self.calls = []

    def accumulate_grad_stats_(self, accum, denom, positions_grad, positions, sensor_position):
        self.calls.append(("accumulate", accum, denom, positions_grad, positions, sensor_position))
        a, d = restated.accumulate_reference(accum, denom, positions_grad, positions, sensor_position, torch.float32)
        accum.copy_(a)
        denom.copy_(d)

    def relayout_plan(self, keep, append, n, device):
        self.calls.append(("plan", n))
        assert all(m is None or (m.dtype == torch.bool and m.shape == (n,) and m.is_contiguous()) for m in (keep, append))
        return (keep, append)

    def relayout(self, tensors, keep=None, append=None, copies=1, zero_append=(), plan=None):
        tensors = list(tensors)
        self.calls.append(("relayout", len(tensors), copies, tuple(zero_append), plan is not None))
        if plan is not None:
            assert keep is None and append is None
            keep, append = plan
        n = tensors[0].shape[0]
        assert all(t.is_contiguous() and t.shape[0] == n for t in tensors)
        assert all(m is None or (m.dtype == torch.bool and m.shape == (n,) and m.is_contiguous()) for m in (keep, append))
        out = [restated.relayout_reference(t, keep, append, copies, zero=j in set(zero_append)) for j, t in enumerate(tensors)]
        return out, n if keep is None else int(keep.sum()), 0 if append is None else int(append.sum())

    def split_tail_(self, positions, scale, rotation, noise, n_keep, copies):
        self.calls.append(("split_tail", noise.clone(), n_keep, copies))
        # the reference's own arithmetic (gs.py:168-186) on the tails, so that the comparison below is exact
        from threedgrut.utils.misc import quaternion_to_so3
        samples = noise * torch.exp(scale[n_keep:])
        positions[n_keep:] += torch.bmm(quaternion_to_so3(rotation[n_keep:]), samples.unsqueeze(-1)).squeeze(-1)
        scale[n_keep:] = torch.log(torch.exp(scale[n_keep:]) / (0.8 * copies))


def _install_on_host(monkeypatch, densify):
    rec = _HostRecorders()
    for name in ("accumulate_grad_stats_", "relayout_plan", "relayout", "split_tail_"):
        monkeypatch.setattr(densify, name, getattr(rec, name))
    # "a contiguous fp32 CUDA tensor": there is no GPU here, so the device half of the precondition is waived (the rest is kept)
    real_ok = densify._device_tensor_ok
    monkeypatch.setattr(densify, "_device_tensor_ok",
                        lambda t, dtypes=(torch.float32,), contiguous=True: isinstance(t, torch.Tensor) and (t.is_contiguous() or not contiguous) and t.dtype in dtypes)
    assert real_ok(torch.zeros(3)) is False
    # the reference allocates two scratch tensors with device="cuda" (gs.py:159, :169)
    real_zeros = torch.zeros
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: real_zeros(*a, **{**k, "device": "cpu"} if k.get("device") == "cuda" else k))
    return rec


def _assert_same_outcome(a, b, what):
    """Model parameters, optimizer param_groups and state, densification buffers of two (strategy, model) pairs."""
    (sa, ma), (sb, mb) = a, b
    assert ma.num_gaussians == mb.num_gaussians, what
    for (name, _), ga, gb in zip(NAMES, ma.optimizer.param_groups, mb.optimizer.param_groups):
        pa, pb = getattr(ma, name), getattr(mb, name)
        assert ga["name"] == gb["name"] == name and gb["params"][0] is pb and isinstance(pb, torch.nn.Parameter), (what, name)
        assert pa.requires_grad == pb.requires_grad and pa.shape == pb.shape and torch.equal(pa.data, pb.data), (what, name)
        ta, tb = ma.optimizer.state[pa], mb.optimizer.state[pb]
        assert list(ta) == list(tb) == ["step", "exp_avg", "exp_avg_sq"], (what, name)
        assert float(tb["step"]) == 7.0 and tb["step"].dim() == 0
        for key in ("exp_avg", "exp_avg_sq"):
            assert tb[key].shape == pb.shape and torch.equal(ta[key], tb[key]), (what, name, key)
    assert len(mb.optimizer.state) == len(NAMES), what                       # the old parameters' entries are gone
    for buf in ("densify_grad_norm_accum", "densify_grad_norm_denom"):
        x, y = getattr(sa, buf), getattr(sb, buf)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (what, buf)


def _one_operation(copies, zero_state):
    """One clone / split / prune: ONE plan (scan + host read), then per group the two moments and the parameter, one tensor each."""
    per_group = [("relayout", 1, copies, (0,) if zero_state else (), True)] * 2 + [("relayout", 1, copies, (), True)]
    return per_group * len(NAMES)


@needs_reference
def test_reference_strategy_takes_the_fused_passes_and_ends_where_the_reference_ends(reference, monkeypatch):  # noqa: F811
    densify = importlib.import_module("3dgrut_amd.densify")
    assert not any(k == "threedgrut.strategy.gs" for k in sys.modules)        # nothing of it before the call
    model_mod = importlib.import_module("threedgrut.model.model")
    gs = importlib.import_module("threedgrut.strategy.gs")
    reference_class = gs.GSStrategy
    fused_class = densify.install_fused_gs_strategy()
    assert gs.GSStrategy is fused_class and issubclass(fused_class, reference_class) and fused_class is not reference_class
    assert densify.install_fused_gs_strategy() is fused_class and fused_class.__name__ == "GSStrategy"
    for method in ("update_gradient_buffer", "clone_gaussians", "split_gaussians", "prune_gaussians_opacity", "prune_gaussians_scale",
                   "prune_gaussians_weight", "prune_densification_buffers"):
        assert getattr(fused_class, method) is not getattr(reference_class, method), method

    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    _REAL.setdefault("gut", gt._GutNative)
    monkeypatch.setattr(gt, "_GutNative", _GutRecorder)
    rec = _install_on_host(monkeypatch, densify)
    conf = _strategy_conf()
    mog_ref = _reference_model(model_mod)
    mog = copy.deepcopy(mog_ref)
    assert mog.optimizer.param_groups[0]["params"][0] is mog.positions       # the deep copy keeps the optimizer bound to its own model
    pairs = [(reference_class(conf, mog_ref), mog_ref), (fused_class(conf, mog), mog)]
    for s, _ in pairs:
        s.init_densification_buffer()

    # 4a: the statistic is handed the model's own tensors and the trainer's strided view
    g = torch.Generator().manual_seed(9)
    pose = torch.eye(4).unsqueeze(0)
    for _ in range(3):
        grad = torch.randn((N0, 3), generator=g) * 4e-4
        grad[torch.rand(N0, generator=g) < 0.3] = 0
        pose[0, :3, 3] = torch.randn(3, generator=g)
        for s, m in pairs:
            m.positions.grad = grad.clone()
            s.update_gradient_buffer(sensor_position=pose[0, :3, 3])
    assert [c[0] for c in rec.calls] == ["accumulate"] * 3
    _, accum, denom, grad_seen, positions_seen, sensor_seen = rec.calls[-1]
    fused = pairs[1][0]
    assert accum is fused.densify_grad_norm_accum and denom is fused.densify_grad_norm_denom
    assert grad_seen is mog.positions.grad and positions_seen.data_ptr() == mog.positions.data_ptr()
    assert sensor_seen.data_ptr() == pose[0, :3, 3].data_ptr() and sensor_seen.stride() == (4,) and sensor_seen.device == pose.device
    assert torch.equal(pairs[0][0].densify_grad_norm_denom, denom)
    torch.testing.assert_close(accum, pairs[0][0].densify_grad_norm_accum, rtol=1e-6, atol=0)
    fused.densify_grad_norm_accum = pairs[0][0].densify_grad_norm_accum.clone()

    # 4b: densify, then each prune
    rec.calls.clear()
    for s, _ in pairs:
        torch.manual_seed(21)
        s.densify_gaussians(scene_extent=1.0)
    state_after = torch.get_rng_state()
    k = 3 * len(NAMES)
    assert rec.calls[0] == ("plan", N0) and rec.calls[1:1 + k] == _one_operation(1, True)                     # the clone
    assert rec.calls[1 + k][0] == "plan" and rec.calls[2 + k:2 + 2 * k] == _one_operation(2, True)            # the split
    assert len(rec.calls) == 3 + 2 * k and rec.calls[-1][0] == "split_tail"
    noise = rec.calls[-1][1]
    torch.manual_seed(21)
    assert torch.equal(noise, torch.randn(noise.shape)) and torch.equal(torch.get_rng_state(), state_after)
    assert mog.num_gaussians > N0 and noise.shape[0] > 0
    _assert_same_outcome(*pairs, "densify")

    dataset = type("Dataset", (), {})()
    import numpy as np
    dataset.poses = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    dataset.intrinsic = [np.array([400.0, 300.0])]
    for s, m in pairs:
        m.rolling_weight_contrib = torch.rand((m.num_gaussians, 1), generator=torch.Generator().manual_seed(1))
        s.densify_grad_norm_accum += torch.arange(m.num_gaussians, dtype=torch.float32).unsqueeze(1)   # so that pruned buffers are told apart
    for prune, args in (("prune_gaussians_opacity", ()), ("prune_gaussians_weight", ()), ("prune_gaussians_scale", (dataset,))):
        before = mog.num_gaussians
        rec.calls.clear()
        for s, m in pairs:
            getattr(s, prune)(*args)
            m.rolling_weight_contrib = m.rolling_weight_contrib[: m.num_gaussians]
        assert rec.calls == [("plan", before)] + _one_operation(1, False) + [("relayout", 2, 1, (), False)], prune
        assert 0 < mog.num_gaussians < before, prune
        _assert_same_outcome(*pairs, prune)
    for s, _ in pairs:
        s.reset_density()
    _assert_same_outcome(*pairs, "reset_density")

    # 4c: another scale activation: the split is the reference's (no relayout, no tail call), the clone still relays out
    for _, m in pairs:
        m.scale_activation = lambda x: torch.exp(x) * 1.0
    for s, m in pairs:
        s.densify_grad_norm_accum = torch.full((m.num_gaussians, 1), 1.0)
        s.densify_grad_norm_denom = torch.ones((m.num_gaussians, 1), dtype=torch.int32)
    rec.calls.clear()
    for s, _ in pairs:
        torch.manual_seed(5)
        s.densify_gaussians(scene_extent=1.0)
    assert rec.calls[0][0] == "plan" and rec.calls[1:] == _one_operation(1, True)
    _assert_same_outcome(*pairs, "non-exp split")

    # parameters the kernels cannot read in place: everything is the reference's
    for _, m in pairs:
        m.scale_activation = torch.exp
        p = m.optimizer.param_groups[0]["params"][0]
        state = m.optimizer.state.pop(p)
        q = torch.nn.Parameter(p.data.double())
        m.optimizer.param_groups[0]["params"] = [q]
        m.optimizer.state[q] = {k: (v.double() if k != "step" else v) for k, v in state.items()}
        m.positions = q
        m.rolling_weight_contrib = torch.rand((m.num_gaussians, 1), generator=torch.Generator().manual_seed(2))
    rec.calls.clear()
    for s, m in pairs:
        getattr(s, "prune_gaussians_weight")()
    assert rec.calls == [("relayout", 2, 1, (), False)]                    # only the fp32 / int32 buffers
    assert pairs[0][1].num_gaussians == pairs[1][1].num_gaussians and torch.equal(pairs[0][1].positions.data, pairs[1][1].positions.data)
