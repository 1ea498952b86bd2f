"""CPU: the opacity / scale regularisers' C-ABI entry points are declared, mirrored and exported (ABI_VERSION unchanged) and the scratch
size is host arithmetic over the kernel's own constants; `means_torch` is the reference's formula bit for bit (against the reference's own
`Trainer3DGRUT.get_losses`, imported as tests/test_photo_loss_cpu.py does); the switch is off by default; and with the switch on, the fused
`get_losses` hands everything the kernels do not take (here: CPU tensors) to the two torch lines and returns the same dict.  What the
kernels compute is covered by tests/test_regularizers_gpu.py."""
import importlib
import os
import re
import sys
import types
from unittest.mock import MagicMock

import pytest
import torch

from test_photo_loss_cpu import _MORE_STUBS, _NoRange
from test_reference_seam_cpu import REFERENCE, _DictConfig, reference  # noqa: F401  (the reference fixture and its import stubs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("grut_reg_partials", "grut_reg_forward", "grut_reg_backward")
KEYS = ["total_loss", "l1_loss", "l2_loss", "ssim_loss", "opacity_loss", "scale_loss"]
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "threedgrut")),
                                     reason="the reference checkout is only present in the build container")


def _reg():
    return importlib.import_module("3dgrut_amd.regularizers")


@pytest.fixture()
def switch_restored():
    reg = _reg()
    before = reg.enabled()
    yield reg
    reg.install_fused_regularizers(before)


def _model(n=40, dtype=torch.float32, seed=5):
    """Raw parameters in the ranges a trained model has, with the reference's standard activations (model.py:237-241)."""
    g = torch.Generator().manual_seed(seed)
    m = types.SimpleNamespace(
        density=(torch.rand(n, 1, generator=g, dtype=dtype) * 24 - 12).requires_grad_(True),
        scale=(torch.rand(n, 3, generator=g, dtype=dtype) * 18 - 15).requires_grad_(True),
        rotation=torch.rand(n, 4, generator=g, dtype=dtype),
        density_activation=torch.sigmoid, scale_activation=torch.exp, rotation_activation=torch.nn.functional.normalize)
    m.get_density, m.get_scale = (lambda: m.density_activation(m.density)), (lambda: m.scale_activation(m.scale))
    return m


def _reference_trainer(monkeypatch):
    """threedgrut.trainer imported from the reference with the stubs of tests/test_photo_loss_cpu.py -> (the class, a trainer factory)."""
    for name in _MORE_STUBS:
        try:
            if not name.startswith("threedgrut"):
                importlib.import_module(name)
                continue
        except ModuleNotFoundError:
            pass
        stub = MagicMock(name=name)
        stub.__path__, stub.__name__ = [], name
        monkeypatch.setitem(sys.modules, name, stub)
    monkeypatch.setattr(torch.cuda.nvtx, "range", _NoRange)                        # no GPU here: a range is a no-op
    trainer_mod = importlib.import_module("threedgrut.trainer")
    assert trainer_mod.__file__.startswith(REFERENCE)
    cls = trainer_mod.Trainer3DGRUT

    def trainer(model, in_color_refine=False, **loss):
        conf = dict(use_l1=True, lambda_l1=0.8, use_l2=False, lambda_l2=1.0, use_ssim=False, lambda_ssim=0.2, use_opacity=True, lambda_opacity=0.01,
                    use_scale=True, lambda_scale=0.02)
        conf.update(loss)
        t = object.__new__(cls)
        t.conf, t.device, t.model, t._in_color_refine = _DictConfig(loss=conf), "cpu", model, in_color_refine
        return t

    return cls, trainer


def _grads(model, loss):
    model.density.grad = model.scale.grad = None
    loss.backward()
    return model.density.grad, model.scale.grad


def test_reg_symbols_are_declared_mirrored_and_exported(grut_lib):
    abi = importlib.import_module("3dgrut_amd._abi")
    reg = _reg()
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b(int|uint32_t) {name}\(", header), name
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(grut_lib, name) and getattr(grut_lib, name).argtypes, name
    assert "trainer.py:722-736" in header and "abs is the identity" in header and "sign(0) = 0" in header
    assert "regularizers.hip" in importlib.import_module("3dgrut_amd.build").SOURCES
    assert abi.ABI_VERSION == 5 and grut_lib.grut_abi_version() == 5           # additive change
    assert len(grut_lib.grut_reg_forward.argtypes) == 6 and len(grut_lib.grut_reg_backward.argtypes) == 7
    # the Python layer's copy of the kernel's constants
    src = open(os.path.join(ROOT, "3dgrut_amd", "csrc", "regularizers.hip")).read()
    assert int(re.search(r"kRegThreads = (\d+);", src).group(1)) == reg.THREADS
    assert int(re.search(r"kRegMaxBlocks = (\d+);", src).group(1)) == reg.MAX_BLOCKS
    # two floats per block, one block per 256 float4 of the [3N] array, capped: a few KiB at any N; 0 where the forward refuses N
    for n in (1, 3, 341, 342, 4099, 349525, 349526, 1_000_000, reg.MAX_PARTICLES):
        blocks = min(-(-(-(-3 * n // 4)) // reg.THREADS), reg.MAX_BLOCKS)
        assert grut_lib.grut_reg_partials(n) == 2 * blocks, n
    assert grut_lib.grut_reg_partials(341) == 2 and grut_lib.grut_reg_partials(342) == 4 and grut_lib.grut_reg_partials(1_000_000) * 4 == 8192
    assert grut_lib.grut_reg_partials(0) == 0 and grut_lib.grut_reg_partials(reg.MAX_PARTICLES + 1) == 0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_means_torch_is_the_two_torch_lines_bit_for_bit(dtype):
    reg = _reg()
    m = _model(dtype=dtype)
    mo, ms = reg.means_torch(m.density, m.scale)
    want_o, want_s = torch.abs(torch.sigmoid(m.density)).mean(), torch.abs(torch.exp(m.scale)).mean()
    assert mo.dtype == dtype and mo.dim() == 0 and ms.dim() == 0
    assert torch.equal(mo, want_o) and torch.equal(ms, want_s)
    gd, gs = (g.clone() for g in _grads(m, 0.01 * mo + 0.02 * ms))
    wd, ws = _grads(m, 0.01 * want_o + 0.02 * want_s)
    assert torch.equal(gd, wd) and torch.equal(gs, ws)
    assert reg.means_torch(None, m.scale)[0] is None and reg.means_torch(m.density, None)[1] is None
    assert torch.equal(reg.means_torch(None, m.scale)[1], want_s) and torch.equal(reg.means_torch(m.density, None)[0], want_o)


@needs_reference
def test_means_torch_is_the_reference_get_losses_formula(reference, monkeypatch):  # noqa: F811
    reg = _reg()
    cls, trainer = _reference_trainer(monkeypatch)
    m = _model(dtype=torch.float64)
    t = trainer(m)
    g = torch.Generator().manual_seed(1)
    batch = _DictConfig(rgb_gt=torch.rand(1, 8, 8, 3, generator=g, dtype=torch.float64), mask=None)
    want = cls.get_losses(t, batch, {"pred_features": torch.rand(1, 8, 8, 3, generator=g, dtype=torch.float64)})
    mo, ms = reg.means_torch(m.density, m.scale)
    assert torch.equal(want["opacity_loss"], 0.01 * mo) and torch.equal(want["scale_loss"], 0.02 * ms)
    wd, ws = (x.clone() for x in _grads(m, want["total_loss"]))
    gd, gs = _grads(m, 0.01 * mo + 0.02 * ms)
    assert torch.equal(gd, wd) and torch.equal(gs, ws)


def test_the_switch_is_off_by_default_and_returns_the_previous_state(switch_restored):
    reg = switch_restored
    assert reg.enabled() is False                                                  # nothing switched it on (every test here restores it)
    assert set(reg.stats) == {"hip_calls", "torch_calls", "hip_backward_calls"}
    assert reg.install_fused_regularizers() is False and reg.enabled() is True
    assert reg.install_fused_regularizers(True) is True
    assert reg.install_fused_regularizers(False) is True and reg.enabled() is False


def test_direct_call_on_cpu_tensors_runs_the_torch_model(switch_restored):
    reg = switch_restored
    m = _model()
    before = dict(reg.stats)
    mo, ms = reg.opacity_scale_means(m.density, m.scale)
    want_o, want_s = reg.means_torch(m.density, m.scale)
    assert torch.equal(mo, want_o) and torch.equal(ms, want_s)
    assert reg.opacity_scale_means(None, m.scale)[0] is None and reg.opacity_scale_means(m.density, None)[1] is None
    assert reg.stats["torch_calls"] == before["torch_calls"] + 3 and reg.stats["hip_calls"] == before["hip_calls"]
    with pytest.raises(ValueError, match="at least one"):
        reg.opacity_scale_means(None, None)


@needs_reference
def test_switch_on_with_cpu_tensors_gives_the_same_dict_through_the_torch_lines(reference, monkeypatch, switch_restored):  # noqa: F811
    reg = switch_restored
    losses = importlib.import_module("3dgrut_amd.losses")
    cls, trainer = _reference_trainer(monkeypatch)
    patched = losses.install_fused_losses()

    def record(pred, gt, mask=None, **kw):                                         # there is no GPU: the image terms in torch
        values = (torch.abs(pred - gt).mean(), torch.nn.functional.mse_loss(pred, gt), torch.tensor(0.9))
        return tuple(v if kw[k] else None for v, k in zip(values, ("l1", "l2", "ssim")))

    monkeypatch.setattr(losses, "photometric_loss", record)

    class Cuda(torch.Tensor):
        is_cuda = True

    g = torch.Generator().manual_seed(2)
    batch = _DictConfig(rgb_gt=torch.rand(1, 16, 16, 3, generator=g).as_subclass(Cuda), mask=None)
    outputs = {"pred_features": torch.rand(1, 16, 16, 3, generator=g).as_subclass(Cuda).requires_grad_(True)}
    m = _model()

    def run(on, **loss):
        reg.install_fused_regularizers(on)
        before = dict(reg.stats)
        out = patched(trainer(m, **loss), batch, outputs)
        grads = tuple(None if x is None else x.clone() for x in _grads(m, out["total_loss"]))
        return out, grads, {k: reg.stats[k] - before[k] for k in before}

    for loss in (dict(), dict(use_scale=False), dict(use_opacity=False), dict(use_opacity=False, use_scale=False)):
        off, g_off, d_off = run(False, **loss)
        on, g_on, d_on = run(True, **loss)
        assert list(on) == KEYS == list(off)
        for k in KEYS:
            assert on[k].shape == off[k].shape and torch.equal(torch.as_tensor(on[k]), torch.as_tensor(off[k])), (loss, k)
        for a, b in zip(g_on, g_off):
            assert (a is None and b is None) or torch.equal(a, b), loss
        asked = loss.get("use_opacity", True) or loss.get("use_scale", True)
        assert d_off == {"hip_calls": 0, "torch_calls": 0, "hip_backward_calls": 0}
        assert d_on == {"hip_calls": 0, "torch_calls": 1 if asked else 0, "hip_backward_calls": 0}, loss


@needs_reference
def test_the_hook_asks_only_for_the_enabled_terms_and_for_none_in_color_refine(reference, monkeypatch, switch_restored):  # noqa: F811
    reg = switch_restored
    losses = importlib.import_module("3dgrut_amd.losses")
    cls, trainer = _reference_trainer(monkeypatch)
    patched = losses.install_fused_losses()
    monkeypatch.setattr(losses, "photometric_loss", lambda pred, gt, mask=None, **kw: (torch.abs(pred - gt).mean(), None, None))
    monkeypatch.setattr(losses, "_fusable", lambda *a: True)
    calls = []
    monkeypatch.setattr(reg, "_fusable", lambda d, s: True)                        # as if the parameters were on the GPU
    monkeypatch.setattr(reg, "opacity_scale_means", lambda d, s: calls.append((d, s)) or reg.means_torch(d, s))
    g = torch.Generator().manual_seed(3)
    batch = _DictConfig(rgb_gt=torch.rand(1, 16, 16, 3, generator=g), mask=None)
    outputs = {"pred_features": torch.rand(1, 16, 16, 3, generator=g)}
    m = _model()
    reg.install_fused_regularizers(True)
    want_o, want_s = reg.means_torch(m.density, m.scale)

    out = patched(trainer(m), batch, outputs)
    assert len(calls) == 1 and calls[0][0] is m.density and calls[0][1] is m.scale
    assert torch.equal(out["opacity_loss"], 0.01 * want_o) and torch.equal(out["scale_loss"], 0.02 * want_s)
    out = patched(trainer(m, use_scale=False), batch, outputs)
    assert len(calls) == 2 and calls[1][0] is m.density and calls[1][1] is None
    assert torch.equal(out["opacity_loss"], 0.01 * want_o) and out["scale_loss"].shape == (1,) and float(out["scale_loss"]) == 0.0
    out = patched(trainer(m, use_opacity=False), batch, outputs)
    assert len(calls) == 3 and calls[2][0] is None and calls[2][1] is m.scale
    assert torch.equal(out["scale_loss"], 0.02 * want_s) and out["opacity_loss"].shape == (1,) and float(out["opacity_loss"]) == 0.0

    # the colour refinement phase: neither term, by either path; the model is not even asked
    def never(*a):
        raise AssertionError("a regulariser was evaluated during colour refinement")

    m.get_density = m.get_scale = never
    for on in (True, False):
        reg.install_fused_regularizers(on)
        out = patched(trainer(m, in_color_refine=True), batch, outputs)
        assert len(calls) == 3
        for k in ("opacity_loss", "scale_loss"):
            assert out[k].shape == (1,) and float(out[k]) == 0.0

    # a model that activates with something else keeps the two torch lines
    other = _model()
    other.density_activation = torch.tanh
    reg.install_fused_regularizers(True)
    before = reg.stats["torch_calls"]
    out = patched(trainer(other), batch, outputs)
    assert len(calls) == 3 and reg.stats["torch_calls"] == before + 1
    assert torch.equal(out["opacity_loss"], 0.01 * torch.abs(torch.tanh(other.density)).mean())
