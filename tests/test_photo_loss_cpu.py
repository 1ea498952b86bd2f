"""CPU: the fused photometric loss's C-ABI entry points are declared, mirrored and exported (ABI_VERSION unchanged); the partials count
follows the tile count; and `install_fused_losses()` is driven against the reference's own `threedgrut/trainer.py`, imported with the
import stubs of tests/test_reference_seam_cpu.py: the class attribute is replaced in place, the new method makes ONE `photometric_loss`
call (replaced here by a recorder: there is no GPU) with the batch's own tensors, returns the reference's dict with the reference's
weighting, and hands every case whose preconditions fail to the reference's method.  What the kernels compute is covered by
tests/test_photo_loss_gpu.py."""
import contextlib
import importlib
import os
import re
import sys
import types
from unittest.mock import MagicMock

import pytest
import torch

from test_reference_seam_cpu import REFERENCE, _DictConfig, reference  # noqa: F401  (the reference fixture and its import stubs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("grut_photo_loss_forward", "grut_photo_loss_backward", "grut_photo_loss_partials")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "threedgrut")),
                                     reason="the reference checkout is only present in the build container")
# what trainer.py imports beyond the seam fixture's stubs and is not on the loss path (typing.Self in utils/timer.py needs Python 3.11)
_MORE_STUBS = ("addict", "torchmetrics", "torchmetrics.image", "torchmetrics.image.lpip", "torchvision", "threedgrut.utils.timer")


class _NoRange(contextlib.ContextDecorator):
    """torch.cuda.nvtx.range as the reference uses it: a decorator (trainer.py:676) and a context manager (trainer.py:700)."""

    def __init__(self, *a, **k):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def test_photo_loss_symbols_are_declared_mirrored_and_exported(grut_lib):
    abi = importlib.import_module("3dgrut_amd._abi")
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b(int|uint32_t) {name}\(", header), name
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(grut_lib, name) and getattr(grut_lib, name).argtypes, name
    assert "trainer.py:701" in header and "trainer.py:709" in header and "trainer.py:717-719" in header   # the lines they replace
    assert abi.ABI_VERSION == 5 and grut_lib.grut_abi_version() == 5           # additive change
    assert len(grut_lib.grut_photo_loss_forward.argtypes) == 18 and len(grut_lib.grut_photo_loss_backward.argtypes) == 19


@pytest.mark.parametrize("shape", [(1, 3, 1080, 1920), (2, 1, 11, 11), (2, 3, 37, 45), (1, 4, 64, 33), (3, 2, 32, 32)])
def test_partials_follow_the_tile_count(grut_lib, shape):
    b, c, h, w = shape
    tiles = -(-h // 32) * -(-w // 32)
    assert grut_lib.grut_photo_loss_partials(b, c, h, w) == 3 * b * c * tiles == 3 * grut_lib.grut_ssim_partials(b, c, h, w)


def test_partials_of_a_bad_shape_are_zero(grut_lib):
    for shape in ((1, 0, 4, 4), (0, 3, 16, 16), (1, 3, -1, 16), (1, 3, 16, 0)):
        assert grut_lib.grut_photo_loss_partials(*shape) == 0


def test_input_checks_raise_before_any_launch(monkeypatch):
    losses = importlib.import_module("3dgrut_amd.losses")
    abi = importlib.import_module("3dgrut_amd._abi")

    def no_launch(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(abi, "load_library", no_launch)

    class Cuda(torch.Tensor):
        is_cuda = True

    cuda = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype).as_subclass(Cuda)   # noqa: E731
    a = torch.rand(1, 16, 16, 3)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        losses.photometric_loss(a, a.clone())
    with pytest.raises(ValueError, match="at least one"):
        losses.photometric_loss(cuda(1, 16, 16, 3), cuda(1, 16, 16, 3), l1=False, l2=False, ssim=False)
    with pytest.raises(ValueError, match="padding"):
        losses.photometric_loss(cuda(1, 16, 16, 3), cuda(1, 16, 16, 3), padding="reflect")
    with pytest.raises(RuntimeError, match="float32"):
        losses.photometric_loss(cuda(1, 16, 16, 3, dtype=torch.float16), cuda(1, 16, 16, 3, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="same shape"):
        losses.photometric_loss(cuda(1, 16, 16, 3), cuda(1, 16, 17, 3))
    with pytest.raises(RuntimeError, match=r"\[B, H, W, C\]"):
        losses.photometric_loss(cuda(16, 16, 3), cuda(16, 16, 3))
    with pytest.raises(RuntimeError, match="H, W >= 11"):
        losses.photometric_loss(cuda(1, 10, 16, 3), cuda(1, 10, 16, 3))
    with pytest.raises(RuntimeError, match=r"mask must be \[1, 16, 16\] or \[1, 16, 16, 1\]"):
        losses.photometric_loss(cuda(1, 16, 16, 3), cuda(1, 16, 16, 3), cuda(1, 16, 16, 3))
    with pytest.raises(RuntimeError, match="mask must be float32"):
        losses.photometric_loss(cuda(1, 16, 16, 3), cuda(1, 16, 16, 3), cuda(1, 16, 16, 1, dtype=torch.bool))


@needs_reference
def test_install_fused_losses_drives_the_reference_trainer(reference, monkeypatch):  # noqa: F811
    losses = importlib.import_module("3dgrut_amd.losses")
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
    from threedgrut.trainer import Trainer3DGRUT as imported_earlier               # however train.py got hold of the class
    original = cls.__dict__["get_losses"]

    patched = losses.install_fused_losses()
    assert cls.__dict__["get_losses"] is patched and imported_earlier.get_losses is patched and patched is not original
    assert trainer_mod.Trainer3DGRUT is cls                                         # the class itself is not replaced
    assert losses.install_fused_losses() is patched and patched._grut_original is original and cls.__dict__["get_losses"] is patched

    # the reference's method reaches `ssim` through its module; a recorder there shows when the ORIGINAL ran (and lets it run without a GPU)
    ssim_calls, photo_calls = [], []
    monkeypatch.setattr(trainer_mod, "ssim", lambda a, b: ssim_calls.append((a, b)) or torch.tensor(0.9))

    def record(pred, gt, mask=None, **kw):
        photo_calls.append((pred, gt, mask, kw))
        m = 1.0 if mask is None else mask
        values = (torch.abs(pred * m - gt * m).mean(), torch.nn.functional.mse_loss(pred, gt * m), torch.tensor(0.9))
        return tuple(v if kw[k] else None for v, k in zip(values, ("l1", "l2", "ssim")))

    monkeypatch.setattr(losses, "photometric_loss", record)

    class Cuda(torch.Tensor):
        is_cuda = True

    g = torch.Generator().manual_seed(4)
    rand = lambda *shape: torch.rand(*shape, generator=g)                          # noqa: E731
    cuda = lambda t: t.as_subclass(Cuda)                                           # noqa: E731
    model = types.SimpleNamespace(get_density=lambda: rand(40, 1) - 0.5, get_scale=lambda: rand(40, 3))

    def trainer(in_color_refine=False, **loss):
        conf = dict(use_l1=True, lambda_l1=0.8, use_l2=False, lambda_l2=1.0, use_ssim=True, lambda_ssim=0.2, use_opacity=False, lambda_opacity=0.01,
                    use_scale=False, lambda_scale=0.02)
        conf.update(loss)
        t = object.__new__(cls)
        t.conf, t.device, t.model, t._in_color_refine = _DictConfig(loss=conf), "cpu", model, in_color_refine
        return t

    def both(t, batch, outputs):
        """-> (patched result, original result, fused calls made, did the patched method fall back)"""
        del ssim_calls[:], photo_calls[:]
        state = g.get_state()
        got = patched(t, batch, outputs)
        fused, fell_back = len(photo_calls), len(ssim_calls)
        g.set_state(state)                                                          # the regularisers draw from it
        want = original(t, batch, outputs)
        return got, want, fused, bool(fell_back) or fused == 0

    keys = ["total_loss", "l1_loss", "l2_loss", "ssim_loss", "opacity_loss", "scale_loss"]
    for mask_shape in (None, (2, 16, 20, 1)):
        for loss in (dict(), dict(use_l2=True), dict(use_ssim=False), dict(use_l1=False, use_opacity=True, use_scale=True),
                     dict(use_opacity=True, use_scale=True, in_color_refine=True)):
            t = trainer(**loss)
            pred, gt = cuda(rand(2, 16, 20, 3)), cuda(rand(2, 16, 20, 3))
            mask = None if mask_shape is None else cuda((rand(*mask_shape) < 0.6).float())
            outputs = {"pred_features": pred}
            got, want, fused, fell_back = both(t, _DictConfig(rgb_gt=gt, mask=mask), outputs)
            assert fused == 1 and not fell_back, loss                               # ONE call, and the reference's method did not run
            p, gt_seen, m, kw = photo_calls[0] if photo_calls else (None,) * 4
            assert outputs["pred_features"] is pred
            assert list(got) == keys == list(want)
            conf = t.conf.loss
            for k in keys:
                assert got[k].shape == want[k].shape and torch.equal(torch.as_tensor(got[k]), torch.as_tensor(want[k])), (loss, k)
            for k, on in (("l1_loss", conf.use_l1), ("l2_loss", conf.use_l2), ("ssim_loss", conf.use_ssim),
                          ("opacity_loss", conf.use_opacity and not t._in_color_refine), ("scale_loss", conf.use_scale and not t._in_color_refine)):
                assert on or (got[k].shape == (1,) and float(got[k]) == 0.0), (loss, k)   # a disabled term is lambda = 0 times torch.zeros(1)
            if conf.use_ssim:
                assert abs(float(got["ssim_loss"]) - 0.2 * (1.0 - 0.9)) < 1e-7

    # the call itself: the batch's own tensors, the reference's terms, "valid" as losses.py:31-33 has it
    t = trainer(use_l2=True)
    pred, gt, mask = cuda(rand(2, 16, 20, 3)), cuda(rand(2, 16, 20, 3)), cuda(rand(2, 16, 20, 1))
    del photo_calls[:]
    patched(t, _DictConfig(rgb_gt=gt, mask=mask), {"pred_features": pred})
    (p, gt_seen, m, kw), = photo_calls
    assert p is pred and gt_seen is gt and m is mask and kw == dict(l1=True, l2=True, ssim=True, padding="valid")

    # every failed precondition goes to the reference's method, which gives what it gives unpatched
    def falls_back(pred, gt, mask=None, **loss):
        got, want, fused, fell_back = both(trainer(**loss), _DictConfig(rgb_gt=gt, mask=mask), {"pred_features": pred})
        assert all(torch.equal(got[k], want[k]) for k in keys)
        return fused == 0 and fell_back

    ok = lambda: (cuda(rand(2, 16, 20, 3)), cuda(rand(2, 16, 20, 3)))              # noqa: E731
    assert not falls_back(*ok()) and not falls_back(*ok(), cuda(rand(2, 16, 20, 1)))
    assert falls_back(rand(2, 16, 20, 3), cuda(rand(2, 16, 20, 3)))                 # pred not on the GPU
    assert falls_back(cuda(rand(2, 16, 20, 3)), rand(2, 16, 20, 3))                 # gt not on the GPU
    assert falls_back(cuda(rand(2, 16, 20, 3).double()), cuda(rand(2, 16, 20, 3).double()))       # not fp32
    assert falls_back(cuda(rand(2, 16, 20, 5)), cuda(rand(2, 16, 20, 5)))           # C > 4
    assert falls_back(cuda(rand(2, 10, 20, 3)), cuda(rand(2, 10, 20, 3)))           # H < 11 with SSIM on
    assert falls_back(cuda(rand(2, 16, 10, 3)), cuda(rand(2, 16, 10, 3)))           # W < 11 with SSIM on
    assert not falls_back(cuda(rand(2, 10, 20, 3)), cuda(rand(2, 10, 20, 3)), use_ssim=False)     # ... and no limit without it
    assert falls_back(*ok(), cuda(rand(2, 16, 20, 3)))                              # a per-channel mask
    assert falls_back(*ok(), cuda(rand(1, 16, 20, 1)))                              # a mask of another batch size
    assert falls_back(*ok(), cuda(rand(2, 16, 20, 1) < 0.5))                        # a bool mask
    assert falls_back(*ok(), rand(2, 16, 20, 1))                                    # a mask that is not on the GPU
    assert falls_back(*ok(), use_l1=False, use_ssim=False)                          # nothing for the kernels to do
    monkeypatch.setattr(losses, "MAX_PLANES", 5)
    assert falls_back(*ok())                                                        # B * C over the kernels' limit
