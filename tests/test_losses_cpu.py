"""CPU: the fused SSIM's C-ABI entry points are declared, mirrored and exported; the `fused_ssim` shim and `losses.install()` make the
reference's unchanged `threedgrut/model/losses.py` import and reach this repository's function; the Python surface rejects bad input
before any launch; and the float64 restatement that the GPU tests trust (tests/ssim_reference.py) is itself sane.  What the kernels
compute is covered by tests/test_losses_gpu.py."""
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

import ssim_reference as ref
from test_reference_seam_cpu import REFERENCE, reference  # noqa: F401  (the reference fixture and its import stubs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("grut_ssim_forward", "grut_ssim_backward", "grut_ssim_partials")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "threedgrut")),
                                     reason="the reference checkout is only present in the build container")


def test_ssim_symbols_are_declared_mirrored_and_exported(grut_lib):
    abi = importlib.import_module("3dgrut_amd._abi")
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b(int|uint32_t) {name}\(", header), name
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(grut_lib, name) and getattr(grut_lib, name).argtypes, name
    assert "loss.hip" in importlib.import_module("3dgrut_amd.build").SOURCES
    assert abi.ABI_VERSION == 5 and grut_lib.grut_abi_version() == 5           # additive change
    # one partial per 32x32 tile of every plane; a bad shape gives 0
    assert grut_lib.grut_ssim_partials(1, 3, 1080, 1920) == 3 * 34 * 60 and grut_lib.grut_ssim_partials(2, 1, 11, 11) == 2
    assert grut_lib.grut_ssim_partials(1, 0, 4, 4) == 0


def test_kernel_taps_are_the_fp32_roundings_of_the_float64_window():
    src = open(os.path.join(ROOT, "3dgrut_amd", "csrc", "loss.hip")).read()
    body = re.search(r"kSsimTap\[kSsimTaps\]\s*=\s*\{([^}]*)\}", src).group(1)
    taps = np.array([np.float32(t.strip().rstrip("f")) for t in body.split(",")], dtype=np.float32)
    assert taps.shape == (11,) and np.array_equal(taps, ref.taps_fp32())


def test_shim_package_exports_this_repositorys_function(monkeypatch):
    losses = importlib.import_module("3dgrut_amd.losses")
    monkeypatch.delitem(sys.modules, "fused_ssim", raising=False)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "shims"))
    mod = importlib.import_module("fused_ssim")
    assert os.path.dirname(os.path.abspath(mod.__file__)) == os.path.join(ROOT, "shims", "fused_ssim")
    assert mod.fused_ssim is losses.fused_ssim
    monkeypatch.delitem(sys.modules, "fused_ssim", raising=False)


def test_install_registers_the_module_without_importing_threedgrut_and_keeps_an_existing_one(monkeypatch):
    losses = importlib.import_module("3dgrut_amd.losses")
    monkeypatch.delitem(sys.modules, "fused_ssim", raising=False)
    before = {k for k in sys.modules if k.split(".")[0] == "threedgrut"}
    losses.install()
    assert sys.modules["fused_ssim"].fused_ssim is losses.fused_ssim
    assert {k for k in sys.modules if k.split(".")[0] == "threedgrut"} == before
    installed = object()                                     # a package that is really installed wins
    monkeypatch.setitem(sys.modules, "fused_ssim", installed)
    losses.install()
    assert sys.modules["fused_ssim"] is installed
    monkeypatch.delitem(sys.modules, "fused_ssim", raising=False)


@needs_reference
def test_reference_losses_module_imports_and_its_ssim_reaches_fused_ssim_with_valid_padding(reference, monkeypatch):  # noqa: F811
    losses = importlib.import_module("3dgrut_amd.losses")
    monkeypatch.delitem(sys.modules, "fused_ssim", raising=False)
    monkeypatch.delitem(sys.modules, "threedgrut.model.losses", raising=False)
    calls = []

    def record(img1, img2, padding="same", train=True):
        calls.append((img1, img2, padding, train))
        return torch.zeros(())

    monkeypatch.setattr(losses, "fused_ssim", record)        # the shim package re-exports whatever the module holds when it is imported
    monkeypatch.setattr(torch.cuda.nvtx, "range", lambda *a, **k: (lambda f: f))   # no GPU here: the range decorator is a no-op
    ref_losses = importlib.import_module("threedgrut.model.losses")
    assert ref_losses.__file__.startswith(REFERENCE)
    assert ref_losses.fused_ssim is record
    a, b = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    ref_losses.ssim(a, b)
    assert len(calls) == 1 and calls[0][0] is a and calls[0][1] is b and calls[0][2] == "valid"
    monkeypatch.delitem(sys.modules, "fused_ssim", raising=False)
    monkeypatch.delitem(sys.modules, "threedgrut.model.losses", raising=False)


def test_input_checks_raise_before_any_launch(monkeypatch):
    losses = importlib.import_module("3dgrut_amd.losses")
    abi = importlib.import_module("3dgrut_amd._abi")

    def no_launch(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(abi, "load_library", no_launch)
    a = torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        losses.fused_ssim(a, a.clone())
    with pytest.raises(ValueError, match="padding"):
        losses.fused_ssim(a, a.clone(), padding="reflect")
    # the remaining checks do not depend on the device: run them on meta tensors that claim to be CUDA tensors
    class Cuda(torch.Tensor):
        is_cuda = True

    def cuda(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(Cuda)

    with pytest.raises(RuntimeError, match="float32"):
        losses.fused_ssim(cuda(1, 3, 16, 16, dtype=torch.float16), cuda(1, 3, 16, 16, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="same shape"):
        losses.fused_ssim(cuda(1, 3, 16, 16), cuda(1, 3, 16, 17))
    with pytest.raises(RuntimeError, match=r"\[B, C, H, W\]"):
        losses.fused_ssim(cuda(3, 16, 16), cuda(3, 16, 16))
    with pytest.raises(RuntimeError, match="H, W >= 11"):
        losses.fused_ssim(cuda(1, 3, 10, 16), cuda(1, 3, 10, 16), padding="valid")
    with pytest.raises(RuntimeError, match="H, W >= 11"):
        losses.ssim(cuda(1, 3, 16, 10), cuda(1, 3, 16, 10))


def test_layouts_read_in_place():
    losses = importlib.import_module("3dgrut_amd.losses")
    nhwc = torch.rand(2, 16, 20, 3)
    assert losses._readable_in_place(nhwc.permute(0, 3, 1, 2)) and losses._readable_in_place(torch.rand(2, 3, 16, 20))
    assert not losses._readable_in_place(torch.rand(1, 1, 16, 20).expand(2, 3, 16, 20))
    assert not losses._readable_in_place(torch.rand(2, 3, 16, 40)[..., ::2])


@pytest.mark.parametrize("padding", ["same", "valid"])
def test_the_float64_restatement_is_sane(padding):
    g = torch.Generator().manual_seed(3)
    x = torch.rand((1, 2, 24, 24), generator=g, dtype=torch.float64)
    y = torch.rand((1, 2, 24, 24), generator=g, dtype=torch.float64)
    assert abs(float(ref.ssim_torch(x, x, padding)) - 1.0) < 1e-13
    assert float((ref.ssim_map(x, x) - 1.0).abs().max()) < 1e-12
    assert abs(float(ref.ssim_torch(x, y, padding)) - float(ref.ssim_torch(y, x, padding))) < 1e-15
    out = ref.reference_and_bounds(x, y, padding, upstream=-3.0)       # (also asserts analytic == autograd gradient inside)
    assert abs(out["value"] - float(ref.ssim_torch(x, y, padding))) == 0.0
    # central finite differences on every 7th pixel
    h = 1e-6
    flat = x.reshape(-1)
    for i in range(0, flat.numel(), 7):
        xp, xm = flat.clone(), flat.clone()
        xp[i] += h
        xm[i] -= h
        fd = -3.0 * (float(ref.ssim_torch(xp.view_as(x), y, padding)) - float(ref.ssim_torch(xm.view_as(x), y, padding))) / (2 * h)
        assert abs(fd - float(out["grad"].reshape(-1)[i])) < 1e-8 * max(1.0, float(out["grad"].abs().max()) / 1e-3), i
    assert out["value_bound"] > 0 and bool((out["grad_bound"] > 0).all())
    # an fp32 evaluation of the same formula (direct 121-term sums) stays inside the bound derived for it
    x32 = x.float().requires_grad_(True)
    v32 = ref.ssim_torch(x32, y.float(), padding)
    (g32,) = torch.autograd.grad(-3.0 * v32, x32)
    out32 = ref.reference_and_bounds(x.float(), y.float(), padding, upstream=-3.0, k=ref.K_DIRECT)
    assert abs(float(v32) - out32["value"]) <= out32["value_bound"]
    assert bool(((g32.double() - out32["grad"]).abs() <= out32["grad_bound"]).all())
