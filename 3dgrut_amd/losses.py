"""Fused, differentiable SSIM on the MI355X: drop-in for the third-party CUDA extension `fused_ssim` that the reference's loss
imports (threedgrut/model/losses.py:17), backed by csrc/loss.hip.  There is no CPU fallback.

    fused_ssim(img1, img2, padding="same", train=True)   the surface of the upstream package; 0-dim result
    ssim(img1, img2, window_size=11, size_average=True)  the reference's wrapper (losses.py:31-33): padding="valid"
    install()      registers a module named `fused_ssim` (unless one is already importable from sys.modules); called by the shims

The gradient flows to img1 only: img2 is the ground truth and is treated as a constant, as upstream does.  There is no double backward.
Both images are read through their strides: a contiguous NCHW tensor and `torch.permute(rgb, (0, 3, 1, 2))` of a [B, H, W, C] tensor
(trainer.py:717-718) are read in place, and the gradient is written with img1's strides.
"""
from __future__ import annotations

import ctypes as C
import sys
import types

import torch
from torch.autograd.function import once_differentiable

from . import _abi

SHIM_MODULE = "fused_ssim"
WINDOW = 11
MAX_PLANES = 65535   # one grid row per (image, channel group): the C layer's limit, checked here before anything is allocated
# the Python layer's own bookkeeping (tests: inference allocates no derivative plane); plain counters, not synchronised across threads
stats = {"forward_calls": 0, "backward_calls": 0, "planes_allocated": 0}


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _strides(t):
    return (C.c_int64 * 4)(*t.stride())


def _check_input(img1, img2, padding):
    if padding not in ("same", "valid"):
        raise ValueError(f"padding must be \"same\" or \"valid\" (got {padding!r})")
    for t, name in ((img1, "img1"), (img2, "img2")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor (there is no CPU fallback)")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be float32 (got {t.dtype})")
        if t.dim() != 4:
            raise RuntimeError(f"{name} must be [B, C, H, W] (got {t.dim()} dimensions)")
    if img1.shape != img2.shape:
        raise RuntimeError(f"img1 and img2 must have the same shape (got {tuple(img1.shape)} and {tuple(img2.shape)})")
    if img1.device != img2.device:
        raise RuntimeError("img1 and img2 must be on the same device")
    if img1.numel() == 0:
        raise RuntimeError("img1 and img2 must not be empty")
    if img1.shape[0] * img1.shape[1] > MAX_PLANES:
        raise RuntimeError(f"B * C must be <= {MAX_PLANES} (got {img1.shape[0]} x {img1.shape[1]})")
    if padding == "valid" and (img1.shape[2] < WINDOW or img1.shape[3] < WINDOW):
        raise RuntimeError(f"padding=\"valid\" needs H, W >= {WINDOW} (got {img1.shape[2]} x {img1.shape[3]})")


def _readable_in_place(t):
    """Dense, non-overlapping memory (any permutation of a contiguous block): the kernels address it through its strides.
    Expanded or overlapping views are copied."""
    if t.is_contiguous():
        return True
    sizes_strides = sorted(((st, sz) for sz, st in zip(t.shape, t.stride()) if sz > 1))
    expect = 1
    for st, sz in sizes_strides:
        if st != expect:
            return False
        expect *= sz
    return True


class _FusedSSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, valid, train):
        lib = _abi.load_library()
        b, c, h, w = (int(s) for s in img1.shape)
        opts = dict(dtype=torch.float32, device=img1.device)
        out = torch.empty((), **opts)
        partials = torch.empty(int(lib.grut_ssim_partials(b, c, h, w)), **opts)
        planes = torch.empty((3, b, c, h, w), **opts) if train else None
        stats["forward_calls"] += 1
        stats["planes_allocated"] += 3 if train else 0
        null = C.c_void_p(None)
        with torch.cuda.device(img1.device):   # the launch goes to the images' device, whichever is current
            _abi.check(lib.grut_ssim_forward(
                _stream(img1), b, c, h, w, _ptr(img1), _strides(img1), _ptr(img2), _strides(img2), valid, _ptr(out), _ptr(partials),
                *([_ptr(planes[i]) for i in range(3)] if train else [null] * 3)), "grut_ssim_forward")
        if train:
            ctx.save_for_backward(img1, img2, planes)
            ctx.valid = valid
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        img1, img2, planes = ctx.saved_tensors
        b, c, h, w = (int(s) for s in img1.shape)
        grad_out = grad_out.reshape(1).to(torch.float32).contiguous()
        grad = torch.empty_strided(img1.shape, img1.stride(), dtype=torch.float32, device=img1.device)   # img1's layout (dense: see forward)
        stats["backward_calls"] += 1
        with torch.cuda.device(img1.device):
            _abi.check(_abi.load_library().grut_ssim_backward(
                _stream(img1), b, c, h, w, _ptr(img1), _strides(img1), _ptr(img2), _strides(img2), ctx.valid, _ptr(grad_out),
                _ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2]), _ptr(grad), _strides(grad)), "grut_ssim_backward")
        return grad, None, None, None


def fused_ssim(img1: torch.Tensor, img2: torch.Tensor, padding: str = "same", train: bool = True) -> torch.Tensor:
    """Mean SSIM of two [B, C, H, W] fp32 CUDA images (11-tap Gaussian window, sigma 1.5, zero padding), as a 0-dim tensor on the current
    stream.  padding="same": mean over every pixel; "valid": over map[:, :, 5:-5, 5:-5].  Differentiable in img1 only (img2 is a
    constant).  With train=False, under torch.no_grad() or when img1 does not require grad, only the value is computed and the three
    derivative planes are neither allocated nor written."""
    _check_input(img1, img2, padding)
    if not _readable_in_place(img1):
        img1 = img1.contiguous()
    if not _readable_in_place(img2):
        img2 = img2.contiguous()
    train = bool(train) and torch.is_grad_enabled() and img1.requires_grad
    if not train:
        img1 = img1.detach()
    return _FusedSSIM.apply(img1, img2.detach(), 1 if padding == "valid" else 0, train)


def ssim(img1, img2, window_size=11, size_average=True):
    """threedgrut/model/losses.py:31-33: predicted and ground-truth image [B, C, H, W]; the window is the extension's fixed 11x11."""
    return fused_ssim(img1, img2, padding="valid")


def install() -> None:
    """Make `from fused_ssim import fused_ssim` (threedgrut/model/losses.py:17) bind to this module's function.  A `fused_ssim` that is
    already in sys.modules wins (setdefault).  Imports nothing of threedgrut."""
    if SHIM_MODULE in sys.modules:
        return
    mod = types.ModuleType(SHIM_MODULE)
    mod.__doc__ = "HIP fused SSIM of 3dgrut_amd.losses under the name of the upstream CUDA package."
    mod.fused_ssim = fused_ssim
    mod.__all__ = ["fused_ssim"]
    sys.modules.setdefault(SHIM_MODULE, mod)
