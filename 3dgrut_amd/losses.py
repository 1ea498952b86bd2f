"""Fused, differentiable SSIM on the MI355X: drop-in for the third-party CUDA extension `fused_ssim` that the reference's loss
imports (threedgrut/model/losses.py:17), backed by csrc/loss.hip.  There is no CPU fallback.

    fused_ssim(img1, img2, padding="same", train=True)   the surface of the upstream package; 0-dim result
    ssim(img1, img2, window_size=11, size_average=True)  the reference's wrapper (losses.py:31-33): padding="valid"
    install()      registers a module named `fused_ssim` (unless one is already importable from sys.modules); called by the shims
    photometric_loss(pred, gt, mask=None, *, l1=True, l2=False, ssim=True, padding="valid")
                   everything Trainer3DGRUT.get_losses takes from the two images (trainer.py:687-720) in one HIP pass each way
    install_fused_losses()   opt-in: Trainer3DGRUT.get_losses makes that one call instead of its chain of torch kernels

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

from . import _abi, regularizers

SHIM_MODULE = "fused_ssim"
WINDOW = 11
MAX_PLANES = 65535   # one grid row per (image, channel group): the C layer's limit, checked here before anything is allocated
# the Python layer's own bookkeeping (tests: inference allocates no derivative plane); plain counters, not synchronised across threads
stats = {"forward_calls": 0, "backward_calls": 0, "planes_allocated": 0,
         "photo_forward_calls": 0, "photo_backward_calls": 0, "photo_planes_allocated": 0}   # the same three for photometric_loss
TERM_L1, TERM_L2, TERM_SSIM = 1, 2, 4   # the `terms` bits of grut_photo_loss_forward / _backward
MAX_FUSED_CHANNELS = 4   # what the trainer hook hands to the fused call: channels-last images are read as contiguous runs up to here


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _strides(t):
    return (C.c_int64 * 4)(*t.stride())


def _plane_ptrs(planes):
    """The three derivative planes of a [3, B, C, H, W] tensor as arguments, or three nulls."""
    return [C.c_void_p(None)] * 3 if planes is None else [_ptr(planes[i]) for i in range(3)]


def _check_padding(padding):
    if padding not in ("same", "valid"):
        raise ValueError(f"padding must be \"same\" or \"valid\" (got {padding!r})")


def _check_input(img1, img2, padding):
    _check_padding(padding)
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


def _in_place(t):
    return t if _readable_in_place(t) else t.contiguous()


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
        with torch.cuda.device(img1.device):   # the launch goes to the images' device, whichever is current
            _abi.check(lib.grut_ssim_forward(
                _stream(img1), b, c, h, w, _ptr(img1), _strides(img1), _ptr(img2), _strides(img2), valid, _ptr(out), _ptr(partials),
                *_plane_ptrs(planes)), "grut_ssim_forward")
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
                *_plane_ptrs(planes), _ptr(grad), _strides(grad)), "grut_ssim_backward")
        return grad, None, None, None


def fused_ssim(img1: torch.Tensor, img2: torch.Tensor, padding: str = "same", train: bool = True) -> torch.Tensor:
    """Mean SSIM of two [B, C, H, W] fp32 CUDA images (11-tap Gaussian window, sigma 1.5, zero padding), as a 0-dim tensor on the current
    stream.  padding="same": mean over every pixel; "valid": over map[:, :, 5:-5, 5:-5].  Differentiable in img1 only (img2 is a
    constant).  With train=False, under torch.no_grad() or when img1 does not require grad, only the value is computed and the three
    derivative planes are neither allocated nor written."""
    _check_input(img1, img2, padding)
    img1, img2 = _in_place(img1), _in_place(img2)
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


# ---- fused photometric loss (trainer.py:687-720) ------------------------------------------------------------------------------------
def _strides3(t):
    return (C.c_int64 * 3)(*t.stride())


class _PhotometricLoss(torch.autograd.Function):
    """pred, gt: [B, C, H, W] views; mask: [B, H, W] or None.  Three 0-dim outputs (l1, l2, ssim); a term that is not selected is 0 and
    its upstream gradient is not read.  One backward launch for all of them."""

    @staticmethod
    def forward(ctx, pred, gt, mask, terms, valid, train):
        lib = _abi.load_library()
        b, c, h, w = (int(s) for s in pred.shape)
        opts = dict(dtype=torch.float32, device=pred.device)
        out = torch.empty(3, **opts)
        partials = torch.empty(int(lib.grut_photo_loss_partials(b, c, h, w)), **opts)
        planes = torch.empty((3, b, c, h, w), **opts) if train and terms & TERM_SSIM else None
        stats["photo_forward_calls"] += 1
        stats["photo_planes_allocated"] += 0 if planes is None else 3
        null = C.c_void_p(None)
        with torch.cuda.device(pred.device):
            _abi.check(lib.grut_photo_loss_forward(
                _stream(pred), b, c, h, w, _ptr(pred), _strides(pred), _ptr(gt), _strides(gt),
                null if mask is None else _ptr(mask), None if mask is None else _strides3(mask), terms, valid, _ptr(out), _ptr(partials),
                *_plane_ptrs(planes)), "grut_photo_loss_forward")
        if train:
            ctx.save_for_backward(*(t for t in (pred, gt, mask, planes) if t is not None))
            ctx.has_mask, ctx.terms, ctx.valid = mask is not None, terms, valid
            ctx.set_materialize_grads(False)
        return out[0], out[1], out[2]

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        saved = list(ctx.saved_tensors)
        pred, gt = saved[0], saved[1]
        mask = saved[2] if ctx.has_mask else None
        planes = saved[-1] if ctx.terms & TERM_SSIM else None
        b, c, h, w = (int(s) for s in pred.shape)
        # the upstream gradients of the selected terms, in order, as one [3] device tensor; entries of other terms are never read
        given = [None if g is None or not (ctx.terms >> k) & 1 else g.reshape(()).to(torch.float32) for k, g in enumerate(grads)]
        if all(g is None for g in given):
            return None, None, None, None, None, None
        filler = next(g for g in given if g is not None)
        grad_out = torch.stack([g if g is not None else (filler if not (ctx.terms >> k) & 1 else torch.zeros_like(filler))
                                for k, g in enumerate(given)])
        grad = torch.empty_strided(pred.shape, pred.stride(), dtype=torch.float32, device=pred.device)   # pred's layout (dense: see below)
        stats["photo_backward_calls"] += 1
        null = C.c_void_p(None)
        with torch.cuda.device(pred.device):
            _abi.check(_abi.load_library().grut_photo_loss_backward(
                _stream(pred), b, c, h, w, _ptr(pred), _strides(pred), _ptr(gt), _strides(gt),
                null if mask is None else _ptr(mask), None if mask is None else _strides3(mask), ctx.terms, ctx.valid, _ptr(grad_out),
                *_plane_ptrs(planes), _ptr(grad), _strides(grad)),
                "grut_photo_loss_backward")
        return grad, None, None, None, None, None


def _photo_mask(mask, b, h, w, device, channels_first):
    """-> the mask as a [B, H, W] view (no copy), or an error naming what is wrong."""
    if not isinstance(mask, torch.Tensor):
        raise TypeError("mask must be a tensor or None")
    if not mask.is_cuda or mask.device != device:
        raise RuntimeError("mask must be a CUDA tensor on the images' device (there is no CPU fallback)")
    if mask.dtype != torch.float32:
        raise RuntimeError(f"mask must be float32 (got {mask.dtype})")
    shape = tuple(mask.shape)
    if shape == (b, h, w):
        return mask.detach()
    if shape == (b, h, w, 1) and not channels_first:
        return mask.detach()[..., 0]
    if shape == (b, 1, h, w) and channels_first:
        return mask.detach()[:, 0]
    expect = f"[{b}, 1, {h}, {w}]" if channels_first else f"[{b}, {h}, {w}, 1]"
    raise RuntimeError(f"mask must be [{b}, {h}, {w}] or {expect} (got {list(shape)})")


def photometric_loss(pred: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor | None = None, *, l1: bool = True, l2: bool = False,
                     ssim: bool = True, padding: str = "valid", channels_first: bool = False):
    """What Trainer3DGRUT.get_losses computes from the rendered and the ground-truth image (trainer.py:687-720), as (l1, l2, ssim):
    0-dim fp32 tensors on the current stream, None for a term that is not asked for.  With a = mask * pred and b = mask * gt (a = pred,
    b = gt without a mask):  l1 = mean |a - b|,  l2 = mean (pred - b)^2 (the reference's mse_loss takes the UNMASKED prediction,
    trainer.py:709),  ssim = mean SSIM(a, b) with `padding` as in fused_ssim (the trainer's `ssim()` is "valid").

    pred, gt: fp32 CUDA [B, H, W, C] (the renderer's output), or [B, C, H, W] with channels_first=True; read in place through their
    strides.  mask: fp32 [B, H, W] or [B, H, W, 1] ([B, 1, H, W] with channels_first), broadcast over the channels.  Differentiable in
    pred only; the gradients of all requested outputs are accumulated in a single backward launch and arrive in pred's own layout.
    Under torch.no_grad(), or when pred does not require grad, only the values are computed and no derivative plane is allocated."""
    if not (l1 or l2 or ssim):
        raise ValueError("at least one of l1, l2, ssim must be asked for")
    for t, name in ((pred, "pred"), (gt, "gt")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor")
        if t.dim() != 4:
            raise RuntimeError(f"{name} must be {'[B, C, H, W]' if channels_first else '[B, H, W, C]'} (got {t.dim()} dimensions)")
    img1, img2 = (pred, gt) if channels_first else (pred.permute(0, 3, 1, 2), gt.permute(0, 3, 1, 2))
    _check_padding(padding)
    _check_input(img1, img2, padding if ssim else "same")   # the window's size limit only binds the SSIM term
    b, _, h, w = (int(s) for s in img1.shape)
    if mask is not None:
        mask = _photo_mask(mask, b, h, w, img1.device, channels_first)
    img1, img2 = _in_place(img1), _in_place(img2)
    train = torch.is_grad_enabled() and img1.requires_grad
    if not train:
        img1 = img1.detach()
    terms = (TERM_L1 if l1 else 0) | (TERM_L2 if l2 else 0) | (TERM_SSIM if ssim else 0)
    out = _PhotometricLoss.apply(img1, img2.detach(), mask, terms, 1 if padding == "valid" else 0, train)
    return tuple(v if on else None for v, on in zip(out, (l1, l2, ssim)))


def _fusable(pred, gt, mask, use_ssim):
    """The preconditions of the trainer hook's fused call; anything else goes to the reference's own get_losses."""
    for t in (pred, gt):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4):
            return False
    if pred.shape != gt.shape or pred.device != gt.device or pred.numel() == 0:
        return False
    b, h, w, c = (int(s) for s in pred.shape)
    if c > MAX_FUSED_CHANNELS or b * c > MAX_PLANES:
        return False
    if use_ssim and (h < WINDOW or w < WINDOW):
        return False
    if mask is not None and not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.device == pred.device and mask.dtype == torch.float32
                                 and tuple(mask.shape) == (b, h, w, 1)):   # the one shape the reference's own products broadcast
        return False
    return True


def install_fused_losses():
    """Opt-in: replace threedgrut.trainer.Trainer3DGRUT.get_losses IN PLACE on the class (so it holds however train.py imported the class)
    with a method that makes one photometric_loss call for the masking, L1, L2 and SSIM of trainer.py:687-720 and returns the reference's
    dict: the same six keys, the same weighting, torch.zeros(1) for disabled terms, the opacity and scale regularisers in torch as the
    reference has them (in one HIP call after regularizers.install_fused_regularizers(), which is off by default).
    outputs["pred_features"] is not replaced.  Whenever a precondition of the fused call does not hold (pred or gt
    not an fp32 CUDA [B, H, W, C] tensor, C > 4, B * C over the kernels' limit, H or W below 11 with SSIM on, a mask that is not an fp32
    [B, H, W, 1] tensor on that device, or no image term enabled) the reference's own method runs.  Returns the new method;
    calling it again returns the same one."""
    cls = __import__("threedgrut.trainer", fromlist=["Trainer3DGRUT"]).Trainer3DGRUT
    if getattr(cls.get_losses, "_grut_fused_losses", False):
        return cls.get_losses
    original = cls.get_losses

    def get_losses(self, gpu_batch, outputs):
        conf = self.conf.loss
        rgb_gt, rgb_pred, mask = gpu_batch.rgb_gt, outputs["pred_features"], gpu_batch.mask
        use_l1, use_l2, use_ssim = bool(conf.use_l1), bool(conf.use_l2), bool(conf.use_ssim)
        if not (use_l1 or use_l2 or use_ssim) or not _fusable(rgb_pred, rgb_gt, mask, use_ssim):
            return original(self, gpu_batch, outputs)
        l1, l2, ssim_mean = photometric_loss(rgb_pred, rgb_gt, mask, l1=use_l1, l2=use_l2, ssim=use_ssim, padding="valid")

        loss_l1, lambda_l1 = (l1, conf.lambda_l1) if use_l1 else (torch.zeros(1, device=self.device), 0.0)
        loss_l2, lambda_l2 = (l2, conf.lambda_l2) if use_l2 else (torch.zeros(1, device=self.device), 0.0)
        loss_ssim, lambda_ssim = (1.0 - ssim_mean, conf.lambda_ssim) if use_ssim else (torch.zeros(1, device=self.device), 0.0)
        means = None   # regularizers.install_fused_regularizers(): both means in one HIP call; None where the two torch lines have to run
        if regularizers.enabled() and not self._in_color_refine and (conf.use_opacity or conf.use_scale):
            means = regularizers.trainer_means(self.model, bool(conf.use_opacity), bool(conf.use_scale))
        loss_opacity, lambda_opacity = torch.zeros(1, device=self.device), 0.0
        if conf.use_opacity and not self._in_color_refine:
            loss_opacity, lambda_opacity = torch.abs(self.model.get_density()).mean() if means is None else means[0], conf.lambda_opacity
        loss_scale, lambda_scale = torch.zeros(1, device=self.device), 0.0
        if conf.use_scale and not self._in_color_refine:
            loss_scale, lambda_scale = torch.abs(self.model.get_scale()).mean() if means is None else means[1], conf.lambda_scale

        loss = lambda_l1 * loss_l1 + lambda_ssim * loss_ssim + lambda_opacity * loss_opacity + lambda_scale * loss_scale
        return dict(total_loss=loss, l1_loss=lambda_l1 * loss_l1, l2_loss=lambda_l2 * loss_l2, ssim_loss=lambda_ssim * loss_ssim,
                    opacity_loss=lambda_opacity * loss_opacity, scale_loss=lambda_scale * loss_scale)

    get_losses.__doc__ = original.__doc__
    get_losses = torch.cuda.nvtx.range("get_losses")(get_losses)   # the range the reference's method carries (trainer.py:676)
    get_losses._grut_fused_losses = True
    get_losses._grut_original = original
    cls.get_losses = get_losses
    return get_losses
