"""The playground's frame denoiser on the MI355X, backed by csrc/denoise.hip: what `playground_tracer.Tracer.denoise` calls.

The reference's engine hands its tonemapped RGB frame to `Tracer.denoise` at the end of every render pass
(threedgrut_playground/engine.py:1091-1094 -> tracer.py:269-271 -> hybridTracer.h:143), which runs OptiX's learned LDR denoiser on RGB
alone.  Those weights are not public, so the ALGORITHM here is this project's choice: classic non-local means (Buades, Coll, Morel
2005).  It needs RGB only, is an exact formula, and removes the isolated outliers a path tracer leaves.

    denoise(rgb, patch_radius=3, search_radius=7, h=0.1)     one HIP launch for fp32 CUDA frames; anything else runs denoise_torch
    denoise_torch(rgb, patch_radius=3, search_radius=7, h=0.1)   the same model in torch: the fallback and the readable statement

The model (include/grut_amd.h: grut_denoise), with f = patch_radius, r = search_radius, n = 3 (2f+1)^2, for a pixel p
and every OTHER pixel q of the same image with |q - p|_inf <= r:

    d2(p,q) = sum over o in [-f,f]^2 and the channels of (I[clamp(p+o)] - I[clamp(q+o)])^2
    w(p,q)  = exp(-min(d2(p,q) / (n h^2), 80))          w(p,p) = max_q w(p,q), or 1 when there is no q (a 1x1 image)
    out[p]  = (sum_q w(p,q) I[q] + w(p,p) I[p]) / (sum_q w(p,q) + w(p,p))

Out of place: the result is a new tensor and the input is never written.  h = 0.1 is a choice, not a measurement: two patches of one
surface under noise of sigma 0.1 differ by d2 / n = 2 sigma^2 on average, so h^2 is half the per-element patch distance such noise
produces and those patches get x = 2.  scripts/bench_denoise.py records what the default does on path-traced frames.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _abi

TILE_W, TILE_H = 32, 16          # kDenoiseTileW, kDenoiseTileH of csrc/denoise.hip: a workgroup's tile of output pixels
MAX_PATCH_RADIUS, MAX_SEARCH_RADIUS = 4, 16
X_MAX = 80.0                     # the exponent's clamp: no weight is below e^-80
MAX_PIXELS = 2 ** 31 - 1         # batch * height * width of the HIP path
DEFAULTS = {"patch_radius": 3, "search_radius": 7, "h": 0.1}
# plain counters, not synchronised across threads: calls that took the kernel, calls evaluated by denoise_torch
stats = {"hip_calls": 0, "torch_calls": 0}


def check_parameters(patch_radius, search_radius, h):
    """The rules of grut_denoise, as ValueError: f in 0..4, r in 1..16 (both integers), h finite and > 0.  -> (f, r, h)"""
    for name, v, lo, hi in (("patch_radius", patch_radius, 0, MAX_PATCH_RADIUS), ("search_radius", search_radius, 1, MAX_SEARCH_RADIUS)):
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
            raise ValueError(f"denoise: {name} = {v!r}, must be an integer in {lo}..{hi}")
    h = float(h)
    if not (math.isfinite(h) and h > 0.0):
        raise ValueError(f"denoise: h = {h!r}, must be finite and above 0")
    return int(patch_radius), int(search_radius), h


def _as_batch(rgb):
    if not (isinstance(rgb, torch.Tensor) and rgb.dim() in (3, 4) and rgb.shape[-1] == 3 and rgb.is_floating_point()):
        raise ValueError("denoise: rgb must be a floating-point tensor [B, H, W, 3] or [H, W, 3]")
    batch = rgb if rgb.dim() == 4 else rgb[None]
    if batch.shape[1] == 0 or batch.shape[2] == 0:
        raise ValueError(f"denoise: height and width must be at least 1, got {tuple(rgb.shape)}")
    return batch


def denoise_torch(rgb, patch_radius=3, search_radius=7, h=0.1):
    """The model above in torch, on rgb's device: [B, H, W, 3] or [H, W, 3] of any floating dtype -> a new tensor of the same shape and
    dtype.  float64 is evaluated in float64, everything else in float32.  One pass per candidate offset: the squared-difference image
    of the frame against its shifted self, box-summed over the patch as 2f+1 row shifts and 2f+1 column shifts."""
    f, r, h = check_parameters(patch_radius, search_radius, h)
    batch = _as_batch(rgb)
    work = batch.detach().to(torch.float64 if batch.dtype == torch.float64 else torch.float32)
    B, H, W, _ = work.shape
    R = r + f
    # clamp(p + o) is replicate padding; index [R + y, R + x] of `padded` is pixel (y, x)
    planes = work.permute(0, 3, 1, 2)
    ys = torch.arange(-R, H + R, device=work.device).clamp_(0, H - 1)
    xs = torch.arange(-R, W + R, device=work.device).clamp_(0, W - 1)
    padded = planes[:, :, ys][:, :, :, xs]
    scale = 1.0 / (3 * (2 * f + 1) ** 2 * h * h)
    row = torch.arange(H, device=work.device)[:, None]
    col = torch.arange(W, device=work.device)[None, :]
    # the frame over the pixels p + o, o in [-f, f]^2: padded rows r .. r + H + 2f
    mine = padded[:, :, r:r + H + 2 * f, r:r + W + 2 * f]
    num = torch.zeros_like(planes)
    den = torch.zeros((B, 1, H, W), dtype=work.dtype, device=work.device)
    w_max = torch.zeros_like(den)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx == 0 and dy == 0:
                continue
            theirs = padded[:, :, r + dy:r + dy + H + 2 * f, r + dx:r + dx + W + 2 * f]
            sq = ((mine - theirs) ** 2).sum(dim=1, keepdim=True)                     # D_d over the pixels p + o
            cols = sq[:, :, 0:H]
            for oy in range(1, 2 * f + 1):
                cols = cols + sq[:, :, oy:oy + H]
            d2 = cols[:, :, :, 0:W]
            for ox in range(1, 2 * f + 1):
                d2 = d2 + cols[:, :, :, ox:ox + W]
            w = torch.exp(-torch.clamp(d2 * scale, max=X_MAX))
            inside = ((row + dy >= 0) & (row + dy < H) & (col + dx >= 0) & (col + dx < W))[None, None]   # q is a pixel of the image
            w = torch.where(inside, w, torch.zeros_like(w))
            num = num + w * padded[:, :, R + dy:R + dy + H, R + dx:R + dx + W]
            den = den + w
            w_max = torch.maximum(w_max, w)
    if H * W == 1:            # no other pixel: the centre's weight is 1 and the image comes back as it is
        w_max = torch.ones_like(w_max)
    out = (num + w_max * planes) / (den + w_max)
    return out.permute(0, 2, 3, 1).reshape(rgb.shape).to(rgb.dtype).contiguous()


def _hip_eligible(batch) -> bool:
    return batch.is_cuda and batch.dtype == torch.float32 and 0 < batch.numel() // 3 <= MAX_PIXELS


def denoise(rgb, patch_radius=3, search_radius=7, h=0.1):
    """Non-local means of a frame, out of place: rgb [B, H, W, 3] or [H, W, 3] -> a new tensor of the same shape, dtype and device; rgb
    is never written.  fp32 CUDA frames (made contiguous if they are not) take csrc/denoise.hip on the current stream: one launch, no
    atomics, two calls bitwise equal.  Any other device or dtype is evaluated by denoise_torch; `stats` counts both.  Parameters
    outside f in 0..4, r in 1..16, h > 0 raise ValueError on either path."""
    f, r, h = check_parameters(patch_radius, search_radius, h)
    batch = _as_batch(rgb)
    if not _hip_eligible(batch):
        stats["torch_calls"] += 1
        return denoise_torch(rgb, f, r, h)
    src = batch.detach().contiguous()
    out = torch.empty_like(src)
    cfg = _abi.GrutDenoiseConfig(f, r, h)
    stats["hip_calls"] += 1
    with torch.cuda.device(src.device):   # the launch goes to the frame's device, whichever is current
        _abi.check(_abi.load_library().grut_denoise(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(cfg), int(src.shape[0]),
                                                    int(src.shape[1]), int(src.shape[2]), C.c_void_p(src.data_ptr()),
                                                    C.c_void_p(out.data_ptr())), "grut_denoise")
    return out.reshape(rgb.shape)
