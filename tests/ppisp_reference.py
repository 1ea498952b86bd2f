"""The PPISP camera model restated in torch, float64 by default, with the gradient rules at its kinks written as explicit masks
(gradients come from autograd).  Shared by tests/test_ppisp_cpu.py, tests/test_ppisp_gpu.py and tests/golden/make_ppisp_golden.py.

    ppisp_model(rgb [...,3], pixel_coords [...,2] | None, (W, H), exposure [1] | None, color [8] | None, vignetting [3,5] | None,
                crf [3,4] | None, dtype=torch.float64) -> [...,3]

A parameter that is None makes its stage the identity.  Kink rules: the vignetting polynomial p passes gradient where 0 <= p <= 1
(inclusive); a channel whose input to the response curve is <= 0 or >= 1 passes no gradient through the curve, neither to the input nor
to the curve's parameters; the branch the homography's cross product took is a constant.
"""
import math

import numpy as np
import torch

LATENT_MAPS = (((0.0480542, -0.0043631), (-0.0043631, 0.0481283)),      # blue
               ((0.0580570, -0.0179872), (-0.0179872, 0.0431061)),      # red
               ((0.0433336, -0.0180537), (-0.0180537, 0.0580500)),      # green
               ((0.0128369, -0.0034654), (-0.0034654, 0.0128158)))      # neutral
CRF_IDENTITY = (math.log(math.expm1(0.7)), math.log(math.expm1(0.7)), math.log(math.expm1(0.9)), 0.0)
SHAPES = ((7, 9), (37, 45), (64, 33), (32, 32))    # (H, W); 32 x 32 = 1024 pixels: exactly one of the kernels' 1024-pixel blocks
KINK_MARGIN = 1e-3
MAX_LEFT_OUT = 0.05


def _skew(n):
    z = torch.zeros((), dtype=n.dtype, device=n.device)
    return torch.stack([torch.stack([z, -n[2], n[1]]), torch.stack([n[2], z, -n[0]]), torch.stack([-n[1], n[0], z])])


def homography(color):
    """[8] latents -> the normalised 3x3."""
    dt, dev = color.dtype, color.device
    maps = torch.tensor(LATENT_MAPS, dtype=dt, device=dev)
    o = torch.einsum("kij,kj->ki", maps, color.reshape(4, 2))
    one = torch.ones((), dtype=dt, device=dev)
    t_b = torch.stack([o[0, 0], o[0, 1], one])
    t_r = torch.stack([1 + o[1, 0], o[1, 1], one])
    t_g = torch.stack([o[2, 0], 1 + o[2, 1], one])
    t_n = torch.stack([1.0 / 3.0 + o[3, 0], 1.0 / 3.0 + o[3, 1], one])
    t = torch.stack([t_b, t_r, t_g], dim=1)
    a = _skew(t_n) @ t
    lam = torch.linalg.cross(a[0], a[1])
    if float((lam.detach() ** 2).sum()) < 1e-20:
        lam = torch.linalg.cross(a[0], a[2])
        if float((lam.detach() ** 2).sum()) < 1e-20:
            lam = torch.linalg.cross(a[1], a[2])
    s = torch.tensor([[-1.0, -1.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=dt, device=dev)
    h = t @ torch.diag(lam) @ s
    if abs(float(h[2, 2].detach())) > 1e-20:
        h = h / h[2, 2]
    return h


def curve_parameters(crf):
    """[3,4] raw -> toe, shoulder, gamma, centre, a, b; each [3]."""
    sp = torch.nn.functional.softplus
    toe, shoulder, gamma = 0.3 + sp(crf[:, 0]), 0.3 + sp(crf[:, 1]), 0.1 + sp(crf[:, 2])
    sg = torch.sigmoid(crf[:, 3])
    inside = (sg >= 1e-6) & (sg <= 1 - 1e-6)
    centre = torch.where(inside, sg, sg.detach().clamp(1e-6, 1 - 1e-6))
    lraw = (shoulder - toe) * centre + toe
    lerp = torch.where(lraw >= 1e-6, lraw, torch.full_like(lraw, 1e-6))
    a = shoulder * centre / lerp
    return toe, shoulder, gamma, centre, a, 1 - a


def curve_input(rgb, pixel_coords, resolution, exposure, color, vignetting, dtype=torch.float64):
    """The three stages in front of the response curve -> [...,3]."""
    x = rgb.to(dtype)
    if exposure is not None:
        x = x * torch.exp2(exposure.to(dtype).reshape(()))
    if vignetting is not None:
        w, h = float(resolution[0]), float(resolution[1])
        vig = vignetting.to(dtype).reshape(3, 5)
        uv = (pixel_coords.to(dtype) - torch.tensor([w / 2, h / 2], dtype=dtype, device=x.device)) / max(w, h)
        d = uv[..., None, :] - vig[:, :2]                                  # [...,3,2]
        r2 = (d * d).sum(-1)
        p = 1 + vig[:, 2] * r2 + vig[:, 3] * r2 ** 2 + vig[:, 4] * r2 ** 3
        passes = (p >= 0) & (p <= 1)                                        # inclusive
        x = x * torch.where(passes, p, p.detach().clamp(0, 1))
    if color is not None:
        hm = homography(color.to(dtype).reshape(8))
        inten = x.sum(-1, keepdim=True)
        v = torch.cat([x[..., :2], inten], -1) @ hm.T
        v = v * (inten / (v[..., 2:3] + 1e-5))
        x = torch.cat([v[..., :2], v[..., 2:3] - v[..., 0:1] - v[..., 1:2]], -1)
    return x


def response_curve(z, crf):
    toe, shoulder, gamma, centre, a, b = curve_parameters(crf.to(z.dtype).reshape(3, 4))
    active = (z > 0) & (z < 1)
    zs = torch.where(active, z, torch.full_like(z, 0.5))                    # a safe stand-in where no gradient may pass
    lo = zs <= centre
    below = a * (torch.where(lo, zs, centre.expand_as(zs)) / centre) ** toe
    above = 1 - b * ((1 - torch.where(lo, centre.expand_as(zs), zs)) / (1 - centre)) ** shoulder
    y = torch.where(lo, below, above)
    positive = y > 0
    live = torch.where(positive, y, torch.ones_like(y)) ** gamma * positive
    with torch.no_grad():                                                   # the clamped ends: a constant
        zc = z.clamp(0, 1)
        lo_c = zc <= centre
        y_c = torch.where(lo_c, a * (zc / centre) ** toe, 1 - b * ((1 - zc) / (1 - centre)) ** shoulder)
        dead = y_c.clamp_min(0) ** gamma
    return torch.where(active, live, dead)


def ppisp_model(rgb, pixel_coords, resolution, exposure=None, color=None, vignetting=None, crf=None, dtype=torch.float64):
    z = curve_input(rgb, pixel_coords, resolution, exposure, color, vignetting, dtype)
    return z if crf is None else response_curve(z, crf)


# ---- the suite's inputs -------------------------------------------------------------------------------------------------------------------
def make_image(h, w, seed):
    """[H,W,3] fp32 with exactly-black and saturated pixels, roughly a third of the samples below the curve's centre."""
    g = torch.Generator().manual_seed(seed)
    img = torch.nn.functional.avg_pool2d(torch.rand(1, 3, h + 4, w + 4, generator=g), 5, 1)
    return ((img - 0.5) * 4 + 0.6).clamp_min(0)[0].permute(1, 2, 0).contiguous()


def pixel_coords(h, w):
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    return torch.stack((x, y), -1) + 0.5


def identity_parameters():
    return dict(exposure=torch.zeros(1), color=torch.zeros(8), vignetting=torch.zeros(3, 5),
                crf=torch.tensor(CRF_IDENTITY, dtype=torch.float32).repeat(3, 1))


def random_parameters(seed):
    """Drawn as the reference's own export test draws them."""
    g = torch.Generator().manual_seed(seed)
    p = identity_parameters()
    p["exposure"] = torch.empty(1).uniform_(-0.35, 0.35, generator=g)
    p["color"] = torch.empty(8).normal_(0.0, 0.35, generator=g)
    p["vignetting"][:, :2] = torch.empty(3, 2).normal_(0.0, 0.04, generator=g)
    p["vignetting"][:, 2:] = torch.empty(3, 3).uniform_(-0.35, 0.02, generator=g)
    p["crf"] = p["crf"] + torch.empty(3, 4).normal_(0.0, 0.08, generator=g)
    return p


GROUPS = ("exposure", "color", "vignetting", "crf")
# which groups are present: all four; each one missing (NULL) in turn; none
CONFIGS = [GROUPS] + [tuple(g for g in GROUPS if g != off) for off in GROUPS] + [()]


def load_golden(path):
    """-> list of dicts: name, h, w, rgb [H,W,3], pc [H,W,2], the four parameter tensors, ref32 [H,W,3], e_ref."""
    z = np.load(path)
    cases = []
    for name in [str(n) for n in z["names"]]:
        shape = name.split("_")[0]
        c = dict(name=name, ref32=torch.from_numpy(z[f"{name}/ref32"]), e_ref=float(z[f"{name}/e_ref"]),
                 rgb=torch.from_numpy(z[f"{shape}/rgb"]), **{k: torch.from_numpy(z[f"{name}/{k}"]) for k in GROUPS})
        c["h"], c["w"] = int(c["rgb"].shape[0]), int(c["rgb"].shape[1])
        c["pc"] = pixel_coords(c["h"], c["w"])
        cases.append(c)
    return cases


def kink_free(case, groups=GROUPS):
    """[H,W] bool: pixels whose three curve inputs all keep KINK_MARGIN from 0, 1 and the centre; an exact 0 is kept.  The inputs are
    evaluated in float64 AND in float32 and a pixel is left out when either evaluation is near a kink: with blue = intensity - red - green
    a blue input of exactly 0 reaches the curve as the residue of a cancellation, which float64 may round to an exact 0 while float32
    lands 1e-8 to either side of the kink - such a pixel is at the kink, whatever one of the two evaluations says."""
    par = {k: (case[k] if k in groups else None) for k in GROUPS}
    if par["crf"] is None:
        return torch.ones(case["rgb"].shape[:-1], dtype=torch.bool)
    near = torch.zeros(case["rgb"].shape[:-1], dtype=torch.bool)
    for dtype in (torch.float64, torch.float32):
        z = curve_input(case["rgb"], case["pc"], (case["w"], case["h"]), par["exposure"], par["color"], par["vignetting"], dtype)
        centre = curve_parameters(par["crf"].to(dtype))[3]
        near |= (((z.abs() < KINK_MARGIN) & (z != 0)) | ((z - 1).abs() < KINK_MARGIN) | ((z - centre).abs() < KINK_MARGIN)).any(-1)
    return ~near


def gradients(case, grad_out, keep, groups=GROUPS, dtype=torch.float64):
    """Autograd of sum(out * grad_out * keep) in `dtype` -> (out, dict of gradients: rgb and every group in `groups`)."""
    leaves = {"rgb": case["rgb"].to(dtype).clone().requires_grad_(True)}
    for k in groups:
        leaves[k] = case[k].to(dtype).clone().requires_grad_(True)
    par = {k: leaves.get(k) for k in GROUPS}
    out = ppisp_model(leaves["rgb"], case["pc"], (case["w"], case["h"]), par["exposure"], par["color"], par["vignetting"], par["crf"], dtype)
    (out * (grad_out.to(dtype) * keep[..., None].to(dtype))).sum().backward()
    return out.detach(), {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in leaves.items()}
