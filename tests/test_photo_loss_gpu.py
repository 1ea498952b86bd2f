"""GPU: the fused photometric loss (loss_*_kernel of csrc/loss.hip through 3dgrut_amd.losses.photometric_loss) against a float64 torch
evaluation of what Trainer3DGRUT.get_losses takes from the two images (trainer.py:687-720), the SSIM part from tests/ssim_reference.py:

    a = m pred, b = m gt;   l1 = mean |a - b|;   l2 = mean (pred - b)^2  (the UNMASKED prediction: trainer.py:709);   ssim = mean SSIM(a, b)
    d/dpred = m dSSIM/da  +  g_l1 m sign(a - b) / P  +  2 g_l2 (pred - b) / P,      P = B C H W

Bounds (none fitted, u = 2^-24):
  * ssim value and the SSIM part of the gradient: the bounds ssim_reference.py derives from the float64 intermediates, evaluated at (a, b)
    with the upstream weight of the SSIM output (so the gradient bound is the existing one scaled by |g_ssim|), times m for the gradient.
  * l1 and l2 values: DEPTH u sum|term| / P.  A term passes through at most 3 roundings of its own (the subtraction, the square, the
    first addition) and a chain of fp32 additions: the lane that stages an element adds it to its running sum, at most
    ceil(42 * 42 * NC / 256) elements per lane (NC channels per workgroup: 21 for RGB channels-last, 7 for a plane), then 6 levels of
    the wave sum, 3 additions over the four waves, and one rounding of the fp64 total to fp32: DEPTH = that + 6 + 3 + 3 + 1.
  * the L1 and L2 parts of the gradient: 2 ulp (4 u) of each term's own size: g / P is rounded once, the product(s) with m sign or with
    (pred - b) once or twice, and adding the term to the rest rounds once more.
  * the L1 gradient alone is exact: m sign(a - b) / P rounded to fp32 once.
The bounds treat a and b as exact.  They are when there is no mask or a binary one; for the fractional mask the inputs are put on a grid
(images on multiples of 2^-12, mask on multiples of 1/8) on which m pred and m gt are exact in fp32, so the float64 reference and the
kernels see the same a and b.

Shapes: 11x11 (one valid pixel), 37x45 (two tiles each way, neither a multiple of the 32x32 tile, inside the halo), 64x33 (an exact tile
multiple down, one pixel over across), always B = 2; RGB channels-last as the renderer writes it and one planar channel.  The anchor
test also takes planar RGB and channels-last images of 2 and 4 channels, so that every channels-per-workgroup instantiation (1..4) runs.
Every test here needs `photometric_loss`, which the parent commit does not have."""
import ctypes as C
import functools
import importlib
import math
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssim_reference as ref

pytestmark = pytest.mark.gpu
U = ref.U
SHAPES = [(11, 11), (37, 45), (64, 33)]
LAYOUTS = [("nhwc", 3), ("nchw", 1)]
MASKS = ["none", "binary", "fractional", "zero"]
WEIGHTS = tuple(float(np.float32(v)) for v in (0.8, 0.3, -0.2))   # upstream weights of (l1, l2, ssim): 0.8 l1 + 0.3 l2 + 0.2 (1 - ssim)


def _losses():
    return importlib.import_module("3dgrut_amd.losses")


def _depth(nc):
    return math.ceil(42 * 42 * nc / 256) + 6 + 3 + 3 + 1


@functools.lru_cache(maxsize=None)
def _case(h, w, layout, c, mask_kind, padding="valid"):
    """Inputs on the CPU as [B, H, W, C] (and the mask as [B, H, W, 1]) and the float64 reference with its bounds; computed once per case
    and shared by the tests below, which do not modify it."""
    b = 2
    g = torch.Generator().manual_seed(1000 * h + 10 * w + c + 7 * MASKS.index(mask_kind))
    base = torch.rand((b, c, h + 8, w + 8), generator=g)
    pred = F.avg_pool2d(base, 9, 1).permute(0, 2, 3, 1).contiguous()                     # smooth, like a render
    gt = (pred + 0.05 * torch.randn((b, h, w, c), generator=g)).clamp(0, 1)
    gt[:, : h // 3, : w // 2] = pred[:, : h // 3, : w // 2]                              # a block of pixels with pred == gt: sign(0) = 0
    mask = None
    if mask_kind == "binary":
        mask = (torch.rand((b, h, w, 1), generator=g) < 0.7).float()
    elif mask_kind == "fractional":
        mask = torch.randint(0, 9, (b, h, w, 1), generator=g).float() / 8.0
        pred, gt = torch.round(pred * 4096.0) / 4096.0, torch.round(gt * 4096.0) / 4096.0
    elif mask_kind == "zero":
        mask = torch.zeros((b, h, w, 1))
    p64, g64 = pred.double(), gt.double()
    m64 = torch.ones((b, h, w, 1), dtype=torch.float64) if mask is None else mask.double()
    a64, b64 = p64 * m64, g64 * m64
    if mask is not None:
        assert torch.equal(a64, (pred * mask).double()) and torch.equal(b64, (gt * mask).double()), "m pred and m gt must be exact in fp32"
    n = float(p64.numel())
    out = dict(pred=pred, gt=gt, mask=mask, P=n, nc=c if layout == "nhwc" else 1)
    out["l1"], out["l2"] = float((a64 - b64).abs().mean()), float(((p64 - b64) ** 2).mean())
    out["l1_bound"], out["l2_bound"] = _depth(out["nc"]) * U * out["l1"], _depth(out["nc"]) * U * out["l2"]
    out["l1_grad_unit"] = m64 * torch.sign(a64 - b64) / n                                # [B, H, W, C] by broadcast
    out["l2_grad_unit"] = 2.0 * (p64 - b64) / n
    if h >= 11 and w >= 11:
        r = ref.reference_and_bounds(a64.permute(0, 3, 1, 2), b64.permute(0, 3, 1, 2), padding, upstream=WEIGHTS[2])
        out["ssim"], out["ssim_bound"] = r["value"], r["value_bound"]
        out["ssim_grad"] = m64 * r["grad"].permute(0, 2, 3, 1)                            # upstream weight included
        out["ssim_grad_bound"] = m64 * r["grad_bound"].permute(0, 2, 3, 1)
    return out


def _device_inputs(case, layout):
    """pred as a leaf in the layout's own memory; what photometric_loss takes, and the keyword that goes with it."""
    if layout == "nhwc":
        pred = case["pred"].cuda().requires_grad_(True)
        return pred, case["gt"].cuda(), None if case["mask"] is None else case["mask"].cuda(), {}
    pred = case["pred"].permute(0, 3, 1, 2).contiguous().cuda().requires_grad_(True)
    mask = None if case["mask"] is None else case["mask"].permute(0, 3, 1, 2).contiguous().cuda()
    return pred, case["gt"].permute(0, 3, 1, 2).contiguous().cuda(), mask, {"channels_first": True}


def _to_nhwc(t, layout):
    return t if layout == "nhwc" else t.permute(0, 2, 3, 1)


def _run(case, layout, weights=None, **terms):
    pred, gt, mask, kw = _device_inputs(case, layout)
    out = _losses().photometric_loss(pred, gt, mask, **terms, **kw)
    if weights is not None:
        sum(wt * v for wt, v in zip(weights, out) if v is not None).backward()
        assert pred.grad.shape == pred.shape and pred.grad.is_contiguous(), "the gradient must come in pred's own layout"
    return out, (None if pred.grad is None else _to_nhwc(pred.grad, layout).cpu().double())


# ---- anchor: without a mask and with only the SSIM term, this IS fused_ssim -----------------------------------------------------------
@pytest.mark.parametrize("padding", ["valid", "same"])
@pytest.mark.parametrize("layout,c", LAYOUTS + [("nchw", 3), ("nhwc", 2), ("nhwc", 4)])   # NC = 3, 1, 1, 2, 4 channels per workgroup
@pytest.mark.parametrize("h,w", SHAPES)
def test_ssim_term_alone_is_bitwise_fused_ssim(h, w, layout, c, padding):
    losses = _losses()
    case = _case(h, w, layout, c, "none")
    pred, gt, _, kw = _device_inputs(case, layout)
    l1, l2, s = losses.photometric_loss(pred, gt, None, l1=False, l2=False, ssim=True, padding=padding, **kw)
    assert l1 is None and l2 is None and s.dim() == 0 and s.dtype == torch.float32
    (-0.2 * s).backward()
    leaf = pred.detach().clone().requires_grad_(True)
    views = (leaf, gt) if layout == "nchw" else (leaf.permute(0, 3, 1, 2), gt.permute(0, 3, 1, 2))
    v = losses.fused_ssim(*views, padding=padding)
    (-0.2 * v).backward()
    assert torch.equal(s.detach(), v.detach()), (float(s), float(v))
    assert torch.equal(pred.grad, leaf.grad) and pred.grad.stride() == leaf.grad.stride()


# ---- values --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("layout,c", LAYOUTS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_values_match_float64(h, w, layout, c, mask_kind):
    case = _case(h, w, layout, c, mask_kind)
    (l1, l2, s), _ = _run(case, layout, l1=True, l2=True, ssim=True)
    d1, d2, ds = abs(float(l1) - case["l1"]), abs(float(l2) - case["l2"]), abs(float(s) - case["ssim"])
    print(f"{h}x{w} {layout} C={c} mask={mask_kind}: l1 {case['l1']:.6e} err {d1:.2e} (bound {case['l1_bound']:.2e}); l2 {case['l2']:.6e} err {d2:.2e} "
          f"(bound {case['l2_bound']:.2e}); ssim {case['ssim']:.6f} err {ds:.2e} (bound {case['ssim_bound']:.2e})")
    assert all(np.isfinite(float(v)) for v in (l1, l2, s))
    assert d1 <= case["l1_bound"] and d2 <= case["l2_bound"] and ds <= case["ssim_bound"]
    if mask_kind == "zero":
        assert float(l1) == 0.0 and abs(float(s) - 1.0) <= case["ssim_bound"]


def test_l1_and_l2_below_the_window_size():
    """Without the SSIM term the 11x11 window's size limit does not apply; with it, the call is refused before any launch."""
    case = _case(7, 9, "nhwc", 3, "binary")
    (l1, l2, s), grad = _run(case, "nhwc", weights=WEIGHTS, l1=True, l2=True, ssim=False)
    assert s is None and abs(float(l1) - case["l1"]) <= case["l1_bound"] and abs(float(l2) - case["l2"]) <= case["l2_bound"]
    t1, t2 = WEIGHTS[0] * case["l1_grad_unit"], WEIGHTS[1] * case["l2_grad_unit"]
    assert bool(((grad - (t1 + t2)).abs() <= 4 * U * (t1.abs() + t2.abs())).all())
    with pytest.raises(RuntimeError, match="H, W >= 11"):
        _run(case, "nhwc", l1=True, l2=False, ssim=True)


# ---- gradients -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("layout,c", LAYOUTS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_l1_gradient_is_exact(h, w, layout, c, mask_kind):
    case = _case(h, w, layout, c, mask_kind)
    _, grad = _run(case, layout, weights=(1.0, 0.0, 0.0), l1=True, l2=False, ssim=False)
    expect = case["l1_grad_unit"].expand_as(grad).float()                   # m sign(m (pred - gt)) / P rounded to fp32
    assert int((expect == 0).sum()) >= (h // 3) * (w // 2) * 2 * c          # the pred == gt block (and whatever the mask removes)
    assert torch.equal(grad.float(), expect)


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("layout,c", LAYOUTS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_combined_gradient_with_distinct_upstream_weights(h, w, layout, c, mask_kind):
    case = _case(h, w, layout, c, mask_kind)
    _, grad = _run(case, layout, weights=WEIGHTS, l1=True, l2=True, ssim=True)
    t1, t2 = WEIGHTS[0] * case["l1_grad_unit"], WEIGHTS[1] * case["l2_grad_unit"]
    expect = case["ssim_grad"] + t1 + t2
    bound = case["ssim_grad_bound"] + 4 * U * (t1.abs() + t2.abs())
    err = (grad - expect).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
    print(f"{h}x{w} {layout} C={c} mask={mask_kind}: gradient max {float(expect.abs().max()):.3e}, error max {float(err.max()):.3e}, worst error / bound {worst:.3f}")
    assert bool(torch.isfinite(grad).all()) and bool((err <= bound).all()), worst


@pytest.mark.parametrize("layout,c", LAYOUTS)
def test_all_zero_mask_gives_exactly_zero_gradient_and_finite_values(layout, c):
    """With m = 0 every term of the gradient that carries the mask vanishes: L1 and SSIM (the trainer's defaults) give exactly 0.  The L2
    term does not carry it (2 g_l2 (pred - 0) / P, the reference's asymmetry), so with L2 on the gradient is that term alone."""
    case = _case(37, 45, layout, c, "zero")
    (l1, _, s), grad = _run(case, layout, weights=WEIGHTS, l1=True, l2=False, ssim=True)
    assert np.isfinite(float(l1)) and np.isfinite(float(s)) and bool((grad == 0).all())
    out, grad = _run(case, layout, weights=WEIGHTS, l1=True, l2=True, ssim=True)
    t2 = WEIGHTS[1] * case["l2_grad_unit"]
    assert all(np.isfinite(float(v)) for v in out) and bool(((grad - t2).abs() <= 4 * U * t2.abs()).all())


# ---- determinism, scratch, inference, layout ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,c", LAYOUTS)
def test_two_calls_are_bitwise_equal(layout, c):
    case = _case(37, 45, layout, c, "fractional")
    out1, g1 = _run(case, layout, weights=WEIGHTS, l1=True, l2=True, ssim=True)
    out2, g2 = _run(case, layout, weights=WEIGHTS, l1=True, l2=True, ssim=True)
    assert all(torch.equal(x, y) for x, y in zip(out1, out2)) and torch.equal(g1, g2)


@pytest.mark.parametrize("mask_kind", ["none", "binary"])
def test_nothing_relies_on_zeroed_scratch(mask_kind):
    """The C entry points with every caller buffer pre-filled with NaN (out, partials, planes, gradient) against the Python layer, as
    test_losses_gpu.py does for the SSIM pair: these kernels take all their scratch from the caller, none from the library's pool that
    GRUT_POISON_SCRATCH fills.  Also: a term that is not selected is written as 0, nothing is written past the stated partials count,
    and bad arguments come back as error codes."""
    abi = importlib.import_module("3dgrut_amd._abi")
    lib = abi.load_library()
    case = _case(37, 45, "nhwc", 3, mask_kind)
    (l1, _, s), g_ref = _run(case, "nhwc", weights=WEIGHTS, l1=True, l2=False, ssim=True)
    pred, gt, mask, _ = _device_inputs(case, "nhwc")
    x, y = pred.detach().permute(0, 3, 1, 2), gt.permute(0, 3, 1, 2)
    b, c, h, w = x.shape
    nan = dict(dtype=torch.float32, device="cuda")
    out = torch.full((3,), float("nan"), **nan)
    count = int(lib.grut_photo_loss_partials(b, c, h, w))
    partials = torch.full((count + 8,), float("nan"), **nan)
    planes = torch.full((3, b, c, h, w), float("nan"), **nan)
    grad = torch.full_like(x, float("nan"))
    assert grad.stride() == x.stride()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    st = lambda t: (C.c_int64 * t.dim())(*t.stride())   # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())              # noqa: E731
    m = None if mask is None else mask[..., 0]
    margs = (None, None) if m is None else (p(m), st(m))
    terms = 1 | 4
    abi.check(lib.grut_photo_loss_forward(stream, b, c, h, w, p(x), st(x), p(y), st(y), *margs, terms, 1, p(out), p(partials), p(planes[0]),
                                          p(planes[1]), p(planes[2])), "grut_photo_loss_forward")
    upstream = torch.tensor([WEIGHTS[0], float("nan"), WEIGHTS[2]], **nan)       # the entry of the term that is not selected is not read
    abi.check(lib.grut_photo_loss_backward(stream, b, c, h, w, p(x), st(x), p(y), st(y), *margs, terms, 1, p(upstream), p(planes[0]),
                                           p(planes[1]), p(planes[2]), p(grad), st(grad)), "grut_photo_loss_backward")
    torch.cuda.synchronize()
    assert torch.equal(out[0], l1) and torch.equal(out[2], s) and float(out[1]) == 0.0
    assert torch.equal(grad.permute(0, 2, 3, 1).cpu().double(), g_ref)
    assert bool(torch.isfinite(planes).all()) and bool(torch.isnan(partials[count:]).all())
    assert lib.grut_photo_loss_forward(stream, b, c, h, w, p(x), st(x), p(y), st(y), *margs, 0, 1, p(out), p(partials), None, None, None) != 0
    assert b"terms" in lib.grut_last_error()
    assert lib.grut_photo_loss_forward(stream, b, c, 10, w, p(x), st(x), p(y), st(y), *margs, 4, 1, p(out), p(partials), None, None, None) != 0
    assert lib.grut_photo_loss_forward(stream, b, c, h, w, p(x), st(x), p(y), st(y), *margs, 1, 1, p(out), p(partials), p(planes[0]),
                                       p(planes[1]), p(planes[2])) != 0        # planes without the SSIM term
    assert lib.grut_photo_loss_backward(stream, b, c, h, w, p(x), st(x), p(y), st(y), *margs, 4, 1, p(upstream), None, None, None, p(grad),
                                        st(grad)) != 0


def test_inference_allocates_no_plane_and_gives_the_training_values():
    losses = _losses()
    case = _case(37, 45, "nhwc", 3, "binary")
    trained, _ = _run(case, "nhwc", weights=WEIGHTS, l1=True, l2=True, ssim=True)
    pred, gt, mask, _ = _device_inputs(case, "nhwc")
    before = dict(losses.stats)
    with torch.no_grad():
        quiet = losses.photometric_loss(pred, gt, mask, l2=True)
    const = losses.photometric_loss(pred.detach(), gt, mask, l2=True)            # pred does not require grad
    assert losses.stats["photo_planes_allocated"] == before["photo_planes_allocated"]
    assert losses.stats["photo_forward_calls"] == before["photo_forward_calls"] + 2
    for got in (quiet, const):
        assert all(not v.requires_grad and torch.equal(v, t) for v, t in zip(got, trained))
    losses.photometric_loss(pred, gt, mask, ssim=False)[0].backward()           # training without the SSIM term needs no plane either
    assert losses.stats["photo_planes_allocated"] == before["photo_planes_allocated"]
    losses.photometric_loss(pred, gt, mask)[2].backward()
    assert losses.stats["photo_planes_allocated"] == before["photo_planes_allocated"] + 3


def test_gradient_lands_in_a_permuted_leafs_own_layout():
    """A planar [B, C, H, W] leaf handed over as its [B, H, W, C] view, and a channels-last leaf as its channels_first view: the gradient
    arrives in the leaf's memory order and equals the one the leaf's natural call gives."""
    losses = _losses()
    case = _case(37, 45, "nhwc", 3, "binary")
    _, g_ref = _run(case, "nhwc", weights=WEIGHTS, l1=True, l2=True, ssim=True)
    planar = case["pred"].permute(0, 3, 1, 2).contiguous().cuda().requires_grad_(True)
    out = losses.photometric_loss(planar.permute(0, 2, 3, 1), case["gt"].cuda(), case["mask"].cuda(), l2=True)
    sum(wt * v for wt, v in zip(WEIGHTS, out)).backward()
    assert planar.grad.shape == planar.shape and planar.grad.is_contiguous()
    assert torch.equal(planar.grad.permute(0, 2, 3, 1).cpu().double(), g_ref)
    last = case["pred"].cuda().requires_grad_(True)
    out = losses.photometric_loss(last.permute(0, 3, 1, 2), case["gt"].cuda().permute(0, 3, 1, 2), case["mask"].cuda()[..., 0], l2=True,
                                  channels_first=True)
    sum(wt * v for wt, v in zip(WEIGHTS, out)).backward()
    assert last.grad.is_contiguous() and torch.equal(last.grad.cpu().double(), g_ref)


# ---- end to end: the trainer hook ---------------------------------------------------------------------------------------------------------
class _Conf(dict):
    __getattr__ = dict.__getitem__


def _formula_trainer_module():
    """A stand-in for `threedgrut.trainer` (the reference is not present where the GPU tests run): a class whose get_losses evaluates the
    formula of trainer.py:687-747 in torch with this repository's fused SSIM, which is what the parent commit runs on every step."""
    losses = _losses()

    class Trainer3DGRUT:
        def __init__(self, conf, model, device):
            self.conf, self.model, self.device, self._in_color_refine = conf, model, device, False

        def get_losses(self, gpu_batch, outputs):
            cfg, zero = self.conf.loss, lambda: torch.zeros(1, device=self.device)   # noqa: E731
            gt, pred = gpu_batch.rgb_gt, outputs["pred_features"]
            if gpu_batch.mask is not None:
                gt, pred = gt * gpu_batch.mask, pred * gpu_batch.mask
            terms = {k: (zero(), 0.0) for k in ("l1", "l2", "ssim", "opacity", "scale")}
            if cfg.use_l1:
                terms["l1"] = ((pred - gt).abs().mean(), cfg.lambda_l1)
            if cfg.use_l2:
                terms["l2"] = (F.mse_loss(outputs["pred_features"], gt), cfg.lambda_l2)
            if cfg.use_ssim:
                terms["ssim"] = (1.0 - losses.ssim(pred.permute(0, 3, 1, 2), gt.permute(0, 3, 1, 2)), cfg.lambda_ssim)
            if cfg.use_opacity and not self._in_color_refine:
                terms["opacity"] = (self.model.get_density().abs().mean(), cfg.lambda_opacity)
            if cfg.use_scale and not self._in_color_refine:
                terms["scale"] = (self.model.get_scale().abs().mean(), cfg.lambda_scale)
            weighted = {k: lam * v for k, (v, lam) in terms.items()}
            total = weighted["l1"] + weighted["ssim"] + weighted["opacity"] + weighted["scale"]
            return dict(total_loss=total, **{f"{k}_loss": v for k, v in weighted.items()})

    mod = types.ModuleType("threedgrut.trainer")
    mod.Trainer3DGRUT = Trainer3DGRUT
    return mod


def test_patched_get_losses_gives_what_the_original_gives(monkeypatch):
    losses = _losses()
    mod = _formula_trainer_module()
    pkg = types.ModuleType("threedgrut")
    pkg.trainer, pkg.__path__ = mod, []
    monkeypatch.setitem(sys.modules, "threedgrut", pkg)
    monkeypatch.setitem(sys.modules, "threedgrut.trainer", mod)
    cls = mod.Trainer3DGRUT
    original = cls.get_losses
    patched = losses.install_fused_losses()
    assert cls.get_losses is patched and patched is not original and losses.install_fused_losses() is patched

    case = _case(37, 45, "nhwc", 3, "binary")
    conf = _Conf(loss=_Conf(use_l1=True, lambda_l1=0.8, use_l2=False, lambda_l2=1.0, use_ssim=True, lambda_ssim=0.2, use_opacity=True,
                            lambda_opacity=0.01, use_scale=True, lambda_scale=0.02))
    model = types.SimpleNamespace(density=torch.rand(50, 1, device="cuda").requires_grad_(True), scale=torch.rand(50, 3, device="cuda").requires_grad_(True))
    model.get_density, model.get_scale = (lambda: model.density), (lambda: model.scale)
    trainer = cls(conf, model, "cuda")
    batch = _Conf(rgb_gt=case["gt"].cuda(), mask=case["mask"].cuda())

    def step(method):
        pred = case["pred"].cuda().requires_grad_(True)
        model.density.grad = model.scale.grad = None
        outputs = {"pred_features": pred}
        calls = losses.stats["photo_forward_calls"]
        got = method(trainer, batch, outputs)
        got["total_loss"].backward()
        assert outputs["pred_features"] is pred
        return got, pred.grad.cpu().double(), model.density.grad.clone(), model.scale.grad.clone(), losses.stats["photo_forward_calls"] - calls

    want, g_want, gd_want, gs_want, n_want = step(original)
    got, g_got, gd_got, gs_got, n_got = step(patched)
    assert n_want == 0 and n_got == 1                                                    # one fused call, and the original makes none
    assert list(got) == list(want) == ["total_loss", "l1_loss", "l2_loss", "ssim_loss", "opacity_loss", "scale_loss"]
    assert got["l2_loss"].shape == want["l2_loss"].shape == (1,) and float(got["l2_loss"]) == 0.0
    assert torch.equal(got["opacity_loss"], want["opacity_loss"]) and torch.equal(got["scale_loss"], want["scale_loss"])
    assert torch.equal(gd_got, gd_want) and torch.equal(gs_got, gs_want)
    # both paths are fp32 evaluations held to the bounds above (torch's tree-shaped mean is shallower than DEPTH), so they differ by
    # at most twice the bound, plus the weighting's own roundings; and the fused one is inside the bound of the float64 reference
    l1_b, ssim_b = 0.8 * case["l1_bound"], 0.2 * case["ssim_bound"]
    few = 8 * U
    assert abs(float(got["l1_loss"]) - 0.8 * case["l1"]) <= l1_b + few * case["l1"]
    assert abs(float(got["ssim_loss"]) - 0.2 * (1.0 - case["ssim"])) <= ssim_b + few
    assert abs(float(got["l1_loss"]) - float(want["l1_loss"])) <= 2 * l1_b + few * case["l1"]
    assert abs(float(got["ssim_loss"]) - float(want["ssim_loss"])) <= 2 * ssim_b + few
    total = float(want["total_loss"])
    assert abs(float(got["total_loss"]) - total) <= 2 * (l1_b + ssim_b) + few * (abs(total) + 1.0)
    t1 = WEIGHTS[0] * case["l1_grad_unit"]
    expect = case["ssim_grad"] + t1                                                      # WEIGHTS[2] = -0.2 is the SSIM output's weight here too
    bound = case["ssim_grad_bound"] + 4 * U * t1.abs()
    assert bool(((g_got - expect).abs() <= bound).all())
    assert bool(((g_got - g_want).abs() <= 2 * bound + few * g_want.abs()).all())

    # a failed precondition goes to the original: five channels
    wide = _Conf(rgb_gt=torch.rand(1, 16, 16, 5, device="cuda"), mask=None)
    calls = losses.stats["photo_forward_calls"]
    out = patched(trainer, wide, {"pred_features": torch.rand(1, 16, 16, 5, device="cuda")})
    assert losses.stats["photo_forward_calls"] == calls and np.isfinite(float(out["total_loss"]))
    monkeypatch.setattr(cls, "get_losses", original)
