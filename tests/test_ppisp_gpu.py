"""GPU: csrc/ppisp.hip against the float64 restatement of the model (tests/ppisp_reference.py), through the C-ABI and through
`ppisp_apply` / the `PPISP` module, on the golden cases of tests/golden/ppisp.npz (four shapes x two parameter draws + the identity).

Forward bound, per case:   |hip - restatement64| <= 4 e_ref,   e_ref = max |reference fp32 - restatement64| as stored in the golden file
(1.9e-7 .. 5.0e-7 over the twelve cases).  4: the device's pow / exp / log are good to about 2 ulp where the host's are about 1, and
-ffp-contract=fast moves roundings; each is worth a factor of 2.  Measured on the MI355X: at most 5.5e-7.

Backward bound, per kind of quantity (grad_rgb, exposure, colour, vignetting, curve):   max |g - g64| / max |g64| <= 4 e32,   where e32 is
the largest such figure, over all cases of the file, of CPU fp32 autograd of the restatement itself, computed where the tests run.
e32 on the build machine: grad_rgb 6.0e-7, exposure 5.8e-7, colour 3.8e-6, vignetting 3.8e-7, curve 7.7e-7 (the sums over pixels move
with the host's reduction order: exposure 7.5e-7, colour 5.4e-6 on the GPU machine's host).  Measured for the kernels on the MI355X:
grad_rgb 1.7e-6, exposure 1.4e-6, colour 2.0e-6, vignetting 4.3e-7, curve 7.2e-7.
Gradient comparisons leave out the pixels of ppisp_reference.kink_free (a curve input within 1e-3 of 0, 1 or the centre; an exact 0
stays; at most 5 % of a case, asserted: 3.2 % at 7x9, below 2 % elsewhere) by zeroing their upstream gradient.
"""
import ctypes as C
import importlib
import os

import pytest
import torch

import ppisp_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("rgb",) + R.GROUPS
CONFIGS = R.CONFIGS   # all four groups; each NULL in turn; all NULL


def _upstream(case):
    return torch.randn(case["h"], case["w"], 3, generator=torch.Generator().manual_seed(5))


@pytest.fixture(scope="module")
def golden():
    """The cases, each with its pixel mask, masked upstream gradient and float64 output / gradients with all four groups, and e32."""
    cases = R.load_golden(os.path.join(ROOT, "tests", "golden", "ppisp.npz"))
    e32 = dict.fromkeys(KINDS, 0.0)
    for c in cases:
        c["keep"] = R.kink_free(c)
        assert 1 - float(c["keep"].float().mean()) <= R.MAX_LEFT_OUT, c["name"]
        c["go"] = _upstream(c) * c["keep"][..., None]
        c["out64"], c["g64"] = R.gradients(c, c["go"], c["keep"])
        _, g32 = R.gradients(c, c["go"], c["keep"], dtype=torch.float32)
        for k in KINDS:
            e32[k] = max(e32[k], float((g32[k].double() - c["g64"][k]).abs().max() / c["g64"][k].abs().max()))
    print("e_ref", {c["name"]: f"{c['e_ref']:.2e}" for c in cases})
    print("e32", {k: f"{v:.2e}" for k, v in e32.items()})
    return cases, e32


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgrut_amd._abi").load_library()


def _ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def _run(lib, case, groups, rgb=None, want_rgb=True, go=None):
    """One forward and one backward call through the C-ABI with the groups in `groups` present -> (out, dict of gradients), on the CPU."""
    abi = importlib.import_module("3dgrut_amd._abi")
    h, w = case["h"], case["w"]
    n = h * w
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rgb = case["rgb"].cuda().reshape(n, 3) if rgb is None else rgb
    pc = case["pc"].cuda().reshape(n, 2)
    par = {k: (case[k].cuda().contiguous() if k in groups else None) for k in R.GROUPS}
    out = torch.full((n, 3), float("nan"), device="cuda")
    abi.check(lib.grut_ppisp_forward(stream, n, _ptr(rgb), _ptr(pc), float(w), float(h), *(_ptr(par[k]) for k in R.GROUPS), _ptr(out)),
              "grut_ppisp_forward")
    go = (case["go"] if go is None else go).cuda().reshape(n, 3).contiguous()
    grads = {k: (torch.full_like(par[k], float("nan")) if k in groups else None) for k in R.GROUPS}
    grads["rgb"] = torch.full((n, 3), float("nan"), device="cuda") if want_rgb else None
    partials = torch.full((lib.grut_ppisp_partials(n),), float("nan"), device="cuda")       # nothing has to be zeroed
    abi.check(lib.grut_ppisp_backward(stream, n, _ptr(rgb), _ptr(pc), float(w), float(h), *(_ptr(par[k]) for k in R.GROUPS), _ptr(go),
                                      _ptr(grads["rgb"]), *(_ptr(grads[k]) for k in R.GROUPS), _ptr(partials)), "grut_ppisp_backward")
    torch.cuda.synchronize()
    return out.cpu().reshape(h, w, 3), {k: (None if v is None else v.cpu().reshape(case["rgb"].shape if k == "rgb" else v.shape)) for k, v in grads.items()}


def _check_gradients(got, g64, e32, what):
    for k, v in got.items():
        if v is None:
            continue
        assert bool(torch.isfinite(v).all()), (what, k)
        err = float((v.double() - g64[k]).abs().max() / g64[k].abs().max())
        print(f"{what} {k}: {err:.2e} (bound {4 * e32[k]:.2e})")
        assert err <= 4 * e32[k], (what, k, err, 4 * e32[k])


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_c_abi_matches_the_restatement(lib, golden, shape):
    cases, e32 = golden
    for c in (c for c in cases if (c["h"], c["w"]) == shape):
        for groups in CONFIGS:
            what = f"{c['name']} {'+'.join(groups) or 'none'}"
            if groups == R.GROUPS:
                out64, g64, keep = c["out64"], c["g64"], c["keep"]
                go = c["go"]
            else:                                   # another model: its own kinks, its own float64 gradients
                keep = R.kink_free(c, groups)
                assert 1 - float(keep.float().mean()) <= R.MAX_LEFT_OUT, what
                go = _upstream(c) * keep[..., None]
                out64, g64 = R.gradients(c, go, keep, groups)
            out, grads = _run(lib, c, groups, go=go)
            if not groups:                          # every stage off: a copy, and the gradient passes through
                assert torch.equal(out, c["rgb"]) and torch.equal(grads["rgb"], go)
                continue
            err = float((out.double() - out64).abs().max())
            print(f"{what} forward: {err:.2e} (bound {4 * c['e_ref']:.2e})")
            assert err <= 4 * c["e_ref"], (what, err)
            _check_gradients(grads, g64, e32, what)


def test_grad_rgb_null_and_bitwise_repeatability(lib, golden):
    cases, e32 = golden
    c = next(c for c in cases if c["name"] == "37x45_s23")
    _, full = _run(lib, c, R.GROUPS)
    _, again = _run(lib, c, R.GROUPS)
    _, without = _run(lib, c, R.GROUPS, want_rgb=False)
    assert without["rgb"] is None
    for k in KINDS:
        assert torch.equal(full[k], again[k]), k                                 # no atomics: bit for bit
        if k != "rgb":
            assert torch.equal(full[k], without[k]), k
    _check_gradients(without, c["g64"], e32, "grad_rgb NULL")


def test_unaligned_views_take_the_scalar_path(lib, golden):
    """A [P,3] view that starts 12 bytes into an allocation is not 16-byte aligned: same numbers from the kernels without float4 access."""
    cases, _ = golden
    c = next(c for c in cases if c["name"] == "64x33_s41")
    n = c["h"] * c["w"]
    out, grads = _run(lib, c, R.GROUPS)
    shifted = torch.empty((n + 1, 3), device="cuda")
    shifted[1:] = c["rgb"].cuda().reshape(n, 3)
    assert shifted[1:].data_ptr() % 16 != 0
    out_u, grads_u = _run(lib, c, R.GROUPS, rgb=shifted[1:])
    assert torch.equal(out, out_u)
    assert all(torch.equal(grads[k], grads_u[k]) for k in KINDS)


def test_bad_arguments_are_refused_before_any_launch(lib):
    rgb, out = torch.rand(8, 3, device="cuda"), torch.empty(8, 3, device="cuda")
    vig = torch.zeros(3, 5, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    none = C.c_void_p(None)
    assert lib.grut_ppisp_forward(stream, 8, _ptr(rgb), none, 4.0, 2.0, none, none, _ptr(vig), none, _ptr(out)) == -1        # no pixel_coords
    assert lib.grut_ppisp_forward(stream, 0, _ptr(rgb), none, 4.0, 2.0, none, none, none, none, _ptr(out)) == -1
    partials = torch.empty(lib.grut_ppisp_partials(8), device="cuda")
    g = torch.empty(1, device="cuda")
    assert lib.grut_ppisp_backward(stream, 8, _ptr(rgb), none, 4.0, 2.0, none, none, none, none, _ptr(out), none, _ptr(g), none, none, none,
                                   _ptr(partials)) == -1                                                                 # a gradient without its stage
    assert b"NULL" in lib.grut_last_error()


def test_a_second_trip_of_the_grid_matches_two_single_trips(lib):
    """More than 1024 blocks' worth of pixels: the grid strides.  Per pixel nothing may change against two calls that do not stride, and
    the parameter gradients are the two calls' sums up to fp32 rounding of sums of 1e6 terms of mixed sign."""
    ppisp = importlib.import_module("3dgrut_amd.ppisp")
    n = 1024 * 1024 + 4099
    g = torch.Generator(device="cuda").manual_seed(3)
    rgb = (torch.rand(n, 3, generator=g, device="cuda") * 1.4 - 0.1).clamp_min(0)
    pc = torch.rand(n, 2, generator=g, device="cuda") * 1000
    go = torch.randn(n, 3, generator=g, device="cuda")
    par = {k: v.cuda() for k, v in R.random_parameters(9).items()}

    def run(sl):
        leaves = {k: v.clone()[None].requires_grad_(True) for k, v in par.items()}
        x = rgb[sl].clone().requires_grad_(True)
        out = ppisp.ppisp_apply(exposure_params=leaves["exposure"].reshape(1), vignetting_params=leaves["vignetting"], color_params=leaves["color"],
                                crf_params=leaves["crf"], rgb_in=x, pixel_coords=pc[sl], resolution_w=1000, resolution_h=1000, camera_idx=0,
                                frame_idx=0)
        out.backward(go[sl])
        return out.detach(), x.grad, {k: v.grad for k, v in leaves.items()}

    half = 1024 * 512
    out, gx, gp = run(slice(0, n))
    out_a, gx_a, gp_a = run(slice(0, half))
    out_b, gx_b, gp_b = run(slice(half, n))
    assert torch.equal(out, torch.cat([out_a, out_b])) and torch.equal(gx, torch.cat([gx_a, gx_b]))
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gx).all())
    for k in R.GROUPS:
        both = gp_a[k] + gp_b[k]
        assert float((gp[k] - both).abs().max()) <= 1e-4 * float(both.abs().max()), k


def test_ppisp_apply_selects_rows_and_accepts_any_leading_shape(golden):
    ppisp = importlib.import_module("3dgrut_amd.ppisp")
    cases, e32 = golden
    c = next(c for c in cases if c["name"] == "37x45_s41")
    full = dict(exposure=torch.randn(4), color=torch.randn(4, 8) * 0.3, vignetting=torch.randn(3, 3, 5) * 0.05, crf=torch.randn(3, 3, 4))
    frame, camera = 2, 1
    full["exposure"][frame], full["color"][frame], full["vignetting"][camera], full["crf"][camera] = c["exposure"][0], c["color"], c["vignetting"], c["crf"]
    results = []
    for flat, contiguous in ((False, True), (True, True), (False, False)):
        leaves = {k: v.cuda().requires_grad_(True) for k, v in full.items()}
        rgb = c["rgb"].cuda()
        if not contiguous:
            rgb = c["rgb"].cuda().permute(1, 0, 2).contiguous().permute(1, 0, 2)           # same values, strides of the transposed image
            assert not rgb.is_contiguous()
        rgb = (rgb.reshape(-1, 3) if flat else rgb).detach().requires_grad_(True)
        pc = c["pc"].cuda().reshape(-1, 2) if flat else c["pc"].cuda()
        before = dict(ppisp.stats)
        out = ppisp.ppisp_apply(exposure_params=leaves["exposure"], vignetting_params=leaves["vignetting"], color_params=leaves["color"],
                                crf_params=leaves["crf"], rgb_in=rgb, pixel_coords=pc, resolution_w=c["w"], resolution_h=c["h"], camera_idx=camera,
                                frame_idx=frame)
        assert out.shape == rgb.shape and out.is_cuda
        (out.reshape(c["h"], c["w"], 3) * c["go"].cuda()).sum().backward()
        assert ppisp.stats["forward_calls"] == before["forward_calls"] + 1 and ppisp.stats["backward_calls"] == before["backward_calls"] + 1
        assert ppisp.stats["torch_calls"] == before["torch_calls"]                         # the kernels ran, not the torch path
        assert float((out.detach().cpu().reshape(c["h"], c["w"], 3).double() - c["out64"]).abs().max()) <= 4 * c["e_ref"]
        rows = {"rgb": rgb.grad.cpu().reshape(c["h"], c["w"], 3), "exposure": leaves["exposure"].grad[frame:frame + 1].cpu(),
                "color": leaves["color"].grad[frame].cpu(), "vignetting": leaves["vignetting"].grad[camera].cpu(), "crf": leaves["crf"].grad[camera].cpu()}
        _check_gradients(rows, c["g64"], e32, f"ppisp_apply flat={flat} contiguous={contiguous}")
        for k, idx in (("exposure", frame), ("color", frame), ("vignetting", camera), ("crf", camera)):
            grad = leaves[k].grad.clone()
            assert grad.shape == full[k].shape
            grad[idx] = 0
            assert float(grad.abs().max()) == 0.0, k                                       # zero outside the selected row
        results.append((out.detach().reshape(-1), rgb.grad.reshape(-1)))
    assert all(torch.equal(results[0][0], r[0]) and torch.equal(results[0][1], r[1]) for r in results[1:])
    cpu = ppisp.ppisp_apply(exposure_params=full["exposure"], vignetting_params=full["vignetting"], color_params=full["color"],
                            crf_params=full["crf"], rgb_in=c["rgb"], pixel_coords=c["pc"], resolution_w=c["w"], resolution_h=c["h"],
                            camera_idx=camera, frame_idx=frame)                             # CPU tensors keep working
    assert not cpu.is_cuda and float((cpu.double() - c["out64"]).abs().max()) <= 4 * c["e_ref"]


def test_the_module_on_the_gpu_matches_the_restatement(golden):
    ppisp = importlib.import_module("3dgrut_amd.ppisp")
    cases, e32 = golden
    c = next(c for c in cases if c["name"] == "64x33_s23")
    module = ppisp.PPISP(num_cameras=2, num_frames=3, config=ppisp.PPISPConfig(use_controller=False)).cuda().train()
    frame, camera = 1, 1
    with torch.no_grad():
        module.exposure_params[frame], module.color_params[frame] = c["exposure"][0].cuda(), c["color"].cuda()
        module.vignetting_params[camera], module.crf_params[camera] = c["vignetting"].cuda(), c["crf"].cuda()
    rgb = c["rgb"].cuda().reshape(-1, 3).requires_grad_(True)
    out = module(rgb, c["pc"].cuda().reshape(-1, 2), resolution=(c["w"], c["h"]), camera_idx=camera, frame_idx=frame)
    loss = (out.reshape(c["h"], c["w"], 3) * c["go"].cuda()).sum()
    loss.backward()
    rows = {"rgb": rgb.grad.cpu().reshape(c["h"], c["w"], 3), "exposure": module.exposure_params.grad[frame:frame + 1].cpu(),
            "color": module.color_params.grad[frame].cpu(), "vignetting": module.vignetting_params.grad[camera].cpu(),
            "crf": module.crf_params.grad[camera].cpu()}
    _check_gradients(rows, c["g64"], e32, "module")
    assert float(module.exposure_params.grad[[0, 2]].abs().max()) == 0 and float(module.color_params.grad[[0, 2]].abs().max()) == 0
    assert float(module.vignetting_params.grad[0].abs().max()) == 0 and float(module.crf_params.grad[0].abs().max()) == 0
    assert module.steps_done == 1 and module.get_regularization_loss().is_cuda


def test_black_and_saturated_pixels_give_finite_gradients(lib):
    ppisp = importlib.import_module("3dgrut_amd.ppisp")
    par = {k: v.cuda()[None].requires_grad_(True) for k, v in R.random_parameters(11).items()}
    rgb = torch.tensor([[0.0, 0.0, 0.0], [5.0, 6.0, 7.0], [0.3, 0.4, 0.2], [0.0, 0.0, 0.0], [9.0, 9.0, 9.0]], device="cuda", requires_grad=True)
    pc = torch.tensor([[0.5, 0.5], [3.5, 1.5], [2.5, 2.5], [1.5, 0.5], [0.5, 2.5]], device="cuda")
    out = ppisp.ppisp_apply(exposure_params=par["exposure"].reshape(1), vignetting_params=par["vignetting"], color_params=par["color"],
                            crf_params=par["crf"], rgb_in=rgb, pixel_coords=pc, resolution_w=4, resolution_h=3, camera_idx=0, frame_idx=0)
    assert torch.equal(out[0].detach().cpu(), torch.zeros(3)) and torch.equal(out[1].detach().cpu(), torch.ones(3))
    weights = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]], device="cuda")
    (out * weights).sum().backward()
    for t in (rgb, *par.values()):                                  # only black and saturated pixels carry an upstream gradient:
        assert bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) == 0.0      # nothing passes the curve at or beyond its ends
    out = ppisp.ppisp_apply(exposure_params=par["exposure"].reshape(1), vignetting_params=par["vignetting"], color_params=par["color"],
                            crf_params=par["crf"], rgb_in=rgb, pixel_coords=pc, resolution_w=4, resolution_h=3, camera_idx=0, frame_idx=0)
    out.sum().backward()
    for t in (rgb, *par.values()):
        assert bool(torch.isfinite(t.grad).all())
    assert float(rgb.grad[2].abs().min()) > 0

    module = ppisp.PPISP(1, 1, ppisp.PPISPConfig(use_controller=False)).cuda()            # every alpha is 0: p == 1 exactly
    module(R.make_image(7, 9, 3).cuda().reshape(-1, 3), R.pixel_coords(7, 9).cuda().reshape(-1, 2), resolution=(9, 7), camera_idx=0,
           frame_idx=0).sum().backward()
    assert float(module.vignetting_params.grad[0, :, 2:].abs().min()) > 0                  # inclusive: the alphas can learn from the start
