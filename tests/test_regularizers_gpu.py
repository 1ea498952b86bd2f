"""GPU: csrc/regularizers.hip against a float64 evaluation on the CPU of the reference's two lines (trainer.py:727, 735):

    opacity = mean |sigmoid(raw_density)|      scale = mean |exp(raw_scale)|

Sizes: a single particle, a float4 tail (3N % 4 != 0), a part of a wave, exactly 64 / 65 lanes' worth, more than one wave, more than one
block, and BIG, taken from the kernel's own constants: the first N at which the capped grid makes a block take a second grid-stride trip
with 3N % 4 != 0.  Inputs: raw density uniform in [-12, 12], raw scale uniform in [-15, 3]; -110 planted in both (sigmoid and exp
underflow to exactly 0) and +20 in the density (sigmoid rounds to 1, where s (1 - s) evaluated naively loses every digit).  With a single
particle the density holds one value, the +20: a lone -110 makes the exact mean 1.7e-48, below fp32's smallest denormal, which no fp32
result meets under a relative bound.

Forward bound (the issue's, unchanged): |a - b| <= (ceil(log2(3N)) + 4) u |b|, u = 2^-24.  That the kernel's own tree is inside it:
every term is non-negative, so a tree of depth D of correctly rounded additions is within D u of the exact sum of its terms, to first
order.  The tree (regularizers.hip): a float4 as (x + y) + (z + w), 2; the lane's grid-stride trips in a compensated sum, 2 however many
there are; the wave's DPP tree, 6; the block's four waves, 2; the finishing block's 1024 partials, 10.  The leaves that are not zero fill
a prefix of every level and adding zeros is exact, so D = min(ceil(log2(count)), 22) for count = N or 3N terms.  Besides D there is the
activation, evaluated in double and rounded to fp32 once, 1 u, and the division by a count that fp32 holds exactly, 1 u: D + 2, with
D <= ceil(log2(3N)) + 1 (the + 1 is BIG's scale sum, 3N just above 2^20).  With the device's expf in place of the double exponential
the kernel missed this bound at N = 1 (6.6 u against 6 u) and the gradient's: that expf is up to 11 ulp (22 u) from the exact value.
Backward bound (the issue's), per element: |a - b| <= 8 u |b| + 1e-37; the kernel computes an element in double and rounds it once."""
import ctypes as C
import functools
import importlib
import math
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
LAMBDAS = (0.01, 0.02)
BAD_INPUT = -1


def _reg():
    return importlib.import_module("3dgrut_amd.regularizers")


def _lib():
    return importlib.import_module("3dgrut_amd._abi").load_library()


def _big():
    """The first N whose [3N] array has more float4 than the capped grid has lanes (a block makes a second trip) with 3N % 4 != 0."""
    reg = _reg()
    n = (4 * reg.MAX_BLOCKS * reg.THREADS) // 3 + 1
    while not (-(-3 * n // 4) > reg.MAX_BLOCKS * reg.THREADS and (3 * n) % 4 != 0):
        n += 1
    return n


BIG = _big()
# (N, the density's planted values): see above for the single particle
CASES = [(1, "high"), (3, "both"), (63, "both"), (64, "both"), (65, "both"), (257, "both"), (4099, "both"), (BIG, "both")]
IDS = [f"{n}-{plant}" for n, plant in CASES]


@functools.lru_cache(maxsize=None)
def _case(n, plant):
    """Inputs (fp32, CPU) and the float64 reference: the two means, and the gradients of lambda_o * opacity + lambda_s * scale with the
    lambdas rounded to fp32 as the kernel receives them.  Computed once per case and not modified."""
    g = torch.Generator().manual_seed(1000 + n)
    density = torch.rand(n, 1, generator=g) * 24 - 12
    scale = torch.rand(n, 3, generator=g) * 18 - 15
    scale.view(-1)[(3 * n) // 2] = -110.0
    if plant in ("high", "both"):
        density[n - 1] = 20.0
    if plant in ("low", "both"):
        density[0] = -110.0
    grad_out = torch.tensor(LAMBDAS, dtype=torch.float32)
    d64, s64 = density.double().requires_grad_(True), scale.double().requires_grad_(True)
    mo, ms = _reg().means_torch(d64, s64)
    gd, gs = torch.autograd.grad(grad_out[0].double() * mo + grad_out[1].double() * ms, (d64, s64))
    assert float(torch.sigmoid(density.view(-1)[0])) == 0.0 or plant == "high"      # the planted values do what they are there for
    assert float(torch.exp(scale.view(-1)[(3 * n) // 2])) == 0.0
    return dict(n=n, density=density, scale=scale, grad_out=grad_out, opacity=float(mo.detach()), mean_scale=float(ms.detach()), g_density=gd,
                g_scale=gs)


def _forward_bound(n, exact):
    return (math.ceil(math.log2(3 * n)) + 4) * U * abs(exact)


def _assert_backward(got, want, what):
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, what
    excess = (got - want).abs() - (8 * U * want.abs() + 1e-37)
    assert bool((excess <= 0).all()), (what, float(excess.max()), int(excess.argmax()))


def _ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _forward(n, density, scale, fill=None):
    """grut_reg_forward on device tensors (either may be None) -> out [2] on the CPU; `fill` pre-fills the scratch."""
    lib = _lib()
    partials = torch.empty(int(lib.grut_reg_partials(n)), device="cuda")
    if fill is not None:
        partials.fill_(fill)
    out = torch.full((2,), float("nan"), device="cuda")
    assert lib.grut_reg_forward(_stream(), n, _ptr(density), _ptr(scale), _ptr(partials), _ptr(out)) == 0, lib.grut_last_error()
    return out.cpu()


def _backward(n, density, scale, grad_out, want_density=True, want_scale=True):
    """grut_reg_backward into NaN-filled buffers with a guard row behind each -> (grad_raw_density, grad_raw_scale), None if not wanted."""
    lib = _lib()
    gd = torch.full((n + 4, 1), float("nan"), device="cuda") if want_density else None
    gs = torch.full((n + 4, 3), float("nan"), device="cuda") if want_scale else None
    assert lib.grut_reg_backward(_stream(), n, _ptr(density), _ptr(scale), _ptr(grad_out), _ptr(gd), _ptr(gs)) == 0, lib.grut_last_error()
    for g in (gd, gs):
        if g is not None:
            assert bool(torch.isnan(g[n:]).all()) and not bool(torch.isnan(g[:n]).any())   # written completely, and nothing behind it
    return (None if gd is None else gd[:n]), (None if gs is None else gs[:n])


@pytest.mark.parametrize("n,plant", CASES, ids=IDS)
def test_forward_matches_float64_and_is_bitwise_reproducible(n, plant):
    case = _case(n, plant)
    d, s = case["density"].cuda(), case["scale"].cuda()
    out = _forward(n, d, s, fill=float("nan"))                                      # the scratch need not be zeroed
    err_o, err_s = abs(float(out[0]) - case["opacity"]), abs(float(out[1]) - case["mean_scale"])
    print(f"N={n}: opacity err {err_o / (U * case['opacity']):.2f} u, scale err {err_s / (U * case['mean_scale']):.2f} u, "
          f"bound {math.ceil(math.log2(3 * n)) + 4} u")
    assert err_o <= _forward_bound(n, case["opacity"]) and err_s <= _forward_bound(n, case["mean_scale"])
    again = _forward(n, d, s, fill=float("nan"))
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    # a NULL input: its slot is +0.0f and the other term is what the pair gave, bit for bit
    only_o, only_s = _forward(n, d, None, fill=float("nan")), _forward(n, None, s, fill=float("nan"))
    assert only_o.view(torch.int32)[0] == out.view(torch.int32)[0] and only_o.view(torch.int32)[1] == 0
    assert only_s.view(torch.int32)[1] == out.view(torch.int32)[1] and only_s.view(torch.int32)[0] == 0


@pytest.mark.parametrize("n,plant", CASES, ids=IDS)
def test_backward_matches_float64(n, plant):
    case = _case(n, plant)
    d, s, go = case["density"].cuda(), case["scale"].cuda(), case["grad_out"].cuda()
    gd, gs = _backward(n, d, s, go)
    _assert_backward(gd, case["g_density"], "density")
    _assert_backward(gs, case["g_scale"], "scale")
    if plant != "high":
        assert float(gd[0]) == 0.0                                                  # sigmoid underflowed: the reference's sign(0) = 0
    assert float(gs.view(-1)[(3 * n) // 2]) == 0.0
    if plant != "low":
        assert float(gd[n - 1]) > 0.0                                               # sigmoid rounded to 1: the derivative keeps its digits
    # a NULL gradient pointer: that term is not wanted, the other is the same bit for bit; its slot of grad_out is not read
    only_d, none = _backward(n, d, s, torch.tensor([LAMBDAS[0], float("nan")], device="cuda"), want_scale=False)
    assert none is None and torch.equal(only_d, gd)
    none, only_s = _backward(n, d, s, torch.tensor([float("nan"), LAMBDAS[1]], device="cuda"), want_density=False)
    assert none is None and torch.equal(only_s, gs)
    assert torch.equal(_backward(n, d, None, go, want_scale=False)[0], gd) and torch.equal(_backward(n, None, s, go, want_density=False)[1], gs)


def test_bad_input_is_refused_before_any_launch():
    """Every tensor is a real one of the stated size, so nothing here could fault even if a check were missing."""
    lib, reg = _lib(), _reg()
    n = 8
    d, s, go = torch.zeros(n + 4, 1, device="cuda"), torch.zeros(n + 4, 3, device="cuda"), torch.ones(2, device="cuda")
    gd, gs = torch.zeros_like(d), torch.zeros_like(s)
    partials, out = torch.zeros(64, device="cuda"), torch.zeros(2, device="cuda")
    off = lambda t: C.c_void_p(t.data_ptr() + 4)                                   # noqa: E731  (4 bytes in: not 16-byte aligned)
    null = C.c_void_p(None)

    def refused(status, text):
        assert status == BAD_INPUT and text in lib.grut_last_error().decode(), (status, lib.grut_last_error())

    st = _stream()
    refused(lib.grut_reg_forward(st, 0, _ptr(d), _ptr(s), _ptr(partials), _ptr(out)), "grut_reg_forward: num_particles is 0")
    refused(lib.grut_reg_forward(st, reg.MAX_PARTICLES + 1, _ptr(d), _ptr(s), _ptr(partials), _ptr(out)), "3 N must be below 2^32")
    refused(lib.grut_reg_forward(st, n, null, null, _ptr(partials), _ptr(out)), "raw_density and raw_scale are both NULL")
    refused(lib.grut_reg_forward(st, n, _ptr(d), _ptr(s), null, _ptr(out)), "partials is NULL")
    refused(lib.grut_reg_forward(st, n, _ptr(d), _ptr(s), _ptr(partials), null), "out is NULL")
    refused(lib.grut_reg_forward(st, n, off(d), _ptr(s), _ptr(partials), _ptr(out)), "raw_density must be 16-byte aligned")
    refused(lib.grut_reg_forward(st, n, _ptr(d), off(s), _ptr(partials), _ptr(out)), "raw_scale must be 16-byte aligned")
    refused(lib.grut_reg_backward(st, 0, _ptr(d), _ptr(s), _ptr(go), _ptr(gd), _ptr(gs)), "grut_reg_backward: num_particles is 0")
    refused(lib.grut_reg_backward(st, reg.MAX_PARTICLES + 1, _ptr(d), _ptr(s), _ptr(go), _ptr(gd), _ptr(gs)), "3 N must be below 2^32")
    refused(lib.grut_reg_backward(st, n, null, null, _ptr(go), null, null), "raw_density and raw_scale are both NULL")
    refused(lib.grut_reg_backward(st, n, _ptr(d), _ptr(s), null, _ptr(gd), _ptr(gs)), "grad_out is NULL")
    refused(lib.grut_reg_backward(st, n, null, _ptr(s), _ptr(go), _ptr(gd), _ptr(gs)), "grad_raw_density given but raw_density is NULL")
    refused(lib.grut_reg_backward(st, n, _ptr(d), null, _ptr(go), _ptr(gd), _ptr(gs)), "grad_raw_scale given but raw_scale is NULL")
    refused(lib.grut_reg_backward(st, n, _ptr(d), _ptr(s), _ptr(go), off(gd), _ptr(gs)), "grad_raw_density must be 16-byte aligned")
    refused(lib.grut_reg_backward(st, n, _ptr(d), _ptr(s), _ptr(go), _ptr(gd), off(gs)), "grad_raw_scale must be 16-byte aligned")
    refused(lib.grut_reg_backward(st, n, off(d), _ptr(s), _ptr(go), _ptr(gd), _ptr(gs)), "raw_density must be 16-byte aligned")
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and float(gd.abs().sum()) == 0.0 and float(gs.abs().sum()) == 0.0   # nothing ran


@pytest.mark.parametrize("n,plant", [(65, "both"), (4099, "both")], ids=["65", "4099"])
def test_autograd_matches_the_torch_lines_and_accumulates_into_an_existing_grad(n, plant):
    reg = _reg()
    case = _case(n, plant)
    d, s = case["density"].cuda().requires_grad_(True), case["scale"].cuda().requires_grad_(True)
    before = dict(reg.stats)
    mo, ms = reg.opacity_scale_means(d, s)
    assert mo.dim() == 0 and ms.dim() == 0 and mo.dtype == torch.float32
    assert abs(float(mo) - case["opacity"]) <= _forward_bound(n, case["opacity"])
    assert abs(float(ms) - case["mean_scale"]) <= _forward_bound(n, case["mean_scale"])
    (LAMBDAS[0] * mo + LAMBDAS[1] * ms).backward()
    _assert_backward(d.grad, case["g_density"], "density")
    _assert_backward(s.grad, case["g_scale"], "scale")
    assert {k: reg.stats[k] - before[k] for k in before} == {"hip_calls": 1, "torch_calls": 0, "hip_backward_calls": 1}
    # the torch lines on the same fp32 tensors are an evaluation of the same model within the same bounds
    d2, s2 = case["density"].cuda().requires_grad_(True), case["scale"].cuda().requires_grad_(True)
    to, ts = reg.means_torch(d2, s2)
    assert abs(float(mo) - float(to)) <= 2 * _forward_bound(n, case["opacity"])
    assert abs(float(ms) - float(ts)) <= 2 * _forward_bound(n, case["mean_scale"])
    # parameters that already hold a gradient (the renderer's) end with the sum: one fp32 addition on top of the kernel's values
    first_d, first_s = d.grad.clone(), s.grad.clone()
    g = torch.Generator().manual_seed(7)
    d.grad, s.grad = torch.randn(n, 1, generator=g).cuda(), torch.randn(n, 3, generator=g).cuda()
    held_d, held_s = d.grad.clone(), s.grad.clone()
    mo, ms = reg.opacity_scale_means(d, s)
    (LAMBDAS[0] * mo + LAMBDAS[1] * ms).backward()
    assert torch.equal(d.grad, held_d + first_d) and torch.equal(s.grad, held_s + first_s)
    # one argument None: its result is None, and only the other parameter gets a gradient
    d.grad = s.grad = None
    only, nothing = reg.opacity_scale_means(d, None)
    assert nothing is None
    (LAMBDAS[0] * only).backward()
    assert torch.equal(d.grad, first_d) and s.grad is None
    nothing, only = reg.opacity_scale_means(None, s)
    assert nothing is None
    (LAMBDAS[1] * only).backward()
    assert torch.equal(s.grad, first_s)


def _model(case, device="cuda"):
    m = types.SimpleNamespace(
        density=case["density"].to(device).requires_grad_(True), scale=case["scale"].to(device).requires_grad_(True),
        rotation=torch.rand(case["n"], 4, device=device),
        density_activation=torch.sigmoid, scale_activation=torch.exp, rotation_activation=torch.nn.functional.normalize)
    m.get_density, m.get_scale = (lambda: m.density_activation(m.density)), (lambda: m.scale_activation(m.scale))
    return m


def test_the_trainer_hook_takes_the_fused_call_only_when_switched_on(monkeypatch):
    from test_photo_loss_gpu import _Conf, _formula_trainer_module
    reg = _reg()
    losses = importlib.import_module("3dgrut_amd.losses")
    mod = _formula_trainer_module()
    pkg = types.ModuleType("threedgrut")
    pkg.trainer, pkg.__path__ = mod, []
    monkeypatch.setitem(sys.modules, "threedgrut", pkg)
    monkeypatch.setitem(sys.modules, "threedgrut.trainer", mod)
    cls = mod.Trainer3DGRUT
    patched = losses.install_fused_losses()
    previous = reg.install_fused_regularizers(False)
    n = 4099
    case = _case(n, "both")
    conf = _Conf(loss=_Conf(use_l1=True, lambda_l1=0.8, use_l2=False, lambda_l2=1.0, use_ssim=True, lambda_ssim=0.2, use_opacity=True,
                            lambda_opacity=LAMBDAS[0], use_scale=True, lambda_scale=LAMBDAS[1]))
    g = torch.Generator().manual_seed(11)
    batch = _Conf(rgb_gt=torch.rand(1, 16, 20, 3, generator=g).cuda(), mask=None)
    pred = torch.rand(1, 16, 20, 3, generator=g)

    def step(model, on, **loss):
        reg.install_fused_regularizers(on)
        trainer = cls(_Conf(loss=_Conf(conf.loss, **loss)), model, "cuda")
        before = dict(reg.stats)
        out = patched(trainer, batch, {"pred_features": pred.cuda().requires_grad_(True)})
        out["total_loss"].backward()
        return out, {k: reg.stats[k] - before[k] for k in before}

    try:
        m_off, m_on = _model(case), _model(case)
        want, delta = step(m_off, False)
        assert delta == {"hip_calls": 0, "torch_calls": 0, "hip_backward_calls": 0}
        got, delta = step(m_on, True)
        assert delta == {"hip_calls": 1, "torch_calls": 0, "hip_backward_calls": 1}                     # one of each per step
        assert list(got) == list(want) == ["total_loss", "l1_loss", "l2_loss", "ssim_loss", "opacity_loss", "scale_loss"]
        for key, exact, lam in (("opacity_loss", case["opacity"], LAMBDAS[0]), ("scale_loss", case["mean_scale"], LAMBDAS[1])):
            bound = lam * _forward_bound(n, exact)
            assert got[key].shape == want[key].shape == ()
            assert abs(float(got[key]) - lam * exact) <= bound + 2 * U * lam * exact                    # the weight's rounding and the product's
            assert abs(float(got[key]) - float(want[key])) <= 2 * bound + 2 * U * lam * exact
        for key in ("l1_loss", "l2_loss", "ssim_loss"):
            assert torch.equal(got[key], want[key])
        reg_bounds = sum(2 * lam * _forward_bound(n, exact) for exact, lam in zip((case["opacity"], case["mean_scale"]), LAMBDAS))
        assert abs(float(got["total_loss"]) - float(want["total_loss"])) <= reg_bounds + 8 * U * abs(float(want["total_loss"]))
        _assert_backward(m_on.density.grad, case["g_density"], "density")
        _assert_backward(m_on.scale.grad, case["g_scale"], "scale")
        # one term enabled: only that one is computed
        m = _model(case)
        got, delta = step(m, True, use_scale=False)
        assert delta == {"hip_calls": 1, "torch_calls": 0, "hip_backward_calls": 1}
        assert got["scale_loss"].shape == (1,) and float(got["scale_loss"]) == 0.0 and m.scale.grad is None
        _assert_backward(m.density.grad, case["g_density"], "density")
        # what the kernels do not take runs the two torch lines: a scale that is a view of a wider tensor, a model with another activation
        m = _model(case)
        wide = torch.cat([case["scale"], torch.zeros(n, 1)], dim=1).cuda().requires_grad_(True)
        m.scale = wide[:, :3]
        assert not m.scale.is_contiguous()
        got, delta = step(m, True)
        assert delta == {"hip_calls": 0, "torch_calls": 1, "hip_backward_calls": 0}
        assert torch.equal(got["opacity_loss"], want["opacity_loss"])
        assert abs(float(got["scale_loss"]) - float(want["scale_loss"])) <= 2 * LAMBDAS[1] * _forward_bound(n, case["mean_scale"])   # torch on a strided view
        m = _model(case)
        m.scale_activation = torch.nn.functional.softplus
        got, delta = step(m, True)
        assert delta == {"hip_calls": 0, "torch_calls": 1, "hip_backward_calls": 0}
        assert torch.equal(got["scale_loss"], LAMBDAS[1] * torch.nn.functional.softplus(m.scale).abs().mean())
    finally:
        reg.install_fused_regularizers(previous)
        monkeypatch.setattr(cls, "get_losses", patched._grut_original)
