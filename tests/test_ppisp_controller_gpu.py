"""GPU: csrc/ppisp_controller.hip against `_PPISPController` in float64 on the CPU (tests/ppisp_controller_reference.py), through the
C-ABI and through the `PPISP` module with install_fused_controller() on.

Shapes: 3x5 (1x1 downsampled: every cell is the same pixel), 9x13 (3x4: cells repeat), 15x15 (one pixel per cell), 31x37 (overlapping
cells, remainders 1 and 1), 121x212 (several rows of several workgroups), 97x1001 (remainders 1 and 2, rows of six units).

Forward bound:   max |out - out64| / max |out64| <= 4 max(e32, 2^-23),   e32 the same figure of CPU fp32 torch on the same case, computed
where the test runs; 4 = 2 for -ffp-contract=fast x 2 for the summation order (the reasoning of tests/test_ppisp_gpu.py).
Backward bound:  the same per tensor, with that tensor's own e32.  Every figure is printed with its bound.
Measured on the MI355X, the largest over the six shapes (e32 in brackets is the host's figure for the same tensor and shape):
  forward 7.1e-8 at 97x1001 (7.1e-8); conv1.w 3.1e-7 (4.1e-7), conv1.b 3.1e-7 (4.8e-7), conv2.w 3.7e-7 (3.9e-7), conv2.b 5.5e-7 (4.9e-6),
  conv3.w 2.5e-7 (2.3e-7), conv3.b 2.1e-7 (2.2e-7), trunk0.w 2.8e-7 (3.2e-7), trunk0.b 2.5e-7 (2.8e-7), trunk1.w 3.2e-7 (5.6e-7),
  trunk1.b 1.6e-7 (1.6e-7), trunk2.w 1.7e-7 (3.5e-7), trunk2.b 7.9e-8 (5.4e-8), exposure.w 1.1e-7 (1.7e-7), colour.w 1.1e-7 (1.7e-7), the two
  head biases exact; the conv biases at 97x1001, where the host's long sums cost it 9.9e-6 / 3.3e-5 / 4.1e-5: 1.2e-7 / 3.2e-7 / 1.8e-7.
  No tensor is above 0.6 of its bound.  Module level (31x37): on against off at most 6.4e-7, on against float64 at most 7.3e-7 of bounds
  from 7.6e-7 up.
Every image is conditioned first (the reference module's docstring): no gate of the model lies within 1e-5 of a rounding decision."""
import ctypes as C
import importlib

import pytest
import torch

import ppisp_controller_reference as R

pytestmark = pytest.mark.gpu
_cases = {}


def case_of(shape):
    """The conditioned case of a shape with its float64 results: computed once, shared, never modified."""
    if shape not in _cases:
        _cases[shape] = R.make_case(*shape)
    return _cases[shape]


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgrut_amd._abi").load_library()


@pytest.fixture()
def ppisp():
    mod = importlib.import_module("3dgrut_amd.ppisp")
    before = mod.install_fused_controller(False)
    yield mod
    mod.install_fused_controller(before)


def _ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def run_c_abi(lib, case, save=True, backward=True):
    """One forward (and one backward) call on NaN-filled buffers -> (out, saved, gradients), on the CPU."""
    abi = importlib.import_module("3dgrut_amd._abi")
    h, w = case["h"], case["w"]
    nan = float("nan")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hdr, prior, go = case["hdr"].cuda().contiguous(), case["prior"].cuda(), case["grad_out"].cuda()
    params = [p.detach().cuda().contiguous() for p in R.parameters(case["ctrl"])]
    weights = (C.c_void_p * 16)(*[p.data_ptr() for p in params])
    out = torch.full((9,), nan, device="cuda")
    saved = torch.full((abi.PPISP_CONTROLLER_SAVED,), nan, device="cuda") if save else None
    scratch = torch.full((lib.grut_ppisp_controller_forward_scratch(h, w),), nan, device="cuda")       # nothing has to be zeroed
    abi.check(lib.grut_ppisp_controller_forward(stream, h, w, _ptr(hdr), _ptr(prior), weights, _ptr(scratch), _ptr(saved), _ptr(out)),
              "grut_ppisp_controller_forward")
    grads = None
    if backward:
        grads = [torch.full_like(p, nan) for p in params]
        scratch_b = torch.full((lib.grut_ppisp_controller_backward_scratch(h, w),), nan, device="cuda")
        abi.check(lib.grut_ppisp_controller_backward(stream, h, w, _ptr(hdr), _ptr(prior), weights, _ptr(saved), _ptr(go), _ptr(scratch_b),
                                                     (C.c_void_p * 16)(*[g.data_ptr() for g in grads])), "grut_ppisp_controller_backward")
    torch.cuda.synchronize()
    return out.cpu(), None if saved is None else saved.cpu(), None if grads is None else [g.cpu() for g in grads]


def check_out(out, case, what):
    assert bool(torch.isfinite(out).all()), what
    err, bound = R.rel(out, case["out64"]), 4 * max(case["e32_out"], R.EPS32)
    print(f"{what} forward: {err:.2e} (e32 {case['e32_out']:.2e}, bound {bound:.2e})")
    assert err <= bound, (what, err, bound)


def check_grads(grads, case, what):
    failures = []
    for name, g, g64, e32 in zip(R.NAMES, grads, case["g64"], case["e32"]):
        assert g.shape == g64.shape and bool(torch.isfinite(g).all()), (what, name)
        err, bound = R.rel(g, g64), 4 * max(e32, R.EPS32)
        print(f"{what} {name}: {err:.2e} (e32 {e32:.2e}, bound {bound:.2e})")
        if err > bound:
            failures.append((name, err, bound))
    assert not failures, (what, failures)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_c_abi_matches_the_float64_module(lib, shape):
    case = case_of(shape)
    what = f"{shape[0]}x{shape[1]}"
    print(f"{what}: {case['redrawn']} windows redrawn in {case['rounds']} rounds")
    out, saved, grads = run_c_abi(lib, case)
    check_out(out, case, what)
    assert bool(torch.isfinite(saved).all())
    check_grads(grads, case, what)
    out2, saved2, grads2 = run_c_abi(lib, case)                                  # no atomics: bit for bit
    assert torch.equal(out, out2) and torch.equal(saved, saved2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    out3, none, _ = run_c_abi(lib, case, save=False, backward=False)             # saved = NULL changes no bit
    assert none is None and torch.equal(out, out3)


def test_prior_null_is_zero(lib):
    case = dict(case_of((9, 13)))
    case["prior"] = torch.zeros(1)
    with_zero, _, _ = run_c_abi(lib, case, backward=False)
    abi = importlib.import_module("3dgrut_amd._abi")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hdr = case["hdr"].cuda().contiguous()
    params = [p.detach().cuda().contiguous() for p in R.parameters(case["ctrl"])]
    out = torch.full((9,), float("nan"), device="cuda")
    scratch = torch.empty(lib.grut_ppisp_controller_forward_scratch(9, 13), device="cuda")
    abi.check(lib.grut_ppisp_controller_forward(stream, 9, 13, _ptr(hdr), _ptr(None), (C.c_void_p * 16)(*[p.data_ptr() for p in params]),
                                                _ptr(scratch), _ptr(None), _ptr(out)), "grut_ppisp_controller_forward")
    assert torch.equal(out.cpu(), with_zero)


def _module_with(ppisp, case, device):
    """Two cameras, three frames; camera 1's controller carries the case's weights, camera 0's its own random heads."""
    with torch.random.fork_rng():
        torch.manual_seed(11)
        module = ppisp.PPISP(num_cameras=2, num_frames=3, config=ppisp.PPISPConfig(controller_distillation=True, controller_activation_ratio=0.5))
        module.controllers[1].load_state_dict(case["ctrl"].state_dict())
        with torch.no_grad():
            module.controllers[0].color_head.weight.normal_(0.0, 0.1)
            module.vignetting_params.normal_(0.0, 0.02)
    return module.to(device)


def _pixel_coords(h, w):
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    return (torch.stack((x, y), -1) + 0.5).reshape(-1, 2)


def _novel_view(module, case):
    h, w = case["h"], case["w"]
    p = next(module.parameters())
    module.eval()
    with torch.no_grad():
        return module(case["hdr"].to(p).reshape(-1, 3), _pixel_coords(h, w).to(p), resolution=(w, h), camera_idx=1, frame_idx=-1,
                      exposure_prior=case["prior"].to(p)).detach().cpu()


def _active_step(module, case, weight):
    """One training step of the controller's phase with controller_distillation -> camera 1's sixteen gradients."""
    h, w = case["h"], case["w"]
    p = next(module.parameters())
    module.train()
    module.create_schedulers(module.create_optimizers(), max_optimization_iters=2)   # active from step 1 on
    module.step.fill_(1)
    module._step_host = 1
    assert module.controller_active
    module.zero_grad(set_to_none=True)
    out = module(case["hdr"].to(p).reshape(-1, 3), _pixel_coords(h, w).to(p), resolution=(w, h), camera_idx=1, frame_idx=0)
    (out * weight.to(p)).sum().backward()
    assert all(q.grad is None for q in module.controllers[0].parameters())        # the other camera's controller gets no gradient
    assert module.exposure_params.grad is None and module.vignetting_params.grad is None   # distillation: only the controller learns
    return [q.grad.detach().cpu() for q in R.parameters(module.controllers[1])]


def test_module_with_the_switch_on_matches_the_switch_off(ppisp):
    case = case_of((31, 37))
    weight = torch.randn(case["h"] * case["w"], 3, generator=torch.Generator().manual_seed(8))
    cpu32, cpu64 = _module_with(ppisp, case, "cpu"), _module_with(ppisp, case, "cpu").double()
    view64, step64 = _novel_view(cpu64, case), _active_step(cpu64, case, weight)
    e32_view = R.rel(_novel_view(cpu32, case), view64)
    e32_step = [R.rel(a, b) for a, b in zip(_active_step(cpu32, case, weight), step64)]

    module = _module_with(ppisp, case, "cuda")
    before = dict(ppisp.stats)
    view_off, step_off = _novel_view(module, case), _active_step(module, case, weight)
    assert ppisp.stats["controller_torch_calls"] == before["controller_torch_calls"] + 2
    assert ppisp.stats["controller_hip_calls"] == before["controller_hip_calls"]

    assert ppisp.install_fused_controller() is False
    before = dict(ppisp.stats)
    view_on = _novel_view(module, case)
    assert ppisp.stats["controller_hip_calls"] == before["controller_hip_calls"] + 1
    assert ppisp.stats["controller_hip_backward_calls"] == before["controller_hip_backward_calls"]   # eval, no_grad: nothing saved, no backward
    step_on = _active_step(module, case, weight)
    assert ppisp.stats["controller_hip_calls"] == before["controller_hip_calls"] + 2
    assert ppisp.stats["controller_hip_backward_calls"] == before["controller_hip_backward_calls"] + 1
    assert ppisp.stats["controller_torch_calls"] == before["controller_torch_calls"]

    failures = []
    for name, on, off, ref, e32 in [("novel view", view_on, view_off, view64, e32_view)] + \
            [(n, a, b, c, e) for n, a, b, c, e in zip(R.NAMES, step_on, step_off, step64, e32_step)]:
        assert bool(torch.isfinite(on).all()), name
        err, err64, bound = R.rel(on, off.double()), R.rel(on, ref), 4 * max(e32, R.EPS32)
        print(f"module {name}: on vs off {err:.2e}, on vs float64 {err64:.2e} (e32 {e32:.2e}, bound {bound:.2e})")
        if err > bound or err64 > bound:
            failures.append((name, err, err64, bound))
    assert not failures, failures


def test_other_inputs_run_the_torch_code(ppisp):
    ppisp.install_fused_controller()
    ctrl = R.make_controller(6).cuda()
    g = torch.Generator().manual_seed(6)
    image, prior = torch.rand(12, 17, 3, generator=g), torch.tensor([0.1])

    def counts(hdr, prior, module=ctrl):
        before = dict(ppisp.stats)
        e, c = module(hdr, prior)
        assert e.shape == () and c.shape == (8,)
        return tuple(ppisp.stats[k] - before[k] for k in ("controller_hip_calls", "controller_torch_calls"))

    assert counts(image.cuda(), prior.cuda()) == (1, 0)
    assert counts(image.cuda().permute(1, 0, 2).contiguous().permute(1, 0, 2), prior.cuda()) == (1, 0)   # made contiguous
    assert counts(image, prior, R.make_controller(6)) == (0, 1)                                          # CPU tensors
    before = dict(ppisp.stats)                                       # 2x7 has no downsampled row: torch's own refusal, not the library's
    with pytest.raises(RuntimeError, match="Output size is too small"):
        ctrl(torch.rand(2, 7, 3).cuda(), prior.cuda())
    assert (ppisp.stats["controller_hip_calls"], ppisp.stats["controller_torch_calls"]) == \
        (before["controller_hip_calls"], before["controller_torch_calls"] + 1)
    assert counts(image.cuda().requires_grad_(True), prior.cuda()) == (0, 1)                              # hdr wants a gradient
    assert counts(image.cuda().double(), prior.cuda().double(), R.make_controller(6).cuda().double()) == (0, 1)   # float64
