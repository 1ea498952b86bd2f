"""CPU: the fused PPISP controller's surface without a GPU - the entry points are declared, mirrored and exported; the scratch sizes are
host arithmetic; every bad argument is refused before any HIP call; the switch of 3dgrut_amd.ppisp changes nothing for CPU tensors;
and the conditioning of the GPU tests' images (tests/ppisp_controller_reference.py) does what it says."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

import ppisp_controller_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = ("grut_ppisp_controller_forward", "grut_ppisp_controller_backward")
SIZES = ("grut_ppisp_controller_forward_scratch", "grut_ppisp_controller_backward_scratch")


@pytest.fixture()
def ppisp():
    mod = importlib.import_module("3dgrut_amd.ppisp")
    before = mod.install_fused_controller(False)
    yield mod
    mod.install_fused_controller(before)


def test_controller_symbols_are_declared_mirrored_and_exported(grut_lib):
    abi = importlib.import_module("3dgrut_amd._abi")
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    for name in LAUNCHES + SIZES:
        assert re.search(rf"\b(int|uint64_t) {name}\(", header), name
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(grut_lib, name) and getattr(grut_lib, name).argtypes, name
    assert abi.ABI_VERSION == 5 and grut_lib.grut_abi_version() == 5           # additive change
    assert re.search(r"#define GRUT_PPISP_CONTROLLER_SAVED 1984\b", header) and abi.PPISP_CONTROLLER_SAVED == 1984
    assert 1984 == 64 * 25 + 3 * 128
    assert len(grut_lib.grut_ppisp_controller_forward.argtypes) == 9 and len(grut_lib.grut_ppisp_controller_backward.argtypes) == 10


def test_scratch_sizes_are_nonzero_and_monotone(grut_lib):
    for fn in (grut_lib.grut_ppisp_controller_forward_scratch, grut_lib.grut_ppisp_controller_backward_scratch):
        for h, w in R.SHAPES + ((1080, 1920), (800, 800), (16384, 16384)):
            assert fn(h, w) > 0, (h, w)
        sizes = [3, 4, 5, 6, 9, 15, 16, 31, 97, 191, 192, 193, 195, 196, 400, 1001, 1080, 1920, 4000, 16384]
        for fixed in (3, 31, 1080):
            along_w = [fn(fixed, s) for s in sizes]
            along_h = [fn(s, fixed) for s in sizes]
            assert along_w == sorted(along_w) and along_h == sorted(along_h), fixed
        assert [fn(h, w) for h, w in ((2, 9), (9, 2), (0, 0), (-1, 9), (16385, 9), (9, 16385))] == [0] * 6
        assert fn(1080, 1920) * 4 < 16 << 20                                    # a few MiB at 1080p


def _arrays(n=16, null=None):
    a = (C.c_void_p * n)(*[0x1000 + 64 * i for i in range(n)])                 # never dereferenced: the refusal comes first
    if null is not None:
        a[null] = None
    return a


def test_bad_arguments_are_refused_without_a_gpu(grut_lib):
    lib = grut_lib
    p = C.c_void_p(0x1000)
    none = C.c_void_p(None)

    def fwd(h=9, w=9, hdr=p, weights=None, scratch=p, out=p):
        return lib.grut_ppisp_controller_forward(none, h, w, hdr, none, _arrays() if weights is None else weights, scratch, none, out)

    def bwd(h=9, w=9, hdr=p, weights=None, saved=p, grad_out=p, scratch=p, grads=None):
        return lib.grut_ppisp_controller_backward(none, h, w, hdr, none, _arrays() if weights is None else weights, saved, grad_out, scratch,
                                                  _arrays() if grads is None else grads)

    def refused(code, *words):
        assert code == -1
        message = lib.grut_last_error().decode()
        assert all(word in message for word in words), message

    for call, fn in ((fwd, "grut_ppisp_controller_forward"), (bwd, "grut_ppisp_controller_backward")):
        refused(call(h=2), fn, "at least 3")
        refused(call(w=2), fn, "at least 3")
        refused(call(h=16385), fn, "at most 16384")
        refused(call(w=16385), fn, "at most 16384")
        refused(call(hdr=none), fn, "hdr")
        refused(call(scratch=none), fn, "scratch")
        for i in (0, 7, 15):
            refused(call(weights=_arrays(null=i)), fn, f"weights[{i}]")
    refused(fwd(out=none), "forward", "out")
    refused(bwd(saved=none), "backward", "saved")
    refused(bwd(grad_out=none), "backward", "grad_out")
    for i in (0, 6, 15):
        refused(bwd(grads=_arrays(null=i)), "backward", f"grads[{i}]")


def test_the_switch_returns_the_previous_state_and_is_idempotent(ppisp):
    assert ppisp.install_fused_controller(False) is False                       # off by default (the fixture restored it)
    assert ppisp.install_fused_controller() is False
    assert ppisp.install_fused_controller() is True
    assert ppisp.install_fused_controller(True) is True
    assert ppisp.install_fused_controller(False) is True
    assert ppisp.install_fused_controller(False) is False
    for key in ("controller_hip_calls", "controller_torch_calls", "controller_hip_backward_calls"):
        assert ppisp.stats[key] >= 0


def test_cpu_tensors_run_the_torch_code_whatever_the_switch_says(ppisp):
    ctrl = R.make_controller(4)
    g = torch.Generator().manual_seed(4)
    hdr, prior, go = torch.rand(12, 17, 3, generator=g), torch.tensor([0.2]), torch.randn(9, generator=g)

    def run():
        for p in ctrl.parameters():
            p.grad = None
        e, c = ctrl(hdr, prior)
        (torch.cat([e.reshape(1), c]) * go).sum().backward()
        return e.detach(), c.detach(), [p.grad.clone() for p in ctrl.parameters()]

    off = run()
    before = dict(ppisp.stats)
    ppisp.install_fused_controller()
    on = run()
    assert ppisp.stats["controller_torch_calls"] == before["controller_torch_calls"] + 1
    assert ppisp.stats["controller_hip_calls"] == before["controller_hip_calls"]
    assert off[0].shape == on[0].shape == () and off[1].shape == on[1].shape == (8,)
    assert torch.equal(off[0], on[0]) and torch.equal(off[1], on[1]) and all(torch.equal(a, b) for a, b in zip(off[2], on[2]))
    assert list(ctrl.state_dict()) == list(ppisp._PPISPController().state_dict())
    fresh = ppisp._PPISPController()
    assert all(float(p.detach().abs().max()) == 0 for head in (fresh.exposure_head, fresh.color_head) for p in head.parameters())


def test_conditioning_keeps_the_gates_away_from_rounding():
    """What the GPU tests rely on: conditioning ends within its rounds (make_case asserts it), leaves no window flagged, and a window
    that sits on a gate is noticed."""
    for shape in ((3, 5), (9, 13), (15, 15), (31, 37)):
        case = R.make_case(*shape)
        print(shape, "redrawn", case["redrawn"], "rounds", case["rounds"])
        assert case["rounds"] <= R.MAX_ROUNDS and case["e32_out"] < 1e-5
    case = R.make_case(121, 212)
    print("121x212: redrawn", case["redrawn"], "rounds", case["rounds"], "e32 out", case["e32_out"])
    assert case["rounds"] <= R.MAX_ROUNDS
    ctrl64 = __import__("copy").deepcopy(case["ctrl"]).double()
    # pushing one window onto a gate is noticed: a constant window ties all nine conv1 outputs
    hdr = case["hdr"].clone()
    hdr[3:6, 6:9] = 0.5
    bad = R.flagged(ctrl64, hdr.double(), case["prior"].double())
    assert bool(bad[1, 2]) and int(bad.sum()) == 1
