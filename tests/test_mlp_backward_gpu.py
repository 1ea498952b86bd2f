"""GPU: csrc/mlp_backward.hip, the fused backward of the NHT decoder's network, through 3dgrut_amd.tcnn with install_fused_backward().

Exact chain: sparse +-1 integer networks on integer inputs with integer grad_out must give gradients BIT-EQUAL to the plain int64 ones -
any slip in the W^T fragments, the gate alignment, either transpose, the tiles of dW that a wave owns, the ordered reduction or the tail
handling moves whole integers.  Gate-exact real gradients: networks whose ReLU gates cannot depend on a summation order, against the
float64 restatement within 4x what mlp_backward_torch (fp32, CPU) showed on the very same arrays - the tight test of the dZ rounding
points, the SH Jacobian and the bias columns.  Random parity under the (gate-flip dominated) grid constants.  Then the behaviour: bitwise
repeatable, grad_input independent of grad_params, live weights, the counters, the fall-backs, the module under autograd."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import mlp_backward_reference as B
import mlp_reference as R
from test_mlp_backward_cpu import parity_grad_out

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHAIN_P = (1, 31, 32, 33, 127, 128, 129, 300)
CHAIN_SHAPES = ((3, 1), (12, 3), (24, 3), (55, 4))      # (F, L): K0 = 16, 32, 48, 80, all with ones-padded columns
SHIPPED = R.Config(24, 3, 3, 128, 3, "sigmoid")


@pytest.fixture(scope="module")
def tcnn():
    return importlib.import_module("3dgrut_amd.tcnn")


@pytest.fixture()
def fused(tcnn):
    """the switch on for one test, then as it was"""
    previous = tcnn.install_fused_backward(True)
    yield tcnn
    tcnn.install_fused_backward(previous)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _grads(tcnn, params, x, grad_out, cfg, need_x=True, need_p=True, expect_hip=True):
    """both gradients of tcnn.mlp through autograd -> (grad_x or None, grad_params or None) on the device"""
    p, v = _dev(params).requires_grad_(need_p), _dev(x).requires_grad_(need_x)
    before = dict(tcnn.stats)
    out = tcnn.mlp(p, v, tcnn.MlpConfig(*cfg))
    got = list(torch.autograd.grad(out, [t for t, need in ((v, need_x), (p, need_p)) if need], _dev(grad_out)))
    assert tcnn.stats["backward_calls"] == before["backward_calls"] + 1
    assert tcnn.stats["hip_backward_calls"] == before["hip_backward_calls"] + bool(expect_hip)
    return (got.pop(0) if need_x else None, got.pop(0) if need_p else None)


def _check_exact(tcnn, cfg, params, x, go, label):
    want_x, want_p, (big_dz, big_sum) = B.integer_backward(params, x, go, cfg)
    assert big_dz <= 256 and big_sum < 2 ** 24, (label, big_dz, big_sum)          # exact in bf16, exact in fp32 sums of any order
    gx, gp = _grads(tcnn, params, x, go, cfg)
    gx, gp = gx.cpu().numpy(), gp.cpu().numpy()
    f = cfg.n_features
    assert gx.shape == x.shape and gp.shape == (R.n_params(cfg),)
    assert np.array_equal(gx[:, :f], want_x.astype(np.float32)), (label, np.argwhere(gx[:, :f] != want_x)[:4])
    assert not gx[:, f:].any(), label                                             # the direction columns: their weights are zero
    live = ~B.sh_columns_of_the_first_matrix(cfg)
    assert np.array_equal(gp[live], want_p.astype(np.float32)[live]), (label, np.argwhere((gp != want_p) & live)[:4])
    padded = gp[-(R.OUT_ROWS - cfg.n_output_dims) * cfg.width:] if cfg.n_output_dims < R.OUT_ROWS else gp[:0]
    assert not padded.view(np.uint32).any(), label                                # the padded output rows: +0.0
    return want_x, want_p


# ---- 1. bit-exact integer chain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [1, 2, 3, 5])
@pytest.mark.parametrize("width", [64, 128])
def test_exact_integer_backward_is_bit_equal(fused, width, layers):
    taken, live = 0, np.zeros(2, dtype=np.int64)
    for f, degree in CHAIN_SHAPES:
        for act in ("none", "relu"):
            cfg = R.Config(f, degree, layers, width, 3, act)
            if fused.backward_lds_bytes(fused.MlpConfig(*cfg)) == 0:
                continue                                                          # the image leaves no room for the tiles: the torch backward
            taken += 1
            params, x, go = R.integer_network(cfg), R.integer_input(cfg, max(CHAIN_P)), B.integer_grad_out(cfg, max(CHAIN_P))
            for n in CHAIN_P:
                want_x, want_p = _check_exact(fused, cfg, params, x[:n], go[:n], (cfg, n))
            live += (np.count_nonzero(want_x), np.count_nonzero(want_p))
    assert taken == (0 if (width, layers) == (128, 5) else 8)
    assert taken == 0 or (live > 1000).all()                                      # not dead networks
    assert fused.backward_lds_bytes(fused.MlpConfig(*SHIPPED)) != 0


@pytest.mark.parametrize("width", [64, 128])
def test_exact_backward_with_sixteen_outputs(fused, width):
    for act in ("none", "relu"):
        cfg = R.Config(24, 3, 2, width, 16, act)
        params, x, go = R.integer_network(cfg), R.integer_input(cfg, 161), B.integer_grad_out(cfg, 161)
        _check_exact(fused, cfg, params, x, go, cfg)


@pytest.mark.parametrize("width", [64, 128])
def test_exact_backward_over_more_than_one_step_per_workgroup(fused, width):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * 128 * cus + 77
    cfg = R.Config(24, 3, 3, width, 3, "relu")
    params, x = R.integer_network(cfg), R.integer_input(cfg, n)
    go = B.integer_grad_out(cfg, n, every=16)                                     # one pixel in 16: the sums stay below 2^24
    _check_exact(fused, cfg, params, x, go, (cfg, n))


def test_the_kernel_writes_every_element_and_nothing_else(fused):
    lib = importlib.import_module("3dgrut_amd._abi").load_library()
    for cfg, n in ((R.Config(24, 3, 3, 128, 3, "none"), 300), (R.Config(12, 3, 2, 64, 16, "relu"), 129)):
        params, x, go = R.integer_network(cfg), R.integer_input(cfg, n), B.integer_grad_out(cfg, n)
        want_x, want_p = _grads(fused, params, x, go, cfg)
        config = fused.MlpConfig(*cfg)
        struct, cols, count = config.as_struct(), cfg.n_features + 3, R.n_params(cfg)
        gx = torch.full((n + 1, cols), 12345.0, device=DEV)
        gp = torch.full((count + cfg.width,), 12345.0, device=DEV)
        scratch = torch.empty(lib.grut_mlp_backward_scratch_bytes(ctypes.byref(struct), n), dtype=torch.uint8, device=DEV)
        dp, dx, dg = _dev(params), _dev(x), _dev(go)
        rc = lib.grut_mlp_backward(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(struct), ctypes.c_void_p(dp.data_ptr()),
                                   ctypes.c_void_p(dx.data_ptr()), ctypes.c_void_p(dg.data_ptr()), n, ctypes.c_void_p(scratch.data_ptr()),
                                   ctypes.c_void_p(gx.data_ptr()), ctypes.c_void_p(gp.data_ptr()))
        assert rc == 0, lib.grut_last_error()
        torch.cuda.synchronize()
        assert torch.equal(gx[:n], want_x) and torch.equal(gp[:count], want_p)    # every element written, pattern gone
        assert (gx[n] == 12345.0).all() and (gp[count:] == 12345.0).all()         # the guard rows untouched


# ---- 2. gate-exact real gradients ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(B.GATE_EXACT_CASES))
def test_gate_exact_gradients_against_the_restatement(fused, name):
    cfg, params, x, go = B.gate_exact_case(name)
    _, cache = R.forward(params, x, cfg)
    want_x, want_p = B.backward_bf16(cache, go.astype(np.float64), cfg)
    gx, gp = _grads(fused, params, x, go, cfg)
    ex, ep = float(np.abs(gx.cpu().numpy() - want_x).max()), float(np.abs(gp.cpu().numpy() - want_p).max())
    print(f"\n{name}: fused backward vs backward_bf16, d/dx {ex:.3e} (bound {4 * B.GATE_EXACT_GRAD_X_TOL:.3e}), "
          f"d/dparams {ep:.3e} (bound {4 * B.GATE_EXACT_GRAD_PARAMS_TOL:.3e})")
    assert np.abs(want_x[:, cfg.n_features:]).max() > 1e-3                        # the direction columns carry a gradient here
    assert ex <= 4 * B.GATE_EXACT_GRAD_X_TOL and ep <= 4 * B.GATE_EXACT_GRAD_PARAMS_TOL


# ---- 3. random parity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.PARITY_CASES))
def test_parity_with_the_restatement_and_with_mlp_backward_torch(fused, name):
    cfg, params, x = R.parity_case(name)
    go = parity_grad_out(name)
    _, cache = R.forward(params, x, cfg)
    want_x, want_p = B.backward_bf16(cache, go, cfg)
    taken = fused.backward_lds_bytes(fused.MlpConfig(*cfg)) != 0
    gx, gp = _grads(fused, params, x, go.astype(np.float32), cfg, expect_hip=taken)
    tx, tp = fused.mlp_backward_torch(_dev(params), _dev(x), _dev(go.astype(np.float32)), fused.MlpConfig(*cfg))
    figures = [float(np.abs(gx.cpu().numpy() - want_x).max()), float(np.abs(gp.cpu().numpy() - want_p).max()),
               float((gx - tx).abs().max()), float((gp - tp).abs().max())]
    print(f"\n{name} ({'fused' if taken else 'torch'} backward): vs backward_bf16 d/dx {figures[0]:.3e}, d/dparams {figures[1]:.3e}; vs "
          f"mlp_backward_torch on the device d/dx {figures[2]:.3e}, d/dparams {figures[3]:.3e}; bounds {4 * B.BWD_GRAD_X_TOL:.3e}, "
          f"{4 * B.BWD_GRAD_PARAMS_TOL:.3e}")
    assert figures[0] <= 4 * B.BWD_GRAD_X_TOL and figures[2] <= 4 * B.BWD_GRAD_X_TOL
    assert figures[1] <= 4 * B.BWD_GRAD_PARAMS_TOL and figures[3] <= 4 * B.BWD_GRAD_PARAMS_TOL


# ---- 4. behaviour ------------------------------------------------------------------------------------------------------------------------------
def test_repeatable_and_grad_input_independent_of_grad_params(fused):
    cfg, params, x = R.parity_case("shipped_scale3")
    go = parity_grad_out("shipped_scale3").astype(np.float32)
    gx, gp = _grads(fused, params, x, go, cfg)
    gx2, gp2 = _grads(fused, params, x, go, cfg)
    assert torch.equal(gx, gx2) and torch.equal(gp, gp2)                          # bitwise
    only_x, _ = _grads(fused, params, x, go, cfg, need_p=False)
    _, only_p = _grads(fused, params, x, go, cfg, need_x=False)
    assert torch.equal(only_x, gx) and torch.equal(only_p, gp)


def test_weights_changed_between_forward_and_backward_are_seen(fused):
    cfg, params, x = R.parity_case("shipped_scale1")
    go = parity_grad_out("shipped_scale1").astype(np.float32)
    p, v = _dev(params).requires_grad_(True), _dev(x).requires_grad_(True)
    out = fused.mlp(p, v, fused.MlpConfig(*cfg))
    version = p._version
    p.data.mul_(0.5)                                                              # what the decoder's EMA swap does: no version bump
    assert p._version == version
    gx, gp = torch.autograd.grad(out, [v, p], _dev(go))
    want_x, want_p = _grads(fused, params * np.float32(0.5), x, go, cfg)          # the backward of the halved weights, bit for bit
    assert torch.equal(gx, want_x) and torch.equal(gp, want_p)
    full_x, _ = _grads(fused, params, x, go, cfg)
    assert not torch.equal(gx, full_x)


def test_the_counter_advances_only_with_the_switch_on(tcnn):
    cfg, params, x = R.parity_case("shipped_scale1")
    go = parity_grad_out("shipped_scale1").astype(np.float32)
    previous = tcnn.install_fused_backward(False)
    try:
        off = _grads(tcnn, params, x[:257], go[:257], cfg, expect_hip=False)
        assert tcnn.install_fused_backward(True) is False
        on = _grads(tcnn, params, x[:257], go[:257], cfg, expect_hip=True)
    finally:
        tcnn.install_fused_backward(previous)
    assert float((on[0] - off[0]).abs().max()) <= 4 * B.BWD_GRAD_X_TOL and float((on[1] - off[1]).abs().max()) <= 4 * B.BWD_GRAD_PARAMS_TOL
    assert not torch.equal(on[1], off[1])                                         # another path did run


def test_what_the_kernel_does_not_take_keeps_the_torch_backward(tcnn):
    """configurations and inputs that fall back give the very gradients they give with the switch off"""
    config = tcnn.MlpConfig(*SHIPPED)
    rng = np.random.default_rng(41)
    go = rng.normal(size=(257, 3)).astype(np.float32)

    def both(run):
        previous = tcnn.install_fused_backward(False)
        try:
            off = run()
            tcnn.install_fused_backward(True)
            calls = tcnn.stats["hip_backward_calls"]
            on = run()
            assert tcnn.stats["hip_backward_calls"] == calls
        finally:
            tcnn.install_fused_backward(previous)
        assert all(torch.equal(a, b) for a, b in zip(off, on))

    for name in sorted(R.FALLBACK_CASES):                                        # eight_layers: the forward kernel does not take it either;
        cfg, params, x = R.parity_case(name)                                      # width_32 likewise
        both(lambda: _torch_grads(tcnn, _dev(params), _dev(x), _dev(go), tcnn.MlpConfig(*cfg)))
    five = R.Config(55, 4, 5, 128, 3, "sigmoid")                                  # the forward kernel takes it, the backward has no room
    assert tcnn.lds_bytes(tcnn.MlpConfig(*five)) != 0 and tcnn.backward_lds_bytes(tcnn.MlpConfig(*five)) == 0
    rng5 = np.random.default_rng(42)
    p5, x5 = R.xavier_params(rng5, five), R.random_input(rng5, 257, 55, 3.0)
    both(lambda: _torch_grads(tcnn, _dev(p5), _dev(x5), _dev(go), tcnn.MlpConfig(*five)))
    _, params, x = R.parity_case("shipped_scale3")
    dp, dx = _dev(params), _dev(x[:257])
    both(lambda: _torch_grads(tcnn, dp, dx.double(), _dev(go), config))           # fp64 rows
    wide = torch.zeros(257, 40, device=DEV)
    wide[:, :27] = dx
    both(lambda: _torch_grads(tcnn, dp, wide[:, :27], _dev(go), config))          # rows that are not contiguous


def _torch_grads(tcnn, params, x, grad_out, config):
    p, v = params.clone().requires_grad_(True), x.clone().requires_grad_(True) if x.is_contiguous() else x.detach().requires_grad_(True)
    out = tcnn.mlp(p, v, config)
    return torch.autograd.grad(out, [v, p], grad_out.to(out.dtype))


def test_the_module_under_autograd(fused):
    enc = {"otype": "Composite", "nested": [{"otype": "Identity", "n_dims_to_encode": 24}, {"otype": "SphericalHarmonics", "degree": 3, "n_dims_to_encode": 3}]}
    net = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "Sigmoid", "n_neurons": 128, "n_hidden_layers": 3}
    module = fused.NetworkWithInputEncoding(27, 3, enc, net).to(DEV)
    cfg, params, x = R.parity_case("shipped_scale3")
    with torch.no_grad():
        module.params.copy_(_dev(params))
    v = _dev(x[:1000]).requires_grad_(True)
    calls = fused.stats["hip_backward_calls"]
    loss = ((module(v) - 0.25) ** 2).mean()
    gx, gp = torch.autograd.grad(loss, [v, module.params])
    assert fused.stats["hip_backward_calls"] == calls + 1
    out, cache = R.forward(params, x[:1000], cfg)
    want_x, want_p = B.backward_bf16(cache, 2.0 * (out - 0.25) / out.size, cfg)
    scale = 2.0 / out.size                                                        # the bounds are for grad_out ~ N(0, 1)
    assert np.abs(gx.cpu().numpy() - want_x).max() <= 4 * B.BWD_GRAD_X_TOL * scale
    assert np.abs(gp.cpu().numpy() - want_p).max() <= 4 * B.BWD_GRAD_PARAMS_TOL * scale
    assert gx.abs().max() > 0 and gp.abs().max() > 0 and not gp[-13 * 128:].any()
    loss.detach()
    (module(v).sum()).backward()                                                  # .backward() into .grad, an expanded grad_out
    assert module.params.grad is not None and v.grad is not None and torch.isfinite(module.params.grad).all()
