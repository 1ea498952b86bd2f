"""GPU: csrc/mlp.hip, the fused forward of the NHT decoder's network, through 3dgrut_amd.tcnn.

Exact chain: sparse +-1 integer networks on integer inputs (tests/mlp_reference.py: integer_network) must come out BIT-EQUAL to the plain
integer matrix products - any slip in the k permutation, the weight image, the input order, the output rows or the tail handling moves
whole integers.  Parity: random weights and inputs against the float64 restatement within 4x the deviation that mlp_torch (fp32, CPU)
showed on the very same case (mlp_reference.PARITY_TOL; 4: the MFMA sums its k-steps in another order than the host, and one flipped
bf16 rounding of a hidden activation moves an output by about 2^-9 of a weight), and against mlp_torch on the device under the same
bound.  Then: weights changed in place through .data are seen by the next call, two calls are bitwise equal, the training Function, and
the configurations that take the torch path."""
import importlib

import numpy as np
import pytest
import torch

import mlp_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHAIN_P = (1, 31, 32, 33, 127, 129, 300)
CHAIN_SHAPES = ((3, 1), (12, 3), (24, 3), (55, 4))      # (F, L): K0 = 16, 32, 48, 80, all with ones-padded columns


@pytest.fixture(scope="module")
def tcnn():
    return importlib.import_module("3dgrut_amd.tcnn")


@pytest.fixture(scope="module")
def parity():
    """name -> (cfg, params, x, float64 restatement), computed once"""
    cases = {}
    for name in (*R.PARITY_CASES, *R.FALLBACK_CASES):
        cfg, params, x = R.parity_case(name)
        cases[name] = (cfg, params, x, R.forward(params, x, cfg)[0])
    return cases


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _hip(tcnn, params, x, cfg):
    """the dispatcher, which has to take the kernel for these tensors"""
    before = dict(tcnn.stats)
    with torch.no_grad():
        out = tcnn.mlp(params, x, tcnn.MlpConfig(*cfg))
    assert tcnn.stats["hip_calls"] == before["hip_calls"] + 1 and tcnn.stats["torch_calls"] == before["torch_calls"]
    return out


@pytest.mark.parametrize("layers", [1, 2, 3, 5])
@pytest.mark.parametrize("width", [64, 128])
def test_exact_integer_chain_is_bit_equal(tcnn, width, layers):
    for f, degree in CHAIN_SHAPES:
        for act in ("none", "relu"):
            cfg = R.Config(f, degree, layers, width, 3, act)
            params = R.integer_network(cfg)
            x = R.integer_input(cfg, max(CHAIN_P))
            want = R.integer_forward(params, x, cfg)
            assert np.count_nonzero(want) > want.size // 8                    # not a dead network
            dp, dx = _dev(params), _dev(x)
            for n in CHAIN_P:
                got = _hip(tcnn, dp, dx[:n].clone(), cfg).cpu().numpy()
                assert got.shape == (n, 3)
                assert np.array_equal(got.view(np.uint32), want[:n].view(np.uint32)), (f, degree, act, n, np.argwhere(got != want[:n])[:4])


def test_exact_chain_with_sixteen_outputs(tcnn):
    cfg = R.Config(24, 3, 2, 128, 16, "none")
    params, x = R.integer_network(cfg), R.integer_input(cfg, 97)
    got = _hip(tcnn, _dev(params), _dev(x), cfg).cpu().numpy()
    assert np.array_equal(got, R.integer_forward(params, x, cfg))


@pytest.mark.parametrize("name", sorted(R.PARITY_CASES))
def test_parity_with_the_restatement_and_with_mlp_torch(tcnn, parity, name):
    cfg, params, x, want = parity[name]
    dp, dx = _dev(params), _dev(x)
    got = _hip(tcnn, dp, dx, cfg)
    with torch.no_grad():
        torch_path = tcnn.mlp_torch(dp, dx, tcnn.MlpConfig(*cfg))
    e_ref = float(np.abs(got.cpu().numpy() - want).max())
    e_torch = float((got - torch_path).abs().max())
    e_torch_ref = float(np.abs(torch_path.cpu().numpy() - want).max())
    print(f"\n{name}: fused vs restatement {e_ref:.3e}, fused vs mlp_torch on the device {e_torch:.3e}, mlp_torch on the device vs "
          f"restatement {e_torch_ref:.3e}; bound {4 * R.PARITY_TOL[name]:.3e}")
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert e_ref <= 4 * R.PARITY_TOL[name]
    assert e_torch <= 4 * R.PARITY_TOL[name]


def test_weights_changed_through_data_are_live_and_calls_are_deterministic(tcnn, parity):
    cfg, params, x, _ = parity["shipped_scale3"]
    enc = {"otype": "Composite", "nested": [{"otype": "Identity", "n_dims_to_encode": 24}, {"otype": "SphericalHarmonics", "degree": 3, "n_dims_to_encode": 3}]}
    net = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "Sigmoid", "n_neurons": 128, "n_hidden_layers": 3}
    module = tcnn.NetworkWithInputEncoding(27, 3, enc, net).to(DEV)
    assert module.params.is_cuda and tuple(module.cfg) == tuple(cfg)
    with torch.no_grad():
        module.params.copy_(_dev(params))
    dx = _dev(x)
    calls = tcnn.stats["hip_calls"]
    with torch.no_grad():
        first, again = module(dx), module(dx)
    assert tcnn.stats["hip_calls"] == calls + 2
    assert torch.equal(first, again)                                              # bitwise
    version = module.params._version
    module.params.data.mul_(0.5)                                                  # what the decoder's EMA swap does: no version bump
    assert module.params._version == version
    with torch.no_grad():
        halved = module(dx)
    want = R.forward(params * np.float32(0.5), x, cfg)[0]
    assert float(np.abs(halved.cpu().numpy() - want).max()) <= 4 * R.PARITY_TOL["shipped_scale3"]
    assert float((halved - first).abs().max()) > 100 * R.PARITY_TOL["shipped_scale3"]
    assert torch.equal(halved, _hip(tcnn, module.params.detach().clone(), dx, cfg))   # and exactly what fresh tensors give


def test_the_training_function(tcnn):
    cfg = R.Config(24, 3, 3, 128, 3, "sigmoid")
    rng = np.random.default_rng(21)
    params, x, go = R.xavier_params(rng, cfg), R.random_input(rng, 37, 24, 3.0), rng.normal(size=(37, 3)).astype(np.float32)
    plain = _hip(tcnn, _dev(params), _dev(x), cfg)
    p1, x1 = _dev(params).requires_grad_(True), _dev(x).requires_grad_(True)
    before = dict(tcnn.stats)
    out = tcnn.mlp(p1, x1, tcnn.MlpConfig(*cfg))
    assert tcnn.stats["hip_calls"] == before["hip_calls"] + 1 and out.requires_grad
    assert torch.equal(out.detach(), plain)                                       # the Function's forward IS the kernel
    gx, gp = torch.autograd.grad(out, [x1, p1], _dev(go))
    assert tcnn.stats["backward_calls"] == before["backward_calls"] + 1
    p2, x2 = _dev(params).requires_grad_(True), _dev(x).requires_grad_(True)
    wx, wp = torch.autograd.grad(tcnn.mlp_torch(p2, x2, tcnn.MlpConfig(*cfg)), [x2, p2], _dev(go))
    ex, ep = float((gx - wx).abs().max()), float((gp - wp).abs().max())
    print(f"\ntraining Function vs mlp_torch alone: d/dx {ex:.3e} (bound {R.GRAD_X_TOL:.3e}), d/dparams {ep:.3e} (bound {R.GRAD_PARAMS_TOL:.3e})")
    assert gx.shape == (37, 27) and gp.shape == (R.n_params(cfg),)
    assert ex <= R.GRAD_X_TOL and ep <= R.GRAD_PARAMS_TOL
    assert gx[:, 24:].abs().max() > 0 and gp.abs().max() > 0                       # the direction columns have a gradient too
    assert not gp[-13 * 128:].any()                                               # the padded output rows: exactly zero
    # and against the float64 restatement's hand-written backward
    want, cache = R.forward(params, x, cfg)
    rx, rp = R.backward(cache, go.astype(np.float64), cfg)
    assert np.abs(gx.cpu().numpy() - rx).max() <= 2 * R.GRAD_X_TOL and np.abs(gp.cpu().numpy() - rp).max() <= 2 * R.GRAD_PARAMS_TOL
    # only one of the two needs a gradient
    gx_only, = torch.autograd.grad(tcnn.mlp(_dev(params), x1, tcnn.MlpConfig(*cfg)), [x1], _dev(go))
    assert torch.equal(gx_only, gx)


@pytest.mark.parametrize("name", sorted(R.FALLBACK_CASES))
def test_configurations_the_kernel_does_not_take_run_mlp_torch(tcnn, parity, name):
    cfg, params, x, want = parity[name]
    assert tcnn.lds_bytes(tcnn.MlpConfig(*cfg)) == 0
    before = dict(tcnn.stats)
    with torch.no_grad():
        got = tcnn.mlp(_dev(params), _dev(x), tcnn.MlpConfig(*cfg))
    assert tcnn.stats["torch_calls"] == before["torch_calls"] + 1 and tcnn.stats["hip_calls"] == before["hip_calls"]
    err = float(np.abs(got.cpu().numpy() - want).max())
    print(f"\n{name}: torch path on the device vs restatement {err:.3e}; bound {4 * R.VALUE_TOL:.3e}")
    assert err <= 4 * R.VALUE_TOL


def test_inputs_the_kernel_does_not_take_agree_with_it(tcnn, parity):
    cfg, params, x, _ = parity["shipped_scale3"]
    tol = 4 * R.PARITY_TOL["shipped_scale3"]
    dp, dx = _dev(params), _dev(x[:513])
    config = tcnn.MlpConfig(*cfg)
    # fp16 rows: the torch path on them against the kernel on the same (already rounded) values
    half = dx.half()
    before = dict(tcnn.stats)
    with torch.no_grad():
        got = tcnn.mlp(dp, half, config)
    assert tcnn.stats["torch_calls"] == before["torch_calls"] + 1 and got.dtype == torch.float32
    assert float((got - _hip(tcnn, dp, half.float(), cfg)).abs().max()) <= tol
    # rows that are not contiguous
    wide = torch.zeros(513, 40, device=DEV)
    wide[:, :27] = dx
    view = wide[:, :27]
    assert not view.is_contiguous()
    before = dict(tcnn.stats)
    with torch.no_grad():
        got = tcnn.mlp(dp, view, config)
    assert tcnn.stats["torch_calls"] == before["torch_calls"] + 1
    assert float((got - _hip(tcnn, dp, dx, cfg)).abs().max()) <= tol
