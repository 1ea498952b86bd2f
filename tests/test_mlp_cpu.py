"""CPU: the `tinycudann` drop-in (3dgrut_amd/tcnn.py, shims/tinycudann) without a GPU.  The shim and install(); the reference's own
FeatureDecoder built on it and driven through everything it does with the network; the refusals; mlp_torch against the float64
restatement of tests/mlp_reference.py, values and both gradients, which is also where the tolerances of mlp_reference.py are measured;
and a host emulation of the 64 lanes of mfma_f32_32x32x16_bf16 that runs the kernel's layer chain with the index functions of
csrc/mlp_layout.hpp on exact integer data.  What the kernel computes is covered by tests/test_mlp_gpu.py."""
import importlib
import importlib.util
import itertools
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import mlp_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"
DECODER = os.path.join(REFERENCE, "threedgrut", "model", "feature_decoder.py")
NEW_SYMBOLS = ("grut_mlp_forward", "grut_mlp_lds_bytes", "grut_mlp_num_params")
needs_reference = pytest.mark.skipif(not os.path.isfile(DECODER), reason="the reference checkout is only present in the build container")

# the grid on which VALUE_TOL, GRAD_X_TOL and GRAD_PARAMS_TOL of mlp_reference.py are measured
GRID = list(itertools.product((3, 12, 24, 55), (1, 3, 4), (64, 128), (1, 3), ("none", "relu", "sigmoid"), (1.0, 3.0)))
GRID_P = 37


@pytest.fixture()
def tcnn():
    return importlib.import_module("3dgrut_amd.tcnn")


def _configs(n_features=24, degree=3, width=128, layers=3, output_activation="Sigmoid", encoding="SphericalHarmonics"):
    """the two dictionaries exactly as threedgrut/model/feature_decoder.py:69-90 writes them"""
    dir_enc = {"otype": "SphericalHarmonics", "degree": degree, "n_dims_to_encode": 3} if encoding == "SphericalHarmonics" else \
        {"otype": "Frequency", "n_frequencies": degree, "n_dims_to_encode": 3}
    return ({"otype": "Composite", "nested": [{"otype": "Identity", "n_dims_to_encode": n_features}, dir_enc]},
            {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": output_activation, "n_neurons": width, "n_hidden_layers": layers})


def _network(tcnn, **kw):
    enc, net = _configs(**kw)
    return tcnn.NetworkWithInputEncoding(n_input_dims=kw.get("n_features", 24) + 3, n_output_dims=3, encoding_config=enc, network_config=net)


# ---- shim and install --------------------------------------------------------------------------------------------------------------------------
def test_mlp_symbols_are_declared_mirrored_and_exported(grut_lib):
    abi = importlib.import_module("3dgrut_amd._abi")
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b(int|uint32_t) {name}\(", header), name
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(grut_lib, name) and getattr(grut_lib, name).argtypes, name
    assert abi.ABI_VERSION == 5 and grut_lib.grut_abi_version() == 5           # additive change
    assert len(grut_lib.grut_mlp_forward.argtypes) == 6
    import ctypes

    def both(*fields):
        c = abi.GrutMlpConfig(*fields)
        return grut_lib.grut_mlp_num_params(ctypes.byref(c)), grut_lib.grut_mlp_lds_bytes(ctypes.byref(c))

    # the shipped shape: K0 = 48; 128 x 48 + 2 x 128 x 128 + 16 x 128 weights; 12 + 2 x 32 + 8 fragments of 1 KiB
    assert both(24, 3, 3, 128, 3, abi.MLP_ACT_SIGMOID) == (40960, 84 * 1024)
    assert both(24, 3, 3, 64, 3, abi.MLP_ACT_NONE) == (64 * 48 + 2 * 64 * 64 + 16 * 64, (6 + 2 * 8 + 4) * 1024)
    assert both(112, 4, 1, 128, 16, abi.MLP_ACT_RELU) == (128 * 128 + 16 * 128, (32 + 8) * 1024)
    assert both(55, 4, 5, 128, 3, abi.MLP_ACT_NONE)[1] == (20 + 4 * 32 + 8) * 1024          # 156 KiB of the 160: fits
    assert both(24, 3, 8, 128, 3, abi.MLP_ACT_SIGMOID)[1] == 0                               # 236 KiB: does not
    for bad in ((24, 3, 3, 32, 3, 0), (24, 3, 3, 128, 17, 0), (24, 3, 3, 128, 0, 0), (24, 5, 3, 128, 3, 0), (24, 0, 3, 128, 3, 0),
                (113, 4, 3, 128, 3, 0), (24, 3, 0, 128, 3, 0), (24, 3, 3, 128, 3, 3)):
        assert both(*bad) == (0, 0), bad
    assert grut_lib.grut_mlp_lds_bytes(None) == 0
    # a refused call launches nothing and says why
    c = abi.GrutMlpConfig(24, 3, 8, 128, 3, abi.MLP_ACT_SIGMOID)
    assert grut_lib.grut_mlp_forward(None, ctypes.byref(c), None, None, 1, None) == -1
    assert b"does not fit" in grut_lib.grut_last_error()


def test_python_and_c_agree_on_the_parameter_count(grut_lib, tcnn):
    import ctypes
    for f, degree, layers, width in ((3, 1, 1, 64), (24, 3, 3, 128), (55, 4, 5, 128), (112, 4, 2, 64)):
        cfg = tcnn.MlpConfig(f, degree, layers, width, 3, "sigmoid")
        assert cfg.n_params == grut_lib.grut_mlp_num_params(ctypes.byref(cfg.as_struct())) == R.n_params(R.Config(*cfg))
        assert tcnn.lds_bytes(cfg) == grut_lib.grut_mlp_lds_bytes(ctypes.byref(cfg.as_struct())) != 0


def test_the_shim_package_resolves_to_this_project(monkeypatch, tcnn):
    monkeypatch.delitem(sys.modules, "tinycudann", raising=False)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "shims"))
    import tinycudann
    assert tinycudann.__file__ == os.path.join(ROOT, "shims", "tinycudann", "__init__.py")
    assert tinycudann.NetworkWithInputEncoding is tcnn.NetworkWithInputEncoding
    assert not hasattr(tinycudann, "supports_jit_fusion")


def test_install_registers_the_package_unless_one_is_there(monkeypatch, tcnn):
    monkeypatch.delitem(sys.modules, "tinycudann", raising=False)
    tcnn.install()
    import tinycudann
    assert tinycudann.NetworkWithInputEncoding is tcnn.NetworkWithInputEncoding and not hasattr(tinycudann, "supports_jit_fusion")
    mine = types.ModuleType("tinycudann")
    monkeypatch.setitem(sys.modules, "tinycudann", mine)
    tcnn.install()
    assert sys.modules["tinycudann"] is mine                                     # a package that is already there wins
    for shim in ("threedgut_tracer", "threedgrt_tracer"):                        # both tracer shims call it, next to the other two
        text = open(os.path.join(ROOT, "shims", shim, "__init__.py")).read()
        assert text.index('"3dgrut_amd.losses").install()') < text.index('"3dgrut_amd.ppisp").install()') < \
            text.index('"3dgrut_amd.tcnn").install()')


@pytest.mark.parametrize("shim", ["threedgut_tracer", "threedgrt_tracer"])
def test_importing_a_tracer_shim_registers_tinycudann(monkeypatch, tcnn, shim):
    for name in ("tinycudann", shim):
        monkeypatch.delitem(sys.modules, name, raising=False)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "shims"))
    importlib.import_module(shim)
    assert sys.modules["tinycudann"].NetworkWithInputEncoding is tcnn.NetworkWithInputEncoding
    monkeypatch.delitem(sys.modules, shim, raising=False)


# ---- the module's surface ---------------------------------------------------------------------------------------------------------------------
def test_module_surface_and_seeded_initialisation(tcnn):
    net = _network(tcnn)
    assert (net.n_input_dims, net.n_output_dims, net.n_params) == (27, 3, 40960)
    assert [n for n, _ in net.named_parameters()] == ["params"] and list(net.state_dict()) == ["params"]
    assert net.params.dtype == torch.float32 and net.params.shape == (40960,) and net.params.requires_grad
    assert torch.equal(net.params, _network(tcnn).params)                        # the default seed, a CPU generator
    enc, cfg = _configs()
    other = tcnn.NetworkWithInputEncoding(27, 3, enc, cfg, seed=7)
    assert not torch.equal(net.params, other.params)
    offset = 0
    for rows, columns in net.cfg.matrices:                                       # Xavier uniform, matrix by matrix
        w = net.params.detach()[offset:offset + rows * columns]
        bound = (6.0 / (rows + columns)) ** 0.5
        assert w.abs().max() <= bound and w.abs().max() > 0.9 * bound and abs(float(w.mean())) < 0.05 * bound
        offset += rows * columns
    assert offset == net.n_params
    with pytest.raises(ValueError, match=r"\[P, 27\]"):
        net(torch.zeros(4, 26))


def test_refusals_name_the_key(tcnn):
    def build(enc=None, net=None, n_in=27, n_out=3):
        e, n = _configs()
        return tcnn.NetworkWithInputEncoding(n_in, n_out, {**e, **(enc or {})}, {**n, **(net or {})})

    with pytest.raises(NotImplementedError, match="Frequency"):
        tcnn.NetworkWithInputEncoding(27, 3, *_configs(encoding="Frequency"))
    sh = {"otype": "SphericalHarmonics", "degree": 3, "n_dims_to_encode": 3}
    ident = {"otype": "Identity", "n_dims_to_encode": 24}
    for enc, key in (({"otype": "HashGrid"}, "encoding_config.otype"),
                     ({"nested": [ident, sh, sh]}, "encoding_config.nested"),
                     ({"nested": [ident]}, "encoding_config.nested"),
                     ({"nested": [sh, ident]}, "encoding_config.nested"),
                     ({"nested": [ident, {**sh, "n_dims_to_encode": 2}]}, "n_dims_to_encode"),
                     ({"nested": [ident, {**sh, "degree": 5}]}, "degree"),
                     ({"nested": [ident, {"otype": "OneBlob", "n_dims_to_encode": 3}]}, "encoding_config.nested.otype")):
        with pytest.raises(NotImplementedError, match=key):
            build(enc=enc)
    for net, key in (({"activation": "Tanh"}, "network_config.activation"), ({"output_activation": "Exponential"}, "output_activation"),
                     ({"otype": "CutlassMLP"}, "network_config.otype"), ({"n_neurons": 100}, "n_neurons"),
                     ({"n_hidden_layers": 0}, "n_hidden_layers")):
        with pytest.raises(NotImplementedError, match=key):
            build(net=net)
    with pytest.raises(NotImplementedError, match="n_output_dims"):
        build(n_out=17)
    with pytest.raises(ValueError, match="n_input_dims"):
        build(n_in=30)
    for activation in ("None", "ReLU", "Sigmoid"):
        assert build(net={"output_activation": activation}).cfg.output_activation == activation.lower()


# ---- the reference's own decoder on the drop-in -----------------------------------------------------------------------------------------------
@pytest.fixture()
def feature_decoder(monkeypatch, tcnn):
    """threedgrut/model/feature_decoder.py imported unchanged, its `import tinycudann` resolved by the shim package"""
    monkeypatch.delitem(sys.modules, "tinycudann", raising=False)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "shims"))
    spec = importlib.util.spec_from_file_location("_reference_feature_decoder", DECODER)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    assert module.tcnn.NetworkWithInputEncoding is tcnn.NetworkWithInputEncoding
    return module


def _decoder_expectation(decoder, features, dirs, alpha=None):
    """what FeatureDecoder.forward has to return, from the float64 restatement"""
    cfg = R.Config(*decoder.network.cfg)
    f = features.reshape(-1, features.shape[-1]).double()
    a = None if alpha is None else alpha.reshape(-1, 1).double().clamp(min=1e-8)
    if a is not None:
        f = f / a
    x = torch.cat([f, (dirs.reshape(-1, 3).double() * decoder.sh_scale + 1.0) * 0.5], dim=-1).float().numpy()
    out, _ = R.forward(decoder.network.params.detach().numpy(), x, cfg)
    out = torch.from_numpy(out)
    return (out if a is None else out * a).reshape(*features.shape[:-1], 3)


@needs_reference
def test_the_reference_decoder_runs_on_the_drop_in(feature_decoder):
    torch.manual_seed(3)
    tol = 2 * R.VALUE_TOL
    decoder = feature_decoder.FeatureDecoder(24, 128, 3, "SphericalHarmonics", 3, 3.0, "Sigmoid", ema_decay=0.95)
    assert decoder.network.cfg == (24, 3, 3, 128, 3, "sigmoid") and not hasattr(decoder.network, "jit_fusion")
    assert list(decoder._ema_shadow) == ["network.params"]
    for shape in ((1, 5, 7), (35,)):
        features, dirs = torch.randn(*shape, 24) * 0.5, torch.nn.functional.normalize(torch.randn(*shape, 3), dim=-1)
        alpha = torch.rand(*shape, 1) * 0.9 + 0.05
        out = decoder(features, dirs)
        assert out.shape == (*shape, 3) and out.dtype == torch.float32
        assert (out - _decoder_expectation(decoder, features, dirs)).abs().max() <= tol
        assert torch.equal(out, decoder(features, dirs, alpha))                   # alpha is ignored unless asked for
        decoder.unpremultiply_alpha = True
        out = decoder(features, dirs, alpha)
        assert (out - _decoder_expectation(decoder, features, dirs, alpha)).abs().max() <= tol
        decoder.unpremultiply_alpha = False
    with pytest.raises(NotImplementedError, match="Frequency"):
        feature_decoder.FeatureDecoder(24, 128, 3, "Frequency", 3)

    reg = decoder.regularization_loss()
    assert torch.allclose(reg, (decoder.network.params.detach().double() ** 2).sum().float())
    reg.backward()
    assert torch.allclose(decoder.network.params.grad, 2 * decoder.network.params.detach())
    decoder.zero_grad()

    # an Adam step changes the weights and the output; the EMA helpers then swap the OUTPUT, not only the tensor
    features, dirs = torch.randn(35, 24) * 0.5, torch.nn.functional.normalize(torch.randn(35, 3), dim=-1)
    before = decoder(features, dirs).detach()
    optimizer = torch.optim.Adam(decoder.parameters(), lr=1e-2)
    loss = ((decoder(features, dirs) - 0.25) ** 2).mean()
    loss.backward()
    assert decoder.network.params.grad is not None and decoder.network.params.grad.abs().max() > 0
    assert not decoder.network.params.grad[-13 * 128:].any()                      # the padded output rows
    optimizer.step()
    trained = decoder(features, dirs).detach()
    assert ((trained - 0.25) ** 2).mean() < loss.detach() and not torch.equal(trained, before)
    decoder.ema_update(global_step=1)                                             # shadow = 0.95 initial + 0.05 trained
    version = decoder.network.params._version
    decoder.apply_ema_shadow()
    assert decoder.network.params._version == version                            # param.data.copy_ is invisible to autograd's counter ...
    shadow = decoder(features, dirs).detach()
    assert not torch.equal(shadow, trained)                                       # ... and the output follows the weights all the same
    assert (shadow - _decoder_expectation(decoder, features, dirs)).abs().max() <= tol
    decoder.restore_ema()
    assert torch.equal(decoder(features, dirs).detach(), trained)

    clone = feature_decoder.FeatureDecoder(24, 128, 3, "SphericalHarmonics", 3, 3.0, "Sigmoid")
    assert not torch.equal(clone(features, dirs), trained)
    assert list(decoder.state_dict()) == ["network.params"]
    clone.load_state_dict(decoder.state_dict())
    assert torch.equal(clone(features, dirs), trained)
    assert decoder.to("cpu") is decoder


# ---- mlp_torch against the restatement ---------------------------------------------------------------------------------------------------------
def test_the_restatement_backward_is_the_derivative_of_its_forward():
    """central differences on the network WITHOUT the roundings (which the backward treats as straight-through)"""
    rng = np.random.default_rng(0)
    for act in ("none", "relu", "sigmoid"):
        cfg = R.Config(5, 4, 2, 16, 3, act)
        params = R.xavier_params(rng, cfg).astype(np.float64) * 2
        x = R.random_input(rng, 6, 5, 3.0).astype(np.float64)
        g = rng.normal(size=(6, 3))
        out, cache = R.forward(params, x, cfg, rounding=False)
        gx, gp = R.backward(cache, g, cfg)
        eps = 1e-6
        for arr, grad, picks in ((x, gx, [(0, 0), (1, 4), (2, 5), (3, 6), (4, 7), (5, 2)]), (params, gp, [0, 17, 16 * 32 + 3, 16 * 32 + 16 * 16 + 5])):
            for i in picks:
                keep = arr[i]
                arr[i] = keep + eps
                hi = (R.forward(params, x, cfg, rounding=False)[0] * g).sum()
                arr[i] = keep - eps
                lo = (R.forward(params, x, cfg, rounding=False)[0] * g).sum()
                arr[i] = keep
                assert abs((hi - lo) / (2 * eps) - grad[i]) <= 1e-6 * max(1.0, abs(grad[i])), (act, i)
        assert not gp[16 * 32 + 16 * 16 + 3 * 16:].any()


def test_bf16_rounding_by_bit_arithmetic_is_torch_bfloat16():
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.normal(size=4096) * 10.0 ** rng.integers(-6, 6, 4096), [0.0, -0.0, 1.0, 1.00390625, 1.01171875, 256.0, 257.0, 3.0e38]])
    want = torch.from_numpy(a).float().to(torch.bfloat16).double().numpy()
    assert np.array_equal(R.bf16_round(a), want)


def _deviation(tcnn, cfg, params, x, grad_out=None):
    """max |mlp_torch - restatement| of the values and, with grad_out, of both gradients"""
    want, cache = R.forward(params, x, cfg)
    xt, pt = torch.from_numpy(x).requires_grad_(grad_out is not None), torch.from_numpy(params).requires_grad_(grad_out is not None)
    got = tcnn.mlp_torch(pt, xt, tcnn.MlpConfig(*cfg))
    assert got.dtype == torch.float32 and got.shape == want.shape
    dev = [np.abs(got.detach().numpy() - want).max()]
    if grad_out is not None:
        gx, gp = torch.autograd.grad(got, [xt, pt], torch.from_numpy(grad_out).float())
        wx, wp = R.backward(cache, grad_out, cfg)
        dev += [np.abs(gx.numpy() - wx).max(), np.abs(gp.numpy() - wp).max()]
        rows = R.matrices(cfg)[-1][1] * (R.OUT_ROWS - cfg.n_output_dims)
        assert not gp[-rows:].any() and not wp[-rows:].any()                      # the padded output rows: exactly zero
    return dev


def test_mlp_torch_agrees_with_the_restatement_values_and_gradients(tcnn):
    worst = np.zeros(3)
    for index, (f, degree, width, layers, act, scale) in enumerate(GRID):
        cfg = R.Config(f, degree, layers, width, 3, act)
        rng = np.random.default_rng(1000 + index)
        params, x = R.xavier_params(rng, cfg), R.random_input(rng, GRID_P, f, scale)
        worst = np.maximum(worst, _deviation(tcnn, cfg, params, x, rng.normal(size=(GRID_P, 3))))
    print(f"\nmlp_torch vs float64 restatement over {len(GRID)} cases of {GRID_P} pixels: values {worst[0]:.3e}, d/dx {worst[1]:.3e}, "
          f"d/dparams {worst[2]:.3e}  (VALUE_TOL {R.VALUE_TOL:.3e}, GRAD_X_TOL {R.GRAD_X_TOL:.3e}, GRAD_PARAMS_TOL {R.GRAD_PARAMS_TOL:.3e})")
    assert worst[0] <= 2 * R.VALUE_TOL and worst[1] <= 2 * R.GRAD_X_TOL and worst[2] <= 2 * R.GRAD_PARAMS_TOL


@pytest.mark.parametrize("name", sorted(R.PARITY_CASES))
def test_the_gpu_parity_cases_on_the_cpu(tcnn, name):
    cfg, params, x = R.parity_case(name)
    dev = _deviation(tcnn, cfg, params, x)[0]
    print(f"\n{name}: mlp_torch vs float64 restatement, values {dev:.3e}  (PARITY_TOL {R.PARITY_TOL[name]:.3e})")
    assert dev <= 2 * R.PARITY_TOL[name]


def test_mlp_torch_dtypes_and_straight_through(tcnn):
    cfg = tcnn.MlpConfig(12, 3, 2, 64, 3, "sigmoid")
    rng = np.random.default_rng(4)
    params, x = torch.from_numpy(R.xavier_params(rng, R.Config(*cfg))), torch.from_numpy(R.random_input(rng, 9, 12, 3.0))
    base = tcnn.mlp_torch(params, x, cfg)
    assert tcnn.mlp_torch(params, x.double(), cfg).dtype == torch.float64
    assert (tcnn.mlp_torch(params, x.double(), cfg) - base).abs().max() <= 2 * R.VALUE_TOL
    for dt in (torch.float16, torch.bfloat16):
        got = tcnn.mlp_torch(params, x.to(dt), cfg)
        assert got.dtype == torch.float32 and torch.equal(got, tcnn.mlp_torch(params, x.to(dt).float(), cfg))
    # a rounding would have zero derivative almost everywhere: the gradient must be the unrounded network's
    xg = x.clone().requires_grad_(True)
    tcnn.mlp_torch(params, xg, cfg).sum().backward()
    assert xg.grad.abs().min(dim=0).values.max() > 0 and torch.isfinite(xg.grad).all()
    net = _network(tcnn, n_features=12, width=64, layers=2)
    before = tcnn.stats["torch_calls"]
    assert net(x).dtype == torch.float32 and tcnn.stats["torch_calls"] == before + 1   # a CPU tensor takes the torch path


# ---- the lane maps, emulated on the host --------------------------------------------------------------------------------------------------------
EMULATION = r"""
// Runs the layer chain of csrc/mlp.hip on the host: the 64 lanes of mfma_f32_32x32x16_bf16 emulated from the instruction's A / B / C maps,
// every index taken from mlp_layout.hpp, exact small-integer data.  Prints nothing and returns 0 when every configuration reproduces the
// plain matrix products.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>
#include "mlp_layout.hpp"
using namespace grut_mlp;

typedef float Frag[64][8];
typedef float Acc[64][16];

// D = A B + C with lane l = 32 h + r holding A[r][8 h + j], B[8 h + j][r] and D[(reg & 3) + 8 (reg >> 2) + 4 h][r]
static void mfma_32x32x16(const Frag a, const Frag b, Acc acc) {
    static float A[32][16], B[16][32], D[32][32];
    for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) A[l & 31][8 * (l >> 5) + j] = a[l][j], B[8 * (l >> 5) + j][l & 31] = b[l][j];
    for (int l = 0; l < 64; ++l)
        for (int reg = 0; reg < 16; ++reg) D[(reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5)][l & 31] = acc[l][reg];
    for (int i = 0; i < 32; ++i)
        for (int n = 0; n < 32; ++n)
            for (int k = 0; k < 16; ++k) D[i][n] += A[i][k] * B[k][n];
    for (int l = 0; l < 64; ++l)
        for (int reg = 0; reg < 16; ++reg) acc[l][reg] = D[(reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5)][l & 31];
}

static unsigned state = 12345u;
static unsigned rnd() { return state = state * 1664525u + 1013904223u, state >> 8; }
static bool is_bf16(float v) { unsigned u; memcpy(&u, &v, 4); return (u & 0xffffu) == 0; }

static int fail(const char* what, const Shape& s, int a, int b) {
    printf("%s: F %d L %d layers %d width %d at (%d, %d)\n", what, s.n_features, s.sh_degree, s.n_hidden_layers, s.width, a, b);
    return 1;
}

static int run(const Shape& s, int n_out) {
    const int nh = s.n_hidden_layers, K0 = k0(s), MB = row_blocks(s), KW = ksteps_hidden(s), nk0 = ksteps_first(s);
    // sparse +-1 weights, at most two non-zeros per row, every row of a matrix distinct; the unread output rows hold 7
    std::vector<float> params(num_params(s), 0.f);
    for (int layer = 0; layer <= nh; ++layer) {
        const int rows = layer_out(s, layer), cols = layer_in(s, layer);
        float* w = params.data() + param_offset(s, layer);
        std::set<std::string> seen;
        for (int r = 0; r < rows; ++r) {
            for (;;) {
                std::vector<float> row(cols, 0.f);
                row[rnd() % cols] = rnd() % 4 ? 1.f : -1.f;
                row[rnd() % cols] = rnd() % 4 ? 1.f : -1.f;
                std::string key((const char*)row.data(), cols * 4);
                if (seen.insert(key).second) { memcpy(w + (size_t)r * cols, row.data(), cols * 4); break; }
            }
            if (layer == nh && r >= n_out) for (int c = 0; c < cols; ++c) w[(size_t)r * cols + c] = 7.f;
        }
    }
    // the encoded input of 32 pixels: integer features and (for the emulation) integer "SH" values, distinct per pixel
    std::vector<float> feat(32 * (s.n_features + 1)), sh(32 * 16);
    for (auto& v : feat) v = (float)((int)(rnd() % 4) - 1);
    for (auto& v : sh) v = (float)((int)(rnd() % 4) - 1);
    auto encoded = [&](int pixel, int k) {   // the contract, in natural order
        return k < s.n_features ? feat[pixel * (s.n_features + 1) + k] : k < encoded_width(s) ? sh[pixel * 16 + k - s.n_features] : 1.f;
    };
    // the plain products
    std::vector<std::vector<float>> h(32, std::vector<float>(K0));
    for (int p = 0; p < 32; ++p) for (int k = 0; k < K0; ++k) h[p][k] = encoded(p, k);
    std::vector<std::vector<float>> want(32, std::vector<float>(n_out));
    for (int layer = 0; layer <= nh; ++layer) {
        const int rows = layer == nh ? n_out : s.width, cols = layer_in(s, layer);
        const float* w = params.data() + param_offset(s, layer);
        for (int p = 0; p < 32; ++p) {
            std::vector<float> z(rows);
            for (int r = 0; r < rows; ++r) { float sum = 0; for (int c = 0; c < cols; ++c) sum += w[(size_t)r * cols + c] * h[p][c]; z[r] = sum; }
            if (layer == nh) want[p] = z; else { for (auto& v : z) v = v > 0 ? v : 0; h[p] = z; }
        }
    }
    // the kernel's image: chunk by chunk, as the kernel builds it
    std::vector<float> image((size_t)num_frags(s) * 64 * 8, -99.f);
    for (uint32_t c = 0; c < num_frags(s) * 64u; ++c) {
        uint32_t src = 0;
        const bool live = image_chunk_source(s, n_out, c, &src);
        for (int j = 0; j < 8; ++j) {
            const float v = live ? params[src + (j >> 2) * 8 + (j & 3)] : 0.f;
            if (!is_bf16(v)) return fail("weight not exact in bf16", s, (int)c, j);
            image[(size_t)c * 8 + j] = v;
        }
    }
    if (image_bytes(s) != image.size() * 2) return fail("image size", s, 0, 0);
    auto weights = [&](int layer, int m, int t, Frag a) {   // one 16-byte read per lane
        for (int l = 0; l < 64; ++l) {
            const uint32_t off = image_offset(s, layer, m, t, l);
            if (off % 16 || off + 16 > image_bytes(s)) exit(fail("image offset", s, layer, l));
            memcpy(a[l], &image[off / 2], 32);
        }
    };
    // the kernel's chain
    static Acc acc[4], out;
    static Frag a, b, hb[8];
    memset(acc, 0, sizeof acc);
    for (int t = 0; t < nk0; ++t) {
        for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j) {
                const int e = mlp_input_element(s, t, l >> 5, j), p = l & 31;
                b[l][j] = e >= 0 ? feat[p * (s.n_features + 1) + e] : e == kInputOne ? 1.f : sh[p * 16 + (-1 - e)];
            }
        for (int m = 0; m < MB; ++m) weights(0, m, t, a), mfma_32x32x16(a, b, acc[m]);
    }
    for (int layer = 1; layer <= nh; ++layer) {
        for (int blk = 0; blk < MB; ++blk)   // ReLU, then registers 8 s .. 8 s + 7 of row block blk are k-step 2 blk + s
            for (int sub = 0; sub < 2; ++sub)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 8; ++j) {
                        const float v = acc[blk][l][8 * sub + j] > 0 ? acc[blk][l][8 * sub + j] : 0.f;
                        if (!is_bf16(v)) return fail("activation not exact in bf16", s, layer, l);
                        hb[2 * blk + sub][l][j] = v;
                    }
        if (layer < nh) {
            memset(acc, 0, sizeof acc);
            for (int m = 0; m < MB; ++m)
                for (int t = 0; t < KW; ++t) weights(layer, m, t, a), mfma_32x32x16(a, hb[t], acc[m]);
        } else {
            memset(out, 0, sizeof out);
            for (int t = 0; t < KW; ++t) weights(layer, 0, t, a), mfma_32x32x16(a, hb[t], out);
        }
    }
    int live_rows = 0;
    for (int l = 0; l < 64; ++l)
        for (int reg = 0; reg < 16; ++reg) {
            const int row = reg < 8 ? mlp_out_row(reg, l >> 5) : -1;   // the kernel stores registers 0 .. 7 only
            if (row >= 0 && row < n_out) {
                if (out[l][reg] != want[l & 31][row]) return fail("output differs", s, l, reg);
                live_rows += want[l & 31][row] != 0;
            } else if (out[l][reg] != 0.f && reg < 8) return fail("a padded row is not zero", s, l, reg);
        }
    if (live_rows < 8) return fail("the case is degenerate (almost every output is zero)", s, live_rows, 0);
    return 0;
}

int main() {
    int bad = 0, cases = 0;
    const int shapes[][2] = {{3, 1}, {12, 3}, {24, 3}, {55, 4}, {112, 4}, {16, 4}, {7, 3}};
    for (const auto& fl : shapes)
        for (int width = 64; width <= 128; width += 64)
            for (int layers = 1; layers <= 3; ++layers)
                for (int n_out = 3; n_out <= 16; n_out += 13) {
                    const Shape s{fl[0], fl[1], layers, width};
                    if (!lds_bytes(s)) return fail("shape not taken", s, 0, 0);
                    bad += run(s, n_out), ++cases;
                }
    // k-permutation and output rows are bijections
    for (int t = 0; t < 8; ++t) {
        bool seen[16] = {};
        for (int h = 0; h < 2; ++h) for (int j = 0; j < 8; ++j) seen[mlp_kperm(t, h, j) - 16 * t] = true;
        for (bool v : seen) bad += !v;
    }
    bool rows[32] = {};
    for (int h = 0; h < 2; ++h) for (int reg = 0; reg < 16; ++reg) rows[mlp_out_row(reg, h)] = true;
    for (bool v : rows) bad += !v;
    printf("%d cases, %d failures\n", cases, bad);
    return bad != 0;
}
"""


def test_lane_map_emulation_reproduces_the_integer_products(tmp_path):
    src, exe = tmp_path / "mlp_lanes.cpp", tmp_path / "mlp_lanes"
    src.write_text(EMULATION)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "3dgrut_amd", "csrc"), str(src), "-o", str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == "84 cases, 0 failures"
