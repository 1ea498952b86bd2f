"""CPU: the NHT decode stage (3dgrut_amd/decoder.py, grut_decode_forward / grut_decode_backward) without a GPU.  The entry points are
declared, mirrored and exported; decode_torch is held against the reference's own apply_feature_decoder and FeatureDecoder (where that
checkout exists); decode_backward_torch against the float64 restatement of tests/decode_reference.py; the host-assembled fp32 rows of the
GPU bit-equality tests against that restatement; the hook; and the tolerances of decode_reference.py are measured here."""
import ctypes
import importlib
import importlib.util
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import decode_reference as D
import mlp_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"
RENDER = os.path.join(REFERENCE, "threedgrut", "utils", "render.py")
DECODER = os.path.join(REFERENCE, "threedgrut", "model", "feature_decoder.py")
needs_reference = pytest.mark.skipif(not (os.path.isfile(RENDER) and os.path.isfile(DECODER)),
                                     reason="the reference checkout is only present in the build container")


@pytest.fixture(scope="module")
def tcnn():
    return importlib.import_module("3dgrut_amd.tcnn")


@pytest.fixture(scope="module")
def decoder():
    return importlib.import_module("3dgrut_amd.decoder")


def _config(decoder, tcnn, dcfg):
    return decoder.DecodeConfig(tcnn.MlpConfig(*dcfg.mlp), dcfg.sh_scale, dcfg.unpremultiply_alpha, dcfg.center_ray)


def _torch(inputs, dtype=torch.float32):
    return [torch.from_numpy(inputs[k]).to(dtype) for k in ("features", "alpha", "rays", "rot")]


# ---- the C surface ----------------------------------------------------------------------------------------------------------------------------------
def test_decode_symbols_are_declared_mirrored_and_exported(grut_lib, tmp_path):
    abi = importlib.import_module("3dgrut_amd._abi")
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    for name in ("grut_decode_forward", "grut_decode_backward"):
        assert re.search(rf"\bint {name}\s*\(", header) and name in abi.EXPORTED_SYMBOLS and hasattr(grut_lib, name)
        assert getattr(grut_lib, name).restype is ctypes.c_int
    assert len(grut_lib.grut_decode_forward.argtypes) == 10 and len(grut_lib.grut_decode_backward.argtypes) == 14
    assert abi.ABI_VERSION == 5 and grut_lib.grut_abi_version() == 5                    # additive: no struct of the ABI changed
    src, exe = tmp_path / "sz.c", tmp_path / "sz"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "grut_amd.h"\nint main(){printf("%zu %zu %zu %zu\\n",sizeof(GrutDecodeConfig),'
                   'offsetof(GrutDecodeConfig,sh_scale),offsetof(GrutDecodeConfig,unpremultiply_alpha),offsetof(GrutDecodeConfig,center_ray));return 0;}')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    mirror = abi.GrutDecodeConfig
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == \
        [ctypes.sizeof(mirror), mirror.sh_scale.offset, mirror.unpremultiply_alpha.offset, mirror.center_ray.offset]


def test_bad_arguments_are_refused_before_a_launch(grut_lib, tcnn, decoder):
    """every check of the two entry points comes before the first use of the device: the pointers here are never followed"""
    abi = importlib.import_module("3dgrut_amd._abi")
    fake = 4096                                                                         # a non-NULL, 16-byte aligned address

    def forward(cfg, alpha=fake, rays=fake, views=1, ppv=33, features=fake):
        return grut_lib.grut_decode_forward(None, ctypes.byref(cfg.as_struct()), fake, features, alpha, rays, fake, views, ppv, fake)

    def backward(cfg, alpha=fake, gf=fake, ga=None, gp=None, scratch=None):
        return grut_lib.grut_decode_backward(None, ctypes.byref(cfg.as_struct()), fake, fake, alpha, fake, fake, 1, 33, fake, scratch, gf, ga, gp)

    def refused(status, text):
        assert abi.STATUS_NAMES[status] == "BAD_INPUT" and text in grut_lib.grut_last_error().decode(), grut_lib.grut_last_error()

    base = _config(decoder, tcnn, D.DecodeConfig(D.SHIPPED, 1.0, False, False))
    refused(forward(base, rays=None), "only with center_ray")
    refused(forward(base._replace(unpremultiply_alpha=True), alpha=None), "needs alpha")
    refused(forward(base, views=0), "num_views > 0")
    refused(forward(base, views=65536, ppv=65536), "< 2^32")
    refused(forward(base, features=None), "features")
    refused(forward(base._replace(mlp=base.mlp._replace(width=32))), "width must be 64 or 128")
    refused(forward(base._replace(mlp=base.mlp._replace(n_hidden_layers=8))), "does not fit into LDS")
    refused(backward(base, gf=None), "all NULL")
    refused(backward(base, ga=fake), "grad_alpha needs unpremultiply_alpha")
    refused(backward(base, gp=fake), "needs the scratch")
    refused(backward(base._replace(mlp=base.mlp._replace(n_hidden_layers=6, width=64))), "more than 5 hidden layers")


# ---- decode_torch against the reference's own functions ---------------------------------------------------------------------------------------------
@pytest.fixture()
def reference(monkeypatch, tcnn):
    """threedgrut/utils/render.py and threedgrut/model/feature_decoder.py imported unchanged, `import tinycudann` resolved by the shim"""
    monkeypatch.delitem(sys.modules, "tinycudann", raising=False)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "shims"))
    modules = []
    for name, path in (("_reference_render", RENDER), ("_reference_feature_decoder", DECODER)):
        spec = importlib.util.spec_from_file_location(name, path)
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        modules.append(module)
    assert modules[1].tcnn.NetworkWithInputEncoding is tcnn.NetworkWithInputEncoding
    return modules


@needs_reference
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("unpremultiply", [False, True])
def test_decode_torch_is_the_references_op_sequence(reference, tcnn, decoder, unpremultiply, center):
    render, feature_decoder = reference
    torch.manual_seed(5)
    b, h, w = 2, 5, 7
    module = feature_decoder.FeatureDecoder(24, 128, 3, "SphericalHarmonics", 3, 3.0, "Sigmoid", unpremultiply_alpha=unpremultiply)
    rng = np.random.default_rng(9)
    pose = torch.eye(4).repeat(b, 1, 1)
    pose[:, :3, :3] = torch.from_numpy(D.random_rotations(rng, b))
    pose[:, :3, 3] = torch.randn(b, 3)
    rays = torch.cat([torch.rand(b, h, w, 2) * 1.6 - 0.8, torch.ones(b, h, w, 1)], dim=-1)
    features, alpha, go = torch.randn(b, h, w, 24) * 0.5, torch.rand(b, h, w) * 0.9 + 0.05, torch.randn(b, h, w, 3)
    alpha[0, 0, :3] = torch.tensor([0.0, float(D.ALPHA_MIN), 2.0 ** -30])
    dcfg = decoder.DecodeConfig(module.network.cfg, 3.0, unpremultiply, center)

    f1, a1 = features.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
    outputs = render.apply_feature_decoder(module, {"pred_features": f1, "pred_opacity": a1}, types.SimpleNamespace(rays_dir=rays, T_to_world=pose),
                                           training=True, center_ray_encoding=center)
    want = outputs["pred_features"]
    leaves = [f1, module.network.params] + ([a1] if unpremultiply else [])
    want_grads = torch.autograd.grad(want, leaves, go)

    f2, a2, p2 = features.clone().requires_grad_(True), alpha.clone().requires_grad_(True), module.network.params.detach().clone().requires_grad_(True)
    got = decoder.decode_torch(p2, f2.view(-1, 24), a2.view(-1), None if center else rays.view(-1, 3), pose[:, :3, :3], h * w, dcfg)
    got_grads = torch.autograd.grad(got, [f2, p2] + ([a2] if unpremultiply else []), go.view(-1, 3))
    assert got.dtype == torch.float32 and torch.equal(got.view(b, h, w, 3), want)       # the same torch operations: equal, not close
    for g, w_ in zip(got_grads, want_grads):
        assert torch.equal(g, w_)
    if unpremultiply:
        assert not got_grads[2][0, 0, 0] and not got_grads[2][0, 0, 2] and got_grads[2][0, 0, 1]   # clamp's gradient: inclusive at 1e-8f
    # and the dispatcher on CPU tensors is decode_torch
    before = dict(decoder.stats)
    with torch.no_grad():
        again = decoder.decode(p2, f2.view(-1, 24), a2.view(-1), None if center else rays.view(-1, 3), pose[:, :3, :3], h * w, dcfg)
    assert torch.equal(again, got) and decoder.stats["torch_calls"] == before["torch_calls"] + 1 and decoder.stats["hip_calls"] == before["hip_calls"]


# ---- the restatement, the host-assembled rows and decode_backward_torch --------------------------------------------------------------------------------
@pytest.mark.parametrize("sh_scale", [1.0, 2.0, 3.0])
@pytest.mark.parametrize("center", [False, True])
def test_host_assembled_rows_agree_with_the_restatement(sh_scale, center):
    """the fp32 rows of the GPU bit-equality tests are the float64 rows rounded: nothing but roundings separates the two statements"""
    for views, ppv in [(1, n) for n in D.SIZES] + [D.STRADDLE]:
        dcfg = D.DecodeConfig(R.Config(24, 3, 3, 128, 3, "sigmoid"), sh_scale, True, center)
        inputs = D.exact_inputs(views, ppv, 24, sh_scale, seed=100 + views * ppv)
        rows, a_s = D.assemble_rows_fp32(inputs, ppv, dcfg)
        want, want_a = D.rows(inputs["features"], inputs["alpha"], inputs["rays"], inputs["rot"], ppv, dcfg)
        assert np.array_equal(a_s.astype(np.float64), want_a)
        assert np.allclose(rows, want, rtol=2.0 ** -22, atol=2.0 ** -21)           # (u can cancel: its error is absolute)
        assert np.abs(np.linalg.norm(2.0 * rows[:, 24:].astype(np.float64) - 1.0, axis=1) - sh_scale).max() < 1e-6
        if views == 2:
            assert not np.array_equal(inputs["rot"][0], inputs["rot"][1])
    assert {0.0, float(D.ALPHA_MIN), 2.0 ** -30} <= set(inputs["alpha"].tolist())


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("unpremultiply", [False, True])
@pytest.mark.parametrize("activation", ["sigmoid", "none"])
def test_decode_backward_torch_agrees_with_the_restatement(tcnn, decoder, activation, unpremultiply, center):
    """In float64 both round at the same points and sum the same numbers: they agree to the rounding of the float64 sums, alpha = 0,
    1e-8f and 2^-30 included (a_s = 1e-8f for all three, the gate open only for the middle one)."""
    cfg = R.Config(24, 3, 3, 128, 3, activation)
    dcfg = D.DecodeConfig(cfg, 3.0, unpremultiply, center)
    rng = np.random.default_rng(17)
    b, ppv = 2, 45
    params = R.xavier_params(rng, cfg)
    inputs = D.exact_inputs(b, ppv, 24, 3.0, seed=3)
    inputs["rot"], inputs["rays"] = D.random_rotations(rng, b), rng.normal(size=(b * ppv, 3)).astype(np.float32)
    assert list(inputs["alpha"][:3]) == [0.0, D.ALPHA_MIN, np.float32(2.0 ** -30)]
    go = rng.normal(size=(b * ppv, 3)).astype(np.float32)
    want_f, want_a, want_p = D.backward(params, inputs["features"], inputs["alpha"], inputs["rays"], inputs["rot"], ppv, go, dcfg)
    feats, alpha, rays, rot = _torch(inputs, torch.float64)
    config = _config(decoder, tcnn, dcfg)
    got_f, got_a, got_p = decoder.decode_backward_torch(torch.from_numpy(params), feats, alpha, rays, rot, ppv, torch.from_numpy(go), config)
    assert got_f.dtype == torch.float64 and got_f.shape == (b * ppv, 24) and got_p.shape == (R.n_params(cfg),)

    def close(got, want):
        return np.abs(got.numpy() - want).max() <= 1e-9 * max(np.abs(want).max(), 1e-30)

    assert close(got_f, want_f) and close(got_p, want_p)
    if not unpremultiply:
        assert got_a is None and want_a is None
    else:
        assert close(got_a, want_a)
        assert got_a[0] == 0 and got_a[2] == 0 and got_a[1] != 0 and want_a[1] != 0           # the gate is inclusive
    # fp32 tensors: fp32 results of the same shapes
    feats, alpha, rays, rot = _torch(inputs)
    f32 = decoder.decode_backward_torch(torch.from_numpy(params), feats, alpha, rays, rot, ppv, torch.from_numpy(go), config)
    assert f32[0].dtype == torch.float32 and f32[2].dtype == torch.float32 and torch.isfinite(f32[0]).all()
    # and it is the derivative that autograd takes of decode_torch, up to the rounding of dZ to bf16 (2^-9 relative per layer)
    fg, ag, pg = feats.double().requires_grad_(True), alpha.double().requires_grad_(True), torch.from_numpy(params).double().requires_grad_(True)
    out = decoder.decode_torch(pg, fg, ag, rays.double(), rot.double(), ppv, config)
    assert out.dtype == torch.float32
    grads = torch.autograd.grad(out, [fg, pg] + ([ag] if unpremultiply else []), torch.from_numpy(go))
    scale = max(np.abs(want_p).max(), 1e-30)
    assert np.abs(grads[1].numpy() - want_p).max() <= 0.05 * scale


def test_parity_tolerances_are_measured_here(tcnn, decoder):
    """decode_torch (fp32, CPU) against the float64 restatement on the general-direction cases of the GPU test: the figures behind
    decode_reference.PARITY_TOL (shown with -s).  Another BLAS may sum in another order: 2x the constant is allowed here."""
    for name in sorted(D.GENERAL_CASES):
        dcfg, params, inputs, ppv = D.general_case(name)
        want = D.forward(params, inputs["features"], inputs["alpha"], inputs["rays"], inputs["rot"], ppv, dcfg)
        feats, alpha, rays, rot = _torch(inputs)
        with torch.no_grad():
            got = decoder.decode_torch(torch.from_numpy(params), feats, alpha, None if dcfg.center_ray else rays, rot, ppv, _config(decoder, tcnn, dcfg))
        err = float(np.abs(got.numpy() - want).max())
        print(f"\n{name}: decode_torch (fp32, CPU) vs restatement {err:.3e}  (PARITY_TOL {D.PARITY_TOL:.3e})")
        assert got.shape == want.shape and err <= 2 * D.PARITY_TOL
        assert 0.05 < want.mean() < 0.95 and want.std() > 0.01                              # not a saturated network


# ---- the hook -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def stand_ins(monkeypatch):
    """threedgrut.utils.render with a counting stand-in, threedgrut.trainer holding a copy of the name, threedgrut.utils.gui holding
    ANOTHER function under that name, and threedgrut.render not imported at all"""
    calls = []

    def original(feature_decoder, outputs, gpu_batch, training=False, center_ray_encoding=False):
        """the replaced function"""
        calls.append((training, center_ray_encoding))
        return outputs

    def other(*args, **kwargs):
        return None

    render, trainer, gui = (types.ModuleType(n) for n in ("threedgrut.utils.render", "threedgrut.trainer", "threedgrut.utils.gui"))
    render.apply_feature_decoder, trainer.apply_feature_decoder, gui.apply_feature_decoder = original, original, other
    utils, package = types.ModuleType("threedgrut.utils"), types.ModuleType("threedgrut")
    utils.render, utils.gui, package.utils, package.trainer = render, gui, utils, trainer
    package.__path__, utils.__path__ = [], []
    for name in [k for k in sys.modules if k == "threedgrut" or k.startswith("threedgrut.")]:
        monkeypatch.delitem(sys.modules, name)
    for module in (package, utils, render, trainer, gui):
        monkeypatch.setitem(sys.modules, module.__name__, module)
    return types.SimpleNamespace(render=render, trainer=trainer, gui=gui, original=original, other=other, calls=calls)


def test_the_hook_is_idempotent_and_rebinds_imported_modules_only(decoder, stand_ins):
    originals = decoder.install_fused_decoder()
    assert originals == {"apply_feature_decoder": stand_ins.original}
    hook = stand_ins.render.apply_feature_decoder
    assert hook is not stand_ins.original and hook.__doc__ == "the replaced function"
    assert stand_ins.trainer.apply_feature_decoder is hook                                  # held the original: rebound
    assert stand_ins.gui.apply_feature_decoder is stand_ins.other                           # held something else: left alone
    assert "threedgrut.render" not in sys.modules and "threedgrut.utils.viser_gui_util" not in sys.modules   # nothing was imported
    assert decoder.install_fused_decoder() is originals and stand_ins.render.apply_feature_decoder is hook


def test_the_hook_calls_the_replaced_function_when_a_precondition_fails(tcnn, decoder, stand_ins):
    decoder.install_fused_decoder()
    hook = stand_ins.render.apply_feature_decoder
    enc = {"otype": "Composite", "nested": [{"otype": "Identity", "n_dims_to_encode": 24}, {"otype": "SphericalHarmonics", "degree": 3, "n_dims_to_encode": 3}]}
    net = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "Sigmoid", "n_neurons": 128, "n_hidden_layers": 3}
    ours = types.SimpleNamespace(network=tcnn.NetworkWithInputEncoding(27, 3, enc, net), sh_scale=3.0, unpremultiply_alpha=True, ray_feature_dim=24)
    outputs = {"pred_features": torch.zeros(1, 2, 3, 24), "pred_opacity": torch.ones(1, 2, 3), "pred_dist": torch.zeros(1, 2, 3, 1)}
    batch = types.SimpleNamespace(rays_dir=torch.ones(1, 2, 3, 3), T_to_world=torch.eye(4)[None])
    before = dict(decoder.stats)
    assert hook(None, outputs, batch) is outputs                                            # no decoder
    assert hook(ours, outputs, batch, training=True, center_ray_encoding=True) is outputs    # CPU features
    foreign = types.SimpleNamespace(network=torch.nn.Linear(27, 3), sh_scale=3.0, unpremultiply_alpha=False, ray_feature_dim=24)
    assert hook(foreign, outputs, batch) is outputs                                         # not this project's network
    assert stand_ins.calls == [(False, False), (True, True), (False, False)] and decoder.stats == before
    assert sorted(outputs) == ["pred_dist", "pred_features", "pred_opacity"]
