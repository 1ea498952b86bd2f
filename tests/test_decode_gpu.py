"""GPU: the fused NHT decode stage (grut_decode_forward / grut_decode_backward: csrc/mlp.hip and csrc/mlp_backward.hip with the decode
input source) through 3dgrut_amd.decoder.

Bit equality: on inputs whose direction operations are exact or one correctly rounded operation (tests/decode_reference.py: signed
permutation poses, integer Pythagorean rays, alpha with 0, 1e-8f and 2^-30) the decode kernels must equal the EXISTING kernels run on
rows [P, F + 3] assembled on the host in numpy fp32 - any slip in the feature stride, the view of a pixel, the tail handling, the order
of the alpha product and the activation derivative, or the IEEE divisions moves bits.  grad_alpha is held against the float64 value
built from those same kernel outputs within the first-order bound of its fp32 sums.  General directions: random rotations and rays
against the float64 restatement within 4x the deviation that decode_torch (fp32, CPU) showed on the same case.  Then determinism, live
weights, centre-ray mode without rays, and the apply_feature_decoder hook."""
import ctypes
import importlib
import sys
import types

import numpy as np
import pytest
import torch

import decode_reference as D
import mlp_backward_reference as B
import mlp_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def tcnn():
    return importlib.import_module("3dgrut_amd.tcnn")


@pytest.fixture(scope="module")
def decoder():
    return importlib.import_module("3dgrut_amd.decoder")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _config(decoder, tcnn, dcfg):
    return decoder.DecodeConfig(tcnn.MlpConfig(*dcfg.mlp), dcfg.sh_scale, dcfg.unpremultiply_alpha, dcfg.center_ray)


def _tensors(inputs, n=None):
    """(features, alpha, rays, rot) on the device, the first n pixels"""
    return (_dev(inputs["features"][:n]), _dev(inputs["alpha"][:n]), _dev(inputs["rays"][:n]), _dev(inputs["rot"]))


def _exact_cases():
    """(shape, sh_scale, unpremultiply, centre ray, activation) of the bit-equality tests: every shape with both flags both ways"""
    cases = []
    for i, shape in enumerate(D.SHAPES):
        for unpremultiply in (False, True):
            cases.append((shape, (1.0, 2.0, 3.0)[i], unpremultiply, False, ("sigmoid", "none", "relu")[i]))
        cases.append((shape, 2.0, True, True, "sigmoid"))
    return cases


@pytest.mark.parametrize("shape,sh_scale,unpremultiply,center,activation", _exact_cases())
def test_decode_equals_the_existing_kernels_on_host_assembled_rows(tcnn, decoder, shape, sh_scale, unpremultiply, center, activation):
    f, degree, layers, width = shape
    cfg = R.Config(f, degree, layers, width, 3, activation)
    dcfg = D.DecodeConfig(cfg, sh_scale, unpremultiply, center)
    mlp_cfg, config = tcnn.MlpConfig(*cfg), _config(decoder, tcnn, dcfg)
    rng = np.random.default_rng(7)
    params = R.xavier_params(rng, cfg)                                               # every SH column matters
    dp = _dev(params)
    layouts = [(1, n) for n in D.SIZES] + [D.STRADDLE]
    for views, ppv in layouts:
        p = views * ppv
        inputs = D.exact_inputs(views, ppv, f, sh_scale, seed=100 + p)
        rows, a_s = D.assemble_rows_fp32(inputs, ppv, dcfg)
        go = rng.normal(size=(p, 3)).astype(np.float32)
        feats, alpha, rays, rot = _tensors(inputs)
        if center:
            rays = None                                                              # centre-ray mode never reads the rays
        # forward
        before = dict(decoder.stats)
        with torch.no_grad():
            got = decoder.decode(dp, feats, alpha, rays, rot, ppv, config)
        assert decoder.stats["hip_calls"] == before["hip_calls"] + 1 and decoder.stats["torch_calls"] == before["torch_calls"]
        y = tcnn.mlp_forward_hip(dp, _dev(rows), mlp_cfg).cpu().numpy()
        want = y if a_s is None else (y * a_s[:, None]).astype(np.float32)
        assert got.shape == (p, 3)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (views, ppv, np.argwhere(got.cpu().numpy() != want)[:4])
        # backward
        upstream = go if a_s is None else (go * a_s[:, None]).astype(np.float32)
        gx_rows, gp = tcnn.mlp_backward_hip(dp, _dev(rows), _dev(upstream), mlp_cfg)
        gx = gx_rows.cpu().numpy()[:, :f]
        want_f = gx if a_s is None else (gx / a_s[:, None]).astype(np.float32)
        gf, ga, gpar = decoder.decode_backward_hip(dp, feats, alpha, rays, rot, ppv, _dev(go), config)
        assert np.array_equal(_bits(gf.cpu().numpy()), _bits(want_f)), (views, ppv)
        assert np.array_equal(_bits(gpar.cpu().numpy()), _bits(gp.cpu().numpy())), (views, ppv)
        # each gradient alone: the others are NULL, and nothing depends on what else is asked for
        only_f, none_a, none_p = decoder.decode_backward_hip(dp, feats, alpha, rays, rot, ppv, _dev(go), config, True, False, False)
        assert none_a is None and none_p is None and torch.equal(only_f, gf)
        none_f, _, only_p = decoder.decode_backward_hip(dp, feats, alpha, rays, rot, ppv, _dev(go), config, False, False, True)
        assert none_f is None and torch.equal(only_p, gpar)
        if not unpremultiply:
            assert ga is None
            continue
        none_f, only_a, none_p = decoder.decode_backward_hip(dp, feats, alpha, rays, rot, ppv, _dev(go), config, False, True, False)
        assert none_f is None and none_p is None and torch.equal(only_a, ga)
        value, magnitude = D.grad_alpha_from(go, y, gx, rows[:, :f], inputs["alpha"], a_s)
        bound = (f + 3 + 4) * 2.0 ** -24 * magnitude
        err = np.abs(ga.cpu().numpy().astype(np.float64) - value)
        assert (err <= bound).all(), (views, ppv, float((err / np.maximum(bound, 1e-300)).max()))
        closed = inputs["alpha"] < D.ALPHA_MIN
        assert not ga.cpu().numpy()[closed].any()                                    # the closed gate: exactly zero
        if p > 3:
            assert closed.sum() >= 2 and ga.cpu().numpy()[~closed].any()             # alpha = 1e-8f itself is OPEN


def test_errors_before_a_launch(tcnn, decoder):
    abi = importlib.import_module("3dgrut_amd._abi")
    dcfg = D.DecodeConfig(D.SHIPPED, 1.0, False, False)
    config = _config(decoder, tcnn, dcfg)
    inputs = D.exact_inputs(1, 33, 24, 1.0, seed=1)
    feats, alpha, rays, rot = _tensors(inputs)
    dp, go = _dev(R.xavier_params(np.random.default_rng(1), D.SHIPPED)), torch.zeros(33, 3, device=DEV)
    with pytest.raises(RuntimeError, match="grad_alpha needs unpremultiply_alpha"):
        lib, struct = abi.load_library(), ctypes.byref(config.as_struct())
        abi.check(lib.grut_decode_backward(None, struct, dp.data_ptr(), feats.data_ptr(), alpha.data_ptr(), rays.data_ptr(), rot.data_ptr(), 1, 33,
                                           go.data_ptr(), None, None, alpha.data_ptr(), None), "grut_decode_backward")
    with pytest.raises(RuntimeError, match="all NULL"):
        abi.check(lib.grut_decode_backward(None, struct, dp.data_ptr(), feats.data_ptr(), None, rays.data_ptr(), rot.data_ptr(), 1, 33,
                                           go.data_ptr(), None, None, None, None), "grut_decode_backward")
    with pytest.raises(RuntimeError, match="only with center_ray"):
        abi.check(lib.grut_decode_forward(None, struct, dp.data_ptr(), feats.data_ptr(), None, None, rot.data_ptr(), 1, 33, go.data_ptr()),
                  "grut_decode_forward")
    unpremultiply = ctypes.byref(_config(decoder, tcnn, dcfg._replace(unpremultiply_alpha=True)).as_struct())
    with pytest.raises(RuntimeError, match="needs alpha"):
        abi.check(lib.grut_decode_forward(None, unpremultiply, dp.data_ptr(), feats.data_ptr(), None, rays.data_ptr(), rot.data_ptr(), 1, 33,
                                          go.data_ptr()), "grut_decode_forward")


@pytest.fixture(scope="module")
def general():
    """name -> (dcfg, params, inputs, pixels_per_view, float64 restatement), computed once"""
    cases = {}
    for name in D.GENERAL_CASES:
        dcfg, params, inputs, ppv = D.general_case(name)
        cases[name] = (dcfg, params, inputs, ppv, D.forward(params, inputs["features"], inputs["alpha"], inputs["rays"], inputs["rot"], ppv, dcfg))
    return cases


@pytest.mark.parametrize("name", sorted(D.GENERAL_CASES))
def test_general_directions_against_the_restatement(tcnn, decoder, general, name):
    dcfg, params, inputs, ppv, want = general[name]
    config = _config(decoder, tcnn, dcfg)
    feats, alpha, rays, rot = _tensors(inputs)
    if dcfg.center_ray:
        rays = None
    before = dict(decoder.stats)
    with torch.no_grad():
        got = decoder.decode(_dev(params), feats, alpha, rays, rot, ppv, config)
        again = decoder.decode(_dev(params), feats, alpha, rays, rot, ppv, config)
    assert decoder.stats["hip_calls"] == before["hip_calls"] + 2
    assert torch.equal(got, again)                                                   # bitwise
    err = float(np.abs(got.cpu().numpy() - want).max())
    print(f"\n{name}: fused decode vs restatement {err:.3e}; bound {4 * D.PARITY_TOL:.3e}")
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert err <= 4 * D.PARITY_TOL


def test_backward_is_deterministic_and_weights_changed_through_data_are_live(tcnn, decoder, general):
    dcfg, params, inputs, ppv, want = general["shipped_rays_unpremultiply"]
    config = _config(decoder, tcnn, dcfg)
    feats, alpha, rays, rot = _tensors(inputs)
    weights = torch.nn.Parameter(_dev(params))
    go = _dev(np.random.default_rng(3).normal(size=want.shape).astype(np.float32))
    first = decoder.decode_backward_hip(weights.detach(), feats, alpha, rays, rot, ppv, go, config)
    again = decoder.decode_backward_hip(weights.detach(), feats, alpha, rays, rot, ppv, go, config)
    assert all(torch.equal(a, b) for a, b in zip(first, again))                      # bitwise
    with torch.no_grad():
        before = decoder.decode(weights, feats, alpha, rays, rot, ppv, config)
    version = weights._version
    weights.data.copy_(weights.data * 0.5)                                           # what the decoder's EMA swap does: no version bump
    assert weights._version == version
    with torch.no_grad():
        halved = decoder.decode(weights, feats, alpha, rays, rot, ppv, config)
    expect = D.forward(params * np.float32(0.5), inputs["features"], inputs["alpha"], inputs["rays"], inputs["rot"], ppv, dcfg)
    assert float(np.abs(halved.cpu().numpy() - expect).max()) <= 4 * D.PARITY_TOL
    assert float((halved - before).abs().max()) > 100 * D.PARITY_TOL
    changed = decoder.decode_backward_hip(weights.detach(), feats, alpha, rays, rot, ppv, go, config)
    assert not torch.equal(changed[2], first[2])


# ---- the hook -------------------------------------------------------------------------------------------------------------------------------------
class _StandInDecoder:
    """what the hook reads of the reference's FeatureDecoder, and a call that states its arithmetic in torch"""

    def __init__(self, tcnn, cfg, params, sh_scale, unpremultiply):
        enc = {"otype": "Composite", "nested": [{"otype": "Identity", "n_dims_to_encode": cfg.n_features},
                                                {"otype": "SphericalHarmonics", "degree": cfg.sh_degree, "n_dims_to_encode": 3}]}
        net = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "Sigmoid", "n_neurons": cfg.width,
               "n_hidden_layers": cfg.n_hidden_layers}
        self.network = tcnn.NetworkWithInputEncoding(cfg.n_features + 3, 3, enc, net).to(DEV)
        with torch.no_grad():
            self.network.params.copy_(_dev(params))
        self.ray_feature_dim, self.sh_scale, self.unpremultiply_alpha = cfg.n_features, sh_scale, unpremultiply

    def __call__(self, features, directions, alpha=None):
        scale = alpha.clamp(min=1e-8) if self.unpremultiply_alpha else None
        rows = torch.cat([features if scale is None else features / scale, (directions * self.sh_scale + 1.0) * 0.5], dim=-1)
        rgb = self.network(rows)
        return (rgb if scale is None else rgb * scale).float()


def _stand_in_apply(feature_decoder, outputs, gpu_batch, training=False, center_ray_encoding=False):
    """the function the hook replaces, on the stand-in decoder: world rays, normalised, then the decoder on flat tensors"""
    if feature_decoder is None:
        return outputs
    features, alpha = outputs["pred_features"], outputs["pred_opacity"]
    b, h, w, n = features.shape
    rot = gpu_batch.T_to_world[:, :3, :3].to(device=gpu_batch.rays_dir.device, dtype=gpu_batch.rays_dir.dtype)
    if center_ray_encoding:
        world = rot[:, :, 2].view(b, 1, 1, 3).expand(b, h, w, 3)
    else:
        world = (rot.view(b, 1, 1, 3, 3) * gpu_batch.rays_dir.view(b, h, w, 1, 3)).sum(dim=-1)
    world = world / world.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    outputs["pred_features"] = feature_decoder(features.reshape(-1, n), world.reshape(-1, 3), alpha=alpha.reshape(-1, 1)).view(b, h, w, 3)
    return outputs


@pytest.fixture()
def hooked(monkeypatch, decoder):
    """stand-in modules threedgrut.utils.render (holding the function to replace) and threedgrut.trainer (holding a copy of the name)"""
    render, trainer = types.ModuleType("threedgrut.utils.render"), types.ModuleType("threedgrut.trainer")
    render.apply_feature_decoder = trainer.apply_feature_decoder = _stand_in_apply
    utils, package = types.ModuleType("threedgrut.utils"), types.ModuleType("threedgrut")
    utils.render, package.utils, package.trainer = render, utils, trainer
    package.__path__, utils.__path__ = [], []
    for name in [k for k in sys.modules if k == "threedgrut" or k.startswith("threedgrut.")]:
        monkeypatch.delitem(sys.modules, name)
    for name, module in (("threedgrut", package), ("threedgrut.utils", utils), ("threedgrut.utils.render", render), ("threedgrut.trainer", trainer)):
        monkeypatch.setitem(sys.modules, name, module)
    originals = decoder.install_fused_decoder()
    assert originals == {"apply_feature_decoder": _stand_in_apply}
    assert trainer.apply_feature_decoder is render.apply_feature_decoder is not _stand_in_apply
    return render.apply_feature_decoder


def _batch(inputs, opacity_shape, pose_device=DEV):
    b, h, w = D.GENERAL_SHAPE
    pose = torch.eye(4).repeat(b, 1, 1)
    pose[:, :3, :3] = torch.from_numpy(inputs["rot"])
    pose[:, :3, 3] = torch.tensor([1.0, -2.0, 0.5])
    outputs = {"pred_features": _dev(inputs["features"]).view(b, h, w, -1), "pred_opacity": _dev(inputs["alpha"]).view(*opacity_shape),
               "pred_dist": torch.zeros(b, h, w, 1, device=DEV)}
    return outputs, types.SimpleNamespace(rays_dir=_dev(inputs["rays"]).view(b, h, w, 3), T_to_world=pose.to(pose_device))


@pytest.mark.parametrize("name", sorted(D.GENERAL_CASES))
def test_the_hook_decodes_through_the_fused_stage(tcnn, decoder, hooked, general, name):
    dcfg, params, inputs, ppv, want = general[name]
    b, h, w = D.GENERAL_SHAPE
    stand_in = _StandInDecoder(tcnn, dcfg.mlp, params, dcfg.sh_scale, dcfg.unpremultiply_alpha)
    tol = 4 * D.PARITY_TOL
    for opacity_shape, pose_device in (((b, h, w), DEV), ((b, h, w, 1), "cpu")):    # a GUI batch keeps its pose on the CPU
        outputs, batch = _batch(inputs, opacity_shape, pose_device)
        with torch.no_grad():
            replaced = _stand_in_apply(stand_in, dict(outputs), batch, center_ray_encoding=dcfg.center_ray)["pred_features"]
        mine, theirs = dict(decoder.stats), dict(tcnn.stats)
        with torch.no_grad():
            result = hooked(stand_in, outputs, batch, training=False, center_ray_encoding=dcfg.center_ray)
        assert decoder.stats["hip_calls"] == mine["hip_calls"] + 1 and tcnn.stats["hip_calls"] == theirs["hip_calls"]
        assert result is outputs and sorted(result) == ["pred_dist", "pred_features", "pred_opacity"]
        got = result["pred_features"]
        assert got.shape == (b, h, w, 3) and got.dtype == torch.float32
        assert float((got - replaced).abs().max()) <= tol
        assert float(np.abs(got.cpu().numpy().reshape(-1, 3) - want).max()) <= tol


def test_the_hook_trains_with_and_without_the_fused_backward(tcnn, decoder, hooked, general):
    """The gradients of the hooked call against autograd through the replaced function.  Without the fused backward both run the same
    torch operations on the saved tensors; with it the bounds are those of the network's fused backward (4x the CPU figures of
    mlp_backward_reference.py), the feature gradient's divided by the smallest a_s (grad_features = gx / a_s) and the parameter
    gradient's unchanged (its upstream gradient is grad_out * a_s with a_s <= 1)."""
    dcfg, params, inputs, ppv, want = general["shipped_rays_unpremultiply"]
    b, h, w = D.GENERAL_SHAPE
    go = _dev(np.random.default_rng(5).normal(size=(b, h, w, 3)).astype(np.float32))
    smallest = float(inputs["alpha"].min())

    def run(fn):
        stand_in = _StandInDecoder(tcnn, dcfg.mlp, params, dcfg.sh_scale, True)
        outputs, batch = _batch(inputs, (b, h, w, 1))
        outputs["pred_features"].requires_grad_(True)
        outputs["pred_opacity"].requires_grad_(True)
        leaves = [outputs["pred_features"], outputs["pred_opacity"], stand_in.network.params]
        rgb = fn(stand_in, outputs, batch, training=True)["pred_features"]
        return rgb.detach(), torch.autograd.grad(rgb, leaves, go)

    value, (wf, wa, wp) = run(_stand_in_apply)
    previous = tcnn.install_fused_backward(False)
    try:
        for fused in (False, True):
            tcnn.install_fused_backward(fused)
            mine, theirs = dict(decoder.stats), dict(tcnn.stats)
            got, (gf, ga, gp) = run(hooked)
            assert decoder.stats["hip_calls"] == mine["hip_calls"] + 1 and decoder.stats["backward_calls"] == mine["backward_calls"] + 1
            assert decoder.stats["hip_backward_calls"] == mine["hip_backward_calls"] + int(fused)
            assert tcnn.stats["hip_calls"] == theirs["hip_calls"] and tcnn.stats["hip_backward_calls"] == theirs["hip_backward_calls"]
            assert float((got - value).abs().max()) <= 4 * D.PARITY_TOL
            assert gf.shape == wf.shape and ga.shape == wa.shape and gp.shape == wp.shape
            ef, ea, ep = (float((g - w_).abs().max()) for g, w_ in ((gf, wf), (ga, wa), (gp, wp)))
            print(f"\nfused backward {fused}: d/dfeatures {ef:.3e}, d/dalpha {ea:.3e}, d/dparams {ep:.3e}")
            assert ef <= 4 * B.BWD_GRAD_X_TOL / smallest and ep <= 4 * B.BWD_GRAD_PARAMS_TOL
            # d/dalpha sums F products gx_j x_j / a_s and 3 products go_c y_c: F feature-gradient errors times |x| / a_s, |x| <~ 4 sigma / a_s
            assert ea <= 24 * (4 * B.BWD_GRAD_X_TOL) * (4 * 0.5 / smallest) / smallest
            assert ga.abs().max() > 0 and gf.abs().max() > 0 and gp.abs().max() > 0
    finally:
        tcnn.install_fused_backward(previous)


def test_the_hook_falls_back_to_the_replaced_function(tcnn, decoder, hooked, general):
    dcfg, params, inputs, ppv, want = general["shipped_rays"]
    b, h, w = D.GENERAL_SHAPE
    stand_in = _StandInDecoder(tcnn, dcfg.mlp, params, dcfg.sh_scale, False)
    outputs, batch = _batch(inputs, (b, h, w))
    with torch.no_grad():
        fused = hooked(stand_in, dict(outputs), batch)["pred_features"]
    batch.rays_dir = batch.rays_dir.double()                                         # rays that are not fp32: the replaced function runs,
    mine, theirs = dict(decoder.stats), dict(tcnn.stats)                             # and the network's own dispatcher is called by it
    with torch.no_grad():
        result = hooked(stand_in, outputs, batch)
    assert decoder.stats == mine
    assert tcnn.stats["hip_calls"] + tcnn.stats["torch_calls"] == theirs["hip_calls"] + theirs["torch_calls"] + 1
    assert float((result["pred_features"] - fused).abs().max()) <= 4 * D.PARITY_TOL
    assert hooked(None, outputs, batch) is outputs
    # every precondition, one at a time: the arguments of decode() are refused and the replaced function would run
    outputs, batch = _batch(inputs, (b, h, w))

    def refused(decoder_object=stand_in, **changed):
        o = {**outputs, **{k: v for k, v in changed.items() if k in outputs}}
        g = types.SimpleNamespace(rays_dir=changed.get("rays_dir", batch.rays_dir), T_to_world=changed.get("T_to_world", batch.T_to_world))
        return decoder._hook_inputs(decoder_object, o, g, False) is None

    assert not refused()
    foreign = types.SimpleNamespace(network=torch.nn.Linear(27, 3).to(DEV), sh_scale=3.0, unpremultiply_alpha=False, ray_feature_dim=24)
    assert refused(foreign)                                                          # not this project's network
    assert refused(pred_features=outputs["pred_features"].half())                   # not fp32
    assert refused(pred_features=outputs["pred_features"].cpu())                    # not on the device
    assert refused(pred_features=outputs["pred_features"][..., :23])                # not ray_feature_dim wide
    assert refused(rays_dir=batch.rays_dir.cpu()) and refused(rays_dir=batch.rays_dir.half())
    assert refused(rays_dir=batch.rays_dir.clone().requires_grad_(True))
    assert refused(T_to_world=batch.T_to_world.clone().requires_grad_(True))
