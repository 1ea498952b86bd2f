"""GPU: the split-SH path of 3DGUT (render.split_sh_features; gut_forward_split / gut_backward_split / gut_backward_unpacked_split).
The model's features_albedo [N,3] and features_specular [N,45] are read where they lie and their gradients written as two contiguous
tensors; only addresses differ from the [N,48] path, so every result must equal that path's bit for bit."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import split_sh_util as u

pytestmark = pytest.mark.gpu
abi, gt = u.abi, u.gt
syn = importlib.import_module("workloads.synthetic")
scenes = importlib.import_module("workloads.scenes")
BAD_INPUT, NOT_READY, UNSUPPORTED = -1, -3, -4


@pytest.fixture(scope="module")
def nat():
    return u.native()


@pytest.mark.parametrize("n", u.SIZES)
def test_split_entry_points_equal_their_twins(nat, n):
    """gut_forward + gut_backward_unpacked on cat(albedo, specular) against the split pair, n_active_features 0..3: the four outputs,
    the four geometry gradients and the SH gradient ([:, :3] / [:, 3:]) bit for bit; NaN guard rows untouched, no NaN left inside;
    a second split call gives equal bits."""
    for n_active in range(4):
        vis = u.check_c_level(nat, n, n_active)
    if n >= 16:   # scene guard: the sizes that matter contain particles with and without tiles
        assert bool((vis != 0).any()) and bool((vis == 0).any())
    if n == 1:
        assert bool((vis != 0).all())


@pytest.mark.parametrize("n", (17, 129, 1000))
@pytest.mark.parametrize("packed,depth", [(True, False), (False, True), (True, True)])
def test_split_packed_and_depth_variants(nat, n, packed, depth):
    """gut_backward_split against gut_backward, and both pairs with a depth gradient (grad_hit_distance non-NULL: the 20-float slots)."""
    for n_active in (0, 2, 3):
        u.check_c_level(nat, n, n_active, packed=packed, depth=depth)


def test_split_gradients_are_not_trivial(nat):
    sc = u.make_split_scene(1000)
    frame = u.frame_of(nat, sc)
    out = nat.trace_split(frame, sc["d12"], sc["albedo"], sc["specular"], sc["ro"], sc["rd"])
    _, _, _, _, g_alb, g_spec = nat.trace_bwd_unpacked_split(frame, sc["d12"], sc["albedo"], sc["specular"], sc["ro"], sc["rd"], out[0],
                                                             sc["g_feat"], sc["g_opa"], out[1], None)
    vis = out[3].view(torch.int32).reshape(-1)
    assert int((vis != 0).sum()) > 100 and int((vis == 0).sum()) > 100
    assert int((g_alb != 0).any(dim=1).sum()) > 50 and int((g_spec[:, 24:] != 0).any(dim=1).sum()) > 50


def test_forward_of_one_kind_backward_of_the_other(nat):
    sc = u.make_split_scene(257)
    frame = u.frame_of(nat, sc)
    out = nat.trace_split(frame, sc["d12"], sc["albedo"], sc["specular"], sc["ro"], sc["rd"])
    geo_a, gs = u.backward_twin(nat, frame, sc, out[0], out[1], packed=False, depth=False)
    out2 = nat.trace(frame, sc["d12"], sc["sph"], sc["ro"], sc["rd"])
    (g_alb, _), (g_spec, _) = u.guarded(257, 3), u.guarded(257, 45)
    rc, geo_b = u.backward_split(nat, frame, sc, out2[0], out2[1], g_alb, g_spec, packed=False, depth=False)
    assert rc == abi.GRUT_OK
    assert torch.equal(g_alb, gs[:, :3]) and torch.equal(g_spec, gs[:, 3:])
    assert all(torch.equal(a, b) for a, b in zip(geo_a, geo_b))


def test_split_two_kernel_finalisation_in_a_fresh_process():
    """GRUT_GUT_UNFUSED_FINALIZE=1 (read by the library once per process) selects gut_project_bwd_kernel's split address maps: the child
    runs the comparison of every size against the twins in that mode."""
    tests = os.path.dirname(os.path.abspath(__file__))
    assert not os.environ.get("GRUT_GUT_UNFUSED_FINALIZE")
    r = subprocess.run([sys.executable, os.path.join(tests, "split_sh_child.py")], env=dict(os.environ, GRUT_GUT_UNFUSED_FINALIZE="1"), timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "split unfused ok" in r.stdout


def _last_error(nat):
    return (nat.lib.grut_last_error() or b"").decode()


@pytest.mark.parametrize("render,reason", [
    (dict(particle_radiance_sph_degree=2), "sph_degree"),
    (dict(particle_feature_half=True), "particle_feature_half"),
    (dict(splat=dict(k_buffer_size=4)), "k_buffer_size"),
    ("nht", "neural harmonic"),
])
def test_unsupported_configurations_are_refused_before_any_launch(render, reason):
    if render == "nht":
        model = {"feature_type": "nht", "nht_features": {"dim": 48, "activation": {"type": "sincos", "num_frequencies": 1}, "interpolation_type": "barycentric"}}
        bad = gt._GutNative(gt.gut_config_from_conf({"render": {"splat": {}}, "model": model}))
    else:
        bad = u.native(**render)
    sc = u.make_split_scene(17)
    frame = u.frame_of(bad, sc)
    outs = [torch.full(s, 7.0, device="cuda") for s in ((u.H, u.W, 4), (u.H, u.W, 1), (u.H, u.W, 1))]
    vis = torch.full((17, 1), 7, dtype=torch.int32, device="cuda")
    rc = bad.lib.gut_forward_split(bad.handle, u._stream(), C.byref(frame), u._p(sc["d12"]), u._p(sc["albedo"]), u._p(sc["specular"]), u._p(sc["ro"]),
                                   u._p(sc["rd"]), u._p(outs[0]), u._p(outs[1]), u._p(outs[2]), u._p(vis))
    assert rc == UNSUPPORTED and reason in _last_error(bad), _last_error(bad)
    (g_alb, alb_buf), (g_spec, spec_buf) = u.guarded(17, 3), u.guarded(17, 45)
    for packed in (True, False):
        rc, _ = u.backward_split(bad, frame, sc, outs[0], outs[1], g_alb, g_spec, packed=packed, depth=False)
        assert rc == UNSUPPORTED and reason in _last_error(bad), _last_error(bad)
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs + [vis]) and bool(torch.isnan(alb_buf).all()) and bool(torch.isnan(spec_buf).all())


def test_null_pointers_and_missing_forward_are_errors(nat):
    sc = u.make_split_scene(65)
    fresh = u.native()
    frame = u.frame_of(fresh, sc)
    (g_alb, alb_buf), (g_spec, spec_buf) = u.guarded(65, 3), u.guarded(65, 45)
    fd, dist = torch.zeros((u.H, u.W, 4), device="cuda"), torch.zeros((u.H, u.W, 1), device="cuda")
    for packed in (True, False):   # no forward on this handle yet
        rc, _ = u.backward_split(fresh, frame, sc, fd, dist, g_alb, g_spec, packed=packed, depth=False)
        assert rc == NOT_READY, _last_error(fresh)
    outs = [torch.full(s, 7.0, device="cuda") for s in ((u.H, u.W, 4), (u.H, u.W, 1), (u.H, u.W, 1))]
    vis = torch.full((65, 1), 7, dtype=torch.int32, device="cuda")
    for albedo, specular in ((None, sc["specular"]), (sc["albedo"], None)):
        rc = fresh.lib.gut_forward_split(fresh.handle, u._stream(), C.byref(frame), u._p(sc["d12"]), u._p(albedo), u._p(specular), u._p(sc["ro"]),
                                         u._p(sc["rd"]), u._p(outs[0]), u._p(outs[1]), u._p(outs[2]), u._p(vis))
        assert rc == BAD_INPUT, _last_error(fresh)
    # a misaligned base (one float into the row) is refused as well: the header's alignment rule
    rc = fresh.lib.gut_forward_split(fresh.handle, u._stream(), C.byref(frame), u._p(sc["d12"]), u._p(sc["albedo"]), C.c_void_p(sc["specular"].data_ptr() + 4),
                                     u._p(sc["ro"]), u._p(sc["rd"]), u._p(outs[0]), u._p(outs[1]), u._p(outs[2]), u._p(vis))
    assert rc == BAD_INPUT and "aligned" in _last_error(fresh)
    out = fresh.trace_split(frame, sc["d12"], sc["albedo"], sc["specular"], sc["ro"], sc["rd"])
    for packed in (True, False):
        for k in range(4):
            args = dict(albedo=sc["albedo"], specular=sc["specular"])
            grads = [g_alb, g_spec]
            if k < 2:
                args[("albedo", "specular")[k]] = None
            else:
                grads[k - 2] = None
            rc, _ = u.backward_split(fresh, frame, sc, out[0], out[1], grads[0], grads[1], packed=packed, depth=False, **args)
            assert rc == BAD_INPUT, (packed, k, _last_error(fresh))
    torch.cuda.synchronize()
    assert bool(torch.isnan(alb_buf).all()) and bool(torch.isnan(spec_buf).all()) and bool((vis == 7).all())
    # the refusals left the forward context alone: the backward still runs
    rc, _ = u.backward_split(fresh, frame, sc, out[0], out[1], g_alb, g_spec, packed=False, depth=False)
    assert rc == abi.GRUT_OK


# ---- Python level -------------------------------------------------------------------------------------------------------------

class CountingGaussians(syn.ActivatedGaussians):
    """The reference model's surface: two SH leaves and get_features() = torch.cat (model.py:94-96), counting its calls."""

    feature_calls = 0

    def get_features(self):
        self.feature_calls += 1
        return super().get_features()


def _tracer(split, **render):
    splat = render.pop("splat", {})
    return gt.Tracer({"render": dict(render, splat=splat, split_sh_features=split)})


def _step(tracer, model, sc, train=True):
    batch = scenes.torch_batch(sc["scene"]["batch"], "cuda")
    out = tracer.render(model, batch, train=train, frame_id=3)
    if train:
        torch.autograd.backward([out["pred_features"], out["pred_opacity"]], [sc["g_feat"][None], sc["g_opa"][None]])
    torch.cuda.synchronize()
    return out


def _assert_same_outputs(a, b):
    for k in ("pred_features", "pred_opacity", "pred_dist", "hits_count", "mog_visibility"):
        assert torch.equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def cat_reference():
    """The switch off: outputs and the six .grad tensors of the cat path, per (fused activations, n_active)."""
    cache = {}

    def get(fused, n_active=3):
        if (fused, n_active) not in cache:
            sc = u.make_split_scene(1000)
            model = CountingGaussians(sc["d12"].cpu().numpy(), sc["sph"].cpu().numpy(), n_active_features=n_active)
            tr = _tracer(False, fused_activations=fused)
            out = _step(tr, model, sc)
            assert tr.stats_split == {"split_calls": 0, "cat_calls": 1} and model.feature_calls == 1
            cache[(fused, n_active)] = (out, [p.grad.clone() for p in model.parameters()])
        return cache[(fused, n_active)]
    return get


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n_active", [3, 1])
def test_plugin_switch_on_equals_switch_off(cat_reference, fused, n_active):
    ref_out, ref_grads = cat_reference(fused, n_active)
    sc = u.make_split_scene(1000)
    model = CountingGaussians(sc["d12"].cpu().numpy(), sc["sph"].cpu().numpy(), n_active_features=n_active)
    tr = _tracer(True, fused_activations=fused)
    out = _step(tr, model, sc)
    assert model.feature_calls == 0 and tr.stats_split == {"split_calls": 1, "cat_calls": 0}
    _assert_same_outputs(out, ref_out)
    for p, want in zip(model.parameters(), ref_grads):
        assert p.grad is not None and p.grad.is_contiguous() and torch.equal(p.grad, want)


def test_split_switch_from_the_environment(monkeypatch, cat_reference):
    monkeypatch.setenv("GRUT_SPLIT_SH", "1")
    sc = u.make_split_scene(1000)
    model = CountingGaussians(sc["d12"].cpu().numpy(), sc["sph"].cpu().numpy())
    tr = gt.Tracer({"render": {"splat": {}}})
    out = _step(tr, model, sc)
    assert model.feature_calls == 0 and tr.stats_split["split_calls"] == 1
    _assert_same_outputs(out, cat_reference(False)[0])


@pytest.mark.parametrize("case", ["simple_gaussians", "non_contiguous_specular", "k_buffer", "gradient_exchange"])
def test_fallback_cases_take_the_cat_path(cat_reference, case):
    sc = u.make_split_scene(1000)
    d12, sph = sc["d12"].cpu().numpy(), sc["sph"].cpu().numpy()
    if case == "simple_gaussians":   # no such attributes
        model, ref = syn.SimpleGaussians(d12, sph), syn.SimpleGaussians(d12, sph)
        out, ref_out = _step(_tr := _tracer(True), model, sc), _step(_tracer(False), ref, sc)
        _assert_same_outputs(out, ref_out)
        assert all(torch.equal(a.grad, b.grad) for a, b in zip(model.parameters(), ref.parameters()))
        assert _tr.stats_split == {"split_calls": 0, "cat_calls": 1}
    elif case == "non_contiguous_specular":
        model = CountingGaussians(d12, sph)
        base = torch.zeros((1000, 46), device="cuda")
        base[:, :45] = model.features_specular.detach()
        base.requires_grad_(True)
        model.features_specular = base[:, :45]
        assert not model.features_specular.is_contiguous()
        tr = _tracer(True)
        out = _step(tr, model, sc)
        ref_out, ref_grads = cat_reference(False)
        _assert_same_outputs(out, ref_out)
        assert tr.stats_split == {"split_calls": 0, "cat_calls": 1} and model.feature_calls == 1
        assert torch.equal(base.grad[:, :45], ref_grads[5]) and torch.equal(model.features_albedo.grad, ref_grads[4])
    elif case == "k_buffer":
        model, ref = CountingGaussians(d12, sph), CountingGaussians(d12, sph)
        tr = _tracer(True, splat=dict(k_buffer_size=4))
        out, ref_out = _step(tr, model, sc), _step(_tracer(False, splat=dict(k_buffer_size=4)), ref, sc)
        _assert_same_outputs(out, ref_out)
        assert tr.stats_split == {"split_calls": 0, "cat_calls": 1} and model.feature_calls == 1
        # (the sorted mode accumulates per-hit float atomics in an order that differs from run to run, also between two runs of the
        # same path: a sum of up to W x H = 3072 terms carries at most 3072 x 2^-24 = 1.8e-4 of its largest possible magnitude as
        # ordering noise, so the two runs are compared to 2e-4 of each tensor's largest gradient instead of bit for bit)
        for a, b in zip(model.parameters(), ref.parameters()):
            assert float((a.grad - b.grad).abs().max()) <= 2e-4 * float(b.grad.abs().max())
    else:   # a set gradient_exchange: the decision alone (a stub, forward only - no process group here)
        model = CountingGaussians(d12, sph)
        tr = _tracer(True)
        tr.gradient_exchange = object()
        with torch.no_grad():
            out = _step(tr, model, sc, train=False)
        _assert_same_outputs(out, cat_reference(False)[0])
        assert tr.stats_split == {"split_calls": 0, "cat_calls": 1} and model.feature_calls == 1
