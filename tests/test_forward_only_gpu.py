"""GPU: forward-only frames of 3DGUT (gut_forward_only / gut_forward_only_split / gut_memory; render.forward_only_inference).
A forward-only frame runs the sweeps' builds without checkpoint stores, writes no boundary tiles, clears no reached marks and owns no
checkpoint tables; everything it returns must equal the training forward's bit for bit (the arithmetic is the same source), every
gut_backward* after it is refused, and training frames before and after it on the same handle differentiate as on a fresh one.

The scene is the smallest that crosses what the mode removes: 1500 translucent Gaussians (density 0.03 .. 0.07) in a blob a few pixels
wide on a 48 x 40 image (3 x 3 tiles, last row and column partial), so that the centre tile's list runs over hundreds of entries with
rays alive to its end - checkpoints are written every 64 entries of a list (every 256 in the neural-harmonic sweep) while rays live.
Every comparison first asserts that list length and a live ray from the frame's own tile ranges and opacity."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import camera_scenes

pytestmark = pytest.mark.gpu
abi = importlib.import_module("3dgrut_amd._abi")
gt = importlib.import_module("3dgrut_amd.gut_tracer")
syn = importlib.import_module("workloads.synthetic")
scenes = importlib.import_module("workloads.scenes")

N, W, H = 1500, 48, 40
TILES = ((W + 15) // 16) * ((H + 15) // 16)
NHT_MODEL = {"feature_type": "nht", "nht_features": {"dim": 48, "activation": {"type": "sincos", "num_frequencies": 1}, "interpolation_type": "barycentric"}}
MIN_TRANSMITTANCE = 1e-4   # the plugin's default (render.min_transmittance)


def _cloud(n=N, seed=17):
    rng = np.random.default_rng(seed)
    pos = rng.normal(0.0, 0.25, (n, 3)).astype(np.float32)
    scale = np.exp(rng.normal(np.log(0.04), 0.4, (n, 3))).astype(np.float32)
    rot = rng.normal(0.0, 1.0, (n, 4)).astype(np.float32)
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    dens = rng.uniform(0.03, 0.07, (n, 1)).astype(np.float32)
    sph = rng.normal(0.0, 0.3, (n, 48)).astype(np.float32)
    feats = rng.uniform(-np.pi / 2, np.pi / 2, (n, 48)).astype(np.float32)
    return syn.pack_density(pos, dens, rot, scale), sph, feats


_cache = {}


def scene_of(kind="pinhole", n=N):
    """Camera, rays and the blob on the device: `pinhole` (global shutter), `fisheye` (tests/camera_scenes.py: rolling right-to-left,
    rotating sensor), `behind` (pinhole, every particle mirrored behind the camera), `origins` (pinhole with a ray origin per pixel:
    the sweeps' copies without a shared origin)."""
    if (kind, n) not in _cache:
        if kind == "fisheye":
            s = camera_scenes.make_camera_path_scene("fisheye_r2l_rot", n=8, w=W, h=H)
        else:
            s = scenes.make_scene(n=8, width=W, height=H)
        d12, sph, feats = _cloud()
        d12, sph, feats = d12[:n].copy(), sph[:n], feats[:n]
        if kind == "behind":
            eye = np.asarray(s["batch"]["T_to_world"][0], np.float32)[:3, 3]
            d12[:, :3] = 2.0 * eye - d12[:, :3]
        ro, rd = np.array(s["rays"][0][0]), np.array(s["rays"][1][0])
        if kind == "origins":
            ro = ro + (1e-3 * np.arange(H * W, dtype=np.float32).reshape(H, W, 1) / (H * W)) * np.ones(3, np.float32)
        rng = np.random.default_rng(5)
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
        _cache[(kind, n)] = dict(
            n=n, scene=s, d12=t(d12), sph=t(sph), sph0=t(sph[:, :3]), albedo=t(sph[:, :3]), specular=t(sph[:, 3:]), feats=t(feats),
            ro=t(ro.astype(np.float32)), rd=t(rd), c2w=t(np.asarray(s["batch"]["T_to_world"][0], np.float32)),
            g_feat=t(rng.normal(size=(H, W, 3)).astype(np.float32)), g_opa=t(rng.normal(size=(H, W, 1)).astype(np.float32)))
    return _cache[(kind, n)]


def native(model=None, **render):
    splat = render.pop("splat", {})
    conf = {"render": dict(render, splat=splat)}
    if model is not None:
        conf["model"] = model
    return gt._GutNative(gt.gut_config_from_conf(conf))


def frame_of(nat, sc, n_active=3, frame_id=7, device_poses=False):
    s = sc["scene"]
    f = nat.make_frame(frame_id, n_active, sc["n"], H, W, s["cam"], s["pose_start"], s["pose_end"])
    if device_poses:   # the library derives the sensor poses from the camera-to-world matrix on the GPU
        f.device_T_to_world = sc["c2w"].data_ptr()
    return f


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def c_forward(nat, frame, sc, sph, only):
    """gut_forward* / gut_forward_only* into poisoned buffers (NaN, -1 for the visibility): -> dict of the six outputs.  `sph`: one
    tensor, or the (albedo, specular) pair of the split entry points."""
    nht = bool(nat.cfg.feature_transform_type)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    out = dict(fd=nan(H, W, nat.ray_feature_dim + 1), dist=nan(H, W, 1), cnt=nan(H, W, 1),
               vis=torch.full((sc["n"],), -1, dtype=torch.int32, device="cuda"))
    if not nht:
        out.update(feat=nan(H, W, 3), opa=nan(H, W, 1))
        frame.out_features, frame.out_opacity = out["feat"].data_ptr(), out["opa"].data_ptr()
    sph = sph if isinstance(sph, tuple) else (sph,)
    name = ("gut_forward_only" if only else "gut_forward") + ("_split" if len(sph) == 2 else "")
    rc = getattr(nat.lib, name)(nat.handle, _stream(), C.byref(frame), _p(sc["d12"]), *map(_p, sph), _p(sc["ro"]), _p(sc["rd"]),
                                _p(out["fd"]), _p(out["dist"]), _p(out["cnt"]), _p(out["vis"]))
    frame.out_features, frame.out_opacity = None, None
    assert rc == abi.GRUT_OK, (name, rc, nat.lib.grut_last_error())
    torch.cuda.synchronize()
    return out


def tile_lists(nat):
    """Lengths of the last frame's tile lists, from gut_debug_fetch's tile ranges."""
    ranges = torch.zeros((TILES, 2), dtype=torch.int32, device="cuda")
    rc = nat.lib.gut_debug_fetch(nat.handle, _stream(), None, None, None, None, None, None, None, _p(ranges))
    assert rc == abi.GRUT_OK, nat.lib.grut_last_error()
    torch.cuda.synchronize()
    return (ranges[:, 1] - ranges[:, 0]).cpu().numpy()


def assert_crosses_boundaries(nat, out, longer_than):
    """The frame reaches what the mode removes: a tile list longer than two checkpoint intervals (any run of 2 k + 1 consecutive
    sorted entries contains two multiples of k) and, in that tile, a ray still alive behind the last entry (so alive at both)."""
    lengths = tile_lists(nat)
    st = nat.stats()
    assert int(st.num_intersections) == int(lengths.sum()) and int(st.num_tiles) == TILES
    t = int(lengths.argmax())
    print(f"longest tile list: tile {t}, {int(lengths[t])} entries of {int(lengths.sum())}")
    assert lengths[t] > longer_than, lengths
    gx = (W + 15) // 16
    y0, x0 = (t // gx) * 16, (t % gx) * 16
    opacity = out["fd"][y0:y0 + 16, x0:x0 + 16, -1]
    hits = out["cnt"][y0:y0 + 16, x0:x0 + 16, 0]
    alive = (1.0 - opacity > 10 * MIN_TRANSMITTANCE) & (hits > 0)
    print(f"pixels of that tile alive behind the list: {int(alive.sum())}, most hits {float(hits.max())}")
    assert bool(alive.any())


def assert_equal_outputs(a, b):
    for k in a:
        assert not bool(torch.isnan(a[k].float()).any()) and not bool((a["vis"] == -1).any()), f"{k}: an element was left unwritten"
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


# ---- outputs equal the training forward's -----------------------------------------------------------------------------------------

SH_CASES = {
    # name: (scene, native kwargs, sph key, n_active, device poses, list length the frame must exceed)
    "sh3_pinhole_device_poses": ("pinhole", {}, "sph", 3, True, 128),
    "sh0_pinhole": ("pinhole", dict(particle_radiance_sph_degree=0), "sph0", 0, False, 128),
    "sh3_fisheye_rolling": ("fisheye", {}, "sph", 3, False, 128),
    "sh3_ray_origin_per_pixel": ("origins", {}, "sph", 3, False, 128),
    "sh3_split": ("pinhole", {}, ("albedo", "specular"), 3, False, 128),
    "sh3_no_hitcounts": ("pinhole", dict(enable_hitcounts=False), "sph", 3, False, 128),
}


@pytest.mark.parametrize("quarter", ["0", "1"])
@pytest.mark.parametrize("case", list(SH_CASES))
def test_sh_outputs_equal_the_training_forward(monkeypatch, case, quarter):
    """Both sweep kernels (GRUT_FWD_QUARTER=0: half tiles, =1: quarter tiles), each in its build without checkpoint stores."""
    monkeypatch.setenv("GRUT_FWD_QUARTER", quarter)
    kind, kw, key, n_active, device_poses, longer_than = SH_CASES[case]
    sc = scene_of(kind)
    sph = tuple(sc[k] for k in key) if isinstance(key, tuple) else sc[key]
    train, only = native(**kw), native(**kw)
    ref = c_forward(train, frame_of(train, sc, n_active, device_poses=device_poses), sc, sph, only=False)
    if not kw.get("enable_hitcounts", True):   # the hit count is untouched then: judge liveness by the opacity alone
        ref["cnt"].fill_(1.0)
    assert_crosses_boundaries(train, ref, longer_than)
    out = c_forward(only, frame_of(only, sc, n_active, device_poses=device_poses), sc, sph, only=True)
    if not kw.get("enable_hitcounts", True):
        out["cnt"].fill_(1.0)
    assert_equal_outputs(out, ref)
    assert float(ref["fd"][..., 3].max()) > 0.5 and int((ref["vis"] != 0).sum()) > N // 2
    # the frame's statistics and binning products are the twin's as well
    a, b = train.stats(), only.stats()
    assert (a.num_particles, a.num_visible, a.num_intersections, a.num_tiles, a.key_bits) == (b.num_particles, b.num_visible, b.num_intersections, b.num_tiles, b.key_bits)
    assert np.array_equal(tile_lists(train), tile_lists(only))
    # same handle: a forward-only frame on the handle that just trained, a training frame on the handle that never did
    again = c_forward(train, frame_of(train, sc, n_active, device_poses=device_poses), sc, sph, only=True)
    back = c_forward(only, frame_of(only, sc, n_active, device_poses=device_poses), sc, sph, only=False)
    for o in (again, back):
        if not kw.get("enable_hitcounts", True):
            o["cnt"].fill_(1.0)
        assert_equal_outputs(o, ref)


def test_k_buffer_outputs_equal_the_training_forward():
    """k_buffer_size = 4: the sorted forward has no checkpoints, the frame only drops the tables around it."""
    sc = scene_of("pinhole")
    train, only = native(splat=dict(k_buffer_size=4)), native(splat=dict(k_buffer_size=4))
    ref = c_forward(train, frame_of(train, sc), sc, sc["sph"], only=False)
    assert_crosses_boundaries(train, ref, 128)
    assert_equal_outputs(c_forward(only, frame_of(only, sc), sc, sc["sph"], only=True), ref)
    assert only.memory()[2] == 0


@pytest.mark.parametrize("generic", [False, True])
def test_nht_outputs_equal_the_training_forward(monkeypatch, generic):
    """The neural-harmonic fast path (checkpoints every 256 entries, a table of its own) in its build without them; and the generic
    feature forward (GRUT_NHT_GENERIC: no checkpoints), which only takes the state flag."""
    if generic:
        monkeypatch.setenv("GRUT_NHT_GENERIC", "1")
    sc = scene_of("pinhole")
    train, only = native(model=NHT_MODEL), native(model=NHT_MODEL)
    ref = c_forward(train, frame_of(train, sc, n_active=0), sc, sc["feats"], only=False)
    assert_crosses_boundaries(train, ref, 512)
    out = c_forward(only, frame_of(only, sc, n_active=0), sc, sc["feats"], only=True)
    assert_equal_outputs(out, ref)
    assert float(ref["fd"][..., :24].abs().max()) > 0.3
    assert only.memory()[2] == 0 and (train.memory()[2] > 0 or generic)


# ---- edge frames ---------------------------------------------------------------------------------------------------------------

def test_no_particles_and_no_intersections_keep_the_initial_values(monkeypatch):
    monkeypatch.setenv("GRUT_POISON_OUTPUTS", "1")
    nat = native()
    # I == 0: every particle behind the camera
    sc = scene_of("behind")
    ref = nat.trace(frame_of(nat, sc), sc["d12"], sc["sph"], sc["ro"], sc["rd"])
    assert int(nat.stats().num_intersections) == 0
    out = nat.trace_forward_only(frame_of(nat, sc), sc["d12"], sc["sph"], sc["ro"], sc["rd"])
    assert int(nat.stats().num_intersections) == 0 and int(nat.stats().num_particles) == N
    torch.cuda.synchronize()
    for a, b in zip(out, ref):
        assert torch.equal(a, b) and not bool(torch.isnan(a).any())
    fd, dist, cnt, vis, feat, opa = out
    assert not bool(fd.any()) and bool((dist == 1e6).all()) and not bool(cnt.any()) and not bool(vis.view(torch.int32).any())
    assert not bool(feat.any()) and not bool(opa.any())
    # N == 0: nothing is launched
    empty = dict(sc, n=0, d12=sc["d12"][:0], sph=sc["sph"][:0])
    ref = nat.trace(frame_of(nat, empty), empty["d12"], empty["sph"], sc["ro"], sc["rd"])
    out = nat.trace_forward_only(frame_of(nat, empty), empty["d12"], empty["sph"], sc["ro"], sc["rd"])
    for a, b in zip(out, ref):
        assert a.shape == b.shape and torch.equal(a, b)
    assert not bool(out[0].any()) and bool((out[1] == 1e6).all())
    assert nat.memory()[2] == 0


# ---- state ---------------------------------------------------------------------------------------------------------------------

def _train_and_differentiate(nat, sc, frame_id=7):
    frame = frame_of(nat, sc, frame_id=frame_id)
    fd, dist, *_ = nat.trace(frame, sc["d12"], sc["sph"], sc["ro"], sc["rd"])
    grads = nat.trace_bwd_unpacked(frame, sc["d12"], sc["sph"], sc["ro"], sc["rd"], fd, sc["g_feat"], sc["g_opa"], dist, None)
    torch.cuda.synchronize()
    return fd, grads


def _forward_only(nat, sc, frame_id=8):
    out = nat.trace_forward_only(frame_of(nat, sc, frame_id=frame_id), sc["d12"], sc["sph"], sc["ro"], sc["rd"])
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def fresh_handle_gradients():
    sc = scene_of("pinhole")
    nat = native()
    fd, grads = _train_and_differentiate(nat, sc)
    assert all(bool(g.any()) and not bool(torch.isnan(g).any()) for g in grads)
    return fd, grads, int(nat.stats().num_intersections)


def test_every_backward_after_a_forward_only_frame_is_refused():
    sc = scene_of("pinhole")
    nat = native()
    frame = frame_of(nat, sc)
    fd, dist, *_ = nat.trace_forward_only(frame, sc["d12"], sc["sph"], sc["ro"], sc["rd"])
    g_fd = torch.cat([sc["g_feat"], sc["g_opa"]], dim=-1)
    common = (frame, sc["d12"], sc["sph"], sc["ro"], sc["rd"], fd)
    split = (frame, sc["d12"], sc["albedo"], sc["specular"], sc["ro"], sc["rd"], fd)
    variants = {
        "gut_backward": lambda: nat.trace_bwd(*common, g_fd, dist, None),
        "gut_backward_unpacked": lambda: nat.trace_bwd_unpacked(*common, sc["g_feat"], sc["g_opa"], dist, None),
        "gut_backward_split": lambda: nat.trace_bwd_split(*split, g_fd, dist, None),
        "gut_backward_unpacked_split": lambda: nat.trace_bwd_unpacked_split(*split, sc["g_feat"], sc["g_opa"], dist, None),
        "gut_backward_factored": lambda: nat.trace_bwd_factored(*common, g_fd, dist, None),
        "gut_backward_factored_chunked": lambda: nat.trace_bwd_factored_chunked(*common, g_fd, dist, None, 2, lambda *a: pytest.fail("a chunk was launched")),
    }
    for name, call in variants.items():
        with pytest.raises(RuntimeError, match="forward-only") as e:
            call()
        assert f"{name} failed" in str(e.value), str(e.value)
    # a forward-only frame with no particles marks the handle just the same
    empty = dict(sc, n=0, d12=sc["d12"][:0], sph=sc["sph"][:0])
    f0 = frame_of(nat, empty)
    out = nat.trace_forward_only(f0, empty["d12"], empty["sph"], sc["ro"], sc["rd"])
    with pytest.raises(RuntimeError, match="forward-only"):
        nat.trace_bwd(f0, empty["d12"], empty["sph"], sc["ro"], sc["rd"], out[0], g_fd, out[1], None)


SMALL = 200   # a frame whose lists are a fraction of the blob's: the scratch it sizes is too short for the frame after it

ORDERS = {
    "forward_only_then_train": ("only",),
    "train_then_forward_only_then_train": ("train", "only"),
    "small_forward_only_then_forward_only_then_train": ("small_only", "only"),
    "small_train_then_forward_only_then_train": ("small_train", "only"),   # lists grown by the forward-only frame, tables still short
    "forward_only_trim_train": ("only", "trim"),
    "train_trim_forward_only_then_train": ("train", "trim", "only"),
    "train_then_forward_only_trim_forward_only": ("train", "only", "trim", "only"),
}


@pytest.mark.parametrize("order", list(ORDERS))
def test_training_frame_after_forward_only_frames_differentiates_as_on_a_fresh_handle(fresh_handle_gradients, order):
    ref_fd, ref_grads, entries = fresh_handle_gradients
    sc, small = scene_of("pinhole"), scene_of("pinhole", SMALL)
    nat = native()
    for step in ORDERS[order]:
        if step == "trim":
            nat.trim()
            assert nat.memory() == (0, 0, 0)
        elif step == "train":
            fd, grads = _train_and_differentiate(nat, sc, frame_id=3)
            assert all(torch.equal(a, b) for a, b in zip(grads, ref_grads))
        elif step in ("small_train", "small_only"):
            if step == "small_train":
                _train_and_differentiate(nat, small, frame_id=3)
            else:
                _forward_only(nat, small)
            # (a frame leaves head-room of half its entries: the blob's frame must need more than that)
            assert 0 < int(nat.stats().num_intersections) * 2 < entries
        else:
            out = _forward_only(nat, sc)
            assert torch.equal(out[0], ref_fd)
    fd, grads = _train_and_differentiate(nat, sc)
    assert torch.equal(fd, ref_fd)
    for name, a, b in zip(("positions", "density", "rotation", "scale", "sph"), grads, ref_grads):
        assert torch.equal(a, b), (order, name)


# ---- memory --------------------------------------------------------------------------------------------------------------------

def test_checkpoint_tables_exist_only_after_a_training_frame():
    sc = scene_of("pinhole")
    only, train = native(), native()
    assert only.memory() == (0, 0, 0)
    for _ in range(2):
        _forward_only(only, sc)
        total, lists, ck = only.memory()
        assert ck == 0 and lists > 0 and total > lists
    _train_and_differentiate(train, sc)
    t_total, t_lists, t_ck = train.memory()
    entries = int(train.stats().num_intersections)
    assert t_lists == lists and t_lists >= 20 * entries        # the same lists in both modes: 20 B per entry (and the head-room)
    assert t_ck >= 80 * entries                                # the tables: 80 B per entry and more
    # (the backward's own slots are part of the total but of neither part)
    assert t_total > total + t_ck
    # its first training frame gives the forward-only handle the tables, sized like the training handle's
    _train_and_differentiate(only, sc)
    assert only.memory()[1:] == (t_lists, t_ck)
    only.trim()
    assert only.memory() == (0, 0, 0)


# ---- plugin --------------------------------------------------------------------------------------------------------------------

def _tracer(switch, model=None, **render):
    conf = {"render": dict(render, splat={}, forward_only_inference=switch)}
    if model is not None:
        conf["model"] = model
    return gt.Tracer(conf)


def _same_dict(a, b):
    for k in ("pred_features", "pred_opacity", "pred_dist", "pred_normals", "hits_count", "mog_visibility"):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("split,fused", [(False, False), (True, False), (False, True), (True, True)])
def test_plugin_switch_on_equals_switch_off(monkeypatch, split, fused):
    monkeypatch.setenv("GRUT_POISON_OUTPUTS", "1")
    sc = scene_of("pinhole")
    batch = scenes.torch_batch(sc["scene"]["batch"], "cuda")
    d12, sph = sc["d12"].cpu().numpy(), sc["sph"].cpu().numpy()
    on, off = _tracer(True, split_sh_features=split, fused_activations=fused), _tracer(False, split_sh_features=split, fused_activations=fused)
    model, ref_model = syn.ActivatedGaussians(d12, sph), syn.ActivatedGaussians(d12, sph)
    # under no_grad: the forward-only entry point, tensors equal to the switch-off call's, whatever `train` says
    with torch.no_grad():
        out, ref = on.render(model, batch, train=True, frame_id=3), off.render(ref_model, batch, train=True, frame_id=3)
    torch.cuda.synchronize()
    _same_dict(out, ref)
    assert on.stats_forward_only == {"forward_only_calls": 1, "training_calls": 0}
    assert off.stats_forward_only == {"forward_only_calls": 0, "training_calls": 1}
    assert on.stats_split == off.stats_split == {"split_calls": int(split), "cat_calls": int(not split)}
    assert on.tracer_wrapper.memory()[2] == 0 and off.tracer_wrapper.memory()[2] > 0
    assert float(out["pred_opacity"].max()) > 0.5
    # grad mode on, leaves require grad: today's path on the same handle, gradients equal to the switch-off ones
    out, ref = on.render(model, batch, train=True, frame_id=4), off.render(ref_model, batch, train=True, frame_id=4)
    for o in (out, ref):
        torch.autograd.backward([o["pred_features"], o["pred_opacity"]], [sc["g_feat"][None], sc["g_opa"][None]])
    torch.cuda.synchronize()
    _same_dict(out, ref)
    assert on.stats_forward_only == {"forward_only_calls": 1, "training_calls": 1}
    for p, q in zip(model.parameters(), ref_model.parameters()):
        assert p.grad is not None and bool(p.grad.any()) and torch.equal(p.grad, q.grad)
    # grad mode on, nothing requires grad: forward-only again, and a backward through its outputs has nothing to reach
    frozen = syn.SimpleGaussians(d12, sph, requires_grad=False)
    out = on.render(frozen, batch, frame_id=5)
    assert on.stats_forward_only == {"forward_only_calls": 2, "training_calls": 1} and not out["pred_features"].requires_grad


def test_plugin_nht_forward_only_equals_the_training_forward():
    sc = scene_of("pinhole")
    batch = scenes.torch_batch(sc["scene"]["batch"], "cuda")
    g = syn.SimpleGaussians(sc["d12"].cpu().numpy(), sc["feats"].cpu().numpy(), requires_grad=False)
    on, off = _tracer(True, model=NHT_MODEL), _tracer(False, model=NHT_MODEL)
    with torch.no_grad():
        out, ref = on.render(g, batch), off.render(g, batch)
    torch.cuda.synchronize()
    _same_dict(out, ref)
    assert tuple(out["pred_features"].shape) == (1, H, W, 24) and float(out["pred_features"].abs().max()) > 0.3
    assert on.stats_forward_only["forward_only_calls"] == 1 and on.tracer_wrapper.memory()[2] == 0 and off.tracer_wrapper.memory()[2] > 0
