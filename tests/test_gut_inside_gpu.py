"""GPU parity of the HIP 3DGUT path on frames rendered from INSIDE the cloud (tests/inside_scenes.py): half of the particles behind
the sensor, a near population on both sides of the near plane, big particles whose sigma points fall behind the sensor plane, whose
boxes cover the whole tile grid and which contain the ray origins; a fisheye of 170 degrees; a rolling shutter whose pose rotates.

Checks and tolerances are those of tests/test_gut_gpu.py (image 1e-4, gradients 1e-3 trimmed / 1e-2 untrimmed against the nearer of
the float32 and float64 oracles); on top of them the gradient metric is applied PER POPULATION (near rows, far rows, each normalised
by its own ||ref||inf): the near field's gradients are 30 to 1000 times the far field's, so the per-tensor metric alone would let a
wrong far-field gradient pass.  tests/test_gut_inside_cpu.py shows that the reference alone (float32 against float64 oracle) stays
within a quarter of every bound used here.

Measured on an MI355X (bounds in brackets; flips = pixels whose hit count differs from the float32 / float64 oracle):

| test                                 | max image error | pixels beyond 1e-4 | flips f32 / f64 | trimmed gradient error near / far [1e-3] |
|--------------------------------------|-----------------|--------------------|-----------------|------------------------------------------|
| frames[pinhole] (depth gradient)     | 1.5e-4          | 1 [12.3]           | 2 / 1 [12.3]    | 3.1e-6 / 6.6e-6                          |
| frames[pinhole_big]                  | 9.5e-7          | 0 [12.3]           | 1 / 1 [12.3]    | 1.9e-6 / not judged                      |
| frames[fisheye_big]                  | 7.2e-7          | 0 [30.7]           | 0 / 0 [12.3]    | 1.1e-6 / 3.4e-6                          |
| frames[pinhole_rs_big] (depth grad.) | 8.3e-7          | 0 [30.7]           | 0 / 1 [12.3]    | 2.1e-6 / not judged                      |
| frames[pinhole_208]                  | 5.3e-4          | 1 [59.9]           | 1 / 5 [59.9]    | 1.2e-6 / 3.1e-7                          |
| sorted hit buffer k16                | within 1e-4     | 0 [12.3]           | 1 / 1           | 1.2e-4 / not judged                      |
| sorted hit buffer k4                 | within 1e-4     | 0 [12.3]           | 0 / 0           | 2.2e-6 / not judged                      |
| nht                                  | 5.1e-4          | 1 (a flip) [6.1]   | 2 [12.3]        | 3.9e-6 (all rows), 8.1e-7 (features)     |

Tile counts: 0 of 5200 (pinhole_208) and 0 of 3600 (pinhole_big) differ from the oracle's, so the lists are compared tile by tile.

What a wrong kernel would trip (the first two were also built and run: every test of this file that renders a frame failed):
* near plane at 0.25 instead of 0.2 - the visible near particles with 0.2 <= view_z < 0.25 lose their tiles:
  test_inside_projection_and_binning_are_exact (98 of 5200 / 40 of 3600 tile counts differ, cap 5.2 / 3.6), then
  test_inside_frames_match_oracle (every pixel: they are the nearest hits).  Of the orbit frames' tests only the 700-particle golden
  of test_projection_and_binning_match_reference_code_golden notices.
* invalid sigma points dropped from the covariance - centre, conic and extent of every particle with a sigma point outside the image
  margin or behind the sensor plane change: test_inside_projection_and_binning_are_exact (448 of 5200 / 217 of 3600 tile counts),
  test_inside_frames_match_oracle (97 % of the pixels).
* the one-step walk record's width field read without its kind check - a box of 9 to 13 tiles across, counted by the cooperative walk
  (kind 0, width - 1 truncated to 3 bits, empty mask), would be expanded as a narrower one-step box whose mask is empty: its entries
  become padding.  test_inside_projection_and_binning_are_exact[pinhole_208] (100 boxes wider than 8 tiles: multiplicity != tile count,
  lists != the oracle's) and test_inside_frames_match_oracle[pinhole_208] (image)."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import oracle
import inside_util as U
from scenes import make_scene
from test_gut_gpu import NHT_MODEL, _check_grads, _image_checks, _tracer, _trimmed_rel_err, torch_batch_rs

pytestmark = pytest.mark.gpu
syn = importlib.import_module("workloads.synthetic")

FLIP_FRAC = {"fisheye_big": 5e-3, "pinhole_rs_big": 5e-3}   # as test_camera_models_and_rolling_shutter_match_oracle; 2e-3 elsewhere
FAR_JUDGED = ("pinhole", "pinhole_208", "fisheye_big")       # behind 48 big particles 2 or 3 far rows receive any gradient at all


def _render(scene, g_fd=None, g_dist=None, tracer=None, **render_kw):
    """test_gut_gpu._run_gpu with the batch of a moving sensor (T_to_world_end) and, optionally, a tracer that has rendered before."""
    import torch
    tr = tracer if tracer is not None else _tracer(**render_kw)
    g = syn.SimpleGaussians(scene["density12"], scene["sph"])
    out = tr.render(g, torch_batch_rs(scene["batch"], "cuda"), train=True)
    res = dict(out=out, tracer=tr, gaussians=g)
    if g_fd is not None:
        fd = torch.cat([out["pred_features"], out["pred_opacity"]], dim=-1)[0]
        loss = (fd * torch.as_tensor(g_fd, device="cuda")).sum()
        if g_dist is not None:
            loss = loss + (out["pred_dist"][0] * torch.as_tensor(g_dist, device="cuda")).sum()
        loss.backward()
        res["grads"] = g.grads_packed()
    torch.cuda.synchronize()
    return res


@functools.lru_cache(maxsize=None)
def _frame(name):
    """The HIP frame of scene `name`, forward and backward, rendered once (its tracer renders nothing else: gut_debug_fetch reads it)."""
    g_fd, g_dist = U.upstream(name)
    return _render(U.scene(name), g_fd, g_dist if U.DEPTH_GRAD.get(name, False) else None, k_buffer_size=U.k_of(name))


@pytest.fixture(scope="module", autouse=True)
def _release_frames():
    """The cached frames (tracers, their scratch from torch's allocator, outputs, gradients) live as long as this module's tests: the
    rest of the session, and the interpreter's exit, see no tracer of this file."""
    yield
    import gc
    import torch
    _frame.cache_clear()
    gc.collect()
    torch.cuda.synchronize()


def _oracles(name):
    o32, o64 = U.oracle_frame(name, np.float32), U.oracle_frame(name, np.float64)
    return o32, o64


def _population_check(name, gpu, populations):
    """The trimmed 1e-3 check per population, against the nearer of the two oracles; returns the figures."""
    s = U.scene(name)
    cnt = gpu["out"]["hits_count"][0, ..., 0].detach().cpu().numpy()
    refs = []
    for o in _oracles(name):
        n_flip = int((cnt != o["fwd"]["hit_count"][..., 0]).sum())
        refs.append((o["grads"][0], o["grads"][1], 3 * n_flip))
    masks = {"near": s["near"], "far": ~s["near"]}
    figures = {pop: U.population_errors(gpu["grads"], refs, masks[pop]) for pop in ("near", "far")}
    print(f"{name}: per-population trimmed gradient error " + ", ".join(f"{p} {max(e.values()):.2e}" for p, e in figures.items())
          + f" (bound 1e-3; judged: {', '.join(populations)})")
    for pop in populations:
        for k, e in figures[pop].items():
            assert e < 1e-3, f"{name}: {pop} population, grad {k}: rel err {e:.3e}"
    return figures


@pytest.mark.parametrize("name", ["pinhole", "pinhole_big", "fisheye_big", "pinhole_rs_big", "pinhole_208"])
def test_inside_frames_match_oracle(name):
    """(a) forward and backward against the oracle with the tolerances of test_gut_gpu.py, (b) the gradient metric per population."""
    s = U.scene(name)
    g_fd, g_dist = U.upstream(name)
    gpu = _frame(name)
    o32, o64 = _oracles(name)
    fwd = o32["fwd"]
    out = gpu["out"]
    fd = np.concatenate([out["pred_features"][0].detach().cpu().numpy(), out["pred_opacity"][0].detach().cpu().numpy()], -1)
    bad = U.image_bad_pixels(fd, out["pred_dist"][0].detach().cpu().numpy(), fwd)
    cnt = out["hits_count"][0, ..., 0].detach().cpu().numpy()
    flips = [int((cnt != o["fwd"]["hit_count"][..., 0]).sum()) for o in (o32, o64)]
    print(f"{name}: max image error {np.abs(fd - fwd['feat_density']).max():.2e}, {int(bad.sum())} of {bad.size} pixels beyond 1e-4 "
          f"(cap {FLIP_FRAC.get(name, 2e-3) * bad.size:.1f}), hit-count flips vs f32 / f64 oracle {flips[0]} / {flips[1]} "
          f"(cap {max(2, 2e-3 * bad.size):.1f})")
    _image_checks(out, fwd, max_flip_frac=FLIP_FRAC.get(name, 2e-3))
    st = gpu["tracer"].tracer_wrapper.stats()
    I_ref = fwd["bins"]["num_intersections"]
    assert abs(int(st.num_intersections) - I_ref) <= max(2, 1e-3 * I_ref)
    vis = out["mog_visibility"].detach().view(-1).bool().cpu().numpy()
    assert (vis != (fwd["visibility"] != 0)).mean() < 1e-3
    assert (cnt != fwd["hit_count"][..., 0]).mean() < 5e-3
    # nothing in front of the near plane is visible, everything just behind it that the oracle sees is
    vz = U.view_z64(s)
    assert not vis[vz < 0.2].any()
    _check_grads(s, gpu, o32, g_fd, g_dist)
    _population_check(name, gpu, ("near", "far") if name in FAR_JUDGED else ("near",))


def _fetch(gpu, n):
    import torch
    nat = gpu["tracer"].tracer_wrapper
    st = nat.stats()
    I, tiles = int(st.num_intersections), int(st.num_tiles)
    tc = torch.zeros(n, dtype=torch.int32, device="cuda")
    pp, ex = torch.zeros((n, 2), device="cuda"), torch.zeros((n, 2), device="cuda")
    depth = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    sidx = torch.zeros(max(I, 1), dtype=torch.int32, device="cuda")
    rng = torch.zeros((tiles, 2), dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert nat.lib.gut_debug_fetch(nat.handle, stream, p(tc), p(pp), None, p(ex), p(depth), None, p(sidx), p(rng)) == 0
    torch.cuda.synchronize()
    return dict(I=I, tiles=tiles, tc=tc.cpu().numpy().view(np.uint32), depth=depth.cpu().numpy(), proj_pos=pp.cpu().numpy(), extent=ex.cpu().numpy(),
                sidx=sidx.cpu().numpy().view(np.uint32)[:I], rng=rng.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("name", ["pinhole_208", "pinhole_big"])
def test_inside_projection_and_binning_are_exact(name):
    """(c) the integer and bit-exact stage through gut_debug_fetch: tile counts, the near-plane cull, depth bits, ranges, order, lists."""
    s = U.scene(name)
    n = len(s["density12"])
    gx, gy = (s["W"] + 15) // 16, (s["H"] + 15) // 16
    got = _fetch(_frame(name), n)
    fwd = U.oracle_frame(name, np.float32)["fwd"]
    proj, bins = fwd["proj"], fwd["bins"]
    tc, I = got["tc"], got["I"]
    differ = tc != proj["tiles_count"]
    print(f"{name}: {int(differ.sum())} of {n} tile counts differ from the oracle's (cap {max(2, 1e-3 * n):.1f}); I = {I}")
    assert differ.sum() <= max(2, 1e-3 * n)
    # the near-plane cull, no exemption: no tiles, not visible, no depth, in no list
    cut = U.view_z64(s) < 0.2
    vis = _frame(name)["out"]["mog_visibility"].detach().view(-1).cpu().numpy() != 0
    assert cut.sum() >= 1000 and not tc[cut].any() and not vis[cut].any()
    assert np.all(got["depth"][cut] == 0.0) and not np.isin(got["sidx"], np.flatnonzero(cut)).any()
    # depth keys: bit for bit the oracle's float32 depth
    both = (tc > 0) & (proj["tiles_count"] > 0)
    assert both.sum() > 500 and np.array_equal(got["depth"][both].view(np.uint32), proj["depth"][both].view(np.uint32))
    assert np.all(got["depth"][tc == 0] == 0.0)
    # ranges tile [0, I)
    rng = got["rng"]
    assert tc.sum() == I
    lens = (rng[:, 1] - rng[:, 0]).astype(np.int64)
    nz = lens > 0
    assert lens.sum() == I
    starts = rng[nz, 0]
    assert starts[0] == 0 and np.all(starts[1:] == rng[nz, 1][:-1])
    # strict (depth bits, index) order inside each tile; multiplicity = tile count
    sidx = got["sidx"]
    keys = (got["depth"].view(np.uint32).astype(np.uint64)[sidx] << np.uint64(32)) | sidx.astype(np.uint64)
    for t in np.flatnonzero(nz):
        k = keys[rng[t, 0]:rng[t, 1]]
        assert np.all(k[1:] > k[:-1]), f"tile {t} not strictly ordered by (depth, index)"
    assert np.array_equal(np.bincount(sidx, minlength=n).astype(np.uint32), tc)
    # the geometry this file is about
    assert (tc == gx * gy).any(), "no box covers the whole tile grid"
    bw, _ = U.tile_boxes(s, dict(proj_pos=got["proj_pos"], extent=got["extent"], tiles_count=tc))
    if s["W"] == 208:
        assert (bw > 8).any(), "no box wider than 8 tiles"
    if not differ.any():   # identical counts: the lists are the oracle's, tile by tile
        assert I == bins["num_intersections"]
        ref_tile = (bins["sorted_keys"] >> np.uint64(32)).astype(np.int64)
        o_start = np.searchsorted(ref_tile, np.arange(got["tiles"]), side="left")
        o_end = np.searchsorted(ref_tile, np.arange(got["tiles"]), side="right")
        for t in range(got["tiles"]):
            assert np.array_equal(sidx[rng[t, 0]:rng[t, 1]] if nz[t] else sidx[:0], bins["sorted_idx"][o_start[t]:o_end[t]]), f"tile {t}: different list"


@pytest.mark.parametrize("name", ["k16", "k4"])
def test_inside_sorted_hit_buffer_matches_oracle(name):
    """(d) the sorted hit buffer (K = 16, K = 4) with ray origins inside particles, as test_sorted_kbuffer_mode_matches_oracle."""
    s = U.scene(name)
    K = U.k_of(name)
    gpu = _frame(name)
    o32, o64 = _oracles(name)
    _image_checks(gpu["out"], o32["fwd"])
    cfg0 = oracle.default_gut_config()
    unsorted = oracle.gut_forward(cfg0, s["cam"], s["pose_start"], s["pose_end"], 3, s["density12"], s["sph"], *s["rays"])
    assert np.abs(unsorted["feat_density"] - o32["fwd"]["feat_density"]).max() > 1e-3   # the sorted image really differs
    gd, gsph = gpu["grads"]
    cnt = gpu["out"]["hits_count"][0, ..., 0].detach().cpu().numpy()
    flips = [int((cnt != o["fwd"]["hit_count"][..., 0]).sum()) for o in (o32, o64)]
    drop = 3 * max(flips)
    (rd, rsph, _), g64 = o32["grads"], o64["grads"]
    errs = {k: min(_trimmed_rel_err(gd[:, sl], rd[:, sl], drop), _trimmed_rel_err(gd[:, sl], g64[0][:, sl], drop)) for k, sl in U.TENSORS.items()}
    errs["sph"] = min(_trimmed_rel_err(gsph, rsph, drop), _trimmed_rel_err(gsph, g64[1], drop))
    print(f"{name}: K = {K}, flips {flips}, trimmed gradient errors {errs}")
    for k, e in errs.items():
        assert e < 1e-3, f"K={K}: grad {k} rel err {e:.3e}"
    _population_check(name, gpu, ("near",))


def test_inside_nht_matches_oracle():
    """(e) neural harmonic features (K = 0, default feature model) on the pinhole frame without big particles: forward under the rule of
    test_nht_forward_matches_oracle, backward under that of test_nht_backward_matches_oracle_on_a_larger_frame."""
    import torch
    s = U.scene("pinhole")
    feats, g_fd = U.nht_inputs("pinhole")
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    tr = gt.Tracer({"render": {"splat": {}}, "model": NHT_MODEL})
    gs = syn.SimpleGaussians(s["density12"], feats)
    out = tr.render(gs, torch_batch_rs(s["batch"], "cuda"), train=True)
    t = torch.as_tensor(g_fd, device="cuda")
    ((out["pred_features"][0] * t[..., :24]).sum() + (out["pred_opacity"][0] * t[..., 24:]).sum()).backward()
    gd, gf = gs.grads_packed()
    ora = U.oracle_nht_frame("pinhole", np.float32)
    fwd, (rd, rf) = ora["fwd"], ora["grads"]
    got = np.concatenate([out["pred_features"][0].detach().cpu().numpy(), out["pred_opacity"][0].detach().cpu().numpy()], -1)
    flips = (out["hits_count"][0].detach().cpu().numpy() != fwd["hit_count"])[..., 0]
    bad = (np.abs(got - fwd["feat_density"]) > 1e-4).any(-1)
    n_flip = int(flips.sum())
    errs = {k: _trimmed_rel_err(gd[:, sl], rd[:, sl], 3 * n_flip) for k, sl in U.TENSORS.items()}
    errs["features"] = _trimmed_rel_err(gf, rf, 3 * n_flip)
    print(f"nht inside: {int(bad.sum())} pixels beyond 1e-4, {n_flip} flips, max image error {np.abs(got - fwd['feat_density']).max():.2e}, gradients {errs}")
    assert flips.mean() <= 2e-3 and (bad & ~flips).mean() <= 1e-3, f"{bad.sum()} pixels beyond tolerance, {flips.sum()} flips"
    assert np.abs(got[..., :24]).max() > 0.3
    for k, e in errs.items():
        assert e < 1e-3, (k, e)


def _outside():
    return make_scene(n=3000, width=96, height=64, median_scale=0.06)


def test_one_tracer_outside_inside_outside_equals_fresh_tracers():
    """(g) one Tracer renders and differentiates an orbit frame, the inside frame with big particles, then the orbit frame again: each
    result is bit-identical to a fresh tracer's (no stale one-step walk records, touch masks or segment boundaries when the shape of
    the tile lists changes abruptly)."""
    import torch
    inside, outside = U.scene("pinhole_big"), _outside()
    g_fd, _ = U.upstream("pinhole_big")     # both frames are 96x64
    tr = _tracer()
    keys = ("pred_features", "pred_opacity", "pred_dist", "hits_count", "mog_visibility")
    stats = []
    for k, sc in enumerate((outside, inside, outside)):
        got = _render(sc, g_fd, None, tracer=tr)
        stats.append(int(tr.tracer_wrapper.stats().num_intersections))
        got_out = {key: got["out"][key].detach().clone() for key in keys}
        fresh = _render(sc, g_fd, None)
        for key in keys:
            assert torch.equal(got_out[key], fresh["out"][key]), f"frame {k}: {key} differs from a fresh tracer's"
        assert np.array_equal(got["grads"][0], fresh["grads"][0]) and np.array_equal(got["grads"][1], fresh["grads"][1]), f"frame {k}: gradients"
        assert float(np.abs(got["grads"][0]).max()) > 0
    assert stats[0] == stats[2] and stats[1] != stats[0]


def test_inside_gradients_are_bitwise_reproducible():
    """(h) two runs of the inside frame with big particles give bit-equal gradients - in it some rows sum contributions from every tile
    of the frame."""
    name = "pinhole_big"
    s = U.scene(name)
    g_fd, _ = U.upstream(name)
    a = _frame(name)["grads"]
    b = _render(s, g_fd, None)["grads"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    full = U.oracle_frame(name, np.float32)["fwd"]["proj"]["tiles_count"] == 24
    assert full.sum() >= 5 and (np.abs(a[0][full]).max(1) > 0).sum() >= 5
