"""The gradient sweep's slot marks (GutGradSlots: one 64-bit word per particle for its first 32 tile entries, one byte per slot beyond)
and their zero invariant: nothing clears them ahead of a backward, the finalisation leaves them zero.

* particles whose tile counts sit on both sides of every boundary of the scheme (1, 32 | 33 tiles: quad path | wave-wide path;
  64, 65, 192: word + bytes) against the oracle, tensor by tensor and row by row;
* no mark survives a backward, a forward without backward, or a change of the particle count;
* run-to-run and path-to-path bit equality of the gradients; the feature (NHT) sweep, the second writer of the marks.
"""
import functools
import importlib

import numpy as np
import pytest

import oracle
from scenes import make_scene, torch_batch
from test_gut_gpu import NHT_MODEL, _image_checks, _run_gpu, _run_oracle, _tracer, _trimmed_rel_err

pytestmark = pytest.mark.gpu
syn = importlib.import_module("workloads.synthetic")

W, H = 256, 192                                                          # 16 x 12 tiles
# tile boxes {x0, y0, width, height} of the hand-placed particles: 1, 32, 33, 64, 65 and 192 tiles
BOXES = [(1, 1, 1, 1), (3, 2, 8, 4), (2, 7, 11, 3), (6, 2, 8, 8), (1, 5, 13, 5), (0, 0, 16, 12)]
COUNTS = [w * h for _, _, w, h in BOXES]
N_BACK = 1500


def _quat_wxyz(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def _front_rows(scene, shrink=1.0):
    """One flat particle per box of BOXES, facing the camera at depths 1.5 .. 1.75 in front of the cloud (which starts at ~3), its axes along the
    image's, density 0.06 (the rays behind stay alive); the two in-plane scales are solved on the CPU projection so that the projected
    rectangle ends 4 pixels inside the box's outer tiles.  Without tile culling the tile count is the box area."""
    cfg = oracle.default_gut_config(tile_based_culling=False)
    c2w = np.asarray(scene["batch"]["T_to_world"][0], np.float64)
    fx, fy, cx, cy = scene["batch"]["intrinsics"]
    q = _quat_wxyz(c2w[:3, :3])
    sph = np.zeros((1, 48), np.float32)
    rows = []
    for k, (x0, y0, tw, th) in enumerate(BOXES):
        u, v, z = x0 * 16 + tw * 8, y0 * 16 + th * 8, 1.5 + 0.05 * k   # (distinct depths: their order must not hang on a rounding)
        want = (200.0, 150.0) if tw * th == 192 else (tw * 8 - 4.0 if tw > 1 else 5.0, th * 8 - 4.0 if th > 1 else 5.0)
        row = np.zeros(12, np.float32)
        row[0:3] = c2w[:3, :3] @ np.array([(u - cx) / fx * z, (v - cy) / fy * z, z]) + c2w[:3, 3]
        row[3], row[4:8], row[8:11] = 0.06, q, (0.01, 0.01, 0.02)
        for _ in range(30):
            ext = oracle.gut_project(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], 3, row[None], sph)["extent"][0]
            row[8] *= want[0] / ext[0]
            row[9] *= want[1] / ext[1]
        row[8:10] *= shrink
        rows.append(row)
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def _boundary_scene(shrink=1.0, n_back=N_BACK, seed=3):
    scene = make_scene(n=n_back, width=W, height=H, median_scale=0.05, seed=seed)
    front = _front_rows(scene, shrink)
    sph = np.random.default_rng(17).normal(0.0, 0.3, (len(front), 48)).astype(np.float32)
    sph[:, :3] = 0.8
    return dict(scene, density12=np.concatenate([front, scene["density12"]]), sph=np.concatenate([sph, scene["sph"]]))


def _upstream(with_depth):
    g_fd, g_dist = syn.upstream_grads(W, H)
    g_fd *= W * H
    if with_depth:
        g_dist = (np.random.default_rng(5).normal(size=g_dist.shape) * 0.1).astype(np.float32)
    return g_fd, g_dist


@functools.lru_cache(maxsize=None)
def _references(culling, with_depth):
    """The f32 and the f64 oracle of the boundary scene (computed once per configuration, never modified).  The scene is only usable if
    the two oracles themselves stay inside the hit-count-flip cap of test_gut_gpu._check_grads."""
    scene = _boundary_scene()
    g_fd, g_dist = _upstream(with_depth)
    kw = dict(tile_based_culling=culling)
    ora = _run_oracle(scene, g_fd, g_dist, **kw)
    cfg = ora["cfg"]
    f64 = oracle.gut_forward(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], 3, scene["density12"], scene["sph"], *scene["rays"],
                             dtype=np.float64)
    g64 = oracle.gut_backward(cfg, scene["cam"], 3, f64, g_fd, g_dist, dtype=np.float64)
    flips = int((ora["fwd"]["hit_count"][..., 0] != f64["hit_count"][..., 0]).sum())
    assert flips <= max(2, 2e-3 * W * H), f"the oracles disagree on {flips} hit counts: the scene sits on a threshold"
    if not culling:
        assert list(ora["fwd"]["proj"]["tiles_count"][:len(BOXES)]) == COUNTS
    return ora, f64, g64


@pytest.mark.parametrize("with_depth", [False, True])
@pytest.mark.parametrize("culling", [False, True])
def test_boundary_tile_counts_match_oracle(culling, with_depth):
    """Tile counts 1, 32, 33, 64, 65, 192: the last count of the quad path and the first of the wave-wide path; the last slot of the
    particle's word and the first slot with a byte; both slot strides (16, and 20 with a depth gradient).

    Rows of the hand-placed particles: a missed or doubled slot of a 60-tile particle moves its row by more than a percent."""
    scene = _boundary_scene()
    g_fd, g_dist = _upstream(with_depth)
    ora, f64, g64 = _references(culling, with_depth)
    gpu = _run_gpu(scene, g_fd, g_dist if with_depth else None, tile_based_culling=culling)
    _image_checks(gpu["out"], ora["fwd"])
    gd, gsph = gpu["grads"]
    cnt = gpu["out"]["hits_count"][0, ..., 0].detach().cpu().numpy()
    refs = []
    for fwd, (rd, rsph, _) in ((ora["fwd"], ora["grads"]), (f64, g64)):     # test_gut_gpu._check_grads: the f32 OR the f64 oracle, flip exemptions
        n_flip = int((cnt != fwd["hit_count"][..., 0]).sum())
        assert n_flip <= max(2, 2e-3 * cnt.size), f"{n_flip} pixels with a different hit count"
        refs.append((rd, rsph, 3 * n_flip))
    for k, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
        e = min(_trimmed_rel_err(gd[:, sl], rd[:, sl], drop) for rd, _, drop in refs)
        print(f"culling={culling} depth={with_depth} grad {k}: rel err {e:.3e}")
        assert e < 1e-3, f"grad {k}: rel err {e:.3e}"
    e = min(_trimmed_rel_err(gsph, rsph, drop) for _, rsph, drop in refs)
    print(f"culling={culling} depth={with_depth} grad sph: rel err {e:.3e}")
    assert e < 1e-3
    if not culling:
        tc = ora["fwd"]["proj"]["tiles_count"]
        assert int(gpu["tracer"].tracer_wrapper.stats().num_intersections) == int(tc.sum())
    for i, count in enumerate(COUNTS):
        for name, got, which in (("geometry", gd[i, :11], 0), ("sph", gsph[i], 1)):
            e = min(np.abs(got.astype(np.float64) - r[which][i, :got.shape[0]]).max() / np.abs(r[which][i, :got.shape[0]]).max() for r in refs)
            print(f"culling={culling} depth={with_depth} particle of {count} tiles, {name} row: rel err {e:.3e}")
            assert e < 1e-3, f"particle of {count} tiles, {name} row: rel err {e:.3e}"


def _step(tr, scene, backward=True):
    """One training step of `scene` on the tracer `tr`; the packed gradients (None without a backward)."""
    import torch
    g_fd, _ = syn.upstream_grads(scene["W"], scene["H"])
    g = syn.SimpleGaussians(scene["density12"], scene["sph"])
    out = tr.render(g, torch_batch(scene["batch"], "cuda"), train=True)
    grads = None
    if backward:
        fd = torch.cat([out["pred_features"], out["pred_opacity"]], dim=-1)[0]
        (fd * torch.as_tensor(g_fd * scene["W"] * scene["H"], device="cuda")).sum().backward()
        grads = g.grads_packed()
    torch.cuda.synchronize()
    return grads


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_no_mark_survives_into_the_next_backward():
    """One tracer, scenes A and B of the same size: the particles that cover 32 .. 192 tiles in A are a hundredth of that in B, so every
    mark that A's backward (or nothing at all, after a forward without backward) left behind would add a stale slot to B's sums."""
    a, b = _boundary_scene(), _boundary_scene(shrink=0.01)
    fresh = _step(_tracer(), b)
    assert np.abs(fresh[0]).max() > 0
    tr = _tracer()
    ga = _step(tr, a)
    assert _same(_step(tr, b), fresh), "after a backward of the scene with the large particles"
    assert _same(_step(tr, a), ga), "... and back"
    _step(tr, a, backward=False)
    assert _same(_step(tr, b), fresh), "after a forward without backward"
    # the particle count grows, then shrinks (the per-particle scratch is reallocated, then reused with head room)
    big, small = _boundary_scene(n_back=4000, seed=4), _boundary_scene(shrink=0.01, n_back=700, seed=5)
    fresh_big, fresh_small = _step(_tracer(), big), _step(_tracer(), small)
    assert _same(_step(tr, big), fresh_big), "after the particle count grew"
    assert _same(_step(tr, small), fresh_small), "after the particle count shrank"
    assert _same(_step(tr, b), fresh)
    tr.tracer_wrapper.trim()
    assert _same(_step(tr, a), ga), "after gut_trim"


def test_backward_paths_agree_bit_for_bit():
    """Two backwards of fresh forwards; the packed, unpacked, factored and chunked-factored (2 and 4 ranges) backwards of one forward:
    every finalisation cleans up after itself, so the next one on the same handle sees the marks of its own sweep only."""
    import torch
    scene = _boundary_scene()
    g_fd, _ = _upstream(False)
    assert _same(_run_gpu(scene, g_fd)["grads"], _run_gpu(scene, g_fd)["grads"])
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    nat = gt._GutNative(gt.gut_config_from_conf({"render": {"splat": {}}}))
    n = scene["density12"].shape[0]
    frame = nat.make_frame(7, 3, n, H, W, scene["cam"], scene["pose_start"], scene["pose_end"])
    d12, sph = torch.as_tensor(scene["density12"], device="cuda"), torch.as_tensor(scene["sph"], device="cuda")
    ro, rd = (torch.as_tensor(r[0], device="cuda").contiguous() for r in scene["rays"])
    fd, dist, cnt, vis, feat, opa = nat.trace(frame, d12, sph, ro, rd)
    g = torch.as_tensor(g_fd, device="cuda")
    gd, gs = nat.trace_bwd(frame, d12, sph, ro, rd, fd, g, dist, None)
    g_pos, g_dns, g_rot, g_scl, gs2 = nat.trace_bwd_unpacked(frame, d12, sph, ro, rd, fd, g[..., :3].contiguous(), g[..., 3:].contiguous(), dist, None)
    fgd, fgr = nat.trace_bwd_factored(frame, d12, sph, ro, rd, fd, g, dist, None)
    chunked = [nat.trace_bwd_factored_chunked(frame, d12, sph, ro, rd, fd, g, dist, None, k, lambda *a: None) for k in (2, 4)]
    gd_again, gs_again = nat.trace_bwd(frame, d12, sph, ro, rd, fd, g, dist, None)
    torch.cuda.synchronize()
    assert bool((gd[:len(BOXES)].abs().amax(1) > 0).all()), "every hand-placed particle is hit"
    assert torch.equal(g_pos, gd[:, 0:3]) and torch.equal(g_dns, gd[:, 3:4]) and torch.equal(g_rot, gd[:, 4:8]) and torch.equal(g_scl, gd[:, 8:11])
    assert torch.equal(gs, gs2)
    assert torch.equal(fgd, gd)
    for k, (cgd, cgr) in zip((2, 4), chunked):
        assert torch.equal(cgd, fgd) and torch.equal(cgr, fgr), f"{k} chunks"
    assert torch.equal(gd_again, gd) and torch.equal(gs_again, gs)


def test_nht_pixel_pair_backward_matches_oracle():
    """The feature sweep writes the marks too (gut_render_nht.inl); tolerance of test_gut_gpu.test_nht_backward_matches_oracle_on_a_larger_frame."""
    import torch
    n, w, h = 3000, 96, 64
    scene = make_scene(n=n, width=w, height=h, median_scale=0.06)
    feats = np.random.default_rng(5).uniform(-np.pi / 2, np.pi / 2, size=(n, 48)).astype(np.float32)
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    tr = gt.Tracer({"render": dict(splat={}), "model": NHT_MODEL})
    g_fd = np.random.default_rng(8).normal(size=(h, w, 25)).astype(np.float32)
    t = torch.as_tensor(g_fd, device="cuda")
    cfg = oracle.default_gut_config()
    fwd = oracle.gut_forward_nht(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], scene["density12"], feats, *scene["rays"])
    rd, rf = oracle.gut_backward_nht(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], scene["density12"], feats, *scene["rays"], fwd, g_fd)
    got = []
    for _ in range(2):   # the second step starts from the marks the first one left: zero
        gs = syn.SimpleGaussians(scene["density12"], feats)
        out = tr.render(gs, torch_batch(scene["batch"], "cuda"), train=True)
        ((out["pred_features"][0] * t[..., :24]).sum() + (out["pred_opacity"][0] * t[..., 24:]).sum()).backward()
        got.append(gs.grads_packed())
    gd, gf = got[0]
    flips = int((out["hits_count"][0, ..., 0].detach().cpu().numpy() != fwd["hit_count"][..., 0]).sum())
    for key, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
        assert _trimmed_rel_err(gd[:, sl], rd[:, sl], 3 * flips) < 1e-3, key
    assert _trimmed_rel_err(gf, rf, 3 * flips) < 1e-3
    assert np.array_equal(got[1][0], gd), "the geometric gradient (slots, no float atomics) is reproducible on one tracer"
