"""GPU parity: the HIP 3DGUT path (through the C-ABI, via the Tracer plugin surface) against the CPU oracle.

Tolerances are BASELINE.json's: RGB / depth within 1e-4 abs, gradients within 1e-3 relative
(||d||inf / ||ref||inf per tensor).  Accept/reject thresholds (alpha > 1/255, response > 0.0113,
T < 1e-4, tile culling) are evaluated in fp32 with different rounding on the two sides, so a
vanishing fraction of pixels / tile entries may flip; those are bounded explicitly below.
"""
import ctypes as C
import os
import importlib
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from scenes import make_camera_scene as _camera_scene, make_scene, rel_err, torch_batch

pytestmark = pytest.mark.gpu
syn = importlib.import_module("workloads.synthetic")


def _tracer(**render_kw):
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    splat_keys = set(gt._SPLAT_DEFAULTS)
    render = {k: v for k, v in render_kw.items() if k not in splat_keys}
    render["splat"] = {k: v for k, v in render_kw.items() if k in splat_keys}
    return gt.Tracer({"render": render})


def _run_gpu(scene, g_fd=None, g_dist=None, n_active=3, **render_kw):
    import torch
    tr = _tracer(**render_kw)
    g = syn.SimpleGaussians(scene["density12"], scene["sph"], n_active_features=n_active)
    out = tr.render(g, torch_batch(scene["batch"], "cuda"), train=True)
    res = dict(out=out, tracer=tr, gaussians=g)
    if g_fd is not None:
        fd = torch.cat([out["pred_features"], out["pred_opacity"]], dim=-1)[0]
        loss = (fd * torch.as_tensor(g_fd, device="cuda")).sum()
        if g_dist is not None:  # otherwise no gradient reaches pred_dist: the library runs its no-depth-gradient variant
            loss = loss + (out["pred_dist"][0] * torch.as_tensor(g_dist, device="cuda")).sum()
        loss.backward()
        res["grads"] = g.grads_packed()
    torch.cuda.synchronize()
    return res


def _run_oracle(scene, g_fd=None, g_dist=None, n_active=3, **cfg_kw):
    cfg = oracle.default_gut_config(**cfg_kw)
    fwd = oracle.gut_forward(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], n_active, scene["density12"], scene["sph"],
                             *scene["rays"])
    res = dict(fwd=fwd, cfg=cfg)
    if g_fd is not None:
        res["grads"] = oracle.gut_backward(cfg, scene["cam"], n_active, fwd, g_fd, g_dist)
    return res


def _image_checks(out, fwd, tol=1e-4, max_flip_frac=2e-3):
    fd = np.concatenate([out["pred_features"][0].detach().cpu().numpy(), out["pred_opacity"][0].detach().cpu().numpy()], -1)
    d_img = np.abs(fd - fwd["feat_density"]).max(-1)
    d_dist = np.abs(out["pred_dist"][0].detach().cpu().numpy() - fwd["hit_distance"])[..., 0]
    bad = (d_img > tol) | (d_dist > tol * np.maximum(1.0, np.abs(fwd["hit_distance"][..., 0])))
    assert bad.mean() <= max_flip_frac, f"{bad.sum()} pixels beyond tolerance (max rgb {d_img.max():.3e}, dist {d_dist.max():.3e})"
    return d_img, d_dist


@pytest.mark.parametrize("n,w,h,scale", [(2000, 64, 64, 0.05), (20000, 200, 120, 0.03), (500, 33, 47, 0.1)])
def test_forward_matches_oracle(n, w, h, scale):
    scene = make_scene(n=n, width=w, height=h, median_scale=scale)
    gpu, ora = _run_gpu(scene), _run_oracle(scene)
    d_img, d_dist = _image_checks(gpu["out"], ora["fwd"])
    st = gpu["tracer"].tracer_wrapper.stats()
    I_ref = ora["fwd"]["bins"]["num_intersections"]
    assert abs(int(st.num_intersections) - I_ref) <= max(2, 1e-3 * I_ref)
    vis = gpu["out"]["mog_visibility"].detach().view(-1).bool().cpu().numpy()
    assert (vis != (ora["fwd"]["visibility"] != 0)).mean() < 1e-3
    cnt = gpu["out"]["hits_count"][0, ..., 0].detach().cpu().numpy()
    assert (cnt != ora["fwd"]["hit_count"][..., 0]).mean() < 5e-3


def _trimmed_rel_err(got, ref, n_drop):
    """||got - ref||inf / ||ref||inf over particles after dropping the n_drop worst particles."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    per_particle = np.abs(got - ref).reshape(got.shape[0], -1).max(1)
    if n_drop > 0:
        per_particle = np.sort(per_particle)[: max(1, len(per_particle) - n_drop)]
    return float(per_particle.max() / (np.abs(ref).max() + 1e-12))


def _check_grads(scene, gpu, ora, g_fd, g_dist):
    """Gradients within 1e-3 relative (||d||inf / ||ref||inf per tensor), threshold-flip aware.

    The reference algorithm is discontinuous at its accept/reject thresholds (alpha > 1/255, response > 0.0113,
    T < 1e-4): a hit that is accepted on one side and rejected on the other moves the gradient of its particle by
    ~1e-3 of the tensor maximum.  Both sides evaluate these tests in fp32 with different rounding, so (i) the f64
    build of the oracle arbitrates — the HIP result must agree with the f32 OR the f64 oracle — and (ii) for every
    pixel whose hit count differs from the reference (a visible flip) up to 3 particles are exempted."""
    gd, gsph = gpu["grads"]
    cfg = ora["cfg"]
    f64 = oracle.gut_forward(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], 3, scene["density12"], scene["sph"],
                             *scene["rays"], dtype=np.float64)
    g64 = oracle.gut_backward(cfg, scene["cam"], 3, f64, g_fd, g_dist, dtype=np.float64)
    cnt = gpu["out"]["hits_count"][0, ..., 0].detach().cpu().numpy()
    refs = []
    for fwd, (rd, rsph, _) in ((ora["fwd"], ora["grads"]), (f64, g64)):
        n_flip = int((cnt != fwd["hit_count"][..., 0]).sum())
        assert n_flip <= max(2, 2e-3 * cnt.size), f"{n_flip} pixels with a different hit count"
        refs.append((rd, rsph, 3 * n_flip))
    names = {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}
    for k, sl in names.items():
        e = min(_trimmed_rel_err(gd[:, sl], rd[:, sl], drop) for rd, _, drop in refs)
        assert e < 1e-3, f"grad {k}: rel err {e:.3e}"
        assert min(rel_err(gd[:, sl], rd[:, sl]) for rd, _, _ in refs) < 1e-2, f"grad {k}: untrimmed error"
    assert min(_trimmed_rel_err(gsph, rsph, drop) for _, rsph, drop in refs) < 1e-3


@pytest.mark.parametrize("n,w,h,scale,with_depth_grad", [(3000, 96, 64, 0.06, True), (3000, 96, 64, 0.06, False),
                                                         (30000, 160, 96, 0.05, False), (30000, 160, 96, 0.05, True)])
def test_backward_matches_oracle(n, w, h, scale, with_depth_grad):
    """The larger scene has tile lists of several hundred entries, i.e. several checkpointed segments per tile."""
    scene = make_scene(n=n, width=w, height=h, median_scale=scale)
    g_fd, g_dist = syn.upstream_grads(w, h)
    g_fd *= w * h
    if with_depth_grad:
        g_dist = (np.random.default_rng(5).normal(size=g_dist.shape) * 0.1).astype(np.float32)
    gpu = _run_gpu(scene, g_fd, g_dist if with_depth_grad else None)
    ora = _run_oracle(scene, g_fd, g_dist)
    _image_checks(gpu["out"], ora["fwd"])
    _check_grads(scene, gpu, ora, g_fd, g_dist)


@pytest.mark.parametrize("kw,n_active", [(dict(particle_kernel_degree=4), 3), (dict(particle_kernel_degree=0), 3), (dict(particle_kernel_degree=3), 2),
                                         (dict(particle_radiance_sph_degree=2), 2), (dict(particle_radiance_sph_degree=3), 0),
                                         (dict(tile_based_culling=False, rect_bounding=False, tight_opacity_bounding=False), 3),
                                         (dict(global_z_order=False, min_transmittance=0.01, particle_kernel_max_alpha=0.9), 1)])
def test_config_variants_match_oracle(kw, n_active):
    """Run-time configuration surface (setup_3dgut.py:41-95 macros): generalized-Gaussian degrees, SH buffer degree vs
    active degree (progressive training), bounding / culling switches, distance ordering, clamps."""
    sph_degree = kw.get("particle_radiance_sph_degree", 3)
    scene = make_scene(n=3000, width=80, height=48, median_scale=0.07, sph_degree=sph_degree)
    w, h = 80, 48
    g_fd, g_dist = syn.upstream_grads(w, h)
    g_fd *= w * h
    gpu = _run_gpu(scene, g_fd, None, n_active=n_active, **kw)
    cfg = oracle.default_gut_config(**{k: (int(v) if isinstance(v, bool) else v) for k, v in kw.items()})
    fwd = oracle.gut_forward(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], n_active, scene["density12"], scene["sph"], *scene["rays"])
    _image_checks(gpu["out"], fwd, max_flip_frac=5e-3)
    rd, rsph, _ = oracle.gut_backward(cfg, scene["cam"], n_active, fwd, g_fd, g_dist)
    f64 = oracle.gut_forward(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], n_active, scene["density12"], scene["sph"], *scene["rays"],
                             dtype=np.float64)
    rd64, rsph64, _ = oracle.gut_backward(cfg, scene["cam"], n_active, f64, g_fd, g_dist, dtype=np.float64)
    gd, gsph = gpu["grads"]
    cnt = gpu["out"]["hits_count"][0, ..., 0].detach().cpu().numpy()
    drop = 3 * max(int((cnt != fwd["hit_count"][..., 0]).sum()), int((cnt != f64["hit_count"][..., 0]).sum()))
    for name, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
        e = min(_trimmed_rel_err(gd[:, sl], rd[:, sl], drop), _trimmed_rel_err(gd[:, sl], rd64[:, sl], drop))
        assert e < 1e-3, f"{kw}: grad {name} rel err {e:.3e}"
    assert min(_trimmed_rel_err(gsph, rsph, drop), _trimmed_rel_err(gsph, rsph64, drop)) < 1e-3
    # coefficients above the active degree receive exactly zero gradient
    nact = (n_active + 1) ** 2
    assert np.all(gsph[:, 3 * nact:] == 0)


@pytest.mark.parametrize("K,with_depth_grad", [(16, False), (16, True), (4, False)])
def test_sorted_kbuffer_mode_matches_oracle(K, with_depth_grad):
    """render.splat.k_buffer_size > 0 (configs/paper/3dgut/base_sorted.yaml): per-ray K-nearest hit buffer, forward and the
    Slang-derived backward (gutKBufferRenderer.cuh:62-122, 158-198)."""
    scene = make_scene(n=4000, width=96, height=64, median_scale=0.07)
    w, h = 96, 64
    g_fd, g_dist = syn.upstream_grads(w, h)
    g_fd *= w * h
    if with_depth_grad:
        g_dist = (np.random.default_rng(5).normal(size=g_dist.shape) * 0.1).astype(np.float32)
    gpu = _run_gpu(scene, g_fd, g_dist if with_depth_grad else None, k_buffer_size=K)
    ora = _run_oracle(scene, g_fd, g_dist, k_buffer_size=K)
    _image_checks(gpu["out"], ora["fwd"])
    # the sorted image really differs from the unsorted one
    unsorted = _run_oracle(scene)
    assert np.abs(unsorted["fwd"]["feat_density"] - ora["fwd"]["feat_density"]).max() > 1e-3
    cfg = ora["cfg"]
    f64 = oracle.gut_forward(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], 3, scene["density12"], scene["sph"], *scene["rays"],
                             dtype=np.float64)
    g64 = oracle.gut_backward(cfg, scene["cam"], 3, f64, g_fd, g_dist, dtype=np.float64)
    gd, gsph = gpu["grads"]
    cnt = gpu["out"]["hits_count"][0, ..., 0].detach().cpu().numpy()
    drop = 3 * max(int((cnt != ora["fwd"]["hit_count"][..., 0]).sum()), int((cnt != f64["hit_count"][..., 0]).sum()))
    rd, rsph, _ = ora["grads"]
    for name, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
        e = min(_trimmed_rel_err(gd[:, sl], rd[:, sl], drop), _trimmed_rel_err(gd[:, sl], g64[0][:, sl], drop))
        assert e < 1e-3, f"K={K}: grad {name} rel err {e:.3e}"
    assert min(_trimmed_rel_err(gsph, rsph, drop), _trimmed_rel_err(gsph, g64[1], drop)) < 1e-3


def test_gradients_are_bitwise_reproducible():
    """No atomics on the 3DGUT gradient path: two runs of the same frame give identical bits (the reference's
    float atomicAdd accumulation does not)."""
    scene = make_scene(n=20000, width=160, height=96, median_scale=0.04)
    g_fd, _ = syn.upstream_grads(160, 96)
    g_fd *= 160 * 96
    a = _run_gpu(scene, g_fd)["grads"]
    b = _run_gpu(scene, g_fd)["grads"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_per_pixel_ray_origins_match_oracle():
    """Rays that do not share an origin (the plugin API takes arbitrary per-pixel rays) run the general sweep."""
    scene = make_scene(n=3000, width=80, height=48, median_scale=0.06)
    ro, rd = scene["rays"]
    ro = ro + (np.random.default_rng(11).normal(size=ro.shape) * 0.02).astype(np.float32)
    scene["rays"] = (ro, rd)
    scene["batch"]["rays_ori"] = ro
    g_fd, g_dist = syn.upstream_grads(80, 48)
    g_fd *= 80 * 48
    g_dist = (np.random.default_rng(5).normal(size=g_dist.shape) * 0.1).astype(np.float32)
    for gd_in in (None, g_dist):
        gpu = _run_gpu(scene, g_fd, gd_in)
        ora = _run_oracle(scene, g_fd, g_dist if gd_in is not None else np.zeros_like(g_dist))
        _image_checks(gpu["out"], ora["fwd"])
        _check_grads(scene, gpu, ora, g_fd, g_dist if gd_in is not None else np.zeros_like(g_dist))


def torch_batch_rs(batch, device):
    tb = torch_batch(batch, device)
    if batch.get("T_to_world_end") is not None:
        import torch
        tb.T_to_world_end = torch.as_tensor(batch["T_to_world_end"], device=device)
    return tb


@pytest.mark.parametrize("kind", ["fisheye", "pinhole_rs", "ftheta"])
def test_camera_models_and_rolling_shutter_match_oracle(kind):
    """cameraProjections.cuh:72-257: OpenCV fisheye, distorted OpenCV pinhole and f-theta projections, the latter two
    under a rolling shutter with a moving sensor (5 pose-refinement iterations, mid-exposure pose for the rays)."""
    import torch
    scene = _camera_scene(kind)
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    tr = gt.Tracer({"render": {"splat": {}}})
    g = syn.SimpleGaussians(scene["density12"], scene["sph"])
    out = tr.render(g, torch_batch_rs(scene["batch"], "cuda"), train=True)
    w, h = scene["W"], scene["H"]
    g_fd, g_dist = syn.upstream_grads(w, h)
    g_fd *= w * h
    fd = torch.cat([out["pred_features"], out["pred_opacity"]], dim=-1)[0]
    (fd * torch.as_tensor(g_fd, device="cuda")).sum().backward()
    torch.cuda.synchronize()
    gpu = dict(out=out, grads=g.grads_packed(), tracer=tr)
    ora = _run_oracle(scene, g_fd, g_dist)
    _image_checks(out, ora["fwd"], max_flip_frac=5e-3)
    st = tr.tracer_wrapper.stats()
    I_ref = ora["fwd"]["bins"]["num_intersections"]
    assert I_ref > 1000 and abs(int(st.num_intersections) - I_ref) <= max(4, 2e-3 * I_ref)
    _check_grads(scene, gpu, ora, g_fd, g_dist)


def test_binning_is_ordered_and_consistent():
    """Integer work: per-tile lists are exactly (depth bits, particle index) ordered, ranges tile the list,
    per-particle multiplicity equals its tile count; membership equals the oracle's up to threshold flips."""
    import torch
    scene = make_scene(n=5000, width=128, height=80, median_scale=0.05)
    gpu, ora = _run_gpu(scene), _run_oracle(scene)
    nat = gpu["tracer"].tracer_wrapper
    st = nat.stats()
    N, I, tiles = st.num_particles, int(st.num_intersections), st.num_tiles
    dev = "cuda"
    tc = torch.zeros(N, dtype=torch.int32, device=dev)
    depth = torch.zeros(N, dtype=torch.float32, device=dev)
    sidx = torch.zeros(max(I, 1), dtype=torch.int32, device=dev)
    rng = torch.zeros((tiles, 2), dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    r = nat.lib.gut_debug_fetch(nat.handle, stream, p(tc), None, None, None, p(depth), None, p(sidx), p(rng))
    assert r == 0
    torch.cuda.synchronize()
    tc, depth = tc.cpu().numpy().view(np.uint32), depth.cpu().numpy()
    sidx, rng = sidx.cpu().numpy().view(np.uint32)[:I], rng.cpu().numpy().view(np.uint32)
    assert tc.sum() == I
    # ranges: contiguous, ascending by tile, cover [0, I)
    lens = (rng[:, 1] - rng[:, 0]).astype(np.int64)
    nz = lens > 0
    assert lens.sum() == I
    starts = rng[nz, 0]
    assert starts[0] == 0 and np.all(starts[1:] == rng[nz, 1][:-1])
    # ordering inside each tile: stable (depth bits, particle index)
    dbits = depth.view(np.uint32).astype(np.uint64)
    keys = (dbits[sidx] << np.uint64(32)) | sidx.astype(np.uint64)
    for t in np.nonzero(nz)[0]:
        k = keys[rng[t, 0]:rng[t, 1]]
        assert np.all(k[1:] > k[:-1]), f"tile {t} not strictly ordered by (depth, index)"
    assert np.array_equal(np.bincount(sidx, minlength=N).astype(np.uint32), tc)
    # membership vs the oracle
    ob = ora["fwd"]["bins"]
    otile = (ob["sorted_keys"] >> np.uint64(32)).astype(np.uint64)
    ref = set(zip(otile.tolist(), ob["sorted_idx"].tolist()))
    tile_of = np.repeat(np.arange(tiles), lens)
    got = set(zip(tile_of.tolist(), sidx.tolist()))
    sym = len(ref ^ got)
    assert sym <= max(2, 2e-3 * len(ref)), f"{sym} (tile, particle) pairs differ from the oracle"


def test_empty_and_degenerate_inputs():
    import torch
    # no particle reaches the image: outputs keep their initial values (gutRenderer.cu:323-325, splatRaster.cpp:212-216)
    scene = make_scene(n=64, width=32, height=32, median_scale=0.05)
    scene["density12"][:, 3] = 0.001  # below 1/255
    g_fd, _ = syn.upstream_grads(32, 32)
    gpu = _run_gpu(scene, g_fd * 1024)
    assert float(gpu["out"]["pred_opacity"].abs().max()) == 0.0
    assert float(gpu["out"]["pred_dist"].min()) == pytest.approx(1e6)
    assert int(gpu["tracer"].tracer_wrapper.stats().num_intersections) == 0
    assert not gpu["out"]["mog_visibility"].view(-1).bool().any()
    gd, gs = gpu["grads"]   # the backward of a frame without intersections: exact zeros, not stale scratch
    assert not gd.any() and not gs.any()


def test_timings_dict_contract():
    scene = make_scene(n=1000, width=64, height=64)
    gpu = _run_gpu(scene, enable_kernel_timings=True)
    t = gpu["tracer"].timings
    assert "forward_render" in t and t["forward_render"] > 0
    assert gpu["out"]["frame_time_ms"] > 0


@pytest.mark.parametrize("kw", [dict(), dict(k_buffer_size=8), dict(enable_hitcounts=False)])
def test_outputs_are_fully_overwritten(monkeypatch, kw):
    """The plugin allocates its outputs without fill passes: with NaN / -1 poison in place of torch.empty every pixel and
    every visibility flag must still come back defined and equal to the oracle's (dead pixels included)."""
    monkeypatch.setenv("GRUT_POISON_OUTPUTS", "1")
    scene = make_scene(n=1500, width=70, height=38, median_scale=0.06)   # not a multiple of the tile size
    gpu = _run_gpu(scene, **kw)
    ora = _run_oracle(scene, **{k: (int(v) if isinstance(v, bool) else v) for k, v in kw.items()})
    out = gpu["out"]
    for key in ("pred_features", "pred_opacity", "pred_dist", "hits_count"):
        assert bool(np.isfinite(out[key].detach().cpu().numpy()).all()), key
    import torch
    vis = out["mog_visibility"].view(-1).view(torch.int32).cpu().numpy()
    assert set(np.unique(vis).tolist()) <= {0, 1}
    _image_checks(out, ora["fwd"], max_flip_frac=5e-3)
    if not kw.get("enable_hitcounts", True):
        assert float(out["hits_count"].abs().max()) == 0.0


def test_one_tracer_across_growing_and_shrinking_frames():
    """The handle's scratch is grow-only and the tail of a frame is launched speculatively against the capacity left by
    earlier frames: a small frame, a much larger one (capacity exceeded -> the tail is redone), then the small one again
    (speculation against a generous capacity) must all match the oracle, with gradients."""
    import torch
    tr = _tracer()
    scenes = [make_scene(n=300, width=48, height=32, median_scale=0.05, seed=11),
              make_scene(n=6000, width=112, height=80, median_scale=0.08, seed=12),
              make_scene(n=300, width=48, height=32, median_scale=0.05, seed=11)]
    stats = []
    for scene in scenes:
        w, h = scene["W"], scene["H"]
        g_fd, g_dist = syn.upstream_grads(w, h)
        g_fd *= w * h
        g = syn.SimpleGaussians(scene["density12"], scene["sph"])
        out = tr.render(g, torch_batch(scene["batch"], "cuda"), train=True)
        fd = torch.cat([out["pred_features"], out["pred_opacity"]], dim=-1)[0]
        (fd * torch.as_tensor(g_fd, device="cuda")).sum().backward()
        torch.cuda.synchronize()
        gpu = dict(out=out, tracer=tr, gaussians=g, grads=g.grads_packed())
        ora = _run_oracle(scene, g_fd, g_dist)
        _image_checks(out, ora["fwd"])
        _check_grads(scene, gpu, ora, g_fd, g_dist)
        stats.append(int(tr.tracer_wrapper.stats().num_intersections))
    assert stats[1] > 4 * stats[0] and stats[2] == stats[0]


def test_runs_on_the_callers_stream():
    """Everything is enqueued on torch's CURRENT stream (tracer.py / splatRaster.cpp use at::cuda::getCurrentCUDAStream):
    a frame rendered and differentiated inside `torch.cuda.stream(side)` gives bit-identical results to the default stream."""
    import torch
    scene = make_scene(n=2500, width=80, height=48, median_scale=0.06)
    g_fd, _ = syn.upstream_grads(80, 48)
    ref = _run_gpu(scene, g_fd * 3840)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _run_gpu(scene, g_fd * 3840)
    side.synchronize()
    assert torch.equal(ref["out"]["pred_features"], got["out"]["pred_features"])
    assert np.array_equal(ref["grads"][0], got["grads"][0]) and np.array_equal(ref["grads"][1], got["grads"][1])


def test_projection_and_binning_match_reference_code_golden():
    """The HIP projection + binning stages DIRECTLY against tests/golden/projector.npz (the reference's own
    GUTProjector::eval / expand run on the host, oracle/ref/ref_projector.cpp): tile counts, projected centres, conics,
    extents, depths, and the per-tile sorted particle lists."""
    import os
    import sys
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    import make_golden
    from test_oracle_cpu import _golden_camera
    abi = importlib.import_module("3dgrut_amd._abi")
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    g = np.load(os.path.join(here, "golden", "projector.npz"))
    for k, c in enumerate(make_golden.projector_cases()):
        nat = gt._GutNative(gt.gut_config_from_conf({"render": {"splat": {}}}))
        n, W, H = len(c["d12"]), c["W"], c["H"]
        frame = nat.make_frame(0, 3, n, H, W, _golden_camera(c), c["ps"], c["pe"])
        d12 = torch.as_tensor(c["d12"], device="cuda")
        sph = torch.zeros((n, 48), device="cuda")
        rays_o = torch.zeros((H, W, 3), device="cuda")
        rays_d = torch.zeros((H, W, 3), device="cuda")
        rays_d[..., 2] = 1.0
        nat.trace(frame, d12, sph, rays_o, rays_d)
        st = nat.stats()
        I, tiles = int(st.num_intersections), int(st.num_tiles)
        tc = torch.zeros(n, dtype=torch.int32, device="cuda")
        pp, co, ex = torch.zeros((n, 2), device="cuda"), torch.zeros((n, 4), device="cuda"), torch.zeros((n, 2), device="cuda")
        dp = torch.zeros(n, device="cuda")
        sidx = torch.zeros(max(I, 1), dtype=torch.int32, device="cuda")
        rng = torch.zeros((tiles, 2), dtype=torch.int32, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())
        abi.check(nat.lib.gut_debug_fetch(nat.handle, stream, p(tc), p(pp), p(co), p(ex), p(dp), None, p(sidx), p(rng)), "gut_debug_fetch")
        torch.cuda.synchronize()
        tc = tc.cpu().numpy().view(np.uint32)
        ref_tc = g[f"p{k}_tiles"]
        dt = np.abs(tc.astype(np.int64) - ref_tc.astype(np.int64))
        assert (dt > 0).sum() <= max(2, 0.01 * n) and dt.max() <= 2, f"case {k}: {int((dt > 0).sum())} tile counts differ"
        both = (tc > 0) & (ref_tc > 0)
        assert np.abs(pp.cpu().numpy()[both] - g[f"p{k}_pos"][both]).max() < 2e-3
        assert np.abs(ex.cpu().numpy()[both] - g[f"p{k}_extent"][both]).max() < 2e-3
        assert np.abs(dp.cpu().numpy()[both] - g[f"p{k}_depth"][both]).max() <= 2e-5 * np.abs(g[f"p{k}_depth"][both]).max()
        a, b = co.cpu().numpy()[both], g[f"p{k}_conic"][both]
        assert (np.abs(a - b) / (np.abs(b) + 1e-6)).max() < 2e-3
        if not (dt > 0).any():   # identical counts: the per-tile lists must be the reference's sorted lists, tile by tile
            ref_keys, ref_idx = g[f"p{k}_sorted_keys"], g[f"p{k}_sorted_idx"]
            assert I == len(ref_idx)
            rng_h = rng.cpu().numpy().view(np.uint32)
            got = sidx.cpu().numpy().view(np.uint32)[:I]
            ref_tile = (ref_keys >> np.uint64(32)).astype(np.int64)
            for t in np.nonzero(rng_h[:, 1] > rng_h[:, 0])[0]:
                want = ref_idx[ref_tile == t]
                # equal depths (bit-identical keys) keep index order on both sides; depths may differ in the last bit
                assert set(got[rng_h[t, 0]:rng_h[t, 1]].tolist()) == set(want.tolist()), f"case {k}, tile {t}: different members"
                if np.array_equal(dp.cpu().numpy().view(np.uint32)[want], g[f"p{k}_depth"].view(np.uint32)[want]):
                    assert np.array_equal(got[rng_h[t, 0]:rng_h[t, 1]], want), f"case {k}, tile {t}: different order"


def test_device_poses_equal_host_poses_bit_for_bit():
    """GutFrame::device_T_to_world: the pose kernel (csrc/gut_poses.hip, built without contraction) against its host twin, which
    tests/test_host_cpu.py pins to the reference's Python bit for bit (tests/golden/pose.npz).  Global shutter (one pose): the whole
    47-float pose block - start / end [t, q], mid-exposure view matrix, sensor-to-world matrix - must be bit-identical for all 1033
    golden poses - including the ones whose unit quaternion has a float32 norm below 1 - 2^-23, for which glm::slerp takes its
    sin / acos branch even between a pose and itself.  Two different poses (rolling shutter): again the whole block (the interpolation's
    sinf / acosf are evaluated in float64 and rounded once on both sides, csrc/camera.hpp: pose_sinf)."""
    import torch
    lib = importlib.import_module("3dgrut_amd._abi").load_library()
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose.npz"))
    fp = C.POINTER(C.c_float)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dev_s, dev_e = torch.as_tensor(g["c2w"], device="cuda").contiguous(), torch.as_tensor(g["c2w_end"], device="cuda").contiguous()
    worst = 0.0
    for i in range(len(g["c2w"])):
        a, b = np.ascontiguousarray(g["c2w"][i]), np.ascontiguousarray(g["c2w_end"][i])
        host, dev = np.zeros(47, np.float32), np.zeros(47, np.float32)
        assert lib.grut_debug_frame_poses(None, 0, a.ctypes.data, None, host.ctypes.data_as(fp)) == 0
        assert lib.grut_debug_frame_poses(stream, 1, dev_s[i].data_ptr(), None, dev.ctypes.data_as(fp)) == 0
        assert np.array_equal(host.view(np.uint32), dev.view(np.uint32)), (i, np.flatnonzero(host.view(np.uint32) != dev.view(np.uint32)))
        assert np.array_equal(dev[9:16].view(np.uint32), g["tquat_start"][i].view(np.uint32))   # = the reference plugin's pose
        if i % 8 == 0:   # rolling shutter pairs
            assert lib.grut_debug_frame_poses(None, 0, a.ctypes.data, b.ctypes.data, host.ctypes.data_as(fp)) == 0
            assert lib.grut_debug_frame_poses(stream, 1, dev_s[i].data_ptr(), dev_e[i].data_ptr(), dev.ctypes.data_as(fp)) == 0
            assert np.array_equal(host[:23].view(np.uint32), dev[:23].view(np.uint32))           # start R / t / q, end t / q
            worst += float(not np.array_equal(host[23:].view(np.uint32), dev[23:].view(np.uint32)))
            assert float(np.abs(host[23:] - dev[23:]).max() / (1.0 + np.abs(host[23:]).max())) < 1e-6
    assert worst <= 1, worst   # (float64 sin / acos of the two sides may round a float differently once in ~1e8 evaluations)


def test_frame_matches_reference_kernels_golden():
    """The HIP frame DIRECTLY against tests/golden/gut_render.npz = the reference's own projectOnTiles / render / renderBackward
    kernels run on the host (oracle/ref/ref_gut_render.cpp).  Forward images for K = 0 and K = 16 against the reference's; the
    gradients against what renderBackward accumulated there, carried through the projection backward (the one stage of the
    backward that is Slang autodiff output in the reference, restated by the oracle) — BASELINE.json's tolerances."""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    import make_golden
    g = np.load(os.path.join(here, "golden", "gut_render.npz"))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    F = np.float32
    for k, kw in enumerate(make_golden.GUT_RENDER_SCENES):
        scene = make_scene(**kw)
        H, W = kw["height"], kw["width"]
        g_fd, g_dist = make_golden.gut_render_upstream(H, W)
        gpu = _run_gpu(scene, g_fd, g_dist)
        ref = dict(feat_density=g[f"s{k}_feat_density"], hit_distance=g[f"s{k}_hit_distance"])
        _image_checks(gpu["out"], ref)
        cnt = gpu["out"]["hits_count"][0, ..., 0].detach().cpu().numpy()
        n_flip = int((cnt != g[f"s{k}_hit_count"][..., 0]).sum())
        assert n_flip <= max(2, 2e-3 * cnt.size), f"scene {k}: {n_flip} pixels with a different hit count"
        st = gpu["tracer"].tracer_wrapper.stats()
        assert abs(int(st.num_intersections) - len(g[f"s{k}_sorted_idx"])) <= 2
        # reference gradients of renderBackward -> projection backward
        n = len(scene["density12"])
        cfg = oracle.default_gut_config()
        ref_gd, ref_grgb = g[f"s{k}_grad_density"].copy(), np.ascontiguousarray(g[f"s{k}_grad_features"])
        ref_gsph = np.zeros((n, 48), F)
        ps, pe = np.asarray(scene["pose_start"], F), np.asarray(scene["pose_end"], F)
        d12, sph = np.ascontiguousarray(scene["density12"], F), np.ascontiguousarray(scene["sph"], F)
        oracle.lib(F).orc_gut_project_bwd(C.byref(cfg), p(ps), p(pe), C.c_uint32(n), C.c_int(3), p(g[f"s{k}_tiles_count"]), p(d12), p(sph),
                                          p(ref_grgb), p(ref_gd), p(ref_gsph))
        gd, gsph = gpu["grads"]
        for name, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
            e = _trimmed_rel_err(gd[:, sl], ref_gd[:, sl], 3 * n_flip)
            assert e < 1e-3, f"scene {k}: grad {name} rel err {e:.3e}"
        assert _trimmed_rel_err(gsph, ref_gsph, 3 * n_flip) < 1e-3
        # sorted mode, K = 16
        gpu16 = _run_gpu(scene, k_buffer_size=16)
        _image_checks(gpu16["out"], dict(feat_density=g[f"s{k}_k16_feat_density"], hit_distance=g[f"s{k}_k16_hit_distance"]))


@pytest.mark.parametrize("sph_degree,n_active", [(3, 2), (2, 2), (3, 0)])
def test_factored_backward_rebuilds_the_sph_gradient(sph_degree, n_active):
    """gut_backward_factored + grut_sph_grad_from_views (the data-parallel exchange of 3dgrut_amd/dp.py): with one view the rebuilt
    SH gradient is bit for bit gut_backward's; with two views it is the sum of the two per-view gradients; the packed geometric
    gradient is untouched by the factoring."""
    import torch
    dp = importlib.import_module("3dgrut_amd.dp")
    abi = importlib.import_module("3dgrut_amd._abi")
    w, h = 96, 64
    g_fd, _ = syn.upstream_grads(w, h)
    g_fd *= w * h
    per_view = []
    for view in (0, 3):
        scene = make_scene(n=3000, width=w, height=h, median_scale=0.06, view=view, sph_degree=sph_degree)
        plain = _run_gpu(scene, g_fd, None, n_active=n_active, particle_radiance_sph_degree=sph_degree)
        tr = _tracer(particle_radiance_sph_degree=sph_degree)
        tr.gradient_exchange = dp.FactoredGradientExchange()          # no process group: one view, sum
        g = syn.SimpleGaussians(scene["density12"], scene["sph"], n_active_features=n_active)
        out = tr.render(g, torch_batch(scene["batch"], "cuda"), train=True)
        fd = torch.cat([out["pred_features"], out["pred_opacity"]], dim=-1)[0]
        (fd * torch.as_tensor(g_fd, device="cuda")).sum().backward()
        gd, gsph = g.grads_packed()
        assert np.array_equal(gd, plain["grads"][0]) and np.array_equal(gsph, plain["grads"][1]), f"view {view}"
        live = 3 * (n_active + 1) ** 2                                               # coefficients of the active degrees only
        assert gsph.shape[1] == 3 * (sph_degree + 1) ** 2 and np.abs(gsph[:, :live]).max() > 0
        assert live == gsph.shape[1] or np.abs(gsph[:, live:]).max() == 0
        per_view.append((scene, plain["grads"][1]))
    # two views through the library entry points directly
    factors = []
    for scene, _ in per_view:
        tr = _tracer(particle_radiance_sph_degree=sph_degree)
        captured = {}

        class Capture:
            def reduce_packed(self, g_density, g_radiance, positions, n_active, deg):
                captured["f"], captured["pos"] = g_radiance.clone(), positions.clone()
                return g_density, abi.sph_grad_from_views(g_radiance.unsqueeze(0), positions, n_active, deg)
        tr.gradient_exchange = Capture()
        g = syn.SimpleGaussians(scene["density12"], scene["sph"], n_active_features=n_active)
        out = tr.render(g, torch_batch(scene["batch"], "cuda"), train=True)
        fd = torch.cat([out["pred_features"], out["pred_opacity"]], dim=-1)[0]
        (fd * torch.as_tensor(g_fd, device="cuda")).sum().backward()
        factors.append(captured["f"])
        # row N of the factor is the view's sensor position
        cam = np.asarray(scene["batch"]["T_to_world"][0], np.float64)[:3, 3]
        assert np.abs(captured["f"][-1].cpu().numpy() - cam).max() < 1e-5
    both = abi.sph_grad_from_views(torch.stack(factors), captured["pos"], n_active, sph_degree).cpu().numpy()
    want = per_view[0][1].astype(np.float64) + per_view[1][1].astype(np.float64)
    assert np.abs(both - want).max() <= 1e-6 * np.abs(want).max()
    mean = abi.sph_grad_from_views(torch.stack(factors), captured["pos"][:, :3].contiguous(), n_active, sph_degree, scale=0.5).cpu().numpy()
    assert np.abs(mean - 0.5 * want).max() <= 1e-6 * np.abs(want).max()


@pytest.mark.parametrize("case", ["deg4", "fisheye", "pinhole_rs", "ftheta"])
def test_forward_matches_reference_kernels_golden_variants(case):
    """HIP images directly against the reference kernels' frames of tests/golden/gut_render.npz for the quartic kernel and for
    the three non-default camera configurations (fisheye with distortion; distorted pinhole and f-theta with rolling shutters)."""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    import make_golden
    import torch
    g = np.load(os.path.join(here, "golden", "gut_render.npz"))
    if case == "deg4":
        scene = make_scene(**make_golden.GUT_RENDER_SCENES[0])
        gpu = _run_gpu(scene, particle_kernel_degree=4)
        out = gpu["out"]
    else:
        kw = dict(make_golden.GUT_RENDER_CAMERA_SCENES)[case]
        scene = _camera_scene(case, **kw)
        tr = _tracer()
        gaussians = syn.SimpleGaussians(scene["density12"], scene["sph"])
        out = tr.render(gaussians, torch_batch_rs(scene["batch"], "cuda"), train=False)
        torch.cuda.synchronize()
    _image_checks(out, dict(feat_density=g[f"{case}_feat_density"], hit_distance=g[f"{case}_hit_distance"]), max_flip_frac=5e-3)
    cnt = out["hits_count"][0, ..., 0].detach().cpu().numpy()
    assert (cnt != g[f"{case}_hit_count"][..., 0]).mean() < 1e-2


@pytest.mark.parametrize("with_depth_grad,with_opacity_grad", [(False, True), (True, True), (False, False)])
def test_unpacked_backward_is_the_packed_backward_bit_for_bit(with_depth_grad, with_opacity_grad):
    """gut_backward_unpacked (split upstream gradients in, the model's four gradient tensors out: what the plugin calls on the
    training path) against gut_backward (the reference's packed [H,W,4] / [N,12] layout) on one forward context."""
    import torch
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    scene = make_scene(n=6000, width=112, height=72, median_scale=0.05)
    nat = gt._GutNative(gt.gut_config_from_conf({"render": {"splat": {}}}))
    n, W, H = scene["density12"].shape[0], scene["W"], scene["H"]
    frame = nat.make_frame(7, 3, n, H, W, scene["cam"], scene["pose_start"], scene["pose_end"])
    d12 = torch.as_tensor(scene["density12"], device="cuda")
    sph = torch.as_tensor(scene["sph"], device="cuda")
    ro, rd = (torch.as_tensor(r[0], device="cuda").contiguous() for r in scene["rays"])
    fd, dist, cnt, vis, feat, opa = nat.trace(frame, d12, sph, ro, rd)
    # the contiguous copies the plugin hands out are the packed image's channels
    assert feat.is_contiguous() and opa.is_contiguous()
    assert torch.equal(feat, fd[..., :3]) and torch.equal(opa, fd[..., 3:])
    rng = np.random.default_rng(2)
    g_feat = torch.as_tensor(rng.normal(size=(H, W, 3)).astype(np.float32), device="cuda")
    g_opa = torch.as_tensor(rng.normal(size=(H, W, 1)).astype(np.float32), device="cuda") if with_opacity_grad else None
    g_dist = torch.as_tensor((rng.normal(size=(H, W, 1)) * 0.1).astype(np.float32), device="cuda") if with_depth_grad else None
    g_fd = torch.cat([g_feat, g_opa if g_opa is not None else torch.zeros((H, W, 1), device="cuda")], dim=-1)
    gd, gs = nat.trace_bwd(frame, d12, sph, ro, rd, fd, g_fd, dist, g_dist)
    g_pos, g_dns, g_rot, g_scl, gs2 = nat.trace_bwd_unpacked(frame, d12, sph, ro, rd, fd, g_feat, g_opa, dist, g_dist)
    torch.cuda.synchronize()
    assert float(gd.abs().max()) > 0
    assert torch.equal(g_pos, gd[:, 0:3]) and torch.equal(g_dns, gd[:, 3:4]) and torch.equal(g_rot, gd[:, 4:8]) and torch.equal(g_scl, gd[:, 8:11])
    assert torch.equal(gs, gs2)


def test_plugin_outputs_are_contiguous_and_safe_to_modify():
    """`pred_features` / `pred_opacity` are contiguous tensors of their own like the reference's (tracer.py:334-337): `.view()` and
    in-place edits (e.g. compositing a background into them) work and do not disturb the backward."""
    import torch
    scene = make_scene(n=3000, width=80, height=48, median_scale=0.06)
    g_fd, _ = syn.upstream_grads(80, 48)
    g_fd *= 80 * 48
    ref = _run_gpu(scene, g_fd)["grads"]
    tr = _tracer()
    g = syn.SimpleGaussians(scene["density12"], scene["sph"])
    out = tr.render(g, torch_batch(scene["batch"], "cuda"), train=True)
    assert out["pred_features"].is_contiguous() and out["pred_opacity"].is_contiguous()
    flat = out["pred_features"].view(-1, 3)          # raises on a non-contiguous slice
    fd = torch.cat([out["pred_features"], out["pred_opacity"]], dim=-1)[0]
    loss = (fd * torch.as_tensor(g_fd, device="cuda")).sum()
    with torch.no_grad():
        flat.clamp_(0.0, 1.0)                          # in place, after the graph was recorded
    loss.backward()
    gd, gs = g.grads_packed()
    assert np.array_equal(gd, ref[0]) and np.array_equal(gs, ref[1])


@pytest.mark.parametrize("name", ["k0", "k4", "k16", "k16_depth"])
def test_gradients_match_autograd_golden(name):
    """The HIP gradients against tests/golden/autograd_gut.npz — float64 torch.autograd of the restated reference forward (Slang
    sources), i.e. what slangc's reverse mode yields for the sorted K > 0 compositing (G11) and the projection / SH backward (G12)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "autograd_gut.npz"))
    n, w, h, K = int(g[f"{name}_n"]), int(g[f"{name}_w"]), int(g[f"{name}_h"]), int(g[f"{name}_K"])
    scene = make_scene(n=n, width=w, height=h, median_scale=0.16, seed=int(g[f"{name}_seed"]))
    g_dist = g[f"{name}_g_dist"]
    gpu = _run_gpu(scene, g[f"{name}_g_fd"], g_dist if np.abs(g_dist).max() > 0 else None, k_buffer_size=K)
    f64 = oracle.gut_forward(oracle.default_gut_config(k_buffer_size=K), scene["cam"], scene["pose_start"], scene["pose_end"], 3, scene["density12"],
                             scene["sph"], *scene["rays"], dtype=np.float64)
    cnt = gpu["out"]["hits_count"][0, ..., 0].detach().cpu().numpy()
    drop = 3 * int((cnt != f64["hit_count"][..., 0]).sum())   # particles of pixels with a visible threshold flip
    assert drop <= 3 * max(2, 5e-3 * cnt.size)
    gd, gsph = gpu["grads"]
    ref = g[f"{name}_grad_density12"]
    for kname, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
        assert _trimmed_rel_err(gd[:, sl], ref[:, sl], drop) < 1e-3, (name, kname)
    assert _trimmed_rel_err(gsph, g[f"{name}_grad_sph"], drop) < 1e-3


@pytest.mark.parametrize("sph_half,out_half", [(True, False), (False, True), (True, True)])
def test_fp16_feature_io_matches_the_fp32_path_and_the_oracle(sph_half, out_half):
    """render.particle_feature_half / feature_output_half (setup_3dgut.py:60-61): coefficients are read from a half buffer and the
    [H,W,4] image is stored as half, arithmetic stays fp32.  So (i) half coefficients give BIT-identical results to the fp32 path fed
    the rounded coefficients, (ii) the half image is the fp32 image rounded once, (iii) the backward differentiates from the rounded
    image (rayPayloadBackward.cuh:50-58): oracle backward on the rounded finals, 1e-3 relative."""
    import torch
    n, w, h = 3000, 96, 64
    scene = make_scene(n=n, width=w, height=h, median_scale=0.06)
    g_fd, g_dist = syn.upstream_grads(w, h)
    g_fd *= w * h
    rounded = dict(scene, sph=oracle.round_to_half(scene["sph"])) if sph_half else scene
    assert not sph_half or np.abs(rounded["sph"] - scene["sph"]).max() > 1e-5   # the rounding is visible in the input
    ref32 = _run_gpu(rounded, g_fd, None)                                         # the fp32 path on the coefficients the kernels see
    gpu = _run_gpu(scene, g_fd, None, particle_feature_half=sph_half, feature_output_half=out_half)
    cat = lambda out: torch.cat([out["pred_features"], out["pred_opacity"]], dim=-1)[0].detach()
    fd32, fd = cat(ref32["out"]), cat(gpu["out"])
    assert fd.dtype == torch.float32   # always fp32 to the caller (tracer.py:214-215)
    if out_half:
        assert torch.equal(fd, fd32.half().float()), "the half image must be the fp32 image rounded once"
    else:
        assert torch.equal(fd, fd32), "half coefficients: same arithmetic on the rounded values"
    assert torch.equal(gpu["out"]["pred_dist"], ref32["out"]["pred_dist"]) and torch.equal(gpu["out"]["hits_count"], ref32["out"]["hits_count"])
    if not out_half:
        assert np.array_equal(gpu["grads"][0], ref32["grads"][0]) and np.array_equal(gpu["grads"][1], ref32["grads"][1])
    assert gpu["grads"][1].dtype == np.float32
    # oracle, half mode
    ora = _run_oracle(rounded)
    fwd = ora["fwd"]
    if out_half:
        fwd = dict(fwd, feat_density=oracle.round_to_half(fwd["feat_density"]))
        got = fd.detach().cpu().numpy()
        ulp = np.spacing(np.abs(got).astype(np.float16)).astype(np.float32)
        assert (np.abs(got - ora["fwd"]["feat_density"]) > 1e-4 + 0.5 * ulp).mean() <= 2e-3
    else:
        _image_checks(gpu["out"], fwd)
    ora = dict(ora, fwd=fwd, grads=oracle.gut_backward(ora["cfg"], scene["cam"], 3, fwd, g_fd, g_dist * 0))
    names = {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}
    cnt = gpu["out"]["hits_count"][0, ..., 0].detach().cpu().numpy()
    drop = 3 * int((cnt != fwd["hit_count"][..., 0]).sum())
    for k, sl in names.items():
        assert _trimmed_rel_err(gpu["grads"][0][:, sl], ora["grads"][0][:, sl], drop) < 1e-3, k
    assert _trimmed_rel_err(gpu["grads"][1], ora["grads"][1], drop) < 1e-3


def test_scratch_comes_from_the_callers_allocator_and_is_quiet_in_steady_state():
    """grut_set_allocator (include/grut_amd.h): the plugins route the library's grow-only scratch through torch's caching allocator.
    Steady state = no allocator traffic at all; a growing scene re-allocates a buffer only when it outgrows its head-room (a handful of
    events over +50 % of growth, not one per step); trim hands everything back and the tracer keeps working."""
    import torch
    abi = importlib.import_module("3dgrut_amd._abi")
    stats = abi.allocator_stats
    scene = make_scene(n=20000, width=160, height=96, median_scale=0.05)
    tr = _tracer()
    batch = torch_batch(scene["batch"], "cuda")

    def frame(n):
        g = syn.SimpleGaussians(scene["density12"][:n], scene["sph"][:n])
        out = tr.render(g, batch, train=True)
        (out["pred_features"].sum() + out["pred_opacity"].sum()).backward()
        return out["pred_features"].detach().clone()
    ref = frame(12000)
    assert stats["allocs"] > 10 and stats["live_bytes"] > 0, "the scratch did not come from torch's allocator"
    frame(12000)
    before = dict(stats)
    for _ in range(10):
        frame(12000)
    assert stats["allocs"] == before["allocs"] and stats["frees"] == before["frees"], "allocator traffic in steady state"
    for k in range(50):           # +1 % per step
        frame(12000 + 120 * (k + 1))
    grown = stats["allocs"] - before["allocs"]
    assert 0 < grown <= 80, f"{grown} allocations over 50 growing frames"   # ~30 buffers x at most two growth steps of 1.25x
    live = stats["live_bytes"]
    tr.tracer_wrapper.trim()
    assert stats["live_bytes"] < 0.05 * live
    torch.cuda.synchronize()
    assert torch.equal(frame(12000), ref)


NHT_MODEL = {"feature_type": "nht", "nht_features": {"dim": 48, "activation": {"type": "sincos", "num_frequencies": 1}, "interpolation_type": "barycentric"}}


def _nht_render(scene, feats, model=NHT_MODEL, **render_kw):
    import torch
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    tr = gt.Tracer({"render": dict(render_kw, splat={}), "model": model})
    g = syn.SimpleGaussians(scene["density12"], feats, requires_grad=False)
    with torch.no_grad():
        out = tr.render(g, torch_batch(scene["batch"], "cuda"))
    torch.cuda.synchronize()
    return tr, out


@pytest.mark.parametrize("k", [0, 1])
def test_nht_forward_matches_reference_kernels_golden(k):
    """model.feature_type = nht through the plugin against tests/golden/gut_nht.npz — the reference's own render kernel built with the
    nht macro set (tests/test_oracle_cpu.py pins the oracle on the same file): [1,H,W,24] ray features + opacity, hit distance, counts."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import make_golden as mg
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "gut_nht.npz"))
    scene = make_scene(**mg.GUT_RENDER_SCENES[k])
    tr, out = _nht_render(scene, g[f"s{k}_features"])
    ref = g[f"s{k}_feat_density"]
    assert tuple(out["pred_features"].shape) == (1,) + ref.shape[:2] + (24,) and tuple(out["pred_opacity"].shape) == (1,) + ref.shape[:2] + (1,)
    f = out["pred_features"][0].cpu().numpy()
    o = out["pred_opacity"][0].cpu().numpy()
    cnt = out["hits_count"][0].cpu().numpy()
    flips = cnt != g[f"s{k}_hit_count"]
    assert flips.mean() <= 2e-3
    bad = (np.abs(f - ref[..., :24]).max(-1) > 1e-4) | (np.abs(o - ref[..., 24:])[..., 0] > 1e-4) | \
          (np.abs(out["pred_dist"][0].cpu().numpy() - g[f"s{k}_hit_distance"])[..., 0] > 1e-4)
    assert (bad & ~flips[..., 0]).sum() == 0 and bad.mean() <= 2e-3, f"{bad.sum()} pixels beyond 1e-4"


@pytest.mark.parametrize("model_kw,half", [({}, False), ({}, True),
                                           ({"nht_features": {"dim": 8, "activation": {"type": "relu", "num_frequencies": 1}, "interpolation_type": "none"}}, False),
                                           ({"nht_features": {"dim": 16, "activation": {"type": "siren", "num_frequencies": 3}, "interpolation_type": "barycentric"}}, False)])
def test_nht_forward_matches_oracle(model_kw, half):
    """Larger frame and the other feature-model variants (centre support, relu / siren, several frequencies; fp16 feature buffer + fp16
    output) against the oracle's orc_gut_render_nht_fwd on the GPU's own tile lists' twin (the oracle bins for itself: binning is pinned
    integer-exactly elsewhere)."""
    import torch
    model = dict(NHT_MODEL, **model_kw)
    nf = model["nht_features"]
    scene = make_scene(n=6000, width=120, height=72, median_scale=0.05)
    feats = np.random.default_rng(3).uniform(-np.pi / 2, np.pi / 2, size=(6000, nf["dim"])).astype(np.float32)
    points = 4 if nf["interpolation_type"] == "barycentric" else 1
    nht = dict(particle_feature_dim=nf["dim"], interp_point_dim=nf["dim"] // points, support=int(points == 4),
               activation={"none": 0, "siren": 1, "sincos": 2, "relu": 3}[nf["activation"]["type"]], num_frequencies=nf["activation"]["num_frequencies"])
    kw = dict(particle_feature_half=True, feature_output_half=True) if half else {}
    tr, out = _nht_render(scene, feats, model, **kw)
    ofeats = oracle.round_to_half(feats) if half else feats
    ora = oracle.gut_forward_nht(oracle.default_gut_config(), scene["cam"], scene["pose_start"], scene["pose_end"], scene["density12"], ofeats,
                                 *scene["rays"], nht=nht)
    nr = oracle.nht_ray_feature_dim(nht)
    assert tr.tracer_wrapper.ray_feature_dim == nr and out["pred_features"].shape[-1] == nr and out["pred_features"].dtype == torch.float32
    got = np.concatenate([out["pred_features"][0].cpu().numpy(), out["pred_opacity"][0].cpu().numpy()], -1)
    ulp = np.spacing(np.abs(got).astype(np.float16)).astype(np.float32) if half else 0.0
    flips = (out["hits_count"][0].cpu().numpy() != ora["hit_count"])[..., 0]
    bad = (np.abs(got - ora["feat_density"]) > 1e-4 + 0.5 * ulp).any(-1)
    assert flips.mean() <= 2e-3 and (bad & ~flips).mean() <= 1e-3, f"{bad.sum()} pixels beyond tolerance, {flips.sum()} flips"
    assert np.abs(got[..., :nr]).max() > 0.3


def test_nht_activation_survives_features_far_outside_the_initial_range():
    """v_sin_f32 / v_cos_f32 return 0 for arguments beyond 256 revolutions; features that drift there during training would silently lose
    their activation on the pixel-pair sweeps (they are initialised in [-pi/2, pi/2], nothing bounds them).  The argument is reduced first
    (csrc/gut_render_nht.inl: v_fract_f32).  Features of +-2000..2600 rad = 320..410 revolutions: the image must follow the oracle's libm
    sincos - loosely (median 5e-3, maximum 0.1; measured 2e-3 / 0.025: one ulp of an fp32 angle of 2600 is 2.4e-4 rad, and the barycentric
    sum that forms the angle has weights beyond [0, 1]) - and must not be the
    all-zero activation.  Both kernel families (pixel-pair fast path and the generic strip kernels) are held to it."""
    scene = make_scene(n=3000, width=96, height=64, median_scale=0.06)
    rng = np.random.default_rng(5)
    feats = (rng.uniform(2000.0, 2600.0, size=(3000, 48)) * rng.choice([-1.0, 1.0], size=(3000, 48))).astype(np.float32)
    nf = NHT_MODEL["nht_features"]
    nht = dict(particle_feature_dim=48, interp_point_dim=12, support=1, activation=2, num_frequencies=nf["activation"]["num_frequencies"])
    ora = oracle.gut_forward_nht(oracle.default_gut_config(), scene["cam"], scene["pose_start"], scene["pose_end"], scene["density12"], feats,
                                 *scene["rays"], nht=nht)
    nr = oracle.nht_ray_feature_dim(nht)
    assert np.abs(ora["feat_density"][..., :nr]).max() > 0.3
    for generic in (False, True):
        if generic:
            os.environ["GRUT_NHT_GENERIC"] = "1"
        try:
            _, out = _nht_render(scene, feats, NHT_MODEL)
        finally:
            os.environ.pop("GRUT_NHT_GENERIC", None)
        got = np.concatenate([out["pred_features"][0].cpu().numpy(), out["pred_opacity"][0].cpu().numpy()], -1)
        flips = (out["hits_count"][0].cpu().numpy() != ora["hit_count"])[..., 0]
        err = np.abs(got - ora["feat_density"]).max(-1)
        assert flips.mean() <= 2e-3 and np.median(err[~flips]) < 5e-3 and err[~flips].max() < 0.1, (generic, float(err[~flips].max()), int(flips.sum()))
        assert np.abs(got[..., :nr]).max() > 0.3, "the activation vanished"


@pytest.mark.parametrize("name", ["nht", "nht_depth"])
def test_nht_gradients_match_autograd_golden(name):
    """The nht backward (Slang autodiff output in the reference) against float64 torch.autograd of the restated forward
    (tests/golden/autograd_gut_nht.npz) and against the oracle's reverse mode: particle rows and the feature buffer."""
    import torch
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "autograd_gut_nht.npz"))
    n, w, h, seed = (int(g[f"{name}_{k}"]) for k in ("n", "w", "h", "seed"))
    scene = make_scene(n=n, width=w, height=h, median_scale=0.16, seed=seed)
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    tr = gt.Tracer({"render": {"splat": {}}, "model": NHT_MODEL})
    gs = syn.SimpleGaussians(scene["density12"], g[f"{name}_features"])
    out = tr.render(gs, torch_batch(scene["batch"], "cuda"), train=True)
    g_fd, g_dist = torch.as_tensor(g[f"{name}_g_fd"], device="cuda"), torch.as_tensor(g[f"{name}_g_dist"], device="cuda")
    loss = (out["pred_features"][0] * g_fd[..., :24]).sum() + (out["pred_opacity"][0] * g_fd[..., 24:]).sum()
    if name == "nht_depth":
        loss = loss + (out["pred_dist"][0] * g_dist).sum()
    loss.backward()
    gd, gf = gs.grads_packed()
    ref_d, ref_f = g[f"{name}_grad_density12"], g[f"{name}_grad_features"]
    for key, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
        assert rel_err(gd[:, sl], ref_d[:, sl]) < 1e-3, (key, rel_err(gd[:, sl], ref_d[:, sl]))
    assert rel_err(gf, ref_f) < 1e-3 and gf.shape == (n, 48) and gf.dtype == np.float32


@pytest.mark.parametrize("half", [False, True])
def test_nht_backward_matches_oracle_on_a_larger_frame(half):
    import torch
    scene = make_scene(n=5000, width=112, height=64, median_scale=0.05)
    feats = np.random.default_rng(5).uniform(-np.pi / 2, np.pi / 2, size=(5000, 48)).astype(np.float32)
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    kw = dict(particle_feature_half=True, feature_output_half=True) if half else {}
    tr = gt.Tracer({"render": dict(kw, splat={}), "model": NHT_MODEL})
    gs = syn.SimpleGaussians(scene["density12"], feats)
    out = tr.render(gs, torch_batch(scene["batch"], "cuda"), train=True)
    rng = np.random.default_rng(8)
    g_fd = rng.normal(size=(64, 112, 25)).astype(np.float32)
    t = torch.as_tensor(g_fd, device="cuda")
    ((out["pred_features"][0] * t[..., :24]).sum() + (out["pred_opacity"][0] * t[..., 24:]).sum()).backward()
    gd, gf = gs.grads_packed()
    cfg = oracle.default_gut_config()
    ofeats = oracle.round_to_half(feats) if half else feats
    fwd = oracle.gut_forward_nht(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], scene["density12"], ofeats, *scene["rays"])
    if half:   # the backward starts from the rounded image (rayPayloadBackward.cuh:50-58)
        fwd = dict(fwd, feat_density=oracle.round_to_half(fwd["feat_density"]))
    rd, rf = oracle.gut_backward_nht(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], scene["density12"], ofeats, *scene["rays"], fwd, g_fd)
    flips = int((out["hits_count"][0, ..., 0].detach().cpu().numpy() != fwd["hit_count"][..., 0]).sum())
    for key, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
        assert _trimmed_rel_err(gd[:, sl], rd[:, sl], 3 * flips) < 1e-3, key
    assert _trimmed_rel_err(gf, rf, 3 * flips) < 1e-3


@pytest.mark.parametrize("depth_grad,inside", [pytest.param(False, False, id="False"), pytest.param(True, False, id="True"),
                                               pytest.param(True, True, id="inside-True")])
def test_nht_pixel_pair_sweeps_equal_the_generic_kernels(depth_grad, inside, monkeypatch):
    """The default feature model (48 = 4 x 12 floats, sincos) runs on the pixel-pair half-tile sweeps (csrc/gut_render_nht.inl: checkpointed
    backward tasks, slot gradients, one 48-lane atomic per entry); every other shape on the generic strip kernels, which the goldens and
    the oracle pin above.  Same frame through both - a dense one, tile lists of several 256-entry segments, so that the backward starts
    most of its tasks from a checkpoint - must agree: images to 2e-5, gradients to 2e-4 of the largest entry.
    `inside`: the same on a frame rendered from inside the cloud (tests/inside_scenes.py, 300 big particles): canonical intersections close
    to and behind the ray origins."""
    import torch
    if inside:
        from inside_scenes import make_inside_scene
        scene = make_inside_scene("pinhole", 96, 64, n_far=3000, n_near=600, n_big=300, seed=3)
    else:
        scene = make_scene(n=30000, width=160, height=96, median_scale=0.06, max_density=0.35)
    n, W, H = len(scene["density12"]), scene["W"], scene["H"]
    feats = np.random.default_rng(9).uniform(-np.pi / 2, np.pi / 2, size=(n, 48)).astype(np.float32)
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    rng = np.random.default_rng(10)
    g_fd = torch.as_tensor(rng.normal(size=(H, W, 25)).astype(np.float32), device="cuda")
    g_dist = torch.as_tensor(rng.normal(size=(H, W, 1)).astype(np.float32), device="cuda")

    def run(generic):
        if generic:
            monkeypatch.setenv("GRUT_NHT_GENERIC", "1")
        else:
            monkeypatch.delenv("GRUT_NHT_GENERIC", raising=False)
        tr = gt.Tracer({"render": {"enable_hitcounts": True, "splat": {}}, "model": NHT_MODEL})
        gs = syn.SimpleGaussians(scene["density12"], feats)
        out = tr.render(gs, torch_batch(scene["batch"], "cuda"), train=True)
        loss = (out["pred_features"][0] * g_fd[..., :24]).sum() + (out["pred_opacity"][0] * g_fd[..., 24:]).sum()
        if depth_grad:
            loss = loss + (out["pred_dist"][0] * g_dist).sum()
        loss.backward()
        torch.cuda.synchronize()
        st = tr.tracer_wrapper.stats()
        return {k: out[k].detach().cpu().numpy() for k in ("pred_features", "pred_opacity", "pred_dist", "hits_count")}, gs.grads_packed(), st
    (o_f, (gd_f, gf_f), st), (o_g, (gd_g, gf_g), _) = run(False), run(True)
    assert int(st.num_intersections) > 40 * int(st.num_tiles) * 4, "the frame should hold tile lists of several segments"
    # the two kernels evaluate the accept tests with differently rounded reciprocals / square roots: a few pixels of ~130 hits each flip one
    flips = (o_f["hits_count"] != o_g["hits_count"])[0, ..., 0]
    print(f"pixel-pair vs generic: {int(flips.sum())} of {flips.size} pixels differ in their hit count")
    assert flips.mean() <= 2e-3
    for k in ("pred_features", "pred_opacity", "pred_dist"):
        assert np.abs(o_f[k] - o_g[k])[0][~flips].max() < 2e-5, k
    nflip = int(flips.sum())
    for key, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
        assert _trimmed_rel_err(gd_f[:, sl], gd_g[:, sl], 3 * nflip) < 2e-4, (key, _trimmed_rel_err(gd_f[:, sl], gd_g[:, sl], 3 * nflip))
    assert _trimmed_rel_err(gf_f, gf_g, 3 * nflip) < 2e-4 and float(np.abs(gf_g).max()) > 0


@pytest.mark.parametrize("depth_grad,rolling,inside", [pytest.param(False, False, False, id="False-False"), pytest.param(True, False, False, id="True-False"),
                                                       pytest.param(False, True, False, id="False-True"), pytest.param(True, False, True, id="inside-True-False")])
def test_quarter_tile_forward_equals_the_half_tile_forward(depth_grad, rolling, inside, monkeypatch):
    """Launches that fit the chip at once (BASELINE configs 1 and 2) run the forward with one pixel per lane, a quarter tile per wave
    (csrc/gut_render.hip: gut_render_fwd_quarter_kernel) - the pair sweep's expressions component by component.  The same dense frame (tile
    lists of many 64-entry segments: most gradient-sweep tasks start from a checkpoint, some from a boundary only ONE quarter of the half
    tile reached alive) through both forwards: images, distances, hit counts and - through the checkpoints - every gradient must be
    bit-identical, with and without a depth gradient.  With per-pixel ray origins (the sweeps' non-uniform-origin form) the two compiled
    sweeps differ by an ulp per hit (median 1.2e-7 on the image): rounding-level agreement is asserted there.
    `inside`: the same equalities on a frame rendered from inside the cloud (tests/inside_scenes.py: 300 big particles, 214 of them on every
    tile of the 96x64 frame, ray origins inside particles, half of the cloud behind the sensor)."""
    import torch
    if inside:
        from inside_scenes import make_inside_scene
        scene = make_inside_scene("pinhole", 96, 64, n_far=3000, n_near=600, n_big=300, seed=3)
    else:
        scene = make_scene(n=30000, width=160, height=96, median_scale=0.06, max_density=0.35)
    W, H = scene["W"], scene["H"]
    rng = np.random.default_rng(12)
    if rolling:   # every pixel its own ray origin (what a moving sensor's rays look like): the sweeps' non-uniform-origin form
        scene["batch"]["rays_ori"] = (scene["batch"]["rays_ori"] + 2e-3 * rng.normal(size=scene["batch"]["rays_ori"].shape)).astype(np.float32)
    g_fd = rng.normal(size=(H, W, 4)).astype(np.float32)
    g_dist = rng.normal(size=(H, W, 1)).astype(np.float32) if depth_grad else None

    def run(quarter):
        monkeypatch.setenv("GRUT_FWD_QUARTER", "1" if quarter else "0")
        r = _run_gpu(scene, g_fd, g_dist, enable_hitcounts=True)
        o = r["out"]
        return [o[k].detach().cpu().numpy() for k in ("pred_features", "pred_opacity", "pred_dist", "hits_count")] + list(r["grads"]), r["tracer"].tracer_wrapper.stats()
    (a, st), (b, _) = run(True), run(False)
    assert int(st.num_intersections) > 64 * 4 * int(st.num_tiles), "the frame should hold tile lists of several segments"
    if not rolling:
        for x, y, name in zip(a, b, ("features", "opacity", "distance", "hit count", "grad density12", "grad sph")):
            assert np.array_equal(x, y), f"{name}: {int((x != y).sum())} values differ"
    else:
        flips = (a[3] != b[3])[0, ..., 0]
        assert flips.mean() <= 1e-3
        for x, y, name in zip(a[:3], b[:3], ("features", "opacity", "distance")):
            assert np.abs(x - y)[0][~flips].max() < 5e-6, name
        nflip = int(flips.sum())
        assert _trimmed_rel_err(a[4][:, :11], b[4][:, :11], 3 * nflip) < 1e-4 and _trimmed_rel_err(a[5], b[5], 3 * nflip) < 1e-4
    assert float(np.abs(a[4]).max()) > 0


@pytest.mark.parametrize("k,K", [(0, 4), (0, 16), (1, 4), (1, 16)])
def test_nht_with_the_sorted_hit_buffer_matches_reference_kernels_golden(k, K):
    """Round 6 (refused until then): model.feature_type = nht together with render.splat.k_buffer_size > 0 - the sorted hit buffer in front of
    the feature integration (gutKBufferRenderer.cuh:158-225, 273-352 with PerRayParticleFeatures) - against tests/golden/gut_nht.npz s*_k{4,16}_* =
    the reference's own kernels built with GAUSSIAN_K_BUFFER_SIZE 4 / 16 AND the feature macros."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import make_golden as mg
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "gut_nht.npz"))
    scene = make_scene(**mg.GUT_RENDER_SCENES[k])
    import torch
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    tr = gt.Tracer({"render": {"splat": {"k_buffer_size": K}}, "model": NHT_MODEL})
    gs = syn.SimpleGaussians(scene["density12"], g[f"s{k}_features"], requires_grad=False)
    with torch.no_grad():
        out = tr.render(gs, torch_batch(scene["batch"], "cuda"))
    ref = g[f"s{k}_k{K}_feat_density"]
    f = out["pred_features"][0].cpu().numpy()
    o = out["pred_opacity"][0].cpu().numpy()
    cnt = out["hits_count"][0].cpu().numpy()
    flips = (cnt != g[f"s{k}_k{K}_hit_count"])[..., 0]
    bad = (np.abs(f - ref[..., :24]).max(-1) > 1e-4) | (np.abs(o - ref[..., 24:])[..., 0] > 1e-4) | \
          (np.abs(out["pred_dist"][0].cpu().numpy() - g[f"s{k}_k{K}_hit_distance"])[..., 0] > 1e-4)
    # (hits whose distances tie to rounding may come out of the buffer in the other order: bounded, like the SH sorted mode's golden test)
    assert flips.mean() <= 5e-3 and (bad & ~flips).mean() <= 5e-3, f"{int(bad.sum())} pixels beyond 1e-4, {int(flips.sum())} flips"
    assert np.abs(ref - g[f"s{k}_feat_density"]).max() > 0.1    # (not the unsorted frame)


@pytest.mark.parametrize("name", ["nht_k4", "nht_k16_depth"])
def test_nht_with_the_sorted_hit_buffer_gradients_match_autograd_golden(name):
    """... and its backward against float64 torch.autograd of the restated forward with the hit buffer's order (tests/golden/autograd_gut_nht.npz:
    nht_k4, nht_k16_depth) - particle rows and the feature buffer, with a hit-distance gradient for K = 16."""
    import torch
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "autograd_gut_nht.npz"))
    n, w, h, seed, K = (int(g[f"{name}_{k}"]) for k in ("n", "w", "h", "seed", "K"))
    scene = make_scene(n=n, width=w, height=h, median_scale=0.16, seed=seed)
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    tr = gt.Tracer({"render": {"splat": {"k_buffer_size": K}}, "model": NHT_MODEL})
    gs = syn.SimpleGaussians(scene["density12"], g[f"{name}_features"])
    out = tr.render(gs, torch_batch(scene["batch"], "cuda"), train=True)
    g_fd, g_dist = torch.as_tensor(g[f"{name}_g_fd"], device="cuda"), torch.as_tensor(g[f"{name}_g_dist"], device="cuda")
    loss = (out["pred_features"][0] * g_fd[..., :24]).sum() + (out["pred_opacity"][0] * g_fd[..., 24:]).sum()
    if name.endswith("depth"):
        loss = loss + (out["pred_dist"][0] * g_dist).sum()
    loss.backward()
    gd, gf = gs.grads_packed()
    ref_d, ref_f = g[f"{name}_grad_density12"], g[f"{name}_grad_features"]
    for key, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
        assert rel_err(gd[:, sl], ref_d[:, sl]) < 1e-3, (key, rel_err(gd[:, sl], ref_d[:, sl]))
    assert rel_err(gf, ref_f) < 1e-3 and gf.shape == (n, 48)


@pytest.mark.parametrize("K,model_kw", [(8, {}), (16, {"nht_features": {"dim": 16, "activation": {"type": "siren", "num_frequencies": 3}, "interpolation_type": "barycentric"}})])
def test_nht_with_the_sorted_hit_buffer_matches_oracle_on_a_larger_frame(K, model_kw):
    import torch
    model = dict(NHT_MODEL, **model_kw)
    nf = model["nht_features"]
    scene = make_scene(n=5000, width=112, height=64, median_scale=0.05)
    feats = np.random.default_rng(5).uniform(-np.pi / 2, np.pi / 2, size=(5000, nf["dim"])).astype(np.float32)
    nht = dict(particle_feature_dim=nf["dim"], interp_point_dim=nf["dim"] // 4, support=1,
               activation={"none": 0, "siren": 1, "sincos": 2, "relu": 3}[nf["activation"]["type"]], num_frequencies=nf["activation"]["num_frequencies"])
    nr = oracle.nht_ray_feature_dim(nht)
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    tr = gt.Tracer({"render": {"splat": {"k_buffer_size": K}}, "model": model})
    gs = syn.SimpleGaussians(scene["density12"], feats)
    out = tr.render(gs, torch_batch(scene["batch"], "cuda"), train=True)
    rng = np.random.default_rng(8)
    g_fd = rng.normal(size=(64, 112, nr + 1)).astype(np.float32)
    t = torch.as_tensor(g_fd, device="cuda")
    ((out["pred_features"][0] * t[..., :nr]).sum() + (out["pred_opacity"][0] * t[..., nr:]).sum()).backward()
    gd, gf = gs.grads_packed()
    cfg = oracle.default_gut_config(k_buffer_size=K)
    fwd = oracle.gut_forward_nht(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], scene["density12"], feats, *scene["rays"], nht=nht)
    got = np.concatenate([out["pred_features"][0].detach().cpu().numpy(), out["pred_opacity"][0].detach().cpu().numpy()], -1)
    flips = (out["hits_count"][0].detach().cpu().numpy() != fwd["hit_count"])[..., 0]
    bad = (np.abs(got - fwd["feat_density"]) > 1e-4).any(-1)
    assert flips.mean() <= 2e-3 and (bad & ~flips).mean() <= 2e-3, f"{int(bad.sum())} pixels beyond tolerance, {int(flips.sum())} flips"
    rd, rf = oracle.gut_backward_nht(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], scene["density12"], feats, *scene["rays"], fwd, g_fd, nht=nht)
    nflip = int((flips | bad).sum())
    for key, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
        assert _trimmed_rel_err(gd[:, sl], rd[:, sl], 3 * nflip) < 1e-3, key
    assert _trimmed_rel_err(gf, rf, 3 * nflip) < 1e-3