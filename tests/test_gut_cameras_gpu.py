"""The HIP 3DGUT projection stage on the camera paths that only a GPU can execute (csrc/camera.hpp is device code): per-particle
parity of gut_project_kernel<MODEL, ROLLING> with the reference's GUTProjector::eval and with the oracle, and whole frames through the
same paths.  The cases and their CPU-side guarantees are tests/test_gut_cameras_cpu.py's.

GPU-executed branches these tests cover, none of which another test of the suite reaches:
  * relative_shutter_time for ROLLING_BOTTOM_TO_TOP and ROLLING_RIGHT_TO_LEFT (ceilf, height - ..., width - ...), on all three camera
    models (shutters-*_b2t / *_r2l, utw / utv cases, the pinhole_b2t_rot, fisheye_r2l_rot and ftheta_a2p_b2t frames);
  * project_ftheta with ftheta_reference_poly = ANGLE_TO_PIXELDIST (shutters-ftheta_l2r / _r2l, utw-ftheta_r2l, the ftheta_a2p_b2t
    frame), and the global-shutter f-theta instantiation on a whole frame (ftheta_p2a_global);
  * the unscented transform with a non-zero centre weight: ut_alpha 0.6, ut_beta 1.5, ut_kappa 1 give lambda = -1.56, ut_w0m = -1.083,
    ut_w0c = 1.057, ut_delta = 1.2 (utw-*), where the defaults give ut_w0m = 0 exactly;
  * ut_in_image_margin_factor 0 and 0.5, n_rolling_shutter_iterations 0, 1 and 2 (utv-*, rs_iter0-*, rs_iter1-*, margin0.5-*);
  * ut_require_all_sigma_points_valid: the `nvalid == 7` side of the kernel cannot be reached, because gut_create refuses the setting as
    the reference's threedgut.cuh:79 refuses to compile with it - that refusal is what is tested;
  * the end-pose fallback of project_point_with_shutter and the clip branch of project_pinhole, which
    test_gut_cameras_cpu.py::test_clouds_populate_the_end_pose_fallback_and_the_pinhole_clip_branch shows to be populated;
  * the in-kernel slerp between two sensor ORIENTATIONS, per particle in every case here (the poses of make_golden.camera_cases()
    differ by several degrees) and on whole frames (pinhole_b2t_rot, fisheye_r2l_rot).
"""
import ctypes as C
import importlib
import json

import numpy as np
import pytest

import oracle
from camera_scenes import KINDS, make_camera_path_scene
from test_gut_cameras_cpu import CASES, ORACLE_ONLY_CASES, SHUTTER_CASES, UT_CASES, comparable, golden_of, oracle_config, oracle_of, tile_cap
from test_gut_gpu import _check_grads, _image_checks, _run_oracle, torch_batch_rs
from test_oracle_cpu import _golden_camera

pytestmark = pytest.mark.gpu
syn = importlib.import_module("workloads.synthetic")


def _hip_projection(name):
    """One gut_forward of case `name` at its render.splat settings, read back through gut_debug_fetch."""
    import torch
    abi = importlib.import_module("3dgrut_amd._abi")
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    c = CASES[name]
    nat = gt._GutNative(gt.gut_config_from_conf({"render": {"splat": dict(c["splat"])}}))
    n, W, H = len(c["d12"]), c["W"], c["H"]
    frame = nat.make_frame(0, 3, n, H, W, _golden_camera(c), c["ps"], c["pe"])
    d12 = torch.as_tensor(c["d12"], device="cuda")
    sph = torch.zeros((n, 48), device="cuda")
    rays_o = torch.zeros((H, W, 3), device="cuda")
    rays_d = torch.zeros((H, W, 3), device="cuda")
    rays_d[..., 2] = 1.0
    vis = nat.trace(frame, d12, sph, rays_o, rays_d)[3]
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
    return dict(tiles=tc.cpu().numpy().view(np.uint32), pos=pp.cpu().numpy(), conic=co.cpu().numpy(), extent=ex.cpu().numpy(),
                depth=dp.cpu().numpy(), vis=vis.view(torch.int32).view(-1).cpu().numpy(), I=I,
                sorted_idx=sidx.cpu().numpy().view(np.uint32)[:I], ranges=rng.cpu().numpy().view(np.uint32))


def _deviations(got, ref_tiles, ref_pos, ref_conic, ref_extent, ref_depth, stable):
    """Worst deviations of the HIP outputs from one reference over the particles both sides see (tile counts: over all particles; the
    rest: over those that do not sit on a shutter row boundary, test_gut_cameras_cpu.py::comparable)."""
    both = (got["tiles"] > 0) & (ref_tiles > 0) & stable
    dt = np.abs(got["tiles"].astype(np.int64) - ref_tiles.astype(np.int64))
    ref_extent = np.asarray(ref_extent, np.float64)[both]
    d_ext = np.abs(got["extent"][both] - ref_extent)
    small = ref_extent <= 100.0
    b = np.asarray(ref_conic, np.float64)[both]
    return dict(both=both, visible=int((ref_tiles > 0).sum()), tiles_differ=int((dt > 0).sum()), tiles_max=int(dt.max()),
                centre=float(np.abs(got["pos"][both] - ref_pos[both]).max()),
                extent_small=float(d_ext[small].max()) if small.any() else 0.0,
                extent_large_rel=float((d_ext[~small] / ref_extent[~small]).max()) if (~small).any() else 0.0,
                extent_max=float(ref_extent.max()), d_ext=d_ext, ref_extent=ref_extent,
                conic=float((np.abs(got["conic"][both] - b) / (np.abs(b) + 1e-6)).max()),
                depth=float(np.abs(got["depth"][both] - ref_depth[both]).max() / np.abs(ref_depth[both]).max()))


def _check_projection(name):
    """The checks of test_gut_gpu.py::test_projection_and_binning_match_reference_code_golden on case `name`, against the reference's golden
    where one exists and against the float32 oracle otherwise, the float64 oracle arbitrating extents beyond 100 px.
    Measured on an MI355X over the 24 cases (per case: DESIGN.md): no tile count and no visibility flag differs, depths bit-identical,
    centres within 1.8e-4 px, extents up to 100 px within 4.1e-4 px and beyond within 2.8e-6 relative, conic terms within 1.4e-3."""
    c = CASES[name]
    n = len(c["d12"])
    got = _hip_projection(name)
    g, o32, o64 = golden_of(name), oracle_of(name), oracle_of(name, np.float64)
    if g is None:   # no build of the reference has these settings: the oracle's projection and the oracle's binning of it
        bins = oracle.gut_bin(oracle_config(c["splat"]), c["W"], c["H"], o32)
        g = dict(tiles=o32["tiles_count"], pos=o32["proj_pos"], conic=o32["conic_opacity"], extent=o32["extent"], depth=o32["depth"],
                 vis=o32["visibility"], sorted_keys=bins["sorted_keys"], sorted_idx=bins["sorted_idx"])
        vis_defined = np.ones(n, bool)
    else:           # the reference's flag is undefined where its unscented projection failed (test_gut_cameras_cpu.py): it is defined
        vis_defined = (g["tiles"] > 0) | (g["vis"] == 0)   # where it led to tiles, and where it says invisible
    stable = comparable(name)
    ref = _deviations(got, g["tiles"], g["pos"], g["conic"], g["extent"], g["depth"], stable)
    f64 = _deviations(got, o64["tiles_count"], o64["proj_pos"], o64["conic_opacity"], o64["extent"], o64["depth"], stable)
    print("PARITY " + json.dumps(dict(case=name, against="golden" if golden_of(name) is not None else "oracle32",
                                     ref={k: v for k, v in ref.items() if not isinstance(v, np.ndarray)},
                                     f64={k: v for k, v in f64.items() if not isinstance(v, np.ndarray)})))
    assert ref["visible"] >= 150
    assert ref["tiles_differ"] <= tile_cap(n) and ref["tiles_max"] <= 2, f"{ref['tiles_differ']} tile counts differ (max {ref['tiles_max']})"
    assert ref["centre"] < 2e-3, f"projected centres differ by {ref['centre']} px"
    assert ref["conic"] < 2e-3, f"conics differ by {ref['conic']} relative"
    assert ref["depth"] <= 2e-5, f"depths differ by {ref['depth']} of the largest"
    # extents: 2e-3 px up to 100 px; beyond, 2e-5 of the extent from the reference OR from the float64 oracle (test_gut_gpu.py::_check_grads'
    # arbitration: both references are float32-rounded evaluations of a quantity of hundreds of pixels)
    assert ref["extent_small"] < 2e-3, f"extents up to 100 px differ by {ref['extent_small']} px"
    both = ref["both"]
    big = ref["ref_extent"] > 100.0
    d64 = np.abs(got["extent"][both] - np.asarray(o64["extent"], np.float64)[both])
    ok = (ref["d_ext"] <= 2e-5 * ref["ref_extent"]) | (d64 <= 2e-5 * ref["ref_extent"])
    assert ok[big].all(), f"extents beyond 100 px: {int((~ok[big]).sum())} further than 2e-5 relative from both references"
    # visibility wherever the reference's flag is defined: a flag flips only where the opacity test lands on its threshold, which takes the
    # particle's tiles with it, so flips share the tile counts' cap; a particle with tiles is visible
    flips = int(((got["vis"] != 0) != (g["vis"] != 0))[vis_defined].sum())
    print(f"PARITY-VIS {name} flags differ: {flips} of {int(vis_defined.sum())} defined")
    assert flips <= tile_cap(n), f"{flips} visibility flags differ"
    assert np.all(got["vis"][got["tiles"] > 0] != 0)
    if ref["tiles_differ"] == 0:   # identical counts: the per-tile lists must be the reference's sorted lists, tile by tile
        ref_keys, ref_idx = g["sorted_keys"], g["sorted_idx"]
        assert got["I"] == len(ref_idx)
        rng_h, lst = got["ranges"], got["sorted_idx"]
        ref_tile = (ref_keys >> np.uint64(32)).astype(np.int64)
        for t in np.nonzero(rng_h[:, 1] > rng_h[:, 0])[0]:
            want = ref_idx[ref_tile == t]
            mine = lst[rng_h[t, 0]:rng_h[t, 1]]
            # equal depths (bit-identical keys) keep index order on both sides; depths may differ in the last bit
            assert set(mine.tolist()) == set(want.tolist()), f"tile {t}: different members"
            if np.array_equal(got["depth"].view(np.uint32)[want], np.asarray(g["depth"], np.float32).view(np.uint32)[want]):
                assert np.array_equal(mine, want), f"tile {t}: different order"


@pytest.mark.parametrize("name", SHUTTER_CASES)
def test_projection_matches_reference_code_golden_on_every_rolling_shutter(name):
    """gut_project_kernel against tests/golden/projector_shutters.npz: the three camera models under the left-to-right, bottom-to-top and
    right-to-left shutters (f-theta l2r / r2l with ANGLE_TO_PIXELDIST), sensor poses several degrees apart, default render.splat."""
    _check_projection(name)


@pytest.mark.parametrize("name", UT_CASES)
def test_projection_matches_reference_code_golden_at_other_unscented_transform_settings(name):
    """gut_project_kernel against tests/golden/projector_ut.npz: the reference built with ut_alpha 0.6 / ut_beta 1.5 / ut_kappa 1 (utw-*:
    the centre sigma point's weights ut_w0m, ut_w0c are non-zero and ut_delta is 1.2) and with ut_in_image_margin_factor 0 and
    n_rolling_shutter_iterations 2 (utv-*), handed to the library as the same render.splat keys."""
    _check_projection(name)


@pytest.mark.parametrize("name", ORACLE_ONLY_CASES)
def test_projection_matches_oracle_at_settings_no_reference_build_has(name):
    """n_rolling_shutter_iterations 0 and 1 and ut_in_image_margin_factor 0.5, on three rolling cases each: against the float32 oracle,
    which test_gut_cameras_cpu.py pins to the reference at the neighbouring settings and whose float64 build agrees with it in every
    tile count."""
    _check_projection(name)


def test_require_all_sigma_points_is_refused_as_the_reference_refuses_it():
    """render.splat.ut_require_all_sigma_points_valid = true: gut_config_from_conf carries it, and gut_create refuses it with BAD_INPUT
    (include/grut_amd.h: must be 0) - the reference's threedgut.cuh:79 static_asserts RequireAllSigmaPoints == false, so no build of it
    runs that way either.  No frame can therefore reach the kernel's `nvalid == 7` rule."""
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    cfg = gt.gut_config_from_conf({"render": {"splat": {"ut_require_all_sigma_points_valid": True}}})
    assert cfg.ut_require_all_sigma_points_valid == 1
    with pytest.raises(RuntimeError, match="BAD_INPUT.*ut_require_all_sigma_points_valid"):
        gt._GutNative(cfg)


@pytest.mark.parametrize("kind", KINDS)
def test_frames_through_the_new_camera_paths_match_oracle(kind):
    """Whole frames, forward and backward (tests/camera_scenes.py): a distorted pinhole read bottom-to-top while the sensor turns ~3 degrees
    and moves, a fisheye read right-to-left while it turns, f-theta ANGLE_TO_PIXELDIST read bottom-to-top, and f-theta PIXELDIST_TO_ANGLE
    under a global shutter (the one projection instantiation no other frame-level test runs)."""
    import torch
    scene = make_camera_path_scene(kind)
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
    I, I_ref = int(tr.tracer_wrapper.stats().num_intersections), ora["fwd"]["bins"]["num_intersections"]
    print("FRAME " + json.dumps(dict(kind=kind, intersections=I, oracle_intersections=int(I_ref))))
    _image_checks(out, ora["fwd"], max_flip_frac=5e-3)
    assert I_ref > 1000 and abs(I - I_ref) <= max(4, 2e-3 * I_ref)
    _check_grads(scene, gpu, ora, g_fd, g_dist)
