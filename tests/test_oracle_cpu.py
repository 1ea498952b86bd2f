"""CPU: pins the oracle (oracle/*.c, the CPU restatement used as checker) to the REFERENCE's own per-hit math.

tests/golden/per_hit_deg{2,4}.npz were produced by the reference's source headers compiled on the host
(tests/golden/make_golden.py, oracle/ref/), and so was tests/golden/gut_hit_seed77.npz; where oracle/_ref/ is built, that
library is also called live on the same cases.  Further CPU checks: analytic backward of the oracle against central finite differences
of its own forward in float64, and basic invariants of the binning restatement.
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

import oracle
from parity_util import unsigned_only_pair
from scenes import make_scene, rel_err

HERE = os.path.dirname(os.path.abspath(__file__))
syn = importlib.import_module("workloads.synthetic")


def _golden(degree):
    return np.load(os.path.join(HERE, "golden", f"per_hit_deg{degree}.npz"))


def _close(a, b, rtol=2e-5, atol=2e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= atol + rtol * np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("degree", [2, 4])
def test_gut_per_hit_forward_matches_reference_vectors(degree):
    g = _golden(degree)
    mr, ma = float(g["params"][0]), float(g["params"][1])
    n = g["ray_o"].shape[0]
    for i in range(n):
        acc, st = oracle.gut_process_hit_fwd(degree, mr, ma, 0.99, g["ray_o"][i], g["ray_d"][i], g["density12"][i], g["feat3"][i],
                                             g["state5"][i])
        assert acc == int(g["gut_fwd_accept"][i]), i
        assert _close(st, g["gut_fwd_state"][i]), (i, st, g["gut_fwd_state"][i])
    assert g["gut_fwd_accept"].sum() > n // 2


@pytest.mark.parametrize("degree", [2, 4])
def test_gut_per_hit_backward_matches_reference_vectors(degree):
    g = _golden(degree)
    mr, ma, mt = float(g["params"][0]), float(g["params"][1]), float(g["params"][2])
    worst = 0.0
    for i in range(g["ray_o"].shape[0]):
        st, gd, gf = oracle.gut_process_hit_bwd(degree, mr, ma, 0.99, mt, g["ray_o"][i], g["ray_d"][i], g["density12"][i], g["feat3"][i],
                                                g["state5"][i], g["fin5"][i], g["grads5"][i])
        assert _close(st, g["gut_bwd_state"][i]), i
        ref = np.concatenate([g["gut_g_density12"][i], g["gut_g_feat3"][i]]).astype(np.float64)
        got = np.concatenate([gd, gf]).astype(np.float64)
        scale = np.abs(ref).max() + 1e-20
        worst = max(worst, np.abs(got - ref).max() / scale)
    # identical formulas in the same arithmetic type: agreement to float rounding of the largest component
    assert worst < 2e-4, worst


def test_sh_radiance_matches_reference_vectors():
    g = _golden(2)
    for i in range(0, g["ray_o"].shape[0], 4):
        for deg in range(4):
            got = oracle.sh_radiance(deg, g["sph48"][i], g["ray_d"][i], clamped=True)
            assert _close(got, g["sh_radiance"][deg, i], rtol=1e-5, atol=1e-6), (i, deg)


def test_gut_per_hit_live_against_reference_library():
    """200 random cases (seed 77) against the reference library's answers stored in tests/golden/gut_hit_seed77.npz
    (make_golden.py --only=gut_hit_seed77); where oracle/_ref/ is built, the library is also called live on the same cases."""
    g = np.load(os.path.join(HERE, "golden", "gut_hit_seed77.npz"))
    lib = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libref_gut_hit_deg2.so")
    ref = C.CDLL(lib) if os.path.exists(lib) else None
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fl = C.c_float
    assert g["ray_o"].shape[0] == 200
    for i in range(g["ray_o"].shape[0]):
        ro, rd, d12, feat, st0 = (np.ascontiguousarray(g[k][i]) for k in ("ray_o", "ray_d", "density12", "feat3", "state5"))
        acc_ref, st_ref = int(g["ref_accept"][i]), g["ref_state5"][i]
        if ref is not None:
            st_live = st0.copy()
            assert ref.ref_gut_process_hit_fwd(p(ro), p(rd), p(d12), p(feat), fl(0.0113), fl(1 / 255), p(st_live)) == acc_ref
            assert np.array_equal(st_live, st_ref), i
        acc, st = oracle.gut_process_hit_fwd(2, 0.0113, 1 / 255, 0.99, ro, rd, d12, feat, st0)
        assert acc == acc_ref and _close(st, st_ref), i


def _fd_check(scene, n_probe=12, eps=1e-6, **cfg_kw):
    """Oracle analytic gradient vs central differences of the oracle forward, float64, scalar loss <g, image>."""
    cfg = oracle.default_gut_config(**cfg_kw)
    W, H = scene["W"], scene["H"]
    g_fd, g_dist = syn.upstream_grads(W, H)
    g_fd = g_fd.astype(np.float64) * W * H
    g_dist = (np.random.default_rng(9).normal(size=g_dist.shape) * 0.05).astype(np.float64)
    d12 = scene["density12"].astype(np.float64)
    sph = scene["sph"].astype(np.float64)

    def loss(d, s):
        f = oracle.gut_forward(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], 3, d, s, *scene["rays"], dtype=np.float64)
        return float((f["feat_density"] * g_fd).sum() + (np.where(f["hit_distance"] < 1e5, f["hit_distance"], 0) * g_dist).sum()), f

    _, fwd = loss(d12, sph)
    gd, gsph, _ = oracle.gut_backward(cfg, scene["cam"], 3, fwd, g_fd, g_dist, dtype=np.float64)
    rng = np.random.default_rng(2)
    vis = np.nonzero(fwd["proj"]["tiles_count"] > 0)[0]
    errs = []
    for _ in range(n_probe):
        i = int(rng.choice(vis))
        for col in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10):
            dp, dm = d12.copy(), d12.copy()
            h = eps * max(1.0, abs(d12[i, col]))
            dp[i, col] += h
            dm[i, col] -= h
            fdiff = (loss(dp, sph)[0] - loss(dm, sph)[0]) / (2 * h)
            errs.append((abs(fdiff - gd[i, col]), abs(gd[i, col]), i, col))
    return errs, np.abs(gd).max(0)


def test_oracle_backward_is_the_gradient_of_oracle_forward():
    """No gradient flows through the 2-D projection in the reference (only via the per-particle radiance direction and
    the 3-D per-ray response), and the binning is piecewise constant, so finite differences of the full forward must
    reproduce the analytic backward wherever no accept/reject threshold is crossed."""
    scene = make_scene(n=300, width=32, height=32, median_scale=0.12, max_density=0.6)
    errs, colmax = _fd_check(scene)
    bad = [e for e in errs if e[0] > 2e-4 * max(colmax[e[3]], 1e-12) + 1e-7]
    # a probe may straddle a threshold (hit accepted on one side only): allow a small fraction of outliers
    assert len(bad) <= max(2, len(errs) // 20), bad[:5]


def test_oracle_kbuffer_backward_is_the_gradient_of_kbuffer_forward():
    """K = 16 "sorted" mode (gutKBufferRenderer.cuh:62-122, 158-198): the restated Slang reverse-mode of the back-to-front
    lerp form against finite differences of the k-buffer forward."""
    scene = make_scene(n=300, width=32, height=32, median_scale=0.12, max_density=0.6)
    errs, colmax = _fd_check(scene, k_buffer_size=16)
    bad = [e for e in errs if e[0] > 2e-4 * max(colmax[e[3]], 1e-12) + 1e-7]
    assert len(bad) <= max(2, len(errs) // 20), bad[:5]
    # and the sorted forward differs from the unsorted one only where centre-depth order and hit order disagree
    cfg0, cfg16 = oracle.default_gut_config(), oracle.default_gut_config(k_buffer_size=16)
    a = oracle.gut_forward(cfg0, scene["cam"], scene["pose_start"], scene["pose_end"], 3, scene["density12"], scene["sph"], *scene["rays"])
    b = oracle.gut_forward(cfg16, scene["cam"], scene["pose_start"], scene["pose_end"], 3, scene["density12"], scene["sph"], *scene["rays"])
    d = np.abs(a["feat_density"] - b["feat_density"]).max()
    assert 0 < d < 0.5
    np.testing.assert_allclose(a["feat_density"][..., 3], b["feat_density"][..., 3], atol=2e-5)  # opacity is order independent


def test_binning_restatement_invariants():
    scene = make_scene(n=3000, width=96, height=64, median_scale=0.06)
    cfg = oracle.default_gut_config()
    fwd = oracle.gut_forward(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], 3, scene["density12"], scene["sph"], *scene["rays"])
    b, proj = fwd["bins"], fwd["proj"]
    assert b["num_intersections"] == int(proj["tiles_count"].sum()) > 0
    keys = b["sorted_keys"]
    assert np.all(keys[1:] >= keys[:-1])
    tiles = (keys >> np.uint64(32)).astype(np.int64)
    lens = (b["tile_ranges"][:, 1].astype(np.int64) - b["tile_ranges"][:, 0])
    assert lens.sum() == b["num_intersections"]
    assert np.array_equal(np.bincount(tiles, minlength=len(lens)), lens)
    # depth bits of each entry equal the particle's view depth
    dbits = proj["depth"].astype(np.float32).view(np.uint32)
    assert np.array_equal((keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), dbits[b["sorted_idx"]])
    assert oracle.lib().orc_higher_msb(C.c_uint32(24)) == 5 and oracle.lib().orc_higher_msb(C.c_uint32(8160)) == 13


def test_empty_scene_outputs_keep_initial_values():
    scene = make_scene(n=16, width=16, height=16)
    scene["density12"][:, 3] = 0.0
    fwd = oracle.gut_forward(oracle.default_gut_config(), scene["cam"], scene["pose_start"], scene["pose_end"], 3, scene["density12"],
                             scene["sph"], *scene["rays"])
    assert fwd["bins"]["num_intersections"] == 0
    assert np.all(fwd["feat_density"] == 0) and np.all(fwd["hit_distance"] == np.float32(1e6))


# ------------------------------------------------------------------------------------------
# 3DGRT oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [2, 4])
def test_grt_per_hit_matches_reference_vectors(degree):
    g = _golden(degree)
    mr, ma, mt = float(g["params"][0]), float(g["params"][1]), float(g["params"][3])
    worst = 0.0
    for i in range(g["ray_o"].shape[0]):
        st0 = np.concatenate([g["state5"][i], np.zeros(3, np.float32)])
        acc, st = oracle.grt_process_hit_fwd(degree, mr, ma, 0.99, g["ray_o"][i], g["ray_d"][i], g["density12"][i], g["sph48"][i], 3, True, st0)
        assert acc == int(g["grt_fwd_accept"][i]), i
        assert _close(st[:5], g["grt_fwd_state"][i][:5]), (i, st, g["grt_fwd_state"][i])
        assert _close(st[5:], g["grt_fwd_state"][i][5:], rtol=2e-4, atol=1e-5), (i, st[5:], g["grt_fwd_state"][i][5:])
        s5, gd, gs = oracle.grt_process_hit_bwd(degree, mr, ma, 0.99, mt, g["ray_o"][i], g["ray_d"][i], g["density12"][i], g["sph48"][i], 3,
                                                g["state5"][i], g["fin5"][i], g["grads5"][i])
        assert _close(s5, g["grt_bwd_state"][i]), i
        ref = np.concatenate([g["grt_g_density12"][i], g["grt_g_sph48"][i]]).astype(np.float64)
        got = np.concatenate([gd, gs]).astype(np.float64)
        worst = max(worst, np.abs(got - ref).max() / (np.abs(ref).max() + 1e-20))
    assert worst < 2e-4, worst


def test_grt_instance_intersection_matches_reference_vectors():
    g = _golden(4)
    for i in range(g["ray_o"].shape[0]):
        ok, t = oracle.grt_intersect_instance(g["instance_ray"][i, :3], g["instance_ray"][i, 3:], 0.0, 1e6, 1.0)
        assert ok == int(g["instance_ok"][i]), i
        assert _close(t, g["instance_t"][i], rtol=1e-6, atol=1e-7), (i, t, g["instance_t"][i])


def test_grt_kernel_scale_known_values():
    """particlePrimitives.cu:27-51: r with exp(a r^b) = min_response, a = -4.5/3^b (~3.0 deg 4 / 2.99 deg 2)."""
    assert oracle.grt_kernel_scale(0.5, 0.0113, False, 4) == pytest.approx((np.log(0.0113) / (-4.5 / 81)) ** 0.25, rel=1e-6)
    assert oracle.grt_kernel_scale(0.5, 0.0113, False, 2) == pytest.approx((np.log(0.0113) / (-0.5)) ** 0.5, rel=1e-6)
    # density clamping: min response modulated by the density, capped at 0.97
    assert oracle.grt_kernel_scale(0.5, 0.0113, True, 4) == pytest.approx((np.log(0.0226) / (-4.5 / 81)) ** 0.25, rel=1e-6)
    assert oracle.grt_kernel_scale(0.005, 0.0113, True, 4) == pytest.approx((np.log(0.97) / (-4.5 / 81)) ** 0.25, rel=1e-5)


def _grt_scene(n=400, w=24, h=16):
    scene = make_scene(n=n, width=w, height=h, median_scale=0.12, max_density=0.7)
    T = scene["batch"]["T_to_world"][0]
    return scene, T


def test_grt_forward_orders_hits_and_matches_brute_force_compositing():
    scene, T = _grt_scene()
    cfg = oracle.default_grt_config()
    out = oracle.grt_forward(cfg, scene["density12"], scene["sph"], 3, 1e-3, T, *scene["rays"], dbg_cap=256)
    assert out["density"].max() > 0.3 and out["hit_count"].max() >= 2
    # hit lists: every processed candidate appears once per ray (distances increase strictly round to round)
    for r in range(0, out["hit_ids"].shape[0], 7):
        ids = out["hit_ids"][r, : out["hit_num"][r]]
        assert len(set(ids.tolist())) == len(ids)
    # visibility = particles with at least one accepted hit
    assert out["visibility"].sum() > 0
    # two cameras' worth of sanity: opacity within [0,1], depth non-negative
    assert np.all(out["density"] >= 0) and np.all(out["density"] <= 1) and np.all(out["hit_distance"][..., 0] >= 0)


@pytest.mark.parametrize("prim", [0, 6])
def test_grt_sequence_compositor_reproduces_the_forward_and_moves_with_the_order(prim):
    """oracle.grt_composite_sequence (round 6; the GPU tests use it to identify order ties against the reference programs' goldens): a ray's
    processed-particle sequence composited hit by hit by the checker's processHit gives the checker's own forward outputs - radiance, opacity,
    integrated distance, accepted-hit count - for the volumetric particles and for the surfels; and the same hits in another order give another
    colour (what a tie against the reference does) at the same opacity."""
    scene, T = _grt_scene(n=600)
    cfg = oracle.default_grt_config(primitive_type=prim)
    out = oracle.grt_forward(cfg, scene["density12"], scene["sph"], 3, 1e-3, T, *scene["rays"], dbg_cap=256)
    M = np.asarray(T, np.float32)[:3, :4]
    ro, rd = (a.reshape(-1, 3) for a in scene["rays"])
    checked = moved = 0
    for r in np.argsort(-out["hit_num"])[:12]:
        n = int(out["hit_num"][r])
        if n < 2:
            continue
        seq = out["hit_ids"][r, :n]
        o_w, d_w = (M[:, :3] @ ro[r] + M[:, 3]).astype(np.float32), (M[:, :3] @ rd[r]).astype(np.float32)
        rgb, opa, dist, acc = oracle.grt_composite_sequence(cfg, 1e-3, o_w, d_w, scene["density12"], scene["sph"], 3, seq)
        assert np.abs(rgb - out["features"].reshape(-1, 3)[r]).max() < 2e-6 and abs(opa - out["density"].reshape(-1)[r]) < 2e-6
        assert abs(dist - out["hit_distance"].reshape(-1, 2)[r, 0]) < 1e-5 and acc == int(out["hit_count"].reshape(-1)[r])
        checked += 1
        rgb2, opa2, _, _ = oracle.grt_composite_sequence(cfg, 1e-3, o_w, d_w, scene["density12"], scene["sph"], 3, seq[::-1])
        moved += int(np.abs(rgb2 - rgb).max() > 1e-5)
        if opa < 0.99:   # nothing terminates either way: the product of the transmittances does not depend on the order
            assert abs(opa2 - opa) < 1e-5
    assert checked >= 6 and moved >= 3


def test_grt_backward_is_the_gradient_of_forward_away_from_the_last_hit():
    """Finite differences of the f64 oracle forward reproduce its analytic backward, except for the reference's own quirk
    that the backward replay excludes the hit AT the saved last-hit distance (endT = tLast + 1e-9, strict compare,
    referenceBwdOptix.cu:126-131); rays that do not saturate process every candidate, and for those the last candidate
    is the one dropped, so the probe compares against a loss whose rays saturate early is avoided by low densities."""
    scene, T = _grt_scene(n=150, w=12, h=8)
    scene["density12"][:, 3] *= 0.5
    cfg = oracle.default_grt_config()
    d12, sph = scene["density12"].astype(np.float64), scene["sph"].astype(np.float64)
    H, W = 8, 12
    rng = np.random.default_rng(3)
    g_rad, g_dns, g_hit = rng.normal(size=(H, W, 3)), rng.normal(size=(H, W, 1)), rng.normal(size=(H, W, 1)) * 0.1

    def run(d):
        return oracle.grt_forward(cfg, d, sph, 3, 1e-3, T, *scene["rays"], dbg_cap=512, dtype=np.float64)

    f0 = run(d12)
    gd, gs = oracle.grt_backward(cfg, 3, 1e-3, f0, g_rad, g_dns, g_hit, dtype=np.float64)
    # the quirk: contributions of each ray's last processed candidate are missing from gd; measure FD on a loss that
    # masks them out is impractical, so check only particles that are never the last candidate of any ray
    last = set()
    for r in range(H * W):
        k = int(f0["hit_num"][r])
        if k:
            last.add(int(f0["hit_ids"][r, k - 1]))
    probes = [i for i in np.nonzero(np.abs(gd).sum(1) > 0)[0] if i not in last][:6]
    assert probes

    def loss(d):
        f = run(d)
        return float((f["features"] * g_rad).sum() + (f["density"] * g_dns).sum() + (f["hit_distance"][..., :1] * g_hit).sum())

    bad = 0
    for i in probes:
        for col in range(11):
            h = 1e-6 * max(1.0, abs(d12[i, col]))
            dp, dm = d12.copy(), d12.copy()
            dp[i, col] += h
            dm[i, col] -= h
            fd = (loss(dp) - loss(dm)) / (2 * h)
            if abs(fd - gd[i, col]) > 2e-4 * np.abs(gd[:, col]).max() + 1e-7:
                bad += 1
    # a probe particle still influences the (dropped) last hits of rays it precedes through their transmittance
    assert bad <= len(probes) * 11 // 4, bad


# ---- SelectiveAdam -------------------------------------------------------------------------------
def test_adam_oracle_matches_reference_kernel_golden():
    """oracle/adam_oracle.py against three consecutive steps of the reference's own selective_adam_update_kernel
    (tests/golden/adam.npz, produced by oracle/ref/ref_adam.cpp): bit-exact, invisible rows untouched."""
    from oracle import adam_oracle
    g = np.load(os.path.join(HERE, "golden", "adam.npz"))
    for M in (1, 3, 4, 45):
        lr, b1, b2, eps = g[f"M{M}_hyper"]
        p = g[f"M{M}_p0"]
        m = np.zeros_like(p)
        v = np.zeros_like(p)
        for step in range(3):
            vis = g[f"M{M}_vis{step}"]
            p1, m1, v1 = adam_oracle.selective_adam_update(p, g[f"M{M}_g{step}"], m, v, vis, lr, b1, b2, eps)
            assert np.array_equal(p1[~vis], p[~vis]) and np.array_equal(m1[~vis], m[~vis])
            assert np.array_equal(p1, g[f"M{M}_p{step + 1}"]), f"M={M} step {step}: parameter differs"
            assert np.array_equal(m1, g[f"M{M}_m{step + 1}"]) and np.array_equal(v1, g[f"M{M}_v{step + 1}"])
            p, m, v = p1, m1, v1
        assert 0.3 < vis.mean() < 0.9


# ---- camera models / rolling shutter / pose math against the reference's own code ---------------------------------
def _golden_camera(c):
    """GrutCamera of a make_golden.camera_cases() entry."""
    import importlib
    abi = importlib.import_module("3dgrut_amd._abi")
    cam = abi.GrutCamera()
    cam.model, cam.shutter, cam.width, cam.height = c["model"], c["shutter"], c["W"], c["H"]
    prm = c["prm"]
    for i in range(2):
        cam.principal_point[i] = prm[i]; cam.focal_length[i] = prm[2 + i]; cam.tangential[i] = prm[10 + i]
    for i in range(6):
        cam.radial[i] = prm[4 + i]; cam.ftheta_pixeldist_to_angle[i] = prm[18 + i]; cam.ftheta_angle_to_pixeldist[i] = prm[24 + i]
    for i in range(4):
        cam.thin_prism[i] = prm[12 + i]
    cam.max_angle = prm[16]
    cam.ftheta_reference_poly = int(prm[17])
    for i in range(3):
        cam.ftheta_linear_cde[i] = prm[30 + i]
    return cam


def test_camera_projection_matches_reference_code_golden():
    """project_point_with_shutter / pose_inverse / pose_interpolate of the oracle against tests/golden/camera.npz, which the
    reference's cameraProjections.cuh + sensors.h produced on the host (oracle/ref/ref_camera.cpp): three camera models x
    five shutter types, 160 points each, with and without rolling-shutter iterations."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    g = np.load(os.path.join(HERE, "golden", "camera.npz"))
    worst, flips, total = 0.0, 0, 0
    for k, c in enumerate(make_golden.camera_cases()):
        cam = _golden_camera(c)
        for n_iter in (5, 0):
            ref_xy, ref_ok = g[f"c{k}_xy{n_iter}"], g[f"c{k}_ok{n_iter}"].astype(bool)
            for i, p in enumerate(c["pts"]):
                ok, xy = oracle.kat_project_point_with_shutter(cam, c["ps"], c["pe"], n_iter, p, 0.1)
                total += 1
                if ok != ref_ok[i]:
                    flips += 1      # a point exactly on a validity threshold may land on either side
                    continue
                if ok:
                    worst = max(worst, float(np.abs(xy - ref_xy[i]).max()))
        assert np.abs(oracle.kat_pose_inverse(c["ps"]) - g[f"c{k}_inv"]).max() < 2e-6, f"case {k}: pose inverse"
        assert np.abs(oracle.kat_pose_interpolate(c["ps"], c["pe"], 0.37) - g[f"c{k}_mid"]).max() < 2e-6, f"case {k}: pose interpolation"
    assert flips <= 2e-3 * total, f"{flips} of {total} validity flags differ"
    assert worst < 2e-3, f"projected pixel positions differ by up to {worst} px"


def test_projection_stage_matches_reference_code_golden():
    """orc_gut_project against tests/golden/projector.npz = the reference's GUTProjector::eval run on the host
    (oracle/ref/ref_projector.cpp): unscented transform through all three camera models, conic / extent, tile box and the
    per-tile culling count, depth and visibility of 700 particles per case."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    g = np.load(os.path.join(HERE, "golden", "projector.npz"))
    cfg = oracle.default_gut_config()
    for k, c in enumerate(make_golden.projector_cases()):
        cam = _golden_camera(c)
        n = len(c["d12"])
        o = oracle.gut_project(cfg, cam, c["ps"], c["pe"], 3, c["d12"], np.zeros((n, 48), np.float32))
        tiles, vis = g[f"p{k}_tiles"], g[f"p{k}_vis"]
        # visibility = validity of the conic estimate (gutProjector.cuh:275).  When the unscented projection itself failed the
        # reference evaluates that estimate on an UNINITIALISED covariance (:246-272), so its flag is undefined there; the
        # oracle (and the HIP path) report 0.  Wherever the oracle says visible the reference must agree.
        assert np.all(vis[o["visibility"] != 0] != 0), f"case {k}: oracle-visible particles the reference calls invisible"
        assert np.all(o["visibility"][tiles > 0] != 0) and np.all(vis[tiles > 0] != 0)
        both = (tiles > 0) & (o["tiles_count"] > 0)
        # a tile whose minimal power lands exactly on the threshold may be counted on either side
        dt = np.abs(o["tiles_count"].astype(np.int64) - tiles.astype(np.int64))
        assert (dt > 0).sum() <= max(2, 0.01 * n) and dt.max() <= 2, f"case {k}: tile counts differ ({(dt > 0).sum()} particles, max {dt.max()})"
        assert both.sum() > 100
        for name, key, tol in (("proj_pos", "pos", 1e-3), ("extent", "extent", 1e-3), ("depth", "depth", 1e-5)):
            a, b = o[name][both], g[f"p{k}_{key}"][both]
            assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), f"case {k}: {name} differs by {np.abs(a - b).max()}"
        a, b = o["conic_opacity"][both], g[f"p{k}_conic"][both]
        assert (np.abs(a - b) / (np.abs(b) + 1e-6)).max() < 1e-3, f"case {k}: conic / opacity"
        # binning on the REFERENCE's projection outputs: expansion keys (tile << 32 | depth bits), padding and the stable
        # sort order must come out identical to GUTProjector::expand + a stable sort by key
        proj = dict(tiles_count=tiles, proj_pos=g[f"p{k}_pos"], conic_opacity=g[f"p{k}_conic"], extent=g[f"p{k}_extent"], depth=g[f"p{k}_depth"])
        bins = oracle.gut_bin(cfg, c["W"], c["H"], proj)
        assert bins["num_intersections"] == int(tiles.sum()) == len(g[f"p{k}_sorted_keys"])
        assert np.array_equal(bins["sorted_keys"], g[f"p{k}_sorted_keys"]), f"case {k}: sorted keys differ"
        assert np.array_equal(bins["sorted_idx"], g[f"p{k}_sorted_idx"]), f"case {k}: sorted particle lists differ"


def test_grt_proxies_match_reference_kernels_golden():
    """kernelScale and the proxy geometry of the 3DGRT oracle against tests/golden/grt_proxies.npz, which the reference's own
    kernels produced (threedgrt_tracer/src/particlePrimitives.cu run on the host, oracle/ref/ref_grt_proxies.cpp)."""
    g = np.load(os.path.join(HERE, "golden", "grt_proxies.npz"))
    for deg in (0, 1, 2, 3, 4, 5, 8):
        for clamp in (0, 1):
            got = np.array([oracle.grt_kernel_scale(float(d), 0.0113, clamp, deg) for d in g["ks_density"]], np.float32)
            ref = g[f"ks_deg{deg}_c{clamp}"]
            assert np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max(), f"kernelScale degree {deg} clamping {clamp}"
    pos, rot, scl, dns = g["px_pos"], g["px_rot"], g["px_scl"], g["px_dns"]
    for deg, clamp in ((4, 1), (2, 0)):
        cfg = oracle.default_grt_config(particle_kernel_degree=deg, particle_kernel_density_clamping=clamp)
        pr = oracle.grt_proxies(cfg, pos, rot, scl, dns)
        T = g[f"px_deg{deg}_c{clamp}_transform"].reshape(-1, 3, 4).astype(np.float64)    # object -> world: [R diag(kscl) | mu]
        W = pr["inst"][:, :9].reshape(-1, 3, 3).astype(np.float64)                       # world -> object rows
        mu = pr["inst"][:, 9:12].astype(np.float64)
        assert np.abs(mu - T[:, :, 3]).max() == 0.0
        eye = np.einsum("nij,njk->nik", W, T[:, :, :3])
        assert np.abs(eye - np.eye(3)).max() < 5e-6, "the oracle's inverse instance map does not invert the reference's instance transform"
        # the oracle's world boxes are the reference's, padded by a hair (culling must stay conservative)
        ref_box = g[f"px_deg{deg}_c{clamp}_aabb"]
        ext = (ref_box[:, 3:] - ref_box[:, :3]).max(1, keepdims=True)
        assert np.all(pr["aabb"][:, :3] <= ref_box[:, :3] + 1e-7) and np.all(pr["aabb"][:, 3:] >= ref_box[:, 3:] - 1e-7)
        assert np.abs(pr["aabb"] - ref_box).max() <= 2e-4 * ext.max() + 2e-5


def test_grt_trace_rounds_match_reference_programs_golden():
    """The oracle's 3DGRT forward and backward against tests/golden/grt_trace.npz = the reference's own OptiX programs
    (referenceOptix.cu / referenceBwdOptix.cu: raygen round loop, intersection, any-hit k-buffer, processHit(Bwd)) run on
    the host over an emulated traversal (oracle/ref/ref_grt_trace*.cpp).  Images, hit counts, visibility and all particle
    gradients — up to 74 accepted hits per ray."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    g = np.load(os.path.join(HERE, "golden", "grt_trace.npz"))
    cfg = oracle.default_grt_config(enable_normals=1)   # the golden library is built with ENABLE_NORMALS / ENABLE_HIT_COUNTS
    for k, kw in enumerate(make_golden.GRT_TRACE_SCENES):
        sc = make_scene(**kw)
        H, W = kw["height"], kw["width"]
        o = oracle.grt_forward(cfg, sc["density12"], sc["sph"], 3, 1e-3, sc["batch"]["T_to_world"][0], *sc["rays"])
        assert np.array_equal(o["hit_count"], g[f"s{k}_hits_count"]), f"scene {k}: accepted-hit counts differ"
        assert np.array_equal(o["visibility"] != 0, g[f"s{k}_visibility"] != 0)
        assert np.abs(o["features"] - g[f"s{k}_features"]).max() < 2e-6 and np.abs(o["density"] - g[f"s{k}_density"]).max() < 2e-6
        assert np.abs(o["normals"] - g[f"s{k}_normals"]).max() < 5e-6
        hd = g[f"s{k}_hit_distance"]
        assert np.abs(o["hit_distance"] - hd).max() <= 5e-6 * max(1.0, np.abs(hd).max())
        assert g[f"s{k}_hits_count"].max() >= 20
        # the other legal OptiX outcome (box test against the ray's already shrunk far end, i.e. a traversal that reaches a
        # proxy whose hit precedes its box late): a few rays lose one hit — order-dependent in the reference, bounded here
        other = g[f"s{k}_hits_count_shrunk_tmax"]
        assert (other != g[f"s{k}_hits_count"]).mean() < 0.05 and np.abs(other - g[f"s{k}_hits_count"]).max() <= 1
        g_rad, g_dns, g_hit = make_golden.grt_trace_upstream(H, W)
        gd, gs = oracle.grt_backward(cfg, 3, 1e-3, o, g_rad, g_dns, g_hit)
        rd, rs = g[f"s{k}_grad_density"], g[f"s{k}_grad_sph"]
        for name, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
            assert rel_err(gd[:, sl], rd[:, sl]) < 1e-4, f"scene {k}: grad {name} {rel_err(gd[:, sl], rd[:, sl]):.2e}"
        assert rel_err(gs, rs) < 1e-4, f"scene {k}: grad sph"


@pytest.mark.parametrize("prim", ["icosahedron", "octahedron", "tetrahedron", "diamond"])
def test_grt_mesh_proxies_match_reference_programs_golden(prim):
    """render.primitive_type = icosahedron (the paper's configuration) / octahedron / tetrahedron / diamond: the oracle with the particle
    offered at the distance at which the ray ENTERS the proxy polyhedron (a clip against its face planes in the proxy's own frame,
    oracle/orc_polyhedra.h) against tests/golden/grt_trace_mesh.npz = the reference's forward and backward programs compiled for that
    primitive type over the emulated OptiX, which walks the TRIANGLES the reference's own mesh kernel wrote (Moeller-Trumbore, back faces
    culled).  Two roundings of the same entry distance: a ray's hit sequence may swap two hits whose distances tie to rounding."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    g = np.load(os.path.join(HERE, "golden", "grt_trace_mesh.npz"))
    code = make_golden.MESH_PRIMITIVES[prim][0]
    cfg = oracle.default_grt_config(primitive_type=code)
    for k, kw in enumerate(make_golden.GRT_TRACE_SCENES[:2 if prim == "icosahedron" else 1]):
        sc = make_scene(**kw)
        H, W = kw["height"], kw["width"]
        o = oracle.grt_forward(cfg, sc["density12"], sc["sph"], 3, 1e-3, sc["batch"]["T_to_world"][0], *sc["rays"])
        ref_cnt = g[f"{prim}_s{k}_hits_count"]
        flips = (o["hit_count"] != ref_cnt)[..., 0]
        assert flips.mean() <= 0.01 and ref_cnt.max() >= 20, f"{prim} scene {k}: {int(flips.sum())} rays with another number of accepted hits"
        ok = ~flips
        e = np.abs(o["features"] - g[f"{prim}_s{k}_features"]).max(-1)
        hd = g[f"{prim}_s{k}_hit_distance"]
        e_depth = np.abs(o["hit_distance"] - hd)[..., 0]
        tied = ok & ((e > 1e-5) | (e_depth > 2e-5 * max(1.0, np.abs(hd).max())))          # same count, other order of two hits that tie to rounding
        assert tied.mean() <= 0.02 and (not tied.any() or (e[tied].max() < 2e-2 and e_depth[tied].max() < 2e-2)), f"{prim} scene {k}: {int(tied.sum())} rays differ with the same hit count"
        ok = ok & ~tied
        assert np.abs(o["density"] - g[f"{prim}_s{k}_density"])[ok].max() < 1e-5
        # the last ENTRY distance: world-space triangles of float32 vertices there, the ideal polyhedron in the proxy's frame here - a
        # grazing entry amplifies the vertices' rounding by 1 / |n . d|
        assert np.abs(o["hit_distance"] - hd)[..., 1][ok].max() <= 1e-3 and np.median(np.abs(o["hit_distance"] - hd)[..., 1][ok]) <= 2e-6
        assert ((o["visibility"] != 0) != (g[f"{prim}_s{k}_visibility"] != 0)).sum() <= 3 * int((flips | tied).sum())
        g_rad, g_dns, g_hit = make_golden.grt_trace_upstream(H, W)
        gd, gs = oracle.grt_backward(cfg, 3, 1e-3, o, g_rad, g_dns, g_hit)
        rd, rs = g[f"{prim}_s{k}_grad_density"], g[f"{prim}_s{k}_grad_sph"]
        ndrop = 3 * int((flips | tied).sum())
        per = np.abs(gd[:, :11].astype(np.float64) - rd[:, :11]).max(1)
        per = np.sort(per)[: max(1, len(per) - ndrop)]
        assert per.max() / np.abs(rd[:, :11]).max() < 2e-4, f"{prim} scene {k}: particle gradients"
        per = np.sort(np.abs(gs.astype(np.float64) - rs).max(1))[: max(1, len(gs) - ndrop)]
        assert per.max() / np.abs(rs).max() < 2e-4, f"{prim} scene {k}: SH gradients"
    # the proxies' world boxes contain the reference's mesh vertices (what the software BVH is built over)
    sc = make_scene(**make_golden.GRT_TRACE_SCENES[0])
    d12 = sc["density12"]
    prox = oracle.grt_proxies(cfg, d12[:, 0:3], d12[:, 4:8], d12[:, 8:11], d12[:, 3])
    box = g[f"{prim}_s0_scene_box"]
    assert (prox["scene"][:3] <= box[:3] + 1e-5).all() and (prox["scene"][3:] >= box[3:] - 1e-5).all()
    assert (prox["scene"][3:] - prox["scene"][:3] <= (box[3:] - box[:3]) * 1.8).all()


def test_grt_trisurfel_checker_matches_reference_programs_golden():
    """render.primitive_type = trisurfel (provided by the HIP plugin since round 5: tests/test_grt_gpu.py::test_trisurfel_*); this pins the
    CHECKER for it: the reference's forward / backward programs compiled with PARTICLE_PRIMITIVE_TYPE =
    MOGTracingTriSurfel (the surfel branches of processHit / processHitBwd, no face culling) over the emulated OptiX walking the two triangles
    per particle the reference's trisurfel kernel wrote, against the oracle (rhombus |x| + |y| <= sqrt 2 in the proxy's z = 0 plane, plane
    crossing as the hit, orc_grt: g_prim 6)."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    g = np.load(os.path.join(HERE, "golden", "grt_trace_mesh.npz"))
    cfg = oracle.default_grt_config(primitive_type=6, enable_normals=1)
    kw = make_golden.GRT_TRACE_SCENES[0]
    sc = make_scene(**kw)
    H, W = kw["height"], kw["width"]
    o = oracle.grt_forward(cfg, sc["density12"], sc["sph"], 3, 1e-3, sc["batch"]["T_to_world"][0], *sc["rays"])
    ref_cnt = g["trisurfel_s0_hits_count"]
    flips = (o["hit_count"] != ref_cnt)[..., 0]
    assert flips.mean() <= 0.02 and ref_cnt.max() >= 20, f"{int(flips.sum())} rays with another number of accepted hits"
    ok = ~flips
    e = np.abs(o["features"] - g["trisurfel_s0_features"]).max(-1)
    hd = g["trisurfel_s0_hit_distance"]
    e_depth = np.abs(o["hit_distance"] - hd)[..., 0]
    tied = ok & ((e > 1e-5) | (e_depth > 2e-5 * max(1.0, np.abs(hd).max())))
    assert tied.mean() <= 0.02 and (not tied.any() or (e[tied].max() < 2e-2 and e_depth[tied].max() < 2e-2)), f"{int(tied.sum())} rays differ with the same hit count"
    ok = ok & ~tied
    assert np.abs(o["density"] - g["trisurfel_s0_density"])[ok].max() < 1e-5
    assert np.abs(o["hit_distance"] - hd)[..., 1][ok].max() <= 1e-3 and np.median(np.abs(o["hit_distance"] - hd)[..., 1][ok]) <= 2e-6
    # not the instances' image: a surfel's response is evaluated where the ray crosses its plane
    inst = np.load(os.path.join(HERE, "golden", "grt_trace.npz"))
    assert np.abs(g["trisurfel_s0_features"] - inst["s0_features"]).max() > 1e-2
    g_rad, g_dns, g_hit = make_golden.grt_trace_upstream(H, W)
    gd, gs = oracle.grt_backward(cfg, 3, 1e-3, o, g_rad, g_dns, g_hit)
    rd, rs = g["trisurfel_s0_grad_density"], g["trisurfel_s0_grad_sph"]
    ndrop = 3 * int((flips | tied).sum())
    per = np.sort(np.abs(gd[:, :11].astype(np.float64) - rd[:, :11]).max(1))[: max(1, len(gd) - ndrop)]
    assert per.max() / np.abs(rd[:, :11]).max() < 2e-4, f"particle gradients {per.max() / np.abs(rd[:, :11]).max():.2e}"
    per = np.sort(np.abs(gs.astype(np.float64) - rs).max(1))[: max(1, len(gs) - ndrop)]
    assert per.max() / np.abs(rs).max() < 2e-4, "SH gradients"


def test_grt_trihexa_checker_matches_reference_programs_golden():
    """render.primitive_type = trihexa (provided by the HIP plugin since round 5: tests/test_grt_gpu.py::test_trihexa_*); the CHECKER for it: the reference's programs compiled with
    PARTICLE_PRIMITIVE_TYPE = MOGTracingTriHexa over the emulated OptiX walking the six triangles per particle of the reference's trihexa
    kernel (back faces culled), against the oracle's three rhombi in the proxy's coordinate planes with the windings' facing (the z = 0 rhombus
    has two halves facing opposite ways).  A ray is offered the same particle up to three times; every offer is processed as a hit."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    g = np.load(os.path.join(HERE, "golden", "grt_trace_mesh.npz"))
    cfg = oracle.default_grt_config(primitive_type=7)
    kw = make_golden.GRT_TRACE_SCENES[0]
    sc = make_scene(**kw)
    H, W = kw["height"], kw["width"]
    o = oracle.grt_forward(cfg, sc["density12"], sc["sph"], 3, 1e-3, sc["batch"]["T_to_world"][0], *sc["rays"], dbg_cap=128)
    ref_cnt = g["trihexa_s0_hits_count"]
    flips = (o["hit_count"] != ref_cnt)[..., 0]
    assert flips.mean() <= 0.02 and ref_cnt.max() >= 20, f"{int(flips.sum())} rays with another number of accepted hits"
    # the quirk is real: some ray processes one particle more than once
    ids, num = o["hit_ids"], o["hit_num"]
    assert any(len(set(ids[r, :min(int(num[r]), 128)].tolist())) < min(int(num[r]), 128) for r in range(H * W))
    ok = ~flips
    e = np.abs(o["features"] - g["trihexa_s0_features"]).max(-1)
    hd = g["trihexa_s0_hit_distance"]
    e_depth = np.abs(o["hit_distance"] - hd)[..., 0]
    tied = ok & ((e > 1e-5) | (e_depth > 2e-5 * max(1.0, np.abs(hd).max())))
    assert tied.mean() <= 0.02 and (not tied.any() or (e[tied].max() < 2e-2 and e_depth[tied].max() < 2e-2)), f"{int(tied.sum())} rays differ with the same hit count"
    ok = ok & ~tied
    assert np.abs(o["density"] - g["trihexa_s0_density"])[ok].max() < 1e-5
    assert np.abs(o["hit_distance"] - hd)[..., 1][ok].max() <= 1e-3 and np.median(np.abs(o["hit_distance"] - hd)[..., 1][ok]) <= 2e-6
    g_rad, g_dns, g_hit = make_golden.grt_trace_upstream(H, W)
    gd, gs = oracle.grt_backward(cfg, 3, 1e-3, o, g_rad, g_dns, g_hit)
    rd, rs = g["trihexa_s0_grad_density"], g["trihexa_s0_grad_sph"]
    ndrop = 3 * int((flips | tied).sum())
    per = np.sort(np.abs(gd[:, :11].astype(np.float64) - rd[:, :11]).max(1))[: max(1, len(gd) - ndrop)]
    assert per.max() / np.abs(rd[:, :11]).max() < 2e-4, f"particle gradients {per.max() / np.abs(rd[:, :11]).max():.2e}"
    per = np.sort(np.abs(gs.astype(np.float64) - rs).max(1))[: max(1, len(gs) - ndrop)]
    assert per.max() / np.abs(rs).max() < 2e-4, "SH gradients"


def test_grt_sphere_checker_matches_reference_programs_golden():
    """render.primitive_type = sphere (round 6): the reference's programs compiled with PARTICLE_PRIMITIVE_TYPE = MOGTracingSphere over the emulated
    OptiX's built-in sphere primitive (oracle/ref/ref_grt_emul.inl: the any-hit program is offered a ray's entry into a particle's enclosing sphere and,
    ignoring it, its exit), centres and radii from the reference's own kernel - against the oracle's two offers per particle.  The intersector's
    arithmetic is the emulation's (NVIDIA publishes none) and the oracle evaluates the same sequence: the frames agree to the last bit."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    g = np.load(os.path.join(HERE, "golden", "grt_trace_sphere.npz"))
    cfg = oracle.default_grt_config(primitive_type=8)
    for k, kw in enumerate(make_golden.GRT_TRACE_SCENES):
        sc = make_scene(**kw)
        H, W = kw["height"], kw["width"]
        o = oracle.grt_forward(cfg, sc["density12"], sc["sph"], 3, 1e-3, sc["batch"]["T_to_world"][0], *sc["rays"], dbg_cap=256)
        # the spheres are the reference kernel's: scene box = union of centre -+ radius
        assert np.abs(o["scene"] - g[f"sphere_s{k}_scene_box"]).max() <= 4e-7 * np.abs(g[f"sphere_s{k}_scene_box"]).max()
        assert np.allclose(1.0 / o["inst"][:, 0], g[f"sphere_s{k}_radii"], rtol=4e-7, atol=0)
        ref_cnt = g[f"sphere_s{k}_hits_count"]
        assert np.array_equal(o["hit_count"], ref_cnt) and ref_cnt.max() >= 20
        assert np.abs(o["features"] - g[f"sphere_s{k}_features"]).max() <= 1e-6
        assert np.abs(o["density"] - g[f"sphere_s{k}_density"]).max() <= 1e-6
        assert np.abs(o["hit_distance"] - g[f"sphere_s{k}_hit_distance"]).max() <= 2e-6
        assert np.array_equal(o["visibility"] != 0, g[f"sphere_s{k}_visibility"] != 0)
        # the quirk is real: rays process a particle at both roots
        ids, num = o["hit_ids"], o["hit_num"]
        assert sum(int(min(int(num[r]), 256) - len(set(ids[r, :min(int(num[r]), 256)].tolist()))) for r in range(H * W)) > 100
        # ... so the frame is not the instances' frame
        assert ref_cnt.sum() != np.load(os.path.join(HERE, "golden", "grt_trace.npz"))[f"s{k}_hits_count"].sum()
        g_rad, g_dns, g_hit = make_golden.grt_trace_upstream(H, W)
        gd, gs = oracle.grt_backward(cfg, 3, 1e-3, o, g_rad, g_dns, g_hit)
        rd, rs = g[f"sphere_s{k}_grad_density"], g[f"sphere_s{k}_grad_sph"]
        assert np.abs(gd[:, :11] - rd[:, :11]).max() / np.abs(rd[:, :11]).max() < 2e-5
        assert np.abs(gs - rs).max() / np.abs(rs).max() < 2e-5


def test_grt_barycentric_surfels_checker_matches_reference_program_golden():
    """render.pipeline_type = barycentricSurfels (round 6): the reference's surfel forward program (barycentricSurfelsOptix.cu: ten hits per trace,
    the response from the hit triangle's barycentrics, depth from the triangle hit distances, the surfel kernel's normals) over the emulated
    OptiX's triangles - tests/golden/grt_trace_bary.npz - against the checker's restatement (oracle/grt_oracle.c: trace_bary_fwd), both scenes.
    The checker evaluates the plane crossing in the proxy frame, the reference Moeller-Trumbore on float32 world vertices: roundings differ."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    g = np.load(os.path.join(HERE, "golden", "grt_trace_bary.npz"))
    cfg = oracle.default_grt_config(primitive_type=6, pipeline_type=1, enable_normals=1)
    for k, kw in enumerate(make_golden.GRT_TRACE_SCENES):
        sc = make_scene(**kw)
        o = oracle.grt_forward(cfg, sc["density12"], sc["sph"], 3, 1e-3, sc["batch"]["T_to_world"][0], *sc["rays"])
        ref_cnt = g[f"bary_s{k}_hits_count"]
        flips = (o["hit_count"] != ref_cnt)[..., 0]
        assert flips.mean() <= 0.01 and ref_cnt.max() >= 20, f"scene {k}: {int(flips.sum())} rays with another number of accepted hits"
        ok = ~flips
        assert np.abs(o["features"] - g[f"bary_s{k}_features"])[ok].max() < 5e-5
        assert np.abs(o["density"] - g[f"bary_s{k}_density"])[ok].max() < 5e-5
        hd = g[f"bary_s{k}_hit_distance"]
        assert np.abs(o["hit_distance"] - hd)[ok].max() <= 5e-5 * max(1.0, np.abs(hd).max())
        assert np.abs(o["normals"] - g[f"bary_s{k}_normals"])[ok].max() < 5e-5
        assert ((o["visibility"] != 0) != (g[f"bary_s{k}_visibility"] != 0)).sum() <= 3 * int(flips.sum())
        # a cross-check program against program: the `reference` pipeline's trisurfel frame integrates the SAME function - the scaled response at
        # the plane crossing is processHit's surfel response in another frame, the triangle hit distance is the crossing's distance - in rounds of
        # sixteen instead of ten (the normals differ: this pipeline flips the surfel's normal ALONG the ray, :160-164)
        tri = np.load(os.path.join(HERE, "golden", "grt_trace_mesh.npz"))
        if k == 0:
            assert np.abs(g["bary_s0_features"] - tri["trisurfel_s0_features"]).max() < 1e-4
            assert np.abs(g["bary_s0_hit_distance"] - tri["trisurfel_s0_hit_distance"]).max() < 1e-4
    # another primitive with this pipeline: refused by the checker as by the plugin
    bad = oracle.default_grt_config(primitive_type=0, pipeline_type=1)
    with pytest.raises(AssertionError):
        oracle.grt_forward(bad, sc["density12"], sc["sph"], 3, 1e-3, sc["batch"]["T_to_world"][0], *sc["rays"])


def test_grt_custom_primitives_match_reference_programs_golden():
    """render.primitive_type = custom: the oracle (world boxes of computeGaussianEnclosingAABBKernel + the maximum-response point within
    3 sigma, orc_grt_custom_boxes / candidate) against tests/golden/grt_trace_mesh.npz `custom_*` = the reference's programs compiled with
    PARTICLE_PRIMITIVE_TYPE = MOGTracingCustom (intersectCustomParticle in world space) over the emulated OptiX's custom-primitive boxes.
    The reference's program evaluates the hit distance in the particle's scale frame, the oracle in the proxy frame (the same point; other
    roundings): two hits that tie to rounding may swap."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    g = np.load(os.path.join(HERE, "golden", "grt_trace_mesh.npz"))
    cfg = oracle.default_grt_config(primitive_type=5)
    for k, kw in enumerate(make_golden.GRT_TRACE_SCENES):
        sc = make_scene(**kw)
        H, W = kw["height"], kw["width"]
        o = oracle.grt_forward(cfg, sc["density12"], sc["sph"], 3, 1e-3, sc["batch"]["T_to_world"][0], *sc["rays"])
        # the boxes are the reference kernel's, to the last bit but for the kernel-scale's own rounding
        box8 = oracle.grt_custom_boxes(cfg, sc["density12"])
        ref_box = g[f"custom_s{k}_boxes"]
        assert np.abs(box8[:, :6] - ref_box).max() <= 4e-7 * np.abs(ref_box).max(), f"scene {k}: world boxes"
        ref_cnt = g[f"custom_s{k}_hits_count"]
        flips = (o["hit_count"] != ref_cnt)[..., 0]
        assert flips.mean() <= 0.01 and ref_cnt.max() >= 20, f"custom scene {k}: {int(flips.sum())} rays with another number of accepted hits"
        ok = ~flips
        e = np.abs(o["features"] - g[f"custom_s{k}_features"]).max(-1)
        hd = g[f"custom_s{k}_hit_distance"]
        e_depth = np.abs(o["hit_distance"] - hd)[..., 0]
        tied = ok & ((e > 1e-5) | (e_depth > 2e-5 * max(1.0, np.abs(hd).max())))
        assert tied.mean() <= 0.02 and (not tied.any() or (e[tied].max() < 2e-2 and e_depth[tied].max() < 2e-2)), f"custom scene {k}: {int(tied.sum())} rays differ with the same hit count"
        ok = ok & ~tied
        assert np.abs(o["density"] - g[f"custom_s{k}_density"])[ok].max() < 1e-5
        assert np.abs(o["hit_distance"] - hd)[..., 1][ok].max() <= 1e-5 * max(1.0, np.abs(hd).max())
        assert ((o["visibility"] != 0) != (g[f"custom_s{k}_visibility"] != 0)).sum() <= 3 * int((flips | tied).sum())
        # not the instances' result: the world box contains the oriented cube, so more rays are offered the particle
        inst_cnt = np.load(os.path.join(HERE, "golden", "grt_trace.npz"))[f"s{k}_hits_count"]
        assert ref_cnt.sum() > inst_cnt.sum()
        g_rad, g_dns, g_hit = make_golden.grt_trace_upstream(H, W)
        gd, gs = oracle.grt_backward(cfg, 3, 1e-3, o, g_rad, g_dns, g_hit)
        rd, rs = g[f"custom_s{k}_grad_density"], g[f"custom_s{k}_grad_sph"]
        ndrop = 3 * int((flips | tied).sum())
        per = np.sort(np.abs(gd[:, :11].astype(np.float64) - rd[:, :11]).max(1))[: max(1, len(gd) - ndrop)]
        assert per.max() / np.abs(rd[:, :11]).max() < 2e-4, f"custom scene {k}: particle gradients"
        per = np.sort(np.abs(gs.astype(np.float64) - rs).max(1))[: max(1, len(gs) - ndrop)]
        assert per.max() / np.abs(rs).max() < 2e-4, f"custom scene {k}: SH gradients"


def test_gut_frame_matches_reference_kernels_golden():
    """The oracle's whole 3DGUT frame against tests/golden/gut_render.npz = the reference's own projectOnTiles / render /
    renderBackward kernels run on the host (oracle/ref/ref_gut_render.cpp: the real particle class, GUTKBufferRenderer's tile
    loop and hit k-buffer, ray payload set-up / write-out, threedgut::processHitBwd with its 32-lane reductions, on a fiber
    emulation of a 16x16 CUDA block): binning products, images for K = 0 and K = 16, and the gradients renderBackward
    accumulates (per-particle density / pose / scale, and the precomputed-radiance gradient the projection backward consumes)."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    g = np.load(os.path.join(HERE, "golden", "gut_render.npz"))
    err, acc_standin, acc_twin = g["standin_check"]
    assert err < 2e-6 and acc_standin == acc_twin > 1000   # the Slang stand-in of that build agreed with the reference's CUDA twin
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    F = np.float32
    for k, kw in enumerate(make_golden.GUT_RENDER_SCENES):
        sc = make_scene(**kw)
        H, W = kw["height"], kw["width"]
        cfg = oracle.default_gut_config(enable_hitcounts=1)
        o = oracle.gut_forward(cfg, sc["cam"], sc["pose_start"], sc["pose_end"], 3, sc["density12"], sc["sph"], *sc["rays"])
        # projection + binning (with the real particle class: includes the per-particle radiance from the SH coefficients)
        assert np.array_equal(o["proj"]["tiles_count"], g[f"s{k}_tiles_count"])
        seen = g[f"s{k}_tiles_count"] > 0
        assert np.abs(o["proj"]["rgb"] - g[f"s{k}_features"])[seen].max() < 2e-6
        # visibility: as in test_projection_stage_matches_reference_code_golden (the reference's flag is undefined when the
        # unscented projection itself failed; wherever the oracle says visible the reference must agree)
        vis = g[f"s{k}_visibility"]
        assert np.all(vis[o["visibility"] != 0] != 0) and np.all(o["visibility"][seen] != 0) and np.all(vis[seen] != 0)
        assert np.array_equal(o["bins"]["sorted_idx"], g[f"s{k}_sorted_idx"]) and np.array_equal(o["bins"]["tile_ranges"], g[f"s{k}_tile_ranges"])
        # render
        assert np.abs(o["feat_density"] - g[f"s{k}_feat_density"]).max() < 2e-6
        assert np.abs(o["hit_distance"] - g[f"s{k}_hit_distance"]).max() <= 2e-6 * max(1.0, np.abs(g[f"s{k}_hit_distance"]).max())
        assert np.array_equal(o["hit_count"], g[f"s{k}_hit_count"]) and g[f"s{k}_hit_count"].max() >= 40
        # renderBackward on the golden's own forward state
        gfd, gdist = make_golden.gut_render_upstream(H, W)
        n = len(sc["density12"])
        gd, grgb = np.zeros((n, 12), F), np.zeros((n, 3), F)
        ps, pe = np.asarray(sc["pose_start"], F), np.asarray(sc["pose_end"], F)
        ro, rd = (np.ascontiguousarray(a, F).reshape(H, W, 3) for a in sc["rays"])
        d12 = np.ascontiguousarray(sc["density12"], F)
        fd, dist, feat = g[f"s{k}_feat_density"], g[f"s{k}_hit_distance"], g[f"s{k}_features"]
        r = oracle.lib(F).orc_gut_render_bwd(C.byref(cfg), W, H, p(ps), p(pe), p(d12), p(feat), p(g[f"s{k}_sorted_idx"]), p(g[f"s{k}_tile_ranges"]),
                                             p(ro), p(rd), p(fd), p(gfd), p(dist), p(gdist), p(gd), p(grgb))
        assert r == 0
        ref_gd, ref_grgb = g[f"s{k}_grad_density"], g[f"s{k}_grad_features"]
        for name, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
            assert rel_err(gd[:, sl], ref_gd[:, sl]) < 2e-5, f"scene {k}: grad {name} {rel_err(gd[:, sl], ref_gd[:, sl]):.2e}"
        assert rel_err(grgb, ref_grgb) < 2e-5
        assert np.abs(ref_gd[:, :11]).max() > 1.0 and not ref_gd[:, 11].any()
        # sorted mode: the hit k-buffer of gutKBufferRenderer.cuh:62-122 with K = 16
        o16 = oracle.gut_forward(oracle.default_gut_config(enable_hitcounts=1, k_buffer_size=16), sc["cam"], sc["pose_start"], sc["pose_end"], 3,
                                 sc["density12"], sc["sph"], *sc["rays"])
        assert np.abs(o16["feat_density"] - g[f"s{k}_k16_feat_density"]).max() < 2e-6
        assert np.abs(o16["hit_distance"] - g[f"s{k}_k16_hit_distance"]).max() <= 2e-6 * max(1.0, np.abs(g[f"s{k}_k16_hit_distance"]).max())
        assert np.array_equal(o16["hit_count"], g[f"s{k}_k16_hit_count"])
        assert np.abs(g[f"s{k}_k16_feat_density"] - g[f"s{k}_feat_density"]).max() > 0.05   # the sorted image really is a different image
        for kk in (4, 8):
            ok = oracle.gut_forward(oracle.default_gut_config(enable_hitcounts=1, k_buffer_size=kk), sc["cam"], sc["pose_start"], sc["pose_end"], 3,
                                    sc["density12"], sc["sph"], *sc["rays"])
            assert np.abs(ok["feat_density"] - g[f"s{k}_k{kk}_feat_density"]).max() < 2e-6, kk
            assert np.abs(ok["hit_distance"] - g[f"s{k}_k{kk}_hit_distance"]).max() <= 2e-6 * max(1.0, np.abs(g[f"s{k}_k{kk}_hit_distance"]).max())
            assert np.array_equal(ok["hit_count"], g[f"s{k}_k{kk}_hit_count"])


@pytest.mark.parametrize("kind", ["fisheye", "pinhole_rs", "ftheta"])
def test_gut_frame_camera_models_match_reference_kernels_golden(kind):
    """As test_gut_frame_matches_reference_kernels_golden, through the other two camera models and two rolling shutters: the
    reference's projectOnTiles (real particle class), render and renderBackward on an OpenCV fisheye with distortion, a distorted
    pinhole whose camera moves during a top-to-bottom exposure, and an f-theta camera with a left-to-right shutter."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    from scenes import make_camera_scene
    g = np.load(os.path.join(HERE, "golden", "gut_render.npz"))
    kw = dict(make_golden.GUT_RENDER_CAMERA_SCENES)[kind]
    sc = make_camera_scene(kind, **kw)
    W, H = kw["w"], kw["h"]
    cfg = oracle.default_gut_config(enable_hitcounts=1)
    o = oracle.gut_forward(cfg, sc["cam"], sc["pose_start"], sc["pose_end"], 3, sc["density12"], sc["sph"], *sc["rays"])
    ref_tc = g[f"{kind}_tiles_count"]
    # shutter-iterated projections differ in the last bits, so a tile count may flip at the culling threshold: bounded, and
    # everything downstream is compared on the golden's own lists
    dt = np.abs(o["proj"]["tiles_count"].astype(np.int64) - ref_tc.astype(np.int64))
    assert (dt > 0).sum() <= max(1, 0.005 * len(ref_tc)) and dt.max() <= 1, f"{int((dt > 0).sum())} tile counts differ"
    seen = (ref_tc > 0) & (o["proj"]["tiles_count"] > 0)
    assert np.abs(o["proj"]["rgb"] - g[f"{kind}_features"])[seen].max() < 5e-6
    if not dt.any():
        assert np.array_equal(o["bins"]["sorted_idx"], g[f"{kind}_sorted_idx"]) and np.array_equal(o["bins"]["tile_ranges"], g[f"{kind}_tile_ranges"])
    F = np.float32
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n = len(sc["density12"])
    ps, pe = np.asarray(sc["pose_start"], F), np.asarray(sc["pose_end"], F)
    ro, rd = (np.ascontiguousarray(a, F).reshape(H, W, 3) for a in sc["rays"])
    d12 = np.ascontiguousarray(sc["density12"], F)
    feat, sidx, rng = g[f"{kind}_features"], g[f"{kind}_sorted_idx"], g[f"{kind}_tile_ranges"]
    fd, dist, cnt = np.zeros((H, W, 4), F), np.full((H, W, 1), 1e6, F), np.zeros((H, W, 1), F)
    lib = oracle.lib(F)
    assert lib.orc_gut_render_fwd(C.byref(cfg), W, H, p(ps), p(pe), p(d12), p(feat), p(sidx), p(rng), p(ro), p(rd), p(fd), p(dist), p(cnt)) == 0
    assert np.abs(fd - g[f"{kind}_feat_density"]).max() < 2e-6
    assert np.abs(dist - g[f"{kind}_hit_distance"]).max() <= 2e-6 * max(1.0, np.abs(g[f"{kind}_hit_distance"]).max())
    assert np.array_equal(cnt, g[f"{kind}_hit_count"]) and cnt.max() >= 10
    gfd, gdist = make_golden.gut_render_upstream(H, W)
    gd, grgb = np.zeros((n, 12), F), np.zeros((n, 3), F)
    assert lib.orc_gut_render_bwd(C.byref(cfg), W, H, p(ps), p(pe), p(d12), p(feat), p(sidx), p(rng), p(ro), p(rd), p(g[f"{kind}_feat_density"]),
                                  p(gfd), p(g[f"{kind}_hit_distance"]), p(gdist), p(gd), p(grgb)) == 0
    ref_gd, ref_grgb = g[f"{kind}_grad_density"], g[f"{kind}_grad_features"]
    for name, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
        assert rel_err(gd[:, sl], ref_gd[:, sl]) < 2e-5, f"{kind}: grad {name} {rel_err(gd[:, sl], ref_gd[:, sl]):.2e}"
    assert rel_err(grgb, ref_grgb) < 2e-5


def test_gut_frame_quartic_kernel_matches_reference_kernels_golden():
    """The same frame pipeline with particle_kernel_degree = 4 (the reference's kernels built with
    GAUSSIAN_PARTICLE_KERNEL_DEGREE=4): images, hit counts and renderBackward gradients."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    g = np.load(os.path.join(HERE, "golden", "gut_render.npz"))
    err, a, b = g["standin_check_deg4"]
    assert err < 2e-6 and a == b > 1000
    kw = make_golden.GUT_RENDER_SCENES[0]
    sc = make_scene(**kw)
    H, W = kw["height"], kw["width"]
    cfg = oracle.default_gut_config(enable_hitcounts=1, particle_kernel_degree=4)
    o = oracle.gut_forward(cfg, sc["cam"], sc["pose_start"], sc["pose_end"], 3, sc["density12"], sc["sph"], *sc["rays"])
    assert np.array_equal(o["proj"]["tiles_count"], g["deg4_tiles_count"]) and np.array_equal(o["bins"]["sorted_idx"], g["deg4_sorted_idx"])
    assert np.abs(o["feat_density"] - g["deg4_feat_density"]).max() < 2e-6
    assert np.abs(o["hit_distance"] - g["deg4_hit_distance"]).max() <= 2e-6 * max(1.0, np.abs(g["deg4_hit_distance"]).max())
    assert np.array_equal(o["hit_count"], g["deg4_hit_count"])
    assert np.abs(g["deg4_feat_density"] - g["s0_feat_density"]).max() > 0.02      # really a different kernel
    F = np.float32
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    n = len(sc["density12"])
    gfd, gdist = make_golden.gut_render_upstream(H, W)
    gd, grgb = np.zeros((n, 12), F), np.zeros((n, 3), F)
    ps, pe = np.asarray(sc["pose_start"], F), np.asarray(sc["pose_end"], F)
    ro, rd = (np.ascontiguousarray(x, F).reshape(H, W, 3) for x in sc["rays"])
    d12 = np.ascontiguousarray(sc["density12"], F)
    assert oracle.lib(F).orc_gut_render_bwd(C.byref(cfg), W, H, p(ps), p(pe), p(d12), p(g["deg4_features"]), p(g["deg4_sorted_idx"]),
                                            p(g["deg4_tile_ranges"]), p(ro), p(rd), p(g["deg4_feat_density"]), p(gfd), p(g["deg4_hit_distance"]),
                                            p(gdist), p(gd), p(grgb)) == 0
    for name, sl in {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}.items():
        assert rel_err(gd[:, sl], g["deg4_grad_density"][:, sl]) < 2e-5, name
    assert rel_err(grgb, g["deg4_grad_features"]) < 2e-5


def test_reference_balanced_forward_agrees_with_the_sequential_one_within_tolerance():
    """`render.splat.fine_grained_load_balancing: true` selects the reference's OTHER forward kernel (renderBalanced: a warp per
    pixel, warp-level prefix products).  Run on the host like the rest of gut_render.npz, it differs from the reference's own
    sequential kernel — and hence from the oracle and the plugin, which always compute the sequential result — only in the
    opacity of rays that end on the transmittance threshold (the batch of 32 entries that contains the terminating hit is
    absorbed whole): within BASELINE's 1e-4, colours and hit counts unchanged.  That is why the plugin may accept the flag."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    g = np.load(os.path.join(HERE, "golden", "gut_render.npz"))
    worst_opacity = 0.0
    for k, kw in enumerate(make_golden.GUT_RENDER_SCENES):
        sc = make_scene(**kw)
        o = oracle.gut_forward(oracle.default_gut_config(enable_hitcounts=1), sc["cam"], sc["pose_start"], sc["pose_end"], 3, sc["density12"],
                               sc["sph"], *sc["rays"])
        bal = g[f"s{k}_balanced_feat_density"]
        assert np.abs(o["feat_density"][..., :3] - bal[..., :3]).max() < 5e-6
        d_op = np.abs(o["feat_density"][..., 3] - bal[..., 3])
        assert d_op.max() < 1e-4
        # only rays that ended on the threshold may differ at all beyond rounding, and only towards MORE opacity
        moved = d_op > 1e-6
        assert np.all(o["feat_density"][..., 3][moved] > 1.0 - 1.001e-4) and np.all(bal[..., 3][moved] >= o["feat_density"][..., 3][moved])
        assert np.abs(o["hit_distance"] - g[f"s{k}_balanced_hit_distance"]).max() < 1e-5 * max(1.0, np.abs(o["hit_distance"]).max())
        assert np.array_equal(o["hit_count"], g[f"s{k}_balanced_hit_count"])
        worst_opacity = max(worst_opacity, float(d_op.max()))
    assert worst_opacity > 1e-5      # the difference is real, not rounding: the second scene has rays that terminate


@pytest.mark.parametrize("name", ["k0", "k4", "k16", "k16_depth"])
def test_backward_matches_autograd_of_the_restated_reference_forward(name):
    """G11 / G12 pinned independently of any hand-derived backward: tests/golden/autograd_gut.npz holds the gradients that float64
    torch.autograd produced from a restatement of the reference FORWARD (Slang sources; tests/golden/make_autograd_golden.py) — what
    slangc's reverse mode computes at the reference's build time.  The oracle's analytic backward (sorted K > 0 compositing,
    projection / SH backward, and the K = 0 path for completeness) must reproduce them."""
    g = np.load(os.path.join(HERE, "golden", "autograd_gut.npz"))
    n, w, h, K = int(g[f"{name}_n"]), int(g[f"{name}_w"]), int(g[f"{name}_h"]), int(g[f"{name}_K"])
    from scenes import make_scene, rel_err
    scene = make_scene(n=n, width=w, height=h, median_scale=0.16, seed=int(g[f"{name}_seed"]))
    assert np.array_equal(scene["density12"], g[f"{name}_density12"]) and np.array_equal(scene["sph"], g[f"{name}_sph"])
    cfg = oracle.default_gut_config(k_buffer_size=K)
    for dtype, tol in ((np.float64, 2e-5), (np.float32, 1e-3)):   # (f64: the two sides differ by the pose's float32 quaternion, 2e-7)
        fwd = oracle.gut_forward(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], 3, scene["density12"], scene["sph"], *scene["rays"], dtype=dtype)
        gd, gsph, grgb = oracle.gut_backward(cfg, scene["cam"], 3, fwd, g[f"{name}_g_fd"], g[f"{name}_g_dist"], dtype=dtype)
        if dtype == np.float32 and not np.array_equal(fwd["hit_count"], oracle.gut_forward(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], 3,
                                                                                          scene["density12"], scene["sph"], *scene["rays"],
                                                                                          dtype=np.float64)["hit_count"].astype(np.float32)):
            continue   # a threshold flip between the f32 and f64 evaluation of this frame: the f64 comparison above is the pin
        ref = g[f"{name}_grad_density12"]
        for sl in (slice(0, 3), slice(3, 4), slice(4, 8), slice(8, 11)):
            assert rel_err(gd[:, sl], ref[:, sl]) < tol, (name, dtype, sl)
        assert rel_err(gsph, g[f"{name}_grad_sph"]) < tol
        # the per-particle radiance gradient between the two stages (render backward output = projection backward input), taken
        # on the clamped radiance on both sides
        assert rel_err(grgb, g[f"{name}_grad_radiance"]) < tol


@pytest.mark.parametrize("k", [0, 1])
def test_nht_forward_matches_reference_kernels_golden(k):
    """model.feature_type = nht (FEATURE_TRANSFORM_TYPE 1): the reference's projectOnTiles / render kernels built with the NHT macro set
    (oracle/ref: libref_gut_render_nht_deg2_k0, tests/golden/make_golden.py: make_gut_nht) against orc_gut_render_nht_fwd — first on the
    reference's own tile lists, then end to end through the oracle's binning."""
    from scenes import make_scene
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import make_golden as mg
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "gut_nht.npz"))
    sc = make_scene(**mg.GUT_RENDER_SCENES[k])
    feats = g[f"s{k}_features"]
    cfg = oracle.default_gut_config()
    on_lists = oracle.gut_forward_nht(cfg, sc["cam"], sc["pose_start"], sc["pose_end"], sc["density12"], feats, *sc["rays"],
                                      lists=(g[f"s{k}_sorted_idx"], g[f"s{k}_tile_ranges"]))
    ref = g[f"s{k}_feat_density"]
    assert ref.shape[-1] == 25 and np.abs(ref[..., :24]).max() > 0.5
    assert np.array_equal(on_lists["hit_count"], g[f"s{k}_hit_count"])
    assert np.abs(on_lists["feat_density"] - ref).max() < 2e-5 and np.abs(on_lists["hit_distance"] - g[f"s{k}_hit_distance"]).max() < 2e-5
    full = oracle.gut_forward_nht(cfg, sc["cam"], sc["pose_start"], sc["pose_end"], sc["density12"], feats, *sc["rays"])
    assert np.array_equal(full["sorted_idx"], g[f"s{k}_sorted_idx"])
    assert np.abs(full["feat_density"] - ref).max() < 2e-5
    # round 6: the sorted hit buffer in front of the feature integration - the reference's kernels built with GAUSSIAN_K_BUFFER_SIZE 4 / 16 AND
    # the feature macros (libref_gut_render_nht_deg2_k{4,16}.so), same tile lists.  Hits whose distances tie to rounding may swap: bounded.
    for K in (4, 16):
        cfg_k = oracle.default_gut_config(k_buffer_size=K)
        ok = oracle.gut_forward_nht(cfg_k, sc["cam"], sc["pose_start"], sc["pose_end"], sc["density12"], feats, *sc["rays"],
                                    lists=(g[f"s{k}_sorted_idx"], g[f"s{k}_tile_ranges"]))
        ref_k = g[f"s{k}_k{K}_feat_density"]
        assert np.abs(ref_k - ref).max() > 0.1      # (not the unsorted frame)
        flips = (ok["hit_count"] != g[f"s{k}_k{K}_hit_count"])[..., 0]
        e = np.abs(ok["feat_density"] - ref_k).max(-1)
        bad = ~flips & (e > 2e-5)
        assert flips.mean() <= 5e-3 and bad.mean() <= 5e-3, (K, int(flips.sum()), int(bad.sum()), float(e.max()))
        assert np.abs(ok["hit_distance"] - g[f"s{k}_k{K}_hit_distance"])[~flips & ~bad].max() < 2e-5


def test_nht_pixel_trace_recomposites_the_frame_and_identifies_a_toggled_decision():
    """The flip identification of the full-size NHT parity (parity_util.identify_flips with orc_gut_pixel_trace_nht): compositing a pixel's
    trace reproduces orc_gut_render_nht_fwd's pixel; a pixel whose most borderline accepted hit is REMOVED from the target is identified by
    exactly one toggle once the margin admits that hit, and is unidentifiable when it does not."""
    from scenes import make_scene
    import parity_util as pu
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import make_golden as mg
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "gut_nht.npz"))
    sc = make_scene(**mg.GUT_RENDER_SCENES[0])
    feats = g["s0_features"]
    cfg = oracle.default_gut_config()
    fwd = oracle.gut_forward_nht(cfg, sc["cam"], sc["pose_start"], sc["pose_end"], sc["density12"], feats, *sc["rays"])
    H, W = sc["H"], sc["W"]
    rays = tuple(np.ascontiguousarray(np.asarray(r, np.float32).reshape(H, W, 3)) for r in sc["rays"])
    tin = dict(poses=(sc["pose_start"], sc["pose_end"]), rays=rays, density12=sc["density12"], nht_features=feats,
               bins=dict(sorted_idx=fwd["sorted_idx"], tile_ranges=fwd["tile_ranges"]))
    trace = lambda pix, dt: oracle.gut_pixel_trace_nht(cfg, sc["cam"], tin, pix, dtype=dt)
    fd, cnt, dist = fwd["feat_density"].copy(), fwd["hit_count"][..., 0].copy(), fwd["hit_distance"].copy()
    pixels = np.flatnonzero(cnt.reshape(-1) > 3)[::37][:12]
    assert len(pixels) >= 8
    for pix in pixels:
        tr = trace(pix, np.float32)
        C_, opa, D, c, _ = pu._composite(tr["alpha"].astype(np.float64), tr["hit_t"].astype(np.float64), tr["colour"].astype(np.float64), tr["margin"] > 0,
                                         float(cfg.min_transmittance))
        assert c == int(cnt.reshape(-1)[pix])
        assert np.abs(C_ - fd.reshape(-1, 25)[pix, :24]).max() < 2e-5 and abs(opa - fd.reshape(-1, 25)[pix, 24]) < 2e-5 and abs(D - dist.reshape(-1)[pix]) < 2e-5
    toggles, rounding, _ = pu.identify_flips(cfg, sc["cam"], tin, None, pixels, fd, cnt, dist, trace_fn=trace)
    assert (toggles == 0).all() and not rounding.any()
    # remove each pixel's most borderline accepted hit from the TARGET
    margins = []
    for pix in pixels:
        tr = trace(pix, np.float32)
        acc = (tr["margin"] > 0) & (tr["alpha"] > 0)
        j = np.flatnonzero(acc)[np.argmin(tr["margin"][acc])]
        acc2 = tr["margin"] > 0
        acc2[j] = False
        C_, opa, D, c, _ = pu._composite(tr["alpha"].astype(np.float64), tr["hit_t"].astype(np.float64), tr["colour"].astype(np.float64), acc2,
                                         float(cfg.min_transmittance))
        fd.reshape(-1, 25)[pix, :24], fd.reshape(-1, 25)[pix, 24], dist.reshape(-1)[pix], cnt.reshape(-1)[pix] = C_, opa, D, c
        margins.append(float(tr["margin"][j]))
    wide, _, _ = pu.identify_flips(cfg, sc["cam"], tin, None, pixels, fd, cnt, dist, margin=max(margins) * 1.01, trace_fn=trace)
    assert (wide >= 1).all() and (wide <= 2).all(), wide                     # (one toggle; a second only where the end of the ray moved with it)
    narrow, _, _ = pu.identify_flips(cfg, sc["cam"], tin, None, pixels, fd, cnt, dist, margin=min(margins) * 0.5, trace_fn=trace)
    assert (narrow == -1).all(), narrow


@pytest.mark.parametrize("name", ["nht", "nht_depth", "nht_k4", "nht_k16_depth"])
def test_nht_backward_matches_autograd_of_the_restated_reference_forward(name):
    """The nht backward is Slang autodiff output in the reference (not in the checkout): the oracle's reverse mode against float64
    torch.autograd of the restated forward (tests/golden/make_autograd_golden.py --nht), gradients w.r.t. the particle rows and the
    per-particle feature buffer, with and without a hit-distance gradient."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "autograd_gut_nht.npz"))
    n, w, h, seed = (int(g[f"{name}_{k}"]) for k in ("n", "w", "h", "seed"))
    scene = make_scene(n=n, width=w, height=h, median_scale=0.16, seed=seed)
    # (round 6: nht_k4 / nht_k16_depth = the sorted hit buffer in front of the feature integration, gutKBufferRenderer.cuh:158-225, 273-352)
    cfg = oracle.default_gut_config(k_buffer_size=int(g[f"{name}_K"]))
    feats = g[f"{name}_features"]
    # float64 build: 5e-6, not 1e-9 - the two sides share float32 INPUTS but the golden carries the ray through the frame's float32
    # pose block while the double build re-derives that block in double (their forwards agree to 8e-7, printed by the generator)
    for dtype, tol in ((np.float64, 5e-6), (np.float32, 3e-4)):
        fwd = oracle.gut_forward_nht(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], scene["density12"], feats, *scene["rays"], dtype=dtype)
        gd, gf = oracle.gut_backward_nht(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], scene["density12"], feats, *scene["rays"], fwd,
                                         g[f"{name}_g_fd"], g[f"{name}_g_dist"], dtype=dtype)
        ref_d, ref_f = g[f"{name}_grad_density12"], g[f"{name}_grad_features"]
        for sl in (slice(0, 3), slice(3, 4), slice(4, 8), slice(8, 11)):
            assert rel_err(gd[:, sl], ref_d[:, sl]) < tol, (dtype, sl, rel_err(gd[:, sl], ref_d[:, sl]))
        assert rel_err(gf, ref_f) < tol, (dtype, rel_err(gf, ref_f))
        assert np.abs(ref_f).max() > 0 and np.abs(ref_d[:, :3]).max() > 0


def test_grt_nht_forward_uses_the_feature_model_pinned_by_the_gut_golden():
    """The 3DGRT restatement of the Slang pipeline with neural harmonic features (orc_grt_trace_nht_fwd, oracle/orc_nht.h) shares no code
    with the 3DGUT one, which the reference's own render kernel pins (gut_nht.npz).  On a scene where both renderers process the same hits
    in the same order per ray — well separated particles, every ray's candidates far fewer than 16 per round — the two must agree."""
    rng = np.random.default_rng(3)
    n, w, h = 60, 24, 16
    scene = make_scene(n=n, width=w, height=h, median_scale=0.07, max_density=0.6, seed=11)
    feats = rng.uniform(-np.pi / 2, np.pi / 2, size=(n, 48)).astype(np.float32)
    T = scene["batch"]["T_to_world"][0]
    gcfg = oracle.default_gut_config(particle_kernel_degree=4, min_transmittance=1e-3)
    rcfg = oracle.default_grt_config()
    gut = oracle.gut_forward_nht(gcfg, scene["cam"], scene["pose_start"], scene["pose_end"], scene["density12"], feats, *scene["rays"], dtype=np.float64)
    grt = oracle.grt_forward_nht(rcfg, scene["density12"], feats, 1e-3, T, *scene["rays"], dtype=np.float64)
    # the two renderers order overlapping hits differently (3DGUT: by particle depth, 3DGRT: by hit distance): rays on which the order
    # matters differ legitimately; on all the others the 24 features agree to rounding, which no error in the feature model would allow
    same = (gut["hit_count"][..., 0] == grt["hit_count"][..., 0])
    close = np.abs(gut["feat_density"][..., :24] - grt["features"]).max(-1) < 1e-6
    assert same.mean() > 0.9 and close.mean() > 0.75, (same.mean(), close.mean())
    assert np.abs(gut["feat_density"][..., 24] - grt["density"][..., 0]).max() < 1e-6 or close.mean() > 0.75
    assert np.abs(grt["features"]).max() > 0.3


def test_grt_nht_backward_is_the_gradient_of_forward_away_from_the_last_hit():
    """Central finite differences (float64) of the 3DGRT nht forward against orc_grt_trace_nht_bwd — the reverse mode of the lerp form with
    the canonical-intersection path — for the feature rows and the particle rows; the backward program drops each ray's last hit
    (endT = tLast + 1e-9), so particles that are some ray's last hit are not probed (as in the SH test above)."""
    rng = np.random.default_rng(5)
    n, w, h = 200, 10, 8
    scene = make_scene(n=n, width=w, height=h, median_scale=0.2, max_density=0.5, seed=2)
    feats = rng.uniform(-np.pi / 2, np.pi / 2, size=(n, 48))
    T = scene["batch"]["T_to_world"][0]
    cfg = oracle.default_grt_config()
    d12 = scene["density12"].astype(np.float64)
    g_f, g_d, g_h = rng.normal(size=(h, w, 24)), rng.normal(size=(h, w, 1)), rng.normal(size=(h, w, 1)) * 0.1

    def run(d, f):
        return oracle.grt_forward_nht(cfg, d, f, 1e-3, T, *scene["rays"], dbg_cap=512, dtype=np.float64)

    f0 = run(d12, feats)
    gd, gf = oracle.grt_backward_nht(cfg, 1e-3, f0, g_f, g_d, g_h.reshape(-1), dtype=np.float64)
    last = set()
    for r in range(h * w):
        k = int(f0["hit_num"][r])
        if k:
            last.add(int(f0["hit_ids"][r, k - 1]))
    probes = [i for i in np.nonzero(np.abs(gd).sum(1) > 0)[0] if i not in last][:5]
    assert probes and np.abs(gf).max() > 0

    def loss(d, f):
        o = run(d, f)
        return float((o["features"] * g_f).sum() + (o["density"] * g_d).sum() + (o["hit_distance"][..., :1] * g_h).sum())

    bad = total = 0
    for i in probes:
        for col in list(range(11)):
            hstep = 1e-6 * max(1.0, abs(d12[i, col]))
            dp, dm = d12.copy(), d12.copy()
            dp[i, col] += hstep
            dm[i, col] -= hstep
            fd = (loss(dp, feats) - loss(dm, feats)) / (2 * hstep)
            total += 1
            bad += abs(fd - gd[i, col]) > 2e-4 * np.abs(gd[:, col]).max() + 1e-7
        for col in (0, 13, 29, 47):
            fp, fm = feats.copy(), feats.copy()
            fp[i, col] += 1e-6
            fm[i, col] -= 1e-6
            fd = (loss(d12, fp) - loss(d12, fm)) / 2e-6
            total += 1
            bad += abs(fd - gf[i, col]) > 2e-4 * np.abs(gf).max() + 1e-7
    assert bad <= total // 4, (bad, total)


def test_grt_nht_forward_matches_reference_slang_programs_golden():
    """orc_grt_trace_nht_fwd against tests/golden/grt_trace_nht.npz = the reference's Slang forward pipeline (referenceSlangOptix.cu: raygen
    round loop, intersection, any-hit k-buffer) with neural harmonic features, run on the host over the emulated traversal
    (oracle/ref/ref_grt_trace_slang.cpp): accepted-hit counts and visibility identical, 24 ray features / opacity / distances to rounding."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    g = np.load(os.path.join(HERE, "golden", "grt_trace_nht.npz"))
    cfg = oracle.default_grt_config()
    for k, kw in enumerate(make_golden.GRT_TRACE_SCENES):
        sc = make_scene(**kw)
        o = oracle.grt_forward_nht(cfg, sc["density12"], g[f"s{k}_nht_features"], 1e-3, sc["batch"]["T_to_world"][0], *sc["rays"])
        assert np.array_equal(o["hit_count"], g[f"s{k}_hits_count"]), f"scene {k}: accepted-hit counts differ"
        assert np.array_equal(o["visibility"] != 0, g[f"s{k}_visibility"] != 0)
        assert np.abs(o["features"] - g[f"s{k}_features"]).max() < 5e-6 and np.abs(o["density"] - g[f"s{k}_density"]).max() < 2e-6
        hd = g[f"s{k}_hit_distance"]
        assert np.abs(o["hit_distance"] - hd).max() <= 5e-6 * max(1.0, np.abs(hd).max())
        assert g[f"s{k}_hits_count"].max() >= 20 and np.abs(g[f"s{k}_features"]).max() > 0.5


@pytest.mark.parametrize("prim,code", [("icosahedron", 1), ("trihexa", 7), ("sphere", 8), ("custom", 5)])
def test_grt_nht_on_icosahedron_proxies_matches_reference_slang_programs_golden(prim, code):
    """(round 6: also trihexa - three offers per particle - and sphere - two - built the same way: libref_grt_trace_slang_{TriHexa,Sphere}_deg4.so)
    model.feature_type = nht together with render.primitive_type = icosahedron (round 5): orc_grt_trace_nht_fwd with the polyhedron clip as
    candidate test against tests/golden/grt_trace_nht_mesh.npz = the reference's Slang forward programs compiled for MOGTracingIcosaHedron
    over the emulated OptiX's built-in triangles (meshes from the reference's mesh kernel, back faces culled).  Like the SH meshes
    (test_grt_mesh_proxies_...): two roundings of the same entry distance - ideal polyhedron in the proxy frame vs float32 world
    vertices - may swap tied hits on a few rays."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    g = np.load(os.path.join(HERE, "golden", "grt_trace_nht_mesh.npz"))
    cfg = oracle.default_grt_config(primitive_type=code)
    kw = make_golden.GRT_TRACE_SCENES[0]
    sc = make_scene(**kw)
    o = oracle.grt_forward_nht(cfg, sc["density12"], g[f"{prim}_s0_nht_features"], 1e-3, sc["batch"]["T_to_world"][0], *sc["rays"])
    flips = (o["hit_count"] != g[f"{prim}_s0_hits_count"])[..., 0]
    assert flips.mean() <= 0.01, f"{int(flips.sum())} rays with another number of accepted hits"
    e = np.abs(o["features"] - g[f"{prim}_s0_features"]).max(-1)
    tied = ~flips & (e > 1e-5)
    assert tied.mean() <= 0.02 and (not tied.any() or e[tied].max() < 5e-2), (int(tied.sum()), float(e[tied].max()) if tied.any() else 0.0)
    ok = ~flips & ~tied
    assert np.abs(o["density"] - g[f"{prim}_s0_density"])[ok].max() < 1e-5
    hd = g[f"{prim}_s0_hit_distance"]
    assert np.abs(o["hit_distance"] - hd)[ok].max() <= 2e-5 * max(1.0, np.abs(hd).max())
    assert (o["visibility"] != 0).sum() > 0 and ((o["visibility"] != 0) != (g[f"{prim}_s0_visibility"] != 0)).sum() <= 3 * int((flips | tied).sum())
    # not the instances' frame: the particle is offered at the distance the ray ENTERS its icosahedron
    inst = np.load(os.path.join(HERE, "golden", "grt_trace_nht.npz"))
    assert np.abs(g[f"{prim}_s0_features"] - inst["s0_features"]).max() > (1e-2 if prim == "icosahedron" else 1e-4) and g[f"{prim}_s0_hits_count"].max() >= 15


def test_slang_forward_with_sh_radiance_is_the_reference_forward():
    """render.pipeline_type = referenceSlang with model.feature_type = sh is served by the kernels of the `reference` pipeline
    (3dgrut_amd/grt_tracer.py): the two reference programs integrate the same function.  Pinned here program against program —
    referenceSlangOptix.cu (tests/golden/grt_trace_slang_sh.npz) against referenceOptix.cu (grt_trace.npz), both run on the host over
    the same emulated traversal on the same scenes: radiance and opacity bit for bit, integrated depth to an ulp, the same rays'
    accepted-hit counts and the same visible particles."""
    a = np.load(os.path.join(HERE, "golden", "grt_trace_slang_sh.npz"))
    b = np.load(os.path.join(HERE, "golden", "grt_trace.npz"))
    k = 0
    while f"s{k}_features" in a:
        assert np.array_equal(a[f"s{k}_features"], b[f"s{k}_features"])
        assert np.array_equal(a[f"s{k}_density"], b[f"s{k}_density"])
        assert np.array_equal(a[f"s{k}_hits_count"], b[f"s{k}_hits_count"])
        assert np.array_equal(a[f"s{k}_visibility"], b[f"s{k}_visibility"])
        assert np.abs(a[f"s{k}_hit_distance"] - b[f"s{k}_hit_distance"]).max() <= 1e-6
        k += 1
    assert k == 2


_SLANG_SH_EQUAL_PRIMS = ["icosahedron", "octahedron", "tetrahedron", "diamond", "trihexa", "sphere", "custom"]


def _hand_written_golden(prim):
    return np.load(os.path.join(HERE, "golden", "grt_trace_sphere.npz" if prim == "sphere" else "grt_trace_mesh.npz"))


@pytest.mark.parametrize("prim", _SLANG_SH_EQUAL_PRIMS)
def test_slang_sh_program_per_primitive_is_the_hand_written_program(prim):
    """render.pipeline_type = referenceSlang with SH radiance and render.primitive_type != instances runs on the kernels of the `reference`
    pipeline.  Pinned program against program, in the terms of test_slang_forward_with_sh_radiance_is_the_reference_forward:
    referenceSlangOptix.cu compiled for the primitive (tests/golden/grt_trace_slang_sh_prims.npz) against referenceOptix.cu compiled for it
    (grt_trace_mesh.npz / grt_trace_sphere.npz), scene 0 - outside the cloud, where the custom primitives' signed and unsigned hit distances
    coincide too (measured: equal; the camera-inside scene is the one that tells them apart, below)."""
    a = np.load(os.path.join(HERE, "golden", "grt_trace_slang_sh_prims.npz"))
    b = _hand_written_golden(prim)
    for key in ("features", "density", "hits_count", "visibility"):
        assert np.array_equal(a[f"{prim}_s0_{key}"], b[f"{prim}_s0_{key}"]), key
    assert np.abs(a[f"{prim}_s0_hit_distance"] - b[f"{prim}_s0_hit_distance"]).max() <= 1e-6
    assert a[f"{prim}_s0_hits_count"].max() >= 15 and np.abs(a[f"{prim}_s0_features"]).max() > 0.5


def test_slang_sh_program_for_trisurfel_is_not_the_hand_written_program():
    """trisurfel is the exception: the Slang forward program as the host stand-in builds it (oracle/ref/shim/3dgrt_slang has no surfel mode:
    GAUSSIAN_PARTICLE_SURFEL, gaussianParticles.slang:49-51, 125-127) and the hand-written program with its surfel branches disagree - measured
    by the golden generator: accepted-hit counts on 315 of 384 rays (6019 / 6419 hits), 0.52 in radiance, 0.48 in opacity, 2.1 in hit distance, 33
    visibility flags.  grt_config_from_conf therefore refuses referenceSlang + trisurfel + SH (test_host_cpu.py) instead of serving it with the
    `reference` kernels; the figures in its message are these."""
    a = np.load(os.path.join(HERE, "golden", "grt_trace_slang_sh_prims.npz"))
    b = _hand_written_golden("trisurfel")
    ca, cb = a["trisurfel_s0_hits_count"], b["trisurfel_s0_hits_count"]
    assert (int((ca != cb).sum()), ca.size, int(ca.sum()), int(cb.sum())) == (315, 384, 6019, 6419)
    assert abs(float(np.abs(a["trisurfel_s0_features"] - b["trisurfel_s0_features"]).max()) - 0.52) < 0.005
    assert abs(float(np.abs(a["trisurfel_s0_density"] - b["trisurfel_s0_density"]).max()) - 0.48) < 0.005
    assert int(((a["trisurfel_s0_visibility"] != 0) != (b["trisurfel_s0_visibility"] != 0)).sum()) == 33


def _custom_inside_scene():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    sc = make_scene(**make_golden.GRT_INSIDE_SCENE)
    return sc, sc["batch"]["T_to_world"][0]


def test_custom_inside_scene_separates_the_slang_program_from_the_hand_written_one():
    """The power of the camera-inside scene (tests/golden/make_golden.py: GRT_INSIDE_SCENE): with primitive_type custom the Slang intersection
    program reports an UNSIGNED hit distance (particleDensityHitCustom, gaussianParticles.slang:489-523), the hand-written one a signed one
    (intersectCustomParticle, gaussianParticles.cuh:407-441), so particles whose point of maximum response lies behind the ray origin are
    candidates of the first only.  `custom_inside_*` (Slang program) against `custom_inside_ref_*` (hand-written program): measured 555 of 768
    rays with another accepted-hit count (17 875 / 17 163 hits), 0.183 in radiance, 3 visibility flags.  If the scene is ever changed so that
    the two programs agree on it, the GPU tests that use it would pass without telling the two conventions apart: this test fails first."""
    g = np.load(os.path.join(HERE, "golden", "grt_trace_slang_sh_prims.npz"))
    differ = (g["custom_inside_hits_count"] != g["custom_inside_ref_hits_count"])[..., 0]
    d_rad = np.abs(g["custom_inside_features"] - g["custom_inside_ref_features"]).max(-1)
    print(f"custom_inside: hit counts differ on {int(differ.sum())} of {differ.size} rays, max radiance difference {d_rad.max():.3f}")
    assert differ.mean() >= 0.25
    assert d_rad.max() > 1e-2
    assert g["custom_inside_hits_count"].sum() > g["custom_inside_ref_hits_count"].sum()


def test_grt_checker_follows_the_slang_custom_hit_test_under_pipeline_type_2():
    """orc_grt_trace_fwd with cfg.pipeline_type = GRUT_PIPELINE_REFERENCE_SLANG takes the unsigned custom distance: against the Slang program's
    golden on the camera-inside scene at most 1 % of the rays may carry another accepted-hit count (expected: none), radiance and opacity
    within 1e-4 on the rest.  With pipeline_type 0 (signed distance) the same checker must MISS that golden on at least a quarter of the rays -
    and reproduce the hand-written program's instead."""
    g = np.load(os.path.join(HERE, "golden", "grt_trace_slang_sh_prims.npz"))
    sc, T = _custom_inside_scene()
    slang = oracle.grt_forward(oracle.default_grt_config(primitive_type=5, pipeline_type=2), sc["density12"], sc["sph"], 3, 1e-3, T, *sc["rays"])
    flips = (slang["hit_count"] != g["custom_inside_hits_count"])[..., 0]
    print(f"checker pipeline_type 2 vs Slang golden: {int(flips.sum())} of {flips.size} rays with another hit count, "
          f"total {int(slang['hit_count'].sum())} / {int(g['custom_inside_hits_count'].sum())}")
    assert flips.mean() <= 0.01
    ok = ~flips
    assert np.abs(slang["features"] - g["custom_inside_features"])[ok].max() <= 1e-4
    assert np.abs(slang["density"] - g["custom_inside_density"])[ok].max() <= 1e-4
    assert ((slang["visibility"] != 0) != (g["custom_inside_visibility"] != 0)).sum() <= 3 * int(flips.sum())
    hand = oracle.grt_forward(oracle.default_grt_config(primitive_type=5, pipeline_type=0), sc["density12"], sc["sph"], 3, 1e-3, T, *sc["rays"])
    miss = (hand["hit_count"] != g["custom_inside_hits_count"])[..., 0]
    print(f"checker pipeline_type 0 vs Slang golden: {int(miss.sum())} of {miss.size} rays with another hit count")
    assert miss.mean() >= 0.25
    assert ((hand["hit_count"] != g["custom_inside_ref_hits_count"])[..., 0]).mean() <= 0.01
    # the flavour is per call: the feature entry points keep the unsigned distance, a later pipeline_type 0 call is signed again
    again = oracle.grt_forward(oracle.default_grt_config(primitive_type=5, pipeline_type=2), sc["density12"], sc["sph"], 3, 1e-3, T, *sc["rays"])
    assert np.array_equal(again["hit_count"], slang["hit_count"])


def test_grt_checker_backward_follows_the_forward_convention_for_custom_primitives():
    """orc_grt_trace_bwd at pipeline_type 2 differentiates the hits the unsigned test admits, and only those.  On the camera-inside scene the
    unsigned convention adds hits in FRONT (17 875 against 17 163 accepted), which use up transmittance: no particle becomes visible through it,
    three (67, 233, 284) stop being reached at all - visible sets 80 of 83.  So: of those three one gets a gradient at pipeline_type 0, none does
    at 2; and on a single ray that processes a particle under the unsigned convention only (unsigned_only_pair), an upstream gradient on that ray
    alone gives that particle a gradient at 2 and none at 0.  (The reference's referenceSlangBwdOptix.cu is not built on the host - its per-hit
    backward functions are Slang autodiff output with no restatement in the stand-in - so the Slang backward is pinned through this checker: the
    forward convention against the program's golden above, the per-hit backward shared with the `reference` path, which the hand-written
    backward program's goldens pin.)"""
    sc, T = _custom_inside_scene()
    H, W = sc["H"], sc["W"]
    rng = np.random.default_rng(4)
    g_rad, g_dns = rng.normal(size=(H, W, 3)).astype(np.float32), rng.normal(size=(H, W, 1)).astype(np.float32)
    zero = np.zeros((H, W, 1), np.float32)
    fwd, grad = {}, {}
    for p in (0, 2):
        cfg = oracle.default_grt_config(primitive_type=5, pipeline_type=p)
        fwd[p] = oracle.grt_forward(cfg, sc["density12"], sc["sph"], 3, 1e-3, T, *sc["rays"], dbg_cap=256)
        grad[p] = oracle.grt_backward(cfg, 3, 1e-3, fwd[p], g_rad, g_dns, zero)
    gone = (fwd[0]["visibility"] != 0) & (fwd[2]["visibility"] == 0)
    assert gone.sum() == 3 and not ((fwd[2]["visibility"] != 0) & (fwd[0]["visibility"] == 0)).any()
    # (two of the three are only ever a ray's LAST hit, which the backward program's end-of-ray clip leaves out: no gradient at 0 either)
    assert np.abs(grad[0][0][gone, :11]).max() > 0 and np.abs(grad[2][0][gone]).max() == 0 and np.abs(grad[2][1][gone]).max() == 0
    assert rel_err(grad[2][0][:, :11], grad[0][0][:, :11]) > 1e-3
    ray, pid = unsigned_only_pair(fwd[0], fwd[2])
    m_rad, m_dns = np.zeros_like(g_rad), np.zeros_like(g_dns)
    m_rad.reshape(-1, 3)[ray], m_dns.reshape(-1, 1)[ray] = g_rad.reshape(-1, 3)[ray], g_dns.reshape(-1, 1)[ray]
    one = {p: oracle.grt_backward(oracle.default_grt_config(primitive_type=5, pipeline_type=p), 3, 1e-3, fwd[p], m_rad, m_dns, zero) for p in (0, 2)}
    assert np.abs(one[2][0][pid, :11]).max() > 0 and np.abs(one[0][0][pid]).max() == 0


def test_grt_backward_is_linear_in_the_upstream_gradient_and_separable_by_ray():
    """What tests/parity_util.py: grt_full_parity (stage G) relies on to price the checker's gradient of a frame with some rays' upstream gradient
    zeroed: it is the whole frame's gradient minus a backward over THOSE rays alone (their own rows of the forward's outputs)."""
    scene, T = _grt_scene(n=150, w=12, h=8)
    cfg = oracle.default_grt_config()
    H, W = 8, 12
    rng = np.random.default_rng(5)
    g_rad, g_dns = rng.normal(size=(H, W, 3)).astype(np.float32), rng.normal(size=(H, W, 1)).astype(np.float32)
    zero = np.zeros((H, W, 1), np.float32)
    fwd = oracle.grt_forward(cfg, scene["density12"], scene["sph"], 3, 1e-3, T, *scene["rays"])
    gd, gs = oracle.grt_backward(cfg, 3, 1e-3, fwd, g_rad, g_dns, zero)
    idx = np.array([3, 17, 40, 41, 77])
    mask = np.zeros(H * W, bool)
    mask[idx] = True
    g_rad2, g_dns2 = g_rad.copy().reshape(-1, 3), g_dns.copy().reshape(-1, 1)
    g_rad2[mask] = 0
    g_dns2[mask] = 0
    gd2, gs2 = oracle.grt_backward(cfg, 3, 1e-3, fwd, g_rad2.reshape(H, W, 3), g_dns2.reshape(H, W, 1), zero)
    sub = dict(fwd)
    sub["rays"] = tuple(np.ascontiguousarray(np.asarray(r_, np.float32).reshape(-1, 3)[idx]).reshape(1, -1, 3) for r_ in fwd["rays"])
    for key, width in (("features", 3), ("density", 1), ("hit_distance", 2)):
        sub[key] = np.ascontiguousarray(fwd[key].reshape(-1, width)[idx]).reshape(1, -1, width)
    gd_s, gs_s = oracle.grt_backward(cfg, 3, 1e-3, sub, g_rad.reshape(-1, 3)[idx].reshape(1, -1, 3), g_dns.reshape(-1, 1)[idx].reshape(1, -1, 1),
                                     np.zeros((1, idx.size, 1), np.float32))
    assert np.abs(gd_s).max() > 0
    assert np.abs((gd - gd_s) - gd2).max() <= 1e-5 * np.abs(gd).max() and np.abs((gs - gs_s) - gs2).max() <= 1e-5 * np.abs(gs).max()
