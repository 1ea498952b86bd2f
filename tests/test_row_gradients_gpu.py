"""Every particle's gradient row of the HIP 3DGUT backward against the f64 oracle, each within its own budget (tests/row_budget.py):

    |gpu - g64| <= (4 C) eps B_T + A_row eps B_1          for every element of every row

The tensor metric of the other gradient tests (||got - ref||inf / ||ref||inf < 1e-3) cannot see a particle whose gradient is small
next to the frame's largest - 60 to 90 % of them on the test scenes; a missed, doubled or stale slot of the gradient sweep hurts
exactly one such row.

Method (stages B and C of parity_util.gut_full_parity at small size): the f32 and the f64 oracle composite the GPU's own tile lists
with the GPU's per-particle radiance and tile counts; pixels whose hit count differs from either oracle or whose image is beyond 1e-4
are masked (at most max(2, 2e-3 pixels)) and receive no upstream gradient on either side; then every row is compared.  A row beyond
its bound is accepted only if the oracle's trace shows an accept decision of that very particle, in an unmasked pixel, within 1e-3 of
its threshold (at most max(2, 2e-3 rows)); every other violation fails with the particle, its tile count, the element and the ratio.

Measured on an MI355X (profiles/row_budget_constants.txt has every case): no case needs an exemption; the largest ratio to the bound is
0.95 (geometry row of a one-tile particle hit once at T = 0.035, per-pixel-origin scene; 0.63 with a depth gradient), every other case stays below 0.3.  Before the
gradient sweep took the closest-point offset from the cross product the position row of a 7 mm thin particle of
the boundary scene stood at 1.08 with a depth gradient and 0.96 without.
"""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import oracle
import row_budget as rb

pytestmark = pytest.mark.gpu


def _fetch_lists(nat, n):
    import torch
    st = nat.stats()
    n_int, tiles = int(st.num_intersections), int(st.num_tiles)
    tc = torch.zeros(n, dtype=torch.int32, device="cuda")
    rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    sidx = torch.zeros(max(n_int, 1), dtype=torch.int32, device="cuda")
    rng = torch.zeros((tiles, 2), dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert nat.lib.gut_debug_fetch(nat.handle, stream, p(tc), None, None, None, None, p(rgb), p(sidx), p(rng)) == 0
    torch.cuda.synchronize()
    return (tc.cpu().numpy().view(np.uint32), rgb.cpu().numpy(), sidx.cpu().numpy().view(np.uint32)[:n_int].copy(),
            rng.cpu().numpy().view(np.uint32))


@functools.lru_cache(maxsize=None)
def _case(name):
    """One forward of configuration `name` on the GPU, the two oracles on its lists, the mask, the masked upstream gradients and the f64
    reference with its budgets.  Computed once per configuration, shared by the tests, never modified."""
    import torch
    conf = rb.CONFIG_BY_NAME[name]
    scene = rb.scene_of(conf.scene)
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    tconf = {"render": dict(conf.render, enable_hitcounts=True)}
    if conf.nht:
        tconf["model"] = rb.NHT_MODEL
    tracer = gt.Tracer(tconf)
    nat = tracer.tracer_wrapper
    n, h, w = len(scene["density12"]), scene["H"], scene["W"]
    frame = nat.make_frame(7, 3, n, h, w, scene["cam"], scene["pose_start"], scene["pose_end"])
    d12 = torch.as_tensor(scene["density12"], device="cuda")
    second = torch.as_tensor(rb.nht_features(n) if conf.nht else scene["sph"], device="cuda")
    ro, rd = (torch.as_tensor(np.asarray(r).reshape(h, w, 3), device="cuda").contiguous() for r in scene["rays"])
    if conf.nht:
        fd, dist, cnt, _, second = nat.trace_nht(frame, d12, second, ro, rd)
    else:
        fd, dist, cnt, _, _, _ = nat.trace(frame, d12, second, ro, rd)
    torch.cuda.synchronize()
    tiles_count, rgb, sidx, rng = _fetch_lists(nat, n)
    # the oracles composite the GPU's candidates: its lists, its per-particle radiance, its tile counts (gut_full_parity's proj_shared)
    cfg = rb.oracle_config(conf)
    if conf.nht:
        proj = dict(tiles_count=tiles_count)
    else:
        own = oracle.gut_project(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], 3, scene["density12"], scene["sph"])
        proj = dict(own, rgb=rgb, tiles_count=tiles_count)
    f32 = rb.oracle_forward(conf, scene, np.float32, proj=proj, lists=(sidx, rng))
    f64 = rb.oracle_forward(conf, scene, np.float64, proj=proj, lists=(sidx, rng))
    fd_h, dist_h, cnt_h = fd.float().cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()[..., 0]
    masked = (cnt_h != rb.hit_count_of(f32)) | (cnt_h != rb.hit_count_of(f64))
    masked |= (np.abs(fd_h - f32["feat_density"]).max(-1) > 1e-4) | (np.abs(dist_h - f32["hit_distance"])[..., 0] > 1e-4)
    assert masked.sum() <= rb.FLIP_CAP(masked.size), f"{name}: {int(masked.sum())} pixels differ from the oracles on identical candidates"
    g_fd, g_dist = rb.upstream(conf, scene)
    g_fd[masked] = 0.0
    g_dist[masked] = 0.0
    ref = rb.oracle_backward(conf, scene, f64, g_fd, g_dist, np.float64)
    gates = None
    if not conf.nht:   # the SH clamp gate on both sides: the radiance the GPU stored, the f64 oracle's own
        cu64 = oracle.gut_project(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], 3, scene["density12"], scene["sph"], dtype=np.float64)["rgb"]
        near = (np.abs(rgb) < 1e-6) | (np.abs(cu64) < 1e-6)
        gates = near & ((rgb > 0) != (cu64 > 0))          # [N,3]: channels the two sides gate differently, within 1e-6 of zero
    return dict(conf=conf, scene=scene, tracer=tracer, nat=nat, frame=frame, d12=d12, second=second, ro=ro, rd=rd, fd=fd, dist=dist,
                g_fd=torch.as_tensor(g_fd, device="cuda"), g_dist=torch.as_tensor(g_dist, device="cuda") if conf.with_depth else None,
                ref=ref, masked=masked, lists=(sidx, rng), tiles_count=tiles_count.astype(np.int64), gates=gates)


def _rows(case, gd, second):
    """The GPU's gradients as row_budget's tensors."""
    gd = gd.cpu().numpy().astype(np.float64)
    got = {k: gd[:, sl] for k, sl in rb.ROWS.items()}
    got["features" if case["conf"].nht else "sph"] = second.cpu().numpy().astype(np.float64)
    return got


def _check_rows(case, got, label):
    conf, (g64, b1, bT, hits) = case["conf"], case["ref"]
    tiles = case["tiles_count"]
    rows_with_gradient = int((bT["geometry"] > 0).sum())
    assert rows_with_gradient > 100
    beyond = {}
    for k, a in got.items():
        a, ref = a.copy(), g64[k]
        if case["gates"] is not None and case["gates"].any():
            # SH clamp gate: a channel within 1e-6 of zero that the two sides gate differently is not compared - its SH columns, and the
            # position row whose direction term it feeds
            if k == "sph":
                skip = np.tile(case["gates"], (1, a.shape[1] // 3))
                a[skip] = ref[skip]
            elif k == "position":
                skip = case["gates"].any(1)
                a[skip] = ref[skip]
        bound = rb.row_bound(conf.family, b1[k], bT[k], tiles, hits)
        ratio = rb.ratio_to_bound(a, ref, bound)
        worst = int(np.argmax(ratio))
        print(f"{label} {k}: largest ratio to the bound {ratio[worst]:.3f} (particle {worst}, {tiles[worst]} tiles), tensor rel err {rb.tensor_rel_err(a, ref):.2e}")
        for p in np.flatnonzero(ratio > 1.0):
            col = int(np.argmax(np.abs(a[p] - ref[p])))
            beyond.setdefault(int(p), []).append(f"particle {p} ({tiles[p]} tiles) {k}[{col}]: gpu {a[p, col]:.9g} oracle {ref[p, col]:.9g}, "
                                                 f"{ratio[p]:.2f} x the bound {bound[p]:.3g}")
    exempt, failures = [], []
    for p, lines in beyond.items():
        near = rb.borderline_entries(conf, case["scene"], case["lists"], p, case["masked"])
        if near:
            exempt.append((p, near[0]))
            print(f"{label} exempt: {'; '.join(lines)} - accept decision at pixel {near[0][0]} within {near[0][1]:+.2e} of its threshold")
        else:
            failures += lines
    assert not failures, f"{label}: {len(failures)} rows beyond their bound with no borderline decision:\n" + "\n".join(failures[:20])
    assert len(exempt) <= rb.EXEMPT_CAP(rows_with_gradient), f"{label}: {len(exempt)} rows needed the borderline exemption"
    return exempt


def _backward(case):
    nat, conf = case["nat"], case["conf"]
    args = (case["frame"], case["d12"], case["second"], case["ro"], case["rd"], case["fd"], case["g_fd"], case["dist"], case["g_dist"])
    return nat.trace_bwd_nht(*args) if conf.nht else nat.trace_bwd(*args)


@pytest.mark.parametrize("name", [c.name for c in rb.CONFIGS])
def test_every_row_within_its_budget(name):
    import torch
    case = _case(name)
    gd, second = _backward(case)
    torch.cuda.synchronize()
    if name.startswith("boundary") and "culling" not in name:
        from test_touch_masks_gpu import COUNTS
        assert list(case["tiles_count"][:len(COUNTS)]) == COUNTS, "the hand-placed particles cover 1, 32, 33, 64, 65 and 192 tiles"
    _check_rows(case, _rows(case, gd, second), name)


def test_packed_unpacked_and_factored_backwards_within_budget():
    """The three ways the SH gradients leave the library (test_touch_masks_gpu.test_backward_paths_agree_bit_for_bit ties them bit for
    bit on another scene), with a depth gradient."""
    import torch
    abi = importlib.import_module("3dgrut_amd._abi")
    case = _case("s3000_depth")
    nat, g = case["nat"], case["g_fd"]
    args = (case["frame"], case["d12"], case["second"], case["ro"], case["rd"], case["fd"])
    gd, gsph = nat.trace_bwd(*args, g, case["dist"], case["g_dist"])
    _check_rows(case, _rows(case, gd, gsph), "packed")
    g_pos, g_dns, g_rot, g_scl, gsph_u = nat.trace_bwd_unpacked(*args, g[..., :3].contiguous(), g[..., 3:].contiguous(), case["dist"], case["g_dist"])
    _check_rows(case, _rows(case, torch.cat([g_pos, g_dns, g_rot, g_scl, torch.zeros_like(g_dns)], 1), gsph_u), "unpacked")
    fgd, fgr = nat.trace_bwd_factored(*args, g, case["dist"], case["g_dist"])
    gsph_f = abi.sph_grad_from_views(fgr.unsqueeze(0), case["d12"], 3, 3)
    torch.cuda.synchronize()
    _check_rows(case, _rows(case, fgd, gsph_f), "factored")
