"""Full-size HIP <-> oracle parity of the 3DGUT path, with every exempted pixel IDENTIFIED (used by tests/test_full_size_gpu.py
and scripts/diag_full_parity.py).

The reference algorithm is discontinuous at its accept / reject thresholds (response > 0.0113, alpha > 1/255, T < 1e-4, the tile
culling of the projection), and both sides evaluate those tests in fp32 with different rounding.  At BASELINE's sizes a frame holds
~3e8 (pixel, particle) evaluations, so some of them land within rounding of a threshold.  The comparison is therefore staged so that
every difference is attributed:

  stage A  projection + binning, integer by integer: per-particle tile counts, depth bits, and the per-tile sorted lists of the
           GPU against the oracle's own (gut_debug_fetch).  Differences here are tile-culling flips; they are counted, bounded, and
           the tiles they touch are known.
  stage B  compositing, on IDENTICAL candidates: the oracle composites the lists the GPU built.  A pixel whose hit count then
           still differs from the GPU's has had an accept / termination flip — that set X is the only exemption of the image
           comparison, it is bounded (<= 0.2 % of the pixels), and every other pixel must agree within 1e-4.
  stage C  gradients: both backward passes run with the upstream gradient zeroed on X (pixels are independent in this algorithm),
           so every gradient contribution compared went through an identical hit sequence; the tolerance is BASELINE's 1e-3
           relative per tensor, no particle is trimmed.
  end-to-end (oracle with its OWN binning, nothing shared): reported, and bounded by the same pixel tolerance outside X and outside
           the tiles stage A found different.
"""
import ctypes as C
import importlib
import os
import time

import numpy as np

import oracle
from scenes import rel_err, torch_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

syn = importlib.import_module("workloads.synthetic")
camera = importlib.import_module("3dgrut_amd.camera")

GRAD_SLICES = {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}


def make_frame_inputs(n, w, h, median_scale, seed=42, view=0, n_views=8, camera_model="pinhole"):
    d12, sph = syn.cloud_trained_like(n, seed=seed, median_scale=median_scale)
    if camera_model == "fisheye":   # OpenCV fisheye with distortion driving the binning, the exact equidistant ray field for the compositing
        Kf = syn.fisheye_intrinsics(w, h, fov_deg=120.0)
        ro, rd = syn.fisheye_rays(w, h, Kf)
        Kf = dict(Kf, radial_coeffs=np.array([0.02, -0.01, 0.003, 0.0], np.float32))
        batch = dict(rays_ori=ro, rays_dir=rd, T_to_world=syn.orbit_pose(view, n_views=n_views)[None], intrinsics_OpenCVFisheyeCameraModelParameters=Kf)
    else:
        K = syn.pinhole_intrinsics(w, h)
        ro, rd = syn.pinhole_rays(w, h, K)
        batch = dict(rays_ori=ro, rays_dir=rd, T_to_world=syn.orbit_pose(view, n_views=n_views)[None], intrinsics=K)
    cam, ps, pe = camera.camera_from_batch(batch)
    return dict(d12=d12, sph=sph, batch=batch, cam=cam, ps=ps, pe=pe, rays=(ro, rd), W=w, H=h, N=n)


def hip_forward(inp, tracer=None, device_pose=False, render=None):
    """One train-mode forward through the plugin; returns images as numpy plus the binning products of that forward.

    device_pose=False: the camera-to-world matrix is handed over as a HOST tensor and the plugin derives the sensor pose exactly as the
    reference plugin does (numpy float64 inverse, float32 quaternion: tracer.py:359-423, pinned by tests/golden/pose.npz).
    device_pose=True: the matrix stays on the GPU (what bench.py and a GPU-resident trainer do) and the library derives the same pose
    there (csrc/gut_poses.hip: float64 LU inverse, one rounding, float32 quaternion, nothing contracted) - since round 4 with the SAME
    bits, so both parametrisations meet the same integer-exact stage A."""
    import torch
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    if tracer is None:
        render = dict(render or {})
        conf = {"render": dict({k: v for k, v in render.items() if k != "splat"}, enable_hitcounts=True, splat=dict(render.get("splat", {})))}
        tracer = gt.Tracer(conf)
    g = syn.SimpleGaussians(inp["d12"], inp["sph"])
    batch = torch_batch(inp["batch"], "cuda")
    if not device_pose:
        batch.T_to_world = torch.as_tensor(inp["batch"]["T_to_world"])
    else:
        assert batch.T_to_world.is_cuda
    out = tracer.render(g, batch, train=True)
    torch.cuda.synchronize()
    nat = tracer.tracer_wrapper
    st = nat.stats()
    N, I, tiles = inp["N"], int(st.num_intersections), int(st.num_tiles)
    dev = dict(device="cuda")
    tc = torch.zeros(N, dtype=torch.int32, **dev)
    depth = torch.zeros(N, dtype=torch.float32, **dev)
    rgb = torch.zeros((N, 3), dtype=torch.float32, **dev)
    sidx = torch.zeros(max(I, 1), dtype=torch.int32, **dev)
    rng = torch.zeros((tiles, 2), dtype=torch.int32, **dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert nat.lib.gut_debug_fetch(nat.handle, stream, p(tc), None, None, None, p(depth), p(rgb), p(sidx), p(rng)) == 0
    torch.cuda.synchronize()
    fd = torch.cat([out["pred_features"], out["pred_opacity"]], dim=-1)[0].detach().cpu().numpy()
    return dict(out=out, gaussians=g, tracer=tracer, fd=fd, dist=out["pred_dist"][0].detach().cpu().numpy(),
                cnt=out["hits_count"][0, ..., 0].detach().cpu().numpy(), vis=out["mog_visibility"].detach().view(-1).bool().cpu().numpy(),
                tiles_count=tc.cpu().numpy().view(np.uint32), depth=depth.cpu().numpy(), rgb=rgb.cpu().numpy(),
                sorted_idx=sidx.cpu().numpy().view(np.uint32)[:I], tile_ranges=rng.cpu().numpy().view(np.uint32), I=I)


def hip_backward(hip, g_fd):
    """Backward of the forward held in `hip` for the upstream gradient g_fd [H,W,4] (no depth gradient: the training path)."""
    import torch
    g = hip["gaussians"]
    g.zero_grad()
    gt_ = torch.as_tensor(g_fd, device="cuda")[None]
    out = hip["out"]
    torch.autograd.backward([out["pred_features"], out["pred_opacity"]], [gt_[..., :3].contiguous(), gt_[..., 3:].contiguous()],
                            retain_graph=True)
    torch.cuda.synchronize()
    return g.grads_packed()


def compare_binning(hip, proj, bins, gx):
    """Stage A.  Returns counts and the boolean per-tile mask of tiles whose sorted list differs from the oracle's."""
    tc_h, tc_o = hip["tiles_count"], proj["tiles_count"]
    both = (tc_h > 0) & (tc_o > 0)
    s = dict(particles_tile_count_differs=int((tc_h != tc_o).sum()), particles_visible_hip=int((tc_h > 0).sum()),
             particles_visible_oracle=int((tc_o > 0).sum()),
             depth_bits_differ=int((hip["depth"].view(np.uint32)[both] != proj["depth"].astype(np.float32).view(np.uint32)[both]).sum()),
             radiance_max_abs_err=float(np.abs(hip["rgb"][both] - proj["rgb"][both]).max()) if both.any() else 0.0,
             I_hip=int(hip["I"]), I_oracle=int(bins["num_intersections"]))
    rh, ro = hip["tile_ranges"].astype(np.int64), bins["tile_ranges"].astype(np.int64)
    tiles = rh.shape[0]
    lh, lo = rh[:, 1] - rh[:, 0], ro[:, 1] - ro[:, 0]
    differs = lh != lo
    sh, so = hip["sorted_idx"], bins["sorted_idx"]
    reordered = 0
    if s["I_hip"] == s["I_oracle"] and np.array_equal(rh, ro) and np.array_equal(sh, so):
        pass  # bit-identical lists: nothing else to look at
    else:
        for t in np.nonzero(~differs)[0]:
            a, b = sh[rh[t, 0]:rh[t, 1]], so[ro[t, 0]:ro[t, 1]]
            if not np.array_equal(a, b):
                differs[t] = True
                reordered += int(np.array_equal(np.sort(a), np.sort(b)))
    s["tiles_total"] = int(tiles)
    s["tiles_list_differs"] = int(differs.sum())
    s["tiles_same_set_other_order"] = int(reordered)
    return s, differs


def pixel_errors(fd, dist, ref_fd, ref_dist):
    """max |d rgb, d opacity| per pixel and the ABSOLUTE hit-distance error (BASELINE.json: RGB / depth within 1e-4 abs; distances
    here are ~4 scene units, a sum over ~100 hits)."""
    d_img = np.abs(fd - ref_fd).max(-1)
    d_dist = np.abs(dist - ref_dist)[..., 0]
    return d_img, d_dist


def _composite(alpha, hit_t, colour, accept, min_T, end_shift=0, K=0, alpha_ref=None, colour_ref=None):
    """The compositing loop (gutKBufferRenderer.cuh:273-352) over one pixel's traced entries with the given accept decisions: K = 0
    composites in list order; K > 0 keeps the K nearest pending hits by hit distance and composites the nearest when the buffer is full
    (HitParticleKBufferT, :62-122), draining what is left at the end of the list.  end_shift toggles the OTHER discontinuity, the end of
    the ray at T < min_transmittance, when the transmittance is within 1e-3 (relative) of the threshold there - T is a product of ~100
    fp32 factors: +1 = the first trigger is ignored (one more hit is composited), -1 = the ray ends at the first hit that leaves T that
    close above the threshold.

    alpha_ref (the float64 alphas of the same entries): also returns S = sum_k |alpha_k - alpha_ref_k| T_k over the composited hits, the
    first-order bound of what the fp32 rounding of the per-hit alphas can move the pixel by (|d opacity| <= S, |d rgb| <= 2 c_max S,
    |d depth| <= 2 t_max S: d out / d alpha_k = T_k (x_k - mean of what lies behind)).  alpha = response * density with response =
    exp(-|v x u|^2 / |v|^2 ...) of canonical-frame vectors of length 1e2..1e3: its fp32 evaluation carries up to ~1e-3 relative noise for
    small distant particles in ANY evaluation order - the reference's CUDA, the float oracle and the HIP kernels each draw their own
    sample of it, the double oracle shows how large it is for the pixel at hand.

    colour_ref (feature path only; the float32 values of what each hit blends, `colour` being the float64 ones): S is returned as the pair
    (S, Sc), Sc = sum_k w_k max|colour_k - colour_ref_k| - the neural harmonic features of a hit are sin / cos of a barycentric
    interpolation AT the hit's canonical intersection point, a position that carries the same fp32 noise as the alpha (a per-particle SH
    colour does not: there Sc = 0)."""
    state = dict(T=1.0, D=0.0, cnt=0, S=0.0, Sc=0.0, alive=True, skip=end_shift > 0)
    C = np.zeros(colour.shape[1] if colour.ndim == 2 else 3)

    def integrate(i):
        a = float(alpha[i])
        w = a * state["T"]
        if alpha_ref is not None:
            state["S"] += abs(a - float(alpha_ref[i])) * state["T"]
        if colour_ref is not None:   # feature path: what a hit blends is itself an fp32 evaluation (sum_k w_k |d colour_k| moves the pixel)
            state["Sc"] += w * float(np.abs(colour[i] - colour_ref[i]).max())
        state["D"] += float(hit_t[i]) * w
        state["T"] *= 1.0 - a
        if w > 0:
            C[:] += w * colour[i]
            state["cnt"] += 1
        T = state["T"]
        if T < min_T:
            if state["skip"] and T > (1.0 - 1e-3) * min_T:
                state["skip"] = False
                return
            state["alive"] = False
        elif end_shift < 0 and T < (1.0 + 1e-3) * min_T:
            state["alive"] = False

    if K == 0:
        for i in np.flatnonzero(accept & (alpha > 0)):
            integrate(i)
            if not state["alive"]:
                break
    else:
        buf = []   # pending hits, ascending in hit distance (ties: the later one goes behind, like the reference's strict `>`)
        for i in np.flatnonzero(accept & (alpha > 0)):
            if len(buf) == K:
                integrate(buf.pop(0))
                if not state["alive"]:
                    break
            pos = len(buf)
            while pos > 0 and not (hit_t[i] > hit_t[buf[pos - 1]]):
                pos -= 1
            buf.insert(pos, i)
        if state["alive"]:
            for i in buf:
                integrate(i)
                if not state["alive"]:
                    break
    return C, 1.0 - state["T"], state["D"], state["cnt"], (state["S"] if colour_ref is None else (state["S"], state["Sc"]))


def identify_flips(cfg, cam, fwd, particle_rgb, pixels, hip_fd, hip_cnt, hip_dist, margin=1e-3, tol=1e-4, tol_half=None, trace_fn=None):
    """For each listed pixel (flat index), finds the smallest set of accept / reject decisions the oracle took within `margin`
    (relative) of their threshold that, taken the other way, reproduces the GPU's pixel: same hit count, colour, opacity AND hit
    distance within `tol` (absolute).  Decisions that close to a threshold are decided by rounding, so such a pixel is an IDENTIFIED
    flip: it is known which particles were toggled.  The transmittance threshold (T < min_transmittance ends the ray) is the other
    discontinuity (see _composite).

    A pixel whose decisions all agree (or agree after the toggles) but whose VALUE is beyond `tol` of the float evaluation is a
    member of the ROUNDING class: it must then lie within `tol` + 3 x the propagated fp32 rounding of its own alphas
    (_composite's S) of the DOUBLE evaluation of the same decisions.

    trace_fn (feature path): callable (pixel, dtype) -> the pixel's trace incl. `colour` [n, channels], the values each entry's hit blends
    (per ray there, not a per-particle table); hip_fd then has channels + 1 columns, the opacity last.

    Returns (toggles per pixel (-1: not reproducible), rounding-class flag per pixel, error / bound ratio per pixel)."""
    import itertools
    min_T = float(cfg.min_transmittance)
    K = int(cfg.k_buffer_size)
    fd = hip_fd.reshape(-1, hip_fd.shape[-1])
    cnt = hip_cnt.reshape(-1)
    dist = hip_dist.reshape(-1)
    out = np.full(len(pixels), -1, np.int32)
    rounding = np.zeros(len(pixels), bool)
    ratio = np.zeros(len(pixels))
    fwd64 = None if trace_fn else dict(fwd, density12=fwd["density12"].astype(np.float64), rays=tuple(r.astype(np.float64) for r in fwd["rays"]),
                                       poses=tuple(p.astype(np.float64) for p in fwd["poses"]))
    for k, pix in enumerate(pixels):
        tr = trace_fn(pix, np.float32) if trace_fn else oracle.gut_pixel_trace(cfg, cam, fwd, pix)
        tr64 = trace_fn(pix, np.float64) if trace_fn else oracle.gut_pixel_trace(cfg, cam, fwd64, pix, dtype=np.float64)
        alpha, hit_t, m = tr["alpha"].astype(np.float64), tr["hit_t"].astype(np.float64), tr["margin"].astype(np.float64)
        alpha64, hit_t64 = tr64["alpha"], tr64["hit_t"]
        colour = tr["colour"].astype(np.float64) if trace_fn else np.maximum(particle_rgb[tr["idx"]].astype(np.float64), 0.0)
        colour64 = tr64["colour"].astype(np.float64) if trace_fn else None
        accept0 = m > 0
        near = np.flatnonzero((np.abs(m) < margin) & (alpha > 0))
        target, tcnt, tdist = fd[pix], int(cnt[pix]), float(dist[pix])
        c_max = float(np.abs(colour).max()) if colour.size else 1.0
        t_max = float(hit_t64.max()) if hit_t64.size else 1.0

        # sorted mode: the k-buffer orders hits by their fp32 hit distance - two hits whose distances agree to rounding (canonical-frame
        # vectors of length 1e2..1e3: ~1e-5 relative between any two evaluation orders) may pop in either order, and with both alphas
        # large the pixel moves by several per cent.  Such a pair is a borderline decision like an accept test at its threshold: the toggle
        # exchanges the two distances.  (K = 0 composites in list order: no such decision exists there.)
        ties = []
        if K > 0:
            live = np.flatnonzero(alpha > 0)
            order = live[np.argsort(hit_t[live], kind="stable")]
            for a_, b_ in zip(order[:-1], order[1:]):
                if abs(hit_t[a_] - hit_t[b_]) <= 2e-5 * max(1.0, abs(hit_t[a_])):
                    ties.append((int(a_), int(b_)))
        toggles_all = [("acc", int(i)) for i in near] + [("swap",) + t for t in ties]

        def matches(acc, end_shift, swaps=()):
            """0: no; 1: the float evaluation of these decisions is within tol; 2: the double evaluation is, up to the propagated rounding"""
            ht, ht64 = hit_t, hit_t64
            if swaps:
                ht, ht64 = hit_t.copy(), hit_t64.copy()
                for a_, b_ in swaps:
                    ht[a_], ht[b_] = ht[b_], ht[a_]
                    ht64[a_], ht64[b_] = ht64[b_], ht64[a_]
            return _matches(acc, end_shift, ht, ht64)

        def _matches(acc, end_shift, hit_t, hit_t64):
            C, opa, D, c, _ = _composite(alpha, hit_t, colour, acc, min_T, end_shift, K)
            # (feature_output_half: the image is the fp32 result rounded to half - half an ulp of the value on top of the tolerance)
            t_rgb = tol + (0.0 if tol_half is None else float(tol_half(np.abs(C).max())))
            t_opa = tol + (0.0 if tol_half is None else float(tol_half(abs(opa))))
            if c == tcnt and np.abs(C - target[:-1]).max() < t_rgb and abs(opa - target[-1]) < t_opa and abs(D - tdist) < tol:
                return 1, 0.0
            if colour64 is not None:   # the double evaluation blends the double features; the float ones bound what their rounding moves
                C, opa, D, c, (S, Sc) = _composite(alpha64, hit_t64, colour64, acc, min_T, end_shift, K, alpha_ref=alpha, colour_ref=colour)
            else:
                (C, opa, D, c, S), Sc = _composite(alpha64, hit_t64, colour, acc, min_T, end_shift, K, alpha_ref=alpha), 0.0
            if c != tcnt:
                return 0, 0.0
            b_rgb, b_opa, b_d = 2.0 * c_max * S + Sc, S, 2.0 * t_max * S
            r = max(np.abs(C - target[:-1]).max() / (t_rgb + 3 * b_rgb), abs(opa - target[-1]) / (t_opa + 3 * b_opa), abs(D - tdist) / (tol + 3 * b_d))
            return (2, float(r)) if r <= 1.0 else (0, float(r))

        found = -1
        for n_toggle in (0, 1, 2, 3):
            for combo in itertools.combinations(toggles_all, n_toggle):
                acc = accept0.copy()
                flip = [t[1] for t in combo if t[0] == "acc"]
                acc[flip] = ~acc[flip]
                swaps = [t[1:] for t in combo if t[0] == "swap"]
                for extra, end_shift in ((0, 0), (1, 1), (1, -1)):
                    how, r = matches(acc, end_shift, swaps)
                    if how == 2 and K > 0:
                        # the double evaluation reproduces the pixel: is it its ORDER of the hits (ties of the fp32 distances resolved as the
                        # float64 distances resolve them), with the fp32 values?  Then this is an order tie - a flip - not a rounding-class pixel
                        C, opa, D, c, _ = _composite(alpha, hit_t64, colour, acc, min_T, end_shift, K)
                        if c == tcnt and np.abs(C - target[:-1]).max() < tol and abs(opa - target[-1]) < tol and abs(D - tdist) < tol:
                            how, extra = 1, extra + 1
                    if how:
                        found = n_toggle + extra
                        rounding[k] = how == 2
                        ratio[k] = r
                        break
                if found >= 0:
                    break
            if found >= 0 or len(toggles_all) < n_toggle + 1:
                break
        out[k] = found
    return out, rounding, ratio


def _pixel_diag(exempt, toggles, rounding, ratio, X, d_img, hip, shared, cap=48):
    """The pixels a verdict hangs on, for analysis off the GPU box (the frame is seeded: the oracle's trace of a pixel can be repeated on
    any host): unidentified pixels, and pixels with EQUAL hit counts beyond 1e-2 - flat index, the GPU's values, the oracle's, and what
    identify_flips concluded."""
    Xf, df = X.reshape(-1), d_img.reshape(-1)
    fd, ofd = hip["fd"].reshape(-1, hip["fd"].shape[-1]), shared["feat_density"].reshape(-1, shared["feat_density"].shape[-1])
    rows = []
    for k, pix in enumerate(exempt):
        if toggles[k] < 0 or (not Xf[pix] and df[pix] > 1e-2):
            rows.append(dict(pix=int(pix), toggles=int(toggles[k]), rounding=bool(rounding[k]), ratio=float(ratio[k]), flip=bool(Xf[pix]),
                             err=float(df[pix]), hip_cnt=float(hip["cnt"].reshape(-1)[pix]), ora_cnt=float(shared["hit_count"].reshape(-1)[pix]),
                             hip_dist=float(hip["dist"].reshape(-1)[pix]), ora_dist=float(shared["hit_distance"].reshape(-1)[pix]),
                             hip_fd=[float(v) for v in fd[pix][:4]] + [float(fd[pix][-1])], ora_fd=[float(v) for v in ofd[pix][:4]] + [float(ofd[pix][-1])]))
    return rows[:cap]


def _half_ulp(x):
    """half an ulp of IEEE half at |x| (the rounding of FEATURE_OUTPUT_HALF)"""
    return 0.5 * np.spacing(np.abs(np.asarray(x, np.float32)).astype(np.float16)).astype(np.float32)


def gut_full_parity(n, w, h, median_scale, seed=42, view=0, log=None, with_backward=True, end_to_end=True, device_pose=False, variant=None):
    """Runs stages A-C (module docstring) and returns a flat dict of the measured statistics.

    variant (non-default configurations at the same size, same staged method): dict with any of
      camera_model = "fisheye"            OpenCV fisheye with distortion (binning) + equidistant rays
      render       = {...}                the plugin's conf.render keys (particle_kernel_degree, splat.k_buffer_size, particle_feature_half ...)
      oracle_cfg   = {...}                the same switches as GutConfig fields of the oracle
      half         = True                 fp16 feature I/O: the oracle reads the rounded coefficients and its image is rounded to half"""
    t_all = time.time()
    variant = variant or {}
    half = bool(variant.get("half"))
    inp = make_frame_inputs(n, w, h, median_scale, seed=seed, view=view, camera_model=variant.get("camera_model", "pinhole"))
    cfg = oracle.default_gut_config(**variant.get("oracle_cfg", {}))
    hip = hip_forward(inp, device_pose=device_pose, render=variant.get("render"))
    if half:
        inp = dict(inp, sph=oracle.round_to_half(inp["sph"]))
    t0 = time.time()
    proj = oracle.gut_project(cfg, inp["cam"], inp["ps"], inp["pe"], 3, inp["d12"], inp["sph"])
    stats = dict(N=n, W=w, H=h, P=w * h, pose="device" if device_pose else "host", variant={k: v for k, v in variant.items()})
    gx = (w + 15) // 16
    # ---- stage A -------------------------------------------------------------------------------------------------------
    own = oracle.gut_forward(cfg, inp["cam"], inp["ps"], inp["pe"], 3, inp["d12"], inp["sph"], *inp["rays"], proj=proj) if end_to_end else None
    bins = own["bins"] if own is not None else oracle.gut_bin(cfg, w, h, proj)
    a, tile_differs = compare_binning(hip, proj, bins, gx)
    stats.update({f"A_{k}": v for k, v in a.items()})
    stats["A_visibility_differs"] = int((hip["vis"] != (proj["visibility"] != 0)).sum())
    # ---- stage B: the oracle composites the GPU's lists -----------------------------------------------------------------
    # (identical candidates = the GPU's lists AND the GPU's per-particle radiance and tile counts, which stage A compared with the
    # oracle's own: a particle that a culling flip gave one tile on the GPU and none in the oracle has no radiance there)
    proj_shared = dict(proj, rgb=hip["rgb"].astype(np.float32), tiles_count=hip["tiles_count"])
    shared = oracle.gut_forward(cfg, inp["cam"], inp["ps"], inp["pe"], 3, inp["d12"], inp["sph"], *inp["rays"], proj=proj_shared,
                                lists=(hip["sorted_idx"], hip["tile_ranges"]))
    if half:   # FEATURE_OUTPUT_HALF: the image is the fp32 image rounded once (rayPayload.cuh:176-186); the backward reads the rounded finals
        unrounded = shared["feat_density"]
        shared = dict(shared, feat_density=oracle.round_to_half(unrounded))
    d_img, d_dist = pixel_errors(hip["fd"], hip["dist"], shared["feat_density"], shared["hit_distance"])
    X = hip["cnt"] != shared["hit_count"][..., 0]                     # identified flips: the hit count differs on identical candidates
    tol_img = 1e-4 + (_half_ulp(np.abs(shared["feat_density"]).max(-1)) * 2.0 if half else 0.0)   # (a value next to a rounding boundary lands one half-ulp step away)
    bad = (d_img > tol_img) | (d_dist > 1e-4)
    # every pixel of X, and every pixel beyond tolerance, must be REPRODUCED by the oracle with at most three of its own borderline
    # decisions (within 1e-3 of a threshold) taken the other way: then it is known which particles flipped
    exempt = np.flatnonzero((X | bad).reshape(-1))
    toggles, rounding, ratio = identify_flips(cfg, inp["cam"], shared, proj_shared["rgb"], exempt, hip["fd"], hip["cnt"], hip["dist"],
                                              tol_half=(lambda v: 2.0 * _half_ulp(v)) if half else None)
    # the exempted pixels are of two classes: FLIPS (an identified accept / termination decision fell the other way) and ROUNDING (every
    # decision agrees, the value is beyond 1e-4 of the float oracle but within 1e-4 + 3 x the propagated fp32 alpha rounding of that
    # very pixel of the double oracle, _composite's S)
    d_img_f, d_dist_f = d_img.reshape(-1), d_dist.reshape(-1)
    pure = rounding & (toggles == 0)   # value-only differences: every decision of the oracle stands (a pixel that needs a toggle AND the rounding
    #                                    allowance is counted with the flips: its distance from the UNtoggled oracle frame is a flip's)
    stats.update(B_flip_pixels=int(X.sum()), B_flip_frac=float(X.mean()), B_bad_pixels=int(bad.sum()),
                 B_bad_outside_flips=int((bad & ~X).sum()), B_exempt_pixels=int(exempt.size), B_exempt_frac=float(exempt.size / X.size),
                 B_exempt_unidentified=int((toggles < 0).sum()), B_exempt_by_toggles={int(t): int((toggles == t).sum()) for t in np.unique(toggles)},
                 B_rounding_class_pixels=int(pure.sum()), B_rounding_after_toggles=int((rounding & ~pure).sum()),
                 B_rounding_class_max_rgb_err=float(d_img_f[exempt][pure].max()) if pure.any() else 0.0,
                 B_rounding_class_max_dist_err=float(d_dist_f[exempt][pure].max()) if pure.any() else 0.0,
                 B_rounding_class_max_ratio_to_bound=float(ratio[rounding].max()) if rounding.any() else 0.0,
                 B_max_rgb_err_outside_flips=float(d_img[~X].max()), B_max_dist_err_outside_flips=float(d_dist[~X].max()),
                 B_max_rgb_err_in_flips=float(d_img[X].max()) if X.any() else 0.0,
                 B_hit_count_l1_in_flips=float(np.abs(hip["cnt"] - shared["hit_count"][..., 0])[X].mean()) if X.any() else 0.0)
    stats["B_diag"] = _pixel_diag(exempt, toggles, rounding, ratio, X, d_img, hip, shared)
    # the largest error on a pixel where NO decision was identified as taken the other way (B_max_rgb_err_outside_flips only excludes the
    # pixels whose hit COUNT differs: an accept flip near the front of a ray that ends at the transmittance threshold displaces the last hit
    # and leaves the count as it was - round 5, sorted mode at 1080p: two such pixels, 0.031 and 0.012, each one decision at
    # alpha = min_alpha to 5e-7 / 3e-5 relative, reproduced to 1e-6 by toggling it)
    identified = np.zeros(d_img_f.shape, bool)
    identified[exempt[toggles > 0]] = True
    stats["B_max_rgb_err_outside_identified_flips"] = float(d_img_f[~identified].max())
    # ---- end to end: the oracle with its own binning ---------------------------------------------------------------------
    if own is not None:
        if half:
            own = dict(own, feat_density=oracle.round_to_half(own["feat_density"]))
        e_img, e_dist = pixel_errors(hip["fd"], hip["dist"], own["feat_density"], own["hit_distance"])
        ty, tx = np.meshgrid(np.arange(h) // 16, np.arange(w) // 16, indexing="ij")
        in_diff_tile = tile_differs[ty * gx + tx]
        Xe = hip["cnt"] != own["hit_count"][..., 0]
        ebad = (e_img > tol_img) | (e_dist > 1e-4)
        stats.update(E_bad_pixels=int(ebad.sum()), E_bad_frac=float(ebad.mean()), E_flip_pixels=int(Xe.sum()),
                     E_pixels_in_differing_tiles=int(in_diff_tile.sum()),
                     E_bad_unexplained=int((ebad & ~Xe & ~in_diff_tile).sum()),
                     E_max_rgb_err_unexplained=float(e_img[~Xe & ~in_diff_tile].max()))
    stats["t_oracle_forward_s"] = time.time() - t0
    # ---- stage C: gradients through identical hit sequences --------------------------------------------------------------
    if with_backward:
        t0 = time.time()
        g_fd, g_dist = syn.upstream_grads(w, h)
        g_fd = g_fd * (w * h)
        g_masked = g_fd.copy()
        g_masked[X | bad] = 0.0
        gd, gsph = hip_backward(hip, g_masked)
        rd, rsph, _ = oracle.gut_backward(cfg, inp["cam"], 3, shared, g_masked, g_dist)
        for k, sl in GRAD_SLICES.items():
            stats[f"C_grad_{k}_rel_err"] = rel_err(gd[:, sl], rd[:, sl])
        stats["C_grad_sph_rel_err"] = rel_err(gsph, rsph)
        stats["C_grad_nonzero_particles"] = int((np.abs(rd[:, :11]).max(1) > 0).sum())
        # unmasked, against the oracle's own frame: what a trainer would see (flips included)
        if own is not None:
            gd2, gsph2 = hip_backward(hip, g_fd)
            rd2, rsph2, _ = oracle.gut_backward(cfg, inp["cam"], 3, own, g_fd, g_dist)
            for k, sl in GRAD_SLICES.items():
                stats[f"E_grad_{k}_rel_err_unmasked"] = rel_err(gd2[:, sl], rd2[:, sl])
            stats["E_grad_sph_rel_err_unmasked"] = rel_err(gsph2, rsph2)
        stats["t_backward_s"] = time.time() - t0
    stats["t_total_s"] = time.time() - t_all
    if log:
        for k, v in stats.items():
            log(f"  {k:38s} {v}")
    return stats


def gut_full_parity_nht(n, w, h, median_scale, seed=42, view=0, log=None, device_pose=True):
    """Neural harmonic features (the reference's default model: 48 = 4 x 12 floats, sincos) at BASELINE size, same stages: A the binning
    as integers (it does not depend on the feature model); B the oracle's orc_gut_render_nht_fwd composites the GPU's lists - pixels whose
    HIT COUNT differs are the flips (an accept / termination decision fell the other way; bounded at 0.2 %), every other pixel must agree
    to 1e-4 up to the rounding class (value-only differences of the fp32 alphas, bounded in number and size like the SH frames'); C the
    gradients w.r.t. particle rows and the feature buffer with the upstream gradient zeroed on the exempted pixels, 1e-3."""
    import torch
    t_all = time.time()
    inp = make_frame_inputs(n, w, h, median_scale, seed=seed, view=view)
    feats = np.random.default_rng(seed + 1).uniform(-np.pi / 2, np.pi / 2, size=(n, 48)).astype(np.float32)   # configs/base_gs.yaml:97-99 init range
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    model = {"feature_type": "nht", "nht_features": {"dim": 48, "activation": {"type": "sincos", "num_frequencies": 1}, "interpolation_type": "barycentric"}}
    tracer = gt.Tracer({"render": {"enable_hitcounts": True, "splat": {}}, "model": model})
    hip = hip_forward(dict(inp, sph=feats), tracer=tracer, device_pose=device_pose)
    cfg = oracle.default_gut_config()
    stats = dict(N=n, W=w, H=h, P=w * h, pose="device" if device_pose else "host", variant="nht")
    proj = oracle.gut_project(cfg, inp["cam"], inp["ps"], inp["pe"], 3, inp["d12"], inp["sph"])
    bins = oracle.gut_bin(cfg, w, h, proj)
    proj_cmp = dict(proj, rgb=hip["rgb"])   # (no per-particle radiance in this mode: nothing to compare there)
    a, _ = compare_binning(hip, proj_cmp, bins, (w + 15) // 16)
    stats.update({f"A_{k}": v for k, v in a.items()})
    shared = oracle.gut_forward_nht(cfg, inp["cam"], inp["ps"], inp["pe"], inp["d12"], feats, *inp["rays"], lists=(hip["sorted_idx"], hip["tile_ranges"]))
    fd = hip["fd"]
    d_img = np.abs(fd - shared["feat_density"]).max(-1)
    d_dist = np.abs(hip["dist"] - shared["hit_distance"])[..., 0]
    X = hip["cnt"] != shared["hit_count"][..., 0]
    bad = (d_img > 1e-4) | (d_dist > 1e-4)
    stats.update(B_flip_pixels=int(X.sum()), B_flip_frac=float(X.mean()), B_bad_pixels=int(bad.sum()), B_bad_outside_flips=int((bad & ~X).sum()),
                 B_max_err_outside_flips=float(d_img[~X].max()), B_max_dist_err_outside_flips=float(d_dist[~X].max()),
                 B_feature_abs_max=float(np.abs(shared["feat_density"][..., :24]).max()))
    # every exempted pixel identified, as on the SH frames (identify_flips): the oracle's own trace of the pixel - per entry the alpha, the
    # hit distance, the accept margin and the 24 feature values its hit would blend - reproduces the GPU's pixel with at most three
    # borderline decisions taken the other way, or is a member of the bounded rounding class
    exempt = np.flatnonzero((X | bad).reshape(-1))
    t0 = time.time()
    rays = tuple(np.ascontiguousarray(r.reshape(h, w, 3)) for r in inp["rays"])
    trace_in = dict(poses=(inp["ps"], inp["pe"]), rays=rays, density12=inp["d12"], nht_features=feats,
                    bins=dict(sorted_idx=shared["sorted_idx"], tile_ranges=shared["tile_ranges"]))
    # (the double traces read float64 copies made ONCE: converting 60 M values per pixel is what took 0.9 s of each 0.9 s trace)
    trace_in64 = dict(trace_in, poses=tuple(np.asarray(p, np.float64) for p in trace_in["poses"]), rays=tuple(r.astype(np.float64) for r in rays),
                      density12=inp["d12"].astype(np.float64), nht_features=feats.astype(np.float64))
    toggles, rounding, ratio = identify_flips(cfg, inp["cam"], trace_in, None, exempt, fd, hip["cnt"], hip["dist"],
                                              trace_fn=lambda pix, dt: oracle.gut_pixel_trace_nht(cfg, inp["cam"], trace_in64 if dt == np.float64 else trace_in, pix, dtype=dt))
    pure = rounding & (toggles == 0)
    d_img_f, d_dist_f = d_img.reshape(-1), d_dist.reshape(-1)
    stats.update(B_exempt_pixels=int(exempt.size), B_exempt_frac=float(exempt.size / X.size), B_exempt_unidentified=int((toggles < 0).sum()),
                 B_exempt_by_toggles={int(t): int((toggles == t).sum()) for t in np.unique(toggles)}, B_rounding_class_pixels=int(pure.sum()),
                 B_rounding_class_max_err=float(d_img_f[exempt][pure].max()) if pure.any() else 0.0,
                 B_rounding_class_max_dist_err=float(d_dist_f[exempt][pure].max()) if pure.any() else 0.0,
                 B_rounding_class_max_ratio_to_bound=float(ratio[rounding].max()) if rounding.any() else 0.0, t_identify_s=time.time() - t0)
    stats["B_diag"] = _pixel_diag(exempt, toggles, rounding, ratio, X, d_img, hip, shared)
    g_fd = np.random.default_rng(seed + 2).normal(size=(h, w, 25)).astype(np.float32)
    g_fd[X | bad] = 0.0
    g = hip["gaussians"]
    g.zero_grad()
    t = torch.as_tensor(g_fd, device="cuda")[None]
    out = hip["out"]
    torch.autograd.backward([out["pred_features"], out["pred_opacity"]], [t[..., :24].contiguous(), t[..., 24:].contiguous()])
    torch.cuda.synchronize()
    gd, gf = g.grads_packed()
    rd, rf = oracle.gut_backward_nht(cfg, inp["cam"], inp["ps"], inp["pe"], inp["d12"], feats, *inp["rays"], shared, g_fd)
    for k, sl in GRAD_SLICES.items():
        stats[f"C_grad_{k}_rel_err"] = rel_err(gd[:, sl], rd[:, sl])
    stats["C_grad_features_rel_err"] = rel_err(gf, rf)
    stats["C_grad_nonzero_particles"] = int((np.abs(rd[:, :11]).max(1) > 0).sum())
    stats["t_total_s"] = time.time() - t_all
    if log:
        for k, v in stats.items():
            log(f"  {k:38s} {v}")
    return stats


def assert_gut_full_parity_nht(stats):
    P, N, tiles = stats["P"], stats["N"], stats["A_tiles_total"]
    assert stats["A_depth_bits_differ"] == 0 and stats["A_tiles_same_set_other_order"] == 0, stats
    assert stats["A_particles_tile_count_differs"] <= max(2, 1e-4 * N) and stats["A_tiles_list_differs"] <= max(2, 2e-2 * tiles), stats
    assert stats["B_exempt_frac"] <= 2e-3, stats
    assert stats["B_exempt_unidentified"] == 0, f"pixels beyond tolerance that no set of borderline decisions explains: {stats}"
    assert stats["B_rounding_class_pixels"] <= max(8, 2e-4 * P), stats
    assert stats["B_rounding_class_max_err"] < 2e-2 and stats["B_rounding_class_max_dist_err"] < 5e-3, stats
    assert stats["B_feature_abs_max"] > 0.3
    for k in list(GRAD_SLICES) + ["features"]:
        assert stats[f"C_grad_{k}_rel_err"] < 1e-3, (k, stats)
    assert stats["C_grad_nonzero_particles"] > 1000


def record_full_parity(name, stats):
    """Appends one configuration's measured statistics (exemption classes included) to gpurun_out/full_parity.json, which travels back
    from the GPU box; the round's copy is committed as profiles/rNN_full_parity.json."""
    import json
    path = os.path.join(ROOT, "gpurun_out", "full_parity.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    try:
        allstats = json.load(open(path))
    except (OSError, ValueError):
        allstats = {}
    allstats[name] = {k: (v if isinstance(v, (int, float, str, dict, list)) else str(v)) for k, v in stats.items()}
    json.dump(allstats, open(path, "w"), indent=1, default=str)


def assert_gut_full_parity(stats, max_flip_frac=2e-3, max_rounding_frac=2e-4):
    """The bar of tests/test_full_size_gpu.py (BASELINE.json: RGB / depth 1e-4 abs, gradients 1e-3 relative)."""
    P, N, tiles = stats["P"], stats["N"], stats["A_tiles_total"]
    # A: binning — integer work
    assert stats["A_depth_bits_differ"] == 0, "depth keys must be bit-identical (they define the per-tile order)"
    assert stats["A_particles_tile_count_differs"] <= max(2, 1e-4 * N), stats
    assert abs(stats["A_I_hip"] - stats["A_I_oracle"]) <= max(2, 1e-4 * stats["A_I_oracle"]), stats
    assert stats["A_tiles_same_set_other_order"] == 0, "a tile holds the same particles in another order"
    assert stats["A_tiles_list_differs"] <= max(2, 2e-2 * tiles), stats
    assert stats["A_visibility_differs"] <= max(2, 1e-4 * N), stats
    assert stats["A_radiance_max_abs_err"] < 1e-5, stats
    # B: compositing on identical candidates
    assert stats["B_exempt_frac"] <= max_flip_frac, stats
    assert stats["B_exempt_unidentified"] == 0, f"pixels beyond tolerance that no set of borderline decisions explains: {stats}"
    assert stats["B_rounding_class_pixels"] <= max(8, max_rounding_frac * P), stats     # value-only differences: a few dozen pixels per frame
    assert stats["B_rounding_class_max_rgb_err"] < 2e-2 and stats["B_rounding_class_max_dist_err"] < 5e-3, stats
    # end to end
    if "E_bad_unexplained" in stats:
        assert stats["E_bad_unexplained"] <= stats["B_bad_outside_flips"], stats   # (the double flips stage B identified)
        assert stats["E_bad_frac"] <= 2.5 * max_flip_frac, stats
    # C: gradients
    if "C_grad_sph_rel_err" in stats:
        for k in list(GRAD_SLICES) + ["sph"]:
            assert stats[f"C_grad_{k}_rel_err"] < 1e-3, (k, stats)
            if f"E_grad_{k}_rel_err_unmasked" in stats:
                # NOT masked: the whole frame against the oracle's own frame, threshold flips included - every flip moves its particle's
                # gradient by about one hit's worth.  Measured <= 4.5e-3 (rotation, 1 M @ 1080p; profiles/rNN_full_parity.json keeps the
                # per-round numbers); the fence is 1e-2, one decade above BASELINE's bar for identical hit sequences (stage C)
                assert stats[f"E_grad_{k}_rel_err_unmasked"] < 1e-2, (k, stats)
        assert stats["C_grad_nonzero_particles"] > 0.05 * stats["A_particles_visible_oracle"]   # (the particles in front of the terminations)


# ---------------------------------------------------------------------------------------------------------------------
# 3DGRT at BASELINE config 3's sizes
# ---------------------------------------------------------------------------------------------------------------------
GRT_PRIMITIVE_CODES = {"instances": 0, "icosahedron": 1, "octahedron": 2, "tetrahedron": 3, "diamond": 4, "custom": 5, "trisurfel": 6, "trihexa": 7, "sphere": 8}


def grt_identify_order_ties(primitive_type, cases, d12, sph, inst, scene_aabb, box8, T_to_world, min_transmittance, tol=1e-4, max_ulp=None):
    """Rays whose colour differs from the reference PROGRAMS' golden although the number of accepted hits is the same: show what each one is.
    cases: [(ray_o[3], ray_d[3] in ray space, particle sequence as the GPU processed it, reference (rgb[3], opacity, integrated distance),
    the GPU's own (rgb[3], opacity, integrated distance))].  Classes:
      tie       ONE transposition of two neighbouring hits of the GPU's sequence (or a permutation inside three neighbouring hits, or two
                transpositions) reproduces the REFERENCE's colour, opacity and distance within `tol` when the checker's processHit composites
                the sequence hit by hit, AND the transposed hits' distances - the checker's candidate arithmetic on a one-particle scene - lie
                within `max_ulp` float32 steps of each other: the reference's intersection program and this library's candidate test round
                the distance differently (referenceOptix.cu:210-246 inserts with a strict <, OptiX leaves the order of equal distances open),
                so hits that close can come out in the other order;
      rounding  no reordering is involved: the GPU's sequence composited in DOUBLE precision lies within 2 tol of the reference AND of the
                GPU's value - two float evaluations of one sequence on opposite sides of the exact value (long sequences; surfels grazed by the ray).
    Returns one record per case with `identified`."""
    import itertools
    # how far apart two hits may be and still come out in the other order: the flat proxies are TRIANGLES to the reference (OptiX's
    # ray-triangle intersection in world space against this library's plane crossing in the proxy frame: measured up to 25 float32 steps
    # on the 1 M frame); the volumetric ones evaluate the same closest-approach formula in two roundings (measured up to 5)
    if max_ulp is None:
        max_ulp = 32 if primitive_type in ("trisurfel", "trihexa", "sphere") else 16
    code = GRT_PRIMITIVE_CODES[primitive_type]
    cfg = oracle.default_grt_config(primitive_type=code)
    M = np.asarray(T_to_world, np.float32)[:3, :4]
    out = []

    def hit_ts(ro, rd, o_w, d_w, pid):
        if primitive_type == "trihexa":   # up to three offers per particle (one per rhombus): every plane crossing, in double
            W = inst[pid][:9].reshape(3, 3).astype(np.float64)
            po, pd = W @ (o_w.astype(np.float64) - inst[pid][9:12]), W @ d_w.astype(np.float64)
            return [float(-po[k] / pd[k]) for k in range(3) if pd[k] != 0]
        if primitive_type == "sphere":    # two offers per particle: both roots of the ray through the enclosing sphere, in double
            r_ = 1.0 / float(inst[pid][0])
            po, pd = (o_w.astype(np.float64) - inst[pid][9:12]) / r_, d_w.astype(np.float64) / r_
            a_, b_, c_ = float(pd @ pd), float(po @ pd), float(po @ po) - 1.0
            disc = b_ * b_ - a_ * c_
            return [(-b_ - disc ** 0.5) / a_, (-b_ + disc ** 0.5) / a_] if disc >= 0 else [float("nan")]
        kw = dict(box8=box8[[pid]]) if primitive_type == "custom" else {}
        o = oracle.grt_forward(cfg, d12[[pid]], sph[[pid]], 3, min_transmittance, T_to_world, ro.reshape(1, 1, 3), rd.reshape(1, 1, 3), inst=inst[[pid]],
                               scene=scene_aabb, **kw)
        return [float(o["hit_distance"][0, 0, 1])]

    def steps(ta, tb):   # float32 steps between the two closest offers
        return min(abs(a - b) / float(np.spacing(np.float32(max(abs(a), abs(b))))) for a in ta for b in tb)

    for ro, rd, seq, ref, gpu in cases:
        ro, rd = np.asarray(ro, np.float32), np.asarray(rd, np.float32)
        o_w = (M[:, :3] @ ro + M[:, 3]).astype(np.float32)
        d_w = (M[:, :3] @ rd).astype(np.float32)
        seq = [int(v) for v in seq]
        scale = max(1.0, abs(float(ref[2])))

        def dist(a, b):
            return max(float(np.abs(np.asarray(a[0], np.float64) - np.asarray(b[0], np.float64)).max()), abs(float(a[1]) - float(b[1])), abs(float(a[2]) - float(b[2])) / scale)

        def comp(order, dtype=np.float32):
            rgb, opa, dst, _ = oracle.grt_composite_sequence(cfg, min_transmittance, o_w, d_w, d12, sph, 3, order, dtype=dtype)
            return rgb, opa, dst

        rec = dict(hits=len(seq), err_as_processed=dist(comp(seq), ref), gpu_vs_reference=dist(gpu, ref), kind=None, identified=False)
        c64 = comp(seq, np.float64)
        rec["double_vs_reference"], rec["double_vs_gpu"] = dist(c64, ref), dist(c64, gpu)
        found, far, best = None, None, (1e30, -1)
        for k in range(len(seq) - 1):   # one transposition
            order = seq[:k] + [seq[k + 1], seq[k]] + seq[k + 2:]
            e = dist(comp(order), ref)
            if e < best[0]:
                best = (e, k)
            if e <= tol:
                if steps(hit_ts(ro, rd, o_w, d_w, seq[k]), hit_ts(ro, rd, o_w, d_w, seq[k + 1])) <= max_ulp:
                    found = ([k, k + 1], e)
                    break
                far = far or ([k, k + 1], e)   # reproduces the reference, but the two hits are not that close: reported, not accepted
        rec["best_single_transposition"] = dict(err=best[0], at=best[1])
        if found is None:
            e_rm = [(dist(comp(seq[:k] + seq[k + 1:]), ref), k) for k in range(len(seq))]
            rec["best_single_removal"] = dict(err=min(e_rm)[0], at=min(e_rm)[1])
        if found is None and far is None:   # three neighbouring hits in another order
            for k in range(len(seq) - 2):
                for perm in itertools.permutations(range(3)):
                    if perm in ((0, 1, 2), (1, 0, 2), (0, 2, 1)):
                        continue
                    order = seq[:k] + [seq[k + q] for q in perm] + seq[k + 3:]
                    e = dist(comp(order), ref)
                    if e <= tol:
                        found = ([k, k + 1, k + 2], e)
                        break
                if found is not None:
                    break
        if found is None and far is None:   # two ties on one ray
            for k in range(len(seq) - 1):
                o1 = seq[:k] + [seq[k + 1], seq[k]] + seq[k + 2:]
                for j in range(k + 2, len(seq) - 1):
                    order = o1[:j] + [o1[j + 1], o1[j]] + o1[j + 2:]
                    e = dist(comp(order), ref)
                    if e <= tol:
                        found = ([k, k + 1, j, j + 1], e)
                        break
                if found is not None:
                    break
        found = found or far
        if found is not None:
            pos = found[0]
            ts = [hit_ts(ro, rd, o_w, d_w, seq[q]) for q in pos]
            gaps = [steps(ts[a], ts[a + 1]) for a in range(len(pos) - 1) if pos[a + 1] == pos[a] + 1]
            rec.update(kind="tie", positions=pos, err_after_reordering=found[1], float_steps_between_reordered_hits=[float(g_) for g_ in gaps],
                       identified=bool(max(gaps) <= max_ulp))
        if not rec["identified"] and max(rec["double_vs_reference"], rec["double_vs_gpu"]) <= 2 * tol:
            for key in ("positions", "err_after_reordering", "float_steps_between_reordered_hits"):   # (a far-apart reordering that happened to fit: not the explanation)
                rec.pop(key, None)
            rec.update(kind="rounding", identified=True)
        out.append(rec)
    return out


def grt_identify_with_reference_log(primitive_type, case, ref_ids, ref_ts, d12, sph, inst, scene_aabb, box8, T_to_world, min_transmittance, tol=1e-4, max_ulp=None):
    """A ray whose value differs from the reference PROGRAMS' golden, explained with the programs' own hit log (round 6;
    tests/golden/fullsize_grt_<prim>_c3_1m_800_hitlog.npz: what every trace returned to the raygen program, in order):
      (1) the CHECKER's processHit composited over the REFERENCE's logged order reproduces the reference's colour, opacity and distance within
          `tol` - the per-hit arithmetic agrees, the difference IS the order;
      (2) every place where the GPU's processed sequence departs from the logged order is one of
            tie        a block of 2-4 neighbouring hits in another order whose distances (the checker's candidate arithmetic) lie within
                       `max_ulp` float32 steps of each other - the two libraries round the same distance differently;
            boundary   a hit the GPU processed that the reference's programs never returned, within `max_ulp` steps of the LAST hit of one of
                       the reference's rounds (log position 16 k - 1): the programs' k-buffer inserts with a strict < and the next trace starts
                       at (last distance + 1e-9) = the last distance itself in fp32, so a candidate that TIES with a round's last hit in the
                       reference's rounding is never returned (referenceOptix.cu:128-130, 210-246) - in this library's rounding it is not a
                       tie and the hit is processed (or the same with the roles exchanged).
    Returns a record with `identified`."""
    if max_ulp is None:
        max_ulp = 32 if primitive_type in ("trisurfel", "trihexa", "sphere") else 16
    ro, rd, seq, ref, gpu = case
    cfg = oracle.default_grt_config(primitive_type=GRT_PRIMITIVE_CODES[primitive_type])
    M = np.asarray(T_to_world, np.float32)[:3, :4]
    ro, rd = np.asarray(ro, np.float32), np.asarray(rd, np.float32)
    o_w = (M[:, :3] @ ro + M[:, 3]).astype(np.float32)
    d_w = (M[:, :3] @ rd).astype(np.float32)
    seq, ref_ids = [int(v) for v in seq], [int(v) for v in ref_ids]
    scale = max(1.0, abs(float(ref[2])))

    def dist(a, b):
        return max(float(np.abs(np.asarray(a[0], np.float64) - np.asarray(b[0], np.float64)).max()), abs(float(a[1]) - float(b[1])), abs(float(a[2]) - float(b[2])) / scale)

    def hit_ts(pid):
        if primitive_type == "trihexa":
            W = inst[pid][:9].reshape(3, 3).astype(np.float64)
            po, pd = W @ (o_w.astype(np.float64) - inst[pid][9:12]), W @ d_w.astype(np.float64)
            return [float(-po[k] / pd[k]) for k in range(3) if pd[k] != 0]
        if primitive_type == "sphere":
            r_ = 1.0 / float(inst[pid][0])
            po, pd = (o_w.astype(np.float64) - inst[pid][9:12]) / r_, d_w.astype(np.float64) / r_
            a_, b_, c_ = float(pd @ pd), float(po @ pd), float(po @ po) - 1.0
            disc = b_ * b_ - a_ * c_
            return [(-b_ - disc ** 0.5) / a_, (-b_ + disc ** 0.5) / a_] if disc >= 0 else [float("nan")]
        kw = dict(box8=box8[[pid]]) if primitive_type == "custom" else {}
        o = oracle.grt_forward(cfg, d12[[pid]], sph[[pid]], 3, min_transmittance, T_to_world, ro.reshape(1, 1, 3), rd.reshape(1, 1, 3), inst=inst[[pid]],
                               scene=scene_aabb, **kw)
        return [float(o["hit_distance"][0, 0, 1])]

    def steps(ta, tb):
        return min(abs(a - b) / float(np.spacing(np.float32(max(abs(a), abs(b))))) for a in ta for b in tb)

    rgb, opa, dst, _ = oracle.grt_composite_sequence(cfg, min_transmittance, o_w, d_w, d12, sph, 3, ref_ids)
    rec = dict(hits=len(seq), logged=len(ref_ids), gpu_vs_reference=dist(gpu, ref), reference_order_composited_vs_reference=dist((rgb, opa, dst), ref), events=[])
    i = j = 0
    ok = rec["reference_order_composited_vs_reference"] <= tol
    while i < len(seq) and j < len(ref_ids):
        if seq[i] == ref_ids[j]:
            i += 1; j += 1
            continue
        done = False
        for m in (2, 3, 4):   # a block of neighbours in another order
            if i + m <= len(seq) and j + m <= len(ref_ids) and sorted(seq[i:i + m]) == sorted(ref_ids[j:j + m]):
                ts = [hit_ts(p_) for p_ in seq[i:i + m]]
                gap = max(steps(ts[a], ts[a + 1]) for a in range(m - 1))
                rec["events"].append(dict(kind="tie", at=i, hits=m, float_steps=float(gap), identified=bool(gap <= max_ulp)))
                i += m; j += m; done = True
                break
        if done:
            continue
        if seq[i] not in ref_ids:       # processed here, never returned to the reference's raygen program
            # (the reference's hit at log position j took the LAST slot of a round, j = 16 k - 1, at a distance that ties with this one's)
            # (... or the round ended just before, at j - 1 = 16 k - 1, and this hit ties with THAT one in the reference's rounding: it lies at or
            # before the next trace's start there, behind it here)
            end = j if j % 16 == 15 else (j - 1 if j % 16 == 0 and j > 0 else -1)
            gap = steps(hit_ts(seq[i]), [float(ref_ts[end])]) if end >= 0 else 1e30
            rec["events"].append(dict(kind="boundary", at=i, particle=seq[i], reference_round_ends_at=end, float_steps=float(gap),
                                      identified=bool(end >= 0 and gap <= max_ulp)))
            i += 1
            continue
        if i == len(seq) - 1 and j + 1 < len(ref_ids) and ref_ids[j + 1] == seq[i] and ref_ids[j] not in seq:
            # a tie at the ray's END: the reference processed Y and stopped on the transmittance threshold with X returned but unprocessed
            # (the log holds what the traces RETURN); here X came first and Y stayed unprocessed behind it - the same two neighbours in the
            # other order, only that the second of them lies behind the end of both processed sequences
            gap = steps(hit_ts(seq[i]), hit_ts(ref_ids[j]))
            rec["events"].append(dict(kind="tie_at_end", at=i, particle=ref_ids[j], float_steps=float(gap), identified=bool(gap <= max_ulp)))
            i += 1; j += 2
            continue
        if ref_ids[j] not in seq:       # returned to the reference's program, not a candidate here: the same tie with the roles exchanged
            end = i if i % 16 == 15 else (i - 1 if i % 16 == 0 and i > 0 else -1)
            gap = steps(hit_ts(ref_ids[j]), hit_ts(seq[end])) if end >= 0 else 1e30
            rec["events"].append(dict(kind="boundary", at=i, particle=ref_ids[j], missing_here=True, round_ends_at=end, float_steps=float(gap),
                                      identified=bool(end >= 0 and gap <= max_ulp)))
            j += 1
            continue
        rec["events"].append(dict(kind="unknown", at=i, identified=False))
        break
    rec["identified"] = bool(ok and rec["events"] and all(e_["identified"] for e_ in rec["events"]))
    rec["kind"] = "+".join(sorted({e_["kind"] for e_ in rec["events"]})) if rec["events"] else None
    return rec


def grt_full_parity(n, w, h, median_scale, seed=42, view=0, ray_stride=1, hit_cap=192, with_backward=True, log=None, wide_stride=0,
                    primitive_type="instances", pipeline_type=None):
    """HIP 3DGRT against the oracle on every `ray_stride`-th ray of the frame (the oracle tests every particle against every
    ray: stride 1 at 100 k particles / 400x400, a >= 4 k-ray subsample at 1 M particles / 800x800).

    The oracle is fed the proxy records the GPU built (`inst`, scene box), so the per-ray ORDER of processed particles can be
    compared bit for bit; the proxies themselves are compared separately (stage P).  Gradients (stride 1 only) are compared
    against the oracle's backward of the same frame.

    primitive_type: render.primitive_type of the plugin and the oracle's candidate test - "icosahedron" is the reference paper's own 3DGRT
    configuration (configs/paper/3dgrt/base_ours_reference.yaml:16; entry distance into the proxy polyhedron), "custom" the world boxes with
    intersectCustomParticle (the oracle gets the GPU's boxes like it gets the GPU's instance records)."""
    import torch
    t_all = time.time()
    grt = importlib.import_module("3dgrut_amd.grt_tracer")
    inp = make_frame_inputs(n, w, h, median_scale, seed=seed, view=view)
    d12, sph = inp["d12"], inp["sph"]
    render_conf = {"enable_hitcounts": True, "primitive_type": primitive_type}
    if pipeline_type:   # render.pipeline_type barycentricSurfels (forward only: stages P, T, W)
        render_conf["pipeline_type"] = pipeline_type
        with_backward = False
    tr = grt.Tracer({"render": dict(render_conf)})
    g = syn.SimpleGaussians(d12, sph)
    tr.build_acc(g, rebuild=True)
    nat = tr.tracer_wrapper
    batch = torch_batch(inp["batch"], "cuda")
    frame = nat.make_frame(0, 3, tr._min_transmittance, n, h, w, batch.T_to_world)
    d12_t = torch.as_tensor(d12, device="cuda").contiguous()
    sph_t = torch.as_tensor(sph, device="cuda").contiguous()
    feat, dns, hit, nrm, cnt, vis, ids, num = nat.trace(frame, d12_t, sph_t, batch.rays_ori.contiguous(), batch.rays_dir.contiguous(),
                                                        hit_capacity=hit_cap)
    inst = nat.instances(n, "cuda").cpu().numpy()
    scene_aabb = np.array(list(nat.stats().scene_aabb), np.float32)
    torch.cuda.synchronize()
    feat, dns, hit, cnt = (t[0].cpu().numpy() for t in (feat, dns, hit, cnt))
    vis = vis.view(torch.int32).reshape(-1).cpu().numpy() != 0
    ids, num = ids.cpu().numpy().view(np.uint32), num.cpu().numpy().astype(np.int64)
    stats = dict(N=n, W=w, H=h, P=w * h, primitive_type=primitive_type)
    cfg = oracle.default_grt_config(primitive_type=GRT_PRIMITIVE_CODES[primitive_type], pipeline_type=1 if pipeline_type == "barycentricSurfels" else 0)
    box_kw = dict(box8=nat.custom_boxes(n, "cuda").cpu().numpy()) if primitive_type == "custom" else {}
    # ---- stage P: proxies ----------------------------------------------------------------------------------------------
    pr = oracle.grt_proxies(cfg, d12[:, 0:3], d12[:, 4:8], d12[:, 8:11], d12[:, 3])
    stats["P_instance_rel_err"] = rel_err(inst, pr["inst"])
    # ---- stage T: traversal order + compositing on the sampled rays -------------------------------------------------------
    sel = np.arange(0, w * h, ray_stride)
    ro, rd = inp["rays"]
    ro_s, rd_s = ro.reshape(-1, 3)[sel][None], rd.reshape(-1, 3)[sel][None]
    T = inp["batch"]["T_to_world"][0]
    t0 = time.time()
    ora = oracle.grt_forward(cfg, d12, sph, 3, tr._min_transmittance, T, ro_s, rd_s, inst=inst, scene=scene_aabb, dbg_cap=hit_cap, **box_kw)
    stats["t_oracle_forward_s"] = time.time() - t0
    o_num = ora["hit_num"].astype(np.int64)
    stats["T_rays_compared"] = int(sel.size)
    stats["T_rays_hit_number_differs"] = int((num[sel] != o_num).sum())
    k = np.minimum(np.minimum(num[sel], o_num), hit_cap)
    col = np.arange(hit_cap)[None, :]
    live = col < k[:, None]
    stats["T_rays_order_differs"] = int(((ids[sel] != ora["hit_ids"]) & live).any(1).sum())
    stats["T_processed_hits_compared"] = int(k.sum())
    stats["T_max_hits_per_ray"] = int(o_num.max())
    differs = np.flatnonzero(((ids[sel] != ora["hit_ids"]) & live).any(1) | (num[sel] != o_num))
    stats["T_diag"] = [dict(ray=int(sel[j]), hip_num=int(num[sel][j]), ora_num=int(o_num[j]), hip_ids=[int(v) for v in ids[sel][j][:min(int(num[sel][j]), hit_cap)]],
                            ora_ids=[int(v) for v in ora["hit_ids"][j][:min(int(o_num[j]), hit_cap)]]) for j in differs[:16]]
    f_s, d_s, h_s, c_s = feat.reshape(-1, 3)[sel], dns.reshape(-1)[sel], hit.reshape(-1, 2)[sel], cnt.reshape(-1)[sel]
    # identified flips: rays whose number of processed or of accepted hits differs (alpha / response / transmittance thresholds of
    # processHit evaluated with different rounding on identical, identically ordered candidates)
    F = (num[sel] != o_num) | (c_s != ora["hit_count"].reshape(-1))
    e_rgb = np.abs(f_s - ora["features"].reshape(-1, 3)).max(-1)
    e_opa = np.abs(d_s - ora["density"].reshape(-1))
    o_hit = ora["hit_distance"].reshape(-1, 2)
    e_dist = (np.abs(h_s - o_hit) / np.maximum(1.0, np.abs(o_hit))).max(-1)
    stats["T_flip_rays"] = int(F.sum())
    stats["T_max_rgb_err_outside_flips_all"] = float(e_rgb[~F].max())
    stats["T_max_opacity_err_outside_flips_all"] = float(e_opa[~F].max())
    stats["T_max_dist_rel_err_outside_flips"] = float(e_dist[~F].max())
    stats["T_max_integrated_depth_rel_err_outside_flips"] = float((np.abs(h_s - o_hit) / np.maximum(1.0, np.abs(o_hit)))[~F, 0].max())
    stats["T_max_last_hit_t_abs_err_outside_flips"] = float(np.abs(h_s - o_hit)[~F, 1].max())
    # BASELINE's bar for the depth is 1e-4 ABSOLUTE on values of ~4: the same rays through the oracle's DOUBLE build tell how far an
    # fp32 evaluation of these very hit sequences is from the exact value (the rounding of the per-hit alphas, see _rounding_bound) —
    # the HIP frame must not be farther from the double oracle than the float oracle is
    ora64 = oracle.grt_forward(cfg, d12, sph, 3, tr._min_transmittance, T, ro_s, rd_s, inst=inst, scene=scene_aabb, dtype=np.float64, **box_kw)
    same = ~F & (ora64["hit_count"].reshape(-1) == ora["hit_count"].reshape(-1))
    # ROUNDING class of this stage (round 6; stage W below has had it since round 5): same sequence, same decisions, the value beyond 1e-4 of
    # the float checker - such a ray must be no farther from the DOUBLE checker than twice the float checker's own distance + 1e-4 (a surfel
    # grazed by the ray: its response is evaluated at gro + grd (-gro.z / grd.z) and the quotient amplifies the last bits of grd.z), and the
    # class is bounded in number by assert_grt_full_parity
    over_t = ~F & ((e_rgb > 1e-4) | (e_opa > 1e-4))
    f64_t, o64_t = ora64["features"].reshape(-1, 3), ora64["density"].reshape(-1)
    d_hip_t = np.maximum(np.abs(f_s - f64_t).max(-1), np.abs(d_s - o64_t))
    d_ora_t = np.maximum(np.abs(ora["features"].reshape(-1, 3) - f64_t).max(-1), np.abs(ora["density"].reshape(-1) - o64_t))
    explained_t = over_t & same & (d_hip_t <= 2.0 * d_ora_t + 1e-4)
    stats["T_rounding_rays"], stats["T_rounding_unexplained"] = int(over_t.sum()), int((over_t & ~explained_t).sum())
    plain = ~F & ~explained_t
    stats["T_max_rgb_err_outside_flips"] = float(e_rgb[plain].max())
    stats["T_max_opacity_err_outside_flips"] = float(e_opa[plain].max())
    d_h32 = np.abs(h_s[:, 0] - o_hit[:, 0])[same]
    d_h64 = np.abs(h_s[:, 0] - ora64["hit_distance"].reshape(-1, 2)[:, 0])[same]
    d_3264 = np.abs(o_hit[:, 0] - ora64["hit_distance"].reshape(-1, 2)[:, 0])[same]
    stats["T_depth_abs_err_hip_vs_f32"] = {q: float(np.quantile(d_h32, float(q))) for q in ("0.5", "0.99", "0.999", "1.0")}
    stats["T_depth_abs_err_hip_vs_f64"] = {q: float(np.quantile(d_h64, float(q))) for q in ("0.5", "0.99", "0.999", "1.0")}
    stats["T_depth_abs_err_f32_vs_f64"] = {q: float(np.quantile(d_3264, float(q))) for q in ("0.5", "0.99", "0.999", "1.0")}
    stats["T_depth_rays_beyond_1e4_abs"] = dict(hip_vs_f32=int((d_h32 > 1e-4).sum()), hip_vs_f64=int((d_h64 > 1e-4).sum()), f32_vs_f64=int((d_3264 > 1e-4).sum()))
    stats["T_max_rgb_err_in_flips"] = float(e_rgb[F].max()) if F.any() else 0.0
    if ray_stride == 1:
        stats["T_visibility_differs"] = int((vis != (ora["visibility"] != 0)).sum())
    # ---- stage W: a much wider ray sample, the oracle's all-pairs scan restricted to each ray's PACKET LIST as the GPU built it ----------
    # (a list holds every particle whose proxy box some ray of the packet can touch; that the restriction changes nothing is CHECKED on the
    # rays of stage T, which went through all pairs: every output of the oracle must be bit-identical with and without it)
    if wide_stride:
        out = tr.render(g, batch, train=True)          # a train-mode forward keeps its lists
        torch.cuda.synchronize()
        ranges_t, entries_t = nat.fetch_lists(w, h, "cuda")
        ranges, entries = ranges_t.cpu().numpy().view(np.uint32), entries_t.cpu().numpy().view(np.uint32)
        gxp = (w + 7) // 8
        packet_of = lambda pix: ((pix // w) // 8) * gxp + (pix % w) // 8
        t0 = time.time()
        oracle.grt_set_candidate_prefilter(ranges, entries, packet_of(sel).astype(np.uint32))
        chk = oracle.grt_forward(cfg, d12, sph, 3, tr._min_transmittance, T, ro_s, rd_s, inst=inst, scene=scene_aabb, dbg_cap=hit_cap, **box_kw)
        stats["W_prefilter_changes_rays"] = int(((chk["hit_ids"] != ora["hit_ids"]).any(1) | (chk["hit_num"] != ora["hit_num"])
                                                 | (chk["features"].reshape(-1, 3) != ora["features"].reshape(-1, 3)).any(1)
                                                 | (chk["hit_distance"].reshape(-1, 2) != ora["hit_distance"].reshape(-1, 2)).any(1)).sum())
        sel2 = np.arange(wide_stride // 2, w * h, wide_stride)
        ro2, rd2 = ro.reshape(-1, 3)[sel2][None], rd.reshape(-1, 3)[sel2][None]
        oracle.grt_set_candidate_prefilter(ranges, entries, packet_of(sel2).astype(np.uint32))
        wide = oracle.grt_forward(cfg, d12, sph, 3, tr._min_transmittance, T, ro2, rd2, inst=inst, scene=scene_aabb, dbg_cap=hit_cap, **box_kw)
        w_num = wide["hit_num"].astype(np.int64)
        kk = np.minimum(np.minimum(num[sel2], w_num), hit_cap)
        live2 = np.arange(hit_cap)[None, :] < kk[:, None]
        F2 = (num[sel2] != w_num) | (cnt.reshape(-1)[sel2] != wide["hit_count"].reshape(-1))
        e_rgb2 = np.abs(feat.reshape(-1, 3)[sel2] - wide["features"].reshape(-1, 3)).max(-1)
        e_opa2 = np.abs(dns.reshape(-1)[sel2] - wide["density"].reshape(-1))
        # ROUNDING class (as on the 3DGUT frames): same sequence, same decisions, value beyond 1e-4 of the float checker.  The surfel's response
        # is evaluated at gro + grd (-gro.z / grd.z): for rays that graze a surfel's plane the quotient amplifies the last bits of grd.z, and the
        # float checker itself sits that far from the exact value - such a ray must be no farther from the DOUBLE checker (same rays, same
        # prefilter) than twice the float checker's own distance + 1e-4, and the class is bounded in number
        over = np.flatnonzero(~F2 & ((e_rgb2 > 1e-4) | (e_opa2 > 1e-4)))
        stats["W_rounding_rays"], stats["W_rounding_unexplained"] = int(over.size), 0
        if 0 < over.size <= 512:
            oracle.grt_set_candidate_prefilter(ranges, entries, packet_of(sel2[over]).astype(np.uint32))
            ro3, rd3 = np.ascontiguousarray(ro2[:, over]), np.ascontiguousarray(rd2[:, over])
            w64 = oracle.grt_forward(cfg, d12, sph, 3, tr._min_transmittance, T, ro3, rd3, inst=inst, scene=scene_aabb, dtype=np.float64, **box_kw)
            f64, o64 = w64["features"].reshape(-1, 3), w64["density"].reshape(-1)
            hip_f, hip_o = feat.reshape(-1, 3)[sel2][over], dns.reshape(-1)[sel2][over]
            ora_f, ora_o = wide["features"].reshape(-1, 3)[over], wide["density"].reshape(-1)[over]
            d_hip = np.maximum(np.abs(hip_f - f64).max(-1), np.abs(hip_o - o64))
            d_ora = np.maximum(np.abs(ora_f - f64).max(-1), np.abs(ora_o - o64))
            same64 = w64["hit_count"].reshape(-1) == wide["hit_count"].reshape(-1)[over]      # (the double checker took the same decisions)
            explained = same64 & (d_hip <= 2.0 * d_ora + 1e-4)
            stats["W_rounding_unexplained"] = int((~explained).sum())
            stats["W_rounding_max_hip_vs_f64"], stats["W_rounding_max_f32_vs_f64"] = float(d_hip.max()), float(d_ora.max())
            keep = np.ones(sel2.size, bool)
            keep[over[explained]] = False
        else:
            keep = np.ones(sel2.size, bool)
        oracle.grt_set_candidate_prefilter()
        stats["t_oracle_wide_s"] = time.time() - t0
        stats.update(W_rays_compared=int(sel2.size), W_list_entries=int(entries.size),
                     W_rays_hit_number_differs=int((num[sel2] != w_num).sum()),
                     W_rays_order_differs=int(((ids[sel2] != wide["hit_ids"]) & live2).any(1).sum()),
                     W_processed_hits_compared=int(kk.sum()), W_flip_rays=int(F2.sum()),
                     W_max_rgb_err_outside_flips=float(e_rgb2[~F2 & keep].max()),
                     W_max_opacity_err_outside_flips=float(e_opa2[~F2 & keep].max()),
                     W_max_last_hit_t_abs_err_outside_flips=float(np.abs(hit.reshape(-1, 2)[sel2] - wide["hit_distance"].reshape(-1, 2))[~F2, 1].max()))
    # ---- stage G: gradients of the whole frame, upstream gradient zeroed on the flipped rays --------------------------------
    if with_backward and ray_stride == 1:
        t0 = time.time()
        rng = np.random.default_rng(4)
        g_rad = rng.normal(size=(h, w, 3)).astype(np.float32)
        g_dns = rng.normal(size=(h, w, 1)).astype(np.float32)
        Fm = F.reshape(h, w)
        g_rad[Fm] = 0.0
        g_dns[Fm] = 0.0
        ora["rays"] = (ora["rays"][0].reshape(1, -1, 3), ora["rays"][1].reshape(1, -1, 3))
        zero_hit = np.zeros((1, w * h, 1), np.float32)
        shifted = np.zeros(w * h, np.uint8)
        rdg, rsg = oracle.grt_backward(cfg, 3, tr._min_transmittance, ora, g_rad.reshape(1, -1, 3), g_dns.reshape(1, -1, 1), zero_hit,
                                       round_shift=shifted)
        shifted = shifted.astype(bool)
        stats["G_round_shift_rays"] = int(shifted.sum())

        def hip_grads(tracer, gr, gdn):
            g.zero_grad()
            out = tracer.render(g, batch, train=True)
            loss = (out["pred_features"][0] * torch.as_tensor(gr, device="cuda")).sum() + (out["pred_opacity"][0] * torch.as_tensor(gdn, device="cuda")).sum()
            loss.backward()
            torch.cuda.synchronize()
            return g.grads_packed()

        # (1) the reference's backward program exactly: the plugin traverses again (render.backward_hit_replay = false)
        tr_exact = grt.Tracer({"render": dict(render_conf, backward_hit_replay=False)})
        tr_exact.build_acc(g, rebuild=True)
        gd, gs = hip_grads(tr_exact, g_rad, g_dns)
        for kname, sl in GRAD_SLICES.items():
            stats[f"G_grad_{kname}_rel_err"] = rel_err(gd[:, sl], rdg[:, sl])
        stats["G_grad_sph_rel_err"] = rel_err(gs, rsg)
        # (2) the default backward (hit-log replay) on the rays where replaying is the same program: upstream gradient also zeroed on
        #     the rays the oracle flags as round-shifted (its backward program's hit set differs from its forward's)
        Sm = shifted.reshape(h, w)
        g_rad2, g_dns2 = g_rad.copy(), g_dns.copy()
        g_rad2[Sm] = 0.0
        g_dns2[Sm] = 0.0
        # the checker's gradient of the masked frame: the backward is linear in the upstream gradient and a ray's contribution depends on that
        # ray alone, so it is the whole frame's gradient minus the contribution of the shifted rays - a backward over THOSE rays only (a few
        # hundred of the frame's) instead of a second pass of every ray against every particle (20-25 s per frame of the suite's 14 minutes)
        idx = np.flatnonzero(shifted)
        if idx.size == 0:
            rdg2, rsg2 = rdg, rsg
        else:
            sub = dict(ora)
            sub["rays"] = (np.ascontiguousarray(ora["rays"][0][:, idx]), np.ascontiguousarray(ora["rays"][1][:, idx]))
            for key, width in (("features", 3), ("density", 1), ("hit_distance", 2)):
                sub[key] = np.ascontiguousarray(ora[key].reshape(-1, width)[idx]).reshape(1, -1, width)
            rd_s, rs_s = oracle.grt_backward(cfg, 3, tr._min_transmittance, sub, np.ascontiguousarray(g_rad.reshape(-1, 3)[idx]).reshape(1, -1, 3),
                                             np.ascontiguousarray(g_dns.reshape(-1, 1)[idx]).reshape(1, -1, 1), np.zeros((1, idx.size, 1), np.float32))
            rdg2, rsg2 = rdg - rd_s, rsg - rs_s
        gd2, gs2 = hip_grads(tr, g_rad2, g_dns2)
        for kname, sl in GRAD_SLICES.items():
            stats[f"G_replay_grad_{kname}_rel_err"] = rel_err(gd2[:, sl], rdg2[:, sl])
        stats["G_replay_grad_sph_rel_err"] = rel_err(gs2, rsg2)
        # (3) the default backward on the whole frame, round-shifted rays included: the forward flags those rays and the backward
        #     re-derives their rounds (grt_trace_bwd_kernel over the frame's packet lists), everything else is replayed
        gd3, gs3 = hip_grads(tr, g_rad, g_dns)
        for kname, sl in GRAD_SLICES.items():
            stats[f"G_replay_unmasked_grad_{kname}_rel_err"] = rel_err(gd3[:, sl], rdg[:, sl])
        stats["G_replay_unmasked_grad_sph_rel_err"] = rel_err(gs3, rsg)
        stats["t_backward_s"] = time.time() - t0
    stats["t_total_s"] = time.time() - t_all
    if log:
        for kk, v in stats.items():
            log(f"  {kk:38s} {v}")
    return stats


def grt_feature_parity(n, w, h, median_scale, seed=42, view=0, ray_stride=149, primitive_type="instances", half=False, log=None):
    """The 3DGRT plugin with neural harmonic features (model.feature_type nht on the Slang pipelines; half = fp16 feature I/O on top) against
    oracle.grt_forward_nht on every `ray_stride`-th ray of a bench-size frame.  The checker gets the GPU's proxy records and scene box (as
    grt_full_parity does) and, with `half`, the rounded feature table; its image is rounded once to half like the kernel's."""
    import torch
    t_all = time.time()
    grt = importlib.import_module("3dgrut_amd.grt_tracer")
    inp = make_frame_inputs(n, w, h, median_scale, seed=seed, view=view)
    d12 = inp["d12"]
    feats = np.random.default_rng(7).uniform(-np.pi / 2, np.pi / 2, size=(n, 48)).astype(np.float32)
    render = {"pipeline_type": "referenceSlang", "enable_hitcounts": True, "primitive_type": primitive_type}
    if half:
        render.update(particle_feature_half=True, feature_output_half=True)
    tr = grt.Tracer({"render": render, "model": {"feature_type": "nht", "nht_features": {"dim": 48, "activation": {"type": "sincos", "num_frequencies": 1},
                                                                                         "interpolation_type": "barycentric"}}})
    g = syn.SimpleGaussians(d12, feats, requires_grad=False)
    tr.build_acc(g, rebuild=True)
    with torch.no_grad():
        out = tr.render(g, torch_batch(inp["batch"], "cuda"))
    nat = tr.tracer_wrapper
    inst = nat.instances(n, "cuda").cpu().numpy()
    aabb = np.array(list(nat.stats().scene_aabb), np.float32)
    f = out["pred_features"][0].cpu().numpy().reshape(w * h, -1)
    dns = out["pred_opacity"][0].cpu().numpy().reshape(-1)
    cnt = out["hits_count"][0].cpu().numpy().reshape(-1)
    sel = np.arange(0, w * h, ray_stride)
    ro, rd = inp["rays"]
    ro_s, rd_s = ro.reshape(-1, 3)[sel][None], rd.reshape(-1, 3)[sel][None]
    cfg = oracle.default_grt_config(primitive_type=GRT_PRIMITIVE_CODES[primitive_type])
    t0 = time.time()
    ora = oracle.grt_forward_nht(cfg, d12, oracle.round_to_half(feats) if half else feats, tr._min_transmittance, inp["batch"]["T_to_world"][0], ro_s, rd_s,
                                 inst=inst, scene=aabb)
    t_or = time.time() - t0
    of = ora["features"].reshape(sel.size, -1)
    if half:
        of = oracle.round_to_half(of)
    # half output: both images are rounded once to half; a value within 1e-4 of a rounding boundary lands one half step (= one ulp of half at
    # that magnitude) away - the allowance is per element, as on the 3DGUT frames (gut_full_parity: tol_img)
    ulp_e = np.spacing(np.abs(of).astype(np.float16)).astype(np.float32) if half else np.zeros_like(of)
    ulp = float(ulp_e.max()) if half else 0.0
    flips = cnt[sel] != ora["hit_count"].reshape(-1)
    err = np.maximum(np.abs(f[sel] - of).max(-1), np.abs(dns[sel] - ora["density"].reshape(-1)))
    bad = (np.abs(f[sel] - of) > 1e-4 + ulp_e).any(-1) | (np.abs(dns[sel] - ora["density"].reshape(-1)) > 1e-4)
    stats = dict(N=n, W=w, H=h, primitive_type=primitive_type, half=bool(half), F_rays_compared=int(sel.size), F_rays_hit_count_differs=int(flips.sum()),
                 F_rays_beyond_tolerance=int(bad.sum()), F_rays_beyond_tolerance_without_a_flip=int((bad & ~flips).sum()),
                 F_max_err_without_a_flip=float(err[~flips].max()) if (~flips).any() else 0.0, F_max_err=float(err.max()),
                 F_half_ulp_allowance=ulp, F_feature_abs_max=float(np.abs(f[sel]).max()), t_oracle_forward_s=t_or, t_total_s=time.time() - t_all)
    if log:
        log(stats)
    return stats


def assert_grt_full_parity(stats):
    assert stats["P_instance_rel_err"] < 5e-6, stats
    if "W_rays_compared" in stats:   # the wide sample through the packet-list prefilter
        assert stats["W_prefilter_changes_rays"] == 0, "restricting the oracle's scan to the GPU's packet lists changed a ray"
        assert stats["W_rays_compared"] >= 64000 and stats["W_rays_order_differs"] == 0, stats
        assert stats["W_flip_rays"] <= max(8, 2e-3 * stats["W_rays_compared"]), stats
        assert stats["W_rounding_rays"] <= max(8, 2e-4 * stats["W_rays_compared"]) and stats["W_rounding_unexplained"] == 0, stats
        assert stats["W_max_rgb_err_outside_flips"] < 1e-4 and stats["W_max_opacity_err_outside_flips"] < 1e-4, stats
        assert stats["W_max_last_hit_t_abs_err_outside_flips"] == 0.0, stats   # the last hit distance is one of the identical candidates' t
    assert stats["T_rays_compared"] >= 2000   # (all-pairs sample: 4296 rays, 2185 for the proxies with the dearest checker test; the wide sample above: >= 64 k)
    assert stats["T_rays_order_differs"] == 0, stats                                   # BVH hit ordering bit-exact
    assert stats["T_processed_hits_compared"] > 10 * stats["T_rays_compared"]
    assert stats["T_flip_rays"] <= max(2, 1e-3 * stats["T_rays_compared"]), stats      # identified compositing flips, bounded
    assert stats["T_rays_hit_number_differs"] <= stats["T_flip_rays"]
    assert stats["T_max_rgb_err_outside_flips"] < 1e-4 and stats["T_max_opacity_err_outside_flips"] < 1e-4, stats
    assert stats.get("T_rounding_unexplained", 0) == 0 and stats.get("T_rounding_rays", 0) <= max(8, 2e-4 * stats["T_rays_compared"]), stats
    assert stats["T_max_last_hit_t_abs_err_outside_flips"] == 0.0, stats   # the last hit distance: bit-exact (same candidate arithmetic)
    # integrated depth, ABSOLUTE: within 1e-4 of the float oracle except where fp32 itself is not — there (a handful of rays) the HIP
    # frame is no farther from the exact (double) value than the float oracle is
    n = stats["T_depth_rays_beyond_1e4_abs"]
    assert n["hip_vs_f32"] <= 2 * n["f32_vs_f64"] + max(3, 1e-4 * stats["T_rays_compared"]), stats
    assert stats["T_depth_abs_err_hip_vs_f64"]["1.0"] <= 2.0 * stats["T_depth_abs_err_f32_vs_f64"]["1.0"] + 1e-4, stats
    assert stats["T_depth_abs_err_hip_vs_f64"]["0.999"] <= 2.0 * stats["T_depth_abs_err_f32_vs_f64"]["0.999"] + 1e-5, stats
    assert stats.get("T_visibility_differs", 0) <= stats["T_flip_rays"], stats
    for kname in list(GRAD_SLICES) + ["sph"]:
        if f"G_grad_{kname}_rel_err" in stats:
            assert stats[f"G_grad_{kname}_rel_err"] < 1e-3, (kname, stats)          # the reference's backward program
            assert stats[f"G_replay_grad_{kname}_rel_err"] < 1e-3, (kname, stats)   # the default (replay) where it is the same program
    if "G_round_shift_rays" in stats:
        assert stats["G_round_shift_rays"] <= 5e-3 * stats["T_rays_compared"], stats
        for kname in list(GRAD_SLICES) + ["sph"]:   # BASELINE's bar for the DEFAULT configuration, no ray exempted but the compositing flips
            assert stats[f"G_replay_unmasked_grad_{kname}_rel_err"] < 1e-3, (kname, stats)


def unsigned_only_pair(signed, unsigned):
    """(ray, particle): a ray of two oracle.grt_forward(..., dbg_cap=...) runs of one scene - `signed` at pipeline_type 0, `unsigned` at 2 - that
    processes `particle` under the unsigned custom hit distance only; of all such pairs the one whose ray processes the fewest hits (so that the
    particle's weight on the ray is as large as it gets)."""
    best = None
    for r in range(unsigned["hit_ids"].shape[0]):
        n0, n2 = int(signed["hit_num"][r]), int(unsigned["hit_num"][r])
        if n2 > unsigned["hit_ids"].shape[1] or n0 > signed["hit_ids"].shape[1]:
            continue
        extra = [int(p) for p in unsigned["hit_ids"][r, :n2] if p not in set(signed["hit_ids"][r, :n0].tolist())]
        if extra and (best is None or n2 < best[0]):
            best = (n2, r, extra[0])
    assert best is not None, "no ray processes a particle under the unsigned convention only"
    return best[1], best[2]
