"""C-level drivers of tests/test_split_sh_gpu.py and its child process tests/split_sh_child.py: the twin entry points on
cat(albedo, specular) against the split entry points on the two tensors, bit for bit, with NaN-filled guard rows around the two
gradient tensors."""
import ctypes as C
import importlib

import numpy as np
import torch

abi = importlib.import_module("3dgrut_amd._abi")
gt = importlib.import_module("3dgrut_amd.gut_tracer")
scenes = importlib.import_module("workloads.scenes")

W, H = 64, 48
# block and wave edges of the three kernels: 16 particles per wave / 64 per block (fused finalisation), 64 / 128 (two-kernel form),
# 256 per block (projection)
SIZES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 257, 1000)
GUARD = 4   # guard rows on either side: 4 x 12 and 4 x 180 bytes keep the interior slices 16-byte aligned

_scene_cache = {}


def make_split_scene(n):
    """A pinhole scene of workloads.scenes with the cloud shrunk into the view, and every third particle (index 2, 5, ...) mirrored
    behind the camera: particles with and without tiles at known places, among them the last rows of most sizes."""
    if n not in _scene_cache:
        s = scenes.make_scene(n=n, width=W, height=H, median_scale=0.05, seed=11)
        d12 = s["density12"].copy()
        eye = np.asarray(s["batch"]["T_to_world"][0], np.float32)[:3, 3]
        d12[:, :3] *= 0.5
        d12[2::3, :3] = 2.0 * eye - d12[2::3, :3]
        dev = "cuda"
        sph = torch.as_tensor(s["sph"], device=dev)
        rng = np.random.default_rng(5)
        _scene_cache[n] = dict(
            n=n, scene=s, d12=torch.as_tensor(d12, device=dev), sph=sph, albedo=sph[:, :3].clone(), specular=sph[:, 3:].clone(),
            ro=torch.as_tensor(s["rays"][0][0], device=dev).contiguous(), rd=torch.as_tensor(s["rays"][1][0], device=dev).contiguous(),
            g_feat=torch.as_tensor(rng.normal(size=(H, W, 3)).astype(np.float32), device=dev),
            g_opa=torch.as_tensor(rng.normal(size=(H, W, 1)).astype(np.float32), device=dev),
            g_dist=torch.as_tensor((rng.normal(size=(H, W, 1)) * 0.1).astype(np.float32), device=dev))
    return _scene_cache[n]


def native(**render):
    splat = render.pop("splat", {})
    return gt._GutNative(gt.gut_config_from_conf({"render": dict(render, splat=splat)}))


def frame_of(nat, sc, n_active=3, frame_id=7):
    s = sc["scene"]
    return nat.make_frame(frame_id, n_active, sc["n"], H, W, s["cam"], s["pose_start"], s["pose_end"])


def guarded(n, cols):
    """([n, cols] interior slice of a NaN-filled buffer with GUARD rows before and after, the buffer)."""
    buf = torch.full((n + 2 * GUARD, cols), float("nan"), dtype=torch.float32, device="cuda")
    return buf[GUARD:GUARD + n], buf


def assert_guards_intact(buf, n):
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), "a guard row was written"
    assert not bool(torch.isnan(buf[GUARD:GUARD + n]).any()), "a gradient element was left unwritten"


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def backward_split(nat, frame, sc, fd, dist, g_albedo, g_specular, packed, depth, albedo="albedo", specular="specular"):
    """gut_backward_split (packed) / gut_backward_unpacked_split into the caller's two gradient tensors; returns (status, the four
    geometry gradients as [N,3], [N,1], [N,4], [N,3])."""
    n = sc["n"]
    opts = dict(dtype=torch.float32, device="cuda")
    g_dist = sc["g_dist"] if depth else None
    alb = sc[albedo] if isinstance(albedo, str) else albedo
    spec = sc[specular] if isinstance(specular, str) else specular
    if packed:
        g_fd = torch.cat([sc["g_feat"], sc["g_opa"]], dim=-1)
        gd = torch.full((n, 12), float("nan"), **opts)
        rc = nat.lib.gut_backward_split(nat.handle, _stream(), C.byref(frame), _p(sc["d12"]), _p(alb), _p(spec), _p(sc["ro"]), _p(sc["rd"]),
                                        _p(fd), _p(g_fd), _p(dist), _p(g_dist), _p(gd), _p(g_albedo), _p(g_specular))
        return rc, (gd[:, 0:3], gd[:, 3:4], gd[:, 4:8], gd[:, 8:11])
    geo = [torch.full((n, c), float("nan"), **opts) for c in (3, 1, 4, 3)]
    io = abi.GutGradIO(_p(sc["g_feat"]), _p(sc["g_opa"]), _p(geo[0]), _p(geo[1]), _p(geo[2]), _p(geo[3]))
    rc = nat.lib.gut_backward_unpacked_split(nat.handle, _stream(), C.byref(frame), _p(sc["d12"]), _p(alb), _p(spec), _p(sc["ro"]), _p(sc["rd"]),
                                             _p(fd), _p(dist), _p(g_dist), C.byref(io), _p(g_albedo), _p(g_specular))
    return rc, tuple(geo)


def backward_twin(nat, frame, sc, fd, dist, packed, depth):
    g_dist = sc["g_dist"] if depth else None
    if packed:
        gd, gs = nat.trace_bwd(frame, sc["d12"], sc["sph"], sc["ro"], sc["rd"], fd, torch.cat([sc["g_feat"], sc["g_opa"]], dim=-1), dist, g_dist)
        return (gd[:, 0:3], gd[:, 3:4], gd[:, 4:8], gd[:, 8:11]), gs
    *geo, gs = nat.trace_bwd_unpacked(frame, sc["d12"], sc["sph"], sc["ro"], sc["rd"], fd, sc["g_feat"], sc["g_opa"], dist, g_dist)
    return tuple(geo), gs


def check_c_level(nat, n, n_active, packed=False, depth=False):
    """One size, one n_active_features: forward and backward of both kinds; everything equal bit for bit, guards intact, and the
    split backward repeated gives equal bits.  Returns the visibility [N] for the scene guard."""
    sc = make_split_scene(n)
    frame = frame_of(nat, sc, n_active)
    ref_out = nat.trace(frame, sc["d12"], sc["sph"], sc["ro"], sc["rd"])
    ref_geo, ref_gs = backward_twin(nat, frame, sc, ref_out[0], ref_out[1], packed, depth)
    out = nat.trace_split(frame, sc["d12"], sc["albedo"], sc["specular"], sc["ro"], sc["rd"])
    for name, a, b in zip(("feat_density", "hit_distance", "hit_count", "visibility"), out[:4], ref_out[:4]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, n, n_active)
    runs = []
    for _ in range(2):
        (g_alb, alb_buf), (g_spec, spec_buf) = guarded(n, 3), guarded(n, 45)
        rc, geo = backward_split(nat, frame, sc, out[0], out[1], g_alb, g_spec, packed, depth)
        assert rc == abi.GRUT_OK, (rc, nat.lib.grut_last_error())
        torch.cuda.synchronize()
        assert_guards_intact(alb_buf, n)
        assert_guards_intact(spec_buf, n)
        runs.append((g_alb, g_spec, geo))
    g_alb, g_spec, geo = runs[0]
    assert torch.equal(g_alb, ref_gs[:, :3]) and torch.equal(g_spec, ref_gs[:, 3:]), (n, n_active, packed, depth)
    for name, a, b in zip(("positions", "density", "rotation", "scale"), geo, ref_geo):
        assert torch.equal(a, b), (name, n, n_active, packed, depth)
    # coefficients beyond 3 (n_active + 1)^2 get zeros, and so do the rows of particles without tiles
    vis = out[3].view(torch.int32).reshape(-1)
    assert not bool(g_spec[:, 3 * (n_active + 1) ** 2 - 3:].any())
    assert not bool(g_alb[vis == 0].any()) and not bool(g_spec[vis == 0].any())
    assert torch.equal(runs[1][0], g_alb) and torch.equal(runs[1][1], g_spec)
    for a, b in zip(runs[1][2], geo):
        assert torch.equal(a, b)
    return vis
