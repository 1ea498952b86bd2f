"""What tests/test_gut_inside_cpu.py and tests/test_gut_inside_gpu.py share: the scenes of tests/inside_scenes.py built once, the
float32 and float64 oracle frames of each computed once (and left unchanged), and the per-population gradient metric."""
import functools
import importlib

import numpy as np

import oracle
from inside_scenes import SCENES, make_inside_scene

syn = importlib.import_module("workloads.synthetic")

TENSORS = {"position": slice(0, 3), "density": slice(3, 4), "rotation": slice(4, 8), "scale": slice(8, 11)}
# the frames whose backward is also run with a gradient on the hit distance
DEPTH_GRAD = {"pinhole": True, "pinhole_big": False, "fisheye_big": False, "pinhole_rs_big": True, "pinhole_208": False}
# the sorted-hit-buffer frames: (K, scene arguments) - pinhole with big particles
K_SCENES = {"k16": (16, dict(SCENES["pinhole_big"])), "k4": (4, dict(SCENES["pinhole_big"], seed=5))}


@functools.lru_cache(maxsize=None)
def scene(name):
    if name in K_SCENES:
        return make_inside_scene(**K_SCENES[name][1])
    return make_inside_scene(**SCENES[name])


def k_of(name):
    return K_SCENES[name][0] if name in K_SCENES else 0


def upstream(name):
    """(g_fd [H,W,4], g_dist [H,W,1]); g_dist is zero unless the frame is differentiated with a depth gradient."""
    s = scene(name)
    g_fd, g_dist = syn.upstream_grads(s["W"], s["H"])
    g_fd *= s["W"] * s["H"]
    if DEPTH_GRAD.get(name, False):
        g_dist = (np.random.default_rng(5).normal(size=g_dist.shape) * 0.1).astype(np.float32)
    return g_fd, g_dist


@functools.lru_cache(maxsize=None)
def oracle_frame(name, dtype):
    """dict(fwd, grads, cfg) of the oracle in `dtype` (np.float32 / np.float64), forward and backward."""
    s = scene(name)
    cfg = oracle.default_gut_config(k_buffer_size=k_of(name))
    g_fd, g_dist = upstream(name)
    fwd = oracle.gut_forward(cfg, s["cam"], s["pose_start"], s["pose_end"], 3, s["density12"], s["sph"], *s["rays"], dtype=dtype)
    grads = oracle.gut_backward(cfg, s["cam"], 3, fwd, g_fd, g_dist, dtype=dtype)
    return dict(fwd=fwd, grads=grads, cfg=cfg)


def trimmed_rel_err(got, ref, n_drop):
    """||got - ref||inf / ||ref||inf over particles after dropping the n_drop worst particles (test_gut_gpu._trimmed_rel_err)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    per_particle = np.abs(got - ref).reshape(got.shape[0], -1).max(1)
    if n_drop > 0:
        per_particle = np.sort(per_particle)[: max(1, len(per_particle) - n_drop)]
    return float(per_particle.max() / (np.abs(ref).max() + 1e-12))


def population_errors(got, refs, mask):
    """The trimmed gradient metric restricted to the rows of `mask`, each tensor normalised by ITS OWN ||ref||inf over those rows - so
    that the far field, whose gradients are 30 to 1000 times smaller than the near field's, counts.  got = (grad_density12, grad_sph);
    refs = [(grad_density12, grad_sph, n_drop), ...] (the float32 and the float64 oracle: the smaller distance holds, as in
    test_gut_gpu._check_grads).  Returns {tensor: error}."""
    gd, gsph = got
    out = {k: min(trimmed_rel_err(gd[mask][:, sl], rd[mask][:, sl], drop) for rd, _, drop in refs) for k, sl in TENSORS.items()}
    out["sph"] = min(trimmed_rel_err(gsph[mask], rsph[mask], drop) for _, rsph, drop in refs)
    return out


def view_z64(s):
    """view_z of every particle under the mid-exposure pose (what the near-plane cull reads, gutProjector.cuh:131-140), float64."""
    t = oracle.kat_pose_interpolate(s["pose_start"], s["pose_end"], 0.5, dtype=np.float64)   # world -> sensor [t(3), q(x,y,z,w)]
    x, y, z, w = t[3:7] / np.linalg.norm(t[3:7])
    row2 = np.array([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])
    return s["density12"][:, 0:3].astype(np.float64) @ row2 + t[2]


def tile_boxes(s, proj):
    """(width, height) in tiles of every particle's box (gutProjector.cuh tile_space_bbox on the oracle's centre and extent); 0 where
    the particle has no tiles."""
    gx, gy = (s["W"] + 15) // 16, (s["H"] + 15) // 16
    p, e = proj["proj_pos"].astype(np.float64), proj["extent"].astype(np.float64)
    lo = np.floor((p - 0.5 - e) / 16.0).astype(np.int64)
    hi = np.ceil((p - 0.5 + e) / 16.0).astype(np.int64)
    g = np.array([gx, gy])
    wh = np.clip(hi, 0, g) - np.clip(lo, 0, g)
    wh[proj["tiles_count"] == 0] = 0
    return wh[:, 0], wh[:, 1]


def sigma_points_behind(s):
    """Per particle: the number of its 7 sigma points with z <= 0 under the start pose (ut_alpha 1, kappa 0: delta = sqrt(3))."""
    pose = np.asarray(s["batch"]["T_to_world"][0], np.float64)
    d = s["density12"].astype(np.float64)
    w, x, y, z = (d[:, 4 + k] for k in range(4))
    n = np.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)   # [N,3,3], columns = axes
    cnt = np.zeros(len(d), np.int64)
    for k in range(3):
        off = R[:, :, k] * (np.sqrt(3.0) * d[:, 8 + k])[:, None]
        for sgn in (1.0, -1.0):
            cnt += ((d[:, 0:3] + sgn * off - pose[:3, 3]) @ pose[:3, 2]) <= 0
    return cnt


def image_bad_pixels(fd, dist, fwd, tol=1e-4):
    """Boolean [H,W]: the pixels test_gut_gpu._image_checks counts against its flip fraction."""
    d_img = np.abs(fd - fwd["feat_density"]).max(-1)
    d_dist = np.abs(dist - fwd["hit_distance"])[..., 0]
    return (d_img > tol) | (d_dist > tol * np.maximum(1.0, np.abs(fwd["hit_distance"][..., 0])))


@functools.lru_cache(maxsize=None)
def scene_stats(name):
    """Scene statistics from the float32 oracle's projection, and the float32 / float64 oracle-pair distances."""
    s = scene(name)
    o32, o64 = oracle_frame(name, np.float32), oracle_frame(name, np.float64)
    f32, f64 = o32["fwd"], o64["fwd"]
    p = f32["proj"]
    vis, has = p["visibility"] != 0, p["tiles_count"] > 0
    vz, near = view_z64(s), s["near"]
    gx, gy = (s["W"] + 15) // 16, (s["H"] + 15) // 16
    bw, bh = tile_boxes(s, p)
    row = has & (bw <= 4) & (bh <= 4)
    half = has & ~row & (((bw <= 8) & (bh <= 4)) | ((bw <= 4) & (bh <= 8)))
    flips = int((f32["hit_count"] != f64["hit_count"]).sum())
    g32, g64 = o32["grads"], o64["grads"]
    refs = [(g64[0], g64[1], 3 * flips)]
    return dict(
        pixels=s["W"] * s["H"], visible=int(vis.sum()), intersections=int(f32["bins"]["num_intersections"]),
        near_cut=int((near & (vz < 0.2)).sum()), near_cut_visible=int((near & (vz < 0.2) & vis).sum()),
        near_band_visible=int((near & (vz >= 0.2) & (vz < 0.3) & vis).sum()), behind=int((vz < 0).sum()),
        near_plane_gap=float(np.abs(vz - 0.2).min()),
        sigma_behind=int((vis & (sigma_points_behind(s) > 0)).sum()), full_grid=int((p["tiles_count"] == gx * gy).sum()),
        walks=(int(row.sum()), int(half.sum()), int((has & ~row & ~half).sum())), wider8=int((has & (bw > 8)).sum()),
        same_counts=bool(np.array_equal(p["tiles_count"], f64["proj"]["tiles_count"])),
        same_visibility=bool(np.array_equal(p["visibility"], f64["proj"]["visibility"])),
        flips=flips, bad=int(image_bad_pixels(f32["feat_density"], f32["hit_distance"], f64).sum()),
        grad_all=population_errors(g32[:2], refs, np.ones_like(near)), grad_near=population_errors(g32[:2], refs, near),
        grad_far=population_errors(g32[:2], refs, ~near),
        rows_near=int((np.abs(g64[0][near]).max(1) > 0).sum()), rows_far=int((np.abs(g64[0][~near]).max(1) > 0).sum()))


def nht_inputs(name):
    """(features [N,48], g_fd [H,W,25]) of the neural-harmonic-features frame on scene `name` (default feature model)."""
    s = scene(name)
    feats = np.random.default_rng(5).uniform(-np.pi / 2, np.pi / 2, size=(len(s["density12"]), 48)).astype(np.float32)
    g_fd = np.random.default_rng(8).normal(size=(s["H"], s["W"], 25)).astype(np.float32)
    return feats, g_fd


@functools.lru_cache(maxsize=None)
def oracle_nht_frame(name, dtype):
    s = scene(name)
    feats, g_fd = nht_inputs(name)
    cfg = oracle.default_gut_config()
    args = (cfg, s["cam"], s["pose_start"], s["pose_end"], s["density12"], feats, *s["rays"])
    fwd = oracle.gut_forward_nht(*args, dtype=dtype)
    return dict(fwd=fwd, grads=oracle.gut_backward_nht(*args, fwd, g_fd, dtype=dtype))
