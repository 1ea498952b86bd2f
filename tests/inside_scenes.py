"""Seeded 3DGUT scenes seen from INSIDE the cloud (NumPy only), for tests/test_gut_inside_cpu.py and tests/test_gut_inside_gpu.py.

The orbit scenes of workloads/scenes.py look at a unit-cube shell from a radius of 4: no particle is behind the sensor, nearer than
~2.5 units or larger than 17 of 24 tiles.  Here the sensor sits in a cloud that fills [-1.5, 1.5]^3 (about half of it behind the
sensor), a `near` population lies in the frustum on both sides of the near plane (view_z = 0.2), and a `big` part of it is so large
that sigma points fall behind the sensor plane, boxes cover the whole tile grid and ray origins lie inside particles."""
import importlib
import math

import numpy as np

from scenes import make_scene

syn = importlib.import_module("workloads.synthetic")
camera = importlib.import_module("3dgrut_amd.camera")

EYE, TARGET = (0.1, -0.2, 0.05), (1.0, 0.3, 0.2)
EYE_END, TARGET_END = (0.1 + 0.04, -0.2 - 0.03, 0.05 + 0.02), (1.0, 0.3 + 0.12, 0.2 - 0.05)   # rolling shutter: translates AND rotates
KINDS = ("pinhole", "fisheye", "pinhole_rs")


def make_inside_scene(kind="pinhole", w=96, h=64, n_far=3000, n_near=600, n_big=0, seed=3):
    """The dict of make_scene (density12, sph, batch, cam, pose_start, pose_end, rays, W, H) plus boolean masks `near` (the last
    n_near particles) and `big` (the last n_big of those)."""
    assert kind in KINDS and 0 <= n_big <= n_near
    n = n_far + n_near
    scene = make_scene(n=n, width=w, height=h, median_scale=0.05, seed=seed)   # scales, rotations, densities, SH
    d12 = scene["density12"]
    rng = np.random.default_rng(1000 + seed)
    d12[:, 0:3] = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    pose = syn.lookat_pose(EYE, TARGET)
    fx, fy, cx, cy = scene["batch"]["intrinsics"]
    # near population: camera space, inside (and just outside) the frustum, on both sides of view_z = 0.2
    z = rng.uniform(0.05, 0.7, n_near)
    x = z * (w / (2.0 * fx)) * rng.uniform(-1.4, 1.4, n_near)
    y = z * (h / (2.0 * fy)) * rng.uniform(-1.4, 1.4, n_near)
    R, t = pose[:3, :3].astype(np.float64), pose[:3, 3].astype(np.float64)
    d12[n_far:, 0:3] = (np.stack([x, y, z], -1) @ R.T + t).astype(np.float32)
    d12[n_far:, 8:11] = np.exp(rng.normal(math.log(0.012), 0.7, (n_near, 3))).astype(np.float32)
    if n_big:
        d12[n - n_big:, 8:11] = np.exp(rng.normal(math.log(0.15), 0.5, (n_big, 3))).astype(np.float32)
    b = scene["batch"]
    b["T_to_world"] = pose[None]
    if kind == "fisheye":
        b.pop("intrinsics")
        Kf = syn.fisheye_intrinsics(w, h, fov_deg=170.0)
        Kf["radial_coeffs"] = np.array([0.02, -0.01, 0.003, 0.0], np.float32)
        b["intrinsics_OpenCVFisheyeCameraModelParameters"] = Kf
        ro, rd = syn.fisheye_rays(w, h, dict(Kf, radial_coeffs=np.zeros(4, np.float32)))
        b["rays_ori"], b["rays_dir"] = ro, rd
        scene["rays"] = (ro, rd)
    elif kind == "pinhole_rs":
        b.pop("intrinsics")
        b["intrinsics_OpenCVPinholeCameraModelParameters"] = dict(
            resolution=np.array([w, h], np.uint32), shutter_type="ROLLING_TOP_TO_BOTTOM", principal_point=np.array([cx, cy], np.float32),
            focal_length=np.array([fx, fy], np.float32), radial_coeffs=np.array([0.05, -0.02, 0.0, 0.01, 0.0, 0.0], np.float32),
            tangential_coeffs=np.array([0.002, -0.001], np.float32), thin_prism_coeffs=np.array([0.001, 0.0, -0.001, 0.0], np.float32))
        b["T_to_world_end"] = syn.lookat_pose(EYE_END, TARGET_END)[None]
    scene["cam"], scene["pose_start"], scene["pose_end"] = camera.camera_from_batch(b)
    idx = np.arange(n)
    scene["near"], scene["big"] = idx >= n_far, idx >= n - n_big
    return scene


# The frames of the two test files: name -> make_inside_scene arguments.
SCENES = {
    "pinhole":        dict(kind="pinhole", w=96, h=64, n_far=3000, n_near=600, n_big=0, seed=3),
    "pinhole_big":    dict(kind="pinhole", w=96, h=64, n_far=3000, n_near=600, n_big=48, seed=3),
    "fisheye_big":    dict(kind="fisheye", w=96, h=64, n_far=3000, n_near=600, n_big=48, seed=3),
    "pinhole_rs_big": dict(kind="pinhole_rs", w=96, h=64, n_far=3000, n_near=600, n_big=48, seed=3),
    "pinhole_208":    dict(kind="pinhole", w=208, h=144, n_far=4000, n_near=1200, n_big=0, seed=3),
}
