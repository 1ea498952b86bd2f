"""Seeded whole-frame 3DGUT scenes for the camera paths that workloads/scenes.py: make_camera_scene leaves out (NumPy only), for
tests/test_gut_cameras_gpu.py:

  pinhole_b2t_rot   distorted OpenCV pinhole, rolling bottom-to-top, the sensor ROTATES ~3 degrees and translates during the exposure
  fisheye_r2l_rot   OpenCV fisheye, rolling right-to-left, the sensor rotates ~3 degrees about its own position
  ftheta_a2p_b2t    f-theta with ANGLE_TO_PIXELDIST as the reference polynomial, rolling bottom-to-top (a few centimetres of translation,
                    so that the shutter time of a pixel row changes what is projected)
  ftheta_p2a_global f-theta with PIXELDIST_TO_ANGLE (the Newton refinement) under a global shutter

As in make_camera_scene the projection only drives binning; compositing uses the rays given, so the pinhole and f-theta frames keep
the pinhole ray field and the fisheye frame the exact inverse of its zero-distortion model.  The f-theta forward polynomial is the
series inverse of the backward one (angle = d / f + k3 d^3  <->  d = f angle - k3 f^4 angle^3), as in make_golden.camera_cases()."""
import importlib

import numpy as np

from scenes import make_scene

syn = importlib.import_module("workloads.synthetic")
camera = importlib.import_module("3dgrut_amd.camera")

KINDS = ("pinhole_b2t_rot", "fisheye_r2l_rot", "ftheta_a2p_b2t", "ftheta_p2a_global")
N, W, H, MEDIAN_SCALE = 3000, 96, 64, 0.06


def _orbit_eye(pose):
    return pose[:3, 3].astype(np.float64)


def _ftheta(w, h, f, cx, cy, shutter, reference_poly):
    k3 = 3e-8   # 1 % of the angle at a pixel distance of 50
    return dict(resolution=np.array([w, h], np.uint32), shutter_type=shutter, principal_point=np.array([cx, cy], np.float32),
                reference_poly=reference_poly, pixeldist_to_angle_poly=np.array([0.0, 1.0 / f, 0.0, k3, 0.0, 0.0], np.float32),
                angle_to_pixeldist_poly=np.array([0.0, f, 0.0, -k3 * f ** 4, 0.0, 0.0], np.float32), max_angle=1.2,
                linear_cde=np.array([1.001, 0.0005, -0.0005], np.float32))


def make_camera_path_scene(kind, n=N, w=W, h=H):
    """The dict of make_scene (density12, sph, batch, cam, pose_start, pose_end, rays, W, H) for one of KINDS."""
    assert kind in KINDS
    scene = make_scene(n=n, width=w, height=h, median_scale=MEDIAN_SCALE)
    b = scene["batch"]
    fx, fy, cx, cy = b.pop("intrinsics")
    eye = _orbit_eye(b["T_to_world"][0])
    if kind == "pinhole_b2t_rot":
        b["intrinsics_OpenCVPinholeCameraModelParameters"] = dict(
            resolution=np.array([w, h], np.uint32), shutter_type="ROLLING_BOTTOM_TO_TOP", principal_point=np.array([cx, cy], np.float32),
            focal_length=np.array([fx, fy], np.float32), radial_coeffs=np.array([0.05, -0.02, 0.0, 0.01, 0.0, 0.0], np.float32),
            tangential_coeffs=np.array([0.002, -0.001], np.float32), thin_prism_coeffs=np.array([0.001, 0.0, -0.001, 0.0], np.float32))
        # the sensor looks at the origin from a distance of 4: at the end of the exposure it has moved and looks 0.29 past it (3.0 degrees)
        b["T_to_world_end"] = syn.lookat_pose(eye + np.array([0.05, -0.03, 0.02]), (0.2, -0.18, 0.1))[None]
    elif kind == "fisheye_r2l_rot":
        Kf = syn.fisheye_intrinsics(w, h, fov_deg=120.0)
        Kf["radial_coeffs"] = np.array([0.02, -0.01, 0.003, 0.0], np.float32)
        Kf["shutter_type"] = "ROLLING_RIGHT_TO_LEFT"
        b["intrinsics_OpenCVFisheyeCameraModelParameters"] = Kf
        ro, rd = syn.fisheye_rays(w, h, dict(Kf, radial_coeffs=np.zeros(4, np.float32)))
        b["rays_ori"], b["rays_dir"] = ro, rd
        scene["rays"] = (ro, rd)
        b["T_to_world_end"] = syn.lookat_pose(eye, (-0.12, 0.15, -0.06))[None]
    elif kind == "ftheta_a2p_b2t":
        b["intrinsics_FThetaCameraModelParameters"] = _ftheta(w, h, fx, cx, cy, "ROLLING_BOTTOM_TO_TOP", "ANGLE_TO_PIXELDIST")
        end = b["T_to_world"][0].copy()
        end[:3, 3] += np.array([0.03, 0.04, -0.02], np.float32)
        b["T_to_world_end"] = end[None]
    else:
        b["intrinsics_FThetaCameraModelParameters"] = _ftheta(w, h, fx, cx, cy, "GLOBAL", "PIXELDIST_TO_ANGLE")
    scene["cam"], scene["pose_start"], scene["pose_end"] = camera.camera_from_batch(b)
    return scene
