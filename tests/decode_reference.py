"""The NHT decode stage (grut_decode_forward / grut_decode_backward in include/grut_amd.h, 3dgrut_amd/decoder.py) restated in numpy
float64 on top of tests/mlp_reference.py and tests/mlp_backward_reference.py, the inputs of the bit-equality tests with their rows
assembled in numpy fp32 one rounded operation at a time, the random cases that the CPU and the GPU tests share, and the tolerances
measured on them.  Imports nothing of the product."""
from __future__ import annotations

import collections
import itertools

import numpy as np

import mlp_backward_reference as B
import mlp_reference as R

DecodeConfig = collections.namedtuple("DecodeConfig", "mlp sh_scale unpremultiply_alpha center_ray")   # as decoder.DecodeConfig
ALPHA_MIN = np.float32(1e-8)          # a_s = max(alpha, 1e-8f)
NORM_EPS = 1e-12

# ---- tolerances: the largest absolute deviation of 3dgrut_amd.decoder.decode_torch (fp32, CPU) from this float64 restatement on the
# general-direction cases (GENERAL_CASES: rays, rays with unpremultiply_alpha, centre ray), measured by tests/test_decode_cpu.py (run it
# with -s to see the figures).  The convention and the reasons of mlp_reference.PARITY_TOL: the CPU test allows 2x the constant, the GPU
# tests 4x (the MFMA's k-step order, a contracted rotation, and one flipped bf16 rounding of a hidden activation more).
PARITY_TOL = 2.9e-4                     # the largest over GENERAL_CASES (3 cases of 2050 pixels)                    measured 2.862e-04

# the shapes of the GPU tests, (F, L, hidden layers, width), and the pixel counts
SHAPES = ((3, 1, 1, 64), (24, 3, 3, 128), (55, 4, 2, 128))
SIZES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300)
STRADDLE = (2, 45)                      # B = 2 views of 45 pixels: the second tile of 32 pixels straddles the views


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------
def world_directions(rays_dir, rot, pixels_per_view, center_ray):
    """[P, 3] float64 unit world directions; rot [B, 3, 3]"""
    rot = np.asarray(rot, dtype=np.float64).reshape(-1, 3, 3)
    if center_ray:
        w = np.repeat(rot[:, :, 2], pixels_per_view, axis=0)
    else:
        d = np.asarray(rays_dir, dtype=np.float64).reshape(rot.shape[0], pixels_per_view, 3)
        w = np.einsum("bij,bpj->bpi", rot, d).reshape(-1, 3)
    return w / np.maximum(np.linalg.norm(w, axis=1, keepdims=True), NORM_EPS)


def rows(features, alpha, rays_dir, rot, pixels_per_view, dcfg):
    """-> (the network's rows [P, F + 3] float64, a_s [P] float64 or None)"""
    x = np.asarray(features, dtype=np.float64)
    a_s = None
    if dcfg.unpremultiply_alpha:
        a_s = np.maximum(np.asarray(alpha, dtype=np.float64).reshape(-1), float(ALPHA_MIN))
        x = x / a_s[:, None]
    u = (world_directions(rays_dir, rot, pixels_per_view, dcfg.center_ray) * dcfg.sh_scale + 1.0) * 0.5
    return np.concatenate([x, u], axis=1), a_s


def forward(params, features, alpha, rays_dir, rot, pixels_per_view, dcfg):
    """-> out [P, n_output_dims] float64"""
    x, a_s = rows(features, alpha, rays_dir, rot, pixels_per_view, dcfg)
    with np.errstate(over="ignore"):                                                  # (features / 1e-8f saturate a sigmoid)
        out, _ = R.forward(params, x, dcfg.mlp)
    return out if a_s is None else out * a_s[:, None]


def grad_alpha_from(grad_out, y, gx, x, alpha, a_s):
    """the contract's grad_alpha in float64 from its ingredients, and the sum of magnitudes that its fp32 error bound scales with:
    [alpha >= 1e-8f] (sum_c go_c y_c - (sum_j gx_j x_j) / a_s),  sum_c |go_c y_c| + sum_j |gx_j x_j| / a_s"""
    go, y, gx, x = (np.asarray(t, dtype=np.float64) for t in (grad_out, y, gx, x))
    a_s = np.asarray(a_s, dtype=np.float64)
    gate = np.asarray(alpha, dtype=np.float64).reshape(-1) >= float(ALPHA_MIN)
    value = (go * y).sum(axis=1) - (gx * x).sum(axis=1) / a_s
    magnitude = np.abs(go * y).sum(axis=1) + np.abs(gx * x).sum(axis=1) / a_s
    return np.where(gate, value, 0.0), magnitude


def backward(params, features, alpha, rays_dir, rot, pixels_per_view, grad_out, dcfg):
    """The contract of grut_decode_backward in float64 (dZ rounded to bf16 at the contract's points)
    -> (grad_features [P, F], grad_alpha [P] or None, grad_params)"""
    cfg = dcfg.mlp
    x, a_s = rows(features, alpha, rays_dir, rot, pixels_per_view, dcfg)
    with np.errstate(over="ignore"):
        y, cache = R.forward(params, x, cfg)
    go = np.asarray(grad_out, dtype=np.float64)
    grad_rows, grad_params = B.backward_bf16(cache, go if a_s is None else go * a_s[:, None], cfg)
    gx = grad_rows[:, :cfg.n_features]
    if a_s is None:
        return gx, None, grad_params
    grad_alpha, _ = grad_alpha_from(go, y, gx, x[:, :cfg.n_features], alpha, a_s)
    return gx / a_s[:, None], grad_alpha, grad_params


# ---- inputs on which every direction operation is exact or ONE correctly rounded operation, under any contraction ----------------------------
PYTHAGOREAN = ((2, 3, 6), (1, 4, 8), (4, 4, 7), (3, 4, 0), (1, 2, 2), (2, 6, 9))        # integer vectors of integer length
AXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1))


def signed_permutations():
    """the 48 signed permutation matrices [48, 3, 3]"""
    mats = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3), np.float32)
            for i in range(3):
                m[i, perm[i]] = signs[i]
            mats.append(m)
    return np.stack(mats)


def exact_inputs(n_views, pixels_per_view, n_features, sh_scale, seed):
    """-> dict of fp32 arrays: features [P, F], alpha [P], rays [P, 3], rot [B, 3, 3].  Rotations are signed permutations (different per
    view), rays are integer Pythagorean vectors (axis vectors for a sh_scale that is no power of two), signed, permuted and scaled by
    powers of two; alpha is arbitrary in [1e-3, 1] with 0, 1e-8f and 2^-30 among the first pixels."""
    rng = np.random.default_rng(seed)
    p = n_views * pixels_per_view
    perms = signed_permutations()
    rot = perms[rng.choice(len(perms), size=n_views, replace=False)]
    base = np.array(PYTHAGOREAN if float(sh_scale) in (1.0, 2.0) else AXES, dtype=np.float32)
    rays = base[rng.integers(0, len(base), p)]
    rays = np.take_along_axis(rays, np.argsort(rng.random((p, 3)), axis=1), axis=1)               # permuted
    rays = rays * rng.choice([-1.0, 1.0], (p, 3)).astype(np.float32)                              # signed
    rays = rays * np.ldexp(1.0, rng.integers(-2, 4, (p, 1))).astype(np.float32)                   # scaled by 2^-2 .. 2^3
    alpha = rng.uniform(1e-3, 1.0, p).astype(np.float32)
    special = np.array([0.0, ALPHA_MIN, 2.0 ** -30], np.float32)
    alpha[:min(p, 3)] = special[:min(p, 3)]
    if p > 40:
        alpha[-3:] = special                                                                      # and in the tail tile
    features = rng.normal(0.0, 0.5, (p, n_features)).astype(np.float32)
    return dict(features=features, alpha=alpha, rays=np.ascontiguousarray(rays, np.float32), rot=np.ascontiguousarray(rot, np.float32))


def assemble_rows_fp32(inputs, pixels_per_view, dcfg):
    """The rows [P, F + 3] that the decode stage feeds the network, in numpy fp32, one rounded operation at a time
    -> (rows fp32, a_s fp32 [P] or None).  Asserts that the inputs are of the exact kind: the rotation, the squared length and the
    product with sh_scale are exact, so that a contraction cannot change any rounding."""
    f32 = np.float32
    rot, p = inputs["rot"], inputs["features"].shape[0]
    view = np.arange(p) // pixels_per_view
    if dcfg.center_ray:
        w64 = rot[view][:, :, 2].astype(np.float64)
    else:
        w64 = np.einsum("pij,pj->pi", rot[view].astype(np.float64), inputs["rays"].astype(np.float64))
    w = w64.astype(f32)
    assert np.array_equal(w.astype(np.float64), w64)                                              # exact
    sq64 = (w64 * w64).sum(axis=1)
    length = np.sqrt(sq64.astype(f32))
    assert np.array_equal(sq64.astype(f32).astype(np.float64), sq64) and np.array_equal(length.astype(np.float64) ** 2, sq64)
    length = np.maximum(length, f32(NORM_EPS))
    n = w / length[:, None]                                                                       # ONE rounded fp32 division
    scaled64 = n.astype(np.float64) * float(dcfg.sh_scale)
    scaled = (n * f32(dcfg.sh_scale)).astype(f32)
    assert n.dtype == f32 and np.array_equal(scaled.astype(np.float64), scaled64)                 # exact: fused or not, one rounding follows
    u = ((scaled + f32(1.0)).astype(f32) * f32(0.5)).astype(f32)
    x, a_s = inputs["features"], None
    if dcfg.unpremultiply_alpha:
        a_s = np.maximum(inputs["alpha"], ALPHA_MIN).astype(f32)
        x = (x / a_s[:, None]).astype(f32)                                                        # ONE rounded fp32 division
    out = np.ascontiguousarray(np.concatenate([x, u], axis=1), dtype=f32)
    tiny = np.abs(out[out != 0]).min() if np.count_nonzero(out) else 1.0
    assert np.isfinite(out).all() and tiny >= np.finfo(f32).tiny                                  # no subnormal intermediate
    return out, a_s


# ---- general directions -------------------------------------------------------------------------------------------------------------------------
SHIPPED = R.Config(24, 3, 3, 128, 3, "sigmoid")
GENERAL_SHAPE = (2, 25, 41)             # B, H, W
# name -> (DecodeConfig, seed)
GENERAL_CASES = {
    "shipped_rays": (DecodeConfig(SHIPPED, 3.0, False, False), 41),
    "shipped_rays_unpremultiply": (DecodeConfig(SHIPPED, 3.0, True, False), 42),
    "shipped_center": (DecodeConfig(SHIPPED, 3.0, False, True), 43),
}


def random_rotations(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 2] *= np.sign(np.linalg.det(q))[:, None]
    return q.astype(np.float32)


def general_case(name):
    """-> (dcfg, params fp32, dict of fp32 inputs, pixels_per_view), the same arrays wherever it is called.  Camera rays are NOT unit
    vectors (pinhole rays with z = 1), alpha lies in [0.05, 1]."""
    dcfg, seed = GENERAL_CASES[name]
    rng = np.random.default_rng(seed)
    b, h, w = GENERAL_SHAPE
    p = b * h * w
    params = R.xavier_params(rng, dcfg.mlp)
    rays = np.concatenate([rng.uniform(-0.8, 0.8, (p, 2)), np.ones((p, 1))], axis=1).astype(np.float32)
    inputs = dict(features=rng.normal(0.0, 0.5, (p, dcfg.mlp.n_features)).astype(np.float32),
                  alpha=rng.uniform(0.05, 1.0, p).astype(np.float32), rays=rays, rot=random_rotations(rng, b))
    return dcfg, params, inputs, h * w
