"""Per-row error budgets of the 3DGUT gradients: the bound, its constants and the configurations both row-gradient tests run
(test_row_gradients_cpu.py establishes the constants on the CPU, test_row_gradients_gpu.py applies them to the HIP backward).

The tensor metric ||got - ref||inf / ||ref||inf is blind to every particle whose gradient is small next to the frame's largest -
most of them.  A row-by-row check needs a bound that scales with the row.  Next to every gradient element the oracle can return
(oracle.gut_backward(..., budgets=True))

    B_1 = sum over hits |c|          B_T = sum over hits |c| / T        (c: the hit's contribution, T: transmittance before the hit)

eps * B_1 is the scale of the summation error; eps * B_T the scale of the per-hit arithmetic, which rebuilds the residual radiance
and distance as (final - running) / nextT and so carries an error proportional to 1 / T, not to the hit's own size.

    |gpu - g64| <= (MARGIN * C) * eps * B_T + A_row * eps * B_1          for every element of the row

A ROW is one particle's slice of one gradient tensor - position (3), geometry = density | rotation | scale (8), the SH or feature
row (48), the per-particle radiance gradient (3) - and the row's B_T and B_1 are the LARGEST of its elements' budgets.  Single
elements do not carry a budget of their own: a hit's contribution to one element is itself a sum that cancels (scale_i =
-(1 / s_i) sum_j R_ji M_ij with M = B (x) ((o - mu) - t d): for a particle seen nearly along one of its axes that element's |c| is
1e-9 of its neighbours' while its rounding error is theirs), so an element-wise ratio has no useful maximum (measured: 1.3e6 on the
fisheye scene, 1.3e4 on the 30000-particle scene, each a particle with one such element), while the row-wise one is 62 and 55 on
the two scenes of test_backward_matches_oracle.

C (per sweep family) is the largest row error of the f32 oracle against the f64 oracle on identical hit lists, in units of
eps * B_T, over this module's configurations; it is measured by `python tests/row_budget.py` (which writes
profiles/row_budget_constants.txt) and pinned below.  MARGIN = 4 is the project's margin over a CPU-measured constant (as in the
MLP backward tests): it covers per-hit arithmetic ordered differently from the oracle's.  A_row is derived from the kernels, see
a_row().
"""
import collections
import functools
import importlib
import os
import sys

import numpy as np

if __name__ == "__main__":   # run as a script: the repository root and tests/ on the path, as tests/conftest.py arranges for pytest
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(_here), _here]

import oracle
from scenes import make_camera_scene, make_scene

syn = importlib.import_module("workloads.synthetic")

EPS = 2.0 ** -24
MARGIN = 4.0
TENSOR_BAR = 1e-3                    # the tensor metric's bar everywhere else in the suite
FLIP_CAP = lambda pixels: max(2, 2e-3 * pixels)          # noqa: E731  (test_gut_gpu._check_grads)
EXEMPT_CAP = lambda rows: max(2, 2e-3 * rows)            # noqa: E731
BORDERLINE = 1e-3                    # parity_util.identify_flips: |accept margin| below this is decided by rounding

# Largest f32-vs-f64 row error / (eps * B_T) per family, over CONFIGS (profiles/row_budget_constants.txt has scene, rows, quantiles).
# Recorded values are the measurement rounded up to two digits; test_row_gradients_cpu.py fails when a fresh measurement exceeds them.
C = {
    "k0_sh": 190.0,       # 183.56: fisheye scene, geometry row (next: per-pixel-origin scene 163.76, SH row)
    "k0_depth": 170.0,    # 163.76: per-pixel-origin scene with a depth gradient, SH row
    "kbuf": 890.0,        # 886.50: K = 4, SH row of particle 3531 (K = 16: 688.88, geometry)
    "nht": 150.0,         # 148.30: position row
}

NHT_MODEL = {"feature_type": "nht", "nht_features": {"dim": 48, "activation": {"type": "sincos", "num_frequencies": 1}, "interpolation_type": "barycentric"}}
ROWS = {"position": slice(0, 3), "geometry": slice(3, 11)}        # of the packed [N,12] gradient; geometry = density | rotation | scale

Config = collections.namedtuple("Config", "name family scene cfg_kw render with_depth nht")


def _origin_scene():
    """test_gut_gpu.test_per_pixel_ray_origins_match_oracle's scene: rays that share no origin run the general sweep"""
    scene = make_scene(n=3000, width=80, height=48, median_scale=0.06)
    ro, rd = scene["rays"]
    ro = ro + (np.random.default_rng(11).normal(size=ro.shape) * 0.02).astype(np.float32)
    scene["rays"] = (ro, rd)
    scene["batch"]["rays_ori"] = ro
    return scene


def _boundary():
    from test_touch_masks_gpu import _boundary_scene   # tile counts 1, 32, 33, 64, 65, 192 (imports no GPU code at module level)
    return _boundary_scene()


_SCENES = {
    "s3000": lambda: make_scene(n=3000, width=96, height=64, median_scale=0.06),
    "s30000": lambda: make_scene(n=30000, width=160, height=96, median_scale=0.05),
    "boundary": _boundary,
    # (192 x 128: at the builder's 96 x 64 the 120 degree fisheye samples most particles with one or two pixels, the reference's own row
    # error is then that of single hits whose terms cancel - f32 against f64 oracle 3901 eps B_T, 99.9 % 398, against 184 / 139 here and
    # <= 164 on every other configuration - and one scene would set the family's constant; 128 x 96: 311, 160 x 96 with 3000: 238)
    "fisheye": lambda: make_camera_scene("fisheye", w=192, h=128),
    "pinhole_rs": lambda: make_camera_scene("pinhole_rs"),
    "ftheta": lambda: make_camera_scene("ftheta"),
    "origins": _origin_scene,
    "s4000": lambda: make_scene(n=4000, width=96, height=64, median_scale=0.07),
}


@functools.lru_cache(maxsize=None)
def scene_of(key):
    return _SCENES[key]()


def _cfg(name, family, scene, cfg_kw=None, splat=None, render=None, with_depth=False, nht=False):
    r = dict(render or {})
    r["splat"] = dict(splat or {})
    return Config(name, family, scene, dict(cfg_kw or {}), r, with_depth, nht)


CONFIGS = [
    _cfg("s3000", "k0_sh", "s3000"),
    _cfg("s3000_depth", "k0_depth", "s3000", with_depth=True),
    _cfg("s30000_segments", "k0_sh", "s30000"),
    _cfg("boundary", "k0_sh", "boundary", cfg_kw=dict(tile_based_culling=0), splat=dict(tile_based_culling=False)),
    _cfg("boundary_culling", "k0_sh", "boundary"),
    _cfg("boundary_depth", "k0_depth", "boundary", cfg_kw=dict(tile_based_culling=0), splat=dict(tile_based_culling=False), with_depth=True),
    _cfg("boundary_culling_depth", "k0_depth", "boundary", with_depth=True),
    _cfg("fisheye", "k0_sh", "fisheye"),
    _cfg("pinhole_rs", "k0_sh", "pinhole_rs"),
    _cfg("ftheta", "k0_sh", "ftheta"),
    _cfg("origins", "k0_sh", "origins"),
    _cfg("origins_depth", "k0_depth", "origins", with_depth=True),
    _cfg("degree0", "k0_sh", "s3000", cfg_kw=dict(particle_kernel_degree=0), render=dict(particle_kernel_degree=0)),
    _cfg("degree4", "k0_sh", "s3000", cfg_kw=dict(particle_kernel_degree=4), render=dict(particle_kernel_degree=4)),
    _cfg("k4", "kbuf", "s4000", cfg_kw=dict(k_buffer_size=4), splat=dict(k_buffer_size=4)),
    _cfg("k16", "kbuf", "s4000", cfg_kw=dict(k_buffer_size=16), splat=dict(k_buffer_size=16)),
    _cfg("nht", "nht", "s3000", nht=True),
]
CONFIG_BY_NAME = {c.name: c for c in CONFIGS}
SELF_TEST = {"k0_sh": "s3000", "k0_depth": "s3000_depth", "kbuf": "k4", "nht": "nht"}   # the configuration each family's seeded faults run on


def nht_features(n):
    return np.random.default_rng(5).uniform(-np.pi / 2, np.pi / 2, size=(n, 48)).astype(np.float32)


def upstream(conf, scene):
    """The upstream gradients of the existing gradient tests: (g_fd [H,W,4 | 25], g_dist [H,W,1]; zeros without a depth gradient)."""
    w, h = scene["W"], scene["H"]
    g_fd, g_dist = syn.upstream_grads(w, h)
    g_fd = g_fd * (w * h)
    if conf.nht:
        g_fd = np.random.default_rng(8).normal(size=(h, w, 25)).astype(np.float32)
    if conf.with_depth:
        g_dist = (np.random.default_rng(5).normal(size=g_dist.shape) * 0.1).astype(np.float32)
    else:
        g_dist = np.zeros_like(g_dist)
    return g_fd, g_dist


def oracle_config(conf):
    return oracle.default_gut_config(**conf.cfg_kw)


def _as(dtype, proj):
    return {k: (np.ascontiguousarray(v, dtype) if np.issubdtype(np.asarray(v).dtype, np.floating) else v) for k, v in proj.items()}


def oracle_forward(conf, scene, dtype, proj=None, lists=None):
    """The oracle's forward in `dtype`; proj / lists given: composites THOSE candidates (another run's, or the GPU's)."""
    cfg = oracle_config(conf)
    s = scene
    if conf.nht:
        feats = nht_features(len(s["density12"]))
        fwd = oracle.gut_forward_nht(cfg, s["cam"], s["pose_start"], s["pose_end"], s["density12"], feats, *s["rays"], dtype=dtype, lists=lists)
        fwd["tiles_count"] = proj["tiles_count"] if proj is not None else fwd["proj"]["tiles_count"]
        return fwd
    return oracle.gut_forward(cfg, s["cam"], s["pose_start"], s["pose_end"], 3, s["density12"], s["sph"], *s["rays"], dtype=dtype,
                              proj=None if proj is None else _as(dtype, proj), lists=lists)


def lists_of(conf, fwd):
    return (fwd["sorted_idx"], fwd["tile_ranges"]) if conf.nht else (fwd["bins"]["sorted_idx"], fwd["bins"]["tile_ranges"])


def tiles_count_of(conf, fwd):
    return np.asarray(fwd["tiles_count"] if conf.nht else fwd["proj"]["tiles_count"]).astype(np.int64)


def hit_count_of(fwd):
    return fwd["hit_count"][..., 0]


def oracle_backward(conf, scene, fwd, g_fd, g_dist, dtype):
    """({tensor: gradient [N, columns]}, {tensor: B_1 [N]}, {tensor: B_T [N]}, hits [N]) of the forward `fwd`: per tensor the rows'
    gradients and the rows' budgets (the largest of the row's elements), and the number of hits the oracle differentiated per particle.
    Tensors: position, geometry and sph + rgb (the per-particle radiance gradient) or features."""
    cfg = oracle_config(conf)
    s = scene
    if conf.nht:
        feats = nht_features(len(s["density12"]))
        gd, gf, b = oracle.gut_backward_nht(cfg, s["cam"], s["pose_start"], s["pose_end"], s["density12"], feats, *s["rays"], fwd, g_fd,
                                            g_dist if conf.with_depth else None, dtype=dtype, budgets=True)
        second = {"features": (gf, b["f1"], b["fT"])}
    else:
        gd, gsph, grgb, b = oracle.gut_backward(cfg, s["cam"], 3, fwd, g_fd, g_dist, dtype=dtype, budgets=True)
        second = {"sph": (gsph, b["sph1"], b["sphT"]), "rgb": (grgb, b["rgb1"], b["rgbT"])}
    g, b1, bT = {}, {}, {}
    for k, sl in ROWS.items():
        g[k], b1[k], bT[k] = gd[:, sl].astype(np.float64), b["d1"][:, sl].max(1), b["dT"][:, sl].max(1)
    for k, (a, x1, xT) in second.items():
        g[k], b1[k], bT[k] = a.astype(np.float64), x1.max(1), xT.max(1)
    return g, b1, bT, b["hits"]


# ----------------------------------------------------------------------------------------------------------------------------
# A_row: the number of f32 additions on the longest path of a row's sum, read from the kernels.
#
# K = 0 sweeps (SH: csrc/gut_render.hip render_bwd_sweep; features: csrc/gut_render_nht.inl, the same reduction).  A hit's terms of
# one (tile entry, half tile) task are summed over the wave's 128 pixels in f32:
#   terms[k] = pixel 0 + pixel 1 of the lane                                   1 addition      (gut_render.hip "terms[0] = B.x.x + B.x.y")
#   part = col[0]; part += col[k], k = 1 .. 15                                 15 additions    ("for (int k = 1; k < 16; ++k) part += col[k]")
#   two lane-swap steps (permlane32_swap, permlane16_swap)                     2 additions     ("s2 = sa.x + sa.y", "tot = sb.x + sb.y")
#   the uniform-origin completion of M at the flush                            1 addition      ("a1.x += a0.x * dl.x")
# = 19, and the total goes to the entry's slot 2 q + half.  gut_grad_gather_kernel (csrc/gut_kernels.hip) then sums the particle's
# written slots: the quad path (count <= 32 tiles) adds up to 2 * count rows one after the other into one accumulator
# (QuadAcc::add_rows4 "a.x += v0.x; if (b1 >= 0) a.x += v1.x ..."), the wave-wide path at most 4 rows per 64 slots and quad plus 4
# butterfly steps (xor_sum_quads), which is shorter.  Longest path: 19 + 2 * tiles_count.  The feature rows of the NHT sweep leave
# the same reduction (18 deep) as one atomic per (half tile, entry): at most 2 * tiles_count further additions, the same bound.
#
# K > 0 (csrc/gut_render_k.hip): every popped hit's 14 terms are summed over the lanes that popped the same particle in that step
# (k_bwd_flush_lds "v += s_terms[...]": up to 63 additions in sequence; k_bwd_flush: the DPP reduce-scatter, 6) and added to the
# particle's row with a float atomic (atomicAdd), one per (strip of 64 pixels, step, particle).  The atomics of a row form one chain
# in an order that is not fixed, so the only bound read from the code is one addition per hit: however the hits are grouped into
# waves and steps, a sum of n terms takes n - 1 additions.  n is the number of hits the oracle differentiates for the particle on the
# same lists (`hits` of the budget mode); the GPU's hits differ from those only in masked pixels, whose upstream gradient is zero on
# both sides, so their terms are exact zeros.  (The bound without that count is every pixel of every tile, 256 * tiles_count: on the
# K = 4 scene 5 to 50 times as much.)
REDUCTION_DEPTH = 19


def a_row(family, tiles_count, hits):
    if family == "kbuf":
        return np.asarray(hits, np.float64)
    return REDUCTION_DEPTH + 2.0 * np.asarray(tiles_count, np.float64)


def row_bound(family, b1, bT, tiles_count, hits, c=None):
    """The bound on every element of each row, [N]."""
    c = C[family] if c is None else c
    return (MARGIN * c) * EPS * bT + a_row(family, tiles_count, hits) * EPS * b1


def ratio_to_bound(got, ref, bound):
    """max over the row of |got - ref| / bound, [N]; 0 where both vanish, inf where only the bound does."""
    d = np.abs(np.asarray(got, np.float64) - ref).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = d / bound
    r[(bound == 0) & (d == 0)] = 0.0
    r[(bound == 0) & (d != 0)] = np.inf
    return r


def tensor_rel_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (np.abs(ref).max() + 1e-12))


# ----------------------------------------------------------------------------------------------------------------------------
# the CPU measurement: f32 against f64 oracle on identical lists
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_pair(name):
    """Both oracles of configuration `name` on the f32 run's projection and lists, the upstream gradient zeroed where their hit counts
    differ.  Computed once, shared by the tests, never modified."""
    conf = CONFIG_BY_NAME[name]
    scene = scene_of(conf.scene)
    f32 = oracle_forward(conf, scene, np.float32)
    proj = dict(tiles_count=f32["tiles_count"]) if conf.nht else f32["proj"]
    f64 = oracle_forward(conf, scene, np.float64, proj=proj, lists=lists_of(conf, f32))
    differ = hit_count_of(f32) != hit_count_of(f64)
    g_fd, g_dist = upstream(conf, scene)
    g_fd[differ] = 0.0
    g_dist[differ] = 0.0
    g32 = oracle_backward(conf, scene, f32, g_fd, g_dist, np.float32)
    g64 = oracle_backward(conf, scene, f64, g_fd, g_dist, np.float64)
    return dict(conf=conf, scene=scene, f32=f32, f64=f64, g32=g32, g64=g64, flips=int(differ.sum()), pixels=int(differ.size), g_fd=g_fd, g_dist=g_dist,
                tiles_count=tiles_count_of(conf, f32))


def row_errors(pair):
    """{tensor: r per row with a nonzero budget} with r = max over the row of |g32 - g64| / (eps * B_T of the f64 run)."""
    (g32, _, _, _), (g64, _, bT, _) = pair["g32"], pair["g64"]
    out = {}
    for k in g64:
        live = bT[k] > 0           # (rows without budget are exactly zero on both sides: asserted by the CPU test)
        out[k] = np.abs(g32[k] - g64[k]).max(1)[live] / (EPS * bT[k][live])
    return out


def trace_input(scene, lists, dtype=np.float32):
    """What oracle.gut_pixel_trace reads of a forward: poses, rays, particles and the tile lists."""
    w, h = scene["W"], scene["H"]
    ro, rd = (np.ascontiguousarray(np.asarray(r, dtype).reshape(h, w, 3)) for r in scene["rays"])
    return dict(poses=(np.ascontiguousarray(scene["pose_start"], dtype), np.ascontiguousarray(scene["pose_end"], dtype)), rays=(ro, rd),
                density12=np.ascontiguousarray(scene["density12"], dtype),
                bins=dict(sorted_idx=np.ascontiguousarray(lists[0], np.uint32), tile_ranges=np.ascontiguousarray(lists[1], np.uint32)))


def borderline_entries(conf, scene, lists, particle, masked, dtype=np.float32):
    """The borderline exemption: the accept decisions of `particle` that rounding decides - its entries within BORDERLINE (relative) of
    their threshold, the margin and the condition of parity_util.identify_flips - in pixels that are not masked.  Such a decision can
    fall the other way without changing the pixel's hit count or moving the image by 1e-4.  Returns [(pixel, margin)].

    The SH trace serves the feature (NHT) path as well: the accept test (response and alpha against their thresholds, hit distance in
    the ray's interval) depends on ray and particle alone, and orc_gut_pixel_trace_nht reports the same margins and alphas
    (test_row_gradients_cpu.test_borderline_lookup_finds_the_decisions_rounding_decides compares them)."""
    cfg = oracle_config(conf)
    sidx, rng = np.asarray(lists[0]), np.asarray(lists[1]).astype(np.int64)
    w, h = scene["W"], scene["H"]
    gx = (w + 15) // 16
    fwd = trace_input(scene, lists, dtype)
    found = []
    masked = np.asarray(masked).reshape(h, w)
    for pos in np.flatnonzero(sidx == particle):
        tile = int(np.flatnonzero((rng[:, 0] <= pos) & (pos < rng[:, 1]))[0])
        ty, tx = divmod(tile, gx)
        for y in range(16 * ty, min(16 * ty + 16, h)):
            for x in range(16 * tx, min(16 * tx + 16, w)):
                if masked[y, x]:
                    continue
                tr = oracle.gut_pixel_trace(cfg, scene["cam"], fwd, y * w + x, dtype=dtype)
                mine = (tr["idx"] == particle) & (np.abs(tr["margin"]) < BORDERLINE) & (tr["alpha"] > 0)
                found += [(y * w + x, float(m)) for m in tr["margin"][mine]]
    return found


def remove_entry(sorted_idx, tile_ranges, tile, k):
    """The lists with entry k of `tile` taken out."""
    pos = int(tile_ranges[tile, 0]) + k
    idx = np.delete(sorted_idx, pos)
    rng = tile_ranges.astype(np.int64).copy()
    rng[tile, 1] -= 1
    later = rng[:, 0] > pos
    rng[later] -= 1
    return np.ascontiguousarray(idx, np.uint32), np.ascontiguousarray(rng, np.uint32)


def seeded_faults(family, n_wanted=30, max_draws=600, seed=1):
    """The self-test: the f64 backward loses one tile entry while the forward's results are kept - what a missed slot or a skipped
    replay entry does to a kernel.  Removals are drawn until n_wanted of them changed the victim's row.  Returns
    (counted removals, flagged by the row check at the GPU bound, flagged by the tensor metric at 1e-3)."""
    pair = oracle_pair(SELF_TEST[family])
    conf, scene, f64 = pair["conf"], pair["scene"], pair["f64"]
    g64, b1, bT, hits = pair["g64"]
    sidx, rng = lists_of(conf, f64)
    bounds = {k: row_bound(family, b1[k], bT[k], pair["tiles_count"], hits) for k in g64}
    filled = np.flatnonzero(rng[:, 1] > rng[:, 0])
    rs = np.random.default_rng(seed)
    counted = by_row = by_tensor = 0
    for _ in range(max_draws):
        if counted >= n_wanted:
            break
        t = int(rs.choice(filled))
        k = int(rs.integers(0, int(rng[t, 1]) - int(rng[t, 0])))
        victim = int(sidx[int(rng[t, 0]) + k])
        lists = remove_entry(sidx, rng, t, k)
        if conf.nht:
            faulty = dict(f64, sorted_idx=lists[0], tile_ranges=lists[1])
        else:
            faulty = dict(f64, bins=dict(f64["bins"], sorted_idx=lists[0], tile_ranges=lists[1], num_intersections=len(lists[0])))
        got, _, _, _ = oracle_backward(conf, scene, faulty, pair["g_fd"], pair["g_dist"], np.float64)
        # (beyond the order of the oracle's double sums, which differs from run to run in the last bits)
        if not any(np.any(np.abs(got[name][victim] - g64[name][victim]) > 1e-12 * b1[name][victim]) for name in g64):
            continue                      # the entry lay behind its rays' ends or was never accepted: nothing was lost
        counted += 1
        by_row += int(any(ratio_to_bound(got[name], g64[name], bounds[name]).max() > 1.0 for name in g64))
        by_tensor += int(any(tensor_rel_err(got[name], g64[name]) > TENSOR_BAR for name in g64))
    return counted, by_row, by_tensor


def measure(log=print):
    """Measures C per family over CONFIGS and runs the self-test with the measured constants; returns the report's lines."""
    lines = ["Per-row gradient budgets of the 3DGUT backward: constants of tests/row_budget.py",
             "r = max over the row of |g32 - g64| / (eps * B_T), eps = 2^-24: f32 oracle against f64 oracle on identical lists,",
             "upstream gradient zeroed where their hit counts differ.  C of a family = largest r over its configurations.", ""]
    worst = {f: 0.0 for f in C}
    for conf in CONFIGS:
        pair = oracle_pair(conf.name)
        lines.append(f"{conf.name} [{conf.family}]: {len(pair['scene']['density12'])} particles, {pair['scene']['W']}x{pair['scene']['H']}, "
                     f"hit counts differ on {pair['flips']} pixels")
        for k, r in row_errors(pair).items():
            q = np.quantile(r, [0.5, 0.99, 0.999]) if r.size else np.zeros(3)
            lines.append(f"    {k:9s} rows {r.size:6d}  median {q[0]:8.3f}  99 % {q[1]:8.2f}  99.9 % {q[2]:8.2f}  max {r.max() if r.size else 0.0:8.2f}")
            worst[conf.family] = max(worst[conf.family], float(r.max()) if r.size else 0.0)
        log(lines[-1])
    lines.append("")
    for f, v in worst.items():
        lines.append(f"C[{f}] measured {v:.2f}")
    return lines, worst


if __name__ == "__main__":
    lines, worst = measure()
    lines += ["", f"Self-test: one tile entry removed from the f64 backward's lists, forward results kept; removals that changed the victim's row,",
              f"flagged by the row check at the GPU bound ({MARGIN:g} C eps B_T + A_row eps B_1, recorded C) | by the tensor metric at {TENSOR_BAR:g}:"]
    for f in C:
        n, by_row, by_tensor = seeded_faults(f)
        lines.append(f"    {f:9s} removals {n:3d}  row check {by_row:3d}  tensor metric {by_tensor:3d}")
    text = "\n".join(lines) + "\n"
    print(text)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "row_budget_constants.txt")
    keep = ""
    if os.path.exists(path):
        old = open(path).read()
        mark = old.find("GPU (MI355X)")
        keep = old[mark:] if mark >= 0 else ""
    open(path, "w").write(text + ("\n" + keep if keep else ""))
