"""The NHT decoder's network (grut_mlp_forward in include/grut_amd.h, 3dgrut_amd/tcnn.py) restated in numpy float64, forward and a
hand-written backward, with the contract's bf16 rounding points done in integer bit arithmetic and treated as straight-through by the
backward.  Also the exact small-integer networks of the bit-equality tests, the random cases that the CPU and the GPU tests share, and
the tolerances measured on them.  Imports nothing of the product."""
from __future__ import annotations

import collections

import numpy as np

Config = collections.namedtuple("Config", "n_features sh_degree n_hidden_layers width n_output_dims output_activation")   # as tcnn.MlpConfig
OUT_ROWS = 16

# ---- tolerances: the largest absolute deviation of 3dgrut_amd.tcnn.mlp_torch (fp32, CPU) from this float64 restatement, measured by
# tests/test_mlp_cpu.py (run it with -s to see the figures).  Both round at the same points; they differ where an fp32 sum lands on the
# other side of a bf16 rounding boundary than the float64 sum, which moves a hidden activation by one bf16 step (2^-8 relative).
# The CPU tests allow 2x the constant (another BLAS sums in another order and flips other roundings), the GPU tests 4x (the MFMA's
# k-step order, and one flipped rounding of a hidden activation more).
VALUE_TOL = 3.7e-4          # values over the grid of test_mlp_cpu.GRID (288 cases of 37 pixels)           measured 3.693e-04
GRAD_X_TOL = 1.8e-1         # d/dx over the same grid, grad_out ~ N(0, 1)                                   measured 1.790e-01
GRAD_PARAMS_TOL = 8.8e-1    # d/dparams over the same grid (37 pixels summed)                               measured 8.769e-01
# The two gradient figures are set by ONE ReLU whose input is within rounding of zero, so that fp32 and float64 disagree on its gate;
# everywhere else the gradients agree to about 2e-6 (median 1e-8).
PARITY_TOL = {              # values of the GPU parity cases (PARITY_CASES), on the very inputs the GPU tests use
    "shipped_scale1": 2.6e-4,       # measured 2.592e-04
    "shipped_scale3": 2.8e-4,       # measured 2.732e-04
    "k0_128_no_padding": 9.2e-4,    # measured 9.175e-04
}

C1, C2, C3, C4, C5 = 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.31539156525251999, 0.54627421529603959
C6, C7, C8, C9, C10 = 0.59004358992664352, 2.8906114426405538, 0.45704579946446572, 0.3731763325901154, 1.4453057213202769


def k0(cfg):
    return (cfg.n_features + cfg.sh_degree ** 2 + 15) // 16 * 16


def matrices(cfg):
    return [(cfg.width, k0(cfg))] + [(cfg.width, cfg.width)] * (cfg.n_hidden_layers - 1) + [(OUT_ROWS, cfg.width)]


def n_params(cfg):
    return sum(r * c for r, c in matrices(cfg))


def bf16_round(a):
    """float64 -> the nearest bf16 (ties to even, through fp32), as float64; by integer arithmetic on the fp32 bits"""
    bits = np.ascontiguousarray(a, dtype=np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


def sh_values(d):
    """[P, 3] -> [P, 16]: the contract's polynomials for d = (x, y, z), not normalised"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    return np.stack([np.full_like(x, 0.28209479177387814), -C1 * y, C1 * z, -C1 * x, C2 * x * y, -C2 * y * z, C3 * zz - C4, -C2 * x * z,
                     C5 * (xx - yy), C6 * y * (-3 * xx + yy), C7 * x * y * z, C8 * y * (1 - 5 * zz), C9 * z * (5 * zz - 3),
                     C8 * x * (1 - 5 * zz), C10 * z * (xx - yy), C6 * x * (-xx + 3 * yy)], axis=1)


def sh_jacobian(d):
    """[P, 3] -> [P, 16, 3]: d sh_i / d (x, y, z)"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    o = np.zeros_like(x)
    one = np.ones_like(x)
    rows = [(o, o, o), (o, -C1 * one, o), (o, o, C1 * one), (-C1 * one, o, o), (C2 * y, C2 * x, o), (o, -C2 * z, -C2 * y), (o, o, 2 * C3 * z),
            (-C2 * z, o, -C2 * x), (2 * C5 * x, -2 * C5 * y, o), (-6 * C6 * x * y, C6 * (-3 * xx + 3 * yy), o), (C7 * y * z, C7 * x * z, C7 * x * y),
            (o, C8 * (1 - 5 * zz), -10 * C8 * y * z), (o, o, C9 * (15 * zz - 3)), (C8 * (1 - 5 * zz), o, -10 * C8 * x * z),
            (2 * C10 * x * z, -2 * C10 * y * z, C10 * (xx - yy)), (C6 * (-3 * xx + 3 * yy), 6 * C6 * x * y, o)]
    return np.stack([np.stack(r, axis=1) for r in rows], axis=1)


def split(params, cfg):
    """the flat parameter vector -> its matrices [out][in]"""
    out, offset = [], 0
    for rows, columns in matrices(cfg):
        out.append(np.asarray(params[offset:offset + rows * columns], dtype=np.float64).reshape(rows, columns))
        offset += rows * columns
    return out


def forward(params, x, cfg, rounding=True):
    """-> (out [P, n_output_dims] float64, cache for backward).  rounding=False: the same network without the bf16 roundings."""
    rnd = bf16_round if rounding else (lambda a: np.asarray(a, dtype=np.float64))
    x = np.asarray(x, dtype=np.float64)
    f, n_sh = cfg.n_features, cfg.sh_degree ** 2
    d = 2.0 * x[:, f:f + 3] - 1.0
    enc = np.concatenate([x[:, :f], sh_values(d)[:, :n_sh], np.ones((x.shape[0], k0(cfg) - f - n_sh))], axis=1)
    ws = [rnd(w) for w in split(params, cfg)]
    hs, zs = [rnd(enc)], []
    for w in ws[:-1]:
        zs.append(hs[-1] @ w.T)
        hs.append(rnd(np.maximum(zs[-1], 0.0)))
    z = hs[-1] @ ws[-1][:cfg.n_output_dims].T
    act = cfg.output_activation
    out = z if act == "none" else np.maximum(z, 0.0) if act == "relu" else 1.0 / (1.0 + np.exp(-z))
    return out, dict(d=d, ws=ws, hs=hs, zs=zs, z=z, out=out)


def backward(cache, grad_out, cfg):
    """-> (grad_x [P, F+3], grad_params [n_params]); the bf16 roundings pass the gradient unchanged, ReLU passes it where its input > 0,
    the output matrix's rows beyond n_output_dims get zero."""
    act = cfg.output_activation
    g = np.asarray(grad_out, dtype=np.float64)
    if act == "relu":
        g = g * (cache["z"] > 0)
    elif act == "sigmoid":
        g = g * cache["out"] * (1.0 - cache["out"])
    ws, hs, zs = cache["ws"], cache["hs"], cache["zs"]
    g_out = np.zeros((OUT_ROWS, cfg.width))
    g_out[:cfg.n_output_dims] = g.T @ hs[-1]
    grads = [g_out]
    g = g @ ws[-1][:cfg.n_output_dims]
    for i in range(len(zs) - 1, -1, -1):
        g = g * (zs[i] > 0)
        grads.insert(0, g.T @ hs[i])
        g = g @ ws[i]
    f, n_sh = cfg.n_features, cfg.sh_degree ** 2
    g_d = np.einsum("pi,pic->pc", g[:, f:f + n_sh], sh_jacobian(cache["d"])[:, :n_sh])
    return np.concatenate([g[:, :f], 2.0 * g_d], axis=1), np.concatenate([m.reshape(-1) for m in grads])


# ---- random cases ----------------------------------------------------------------------------------------------------------------------------
def random_input(rng, n_pixels, n_features, sh_scale):
    """[P, F+3] fp32 rows as the decoder builds them: features, then (unit direction * sh_scale + 1) / 2"""
    feats = rng.normal(0.0, 0.5, (n_pixels, n_features))
    dirs = rng.normal(size=(n_pixels, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return np.concatenate([feats, (dirs * sh_scale + 1.0) * 0.5], axis=1).astype(np.float32)


def xavier_params(rng, cfg):
    return np.concatenate([rng.uniform(-1.0, 1.0, r * c) * np.sqrt(6.0 / (r + c)) for r, c in matrices(cfg)]).astype(np.float32)


# the GPU parity cases (test_mlp_gpu.py), measured on the CPU by test_mlp_cpu.py on the very same inputs: name -> (config, P, sh_scale, seed)
PARITY_CASES = {
    "shipped_scale1": (Config(24, 3, 3, 128, 3, "sigmoid"), 4099, 1.0, 11),
    "shipped_scale3": (Config(24, 3, 3, 128, 3, "sigmoid"), 4099, 3.0, 12),
    "k0_128_no_padding": (Config(112, 4, 3, 128, 3, "sigmoid"), 4099, 3.0, 13),
}
# configurations the kernel does not take: the torch path on the device is held against the restatement under 4 VALUE_TOL, the figure
# for mlp_torch over configurations in general (the deviation on one small case says little: one flipped rounding more or less sets it)
FALLBACK_CASES = {
    "eight_layers": (Config(24, 3, 8, 128, 3, "sigmoid"), 257, 3.0, 14),        # the weight image does not fit into LDS
    "width_32": (Config(24, 3, 3, 32, 3, "sigmoid"), 257, 3.0, 15),
}


def parity_case(name):
    """-> (cfg, params fp32, x fp32), the same arrays wherever it is called"""
    cfg, n_pixels, sh_scale, seed = {**PARITY_CASES, **FALLBACK_CASES}[name]
    rng = np.random.default_rng(seed)
    return cfg, xavier_params(rng, cfg), random_input(rng, n_pixels, cfg.n_features, sh_scale)


# ---- exact small-integer networks ------------------------------------------------------------------------------------------------------------
def integer_network(cfg, seed=5):
    """Sparse +-1 weights, at most two non-zeros per row, every row of a matrix distinct, asymmetric; the first matrix has zeros on the SH
    columns and non-zeros on some of the ones-padded columns; the output matrix's rows beyond n_output_dims hold 7 (they are never read).
    With inputs in -1 .. 2 every intermediate is an integer of magnitude <= 2^(layers + 2): exact in bf16 up to 6 matrices."""
    rng = np.random.default_rng(seed)
    f, n_sh = cfg.n_features, cfg.sh_degree ** 2
    mats = []
    for index, (rows, columns) in enumerate(matrices(cfg)):
        allowed = np.array([c for c in range(columns) if index != 0 or not f <= c < f + n_sh])
        pads = np.array([c for c in range(f + n_sh, columns)]) if index == 0 else np.array([], dtype=int)
        m = np.zeros((rows, columns))
        seen = set()
        for r in range(rows):
            while True:
                row = np.zeros(columns)
                cols = rng.choice(allowed, size=2, replace=False)
                if len(pads) and r % 3 == 0:
                    cols[1] = pads[(r // 3) % len(pads)]                      # a one-padded column: the learnable bias
                for c in cols if cols[0] != cols[1] else cols[:1]:
                    row[c] = -1.0 if rng.random() < 0.25 else 1.0
                if row.tobytes() not in seen:
                    seen.add(row.tobytes())
                    m[r] = row
                    break
        if index == cfg.n_hidden_layers:
            m[cfg.n_output_dims:] = 7.0
        mats.append(m)
    return np.concatenate([m.reshape(-1) for m in mats]).astype(np.float32)


def integer_input(cfg, n_pixels, seed=6):
    """[P, F+3] fp32: integer features in -1 .. 2; the direction columns hold non-integers (their SH values meet zero weights)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-1, 3, (n_pixels, cfg.n_features + 3)).astype(np.float32)
    x[:, cfg.n_features:] = rng.uniform(0.0, 1.0, (n_pixels, 3))
    return x


def integer_forward(params, x, cfg):
    """The plain integer matrix products (int64) of an integer_network on an integer_input -> [P, n_output_dims] fp32; the SH columns are
    skipped (zero weights), the padding is ones.  Output activation none or relu."""
    f, n_sh = cfg.n_features, cfg.sh_degree ** 2
    ws = [np.rint(w).astype(np.int64) for w in split(params, cfg)]
    assert not ws[0][:, f:f + n_sh].any()
    h = np.concatenate([np.rint(x[:, :f]).astype(np.int64), np.zeros((x.shape[0], n_sh), np.int64),
                        np.ones((x.shape[0], k0(cfg) - f - n_sh), np.int64)], axis=1)
    for w in ws[:-1]:
        h = np.maximum(h @ w.T, 0)
        assert np.abs(h).max() <= 256
    z = h @ ws[-1][:cfg.n_output_dims].T
    assert cfg.output_activation in ("none", "relu")
    return (np.maximum(z, 0) if cfg.output_activation == "relu" else z).astype(np.float32)
