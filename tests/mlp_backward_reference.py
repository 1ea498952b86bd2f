"""The backward of the NHT decoder's network as grut_mlp_backward (include/grut_amd.h) defines it, restated in numpy float64 on top of
tests/mlp_reference.py: the hand-written backward with dZ rounded to bf16 at the contract's points, the plain int64 gradients of the exact
small-integer networks, a generator of GATE-EXACT networks (no ReLU gate can depend on the summation order), and the tolerances measured
on them.  Imports nothing of the product."""
from __future__ import annotations

import numpy as np

import mlp_reference as R

# ---- tolerances: the largest absolute deviation of 3dgrut_amd.tcnn.mlp_backward_torch (fp32, CPU) from backward_bf16 (float64), measured
# by tests/test_mlp_backward_cpu.py (run it with -s to see the figures).  Both round at the same points.  On random networks the figures
# are set, like GRAD_X_TOL of mlp_reference.py, by ONE ReLU whose input is within rounding of zero, so that fp32 and float64 disagree on
# its gate.  On the gate-exact networks no gate can flip; what is left is a dZ that lands on the other side of a bf16 rounding boundary
# (2^-9 relative of one dZ) and the fp32 sums.  The CPU test allows 2x, the GPU tests 4x (the MFMA's summation order, and one more
# flipped bf16 rounding).
BWD_GRAD_X_TOL = 1.8e-1               # d/dx over test_mlp_cpu.GRID and PARITY_CASES, grad_out ~ N(0, 1)           measured 1.786e-01
BWD_GRAD_PARAMS_TOL = 8.8e-1          # d/dparams over the same                                                    measured 8.759e-01
GATE_EXACT_GRAD_X_TOL = 1.3e-4        # d/dx on the gate-exact cases (GATE_EXACT_CASES)                            measured 1.221e-04
GATE_EXACT_GRAD_PARAMS_TOL = 8.5e-4   # d/dparams on the gate-exact cases (4099 pixels summed)                     measured 8.469e-04


def backward_bf16(cache, grad_out, cfg, rounding=True):
    """R.backward with the contract's roundings of dZ: the gradient with respect to every layer's pre-activation, after its gate or the
    output activation's derivative, is rounded once to bf16 before it enters the weight-gradient and the data-gradient product.
    -> (grad_x [P, F+3], grad_params [n_params]).  rounding=False is R.backward."""
    rnd = R.bf16_round if rounding else (lambda a: a)
    act = cfg.output_activation
    g = np.asarray(grad_out, dtype=np.float64)
    if act == "relu":
        g = g * (cache["z"] > 0)
    elif act == "sigmoid":
        g = g * cache["out"] * (1.0 - cache["out"])
    g = rnd(g)
    ws, hs, zs = cache["ws"], cache["hs"], cache["zs"]
    g_out = np.zeros((R.OUT_ROWS, cfg.width))
    g_out[:cfg.n_output_dims] = g.T @ hs[-1]
    grads = [g_out]
    g = g @ ws[-1][:cfg.n_output_dims]
    for i in range(len(zs) - 1, -1, -1):
        g = rnd(g * (zs[i] > 0))
        grads.insert(0, g.T @ hs[i])
        g = g @ ws[i]
    f, n_sh = cfg.n_features, cfg.sh_degree ** 2
    g_d = np.einsum("pi,pic->pc", g[:, f:f + n_sh], R.sh_jacobian(cache["d"])[:, :n_sh])
    return np.concatenate([g[:, :f], 2.0 * g_d], axis=1), np.concatenate([m.reshape(-1) for m in grads])


# ---- exact small-integer networks ------------------------------------------------------------------------------------------------------------
def integer_grad_out(cfg, n_pixels, seed=7, every=1):
    """[P, n_output_dims] fp32 integers in -1 .. 2; with every > 1 only one pixel in `every` is non-zero"""
    rng = np.random.default_rng(seed)
    g = rng.integers(-1, 3, (n_pixels, cfg.n_output_dims)).astype(np.float32)
    if every > 1:
        g[np.arange(n_pixels) % every != 0] = 0.0
    return g


def integer_backward(params, x, grad_out, cfg):
    """The plain int64 gradients of an R.integer_network on an R.integer_input for an integer grad_out (output activation none or relu);
    the products run in float64, where integers of this size are exact, and the results are returned as int64.
    -> (grad_x feature columns [P, F] int64, grad_params [n_params] int64, ranges); the first matrix's SH columns of grad_params are
    returned as zero (their true value is dZ x the SH values, no integer): the tests leave them out.  ranges = (largest |dZ|, largest sum
    over the pixels of |dZ x H| of one weight): the tests hold them under 256 and 2^24, where bf16 and fp32 sums are exact."""
    f, n_sh = cfg.n_features, cfg.sh_degree ** 2
    ws = [np.rint(w) for w in R.split(params, cfg)]
    assert not ws[0][:, f:f + n_sh].any() and cfg.output_activation in ("none", "relu")
    hs = [np.concatenate([np.rint(x[:, :f].astype(np.float64)), np.zeros((x.shape[0], n_sh)), np.ones((x.shape[0], R.k0(cfg) - f - n_sh))], axis=1)]
    zs = []
    for w in ws[:-1]:
        zs.append(hs[-1] @ w.T)
        hs.append(np.maximum(zs[-1], 0))
    z = hs[-1] @ ws[-1][:cfg.n_output_dims].T
    g = np.rint(np.asarray(grad_out, dtype=np.float64))
    if cfg.output_activation == "relu":
        g = g * (z > 0)
    big_dz, big_sum = np.abs(g).max(), 0
    g_out = np.zeros((R.OUT_ROWS, cfg.width))
    g_out[:cfg.n_output_dims] = g.T @ hs[-1]
    big_sum = max(big_sum, (np.abs(g).T @ np.abs(hs[-1])).max())
    grads = [g_out]
    g = g @ ws[-1][:cfg.n_output_dims]
    for i in range(len(zs) - 1, -1, -1):
        g = g * (zs[i] > 0)
        big_dz = max(big_dz, np.abs(g).max())
        grads.insert(0, g.T @ hs[i])
        big_sum = max(big_sum, (np.abs(g).T @ np.abs(hs[i])).max())
        g = g @ ws[i]
    assert big_sum < 2.0 ** 53
    return g[:, :f].astype(np.int64), np.concatenate([m.reshape(-1) for m in grads]).astype(np.int64), (int(big_dz), int(big_sum))


def sh_columns_of_the_first_matrix(cfg):
    """boolean mask [n_params]: the first matrix's SH columns"""
    mask = np.zeros(R.n_params(cfg), dtype=bool)
    first = mask[:cfg.width * R.k0(cfg)].reshape(cfg.width, R.k0(cfg))
    first[:, cfg.n_features:cfg.n_features + cfg.sh_degree ** 2] = True
    return mask


# ---- gate-exact networks ------------------------------------------------------------------------------------------------------------------------
# name -> (config, P, seed): the cases of the GPU test, measured on the CPU on the very same arrays
GATE_EXACT_CASES = {
    "shipped_sigmoid": (R.Config(24, 3, 3, 128, 3, "sigmoid"), 4099, 31),
    "shipped_none": (R.Config(24, 3, 3, 128, 3, "none"), 4099, 32),
    "f55_l4_sigmoid": (R.Config(55, 4, 3, 128, 3, "sigmoid"), 4099, 33),
    "f55_l4_none": (R.Config(55, 4, 3, 128, 3, "none"), 4099, 34),
}
ROUNDING_MARGIN = 64 * 2.0 ** -24   # of max(|z|, 1): how far a first-layer sum stays from a bf16 rounding boundary (fp32 sums of K0 <= 128 terms err less)


def gate_exact_network(cfg, rng):
    """Layers >= 1: sparse +-1 rows with at most two non-zeros.  Layer 0: at most two +-1 on feature columns, 0.5 on a ones-padded column,
    +-2^-7 on every SH column.  With integer features and unit directions a first-layer pre-activation is an integer + 0.5 + an SH part of
    magnitude < 0.25: at least 0.25 from zero.  Later pre-activations are sums of two bf16 numbers: exact in fp32, in any order."""
    f, n_sh, k0 = cfg.n_features, cfg.sh_degree ** 2, R.k0(cfg)
    assert k0 > f + n_sh, "the generator needs a ones-padded column"
    mats = []
    for index, (rows, columns) in enumerate(R.matrices(cfg)):
        m = np.zeros((rows, columns))
        for r in range(rows):
            cols = rng.choice(f if index == 0 else columns, size=2, replace=False)
            for c in cols[:1 + (rng.random() < 0.8)]:
                m[r, c] = -1.0 if rng.random() < 0.3 else 1.0
            if index == 0:
                m[r, f + n_sh + rng.integers(0, k0 - f - n_sh)] = 0.5
                m[r, f:f + n_sh] = np.where(rng.random(n_sh) < 0.5, -1.0, 1.0) * 2.0 ** -7
        if index == cfg.n_hidden_layers:
            m[cfg.n_output_dims:] = 7.0
        mats.append(m)
    return np.concatenate([m.reshape(-1) for m in mats]).astype(np.float32)


def _forward_float32(params, x, cfg):
    """the forward in np.float32 arithmetic with the contract's roundings -> (gates, rounded activations) per layer"""
    f, n_sh = cfg.n_features, cfg.sh_degree ** 2
    x = np.asarray(x, dtype=np.float32)
    d = np.float32(2.0) * x[:, f:f + 3] - np.float32(1.0)
    enc = np.concatenate([x[:, :f], R.sh_values(d)[:, :n_sh].astype(np.float32), np.ones((x.shape[0], R.k0(cfg) - f - n_sh), np.float32)], axis=1)
    h = R.bf16_round(enc).astype(np.float32)
    gates, acts = [], []
    for w in R.split(params, cfg)[:-1]:
        z = h @ R.bf16_round(w).astype(np.float32).T
        assert z.dtype == np.float32
        h = R.bf16_round(np.maximum(z, 0)).astype(np.float32)
        gates.append(z > 0)
        acts.append(h)
    return gates, acts


def gate_exact_case(name):
    """-> (cfg, params fp32, x fp32 [P, F+3], grad_out fp32 [P, n_out]), the same arrays wherever it is called.  Pixels whose first-layer
    sums come within ROUNDING_MARGIN of a bf16 rounding boundary are drawn again, and the function asserts what the name promises:
    every first-layer pre-activation at least 0.25 from zero, every later one a sum of at most two terms, and an np.float32 forward with
    the same gates and the same rounded activations as the float64 one."""
    cfg, n_pixels, seed = GATE_EXACT_CASES[name]
    rng = np.random.default_rng(seed)
    params = gate_exact_network(cfg, rng)
    x = R.integer_input(cfg, 2 * n_pixels, seed=seed + 100)
    dirs = rng.normal(size=(x.shape[0], 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    x[:, cfg.n_features:] = ((dirs + 1.0) * 0.5).astype(np.float32)                 # unit directions, sh_scale 1
    _, cache = R.forward(params, x, cfg)
    z0 = cache["zs"][0]
    a = np.maximum(z0, 0.0)
    up = R.bf16_round(a)                                                            # distance to the nearest rounding boundary, from both sides
    mantissa, exponent = np.frexp(np.maximum(up, 2.0 ** -100))
    ulp = np.ldexp(1.0, exponent - 8)                                               # bf16 has 8 significant bits
    below = np.where(mantissa == 0.5, ulp / 4, ulp / 2)                             # a power of two: the spacing halves below it
    boundary = np.minimum(np.abs(a - (up - below)), np.abs(a - (up + ulp / 2)))
    keep = np.where(((boundary > ROUNDING_MARGIN * np.maximum(np.abs(z0), 1.0)) | (z0 < 0)).all(axis=1))[0][:n_pixels]
    assert len(keep) == n_pixels, (name, len(keep))
    x = np.ascontiguousarray(x[keep])
    _, cache = R.forward(params, x, cfg)
    assert np.abs(cache["zs"][0]).min() >= 0.25
    for w in cache["ws"][1:]:
        assert (np.count_nonzero(w[:cfg.n_output_dims if w.shape[0] == R.OUT_ROWS else None], axis=1) <= 2).all()
    gates, acts = _forward_float32(params, x, cfg)
    for i, (g32, a32) in enumerate(zip(gates, acts)):
        assert np.array_equal(g32, cache["zs"][i] > 0) and np.array_equal(a32.astype(np.float64), cache["hs"][i + 1]), (name, i)
    assert all((z > 0).mean() > 0.2 for z in cache["zs"])                           # not a dead network
    grad_out = rng.normal(size=(n_pixels, cfg.n_output_dims)).astype(np.float32)
    return cfg, params, x, grad_out
