"""Float64 numpy restatement of the denoiser's model (include/grut_amd.h: grut_denoise), evaluated directly on the fp32
inputs.  No shortcuts: every clamp is explicit, every candidate offset and every patch offset is a loop of its own; only the pixels of
the frame are taken together as arrays (and a clamped gather that several pairs of offsets share is made once).

    d2(p,q) = sum over o in [-f,f]^2, c of (I[clamp(p+o)]_c - I[clamp(q+o)]_c)^2
    x(p,q)  = min(d2 / (n h^2), X_MAX),  n = 3 (2f+1)^2,  X_MAX = 80
    w(p,q)  = exp(-x);   w(p,p) = max_q w(p,q), or 1 when there is no q
    out[p]  = (sum_q w(p,q) I[q] + w(p,p) I[p]) / (sum_q w(p,q) + w(p,p))         q != p, |q - p|_inf <= r, q inside the image

and the error bound every comparison with it uses, with u = 2^-24:

    eps = X_MAX (n + 4) u + 24 u          |a - b| <= 2 eps S + ((2r+1)^2 + 4) u M

S the channel's max minus min over the image, M its largest magnitude.  Each squared difference carries 3 u, any order of summing n
non-negative terms adds at most (n - 1) u, the scaling 2 u: a relative error of d2 / (n h^2) that, times x <= X_MAX, is an absolute error
of the exponent; the device's expf is allowed 24 u; a ratio of sums whose weights are off by eps relatively moves by at most 2 eps times
the spread of the values; the last term is the accumulation itself.
"""
import functools

import numpy as np

X_MAX = 80.0
U = 2.0 ** -24


def denoise_reference(image, f=3, r=7, h=0.1):
    """image [B, H, W, 3] (any real dtype, read as float64) -> float64 [B, H, W, 3]."""
    I = np.asarray(image, dtype=np.float64)
    B, H, W, C = I.shape
    assert C == 3 and H >= 1 and W >= 1
    n = 3 * (2 * f + 1) ** 2
    ys, xs = np.arange(H), np.arange(W)
    clamp_y = lambda y: np.minimum(np.maximum(y, 0), H - 1)   # noqa: E731
    clamp_x = lambda x: np.minimum(np.maximum(x, 0), W - 1)   # noqa: E731

    gathered = {}

    def shifted(sy, sx):
        """I[clamp(y + sy), clamp(x + sx)] for every pixel (y, x) of every image: [B, H, W, 3].  Kept while the candidate rows that
        read it are being evaluated, since p + d + o takes the same value for many pairs (d, o): the same gather, not another formula."""
        if (sy, sx) not in gathered:
            gathered[(sy, sx)] = I[:, clamp_y(ys + sy)[:, None], clamp_x(xs + sx)[None, :], :]
        return gathered[(sy, sx)]

    offsets = [(oy, ox) for oy in range(-f, f + 1) for ox in range(-f, f + 1)]
    mine = [shifted(oy, ox).copy() for oy, ox in offsets]                              # I[clamp(p + o)]
    num = np.zeros_like(I)
    den = np.zeros((B, H, W))
    w_max = np.zeros((B, H, W))
    any_q = np.zeros((H, W), dtype=bool)
    for dy in range(-r, r + 1):
        for key in [k for k in gathered if k[0] < dy - f]:
            del gathered[key]
        for dx in range(-r, r + 1):
            if dy == 0 and dx == 0:
                continue
            inside = ((ys + dy >= 0) & (ys + dy < H))[:, None] & ((xs + dx >= 0) & (xs + dx < W))[None, :]   # q = p + d is a pixel
            if not inside.any():
                continue
            d2 = np.zeros((B, H, W))
            for k, (oy, ox) in enumerate(offsets):
                diff = mine[k] - shifted(dy + oy, dx + ox)                           # I[clamp(p + o)] - I[clamp(q + o)]
                d2 += np.einsum("bhwc,bhwc->bhw", diff, diff)
            w = np.exp(-np.minimum(d2 / (n * h * h), X_MAX))
            w = np.where(inside[None], w, 0.0)
            q = shifted(dy, dx)                                                      # I[q] where q is inside (weight 0 elsewhere)
            num += w[..., None] * q
            den += w
            w_max = np.where(inside[None], np.maximum(w_max, w), w_max)
            any_q |= inside
    w_max = np.where(any_q[None], w_max, 1.0)
    return (num + w_max[..., None] * I) / (den + w_max)[..., None]


def bound(image, f, r):
    """The bound above per channel: float64 [3], from the image's own spread and magnitude."""
    I = np.asarray(image, dtype=np.float64).reshape(-1, 3)
    n = 3 * (2 * f + 1) ** 2
    eps = X_MAX * (n + 4) * U + 24 * U
    spread, mag = I.max(axis=0) - I.min(axis=0), np.abs(I).max(axis=0)
    return 2 * eps * spread + ((2 * r + 1) ** 2 + 4) * U * mag


def worst_ratio(got, want, image, f, r):
    """max over pixels and channels of |got - want| / bound"""
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / bound(image, f, r)).max())


def window_range(image, r):
    """Per pixel and channel, the min and max of the channel over the pixel's search window (clipped to the image): two float64
    arrays of the image's shape."""
    I = np.asarray(image, dtype=np.float64)
    B, H, W, _ = I.shape
    lo, hi = I.copy(), I.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            shifted = I[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            lo[:, y0:y1, x0:x1] = np.minimum(lo[:, y0:y1, x0:x1], shifted)
            hi[:, y0:y1, x0:x1] = np.maximum(hi[:, y0:y1, x0:x1], shifted)
    return lo, hi


def in_window_range(got, image, f, r):
    """Every output channel lies within the min and max of that channel over the pixel's search window, enlarged by the bound."""
    lo, hi = window_range(image, r)
    b = bound(image, f, r)
    got = np.asarray(got, dtype=np.float64)
    return bool(((got >= lo - b) & (got <= hi + b)).all())


@functools.lru_cache(maxsize=None)
def uniform_case(shape, f, r, h=0.1):
    """Uniform noise in [0, 1] of `shape` (B, H, W) as fp32 and its reference, computed once per case and not modified."""
    rng = np.random.default_rng(1000 * shape[0] + 100 * shape[1] + shape[2])
    image = rng.random(shape + (3,)).astype(np.float32)
    want = denoise_reference(image, f, r, h)
    image.setflags(write=False)
    want.setflags(write=False)
    return image, want


@functools.lru_cache(maxsize=None)
def fixture_q():
    """Fixture Q: 40 x 56; the left half (0.8, 0.3, 0.2), the right half (0.1, 0.5, 0.7); linspace(0, 0.2, W) added to all channels of
    the lower half; clipped to [0, 1]; normal noise of sigma 0.1 from default_rng(7) added, the sum cast to fp32.
    -> (clean float64 [1,40,56,3], noisy fp32 [1,40,56,3])"""
    H, W = 40, 56
    clean = np.zeros((H, W, 3))
    clean[:, :W // 2] = (0.8, 0.3, 0.2)
    clean[:, W // 2:] = (0.1, 0.5, 0.7)
    clean[H // 2:] += np.linspace(0.0, 0.2, W)[None, :, None]
    clean = np.clip(clean, 0.0, 1.0)
    noisy = (clean + np.random.default_rng(7).normal(0.0, 0.1, clean.shape)).astype(np.float32)
    clean, noisy = clean[None], noisy[None]
    clean.setflags(write=False)
    noisy.setflags(write=False)
    return clean, noisy


@functools.lru_cache(maxsize=None)
def fixture_q_reference(f=3, r=7, h=0.1, roll=0):
    """The reference on Fixture Q (rolled by `roll` columns), computed once per setting."""
    _, noisy = fixture_q()
    want = denoise_reference(np.roll(noisy, roll, axis=2) if roll else noisy, f, r, h)
    want.setflags(write=False)
    return want
