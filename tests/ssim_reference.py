"""The yardstick of the fused SSIM tests: the published formula (Wang et al. 2004, as used by the original Gaussian-splatting `ssim()`),
restated in torch so that it can be evaluated in float64 on the CPU, and a rounding-error bound for an fp32 evaluation of it.

    map = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),  mu = G*x,  s1 = G*(xx) - mu1^2,  s12 = G*(xy) - mu1 mu2
    G = outer product of the 11-tap Gaussian (sigma 1.5, normalised, ROUNDED TO fp32 and widened again: the kernel's taps), zero padding,
    conv2d with groups = C.  "same": mean over every pixel;  "valid": mean over map[:, :, 5:-5, 5:-5].

`ssim_torch` is the formula in any dtype on any device (float64 on the CPU is the reference; float32 on the GPU is "what a user would
write today").  `reference_and_bounds` returns the float64 value and gradient (autograd) together with per-pixel bounds on what an fp32
evaluation may differ by.  The bound is a running first-order error analysis over the float64 intermediates (u = 2^-24):

    * a window sum of 121 = 11 + 11 separable terms: every term passes through at most 1 product + 11 additions per pass, 23 roundings
      over both passes, +1 for forming x*x: |error| <= K u G*|terms| with K = 24 (K = 124 for a direct 121-term 2-D sum);
    * a + b: e_a + e_b + u |a + b|;   a b: |a| e_b + |b| e_a + e_a e_b + u |a b|;   a / b: (e_a + |a / b| e_b) / (|b| - e_b) + u |a / b|;
    * the expressions are the ones csrc/loss.hip evaluates, in its order (a fused multiply-add rounds once where this model rounds
      twice, so contraction only makes the true error smaller);
    * the mean: the per-pixel errors' mean plus 32 u mean|map| for the fixed-order fp32 tile sums (at most 16 sequential + 6 + 3 additions);
    * FACTOR = 2 on top for what is not modelled (second-order terms, the rounding of 1 / count, of C1 and C2).
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
K_SEPARABLE, K_DIRECT = 24, 124
FACTOR = 2.0
C1, C2 = 0.01 ** 2, 0.03 ** 2


def taps_fp32():
    i = np.arange(11, dtype=np.float64)
    g = np.exp(-((i - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    return (g / g.sum()).astype(np.float32)


def _window(channels, dtype, device):
    t = torch.as_tensor(taps_fp32().astype(np.float64))
    w = torch.outer(t, t).to(dtype)     # float64: the exact product of the fp32 taps
    return w.expand(channels, 1, 11, 11).contiguous().to(device)


def _conv(x, w):
    return F.conv2d(x, w, padding=5, groups=x.shape[1])


def ssim_map(x, y):
    w = _window(x.shape[1], x.dtype, x.device)
    mu1, mu2 = _conv(x, w), _conv(y, w)
    s1 = _conv(x * x, w) - mu1 * mu1
    s2 = _conv(y * y, w) - mu2 * mu2
    s12 = _conv(x * y, w) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def ssim_torch(x, y, padding="same"):
    m = ssim_map(x, y)
    if padding == "valid":
        m = m[:, :, 5:-5, 5:-5]
    return m.mean()


# ---- running error analysis: (value, error bound) pairs of float64 tensors -------------------------------------------------------------
def _leaf(v):
    return v, torch.zeros_like(v)


def _add(a, b, sign=1.0):
    r = a[0] + sign * b[0]
    return r, a[1] + b[1] + U * r.abs()


def _sub(a, b):
    return _add(a, b, -1.0)


def _mul(a, b):
    r = a[0] * b[0]
    return r, a[0].abs() * b[1] + b[0].abs() * a[1] + a[1] * b[1] + U * r.abs()


def _div(a, b):
    r = a[0] / b[0]
    room = b[0].abs() - b[1]
    assert bool((room > 0).all()), "a denominator's error bound reaches its value: the first-order analysis does not apply"
    return r, (a[1] + r.abs() * b[1]) / room + U * r.abs()


def _scale(a, c):   # times an exact power of two or sign
    return a[0] * c, a[1] * abs(c)


def _const(like, c):
    return torch.full_like(like, c), torch.zeros_like(like)


def _window_sum(terms, w, k):
    return _conv(terms, w), k * U * _conv(terms.abs(), w)


def _window_sum_of(a, w, k):   # of a quantity that already carries an error
    return _conv(a[0], w), _conv(a[1], w) + k * U * _conv(a[0].abs(), w)


def reference_and_bounds(x, y, padding="same", upstream=1.0, k=K_SEPARABLE):
    """x, y: [B, C, H, W] CPU tensors (any float dtype; widened to float64).  -> dict(value, grad, value_bound, grad_bound):
    the float64 mean SSIM, upstream * d value / d x (autograd), and the bounds (FACTOR included) for an fp32 evaluation with window sums
    of error constant k."""
    x = x.detach().to(torch.float64).contiguous()
    y = y.detach().to(torch.float64).contiguous()
    xr = x.clone().requires_grad_(True)
    value = ssim_torch(xr, y, padding)
    (grad,) = torch.autograd.grad(value * upstream, xr)
    value = value.detach()

    b, c, h, wd = x.shape
    w = _window(c, torch.float64, "cpu")
    mask = torch.zeros_like(x)
    if padding == "valid":
        mask[:, :, 5:-5, 5:-5] = 1.0
    else:
        mask[:] = 1.0
    count = float(mask.sum())

    mu1, mu2 = _window_sum(x, w, k), _window_sum(y, w, k)
    exx, eyy, exy = _window_sum(x * x, w, k), _window_sum(y * y, w, k), _window_sum(x * y, w, k)
    mu1s, mu2s, mu12 = _mul(mu1, mu1), _mul(mu2, mu2), _mul(mu1, mu2)
    s1, s2, s12 = _sub(exx, mu1s), _sub(eyy, mu2s), _sub(exy, mu12)
    a1 = _add(_scale(mu12, 2.0), _const(x, C1))
    a2 = _add(_scale(s12, 2.0), _const(x, C2))
    b1 = _add(_add(mu1s, mu2s), _const(x, C1))
    b2 = _add(_add(s1, s2), _const(x, C2))
    den = _mul(b1, b2)
    smap = _div(_mul(a1, a2), den)
    value_bound = FACTOR * (float((smap[1] * mask).sum()) / count + 32 * U * float((smap[0].abs() * mask).sum()) / count + U * abs(float(value)))

    d_s1 = _scale(_div(smap, b2), -1.0)
    d_s12 = _div(_scale(a1, 2.0), den)
    first = _mul(_div(_scale(a2, 2.0), den), _sub(mu2, _mul(mu1, _div(a1, b1))))
    d_mu1 = _sub(_sub(first, _mul(_scale(mu1, 2.0), d_s1)), _mul(mu2, d_s12))
    masked = [(p[0] * mask, p[1] * mask) for p in (d_mu1, d_s1, d_s12)]
    g0, g1, g2 = (_window_sum_of(p, w, k) for p in masked)
    total = _add(_add(g0, _mul(_scale(_leaf(x), 2.0), g1)), _mul(_leaf(y), g2))
    scale = torch.full_like(x, upstream / count)
    gfull = _mul((scale, 2 * U * scale.abs()), total)
    assert torch.allclose(gfull[0], grad, rtol=1e-9, atol=1e-12 * (1.0 + float(grad.abs().max()))), "the analytic gradient disagrees with autograd"
    return dict(value=float(value), grad=grad, value_bound=value_bound, grad_bound=FACTOR * gfull[1])
