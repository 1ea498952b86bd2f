"""torch's fused Adam (no amsgrad, no maximize, no grad scaler, coupled weight decay) restated in NumPy for fp32 tensors: float64
statements with an explicit fp32 narrowing wherever the kernel's contract narrows (include/grut_amd.h: grut_adam_update), plus a
float64 k-step version that never narrows, the yardstick of the k-step comparison.  Nothing here contracts a multiply-add."""
import numpy as np

f32, f64 = np.float32, np.float64


def bias_corrections(step, beta1, beta2):
    """(bc1, bc2s) as fp32 from the fp32 step count AFTER its increment: pow and sqrt in double, then narrowed."""
    s = f64(f32(step))
    return f32(f64(1.0) - np.power(f64(beta1), s)), f32(np.sqrt(f64(1.0) - np.power(f64(beta2), s)))


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """One step from fp32 arrays (any shape) and the fp32 step count before the call -> (param, exp_avg, exp_avg_sq, step), fp32."""
    p, g, m, v = (np.asarray(a, dtype=f32) for a in (param, grad, exp_avg, exp_avg_sq))
    lr, beta1, beta2, eps, weight_decay = (f64(x) for x in (lr, beta1, beta2, eps, weight_decay))
    step = f32(f32(step) + f32(1.0))
    bc1, bc2s = bias_corrections(step, beta1, beta2)
    if weight_decay != 0:
        g = (g.astype(f64) + p.astype(f64) * weight_decay).astype(f32)
    g64 = g.astype(f64)
    m = (beta1 * m.astype(f64) + (f64(1.0) - beta1) * g64).astype(f32)
    v = (beta2 * v.astype(f64) + (f64(1.0) - beta2) * g64 * g64).astype(f32)
    step_size = f32(lr / f64(bc1))
    denom = ((np.sqrt(v) / bc2s).astype(f64) + eps).astype(f32)   # fp32 sqrt and division (NumPy rounds both correctly), double addition
    assert np.sqrt(v).dtype == f32 and (np.sqrt(v) / bc2s).dtype == f32
    p = (p - (step_size * m) / denom).astype(f32)
    assert (step_size * m).dtype == f32
    return p, m, v, step


def adam_steps(param, grads, exp_avg, exp_avg_sq, step, lr, **hyper):
    """k fp32 steps, one per entry of `grads`."""
    p, m, v = param, exp_avg, exp_avg_sq
    for g in grads:
        p, m, v, step = adam_step(p, g, m, v, step, lr, **hyper)
    return p, m, v, step


def adam_steps_f64(param, grads, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """The same k steps with every statement and every carried value in float64 (inputs are the fp32 values, widened)."""
    p, m, v = (np.asarray(a, dtype=f32).astype(f64) for a in (param, exp_avg, exp_avg_sq))
    step = f64(step)
    for g in grads:
        g = np.asarray(g, dtype=f32).astype(f64)
        step = step + 1.0
        bc1 = 1.0 - np.power(f64(beta1), step)
        bc2s = np.sqrt(1.0 - np.power(f64(beta2), step))
        if weight_decay != 0:
            g = g + p * f64(weight_decay)
        m = f64(beta1) * m + (1.0 - f64(beta1)) * g
        v = f64(beta2) * v + (1.0 - f64(beta2)) * g * g
        p = p - (f64(lr) / bc1) * m / (np.sqrt(v) / bc2s + f64(eps))
    return p, m, v, step
