#!/usr/bin/env python
"""The MCMC strategy's device work at 1 M and 3 M Gaussians (raw parameters distributed like a trained model's): ms per call and GB/s.

  perturbation  the reference's MCMCStrategy.perturb_gaussians restated with torch ops (threedgrut/strategy/mcmc.py:167-187: covariance
                from get_covariance / quaternion_to_so3, randn_like, sigmoid, bmm, add_) against 3dgrut_amd.mcmc.perturb_gaussians
                (the same randn_like + one fused kernel) and against the kernel alone (perturb_positions_ on a drawn noise buffer).
                Byte model of the kernel: 56 B read (rotation 16, scale 12, density 4, noise 12, positions 12) + 12 B written = 68 B
                per Gaussian.
  relocation    compute_relocation_tensor on 5 % and 50 % of the rows sampled as mcmc.py:189-222 samples them (binom_n_max 51);
                byte model 4 + 12 + 4 read, 4 + 12 written = 36 B per sampled row (the 10 KB table stays in cache).

    python scripts/bench_mcmc.py [--sizes 1000000,3000000] [--iters 50] [--out FILE]
"""
import argparse
import importlib
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mcmc = importlib.import_module("3dgrut_amd.mcmc")

PERTURB_BYTES = 68
RELOCATION_BYTES = 36
HBM_GBS = 8000.0
NOISE_LR, LR, N_MAX = 5e5, 1.6e-4, 51


class Model:
    """Raw parameters with the default activations and an optimizer holding the "positions" group (what perturb_gaussians reads)."""

    def __init__(self, n, seed=0):
        g = torch.Generator(device="cuda").manual_seed(seed)
        P = torch.nn.Parameter
        self.positions = P(torch.randn(n, 3, device="cuda", generator=g))
        self.rotation = P(torch.randn(n, 4, device="cuda", generator=g))
        self.scale = P(torch.randn(n, 3, device="cuda", generator=g) * 0.8 - 4.6)      # exp: log-normal around 0.01
        self.density = P(torch.randn(n, 1, device="cuda", generator=g) * 2.5 - 1.0)    # sigmoid: dead, mid and dense particles
        self.rotation_activation = torch.nn.functional.normalize
        self.scale_activation = torch.exp
        self.density_activation = torch.sigmoid
        self.optimizer = torch.optim.SGD([{"params": [self.positions], "name": "positions", "lr": LR}])

    def get_rotation(self):
        return self.rotation_activation(self.rotation)

    def get_scale(self):
        return self.scale_activation(self.scale)

    def get_density(self):
        return self.density_activation(self.density)


@torch.no_grad()
def torch_perturb(model, noise_lr):
    """mcmc.py:167-187 with model.py:120-130 and utils/misc.py:67-88, op for op in torch (fp32)."""
    scales = model.get_scale()
    n = scales.shape[0]
    S = torch.zeros((n, 3, 3), dtype=scales.dtype, device=scales.device)
    r = model.get_rotation()
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((n, 3, 3), dtype=r.dtype, device=r.device)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    S[:, 0, 0], S[:, 1, 1], S[:, 2, 2] = scales[:, 0], scales[:, 1], scales[:, 2]
    cov = R @ S @ S.transpose(1, 2) @ R.transpose(1, 2)
    positions = model.positions
    dens = model.get_density()
    lr = 0.0
    for group in model.optimizer.param_groups:
        if group["name"] == "positions":
            lr = group["lr"]
    noise = torch.randn_like(positions) * (1 / (1 + torch.exp(-100 * ((1 - dens) - 0.995)))) * noise_lr * lr
    noise = torch.bmm(cov, noise.unsqueeze(-1)).squeeze(-1)
    model.positions.add_(noise)


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,3000000")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    binoms = torch.tensor([[math.comb(n, k) if k <= n else 0 for k in range(N_MAX)] for n in range(N_MAX)], dtype=torch.float32, device="cuda")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "noise_lr": NOISE_LR, "lr": LR}
    for n in [int(s) for s in args.sizes.split(",")]:
        m = Model(n)
        noise = torch.randn(n, 3, device="cuda")
        t_torch = timed(lambda: torch_perturb(m, NOISE_LR), args.iters)
        t_fused = timed(lambda: mcmc.perturb_gaussians(m, NOISE_LR), args.iters)
        t_kernel = timed(lambda: mcmc.perturb_positions_(m.positions.data, m.rotation.data, m.scale.data, m.density.data, noise, NOISE_LR, LR),
                         args.iters)
        t_randn = timed(lambda: torch.randn_like(m.positions), args.iters)
        gbs = PERTURB_BYTES * n / t_kernel / 1e6
        entry = {"perturb": {
            "torch_reference_ms": round(t_torch, 4), "fused_ms": round(t_fused, 4), "speedup": round(t_torch / t_fused, 2),
            "kernel_ms": round(t_kernel, 4), "randn_like_ms": round(t_randn, 4), "kernel_GB/s": round(gbs, 1),
            "kernel_frac_of_8TBs": round(gbs / HBM_GBS, 3), "bytes_per_gaussian": PERTURB_BYTES}}
        dens = m.get_density().detach()
        scales = m.get_scale().detach()
        for frac in (0.05, 0.5):
            k = int(frac * n)
            idx = torch.multinomial(dens.flatten(), k, replacement=True)
            ratios = (torch.bincount(idx)[idx] + 1).clamp_(min=1, max=N_MAX).int()
            o, s = dens[idx].contiguous(), scales[idx].contiguous()
            t = timed(lambda: mcmc.compute_relocation_tensor(o, s, ratios, binoms, N_MAX), args.iters)
            entry[f"relocation_{int(frac * 100)}pct"] = {"rows": k, "max_ratio": int(ratios.max()), "ms": round(t, 4),
                                                        "GB/s": round(RELOCATION_BYTES * k / t / 1e6, 1)}
        res[f"n_{n}"] = entry
        del m, noise
        torch.cuda.empty_cache()
    line = json.dumps({"mcmc": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
