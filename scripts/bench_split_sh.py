#!/usr/bin/env python
"""What render.split_sh_features is for: a 3DGUT training step through a model that keeps the SH coefficients as the reference does - two
leaf tensors, features_albedo [N,3] and features_specular [N,45], joined by torch.cat in get_features() (threedgrut/model/model.py:94-96,
204-210) - with the switch off (the cat forward, CatBackward's two slices and AccumulateGrad's two clones around the library) and on (the
library reads the two tensors and writes their two gradients in place).

  workload   1 M Gaussians of workloads.synthetic at 1920x1080 (bench.py's c4_1m_1080p cloud and view)
  one step   clear the gradients, render(train=True), torch.autograd.backward with fixed upstream gradients
  timing     a host clock around a device synchronise; both modes in this process, in alternating blocks of --steps steps after a
             warm-up of both; per mode the median block and the spread (max - min) of its blocks
  stages     the library's forward_project / backward finalisation stage times (gut_profile_read) of both modes, from separate blocks
             after the timed ones (the stage events cost idle stream: they are off while the steps are timed)
  accepted   the split step is not slower than the cat step by more than the measured spread

Without a ROCm GPU nothing is measured and every number reads "not measured".

    python scripts/bench_split_sh.py [--steps 600] [--blocks 4] [--out profiles/split_sh_bench.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
abi = importlib.import_module("3dgrut_amd._abi")
gt = importlib.import_module("3dgrut_amd.gut_tracer")
syn = importlib.import_module("workloads.synthetic")
scenes = importlib.import_module("workloads.scenes")

N, W, H, MEDIAN_SCALE = 1_000_000, 1920, 1080, 0.01


class SplitFeatureGaussians(syn.SimpleGaussians):
    """SimpleGaussians with the SH coefficients kept as the reference model keeps them."""

    def __init__(self, density12, sph, device="cuda"):
        super().__init__(density12, sph, device=device)
        f = self._features.detach()
        del self._features
        self.features_albedo = f[:, :3].clone().requires_grad_(True)
        self.features_specular = f[:, 3:].clone().requires_grad_(True)

    def get_features(self):
        return torch.cat([self.features_albedo, self.features_specular], dim=1)

    def parameters(self):
        return [self.positions, self._rotation, self._scale, self._density, self.features_albedo, self.features_specular]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600, help="steps per block (a block should last well over a second)")
    ap.add_argument("--blocks", type=int, default=4, help="timed blocks per mode")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_sh_bench.json"))
    args = ap.parse_args()
    result = {"workload": f"{N} Gaussians, {W}x{H}, SH degree 3, forward + backward through a model with two SH leaves",
              "steps_per_block": args.steps, "blocks_per_mode": args.blocks}
    if not torch.cuda.is_available():
        result.update(cat_step_ms="not measured", split_step_ms="not measured", gain_ms="not measured", accepted="not measured")
        json.dump(result, open(args.out, "w"), indent=1)
        print(json.dumps(result))
        return
    dev = "cuda"
    d12, sph = syn.cloud_trained_like(N, seed=42, median_scale=MEDIAN_SCALE)
    K = syn.pinhole_intrinsics(W, H)
    ro, rd = syn.pinhole_rays(W, H, K)
    batch = scenes.torch_batch(dict(rays_ori=ro, rays_dir=rd, T_to_world=syn.orbit_pose(0, n_views=8)[None], intrinsics=K), dev)
    g_fd = torch.as_tensor(syn.upstream_grads(W, H)[0], device=dev)
    g_rgb, g_opa = g_fd[None, ..., :3].contiguous(), g_fd[None, ..., 3:].contiguous()
    model = SplitFeatureGaussians(d12, sph, device=dev)
    tracers = {"cat": gt.Tracer({"render": {"splat": {}, "split_sh_features": False}}),
               "split": gt.Tracer({"render": {"splat": {}, "split_sh_features": True}})}

    def step(mode):
        model.zero_grad()
        out = tracers[mode].render(model, batch, train=True)
        torch.autograd.backward([out["pred_features"], out["pred_opacity"]], [g_rgb, g_opa])

    def block(mode, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(mode)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    grads = {}
    for mode in ("cat", "split"):   # warm-up of both (allocations, speculation capacity), and the two paths' gradients for the record
        block(mode, 30)
        grads[mode] = [p.grad.clone() for p in model.parameters()]
    result["gradients_bit_identical"] = all(torch.equal(a, b) for a, b in zip(grads["cat"], grads["split"]))
    result["paths"] = {m: dict(t.stats_split) for m, t in tracers.items()}
    times = {"cat": [], "split": []}
    for _ in range(args.blocks):
        for mode in ("cat", "split"):
            times[mode].append(block(mode, args.steps))
    stages = {}
    for mode in ("cat", "split"):
        nat = tracers[mode].tracer_wrapper
        abi.check(nat.lib.gut_profile_enable(nat.handle, 1), "gut_profile_enable")
        block(mode, 5)
        buf = (C.c_float * len(abi.GUT_STAGES))()
        abi.check(nat.lib.gut_profile_read(nat.handle, buf), "gut_profile_read")   # drop the first frames' times
        block(mode, 100)
        abi.check(nat.lib.gut_profile_read(nat.handle, buf), "gut_profile_read")
        abi.check(nat.lib.gut_profile_enable(nat.handle, 0), "gut_profile_enable")
        stages[mode] = {"forward_project_ms": round(float(buf[abi.GUT_STAGES.index("project")]), 4),
                        "backward_finalisation_ms": round(float(buf[abi.GUT_STAGES.index("project_bwd")]), 4)}
    cat_ms, split_ms = statistics.median(times["cat"]), statistics.median(times["split"])
    spread = {m: max(v) - min(v) for m, v in times.items()}
    result.update(
        cat_step_ms=round(cat_ms, 4), split_step_ms=round(split_ms, 4), gain_ms=round(cat_ms - split_ms, 4),
        gain_percent=round(100.0 * (cat_ms - split_ms) / cat_ms, 2),
        block_spread_ms={m: round(v, 4) for m, v in spread.items()}, block_step_ms={m: [round(x, 4) for x in v] for m, v in times.items()},
        stage_ms=stages, accepted=bool(split_ms - cat_ms <= max(spread.values())))
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
