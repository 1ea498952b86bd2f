#!/usr/bin/env python
"""The default strategy's trainer-side work at 1 M Gaussians, SH degree 3, Adam state present: plain torch (a restatement of the
reference's GSStrategy by boolean indexing, repeat and cat, with the gradient statistic by four boolean-index operations) against the
fused path (3dgrut_amd.densify.FusedGSStrategyMixin over the same base).

The restatement is the tests' own (tests/densify_reference.py, imported from the tests/ directory of this checkout): the script needs
the whole repository tree, not only scripts/ and the package.

  update_gradient_buffer   ms per call (70 % of the rows have a gradient), back to back on an otherwise idle stream
  densify event            clone + split + opacity prune: wall-clock ms (the host waits inside are part of it) and
                           torch.cuda.max_memory_allocated() over the event, minus what was allocated when it began

    python scripts/bench_densify.py [--n 1000000] [--iters 50] [--events 7] [--out FILE]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
densify = importlib.import_module("3dgrut_amd.densify")
import densify_reference as restated  # noqa: E402


class TorchStrategy(restated.RestatedGSStrategy):
    @torch.no_grad()
    def update_gradient_buffer(self, sensor_position):   # four boolean-index operations, as the reference's method has
        restated.accumulate_indexed_(self.densify_grad_norm_accum, self.densify_grad_norm_denom, self.model.positions.grad,
                                     self.model.positions.data, sensor_position)


class FusedStrategy(densify.FusedGSStrategyMixin, TorchStrategy):
    pass


def make_model(n, base):
    m = restated.DuckModel(1, "cuda")
    groups = []
    for name, _ in restated.DuckModel.NAMES:
        p = torch.nn.Parameter(base[name].clone())
        setattr(m, name, p)
        groups.append({"params": [p], "name": name, "lr": 1e-3})
    m.optimizer = torch.optim.Adam(groups, lr=1e-3, eps=1e-15)
    for name, _ in restated.DuckModel.NAMES:
        p = getattr(m, name)
        m.optimizer.state[p] = {"step": torch.tensor(7.0), "exp_avg": base[name + ".m"].clone(), "exp_avg_sq": base[name + ".v"].clone()}
    return m


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
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--events", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.n
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g)   # noqa: E731
    base = {"positions": rnd(n, 3), "rotation": rnd(n, 4), "scale": rnd(n, 3) * 0.8 - 4.6,      # exp: log-normal around 0.01
            "density": rnd(n, 1) * 2.5 - 1.0, "features_albedo": rnd(n, 3), "features_specular": rnd(n, restated.SH_ROW) * 0.1}
    for name, _ in restated.DuckModel.NAMES:
        base[name + ".m"], base[name + ".v"] = rnd(*base[name].shape) * 1e-3, rnd(*base[name].shape).abs() * 1e-6
    grad = rnd(n, 3) * 1e-4
    grad[torch.rand(n, device="cuda", generator=g) < 0.3] = 0
    accum = torch.rand((n, 1), device="cuda", generator=g) * 2.3e-4          # ~ 13 % of the rows above the 2e-4 thresholds
    pose = torch.eye(4, device="cuda").unsqueeze(0)
    pose[0, :3, 3] = torch.tensor([0.5, -1.0, 3.0])
    conf = restated.make_conf(split_n=2)
    res = {"device": torch.cuda.get_device_name(0), "n": n, "iters": args.iters, "events": args.events}
    for label, cls in (("torch", TorchStrategy), ("fused", FusedStrategy)):
        model = make_model(n, base)
        strategy = cls(conf, model)
        model.positions.grad = grad
        sensor = pose[0, :3, 3]
        t_stat = timed(lambda: strategy.update_gradient_buffer(sensor_position=sensor), args.iters)
        del model, strategy
        walls, peaks, sizes = [], [], None
        for it in range(args.events + 2):                                     # two warm-up events (allocator pool, first launches)
            model = make_model(n, base)
            strategy = cls(conf, model)
            strategy.densify_grad_norm_accum = accum.clone()
            strategy.densify_grad_norm_denom = torch.ones((n, 1), dtype=torch.int32, device="cuda")
            torch.manual_seed(1)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            strategy.densify_gaussians(scene_extent=1.0)
            after_densify = model.num_gaussians
            strategy.prune_gaussians_opacity()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            if it >= 2:
                walls.append(wall)
                peaks.append((torch.cuda.max_memory_allocated() - before) / 2 ** 20)
            sizes = (after_densify, model.num_gaussians)
            del model, strategy
            torch.cuda.empty_cache()
        res[label] = {"update_gradient_buffer_ms": round(t_stat, 4), "event_ms_median": round(statistics.median(walls), 3),
                      "event_ms_min": round(min(walls), 3), "event_ms_max": round(max(walls), 3),
                      "event_peak_extra_MiB": round(max(peaks), 1), "gaussians_after_densify": sizes[0], "gaussians_after_prune": sizes[1]}
    res["model_and_state_MiB"] = round(sum(v.numel() * 4 for v in base.values()) / 2 ** 20, 1)
    res["speedup_update_gradient_buffer"] = round(res["torch"]["update_gradient_buffer_ms"] / res["fused"]["update_gradient_buffer_ms"], 2)
    res["speedup_event"] = round(res["torch"]["event_ms_median"] / res["fused"]["event_ms_median"], 2)
    line = json.dumps({"densify": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
