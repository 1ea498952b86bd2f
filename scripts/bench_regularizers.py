"""The opacity and scale regularisers of one MCMC training step, forward plus backward, two ways on one MI355X, in one process, alternating:

    python scripts/bench_regularizers.py [--n 1000000] [--rounds 15] [--window 0.2] [--out profiles/regularizers_bench.json]

  torch    what every step runs without the switch: the two lines of Trainer3DGRUT.get_losses (trainer.py:727, 735) on the model's activated
           parameters, torch.abs(sigmoid(density)).mean() and torch.abs(exp(scale)).mean(), and autograd's mirror image of them
  fused    one regularizers.opacity_scale_means call on the raw parameters (csrc/regularizers.hip: two launches forward, one backward)

Both weight the two means with the lambdas of configs/base_mcmc.yaml (0.01 each), call backward() and ACCUMULATE into a .grad that already
exists, as in a training step, where the renderer's gradient of the same two parameters arrives through the same backward().  The
parameters are those of an SH-degree-3 model of N Gaussians (positions, density, rotation, scale, albedo, specular); only density [N, 1]
and scale [N, 3] take part.  Method of scripts/bench_photo_loss.py: both versions warmed up, device events around as many calls as fill
`--window` seconds (at least 20), the versions alternating inside every round; median and spread (min / max) over the rounds.  These are
whole-call times (autograd, allocations, every launch), which is what a training step pays.  `spread_ms` is the larger of the two versions'
(max - min) over the rounds: a difference of the medians below it is not a difference.  Values and gradients of the two versions are
compared first.  Prints one JSON line and writes it to --out.  Fails without a GPU: there is nothing to fall back to."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAMBDA_OPACITY, LAMBDA_SCALE = 0.01, 0.01   # configs/base_mcmc.yaml


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regularizers_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_regularizers.py needs a GPU (there is no CPU fallback)")
    reg = importlib.import_module("3dgrut_amd.regularizers")
    n = args.n
    g = torch.Generator(device="cuda").manual_seed(1)
    rand = lambda *shape: torch.rand(shape, generator=g, device="cuda")   # noqa: E731
    model = {"positions": rand(n, 3), "density": rand(n, 1) * 8 - 4, "rotation": rand(n, 4), "scale": rand(n, 3) * 4 - 6,
             "features_albedo": rand(n, 3), "features_specular": rand(n, 45)}
    density, scale = model["density"].requires_grad_(True), model["scale"].requires_grad_(True)

    def torch_step():
        loss_opacity = torch.abs(torch.sigmoid(density)).mean()
        loss_scale = torch.abs(torch.exp(scale)).mean()
        (LAMBDA_OPACITY * loss_opacity + LAMBDA_SCALE * loss_scale).backward()

    def fused_step():
        loss_opacity, loss_scale = reg.opacity_scale_means(density, scale)
        (LAMBDA_OPACITY * loss_opacity + LAMBDA_SCALE * loss_scale).backward()

    fns = {"torch": torch_step, "fused": fused_step}
    grads, values = {}, {}
    for k, fn in fns.items():              # faster and different is not faster
        density.grad = scale.grad = None
        fn()
        grads[k] = (density.grad.clone(), scale.grad.clone())
    with torch.no_grad():
        values["torch"] = [float(v) for v in reg.means_torch(density, scale)]
        values["fused"] = [float(v) for v in reg.opacity_scale_means(density, scale)]
    agree = [float((a - b).abs().max() / a.abs().max()) for a, b in zip(grads["torch"], grads["fused"])]
    density.grad, scale.grad = torch.zeros_like(density), torch.zeros_like(scale)   # from here on every call accumulates
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    inner = {k: max(20, int(args.window / (timed(fn, 10) * 1e-3))) for k, fn in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(args.rounds):           # alternate the versions inside every round
        for k, fn in fns.items():
            times[k].append(timed(fn, inner[k]))
    result = {"device": torch.cuda.get_device_name(0), "N": n, "rounds": args.rounds, "window_s": args.window,
              "lambda_opacity": LAMBDA_OPACITY, "lambda_scale": LAMBDA_SCALE, "means": values,
              "grad_rel_diff_fused_vs_torch": {"density": agree[0], "scale": agree[1]}}
    for k, ts in times.items():
        result[k] = {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "calls_per_window": inner[k]}
    result["saved_ms"] = round(result["torch"]["ms"] - result["fused"]["ms"], 4)
    result["spread_ms"] = round(max(result[k]["max_ms"] - result[k]["min_ms"] for k in fns), 4)
    result["speedup"] = round(result["torch"]["ms"] / result["fused"]["ms"], 2)
    result["faster_by_more_than_the_spread"] = result["saved_ms"] > result["spread_ms"]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
