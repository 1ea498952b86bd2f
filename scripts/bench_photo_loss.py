"""The image part of one training step's loss, forward plus backward, two ways on one MI355X, in one process, alternating:

    python scripts/bench_photo_loss.py [--rounds 15] [--window 0.2] [--size 1080p|800x800|all] [--out profiles/photo_loss_bench.json]

  parent   what the commit before the fused call runs on every step: the formula of Trainer3DGRUT.get_losses (trainer.py:687-747) as a
           chain of torch kernels (mask products, abs / mean, the permuted views) around this repository's fused_ssim, and autograd's
           mirror image of it, including the kernel that adds the L1 and the SSIM gradient into pred.grad
  fused    one photometric_loss call (csrc/loss.hip: loss_forward_kernel + loss_mean_kernel, loss_backward_kernel) and the same
           weighting of its three 0-dim results

Both compute total = 0.8 l1 + 0.2 (1 - ssim) (the reference's default weights; L2 off, as in its configs) on channels-last RGB, the
renderer's [1, H, W, 3] output, at 1080p and 800x800, with and without a [1, H, W, 1] mask, and call backward(); pred.grad is reset
before every call.  Method of scripts/bench_ssim.py: every variant warmed up, device events around as many calls as fill `--window`
seconds (counted per variant from a calibration run, at least 20), the two versions alternating inside every round; median and spread
(min / max) over the rounds.  These are whole-call times (autograd, allocations, every launch), which is what a training step pays.
`spread_ms` is the larger of the two versions' (max - min) over the rounds: a difference of the medians below it is not a difference.
The gradients of the two versions are compared first (faster and different is not faster).  Prints one JSON line and writes it to --out.
Fails without a GPU: there is nothing to fall back to."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAMBDA_L1, LAMBDA_SSIM = 0.8, 0.2


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
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--size", default="all", choices=["all", "1080p", "800x800"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photo_loss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_photo_loss.py needs a GPU (there is no CPU fallback)")
    losses = importlib.import_module("3dgrut_amd.losses")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "lambda_l1": LAMBDA_L1,
              "lambda_ssim": LAMBDA_SSIM, "cases": {}}
    for name, (h, w) in (("1080p", (1080, 1920)), ("800x800", (800, 800))):
        if args.size not in ("all", name):
            continue
        for masked in (False, True):
            g = torch.Generator(device="cuda").manual_seed(1)
            pred = torch.rand((1, h, w, 3), generator=g, device="cuda").requires_grad_(True)     # the renderer's [B, H, W, 3] output
            gt = (pred.detach() + 0.02 * torch.randn((1, h, w, 3), generator=g, device="cuda")).clamp(0, 1)
            mask = (torch.rand((1, h, w, 1), generator=g, device="cuda") < 0.8).float() if masked else None

            def parent_step():
                pred.grad = None
                rgb_gt, rgb_pred = gt, pred
                if mask is not None:
                    rgb_gt, rgb_pred = rgb_gt * mask, rgb_pred * mask
                l1 = torch.abs(rgb_pred - rgb_gt).mean()
                dssim = 1.0 - losses.ssim(torch.permute(rgb_pred, (0, 3, 1, 2)), torch.permute(rgb_gt, (0, 3, 1, 2)))
                (LAMBDA_L1 * l1 + LAMBDA_SSIM * dssim).backward()

            def fused_step():
                pred.grad = None
                l1, _, ssim = losses.photometric_loss(pred, gt, mask, l1=True, l2=False, ssim=True, padding="valid")
                (LAMBDA_L1 * l1 + LAMBDA_SSIM * (1.0 - ssim)).backward()

            fns = {"parent": parent_step, "fused": fused_step}
            parent_step()
            want = pred.grad.clone()
            fused_step()
            agree = float((want - pred.grad).abs().max() / want.abs().max())
            for fn in fns.values():        # warm up both versions
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            inner = {k: max(20, int(args.window / (timed(fn, 10) * 1e-3))) for k, fn in fns.items()}   # enough calls to fill the window
            times = {k: [] for k in fns}
            for _ in range(args.rounds):   # alternate the versions inside every round
                for k, fn in fns.items():
                    times[k].append(timed(fn, inner[k]))
            entry = {"H": h, "W": w, "masked": masked, "grad_rel_diff_fused_vs_parent": agree}
            for k, ts in times.items():
                entry[k] = {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                            "calls_per_window": inner[k]}
            entry["saved_ms"] = round(entry["parent"]["ms"] - entry["fused"]["ms"], 4)
            entry["spread_ms"] = round(max(entry[k]["max_ms"] - entry[k]["min_ms"] for k in fns), 4)
            entry["speedup"] = round(entry["parent"]["ms"] / entry["fused"]["ms"], 2)
            entry["faster_by_more_than_the_spread"] = entry["saved_ms"] > entry["spread_ms"]
            result["cases"][f"{name}{'-mask' if masked else ''}"] = entry
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
