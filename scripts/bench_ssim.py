"""Fused SSIM (csrc/loss.hip through 3dgrut_amd/losses.py) against the plain-torch formulation a user would have to write without it,
on one MI355X, in one process, alternating:

    python scripts/bench_ssim.py [--rounds 15] [--window 0.2] [--size 1080p|800x800|all]

Sizes: 1080p and 800x800, RGB, channels-last views exactly as trainer.py:717-718 passes them.  For each size: forward (inference) and
forward + backward, fused and torch, every shape warmed up, device events around as many calls as fill `--window` seconds (counted per
variant from a calibration run, at least 20), the two versions alternating inside every round; median and spread (min / max) over the
rounds.  GB/s come from the byte model of DESIGN.md §7e with P = B C H W: forward
training reads 8P and writes 12P, backward reads 20P and writes 4P (44P per training step), forward inference reads 8P; the fraction is
of the 8 TB/s HBM peak.  The working set (images, three planes, gradient: 24P bytes, 149 MB at 1080p) fits the 256 MiB Infinity Cache and
the calls repeat on the same buffers, so the rate is what the memory system as a whole delivers, not an HBM-only rate; kernel times
come from a kernel trace of this script (profiles/ssim_kernel_stats.txt).  These are whole-call rates (launches and the tiny reduction included), not kernel rates.  Prints one JSON line.
Fails without a GPU: there is nothing to fall back to."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def torch_ssim(img1, img2, window):
    """The published formula with grouped conv2d (zero padding), mean over the 5-pixel crop: padding="valid"."""
    c = img1.shape[1]
    conv = lambda t: F.conv2d(t, window, padding=5, groups=c)   # noqa: E731
    mu1, mu2 = conv(img1), conv(img2)
    s1, s2, s12 = conv(img1 * img1) - mu1 * mu1, conv(img2 * img2) - mu2 * mu2, conv(img1 * img2) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s1 + s2 + 9e-4))
    return m[:, :, 5:-5, 5:-5].mean()


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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim.py needs a GPU (there is no CPU fallback)")
    losses = importlib.import_module("3dgrut_amd.losses")
    i = torch.arange(11, dtype=torch.float64)
    taps = torch.exp(-((i - 5) ** 2) / 4.5)
    taps = (taps / taps.sum()).float()
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "sizes": {}}
    for name, (h, w) in (("1080p", (1080, 1920)), ("800x800", (800, 800))):
        if args.size not in ("all", name):
            continue
        g = torch.Generator(device="cuda").manual_seed(1)
        pred = torch.rand((1, h, w, 3), generator=g, device="cuda").requires_grad_(True)     # the renderer's [B, H, W, 3] output
        gt = (pred.detach() + 0.02 * torch.randn((1, h, w, 3), generator=g, device="cuda")).clamp(0, 1)
        window = torch.outer(taps, taps).cuda().expand(3, 1, 11, 11).contiguous()
        views = lambda: (torch.permute(pred, (0, 3, 1, 2)), torch.permute(gt, (0, 3, 1, 2)))   # noqa: E731

        def fused_fwd():
            with torch.no_grad():
                losses.fused_ssim(*views(), padding="valid")

        def fused_step():
            pred.grad = None
            (1.0 - losses.fused_ssim(*views(), padding="valid")).backward()

        def torch_fwd():
            with torch.no_grad():
                torch_ssim(*views(), window)

        def torch_step():
            pred.grad = None
            (1.0 - torch_ssim(*views(), window)).backward()

        fns = {"fused_fwd": fused_fwd, "torch_fwd": torch_fwd, "fused_fwd_bwd": fused_step, "torch_fwd_bwd": torch_step}
        fused_step()
        gf = pred.grad.clone()
        torch_step()
        agree = float((gf - pred.grad).abs().max() / pred.grad.abs().max())     # faster and different is not faster
        for fn in fns.values():        # warm up every shape and both versions
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        inner = {k: max(20, int(args.window / (timed(fn, 10) * 1e-3))) for k, fn in fns.items()}   # enough calls to fill the window
        times = {k: [] for k in fns}
        for _ in range(args.rounds):   # alternate the versions inside every round
            for k, fn in fns.items():
                times[k].append(timed(fn, inner[k]))
        p = 3 * h * w
        model = {"fused_fwd": 8 * p, "fused_fwd_bwd": 44 * p}
        entry = {"P": p, "grad_rel_diff_fused_vs_torch": agree}
        for k, ts in times.items():
            ms = statistics.median(ts)
            entry[k] = {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "calls_per_window": inner[k]}
            if k in model:
                rate = model[k] / (ms * 1e-3)
                entry[k].update(model_bytes=model[k], GBps=round(rate / 1e9, 1), hbm_fraction=round(rate / HBM_PEAK, 4))
        entry["speedup_fwd"] = round(entry["torch_fwd"]["ms"] / entry["fused_fwd"]["ms"], 2)
        entry["speedup_fwd_bwd"] = round(entry["torch_fwd_bwd"]["ms"] / entry["fused_fwd_bwd"]["ms"], 2)
        result["sizes"][name] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
