"""PPISP post-processing of one training step, forward plus backward, two ways on one MI355X, in one process, alternating:

    python scripts/bench_ppisp.py [--rounds 15] [--window 0.2] [--size 1080p|800x800|all] [--time-limit 240] [--out profiles/ppisp_bench.json]

  torch    the model restated in fp32 torch (3dgrut_amd.ppisp.ppisp_torch, the path of every tensor that is not an fp32 CUDA tensor):
           several dozen elementwise kernels forward, autograd's mirror image backward
  fused    one ppisp_apply call (csrc/ppisp.hip: ppisp_forward_kernel; ppisp_backward_kernel + ppisp_finish_kernel)

Both take the renderer's [H*W, 3] output and the batch's pixel coordinates, apply exposure, vignetting, colour and response curve with
randomly drawn parameters (one camera, one frame), and call backward() on a weighted sum; the gradients reach rgb and all four parameter
tensors and are reset before every call.  Method of scripts/bench_photo_loss.py: every variant warmed up, device events around as many
calls as fill `--window` seconds (counted per variant from a calibration run, at least 20), the two versions alternating inside every
round; median and spread (min / max) over the rounds.  These are whole-call times (autograd, allocations, every launch), which is what a
training step pays.  The two versions' gradients are compared first; pixels with a curve input within 1e-3 of a kink of the response
curve (0, 1, the centre), where two fp32 evaluations may land on either side, carry no upstream gradient.  No assertion on the ratio.
The script ends itself after `--time-limit` seconds.  Prints one JSON line and writes it to --out.  Fails without a GPU: the fused path
has nothing to fall back to."""
import argparse
import importlib
import json
import os
import signal
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def draw_parameters(ppisp, device):
    """One camera, one frame, drawn like the reference's export test draws them."""
    g = torch.Generator().manual_seed(23)
    crf = torch.tensor(ppisp.CRF_IDENTITY).repeat(1, 3, 1) + torch.empty(1, 3, 4).normal_(0.0, 0.08, generator=g)
    vig = torch.cat([torch.empty(1, 3, 2).normal_(0.0, 0.04, generator=g), torch.empty(1, 3, 3).uniform_(-0.35, 0.02, generator=g)], -1)
    par = dict(exposure=torch.empty(1).uniform_(-0.35, 0.35, generator=g), color=torch.empty(1, 8).normal_(0.0, 0.35, generator=g), vignetting=vig, crf=crf)
    return {k: v.to(device).requires_grad_(True) for k, v in par.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--size", default="all", choices=["all", "1080p", "800x800"])
    ap.add_argument("--time-limit", type=int, default=240, help="seconds after which the script ends itself")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppisp_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ppisp.py needs a GPU (the fused path has no CPU fallback)")
    signal.alarm(args.time_limit)
    ppisp = importlib.import_module("3dgrut_amd.ppisp")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "cases": {}}
    for name, (h, w) in (("1080p", (1080, 1920)), ("800x800", (800, 800))):
        if args.size not in ("all", name):
            continue
        g = torch.Generator(device="cuda").manual_seed(1)
        rgb = (torch.rand((h * w, 3), generator=g, device="cuda") * 1.3).requires_grad_(True)     # some samples beyond the curve's end
        weight = torch.randn((h * w, 3), generator=g, device="cuda")
        y, x = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
        pc = (torch.stack((x, y), -1) + 0.5).reshape(-1, 2)
        par = draw_parameters(ppisp, "cuda")
        leaves = [rgb, *par.values()]
        with torch.no_grad():          # keep the upstream gradient away from the curve's kinks
            z = ppisp.ppisp_torch(rgb, pc, w, h, par["exposure"][0], par["color"][0], par["vignetting"][0], None)
            centre = torch.sigmoid(par["crf"][0, :, 3])
            near = (((z.abs() < 1e-3) & (z != 0)) | ((z - 1).abs() < 1e-3) | ((z - centre).abs() < 1e-3)).any(-1, keepdim=True)
            weight = weight * ~near

        def reset():
            for t in leaves:
                t.grad = None

        def torch_step():
            reset()
            out = ppisp.ppisp_torch(rgb, pc, w, h, par["exposure"][0], par["color"][0], par["vignetting"][0], par["crf"][0])
            (out * weight).sum().backward()

        def fused_step():
            reset()
            out = ppisp.ppisp_apply(exposure_params=par["exposure"], vignetting_params=par["vignetting"], color_params=par["color"],
                                    crf_params=par["crf"], rgb_in=rgb, pixel_coords=pc, resolution_w=w, resolution_h=h, camera_idx=0, frame_idx=0)
            (out * weight).sum().backward()

        fns = {"torch": torch_step, "fused": fused_step}
        torch_step()
        want = [t.grad.clone() for t in leaves]
        fused_step()
        agree = max(float((a - t.grad).abs().max() / a.abs().max()) for a, t in zip(want, leaves))
        for fn in fns.values():        # warm up both versions
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        inner = {k: max(20, int(args.window / (timed(fn, 10) * 1e-3))) for k, fn in fns.items()}   # enough calls to fill the window
        times = {k: [] for k in fns}
        for _ in range(args.rounds):   # alternate the versions inside every round
            for k, fn in fns.items():
                times[k].append(timed(fn, inner[k]))
        entry = {"H": h, "W": w, "grad_rel_diff_fused_vs_torch": agree, "pixels_without_upstream_gradient": float(near.float().mean())}
        for k, ts in times.items():
            entry[k] = {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "calls_per_window": inner[k]}
        entry["saved_ms"] = round(entry["torch"]["ms"] - entry["fused"]["ms"], 4)
        entry["spread_ms"] = round(max(entry[k]["max_ms"] - entry[k]["min_ms"] for k in fns), 4)
        entry["ratio"] = round(entry["torch"]["ms"] / entry["fused"]["ms"], 2)
        result["cases"][name] = entry
    signal.alarm(0)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
