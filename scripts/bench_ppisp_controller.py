"""The PPISP controller of one camera, two ways on one MI355X, in one process, alternating:

    python scripts/bench_ppisp_controller.py [--rounds 15] [--window 0.2] [--size 1080p|800x800|all] [--time-limit 240]
                                             [--out profiles/ppisp_controller_bench.json]

  torch    `_PPISPController.forward` as nn.Sequential runs it (the path of every input the kernels do not take): a 16-channel
           full-resolution activation, a max-pool, two more 1x1 convolutions, an adaptive pool and the trunk, autograd's mirror image backward
  fused    the same module with install_fused_controller() on (csrc/ppisp_controller.hip: three launches forward, five backward)

Two workloads per size: `forward` is a novel view (no_grad: validation, Renderer.from_checkpoint, the GUI), `step` is forward plus
backward() of a weighted sum of the nine outputs with the gradients reset before every call (a training step of the controller's phase).
Method of scripts/bench_ppisp.py: every variant warmed up, device events around as many calls as fill `--window` seconds (counted per
variant from a calibration run, at least 20), the variants alternating inside every round; median and spread (min / max) over the rounds.
These are whole-call times (autograd, allocations, every launch).  The heads are drawn at random (at their zero initialisation every
gradient below them is 0); outputs and gradients of the two paths are compared first and reported, no assertion on any ratio.
The script ends itself after `--time-limit` seconds.  Prints one JSON line and writes it to --out.  Fails without a GPU."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--size", default="all", choices=["all", "1080p", "800x800"])
    ap.add_argument("--time-limit", type=int, default=240, help="seconds after which the script ends itself")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppisp_controller_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ppisp_controller.py needs a GPU (the fused path has no CPU fallback)")
    signal.alarm(args.time_limit)
    ppisp = importlib.import_module("3dgrut_amd.ppisp")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "cases": {}}
    for name, (h, w) in (("1080p", (1080, 1920)), ("800x800", (800, 800))):
        if args.size not in ("all", name):
            continue
        torch.manual_seed(1)
        ctrl = ppisp._PPISPController()
        with torch.no_grad():
            for head in (ctrl.exposure_head, ctrl.color_head):
                head.weight.normal_(0.0, 0.1)
                head.bias.normal_(0.0, 0.1)
        ctrl = ctrl.cuda()
        g = torch.Generator(device="cuda").manual_seed(1)
        hdr = torch.rand((h, w, 3), generator=g, device="cuda") * 1.5
        prior = torch.full((1,), 0.3, device="cuda")
        weight = torch.randn(9, generator=g, device="cuda")
        params = list(ctrl.parameters())

        def forward():
            with torch.no_grad():
                return ctrl(hdr, prior)

        def step():
            for p in params:
                p.grad = None
            e, c = ctrl(hdr, prior)
            (e * weight[0] + (c * weight[1:]).sum()).backward()

        def variant(fn, fused):
            def run():
                ppisp.install_fused_controller(fused)
                return fn()
            return run

        fns = {"forward_torch": variant(forward, False), "forward_fused": variant(forward, True),
               "step_torch": variant(step, False), "step_fused": variant(step, True)}
        e_t, c_t = fns["forward_torch"]()
        e_f, c_f = fns["forward_fused"]()
        out_t, out_f = torch.cat([e_t.reshape(1), c_t]), torch.cat([e_f.reshape(1), c_f])
        fns["step_torch"]()
        want = [p.grad.clone() for p in params]
        fns["step_fused"]()
        agree = max(float((a - p.grad).abs().max() / a.abs().max()) for a, p in zip(want, params))
        for fn in fns.values():        # warm up every variant
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        inner = {k: max(20, int(args.window / (timed(fn, 10) * 1e-3))) for k, fn in fns.items()}   # enough calls to fill the window
        times = {k: [] for k in fns}
        for _ in range(args.rounds):   # alternate the variants inside every round
            for k, fn in fns.items():
                times[k].append(timed(fn, inner[k]))
        ppisp.install_fused_controller(False)
        entry = {"H": h, "W": w, "out_rel_diff_fused_vs_torch": float((out_f - out_t).abs().max() / out_t.abs().max()),
                 "grad_rel_diff_fused_vs_torch": agree}
        for k, ts in times.items():
            entry[k] = {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "calls_per_window": inner[k]}
        for kind in ("forward", "step"):
            entry[f"{kind}_ratio"] = round(entry[f"{kind}_torch"]["ms"] / entry[f"{kind}_fused"]["ms"], 2)
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
