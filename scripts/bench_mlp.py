"""The NHT decoder's network (3dgrut_amd/tcnn.py) at the shipped shape - 24 features, SH degree 3, 3 hidden layers of 128, sigmoid -
five ways on one MI355X, in one process, alternating:

    python scripts/bench_mlp.py [--rounds 15] [--window 0.2] [--size 1080p|800x800|all] [--time-limit 300] [--out profiles/mlp_bench.json]

  torch_fwd        mlp_torch under no_grad: the model in plain fp32 torch (what every tensor takes that the kernel does not)
  fused_fwd        the fused HIP forward (csrc/mlp.hip), under no_grad: inference, validation, the GUI
  fused_fwd_bwd    the training Function: the HIP forward, then a backward that recomputes mlp_torch from the saved input and weights
  torch_fwd_bwd    mlp_torch alone, forward and autograd's backward
  fused_step       the training Function after install_fused_backward(): the HIP forward and the fused HIP backward (csrc/mlp_backward.hip)

Random data: weights from the module's Xavier initialisation, features ~ N(0, 0.5), unit directions scaled by sh_scale = 3 (zero-filled
operands would read high).  The fused forward is first held against mlp_torch on the timed input.  Method of scripts/bench_ppisp.py:
every variant warmed up, device events around as many calls as fill `--window` seconds (counted per variant from a calibration run, at
least 10), the variants alternating inside every round; median and spread (min / max) over the rounds.  These are whole-call times
(allocations, autograd, every launch).  The forward's arithmetic (2 flops per weight and pixel) and its least memory traffic (the input
row and the output row) are printed with the rates they imply.  No assertion on any time.  The script ends itself after `--time-limit`
seconds.  Prints one JSON line and writes it to --out.  Fails without a GPU: the fused path has nothing to fall back to."""
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
    ap.add_argument("--time-limit", type=int, default=300, help="seconds after which the script ends itself")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp.py needs a GPU (the fused path has no CPU fallback)")
    signal.alarm(args.time_limit)
    tcnn = importlib.import_module("3dgrut_amd.tcnn")
    features, degree, width, layers, sh_scale = 24, 3, 128, 3, 3.0
    net = tcnn.NetworkWithInputEncoding(
        features + 3, 3,
        {"otype": "Composite", "nested": [{"otype": "Identity", "n_dims_to_encode": features},
                                          {"otype": "SphericalHarmonics", "degree": degree, "n_dims_to_encode": 3}]},
        {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "Sigmoid", "n_neurons": width, "n_hidden_layers": layers}).cuda()
    cfg, params = net.cfg, net.params
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "config": cfg._asdict(),
              "lds_image_bytes": tcnn.lds_bytes(cfg), "cases": {}}
    for name, (h, w) in (("1080p", (1080, 1920)), ("800x800", (800, 800))):
        if args.size not in ("all", name):
            continue
        pixels = h * w
        g = torch.Generator(device="cuda").manual_seed(1)
        dirs = torch.nn.functional.normalize(torch.randn((pixels, 3), generator=g, device="cuda"), dim=-1)
        x = torch.cat([torch.randn((pixels, features), generator=g, device="cuda") * 0.5, (dirs * sh_scale + 1.0) * 0.5], dim=-1).contiguous()
        xg = x.clone().requires_grad_(True)
        weight = torch.randn((pixels, 3), generator=g, device="cuda")
        assert tcnn.takes_hip(params, x, cfg)

        def torch_fwd():
            with torch.no_grad():
                return tcnn.mlp_torch(params, x, cfg)

        def fused_fwd():
            with torch.no_grad():
                return net(x)

        def fused_fwd_bwd():
            params.grad = xg.grad = None
            (net(xg) * weight).sum().backward()

        def torch_fwd_bwd():
            params.grad = xg.grad = None
            (tcnn.mlp_torch(params, xg, cfg) * weight).sum().backward()

        def fused_step():
            previous = tcnn.install_fused_backward(True)
            try:
                fused_fwd_bwd()
            finally:
                tcnn.install_fused_backward(previous)

        fns = {"torch_fwd": torch_fwd, "fused_fwd": fused_fwd, "fused_fwd_bwd": fused_fwd_bwd, "torch_fwd_bwd": torch_fwd_bwd,
               "fused_step": fused_step}
        calls = tcnn.stats["hip_backward_calls"]
        fused_step()
        assert tcnn.stats["hip_backward_calls"] == calls + 1, "the fused backward did not run"
        grads_fused = (xg.grad.clone(), params.grad.clone())
        fused_fwd_bwd()
        backward_agree = [float((a - b).abs().max()) for a, b in zip(grads_fused, (xg.grad, params.grad))]
        agree = float((fused_fwd() - torch_fwd()).abs().max())
        for fn in fns.values():        # warm up every variant
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        inner = {k: max(10, int(args.window / (timed(fn, 5) * 1e-3))) for k, fn in fns.items()}   # enough calls to fill the window
        times = {k: [] for k in fns}
        for _ in range(args.rounds):   # alternate the variants inside every round
            for k, fn in fns.items():
                times[k].append(timed(fn, inner[k]))
        flops = 2.0 * pixels * (width * cfg.k0 + (layers - 1) * width * width + 3 * width)          # the arithmetic the model needs
        traffic = 4.0 * pixels * (features + 3 + 3)                                                   # input row + output row
        entry = {"H": h, "W": w, "max_abs_diff_fused_vs_torch": agree,
                 "max_abs_diff_fused_backward_vs_torch_backward": {"grad_x": backward_agree[0], "grad_params": backward_agree[1]}, "forward_gflop": round(flops * 1e-9, 2), "forward_mbytes": round(traffic * 1e-6, 1)}
        for k, ts in times.items():
            entry[k] = {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "calls_per_window": inner[k]}
        entry["fused_fwd"]["tflops"] = round(flops / (entry["fused_fwd"]["ms"] * 1e-3) * 1e-12, 1)
        entry["fused_fwd"]["gbytes_per_s"] = round(traffic / (entry["fused_fwd"]["ms"] * 1e-3) * 1e-9, 1)
        entry["forward_ratio_torch_over_fused"] = round(entry["torch_fwd"]["ms"] / entry["fused_fwd"]["ms"], 2)
        entry["step_ratio_torch_over_fused"] = round(entry["torch_fwd_bwd"]["ms"] / entry["fused_fwd_bwd"]["ms"], 2)
        entry["step_ratio_torch_over_fused_step"] = round(entry["torch_fwd_bwd"]["ms"] / entry["fused_step"]["ms"], 2)
        entry["fused_step_over_fused_fwd"] = round(entry["fused_step"]["ms"] / entry["fused_fwd"]["ms"], 2)
        result["cases"][name] = entry
        del x, xg, weight, dirs
        torch.cuda.empty_cache()
    signal.alarm(0)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
