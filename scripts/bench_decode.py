"""The NHT decode stage at the shipped shape - 24 features, SH degree 3, 3 hidden layers of 128, sigmoid, sh_scale 3 - two ways on one
MI355X, in one process, alternating:

    python scripts/bench_decode.py [--rounds 15] [--window 0.2] [--size 1080p|800x800|all] [--time-limit 300] [--out profiles/decode_bench.json]

  parent_fwd   the operations of the reference's apply_feature_decoder and FeatureDecoder._process in torch (einsum, normalize, clamp and
               divide, scale, cat, then the product with alpha) around the fused network of 3dgrut_amd.tcnn, under no_grad
  fused_fwd    3dgrut_amd.decoder.decode under no_grad: ONE launch of csrc/mlp.hip's decode instantiation
  parent_step  the same torch operations with grad enabled around the network's training Function, forward and backward
  fused_step   decoder.decode with grad enabled, forward and backward: the decode instantiations of csrc/mlp.hip and csrc/mlp_backward.hip

each with unpremultiply_alpha off and on, always after tcnn.install_fused_backward(): both paths run the fused HIP backward of the
network, so the difference is the torch operations around it.  Gradients go to the feature map, to the weights and (with
unpremultiply_alpha) to alpha, as in training.

Random data: weights from the module's Xavier initialisation, features ~ N(0, 0.5), pinhole camera rays, one random rotation, alpha in
[0.05, 1].  The fused call is first held against the parent's path on the timed input.  Method of scripts/bench_mlp.py: every variant
warmed up, device events around as many calls as fill `--window` seconds (counted per variant from a calibration run, at least 10),
the variants alternating inside every round; median and spread (min / max) over the rounds.  These are whole-call times (allocations,
autograd, every launch).  The bytes each path has to move at the least (every tensor an operation reads or writes, once) are printed
with the result.  No assertion on any time.  The script ends itself after `--time-limit` seconds.  Prints one JSON line and writes it
to --out.  Fails without a GPU: the fused path has nothing to fall back to."""
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


def forward_bytes(pixels, features, n_out, unpremultiply):
    """(parent, fused): the bytes of every tensor that an operation of the forward reads or writes, once each"""
    p, row, d, o = 4.0 * pixels, features + 3, 3, n_out
    parent = p * (2 * d) + p * (2 * d) + p * (2 * d)               # einsum, normalize, (dirs * sh_scale + 1) * 0.5 as one pass
    parent += p * (features + d + row)                            # cat: reads both parts, writes the rows
    parent += p * (row + o)                                       # the network: reads the rows, writes the output
    fused = p * (features + d + o)
    if unpremultiply:
        parent += p * 2 + p * (2 * features + 1) + p * (2 * o + 1)   # clamp, divide, product with a_s
        fused += p
    return parent, fused


def step_bytes(pixels, features, n_out, unpremultiply):
    """(parent, fused): forward plus backward; the backward reads what it saved and grad_out and writes every gradient once"""
    p, row, d, o = 4.0 * pixels, features + 3, 3, n_out
    parent_fwd, fused_fwd = forward_bytes(pixels, features, n_out, unpremultiply)
    parent = parent_fwd + p * (row + o + row)                     # the network's backward: rows, grad_out, grad of the rows
    parent += p * (row + features)                                # cat's backward: the slice of the feature columns into its own tensor
    fused = fused_fwd + p * (features + d + o + features)         # features, rays, grad_out in; grad_features out
    if unpremultiply:
        parent += p * (3 * o + 1) + p * (2 * o + 1)                # product's backward: grad of y (reads go, a_s) and of a_s (reads go, y; reduces)
        parent += p * (2 * features + 1) + p * (3 * features + 2)  # divide's backward: grad of features, and of a_s (reduces)
        parent += p * 3 + p * 2                                    # the two gradients of a_s summed, clamp's gate
        fused += p * 2                                             # alpha in, grad_alpha out
    return parent, fused


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--size", default="all", choices=["all", "1080p", "800x800"])
    ap.add_argument("--time-limit", type=int, default=300, help="seconds after which the script ends itself")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode.py needs a GPU (the fused path has no CPU fallback)")
    signal.alarm(args.time_limit)
    tcnn = importlib.import_module("3dgrut_amd.tcnn")
    decoder = importlib.import_module("3dgrut_amd.decoder")
    features, degree, width, layers, sh_scale = 24, 3, 128, 3, 3.0
    net = tcnn.NetworkWithInputEncoding(
        features + 3, 3,
        {"otype": "Composite", "nested": [{"otype": "Identity", "n_dims_to_encode": features},
                                          {"otype": "SphericalHarmonics", "degree": degree, "n_dims_to_encode": 3}]},
        {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "Sigmoid", "n_neurons": width, "n_hidden_layers": layers}).cuda()
    params = net.params
    previous = tcnn.install_fused_backward(True)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "config": net.cfg._asdict(),
              "sh_scale": sh_scale, "fused_backward": True, "cases": {}}
    for name, (h, w) in (("1080p", (1080, 1920)), ("800x800", (800, 800))):
        if args.size not in ("all", name):
            continue
        pixels = h * w
        g = torch.Generator(device="cuda").manual_seed(1)
        feats = (torch.randn((pixels, features), generator=g, device="cuda") * 0.5).requires_grad_(True)
        rays = torch.cat([torch.rand((pixels, 2), generator=g, device="cuda") * 1.6 - 0.8, torch.ones((pixels, 1), device="cuda")], dim=-1).contiguous()
        alpha = (torch.rand(pixels, generator=g, device="cuda") * 0.95 + 0.05).requires_grad_(True)
        rot = torch.linalg.qr(torch.randn((1, 3, 3), generator=g, device="cuda"))[0].contiguous()
        weight = torch.randn((pixels, 3), generator=g, device="cuda")
        for unpremultiply in (False, True):
            cfg = decoder.DecodeConfig(net.cfg, sh_scale, unpremultiply, False)
            assert decoder.takes_hip(params, feats, alpha, rays, rot, pixels, cfg)

            def parent():
                rows, a_s = decoder.assemble_rows(feats, alpha, rays, rot, pixels, cfg)
                rgb = net(rows)
                return (rgb if a_s is None else rgb * a_s).float()

            def fused():
                return decoder.decode(params, feats, alpha, rays, rot, pixels, cfg)

            def no_grad(fn):
                def run():
                    with torch.no_grad():
                        return fn()
                return run

            def step(fn):
                def run():
                    params.grad = feats.grad = alpha.grad = None
                    (fn() * weight).sum().backward()
                return run

            fns = {"parent_fwd": no_grad(parent), "fused_fwd": no_grad(fused), "parent_step": step(parent), "fused_step": step(fused)}
            calls = (decoder.stats["hip_calls"], decoder.stats["hip_backward_calls"], tcnn.stats["hip_backward_calls"])
            fns["fused_step"]()
            grads_fused = [t.grad.clone() for t in (feats, params)] + ([alpha.grad.clone()] if unpremultiply else [])
            fns["parent_step"]()
            grads_parent = [feats.grad, params.grad] + ([alpha.grad] if unpremultiply else [])
            assert (decoder.stats["hip_calls"], decoder.stats["hip_backward_calls"], tcnn.stats["hip_backward_calls"]) == \
                (calls[0] + 1, calls[1] + 1, calls[2] + 1), "a fused kernel did not run"
            agree = {"forward": float((fns["fused_fwd"]() - fns["parent_fwd"]()).abs().max()),
                     "grad": [float((a - b).abs().max()) for a, b in zip(grads_fused, grads_parent)]}
            for fn in fns.values():        # warm up every variant
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            inner = {k: max(10, int(args.window / (timed(fn, 5) * 1e-3))) for k, fn in fns.items()}   # enough calls to fill the window
            times = {k: [] for k in fns}
            for _ in range(args.rounds):   # alternate the variants inside every round
                for k, fn in fns.items():
                    times[k].append(timed(fn, inner[k]))
            fwd_bytes, all_bytes = forward_bytes(pixels, features, 3, unpremultiply), step_bytes(pixels, features, 3, unpremultiply)
            entry = {"H": h, "W": w, "unpremultiply_alpha": unpremultiply, "max_abs_diff_fused_vs_parent": agree,
                     "forward_mbytes": {"parent": round(fwd_bytes[0] * 1e-6, 1), "fused": round(fwd_bytes[1] * 1e-6, 1)},
                     "step_mbytes": {"parent": round(all_bytes[0] * 1e-6, 1), "fused": round(all_bytes[1] * 1e-6, 1)}}
            for k, ts in times.items():
                entry[k] = {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "calls_per_window": inner[k]}
            entry["forward_ratio_parent_over_fused"] = round(entry["parent_fwd"]["ms"] / entry["fused_fwd"]["ms"], 2)
            entry["step_ratio_parent_over_fused"] = round(entry["parent_step"]["ms"] / entry["fused_step"]["ms"], 2)
            result["cases"][f"{name}_unpremultiply_{'on' if unpremultiply else 'off'}"] = entry
        del feats, rays, alpha, weight
        torch.cuda.empty_cache()
    tcnn.install_fused_backward(previous)
    signal.alarm(0)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
