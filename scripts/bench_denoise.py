"""The playground's frame denoiser (3dgrut_amd/denoise.py) on one MI355X: what a call costs, and what it does to a path-traced frame.

    python scripts/bench_denoise.py [--rounds 7] [--window 0.2] [--frames 256] [--width 320] [--height 240] [--out profiles/denoise_bench.json]

Timing, at 1920x1080 and 800x800 on uniform random frames, the defaults (f = 3, r = 7, h = 0.1), one process, alternating:

  torch    denoise_torch: the model as a chain of torch ops, one pass of about twenty launches per candidate offset (224 of them)
  fused    denoise: one launch of csrc/denoise.hip

Method of scripts/bench_regularizers.py: both versions warmed up, device events around as many calls as fill `--window` seconds (at least
3), the versions alternating inside every round; median and spread (min / max) over the rounds.  These are whole-call times (allocation of
the result included).  `spread_ms` is the larger of the two versions' (max - min): a difference of the medians below it is not a
difference.  The two results are compared first, against the model's own error bound (tests/denoise_reference.py states it).

Sweep against a converged frame: the `mixed` scene of workloads/playground_scenes.py, `--frames` frames with different frame_id (the seed
of the path tracer's random streams).  As in the reference's engine (engine.py:865-870, 1077-1078) a frame is clamped to [0, 1], frames are
averaged before the output gamma and the gamma (1 / 2.2) comes last: the converged frame is mean(clamp(frame_i)) ^ (1 / 2.2), the
one-sample frame clamp(frame_0) ^ (1 / 2.2).  For h in {0.05, 0.1, 0.15, 0.2, 0.3} and r in {5, 7, 10} (f = 3): PSNR (peak 1) of the
denoised one-sample frame against the converged frame, next to the raw one-sample frame's.  Prints one JSON line and writes it to --out.
Fails without a GPU: there is nothing to measure."""
import argparse
import importlib
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SWEEP_H = (0.05, 0.1, 0.15, 0.2, 0.3)
SWEEP_R = (5, 7, 10)
U = 2.0 ** -24


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def time_pair(dn, height, width, rounds, window):
    g = torch.Generator(device="cuda").manual_seed(height * 10000 + width)
    frame = torch.rand((1, height, width, 3), generator=g, device="cuda")
    fns = {"torch": lambda: dn.denoise_torch(frame), "fused": lambda: dn.denoise(frame)}
    got = {k: fn() for k, fn in fns.items()}                # faster and different is not faster
    f, r = dn.DEFAULTS["patch_radius"], dn.DEFAULTS["search_radius"]
    eps = dn.X_MAX * (3 * (2 * f + 1) ** 2 + 4) * U + 24 * U
    bound = 2 * eps * 1.0 + ((2 * r + 1) ** 2 + 4) * U * 1.0    # spread and magnitude of uniform noise in [0, 1): at most 1
    diff = float((got["torch"] - got["fused"]).abs().max())
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    inner = {k: max(3, int(window / (timed(fn, 2) * 1e-3))) for k, fn in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, inner[k]))
    out = {"height": height, "width": width, "max_abs_diff_fused_vs_torch": diff, "two_bounds": 2 * bound}
    for k, ts in times.items():
        out[k] = {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "calls_per_window": inner[k]}
    out["saved_ms"] = round(out["torch"]["ms"] - out["fused"]["ms"], 4)
    out["spread_ms"] = round(max(out[k]["max_ms"] - out[k]["min_ms"] for k in fns), 4)
    out["speedup"] = round(out["torch"]["ms"] / out["fused"]["ms"], 2)
    out["faster_by_more_than_the_spread"] = out["saved_ms"] > out["spread_ms"]
    return out


def render_frames(width, height, frames, gaussians, bounces):
    """-> (one-sample frame, converged frame), both [1, H, W, 3] on the device, after the output gamma."""
    ps = importlib.import_module("workloads.playground_scenes")
    syn = importlib.import_module("workloads.synthetic")
    pt = importlib.import_module("3dgrut_amd.playground_tracer")
    sc = ps.make_playground_scene("mixed", width=width, height=height, n=gaussians, seed=11)
    tr = pt.Tracer({"render": {}})
    g = syn.SimpleGaussians(sc["density12"], sc["sph"], requires_grad=False)
    tr.build_gs_acc(g, rebuild=True)
    t = lambda a: None if a is None else torch.as_tensor(a, device="cuda")   # noqa: E731
    m = sc["mesh"]
    tr.build_mesh_acc(t(m["vertices"]), t(m["triangles"]))
    mats = [dict(diffuse_map=t(x["diffuse_tex"]), emissive_map=t(x["emissive_tex"]), metallic_roughness_map=t(x["metallic_roughness_tex"]),
                 normal_map=t(x["normal_tex"]), diffuse_factor=x["diffuse_factor"], emissive_factor=x["emissive_factor"],
                 metallic_factor=x["metallic_factor"], roughness_factor=x["roughness_factor"], alpha_mode=x["alpha_mode"],
                 alpha_cutoff=x["alpha_cutoff"], transmission_factor=x["transmission_factor"], ior=x["ior"]) for x in sc["materials"]]
    fixed = dict(ray_max_t=t(sc["ray_max_t"])[None], material_uv=t(m["mat_uv"]), material_id=t(m["mat_id"])[:, None], materials=mats,
                 refractive_index=t(m["refractive_index"]), envmap=t(sc["envmap"]), envmap_offset=t(sc["envmap_offset"]), max_pbr_bounces=bounces)
    ray_o, ray_d = t(sc["ray_o"])[None], t(sc["ray_d"])[None]
    mesh_args = (t(m["triangles"]), t(m["vertex_normals"]), t(m["vertex_tangents"]), t(m["vertex_has_tangents"]), t(m["prim_type"]))
    total = torch.zeros((1, height, width, 3), dtype=torch.float64, device="cuda")
    first = None
    for frame_id in range(frames):
        out = tr.render_playground(g, ray_o, ray_d, ps.OPT_SMOOTH_NORMALS, *mesh_args, frame_id=frame_id, **fixed)
        linear = out["pred_features"].clamp(0, 1)
        total += linear.double()
        if first is None:
            first = linear.clone()
    gamma = 1 / 2.2
    return first ** gamma, (total / frames).float() ** gamma, tr


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else round(10 * math.log10(1.0 / mse), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--gaussians", type=int, default=12000)
    ap.add_argument("--bounces", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_denoise.py needs a GPU (there is nothing to measure without one)")
    dn = importlib.import_module("3dgrut_amd.denoise")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "defaults": dict(dn.DEFAULTS),
              "timing": [time_pair(dn, h, w, args.rounds, args.window) for h, w in ((1080, 1920), (800, 800))]}
    one, converged, tracer = render_frames(args.width, args.height, args.frames, args.gaussians, args.bounces)
    sweep = {"scene": "mixed", "width": args.width, "height": args.height, "frames": args.frames, "gaussians": args.gaussians,
             "patch_radius": dn.DEFAULTS["patch_radius"], "psnr_raw_db": psnr(one, converged),
             "psnr_db": {f"r={r}": {f"h={h}": psnr(dn.denoise(one, dn.DEFAULTS["patch_radius"], r, h), converged) for h in SWEEP_H} for r in SWEEP_R}}
    sweep["psnr_tracer_defaults_db"] = psnr(tracer.denoise(one), converged)
    sweep["default_moves_towards_converged"] = sweep["psnr_tracer_defaults_db"] > sweep["psnr_raw_db"]
    result["sweep"] = sweep
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
