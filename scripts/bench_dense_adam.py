"""The optimizer step of the shipped configs (optimizer.type: adam) three ways on one MI355X, in one process, alternating:

    python scripts/bench_dense_adam.py [--n 1000000] [--rounds 21] [--steps 50] [--device-steps 20] [--sleep-ms 60] [--out profiles/dense_adam_bench.json]

  torch      torch.optim.Adam(params, lr=0, eps=1e-15, fused=True), what threedgrut/model/model.py:807-810 builds: one pass through the
             optimizer per parameter group
  fused      3dgrut_amd.optimizers.FusedAdam over the same parameters: grut_adam_update, one streaming launch behind a prologue launch
  selective  grut_selective_adam_update with GRUT_VIS_NONE called directly on the same parameters and grads (the existing launch that moves
             the same 28 B per element; its `step` here is the bare library call, no optimizer object around it)

The model is N Gaussians at SH degree 3 with the six groups and learning rates of configs/base_gs.yaml (positions, density, rotation,
scale, albedo, specular: 59 floats per Gaussian); every optimizer has moments of its own, the parameters and grads are shared.  Per
round and optimizer, a block of steps (--device-steps for (a), --steps for (b) and (c)) is timed three ways:

  (a) device_ms   device events around the block while the host is ahead of the device: a torch.cuda._sleep kernel of about
                  --sleep-ms runs first and the block is queued behind it, so the events see the kernels and the gaps the DEVICE leaves
                  between them, not the host's enqueue time; `host_ahead_in_every_device_block` says whether the head start was still
                  running when the last step had been queued (where it is false, device_ms may be bound by the host: an upper bound -
                  unless the host was merely held with a backlog queued, which scripts/probe_dense_adam_queue.py tells apart)
  (b) call_ms     host clock around the block with one synchronisation at its end: max(host, device) per step
  (c) sync_ms     host clock around the block with a synchronisation after every step, which is what a trainer that reads its losses
                  with .item() every iteration imposes

and (d) GB/s = 28 B x elements / device_ms.  Medians over the rounds with min and max; `spread_ms` of a comparison is the larger
(max - min) of the two versions: a difference of medians below it is reported as not resolved.  The three versions' results are compared
first (three steps from equal state).  Host times depend on the host CPU: they are this machine's.  Prints one JSON line and writes it
to --out.  Fails without a GPU: there is nothing to fall back to."""
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
GROUPS = (("positions", 3, 0.00016), ("density", 1, 0.05), ("rotation", 4, 0.001), ("scale", 3, 0.005), ("features_albedo", 3, 0.0025),
          ("features_specular", 45, 0.0025 / 20))   # configs/base_gs.yaml:138-152
EPS = 1e-15


def summary(ts):
    return {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--steps", type=int, default=50, help="steps per timed block")
    ap.add_argument("--device-steps", type=int, default=20, help="steps per device-time block (all queued behind the head start)")
    ap.add_argument("--sleep-ms", type=float, default=60.0, help="device-side head start of the host in the device-time blocks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_adam_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dense_adam.py needs a GPU (there is no CPU fallback)")
    opt_mod = importlib.import_module("3dgrut_amd.optimizers")
    abi = importlib.import_module("3dgrut_amd._abi")
    lib = abi.load_library()
    n = args.n
    gen = torch.Generator(device="cuda").manual_seed(1)
    params = [torch.nn.Parameter(torch.randn((n, w), generator=gen, device="cuda")) for _, w, _ in GROUPS]
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen, device="cuda")
    elements = sum(p.numel() for p in params)

    def groups_of(ps):
        return [{"params": [p], "name": name, "lr": lr} for p, (name, _, lr) in zip(ps, GROUPS)]

    # faster and different is not faster: three steps from equal state on copies
    copies = {k: [torch.nn.Parameter(p.detach().clone()) for p in params] for k in ("torch", "fused")}
    for ps in copies.values():
        for p, q in zip(ps, params):
            p.grad = q.grad
    pair = {"torch": torch.optim.Adam(groups_of(copies["torch"]), lr=0.0, eps=EPS, fused=True),
            "fused": opt_mod.FusedAdam(groups_of(copies["fused"]), lr=0.0, eps=EPS)}
    for _ in range(3):
        for o in pair.values():
            o.step()
    agree = {"param_max_abs_diff": max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(copies["torch"], copies["fused"])),
             "exp_avg_sq_max_abs_diff": max(float((pair["torch"].state[a]["exp_avg_sq"] - pair["fused"].state[b]["exp_avg_sq"]).abs().max())
                                            for a, b in zip(copies["torch"], copies["fused"]))}
    del copies, pair
    torch.cuda.empty_cache()

    torch_opt = torch.optim.Adam(groups_of(params), lr=0.0, eps=EPS, fused=True)
    fused_opt = opt_mod.FusedAdam(groups_of(params), lr=0.0, eps=EPS)
    moments = [(torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    sel = (abi.GrutAdamGroup * len(params))()
    for g, p, (m, v), (_, w, lr) in zip(sel, params, moments, GROUPS):
        g.param, g.grad, g.exp_avg, g.exp_avg_sq = p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr()
        g.row_width, g.lr, g.beta1, g.beta2, g.eps = w, lr, 0.9, 0.999, EPS
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def selective_step():
        abi.check(lib.grut_selective_adam_update(stream, sel, len(params), n, None, abi.VIS_NONE), "grut_selective_adam_update")

    fns = {"torch": torch_opt.step, "fused": fused_opt.step, "selective": selective_step}
    before = dict(opt_mod.stats)
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    assert opt_mod.stats["hip_steps"] == before["hip_steps"] + 5, "FusedAdam did not take the HIP path"

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(10_000_000)
    b.record()
    b.synchronize()
    sleep_cycles = int(10_000_000 * args.sleep_ms / a.elapsed_time(b))

    def device_ms(fn):
        torch.cuda._sleep(sleep_cycles)
        a.record()
        for _ in range(args.device_steps):
            fn()
        b.record()
        queued = not a.query()   # the block was queued before the head start ran out
        b.synchronize()
        return a.elapsed_time(b) / args.device_steps, queued

    def call_ms(fn, sync_every_step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
            if sync_every_step:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    times = {k: {"device_ms": [], "call_ms": [], "sync_ms": []} for k in fns}
    host_was_ahead = {k: True for k in fns}
    for _ in range(args.rounds):           # alternate the versions inside every round
        for k, fn in fns.items():
            ms, queued = device_ms(fn)
            host_was_ahead[k] &= queued
            times[k]["device_ms"].append(ms)
            times[k]["call_ms"].append(call_ms(fn, False))
            times[k]["sync_ms"].append(call_ms(fn, True))
    result = {"device": torch.cuda.get_device_name(0), "N": n, "elements": elements, "bytes_per_step": 28 * elements, "rounds": args.rounds,
              "steps_per_block": args.steps, "steps_per_device_block": args.device_steps, "sleep_ms": args.sleep_ms, "torch_version": torch.__version__, "agreement_after_3_steps_torch_vs_fused": agree,
              "host_ahead_in_every_device_block": host_was_ahead}
    for k in fns:
        result[k] = {key: summary(ts) for key, ts in times[k].items()}
        result[k]["GB/s"] = round(28 * elements / result[k]["device_ms"]["ms"] / 1e6, 1)
    result["fused_over_selective_device"] = round(result["fused"]["device_ms"]["ms"] / result["selective"]["device_ms"]["ms"], 4)
    result["kernel_within_15_percent_of_selective"] = result["fused_over_selective_device"] <= 1.15
    for key in ("device_ms", "call_ms", "sync_ms"):
        t, f = result["torch"][key], result["fused"][key]
        saved, spread = t["ms"] - f["ms"], max(t["max_ms"] - t["min_ms"], f["max_ms"] - f["min_ms"])
        result[f"torch_vs_fused_{key}"] = {"saved_ms": round(saved, 4), "spread_ms": round(spread, 4), "resolved": abs(saved) > spread}
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
