"""What `host_ahead_in_every_device_block: false` of bench_dense_adam.py means for torch.optim.Adam(fused=True):

    python scripts/probe_dense_adam_queue.py [--n 1000000] [--steps 20] [--out profiles/dense_adam_queue_probe.json]

bench_dense_adam.py queues a block of steps behind a device-side sleep and asks afterwards whether the sleep is still running.  This
probe queues the same block (the six groups of configs/base_gs.yaml, torch's fused Adam and FusedAdam) behind a sleep of 60 and of
200 ms and records, after EVERY step(), the host clock since the block began and whether the event behind the sleep has completed.
A host that falls behind the device shows a steady host clock above the device's time per step; a runtime that holds the host back
once a bounded number of launches is outstanding shows one jump of about the sleep's length at the same step whatever the sleep, with
a fast clock before and after it - then the device has a backlog when the sleep ends and never waits for the host, and the block's
events measure device time.  Prints one JSON line and writes it to --out.  Needs a GPU."""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GROUPS = ((3, 0.00016), (1, 0.05), (4, 0.001), (3, 0.005), (3, 0.0025), (45, 0.0025 / 20))   # configs/base_gs.yaml:138-152


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_adam_queue_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_dense_adam_queue.py needs a GPU")
    opt_mod = importlib.import_module("3dgrut_amd.optimizers")
    params = [torch.nn.Parameter(torch.randn((args.n, w), device="cuda")) for w, _ in GROUPS]
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda")

    def groups():
        return [{"params": [p], "lr": lr} for p, (_, lr) in zip(params, GROUPS)]

    opts = {"torch": torch.optim.Adam(groups(), lr=0.0, eps=1e-15, fused=True), "fused": opt_mod.FusedAdam(groups(), lr=0.0, eps=1e-15)}
    for o in opts.values():
        for _ in range(5):
            o.step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(10_000_000)
    b.record()
    b.synchronize()
    cycles_per_ms = 10_000_000 / a.elapsed_time(b)
    out = {"device": torch.cuda.get_device_name(0), "N": args.n, "steps": args.steps, "torch_version": torch.__version__, "blocks": {}}
    for sleep_ms in (60, 200):
        for name, o in opts.items():
            for rep in range(2):
                torch.cuda.synchronize()
                s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                s0.record()
                torch.cuda._sleep(int(cycles_per_ms * sleep_ms))
                a.record()
                s1.record()
                host, done = [], []
                for _ in range(args.steps):
                    o.step()
                    host.append(round((time.perf_counter() - t0) * 1e3, 3))
                    done.append(bool(a.query()))
                b.record()
                b.synchronize()
                out["blocks"][f"{name}_sleep{sleep_ms}_rep{rep}"] = {
                    "sleep_measured_ms": round(s0.elapsed_time(s1), 3), "device_ms_per_step": round(a.elapsed_time(b) / args.steps, 4),
                    "host_ms_after_each_step": host, "sleep_over_after_each_step": done}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
