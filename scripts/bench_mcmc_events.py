#!/usr/bin/env python
"""The MCMC strategy's two periodic events at 1 M Gaussians, SH degree 3, Adam moments present: plain torch (the restatement of the
reference's relocate_gaussians / add_new_gaussians by indexing and cat, tests/mcmc_events_reference.py, with this library's relocation
kernel behind compute_relocation_tensor, as the reference has it) against the fused passes (3dgrut_amd.mcmc.relocate / add).

The restatement is the tests' own (imported from the tests/ directory of this checkout): the script needs the whole repository tree.

  relocate event   5 % of the Gaussians dead: wall-clock ms of the whole call, synchronised (the host reads inside are part of it)
  add event        5 % more Gaussians: the same
  both             torch.cuda.max_memory_allocated() over the event, minus what was allocated when it began
  append pass      the one launch of the add event alone (device time between two events) and its bytes moved per second

The two paths alternate event by event from fresh copies of one model; medians over --events timed events after two warm-up ones.

    python scripts/bench_mcmc_events.py [--n 1000000] [--events 20] [--out profiles/mcmc_events_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
mcmc = importlib.import_module("3dgrut_amd.mcmc")
import mcmc_events_reference as restated  # noqa: E402

THRESHOLD, N_MAX = 0.005, 51


def make_model(base):
    m = restated.DuckModel(1, "cuda")
    groups = []
    for name, _ in restated.DuckModel.NAMES:
        p = torch.nn.Parameter(base[name].clone())
        setattr(m, name, p)
        groups.append({"params": [p], "name": name, "lr": 1e-3})
    m.optimizer = torch.optim.Adam(groups, lr=1e-3, eps=1e-15)
    for name, _ in restated.DuckModel.NAMES:
        p = getattr(m, name)
        m.optimizer.state[p] = {"step": torch.tensor(7.0), "exp_avg": base[name + ".m"].clone(), "exp_avg_sq": base[name + ".v"].clone()}
    return m


def run_event(base, event):
    """One event on a fresh model: (wall ms, extra peak MiB, result of the event)."""
    model = make_model(base)
    torch.manual_seed(1)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = event(model)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    peak = (torch.cuda.max_memory_allocated() - before) / 2 ** 20
    n_after = model.num_gaussians
    del model
    return wall, peak, out, n_after


def summary(walls, peaks):
    return {"event_ms_median": round(statistics.median(walls), 3), "event_ms_min": round(min(walls), 3), "event_ms_max": round(max(walls), 3),
            "event_peak_extra_MiB": round(max(peaks), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--events", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.n
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g)   # noqa: E731
    base = {"positions": rnd(n, 3), "rotation": rnd(n, 4), "scale": rnd(n, 3) * 0.8 - 4.6,      # exp: log-normal around 0.01
            "density": rnd(n, 1).clamp(-2.5, 2.5) + 0.5, "features_albedo": rnd(n, 3), "features_specular": rnd(n, restated.SH_ROW) * 0.1}
    base["density"][torch.randperm(n, device="cuda", generator=g)[: n // 20]] = -7.0          # 5 % dead: sigmoid(-7) = 9e-4
    for name, _ in restated.DuckModel.NAMES:
        base[name + ".m"], base[name + ".v"] = rnd(*base[name].shape) * 1e-3, rnd(*base[name].shape).abs() * 1e-6
    binoms = restated.binomial_table(N_MAX, "cuda")

    def torch_events(model):
        return restated.RestatedMCMCEvents(model, threshold=THRESHOLD, n_max=N_MAX, relocation=mcmc.compute_relocation_tensor, binoms=binoms)

    events = {
        "relocate": {"torch": lambda m: torch_events(m).relocate()["n_dead"], "fused": lambda m: mcmc.relocate(m, THRESHOLD, binoms, N_MAX).n_dead},
        "add": {"torch": lambda m: torch_events(m).add()["n_added"], "fused": lambda m: mcmc.add(m, 10 ** 9, THRESHOLD, binoms, N_MAX).n_added},
    }
    res = {"device": torch.cuda.get_device_name(0), "n": n, "events": args.events,
           "model_and_state_MiB": round(sum(v.numel() * 4 for v in base.values()) / 2 ** 20, 1)}
    hip_before = (mcmc.stats.hip_relocations, mcmc.stats.hip_adds, mcmc.stats.torch_events)
    for kind, paths in events.items():
        walls, peaks, counts = {k: [] for k in paths}, {k: [] for k in paths}, {}
        for it in range(args.events + 2):                                      # two warm-up events (allocator pool, first launches)
            for label, event in paths.items():                                  # alternating: both paths see the same machine state
                wall, peak, count, n_after = run_event(base, event)
                counts[label] = (count, n_after)
                if it >= 2:
                    walls[label].append(wall)
                    peaks[label].append(peak)
        assert counts["torch"] == counts["fused"], counts
        res[kind] = {label: summary(walls[label], peaks[label]) for label in paths}
        res[kind]["rows"], res[kind]["gaussians_after"] = counts["fused"]
        res[kind]["speedup"] = round(res[kind]["torch"]["event_ms_median"] / res[kind]["fused"]["event_ms_median"], 2)
    ran = args.events + 2
    assert (mcmc.stats.hip_relocations, mcmc.stats.hip_adds, mcmc.stats.torch_events) == (hip_before[0] + ran, hip_before[1] + ran, hip_before[2])

    # the append pass alone: every parameter and moment of the model, one launch
    model = make_model(base)
    found = mcmc._event_tensors(model)
    _, _, tensors, roles = found
    m = int(1.05 * n) - n
    density_act = model.get_density().detach()
    sampled = torch.multinomial(density_act.flatten(), m, replacement=True)
    plan = mcmc.sample_plan(sampled, density_act, model.scale.data, binoms, N_MAX, THRESHOLD)
    moved = 0
    for t, role in zip(tensors, roles):
        w = t.numel() // n
        moved += 4 * w * (n + (n + m) + (m if role == mcmc.ROLE_COPY else 0))      # read the old rows (and the gathered ones), write the new tensor
    times = []
    for it in range(args.events + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        outs = mcmc.append_rows(tensors, roles, plan)
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            times.append(e0.elapsed_time(e1))
        del outs
    ms = statistics.median(times)
    res["append_pass"] = {"tensors": len(tensors), "ms_median": round(ms, 4), "ms_min": round(min(times), 4), "bytes_moved": moved,
                          "GB_per_s": round(moved / (ms * 1e-3) / 1e9, 1)}
    line = json.dumps({"mcmc_events": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
