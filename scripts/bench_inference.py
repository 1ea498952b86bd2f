#!/usr/bin/env python
"""What render.forward_only_inference is for: a 3DGUT frame nobody differentiates (validation, rendering, viewers, visibility filters)
through the training forward - gut_forward: checkpoint stores in the sweep, boundary tiles, reached marks, the checkpoint tables - and
through the forward-only frame, gut_forward_only, which has none of them.

  workload   1 M Gaussians of workloads.synthetic at 1920x1080 (bench.py's c4_1m_1080p cloud and view), SH degree 3
  one frame  one call of the C entry point into preallocated outputs (the call waits for the frame's entry count itself); and, for the
             record, one Tracer.render under torch.no_grad() with the switch off and on
  timing     a host clock around a device synchronise; every mode in this process, in alternating blocks of --steps frames after a
             warm-up of all; per mode the median block and its (min - max)
  memory     gut_memory of a handle that has only rendered training frames and of one that has only rendered forward-only frames:
             bytes of {all scratch, the per-intersection lists, the checkpoint tables}
  parent     with --parent-lib PATH (libgrut_amd.so built from the parent commit) that library's gut_forward runs as a third mode in the
             same blocks; accepted = the forward-only frame is not slower than the parent's training forward by more than the parent's
             own block-to-block spread (without a parent library: than this library's training forward, by its spread).  A library
             loaded by path allocates its scratch with hipMalloc, the in-tree one through torch's allocator: GRUT_AMD_HIP_MALLOC=1
             puts both on hipMalloc (the two training forwards then differ by what the code differs, not by where the tables lie)

Without a ROCm GPU nothing is measured and every number reads "not measured".

    python scripts/bench_inference.py [--parent-lib PATH] [--steps 600] [--blocks 4] [--out profiles/inference_bench.json]
"""
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
abi = importlib.import_module("3dgrut_amd._abi")
gt = importlib.import_module("3dgrut_amd.gut_tracer")
syn = importlib.import_module("workloads.synthetic")
scenes = importlib.import_module("workloads.scenes")
camera = importlib.import_module("3dgrut_amd.camera")

N, W, H, MEDIAN_SCALE = 1_000_000, 1920, 1080, 0.01
PARENT_SYMBOLS = ("gut_create", "gut_destroy", "gut_forward", "gut_stats", "grut_last_error", "grut_abi_version")


def load_parent(path, new):
    """The parent commit's library next to this one: only the entry points both have, with this library's prototypes."""
    lib = C.CDLL(os.path.abspath(path))
    for name in PARENT_SYMBOLS:
        getattr(lib, name).argtypes, getattr(lib, name).restype = getattr(new, name).argtypes, getattr(new, name).restype
    assert lib.grut_abi_version() == abi.ABI_VERSION, "the parent library has another ABI version"
    return lib


class Handle:
    """One C handle of one library and the preallocated outputs of its frames."""

    def __init__(self, lib, cfg, dev):
        self.lib, self.handle = lib, C.c_void_p()
        assert lib.gut_create(C.byref(cfg), C.byref(self.handle)) == abi.GRUT_OK, lib.grut_last_error()
        f32 = dict(dtype=torch.float32, device=dev)
        self.out = [torch.empty((H, W, 4), **f32), torch.empty((H, W, 1), **f32), torch.empty((H, W, 1), **f32),
                    torch.empty((N, 1), dtype=torch.int32, device=dev)]

    def frame(self, entry, frame, inputs):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = getattr(self.lib, entry)(self.handle, stream, C.byref(frame), *[C.c_void_p(t.data_ptr()) for t in inputs + self.out])
        assert rc == abi.GRUT_OK, (entry, self.lib.grut_last_error())

    def close(self):
        self.lib.gut_destroy(self.handle)


def summary(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libgrut_amd.so built from the parent commit: its gut_forward is timed in the same blocks")
    ap.add_argument("--steps", type=int, default=600, help="frames per block (a block should last well over a second)")
    ap.add_argument("--blocks", type=int, default=4, help="timed blocks per mode")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inference_bench.json"))
    args = ap.parse_args()
    result = {"workload": f"{N} Gaussians, {W}x{H}, SH degree 3, one frame without a backward",
              "steps_per_block": args.steps, "blocks_per_mode": args.blocks, "parent_library": bool(args.parent_lib)}
    if not torch.cuda.is_available():
        result.update(frame_ms="not measured", memory_bytes="not measured", accepted="not measured")
        json.dump(result, open(args.out, "w"), indent=1)
        print(json.dumps(result))
        return
    dev = "cuda"
    result["device"] = torch.cuda.get_device_name(0)
    d12, sph = syn.cloud_trained_like(N, seed=42, median_scale=MEDIAN_SCALE)
    K = syn.pinhole_intrinsics(W, H)
    ro, rd = syn.pinhole_rays(W, H, K)
    batch = dict(rays_ori=ro, rays_dir=rd, T_to_world=syn.orbit_pose(0, n_views=8)[None], intrinsics=K)
    cam, pose_start, pose_end = camera.camera_from_batch(batch)
    cfg = gt.gut_config_from_conf({"render": {"splat": {}}})
    t = lambda a: torch.as_tensor(a, device=dev).contiguous()
    inputs = [t(d12), t(sph), t(ro[0]), t(rd[0])]
    new = abi.load_library()
    modes = {"training": (Handle(new, cfg, dev), "gut_forward"), "forward_only": (Handle(new, cfg, dev), "gut_forward_only")}
    if args.parent_lib:
        modes["parent_training"] = (Handle(load_parent(args.parent_lib, new), cfg, dev), "gut_forward")
    frame = gt._GutNative.make_frame(None, 0, 3, N, H, W, cam, pose_start, pose_end)

    def block(mode, steps):
        handle, entry = modes[mode]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            handle.frame(entry, frame, inputs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for mode in modes:   # warm-up of all (allocations, speculation capacity)
        block(mode, 30)
    ref = modes["training"][0].out
    result["outputs_bit_identical"] = {m: all(torch.equal(a, b) for a, b in zip(h.out, ref)) for m, (h, _) in modes.items() if m != "training"}
    stats = abi.GutStats()
    abi.check(new.gut_stats(modes["forward_only"][0].handle, C.byref(stats)), "gut_stats")
    result["tile_entries"] = int(stats.num_intersections)
    times = {m: [] for m in modes}
    for _ in range(args.blocks):
        for mode in modes:
            times[mode].append(block(mode, args.steps))
    memory = {}
    for mode in ("training", "forward_only"):
        out = (C.c_uint64 * 3)()
        abi.check(new.gut_memory(modes[mode][0].handle, out), "gut_memory")
        memory[mode] = dict(zip(("total", "lists", "checkpoint_tables"), (int(v) for v in out)))
    for handle, _ in modes.values():
        handle.close()

    # the plugin: Tracer.render under no_grad with the switch off and on (what a validation loop or a viewer calls)
    model = syn.SimpleGaussians(d12, sph, device=dev, requires_grad=False)
    tbatch = scenes.torch_batch(batch, dev)
    tracers = {"switch_off": gt.Tracer({"render": {"splat": {}, "forward_only_inference": False}}),
               "switch_on": gt.Tracer({"render": {"splat": {}, "forward_only_inference": True}})}

    def render_block(mode, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for _ in range(steps):
                tracers[mode].render(model, tbatch)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    render_times = {m: [] for m in tracers}
    for mode in tracers:
        render_block(mode, 30)
    for _ in range(args.blocks):
        for mode in tracers:
            render_times[mode].append(render_block(mode, args.steps))

    against = "parent_training" if args.parent_lib else "training"
    margin = max(times[against]) - min(times[against])
    fo, base = statistics.median(times["forward_only"]), statistics.median(times[against])
    result.update(
        frame_ms={m: summary(v) for m, v in times.items()}, block_frame_ms={m: [round(x, 4) for x in v] for m, v in times.items()},
        plugin_render_ms={m: summary(v) for m, v in render_times.items()},
        plugin_paths={m: dict(tr.stats_forward_only) for m, tr in tracers.items()},
        memory_bytes=memory, checkpoint_bytes_saved=memory["training"]["checkpoint_tables"] - memory["forward_only"]["checkpoint_tables"],
        compared_against=against, margin_ms=round(margin, 4), gain_ms=round(base - fo, 4), gain_percent=round(100.0 * (base - fo) / base, 2),
        accepted=bool(fo - base <= margin))
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
