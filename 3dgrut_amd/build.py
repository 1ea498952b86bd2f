"""In-tree build of libgrut_amd.so with hipcc for gfx950 (cross-compiles without a GPU).

    python 3dgrut_amd/build.py [--force] [--verbose]
    python 3dgrut_amd/build.py --variant NAME FILE.hip [flags...]

One object per .hip file, rebuilt only when its sources are newer; linked into csrc/libgrut_amd.so,
which travels to the GPU box with the repository snapshot.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(CSRC, "libgrut_amd.so")
SOURCES = ["scan_sort.hip", "gut_kernels.hip", "gut_poses.hip", "gut_render.hip", "gut_render_k.hip", "gut_api.hip", "grt_kernels.hip", "grt_api.hip", "optim.hip", "mcmc.hip", "mcmc_events.hip", "loss.hip", "densify.hip", "knn.hip", "ppisp.hip", "ppisp_controller.hip", "mlp.hip", "mlp_backward.hip", "regularizers.hip", "denoise.hip"]
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-munsafe-fp-atomics", "-ffp-contract=fast",
         # SLP-packing scalar f32 math into v_pk_*_f32 costs register-pair shuffles (v_mov) and VGPRs on gfx950
         "-fno-slp-vectorize",
         "-Wall", "-Wno-unused-function", "-Wno-unused-variable"]
# per-file additions.  grt_kernels.hip evaluates hit distances under `#pragma clang fp contract(off)` so that the per-ray
# hit ORDER is reproducible bit for bit by the CPU checker; the pragma is only honoured when the command-line mode is
# `on` (with `fast` the backend fuses regardless), so that file is built with -ffp-contract=on.
# gut_poses.hip derives the frame's poses the way the reference's HOST code does (numpy / torch / host C++: nothing contracts there).
# gut_render.hip (the compositing sweeps: fp32 VALU issue while their waves run, latency in the launch's ramp-down): the backend's max-ILP
# scheduling strategy instead of the default occupancy-first one - the kernels' occupancy is pinned by amdgpu_waves_per_eu anyway.  Same
# instructions in another order: gradient sweep 0.807 -> 0.792 ms, forward 0.449 -> 0.443 ms, step -1.1 % (A/B on one box, interleaved:
# scripts/ab_sched_variants.sh, profiles/r06_sched_strategy_ab.txt).  Measured and NOT applied: gut_kernels.hip (the gradient gather loses
# 12 us), grt_kernels.hip (trace forward -0.1 ms, replay backward +0.03: one file), max-memory-clause (slower everywhere).
# The sorted hit buffer's kernels with SH radiance LOSE with it (K = 16 frame 10.87 -> 11.32 ms, 4 %) where the unsorted sweeps gain 1-2 % and
# the feature sweeps 2.5 %: that is why they are a source of their own, gut_render_k.hip, built with the default strategy; what the two share
# is gut_render_common.inl.
# knn.hip reports distances recomputed in double that must round like the host's float64 arithmetic (no fused multiply-add there).
FILE_FLAGS = {"grt_kernels.hip": ["-ffp-contract=on"], "gut_poses.hip": ["-ffp-contract=off"], "knn.hip": ["-ffp-contract=off"],
              "gut_render.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]}


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    raise RuntimeError("hipcc not found")


def _deps():
    """What every object depends on besides its own source: the headers, and this file (the flags)."""
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".h", ".inl"))] + \
           [os.path.join(HERE, "..", "include", "grut_amd.h"), os.path.abspath(__file__)]


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _object(src: str) -> str:
    return os.path.join(CSRC, src.replace(".hip", ".o"))


def compile_command(src: str, extra=(), out=None):
    """The full compile argv of one source of SOURCES: the build's, the resource scripts' and the variants'."""
    return [_hipcc(), "-x", "hip", *FLAGS, *FILE_FLAGS.get(src, []), *extra, "-c", os.path.join(CSRC, src), "-o", out or _object(src)]


def _run(cmd, verbose=False):
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    if verbose and r.stderr:
        print(r.stderr)


def _link(objs, out, verbose=False):
    _run([_hipcc(), "-shared", "-fPIC", f"--offload-arch={ARCH}", *objs, "-o", out], verbose)


def build(force: bool = False, verbose: bool = False, extra_flags=()) -> str:
    deps = _deps()
    objs = [_object(src) for src in SOURCES]
    jobs = [compile_command(src, extra_flags) for src, obj in zip(SOURCES, objs) if force or _stale(obj, [os.path.join(CSRC, src)] + deps)]
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(lambda cmd: _run(cmd, verbose), jobs))
    if force or jobs or _stale(OUT, objs):
        _link(objs, OUT, verbose)
    return OUT


def variant(name: str, src: str, extra_flags=(), verbose: bool = False) -> str:
    """One source compiled with extra flags (a tuning switch: -DGRT_FWD_WAVES=3; a build-time diagnostic: -DGRT_ONLY_DEGREE_4) and linked with
    the in-tree objects of every other source into variants/libgrut_amd_NAME.so, which GRUT_AMD_LIB selects at load time."""
    if src not in SOURCES:
        raise ValueError(f"{src} is not one of {SOURCES}")
    build(verbose=verbose)
    vdir = os.path.join(HERE, "..", "variants")
    os.makedirs(vdir, exist_ok=True)
    obj = os.path.join(vdir, f"{src[:-4]}_{name}.o")
    _run(compile_command(src, extra_flags, out=obj), verbose)
    out = os.path.abspath(os.path.join(vdir, f"libgrut_amd_{name}.so"))
    _link([obj if s_ == src else _object(s_) for s_ in SOURCES], out, verbose)
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--verbose"]
    if args[:1] == ["--variant"]:
        print(variant(args[1], args[2], args[3:], verbose="--verbose" in sys.argv))
    else:
        print(build(force="--force" in args, verbose="--verbose" in sys.argv))
