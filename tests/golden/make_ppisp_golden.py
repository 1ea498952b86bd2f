"""Regenerates tests/golden/ppisp.npz from the reference checkout:

    python tests/golden/make_ppisp_golden.py [--reference /path/to/reference]

The reference states the PPISP forward model in fp32 in threedgrut/export/usd/post_processing/ppisp_spg/ppisp_usd_spg.cu
(`applyPPISPColor`), a file its own tests hold against the torch module.  This script compiles that function for the HOST, unchanged and
by path, behind the few declarations below that a C++ compiler needs to read a CUDA source, into a temporary directory, and evaluates it
on the suite's inputs.  Nothing compiled and no line of the reference is kept: the .npz holds, per case, the input image, the four
parameter rows, the reference's fp32 output and e_ref = max |ref32 - restatement64| (tests/ppisp_reference.py).

Cases: every shape of ppisp_reference.SHAPES x (two random parameter draws + the identity parameters).  The image of a shape is stored
once and shared by its three cases.  Image seeds: the first seed from 100 H + W on whose image meets the suite's condition on its own inputs in
every configuration the GPU tests run (ppisp_reference.CONFIGS: all four parameter groups, each one missing in turn) with each of the three
parameter sets: at most 5 % of the pixels within the margin of a kink of the response curve, as the float64 and fp32 restatements see it.
At 7 x 9 that is at most 3 pixels, which not every draw of 63 pixels manages.
"""
import argparse
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ppisp_reference as R  # noqa: E402

SOURCE = "threedgrut/export/usd/post_processing/ppisp_spg/ppisp_usd_spg.cu"
PARAMETER_SEEDS = (23, 41)
HOST_SHIM = r'''
#include <algorithm>
#include <cmath>
#define __device__
#define __global__
#define __forceinline__ inline
#define __restrict__
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct uchar4 { unsigned char x, y, z, w; };
struct dim3_ { int x, y, z; };
static dim3_ blockIdx, blockDim, threadIdx;
typedef unsigned long long cudaTextureObject_t;
typedef unsigned long long cudaSurfaceObject_t;
template <class T> static T tex2D(cudaTextureObject_t, int, int) { return T(); }
template <class T> static void surf2Dwrite(T, cudaSurfaceObject_t, int, int) {}
using std::max;
using std::min;
#include PPISP_SOURCE
extern "C" void ppisp_reference_forward(int n, const float* rgb, const float* uv, const float* exposure, const float* color,
                                        const float* vig, const float* crf, float* out) {
    for (int i = 0; i < n; ++i) {
        float3 in = {rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]};
        float2 p = {uv[2 * i], uv[2 * i + 1]};
        float2 cr = {vig[0], vig[1]}, cg = {vig[5], vig[6]}, cb = {vig[10], vig[11]};
        float2 lb = {color[0], color[1]}, lr = {color[2], color[3]}, lg = {color[4], color[5]}, ln = {color[6], color[7]};
        float3 o = applyPPISPColor(in, p, 1.0f, exposure[0], cr, vig[2], vig[3], vig[4], cg, vig[7], vig[8], vig[9], cb, vig[12], vig[13],
                                   vig[14], lb, lr, lg, ln, crf[0], crf[1], crf[2], crf[3], crf[4], crf[5], crf[6], crf[7], crf[8], crf[9],
                                   crf[10], crf[11]);
        out[3 * i] = o.x, out[3 * i + 1] = o.y, out[3 * i + 2] = o.z;
    }
}
'''


def build_reference(reference, workdir):
    src = os.path.join(reference, SOURCE)
    if not os.path.exists(src):
        raise SystemExit(f"{src} not found: the golden file can only be regenerated next to the reference checkout")
    shim, lib = os.path.join(workdir, "ppisp_host.cpp"), os.path.join(workdir, "ppisp_host.so")
    with open(shim, "w") as f:
        f.write(HOST_SHIM)
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", f'-DPPISP_SOURCE="{src}"', shim, "-o", lib])
    return ctypes.CDLL(lib)


def image_for(h, w, parameter_sets):
    for seed in range(100 * h + w, 100 * h + w + 100):
        img = R.make_image(h, w, seed)
        case = dict(rgb=img, pc=R.pixel_coords(h, w), h=h, w=w)
        if all(1 - float(R.kink_free({**case, **par}, groups).float().mean()) <= R.MAX_LEFT_OUT for _, par in parameter_sets for groups in R.CONFIGS):
            return seed, img
    raise SystemExit(f"no image seed meets the condition at {h} x {w}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GRUT_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(HERE, "ppisp.npz"))
    args = ap.parse_args()
    arrays, names = {}, []
    parameter_sets = [(f"s{s}", R.random_parameters(s)) for s in PARAMETER_SEEDS] + [("identity", R.identity_parameters())]
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_reference(args.reference, tmp)
        for h, w in R.SHAPES:
            seed, img = image_for(h, w, parameter_sets)
            arrays[f"{h}x{w}/rgb"] = np.ascontiguousarray(img.numpy())
            arrays[f"{h}x{w}/image_seed"] = np.int64(seed)
            pc = R.pixel_coords(h, w)
            uv = ((pc.numpy() - np.array([w / 2, h / 2], dtype=np.float32)) / np.float32(max(w, h))).astype(np.float32)
            for tag, par in parameter_sets:
                name = f"{h}x{w}_{tag}"
                rgb = np.ascontiguousarray(img.numpy())
                p = {k: np.ascontiguousarray(v.numpy(), dtype=np.float32) for k, v in par.items()}
                ref32 = np.empty_like(rgb)
                lib.ppisp_reference_forward(h * w, ptr(rgb), ptr(np.ascontiguousarray(uv)), ptr(p["exposure"]), ptr(p["color"]), ptr(p["vignetting"]),
                                            ptr(p["crf"]), ptr(ref32))
                r64 = R.ppisp_model(img, pc, (w, h), par["exposure"], par["color"], par["vignetting"], par["crf"]).numpy()
                e_ref = float(np.abs(ref32.astype(np.float64) - r64).max())
                names.append(name)
                arrays[f"{name}/ref32"], arrays[f"{name}/e_ref"] = ref32, np.float64(e_ref)
                for k, v in p.items():
                    arrays[f"{name}/{k}"] = v
                print(f"{name}: image seed {seed}, e_ref {e_ref:.3e}, samples exactly 0: {int((img == 0).sum())}, samples >= 1: {int((img >= 1).sum())}")
    np.savez_compressed(args.out, names=np.array(names), **arrays)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {len(names)} cases")


if __name__ == "__main__":
    main()
