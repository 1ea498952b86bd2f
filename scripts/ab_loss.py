"""The loss entry points of two builds of the library against each other on one MI355X, in one process: bitwise identity of everything
they write, then their times, alternating.

    python scripts/ab_loss.py --parent-lib PATH [--rounds 15] [--window 0.2] [--out profiles/loss_refactor_ab.json]

"new" is the in-tree build (`_abi.load_library()`), "parent" the library at PATH (`_abi.load_library(PATH)`, built from another commit
with the same ABI).  Both are called through the C entry points directly, on the same seeded tensors and the same stream.

Identity (torch.equal, no tolerance: nothing in these kernels depends on an order that can vary).  Every output buffer is filled with a
sentinel before the call, so words that one build writes and the other does not differ too.
  grut_ssim_forward (training and inference) and grut_ssim_backward: mean, partials, the three planes, the gradient;
  grut_photo_loss_forward (training and inference) and _backward: out[3], partials, planes, gradient, for terms 4, 1|4 and 1|2|4,
  without a mask and with a binary one;
  on channels-last RGB at 1080p and 800x800 (the sizes that are timed), 2x3x37x45 channels-last, 2x1x37x45 planar, 1x2x64x33 and
  1x4x64x33 channels-last; padding "valid" and "same".

Time, at 1080p and 800x800 RGB channels-last, "valid": grut_ssim_forward training and inference, grut_ssim_backward, and
grut_photo_loss_forward / _backward for terms 1|4 with and without a mask.  Method of scripts/bench_photo_loss.py: both builds warmed up,
device events around as many calls as fill `--window` seconds, the two builds alternating inside every round; median and min / max over
the rounds.  `spread_ms` is the larger of the two builds' (max - min): a difference of the medians below it is not a difference, and
`not_slower` says that new - parent does not exceed it.  These are times of the bare entry points (no autograd, no allocation).

Prints one JSON line and writes it to --out.  Exit status 1 if any output differs, 2 if a case is slower beyond the spread.
Fails without a GPU: there is nothing to fall back to."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SENTINEL = 123.0
L1, L2, SSIM = 1, 2, 4
# name, B, C, H, W, channels-last memory
SHAPES = [("1080p", 1, 3, 1080, 1920, True), ("800x800", 1, 3, 800, 800, True), ("2x3x37x45", 2, 3, 37, 45, True),
          ("2x1x37x45-planar", 2, 1, 37, 45, False), ("1x2x64x33", 1, 2, 64, 33, True), ("1x4x64x33", 1, 4, 64, 33, True)]
TIMED = ("1080p", "800x800")


def _ptr(t):
    return C.c_void_p(None) if t is None else C.c_void_p(t.data_ptr())


def _strides(t):
    return None if t is None else (C.c_int64 * t.dim())(*t.stride())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def inputs(b, c, h, w, channels_last, seed):
    """img1, img2 as [B, C, H, W] views of the layout's own memory, a binary mask [B, H, W], upstream gradients."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = (b, h, w, c) if channels_last else (b, c, h, w)
    pred = torch.rand(shape, generator=g, device="cuda")
    gt = (pred + 0.02 * torch.randn(shape, generator=g, device="cuda")).clamp(0, 1)
    mask = (torch.rand((b, h, w), generator=g, device="cuda") < 0.8).float()
    if channels_last:
        pred, gt = pred.permute(0, 3, 1, 2), gt.permute(0, 3, 1, 2)
    return pred, gt, mask


def filled(shape):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), SENTINEL, dtype=torch.float32, device="cuda")


class Calls:
    """The six entry points of one library on one pair of images; every method returns what the call wrote."""

    def check(self, status, what):   # the message comes from the library that was called (_abi.check asks the in-tree one)
        if status != self.abi.GRUT_OK:
            msg = self.lib.grut_last_error()
            raise RuntimeError(f"{what} failed with {self.abi.STATUS_NAMES.get(status, status)}: {msg.decode() if msg else ''}")

    def __init__(self, abi, lib, img1, img2, valid):
        self.abi, self.lib, self.img1, self.img2, self.valid = abi, lib, img1, img2, valid
        self.dims = tuple(int(s) for s in img1.shape)
        self.head = lambda: (_stream(), *self.dims, _ptr(img1), _strides(img1), _ptr(img2), _strides(img2))

    def _planes(self, train):
        return filled((3, *self.dims)) if train else None

    @staticmethod
    def _plane_args(planes):
        return [_ptr(None if planes is None else planes[i]) for i in range(3)]

    def _grad(self):
        return torch.full_like(self.img1, SENTINEL)   # preserve_format: img1's own (dense) strides

    def ssim_forward(self, train, out=None):
        out = out or dict(mean=filled(()), partials=filled(int(self.lib.grut_ssim_partials(*self.dims))), planes=self._planes(train))
        self.check(self.lib.grut_ssim_forward(*self.head(), self.valid, _ptr(out["mean"]), _ptr(out["partials"]),
                                                  *self._plane_args(out["planes"])), "grut_ssim_forward")
        return out

    def ssim_backward(self, planes, grad_out, grad=None):
        grad = self._grad() if grad is None else grad
        self.check(self.lib.grut_ssim_backward(*self.head(), self.valid, _ptr(grad_out), *self._plane_args(planes), _ptr(grad),
                                                   _strides(grad)), "grut_ssim_backward")
        return dict(grad=grad)

    def photo_forward(self, mask, terms, train, out=None):
        out = out or dict(out=filled(3), partials=filled(int(self.lib.grut_photo_loss_partials(*self.dims))),
                          planes=self._planes(train and terms & SSIM))
        self.check(self.lib.grut_photo_loss_forward(*self.head(), _ptr(mask), _strides(mask), terms, self.valid, _ptr(out["out"]),
                                                        _ptr(out["partials"]), *self._plane_args(out["planes"])), "grut_photo_loss_forward")
        return out

    def photo_backward(self, mask, terms, planes, grad_out, grad=None):
        grad = self._grad() if grad is None else grad
        self.check(self.lib.grut_photo_loss_backward(*self.head(), _ptr(mask), _strides(mask), terms, self.valid, _ptr(grad_out),
                                                         *self._plane_args(planes), _ptr(grad), _strides(grad)), "grut_photo_loss_backward")
        return dict(grad=grad)


def differing(a, b):
    """Names of the buffers that are not bitwise equal between two results."""
    return [k for k in a if a[k] is not None and not torch.equal(a[k], b[k])]


def identity(abi, libs, result):
    g_ssim = torch.tensor([-0.2], device="cuda")
    g_photo = torch.tensor([0.8, 0.3, -0.2], device="cuda")
    cases, bad = 0, []
    for seed, (name, b, c, h, w, cl) in enumerate(SHAPES):
        img1, img2, mask = inputs(b, c, h, w, cl, seed)
        for valid in (1, 0):
            new, old = (Calls(abi, libs[k], img1, img2, valid) for k in ("new", "parent"))
            runs = {"ssim_forward_train": lambda s: s.ssim_forward(True), "ssim_forward_inference": lambda s: s.ssim_forward(False)}
            planes = new.ssim_forward(True)["planes"]
            runs["ssim_backward"] = lambda s: s.ssim_backward(planes, g_ssim)
            for terms in (SSIM, L1 | SSIM, L1 | L2 | SSIM):
                for m in (None, mask):
                    tag = f"photo_terms{terms}{'_mask' if m is not None else ''}"
                    runs[f"{tag}_forward_train"] = lambda s, m=m, terms=terms: s.photo_forward(m, terms, True)
                    runs[f"{tag}_forward_inference"] = lambda s, m=m, terms=terms: s.photo_forward(m, terms, False)
                    pl = new.photo_forward(m, terms, True)["planes"]
                    runs[f"{tag}_backward"] = lambda s, m=m, terms=terms, pl=pl: s.photo_backward(m, terms, pl, g_photo)
            for what, run in runs.items():
                diff = differing(run(new), run(old))
                cases += 1
                if diff:
                    bad.append(f"{name} valid={valid} {what}: {', '.join(diff)}")
    torch.cuda.synchronize()
    result["identity"] = {"cases": cases, "differing": len(bad), "differing_cases": bad}


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def times(abi, libs, args, result):
    g_ssim = torch.tensor([-0.2], device="cuda")
    g_photo = torch.tensor([0.8, 0.3, -0.2], device="cuda")
    terms = L1 | SSIM
    result["time"] = {}
    for seed, (name, b, c, h, w, cl) in enumerate(SHAPES):
        if name not in TIMED:
            continue
        img1, img2, mask = inputs(b, c, h, w, cl, seed)
        fns = {}   # case -> {build -> call}; every call reuses its build's own buffers
        for k in ("parent", "new"):
            s = Calls(abi, libs[k], img1, img2, 1)
            tr, inf, grad = s.ssim_forward(True), s.ssim_forward(False), s._grad()
            entry = {"ssim_forward_train": lambda s=s, tr=tr: s.ssim_forward(True, tr),
                     "ssim_forward_inference": lambda s=s, inf=inf: s.ssim_forward(False, inf),
                     "ssim_backward": lambda s=s, tr=tr, grad=grad: s.ssim_backward(tr["planes"], g_ssim, grad)}
            for m, tag in ((None, ""), (mask, "_mask")):
                ph = s.photo_forward(m, terms, True)
                entry[f"photo_forward{tag}"] = lambda s=s, m=m, ph=ph: s.photo_forward(m, terms, True, ph)
                entry[f"photo_backward{tag}"] = lambda s=s, m=m, ph=ph, grad=grad: s.photo_backward(m, terms, ph["planes"], g_photo, grad)
            for case, fn in entry.items():
                fns.setdefault(case, {})[k] = fn
        for case, pair in fns.items():
            for fn in pair.values():       # warm up both builds
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            inner = {k: max(20, int(args.window / (timed(fn, 10) * 1e-3))) for k, fn in pair.items()}   # enough calls to fill the window
            ts = {k: [] for k in pair}
            for _ in range(args.rounds):   # alternate the builds inside every round
                for k, fn in pair.items():
                    ts[k].append(timed(fn, inner[k]))
            e = {k: {"ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5), "calls_per_window": inner[k]}
                 for k, v in ts.items()}
            e["new_minus_parent_ms"] = round(e["new"]["ms"] - e["parent"]["ms"], 5)
            e["spread_ms"] = round(max(e[k]["max_ms"] - e[k]["min_ms"] for k in pair), 5)
            e["not_slower"] = e["new_minus_parent_ms"] <= e["spread_ms"]
            result["time"][f"{name} {case}"] = e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libgrut_amd.so built from the commit to compare against")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_refactor_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_loss.py needs a GPU (there is no CPU fallback)")
    abi = importlib.import_module("3dgrut_amd._abi")
    libs = {"new": abi.load_library(), "parent": abi.load_library(os.path.abspath(args.parent_lib))}
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window}
    identity(abi, libs, result)
    times(abi, libs, args, result)
    slower = [k for k, e in result["time"].items() if not e["not_slower"]]
    result["slower_beyond_spread"] = slower
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    sys.exit(1 if result["identity"]["differing"] else 2 if slower else 0)


if __name__ == "__main__":
    main()
