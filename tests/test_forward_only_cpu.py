"""CPU: the forward-only surface of 3DGUT (render.forward_only_inference; gut_forward_only / gut_forward_only_split / gut_memory).
The three C entry points are declared, exported and mirrored in ctypes with their twins' argument lists and the ABI version stays;
the switch reads its key and its environment variable; and, with a recording fake in place of the C handle (the kind
tests/test_reference_seam_cpu.py uses) and of the two packing kernels, Tracer.render picks the forward-only entry point exactly for
the frames that cannot be differentiated - as a plain call, with no autograd node - and today's path for every other frame."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
abi = importlib.import_module("3dgrut_amd._abi")
gt = importlib.import_module("3dgrut_amd.gut_tracer")
syn = importlib.import_module("workloads.synthetic")
scenes = importlib.import_module("workloads.scenes")
NEW_ENTRY_POINTS = ("gut_forward_only", "gut_forward_only_split", "gut_memory")
N, W, H = 20, 16, 12


def _header_prototype(header, name):
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/grut_amd.h"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def _types(args):
    """The argument types of a prototype: the parameter names dropped."""
    return [re.sub(r"\s*\b\w+(\[\d*\])?$", "", a) for a in args]


def test_entry_points_are_declared_exported_and_mirrored(grut_lib, tmp_path):
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(grut_lib, name), f"{name} missing from libgrut_amd.so"
        assert len(getattr(grut_lib, name).argtypes) == len(_header_prototype(header, name)), name
    # argument lists match the twins', type by type, in the header and in the ctypes mirror
    for name, twin in (("gut_forward_only", "gut_forward"), ("gut_forward_only_split", "gut_forward_split")):
        assert _types(_header_prototype(header, name)) == _types(_header_prototype(header, twin)), name
        assert list(getattr(grut_lib, name).argtypes) == list(getattr(grut_lib, twin).argtypes), name
        assert getattr(grut_lib, name).restype is getattr(grut_lib, twin).restype
    # the C compiler's view of the three prototypes: typed function pointers must accept them as they are
    f = "const float*"
    src = tmp_path / "forward_only.c"
    src.write_text(
        '#include "grut_amd.h"\n'
        f"int (*a)(GutHandle*, void*, const GutFrame*, {f}, const void*, {f}, {f}, void*, float*, float*, int32_t*) = gut_forward_only;\n"
        f"int (*b)(GutHandle*, void*, const GutFrame*, {f}, {f}, {f}, {f}, {f}, void*, float*, float*, int32_t*) = gut_forward_only_split;\n"
        "int (*c)(GutHandle*, uint64_t*) = gut_memory;\n"
        "int main(void) { return a && b && c ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "forward_only.o")])
    # additive: the version stays
    assert abi.ABI_VERSION == 5 and grut_lib.grut_abi_version() == 5
    common = open(os.path.join(ROOT, "3dgrut_amd", "csrc", "common.hpp")).read()
    assert re.search(r"#define\s+GRUT_ABI_VERSION\s+5\b", common)


def test_null_handles_are_refused_on_the_host(grut_lib):
    """gut_memory is a host function and the forwards check their handle before anything else: both can be called without a GPU."""
    out = (ctypes.c_uint64 * 3)(7, 7, 7)
    assert grut_lib.gut_memory(None, out) == -1 and b"gut_memory" in grut_lib.grut_last_error()
    assert list(out) == [7, 7, 7]
    assert grut_lib.gut_forward_only(None, None, None, None, None, None, None, None, None, None, None) == -1
    assert grut_lib.gut_forward_only_split(None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"gut_forward_only_split" in grut_lib.grut_last_error()


def test_forward_only_requested_reads_the_key_and_the_environment(monkeypatch):
    monkeypatch.delenv("GRUT_FORWARD_ONLY", raising=False)
    assert not gt.forward_only_requested({"render": {}})
    assert not gt.forward_only_requested({"render": {"forward_only_inference": False}})
    assert not gt.forward_only_requested(None)
    assert gt.forward_only_requested({"render": {"forward_only_inference": True}})
    monkeypatch.setenv("GRUT_FORWARD_ONLY", "1")
    assert gt.forward_only_requested({"render": {}})


# ---- the selection logic against a fake native ---------------------------------------------------------------------------------

class _Recorder:
    """Stands in for the C handle: records which entry point a render() reaches and returns tensors of the contract's shapes."""

    def __init__(self, cfg):
        self.cfg, self.calls = cfg, []
        self.ncoef = (cfg.particle_radiance_sph_degree + 1) ** 2

    def make_frame(self, *a):
        return _REAL_NATIVE.make_frame(self, *a)   # the product's own marshalling (pure ctypes)

    def collect_times(self):
        return {}

    def _forward(self, name, frame, pd, sph):
        H_, W_, n = frame.height, frame.width, frame.num_particles
        assert pd.shape == (n, 12) and pd.dtype == torch.float32 and pd.is_contiguous() and not pd.requires_grad
        assert sum(t.shape[1] for t in sph) == 3 * self.ncoef and all(t.shape[0] == n and t.is_contiguous() for t in sph)
        self.calls.append(name)
        fd = torch.rand((H_, W_, 4))
        return fd, torch.rand((H_, W_, 1)), torch.zeros((H_, W_, 1)), torch.ones((n, 1)), fd[..., :3].contiguous(), fd[..., 3:].contiguous()

    def trace(self, frame, pd, sph, ro, rd):
        return self._forward("trace", frame, pd, (sph,))

    def trace_split(self, frame, pd, albedo, specular, ro, rd):
        return self._forward("trace_split", frame, pd, (albedo, specular))

    def trace_forward_only(self, frame, pd, sph, ro, rd):
        assert not torch.is_grad_enabled()
        return self._forward("trace_forward_only", frame, pd, (sph,))

    def trace_split_forward_only(self, frame, pd, albedo, specular, ro, rd):
        assert not torch.is_grad_enabled()
        return self._forward("trace_split_forward_only", frame, pd, (albedo, specular))


_REAL_NATIVE = gt._GutNative


class _CountingGaussians(syn.ActivatedGaussians):
    feature_calls = 0

    def get_features(self):
        self.feature_calls += 1
        return super().get_features()


@pytest.fixture()
def fake(monkeypatch):
    """(make_tracer, packs): Tracer over the recorder, the two packing kernels replaced by torch.cat twins that record their names."""
    packs = []

    def pack(name):
        def f(pos, dns, rot, scl):
            packs.append(name)
            return torch.cat([t.detach().reshape(pos.shape[0], -1) for t in (pos, dns, rot, scl)] + [torch.zeros((pos.shape[0], 1))], dim=1)
        return f
    monkeypatch.delenv("GRUT_FORWARD_ONLY", raising=False)
    monkeypatch.delenv("GRUT_SPLIT_SH", raising=False)
    monkeypatch.delenv("GRUT_FUSED_ACTIVATIONS", raising=False)
    monkeypatch.setattr(gt, "_GutNative", _Recorder)
    monkeypatch.setattr(abi, "pack_particles", pack("pack_particles"))
    monkeypatch.setattr(abi, "activate_pack", pack("activate_pack"))
    return (lambda **render: gt.Tracer({"render": dict(render, splat={})})), packs


def _model_and_batch(requires_grad=True):
    s = scenes.make_scene(n=N, width=W, height=H)
    model = _CountingGaussians(s["density12"], s["sph"], device="cpu")
    if not requires_grad:
        for p in model.parameters():
            p.requires_grad_(False)
    return model, scenes.torch_batch(s["batch"], "cpu")


CASES = {
    # name: (switch, grad mode, which leaves require grad, forward-only expected)
    "switch_off": (False, True, "all", False),
    "switch_off_no_grad": (False, False, "all", False),
    "on_grad_and_leaves": (True, True, "all", False),
    "on_grad_one_sh_leaf": (True, True, "specular", False),
    "on_grad_one_raw_leaf": (True, True, "scale", False),
    "on_no_grad": (True, False, "all", True),
    "on_grad_nothing_requires_grad": (True, True, "none", True),
}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_render_selects_the_entry_point(fake, case, split, fused):
    make_tracer, packs = fake
    switch, grad_mode, leaves, expect_forward_only = CASES[case]
    model, batch = _model_and_batch(requires_grad=leaves == "all")
    if leaves == "specular":
        model.features_specular.requires_grad_(True)
    elif leaves == "scale":
        model.scale.requires_grad_(True)
    tr = make_tracer(forward_only_inference=switch, split_sh_features=split, fused_activations=fused)
    assert tr._forward_only is switch
    with torch.set_grad_enabled(grad_mode):
        out = tr.render(model, batch, train=True, frame_id=4)   # (`train` decides nothing: the reference's 3DGUT ignores it)
    name = ("trace_split" if split else "trace") + ("_forward_only" if expect_forward_only else "")
    assert tr.tracer_wrapper.calls == [name]
    assert packs == ["activate_pack" if fused else "pack_particles"]
    if split:
        assert model.feature_calls == 0
    elif switch and not expect_forward_only and leaves != "all":
        # positions frozen, another leaf trainable: get_features() is evaluated to find that out and again by the path taken instead
        assert model.feature_calls in (1, 2)
    else:
        assert model.feature_calls == 1
    assert tr.stats_forward_only == {"forward_only_calls": int(expect_forward_only), "training_calls": int(not expect_forward_only)}
    assert tr.stats_split == {"split_calls": int(split), "cat_calls": int(not split)}
    # the dict is today's: keys, shapes, dtypes
    assert set(out) == {"pred_features", "pred_opacity", "pred_dist", "pred_normals", "hits_count", "frame_time_ms", "mog_visibility"}
    shapes = dict(pred_features=(1, H, W, 3), pred_opacity=(1, H, W, 1), pred_dist=(1, H, W, 1), pred_normals=(1, H, W, 3), hits_count=(1, H, W, 1),
                  mog_visibility=(N, 1))
    for k, shape in shapes.items():
        assert tuple(out[k].shape) == shape and out[k].dtype == torch.float32, k
    assert out["pred_features"].is_contiguous() and out["pred_opacity"].is_contiguous()
    # a plain call leaves no autograd node; a frame that can be differentiated keeps its node
    differentiable = grad_mode and leaves != "none"
    assert (out["pred_features"].grad_fn is not None) == differentiable
    if expect_forward_only:
        assert all(out[k].grad_fn is None and not out[k].requires_grad for k in shapes)


def test_switch_from_the_environment_and_train_flag_is_ignored(fake, monkeypatch):
    make_tracer, _ = fake
    monkeypatch.setenv("GRUT_FORWARD_ONLY", "1")
    tr = make_tracer()
    model, batch = _model_and_batch()
    with torch.no_grad():
        tr.render(model, batch, train=True)
        tr.render(model, batch, train=False)
    tr.render(model, batch, train=False)   # grad mode on, leaves require grad: differentiable whatever `train` says
    assert tr.tracer_wrapper.calls == ["trace_forward_only", "trace_forward_only", "trace"]
    assert tr.stats_forward_only == {"forward_only_calls": 2, "training_calls": 1}
