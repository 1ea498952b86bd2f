"""CPU: the split-SH surface (render.split_sh_features) - the three C entry points are declared, exported and mirrored in ctypes with
the header's argument counts; the switch reads its key and its environment variable; and, under the reference's own
MixtureOfGaussians with the recording fake of tests/test_reference_seam_cpu.py in place of the C handle, the plugin hands the library
the model's two SH Parameters themselves (no get_features call) and routes the two returned gradients into their .grad."""
import importlib
import os
import re
import subprocess

import pytest
import torch

import test_reference_seam_cpu as seam
from test_reference_seam_cpu import reference  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_ENTRY_POINTS = ("gut_forward_split", "gut_backward_split", "gut_backward_unpacked_split")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(seam.REFERENCE, "threedgrut")),
                                     reason="the reference checkout is only present in the build container")


def _header_prototype(header, name):
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/grut_amd.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_split_entry_points_are_declared_exported_and_mirrored(grut_lib, tmp_path):
    abi = importlib.import_module("3dgrut_amd._abi")
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    for name in SPLIT_ENTRY_POINTS:
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(grut_lib, name), f"{name} missing from libgrut_amd.so"
        args = _header_prototype(header, name)
        assert len(getattr(grut_lib, name).argtypes) == len(args), (name, args)
    assert len(_header_prototype(header, "gut_forward_split")) == len(_header_prototype(header, "gut_forward")) + 1
    assert len(_header_prototype(header, "gut_backward_split")) == len(_header_prototype(header, "gut_backward")) + 2
    assert len(_header_prototype(header, "gut_backward_unpacked_split")) == len(_header_prototype(header, "gut_backward_unpacked")) + 2
    # the C compiler's view of the three prototypes: typed function pointers must accept them as they are
    f = "const float*"
    src = tmp_path / "split.c"
    src.write_text(
        '#include "grut_amd.h"\n'
        f"int (*a)(GutHandle*, void*, const GutFrame*, {f}, {f}, {f}, {f}, {f}, void*, float*, float*, int32_t*) = gut_forward_split;\n"
        f"int (*b)(GutHandle*, void*, const GutFrame*, {f}, {f}, {f}, {f}, {f}, const void*, {f}, {f}, {f}, float*, float*, float*) = gut_backward_split;\n"
        f"int (*c)(GutHandle*, void*, const GutFrame*, {f}, {f}, {f}, {f}, {f}, const void*, {f}, {f}, const GutGradIO*, float*, float*) = gut_backward_unpacked_split;\n"
        "int main(void) { return a && b && c ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "split.o")])
    assert grut_lib.grut_abi_version() == abi.ABI_VERSION   # additive: the version stays


def test_split_sh_requested_reads_the_key_and_the_environment(monkeypatch):
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    monkeypatch.delenv("GRUT_SPLIT_SH", raising=False)
    assert not gt.split_sh_requested({"render": {}})
    assert not gt.split_sh_requested({"render": {"split_sh_features": False}})
    assert not gt.split_sh_requested(None)
    assert gt.split_sh_requested({"render": {"split_sh_features": True}})
    assert gt.split_sh_requested(seam._DictConfig({"render": {"split_sh_features": True}}))
    monkeypatch.setenv("GRUT_SPLIT_SH", "1")
    assert gt.split_sh_requested({"render": {}})


class _SplitRecorder(seam._GutRecorder):
    """The seam test's recorder with the split methods of the native wrapper: records the addresses that cross the boundary."""

    def _check_split(self, pd, albedo, specular, n):
        assert pd.shape == (n, 12) and pd.dtype == torch.float32 and pd.is_contiguous()
        assert albedo.shape == (n, 3) and specular.shape == (n, 45)
        assert albedo.dtype == specular.dtype == torch.float32 and albedo.is_contiguous() and specular.is_contiguous()

    def trace_split(self, frame, pd, albedo, specular, ro, rd):
        H, W, n = frame.height, frame.width, frame.num_particles
        self._check_split(pd, albedo, specular, n)
        self.calls.append(("trace_split", albedo.data_ptr(), specular.data_ptr(), int(frame.n_active_features)))
        fd = torch.rand((H, W, 4))
        return fd, torch.rand((H, W, 1)), torch.zeros((H, W, 1)), torch.ones((n, 1)), fd[..., :3].contiguous(), fd[..., 3:].contiguous()

    def trace_bwd_unpacked_split(self, frame, pd, albedo, specular, ro, rd, fd, g_feat, g_opa, dist, g_dist):
        n = frame.num_particles
        self._check_split(pd, albedo, specular, n)
        self.calls.append(("trace_bwd_split", albedo.data_ptr(), specular.data_ptr(), int(frame.n_active_features)))
        return (torch.ones((n, 3)), torch.ones((n, 1)), torch.ones((n, 4)), torch.ones((n, 3)),
                torch.full((n, 3), 2.0), torch.arange(n * 45, dtype=torch.float32).reshape(n, 45))


@needs_reference
@pytest.mark.parametrize("n_active", [3, 1])
def test_reference_model_hands_over_its_two_sh_parameters(reference, monkeypatch, n_active):  # noqa: F811
    abi = importlib.import_module("3dgrut_amd._abi")
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    seam._REAL.update(gut=gt._GutNative)
    monkeypatch.setattr(gt, "_GutNative", _SplitRecorder)
    monkeypatch.setattr(abi, "pack_particles", lambda pos, dns, rot, scl: torch.cat([pos, dns, rot, scl, torch.zeros_like(dns)], dim=1))
    model_mod = importlib.import_module("threedgrut.model.model")
    Batch = importlib.import_module("threedgrut.datasets.protocols").Batch
    conf = seam._conf("3dgut")
    conf["render"]["split_sh_features"] = True
    mog = model_mod.MixtureOfGaussians(conf, scene_extent=1.0)
    assert type(mog.renderer) is gt.Tracer and mog.renderer._split_sh
    n, H, W = 50, 20, 28
    g = torch.Generator().manual_seed(0)
    P = torch.nn.Parameter
    mog.positions, mog.rotation = P(torch.randn((n, 3), generator=g)), P(torch.randn((n, 4), generator=g))
    mog.scale, mog.density = P(torch.randn((n, 3), generator=g) - 3), P(torch.randn((n, 1), generator=g))
    mog.features_albedo, mog.features_specular = P(torch.rand((n, 3), generator=g)), P(torch.rand((n, 45), generator=g))
    mog.n_active_features = n_active   # progressive training (model.py: init_n_features .. max_n_features)
    feature_calls = []
    real_get_features = mog.get_features
    monkeypatch.setattr(mog, "get_features", lambda *a, **k: (feature_calls.append(1), real_get_features(*a, **k))[1])
    mog.build_acc(rebuild=True)
    d = torch.nn.functional.normalize(torch.randn((1, H, W, 3), generator=g), dim=-1)
    batch = Batch(rays_ori=torch.zeros((1, H, W, 3)), rays_dir=d, T_to_world=torch.eye(4)[None], intrinsics=[30.0, 30.0, W / 2, H / 2])
    out = mog(batch, train=True, frame_id=5)
    assert out["pred_features"].shape == (1, H, W, 3) and out["pred_opacity"].shape == (1, H, W, 1)
    (out["pred_features"].sum() + out["pred_opacity"].sum()).backward()
    ptrs = (mog.features_albedo.data_ptr(), mog.features_specular.data_ptr())
    assert mog.renderer.tracer_wrapper.calls == [("trace_split", *ptrs, n_active), ("trace_bwd_split", *ptrs, n_active)]
    assert feature_calls == [] and mog.renderer.stats_split == {"split_calls": 1, "cat_calls": 0}
    assert torch.equal(mog.features_albedo.grad, torch.full((n, 3), 2.0))
    assert torch.equal(mog.features_specular.grad, torch.arange(n * 45, dtype=torch.float32).reshape(n, 45))
    assert mog.features_albedo.grad.is_contiguous() and mog.features_specular.grad.is_contiguous()
    for name in ("positions", "rotation", "scale", "density"):
        grad = getattr(mog, name).grad
        assert grad is not None and grad.shape == getattr(mog, name).shape, name


@needs_reference
def test_reference_model_without_the_key_keeps_get_features(reference, monkeypatch):  # noqa: F811
    """Off unless asked for: the same model on the seam test's own recorder (which has no split methods) takes the cat path."""
    abi = importlib.import_module("3dgrut_amd._abi")
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    monkeypatch.delenv("GRUT_SPLIT_SH", raising=False)
    seam._REAL.update(gut=gt._GutNative)
    monkeypatch.setattr(gt, "_GutNative", seam._GutRecorder)
    monkeypatch.setattr(abi, "pack_particles", lambda pos, dns, rot, scl: torch.cat([pos, dns, rot, scl, torch.zeros_like(dns)], dim=1))
    model_mod = importlib.import_module("threedgrut.model.model")
    Batch = importlib.import_module("threedgrut.datasets.protocols").Batch
    mog = model_mod.MixtureOfGaussians(seam._conf("3dgut"), scene_extent=1.0)
    n, H, W = 20, 12, 16
    P = torch.nn.Parameter
    mog.positions, mog.rotation, mog.scale, mog.density = P(torch.randn(n, 3)), P(torch.randn(n, 4)), P(torch.randn(n, 3) - 3), P(torch.randn(n, 1))
    mog.features_albedo, mog.features_specular = P(torch.rand(n, 3)), P(torch.rand(n, 45))
    d = torch.nn.functional.normalize(torch.randn(1, H, W, 3), dim=-1)
    batch = Batch(rays_ori=torch.zeros((1, H, W, 3)), rays_dir=d, T_to_world=torch.eye(4)[None], intrinsics=[30.0, 30.0, W / 2, H / 2])
    mog(batch, train=True, frame_id=1)
    assert [c[0] for c in mog.renderer.tracer_wrapper.calls] == ["trace"]
    assert mog.renderer.stats_split == {"split_calls": 0, "cat_calls": 1}
