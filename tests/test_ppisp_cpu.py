"""CPU: the `ppisp` drop-in (3dgrut_amd/ppisp.py, shims/ppisp) without a GPU.  The model's float64 restatement (tests/ppisp_reference.py)
is held against the reference's own fp32 statement of it through tests/golden/ppisp.npz; the module's surface - parameters, state_dict,
controllers, novel views, the activation switch, distillation, optimizers, schedulers, regulariser, report - is driven on the torch path
that every tensor that is not an fp32 CUDA tensor takes, which obeys the same gradient conventions at the kinks as the kernels; and the
reference's own `Trainer3DGRUT.init_post_processing` / `apply_post_processing` are run against it.  What the kernels compute is covered by
tests/test_ppisp_gpu.py."""
import importlib
import importlib.util
import json
import os
import re
import sys
import types

import pytest
import torch

import ppisp_reference as R
from test_photo_loss_cpu import _MORE_STUBS, _NoRange
from test_reference_seam_cpu import REFERENCE, _DictConfig, reference  # noqa: F401  (the reference fixture and its import stubs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ppisp.npz")
NEW_SYMBOLS = ("grut_ppisp_forward", "grut_ppisp_backward", "grut_ppisp_partials")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "threedgrut")),
                                     reason="the reference checkout is only present in the build container")


@pytest.fixture(scope="module")
def golden():
    return R.load_golden(GOLDEN)


@pytest.fixture()
def ppisp():
    return importlib.import_module("3dgrut_amd.ppisp")


def test_ppisp_symbols_are_declared_mirrored_and_exported(grut_lib):
    abi = importlib.import_module("3dgrut_amd._abi")
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b(int|uint32_t) {name}\(", header), name
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(grut_lib, name) and getattr(grut_lib, name).argtypes, name
    assert abi.ABI_VERSION == 5 and grut_lib.grut_abi_version() == 5           # additive change
    assert len(grut_lib.grut_ppisp_forward.argtypes) == 11 and len(grut_lib.grut_ppisp_backward.argtypes) == 17
    # one 48-float row per block of 1024 pixels, at most 1024 blocks; nothing for an empty image
    assert [grut_lib.grut_ppisp_partials(n) for n in (0, 1, 1024, 1025, 1920 * 1080, 2 ** 32 - 1)] == [0, 48, 48, 96, 48 * 1024, 48 * 1024]


def test_the_shim_package_resolves_to_this_project(monkeypatch, ppisp):
    for name in ("ppisp", "ppisp.report"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "shims"))
    from ppisp import PPISP, PPISPConfig, ppisp_apply
    from ppisp.report import export_ppisp_report
    assert sys.modules["ppisp"].__file__ == os.path.join(ROOT, "shims", "ppisp", "__init__.py")
    assert PPISP is ppisp.PPISP and PPISPConfig is ppisp.PPISPConfig and ppisp_apply is ppisp.ppisp_apply
    assert export_ppisp_report is ppisp.export_ppisp_report


def test_install_registers_the_package_unless_one_is_there(monkeypatch, ppisp):
    for name in ("ppisp", "ppisp.report"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    ppisp.install()
    from ppisp import PPISP, PPISPConfig, ppisp_apply  # noqa: F401
    from ppisp.report import export_ppisp_report
    assert PPISP is ppisp.PPISP and export_ppisp_report is ppisp.export_ppisp_report
    mine = types.ModuleType("ppisp")
    monkeypatch.setitem(sys.modules, "ppisp", mine)
    ppisp.install()
    assert sys.modules["ppisp"] is mine                                          # a package that is already there wins
    for shim in ("threedgut_tracer", "threedgrt_tracer"):                        # both tracer shims call it, next to losses.install()
        text = open(os.path.join(ROOT, "shims", shim, "__init__.py")).read()
        assert text.index('"3dgrut_amd.losses").install()') < text.index('"3dgrut_amd.ppisp").install()')


def test_the_restatement_agrees_with_the_golden_reference(golden):
    assert len(golden) == 3 * len(R.SHAPES) and {(c["h"], c["w"]) for c in golden} == set(R.SHAPES)
    assert os.path.getsize(GOLDEN) < 256 * 1024
    for c in golden:
        out = R.ppisp_model(c["rgb"], c["pc"], (c["w"], c["h"]), c["exposure"], c["color"], c["vignetting"], c["crf"])
        e_ref = float((c["ref32"].double() - out).abs().max())
        print(f"{c['name']}: e_ref {e_ref:.3e} (stored {c['e_ref']:.3e})")
        assert abs(e_ref - c["e_ref"]) <= 0.01 * c["e_ref"], c["name"]
        assert e_ref < 1 / 510, c["name"]     # half the 8-bit step at which the reference compares its two implementations
        assert bool((c["rgb"] == 0).any()) or c["h"] * c["w"] <= 1024, c["name"]
        assert bool((c["rgb"] >= 1).any())
        left_out = 1 - float(R.kink_free(c).float().mean())
        assert left_out <= R.MAX_LEFT_OUT, (c["name"], left_out)


def test_the_torch_path_agrees_with_the_restatement(golden, ppisp):
    """fp32 on the CPU: within 4 e_ref of the float64 restatement, like the kernels (the host's libm is the better of the two)."""
    for c in golden:
        want = R.ppisp_model(c["rgb"], c["pc"], (c["w"], c["h"]), c["exposure"], c["color"], c["vignetting"], c["crf"])
        got = ppisp.ppisp_apply(exposure_params=c["exposure"], vignetting_params=c["vignetting"][None], color_params=c["color"][None],
                                crf_params=c["crf"][None], rgb_in=c["rgb"], pixel_coords=c["pc"], resolution_w=c["w"], resolution_h=c["h"],
                                camera_idx=0, frame_idx=0)
        assert got.dtype == torch.float32 and got.shape == c["rgb"].shape
        assert float((got.double() - want).abs().max()) <= 4 * c["e_ref"], c["name"]


def test_identity_initialisation_returns_the_clamped_input(golden, ppisp):
    module = ppisp.PPISP(num_cameras=2, num_frames=3, config=ppisp.PPISPConfig(use_controller=False)).eval()
    for c in (c for c in golden if c["name"].endswith("identity")):
        rgb = c["rgb"].reshape(-1, 3)
        out = module(rgb, c["pc"].reshape(-1, 2), resolution=(c["w"], c["h"]), camera_idx=1, frame_idx=2)
        inten = rgb.sum(-1)
        bound = 1e-5 * float(rgb.max()) / float(inten[inten > 0].min()) + 4 * c["e_ref"]
        assert float((out.detach() - rgb.clamp(0, 1)).abs().max()) <= bound, c["name"]


def test_parameters_state_dict_and_round_trip(ppisp):
    module = ppisp.PPISP(num_cameras=2, num_frames=5)
    shapes = {k: tuple(v.shape) for k, v in module.named_parameters() if "." not in k}
    assert shapes == {"exposure_params": (5,), "color_params": (5, 8), "vignetting_params": (2, 3, 5), "crf_params": (2, 3, 4)}
    assert float(module.exposure_params.abs().max()) == 0 and float(module.color_params.abs().max()) == 0
    assert float(module.vignetting_params.abs().max()) == 0
    assert torch.equal(module.crf_params, torch.tensor(R.CRF_IDENTITY, dtype=torch.float32).repeat(2, 3, 1))
    assert isinstance(module.controllers, torch.nn.ModuleList) and len(module.controllers) == 2
    keys = set(module.state_dict())
    assert {"exposure_params", "color_params", "vignetting_params", "crf_params", "controllers.1.color_head.bias"} <= keys
    assert len(ppisp.PPISP(2, 5, ppisp.PPISPConfig(use_controller=False)).controllers) == 0
    with torch.no_grad():
        for p in module.parameters():
            p.add_(torch.randn_like(p) * 0.1)
    for config in (None, ppisp.PPISPConfig(use_controller=True)):
        clone = ppisp.PPISP.from_state_dict(module.state_dict(), config=config)
        assert clone.num_cameras == 2 and clone.num_frames == 5 and len(clone.controllers) == 2
        assert all(torch.equal(v, clone.state_dict()[k]) for k, v in module.state_dict().items())
    upstream = {k: v for k, v in module.state_dict().items() if k != "step"}     # a checkpoint without this module's counter
    assert ppisp.PPISP.from_state_dict(upstream).steps_done == 0
    plain = ppisp.PPISP.from_state_dict(ppisp.PPISP(1, 2, ppisp.PPISPConfig(use_controller=False)).state_dict())
    assert len(plain.controllers) == 0 and not plain.config.use_controller


@needs_reference
def test_the_controller_passes_the_reference_architecture_check(ppisp):
    path = os.path.join(REFERENCE, "threedgrut", "export", "usd", "post_processing", "ppisp_controller_weights.py")
    spec = importlib.util.spec_from_file_location("_reference_ppisp_controller_weights", path)
    ref = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = ref            # its dataclass looks its own module up
    try:
        spec.loader.exec_module(ref)
        module = ppisp.PPISP(num_cameras=2, num_frames=1)
        controller = ref.select_camera_controller(module, 1)
        ref.validate_controller_architecture(controller)
        flat = ref.flatten_controller_weights(controller)
        assert flat.shape == (241961,) == (ref.EXPECTED_CONTROLLER_WEIGHTS_LEN,)
    finally:
        del sys.modules[spec.name]
    exposure, color = controller(torch.rand(31, 37, 3), torch.tensor([0.17]))
    assert exposure.numel() == 1 and color.shape == (8,)


def _randomise(module, seed):
    par = R.random_parameters(seed)
    with torch.no_grad():
        module.exposure_params.uniform_(-0.35, 0.35)
        module.color_params.normal_(0, 0.35)
        module.vignetting_params.copy_(par["vignetting"].expand_as(module.vignetting_params))
        module.crf_params.copy_(par["crf"].expand_as(module.crf_params))
        for c in module.controllers:
            for name, p in c.named_parameters():
                p.normal_(0, 0.03)


def test_novel_views(golden, ppisp):
    c = golden[3]
    rgb, pc, res = c["rgb"].reshape(-1, 3), c["pc"].reshape(-1, 2), (c["w"], c["h"])
    torch.manual_seed(0)
    plain = ppisp.PPISP(2, 3, ppisp.PPISPConfig(use_controller=False)).eval()
    _randomise(plain, 7)
    out = plain(rgb, pc, resolution=res, camera_idx=1, frame_idx=-1)
    zero = ppisp.ppisp_apply(exposure_params=torch.zeros(1), vignetting_params=plain.vignetting_params, color_params=torch.zeros(1, 8),
                             crf_params=plain.crf_params, rgb_in=rgb, pixel_coords=pc, resolution_w=res[0], resolution_h=res[1], camera_idx=1,
                             frame_idx=0)
    inten = rgb.sum(-1)
    assert float((out - zero).abs().max()) <= 1e-5 * float(rgb.max()) / float(inten[inten > 0].min()) * 4 + 1e-5   # the 1e-5 of the intensity ratio
    off = ppisp.ppisp_apply(vignetting_params=plain.vignetting_params, crf_params=plain.crf_params, rgb_in=rgb, pixel_coords=pc,
                            resolution_w=res[0], resolution_h=res[1], camera_idx=1, frame_idx=-1)
    assert torch.equal(out, off)                                                 # the two stages are the identity
    assert torch.equal(plain(rgb, pc, resolution=res, camera_idx=-1, frame_idx=-1), rgb)     # no camera either: nothing applies

    module = ppisp.PPISP(2, 3).eval()
    _randomise(module, 7)
    prior = torch.tensor([0.3])
    got = module(rgb, pc, resolution=res, camera_idx=1, frame_idx=-1, exposure_prior=prior)
    e, col = module.controllers[1](rgb.reshape(c["h"], c["w"], 3), prior)
    assert float(e.abs()) > 0 and float(col.abs().max()) > 0
    want = ppisp.ppisp_apply(exposure_params=e.reshape(1), vignetting_params=module.vignetting_params, color_params=col.reshape(1, 8),
                             crf_params=module.crf_params, rgb_in=rgb, pixel_coords=pc, resolution_w=res[0], resolution_h=res[1], camera_idx=1,
                             frame_idx=0)
    assert torch.equal(got, want)
    e0, col0 = module.controllers[1](rgb.reshape(c["h"], c["w"], 3), torch.zeros(1))      # no prior given: zeros(1)
    assert torch.equal(module(rgb, pc, resolution=res, camera_idx=1, frame_idx=-1),
                       ppisp.ppisp_apply(exposure_params=e0.reshape(1), vignetting_params=module.vignetting_params, color_params=col0.reshape(1, 8),
                                         crf_params=module.crf_params, rgb_in=rgb, pixel_coords=pc, resolution_w=res[0], resolution_h=res[1],
                                         camera_idx=1, frame_idx=0))
    with pytest.raises(ValueError, match="whole image"):
        module(rgb[:-1], pc[:-1], resolution=res, camera_idx=1, frame_idx=-1)
    assert torch.equal(module(rgb, pc, resolution=res, camera_idx=1, frame_idx=2),           # with a frame row the controller is not asked
                       ppisp.ppisp_apply(exposure_params=module.exposure_params, vignetting_params=module.vignetting_params,
                                         color_params=module.color_params, crf_params=module.crf_params, rgb_in=rgb, pixel_coords=pc,
                                         resolution_w=res[0], resolution_h=res[1], camera_idx=1, frame_idx=2))


@pytest.mark.parametrize("distillation", [False, True])
def test_activation_switch_and_distillation(golden, ppisp, distillation):
    c = golden[0]
    rgb, pc, res = c["rgb"].reshape(-1, 3), c["pc"].reshape(-1, 2), (c["w"], c["h"])
    torch.manual_seed(1)
    module = ppisp.PPISP(1, 2, ppisp.PPISPConfig(controller_activation_ratio=0.4, controller_distillation=distillation)).train()
    _randomise(module, 3)
    for _ in range(6):
        module(rgb, pc, resolution=res, camera_idx=0, frame_idx=1)
        assert not module.controller_active                                      # never before create_schedulers was called
    module = ppisp.PPISP(1, 2, ppisp.PPISPConfig(controller_activation_ratio=0.4, controller_distillation=distillation)).train()
    _randomise(module, 3)
    optimizers = module.create_optimizers()
    module.create_schedulers(optimizers, max_optimization_iters=10)
    for step in range(7):
        assert module.controller_active == (step >= 4) and module.steps_done == step and int(module.step) == step
        module(rgb, pc, resolution=res, camera_idx=0, frame_idx=1)
    module(rgb, pc, resolution=res, camera_idx=0, frame_idx=-1)                  # a novel view does not advance the counter
    module.eval()
    module(rgb, pc, resolution=res, camera_idx=0, frame_idx=1)                   # nor does an evaluation
    assert module.steps_done == 7 and not module.controller_active              # the switch is a training-mode matter
    module.train()
    resumed = ppisp.PPISP.from_state_dict(module.state_dict(), config=module.config).train()
    resumed.create_schedulers(resumed.create_optimizers(), max_optimization_iters=10)
    assert resumed.steps_done == 7 and resumed.controller_active                 # the counter travels in the checkpoint

    leaf = rgb.clone().requires_grad_(True)
    out = module(leaf, pc, resolution=res, camera_idx=0, frame_idx=1)            # active: exposure and colour come from the controller
    e, col = module.controllers[0](rgb.reshape(c["h"], c["w"], 3), torch.zeros(1))
    want = ppisp.ppisp_apply(exposure_params=e.reshape(1), vignetting_params=module.vignetting_params, color_params=col.reshape(1, 8),
                             crf_params=module.crf_params, rgb_in=rgb, pixel_coords=pc, resolution_w=res[0], resolution_h=res[1], camera_idx=0,
                             frame_idx=0)
    assert torch.equal(out.detach(), want.detach())
    out.sum().backward()
    four = (module.exposure_params, module.color_params, module.vignetting_params, module.crf_params)
    assert module.controllers[0].color_head.weight.grad is not None and float(module.controllers[0].color_head.weight.grad.abs().max()) > 0
    assert module.exposure_params.grad is None and module.color_params.grad is None          # their rows are not used any more
    if distillation:                                                            # only the controller learns
        assert all(p.grad is None for p in four) and leaf.grad is None
    else:
        assert module.vignetting_params.grad is not None and module.crf_params.grad is not None and leaf.grad is not None


def test_optimizers_schedulers_regulariser_and_report(ppisp, tmp_path):
    module = ppisp.PPISP(2, 5)
    optimizers = module.create_optimizers()
    assert [type(o) for o in optimizers] == [torch.optim.Adam, torch.optim.Adam]
    g0, g1 = optimizers[0].param_groups[0], optimizers[1].param_groups[0]
    assert g0["lr"] == 2e-3 and g0["eps"] == 1e-15 and {id(p) for p in g0["params"]} == {id(p) for n, p in module.named_parameters() if "." not in n}
    assert g1["lr"] == 2e-3 and len(g1["params"]) == len(list(module.controllers.parameters()))
    assert len(ppisp.PPISP(2, 5, ppisp.PPISPConfig(use_controller=False)).create_optimizers()) == 1
    schedulers = module.create_schedulers(optimizers, max_optimization_iters=2000)
    assert len(schedulers) == 2 and all(isinstance(s, torch.optim.lr_scheduler.LambdaLR) for s in schedulers)
    lrs = []
    for _ in range(2000):
        lrs.append(optimizers[0].param_groups[0]["lr"])
        optimizers[0].step()
        schedulers[0].step()
    lrs.append(optimizers[0].param_groups[0]["lr"])
    decay = lambda s: 0.01 ** (s / 2000)   # noqa: E731
    assert lrs[0] == pytest.approx(2e-3 * 0.01) and lrs[250] == pytest.approx(2e-3 * (0.01 + 0.99 * 0.5) * decay(250))
    assert lrs[500] == pytest.approx(2e-3 * decay(500)) and lrs[2000] == pytest.approx(2e-3 * 0.01)

    assert float(module.get_regularization_loss()) == 0.0 and module.get_regularization_loss().dim() == 0       # the identity costs nothing
    torch.manual_seed(2)
    _randomise(module, 5)
    with torch.no_grad():
        module.vignetting_params.add_(torch.randn_like(module.vignetting_params) * 0.05)
        module.crf_params.add_(torch.randn_like(module.crf_params) * 0.05)
    e, col, vig, crf = module.exposure_params, module.color_params, module.vignetting_params, module.crf_params
    want = (1.0 * e.mean() ** 2 + 1.0 * (col.mean(0) ** 2).mean() + 0.02 * (vig[..., :2] ** 2).mean() + 0.01 * (vig[..., 2:].clamp_min(0) ** 2).mean()
            + 0.1 * ((vig - vig.mean(1, keepdim=True)) ** 2).mean(1).mean() + 0.1 * ((crf - crf.mean(1, keepdim=True)) ** 2).mean(1).mean())
    assert float(module.get_regularization_loss()) == pytest.approx(float(want), rel=1e-5) and float(want) > 0
    module.config.exposure_mean_weight = 3.0                                      # the weights are config fields
    assert float(module.get_regularization_loss()) == pytest.approx(float(want + 2.0 * e.mean() ** 2), rel=1e-5)

    paths = ppisp.export_ppisp_report(module, frames_per_camera=[3, 2], output_dir=tmp_path / "report", camera_names=["left", "right"])
    assert [os.path.basename(p) for p in paths] == ["left.json", "right.json"]
    right = json.load(open(paths[1]))
    assert right["camera"] == "right" and [f["frame_index"] for f in right["frames"]] == [3, 4]
    assert right["frames"][1]["exposure"] == pytest.approx(float(e[4])) and right["frames"][0]["color"] == pytest.approx(col[3].tolist())
    assert torch.allclose(torch.tensor(right["vignetting_params"]), vig[1])
    assert torch.allclose(torch.tensor(right["crf_params"]), crf[1])
    assert len(ppisp.export_ppisp_report(module, [3, 2], tmp_path / "unnamed")) == 2


def test_kink_rules_on_the_torch_path(ppisp):
    par = R.random_parameters(11)
    rgb = torch.tensor([[0.0, 0.0, 0.0], [5.0, 6.0, 7.0], [0.3, 0.4, 0.2]], requires_grad=True)      # black, saturated, ordinary
    pc = torch.tensor([[0.5, 0.5], [3.5, 1.5], [2.5, 2.5]])
    leaves = {k: v.clone()[None].requires_grad_(True) for k, v in par.items()}
    out = ppisp.ppisp_apply(exposure_params=leaves["exposure"].reshape(1), vignetting_params=leaves["vignetting"], color_params=leaves["color"],
                            crf_params=leaves["crf"], rgb_in=rgb, pixel_coords=pc, resolution_w=4, resolution_h=3, camera_idx=0, frame_idx=0)
    assert torch.equal(out[0].detach(), torch.zeros(3)) and torch.equal(out[1].detach(), torch.ones(3))
    (out[:2] * torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])).sum().backward()
    for t in (rgb, *leaves.values()):
        assert bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) == 0.0     # nothing passes the curve at or beyond its ends
    out = ppisp.ppisp_apply(exposure_params=leaves["exposure"].reshape(1), vignetting_params=leaves["vignetting"], color_params=leaves["color"],
                            crf_params=leaves["crf"], rgb_in=rgb, pixel_coords=pc, resolution_w=4, resolution_h=3, camera_idx=0, frame_idx=0)
    out.sum().backward()
    for t in (rgb, *leaves.values()):
        assert bool(torch.isfinite(t.grad).all())
    assert float(rgb.grad[2].abs().min()) > 0 and float(leaves["crf"].grad.abs().min()) > 0

    module = ppisp.PPISP(1, 1, ppisp.PPISPConfig(use_controller=False))                     # every alpha is 0: p == 1 exactly
    image, coords = R.make_image(7, 9, 3).reshape(-1, 3), R.pixel_coords(7, 9).reshape(-1, 2)
    module(image, coords, resolution=(9, 7), camera_idx=0, frame_idx=0).sum().backward()
    assert float(module.vignetting_params.grad[0, :, 2:].abs().min()) > 0                   # an exclusive rule would never let them learn


@needs_reference
def test_the_reference_trainer_builds_and_steps_the_module(reference, monkeypatch, ppisp):  # noqa: F811
    from unittest.mock import MagicMock
    for name in _MORE_STUBS:
        try:
            if not name.startswith("threedgrut"):
                importlib.import_module(name)
                continue
        except ModuleNotFoundError:
            pass
        stub = MagicMock(name=name)
        stub.__path__, stub.__name__ = [], name
        monkeypatch.setitem(sys.modules, name, stub)
    for name in ("ppisp", "ppisp.report"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    monkeypatch.setattr(torch.cuda.nvtx, "range", _NoRange)
    trainer_mod = importlib.import_module("threedgrut.trainer")
    assert trainer_mod.__file__.startswith(REFERENCE)
    trainer = object.__new__(trainer_mod.Trainer3DGRUT)
    trainer.device = "cpu"
    trainer.train_dataset = types.SimpleNamespace(get_frames_per_camera=lambda: [3, 2])
    conf = _DictConfig(n_iterations=20, post_processing=dict(method="ppisp", use_controller=True, n_distillation_steps=5))
    trainer.init_post_processing(conf)

    module = trainer.post_processing
    assert isinstance(module, ppisp.PPISP) and module.num_cameras == 2 and module.num_frames == 5 and len(module.controllers) == 2
    assert module.config.controller_distillation and module.config.controller_activation_ratio == 0.75
    assert len(trainer.post_processing_optimizers) == 2 and len(trainer.post_processing_schedulers) == 2
    assert module.max_optimization_iters == 20 and trainer._distillation_start_step == 15

    h, w = 7, 9
    pred = R.make_image(h, w, 5)[None].requires_grad_(True)
    batch = types.SimpleNamespace(camera_idx=1, frame_idx=3, pixel_coords=R.pixel_coords(h, w)[None], exposure=None)
    outputs = trainer_mod.apply_post_processing(module, {"pred_features": pred}, batch, training=True)
    assert outputs["pred_features"].shape == (1, h, w, 3) and module.steps_done == 1
    reg = module.get_regularization_loss()
    before = [p.detach().clone() for p in (module.exposure_params, module.color_params, module.vignetting_params, module.crf_params)]
    ((outputs["pred_features"] - 0.5) ** 2).mean().add(reg).backward()
    assert pred.grad is not None and bool(torch.isfinite(pred.grad).all())
    assert float(module.exposure_params.grad[3].abs()) > 0 and float(module.exposure_params.grad[[0, 1, 2, 4]].abs().max()) == 0
    assert float(module.crf_params.grad[1].abs().max()) > 0 and float(module.crf_params.grad[0].abs().max()) == 0
    for opt in trainer.post_processing_optimizers:
        opt.step()
        opt.zero_grad()
    for sched in trainer.post_processing_schedulers:
        sched.step()
    after = (module.exposure_params, module.color_params, module.vignetting_params, module.crf_params)
    assert all(not torch.equal(a, b) for a, b in zip(after, before))
    novel = trainer_mod.apply_post_processing(module.eval(), {"pred_features": pred.detach()}, batch, training=False)
    assert novel["pred_features"].shape == (1, h, w, 3) and bool(torch.isfinite(novel["pred_features"]).all())
