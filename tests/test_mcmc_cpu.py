"""CPU: the MCMC strategy's two C-ABI entry points are declared, mirrored and exported, the Python surface rejects what the reference's
extension rejects, and the seam with the reference's own `threedgrut.strategy.mcmc` holds: with `shims/` on the path the strategy's
`load_mcmc_plugin()` binds this repository's module (the nvcc JIT is never reached) and `install_fused_perturb()` swaps in a subclass
whose `perturb_gaussians` drives the fused kernel.  What the kernels compute is covered by tests/test_mcmc_gpu.py."""
import importlib
import os
import re
import sys
import types

import pytest
import torch

from test_reference_seam_cpu import REFERENCE, _REAL, _conf, _DictConfig, _GutRecorder, reference  # noqa: F401  (the reference fixture, its stubs and its ctypes fake)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("grut_mcmc_relocation", "grut_mcmc_perturb")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "threedgrut")),
                                     reason="the reference checkout is only present in the build container")


def test_mcmc_symbols_are_declared_mirrored_and_exported(grut_lib):
    abi = importlib.import_module("3dgrut_amd._abi")
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(void\* stream, uint32_t n,", header), name
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(grut_lib, name) and getattr(grut_lib, name).argtypes, name
    assert "mcmc.hip" in importlib.import_module("3dgrut_amd.build").SOURCES


def test_relocation_input_checks_match_the_extension():
    """bindings.cpp:32-37 / gaussian_mcmc.cu:75-77: CUDA, contiguous, matching sizes -> RuntimeError (checked before any launch)."""
    mcmc = importlib.import_module("3dgrut_amd.mcmc")
    n, n_max = 8, 51
    args = [torch.rand(n, 1), torch.rand(n, 3), torch.ones(n, dtype=torch.int32), torch.zeros(n_max, n_max)]
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        mcmc.compute_relocation_tensor(*args, n_max)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        mcmc.perturb_positions_(torch.zeros(n, 3), torch.ones(n, 4), torch.zeros(n, 3), torch.zeros(n, 1), torch.zeros(n, 3), 5e5, 1e-4)


def test_install_registers_the_plugin_module_without_importing_threedgrut(monkeypatch):
    mcmc = importlib.import_module("3dgrut_amd.mcmc")
    monkeypatch.delitem(sys.modules, mcmc.PLUGIN_MODULE, raising=False)
    before = {k for k in sys.modules if k.split(".")[0] == "threedgrut"}
    mcmc.install()
    assert sys.modules[mcmc.PLUGIN_MODULE] is mcmc
    assert {k for k in sys.modules if k.split(".")[0] == "threedgrut"} - before == {mcmc.PLUGIN_MODULE}


@needs_reference
def test_reference_strategy_loads_this_plugin_and_takes_the_fused_perturbation(reference, monkeypatch):  # noqa: F811
    mcmc = importlib.import_module("3dgrut_amd.mcmc")
    # the JIT fallback must never run: a setup_mcmc that raises stands in for nvcc being absent
    jit = types.ModuleType("threedgrut.strategy.src.setup_mcmc")

    def no_nvcc():
        raise AssertionError("the nvcc JIT fallback was reached")

    jit.setup_mcmc = no_nvcc
    monkeypatch.setitem(sys.modules, "threedgrut.strategy.src.setup_mcmc", jit)
    model_mod = importlib.import_module("threedgrut.model.model")       # imports the shims -> install()
    ref = importlib.import_module("threedgrut.strategy.mcmc")
    reference_class = ref.MCMCStrategy
    ref.load_mcmc_plugin()
    assert ref._mcmc_plugin is mcmc

    fused = mcmc.install_fused_perturb()
    assert ref.MCMCStrategy is fused and issubclass(fused, reference_class) and fused is not reference_class
    assert mcmc.install_fused_perturb() is fused

    # the subclass constructed around the reference's own model, as trainer.py:259-262 does (the renderer's ctypes layer faked as in
    # test_reference_seam_cpu.py: there is no GPU here)
    gt = importlib.import_module("3dgrut_amd.gut_tracer")
    _REAL.setdefault("gut", gt._GutNative)
    monkeypatch.setattr(gt, "_GutNative", _GutRecorder)
    mog = model_mod.MixtureOfGaussians(_conf("3dgut"), scene_extent=1.0)
    mog.device = "cpu"
    n = 40
    g = torch.Generator().manual_seed(1)
    P = torch.nn.Parameter
    mog.positions, mog.rotation = P(torch.randn((n, 3), generator=g)), P(torch.randn((n, 4), generator=g))
    mog.scale, mog.density = P(torch.randn((n, 3), generator=g) - 3), P(torch.randn((n, 1), generator=g))
    mog.optimizer = torch.optim.Adam([{"params": [mog.positions], "name": "positions", "lr": 1.6e-4},
                                      {"params": [mog.density], "name": "density", "lr": 5e-2}])
    conf = _DictConfig({"strategy": {"binom_n_max": 51, "opacity_threshold": 0.005, "perturb": {"noise_lr": 5e5}}})
    strategy = ref.MCMCStrategy(conf, mog)
    assert tuple(strategy.binoms.shape) == (51, 51) and float(strategy.binoms[50, 25]) > 1e13

    calls = []

    def record(positions, rotation, scale, density, noise, noise_lr, lr, activated=False):   # the kernel's operands, on the host
        calls.append(dict(positions=positions, rotation=rotation, scale=scale, density=density, noise=noise.clone(), noise_lr=noise_lr,
                          lr=lr, activated=activated))

    monkeypatch.setattr(mcmc, "perturb_positions_", record)
    torch.manual_seed(7)
    ptr = mog.positions.data_ptr()
    strategy.perturb_gaussians()
    (c,) = calls
    after = torch.get_rng_state()
    torch.manual_seed(7)
    assert torch.equal(c["noise"], torch.randn_like(mog.positions))       # one randn_like draw: the generator advances as the reference's
    assert torch.equal(torch.get_rng_state(), after)
    assert c["positions"].data_ptr() == ptr and c["lr"] == 1.6e-4 and c["noise_lr"] == 5e5
    assert c["activated"] is False and c["rotation"].data_ptr() == mog.rotation.data_ptr()   # raw path: the model's own tensors
    assert c["density"].data_ptr() == mog.density.data_ptr() and c["scale"].data_ptr() == mog.scale.data_ptr()

    mog.density_activation = lambda x: torch.sigmoid(x) * 0.5                           # a non-default activation: activated path
    calls.clear()
    strategy.perturb_gaussians()
    assert calls[0]["activated"] is True and torch.equal(calls[0]["density"], torch.sigmoid(mog.density) * 0.5)
