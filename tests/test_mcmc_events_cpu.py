"""CPU: the MCMC events' C-ABI entry points are declared, mirrored and exported; the Python surface rejects what the kernels cannot
take before anything is launched; `install_fused_events()` swaps in a subclass of whatever class is bound, stacks with
`install_fused_perturb()` in both orders and hands a model it cannot take to the reference's method; and the restatement of
tests/mcmc_events_reference.py equals the reference's OWN class bit for bit.  What the kernels compute is covered by
tests/test_mcmc_events_gpu.py."""
import importlib
import os
import re
import sys
import types

import pytest
import torch

import mcmc_events_reference as mer
from test_reference_seam_cpu import REFERENCE, _DictConfig, reference  # noqa: F401  (the reference fixture and its stubs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("grut_mcmc_classify", "grut_mcmc_sample_plan", "grut_mcmc_relocate_rows", "grut_mcmc_append_rows")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "threedgrut")),
                                     reason="the reference checkout is only present in the build container")


def _mcmc():
    return importlib.import_module("3dgrut_amd.mcmc")


def test_event_symbols_are_declared_mirrored_and_exported(grut_lib):
    abi = importlib.import_module("3dgrut_amd._abi")
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\(void\* stream,", header), name
    assert re.search(r"\buint64_t grut_mcmc_classify_scratch_bytes\(uint32_t n\);", header)
    for name in ENTRY_POINTS + ("grut_mcmc_classify_scratch_bytes",):
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(grut_lib, name) and getattr(grut_lib, name).argtypes, name
    sources = importlib.import_module("3dgrut_amd.build").SOURCES
    csrc = os.path.join(ROOT, "3dgrut_amd", "csrc")
    defined = "".join(open(os.path.join(csrc, s)).read() for s in sources if s.startswith("mcmc"))
    for name in ENTRY_POINTS:
        assert re.search(rf'extern "C" int {name}\(', defined), name
    # the descriptor of the two row passes: 16 bytes, as the header lays it out
    assert (abi.McmcTensor.data.offset, abi.McmcTensor.row_elems.offset, abi.McmcTensor.role.offset) == (0, 8, 12)
    assert abi.MCMC_MAX_TENSORS == int(re.search(r"GRUT_MCMC_MAX_TENSORS = (\d+)", header).group(1))
    for role in ("COPY", "NEW_DENSITY", "NEW_SCALE", "STATE"):
        assert getattr(abi, f"MCMC_ROLE_{role}") == int(re.search(rf"GRUT_MCMC_ROLE_{role} = (\d+)", header).group(1))
    # nothing is launched for zero rows, and a NULL is refused before any HIP call with the argument's name (no GPU is needed for either)
    assert grut_lib.grut_mcmc_relocate_rows(None, None, 0, 0, None, None, None, None, None) == 0
    assert grut_lib.grut_mcmc_append_rows(None, None, None, 0, 0, 0, None, None, None, None, None) == 0
    assert grut_lib.grut_mcmc_sample_plan(None, 0, 0, None, None, 0, None, None, 0, None, 51, 0.005, *([None] * 7)) == 0
    assert grut_lib.grut_mcmc_classify(None, 8, None, 0.005, None, None, None, None, None, 0) != 0 and b"counts" in grut_lib.grut_last_error()
    assert grut_lib.grut_mcmc_sample_plan(None, 8, 4, None, None, 0, None, None, 0, None, 51, 0.005, *([None] * 7)) != 0
    assert b"count" in grut_lib.grut_last_error()
    assert grut_lib.grut_mcmc_sample_plan(None, 8, 4, None, None, 0, None, None, 0, None, 0, 0.005, *([None] * 7)) != 0
    assert b"n_max" in grut_lib.grut_last_error()
    one = (abi.McmcTensor * 1)(abi.McmcTensor(None, 3, abi.MCMC_ROLE_COPY))
    assert grut_lib.grut_mcmc_relocate_rows(None, one, 1, 4, None, None, None, None, None) != 0 and b"data" in grut_lib.grut_last_error()
    assert grut_lib.grut_mcmc_relocate_rows(None, one, 33, 4, None, None, None, None, None) != 0 and b"num_tensors" in grut_lib.grut_last_error()
    assert grut_lib.grut_mcmc_append_rows(None, one, None, 1, 4, 1, None, None, None, None, None) != 0 and b"outs" in grut_lib.grut_last_error()


def test_python_surface_rejects_bad_tensors_before_any_launch(monkeypatch):
    mcmc = _mcmc()

    def no_library(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(importlib.import_module("3dgrut_amd._abi"), "load_library", no_library)
    n, m = 8, 4
    f = torch.rand
    binoms = mer.binomial_table(51, "cpu")
    with pytest.raises(RuntimeError, match="density_act must be a CUDA tensor"):
        mcmc.classify_alive(f(n, 1), 0.005)
    with pytest.raises(RuntimeError, match="density_act must be float32"):
        mcmc.classify_alive(f(n, 1).double(), 0.005)
    with pytest.raises(RuntimeError, match="density_act must be contiguous"):
        mcmc.classify_alive(f(n, 2)[:, :1], 0.005)
    draws = torch.zeros(m, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        mcmc.sample_plan(draws, f(n, 1), f(n, 3), binoms, 51, 0.005)
    with pytest.raises(RuntimeError, match="sampled must be int64"):
        mcmc.sample_plan(draws.int(), f(n, 1), f(n, 3), binoms, 51, 0.005)
    with pytest.raises(RuntimeError, match="scale must be contiguous"):
        mcmc.sample_plan(draws, f(n, 1), f(3, n).t(), binoms, 51, 0.005)
    with pytest.raises(RuntimeError, match="index_map must be int64"):
        mcmc.sample_plan(draws, f(n, 1), f(n, 3), binoms, 51, 0.005, index_map=torch.zeros(n, dtype=torch.int32))
    plan = mcmc.SamplePlan(n, m, draws, torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), f(m, 1), f(m, 3), None, None)
    dead = torch.arange(m)
    for call in (lambda t, r: mcmc.relocate_rows_(t, r, plan, dead), lambda t, r: mcmc.append_rows(t, r, plan)):
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            call([f(n, 3)], [mcmc.ROLE_COPY])
        with pytest.raises(RuntimeError, match="must be float32"):
            call([f(n, 3).double()], [mcmc.ROLE_COPY])
        with pytest.raises(RuntimeError, match="must be contiguous"):
            call([f(3, n).t()], [mcmc.ROLE_STATE])
        with pytest.raises(RuntimeError, match="at most 32"):
            call([f(n, 3)] * 33, [mcmc.ROLE_COPY] * 33)
        with pytest.raises(RuntimeError, match="roles"):
            call([f(n, 3)], [mcmc.ROLE_COPY, mcmc.ROLE_STATE])


def _strategy_conf(print_stats=False):
    return _DictConfig({"strategy": {"binom_n_max": 51, "opacity_threshold": 0.005, "print_stats": print_stats,
                                     "add": {"max_n_gaussians": 10 ** 6}, "perturb": {"noise_lr": 5e5}}})


def _duck(n=400, seed=3):
    model = mer.DuckModel(n, "cpu", seed=seed)
    model.seed_optimizer_state()
    return model


@needs_reference
@pytest.mark.parametrize("order", ["events_first", "perturb_first"])
def test_install_fused_events_is_idempotent_and_stacks_with_the_fused_perturbation(reference, order):  # noqa: F811
    mcmc = _mcmc()
    importlib.import_module("threedgrut.model.model")       # imports the shims -> install()
    ref = importlib.import_module("threedgrut.strategy.mcmc")
    reference_class = ref.MCMCStrategy
    try:
        if order == "perturb_first":
            below = mcmc.install_fused_perturb()
            assert below is not reference_class
        else:
            below = reference_class
        fused = mcmc.install_fused_events()
        assert ref.MCMCStrategy is fused and fused is not below and fused.__mro__[1] is below and issubclass(fused, reference_class)
        assert mcmc.install_fused_events() is fused and ref.MCMCStrategy is fused
        top = mcmc.install_fused_perturb()
        assert ref.MCMCStrategy is top and issubclass(top, fused)
        assert (top is fused) == (order == "perturb_first")
        assert mcmc.install_fused_events() is top and mcmc.install_fused_perturb() is top
        # both overrides are live on the class the trainer will construct
        assert top._grut_fused_events and top._grut_fused_perturb
        for method in ("relocate_gaussians", "add_new_gaussians", "perturb_gaussians"):
            assert getattr(top, method) is not getattr(reference_class, method), method
            assert getattr(top, method).__module__ == mcmc.__name__
        for method in ("sample_new_gaussians", "_post_optimizer_step"):
            assert getattr(top, method) is getattr(reference_class, method)
    finally:
        ref.MCMCStrategy = reference_class


@needs_reference
def test_restatement_equals_the_reference_class_and_a_cpu_model_takes_the_reference_method(reference, monkeypatch, caplog):  # noqa: F811
    """Three identical CPU models and one seed: the reference's own class, the restatement, and the fused subclass (whose preconditions
    a CPU model fails: it must run the reference's method and count that).  One torch relocation function stands behind all three."""
    mcmc = _mcmc()
    importlib.import_module("threedgrut.model.model")
    ref = importlib.import_module("threedgrut.strategy.mcmc")
    reference_class = ref.MCMCStrategy
    ref.load_mcmc_plugin()
    monkeypatch.setattr(ref, "_mcmc_plugin", types.SimpleNamespace(compute_relocation_tensor=mer.torch_relocation))
    try:
        fused_class = mcmc.install_fused_events()
        conf = _strategy_conf()
        models = [_duck(), _duck(), _duck()]
        n = models[0].num_gaussians
        assert 0 < int((models[0].get_density() <= 0.005).sum()) < n // 4      # there are dead Gaussians to move
        runners = [reference_class(conf, models[0]), None, fused_class(conf, models[2])]
        restated = mer.RestatedMCMCEvents(models[1], threshold=0.005, n_max=51, max_n=10 ** 6, relocation=mer.torch_relocation,
                                          sampler=ref._multinomial_sample)
        events = [(runners[0].relocate_gaussians, runners[0].add_new_gaussians), (restated.relocate, restated.add),
                  (runners[2].relocate_gaussians, runners[2].add_new_gaussians)]
        before = types.SimpleNamespace(**vars(mcmc.stats))
        results = []
        for model, (relocate, add) in zip(models, events):
            old = [g["params"][0] for g in model.optimizer.param_groups]
            torch.manual_seed(21)
            relocate()
            after_relocate = mer.snapshot(model)
            add()
            results.append((after_relocate, mer.snapshot(model), torch.get_rng_state()))
            assert model.num_gaussians == int(1.05 * n)
            for g, p_old in zip(model.optimizer.param_groups, old):   # the update contract
                p = g["params"][0]
                assert p is not p_old and isinstance(p, torch.nn.Parameter) and p.requires_grad == p_old.requires_grad
                assert p_old not in model.optimizer.state and set(model.optimizer.state[p]) == {"step", "exp_avg", "exp_avg_sq"}
                assert float(model.optimizer.state[p]["step"]) == 7.0
        assert (mcmc.stats.torch_events, mcmc.stats.hip_relocations, mcmc.stats.hip_adds) == \
            (before.torch_events + 2, before.hip_relocations, before.hip_adds)
        moved = False
        for other in results[1:]:
            assert torch.equal(other[2], results[0][2])                     # the generator is where the reference leaves it
            for stage in (0, 1):
                assert list(other[stage]) == list(results[0][stage])        # the optimizer's groups, in order
                for name, (p, state) in results[0][stage].items():
                    q, state_q = other[stage][name]
                    assert p.shape == q.shape and torch.equal(p.view(torch.int32), q.view(torch.int32)), name
                    assert list(state) == list(state_q)
                    for key in state:
                        assert torch.equal(state[key], state_q[key]), (name, key)
        fresh = _duck()
        for name, (p, state) in results[0][0].items():
            moved |= not torch.equal(p, getattr(fresh, name).detach())
            assert bool(torch.isfinite(p).all())
        assert moved
    finally:
        ref.MCMCStrategy = reference_class


@needs_reference
def test_fused_events_keep_the_log_lines(reference, monkeypatch):  # noqa: F811
    """print_stats: the subclass logs what the reference logs (here through the fallback, which logs for itself: exactly one line each)."""
    mcmc = _mcmc()
    importlib.import_module("threedgrut.model.model")
    ref = importlib.import_module("threedgrut.strategy.mcmc")
    reference_class = ref.MCMCStrategy
    ref.load_mcmc_plugin()
    monkeypatch.setattr(ref, "_mcmc_plugin", types.SimpleNamespace(compute_relocation_tensor=mer.torch_relocation))
    lines = []
    monkeypatch.setattr(ref.logger, "info", lambda msg, *a, **k: lines.append(str(msg)))
    try:
        strategy = mcmc.install_fused_events()(_strategy_conf(print_stats=True), _duck())
        torch.manual_seed(1)
        strategy.relocate_gaussians()
        strategy.add_new_gaussians()
        assert len(lines) == 2 and re.match(r"Relocated \d+ \(\d+\.\d\d%\) gaussians", lines[0]) and lines[1] == "Added 20 (5.00%) gaussians"
        # and on its own path the subclass words them the same way
        lines.clear()
        record = types.SimpleNamespace(n_dead=3, n_added=20, n_before=400)
        monkeypatch.setattr(mcmc, "relocate", lambda *a, **k: record)
        monkeypatch.setattr(mcmc, "add", lambda *a, **k: record)
        strategy.relocate_gaussians()
        strategy.add_new_gaussians()
        assert lines == ["Relocated 3 (0.75%) gaussians", "Added 20 (5.00%) gaussians"]
    finally:
        ref.MCMCStrategy = reference_class
