"""GPU: the fused passes of the MCMC strategy's two periodic events (csrc/mcmc_events.hip, 3dgrut_amd/mcmc.py) against torch indexing,
against the restatement of tests/mcmc_events_reference.py from identical copies and one seed, and in the teacher-scene training loop
of tests/test_mcmc_gpu.py.

Bounds.  The activated values of the plan are held to the bounds of test_relocation_matches_restatements (same formula, same device
function).  The raw values y = log(x / (1 - x)) resp. log(s) are compared with float64 evaluated from the kernel's OWN fp32 activated
value (clamped as the kernel clamps it): at most two roundings in x / (1 - x) move the logarithm by 2u absolute, logf is within 1 ulp
<= 2u |y|; the bound is twice that sum, |delta| <= 4u (1 + |y|), u = 2^-24.  Everything that only moves rows is bitwise."""
import importlib

import numpy as np
import pytest

import mcmc_events_reference as mer
import oracle
from scenes import make_scene, torch_batch
from test_mcmc_gpu import U, _binoms, _psnr, _restate_denominator

pytestmark = pytest.mark.gpu
syn = importlib.import_module("workloads.synthetic")
INT32_MAX = 2 ** 31 - 1
THRESHOLD = 0.005


def _mcmc():
    return importlib.import_module("3dgrut_amd.mcmc")


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ---- classify ----------------------------------------------------------------------------------------------------------------------
# the scan's per-block span is 2048 items (kScanTile of scan_sort.hip): 70 001 rows are 35 of its blocks
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70_001])
def test_classify_matches_torch_where(n):
    import torch
    thr = float(np.float32(THRESHOLD))
    g = torch.Generator(device="cuda").manual_seed(n)
    mixed = torch.rand(n, 1, device="cuda", generator=g) * 0.02
    mixed[::7] = thr                                        # exactly at the threshold: dead
    mixed[3::11] = float("nan")                             # in neither list
    mixed[5::13] = float(np.nextafter(np.float32(thr), np.float32(1)))   # one ulp above: alive
    cases = {"mixed": mixed, "all_dead": torch.full((n, 1), 1e-3, device="cuda"), "all_alive": torch.full((n, 1), 0.7, device="cuda"),
             "all_nan": torch.full((n, 1), float("nan"), device="cuda"), "flat": mixed.reshape(-1).clone()}
    for name, d in cases.items():
        before = d.clone()
        dead, alive, prob = _mcmc().classify_alive(d, THRESHOLD)
        want_dead, want_alive = torch.where(d.reshape(-1, 1) <= THRESHOLD)[0], torch.where(d.reshape(-1, 1) > THRESHOLD)[0]
        assert dead.dtype == alive.dtype == torch.int64 and prob.dtype == torch.float32, name
        assert torch.equal(dead, want_dead) and torch.equal(alive, want_alive), name
        assert _same_bits(prob, d.reshape(-1, 1)[want_alive].flatten()), name
        assert _same_bits(d, before), name
        assert len(dead) + len(alive) == n - int(torch.isnan(d).sum()), name
    if n >= 255:
        dead, alive, _ = _mcmc().classify_alive(mixed, THRESHOLD)
        assert len(dead) > n // 7 and len(alive) > 0 and len(dead) + len(alive) < n
    e_dead, e_alive, e_prob = _mcmc().classify_alive(torch.empty(0, 1, device="cuda"), THRESHOLD)
    assert e_dead.shape == e_alive.shape == e_prob.shape == (0,)


# ---- plan --------------------------------------------------------------------------------------------------------------------------
def _plan_inputs(n, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    density = torch.rand(n, 1, device="cuda", generator=g) * 0.98 + 0.01
    density[:4, 0] = torch.tensor([0.0051, 1 - 1e-6, 0.5, 0.999], device="cuda")
    scale_raw = torch.randn(n, 3, device="cuda", generator=g) - 4.0
    return density, scale_raw


def _check_plan(plan, sampled, index_map, density, scale_act, n_max, raw_scale_input=False):
    """Everything a plan promises, for activated scales `scale_act` (what the kernel was given, or exp of it when it got raw ones)."""
    import torch
    n, m = density.shape[0], sampled.shape[0]
    source = sampled if index_map is None else index_map[sampled]
    assert plan.n == n and plan.m == m and plan.source.dtype == torch.int64 and torch.equal(plan.source, source)
    assert plan.count.dtype == torch.int32 and torch.equal(plan.count.long(), torch.bincount(source, minlength=n))
    first = torch.full((n,), INT32_MAX, dtype=torch.int64, device="cuda")
    first.scatter_reduce_(0, source, torch.arange(m, device="cuda"), "amin")
    assert plan.first.dtype == torch.int32 and torch.equal(plan.first.long(), first)
    assert plan.new_density_raw.shape == plan.new_density_act.shape == (m, 1) and plan.new_scale_raw.shape == plan.new_scale_act.shape == (m, 3)
    if m == 0:
        return
    # duplicates of a source: bit-identical values
    rep = plan.first.long()[source]
    for t in (plan.new_density_raw, plan.new_scale_raw, plan.new_density_act, plan.new_scale_act):
        assert _same_bits(t, t[rep])
    # activated values: the bounds of test_relocation_matches_restatements
    ratios = (plan.count.long()[source] + 1).clamp(1, n_max).cpu().numpy().astype(np.int32)
    o = density.reshape(-1)[source].cpu().numpy()
    scales = scale_act[source].cpu().numpy()
    new_o, new_s = plan.new_density_act.cpu().numpy()[:, 0], plan.new_scale_act.cpu().numpy()
    base = (np.float32(1) - o).astype(np.float64)
    expo = (np.float32(1) / ratios.astype(np.float32)).astype(np.float64)
    o64 = 1.0 - base ** expo
    assert np.all(np.abs(new_o - o64) <= 4 * U + 2 * U * np.abs(o64)), np.abs(new_o - o64).max()
    binoms = _binoms(n_max)
    d64, abs_terms, abs_partials = _restate_denominator(new_o, ratios, binoms, n_max, np.float64)
    s64 = (o.astype(np.float64) / d64)[:, None] * scales.astype(np.float64)
    rel64 = (U * (abs_partials + 8 * abs_terms) / np.abs(d64) + 4 * U)[:, None]
    if raw_scale_input:
        rel64 = rel64 + 2 * U      # the kernel's own expf of the raw scale: within 1 ulp <= 2u of exp
    err64 = np.abs(new_s - s64) / np.abs(s64)
    assert np.all(err64 <= rel64), float((err64 / rel64).max())
    # raw values: float64 from the kernel's own fp32 activated values
    x = np.minimum(np.maximum(new_o, np.float32(THRESHOLD)), np.float32(1) - np.finfo(np.float32).eps).astype(np.float64)
    y_d = np.log(x / (1.0 - x))
    y_s = np.log(new_s.astype(np.float64))
    raw_d, raw_s = plan.new_density_raw.cpu().numpy()[:, 0].astype(np.float64), plan.new_scale_raw.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(raw_d - y_d) <= 4 * U * (1 + np.abs(y_d))), float((np.abs(raw_d - y_d) / (4 * U * (1 + np.abs(y_d)))).max())
    assert np.all(np.abs(raw_s - y_s) <= 4 * U * (1 + np.abs(y_s))), float((np.abs(raw_s - y_s) / (4 * U * (1 + np.abs(y_s)))).max())


@pytest.mark.parametrize("case", ["m0", "m1", "clamped", "unmapped", "raw_scale"])
def test_sample_plan_counts_first_and_values(case):
    import torch
    n = 300
    density, scale_raw = _plan_inputs(n, seed=17)
    scale_act = torch.exp(scale_raw)
    g = torch.Generator(device="cuda").manual_seed(3)
    n_max, index_map = 51, None
    if case == "m0":
        sampled = torch.empty(0, dtype=torch.int64, device="cuda")
    elif case == "m1":
        sampled = torch.tensor([n - 1], device="cuda")
    elif case == "clamped":                                   # m = 3 N over 5 alive rows: counts of ~180 against a table of 10
        n_max = 10
        index_map = torch.tensor([0, 1, 2, 150, n - 1], device="cuda")
        sampled = torch.randint(0, 5, (3 * n,), device="cuda", generator=g)
    else:
        sampled = torch.randint(0, n, (1000,), device="cuda", generator=g)
    binoms = torch.as_tensor(_binoms(n_max), dtype=torch.float32, device="cuda")
    raw = case == "raw_scale"
    keep = [t.clone() for t in (sampled, density, scale_raw, scale_act)]
    plan = _mcmc().sample_plan(sampled, density, scale_raw if raw else scale_act, binoms, n_max, THRESHOLD, index_map=index_map,
                               scale_activated=not raw)
    for a, b in zip((sampled, density, scale_raw, scale_act), keep):
        assert torch.equal(a, b)
    _check_plan(plan, sampled, index_map, density, scale_act, n_max, raw_scale_input=raw)
    if case == "clamped":
        assert int(plan.count.max()) > 10 * n_max and int((plan.count > 0).sum()) == 5
    if case == "m1":
        assert int(plan.count[n - 1]) == 1 and int(plan.count.sum()) == 1 and int(plan.first[n - 1]) == 0
    # without the activated outputs: the same raw values
    lean = _mcmc().sample_plan(sampled, density, scale_raw if raw else scale_act, binoms, n_max, THRESHOLD, index_map=index_map,
                               scale_activated=not raw, with_activated=False)
    assert lean.new_density_act is None and lean.new_scale_act is None
    assert _same_bits(lean.new_density_raw, plan.new_density_raw) and _same_bits(lean.new_scale_raw, plan.new_scale_raw)


# ---- rows --------------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 3, 4, 16, 45)
ROWS = 701          # 701 w is no multiple of 4 for w = 1, 3, 45 (the words after the last whole 16 bytes) and several blocks for w = 45


def _row_tensors(seed, misaligned=False):
    """A COPY and a STATE tensor of every width, the density [.,1] and the scale [.,3]; misaligned: every base 4 bytes off 16."""
    import torch
    mcmc = _mcmc()
    g = torch.Generator(device="cuda").manual_seed(seed)
    tensors, roles = [], []

    def make(w):
        if not misaligned:
            return torch.randn(ROWS, w, device="cuda", generator=g)
        return torch.randn(ROWS * w + 1, device="cuda", generator=g)[1:].view(ROWS, w)

    for w in WIDTHS:
        tensors += [make(w), make(w)]
        roles += [mcmc.ROLE_COPY, mcmc.ROLE_STATE]
    tensors += [make(1), make(3)]
    roles += [mcmc.ROLE_NEW_DENSITY, mcmc.ROLE_NEW_SCALE]
    assert all(t.is_contiguous() and (t.data_ptr() % 16 == 4) == misaligned for t in tensors)
    return tensors, roles


def _hand_plan(source, n):
    """A plan with the lists given explicitly; duplicates of a source share their new values, as a plan guarantees."""
    import torch
    mcmc = _mcmc()
    m = source.shape[0]
    first = torch.full((n,), INT32_MAX, dtype=torch.int64, device="cuda")
    first.scatter_reduce_(0, source, torch.arange(m, device="cuda"), "amin")
    g = torch.Generator(device="cuda").manual_seed(m)
    per_row_d, per_row_s = torch.randn(n, 1, device="cuda", generator=g), torch.randn(n, 3, device="cuda", generator=g)
    return mcmc.SamplePlan(n, m, source, torch.bincount(source, minlength=n).int(), first.int(), per_row_d[source].contiguous(),
                           per_row_s[source].contiguous(), None, None)


def _row_cases():
    import torch
    g = torch.Generator(device="cuda").manual_seed(9)
    perm = torch.randperm(ROWS, device="cuda", generator=g)
    few = perm[:5]                                                         # 5 alive rows ...
    return {"m0": (torch.empty(0, dtype=torch.int64, device="cuda"), perm[:0].clone()),
            "duplicates": (perm[torch.randint(0, 60, (90,), device="cuda", generator=g)], perm[100:190].clone()),
            "more_than_alive": (few[torch.randint(0, 5, (40,), device="cuda", generator=g)], perm[5:45].clone())}   # ... drawn 40 times


@pytest.mark.parametrize("misaligned", [False, True])
def test_relocate_rows_match_torch_indexing(misaligned):
    import torch
    mcmc = _mcmc()
    for name, (source, dead) in _row_cases().items():
        plan = _hand_plan(source, ROWS)
        tensors, roles = _row_tensors(seed=1, misaligned=misaligned)
        want = []
        for t, role in zip(tensors, roles):
            w = t.clone()
            if role == mcmc.ROLE_STATE:
                w[source] = 0
            else:
                if role == mcmc.ROLE_NEW_DENSITY:
                    w[source] = plan.new_density_raw
                elif role == mcmc.ROLE_NEW_SCALE:
                    w[source] = plan.new_scale_raw
                w[dead] = w[source]
            want.append(w)
        again = [t.clone() for t in tensors]
        out = mcmc.relocate_rows_(tensors, roles, plan, dead)
        assert all(a is b for a, b in zip(out, tensors))                     # in place
        mcmc.relocate_rows_(again, roles, plan, dead)
        for k, (t, w, a) in enumerate(zip(tensors, want, again)):
            assert _same_bits(t, w), (name, k, roles[k], tuple(t.shape))
            assert _same_bits(t, a), (name, k)


@pytest.mark.parametrize("misaligned", [False, True])
def test_append_rows_match_torch_cat(misaligned):
    import torch
    mcmc = _mcmc()
    for name, (source, _) in _row_cases().items():
        plan = _hand_plan(source, ROWS)
        tensors, roles = _row_tensors(seed=2, misaligned=misaligned)
        keep = [t.clone() for t in tensors]
        want = []
        for t, role in zip(tensors, roles):
            if role == mcmc.ROLE_STATE:
                want.append(torch.cat([t, torch.zeros((len(source), t.shape[1]), device="cuda")]))
                continue
            w = t.clone()
            if role == mcmc.ROLE_NEW_DENSITY:
                w[source] = plan.new_density_raw
            elif role == mcmc.ROLE_NEW_SCALE:
                w[source] = plan.new_scale_raw
            want.append(torch.cat([w, w[source]]))
        out = mcmc.append_rows(tensors, roles, plan)
        again = mcmc.append_rows(tensors, roles, plan)
        for k, (o, w, a, t, t0) in enumerate(zip(out, want, again, tensors, keep)):
            assert _same_bits(o, w), (name, k, roles[k], tuple(o.shape))
            assert _same_bits(o, a) and o.data_ptr() != a.data_ptr() and _same_bits(t, t0), (name, k)


def test_row_passes_reject_what_they_cannot_take():
    import torch
    mcmc = _mcmc()
    source, dead = _row_cases()["duplicates"]
    plan = _hand_plan(source, ROWS)
    t3 = torch.zeros(ROWS, 3, device="cuda")
    with pytest.raises(RuntimeError, match="role needs 1"):
        mcmc.append_rows([t3], [mcmc.ROLE_NEW_DENSITY], plan)
    with pytest.raises(RuntimeError, match="must have 701 rows"):
        mcmc.append_rows([t3[:-1]], [mcmc.ROLE_COPY], plan)
    with pytest.raises(RuntimeError, match="dead_idx has"):
        mcmc.relocate_rows_([t3], [mcmc.ROLE_COPY], plan, dead[:-1])
    with pytest.raises(RuntimeError, match="contiguous"):
        mcmc.relocate_rows_([torch.zeros(3, ROWS, device="cuda").t()], [mcmc.ROLE_COPY], plan, dead)
    abi = importlib.import_module("3dgrut_amd._abi")
    lib = abi.load_library()
    bad = (abi.McmcTensor * 1)(abi.McmcTensor(t3.data_ptr(), 3, mcmc.ROLE_NEW_DENSITY))
    assert lib.grut_mcmc_relocate_rows(None, bad, 1, 4, source.data_ptr(), dead.data_ptr(), plan.first.data_ptr(), None, None) != 0
    assert b"NEW_DENSITY" in lib.grut_last_error()
    ok = (abi.McmcTensor * 1)(abi.McmcTensor(t3.data_ptr(), 3, mcmc.ROLE_COPY))
    assert lib.grut_mcmc_relocate_rows(None, ok, 1, 4, None, dead.data_ptr(), plan.first.data_ptr(), None, None) != 0
    assert b"source" in lib.grut_last_error()
    assert lib.grut_mcmc_relocate_rows(None, ok, 1, 0, None, None, None, None, None) == 0     # no draws: nothing launched
    assert bool((t3 == 0).all())


# ---- events ------------------------------------------------------------------------------------------------------------------------
N_EVENT = 3001


def _event_models(seeded=True, frozen=None):
    import torch
    a = mer.DuckModel(N_EVENT, "cuda", seed=4)
    a.density.data[::9] = -7.0                      # sigmoid(-7) = 9e-4: dead
    if seeded:
        a.seed_optimizer_state()
    if frozen:
        getattr(a, frozen).requires_grad_(False)
    return a, mer.clone_model(a)


def _restated(model, max_n=10 ** 9):
    return mer.RestatedMCMCEvents(model, threshold=THRESHOLD, n_max=51, max_n=max_n, relocation=_mcmc().compute_relocation_tensor)


def _check_contract(model, old_params, seeded):
    import torch
    opt = model.optimizer
    assert len(opt.state) == len(opt.param_groups)
    for g, old in zip(opt.param_groups, old_params):
        p = g["params"][0]
        assert isinstance(p, torch.nn.Parameter) and p is not old and p.requires_grad == old.requires_grad and getattr(model, g["name"]) is p
        assert old not in opt.state and p in opt.state
        state = opt.state[p]
        assert set(state) == ({"step", "exp_avg", "exp_avg_sq"} if seeded else set())
        if seeded:
            assert float(state["step"]) == 7.0 and state["exp_avg"].shape == p.shape == state["exp_avg_sq"].shape


def _compare_models(a, b, touched, new_rows):
    """Bitwise equal parameters and moments, except density / scale at `touched`, which hold `new_rows` = {name: (rows, values)}."""
    import torch
    sa, sb = mer.snapshot(a), mer.snapshot(b)
    assert list(sa) == list(sb)
    for name in sa:
        (p, state), (q, state_q) = sa[name], sb[name]
        assert p.shape == q.shape and list(state) == list(state_q), name
        for key in state:
            assert _same_bits(state[key], state_q[key]) if key != "step" else torch.equal(state[key], state_q[key]), (name, key)
        if name in ("density", "scale"):
            same = torch.ones(p.shape[0], dtype=torch.bool, device="cuda")
            same[touched] = False
            assert _same_bits(p[same], q[same]), name
            rows, values = new_rows[name]
            assert _same_bits(p[rows], values), name
            # and within twice the plan's bound of what the torch chain computes: both are within 4u (1 + |y|) of the exact logarithm
            d = (p[touched].double() - q[touched].double()).abs()
            assert bool((d <= 8 * U * (1 + q[touched].double().abs())).all()), (name, float(d.max()))
        else:
            assert _same_bits(p, q), name


@pytest.mark.parametrize("seeded", [True, False])
def test_relocate_event_matches_the_restatement(seeded):
    import torch
    mcmc = _mcmc()
    a, b = _event_models(seeded, frozen="features_albedo")
    binoms = mer.binomial_table(51, "cuda")
    old = [g["params"][0] for g in a.optimizer.param_groups]
    ptrs = [p.data_ptr() for p in old]
    before = mcmc.stats.hip_relocations
    torch.manual_seed(77)
    rec = mcmc.relocate(a, THRESHOLD, binoms, 51)
    state_a = torch.cuda.get_rng_state()
    torch.manual_seed(77)
    ref = _restated(b).relocate()
    assert torch.equal(state_a, torch.cuda.get_rng_state())
    assert mcmc.stats.hip_relocations == before + 1
    assert rec.n_dead == ref["n_dead"] >= N_EVENT // 9 and rec.n_added == 0 and rec.n_before == rec.n_after == N_EVENT
    assert torch.equal(rec.dead_idx, ref["dead"]) and torch.equal(rec.source, ref["picks"].long())
    assert torch.equal(rec.count.long(), torch.bincount(rec.source, minlength=N_EVENT))
    assert int(rec.count.max()) > 1                                           # duplicates occurred
    _check_contract(a, old, seeded)
    assert [g["params"][0].data_ptr() for g in a.optimizer.param_groups] == ptrs    # in place: the new Parameters share the storage
    touched = torch.cat([rec.source, rec.dead_idx])
    new_rows = {"density": (touched, torch.cat([rec.new_density_raw, rec.new_density_raw])),
                "scale": (touched, torch.cat([rec.new_scale_raw, rec.new_scale_raw]))}
    _compare_models(a, b, touched, new_rows)
    assert bool((a.get_density() > THRESHOLD - 4e-9).all())                  # nothing is dead any more


@pytest.mark.parametrize("seeded", [True, False])
def test_add_event_matches_the_restatement(seeded):
    import torch
    mcmc = _mcmc()
    a, b = _event_models(seeded, frozen="rotation")
    binoms = mer.binomial_table(51, "cuda")
    old = [g["params"][0] for g in a.optimizer.param_groups]
    before = mcmc.stats.hip_adds
    torch.manual_seed(78)
    rec = mcmc.add(a, 10 ** 9, THRESHOLD, binoms, 51)
    state_a = torch.cuda.get_rng_state()
    torch.manual_seed(78)
    ref = _restated(b).add()
    assert torch.equal(state_a, torch.cuda.get_rng_state())
    assert mcmc.stats.hip_adds == before + 1
    num = int(1.05 * N_EVENT) - N_EVENT
    assert rec.n_added == ref["n_added"] == num and rec.n_dead == 0 and rec.n_before == N_EVENT and rec.n_after == N_EVENT + num
    assert a.num_gaussians == b.num_gaussians == N_EVENT + num
    assert torch.equal(rec.source, ref["picks"].long())
    _check_contract(a, old, seeded)
    appended = torch.arange(N_EVENT, N_EVENT + num, device="cuda")
    touched = torch.cat([rec.source, appended])
    new_rows = {"density": (touched, torch.cat([rec.new_density_raw, rec.new_density_raw])),
                "scale": (touched, torch.cat([rec.new_scale_raw, rec.new_scale_raw]))}
    _compare_models(a, b, touched, new_rows)
    # capped by max_n
    rec = mcmc.add(a, a.num_gaussians + 3, THRESHOLD, binoms, 51)
    assert rec.n_added == 3 and a.num_gaussians == N_EVENT + num + 3


def test_events_draw_nothing_when_there_is_nothing_to_do():
    import torch
    mcmc = _mcmc()
    a, _ = _event_models()
    a.density.data.fill_(2.0)
    binoms = mer.binomial_table(51, "cuda")
    old = [g["params"][0] for g in a.optimizer.param_groups]

    def no_draw(*args, **kwargs):
        raise AssertionError("the sampler was called")

    torch.manual_seed(5)
    state = torch.cuda.get_rng_state()
    rec = mcmc.relocate(a, THRESHOLD, binoms, 51, sampler=no_draw)
    assert rec.n_dead == 0 and rec.source is None and rec.n_after == N_EVENT
    rec = mcmc.add(a, N_EVENT, THRESHOLD, binoms, 51, sampler=no_draw)
    assert rec.n_added == 0 and rec.n_after == N_EVENT
    assert torch.equal(state, torch.cuda.get_rng_state())
    assert [g["params"][0] for g in a.optimizer.param_groups] == old         # nothing was rebuilt, as in the reference
    # the sampler is called once, with the reference's arguments
    calls = []

    def sampler(p, num, replacement):
        calls.append((p.clone(), num, replacement))
        return torch.multinomial(p, num, replacement=replacement)

    a.density.data[:10] = -7.0
    mcmc.relocate(a, THRESHOLD, binoms, 51, sampler=sampler)
    mcmc.add(a, 10 ** 9, THRESHOLD, binoms, 51, sampler=sampler)
    assert len(calls) == 2 and calls[0][1:] == (10, True) and calls[1][1:] == (int(1.05 * N_EVENT) - N_EVENT, True)
    assert calls[0][0].shape == (N_EVENT - 10,) and calls[1][0].shape == (N_EVENT,)


def test_a_model_the_passes_cannot_take_runs_the_replaced_path():
    import torch
    mcmc = _mcmc()
    a, b = _event_models()
    for m in (a, b):                                       # not the default activation: the kernels' sigmoid would be wrong
        m.density_activation = lambda x: torch.sigmoid(x) * 0.999
        m.density_activation_inv = lambda y: torch.log((y / 0.999) / (1 - y / 0.999))
    binoms = mer.binomial_table(51, "cuda")
    before = (mcmc.stats.torch_events, mcmc.stats.hip_relocations, mcmc.stats.hip_adds)
    torch.manual_seed(3)
    rec_r = mcmc.relocate(a, THRESHOLD, binoms, 51)
    rec_a = mcmc.add(a, 10 ** 9, THRESHOLD, binoms, 51)
    state_a = torch.cuda.get_rng_state()
    torch.manual_seed(3)
    restated = _restated(b)
    ref_r, ref_a = restated.relocate(), restated.add()
    assert torch.equal(state_a, torch.cuda.get_rng_state())
    assert (mcmc.stats.torch_events, mcmc.stats.hip_relocations, mcmc.stats.hip_adds) == (before[0] + 2, before[1], before[2])
    assert rec_r.n_dead == ref_r["n_dead"] > 0 and rec_a.n_added == ref_a["n_added"] > 0
    sa, sb = mer.snapshot(a), mer.snapshot(b)
    for name in sa:
        assert _same_bits(sa[name][0], sb[name][0]), name
        for key in sa[name][1]:
            assert torch.equal(sa[name][1][key], sb[name][1][key]), (name, key)
    called = []
    mcmc.relocate(a, THRESHOLD, binoms, 51, fallback=lambda: called.append("relocate"))
    mcmc.add(a, 10 ** 9, THRESHOLD, binoms, 51, fallback=lambda: called.append("add"))
    assert called == ["relocate", "add"]


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_mcmc_training_with_the_fused_events_recovers_a_teacher_scene():
    """The teacher-scene loop of test_mcmc_training_recovers_a_teacher_scene (3DGUT, same sizes, seed and 150 steps) with relocate() /
    add() of the product in place of that test's torch _Strategy, and the same assertions."""
    import torch
    mcmc = _mcmc()
    n, w, h, views = 600, 48, 48, 3
    scenes = [make_scene(n=n, width=w, height=h, median_scale=0.09, seed=5, view=v, max_density=0.9) for v in range(views)]
    d12, sph = scenes[0]["density12"], scenes[0]["sph"]

    def oracle_images(d12_, sph_):
        imgs = []
        for s in scenes:
            f = oracle.gut_forward(oracle.default_gut_config(), s["cam"], s["pose_start"], s["pose_end"], 3, d12_, sph_, *s["rays"])
            imgs.append(f["feat_density"][..., :3])
        return np.stack(imgs)

    teacher = oracle_images(d12, sph)
    rng = np.random.default_rng(9)
    d12_0, sph_0 = d12.copy(), sph.copy()
    d12_0[:, 0:3] += rng.normal(size=(n, 3)).astype(np.float32) * 0.02
    d12_0[:, 8:11] *= np.exp(rng.normal(size=(n, 3)) * 0.3).astype(np.float32)
    sph_0[:, :3] += rng.normal(size=(n, 3)).astype(np.float32) * 0.4
    sph_0[:, 3:] = 0
    d12_0[::10, 3] = 0.002                                              # some dead Gaussians for the first relocation to move
    psnr_before = _psnr(oracle_images(d12_0, sph_0), teacher)

    tracer = importlib.import_module("3dgrut_amd.gut_tracer").Tracer({"render": {"splat": {}}})
    g = syn.ActivatedGaussians(d12_0, sph_0)
    opt_mod = importlib.import_module("3dgrut_amd.optimizers")
    names = ["positions", "density", "rotation", "scale", "features_albedo", "features_specular"]
    lrs = [2e-3, 2e-2, 2e-3, 1e-2, 2e-2, 2e-3]
    opt = opt_mod.SelectiveAdam([{"params": [p], "lr": lr, "name": nm} for p, lr, nm in zip(g.parameters(), lrs, names)], eps=1e-15)
    g.optimizer = opt
    threshold, n_max, max_n = 0.005, 51, 100_000
    binoms = mer.binomial_table(n_max, "cuda")
    batches = [torch_batch(s["batch"], "cuda") for s in scenes]
    target = torch.as_tensor(teacher, device="cuda")
    torch.manual_seed(0)
    relocated, sizes = 0, [g.num_gaussians]
    events_before = (mcmc.stats.hip_relocations, mcmc.stats.hip_adds, mcmc.stats.torch_events)
    for it in range(150):
        v = it % views
        for p in g.parameters():                                         # (the events rebind them)
            p.grad = None
        tracer.build_acc(g, rebuild=True)
        out = tracer.render(g, batches[v], train=True)
        loss = ((out["pred_features"][0] - target[v]) ** 2).mean()
        loss.backward()
        opt.step(out["mog_visibility"])
        if it % 25 == 0:                                                 # mcmc.py:79-94 order: relocate, add, perturb
            relocated += mcmc.relocate(g, threshold, binoms, n_max).n_dead
            assert bool((g.get_density() > threshold - 4e-9).all())
            cur = g.num_gaussians
            added = mcmc.add(g, max_n, threshold, binoms, n_max).n_added
            assert added == min(max_n, int(1.05 * cur)) - cur and g.num_gaussians == cur + added
            sizes.append(g.num_gaussians)
        mcmc.perturb_gaussians(g, noise_lr=5e3)
        assert bool(torch.isfinite(g.positions).all())
    torch.cuda.synchronize()
    # every event ran on the HIP passes
    assert (mcmc.stats.hip_relocations, mcmc.stats.hip_adds, mcmc.stats.torch_events) == \
        (events_before[0] + 6, events_before[1] + 6, events_before[2])
    assert relocated >= n // 10 and sizes[-1] > sizes[0]
    d12_1, sph_1 = g.packed()
    assert np.isfinite(d12_1).all() and np.isfinite(sph_1).all()
    psnr_after = _psnr(oracle_images(d12_1, sph_1), teacher)
    print(f"3dgut: MCMC training with the fused events, N {sizes}, relocated {relocated}; PSNR vs oracle-rendered teacher "
          f"{psnr_before:.2f} dB -> {psnr_after:.2f} dB")
    assert psnr_after > psnr_before + 6.0, (psnr_before, psnr_after)

