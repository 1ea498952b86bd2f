"""GPU: the default strategy's device passes (csrc/densify.hip through 3dgrut_amd/densify.py) against the plain-torch / float64
restatement of tests/densify_reference.py.  Sizes: one thread, a partial wave, one element past the 2048-wide scan tile, and a
multi-tile scan with a ragged end."""
import importlib

import pytest
import torch

import densify_reference as ref

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 2049, 100_003)


@pytest.fixture(scope="module")
def densify(grut_lib):
    return importlib.import_module("3dgrut_amd.densify")


def _cpu_gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- 1. accumulate -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_accumulate_matches_float64_and_leaves_other_rows_alone(densify, n):
    """Each increment passes through at most 16 fp32 roundings (3 subtractions, two 3-term norms with their roots, 3 products, the
    halving, the final add): relative to the accumulated value the difference to float64 is bounded by 16 * 2^-24 ~ 1e-6; 2e-6 allowed."""
    g = _cpu_gen(n)
    dev = "cuda"
    grad = torch.randn((n, 3), generator=g) * 1e-3
    grad[torch.rand(n, generator=g) < 0.4] = 0                      # 40 % of the rows without gradient
    last_only, nan_row = (n // 2, n // 3) if n > 2 else (0, None)
    grad[last_only] = torch.tensor([0.0, 0.0, 3e-4])               # only the last component
    if nan_row is not None and nan_row != last_only:
        grad[nan_row] = torch.tensor([0.0, float("nan"), 0.0])
    else:
        nan_row = None
    grad = grad.to(dev)
    positions = (torch.randn((n, 3), generator=g) * 3).to(dev)
    pose = torch.eye(4).repeat(2, 1, 1)
    pose[0, :3, 3] = torch.tensor([0.3, -1.2, 2.5])
    sensor = pose.to(dev)[0, :3, 3]                                 # the trainer's view: stride 4
    assert sensor.stride(0) == 4
    accum0 = (torch.rand((n, 1), generator=g) * 5e-3).to(dev)        # accumulators that start non-zero
    denom0 = torch.randint(0, 9, (n, 1), generator=g, dtype=torch.int32).to(dev)
    want_acc, want_den = ref.accumulate_reference(accum0, denom0, grad, positions, sensor, torch.float64)
    ctrl_acc, ctrl_den = ref.accumulate_reference(accum0, denom0, grad, positions, sensor, torch.float32)
    idx_acc, idx_den = accum0.clone(), denom0.clone()
    ref.accumulate_indexed_(idx_acc, idx_den, grad, positions, sensor)          # the benchmark's baseline computes the same thing
    assert torch.equal(idx_den, want_den) and torch.allclose(idx_acc, ctrl_acc, rtol=1e-6, atol=0, equal_nan=True)
    accum, denom = accum0.clone(), denom0.clone()
    densify.accumulate_grad_stats_(accum, denom, grad, positions, sensor)
    has = (grad != 0).any(dim=1)
    finite = has.clone()
    if nan_row is not None:
        finite[nan_row] = False
        assert bool(accum[nan_row].isnan()) and int(denom[nan_row]) == int(denom0[nan_row]) + 1   # NaN counts as a gradient
    bound = 2e-6 * want_acc.abs()
    err_ctrl = (ctrl_acc.double() - want_acc).abs()
    err = (accum.double() - want_acc).abs()
    print(f"n={n}: max err / bound: torch fp32 {float((err_ctrl / bound)[finite].max()):.3f}, fused {float((err / bound)[finite].max()):.3f}")
    assert bool((err_ctrl <= bound)[finite].all()), "the fp32 restatement misses the bound: the inputs are wrong"
    assert bool((err <= bound)[finite].all())
    assert torch.equal(denom, want_den) and torch.equal(ctrl_den, want_den)
    assert torch.equal(accum[~has].view(torch.int32), accum0[~has].view(torch.int32))            # bit-identical
    assert torch.equal(denom[~has], denom0[~has])
    assert int(has.sum()) < n or n < 3


# ---- 2. relayout -------------------------------------------------------------------------------------------------------------------
def _masks(n, g):
    f, t = torch.zeros(n, dtype=torch.bool), torch.ones(n, dtype=torch.bool)
    r1, r2 = torch.rand(n, generator=g) < 0.6, torch.rand(n, generator=g) < 0.3
    return {"all-false": (f, f), "all-true": (t, t), "random": (r1, r2), "split": (~r2, r2), "keep-none": (None, r2),
            "append-none": (r1, None), "both-none": (None, None), "append-only": (f, r2)}


@pytest.mark.parametrize("n", SIZES)
def test_relayout_is_bit_exact(densify, n):
    g = _cpu_gen(100 + n)
    dev = "cuda"
    tensors = []
    for width in (1, 3, 4, 45):
        tensors.append(torch.randn((n, width), generator=g).to(dev))
        tensors.append(torch.randint(-2 ** 31, 2 ** 31 - 1, (n, width), generator=g, dtype=torch.int64).to(torch.int32).to(dev))
    tensors.append(torch.randn(n, generator=g).to(dev))            # a 1-D tensor is a row of one element
    tensors.append(torch.randn((n, 5, 2), generator=g).to(dev))    # a width without a specialised kernel, more than two dimensions
    zero = {1, 2, 5, 6, 9}
    for kind, (keep, append) in _masks(n, g).items():
        keep = keep.to(dev) if keep is not None else None
        append = append.to(dev) if append is not None else None
        for copies in (1, 2):
            out, n_keep, n_append = densify.relayout(tensors, keep=keep, append=append, copies=copies, zero_append=zero)
            assert n_keep == (n if keep is None else int(keep.sum())) and n_append == (0 if append is None else int(append.sum())), kind
            for j, (t, o) in enumerate(zip(tensors, out)):
                want = ref.relayout_reference(t, keep, append, copies, zero=j in zero)
                assert o.dtype == t.dtype and o.shape == want.shape and o.is_contiguous(), (kind, copies, j)
                assert torch.equal(o.view(torch.int32), want.view(torch.int32)), (kind, copies, j)


def test_relayout_of_zero_rows_launches_nothing(densify, grut_lib, monkeypatch):
    launches = []
    real = grut_lib.grut_relayout_rows
    monkeypatch.setattr(grut_lib, "grut_relayout_rows", lambda *a: launches.append(a) or real(*a))
    v = torch.randn((63, 3), device="cuda")
    none = torch.zeros(63, dtype=torch.bool, device="cuda")
    out, n_keep, n_append = densify.relayout([v], keep=none, append=none, copies=2)
    assert (n_keep, n_append) == (0, 0) and out[0].shape == (0, 3) and not launches
    out, n_keep, n_append = densify.relayout([v[:0]], keep=none[:0])
    assert (n_keep, n_append) == (0, 0) and out[0].shape == (0, 3) and not launches
    out, _, _ = densify.relayout([v], keep=~none)
    assert len(launches) == 1 and torch.equal(out[0], v)


def test_input_checks_on_device_tensors(densify):
    v = torch.randn((8, 3), device="cuda")
    with pytest.raises(RuntimeError, match="contiguous"):
        densify.relayout([v.t()])
    with pytest.raises(RuntimeError, match="float32 or int32"):
        densify.relayout([v.half()])
    with pytest.raises(RuntimeError, match="must have 8 rows"):
        densify.relayout([v, v[:4]])
    with pytest.raises(RuntimeError, match="bool"):
        densify.relayout([v], keep=torch.ones(8, device="cuda"))
    with pytest.raises(RuntimeError, match="noise"):
        densify.split_tail_(v.clone(), v.clone(), torch.randn((8, 4), device="cuda"), torch.randn((3, 3), device="cuda"), 4, 2)


# ---- 3. split tail -----------------------------------------------------------------------------------------------------------------
def _split_inputs(m, seed, dev="cuda"):
    g = _cpu_gen(seed)
    rotation = torch.nn.functional.normalize(torch.randn((m, 4), generator=g)) * (0.1 + 9.9 * torch.rand((m, 1), generator=g))
    return ((torch.randn((m, 3), generator=g) * 2).to(dev), (-8 * torch.rand((m, 3), generator=g)).to(dev), rotation.to(dev),
            torch.randn((m, 3), generator=g).to(dev))


@pytest.mark.parametrize("copies", (2, 3))
@pytest.mark.parametrize("n", SIZES)
def test_split_tail_matches_float64(densify, n, copies):
    """Scale: |diff| <= 1e-6 (three roundings and two <= 2-ulp library calls at |s| <= 8).  Positions, per component:
    2^-24 |p| + 64 2^-24 max|noise * sigma| of the row."""
    n_keep, m = 5, n * copies
    positions, scale, rotation, noise = _split_inputs(n_keep + m, 7 * n + copies)
    noise = noise[n_keep:].contiguous()
    want_pos, want_scale, smax = ref.split_tail_reference(positions[n_keep:], scale[n_keep:], rotation[n_keep:], noise, copies, torch.float64)
    ctrl_pos, ctrl_scale, _ = ref.split_tail_reference(positions[n_keep:], scale[n_keep:], rotation[n_keep:], noise, copies, torch.float32)
    pos, scl = positions.clone(), scale.clone()
    densify.split_tail_(pos, scl, rotation, noise, n_keep, copies)
    assert torch.equal(pos[:n_keep], positions[:n_keep]) and torch.equal(scl[:n_keep], scale[:n_keep])     # the kept rows are not touched
    bound = ref.split_position_bound(want_pos, smax)
    e_ctrl, e = (ctrl_pos.double() - want_pos).abs() / bound, (pos[n_keep:].double() - want_pos).abs() / bound
    s_ctrl, s = (ctrl_scale.double() - want_scale).abs().max(), (scl[n_keep:].double() - want_scale).abs().max()
    print(f"n={n} copies={copies}: positions err / bound: torch fp32 {float(e_ctrl.max()):.3f}, fused {float(e.max()):.3f}; "
          f"scale abs err: torch fp32 {float(s_ctrl):.2e}, fused {float(s):.2e}")
    assert float(e_ctrl.max()) <= 1 and float(s_ctrl) <= 1e-6, "the fp32 restatement misses the bound: the inputs are wrong"
    assert float(e.max()) <= 1
    assert float(s) <= 1e-6
    # the offsets were scaled by the OLD sigma: with sigma / (0.8 copies) instead, the row's offset would shrink by 1.6x / 2.4x
    late, _, _ = ref.split_tail_reference(positions[n_keep:], want_scale, rotation[n_keep:], noise, copies, torch.float64)
    big = (late - want_pos).abs() > 4 * bound
    assert bool(big.any()) and bool(((pos[n_keep:].double() - late).abs() > bound)[big].all())


# ---- 4. generator and 5. the strategy end to end --------------------------------------------------------------------------------------
def _fused_class(densify):
    class Fused(densify.FusedGSStrategyMixin, ref.RestatedGSStrategy):
        pass
    return Fused


def _pair(densify, n, optimizer="adam", split_n=2):
    models = [ref.DuckModel(n, "cuda", seed=3, optimizer=optimizer) for _ in range(2)]
    for m in models:
        m.seed_optimizer_state()
    conf = ref.make_conf(split_n=split_n)
    return (ref.RestatedGSStrategy(conf, models[0]), _fused_class(densify)(conf, models[1])), models


def _snapshot(model, norm):
    return {"positions": model.positions.data.clone(), "scale": model.scale.data.clone(), "rotation": model.rotation.data.clone(), "norm": norm.clone()}


def _assert_split_within_bounds(models, pre, copies, seed):
    """Both models against the float64 restatement of the split over the recorded pre-split tensors, with the noise that
    torch.randn draws after the same seeding: relaid rows bit-exact, tails of positions / scale within the bounds of test 3.  The
    restated strategy (torch.normal) is the control: if it misses, randn does not draw torch.normal's samples."""
    n0 = pre["positions"].shape[0]
    norm = torch.zeros(n0, device="cuda")
    norm[: pre["norm"].shape[0]] = pre["norm"]
    mask = (norm >= 2e-4) & (torch.exp(pre["scale"]).amax(dim=1) > 0.01)
    m = copies * int(mask.sum())
    assert 0 < m < copies * n0
    torch.manual_seed(seed)
    noise = torch.randn((m, 3), device="cuda")
    src = [pre[k][mask].repeat(copies, 1) for k in ("positions", "scale", "rotation")]
    want_pos, want_scale, smax = ref.split_tail_reference(*src, noise, copies, torch.float64)
    bound = ref.split_position_bound(want_pos, smax)
    head = n0 - m // copies
    for label, model in zip(("torch.normal restatement", "fused"), models):
        assert model.num_gaussians == head + m, label
        assert torch.equal(model.positions.data[:head], pre["positions"][~mask]) and torch.equal(model.scale.data[:head], pre["scale"][~mask]), label
        assert torch.equal(model.rotation.data, torch.cat([pre["rotation"][~mask], src[2]])), label
        e = float(((model.positions.data[head:].double() - want_pos).abs() / bound).max())
        es = float((model.scale.data[head:].double() - want_scale).abs().max())
        print(f"{label}: positions err / bound {e:.3f}, scale abs err {es:.2e}")
        assert e <= 1 and es <= 1e-6, label
    for name, _ in ref.DuckModel.NAMES:
        if name not in ("positions", "scale"):
            assert torch.equal(getattr(models[0], name).data, getattr(models[1], name).data), name
    return head, m


@pytest.mark.parametrize("n", (63, 2049))
def test_fused_split_advances_the_generator_like_torch_normal(densify, n):
    (plain, fused), models = _pair(densify, n, split_n=3)
    norm = torch.rand(n, generator=_cpu_gen(n)).to("cuda") * 4e-4          # about half above the threshold
    pre = _snapshot(models[0], norm)
    states = []
    for s in (plain, fused):
        torch.manual_seed(11)
        unused = torch.cuda.get_rng_state()
        s.split_gaussians(norm, scene_extent=1.0)
        states.append(torch.cuda.get_rng_state())
    assert torch.equal(states[0], states[1])
    assert not torch.equal(unused, states[0])                                # the draw did advance it
    _assert_split_within_bounds(models, pre, 3, seed=11)
    _assert_state_equal(models)


@pytest.mark.parametrize("optimizer", ("adam", "selective"))
def test_strategy_end_to_end_agrees_with_the_restatement(densify, optimizer):
    n = 2049
    opt = "adam" if optimizer == "adam" else importlib.import_module("3dgrut_amd.optimizers").SelectiveAdam
    (plain, fused), models = _pair(densify, n, optimizer=opt)
    g = _cpu_gen(5)
    pose = torch.eye(4).unsqueeze(0).to("cuda")
    for step in range(3):
        grad = torch.randn((n, 3), generator=g) * 2e-4
        grad[torch.rand(n, generator=g) < 0.3] = 0
        pose[0, :3, 3] = torch.randn(3, generator=g).to("cuda")
        for s, m in zip((plain, fused), models):
            m.positions.grad = grad.to("cuda")
            s.update_gradient_buffer(sensor_position=pose[0, :3, 3])
    assert torch.equal(plain.densify_grad_norm_denom, fused.densify_grad_norm_denom)
    assert int(plain.densify_grad_norm_denom.max()) == 3 and int(plain.densify_grad_norm_denom.min()) == 0
    torch.testing.assert_close(fused.densify_grad_norm_accum, plain.densify_grad_norm_accum, rtol=4e-6, atol=0)   # 2e-6 of test 1, both fp32
    fused.densify_grad_norm_accum = plain.densify_grad_norm_accum.clone()    # the same masks from here on
    n_small = int((models[0].get_scale().amax(dim=1) <= 0.01).sum())
    assert 0 < n_small < n                                                   # candidates for the clone and for the split
    # record what the restated split starts from (the model after the clone)
    pre = {}
    restated_split = plain.split_gaussians

    def recording_split(norm, scene_extent):
        pre.update(_snapshot(models[0], norm))
        restated_split(norm, scene_extent)

    plain.split_gaussians = recording_split
    for s in (plain, fused):
        torch.manual_seed(3)
        s.densify_gaussians(scene_extent=1.0)
    n_cloned = pre["positions"].shape[0] - n
    assert n_cloned > 0
    head, tail = _assert_split_within_bounds(models, pre, 2, seed=3)           # the clone draws nothing: the split's is the first draw
    grown = head + tail
    _assert_state_equal(models)
    moments = models[1].optimizer.state[models[1].features_specular]
    assert not bool(moments["exp_avg"][head:].any()) and not bool(moments["exp_avg_sq"][head:].any()) and bool(moments["exp_avg"][:n // 2].any())
    for s in (plain, fused):
        assert s.densify_grad_norm_accum.shape == (grown, 1) and not bool(s.densify_grad_norm_accum.any())
        assert s.densify_grad_norm_denom.dtype == torch.int32 and s.densify_grad_norm_denom.shape == (grown, 1)
    # make the two models identical again (the tails differ within the bound), then prune and reset
    for name, _ in ref.DuckModel.NAMES:
        getattr(models[1], name).data.copy_(getattr(models[0], name).data)
    for s in (plain, fused):
        s.densify_grad_norm_accum += torch.arange(grown, device="cuda", dtype=torch.float32).unsqueeze(1)
        s.prune_gaussians_opacity()
        s.reset_density()
    pruned = models[0].num_gaussians
    assert 0 < pruned < grown and models[1].num_gaussians == pruned
    for name, _ in ref.DuckModel.NAMES:
        assert torch.equal(getattr(models[0], name).data, getattr(models[1], name).data), name
        assert getattr(models[1], name).requires_grad
    _assert_state_equal(models)
    assert torch.equal(plain.densify_grad_norm_accum, fused.densify_grad_norm_accum) and fused.densify_grad_norm_accum.shape == (pruned, 1)
    assert torch.equal(plain.densify_grad_norm_denom, fused.densify_grad_norm_denom)
    # the optimizer still steps on the new parameters
    vis = torch.ones((pruned, 1), device="cuda")
    for m in models:
        before = m.positions.data.clone()
        for name, _ in ref.DuckModel.NAMES:
            p = getattr(m, name)
            p.grad = torch.full_like(p, 1e-3)
        m.optimizer.step(vis) if optimizer == "selective" else m.optimizer.step()
        assert not torch.equal(before, m.positions.data)
    for name, _ in ref.DuckModel.NAMES:
        assert torch.equal(getattr(models[0], name).data, getattr(models[1], name).data), name


def _assert_state_equal(models):
    a, b = (m.optimizer for m in models)
    assert [g["name"] for g in a.param_groups] == [g["name"] for g in b.param_groups]
    for ga, gb, m in zip(a.param_groups, b.param_groups, [models[1]] * len(a.param_groups)):
        pa, pb = ga["params"][0], gb["params"][0]
        assert pb is getattr(m, gb["name"]) and len(b.state) == len(b.param_groups)
        sa, sb = a.state[pa], b.state[pb]
        assert set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(sb["step"]) == 7.0 and sb["step"].device.type == "cpu"            # untouched
        for key in ("exp_avg", "exp_avg_sq"):
            assert sb[key].shape == pb.shape and torch.equal(sa[key], sb[key]), (gb["name"], key)   # zeros on the new rows included
