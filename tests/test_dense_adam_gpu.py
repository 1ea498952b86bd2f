"""GPU: FusedAdam / grut_adam_update against the NumPy restatement of torch's fused Adam (tests/adam_reference.py) and against
torch.optim.Adam(fused=True) on the same device.

The layout of every case: the six Gaussian groups [N, w], w in (3, 1, 4, 3, 3, 45) (numels that are no multiple of 4 for odd N), one
group holding TWO tensors of 1024 and 1025 elements (exactly one block of 256 lanes x 4 floats; one block plus a one-element tail),
one group with an empty tensor and a parameter without a grad, and a ninth group: nine non-empty tensors need a second batch of
kAdamMaxGroups = 8."""
import importlib

import numpy as np
import pytest
import torch

import adam_reference as ref

pytestmark = pytest.mark.gpu
WIDTHS = (3, 1, 4, 3, 3, 45)
LRS = (0.00016, 0.05, 0.001, 0.005, 0.0025, 0.000125, 0.01, 0.02, 0.03)   # configs/base_gs.yaml:138-152, then three more groups
EPS = 1e-15


def _mod():
    return importlib.import_module("3dgrut_amd.optimizers")


def _layout(n, seed=0, device="cuda", dtype=torch.float32):
    """-> (param groups, {name: parameter}).  Host-generated so that two calls with one seed give equal tensors."""
    g = torch.Generator().manual_seed(seed)
    P = lambda *shape: torch.nn.Parameter(torch.randn(shape, generator=g).to(device=device, dtype=dtype))   # noqa: E731
    named = {f"w{w}_{i}": P(n, w) for i, w in enumerate(WIDTHS)}
    named.update(block=P(1024), tail=P(1025), empty=P(0, 3), nograd=P(7, 3), last=P(n, 2))
    tensors = [[named[f"w{w}_{i}"]] for i, w in enumerate(WIDTHS)] + [[named["block"], named["tail"]], [named["empty"], named["nograd"]], [named["last"]]]
    return [{"params": ps, "lr": lr} for ps, lr in zip(tensors, LRS)], named


def _grads(named, seed):
    g = torch.Generator().manual_seed(10_000 + seed)
    return {k: torch.randn(p.shape, generator=g) for k, p in named.items() if k != "nograd"}


def _set_grads(named, grads):
    for k, g in grads.items():
        named[k].grad = g.to(device=named[k].device, dtype=named[k].dtype)


def _seed_state(opt, named, seed, skip=("block", "tail")):
    """Moments and a step count of 3 as if three steps had run (the block / tail tensors stay fresh: lazy initialisation)."""
    g = torch.Generator().manual_seed(20_000 + seed)
    for k, p in named.items():
        if k in skip:
            continue
        opt.state[p] = {"step": torch.tensor(3.0, dtype=torch.float32, device=p.device),
                        "exp_avg": (0.1 * torch.randn(p.shape, generator=g)).to(p.device),
                        "exp_avg_sq": (0.1 * torch.randn(p.shape, generator=g) ** 2).to(p.device)}


def _snapshot(opt, named):
    out = {}
    for k, p in named.items():
        st = opt.state.get(p, {})
        out[k] = {"param": p.detach().cpu().numpy().copy(),
                  **{key: st[key].detach().cpu().numpy().copy() for key in ("step", "exp_avg", "exp_avg_sq") if key in st}}
    return out


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("n", [1, 5, 341, 3001])
def test_one_step_matches_the_restatement(n, weight_decay):
    """exp_avg / exp_avg_sq within 1 fp32 ulp, param within ulp(p) + 2^-22 |dp|: every fp32 operation of the last statement is
    correctly rounded and cannot be contracted, so what is left is the last bit of the double pow and fma contraction inside the double
    statements ahead of their single rounding.  Measured on an MI355X (error / bound, worst element of the eight cases): exp_avg 1.0 (one
    ulp, from N = 341 on), exp_avg_sq 0, param 0.9999 (one ulp of a parameter whose update is small against it)."""
    mod = _mod()
    groups, named = _layout(n, seed=n)
    opt = mod.FusedAdam(groups, lr=0.0, eps=EPS, weight_decay=weight_decay, fused=True)
    _seed_state(opt, named, seed=n)
    grads = _grads(named, 0)
    _set_grads(named, grads)
    before = _snapshot(opt, named)
    count = dict(mod.stats)
    opt.step()
    torch.cuda.synchronize()
    assert mod.stats["hip_steps"] == count["hip_steps"] + 1 and mod.stats["torch_steps"] == count["torch_steps"]
    after = _snapshot(opt, named)

    # torch's step counts on a twin (the empty tensor included)
    tgroups, tnamed = _layout(n, seed=n)
    twin = torch.optim.Adam(tgroups, lr=0.0, eps=EPS, weight_decay=weight_decay, fused=True)
    _seed_state(twin, tnamed, seed=n)
    _set_grads(tnamed, grads)
    twin.step()

    lr_of = {id(p): g["lr"] for g in opt.param_groups for p in g["params"]}
    worst = {"exp_avg": 0.0, "exp_avg_sq": 0.0, "param": 0.0}
    for k, p in named.items():
        b, a = before[k], after[k]
        if k == "nograd":   # skipped: parameter, state and step untouched
            assert all(np.array_equal(a[key], b[key]) for key in b) and float(a["step"]) == 3.0
            continue
        old_step = float(b["step"]) if "step" in b else 0.0
        assert float(a["step"]) == old_step + 1.0 == float(twin.state[tnamed[k]]["step"]), k
        if p.numel() == 0:
            continue
        zeros = np.zeros(p.shape, np.float32)
        rp, rm, rv, _ = ref.adam_step(b["param"], grads[k].numpy(), b.get("exp_avg", zeros), b.get("exp_avg_sq", zeros), old_step, lr_of[id(p)],
                                      eps=EPS, weight_decay=weight_decay)
        for key, r in (("exp_avg", rm), ("exp_avg_sq", rv)):
            err = np.abs(a[key].astype(np.float64) - r.astype(np.float64))
            worst[key] = max(worst[key], float((err / np.spacing(np.abs(r))).max()))
            assert (err <= np.spacing(np.abs(r))).all(), (k, key)
        err = np.abs(a["param"].astype(np.float64) - rp.astype(np.float64))
        bound = np.spacing(np.abs(rp)).astype(np.float64) + 2.0 ** -22 * np.abs(rp.astype(np.float64) - b["param"].astype(np.float64))
        worst["param"] = max(worst["param"], float((err / bound).max()))
        assert (err <= bound).all(), (k, "param")
    print(f"dense adam one step n={n} wd={weight_decay}: worst error / bound {worst}")


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_twenty_steps_stay_as_close_to_torch_as_torch_is_to_float64(weight_decay):
    """max |FusedAdam - torch| <= 4 x max |torch - float64 restatement| for param, exp_avg and exp_avg_sq after 20 steps with fresh
    random grads: the yardstick is torch's own distance from the exact recurrence; 4 allows the two fp32 implementations to sit on
    opposite sides of it.  Measured on an MI355X: ratios 0.12 / 0.49 / 0 (param / exp_avg / exp_avg_sq) without weight decay and
    0.20 / 0.51 / 0 with 0.01."""
    mod = _mod()
    n, k = 341, 20
    (groups, named), (tgroups, tnamed) = _layout(n, seed=1), _layout(n, seed=1)
    mine = mod.FusedAdam(groups, lr=0.0, eps=EPS, weight_decay=weight_decay)
    theirs = torch.optim.Adam(tgroups, lr=0.0, eps=EPS, weight_decay=weight_decay, fused=True)
    start = _snapshot(mine, named)
    all_grads = [_grads(named, s) for s in range(k)]
    count = mod.stats["hip_steps"]
    for grads in all_grads:
        _set_grads(named, grads)
        _set_grads(tnamed, grads)
        mine.step()
        theirs.step()
    torch.cuda.synchronize()
    assert mod.stats["hip_steps"] == count + k
    got, want = _snapshot(mine, named), _snapshot(theirs, tnamed)
    lr_of = {id(p): g["lr"] for g in mine.param_groups for p in g["params"]}
    ours = {"param": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
    torchs = dict(ours)
    for name, p in named.items():
        if name == "nograd" or p.numel() == 0:
            continue
        zeros = np.zeros(p.shape, np.float32)
        exact = dict(zip(("param", "exp_avg", "exp_avg_sq"),
                         ref.adam_steps_f64(start[name]["param"], [g[name].numpy() for g in all_grads], zeros, zeros, 0.0, lr_of[id(p)],
                                            eps=EPS, weight_decay=weight_decay)))
        assert float(got[name]["step"]) == float(want[name]["step"]) == float(k)
        for key in ours:
            ours[key] = max(ours[key], float(np.abs(got[name][key].astype(np.float64) - want[name][key].astype(np.float64)).max()))
            torchs[key] = max(torchs[key], float(np.abs(want[name][key].astype(np.float64) - exact[key]).max()))
    ratios = {key: ours[key] / torchs[key] for key in ours}
    print(f"dense adam {k} steps wd={weight_decay}: |ours - torch| {ours}  |torch - f64| {torchs}  ratio {ratios}")
    for key in ours:
        assert torchs[key] > 0.0 and ours[key] <= 4.0 * torchs[key], (key, ours[key], torchs[key])


def _run(mod, n, steps, seed, lr_change=None, stream=None):
    groups, named = _layout(n, seed=seed)
    opt = mod.FusedAdam(groups, lr=0.0, eps=EPS, weight_decay=0.01)
    for s in range(steps):
        _set_grads(named, _grads(named, s))
        if lr_change is not None and s == lr_change[0]:
            opt.param_groups[5]["lr"] = lr_change[1]
        if stream is None:
            opt.step()
        else:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                opt.step()
            torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    return opt, named, _snapshot(opt, named)


def _equal(x, y):
    return all(np.array_equal(x[k][key], y[k][key]) for k in x for key in x[k])


def test_equal_inputs_give_equal_bits_and_a_side_stream_works():
    mod = _mod()
    count = mod.stats["hip_steps"]
    _, _, first = _run(mod, 341, 3, seed=2)
    _, _, second = _run(mod, 341, 3, seed=2)
    _, _, side = _run(mod, 341, 3, seed=2, stream=torch.cuda.Stream())
    assert mod.stats["hip_steps"] == count + 9
    assert _equal(first, second)
    assert _equal(first, side)


def test_a_changed_learning_rate_is_used_by_the_next_step():
    mod = _mod()
    opt, named, changed = _run(mod, 341, 3, seed=2, lr_change=(2, 0.5))
    _, _, plain = _run(mod, 341, 3, seed=2)
    assert not np.array_equal(changed["w45_5"]["param"], plain["w45_5"]["param"])
    assert all(np.array_equal(changed[k]["param"], plain[k]["param"]) for k in changed if k != "w45_5")   # the other groups kept theirs
    # the third step of that group restated from the second's state with the new rate
    _, named2, two = _run(mod, 341, 2, seed=2)
    g = _grads(named2, 2)["w45_5"].numpy()
    rp, _, _, _ = ref.adam_step(two["w45_5"]["param"], g, two["w45_5"]["exp_avg"], two["w45_5"]["exp_avg_sq"], 2.0, 0.5, eps=EPS, weight_decay=0.01)
    err = np.abs(changed["w45_5"]["param"].astype(np.float64) - rp.astype(np.float64))
    bound = np.spacing(np.abs(rp)).astype(np.float64) + 2.0 ** -22 * np.abs(rp.astype(np.float64) - two["w45_5"]["param"].astype(np.float64))
    assert (err <= bound).all()


@pytest.mark.parametrize("case", ["amsgrad", "float64"])
def test_what_the_kernel_does_not_cover_takes_torchs_path(case):
    mod = _mod()
    kwargs, dtype = ({"amsgrad": True}, torch.float32) if case == "amsgrad" else ({}, torch.float64)
    (groups, named), (tgroups, tnamed) = _layout(5, seed=3, dtype=dtype), _layout(5, seed=3, dtype=dtype)
    mine = mod.FusedAdam(groups, lr=0.0, eps=EPS, **kwargs)
    theirs = torch.optim.Adam(tgroups, lr=0.0, eps=EPS, fused=True, **kwargs)
    count = dict(mod.stats)
    for s in range(2):
        grads = _grads(named, s)
        _set_grads(named, grads)
        _set_grads(tnamed, grads)
        mine.step()
        theirs.step()
    torch.cuda.synchronize()
    assert mod.stats["torch_steps"] == count["torch_steps"] + 2 and mod.stats["hip_steps"] == count["hip_steps"]
    assert _equal(_snapshot(mine, named), _snapshot(theirs, tnamed))
    if case == "amsgrad":
        assert "max_exp_avg_sq" in mine.state[named["last"]]


def test_a_replaced_parameter_keeps_its_step_on_the_hip_path():
    """threedgrut/strategy/base.py:77-107 (_update_param_with_optimizer): a new Parameter with more rows takes the group's slot, the
    state moves to the new key with its `step` kept and its moments extended."""
    mod = _mod()
    opt, named, _ = _run(mod, 341, 2, seed=4)
    group = opt.param_groups[5]
    old = group["params"][0]
    state = opt.state.pop(old)
    extra = 100
    new = torch.nn.Parameter(torch.cat([old.detach(), old.detach()[:extra] * 0.5]))
    for key in ("exp_avg", "exp_avg_sq"):
        state[key] = torch.cat([state[key], torch.zeros_like(state[key][:extra])])
    group["params"] = [new]
    opt.state[new] = state
    named = {**named, "w45_5": new}
    grads = _grads(named, 9)
    _set_grads(named, grads)
    before = _snapshot(opt, named)["w45_5"]
    count = mod.stats["hip_steps"]
    opt.step()
    torch.cuda.synchronize()
    assert mod.stats["hip_steps"] == count + 1
    after = _snapshot(opt, named)["w45_5"]
    assert float(before["step"]) == 2.0 and float(after["step"]) == 3.0 and after["param"].shape == (341 + extra, 45)
    rp, rm, rv, _ = ref.adam_step(before["param"], grads["w45_5"].numpy(), before["exp_avg"], before["exp_avg_sq"], 2.0, group["lr"], eps=EPS,
                                  weight_decay=0.01)
    assert (np.abs(after["exp_avg"] - rm) <= np.spacing(np.abs(rm))).all() and (np.abs(after["exp_avg_sq"] - rv) <= np.spacing(np.abs(rv))).all()
    err = np.abs(after["param"].astype(np.float64) - rp.astype(np.float64))
    assert (err <= np.spacing(np.abs(rp)).astype(np.float64) + 2.0 ** -22 * np.abs(rp.astype(np.float64) - before["param"].astype(np.float64))).all()


def test_a_strided_grad_is_copied_and_the_library_is_called_directly():
    """A non-contiguous grad goes through a contiguous copy; grut_adam_update itself with a group of numel 0 leaves that `step` alone."""
    import ctypes as C
    mod = _mod()
    abi = importlib.import_module("3dgrut_amd._abi")
    p = torch.nn.Parameter(torch.randn(33, 5, device="cuda"))
    q = torch.nn.Parameter(p.detach().clone())
    g = torch.randn(5, 33, device="cuda")
    p.grad, q.grad = g.t(), g.t().contiguous()
    assert not p.grad.is_contiguous()
    a, b = mod.FusedAdam([p], lr=1e-2), mod.FusedAdam([q], lr=1e-2)
    count = mod.stats["hip_steps"]
    a.step()
    b.step()
    assert mod.stats["hip_steps"] == count + 2 and torch.equal(p, q) and torch.equal(a.state[p]["exp_avg"], b.state[q]["exp_avg"])

    step = torch.full((2,), 5.0, device="cuda")
    grp = (abi.GrutDenseAdamGroup * 1)()
    grp[0].step, grp[0].numel = step.data_ptr(), 0
    scratch = torch.zeros(2, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    abi.check(abi.load_library().grut_adam_update(stream, grp, 1, C.c_void_p(scratch.data_ptr())), "grut_adam_update")
    torch.cuda.synchronize()
    assert step.tolist() == [5.0, 5.0]


@pytest.mark.parametrize("with_scheduler", [False, True])
def test_adopting_a_foreach_adam_moves_its_host_step_to_the_device(with_scheduler):
    """A non-fused torch.optim.Adam on device parameters keeps `step` on the host; the HIP pass needs it on the device.  After one
    torch step, adopt() moves it, the next step runs on the HIP path from the kept state, and - where an lr_scheduler was attached
    to the old optimizer first, as trainer.py:573-590 does for the decoder - the rate the scheduler writes is the rate used."""
    mod = _mod()
    groups, named = _layout(5, seed=6)
    old = torch.optim.Adam(groups, lr=0.0, eps=EPS, weight_decay=0.01, foreach=True)
    sched = torch.optim.lr_scheduler.ExponentialLR(old, gamma=0.5) if with_scheduler else None
    _set_grads(named, _grads(named, 0))
    old.step()
    assert old.state[named["w45_5"]]["step"].device.type == "cpu"
    if sched is not None:
        sched.step()
    new = mod.FusedAdam.adopt(old)
    assert new.state[named["w45_5"]]["step"].is_cuda and new.state[named["w45_5"]]["step"].dtype == torch.float32
    grads = _grads(named, 1)
    _set_grads(named, grads)
    before, count = _snapshot(new, named), dict(mod.stats)
    new.step()
    torch.cuda.synchronize()
    assert mod.stats["hip_steps"] == count["hip_steps"] + 1 and mod.stats["torch_steps"] == count["torch_steps"]
    after = _snapshot(new, named)
    assert "step" not in after["nograd"] and np.array_equal(after["nograd"]["param"], before["nograd"]["param"])
    for k in grads:
        assert float(before[k]["step"]) == 1.0 and float(after[k]["step"]) == 2.0
    lr = LRS[5] * (0.5 if with_scheduler else 1.0)
    assert new.param_groups[5]["lr"] == lr
    b, a = before["w45_5"], after["w45_5"]
    rp, rm, rv, _ = ref.adam_step(b["param"], grads["w45_5"].numpy(), b["exp_avg"], b["exp_avg_sq"], 1.0, lr, eps=EPS, weight_decay=0.01)
    assert (np.abs(a["exp_avg"] - rm) <= np.spacing(np.abs(rm))).all() and (np.abs(a["exp_avg_sq"] - rv) <= np.spacing(np.abs(rv))).all()
    err = np.abs(a["param"].astype(np.float64) - rp.astype(np.float64))
    assert (err <= np.spacing(np.abs(rp)).astype(np.float64) + 2.0 ** -22 * np.abs(rp.astype(np.float64) - b["param"].astype(np.float64))).all()
