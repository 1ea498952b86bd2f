"""GPU: the MCMC strategy's kernels (csrc/mcmc.hip) against restatements written here from the reference's formulas, the random
generator left exactly where the reference leaves it, and a short MCMC training loop through both renderer plugins.

The formulas restated (threedgrut/strategy/...):
  relocation    gaussian_mcmc.cu:36-66   new_o = 1 - (1 - o)^(1/n);  new_s = o / D * s,
                                         D = sum_{i=1..n} sum_{k=0..i-1} C(i-1, k) (-1)^k / sqrt(k+1) new_o^(k+1)
                mcmc.py:70-77            binoms[n][k] = C(n, k) for k <= n else 0, an [n_max, n_max] table
  perturbation  mcmc.py:167-187          positions += R S S^T R^T (randn * sigmoid_100(1 - d) * noise_lr * lr),
                                         sigmoid_100(x) = 1 / (1 + exp(-100 (x - 0.995)))
                model.py:120-130, utils/misc.py:67-88   covariance and quaternion_to_so3 (q = (r, x, y, z), normalised)
  relocate/add  mcmc.py:109-166, 189-222 (the parameter / Adam-state scatter, restated in the training test below)
"""
import importlib
import math

import numpy as np
import pytest

import oracle
from scenes import make_scene, torch_batch

pytestmark = pytest.mark.gpu
syn = importlib.import_module("workloads.synthetic")
U = 2.0 ** -24   # unit roundoff of fp32


def _mcmc():
    return importlib.import_module("3dgrut_amd.mcmc")


def _binoms(n_max):   # mcmc.py:70-77
    return np.array([[math.comb(n, k) if k <= n else 0 for k in range(n_max)] for n in range(n_max)], np.float64)


# ---- relocation ------------------------------------------------------------------------------------------------------------------
def _relocation_inputs(n, n_max, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(0.005, 1 - 1e-6, n).astype(np.float32)
    o[:4] = np.float32(0.005), np.float32(1 - 1e-6), np.float32(0.005), np.float32(1 - 1e-6)
    ratios = np.ones(n, np.int32)                               # most sampled Gaussians are drawn once (ratio 1)
    some = rng.uniform(size=n) < 0.4
    ratios[some] = rng.integers(1, n_max + 1, int(some.sum()))
    ratios[::97] = n_max                                         # and some exactly at the table's end
    ratios[1] = ratios[3] = n_max
    scales = np.exp(rng.normal(-4.0, 1.0, (n, 3))).astype(np.float32)   # log-normal, as exp(raw scale)
    return o, scales, ratios


def _restate_denominator(new_o, ratios, binoms, n_max, dtype):
    """D in the reference's order (i outer, k inner, one running sum) in `dtype`; also (in float64) sum |terms| and sum |partial sums|."""
    no = new_o.astype(dtype)
    d = np.zeros_like(no)
    abs_terms = np.zeros(len(no))
    abs_partials = np.zeros(len(no))
    for i in range(1, n_max + 1):
        act = ratios >= i
        for k in range(i):
            term = (dtype(-1.0 if k & 1 else 1.0) / np.sqrt(dtype(k + 1))) * np.power(no, dtype(k + 1))
            bt = (dtype(binoms[i - 1, k]) * term).astype(dtype)
            d = np.where(act, (d + bt).astype(dtype), d)
            abs_terms += np.where(act, np.abs(bt.astype(np.float64)), 0.0)
            abs_partials += np.where(act, np.abs(d.astype(np.float64)), 0.0)
    return d, abs_terms, abs_partials


@pytest.mark.parametrize("n_max", [51, 10])
def test_relocation_matches_restatements(n_max):
    import torch
    n = 70_001
    o, scales, ratios = _relocation_inputs(n, n_max, seed=n_max)
    binoms = _binoms(n_max)
    dev = dict(device="cuda")
    new_o, new_s = _mcmc().compute_relocation_tensor(torch.as_tensor(o[:, None], **dev), torch.as_tensor(scales, **dev),
                                                     torch.as_tensor(ratios, **dev), torch.as_tensor(binoms, dtype=torch.float32, **dev), n_max)
    assert new_o.shape == (n, 1) and new_s.shape == (n, 3)
    new_o, new_s = new_o.cpu().numpy()[:, 0], new_s.cpu().numpy()

    # opacity: float64 from the fp32 operands the kernel rounds to (1 - o and 1/n); what remains is powf's error (a few ulp of a value
    # below 1, each ulp <= 2^-24) and the rounding of the final 1 - p
    base = (np.float32(1) - o).astype(np.float64)
    expo = (np.float32(1) / ratios.astype(np.float32)).astype(np.float64)
    o64 = 1.0 - base ** expo
    assert np.all(np.abs(new_o - o64) <= 4 * U + 2 * U * np.abs(o64)), np.abs(new_o - o64).max()

    # scale: D restated in fp32 (same order) and in float64, both from the kernel's new opacity so that only the sum is compared
    d32, _, _ = _restate_denominator(new_o, ratios, binoms, n_max, np.float32)
    d64, abs_terms, abs_partials = _restate_denominator(new_o, ratios, binoms, n_max, np.float64)
    s32 = (o / d32)[:, None] * scales
    s64 = (o.astype(np.float64) / d64)[:, None] * scales.astype(np.float64)
    # Bound from the sum's conditioning: an fp32 running sum is off by at most u * sum |partial sums| (the rounding of every addition,
    # to first order) plus a few roundings per term (sqrt, division, powf, products: <= 8 u |term|); o / D * s adds two more roundings.
    # (1e-6 * sum |terms| / |D| alone is not a bound: with up to 1326 additions the running sum's own rounding reaches ~1.3e-6 relative
    # at conditioning ~1 in an fp32 restatement.)
    rel64 = (U * (abs_partials + 8 * abs_terms) / np.abs(d64) + 4 * U)[:, None]
    err64 = np.abs(new_s - s64) / np.abs(s64)
    assert np.all(err64 <= rel64), float((err64 / rel64).max())
    cond = abs_terms / np.abs(d64)
    print(f"n_max={n_max}: conditioning max {cond.max():.1f}, rel err vs float64 max {err64.max():.2e}, "
          f"max err / (1e-6 sum|terms|/|D|) = {float((err64.max(1) / (1e-6 * cond)).max()):.2f}")
    # the fp32 restatement (the reference's arithmetic without fused multiply-adds) lies within the same bound of float64, so the two
    # fp32 evaluations agree to twice it
    assert np.all(np.abs(new_s - s32) / np.abs(s64) <= 2 * rel64)
    ulps = np.abs(new_s - s32) / np.spacing(np.abs(s32))
    print(f"n_max={n_max}: kernel vs fp32 restatement: max {ulps.max():.0f} ulp, ratio-1 rows max {ulps[ratios == 1].max():.0f} ulp, "
          f"{(ulps == 0).mean() * 100:.1f} % of values bitwise equal")
    assert np.isfinite(new_s).all() and np.all(new_s > 0) and np.all((new_o > 0) & (new_o <= o + 4 * U))


def test_relocation_empty_and_error_paths():
    import torch
    mcmc = _mcmc()
    binoms = torch.as_tensor(_binoms(51), dtype=torch.float32, device="cuda")
    e_o, e_s = mcmc.compute_relocation_tensor(torch.empty(0, 1, device="cuda"), torch.empty(0, 3, device="cuda"),
                                              torch.empty(0, dtype=torch.int32, device="cuda"), binoms, 51)
    assert e_o.shape == (0, 1) and e_s.shape == (0, 3)
    n = 100
    o = torch.rand(n, 1, device="cuda")
    s = torch.rand(n, 3, device="cuda")
    r = torch.ones(n, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="CUDA"):
        mcmc.compute_relocation_tensor(o.cpu(), s, r, binoms, 51)
    with pytest.raises(RuntimeError, match="contiguous"):
        mcmc.compute_relocation_tensor(o, torch.rand(3, n, device="cuda").t(), r, binoms, 51)
    with pytest.raises(RuntimeError, match="size mismatch"):
        mcmc.compute_relocation_tensor(o, s[:-1].contiguous(), r, binoms, 51)
    with pytest.raises(RuntimeError, match="size mismatch"):
        mcmc.compute_relocation_tensor(o, s, r[:-1].contiguous(), binoms, 51)
    with pytest.raises(RuntimeError, match="binoms"):
        mcmc.compute_relocation_tensor(o, s, r, binoms, 52)   # a table too small for n_max would be read past its end
    lib = importlib.import_module("3dgrut_amd._abi").load_library()
    assert lib.grut_mcmc_relocation(None, 1, None, None, None, None, 51, None, None) != 0   # null pointers, before any launch
    assert lib.grut_mcmc_relocation(None, 1, o.data_ptr(), s.data_ptr(), r.data_ptr(), binoms.data_ptr(), 0, o.data_ptr(), s.data_ptr()) != 0
    assert b"n_max" in lib.grut_last_error()
    assert lib.grut_mcmc_perturb(None, 1, s.data_ptr(), s.data_ptr(), s.data_ptr(), o.data_ptr(), s.data_ptr(), 1.0, 1.0, 2) != 0
    assert b"activated" in lib.grut_last_error()
    assert lib.grut_mcmc_perturb(None, 1, None, None, None, None, None, 1.0, 1.0, 0) != 0
    assert lib.grut_mcmc_perturb(None, 0, None, None, None, None, None, 1.0, 1.0, 0) == 0   # n = 0 launches nothing


# ---- perturbation ------------------------------------------------------------------------------------------------------------------
def _restate_delta64(rotation, scale, density, noise, noise_lr, lr, activated):
    """float64 Delta of mcmc.py:169-187 and the magnitudes its fp32 error is measured in:
    M_i  = s noise_lr lr sum_j (|R| S^2 |R|^T)_ij |n_j|            (relative rounding of every product and sum),
    MR_i = s noise_lr lr sum_j (1 S^2 |R|^T + |R| S^2 1^T)_ij |n_j|  (an ABSOLUTE error in the rotation entries: 1 - 2 (y^2 + z^2) and
           its kin are O(1) expressions of the twice normalised quaternion, off by up to ~16 u whatever their size; where an entry
           nearly vanishes along the dominant scale axis, M alone would ask for a relative accuracy its rounding cannot give)."""
    import torch
    q, s, d, nz = (t.double() for t in (rotation, scale, density, noise))
    if not activated:
        q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
        s, d = torch.exp(s), torch.sigmoid(d)
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    s2 = (s * s)[:, None, :]
    cov = (R * s2) @ R.transpose(1, 2)
    mag = (R.abs() * s2) @ R.abs().transpose(1, 2)
    ones = torch.ones_like(R)
    mag_r = (ones * s2) @ R.abs().transpose(1, 2) + (R.abs() * s2) @ ones.transpose(1, 2)
    sg = 1.0 / (1.0 + torch.exp(-100.0 * ((1.0 - d) - 0.995)))
    v = nz * sg * noise_lr * lr
    delta = (cov @ v[..., None])[..., 0]
    w = (nz.abs() * sg * noise_lr * lr)[..., None]
    return delta, (mag @ w)[..., 0] + 16 * U / 1e-5 * (mag_r @ w)[..., 0]


def _raw_gaussians(n, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    rot = torch.randn(n, 4, device="cuda", generator=g)
    scl = torch.randn(n, 3, device="cuda", generator=g) - 4.5        # exp(raw): log-normal around 0.011
    dns = torch.randn(n, 1, device="cuda", generator=g) * 3.0        # sigmoid(raw) spans (0, 1): dead, mid and dense (overflow) particles
    dns[:1000] = torch.linspace(-1e-3, 1e-3, 1000, device="cuda")[:, None]   # density ~ 0.5
    return rot, scl, dns


TINY = 1e-24   # absolute floor: where density > ~0.6 the factor sigmoid_100(1 - d) < 1e-26 and Delta is below any position's ulp


@pytest.mark.parametrize("activated", [0, 1])
def test_perturbation_matches_float64_restatement(activated):
    import torch
    n, noise_lr, lr = 1_000_003, 5e5, 1.6e-4
    rot, scl, dns = _raw_gaussians(n, seed=11 + activated)
    if activated:
        rot, scl, dns = torch.nn.functional.normalize(rot), torch.exp(scl), torch.sigmoid(dns)
    torch.manual_seed(5)
    noise = torch.randn(n, 3, device="cuda")
    before = [t.clone() for t in (rot, scl, dns, noise)]
    pos = torch.zeros(n, 3, device="cuda")           # zero positions: the result IS the kernel's Delta, exactly
    ptr = pos.data_ptr()
    _mcmc().perturb_positions_(pos, rot, scl, dns, noise, noise_lr, lr, activated=bool(activated))
    torch.cuda.synchronize()
    assert pos.data_ptr() == ptr
    for a, b in zip((rot, scl, dns, noise), before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))   # inputs untouched, bit for bit
    delta64, mag = _restate_delta64(rot, scl, dns, noise, noise_lr, lr, activated)
    err = (pos.double() - delta64).abs()
    bound = 1e-5 * mag + TINY   # (mag carries the rotation entries' absolute error, see _restate_delta64)
    assert bool(torch.isfinite(pos).all())
    assert bool((err <= bound).all()), float((err / bound).max())
    # the overflow regime: for dense particles exp(-100 ((1 - d) - 0.995)) is +inf in fp32 and the factor is exactly 0
    d = dns[:, 0] if activated else torch.sigmoid(dns[:, 0])
    dense = d >= 0.9
    assert int(dense.sum()) > 1000 and bool((pos[dense] == 0).all())
    mid = d.sub(0.5).abs() < 1e-3                 # density ~ 0.5: finite and negligible (factor ~ 3e-22)
    assert int(mid.sum()) >= 1000 and bool((pos[mid].abs() < 1e-12).all())
    live = d < 0.3
    assert bool((pos[live].abs().sum(1) > 0).all())
    # the update is in place on top of existing positions: p + Delta, rounded once
    pos2 = torch.randn(n, 3, device="cuda")
    expect = pos2 + pos
    _mcmc().perturb_positions_(pos2, rot, scl, dns, noise, noise_lr, lr, activated=bool(activated))
    assert torch.equal(pos2, expect)


class _TinyModel:
    """The surface MCMCStrategy.perturb_gaussians touches: positions Parameter, raw parameters with the default activations, an
    optimizer with a "positions" group."""

    def __init__(self, n, seed, standard=True):
        import torch
        rot, scl, dns = _raw_gaussians(n, seed)
        g = torch.Generator(device="cuda").manual_seed(seed + 1)
        P = torch.nn.Parameter
        self.positions = P(torch.randn(n, 3, device="cuda", generator=g))
        self.rotation, self.scale, self.density = P(rot), P(scl), P(dns)
        self.rotation_activation = torch.nn.functional.normalize
        self.scale_activation = torch.exp
        self.density_activation = torch.sigmoid if standard else (lambda x: torch.sigmoid(x) * 0.999)
        self.optimizer = torch.optim.Adam([{"params": [self.positions], "name": "positions", "lr": 1.6e-4},
                                           {"params": [self.density], "name": "density", "lr": 5e-2}])

    def get_rotation(self):
        return self.rotation_activation(self.rotation)

    def get_scale(self):
        return self.scale_activation(self.scale)

    def get_density(self):
        return self.density_activation(self.density)


def _reference_perturb(model, noise_lr):
    """mcmc.py:167-187 restated with torch ops in fp32 (the reference's arithmetic and its one randn_like draw)."""
    import torch
    with torch.no_grad():
        s = model.get_scale()
        q = model.get_rotation()
        q = q / torch.sqrt((q * q).sum(1, keepdim=True))
        r, x, y, z = q.unbind(1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
        S = torch.diag_embed(s)
        cov = R @ S @ S.transpose(1, 2) @ R.transpose(1, 2)
        d = model.get_density()
        lr = [g["lr"] for g in model.optimizer.param_groups if g["name"] == "positions"][-1]
        noise = torch.randn_like(model.positions) * (1 / (1 + torch.exp(-100 * ((1 - d) - 0.995)))) * noise_lr * lr
        model.positions.add_(torch.bmm(cov, noise.unsqueeze(-1)).squeeze(-1))


@pytest.mark.parametrize("standard", [True, False])
def test_generator_advances_as_the_reference_method(standard):
    import torch
    n, noise_lr = 20_011, 5e5
    a, b = _TinyModel(n, 3, standard), _TinyModel(n, 3, standard)
    p0 = a.positions.detach().clone()
    torch.manual_seed(1234)
    _mcmc().perturb_gaussians(a, noise_lr)
    state_a = torch.cuda.get_rng_state()
    draw_a = torch.multinomial(torch.sigmoid(a.density[:, 0]).detach(), 4096, replacement=True)
    torch.manual_seed(1234)
    _reference_perturb(b, noise_lr)
    state_b = torch.cuda.get_rng_state()
    draw_b = torch.multinomial(torch.sigmoid(b.density[:, 0]).detach(), 4096, replacement=True)
    assert torch.equal(state_a, state_b) and torch.equal(draw_a, draw_b)
    torch.manual_seed(1234)
    noise = torch.randn_like(p0)
    act = not standard
    args = (a.get_rotation(), a.get_scale(), a.get_density()) if act else (a.rotation, a.scale, a.density)
    delta64, mag = _restate_delta64(*[t.detach() for t in args], noise, noise_lr, 1.6e-4, act)
    ulp = torch.finfo(torch.float32).eps * (p0.abs() + delta64.abs().float())   # the two fp32 additions to the positions
    bound = 2e-5 * mag + TINY + ulp.double()
    for m in (a, b):
        assert bool(((m.positions.detach().double() - p0.double() - delta64).abs() <= bound).all())
    assert bool(((a.positions - b.positions).abs().double() <= bound).all())


# ---- end to end: MCMC training through the plugins -------------------------------------------------------------------------------
def _psnr(a, b):
    return float(-10.0 * np.log10(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2) + 1e-20))


class _Strategy:
    """relocate_gaussians / add_new_gaussians / sample_new_gaussians (mcmc.py:109-166, 189-222) restated over the test's model and
    SelectiveAdam, with the relocation kernel behind compute_relocation_tensor."""

    def __init__(self, g, opt, n_max=51, threshold=0.005, max_n=100_000):
        import torch
        self.g, self.opt, self.n_max, self.threshold, self.max_n = g, opt, n_max, threshold, max_n
        self.binoms = torch.as_tensor(_binoms(n_max), dtype=torch.float32, device="cuda")

    def _update(self, param_fn, state_fn):   # BaseStrategy._update_param_with_optimizer, for one-tensor groups
        import torch
        for group in self.opt.param_groups:
            p = group["params"][0]
            new = torch.nn.Parameter(param_fn(group["name"], p.detach()), requires_grad=p.requires_grad)
            state = self.opt.state.pop(p, {})
            for k in ("exp_avg", "exp_avg_sq"):
                if k in state:
                    state[k] = state_fn(state[k])
            group["params"][0] = new
            self.opt.state[new] = state
            setattr(self.g, group["name"], new)

    def _sample(self, num, valid=None):
        import torch
        dens, scales = self.g.get_density().detach(), self.g.get_scale().detach()
        if valid is None:
            valid = torch.arange(0, dens.shape[0], device="cuda", dtype=torch.int32)
        idx = valid[torch.multinomial(dens[valid].flatten(), num, replacement=True)]
        ratios = (torch.bincount(idx)[idx] + 1).clamp_(min=1, max=self.n_max).int()
        new_d, new_s = _mcmc().compute_relocation_tensor(dens[idx].contiguous(), scales[idx].contiguous(), ratios.contiguous(),
                                                         self.binoms, self.n_max)
        new_d = torch.clamp(new_d, max=1.0 - torch.finfo(torch.float32).eps, min=self.threshold)
        return idx, torch.log(new_d / (1 - new_d)), torch.log(new_s)

    def relocate(self):
        import torch
        dens = self.g.get_density().detach()
        dead = torch.where(dens <= self.threshold)[0]
        alive = torch.where(dens > self.threshold)[0]
        if len(dead):
            idx, new_d, new_s = self._sample(len(dead), alive)

            def param_fn(name, p):
                p = p.clone()
                if name == "density":
                    p[idx] = new_d
                elif name == "scale":
                    p[idx] = new_s
                p[dead] = p[idx]
                return p

            def state_fn(v):
                v[idx] = 0
                return v
            self._update(param_fn, state_fn)
        return int(len(dead))

    def add(self):
        import torch
        cur = self.g.num_gaussians
        num = max(0, min(self.max_n, int(1.05 * cur)) - cur)
        if num:
            idx, new_d, new_s = self._sample(num)

            def param_fn(name, p):
                p = p.clone()
                if name == "density":
                    p[idx] = new_d
                elif name == "scale":
                    p[idx] = new_s
                return torch.cat([p, p[idx]])
            self._update(param_fn, lambda v: torch.cat([v, torch.zeros((len(idx), *v.shape[1:]), device=v.device)]))
        return num


@pytest.mark.parametrize("method", ["3dgut", "3dgrt"])
def test_mcmc_training_recovers_a_teacher_scene(method):
    """test_optim_gpu.py's teacher-scene loop with the MCMC strategy on top: perturbation (fused kernel) after every SelectiveAdam step,
    relocation and a 5 % add every 25 steps (relocation kernel).  Teacher images and the final certificate come from the ORACLE."""
    import torch
    n, w, h, views = 600, 48, 48, 3
    scenes = [make_scene(n=n, width=w, height=h, median_scale=0.09, seed=5, view=v, max_density=0.9) for v in range(views)]
    d12, sph = scenes[0]["density12"], scenes[0]["sph"]

    def oracle_images(d12_, sph_):
        imgs = []
        for s in scenes:
            if method == "3dgut":
                f = oracle.gut_forward(oracle.default_gut_config(), s["cam"], s["pose_start"], s["pose_end"], 3, d12_, sph_, *s["rays"])
                imgs.append(f["feat_density"][..., :3])
            else:
                f = oracle.grt_forward(oracle.default_grt_config(), d12_, sph_, 3, 1e-3, s["batch"]["T_to_world"][0], *s["rays"])
                imgs.append(f["features"])
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

    mod = importlib.import_module("3dgrut_amd.gut_tracer" if method == "3dgut" else "3dgrut_amd.grt_tracer")
    tracer = mod.Tracer({"render": {"splat": {}}} if method == "3dgut" else {"render": {}})
    g = syn.ActivatedGaussians(d12_0, sph_0)
    opt_mod = importlib.import_module("3dgrut_amd.optimizers")
    names = ["positions", "density", "rotation", "scale", "features_albedo", "features_specular"]
    lrs = [2e-3, 2e-2, 2e-3, 1e-2, 2e-2, 2e-3]
    opt = opt_mod.SelectiveAdam([{"params": [p], "lr": lr, "name": nm} for p, lr, nm in zip(g.parameters(), lrs, names)], eps=1e-15)
    g.optimizer = opt
    strategy = _Strategy(g, opt)
    batches = [torch_batch(s["batch"], "cuda") for s in scenes]
    target = torch.as_tensor(teacher, device="cuda")
    torch.manual_seed(0)
    relocated, sizes = 0, [g.num_gaussians]
    for it in range(150):
        v = it % views
        for p in g.parameters():
            p.grad = None
        tracer.build_acc(g, rebuild=True)
        out = tracer.render(g, batches[v], train=True)
        loss = ((out["pred_features"][0] - target[v]) ** 2).mean()
        loss.backward()
        opt.step(out["mog_visibility"])
        if it % 25 == 0:                                                 # mcmc.py:79-94 order: relocate, add, perturb
            relocated += strategy.relocate()
            # right after a relocation nothing is dead (the new densities are clamped to the threshold, mcmc.py:211-215; sigmoid of
            # their logit comes back within a few fp32 ulp of it)
            assert bool((g.get_density() > strategy.threshold - 4e-9).all())
            cur = g.num_gaussians
            added = strategy.add()
            assert added == min(strategy.max_n, int(1.05 * cur)) - cur and g.num_gaussians == cur + added
            sizes.append(g.num_gaussians)
        _mcmc().perturb_gaussians(g, noise_lr=5e3)
        assert bool(torch.isfinite(g.positions).all())
    torch.cuda.synchronize()
    assert relocated >= n // 10 and sizes[-1] > sizes[0]
    d12_1, sph_1 = g.packed()
    assert np.isfinite(d12_1).all() and np.isfinite(sph_1).all()
    psnr_after = _psnr(oracle_images(d12_1, sph_1), teacher)
    print(f"{method}: MCMC training, N {sizes}, relocated {relocated}; PSNR vs oracle-rendered teacher {psnr_before:.2f} dB -> "
          f"{psnr_after:.2f} dB")
    assert psnr_after > psnr_before + 6.0, (psnr_before, psnr_after)
