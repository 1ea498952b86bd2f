"""Plain-torch restatement of the MCMC strategy's two periodic events (the observable behaviour of relocate_gaussians,
add_new_gaussians and sample_new_gaussians of threedgrut/strategy/mcmc.py and of the update contract of strategy/base.py, written anew):
the yardstick of tests/test_mcmc_events_gpu.py and the baseline of scripts/bench_mcmc_events.py.  tests/test_mcmc_events_cpu.py holds
it against the reference's own class, bit for bit.

    torch_relocation(opacities, scales, ratios, binoms, n_max)   the relocation formula in fp32 torch ops, on any device
    binomial_table(n_max, device)                                 the strategy's [n_max, n_max] table
    RestatedMCMCEvents(model, ...)                                the two events over a duck model (densify_reference.DuckModel)
    snapshot(model) / clone_model(model)                          what the tests compare and how they start from identical copies
"""
import copy
import math

import torch

from densify_reference import SH_ROW, DuckModel  # noqa: F401  (re-exported: the duck model the events run over)


def binomial_table(n_max, device):
    rows = [[math.comb(n, k) if k <= n else 0 for k in range(n_max)] for n in range(n_max)]
    return torch.tensor(rows, dtype=torch.float32, device=device)


def torch_relocation(opacities, scales, ratios, binoms, n_max):
    """new_o = 1 - (1 - o)^(1/n), new_s = o / D * s with D = sum_{i=1..n} sum_{k<i} binoms[i-1, k] (-1)^k / sqrt(k+1) new_o^(k+1), the
    running sum in fp32 with i outer and k inner.  Shapes as the extension's: opacities [M] or [M,1], scales [M,3], ratios int [M]."""
    o = opacities.reshape(-1)
    n = ratios.reshape(-1).clamp(1, n_max)
    new_o = 1.0 - torch.pow(1.0 - o, 1.0 / n.to(torch.float32))
    total = torch.zeros_like(o)
    for i in range(1, int(n.max().item()) + 1 if o.numel() else 1):
        active = n >= i
        for k in range(i):
            term = (-1.0 if k & 1 else 1.0) / math.sqrt(k + 1) * torch.pow(new_o, float(k + 1))
            total = torch.where(active, total + binoms[i - 1, k] * term, total)
    return new_o.reshape(opacities.shape), (o / total)[:, None] * scales


class RestatedMCMCEvents:
    """relocate() and add() by torch indexing, one tensor at a time.  `relocation` is the function behind compute_relocation_tensor
    (the product's kernel on the GPU, torch_relocation anywhere); `sampler` draws like torch.multinomial."""

    def __init__(self, model, threshold=0.005, n_max=51, max_n=10 ** 9, relocation=torch_relocation, sampler=torch.multinomial, binoms=None):
        self.model, self.threshold, self.n_max, self.max_n = model, threshold, n_max, max_n
        self.relocation, self.sampler = relocation, sampler
        self.binoms = binomial_table(n_max, model.device) if binoms is None else binoms

    @torch.no_grad()
    def _rebuild(self, new_param, new_state):
        """Every group: a new Parameter (same requires_grad) takes over the old one's optimizer state, whose tensors other than `step`
        go through new_state (before the parameter is touched); the model attribute is rebound."""
        opt = self.model.optimizer
        for group in opt.param_groups:
            old = group["params"][0]
            state = opt.state.pop(old, {})
            for key in list(state):
                if key != "step":
                    state[key] = new_state(state[key])
            fresh = torch.nn.Parameter(new_param(group["name"], old.data), requires_grad=old.requires_grad)
            group["params"] = [fresh]
            opt.state[fresh] = state
            setattr(self.model, group["name"], fresh)

    @torch.no_grad()
    def draw(self, num, candidates=None):
        """-> (picks, new raw densities [num,1], new raw scales [num,3]): `num` Gaussians drawn in proportion to their density among
        `candidates` (all of them if None), split into count + 1 copies each."""
        density, scale = self.model.get_density(), self.model.get_scale()
        if candidates is None:
            candidates = torch.arange(density.shape[0], device=density.device, dtype=torch.int32)
        picks = candidates[self.sampler(density[candidates].flatten(), num, replacement=True)]
        copies = (torch.bincount(picks)[picks] + 1).clamp(1, self.n_max).to(torch.int32)
        new_o, new_s = self.relocation(density[picks].contiguous(), scale[picks].contiguous(), copies.contiguous(), self.binoms, self.n_max)
        new_o = new_o.clamp(min=self.threshold, max=1.0 - torch.finfo(torch.float32).eps)
        return picks, self.model.density_activation_inv(new_o), self.model.scale_activation_inv(new_s)

    def _with_new_values(self, name, v, picks, new_density, new_scale):
        if name == "density":
            v[picks] = new_density
        elif name == "scale":
            v[picks] = new_scale
        return v

    @torch.no_grad()
    def relocate(self):
        """-> dict(n_dead, dead, picks, new_density, new_scale).  Nothing is drawn when nothing is dead."""
        density = self.model.get_density()
        dead = torch.where(density <= self.threshold)[0]
        alive = torch.where(density > self.threshold)[0]
        out = dict(n_dead=int(dead.shape[0]), dead=dead, picks=None, new_density=None, new_scale=None)
        if out["n_dead"] == 0:
            return out
        picks, new_density, new_scale = self.draw(out["n_dead"], alive)

        def new_param(name, v):
            v = self._with_new_values(name, v, picks, new_density, new_scale)
            v[dead] = v[picks]
            return v

        def new_state(v):
            v[picks] = 0
            return v

        self._rebuild(new_param, new_state)
        out.update(picks=picks, new_density=new_density, new_scale=new_scale)
        return out

    @torch.no_grad()
    def add(self):
        """-> dict(n_added, picks, new_density, new_scale): grows by 5 % up to max_n.  Nothing is drawn when nothing is added."""
        n = self.model.num_gaussians
        num = max(0, min(self.max_n, int(1.05 * n)) - n)
        out = dict(n_added=num, picks=None, new_density=None, new_scale=None)
        if num == 0:
            return out
        picks, new_density, new_scale = self.draw(num)

        def new_param(name, v):
            v = self._with_new_values(name, v, picks, new_density, new_scale)
            return torch.cat([v, v[picks]])

        self._rebuild(new_param, lambda v: torch.cat([v, torch.zeros((num, *v.shape[1:]), device=v.device)]))
        out.update(picks=picks, new_density=new_density, new_scale=new_scale)
        return out


def clone_model(model):
    """An independent copy of a DuckModel: same parameter and moment bits, its own optimizer."""
    twin = copy.copy(model)
    groups = []
    for g in model.optimizer.param_groups:
        p = torch.nn.Parameter(g["params"][0].detach().clone(), requires_grad=g["params"][0].requires_grad)
        setattr(twin, g["name"], p)
        groups.append({"params": [p], "name": g["name"], "lr": g["lr"]})
    twin.optimizer = type(model.optimizer)(groups, lr=1e-3, eps=1e-15)
    for g_old, g_new in zip(model.optimizer.param_groups, twin.optimizer.param_groups):
        state = model.optimizer.state.get(g_old["params"][0])
        if state is not None:
            twin.optimizer.state[g_new["params"][0]] = {k: v.clone() for k, v in state.items()}
    return twin


def snapshot(model):
    """{name: (parameter bits, {key: moment bits or step})} in group order."""
    out = {}
    for g in model.optimizer.param_groups:
        p = g["params"][0]
        assert getattr(model, g["name"]) is p
        out[g["name"]] = (p.detach().clone(), {k: v.clone() for k, v in model.optimizer.state.get(p, {}).items()})
    return out
