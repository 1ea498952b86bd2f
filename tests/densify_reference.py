"""Plain-torch restatement of the default densification strategy (the method names and the observable behaviour of
threedgrut/strategy/gs.py and strategy/base.py, written anew): what tests/test_densify_gpu.py compares the HIP path against where
the reference checkout is absent.  Everything takes a `dtype`, so the same code is the float64 yardstick and the fp32 control.

    accumulate_reference / split_tail_reference / relayout_reference    the three device functions, out of place
    accumulate_indexed_                                                 the statistic by boolean indexing, in place (benchmark baseline)
    DuckModel                                                           six raw parameter tensors, activations and an optimizer
    RestatedGSStrategy                                                  the strategy, by boolean indexing and torch.cat
"""
import types

import torch

SH_ROW = 45   # SH degree 3: 15 coefficients x 3 channels besides the albedo


def accumulate_reference(accum, denom, grad, positions, sensor_position, dtype=torch.float64):
    """-> (accum', denom'): rows with any non-zero gradient component gain ||g * ||p - c|| || / 2 resp. 1, in `dtype`."""
    has = (grad != 0).any(dim=1, keepdim=True)
    dist = (positions.to(dtype) - sensor_position.to(dtype)).norm(dim=1, keepdim=True)
    inc = (grad.to(dtype) * dist).norm(dim=1, keepdim=True) / 2
    acc = accum.to(dtype).reshape(-1, 1)
    return torch.where(has, acc + inc, acc).reshape(accum.shape), denom + has.reshape(denom.shape).to(denom.dtype)


def accumulate_indexed_(accum, denom, grad, positions, sensor_position):
    """The same statistic in fp32 and in place, the way an implementation that selects rows with a boolean mask pays for it: two
    masked gathers and two masked read-modify-writes (each one a nonzero and a host wait on the GPU).  The baseline of
    scripts/bench_densify.py."""
    moved = grad.ne(0).any(dim=1)
    reach = torch.linalg.vector_norm(positions[moved] - sensor_position, dim=1, keepdim=True)
    accum[moved] += 0.5 * torch.linalg.vector_norm(grad[moved] * reach, dim=1, keepdim=True)
    denom[moved] += 1


def rotation_matrices(q):
    """[M,4] (w, x, y, z), not normalised -> [M,3,3]."""
    w, x, y, z = (q / q.norm(dim=1, keepdim=True)).unbind(dim=1)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def split_tail_reference(positions, scale, rotation, noise, copies, dtype=torch.float64):
    """-> (positions + R (noise * exp(scale)), log(exp(scale) / (0.8 copies)), max_k |noise * exp(scale)| per row), in `dtype`."""
    sigma = torch.exp(scale.to(dtype))
    sample = noise.to(dtype) * sigma
    offset = torch.bmm(rotation_matrices(rotation.to(dtype)), sample.unsqueeze(-1)).squeeze(-1)
    return positions.to(dtype) + offset, torch.log(sigma / (0.8 * copies)), sample.abs().amax(dim=1, keepdim=True)


def split_position_bound(positions64, sample_max):
    """2^-24 |p| + 64 2^-24 max|noise * sigma| per component: the final add, plus ~20 roundings of normalisation, matrix entries and
    the 3-term dot, tripled."""
    return 2.0 ** -24 * positions64.abs() + 64 * 2.0 ** -24 * sample_max


def relayout_reference(v, keep, append, copies, zero):
    n = v.shape[0]
    kept = v if keep is None else v[keep]
    block = v[:0] if append is None else v[append]
    block = block.repeat(copies, *([1] * (v.dim() - 1)))
    return torch.cat([kept, torch.zeros_like(block) if zero else block])


class DuckModel:
    """The attributes of the reference's MixtureOfGaussians that the strategy touches."""
    NAMES = (("positions", 3), ("rotation", 4), ("scale", 3), ("density", 1), ("features_albedo", 3), ("features_specular", SH_ROW))

    def __init__(self, n, device, seed=0, optimizer="adam"):
        g = torch.Generator().manual_seed(seed)
        self.device = device
        raw = {"positions": torch.randn((n, 3), generator=g) * 2,
               "rotation": torch.nn.functional.normalize(torch.randn((n, 4), generator=g)) * (0.1 + 9.9 * torch.rand((n, 1), generator=g)),
               "scale": -8 * torch.rand((n, 3), generator=g),
               "density": torch.randn((n, 1), generator=g) * 3,
               "features_albedo": torch.randn((n, 3), generator=g),
               "features_specular": torch.randn((n, SH_ROW), generator=g) * 0.1}
        for name, _ in self.NAMES:
            setattr(self, name, torch.nn.Parameter(raw[name].to(device)))
        self.scale_activation, self.scale_activation_inv = torch.exp, torch.log
        self.density_activation = torch.sigmoid
        self.density_activation_inv = lambda x: torch.log(x / (1 - x))
        self.rotation_activation = torch.nn.functional.normalize
        groups = [{"params": [getattr(self, name)], "name": name, "lr": 1e-3} for name, _ in self.NAMES]
        if optimizer == "adam":
            self.optimizer = torch.optim.Adam(groups, lr=1e-3, eps=1e-15)
        else:
            self.optimizer = optimizer(groups, lr=1e-3, eps=1e-15)

    def seed_optimizer_state(self, seed=1):
        """exp_avg / exp_avg_sq / step as after some steps, without running one (the same numbers for every optimizer class)."""
        g = torch.Generator().manual_seed(seed)
        for name, _ in self.NAMES:
            p = getattr(self, name)
            self.optimizer.state[p] = {"step": torch.tensor(7.0), "exp_avg": (torch.randn(p.shape, generator=g) * 1e-3).to(p.device),
                                       "exp_avg_sq": (torch.rand(p.shape, generator=g) * 1e-6).to(p.device)}

    @property
    def num_gaussians(self):
        return self.positions.shape[0]

    def get_positions(self):
        return self.positions

    def get_scale(self):
        return self.scale_activation(self.scale)

    def get_density(self):
        return self.density_activation(self.density)


def make_conf(split_n=2, print_stats=False):
    ns = types.SimpleNamespace
    return ns(strategy=ns(print_stats=print_stats,
                          densify=ns(split=ns(n_gaussians=split_n), relative_size_threshold=0.01, clone_grad_threshold=2e-4, split_grad_threshold=2e-4),
                          prune=ns(density_threshold=0.01), reset_density=ns(new_max_density=0.01)))


class RestatedGSStrategy:
    """The default strategy by boolean indexing and torch.cat.  Same attribute and method names as the reference class, so that
    `class Fused(FusedGSStrategyMixin, RestatedGSStrategy)` is the fused strategy over this base."""

    def __init__(self, config, model):
        self.conf, self.model = config, model
        s = config.strategy
        self.split_n_gaussians = s.densify.split.n_gaussians
        self.relative_size_threshold = s.densify.relative_size_threshold
        self.clone_grad_threshold, self.split_grad_threshold = s.densify.clone_grad_threshold, s.densify.split_grad_threshold
        self.prune_density_threshold = s.prune.density_threshold
        self.new_max_density = s.reset_density.new_max_density
        n = model.num_gaussians
        self.densify_grad_norm_accum = torch.zeros((n, 1), dtype=torch.float32, device=model.device)
        self.densify_grad_norm_denom = torch.zeros((n, 1), dtype=torch.int32, device=model.device)

    @torch.no_grad()
    def update_gradient_buffer(self, sensor_position):
        self.densify_grad_norm_accum, self.densify_grad_norm_denom = accumulate_reference(
            self.densify_grad_norm_accum, self.densify_grad_norm_denom, self.model.positions.grad, self.model.positions.data,
            sensor_position, dtype=torch.float32)

    @torch.no_grad()
    def _rebuild(self, new_param, new_state, names=None):
        """Every named group: a new Parameter (same requires_grad) takes over the old one's optimizer state, whose tensors other than
        `step` go through new_state; the model attribute is rebound."""
        opt = self.model.optimizer
        for group in opt.param_groups:
            if names is not None and group["name"] not in names:
                continue
            old = group["params"][0]
            state = opt.state.pop(old, {})
            for key in list(state):
                if key != "step":
                    state[key] = new_state(state[key])
            fresh = torch.nn.Parameter(new_param(group["name"], old.data), requires_grad=old.requires_grad)
            group["params"] = [fresh]
            opt.state[fresh] = state
            setattr(self.model, group["name"], fresh)

    def reset_densification_buffers(self):
        n = self.model.num_gaussians
        self.densify_grad_norm_accum = torch.zeros((n, 1), dtype=self.densify_grad_norm_accum.dtype, device=self.model.device)
        self.densify_grad_norm_denom = torch.zeros((n, 1), dtype=self.densify_grad_norm_denom.dtype, device=self.model.device)

    def prune_densification_buffers(self, valid_mask):
        self.densify_grad_norm_accum = self.densify_grad_norm_accum[valid_mask]
        self.densify_grad_norm_denom = self.densify_grad_norm_denom[valid_mask]

    def densify_gaussians(self, scene_extent):
        norm = self.densify_grad_norm_accum / self.densify_grad_norm_denom
        norm = torch.where(norm.isnan(), torch.zeros_like(norm), norm)
        self.clone_gaussians(norm.squeeze(1), scene_extent)
        self.split_gaussians(norm.squeeze(1), scene_extent)

    @torch.no_grad()
    def clone_gaussians(self, densify_grad_norm, scene_extent):
        small = self.model.get_scale().amax(dim=1) <= self.relative_size_threshold * scene_extent
        mask = (densify_grad_norm >= self.clone_grad_threshold) & small
        self._rebuild(lambda name, v: relayout_reference(v, None, mask, 1, zero=False), lambda v: relayout_reference(v, None, mask, 1, zero=True))
        self.reset_densification_buffers()

    @torch.no_grad()
    def split_gaussians(self, densify_grad_norm, scene_extent):
        model, k = self.model, self.split_n_gaussians
        norm = torch.zeros(model.num_gaussians, device=model.device)
        norm[: densify_grad_norm.shape[0]] = densify_grad_norm          # the clones appended meanwhile have no gradient norm
        mask = (norm >= self.split_grad_threshold) & (model.get_scale().amax(dim=1) > self.relative_size_threshold * scene_extent)
        stds = model.get_scale()[mask].repeat(k, 1)
        samples = torch.normal(mean=torch.zeros_like(stds), std=stds)
        offsets = torch.bmm(rotation_matrices(model.rotation.data[mask]).repeat(k, 1, 1), samples.unsqueeze(-1)).squeeze(-1)

        def new_param(name, v):
            out = relayout_reference(v, ~mask, mask, k, zero=False)
            tail = out[out.shape[0] - offsets.shape[0]:]
            if name == "positions":
                tail += offsets
            elif name == "scale":
                tail.copy_(model.scale_activation_inv(model.scale_activation(tail) / (0.8 * k)))
            return out

        self._rebuild(new_param, lambda v: relayout_reference(v, ~mask, mask, k, zero=True))
        self.reset_densification_buffers()

    @torch.no_grad()
    def prune_gaussians_opacity(self):
        mask = self.model.get_density().squeeze(1) >= self.prune_density_threshold
        self._rebuild(lambda name, v: v[mask], lambda v: v[mask])
        self.prune_densification_buffers(mask)

    @torch.no_grad()
    def reset_density(self):
        cap = self.model.density_activation_inv(torch.tensor(self.new_max_density)).item()
        self._rebuild(lambda name, v: v.clamp(max=cap), torch.zeros_like, names=["density"])
