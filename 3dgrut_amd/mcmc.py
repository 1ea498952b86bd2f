"""MCMC densification strategy on the MI355X: drop-in for the reference's `threedgrut.strategy.lib_mcmc_cc` extension and an opt-in
fused `perturb_gaussians` (threedgrut/strategy/mcmc.py), both backed by csrc/mcmc.hip, and the opt-in fused relocate / add events
backed by csrc/mcmc_events.hip.  There is no CPU fallback.

    compute_relocation_tensor(opacities, scales, ratios, binoms, n_max)   the surface of lib_mcmc_cc (bindings.cpp:39-55)
    perturb_positions_(positions, rotation, scale, density, noise, noise_lr, lr, activated=False)
    perturb_gaussians(model, noise_lr)                                     MCMCStrategy.perturb_gaussians (mcmc.py:167-187)
    classify_alive(density_act, threshold)                                 the two torch.where of relocate_gaussians (mcmc.py:112-116)
    sample_plan(sampled, density_act, scale, binoms, n_max, threshold, ...) sample_new_gaussians after its draw (mcmc.py:202-222)
    relocate_rows_(tensors, roles, plan, dead_idx) / append_rows(tensors, roles, plan)   every indexed write / cat of an event, one launch
    relocate(model, threshold, binoms, n_max) / add(model, max_n, threshold, binoms, n_max)   the two events (mcmc.py:109-165)
    install()                 registers this module as threedgrut.strategy.lib_mcmc_cc (called by the shims: the nvcc JIT is never reached)
    install_fused_perturb()   rebinds threedgrut.strategy.mcmc.MCMCStrategy to a subclass whose perturb_gaussians is the fused pass
    install_fused_events()    the same for relocate_gaussians / add_new_gaussians; the two installers stack in either order
"""
from __future__ import annotations

import ctypes as C
import sys
import types

import torch

from . import _abi

PLUGIN_MODULE = "threedgrut.strategy.lib_mcmc_cc"


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _check_input(t, name):   # CHECK_INPUT of bindings.cpp:32-37
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def compute_relocation_tensor(opacities: torch.Tensor, scales: torch.Tensor, ratios: torch.Tensor, binoms: torch.Tensor, n_max: int):
    """-> (new_opacities, new_scales), shaped like opacities / scales, computed on the current stream.  opacities [N] or [N,1] fp32,
    scales [N,3] fp32, ratios int32 [N] (clamped to [1, n_max] in the kernel), binoms fp32 [n_max, n_max] (mcmc.py:70-77)."""
    for t, name in ((opacities, "opacities"), (scales, "scales"), (ratios, "ratios"), (binoms, "binoms")):
        _check_input(t, name)
    n = int(opacities.shape[0]) if opacities.dim() else 1
    if scales.shape[0] != n:
        raise RuntimeError("scales size mismatch")
    if ratios.shape[0] != n:
        raise RuntimeError("ratios size mismatch")
    if opacities.dtype != torch.float32 or scales.dtype != torch.float32 or binoms.dtype != torch.float32:
        raise RuntimeError("opacities, scales and binoms must be float32")
    if ratios.dtype != torch.int32:
        raise RuntimeError("ratios must be int32")
    if opacities.numel() != n or ratios.numel() != n or scales.numel() != 3 * n:
        raise RuntimeError("expected opacities [N] or [N,1], scales [N,3] and ratios [N]")
    n_max = int(n_max)
    if n_max < 1 or binoms.numel() < n_max * n_max:
        raise RuntimeError(f"binoms must hold an [n_max, n_max] table (n_max = {n_max}, {binoms.numel()} entries)")
    new_opacities = torch.empty_like(opacities)
    new_scales = torch.empty_like(scales)
    if n:
        _abi.check(_abi.load_library().grut_mcmc_relocation(
            _stream(opacities), n, C.c_void_p(opacities.data_ptr()), C.c_void_p(scales.data_ptr()), C.c_void_p(ratios.data_ptr()),
            C.c_void_p(binoms.data_ptr()), n_max, C.c_void_p(new_opacities.data_ptr()), C.c_void_p(new_scales.data_ptr())),
            "grut_mcmc_relocation")
    return new_opacities, new_scales


def perturb_positions_(positions, rotation, scale, density, noise, noise_lr: float, lr: float, activated: bool = False):
    """positions += R S S^T R^T (noise * sigmoid(-100 ((1 - density) - 0.995)) * noise_lr * lr), in place (the tensor keeps its
    identity).  rotation [N,4], scale [N,3], density [N,1]: RAW parameters (activated=False: normalize / exp / sigmoid are applied in
    the kernel) or already activated; noise [N,3].  All contiguous fp32 CUDA tensors; only positions is written."""
    n = int(positions.shape[0])
    widths = ((positions, "positions", 3), (rotation, "rotation", 4), (scale, "scale", 3), (density, "density", 1), (noise, "noise", 3))
    for t, name, m in widths:
        _check_input(t, name)
        if t.dtype != torch.float32 or t.numel() != n * m or (t.dim() and t.shape[0] != n):
            raise RuntimeError(f"{name} must be a float32 [{n},{m}] tensor")
    if n:
        _abi.check(_abi.load_library().grut_mcmc_perturb(
            _stream(positions), n, C.c_void_p(positions.data_ptr()), C.c_void_p(rotation.data_ptr()), C.c_void_p(scale.data_ptr()),
            C.c_void_p(density.data_ptr()), C.c_void_p(noise.data_ptr()), float(noise_lr), float(lr), 1 if activated else 0),
            "grut_mcmc_perturb")
    return positions


def positions_lr(model) -> float:
    """The learning rate of the "positions" param group (mcmc.py:172-175: the last group of that name, 0 if there is none)."""
    lr = 0.0
    for group in model.optimizer.param_groups:
        if group.get("name") == "positions":
            lr = group["lr"]
    return lr


@torch.no_grad()
def perturb_gaussians(model, noise_lr: float) -> None:
    """MCMCStrategy.perturb_gaussians (mcmc.py:167-187) over a duck-typed model (positions Parameter, optimizer with a "positions"
    group, get_rotation / get_scale / get_density).  The noise is drawn here with torch.randn_like(positions), once, exactly as the
    reference draws it, so the global generator advances identically (later torch.multinomial draws of relocate / add match)."""
    from .gut_tracer import has_standard_activations
    positions = model.positions
    lr = positions_lr(model)
    noise = torch.randn_like(positions)
    if has_standard_activations(model):
        perturb_positions_(positions.data, model.rotation.data.contiguous(), model.scale.data.contiguous(), model.density.data.contiguous(),
                           noise, noise_lr, lr, activated=False)
    else:
        perturb_positions_(positions.data, model.get_rotation().contiguous(), model.get_scale().contiguous(), model.get_density().contiguous(),
                           noise, noise_lr, lr, activated=True)


# ---- the two periodic events: relocate_gaussians / add_new_gaussians (mcmc.py:109-165, 189-224) -----------------------------------
ROLE_COPY, ROLE_NEW_DENSITY, ROLE_NEW_SCALE, ROLE_STATE = (_abi.MCMC_ROLE_COPY, _abi.MCMC_ROLE_NEW_DENSITY, _abi.MCMC_ROLE_NEW_SCALE,
                                                           _abi.MCMC_ROLE_STATE)
_ROLE_WIDTH = {ROLE_NEW_DENSITY: 1, ROLE_NEW_SCALE: 3}

# events that ran on the HIP passes, and events handed to the replaced torch path (a failed precondition, or no alive Gaussian)
stats = types.SimpleNamespace(hip_relocations=0, hip_adds=0, torch_events=0)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _check_tensor(t, name, dtype, shape=None, cuda=True):
    """Type, dtype, layout, (with cuda) device, shape: RuntimeError before anything is launched.  Callers with several tensors pass
    cuda=False and check the devices afterwards, so that a wrong dtype or layout is named whatever device the tensors are on."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {str(dtype).replace('torch.', '')} (got {str(t.dtype).replace('torch.', '')})")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if cuda:
        _check_input(t, name)
    if shape is not None and (t.numel() != shape[0] * shape[1] or (t.dim() and t.shape[0] != shape[0])):
        raise RuntimeError(f"{name} must be a [{shape[0]},{shape[1]}] tensor (got {tuple(t.shape)})")


def _check_rows_count(n, what="the tensors"):
    if not 0 <= n < 2 ** 31:
        raise RuntimeError(f"{what} must have fewer than 2^31 rows (got {n})")


def classify_alive(density_act: torch.Tensor, threshold: float):
    """-> (dead_idx, alive_idx, alive_prob): torch.where(d <= threshold)[0], torch.where(d > threshold)[0] and d[alive_idx].flatten()
    (mcmc.py:114-115, :198), bit for bit, for the ACTIVATED densities d [N] or [N,1] (contiguous fp32 CUDA).  One scan-based compaction
    and ONE device-to-host read, of the two counts.  The results are views of buffers of N entries."""
    _check_tensor(density_act, "density_act", torch.float32)
    n = density_act.numel()
    _check_rows_count(n, "density_act")
    dev = density_act.device
    dead = torch.empty(n, dtype=torch.int64, device=dev)
    alive = torch.empty(n, dtype=torch.int64, device=dev)
    prob = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return dead, alive, prob
    lib = _abi.load_library()
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    scratch_bytes = int(lib.grut_mcmc_classify_scratch_bytes(n))
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
    _abi.check(lib.grut_mcmc_classify(_stream(density_act), n, _ptr(density_act), float(threshold), _ptr(dead), _ptr(alive), _ptr(prob),
                                      _ptr(counts), _ptr(scratch), scratch_bytes), "grut_mcmc_classify")
    n_dead, n_alive = counts.tolist()   # the only device-to-host transfer
    return dead[:n_dead], alive[:n_alive], prob[:n_alive]


class SamplePlan:
    """What one event does, on the device: source int64 [m] (the sampled Gaussians), count int32 [n] (how often each was drawn), first
    int32 [n] (the first draw of each; INT32_MAX where count is 0), the new raw values new_density_raw [m,1] / new_scale_raw [m,3] that
    the sources and their copies take, and (when asked for) the activated values before the clamp, new_density_act / new_scale_act."""

    def __init__(self, n, m, source, count, first, new_density_raw, new_scale_raw, new_density_act, new_scale_act):
        self.n, self.m, self.source, self.count, self.first = n, m, source, count, first
        self.new_density_raw, self.new_scale_raw = new_density_raw, new_scale_raw
        self.new_density_act, self.new_scale_act = new_density_act, new_scale_act


def sample_plan(sampled, density_act, scale, binoms, n_max: int, threshold: float, index_map=None, scale_activated: bool = False,
                with_activated: bool = True) -> SamplePlan:
    """sample_new_gaussians after its draw (mcmc.py:202-222) in three small kernels and no host read.  sampled int64 [m]: the draws,
    mapped through index_map (int64, e.g. alive_idx) in the kernel when given; density_act [N] or [N,1]: the ACTIVATED densities;
    scale [N,3]: raw (exp is applied in the kernel) or, with scale_activated, activated; binoms fp32 [n_max, n_max]."""
    _check_tensor(density_act, "density_act", torch.float32, cuda=False)
    n = density_act.numel()
    _check_tensor(scale, "scale", torch.float32, (n, 3), cuda=False)
    _check_tensor(sampled, "sampled", torch.int64, cuda=False)
    _check_tensor(binoms, "binoms", torch.float32, cuda=False)
    if index_map is not None:
        _check_tensor(index_map, "index_map", torch.int64, cuda=False)
        if index_map.numel() > n:
            raise RuntimeError(f"index_map has {index_map.numel()} entries for {n} rows")
    for t, name in ((density_act, "density_act"), (scale, "scale"), (sampled, "sampled"), (binoms, "binoms"), (index_map, "index_map")):
        if t is not None:
            _check_input(t, name)
            if t.device != density_act.device:
                raise RuntimeError(f"{name} is on {t.device}, density_act on {density_act.device}")
    m, n_max = sampled.numel(), int(n_max)
    _check_rows_count(n, "density_act")
    _check_rows_count(m, "sampled")
    if n_max < 1 or binoms.numel() < n_max * n_max:
        raise RuntimeError(f"binoms must hold an [n_max, n_max] table (n_max = {n_max}, {binoms.numel()} entries)")
    if m and (n == 0 or (index_map is not None and index_map.numel() == 0)):
        raise RuntimeError(f"{m} draws over no rows")
    dev = density_act.device
    f32 = dict(dtype=torch.float32, device=dev)
    plan = SamplePlan(n, m, torch.empty(m, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                      torch.empty(n, dtype=torch.int32, device=dev), torch.empty((m, 1), **f32), torch.empty((m, 3), **f32),
                      torch.empty((m, 1), **f32) if with_activated else None, torch.empty((m, 3), **f32) if with_activated else None)
    if n:
        _abi.check(_abi.load_library().grut_mcmc_sample_plan(
            _stream(density_act), n, m, _ptr(sampled), _ptr(index_map), index_map.numel() if index_map is not None else 0,
            _ptr(density_act), _ptr(scale), 1 if scale_activated else 0, _ptr(binoms), n_max, float(threshold), _ptr(plan.source),
            _ptr(plan.count), _ptr(plan.first), _ptr(plan.new_density_raw), _ptr(plan.new_scale_raw), _ptr(plan.new_density_act),
            _ptr(plan.new_scale_act)), "grut_mcmc_sample_plan")
    return plan


def _describe(tensors, roles, n):
    """The descriptor array of the two row passes, after the checks of everything the kernel will dereference."""
    tensors, roles = list(tensors), [int(r) for r in roles]
    if len(tensors) != len(roles):
        raise RuntimeError(f"{len(tensors)} tensors but {len(roles)} roles")
    if len(tensors) > _abi.MCMC_MAX_TENSORS:
        raise RuntimeError(f"at most {_abi.MCMC_MAX_TENSORS} tensors per launch (got {len(tensors)})")
    _check_rows_count(n)
    desc = (_abi.McmcTensor * max(len(tensors), 1))()
    for k, (t, role) in enumerate(zip(tensors, roles)):
        _check_tensor(t, f"tensors[{k}]", torch.float32)
        if role not in (ROLE_COPY, ROLE_NEW_DENSITY, ROLE_NEW_SCALE, ROLE_STATE):
            raise RuntimeError(f"roles[{k}] = {role} is unknown")
        if t.dim() < 1 or t.shape[0] != n:
            raise RuntimeError(f"tensors[{k}] must have {n} rows (got shape {tuple(t.shape)})")
        width = 1
        for d in t.shape[1:]:
            width *= d
        if width < 1:
            raise RuntimeError(f"tensors[{k}] has empty rows")
        if role in _ROLE_WIDTH and width != _ROLE_WIDTH[role]:
            raise RuntimeError(f"tensors[{k}] has rows of {width} elements; its role needs {_ROLE_WIDTH[role]}")
        desc[k] = _abi.McmcTensor(t.data_ptr(), width, role)
    return tensors, desc


def _check_plan(plan, n, dev):
    if plan.n != n or plan.count.device != dev:
        raise RuntimeError(f"the plan is for {plan.n} rows on {plan.count.device}, the tensors have {n} on {dev}")


def relocate_rows_(tensors, roles, plan: SamplePlan, dead_idx):
    """The indexed writes of a relocation (mcmc.py:121-131) on every tensor IN PLACE, one launch: ROLE_COPY t[dead] = t[source];
    ROLE_NEW_DENSITY / ROLE_NEW_SCALE t[source] = new, t[dead] = new; ROLE_STATE t[source] = 0.  tensors: contiguous fp32 CUDA tensors
    with plan.n rows; dead_idx int64 [plan.m]: distinct rows, none of them a source.  -> tensors."""
    tensors, desc = _describe(tensors, roles, plan.n)
    _check_tensor(dead_idx, "dead_idx", torch.int64)
    if dead_idx.numel() != plan.m:
        raise RuntimeError(f"dead_idx has {dead_idx.numel()} entries for {plan.m} draws")
    for t in tensors:
        _check_plan(plan, plan.n, t.device)
    if tensors and plan.m:
        _abi.check(_abi.load_library().grut_mcmc_relocate_rows(
            _stream(tensors[0]), desc, len(tensors), plan.m, _ptr(plan.source), _ptr(dead_idx), _ptr(plan.first),
            _ptr(plan.new_density_raw), _ptr(plan.new_scale_raw)), "grut_mcmc_relocate_rows")
    return tensors


def append_rows(tensors, roles, plan: SamplePlan):
    """-> new tensors [plan.n + plan.m, ...], one launch for all of them: what the indexed write followed by cat([t, t[source]])
    (ROLE_COPY, ROLE_NEW_*) resp. cat([t, zeros]) (ROLE_STATE) of add_new_gaussians (mcmc.py:148-158) leaves, bit for bit."""
    tensors, desc = _describe(tensors, roles, plan.n)
    _check_rows_count(plan.n + plan.m)
    for t in tensors:
        _check_plan(plan, plan.n, t.device)
    outs = [torch.empty((plan.n + plan.m, *t.shape[1:]), dtype=t.dtype, device=t.device) for t in tensors]
    if tensors and plan.n + plan.m:
        ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        _abi.check(_abi.load_library().grut_mcmc_append_rows(
            _stream(tensors[0]), desc, ptrs, len(tensors), plan.n, plan.m, _ptr(plan.source), _ptr(plan.count), _ptr(plan.first),
            _ptr(plan.new_density_raw), _ptr(plan.new_scale_raw)), "grut_mcmc_append_rows")
    return outs


class EventRecord:
    """What relocate() / add() did: n_dead, n_added, n_before, n_after; dead_idx (relocate), source, count and the plan's new values
    (None where nothing was drawn)."""

    def __init__(self, n_before, n_after, n_dead=0, n_added=0, dead_idx=None, plan=None):
        self.n_before, self.n_after, self.n_dead, self.n_added, self.dead_idx, self.plan = n_before, n_after, n_dead, n_added, dead_idx, plan
        for name in ("source", "count", "first", "new_density_raw", "new_scale_raw", "new_density_act", "new_scale_act"):
            setattr(self, name, getattr(plan, name) if plan is not None else None)


def _event_tensors(model):
    """-> (n, groups, tensors, roles) over model.optimizer.param_groups, or None when a precondition of the fused passes fails: one
    contiguous fp32 CUDA tensor of N rows per named group, every optimizer-state entry besides `step` a tensor shaped like its
    parameter, raw density [N,1] / scale [N,3] with the default activations, at most 32 tensors, N < 2^31."""
    from .gut_tracer import has_standard_activations

    def ok(t):
        return isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.dim() >= 1

    optimizer = getattr(model, "optimizer", None)
    if optimizer is None or not has_standard_activations(model):
        return None
    density, scale = model.density.data, model.scale.data
    if not (ok(density) and ok(scale)) or not 0 < density.shape[0] < 2 ** 31:
        return None
    n, dev = density.shape[0], density.device
    if density.numel() != n or scale.numel() != 3 * n or scale.shape[0] != n or scale.device != dev:
        return None
    groups, tensors, roles = [], [], []
    for group in optimizer.param_groups:
        if len(group["params"]) != 1 or "name" not in group:
            return None
        p = group["params"][0]
        if not ok(p.data) or p.shape[0] != n or p.device != dev or p.numel() == 0:
            return None
        name = group["name"]
        if (name == "density" and p is not model.density) or (name == "scale" and p is not model.scale):
            return None
        state = optimizer.state.get(p, {})
        tensors.append(p.data)
        roles.append(ROLE_NEW_DENSITY if name == "density" else ROLE_NEW_SCALE if name == "scale" else ROLE_COPY)
        for key, v in state.items():
            if key == "step":
                continue
            if not ok(v) or v.shape != p.shape or v.device != dev:
                return None
            tensors.append(v)
            roles.append(ROLE_STATE)
        groups.append((group, p, state))
    if not groups or len(tensors) > _abi.MCMC_MAX_TENSORS:
        return None
    return n, groups, tensors, roles


def _rebind(model, groups, new_tensors):
    """The contract of _update_param_with_optimizer (strategy/base.py:77-107): every group gets a NEW Parameter (requires_grad kept)
    that takes over the old one's optimizer state (`step` untouched, the other entries in the order they were listed), setattr."""
    optimizer, it = model.optimizer, iter(new_tensors)
    for group, old, _ in groups:
        state = optimizer.state.pop(old, {})
        fresh = torch.nn.Parameter(next(it), requires_grad=old.requires_grad)
        for key in state:
            if key != "step":
                state[key] = next(it)
        group["params"] = [fresh]
        optimizer.state[fresh] = state
        setattr(model, group["name"], fresh)


def _as_draws(sampled, dev):
    return sampled.to(device=dev, dtype=torch.int64).contiguous()


def _replaced_sample(model, num, valid, threshold, binoms, n_max, sampler):   # sample_new_gaussians (mcmc.py:189-224)
    densities, scales = model.get_density(), model.get_scale()
    if valid is None:
        valid = torch.arange(0, int(densities.shape[0]), device=densities.device, dtype=torch.int32)
    idx = valid[sampler(densities[valid].flatten(), num, replacement=True)]
    ratios = (torch.bincount(idx)[idx] + 1).clamp_(min=1, max=n_max).int()
    new_d, new_s = compute_relocation_tensor(densities[idx].contiguous(), scales[idx].contiguous(), ratios.contiguous(), binoms, n_max)
    new_d = model.density_activation_inv(torch.clamp(new_d, max=1.0 - torch.finfo(torch.float32).eps, min=threshold))
    return idx, new_d, model.scale_activation_inv(new_s)


def _replaced_update(model, param_fn, state_fn):   # _update_param_with_optimizer (strategy/base.py:77-107)
    optimizer = model.optimizer
    for group in optimizer.param_groups:
        old = group["params"][0]
        state = optimizer.state.pop(old, {})
        for key in state:
            if key != "step":
                state[key] = state_fn(state[key])
        fresh = torch.nn.Parameter(param_fn(group["name"], old.data), requires_grad=old.requires_grad)
        group["params"] = [fresh]
        optimizer.state[fresh] = state
        setattr(model, group["name"], fresh)


def _replaced_relocate(model, threshold, binoms, n_max, sampler):
    """relocate_gaussians (mcmc.py:109-136) as the chain of torch indexing it is: the path of a model the fused passes do not take."""
    densities = model.get_density()
    dead = torch.where(densities <= threshold)[0]
    alive = torch.where(densities > threshold)[0]
    n = int(densities.shape[0])
    if not len(dead):
        return EventRecord(n, n)
    idx, new_d, new_s = _replaced_sample(model, len(dead), alive, threshold, binoms, n_max, sampler)

    def param_fn(name, p):
        if name == "density":
            p[idx] = new_d
        elif name == "scale":
            p[idx] = new_s
        p[dead] = p[idx]
        return p

    def state_fn(v):
        v[idx] = 0
        return v

    _replaced_update(model, param_fn, state_fn)
    return EventRecord(n, n, n_dead=len(dead), dead_idx=dead)


def _replaced_add(model, num, threshold, binoms, n_max, sampler):
    """add_new_gaussians (mcmc.py:145-160) as the chain of torch indexing and torch.cat it is."""
    n = int(model.get_density().shape[0])
    idx, new_d, new_s = _replaced_sample(model, num, None, threshold, binoms, n_max, sampler)

    def param_fn(name, p):
        if name == "density":
            p[idx] = new_d
        elif name == "scale":
            p[idx] = new_s
        return torch.cat([p, p[idx]])

    _replaced_update(model, param_fn, lambda v: torch.cat([v, torch.zeros((len(idx), *v.shape[1:]), device=v.device)]))
    return EventRecord(n, n + num, n_added=num)


@torch.no_grad()
def relocate(model, threshold: float, binoms, n_max: int, sampler=None, *, fallback=None):
    """MCMCStrategy.relocate_gaussians (mcmc.py:109-136) over a duck-typed model (raw density / scale Parameters with the default
    activations, get_density(), optimizer with named one-tensor groups): dead Gaussians (density <= threshold) move onto alive ones
    drawn by `sampler` (default torch.multinomial), which is called once as sampler(p, n_dead, replacement=True) with the reference's
    p, and not at all when nothing is dead: the global generator advances as in the reference.  One host read (the two counts), four
    small kernels and ONE launch over every parameter and moment.  -> EventRecord.
    A model that fails a precondition of _event_tensors(), or one without an alive Gaussian, takes the replaced torch path (counted in
    stats.torch_events): `fallback()` when given (its result is returned), the restatement in this module otherwise."""
    sampler = sampler or torch.multinomial
    found = _event_tensors(model)
    if found is not None:
        n, groups, tensors, roles = found
        density_act = model.get_density()
        if not (isinstance(density_act, torch.Tensor) and density_act.is_cuda and density_act.is_contiguous()
                and density_act.dtype == torch.float32 and density_act.numel() == n and binoms.is_cuda):
            found = None
    if found is not None:
        dead_idx, alive_idx, alive_prob = classify_alive(density_act, threshold)
        n_dead = dead_idx.shape[0]
        if n_dead == 0:
            stats.hip_relocations += 1
            return EventRecord(n, n, dead_idx=dead_idx)
        if alive_idx.shape[0]:
            sampled = _as_draws(sampler(alive_prob, n_dead, replacement=True), density_act.device)
            plan = sample_plan(sampled, density_act, model.scale.data, binoms, n_max, threshold, index_map=alive_idx)
            relocate_rows_(tensors, roles, plan, dead_idx)
            _rebind(model, groups, tensors)   # new Parameters over the same storage, as the reference's (mcmc.py:127)
            stats.hip_relocations += 1
            return EventRecord(n, n, n_dead=n_dead, dead_idx=dead_idx, plan=plan)
    stats.torch_events += 1
    return fallback() if fallback is not None else _replaced_relocate(model, threshold, binoms, n_max, sampler)


@torch.no_grad()
def add(model, max_n: int, threshold: float, binoms, n_max: int, sampler=None, *, fallback=None):
    """MCMCStrategy.add_new_gaussians (mcmc.py:138-165): min(max_n, int(1.05 N)) - N new Gaussians, copies of ones drawn by `sampler`
    (called once as sampler(p, n_add, replacement=True) over all densities; not at all when nothing is to be added).  No host read
    (the size is host arithmetic), three small kernels and ONE launch that writes every new parameter and moment.  -> EventRecord.
    Preconditions and `fallback` as for relocate()."""
    sampler = sampler or torch.multinomial
    n = int(model.num_gaussians) if hasattr(model, "num_gaussians") else int(model.density.shape[0])
    num = max(0, min(int(max_n), int(1.05 * n)) - n)
    if num == 0:
        return EventRecord(n, n)
    found = _event_tensors(model)
    if found is not None and found[0] == n and n + num < 2 ** 31:
        _, groups, tensors, roles = found
        density_act = model.get_density()
        if (isinstance(density_act, torch.Tensor) and density_act.is_cuda and density_act.is_contiguous()
                and density_act.dtype == torch.float32 and density_act.numel() == n and binoms.is_cuda):
            sampled = _as_draws(sampler(density_act.flatten(), num, replacement=True), density_act.device)
            plan = sample_plan(sampled, density_act, model.scale.data, binoms, n_max, threshold)
            _rebind(model, groups, append_rows(tensors, roles, plan))
            stats.hip_adds += 1
            return EventRecord(n, n + num, n_added=num, plan=plan)
    stats.torch_events += 1
    return fallback() if fallback is not None else _replaced_add(model, num, threshold, binoms, n_max, sampler)


def install() -> None:
    """Make `from . import lib_mcmc_cc` in threedgrut/strategy/mcmc.py:41 bind to this module (MCMCStrategy's plugin: relocation).
    Imports nothing of threedgrut: the shims call it while threedgrut/model/model.py is still being imported."""
    sys.modules.setdefault(PLUGIN_MODULE, sys.modules[__name__])


def install_fused_perturb():
    """Opt-in: replace threedgrut.strategy.mcmc.MCMCStrategy with a subclass whose perturb_gaussians is the one-pass HIP kernel.
    The trainer looks the class up when it builds its strategy (trainer.py:259-262), so call this before constructing the trainer.
    Returns the subclass; calling it again returns the same class."""
    install()
    mod = __import__("threedgrut.strategy.mcmc", fromlist=["MCMCStrategy"])
    base = mod.MCMCStrategy
    if getattr(base, "_grut_fused_perturb", False):
        return base

    class MCMCStrategy(base):
        _grut_fused_perturb = True

        @torch.no_grad()
        def perturb_gaussians(self) -> None:
            perturb_gaussians(self.model, self.conf.strategy.perturb.noise_lr)

    MCMCStrategy.__qualname__ = MCMCStrategy.__name__ = "MCMCStrategy"
    MCMCStrategy.__module__ = __name__
    mod.MCMCStrategy = MCMCStrategy
    return MCMCStrategy


def install_fused_events():
    """Opt-in: replace threedgrut.strategy.mcmc.MCMCStrategy with a subclass OF THE CLASS BOUND THERE (the reference's, or the one
    install_fused_perturb() left: the two installers stack in either order) whose relocate_gaussians / add_new_gaussians are relocate()
    / add() above, with the reference's _multinomial_sample as sampler (its numpy path above 2^24 probabilities stays the reference's)
    and the reference's log lines.  A model that fails a precondition goes through the base class's method.  Call it before constructing
    the trainer (trainer.py:259-262).  Returns the subclass; calling it again returns the same class."""
    install()
    mod = __import__("threedgrut.strategy.mcmc", fromlist=["MCMCStrategy"])
    base = mod.MCMCStrategy
    if getattr(base, "_grut_fused_events", False):
        return base

    class MCMCStrategy(base):
        _grut_fused_events = True

        @torch.no_grad()
        def relocate_gaussians(self) -> None:
            s = self.conf.strategy
            rec = relocate(self.model, s.opacity_threshold, self.binoms, s.binom_n_max, sampler=mod._multinomial_sample,
                           fallback=super().relocate_gaussians)
            if rec is not None and s.print_stats:   # (the base class's method logs for itself)
                mod.logger.info(f"Relocated {rec.n_dead} ({rec.n_dead / rec.n_before * 100:.2f}%) gaussians")

        @torch.no_grad()
        def add_new_gaussians(self) -> None:
            s = self.conf.strategy
            rec = add(self.model, s.add.max_n_gaussians, s.opacity_threshold, self.binoms, s.binom_n_max, sampler=mod._multinomial_sample,
                      fallback=super().add_new_gaussians)
            if rec is not None and s.print_stats:
                mod.logger.info(f"Added {rec.n_added} ({rec.n_added / rec.n_before * 100:.2f}%) gaussians")

    MCMCStrategy.__qualname__ = MCMCStrategy.__name__ = "MCMCStrategy"
    MCMCStrategy.__module__ = __name__
    mod.MCMCStrategy = MCMCStrategy
    return MCMCStrategy
