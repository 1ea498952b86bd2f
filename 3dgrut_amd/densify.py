"""Default densification strategy on the MI355X: the per-step gradient statistic and the row relayout of clone / split / prune of the
reference's `GSStrategy` (threedgrut/strategy/gs.py), backed by csrc/densify.hip.  There is no CPU fallback.

    accumulate_grad_stats_(accum, denom, positions_grad, positions, sensor_position)   update_gradient_buffer (gs.py:131-139), one pass
    relayout(tensors, keep=None, append=None, copies=1, zero_append=())                cat([v[keep], v[append].repeat(copies, 1)]) per tensor
    relayout_plan(keep, append, n, device)                                             the scan and the one host read, reusable: relayout(..., plan=)
    split_tail_(positions, scale, rotation, noise, n_keep, copies)                     the appended block of a split (gs.py:168-186)
    install_fused_gs_strategy()   rebinds threedgrut.strategy.gs.GSStrategy to a subclass that drives the three functions above
"""
from __future__ import annotations

import ctypes as C
import logging

import torch

from . import _abi

APPEND_COPY, APPEND_ZERO = 0, 1   # GRUT_APPEND_* of include/grut_amd.h


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _check_input(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _check_rows(t, name, n, width, dtype=torch.float32):
    _check_input(t, name)
    if t.dtype != dtype or t.numel() != n * width or (t.dim() and t.shape[0] != n):
        raise RuntimeError(f"{name} must be a {str(dtype).replace('torch.', '')} [{n},{width}] tensor")


def accumulate_grad_stats_(accum, denom, positions_grad, positions, sensor_position):
    """accum[i] += ||positions_grad[i] * ||positions[i] - sensor_position|||| / 2 and denom[i] += 1 for the rows of positions_grad with
    a non-zero component (NaN counts), in place; every other row keeps its bits.  accum fp32 [N] or [N,1], denom int32 likewise,
    positions_grad / positions fp32 [N,3] contiguous; sensor_position: 3 fp32 values on the device, any stride (read in place)."""
    n = int(positions.shape[0])
    _check_rows(positions, "positions", n, 3)
    _check_rows(positions_grad, "positions_grad", n, 3)
    _check_rows(accum, "accum", n, 1)
    _check_rows(denom, "denom", n, 1, torch.int32)
    if not sensor_position.is_cuda:
        raise RuntimeError("sensor_position must be a CUDA tensor")
    if sensor_position.dtype != torch.float32 or sensor_position.dim() != 1 or sensor_position.shape[0] != 3:
        raise RuntimeError("sensor_position must be a float32 [3] tensor (a strided view is read in place)")
    if n:
        _abi.check(_abi.load_library().grut_densify_accumulate(
            _stream(positions), n, _ptr(positions_grad), _ptr(positions), _ptr(sensor_position), int(sensor_position.stride(0)),
            _ptr(accum), _ptr(denom)), "grut_densify_accumulate")
    return accum, denom


def _check_mask(mask, name, n):
    if mask is None:
        return
    _check_input(mask, name)
    if mask.dtype != torch.bool or mask.dim() != 1 or mask.shape[0] != n:
        raise RuntimeError(f"{name} must be a bool [{n}] tensor")


class RelayoutPlan:
    """The destinations of one (keep, append) pair over n rows: the masks, their exclusive offsets on the device and the two counts on
    the host.  Made by relayout_plan(); relayout(..., plan=) applies it to any number of tensors without scanning or reading again."""

    def __init__(self, n, keep, append, offsets, n_keep, n_append):
        self.n, self.keep, self.append, self.offsets, self.n_keep, self.n_append = n, keep, append, offsets, n_keep, n_append


def relayout_plan(keep, append, n: int, device) -> RelayoutPlan:
    """One scan of the two masks (either may be None: keep all / append none) and ONE device-to-host read, of the two counts."""
    n = int(n)
    _check_mask(keep, "keep", n)
    _check_mask(append, "append", n)
    if not 0 <= n < 2 ** 31:
        raise RuntimeError("relayout supports fewer than 2^31 rows")
    if n == 0:
        return RelayoutPlan(0, keep, append, None, 0, 0)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("relayout_plan needs a CUDA device")
    lib = _abi.load_library()
    offsets = torch.empty((2, (n + 3) // 4 * 4), dtype=torch.int32, device=device)   # rows 16-byte aligned
    counts = torch.empty(2, dtype=torch.int32, device=device)
    scratch_bytes = int(lib.grut_relayout_scratch_bytes(n))
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=device)
    _abi.check(lib.grut_relayout_scan(_stream(offsets), n, _ptr(keep), _ptr(append), _ptr(offsets[0]), _ptr(offsets[1]), _ptr(counts),
                                      _ptr(scratch), scratch_bytes), "grut_relayout_scan")
    n_keep, n_append = counts.tolist()   # the only device-to-host transfer
    return RelayoutPlan(n, keep, append, offsets, n_keep, n_append)


def relayout(tensors, keep=None, append=None, copies: int = 1, zero_append=(), plan: RelayoutPlan | None = None):
    """-> (new_tensors, n_keep, n_append) with new_tensors[j] = cat([t[keep], t[append].repeat(copies, 1, ...)]) for every t in
    `tensors` (bit for bit; the appended block is zeros for the indices listed in zero_append).  keep = None keeps every row, append =
    None appends none.  All tensors are contiguous CUDA tensors of 4-byte elements (float32 / int32) with the same first dimension.
    One scan of the masks, ONE device-to-host read (the two counts), one copy kernel per tensor into freshly allocated outputs.
    With plan = relayout_plan(keep, append, n, device) the scan and the read are the plan's and the masks are taken from it."""
    tensors = list(tensors)
    if not tensors:
        raise RuntimeError("relayout needs at least one tensor")
    n = int(tensors[0].shape[0]) if tensors[0].dim() else -1
    for j, t in enumerate(tensors):
        _check_input(t, f"tensors[{j}]")
        if t.dim() < 1 or t.shape[0] != n:
            raise RuntimeError(f"tensors[{j}] must have {n} rows (got shape {tuple(t.shape)})")
        if t.element_size() != 4 or t.dtype not in (torch.float32, torch.int32):
            raise RuntimeError(f"tensors[{j}] must be float32 or int32 (got {t.dtype})")
        if t.device != tensors[0].device:
            raise RuntimeError("all tensors must be on one device")
    copies = int(copies)
    if copies < 1:
        raise RuntimeError(f"copies must be >= 1 (got {copies})")
    dev = tensors[0].device
    if plan is None:
        plan = relayout_plan(keep, append, n, dev)
    elif keep is not None or append is not None:
        raise RuntimeError("pass the masks or a plan, not both")
    elif plan.n != n or (plan.offsets is not None and plan.offsets.device != dev):
        raise RuntimeError(f"the plan is for {plan.n} rows on {None if plan.offsets is None else plan.offsets.device}, the tensors have {n} on {dev}")
    zero_append = set(zero_append)
    lib = _abi.load_library()
    stream = _stream(tensors[0])
    n_out = plan.n_keep + copies * plan.n_append
    out = []
    for j, t in enumerate(tensors):
        new = torch.empty((n_out, *t.shape[1:]), dtype=t.dtype, device=dev)
        row_elems = t.numel() // n if n else 0
        if n_out and row_elems:
            _abi.check(lib.grut_relayout_rows(stream, n, row_elems, _ptr(t), _ptr(plan.keep), _ptr(plan.append), _ptr(plan.offsets[0]),
                                              _ptr(plan.offsets[1]), plan.n_keep, plan.n_append, copies,
                                              APPEND_ZERO if j in zero_append else APPEND_COPY, _ptr(new)), "grut_relayout_rows")
        out.append(new)
    return out, plan.n_keep, plan.n_append


def split_tail_(positions, scale, rotation, noise, n_keep: int, copies: int):
    """Finishes a split in place on the rows [n_keep:] of the NEW raw tensors (relayout's output with keep = ~mask, append = mask):
    positions += R(rotation / |rotation|) (noise * exp(scale)), then scale = log(exp(scale) / (0.8 copies)).  positions / scale [N,3],
    rotation [N,4], noise [N - n_keep, 3] standard normals; contiguous fp32 CUDA tensors.  exp scale activation only."""
    n = int(positions.shape[0])
    n_keep, copies = int(n_keep), int(copies)
    _check_rows(positions, "positions", n, 3)
    _check_rows(scale, "scale", n, 3)
    _check_rows(rotation, "rotation", n, 4)
    if not 0 <= n_keep <= n or copies < 1 or (n - n_keep) % copies:
        raise RuntimeError(f"the tail of {n - n_keep} rows (n_keep = {n_keep} of {n}) is not {copies} copies of a block")
    m = n - n_keep
    _check_rows(noise, "noise", m, 3)
    if m:
        _abi.check(_abi.load_library().grut_split_tail(_stream(positions), m, _ptr(positions[n_keep:]), _ptr(scale[n_keep:]),
                                                       _ptr(rotation[n_keep:]), _ptr(noise), copies), "grut_split_tail")
    return positions, scale


# ---- the strategy -------------------------------------------------------------------------------------------------------------------
def _device_tensor_ok(t, dtypes=(torch.float32,), contiguous=True) -> bool:
    """What the kernels read in place: a (contiguous) CUDA tensor of one of `dtypes`."""
    return isinstance(t, torch.Tensor) and t.is_cuda and (t.is_contiguous() or not contiguous) and t.dtype in dtypes


def _model_is_fusable(model) -> bool:
    """Every parameter of the optimizer is a contiguous fp32 CUDA tensor [N, ...] and every optimizer-state entry besides `step` is a
    contiguous fp32 / int32 CUDA tensor with N rows (torch.optim.Adam and SelectiveAdam: exp_avg, exp_avg_sq)."""
    n = None
    for group in model.optimizer.param_groups:
        if len(group["params"]) != 1 or "name" not in group:
            return False
        p = group["params"][0]
        if not _device_tensor_ok(p.data) or p.dim() < 1:
            return False
        n = p.shape[0] if n is None else n
        if p.shape[0] != n:
            return False
        for key, v in model.optimizer.state.get(p, {}).items():
            if key != "step" and not (_device_tensor_ok(v, (torch.float32, torch.int32)) and v.dim() >= 1 and v.shape[0] == n):
                return False
    return n is not None


@torch.no_grad()
def relayout_model(model, keep, append, copies: int, zero_state: bool):
    """What the reference's _update_param_with_optimizer (strategy/base.py:76-107) does for a clone, split or prune, with ONE
    relayout_plan() for the whole model and one relayout() per tensor, so that each old tensor is released before the next new one is
    allocated: new Parameters keep requires_grad, the optimizer state moves to the new parameter with `step` untouched and every other
    entry relaid out (zeros appended when zero_state), setattr on the model.  -> (n_keep, n_append)."""
    optimizer = model.optimizer
    first = optimizer.param_groups[0]["params"][0]
    plan = relayout_plan(keep, append, first.shape[0], first.device)
    for group in optimizer.param_groups:
        old = group["params"][0]
        state = optimizer.state.pop(old, {})
        for key in state:
            if key != "step":
                (state[key],), _, _ = relayout([state[key]], copies=copies, zero_append=(0,) if zero_state else (), plan=plan)
        (data,), n_keep, n_append = relayout([old.data], copies=copies, plan=plan)
        fresh = torch.nn.Parameter(data, requires_grad=old.requires_grad)
        group["params"] = [fresh]
        optimizer.state[fresh] = state
        setattr(model, group["name"], fresh)
        del old, data
    return n_keep, n_append


class FusedGSStrategyMixin:
    """The overrides of the fused strategy, to be placed in front of a class with the reference's GSStrategy interface (gs.py): the
    installer below combines it with the reference class itself.  Every mask has the VALUES of the reference's (same comparisons on the
    same fp32 quantities; tests/test_densify_cpu.py holds the outcome against the unmodified reference class); an override whose
    preconditions do not hold calls the next class's method."""
    _grut_fused_gs = True
    _grut_logger = logging.getLogger(__name__)

    def _fusable(self) -> bool:
        return self.model.optimizer is not None and _model_is_fusable(self.model)

    def _log(self, what: str, count: int, n_before: int) -> None:
        if self.conf.strategy.print_stats:
            self._grut_logger.info(f"{what} {count} / {n_before} ({count / max(n_before, 1) * 100:.2f}%) gaussians")

    def _largest_scale(self) -> torch.Tensor:
        """[N]: the largest activated scale; above relative_size_threshold * scene_extent a Gaussian is split, otherwise cloned."""
        return self.model.get_scale().amax(dim=1)

    @torch.no_grad()
    def update_gradient_buffer(self, sensor_position: torch.Tensor) -> None:
        positions = self.model.positions
        grad = positions.grad
        accum, denom = self.densify_grad_norm_accum, self.densify_grad_norm_denom
        if not (grad is not None and _device_tensor_ok(grad) and _device_tensor_ok(positions.data) and _device_tensor_ok(accum)
                and _device_tensor_ok(denom, (torch.int32,)) and _device_tensor_ok(sensor_position, contiguous=False)
                and sensor_position.dim() == 1 and sensor_position.shape[0] == 3
                and accum.shape[0] == positions.shape[0] == denom.shape[0]):
            return super().update_gradient_buffer(sensor_position)
        accumulate_grad_stats_(accum, denom, grad, positions.data, sensor_position)

    @torch.no_grad()
    def clone_gaussians(self, densify_grad_norm: torch.Tensor, scene_extent: float):
        if densify_grad_norm is None or not self._fusable():
            return super().clone_gaussians(densify_grad_norm, scene_extent)
        selected = (densify_grad_norm >= self.clone_grad_threshold) & (self._largest_scale() <= self.relative_size_threshold * scene_extent)
        _, n_cloned = relayout_model(self.model, None, selected.contiguous(), 1, zero_state=True)
        self._log("Cloned", n_cloned, selected.shape[0])
        self.reset_densification_buffers()

    @torch.no_grad()
    def split_gaussians(self, densify_grad_norm: torch.Tensor, scene_extent: float):
        if not self._fusable() or self.model.scale_activation is not torch.exp:
            return super().split_gaussians(densify_grad_norm, scene_extent)
        model, copies = self.model, self.split_n_gaussians
        device = model.positions.device
        # the rows the clone has just appended come after the gradient norms: they count as norm 0
        norms = densify_grad_norm.reshape(-1)
        over = torch.full((model.num_gaussians,), bool(0.0 >= self.split_grad_threshold), dtype=torch.bool, device=device)
        over[: norms.shape[0]] = norms >= self.split_grad_threshold
        selected = over & (self._largest_scale() > self.relative_size_threshold * scene_extent)
        n_keep, n_split = relayout_model(model, ~selected, selected, copies, zero_state=True)
        # the reference draws torch.normal(mean=zeros, std=stds) over [copies n_split, 3] (gs.py:169-170): the same standard normals,
        # scaled, and the same advance of the generator as this draw
        noise = torch.randn((copies * n_split, 3), device=device)
        split_tail_(model.positions.data, model.scale.data, model.rotation.data, noise, n_keep, copies)
        self._log("Splitted", n_split, selected.shape[0])
        self.reset_densification_buffers()

    def _prune(self, valid: torch.Tensor, what: str) -> None:
        valid = valid.reshape(-1).contiguous()
        n_keep, _ = relayout_model(self.model, valid, None, 1, zero_state=False)
        self._log(what, valid.shape[0] - n_keep, valid.shape[0])
        self.prune_densification_buffers(valid)

    @torch.no_grad()
    def prune_gaussians_weight(self):
        if not self._fusable():
            return super().prune_gaussians_weight()
        self._prune(self.model.rolling_weight_contrib[:, 0] >= self.conf.strategy.prune_weight.weight_threshold, "Weight-pruned")

    @torch.no_grad()
    def prune_gaussians_scale(self, dataset):
        if not self._fusable():
            return super().prune_gaussians_scale(dataset)
        model = self.model
        # projected size of the smallest axis at the nearest camera plane: min scale / min_k <p, z_k> (floored) * the larger focal length
        view_axes = torch.from_numpy(dataset.poses[:, :3, 2]).to(model.device)
        nearest = (model.positions @ view_axes.T).amin(dim=1).clamp(min=1e-8)
        projected = model.get_scale().amin(dim=1) / nearest * dataset.intrinsic[0].max()
        self._prune(projected >= self.conf.strategy.prune_scale.threshold, "Scale-pruned")

    @torch.no_grad()
    def prune_gaussians_opacity(self):
        if not self._fusable():
            return super().prune_gaussians_opacity()
        self._prune(self.model.get_density().reshape(-1) >= self.prune_density_threshold, "Density-pruned")

    def prune_densification_buffers(self, valid_mask: torch.Tensor) -> None:
        accum, denom = self.densify_grad_norm_accum, self.densify_grad_norm_denom
        if not (_device_tensor_ok(accum) and _device_tensor_ok(denom, (torch.int32,)) and _device_tensor_ok(valid_mask, (torch.bool,))
                and valid_mask.dim() == 1 and accum.shape[0] == denom.shape[0] == valid_mask.shape[0]):
            return super().prune_densification_buffers(valid_mask)
        (self.densify_grad_norm_accum, self.densify_grad_norm_denom), _, _ = relayout([accum, denom], keep=valid_mask)


def install_fused_gs_strategy():
    """Opt-in: replace threedgrut.strategy.gs.GSStrategy with a subclass whose gradient statistic, clone, split and prunes run on the
    HIP kernels.  The masks and thresholds stay the reference's; an override whose preconditions do not hold (parameters that are not
    contiguous fp32 CUDA tensors, a scale activation other than exp for the split) calls the reference method.  The trainer looks the
    class up when it builds its strategy (trainer.py:254-257), so call this before constructing the trainer.  Returns the subclass;
    calling it again returns the same class."""
    mod = __import__("threedgrut.strategy.gs", fromlist=["GSStrategy"])
    base = mod.GSStrategy
    if getattr(base, "_grut_fused_gs", False):
        return base

    class GSStrategy(FusedGSStrategyMixin, base):
        _grut_logger = mod.logger

    GSStrategy.__qualname__ = GSStrategy.__name__ = "GSStrategy"
    GSStrategy.__module__ = __name__
    mod.GSStrategy = GSStrategy
    return GSStrategy
