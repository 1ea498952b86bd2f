"""The trainer's two optimizers on HIP (csrc/optim.hip).

FusedAdam — torch.optim.Adam(fused=True), what `optimizer.type: adam` builds (threedgrut/model/model.py:807-810), with all parameter
groups in one launch; same constructor, state and state_dict; `FusedAdam.adopt(optimizer)` / `install_fused_adam()` switch an existing
optimizer / the reference model's.  Calls the HIP pass does not cover run torch's own fused step on the same state.

SelectiveAdam — the visibility-masked Adam of the reference trainer (threedgrut/optimizers/__init__.py:38-124),
backed by one HIP launch for all parameter groups (csrc/optim.hip) instead of one CUDA launch per group.

Same surface: `SelectiveAdam(params, lr, betas, eps)`; `step(visibility)` where `visibility` is the tracers'
`mog_visibility` ([N,1] float tensor holding an int bit pattern, or a bool / int tensor); one tensor per param group;
no bias correction; rows that were not visible keep parameter and moments.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import functools
import weakref

import torch

from . import _abi


class SelectiveAdam(torch.optim.Adam):
    def __init__(self, params, lr=0.001, betas=(0.9, 0.999), eps=1e-08):
        super().__init__(params=params, lr=lr, eps=eps, betas=betas)
        self._lib = _abi.load_library()

    @torch.no_grad()
    def step(self, visibility):
        groups, keep = [], []
        n_rows, device = None, None
        for group in self.param_groups:
            assert len(group["params"]) == 1, "More than one tensor in group is not supported"
            param = group["params"][0]
            if param.grad is None:
                continue
            if not param.is_cuda:
                raise RuntimeError("3dgrut_amd.SelectiveAdam updates GPU tensors only (there is no CPU fallback)")
            if param.dtype != torch.float32 or not param.is_contiguous():
                raise RuntimeError("3dgrut_amd.SelectiveAdam needs contiguous float32 parameters")
            state = self.state[param]
            if len(state) == 0:  # lazy state initialisation, as optimizers/__init__.py:101-105
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["exp_avg"] = torch.zeros_like(param, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(param, memory_format=torch.preserve_format)
            if param.numel() == 0:
                continue
            rows = int(param.shape[0])
            if n_rows is None:
                n_rows, device = rows, param.device
            elif rows != n_rows:
                raise RuntimeError(f"SelectiveAdam: parameter groups disagree on the number of rows ({rows} vs {n_rows})")
            grad = param.grad.contiguous()
            beta1, beta2 = group["betas"]
            g = _abi.GrutAdamGroup()
            g.param, g.grad = param.data_ptr(), grad.data_ptr()
            g.exp_avg, g.exp_avg_sq = state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr()
            g.row_width = param.numel() // rows
            g.lr, g.beta1, g.beta2, g.eps = float(group["lr"]), float(beta1), float(beta2), float(group["eps"])
            groups.append(g)
            keep.append(grad)
        if not groups:
            return
        vis = visibility.reshape(-1)
        if vis.numel() != n_rows:
            raise RuntimeError(f"SelectiveAdam: visibility has {vis.numel()} entries for {n_rows} rows")
        if vis.device != device:
            vis = vis.to(device)
        if vis.dtype == torch.bool:
            kind = _abi.VIS_BOOL_U8
        elif vis.dtype == torch.float32:
            kind = _abi.VIS_FLOAT_BITS  # `.bool()` of the tracers' float tensor: any non-zero bit pattern (denormals included)
        elif vis.dtype == torch.int32:
            kind = _abi.VIS_INT32
        else:
            vis, kind = vis.bool(), _abi.VIS_BOOL_U8
        vis = vis.contiguous()
        arr = (_abi.GrutAdamGroup * len(groups))(*groups)
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _abi.check(self._lib.grut_selective_adam_update(stream, arr, len(groups), n_rows, C.c_void_p(vis.data_ptr()), kind),
                   "grut_selective_adam_update")


# ---- dense Adam: the optimizer of every shipped config (optimizer.type: adam, threedgrut/model/model.py:807-810) -----------------
stats = {"hip_steps": 0, "torch_steps": 0}   # which path a FusedAdam.step() took (tests); plain counters


def _device_tensor_ok(t) -> bool:
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and not t.is_sparse and t.is_contiguous()
            and t.data_ptr() % 16 == 0)


def _torch_adam_step(self, closure):
    """torch.optim.Adam.step without the hook runner torch wraps around a class's step once (ours has run the hooks already)."""
    fn = torch.optim.Adam.step
    if getattr(fn, "hooked", False):
        fn = fn.__wrapped__
    return fn(self, closure)


def _track_step_called(new, old):
    """The `step` an lr_scheduler puts on its optimizer's instance (torch/optim/lr_scheduler.py, patch_track_step_called), for an
    adopted optimizer: it sets `_opt_called`, which the scheduler reads to warn about a scheduler.step() ahead of optimizer.step(),
    on `new` and on `old` - the scheduler still holds `old` - and runs `new`'s own class step.  Weak references, as torch's."""
    new_ref, old_ref = weakref.ref(new), weakref.ref(old)

    @functools.wraps(type(new).step)
    def wrapper(*args, **kwargs):
        opt, prev = new_ref(), old_ref()
        opt._opt_called = True
        if prev is not None:
            prev._opt_called = True
        return type(opt).step(opt, *args, **kwargs)

    wrapper._wrapped_by_lr_sched = True
    return wrapper


class FusedAdam(torch.optim.Adam):
    """torch.optim.Adam(fused=True) with the step of ALL parameter groups in one HIP launch (grut_adam_update, csrc/optim.hip).

    Constructor, param_groups, state (`step` as a 0-dim fp32 tensor on the parameter's device, `exp_avg`, `exp_avg_sq`) and
    state_dict are torch's, so whatever edits the optimizer state of a torch.optim.Adam edits this one the same way.  step() runs
    torch's own fused path on the same state whenever the HIP pass does not cover the call: see `_plan`.

    A step on the HIP path is two launches per batch of 8 tensors (the per-tensor prologue and the update).  An EMPTY parameter that
    has a grad adds one torch launch of its own (`step += 1`, as torch counts it): the library skips tensors without elements."""

    def __init__(self, params, *args, **kwargs):
        kwargs["fused"] = True
        super().__init__(params, *args, **kwargs)

    @classmethod
    def adopt(cls, optimizer):
        """A FusedAdam over the SAME param_groups (the dict objects) and state as `optimizer`, a torch.optim.Adam of any flavour
        (single-tensor, foreach or fused).  A `step` kept on the host moves to its parameter's device as fp32, as torch's
        load_state_dict does for fused optimizers.  Use the returned object in place of `optimizer`.  An lr_scheduler already
        attached to `optimizer` keeps working: it writes the rates into the shared param_groups, which step() reads at every call."""
        if isinstance(optimizer, cls):
            return optimizer
        if type(optimizer) is not torch.optim.Adam:
            raise TypeError(f"FusedAdam.adopt takes a torch.optim.Adam, not {type(optimizer).__name__}")
        new = cls.__new__(cls)
        attrs = dict(optimizer.__dict__)
        # An lr_scheduler built on `optimizer` has put a `step` on the instance that runs the OLD object's step through a weakref:
        # it is not carried over (nor is any other instance-level `step`); the scheduler's bookkeeping is re-installed below.
        old_step = attrs.pop("step", None)
        new.__dict__.update(attrs)
        new._patch_step_function()
        if getattr(old_step, "_wrapped_by_lr_sched", False):
            new.step = _track_step_called(new, optimizer)
        supported = ("cuda", "cpu")
        fused_all = True
        for group in new.param_groups:
            if group["differentiable"] or not all(torch.is_floating_point(p) and p.device.type in supported for p in group["params"]):
                fused_all = False   # torch's fused path does not take these: the group keeps its flavour, step() takes torch's path
                continue
            group["fused"], group["foreach"] = True, None
            for p in group["params"]:
                state = new.state.get(p)
                if state and "step" in state:
                    step = state["step"]
                    state["step"] = (step.to(device=p.device, dtype=torch.float32) if torch.is_tensor(step)
                                     else torch.tensor(float(step), dtype=torch.float32, device=p.device))
        if fused_all:
            new.defaults = {**optimizer.defaults, "fused": True, "foreach": None}
            new._step_supports_amp_scaling = True
        return new

    def _plan(self):
        """[(group, param)] for every parameter with a grad when the HIP pass covers this call, else None: a GradScaler's
        grad_scale / found_inf, amsgrad, maximize, capturable, differentiable, decoupled weight decay, a tensor lr or betas, parameters
        on several devices, and any parameter, grad or state tensor that is not a contiguous fp32 CUDA tensor on a 16-byte aligned base
        (a strided grad is copied) go to torch."""
        if getattr(self, "grad_scale", None) is not None or getattr(self, "found_inf", None) is not None:
            return None
        work, device = [], None
        for group in self.param_groups:
            if (group["amsgrad"] or group["maximize"] or group["capturable"] or group["differentiable"] or not group["fused"]
                    or group.get("decoupled_weight_decay", False)):
                return None
            if any(torch.is_tensor(h) for h in (group["lr"], *group["betas"], group["eps"], group["weight_decay"])):
                return None
            for p in group["params"]:
                grad = p.grad
                if grad is None:
                    continue
                if not _device_tensor_ok(p) or grad.is_sparse or grad.dtype != torch.float32 or grad.device != p.device:
                    return None
                if device is None:
                    device = p.device
                elif p.device != device:
                    return None
                state = self.state.get(p)
                if state:
                    step = state["step"]
                    if not (_device_tensor_ok(state["exp_avg"]) and _device_tensor_ok(state["exp_avg_sq"]) and torch.is_tensor(step)
                            and step.dtype == torch.float32 and step.numel() == 1
                            and step.device == state["exp_avg"].device == state["exp_avg_sq"].device == device):
                        return None
                work.append((group, p))
        return work

    def step(self, closure=None):
        work = None if closure is not None else self._plan()   # (torch runs a closure with grad enabled: its path)
        if work is None:
            stats["torch_steps"] += 1
            return _torch_adam_step(self, closure)
        self._cuda_graph_capture_health_check()
        stats["hip_steps"] += 1
        if not work:
            return None
        with torch.no_grad():
            entries, keep = [], []
            for group, p in work:
                state = self.state[p]
                if len(state) == 0:   # lazy state initialisation, as torch.optim.Adam._init_group with fused=True
                    state["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if p.numel() == 0:
                    state["step"] += 1   # torch counts the step of an empty tensor too; the library skips it
                    continue
                grad = p.grad.contiguous()
                if grad.data_ptr() % 16:
                    grad = grad.clone()
                keep.append(grad)   # alive until the launch is issued
                entries.append((group, p, grad, state))
            if not entries:
                return None
            device = entries[0][1].device
            arr = (_abi.GrutDenseAdamGroup * len(entries))()
            for g, (group, p, grad, state) in zip(arr, entries):
                g.param, g.grad = p.data_ptr(), grad.data_ptr()
                g.exp_avg, g.exp_avg_sq, g.step = state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(), state["step"].data_ptr()
                g.numel = p.numel()
                g.lr, g.eps, g.weight_decay = float(group["lr"]), float(group["eps"]), float(group["weight_decay"])
                g.beta1, g.beta2 = float(group["betas"][0]), float(group["betas"][1])
            scratch = self.__dict__.get("_grut_scratch")
            if scratch is None or scratch.device != device or scratch.shape[0] < len(entries):
                scratch = self._grut_scratch = torch.empty((len(entries), 2), dtype=torch.float32, device=device)
            lib = _abi.load_library()
            with torch.cuda.device(device):
                stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
                _abi.check(lib.grut_adam_update(stream, arr, len(entries), C.c_void_p(scratch.data_ptr())), "grut_adam_update")
        return None


def install_fused_adam():
    """Opt-in: wrap threedgrut.model.model.MixtureOfGaussians.setup_optimizer so that, after the reference's method has run
    (model.py:782-826: the groups and their names, positions' rate times scene_extent, the schedulers, an optional load_state_dict),
    an optimizer whose type is exactly torch.optim.Adam is adopted as a FusedAdam.  SelectiveAdam configs are left alone.  Returns the
    method it replaced; calling it again changes nothing and returns the same method."""
    cls = __import__("threedgrut.model.model", fromlist=["MixtureOfGaussians"]).MixtureOfGaussians
    replaced = cls.setup_optimizer
    if getattr(replaced, "_grut_replaced", None) is not None:
        return replaced._grut_replaced

    @functools.wraps(replaced)
    def setup_optimizer(self, *args, **kwargs):
        out = replaced(self, *args, **kwargs)
        if type(self.optimizer) is torch.optim.Adam:
            self.optimizer = FusedAdam.adopt(self.optimizer)
        return out

    setup_optimizer._grut_replaced = replaced
    cls.setup_optimizer = setup_optimizer
    return replaced
