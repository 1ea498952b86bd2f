"""The opacity and scale regularisers of the MCMC configurations on the MI355X, backed by csrc/regularizers.hip.

Every configuration that inherits configs/base_mcmc.yaml trains with loss.use_opacity and loss.use_scale, and on every step
Trainer3DGRUT.get_losses (threedgrut/trainer.py:722-736) evaluates

    torch.abs(model.get_density()).mean()     # sigmoid(density)  [N, 1]
    torch.abs(model.get_scale()).mean()       # exp(scale)        [N, 3]

and autograd differentiates both back to the raw parameters: about seven small launches forward and ten backward.

    opacity_scale_means(density, scale)   both means from the RAW parameters: two launches forward, one backward
    means_torch(density, scale)           the same model in torch (any device and dtype): the tests' reference and the fallback
    install_fused_regularizers()          opt-in: the get_losses that losses.install_fused_losses() installs makes that one call

The activations are non-negative, so the reference's abs is the identity; where one underflows to exactly 0, torch's sign(0) = 0 and the
kernel's derivative, 0, agree.  The kernels evaluate every exponential in double and round once (the device's expf is up to 11 ulp off,
more than the gradient's tolerance): the means are those of the exactly activated parameters, within that distance of the values rendered.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _abi

THREADS, MAX_BLOCKS = 256, 1024   # kRegThreads, kRegMaxBlocks of csrc/regularizers.hip: the forward grid is min(ceil(ceil(3N / 4) / 256), 1024)
MAX_PARTICLES = 0x55555555        # 3 N < 2^32
# plain counters, not synchronised across threads: fused forward calls, evaluations in torch because a precondition failed, fused backward calls
stats = {"hip_calls": 0, "torch_calls": 0, "hip_backward_calls": 0}
_enabled = False


def install_fused_regularizers(enable: bool = True) -> bool:
    """Switch the opacity and scale terms of the fused `get_losses` (the method losses.install_fused_losses() puts on Trainer3DGRUT) to
    one opacity_scale_means call on model.density / model.scale.  Off by default; returns the previous state.  With the reference's own
    get_losses bound (fused losses not installed) the switch has no effect: nothing consults it.  A model or parameters the kernels do
    not take (see trainer_means) keep running the two torch lines."""
    global _enabled
    previous, _enabled = _enabled, bool(enable)
    return previous


def enabled() -> bool:
    return _enabled


def means_torch(density, scale):
    """(mean |sigmoid(density)|, mean |exp(scale)|) of the raw parameters as the reference evaluates them (trainer.py:726, 734 on model.py's
    get_density / get_scale with the standard activations), in the tensors' own device and dtype; None for an argument that is None."""
    return (None if density is None else torch.abs(torch.sigmoid(density)).mean(),
            None if scale is None else torch.abs(torch.exp(scale)).mean())


def _ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def _rows(t, width):
    """-> N if t is a parameter the kernels read in place ([N, width], fp32, CUDA, contiguous, 16-byte aligned, 1 <= N, 3 N < 2^32), else None."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == width
            and 1 <= t.shape[0] <= MAX_PARTICLES and t.is_contiguous() and t.data_ptr() % 16 == 0):
        return None
    return int(t.shape[0])


def _fusable(density, scale) -> bool:
    """The preconditions of the fused call on whichever of the two tensors is given."""
    nd = None if density is None else _rows(density, 1)
    ns = None if scale is None else _rows(scale, 3)
    if (density is not None and nd is None) or (scale is not None and ns is None):
        return False
    return density is None or scale is None or (nd == ns and density.device == scale.device)


class _Means(torch.autograd.Function):
    """density [N, 1] or None, scale [N, 3] or None -> two 0-dim outputs (the one of a None input is +0 and not differentiable)."""

    @staticmethod
    def forward(ctx, density, scale):
        lib = _abi.load_library()
        given = density if density is not None else scale
        n = int(given.shape[0])
        out = torch.empty(2, dtype=torch.float32, device=given.device)
        partials = torch.empty(int(lib.grut_reg_partials(n)), dtype=torch.float32, device=given.device)
        stats["hip_calls"] += 1
        with torch.cuda.device(given.device):   # the launch goes to the parameters' device, whichever is current
            _abi.check(lib.grut_reg_forward(C.c_void_p(torch.cuda.current_stream().cuda_stream), n, _ptr(density), _ptr(scale), _ptr(partials),
                                            _ptr(out)), "grut_reg_forward")
        ctx.save_for_backward(*(t for t in (density, scale) if t is not None))
        ctx.has = (density is not None, scale is not None)
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_opacity, g_scale):
        saved = list(ctx.saved_tensors)
        density = saved.pop(0) if ctx.has[0] else None
        scale = saved.pop(0) if ctx.has[1] else None
        want_d = density is not None and ctx.needs_input_grad[0] and g_opacity is not None
        want_s = scale is not None and ctx.needs_input_grad[1] and g_scale is not None
        if not (want_d or want_s):
            return None, None
        given = density if density is not None else scale
        filler = g_opacity if want_d else g_scale   # the slot of a term that is not wanted is never read
        grad_out = torch.stack([(g if want else filler).reshape(()).to(torch.float32)
                                for g, want in ((g_opacity, want_d), (g_scale, want_s))])
        g_density = torch.empty_like(density) if want_d else None
        g_raw_scale = torch.empty_like(scale) if want_s else None
        stats["hip_backward_calls"] += 1
        with torch.cuda.device(given.device):
            _abi.check(_abi.load_library().grut_reg_backward(
                C.c_void_p(torch.cuda.current_stream().cuda_stream), int(given.shape[0]), _ptr(density), _ptr(scale), _ptr(grad_out),
                _ptr(g_density), _ptr(g_raw_scale)), "grut_reg_backward")
        return g_density, g_raw_scale


def opacity_scale_means(density, scale):
    """(mean sigmoid(density), mean exp(scale)) of the RAW parameters density [N, 1] and scale [N, 3] as 0-dim tensors on the current
    stream; either argument may be None and its result is then None.  Differentiable in both.  fp32 contiguous CUDA tensors (one device,
    one N, 1 <= N, 3 N < 2^32, 16-byte aligned) take csrc/regularizers.hip: one forward pair of launches and one backward launch for both
    terms, sums in a fixed order (two calls are bitwise equal).  Anything else is evaluated by means_torch."""
    if density is None and scale is None:
        raise ValueError("at least one of density, scale must be given")
    if not _fusable(density, scale):
        stats["torch_calls"] += 1
        return means_torch(density, scale)
    opacity, mean_scale = _Means.apply(density, scale)
    return (None if density is None else opacity), (None if scale is None else mean_scale)


def trainer_means(model, want_opacity: bool, want_scale: bool):
    """What the fused get_losses asks when the switch is on: (mean opacity, mean scale) with None for a term that is not wanted, or None
    when the two torch lines have to run: the model does not activate with sigmoid / exp (gut_tracer.has_standard_activations), or
    model.density [N, 1] and model.scale [N, 3] are not both parameters the kernels read in place."""
    from .gut_tracer import has_standard_activations
    if not (has_standard_activations(model) and _fusable(model.density, model.scale)):
        stats["torch_calls"] += 1
        return None
    return opacity_scale_means(model.density if want_opacity else None, model.scale if want_scale else None)
