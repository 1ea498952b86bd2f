"""MCMC densification strategy on the MI355X: drop-in for the reference's `threedgrut.strategy.lib_mcmc_cc` extension and an opt-in
fused `perturb_gaussians` (threedgrut/strategy/mcmc.py), both backed by csrc/mcmc.hip.  There is no CPU fallback.

    compute_relocation_tensor(opacities, scales, ratios, binoms, n_max)   the surface of lib_mcmc_cc (bindings.cpp:39-55)
    perturb_positions_(positions, rotation, scale, density, noise, noise_lr, lr, activated=False)
    perturb_gaussians(model, noise_lr)                                     MCMCStrategy.perturb_gaussians (mcmc.py:167-187)
    install()                 registers this module as threedgrut.strategy.lib_mcmc_cc (called by the shims: the nvcc JIT is never reached)
    install_fused_perturb()   rebinds threedgrut.strategy.mcmc.MCMCStrategy to a subclass whose perturb_gaussians is the fused pass
"""
from __future__ import annotations

import ctypes as C
import sys

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
