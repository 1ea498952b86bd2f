"""The NHT decode stage on the MI355X: what the reference does around the decoder's network for `model.feature_type: nht` -
apply_feature_decoder (threedgrut/utils/render.py:54-92) and FeatureDecoder._process (threedgrut/model/feature_decoder.py:188-206) - as ONE
fused HIP pass each way: the kernels of 3dgrut_amd.tcnn (csrc/mlp.hip, csrc/mlp_backward.hip) reading the feature map, the camera rays, the
poses and alpha where they lie.  No [P, F + 3] rows are assembled, saved or read back.

    DecodeConfig(mlp, sh_scale, unpremultiply_alpha, center_ray)      GrutDecodeConfig of include/grut_amd.h
    decode_torch(params, features, alpha, rays_dir, rot, pixels_per_view, cfg)
                the contract of grut_decode_forward in plain torch, on any device; differentiable in features, alpha and params: the
                reference's op sequence around tcnn.mlp_torch
    decode_backward_torch(params, features, alpha, rays_dir, rot, pixels_per_view, grad_out, cfg)
                the contract of grut_decode_backward stated by hand -> (grad_features, grad_alpha or None, grad_params)
    decode(params, features, alpha, rays_dir, rot, pixels_per_view, cfg)      the dispatcher
    install_fused_decoder()     opt-in: rebinds threedgrut.utils.render.apply_feature_decoder (and the copies of the name that already
                imported modules hold) to a function that calls decode(); returns the originals

Tensors.  P = B * pixels_per_view pixels, view b owning pixels b * pixels_per_view ..: features [P, F], alpha [P] or None (needed with
unpremultiply_alpha, otherwise never read), rays_dir [P, 3] in camera space or None (only with center_ray), rot [B, 3, 3] =
T_to_world[:, :3, :3].  The model is stated at grut_decode_forward in include/grut_amd.h.

Dispatch.  decode() runs the kernel for tensors and configurations that tcnn.takes_hip takes (features as the rows), with fp32 contiguous
alpha, rays and poses on the same device that do not require grad; everything else runs decode_torch.  With grad enabled, one
autograd.Function saves features, alpha, rays, poses and params - no assembled rows.  Its backward calls grut_decode_backward exactly when
tcnn.install_fused_backward() is on and the configuration is taken by it (tcnn.backward_lds_bytes != 0); otherwise it re-runs decode_torch
under autograd, like the network's own training Function.  Rays and poses get no gradient.
"""
from __future__ import annotations

import ctypes as C
import sys
from typing import NamedTuple

import torch
from torch.autograd.function import once_differentiable

from . import _abi, tcnn

ALPHA_MIN = 9.99999993922529e-09   # 1e-8f, the fp32 value that alpha.clamp(min=1e-8) of FeatureDecoder._process clamps an fp32 alpha to
HOOK_MODULES = ("threedgrut.trainer", "threedgrut.render", "threedgrut.utils.gui", "threedgrut.utils.viser_gui_util")
stats = {"hip_calls": 0, "torch_calls": 0, "backward_calls": 0, "hip_backward_calls": 0}   # which path ran (tests); plain counters


class DecodeConfig(NamedTuple):
    """GrutDecodeConfig of include/grut_amd.h"""
    mlp: tcnn.MlpConfig
    sh_scale: float
    unpremultiply_alpha: bool
    center_ray: bool

    def as_struct(self):
        return _abi.GrutDecodeConfig(self.mlp.as_struct(), float(self.sh_scale), int(bool(self.unpremultiply_alpha)), int(bool(self.center_ray)))


# ---- the model in torch -------------------------------------------------------------------------------------------------------------------------
def _check(params, features, alpha, rays_dir, rot, pixels_per_view, cfg: DecodeConfig):
    p, b = features.shape[0], rot.shape[0]
    if features.dim() != 2 or features.shape[1] != cfg.mlp.n_features or params.dim() != 1 or params.numel() != cfg.mlp.n_params:
        raise ValueError(f"decode: features must be [P, {cfg.mlp.n_features}] and params [{cfg.mlp.n_params}] "
                         f"(got {list(features.shape)} and {list(params.shape)})")
    if rot.shape[1:] != (3, 3) or pixels_per_view < 1 or b * pixels_per_view != p:
        raise ValueError(f"decode: rot must be [B, 3, 3] with B * pixels_per_view = P (got {list(rot.shape)}, {pixels_per_view}, P = {p})")
    if cfg.unpremultiply_alpha and (alpha is None or alpha.numel() != p):
        raise ValueError("decode: unpremultiply_alpha needs alpha [P]")
    if not cfg.center_ray and (rays_dir is None or tuple(rays_dir.shape) != (p, 3)):
        raise ValueError("decode: rays_dir [P, 3] is needed unless center_ray")


def world_directions(rays_dir, rot, pixels_per_view: int, center_ray: bool):
    """the unit world direction of every pixel [P, 3], by the reference's operations (render.py:72-84)"""
    b = rot.shape[0]
    if center_ray:
        w = torch.nn.functional.normalize(rot[:, :, 2], dim=-1)
        return w.view(b, 1, 1, 3).expand(b, 1, pixels_per_view, 3).contiguous().view(-1, 3)
    w = torch.einsum("bij,bhwj->bhwi", rot, rays_dir.reshape(b, 1, pixels_per_view, 3))
    return torch.nn.functional.normalize(w, dim=-1).contiguous().view(-1, 3)


def assemble_rows(features, alpha, rays_dir, rot, pixels_per_view: int, cfg: DecodeConfig):
    """-> (the network's rows [P, F + 3], a_s [P, 1] or None), by the reference's operations (feature_decoder.py:194-200)"""
    dirs = world_directions(rays_dir, rot.to(features.dtype), pixels_per_view, cfg.center_ray)
    a_s = None
    if cfg.unpremultiply_alpha:
        a_s = alpha.reshape(-1, 1).clamp(min=ALPHA_MIN)
        features = features / a_s
    unit_cube = (dirs * cfg.sh_scale + 1.0) * 0.5
    return torch.cat([features, unit_cube], dim=-1), a_s


def decode_torch(params, features, alpha, rays_dir, rot, pixels_per_view: int, cfg: DecodeConfig):
    """The decode stage in plain torch: the reference's op sequence around tcnn.mlp_torch -> [P, n_output_dims] fp32."""
    _check(params, features, alpha, rays_dir, rot, pixels_per_view, cfg)
    rows, a_s = assemble_rows(features, alpha, rays_dir, rot, pixels_per_view, cfg)
    rgb = tcnn.mlp_torch(params, rows, cfg.mlp)
    if a_s is not None:
        rgb = rgb * a_s
    return rgb.float()


@torch.no_grad()
def decode_backward_torch(params, features, alpha, rays_dir, rot, pixels_per_view: int, grad_out, cfg: DecodeConfig):
    """The contract of grut_decode_backward (include/grut_amd.h) in plain torch, on any device: fp64 arithmetic for fp64 features, fp32
    otherwise.  The rules of tcnn.mlp_backward_torch on the assembled rows, with the upstream gradient grad_out * a_s formed first,
    grad_features = gx / a_s and grad_alpha = [alpha >= 1e-8f] (sum_c grad_out_c y_c - (sum_j gx_j x_j) / a_s); the SH Jacobian's columns
    are dropped.  -> (grad_features [P, F], grad_alpha [P] or None without unpremultiply_alpha, grad_params)."""
    _check(params, features, alpha, rays_dir, rot, pixels_per_view, cfg)
    dt = torch.float64 if features.dtype == torch.float64 else torch.float32
    f = cfg.mlp.n_features
    alpha_dt = None if alpha is None else alpha.to(dt)
    rays_dt = None if rays_dir is None else rays_dir.to(dt)
    rows, a_s = assemble_rows(features.to(dt), alpha_dt, rays_dt, rot.to(dt), pixels_per_view, cfg)
    go = grad_out.to(dt)
    upstream = go if a_s is None else go * a_s
    grad_rows, grad_params = tcnn.mlp_backward_torch(params, rows, upstream, cfg.mlp)
    gx = grad_rows[:, :f]
    if a_s is None:
        return gx, None, grad_params
    y = tcnn.mlp_torch(params, rows, cfg.mlp)
    inner = (go * y).sum(dim=1) - (gx * rows[:, :f]).sum(dim=1) / a_s[:, 0]
    gate = alpha_dt.reshape(-1) >= ALPHA_MIN
    return gx / a_s, torch.where(gate, inner, torch.zeros_like(inner)), grad_params


# ---- the HIP path -------------------------------------------------------------------------------------------------------------------------------
def _plain(t, device, shape) -> bool:
    return (t.is_cuda and t.device == device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)
            and not t.requires_grad)


def takes_hip(params, features, alpha, rays_dir, rot, pixels_per_view: int, cfg: DecodeConfig) -> bool:
    """the dispatch rule of the module's docstring"""
    if features.dim() != 2 or not tcnn.takes_hip(params, features, cfg.mlp):
        return False
    p, dev = features.shape[0], features.device
    if cfg.unpremultiply_alpha and not (alpha.is_cuda and alpha.device == dev and alpha.dtype == torch.float32 and alpha.is_contiguous()):
        return False
    if not cfg.center_ray and not _plain(rays_dir, dev, (p, 3)):
        return False
    return _plain(rot, dev, (p // pixels_per_view, 3, 3))


def _ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def decode_forward_hip(params, features, alpha, rays_dir, rot, pixels_per_view: int, cfg: DecodeConfig):
    """One launch of csrc/mlp.hip's decode instantiation on tensors that takes_hip() accepts -> [P, n_output_dims] fp32.  Not differentiable."""
    lib = _abi.load_library()
    out = torch.empty((features.shape[0], cfg.mlp.n_output_dims), dtype=torch.float32, device=features.device)
    stats["hip_calls"] += 1
    with torch.cuda.device(features.device):   # the launch goes to the input's device, whichever is current
        _abi.check(lib.grut_decode_forward(C.c_void_p(torch.cuda.current_stream(features.device).cuda_stream), C.byref(cfg.as_struct()),
                                           _ptr(params), _ptr(features), _ptr(alpha if cfg.unpremultiply_alpha else None),
                                           _ptr(None if cfg.center_ray else rays_dir), _ptr(rot), rot.shape[0], pixels_per_view, _ptr(out)),
                   "grut_decode_forward")
    return out


def decode_backward_hip(params, features, alpha, rays_dir, rot, pixels_per_view: int, grad_out, cfg: DecodeConfig, need_features: bool = True,
                        need_alpha: bool = True, need_params: bool = True):
    """csrc/mlp_backward.hip's decode instantiation on tensors that takes_hip() accepts, for a configuration with
    tcnn.backward_lds_bytes != 0 and a contiguous fp32 grad_out [P, n_output_dims] -> (grad_features, grad_alpha, grad_params), None for
    what was not asked for.  The scratch comes from torch's allocator, per call."""
    lib = _abi.load_library()
    struct, p = cfg.as_struct(), features.shape[0]
    need_alpha = need_alpha and cfg.unpremultiply_alpha
    grad_features = torch.empty_like(features) if need_features else None
    grad_alpha = torch.empty(p, dtype=torch.float32, device=features.device) if need_alpha else None
    grad_params = torch.empty_like(params) if need_params else None
    scratch = None
    if need_params:
        scratch = torch.empty(int(lib.grut_mlp_backward_scratch_bytes(C.byref(struct.mlp), p)), dtype=torch.uint8, device=features.device)
    stats["hip_backward_calls"] += 1
    with torch.cuda.device(features.device):
        _abi.check(lib.grut_decode_backward(C.c_void_p(torch.cuda.current_stream(features.device).cuda_stream), C.byref(struct), _ptr(params),
                                            _ptr(features), _ptr(alpha if cfg.unpremultiply_alpha else None),
                                            _ptr(None if cfg.center_ray else rays_dir), _ptr(rot), rot.shape[0], pixels_per_view, _ptr(grad_out),
                                            _ptr(scratch), _ptr(grad_features), _ptr(grad_alpha), _ptr(grad_params)),
                   "grut_decode_backward")
    return grad_features, grad_alpha, grad_params


class _DecodeFunction(torch.autograd.Function):
    """The training step: the forward is the kernel and keeps only features, alpha, rays, poses and params; the backward recomputes the
    forward from them, in decode_torch under autograd or, after tcnn.install_fused_backward(), in the fused kernel."""

    @staticmethod
    def forward(ctx, features, alpha, params, rays_dir, rot, pixels_per_view, cfg):
        ctx.save_for_backward(features, alpha, params, rays_dir, rot)
        ctx.pixels_per_view, ctx.cfg = pixels_per_view, cfg
        return decode_forward_hip(params.detach(), features.detach(), None if alpha is None else alpha.detach(), rays_dir, rot, pixels_per_view,
                                  cfg)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        features, alpha, params, rays_dir, rot = ctx.saved_tensors
        cfg, ppv = ctx.cfg, ctx.pixels_per_view
        need_f, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        need_a = ctx.needs_input_grad[1] and cfg.unpremultiply_alpha            # without the flag alpha does not enter the result
        stats["backward_calls"] += 1
        if not (need_f or need_a or need_p):
            return (None,) * 7
        if tcnn._fused_backward and takes_hip(params, features, alpha, rays_dir, rot, ppv, cfg) and tcnn.backward_lds_bytes(cfg.mlp) != 0 \
                and grad_out.device == features.device:
            gf, ga, gp = decode_backward_hip(params.detach(), features.detach(), None if alpha is None else alpha.detach(), rays_dir, rot, ppv,
                                             grad_out.detach().to(torch.float32).contiguous(), cfg, need_f, need_a, need_p)
            return gf, None if ga is None else ga.view(alpha.shape), gp, None, None, None, None
        with torch.enable_grad():
            fg, pg = features.detach().requires_grad_(need_f), params.detach().requires_grad_(need_p)
            ag = None if alpha is None else alpha.detach().requires_grad_(need_a)
            y = decode_torch(pg, fg, ag, rays_dir, rot, ppv, cfg)
            grads = list(torch.autograd.grad(y, [t for t, need in ((fg, need_f), (ag, need_a), (pg, need_p)) if need], grad_out.to(y.dtype)))
        return (grads.pop(0) if need_f else None, grads.pop(0) if need_a else None, grads.pop(0) if need_p else None, None, None, None, None)


def decode(params, features, alpha, rays_dir, rot, pixels_per_view: int, cfg: DecodeConfig):
    """The decode stage with the dispatch of the module's docstring; differentiable in features, alpha and params."""
    _check(params, features, alpha, rays_dir, rot, pixels_per_view, cfg)
    if not takes_hip(params, features, alpha, rays_dir, rot, pixels_per_view, cfg):
        stats["torch_calls"] += 1
        return decode_torch(params, features, alpha, rays_dir, rot, pixels_per_view, cfg)
    if cfg.unpremultiply_alpha:
        alpha = alpha.view(-1)
    if torch.is_grad_enabled() and (features.requires_grad or params.requires_grad or (cfg.unpremultiply_alpha and alpha.requires_grad)):
        return _DecodeFunction.apply(features, alpha if cfg.unpremultiply_alpha else None, params, rays_dir, rot, pixels_per_view, cfg)
    return decode_forward_hip(params.detach(), features.detach(), alpha.detach() if cfg.unpremultiply_alpha else None, rays_dir, rot,
                              pixels_per_view, cfg)


# ---- the hook -----------------------------------------------------------------------------------------------------------------------------------
def _hook_inputs(feature_decoder, outputs, gpu_batch, center_ray: bool):
    """The arguments of decode() for one call of apply_feature_decoder, or None when a precondition does not hold."""
    network = getattr(feature_decoder, "network", None)
    if not isinstance(network, tcnn.NetworkWithInputEncoding):
        return None
    features, alpha = outputs.get("pred_features"), outputs.get("pred_opacity")
    rays, pose = getattr(gpu_batch, "rays_dir", None), getattr(gpu_batch, "T_to_world", None)
    if not all(isinstance(t, torch.Tensor) for t in (features, alpha, rays, pose)):
        return None
    if not (features.dim() == 4 and features.is_cuda and features.dtype == torch.float32
            and features.shape[-1] == feature_decoder.ray_feature_dim == network.cfg.n_features and network.cfg.n_output_dims == 3):
        return None
    b, h, w, n = features.shape
    if not (rays.dtype == torch.float32 and rays.device == features.device and tuple(rays.shape) == (b, h, w, 3)):
        return None
    if rays.requires_grad or pose.requires_grad or b * h * w >= 2 ** 32 or b * h * w == 0 or pose.dim() != 3 or pose.shape[0] != b:
        return None
    unpremultiply = bool(feature_decoder.unpremultiply_alpha)
    if alpha.numel() != b * h * w or (unpremultiply and not (alpha.dtype == torch.float32 and alpha.device == features.device)):
        return None
    rot = pose[:, :3, :3].to(device=rays.device, dtype=rays.dtype).contiguous()   # a GUI batch keeps its pose on the CPU
    cfg = DecodeConfig(network.cfg, float(feature_decoder.sh_scale), unpremultiply, bool(center_ray))
    return (network.params, features.contiguous().view(-1, n), alpha.contiguous().view(-1) if unpremultiply else None,
            None if center_ray else rays.contiguous().view(-1, 3), rot, h * w, cfg)


def install_fused_decoder():
    """Opt-in: rebind apply_feature_decoder on threedgrut.utils.render, and on each of threedgrut.trainer, threedgrut.render,
    threedgrut.utils.gui and threedgrut.utils.viser_gui_util that is ALREADY imported and still holds the original (none of them is
    imported here), to a function of the same signature and returned dict that runs the decode stage through decode().  It calls the
    function it replaced whenever a precondition does not hold: decoder.network is not this project's NetworkWithInputEncoding, the
    features are not fp32 CUDA [B, H, W, ray_feature_dim], the rays are not fp32 on the same device, rays or pose require grad, or
    P >= 2^32.  Returns the dict of the replaced (original) functions by name; calling it again changes nothing and returns the same dict."""
    render = __import__("threedgrut.utils.render", fromlist=["apply_feature_decoder"])
    if getattr(render.apply_feature_decoder, "_grut_fused_decoder", False):
        return render.apply_feature_decoder._grut_originals
    original = render.apply_feature_decoder
    originals = {"apply_feature_decoder": original}

    def apply_feature_decoder(feature_decoder, outputs: dict, gpu_batch, training: bool = False, center_ray_encoding: bool = False) -> dict:
        args = None if feature_decoder is None else _hook_inputs(feature_decoder, outputs, gpu_batch, center_ray_encoding)
        if args is None:
            return original(feature_decoder, outputs, gpu_batch, training=training, center_ray_encoding=center_ray_encoding)
        b, h, w, _ = outputs["pred_features"].shape
        outputs["pred_features"] = decode(*args).view(b, h, w, 3)
        return outputs

    apply_feature_decoder.__doc__ = original.__doc__
    apply_feature_decoder._grut_fused_decoder = True
    apply_feature_decoder._grut_originals = originals
    render.apply_feature_decoder = apply_feature_decoder
    for name in HOOK_MODULES:
        module = sys.modules.get(name)
        if module is not None and getattr(module, "apply_feature_decoder", None) is original:
            module.apply_feature_decoder = apply_feature_decoder
    return originals
