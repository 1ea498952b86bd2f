"""PPISP post-processing on the MI355X: drop-in for the third-party CUDA package `ppisp` that the reference's trainer imports for
`post_processing.method: ppisp` (threedgrut/trainer.py:470), backed by csrc/ppisp.hip.

    ppisp_apply(exposure_params=, vignetting_params=, color_params=, crf_params=, rgb_in=, pixel_coords=, resolution_w=, resolution_h=,
                camera_idx=, frame_idx=)       the learned camera model on [..., 3] colours: one HIP pass forward, one backward
    PPISPConfig, PPISP(num_cameras, num_frames, config)   the module the trainer builds (trainer.py:496-512), its optimizers, schedulers,
                regulariser and per-camera controllers
    export_ppisp_report(module, frames_per_camera, output_dir, camera_names=None)   one JSON file per camera (trainer.py:1000-1005)
    install()   registers modules named `ppisp` and `ppisp.report` (unless they are already in sys.modules); called by the tracer shims

The model (exposure, vignetting, colour homography, response curve), its NULL rules and its gradient conventions at the kinks are stated
at grut_ppisp_forward in include/grut_amd.h.  fp32 CUDA tensors go through the HIP kernels; anything else (CPU tensors, other dtypes)
goes through `ppisp_torch`, the same model restated in torch with the same conventions, which is also the benchmark's baseline
(scripts/bench_ppisp.py).  What the reference checkout does not pin - the regulariser, the learning rates and schedules, how the
module learns that its controller is active, the gradient conventions - is this project's choice.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import math
import os
import sys
import types

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _abi

SHIM_MODULE = "ppisp"
CRF_IDENTITY = (math.log(math.expm1(0.7)), math.log(math.expm1(0.7)), math.log(math.expm1(0.9)), 0.0)   # toe = shoulder = gamma = 1, centre = 1/2
_LATENT_MAPS = (((0.0480542, -0.0043631), (-0.0043631, 0.0481283)),     # blue
                ((0.0580570, -0.0179872), (-0.0179872, 0.0431061)),     # red
                ((0.0433336, -0.0180537), (-0.0180537, 0.0580500)),     # green
                ((0.0128369, -0.0034654), (-0.0034654, 0.0128158)))     # neutral
stats = {"forward_calls": 0, "backward_calls": 0, "torch_calls": 0,   # which path ran (tests); plain counters
         "controller_hip_calls": 0, "controller_torch_calls": 0, "controller_hip_backward_calls": 0}


# ---- the model in torch: the path of everything that is not an fp32 CUDA tensor, and the benchmark's baseline ------------------------------
def _homography(color):
    dt, dev = color.dtype, color.device
    o = torch.einsum("kij,kj->ki", torch.tensor(_LATENT_MAPS, dtype=dt, device=dev), color.reshape(4, 2))
    one, zero = torch.ones((), dtype=dt, device=dev), torch.zeros((), dtype=dt, device=dev)
    t = torch.stack([torch.stack([o[0, 0], o[0, 1], one]), torch.stack([1 + o[1, 0], o[1, 1], one]),
                     torch.stack([o[2, 0], 1 + o[2, 1], one])], dim=1)                       # columns: blue, red, green targets
    n = torch.stack([1.0 / 3.0 + o[3, 0], 1.0 / 3.0 + o[3, 1], one])
    k = torch.stack([torch.stack([zero, -n[2], n[1]]), torch.stack([n[2], zero, -n[0]]), torch.stack([-n[1], n[0], zero])])
    a = k @ t
    l01, l02, l12 = torch.linalg.cross(a[0], a[1]), torch.linalg.cross(a[0], a[2]), torch.linalg.cross(a[1], a[2])
    small = lambda v: (v.detach() ** 2).sum() < 1e-20                                          # noqa: E731  (the branch is a constant)
    lam = torch.where(small(l01), torch.where(small(l02), l12, l02), l01)
    s = torch.tensor([[-1.0, -1.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=dt, device=dev)
    h = (t * lam) @ s
    ok = h[2, 2].detach().abs() > 1e-20
    return torch.where(ok, h / torch.where(ok, h[2, 2], one), h)


def _curve(z, crf):
    sp = nn.functional.softplus
    toe, shoulder, gamma = 0.3 + sp(crf[:, 0]), 0.3 + sp(crf[:, 1]), 0.1 + sp(crf[:, 2])
    centre = torch.sigmoid(crf[:, 3]).clamp(1e-6, 1 - 1e-6)
    a = shoulder * centre / ((shoulder - toe) * centre + toe).clamp_min(1e-6)
    b = 1 - a
    active = (z > 0) & (z < 1)                                   # elsewhere the curve passes no gradient at all
    zs = torch.where(active, z, torch.full_like(z, 0.5))
    lo = zs <= centre
    below = a * (torch.where(lo, zs, centre.expand_as(zs)) / centre) ** toe
    above = 1 - b * ((1 - torch.where(lo, centre.expand_as(zs), zs)) / (1 - centre)) ** shoulder
    y = torch.where(lo, below, above)
    pos = y > 0
    live = torch.where(pos, torch.where(pos, y, torch.ones_like(y)) ** gamma, torch.zeros_like(y))
    with torch.no_grad():
        zc = z.clamp(0, 1)
        dead = torch.where(zc <= centre, a * (zc / centre) ** toe, 1 - b * ((1 - zc) / (1 - centre)) ** shoulder).clamp_min(0) ** gamma
    return torch.where(active, live, dead)


def ppisp_torch(rgb, pixel_coords, resolution_w, resolution_h, exposure=None, color=None, vignetting=None, crf=None):
    """The model on the already selected rows (exposure [1], color [8], vignetting [3,5], crf [3,4]; None: stage off), in rgb's dtype."""
    x = rgb
    dt = x.dtype
    if exposure is not None:
        x = x * torch.exp2(exposure.to(dt).reshape(()))
    if vignetting is not None:
        w, h = float(resolution_w), float(resolution_h)
        vig = vignetting.to(dt).reshape(3, 5)
        uv = (pixel_coords.to(dt) - torch.tensor([w / 2, h / 2], dtype=dt, device=x.device)) / max(w, h)
        d = uv[..., None, :] - vig[:, :2]
        r2 = (d * d).sum(-1)
        x = x * torch.clamp(1 + vig[:, 2] * r2 + vig[:, 3] * r2 ** 2 + vig[:, 4] * r2 ** 3, 0, 1)   # clamp's gradient passes on [0, 1], inclusive
    if color is not None:
        hm = _homography(color.to(dt).reshape(8))
        inten = x.sum(-1, keepdim=True)
        v = torch.cat([x[..., :2], inten], -1) @ hm.T
        v = v * (inten / (v[..., 2:3] + 1e-5))
        x = torch.cat([v[..., :2], v[..., 2:3] - v[..., 0:1] - v[..., 1:2]], -1)
    if crf is not None:
        x = _curve(x, crf.to(dt).reshape(3, 4))
    return x


# ---- the HIP path -----------------------------------------------------------------------------------------------------------------------
def _row_ptr(t, row):
    """Device pointer of row `row` of a contiguous fp32 tensor (None: NULL, the stage is off / the gradient is not wanted)."""
    if t is None:
        return C.c_void_p(None)
    return C.c_void_p(t.data_ptr() + row * (t.numel() // t.shape[0]) * 4)


class _PPISPApply(torch.autograd.Function):
    """rgb [P,3], pc [P,2] or None, the four FULL parameter tensors (None: stage off) and the row of each that applies."""

    @staticmethod
    def forward(ctx, rgb, pc, exposure, color, vignetting, crf, res_w, res_h, frame, camera):
        lib = _abi.load_library()
        out = torch.empty_like(rgb)
        stats["forward_calls"] += 1
        with torch.cuda.device(rgb.device):   # the launch goes to the image's device, whichever is current
            _abi.check(lib.grut_ppisp_forward(
                C.c_void_p(torch.cuda.current_stream(rgb.device).cuda_stream), rgb.shape[0], _row_ptr(rgb, 0), _row_ptr(pc, 0), res_w, res_h,
                _row_ptr(exposure, frame), _row_ptr(color, frame), _row_ptr(vignetting, camera), _row_ptr(crf, camera), _row_ptr(out, 0)),
                "grut_ppisp_forward")
        ctx.save_for_backward(rgb, pc, exposure, color, vignetting, crf)
        ctx.args = (res_w, res_h, frame, camera)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        rgb, pc, exposure, color, vignetting, crf = ctx.saved_tensors
        res_w, res_h, frame, camera = ctx.args
        lib = _abi.load_library()
        grad_out = grad_out.contiguous()
        need = ctx.needs_input_grad
        g_rgb = torch.empty_like(rgb) if need[0] else None
        # full-shape gradients, zero outside the selected row, which the library writes in place
        g_par = [torch.zeros_like(t) if t is not None and need[2 + i] else None for i, t in enumerate((exposure, color, vignetting, crf))]
        partials = torch.empty(int(lib.grut_ppisp_partials(rgb.shape[0])), dtype=torch.float32, device=rgb.device)
        stats["backward_calls"] += 1
        with torch.cuda.device(rgb.device):
            _abi.check(lib.grut_ppisp_backward(
                C.c_void_p(torch.cuda.current_stream(rgb.device).cuda_stream), rgb.shape[0], _row_ptr(rgb, 0), _row_ptr(pc, 0), res_w, res_h,
                _row_ptr(exposure, frame), _row_ptr(color, frame), _row_ptr(vignetting, camera), _row_ptr(crf, camera), _row_ptr(grad_out, 0),
                _row_ptr(g_rgb, 0), _row_ptr(g_par[0], frame), _row_ptr(g_par[1], frame), _row_ptr(g_par[2], camera), _row_ptr(g_par[3], camera),
                _row_ptr(partials, 0)), "grut_ppisp_backward")
        return (g_rgb, None, *g_par, None, None, None, None)


def _is_hip_tensor(t):
    return t is None or (t.is_cuda and t.dtype == torch.float32)


def ppisp_apply(exposure_params=None, vignetting_params=None, color_params=None, crf_params=None, rgb_in=None, pixel_coords=None,
                resolution_w=1, resolution_h=1, camera_idx=-1, frame_idx=-1):
    """The PPISP camera model on rgb_in [..., 3] with pixel_coords [..., 2] ((x, y) with their +0.5) -> [..., 3].

    exposure_params [F], color_params [F, 8]: row frame_idx applies; frame_idx < 0 (or None for the tensor) turns the stage off.
    vignetting_params [C, 3, 5], crf_params [C, 3, 4]: row camera_idx applies; camera_idx < 0 (or None) turns the stage off.
    Differentiable in rgb_in and the four parameter tensors; a parameter's gradient has the full tensor's shape and is zero outside the
    selected row.  fp32 CUDA tensors run csrc/ppisp.hip (non-contiguous inputs are made contiguous); anything else runs ppisp_torch."""
    if rgb_in is None or rgb_in.shape[-1] != 3:
        raise ValueError("rgb_in must be a [..., 3] tensor")
    frame, camera = int(frame_idx), int(camera_idx)
    if frame < 0:
        exposure_params = color_params = None
    if camera < 0:
        vignetting_params = crf_params = None
    for t, name, idx, tail in ((exposure_params, "exposure_params", frame, ()), (color_params, "color_params", frame, (8,)),
                               (vignetting_params, "vignetting_params", camera, (3, 5)), (crf_params, "crf_params", camera, (3, 4))):
        if t is not None and (t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail or idx >= t.shape[0]):
            raise ValueError(f"{name} must be [N{''.join(f', {d}' for d in tail)}] with N > {idx} (got {list(t.shape)})")
    if vignetting_params is not None and (pixel_coords is None or pixel_coords.shape[:-1] != rgb_in.shape[:-1] or pixel_coords.shape[-1] != 2):
        raise ValueError("pixel_coords must be [..., 2] with rgb_in's leading shape")
    tensors = (rgb_in, pixel_coords if vignetting_params is not None else None, exposure_params, color_params, vignetting_params, crf_params)
    if rgb_in.numel() == 0 or not all(_is_hip_tensor(t) for t in tensors) or any(t is not None and t.device != rgb_in.device for t in tensors):
        stats["torch_calls"] += 1
        return ppisp_torch(rgb_in, pixel_coords, resolution_w, resolution_h,
                           None if exposure_params is None else exposure_params[frame], None if color_params is None else color_params[frame],
                           None if vignetting_params is None else vignetting_params[camera], None if crf_params is None else crf_params[camera])
    pc = None if vignetting_params is None else pixel_coords.detach().reshape(-1, 2).contiguous()
    out = _PPISPApply.apply(rgb_in.reshape(-1, 3).contiguous(), pc, *(None if t is None else t.contiguous() for t in tensors[2:]),
                            float(resolution_w), float(resolution_h), max(frame, 0), max(camera, 0))
    return out.reshape(rgb_in.shape)


# ---- the module ----------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class PPISPConfig:
    use_controller: bool = True
    controller_distillation: bool = False
    controller_activation_ratio: float = 0.8
    # the regulariser's weights (get_regularization_loss) and the optimisers' settings: this project's choices
    exposure_mean_weight: float = 1.0
    color_mean_weight: float = 1.0
    vignetting_center_weight: float = 0.02
    vignetting_positive_alpha_weight: float = 0.01
    vignetting_channel_variance_weight: float = 0.1
    crf_channel_variance_weight: float = 0.1
    lr: float = 2e-3
    eps: float = 1e-15
    controller_lr: float = 2e-3
    warmup_steps: int = 500
    warmup_start_factor: float = 0.01
    final_lr_factor: float = 0.01


_fused_controller = False


def install_fused_controller(enable: bool = True) -> bool:
    """Switch the controllers' fp32 CUDA forward (and their weight gradients) to csrc/ppisp_controller.hip.  Off by default; returns the
    previous state.  Inputs the kernels do not take keep running the torch code (see _PPISPController.forward)."""
    global _fused_controller
    previous, _fused_controller = _fused_controller, bool(enable)
    return previous


class _ControllerApply(torch.autograd.Function):
    """hdr [H, W, 3], prior [1] (neither differentiable), keep (a backward may follow: the forward writes what it needs) and the sixteen
    parameters in the order of the C entry point -> [9]: the exposure, then the colour latents."""

    @staticmethod
    def forward(ctx, hdr, prior, keep, *params):
        lib = _abi.load_library()
        h, w = int(hdr.shape[0]), int(hdr.shape[1])
        dev = hdr.device
        out = torch.empty(9, dtype=torch.float32, device=dev)
        saved = torch.empty(_abi.PPISP_CONTROLLER_SAVED, dtype=torch.float32, device=dev) if keep else None
        scratch = torch.empty(int(lib.grut_ppisp_controller_forward_scratch(h, w)), dtype=torch.float32, device=dev)
        weights = (C.c_void_p * 16)(*[p.data_ptr() for p in params])   # read live at every launch: nothing of the weights is cached
        stats["controller_hip_calls"] += 1
        with torch.cuda.device(dev):
            _abi.check(lib.grut_ppisp_controller_forward(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), h, w, _row_ptr(hdr, 0),
                                                         _row_ptr(prior, 0), weights, _row_ptr(scratch, 0), _row_ptr(saved, 0), _row_ptr(out, 0)),
                       "grut_ppisp_controller_forward")
        if saved is not None:
            ctx.save_for_backward(hdr, prior, saved, *params)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        hdr, prior, saved, *params = ctx.saved_tensors
        lib = _abi.load_library()
        h, w = int(hdr.shape[0]), int(hdr.shape[1])
        dev = hdr.device
        grad_out = grad_out.to(torch.float32).contiguous()
        grads = [torch.empty_like(p) for p in params]   # the library writes every tensor completely
        scratch = torch.empty(int(lib.grut_ppisp_controller_backward_scratch(h, w)), dtype=torch.float32, device=dev)
        stats["controller_hip_backward_calls"] += 1
        with torch.cuda.device(dev):
            _abi.check(lib.grut_ppisp_controller_backward(
                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), h, w, _row_ptr(hdr, 0), _row_ptr(prior, 0),
                (C.c_void_p * 16)(*[p.data_ptr() for p in params]), _row_ptr(saved, 0), _row_ptr(grad_out, 0), _row_ptr(scratch, 0),
                (C.c_void_p * 16)(*[g.data_ptr() for g in grads])), "grut_ppisp_controller_backward")
        return (None, None, None, *(g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:])))


class _PPISPController(nn.Module):
    """Per-camera predictor of a frame's exposure and colour latents from the rendered image: the architecture the reference's exporter
    checks (export/usd/post_processing/ppisp_controller_weights.py).  The heads start at zero: no correction."""

    def __init__(self):
        super().__init__()
        self.cnn_encoder = nn.Sequential(nn.Conv2d(3, 16, 1), nn.MaxPool2d(3, 3), nn.ReLU(), nn.Conv2d(16, 32, 1), nn.ReLU(),
                                         nn.Conv2d(32, 64, 1), nn.AdaptiveAvgPool2d((5, 5)))
        self.mlp_trunk = nn.Sequential(nn.Linear(64 * 5 * 5 + 1, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU())
        self.exposure_head = nn.Linear(128, 1)
        self.color_head = nn.Linear(128, 8)
        for head in (self.exposure_head, self.color_head):
            nn.init.zeros_(head.weight)
            nn.init.zeros_(head.bias)

    def _fused_parameters(self):
        """The sixteen tensors in the order of grut_ppisp_controller_forward (the reference's flatten_controller_weights)."""
        layers = (self.cnn_encoder[0], self.cnn_encoder[3], self.cnn_encoder[5], self.mlp_trunk[0], self.mlp_trunk[2], self.mlp_trunk[4],
                  self.exposure_head, self.color_head)
        return [p for layer in layers for p in (layer.weight, layer.bias)]

    def forward(self, hdr, prior):
        """hdr [H, W, 3], prior [1] -> (exposure [], color [8]).  With install_fused_controller() on, an fp32 CUDA image that does not
        require grad (nor does prior), with all sixteen parameters fp32, contiguous and on its device, runs csrc/ppisp_controller.hip;
        every other input runs the torch code below."""
        if _fused_controller:
            params = self._fused_parameters()
            if (torch.is_tensor(hdr) and hdr.is_cuda and hdr.dtype == torch.float32 and hdr.dim() == 3 and hdr.shape[2] == 3
                    and min(hdr.shape[:2]) >= 3 and max(hdr.shape[:2]) <= 16384 and not hdr.requires_grad
                    and torch.is_tensor(prior) and prior.numel() >= 1 and prior.device == hdr.device and not prior.requires_grad
                    and all(p.is_cuda and p.device == hdr.device and p.dtype == torch.float32 and p.is_contiguous() for p in params)):
                keep = torch.is_grad_enabled() and any(p.requires_grad for p in params)
                out = _ControllerApply.apply(hdr.contiguous(), prior.reshape(-1)[:1].to(torch.float32).contiguous(), keep, *params)
                return out[0], out[1:]
        stats["controller_torch_calls"] += 1
        features = self.cnn_encoder(hdr.permute(2, 0, 1).unsqueeze(0)).reshape(-1)
        trunk = self.mlp_trunk(torch.cat([features, prior.reshape(1).to(features.dtype)]))
        return self.exposure_head(trunk).reshape(()), self.color_head(trunk)


class PPISP(nn.Module):
    """Per-frame exposure and colour latents, per-camera vignetting and response curve, identity-initialised, and (use_controller) one
    controller per camera that predicts exposure and colour for frames that have no row: novel views, and every frame once the
    controller is active."""

    def __init__(self, num_cameras: int, num_frames: int, config: PPISPConfig | None = None):
        super().__init__()
        self.config = config if config is not None else PPISPConfig()
        self.num_cameras, self.num_frames = int(num_cameras), int(num_frames)
        self.exposure_params = nn.Parameter(torch.zeros(self.num_frames))
        self.color_params = nn.Parameter(torch.zeros(self.num_frames, 8))
        self.vignetting_params = nn.Parameter(torch.zeros(self.num_cameras, 3, 5))
        self.crf_params = nn.Parameter(torch.tensor(CRF_IDENTITY, dtype=torch.float32).repeat(self.num_cameras, 3, 1))
        self.controllers = nn.ModuleList([_PPISPController() for _ in range(self.num_cameras)] if self.config.use_controller else [])
        self.register_buffer("step", torch.zeros((), dtype=torch.long))   # training-mode forwards with a frame row, kept in the checkpoint
        self._step_host = 0            # the same count on the host: reading the buffer every step would wait for the device
        self.max_optimization_iters = None   # set by create_schedulers; the controller is never active before

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self._step_host = None         # re-read from the buffer on next use

    @property
    def steps_done(self) -> int:
        if self._step_host is None:
            self._step_host = int(self.step.item())
        return self._step_host

    @property
    def controller_active(self) -> bool:
        """In training mode, from step controller_activation_ratio * max_optimization_iters on (create_schedulers tells the length)."""
        if not (self.training and len(self.controllers) and self.max_optimization_iters is not None):
            return False
        return self.steps_done >= self.config.controller_activation_ratio * self.max_optimization_iters

    @classmethod
    def from_state_dict(cls, state_dict, config: PPISPConfig | None = None):
        if config is None:
            config = PPISPConfig(use_controller=any(k.startswith("controllers.") for k in state_dict))
        module = cls(num_cameras=state_dict["crf_params"].shape[0], num_frames=state_dict["exposure_params"].shape[0], config=config)
        missing, unexpected = module.load_state_dict(state_dict, strict=False)
        if unexpected or [k for k in missing if k != "step"]:
            raise RuntimeError(f"PPISP.from_state_dict: missing {missing}, unexpected {unexpected}")
        return module

    def forward(self, rgb, pixel_coords, resolution, camera_idx=-1, frame_idx=-1, exposure_prior=None):
        """rgb [P, 3] (or [H, W, 3]), pixel_coords likewise with 2, resolution (W, H) -> rgb's shape (utils/render.py:140-147)."""
        w, h = int(resolution[0]), int(resolution[1])
        camera = -1 if camera_idx is None else int(camera_idx)
        frame = -1 if frame_idx is None else int(frame_idx)
        active = self.controller_active
        if self.training and frame >= 0:
            self.step += 1
            self._step_host = self.steps_done + 1
        exposure, color, vignetting, crf = self.exposure_params, self.color_params, self.vignetting_params, self.crf_params
        if frame < 0 or active:
            frame = -1
            if len(self.controllers) and camera >= 0:
                if rgb.numel() != w * h * 3:
                    raise ValueError(f"the controller needs the whole image: {rgb.numel() // 3} pixels for a resolution of {w} x {h}")
                prior = torch.zeros(1, dtype=rgb.dtype, device=rgb.device) if exposure_prior is None else \
                    torch.as_tensor(exposure_prior, dtype=rgb.dtype, device=rgb.device).reshape(-1)[:1]
                e, c = self.controllers[camera](rgb.detach().reshape(h, w, 3), prior)
                exposure, color, frame = e.reshape(1), c.reshape(1, 8), 0
            if active and self.config.controller_distillation:   # only the controller learns
                rgb, vignetting, crf = rgb.detach(), vignetting.detach(), crf.detach()
        return ppisp_apply(exposure_params=exposure, vignetting_params=vignetting, color_params=color, crf_params=crf, rgb_in=rgb,
                           pixel_coords=pixel_coords, resolution_w=w, resolution_h=h, camera_idx=camera, frame_idx=frame)

    def create_optimizers(self):
        c = self.config
        optimizers = [torch.optim.Adam([self.exposure_params, self.color_params, self.vignetting_params, self.crf_params], lr=c.lr, eps=c.eps)]
        if len(self.controllers):
            optimizers.append(torch.optim.Adam(self.controllers.parameters(), lr=c.controller_lr))
        return optimizers

    def create_schedulers(self, optimizers, max_optimization_iters: int):
        """One LambdaLR each: linear warm-up from warmup_start_factor over warmup_steps, times an exponential decay that reaches
        final_lr_factor at the last iteration."""
        self.max_optimization_iters = int(max_optimization_iters)
        c, total = self.config, max(int(max_optimization_iters), 1)

        def factor(step):
            warm = c.warmup_start_factor + (1.0 - c.warmup_start_factor) * min(step / max(c.warmup_steps, 1), 1.0)
            return warm * c.final_lr_factor ** (min(step, total) / total)

        return [torch.optim.lr_scheduler.LambdaLR(o, factor) for o in optimizers]

    def get_regularization_loss(self):
        c = self.config
        vig = self.vignetting_params
        return (c.exposure_mean_weight * self.exposure_params.mean() ** 2
                + c.color_mean_weight * (self.color_params.mean(0) ** 2).mean()
                + c.vignetting_center_weight * (vig[..., :2] ** 2).mean()
                + c.vignetting_positive_alpha_weight * (torch.relu(vig[..., 2:]) ** 2).mean()
                + c.vignetting_channel_variance_weight * vig.var(dim=1, unbiased=False).mean()
                + c.crf_channel_variance_weight * self.crf_params.var(dim=1, unbiased=False).mean())


def export_ppisp_report(module: PPISP, frames_per_camera, output_dir, camera_names=None):
    """One `<camera name>.json` per camera under output_dir: its vignetting and response-curve parameters and the exposure and colour rows
    of its frames (the frames are numbered camera by camera, frames_per_camera[i] of them for camera i).  -> the paths written."""
    os.makedirs(output_dir, exist_ok=True)
    frames_per_camera = [int(n) for n in frames_per_camera]
    names = list(camera_names) if camera_names is not None else [f"camera_{i}" for i in range(len(frames_per_camera))]
    if len(names) != len(frames_per_camera):
        raise ValueError("camera_names and frames_per_camera must have the same length")
    tolist = lambda t: t.detach().cpu().tolist()   # noqa: E731
    paths, first = [], 0
    for cam, (name, count) in enumerate(zip(names, frames_per_camera)):
        rows = range(first, min(first + count, module.num_frames))
        report = {"camera": str(name), "camera_index": cam,
                  "vignetting_params": tolist(module.vignetting_params[cam]) if cam < module.num_cameras else None,
                  "crf_params": tolist(module.crf_params[cam]) if cam < module.num_cameras else None,
                  "has_controller": cam < len(module.controllers),
                  "frames": [{"frame_index": f, "exposure": float(module.exposure_params[f]), "color": tolist(module.color_params[f])} for f in rows]}
        path = os.path.join(str(output_dir), f"{str(name).replace(os.sep, '_')}.json")
        with open(path, "w") as fh:
            json.dump(report, fh, indent=1)
        paths.append(path)
        first += count
    return paths


def install() -> None:
    """Make `from ppisp import PPISP, PPISPConfig` (threedgrut/trainer.py:470) and `from ppisp.report import export_ppisp_report`
    (trainer.py:988) bind to this module.  Modules of those names that are already in sys.modules win.  Imports nothing of threedgrut."""
    this = sys.modules[__name__]
    if SHIM_MODULE not in sys.modules:
        mod = types.ModuleType(SHIM_MODULE)
        mod.__doc__ = "HIP PPISP of 3dgrut_amd.ppisp under the name of the upstream CUDA package."
        mod.__path__ = []
        for name in ("PPISP", "PPISPConfig", "ppisp_apply"):
            setattr(mod, name, getattr(this, name))
        mod.__all__ = ["PPISP", "PPISPConfig", "ppisp_apply"]
        sys.modules.setdefault(SHIM_MODULE, mod)
    if SHIM_MODULE + ".report" not in sys.modules:
        report = types.ModuleType(SHIM_MODULE + ".report")
        report.export_ppisp_report = export_ppisp_report
        report.__all__ = ["export_ppisp_report"]
        sys.modules.setdefault(SHIM_MODULE + ".report", report)
        if getattr(sys.modules[SHIM_MODULE], "report", None) is None:
            sys.modules[SHIM_MODULE].report = report
