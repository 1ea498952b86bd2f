"""The NHT decoder's network on the MI355X: drop-in for the CUDA-only package `tinycudann` that the reference's feature decoder imports
(threedgrut/model/feature_decoder.py:16) for `model.feature_type: nht`, with a fused HIP forward (csrc/mlp.hip) and an opt-in fused HIP
backward (csrc/mlp_backward.hip).

    NetworkWithInputEncoding(n_input_dims=F+3, n_output_dims=, encoding_config=, network_config=, seed=1337)
                the module the decoder builds (feature_decoder.py:69-99): `params` (one flat fp32 nn.Parameter), n_input_dims,
                n_output_dims, n_params; called with [P, F+3] rows whose last three columns are (dir * sh_scale + 1) / 2 -> [P, n_output_dims] fp32
    mlp_torch(params, x, cfg)   the same model in plain torch, on any device and float dtype, differentiable in x and params: the path of
                everything the kernel does not take, the backward of the training step, and the benchmark's baseline (scripts/bench_mlp.py)
    mlp_backward_torch(params, x, grad_out, cfg)   the contract of grut_mlp_backward in plain torch, on any device -> (grad_x, grad_params)
    install_fused_backward(enable=True)   opt-in: the training step's backward runs csrc/mlp_backward.hip; returns the previous state
    install()   registers a module named `tinycudann` (unless one is already in sys.modules); called by the tracer shims

The model - encoding, layer shapes, the layout of `params`, the bf16 rounding points - is stated at grut_mlp_forward in include/grut_amd.h.
tiny-cuda-nn's source is not part of the reference checkout, so everything beyond the call surface above is this project's choice
(INTEGRATION.md section 3c); checkpoints of decoders trained by tiny-cuda-nn are not claimed to load.

Dispatch.  A contiguous fp32 CUDA [P >= 1, F+3] input with fp32 `params` on the same device, width 64 or 128, n_output_dims <= 16,
K0 <= 128 and a weight image that fits into LDS runs the HIP kernel; anything else runs mlp_torch, which agrees with it within the
tolerance of tests/mlp_reference.py.  With grad enabled the forward is still the kernel.  The backward, by default, re-runs mlp_torch
on the saved input and weights under autograd.  After install_fused_backward() it is ONE fused HIP kernel (plus an ordered reduction of
the weight gradient) for every configuration with grut_mlp_backward_lds_bytes != 0: it recomputes the forward from the saved input and
the live weights, rounds every dZ once to bf16 and sums in fp32 without atomics (the rules: grut_mlp_backward in include/grut_amd.h;
mlp_backward_torch states them in torch).  The switch is off by default until a training run of an NHT configuration has used it.
Both kernels read `params` afresh at every launch: nothing derived from the weights is kept anywhere, because the decoder's EMA swaps
them through `param.data.copy_`, which no version counter sees.
"""
from __future__ import annotations

import ctypes as C
import math
import sys
import types
from typing import NamedTuple

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _abi

SHIM_MODULE = "tinycudann"
OUT_ROWS = 16                 # rows of the output matrix in `params`
ACTIVATIONS = {"none": _abi.MLP_ACT_NONE, "relu": _abi.MLP_ACT_RELU, "sigmoid": _abi.MLP_ACT_SIGMOID}
stats = {"hip_calls": 0, "torch_calls": 0, "backward_calls": 0, "hip_backward_calls": 0}   # which path ran (tests); plain counters
_fused_backward = False       # install_fused_backward()


class MlpConfig(NamedTuple):
    """GrutMlpConfig of include/grut_amd.h; output_activation is one of ACTIVATIONS' keys."""
    n_features: int
    sh_degree: int
    n_hidden_layers: int
    width: int
    n_output_dims: int
    output_activation: str

    @property
    def k0(self) -> int:
        """the encoded width F + L^2, padded with ones to a multiple of 16"""
        return (self.n_features + self.sh_degree ** 2 + 15) // 16 * 16

    @property
    def matrices(self):
        """(rows, columns) of the matrices of `params`, in order"""
        return [(self.width, self.k0)] + [(self.width, self.width)] * (self.n_hidden_layers - 1) + [(OUT_ROWS, self.width)]

    @property
    def n_params(self) -> int:
        return sum(r * c for r, c in self.matrices)

    def as_struct(self):
        return _abi.GrutMlpConfig(self.n_features, self.sh_degree, self.n_hidden_layers, self.width, self.n_output_dims,
                                  ACTIVATIONS[self.output_activation])


# ---- the model in torch ---------------------------------------------------------------------------------------------------------------------
def _bf16(t):
    """round to bf16 (nearest even), straight-through for the gradient"""
    return t + (t.detach().to(torch.bfloat16).to(t.dtype) - t.detach())


def sh_encoding(d, degree: int):
    """the first degree^2 real SH polynomials of the contract for d [..., 3] (not normalised) -> [..., degree^2]"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz = x * x, y * y, z * z
    v = [torch.full_like(x, 0.28209479177387814),
         -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
         1.0925484305920792 * (x * y), -1.0925484305920792 * (y * z), 0.94617469575755997 * zz - 0.31539156525251999,
         -1.0925484305920792 * (x * z), 0.54627421529603959 * (xx - yy),
         0.59004358992664352 * (y * (-3.0 * xx + yy)), 2.8906114426405538 * (x * y * z), 0.45704579946446572 * (y * (1.0 - 5.0 * zz)),
         0.3731763325901154 * (z * (5.0 * zz - 3.0)), 0.45704579946446572 * (x * (1.0 - 5.0 * zz)), 1.4453057213202769 * (z * (xx - yy)),
         0.59004358992664352 * (x * (-xx + 3.0 * yy))]
    return torch.stack(v[:degree * degree], dim=-1)


def mlp_torch(params, x, cfg: MlpConfig):
    """The model on x [P, F+3] with the flat `params`: fp64 arithmetic for an fp64 x, fp32 otherwise; -> [P, n_output_dims] in that dtype.
    The bf16 roundings of the weights, the encoded input and the hidden activations are straight-through."""
    dt = torch.float64 if x.dtype == torch.float64 else torch.float32
    x = x.to(dt)
    f, k0 = cfg.n_features, cfg.k0
    enc = [x[:, :f], sh_encoding(2.0 * x[:, f:f + 3] - 1.0, cfg.sh_degree)]
    if k0 > f + cfg.sh_degree ** 2:
        enc.append(torch.ones((x.shape[0], k0 - f - cfg.sh_degree ** 2), dtype=dt, device=x.device))
    h = _bf16(torch.cat(enc, dim=1))
    offset = 0
    for i, (rows, columns) in enumerate(cfg.matrices):
        last = i == cfg.n_hidden_layers
        rows = cfg.n_output_dims if last else rows              # the padded output rows are never read
        w = _bf16(params[offset:offset + rows * columns].to(dt).reshape(rows, columns))
        offset += cfg.matrices[i][0] * columns
        h = h @ w.T
        if not last:
            h = _bf16(torch.relu(h))
    if cfg.output_activation == "relu":
        h = torch.relu(h)
    elif cfg.output_activation == "sigmoid":
        h = torch.sigmoid(h)
    return h


def sh_jacobian(d, degree: int):
    """d sh_encoding(d, degree) / d d for d [P, 3] -> [P, degree^2, 3]"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz = x * x, y * y, z * z
    o, one = torch.zeros_like(x), torch.ones_like(x)
    c1, c2, c3, c5 = 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.54627421529603959
    c6, c7, c8, c9, c10 = 0.59004358992664352, 2.8906114426405538, 0.45704579946446572, 0.3731763325901154, 1.4453057213202769
    rows = [(o, o, o), (o, -c1 * one, o), (o, o, c1 * one), (-c1 * one, o, o), (c2 * y, c2 * x, o), (o, -c2 * z, -c2 * y), (o, o, 2 * c3 * z),
            (-c2 * z, o, -c2 * x), (2 * c5 * x, -2 * c5 * y, o), (-6 * c6 * x * y, c6 * (-3 * xx + 3 * yy), o),
            (c7 * y * z, c7 * x * z, c7 * x * y), (o, c8 * (1 - 5 * zz), -10 * c8 * y * z), (o, o, c9 * (15 * zz - 3)),
            (c8 * (1 - 5 * zz), o, -10 * c8 * x * z), (2 * c10 * x * z, -2 * c10 * y * z, c10 * (xx - yy)),
            (c6 * (-3 * xx + 3 * yy), 6 * c6 * x * y, o)]
    return torch.stack([torch.stack(r, dim=-1) for r in rows[:degree * degree]], dim=-2)


@torch.no_grad()
def mlp_backward_torch(params, x, grad_out, cfg: MlpConfig):
    """The contract of grut_mlp_backward (include/grut_amd.h) in plain torch, on any device: fp64 arithmetic for an fp64 x, fp32
    otherwise.  The forward is computed again with its rounding points; every dZ (the gradient with respect to a layer's pre-activation,
    after its ReLU gate or the output activation's derivative) is rounded once to bf16 and that rounded dZ enters both W^T dZ and
    dZ H^T; the forward's roundings are straight-through; the SH Jacobian and the factor 2 are not rounded.
    -> (grad_x [P, F+3], grad_params [n_params]) in that dtype; the output matrix's rows >= n_output_dims get zero."""
    dt = torch.float64 if x.dtype == torch.float64 else torch.float32

    def rb(t):
        return t.to(torch.bfloat16).to(dt)

    x = x.to(dt)
    f, k0, n_sh = cfg.n_features, cfg.k0, cfg.sh_degree ** 2
    d = 2.0 * x[:, f:f + 3] - 1.0
    enc = [x[:, :f], sh_encoding(d, cfg.sh_degree)]
    if k0 > f + n_sh:
        enc.append(torch.ones((x.shape[0], k0 - f - n_sh), dtype=dt, device=x.device))
    hs, zs, ws, offset = [rb(torch.cat(enc, dim=1))], [], [], 0
    for i, (rows, columns) in enumerate(cfg.matrices):
        used = cfg.n_output_dims if i == cfg.n_hidden_layers else rows
        ws.append(rb(params[offset:offset + used * columns].to(dt).reshape(used, columns)))
        offset += rows * columns
        zs.append(hs[-1] @ ws[-1].T)
        if i < cfg.n_hidden_layers:
            hs.append(rb(torch.relu(zs[-1])))
    g = grad_out.to(dt)
    if cfg.output_activation == "relu":
        g = g * (zs[-1] > 0)
    elif cfg.output_activation == "sigmoid":
        y = torch.sigmoid(zs[-1])
        g = g * (y * (1.0 - y))
    grads = []
    for i in range(cfg.n_hidden_layers, -1, -1):
        if i < cfg.n_hidden_layers:
            g = g * (zs[i] > 0)
        g = rb(g)
        gw = g.T @ hs[i]
        if i == cfg.n_hidden_layers:
            gw = torch.cat([gw, torch.zeros((OUT_ROWS - cfg.n_output_dims, gw.shape[1]), dtype=dt, device=x.device)])
        grads.insert(0, gw.reshape(-1))
        g = g @ ws[i]
    g_d = torch.einsum("pi,pic->pc", g[:, f:f + n_sh], sh_jacobian(d, cfg.sh_degree))
    return torch.cat([g[:, :f], 2.0 * g_d], dim=1), torch.cat(grads)


# ---- the HIP path -----------------------------------------------------------------------------------------------------------------------------
def lds_bytes(cfg: MlpConfig) -> int:
    """grut_mlp_lds_bytes: the size of the kernel's weight image, 0 when the kernel does not take the configuration"""
    if cfg.output_activation not in ACTIVATIONS:
        return 0
    return int(_abi.load_library().grut_mlp_lds_bytes(C.byref(cfg.as_struct())))


def takes_hip(params, x, cfg: MlpConfig) -> bool:
    """the dispatch rule of the module's docstring"""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] >= 1 and x.shape[0] < 2 ** 32 and x.is_contiguous()
            and params.dtype == torch.float32 and params.device == x.device and params.is_contiguous() and params.data_ptr() % 16 == 0
            and cfg.width in (64, 128) and cfg.n_output_dims <= OUT_ROWS and cfg.k0 <= 128 and lds_bytes(cfg) != 0)


def mlp_forward_hip(params, x, cfg: MlpConfig):
    """One launch of csrc/mlp.hip on tensors that takes_hip() accepts -> [P, n_output_dims] fp32.  Not differentiable."""
    lib = _abi.load_library()
    out = torch.empty((x.shape[0], cfg.n_output_dims), dtype=torch.float32, device=x.device)
    stats["hip_calls"] += 1
    with torch.cuda.device(x.device):   # the launch goes to the input's device, whichever is current
        _abi.check(lib.grut_mlp_forward(C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream), C.byref(cfg.as_struct()),
                                        C.c_void_p(params.data_ptr()), C.c_void_p(x.data_ptr()), x.shape[0], C.c_void_p(out.data_ptr())),
                   "grut_mlp_forward")
    return out


def backward_lds_bytes(cfg: MlpConfig) -> int:
    """grut_mlp_backward_lds_bytes: the LDS of the fused backward, 0 when it does not take the configuration"""
    if cfg.output_activation not in ACTIVATIONS:
        return 0
    return int(_abi.load_library().grut_mlp_backward_lds_bytes(C.byref(cfg.as_struct())))


def mlp_backward_hip(params, x, grad_out, cfg: MlpConfig, need_x: bool = True, need_params: bool = True):
    """csrc/mlp_backward.hip on tensors that takes_hip() accepts, for a configuration with backward_lds_bytes != 0 and a contiguous fp32
    grad_out [P, n_output_dims] -> (grad_x or None, grad_params or None).  The scratch comes from torch's allocator, per call."""
    lib = _abi.load_library()
    struct, n = cfg.as_struct(), x.shape[0]
    grad_x = torch.empty_like(x) if need_x else None
    grad_params = torch.empty_like(params) if need_params else None
    scratch = None
    if need_params:
        scratch = torch.empty(int(lib.grut_mlp_backward_scratch_bytes(C.byref(struct), n)), dtype=torch.uint8, device=x.device)
    stats["hip_backward_calls"] += 1
    with torch.cuda.device(x.device):
        _abi.check(lib.grut_mlp_backward(C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream), C.byref(struct),
                                         C.c_void_p(params.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(grad_out.data_ptr()), n,
                                         C.c_void_p(scratch.data_ptr() if need_params else None),
                                         C.c_void_p(grad_x.data_ptr() if need_x else None),
                                         C.c_void_p(grad_params.data_ptr() if need_params else None)),
                   "grut_mlp_backward")
    return grad_x, grad_params


def install_fused_backward(enable: bool = True) -> bool:
    """Opt-in: while on, the backward of the training Function runs the fused HIP kernel wherever it takes the tensors and the
    configuration (takes_hip, backward_lds_bytes != 0); everything else keeps the mlp_torch backward.  Returns the previous state."""
    global _fused_backward
    previous, _fused_backward = _fused_backward, bool(enable)
    return previous


class _MlpFunction(torch.autograd.Function):
    """The training step: the forward is the kernel and keeps only x and params; the backward recomputes the forward from them, in
    mlp_torch under autograd or, after install_fused_backward(), in the fused kernel."""

    @staticmethod
    def forward(ctx, x, params, cfg):
        ctx.save_for_backward(x, params)
        ctx.cfg = cfg
        return mlp_forward_hip(params.detach(), x.detach(), cfg)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, params = ctx.saved_tensors
        need_x, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        stats["backward_calls"] += 1
        if _fused_backward and (need_x or need_p) and takes_hip(params, x, ctx.cfg) and backward_lds_bytes(ctx.cfg) != 0 \
                and grad_out.device == x.device:
            grad_x, grad_params = mlp_backward_hip(params.detach(), x.detach(), grad_out.detach().to(torch.float32).contiguous(), ctx.cfg,
                                                   need_x, need_p)
            return grad_x, grad_params, None
        with torch.enable_grad():
            xg, pg = x.detach().requires_grad_(need_x), params.detach().requires_grad_(need_p)
            y = mlp_torch(pg, xg, ctx.cfg)
            grads = torch.autograd.grad(y, [t for t, need in ((xg, need_x), (pg, need_p)) if need], grad_out.to(y.dtype))
        grads = list(grads)
        return (grads.pop(0) if need_x else None, grads.pop(0) if need_p else None, None)


def mlp(params, x, cfg: MlpConfig):
    """The model with the dispatch of the module's docstring; differentiable in x and params."""
    if x.dim() != 2 or x.shape[1] != cfg.n_features + 3 or params.dim() != 1 or params.numel() != cfg.n_params:
        raise ValueError(f"tinycudann drop-in: x must be [P, {cfg.n_features + 3}] and params [{cfg.n_params}] "
                         f"(got {list(x.shape)} and {list(params.shape)})")
    if not takes_hip(params, x, cfg):
        stats["torch_calls"] += 1
        return mlp_torch(params, x, cfg)
    if torch.is_grad_enabled() and (x.requires_grad or params.requires_grad):
        return _MlpFunction.apply(x, params, cfg)
    return mlp_forward_hip(params.detach(), x.detach(), cfg)


# ---- the module -------------------------------------------------------------------------------------------------------------------------------
def _refuse(key, value, supported):
    raise NotImplementedError(f"tinycudann drop-in: {key} = {value!r} is not supported (supported: {supported})")


def parse_configs(n_input_dims: int, n_output_dims: int, encoding_config, network_config) -> MlpConfig:
    """The two dictionaries of feature_decoder.py:69-90 -> MlpConfig.  Anything the model does not cover raises NotImplementedError
    naming the key."""
    enc = dict(encoding_config)
    if enc.get("otype") != "Composite":
        _refuse("encoding_config.otype", enc.get("otype"), "Composite of Identity and SphericalHarmonics")
    nested = [dict(e) for e in enc.get("nested", [])]
    identity = [e for e in nested if e.get("otype") == "Identity"]
    others = [e for e in nested if e.get("otype") != "Identity"]
    if len(identity) > 1 or (identity and nested[0] is not identity[0]):
        _refuse("encoding_config.nested", [e.get("otype") for e in nested], "one leading Identity, then one SphericalHarmonics")
    if len(others) != 1:
        _refuse("encoding_config.nested", [e.get("otype") for e in nested], "exactly one nested encoding besides Identity")
    sh = others[0]
    if sh.get("otype") != "SphericalHarmonics":
        _refuse("encoding_config.nested.otype", sh.get("otype"), "SphericalHarmonics")
    if int(sh.get("n_dims_to_encode", 3)) != 3:
        _refuse("encoding_config.nested.n_dims_to_encode", sh.get("n_dims_to_encode"), "3 for SphericalHarmonics")
    degree = int(sh.get("degree", 4))
    if not 1 <= degree <= 4:
        _refuse("encoding_config.nested.degree", sh.get("degree"), "1..4")
    n_features = int(identity[0].get("n_dims_to_encode", int(n_input_dims) - 3)) if identity else 0
    if n_features + 3 != int(n_input_dims):
        raise ValueError(f"tinycudann drop-in: the encodings take {n_features} + 3 input columns, n_input_dims is {n_input_dims}")
    net = dict(network_config)
    if net.get("otype", "FullyFusedMLP") != "FullyFusedMLP":
        _refuse("network_config.otype", net.get("otype"), "FullyFusedMLP")
    if str(net.get("activation", "ReLU")) != "ReLU":
        _refuse("network_config.activation", net.get("activation"), "ReLU")
    output_activation = str(net.get("output_activation", "None")).lower()
    if output_activation not in ACTIVATIONS:
        _refuse("network_config.output_activation", net.get("output_activation"), "None, ReLU, Sigmoid")
    width, layers = int(net.get("n_neurons", 128)), int(net.get("n_hidden_layers", 5))
    if width < 1 or width % 16:
        _refuse("network_config.n_neurons", net.get("n_neurons"), "a positive multiple of 16")
    if layers < 1:
        _refuse("network_config.n_hidden_layers", net.get("n_hidden_layers"), ">= 1")
    if not 1 <= int(n_output_dims) <= OUT_ROWS:
        _refuse("n_output_dims", n_output_dims, f"1..{OUT_ROWS}")
    return MlpConfig(n_features, degree, layers, width, int(n_output_dims), output_activation)


def initial_params(cfg: MlpConfig, seed: int = 1337):
    """Xavier uniform per matrix (the output matrix with its 16 rows) from a CPU generator: the same seed gives the same weights on every
    device."""
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    parts = []
    for rows, columns in cfg.matrices:
        bound = math.sqrt(6.0 / (rows + columns))
        parts.append((torch.rand(rows * columns, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound)
    return torch.cat(parts)


class NetworkWithInputEncoding(nn.Module):
    """tinycudann.NetworkWithInputEncoding as the reference's decoder uses it: [P, n_input_dims] -> [P, n_output_dims] fp32."""

    def __init__(self, n_input_dims: int, n_output_dims: int, encoding_config, network_config, seed: int = 1337):
        super().__init__()
        self.cfg = parse_configs(n_input_dims, n_output_dims, encoding_config, network_config)
        self.n_input_dims, self.n_output_dims = int(n_input_dims), int(n_output_dims)
        self.encoding_config, self.network_config, self.seed = encoding_config, network_config, int(seed)
        self.params = nn.Parameter(initial_params(self.cfg, seed))
        self.n_params = self.params.numel()

    def forward(self, x):
        if x.dim() != 2 or x.shape[1] != self.n_input_dims:
            raise ValueError(f"tinycudann drop-in: the input must be [P, {self.n_input_dims}] (got {list(x.shape)})")
        return mlp(self.params, x, self.cfg)

    def extra_repr(self) -> str:
        return f"n_input_dims={self.n_input_dims}, n_output_dims={self.n_output_dims}, n_params={self.n_params}, {self.cfg}"


def install() -> None:
    """Make `import tinycudann as tcnn` (threedgrut/model/feature_decoder.py:16) bind to this module.  A module of that name that is
    already in sys.modules wins.  Imports nothing of threedgrut."""
    if SHIM_MODULE in sys.modules:
        return
    mod = types.ModuleType(SHIM_MODULE)
    mod.__doc__ = "HIP decoder network of 3dgrut_amd.tcnn under the name of the upstream CUDA package."
    mod.__path__ = []
    mod.NetworkWithInputEncoding = NetworkWithInputEncoding
    mod.__all__ = ["NetworkWithInputEncoding"]
    sys.modules.setdefault(SHIM_MODULE, mod)
