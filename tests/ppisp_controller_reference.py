"""The yardstick of the fused PPISP controller's tests: `_PPISPController` itself in float64 on the CPU, autograd for the gradients, and
the conditioning that keeps every gate (max-pool choice, ReLU) of a test image away from rounding.

A gate that flips between fp32 and fp64 is another model, not an error.  `make_case` therefore evaluates the float64 model and redraws
the 3x3 input window of every downsampled pixel with a conv1 maximum or a conv2 pre-activation within MARGIN of 0, or a runner-up
within MARGIN of a maximum that is above -MARGIN (below, the ReLU hides the choice); a trunk pre-activation within MARGIN of 0 redraws
window (0, 0).  At most MAX_ROUNDS rounds, asserted, and afterwards no pixel is flagged: none is left out of any comparison."""
import copy
import importlib

import torch

MARGIN = 1e-5
MAX_ROUNDS = 10
SHAPES = ((3, 5), (9, 13), (15, 15), (31, 37), (121, 212), (97, 1001))
SEEDS = {(31, 37): 2}      # every other shape: seed 0
NAMES = ("conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b", "trunk0.w", "trunk0.b", "trunk1.w", "trunk1.b",
         "trunk2.w", "trunk2.b", "exposure.w", "exposure.b", "colour.w", "colour.b")
EPS32 = 2.0 ** -23


def parameters(ctrl):
    """The sixteen tensors in the order of the C entry point."""
    layers = (ctrl.cnn_encoder[0], ctrl.cnn_encoder[3], ctrl.cnn_encoder[5], ctrl.mlp_trunk[0], ctrl.mlp_trunk[2], ctrl.mlp_trunk[4],
              ctrl.exposure_head, ctrl.color_head)
    return [p for layer in layers for p in (layer.weight, layer.bias)]


def make_controller(seed):
    """Default initialisation, except the heads: at their zero initialisation every trunk and CNN gradient is 0."""
    ppisp = importlib.import_module("3dgrut_amd.ppisp")
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        ctrl = ppisp._PPISPController()
        with torch.no_grad():
            for head in (ctrl.exposure_head, ctrl.color_head):
                head.weight.normal_(0.0, 0.1)
                head.bias.normal_(0.0, 0.1)
    return ctrl


def flagged(ctrl64, hdr64, prior64):
    """[dsH, dsW] bool: the downsampled pixels whose window has to be redrawn."""
    h, w = hdr64.shape[:2]
    dsh, dsw = h // 3, w // 3
    w1, b1, w2, b2 = (p.detach() for p in parameters(ctrl64)[:4])
    win = hdr64[:3 * dsh, :3 * dsw].reshape(dsh, 3, dsw, 3, 3).permute(0, 2, 1, 3, 4).reshape(dsh, dsw, 9, 3)
    c1 = win @ w1.reshape(16, 3).T + b1
    top = c1.topk(2, dim=2).values
    m, runner = top[:, :, 0], top[:, :, 1]
    z2 = torch.relu(m) @ w2.reshape(32, 16).T + b2
    bad = (m.abs() < MARGIN).any(-1) | (z2.abs() < MARGIN).any(-1) | (((m - runner) < MARGIN) & (m > -MARGIN)).any(-1)
    with torch.no_grad():
        x = torch.cat([ctrl64.cnn_encoder(hdr64.permute(2, 0, 1).unsqueeze(0)).reshape(-1), prior64.reshape(1)])
        for layer in ctrl64.mlp_trunk:
            if isinstance(layer, torch.nn.Linear) and bool(((layer(x)).abs() < MARGIN).any()):
                bad[0, 0] = True
            x = layer(x)
    return bad


def evaluate(ctrl, hdr, prior, grad_out, dtype):
    """-> (out [9], the sixteen gradients of sum(out * grad_out)) of a copy of ctrl in dtype, on the CPU."""
    c = copy.deepcopy(ctrl).to(dtype)
    for p in c.parameters():
        p.grad = None
    e, col = c(hdr.to(dtype), prior.to(dtype))
    out = torch.cat([e.reshape(1), col])
    (out * grad_out.to(dtype)).sum().backward()
    return out.detach(), [p.grad.detach() for p in parameters(c)]


def rel(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def make_case(h, w, seed=None):
    """A conditioned image with its float64 results and the errors of CPU fp32 torch against them."""
    seed = SEEDS.get((h, w), 0) if seed is None else seed
    ctrl = make_controller(seed)
    g = torch.Generator().manual_seed(seed)
    hdr = torch.rand(h, w, 3, generator=g) * 1.5
    prior = torch.tensor([0.3])
    grad_out = torch.randn(9, generator=g)
    ctrl64 = copy.deepcopy(ctrl).double()
    redrawn, rounds = 0, 0
    while True:
        bad = flagged(ctrl64, hdr.double(), prior.double())
        if not bool(bad.any()):
            break
        rounds += 1
        assert rounds <= MAX_ROUNDS, f"{h}x{w}: still {int(bad.sum())} windows within {MARGIN} of a gate after {MAX_ROUNDS} rounds"
        for dy, dx in bad.nonzero().tolist():
            hdr[3 * dy:3 * dy + 3, 3 * dx:3 * dx + 3] = torch.rand(3, 3, 3, generator=g) * 1.5
            redrawn += 1
    assert not bool(flagged(ctrl64, hdr.double(), prior.double()).any())       # no pixel is left out of any comparison
    out64, g64 = evaluate(ctrl, hdr, prior, grad_out, torch.float64)
    out32, g32 = evaluate(ctrl, hdr, prior, grad_out, torch.float32)
    assert all(float(t.abs().max()) > 0 for t in g64)
    return {"h": h, "w": w, "ctrl": ctrl, "hdr": hdr, "prior": prior, "grad_out": grad_out, "out64": out64, "g64": g64,
            "e32_out": rel(out32, out64), "e32": [rel(a, b) for a, b in zip(g32, g64)], "redrawn": redrawn, "rounds": rounds}
