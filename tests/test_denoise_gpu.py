"""GPU: csrc/denoise.hip (grut_denoise, 3dgrut_amd.denoise.denoise, playground_tracer.Tracer.denoise) against tests/denoise_reference.py,
the float64 restatement of the model evaluated on the same fp32 inputs.

Sizes, from the kernel's own tile (denoise.TILE_W x TILE_H): images smaller than the patch, than the search window and than a tile;
exactly one tile; one past a tile on both axes; several ragged tiles; and the widest halo (f = 4, r = 16: the LDS image above 64 KiB).
Inputs are uniform noise in [0, 1], and Fixture Q (two flat colours, a ramp, noise of sigma 0.1).

Bound (denoise_reference.bound, the issue's, unchanged), u = 2^-24, n = 3 (2f+1)^2:
    eps = 80 (n + 4) u + 24 u        |a - b| <= 2 eps S + ((2r+1)^2 + 4) u M        S the channel's spread, M its largest magnitude
Largest error / bound measured on the MI355X over the cases below: 0.0040 ((2, 37, 53) at f = 0, r = 1, where n is smallest and the
bound tightest); 0.0005 at the defaults and on Fixture Q, 0.0005 at f = 4, r = 16.  The bound is a worst case over n roundings of one
sign; the sums' roundings largely cancel.

No case provokes anything: every pointer handed to the entry point is a live allocation of at least the stated size, and stray writes
are looked for in sentinel bands around a view, not by running past an allocation."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import denoise_reference as ref

pytestmark = pytest.mark.gpu
BAD_INPUT = -1
DEFAULTS = (3, 7)


def _dn():
    return importlib.import_module("3dgrut_amd.denoise")


def _abi():
    return importlib.import_module("3dgrut_amd._abi")


def _cases():
    tw, th = _dn().TILE_W, _dn().TILE_H
    shapes = [(1, 1, 1), (1, 1, 7), (1, 5, 3), (1, th, tw), (1, th + 1, tw + 1), (1, 2 * th + 3, 3 * tw + 5), (2, 37, 53)]
    return [(s, 3, 7) for s in shapes] + [((2, 37, 53), f, r) for f, r in ((0, 1), (1, 2), (2, 5), (4, 16))]


CASES = _cases()
IDS = ["x".join(map(str, s)) + f"-f{f}r{r}" for s, f, r in CASES]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("shape,f,r", CASES, ids=IDS)
def test_hip_matches_the_reference(shape, f, r):
    image, want = ref.uniform_case(shape, f, r)
    x = torch.from_numpy(image.copy()).cuda()
    before = dict(_dn().stats)
    got = _dn().denoise(x, f, r, 0.1)
    assert {k: _dn().stats[k] - before[k] for k in before} == {"hip_calls": 1, "torch_calls": 0}
    assert got.shape == x.shape and got.dtype == torch.float32 and got.is_cuda and got.data_ptr() != x.data_ptr()
    ratio = ref.worst_ratio(got.cpu().numpy(), want, image, f, r)
    print(f"{shape} f={f} r={r}: error / bound = {ratio:.4f}")
    assert ratio <= 1.0
    assert torch.equal(_bits(x.cpu()), _bits(torch.from_numpy(image.copy())))      # the input is not written
    # determinism: two calls on the same input are bitwise equal
    assert torch.equal(_bits(got), _bits(_dn().denoise(x, f, r, 0.1)))
    # batch isolation: a batch equals its single-image calls bitwise
    for b in range(shape[0]):
        assert torch.equal(_bits(got[b]), _bits(_dn().denoise(x[b], f, r, 0.1)))
    if shape == (2, 37, 53):
        assert ref.in_window_range(got.cpu().numpy(), image, f, r)
        if (f, r) == DEFAULTS:                                                         # the two images in the other order: still isolated
            assert torch.equal(_bits(_dn().denoise(x.flip(0).contiguous(), f, r, 0.1)), _bits(got.flip(0)))


def test_fixture_q_matches_the_reference_and_meets_the_quality_condition():
    clean, noisy = ref.fixture_q()
    got = _dn().denoise(torch.from_numpy(noisy.copy()).cuda()).cpu().numpy()
    ratio = ref.worst_ratio(got, ref.fixture_q_reference(), noisy, *DEFAULTS)
    mse_noisy, mse_out = float(((noisy.astype(np.float64) - clean) ** 2).mean()), float(((got.astype(np.float64) - clean) ** 2).mean())
    print(f"Fixture Q: error / bound = {ratio:.4f}; MSE noisy {mse_noisy:.3e}, denoised {mse_out:.3e}: 1/{mse_noisy / mse_out:.1f}")
    assert ratio <= 1.0
    assert mse_out <= mse_noisy / 8
    assert ref.in_window_range(got, noisy, *DEFAULTS)


def _call(lib, cfg, batch, height, width, src, dst):
    ptr = lambda t: t if isinstance(t, C.c_void_p) else C.c_void_p(t.data_ptr())      # noqa: E731
    return lib.grut_denoise(C.c_void_p(torch.cuda.current_stream().cuda_stream), None if cfg is None else C.byref(cfg), batch, height, width,
                            ptr(src), ptr(dst))


def test_guard_bands_stay_intact():
    """rgb_out and rgb_in are views into the middle of larger sentinel-filled allocations."""
    abi, lib = _abi(), _abi().load_library()
    shape, (f, r) = (2, 37, 53), DEFAULTS
    image, want = ref.uniform_case(shape, f, r)
    count, band = image.size, 4096
    sentinel_in, sentinel_out = 12345.0, -54321.0
    src = torch.full((count + 2 * band,), sentinel_in, device="cuda")
    dst = torch.full((count + 2 * band,), sentinel_out, device="cuda")
    src[band:band + count] = torch.from_numpy(image.copy()).reshape(-1).cuda()
    held = src.clone()
    assert _call(lib, abi.GrutDenoiseConfig(f, r, 0.1), *shape, src[band:], dst[band:]) == 0, lib.grut_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(src), _bits(held))                                      # the input and its bands
    assert bool((dst[:band] == sentinel_out).all()) and bool((dst[band + count:] == sentinel_out).all())
    got = dst[band:band + count].reshape(image.shape).cpu().numpy()
    assert not (got == sentinel_out).any() and ref.worst_ratio(got, want, image, f, r) <= 1.0


def test_bad_input_is_refused_before_any_launch():
    """Every tensor is a real one of the stated size, so nothing here could fault even if a check were missing."""
    abi, lib = _abi(), _abi().load_library()
    B, H, W = 2, 6, 5
    src = torch.rand(B, H, W, 3, device="cuda")
    dst = torch.zeros(B, H, W, 3, device="cuda")
    good = abi.GrutDenoiseConfig(3, 7, 0.1)
    null = C.c_void_p(None)

    def refused(status, text):
        assert status == BAD_INPUT and text in lib.grut_last_error().decode(), (status, lib.grut_last_error())

    refused(_call(lib, None, B, H, W, src, dst), "cfg is NULL")
    refused(_call(lib, good, B, H, W, null, dst), "rgb_in is NULL")
    refused(_call(lib, good, B, H, W, src, null), "rgb_out is NULL")
    refused(_call(lib, good, B, H, W, src, src), "rgb_in and rgb_out overlap")
    both = torch.zeros(2 * B * H * W * 3 - 3, device="cuda")                          # two ranges that share their last / first pixel
    refused(_call(lib, good, B, H, W, both, both[B * H * W * 3 - 3:]), "rgb_in and rgb_out overlap")
    refused(_call(lib, good, B, H, W, both[B * H * W * 3 - 3:], both), "rgb_in and rgb_out overlap")
    for f in (-1, 5):
        refused(_call(lib, abi.GrutDenoiseConfig(f, 7, 0.1), B, H, W, src, dst), "patch_radius")
    for r in (0, 17, -3):
        refused(_call(lib, abi.GrutDenoiseConfig(3, r, 0.1), B, H, W, src, dst), "search_radius")
    for h in (0.0, -0.1, float("inf"), float("nan")):
        refused(_call(lib, abi.GrutDenoiseConfig(3, 7, h), B, H, W, src, dst), "grut_denoise: h =")
    refused(_call(lib, good, B, 0, W, src, dst), "height is 0")
    refused(_call(lib, good, B, H, 0, src, dst), "width is 0")
    refused(_call(lib, good, 2, 32768, 32768, src, dst), "must be below 2^31")         # exactly 2^31 pixels
    refused(_call(lib, good, 65536, 65536, 65536, src, dst), "must be below 2^31")     # a product that wraps 64 bits' lower half
    assert _call(lib, good, 0, H, W, src, dst) == 0                                    # an empty batch: OK, nothing launched
    torch.cuda.synchronize()
    assert float(dst.abs().sum()) == 0.0 and float(both.abs().sum()) == 0.0            # nothing ran
    # adjacent, not overlapping: accepted
    pair = torch.rand(2, B, H, W, 3, device="cuda")
    assert _call(lib, good, B, H, W, pair[0], pair[1]) == 0, lib.grut_last_error()
    torch.cuda.synchronize()


def test_fallback_and_stats():
    dn = _dn()
    image, want = ref.uniform_case((2, 37, 53), *DEFAULTS)
    x = torch.from_numpy(image.copy())
    before = dict(dn.stats)
    half = dn.denoise(x.cuda().half())
    assert half.dtype == torch.float16 and half.is_cuda and half.shape == x.shape
    cpu = dn.denoise(x)
    assert not cpu.is_cuda and cpu.dtype == torch.float32
    assert {k: dn.stats[k] - before[k] for k in before} == {"hip_calls": 0, "torch_calls": 2}
    assert ref.worst_ratio(cpu.numpy(), want, image, *DEFAULTS) <= 1.0
    # the torch statement on the device is the same model within the same bound
    assert ref.worst_ratio(dn.denoise_torch(x.cuda()).cpu().numpy(), want, image, *DEFAULTS) <= 1.0
    # a non-contiguous fp32 CUDA view takes the kernel and matches the contiguous call bitwise
    wide = torch.cat([x, torch.zeros_like(x)], dim=-1).cuda()
    view = wide[..., :3]
    assert not view.is_contiguous()
    before = dict(dn.stats)
    got = dn.denoise(view)
    assert {k: dn.stats[k] - before[k] for k in before} == {"hip_calls": 1, "torch_calls": 0}
    assert torch.equal(_bits(got), _bits(dn.denoise(x.cuda())))
    assert torch.equal(wide.cpu(), torch.cat([x, torch.zeros_like(x)], dim=-1))         # and the view's parent is as it was
    with pytest.raises(ValueError):
        dn.denoise(x.cuda(), search_radius=17)


def test_end_to_end_through_the_playground_tracer():
    """One frame of the `mixed` scene at 48 x 32, tonemapped as the engine does, through Tracer.denoise."""
    import playground_scenes as ps
    from test_hybrid_gpu import _render
    dn = _dn()
    sc = ps.make_playground_scene("mixed", width=48, height=32)
    res, tracer = _render(sc, ps.OPT_SMOOTH_NORMALS, 5, 3)
    frame = torch.as_tensor(res["pred_features"], device="cuda")[None].clamp(0, 1) ** (1 / 2.2)
    assert frame.shape == (1, 32, 48, 3)
    held = frame.clone()
    before = dict(dn.stats)
    out = tracer.denoise(frame)
    assert {k: dn.stats[k] - before[k] for k in before} == {"hip_calls": 1, "torch_calls": 0}
    assert out.shape == frame.shape and out.dtype == frame.dtype and out.device == frame.device
    assert bool(torch.isfinite(out).all())
    assert torch.equal(_bits(frame), _bits(held)) and out.data_ptr() != frame.data_ptr()
    assert ref.in_window_range(out.cpu().numpy(), frame.cpu().numpy(), *DEFAULTS)
    assert torch.equal(_bits(out), _bits(dn.denoise(frame)))
    # the plugin's keys reach the kernel
    pt = importlib.import_module("3dgrut_amd.playground_tracer")
    other = pt.Tracer({"render": {"denoiser": {"patch_radius": 1, "search_radius": 2, "strength": 0.15}}})
    assert torch.equal(_bits(other.denoise(frame)), _bits(dn.denoise(frame, 1, 2, 0.15)))
    assert not torch.equal(_bits(other.denoise(frame)), _bits(out))
