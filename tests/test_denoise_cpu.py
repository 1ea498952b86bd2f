"""CPU: the denoiser's model (3dgrut_amd/denoise.py: denoise_torch, the fallback of denoise) against tests/denoise_reference.py, the
properties of the model that the GPU tests lean on, the parameter rules, and the contract of playground_tracer.Tracer.denoise as the
reference's engine uses it (threedgrut_playground/engine.py:1091-1094).  The bound of every comparison is denoise_reference.bound."""
import importlib
import sys
import types

import numpy as np
import pytest
import torch

import denoise_reference as ref

DEFAULTS = (3, 7)
SHAPES = [(1, 1, 1), (1, 1, 7), (1, 5, 3), (2, 19, 23)]
CASES = [(s, f, r) for s in SHAPES for f, r in ((3, 7), (0, 1), (1, 2))] + [((2, 19, 23), 4, 16)]
IDS = ["x".join(map(str, s)) + f"-f{f}r{r}" for s, f, r in CASES]


def _dn():
    return importlib.import_module("3dgrut_amd.denoise")


@pytest.mark.parametrize("shape,f,r", CASES, ids=IDS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_denoise_torch_matches_the_reference(shape, f, r, dtype):
    image, want = ref.uniform_case(shape, f, r)
    x = torch.from_numpy(image.copy()).to(dtype)
    got = _dn().denoise_torch(x, f, r, 0.1)
    assert got.shape == x.shape and got.dtype == dtype
    ratio = ref.worst_ratio(got.numpy(), want, image, f, r)
    print(f"{shape} f={f} r={r} {dtype}: error / bound = {ratio:.4f}")
    assert ratio <= 1.0
    assert torch.equal(x, torch.from_numpy(image.copy()).to(dtype))            # the input is not written
    # [H, W, 3] is the batch of one
    single = _dn().denoise_torch(x[0], f, r, 0.1)
    assert single.shape == x.shape[1:] and torch.equal(single, got[0])


def test_the_inputs_discriminate_a_halo_off_by_one():
    """On Fixture Q at h = 0.15 a search radius of 6 instead of 7, and the image rolled by one column, each move the reference by more
    than ten times the bound: a kernel whose halo or whose indexing is off by one cannot pass the comparison."""
    _, noisy = ref.fixture_q()
    b = ref.bound(noisy, 3, 7).max()
    base = ref.fixture_q_reference(3, 7, 0.15)
    by_radius = np.abs(ref.fixture_q_reference(3, 6, 0.15) - base).max()
    by_roll = np.abs(ref.fixture_q_reference(3, 7, 0.15, roll=1) - base).max()
    print(f"bound {b:.3e}, r = 6 against 7: {by_radius:.3e}, rolled by one column: {by_roll:.3e}")
    assert by_radius > 10 * b and by_roll > 10 * b


def test_quality_condition_on_fixture_q():
    """At the defaults the reference's MSE against the clean image is at most 1/8 of the noisy image's."""
    clean, noisy = ref.fixture_q()
    mse_noisy = float(((noisy.astype(np.float64) - clean) ** 2).mean())
    mse_out = float(((ref.fixture_q_reference() - clean) ** 2).mean())
    print(f"MSE noisy {mse_noisy:.3e}, denoised {mse_out:.3e}: 1/{mse_noisy / mse_out:.1f}")
    assert mse_out <= mse_noisy / 8
    # and the torch statement of the model meets the same condition through the same comparison
    got = _dn().denoise_torch(torch.from_numpy(noisy.copy())).numpy()
    assert ref.worst_ratio(got, ref.fixture_q_reference(), noisy, *DEFAULTS) <= 1.0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_value_checks(dtype):
    dn = _dn()
    f, r = DEFAULTS
    # a constant image comes back unchanged within the accumulation's own error
    value = torch.tensor([0.7, 0.25, 0.05], dtype=dtype)
    const = value.expand(2, 9, 11, 3).contiguous()
    out = dn.denoise_torch(const)
    assert float((out - const).abs().max()) <= ((2 * r + 1) ** 2 + 4) * ref.U * float(value.max())
    # every output channel lies in the range of its search window, enlarged by the bound
    for shape, ff, rr in (((2, 19, 23), 3, 7), ((2, 19, 23), 1, 2)):
        image, _ = ref.uniform_case(shape, ff, rr)
        got = dn.denoise_torch(torch.from_numpy(image.copy()).to(dtype), ff, rr, 0.1).numpy()
        assert ref.in_window_range(got, image, ff, rr)
    # a 1x1 image returns itself
    one = torch.tensor([[[[0.3, 0.9, 0.6]]]], dtype=dtype)
    assert torch.equal(dn.denoise_torch(one), one) and torch.equal(dn.denoise(one), one)
    # a window narrower than the image really is a constraint the reference meets and a wrong window would not
    image, want = ref.uniform_case((2, 19, 23), 1, 2)
    assert ref.in_window_range(want, image, 1, 2) and not ref.in_window_range(np.roll(want, 5, axis=2), image, 1, 2)


@pytest.mark.parametrize("kwargs", [dict(patch_radius=-1), dict(patch_radius=5), dict(patch_radius=1.5), dict(search_radius=0),
                                    dict(search_radius=17), dict(h=0.0), dict(h=-0.1), dict(h=float("inf")), dict(h=float("nan"))],
                         ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_parameter_rules_raise_value_error(kwargs):
    dn = _dn()
    x = torch.rand(1, 4, 5, 3)
    for fn in (dn.denoise, dn.denoise_torch):
        with pytest.raises(ValueError):
            fn(x, **kwargs)
    for bad in (torch.rand(4, 5), torch.rand(1, 4, 5, 4), torch.zeros(1, 4, 5, 3, dtype=torch.int32), torch.rand(1, 0, 5, 3)):
        with pytest.raises(ValueError):
            dn.denoise(bad)


def _cpu_tracer(monkeypatch, conf):
    """playground_tracer.Tracer through its own constructor, with the native handle (which needs a GPU) replaced by a stub."""
    grt = importlib.import_module("3dgrut_amd.grt_tracer")
    monkeypatch.setattr(grt, "_GrtNative", lambda cfg: types.SimpleNamespace(cfg=cfg))
    return importlib.import_module("3dgrut_amd.playground_tracer").Tracer(conf)


def test_tracer_denoise_contract_on_the_fallback(monkeypatch):
    dn = _dn()
    _, noisy = ref.fixture_q()
    for dtype in (torch.float32, torch.float64, torch.float16):
        frame = torch.from_numpy(noisy.copy()).to(dtype)
        held = frame.clone()
        tracer = _cpu_tracer(monkeypatch, {"render": {}})
        assert tracer._denoiser == (3, 7, 0.1)                                        # no render.denoiser node: the defaults
        before = dict(dn.stats)
        out = tracer.denoise(frame)
        assert {k: dn.stats[k] - before[k] for k in before} == {"hip_calls": 0, "torch_calls": 1}
        assert out.shape == frame.shape and out.dtype == frame.dtype and out.device == frame.device
        assert torch.equal(frame.view(torch.int16 if dtype == torch.float16 else torch.int32 if dtype == torch.float32 else torch.int64),
                           held.view(torch.int16 if dtype == torch.float16 else torch.int32 if dtype == torch.float32 else torch.int64))
        assert out.untyped_storage().data_ptr() != frame.untyped_storage().data_ptr()
        if dtype != torch.float16:
            assert ref.worst_ratio(out.numpy(), ref.fixture_q_reference(), noisy, *DEFAULTS) <= 1.0
    # [H, W, 3] and a view that is not contiguous
    frame = torch.from_numpy(noisy.copy())
    wide = torch.cat([frame, torch.zeros_like(frame)], dim=-1)
    assert not wide[..., :3].is_contiguous()
    assert torch.equal(tracer.denoise(wide[..., :3]), tracer.denoise(frame)) and torch.equal(tracer.denoise(frame[0]), tracer.denoise(frame)[0])


def test_tracer_honours_render_denoiser_keys(monkeypatch):
    _, noisy = ref.fixture_q()
    frame = torch.from_numpy(noisy.copy())
    conf = {"render": {"denoiser": {"patch_radius": 1, "search_radius": 2, "strength": 0.15}}}
    tracer = _cpu_tracer(monkeypatch, conf)
    assert tracer._denoiser == (1, 2, 0.15)
    want = ref.fixture_q_reference(1, 2, 0.15)
    assert ref.worst_ratio(tracer.denoise(frame).numpy(), want, noisy, 1, 2) <= 1.0
    assert np.abs(want - ref.fixture_q_reference()).max() > 10 * ref.bound(noisy, 3, 7).max()      # and that is not what the defaults give
    # attribute-style nodes (OmegaConf, SimpleNamespace) and a partial node: an absent key gives the default
    ns = types.SimpleNamespace(render=types.SimpleNamespace(denoiser=types.SimpleNamespace(strength=0.2)))
    assert _cpu_tracer(monkeypatch, ns)._denoiser == (3, 7, 0.2)
    with pytest.raises(ValueError):
        _cpu_tracer(monkeypatch, {"render": {"denoiser": {"search_radius": 40}}})


def test_engine_shaped_stub_keeps_its_accumulation_buffer(monkeypatch):
    """threedgrut_playground/engine.py:1091-1094 with use_optix_denoiser on, as Engine's constructor sets it."""
    _, noisy = ref.fixture_q()
    tracer = _cpu_tracer(monkeypatch, {"render": {}})
    engine = types.SimpleNamespace(tracer=tracer, use_optix_denoiser=True)
    rb = {"rgb": torch.from_numpy(noisy.copy())}
    held = rb["rgb"].clone()
    rb["rgb_buffer"] = rb["rgb"]
    if engine.use_optix_denoiser:
        rb["rgb"] = engine.tracer.denoise(rb["rgb"])
    assert torch.equal(rb["rgb_buffer"], held) and rb["rgb"] is not rb["rgb_buffer"]
    assert rb["rgb"].untyped_storage().data_ptr() != rb["rgb_buffer"].untyped_storage().data_ptr()
    rb["rgb"][:, :4] = 0.0                                                             # the engine's mask writes (engine.py:1096-1099) stay apart
    assert torch.equal(rb["rgb_buffer"], held)
    assert not torch.equal(rb["rgb"], rb["rgb_buffer"])
