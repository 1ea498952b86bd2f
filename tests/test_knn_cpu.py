"""CPU: the nearest-neighbour entry points are declared, mirrored and exported; they refuse bad arguments before anything is launched;
the float64 brute force that the GPU tests trust (tests/knn_reference.py) is pinned, bit for bit, to the reference's sklearn functions;
and `install_gpu_knn()` rebinds the reference's names and falls through to them for CPU tensors.  What the kernels compute is covered
by tests/test_knn_gpu.py."""
import ctypes as C
import importlib
import os
import re
import sys
import types

import pytest
import torch

import knn_reference as ref
from test_reference_seam_cpu import REFERENCE, reference  # noqa: F401  (the reference fixture and its import stubs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "threedgrut")),
                                     reason="the reference checkout is only present in the build container")
HOOKED = ("k_nearest_neighbors", "nearest_neighbors", "nearest_neighbor_dist_cpuKD")
BAD_INPUT = -1


def test_knn_symbols_are_declared_mirrored_and_exported(grut_lib):
    abi = importlib.import_module("3dgrut_amd._abi")
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    assert re.search(r"\bsize_t grut_knn_scratch_bytes\(uint32_t num_points, uint32_t num_queries\);", header)
    assert re.search(r"\bint grut_knn\(void\* stream, uint32_t num_points, const float\* points,", header)
    for name in ("grut_knn", "grut_knn_scratch_bytes"):
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(grut_lib, name) and getattr(grut_lib, name).argtypes, name
    assert "knn.hip" in importlib.import_module("3dgrut_amd.build").SOURCES
    assert abi.ABI_VERSION == 5 and grut_lib.grut_abi_version() == 5           # additive change


def test_scratch_bytes_is_non_zero_and_monotone(grut_lib):
    sizes = [int(grut_lib.grut_knn_scratch_bytes(n, 0)) for n in (1, 2, 255, 256, 257, 10_007, 1_000_000, 4_000_000, 2 ** 31 - 1)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert sizes[6] >= 1_000_000 * (16 + 4 * 4)        # the sorted rows and the four key / payload arrays at least
    with_queries = [int(grut_lib.grut_knn_scratch_bytes(10_007, q)) for q in (0, 1, 64, 2_049, 1_000_000)]
    assert all(a <= b for a, b in zip(with_queries, with_queries[1:])) and with_queries[-1] > with_queries[0]


def test_argument_refusals_return_bad_input_without_a_gpu(grut_lib):
    null, ptr = C.c_void_p(None), C.c_void_p(256)     # never dereferenced: every case is refused before anything is launched
    big = 1 << 40

    def call(p=100, points=ptr, q=0, queries=null, k=4, exclude=0, dist=ptr, index=ptr, scratch=ptr, nbytes=big, nonfinite=ptr):
        return grut_lib.grut_knn(null, p, points, q, queries, k, exclude, dist, index, scratch, nbytes, nonfinite)

    def refused(match, **kw):
        assert call(**kw) == BAD_INPUT
        assert re.search(match, grut_lib.grut_last_error().decode()), grut_lib.grut_last_error()

    refused("k must be in", k=17)
    refused("k must be in", k=0)
    refused("exceeds the 3 available", p=3, k=4)
    refused("exceeds the 3 available", p=4, k=4, exclude=1)
    refused("both NULL", dist=null, index=null)
    refused("points is NULL", points=null)
    refused("out_nonfinite is NULL", nonfinite=null)
    refused("scratch too small", nbytes=int(grut_lib.grut_knn_scratch_bytes(100, 0)) - 1)
    refused("scratch too small", scratch=null)
    refused("16-byte aligned", scratch=C.c_void_p(264))
    refused("exclude_self only applies", q=10, queries=ptr, exclude=1)
    refused("num_points must be in", p=0)
    refused("num_points must be in", p=2 ** 31)
    refused("num_points must be in", q=2 ** 31, queries=ptr)
    refused("num_queries = 0", q=0, queries=ptr)


def test_the_brute_force_is_sane():
    x = ref.uniform(300)
    d, i = ref.brute_force(x, k=4)
    assert bool((d[:, 0] == 0).all()) and bool((i[:, 0] == torch.arange(300)).all())        # no duplicates: a point is its own nearest
    assert bool((d[:, 1:] >= d[:, :-1]).all())
    assert torch.equal(ref.recomputed_distance(x, i), d)
    de, ie = ref.brute_force(x, k=3, exclude_self=True)
    assert torch.equal(de, d[:, 1:]) and torch.equal(ie, i[:, 1:])
    q = ref.uniform(50, seed=9) * 2 - 5
    dq, iq = ref.brute_force(x, q, k=2)
    full = torch.cdist(q.double(), x.double())
    assert torch.allclose(dq, full.sort(dim=1).values[:, :2], rtol=1e-12, atol=0)
    # chunking does not change anything
    saved, ref.CHUNK_ELEMS = ref.CHUNK_ELEMS, 1000
    try:
        d2, i2 = ref.brute_force(x, k=4)
    finally:
        ref.CHUNK_ELEMS = saved
    assert torch.equal(d2, d) and torch.equal(i2, i)
    # ties go to the lower index; more than k coincident points give exact zeros
    same = ref.identical(9)
    ds, is_ = ref.brute_force(same, k=4, exclude_self=True)
    assert bool((ds == 0).all()) and is_[0].tolist() == [1, 2, 3, 4] and is_[8].tolist() == [0, 1, 2, 3]


@needs_reference
@pytest.mark.parametrize("name", ["uniform", "clustered", "lattice"])
def test_brute_force_is_bit_equal_to_the_references_sklearn_functions(reference, name):  # noqa: F811
    pytest.importorskip("sklearn")
    geometry = importlib.import_module("threedgrut.model.geometry")
    assert geometry.__file__.startswith(REFERENCE)
    x = ref.DISTRIBUTIONS[name](3000)
    d64, _ = ref.brute_force(x, k=4)
    got = geometry.k_nearest_neighbors(x, 4)
    assert got.dtype == torch.float32 and torch.equal(got, d64.float())
    # nearest other point / nearest target: the reference recomputes the distance in torch from the index it found; the brute force's
    # index must give the same bits through the same expression (where several neighbours tie, they are at the same distance)
    _, i_other = ref.brute_force(x, k=1, exclude_self=True)
    want = torch.linalg.norm(x - x[i_other[:, 0], :], dim=-1)
    got = geometry.nearest_neighbor_dist_cpuKD(x)
    assert torch.equal(got, want)
    targets = ref.uniform(300, seed=11) * 1.5 - 2.0
    _, i_target = ref.brute_force(targets, x, k=1)
    want = torch.linalg.norm(x - targets[i_target[:, 0], :], dim=-1)
    assert torch.equal(geometry.nearest_neighbor_dist_cpuKD(x, targets), want)


def _fake_reference_modules(monkeypatch, calls):
    """threedgrut.model.geometry / .model as far as the hook touches them, with recording originals (no sklearn, no reference needed)."""
    def k_nearest_neighbors(x, K=4):
        """original k_nearest_neighbors"""
        calls.append(("k_nearest_neighbors", K))
        return torch.full((x.shape[0], K), 7.0)

    def nearest_neighbors(pts_src, k=2):
        calls.append(("nearest_neighbors", k))
        return torch.zeros((pts_src.shape[0], k - 1), dtype=torch.int64)

    def nearest_neighbor_dist_cpuKD(pts_src, pts_target=None):
        calls.append(("nearest_neighbor_dist_cpuKD", pts_target is not None))
        return torch.full((pts_src.shape[0],), 3.0)

    pkg, sub = types.ModuleType("threedgrut"), types.ModuleType("threedgrut.model")
    geometry, model = types.ModuleType("threedgrut.model.geometry"), types.ModuleType("threedgrut.model.model")
    pkg.__path__, sub.__path__ = [], []
    for fn in (k_nearest_neighbors, nearest_neighbors, nearest_neighbor_dist_cpuKD):
        setattr(geometry, fn.__name__, fn)
    model.k_nearest_neighbors, model.nearest_neighbor_dist_cpuKD = k_nearest_neighbors, nearest_neighbor_dist_cpuKD
    pkg.model, sub.geometry, sub.model = sub, geometry, model
    for name, mod in (("threedgrut", pkg), ("threedgrut.model", sub), ("threedgrut.model.geometry", geometry), ("threedgrut.model.model", model)):
        monkeypatch.setitem(sys.modules, name, mod)
    return geometry, model


def test_install_gpu_knn_rebinds_five_names_is_idempotent_and_falls_through_for_cpu_tensors(monkeypatch):
    knn = importlib.import_module("3dgrut_amd.knn")
    calls = []
    geometry, model = _fake_reference_modules(monkeypatch, calls)
    before = {name: getattr(geometry, name) for name in HOOKED}
    originals = knn.install_gpu_knn()
    assert originals == before
    for name in HOOKED:
        assert getattr(geometry, name) is not before[name] and getattr(geometry, name)._grut_gpu_knn
        assert getattr(geometry, name).__name__ == name
    assert model.k_nearest_neighbors is geometry.k_nearest_neighbors
    assert model.nearest_neighbor_dist_cpuKD is geometry.nearest_neighbor_dist_cpuKD
    installed = {name: getattr(geometry, name) for name in HOOKED}
    assert knn.install_gpu_knn() is originals                                   # a second call changes nothing
    assert all(getattr(geometry, name) is installed[name] for name in HOOKED)

    launched = knn.stats["calls"]
    x = torch.rand(10, 3)
    assert torch.equal(geometry.k_nearest_neighbors(x, 4), torch.full((10, 4), 7.0))
    assert torch.equal(geometry.nearest_neighbors(x, 3), torch.zeros((10, 2), dtype=torch.int64))
    assert torch.equal(model.nearest_neighbor_dist_cpuKD(x), torch.full((10,), 3.0))
    assert torch.equal(model.nearest_neighbor_dist_cpuKD(x, torch.rand(4, 3)), torch.full((10,), 3.0))
    assert calls == [("k_nearest_neighbors", 4), ("nearest_neighbors", 3), ("nearest_neighbor_dist_cpuKD", False),
                     ("nearest_neighbor_dist_cpuKD", True)]
    assert knn.stats["calls"] == launched

    # the other preconditions, on tensors that claim to be CUDA tensors: K > 16, a wrong dtype, a wrong shape
    class Cuda(torch.Tensor):
        is_cuda = True

    def no_kernel(*a, **k):
        raise AssertionError("the kernel wrapper was reached")

    monkeypatch.setattr(knn, "knn", no_kernel)
    cuda = torch.zeros(40, 3).as_subclass(Cuda)
    del calls[:]
    geometry.k_nearest_neighbors(cuda, 17)
    geometry.nearest_neighbors(cuda, 18)
    geometry.k_nearest_neighbors(torch.zeros(40, 3, dtype=torch.float64).as_subclass(Cuda), 4)
    geometry.nearest_neighbor_dist_cpuKD(torch.zeros(40, 2).as_subclass(Cuda))
    geometry.nearest_neighbor_dist_cpuKD(cuda, torch.zeros(5, 3))                # targets on the CPU
    assert [c[0] for c in calls] == ["k_nearest_neighbors", "nearest_neighbors", "k_nearest_neighbors", "nearest_neighbor_dist_cpuKD",
                                     "nearest_neighbor_dist_cpuKD"]
    with pytest.raises(AssertionError, match="wrapper was reached"):            # and a cloud that meets them does go to the kernel
        geometry.k_nearest_neighbors(cuda, 4)


@needs_reference
def test_install_gpu_knn_on_the_reference_modules_leaves_cpu_results_unchanged(reference):  # noqa: F811
    pytest.importorskip("sklearn")
    knn = importlib.import_module("3dgrut_amd.knn")
    geometry = importlib.import_module("threedgrut.model.geometry")
    model = importlib.import_module("threedgrut.model.model")
    assert geometry.__file__.startswith(REFERENCE) and model.k_nearest_neighbors is geometry.k_nearest_neighbors
    originals = knn.install_gpu_knn()
    assert model.k_nearest_neighbors is geometry.k_nearest_neighbors and geometry.k_nearest_neighbors is not originals["k_nearest_neighbors"]
    assert model.nearest_neighbor_dist_cpuKD is geometry.nearest_neighbor_dist_cpuKD
    assert knn.install_gpu_knn() is originals
    x, t = ref.clustered(500), ref.uniform(40, seed=3)
    assert torch.equal(geometry.k_nearest_neighbors(x, 4), originals["k_nearest_neighbors"](x, 4))
    assert torch.equal(geometry.nearest_neighbors(x, 3), originals["nearest_neighbors"](x, 3))
    assert torch.equal(geometry.nearest_neighbor_dist_cpuKD(x), originals["nearest_neighbor_dist_cpuKD"](x))
    assert torch.equal(geometry.nearest_neighbor_dist_cpuKD(x, t), originals["nearest_neighbor_dist_cpuKD"](x, t))


def test_wrapper_checks_raise_before_any_launch(monkeypatch):
    knn = importlib.import_module("3dgrut_amd.knn")
    abi = importlib.import_module("3dgrut_amd._abi")

    def no_launch(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(abi, "load_library", no_launch)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        knn.knn(torch.rand(10, 3))

    class Cuda(torch.Tensor):
        is_cuda = True

    def cuda(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(Cuda)

    with pytest.raises(RuntimeError, match="float32"):
        knn.knn(cuda(10, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"\[N, 3\]"):
        knn.knn(cuda(10, 4))
    with pytest.raises(ValueError, match="k must be in"):
        knn.knn(cuda(40, 3), k=17)
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        knn.knn(cuda(3, 3), k=4)
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        knn.knn(cuda(4, 3), k=4, exclude_self=True)
    with pytest.raises(ValueError, match="exclude_self"):
        knn.knn(cuda(10, 3), cuda(5, 3), k=1, exclude_self=True)
