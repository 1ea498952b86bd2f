"""GPU: the exact k-nearest-neighbour search of csrc/knn.hip against the float64 brute force of tests/knn_reference.py.

Sizes are the smallest at which each mechanism can break: K and K + 1 (everyone is everyone's neighbour; exclude_self at the limit),
63 and 65 (partial wave, second wave), 257 (one point past a box), 10 007 (40 boxes, ragged last box, pruning active); the cross-set
test adds 16 700 targets (66 boxes: a second round of the one-box-per-lane test).

The rank-wise bound.  With u = 2^-24, the selection key (dx dx + dy dy) + dz dz carries at most five fp32 roundings on top of one
another (a difference, a product, and the sums, contracted or not), so it is within a factor (1 +- 5u) of the exact squared distance of
the fp32 coordinates.  Order statistics move by at most the perturbation of the values: the exact squared distance of the point at
key-rank r is within (1 + 5u) / (1 - 5u) of the true r-th smallest.  The square root halves that to 5u, and the two final roundings
(the double arithmetic is exact at this scale; the cast to fp32 and the comparison value) add u: at most 6u in total.  8u is allowed.
Where the true r-th distance is 0 the selected point must be a coincident one: exactly 0.
"""
import ctypes as C
import importlib

import pytest
import torch

import knn_reference as ref
from test_knn_cpu import _fake_reference_modules

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
KS = (1, 2, 4, 16)
SIZES = sorted({k + d for k in KS for d in (0, 1)} | {63, 65, 257, 10_007})
KMAX = 17          # 16 neighbours and the point itself
DEV = "cuda:0"

_cache = {}


def knn_mod():
    return importlib.import_module("3dgrut_amd.knn")


def cloud(name, n):
    """(points on the CPU, points on the GPU, sorted float64 distances [n, min(n, 17)] of the self query) - computed once and shared."""
    key = (name, n)
    if key not in _cache:
        x = ref.DISTRIBUTIONS[name](n)
        _cache[key] = (x, x.to(DEV), ref.brute_force(x, k=min(n, KMAX))[0])
    return _cache[key]


def clearly_ordered(d):
    """Rows of sorted float64 distances [Q,m] whose neighbours are further apart than the fp32 key can confuse (16 u, twice the rank-wise
    bound): there the k nearest are unique as a sequence and the kernel's indices must be the brute force's."""
    return (d[:, 1:] - d[:, :-1] > 16 * U * d[:, 1:]).all(dim=1)


def check_rows(dist, index, want, points, queries=None, own=None, label=""):
    """The assertions every result must pass.  dist [Q,k] fp32, index [Q,k] int64 (both on the CPU), want [Q,k] float64."""
    q, k = dist.shape
    n = points.shape[0]
    # index consistency
    assert int(index.min()) >= 0 and int(index.max()) < n, label
    if k > 1:
        s = index.sort(dim=1).values
        assert bool((s[:, 1:] != s[:, :-1]).all()), f"{label}: an index repeats within a row"
    if own is not None:
        assert bool((index != own[:, None]).all()), f"{label}: a point is its own neighbour"
    # self-consistency, to the bit: the reported distance IS the double-recomputed distance of the reported index
    recomputed = ref.recomputed_distance(points, index, queries).float()
    assert torch.equal(dist, recomputed), f"{label}: {(dist != recomputed).sum()} distances are not those of their indices"
    # rank-wise against the float64 brute force
    err = (dist.double() - want).abs()
    worst = float((err / want.clamp_min(1e-300))[want > 0].max()) / U if bool((want > 0).any()) else 0.0
    print(f"{label}: max rank-wise error {worst:.3f} u, bit-equal rows {float((dist == want.float()).all(dim=1).float().mean()):.4f}")
    assert bool((err <= 8 * U * want).all()), f"{label}: rank-wise error {worst:.2f} u > 8 u"
    assert bool((dist[want == 0] == 0).all()), label


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(ref.DISTRIBUTIONS))
def test_self_query_against_the_float64_brute_force(name, n):
    knn = knn_mod()
    x, xg, d_all = cloud(name, n)
    own = torch.arange(n)
    for k in KS:
        for exclude in (False, True):
            if k > n - (1 if exclude else 0):
                with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
                    knn.knn(xg, k=k, exclude_self=exclude)
                continue
            label = f"{name} n={n} k={k} exclude_self={exclude}"
            dist_g, index_g = knn.knn(xg, k=k, exclude_self=exclude, return_indices=True)
            again = knn.knn(xg, k=k, exclude_self=exclude, return_indices=True)
            assert dist_g.shape == (n, k) and dist_g.dtype == torch.float32 and index_g.dtype == torch.int64
            assert torch.equal(dist_g, again[0]) and torch.equal(index_g, again[1]), f"{label}: two calls differ"
            assert torch.equal(knn.knn(xg, k=k, exclude_self=exclude), dist_g)         # without the index output
            dist, index = dist_g.cpu(), index_g.cpu()
            # the query itself is at distance 0 and the smallest of every row, so excluding it (by index) drops one leading zero
            want = d_all[:, 1:k + 1] if exclude else d_all[:, :k]
            check_rows(dist, index, want, x, own=own if exclude else None, label=label)
            if not exclude:
                assert bool((dist[:, 0] == 0).all()), label
            if name in ("uniform", "clustered"):
                assert float((dist == want.float()).all(dim=1).float().mean()) >= 0.99, f"{label}: a systematically different neighbour"


@pytest.mark.parametrize("name", ["uniform", "clustered", "two_clusters"])
def test_the_models_initial_scale_formula(name):
    """model.py:732-733: sqrt(mean of the squared distances to the three nearest other points), evaluated in float64 on the fp32
    distances the kernel reports against the same on the brute force's: each distance is within 6 u (module docstring), so is the root
    of the mean of their squares; 8 u allowed."""
    knn = knn_mod()
    x, xg, d_all = cloud(name, 10_007)
    got = knn.k_nearest_neighbors(xg, 4)
    assert got.dtype == xg.dtype and got.device == xg.device and got.shape == (10_007, 4)
    mine = (got.cpu().double()[:, 1:] ** 2).mean(dim=-1).sqrt()
    want = (d_all[:, 1:4] ** 2).mean(dim=-1).sqrt()
    assert bool(((mine - want).abs() <= 8 * U * want).all())
    assert bool((mine[want == 0] == 0).all())


@pytest.mark.parametrize("p", [1, 7, 300, 5_000, 16_700])
def test_cross_set_queries(p):
    knn = knn_mod()
    g = torch.Generator().manual_seed(100 + p)
    targets = torch.rand((p, 3), generator=g) * 4.0 - 2.0
    q = 2_049
    queries = torch.rand((q, 3), generator=g) * 4.0 - 2.0
    queries[q // 2:] = queries[q // 2:] * 3.0 + torch.tensor([9.0, -1.0, 0.5])       # half of them outside the targets' bounding box
    tg, qg = targets.to(DEV), queries.to(DEV)
    for k in (1, 4):
        if k > p:
            with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
                knn.knn(tg, qg, k=k)
            continue
        label = f"cross P={p} k={k}"
        want, want_index = ref.brute_force(targets, queries, k=k)
        dist_g, index_g = knn.knn(tg, qg, k=k, return_indices=True)
        again = knn.knn(tg, qg, k=k, return_indices=True)
        assert dist_g.shape == (q, k) and torch.equal(dist_g, again[0]) and torch.equal(index_g, again[1]), f"{label}: two calls differ"
        check_rows(dist_g.cpu(), index_g.cpu(), want, targets, queries, label=label)
        if k == 1:
            # the observer call of model.py:728: random targets, so the nearest one is unique (and not a near-tie for all but a few
            # queries) and the index must be the brute force's
            unique = clearly_ordered(ref.brute_force(targets, queries, k=2)[0]) if p >= 2 else torch.ones(q, dtype=torch.bool)
            assert float(unique.float().mean()) > 0.99
            assert torch.equal(index_g.cpu()[unique], want_index[unique]), label
            expect = torch.linalg.norm(qg - tg[want_index[:, 0].to(DEV), :], dim=-1)
            assert torch.equal(knn.nearest_neighbor_dist(qg, tg)[unique.to(DEV)], expect[unique.to(DEV)]), label


def test_nearest_other_point_surfaces_and_gradient():
    knn = knn_mod()
    x, xg, d_all = cloud("uniform", 10_007)
    want, want_index = ref.brute_force(x, k=3, exclude_self=True)
    unique = clearly_ordered(d_all[:, :5])                                       # no ties in this cloud, and hardly a near-tie
    assert float(unique.float().mean()) > 0.99
    index = knn.nearest_neighbors(xg, k=4)
    assert index.dtype == torch.int64 and index.shape == (10_007, 3) and torch.equal(index.cpu()[unique], want_index[unique])
    leaf = xg.clone().requires_grad_(True)
    dist = knn.nearest_neighbor_dist(leaf)
    expect = torch.linalg.norm(xg - xg[want_index[:, 0].to(DEV), :], dim=-1)
    assert torch.equal(dist.detach()[unique.to(DEV)], expect[unique.to(DEV)])
    dist.sum().backward()                                                        # the reference's expression: differentiable
    assert leaf.grad is not None and bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().sum()) > 0


def test_wrapper_behaviour():
    knn = knn_mod()
    x, xg, d_all = cloud("uniform", 10_007)
    base = knn.knn(xg, k=4)
    for bad in (float("nan"), float("inf"), float("-inf")):
        y = xg.clone()
        y[5_000, 1] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            knn.knn(y, k=4)
        with pytest.raises(ValueError, match="NaN or infinity"):
            knn.knn(xg, y[4_000:6_000], k=1)
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        knn.knn(xg[:3], k=4)
    x4 = torch.zeros((10_007, 4), device=DEV)
    x4[:, :3] = xg
    view = x4[:, :3]
    assert not view.is_contiguous() and torch.equal(knn.knn(view, k=4), base)
    assert torch.equal(knn.knn(xg, x4[:100, :3], k=4), base[:100])                # (every point is its own nearest: the same rows)
    # the order of the rows only matters for ties, and this cloud has none
    perm = torch.randperm(10_007, generator=torch.Generator().manual_seed(7)).to(DEV)
    d_perm, i_perm = knn.knn(xg[perm], k=4, return_indices=True)
    assert torch.equal(d_perm, base[perm])
    assert torch.equal(perm[i_perm], knn.knn(xg, k=4, return_indices=True)[1][perm])
    assert knn.knn(xg, xg[:0], k=2).shape == (0, 2)


@pytest.mark.parametrize("cross", [False, True])
def test_nothing_relies_on_zeroed_scratch(cross):
    abi = importlib.import_module("3dgrut_amd._abi")
    lib = abi.load_library()
    x, xg, _ = cloud("clustered", 10_007)
    queries = (cloud("uniform", 257)[1] - 5.0) * 3.0 if cross else None
    p, q, k = 10_007, (257 if cross else 10_007), 4
    nbytes = int(lib.grut_knn_scratch_bytes(p, 257 if cross else 0))
    results = []
    for fill in (0x00, 0xFF, 0x7F):
        scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        dist = torch.full((q, k), -1.0, device=DEV)
        index = torch.full((q, k), -7, dtype=torch.int32, device=DEV)
        nonfinite = torch.full((1,), 123, dtype=torch.int32, device=DEV)
        abi.check(lib.grut_knn(C.c_void_p(torch.cuda.current_stream().cuda_stream), p, C.c_void_p(xg.data_ptr()), q if cross else 0,
                               C.c_void_p(queries.data_ptr() if cross else None), k, 0, C.c_void_p(dist.data_ptr()),
                               C.c_void_p(index.data_ptr()), C.c_void_p(scratch.data_ptr()), nbytes, C.c_void_p(nonfinite.data_ptr())),
                  "grut_knn")
        torch.cuda.synchronize()
        assert int(nonfinite.item()) == 0
        results.append((dist.cpu(), index.cpu()))
    for d, i in results[1:]:
        assert torch.equal(d, results[0][0]) and torch.equal(i, results[0][1])
    assert bool((results[0][1] >= 0).all())


def test_hook_sends_cuda_clouds_to_the_kernel(monkeypatch):
    knn = knn_mod()
    calls = []
    geometry, model = _fake_reference_modules(monkeypatch, calls)
    knn.install_gpu_knn()
    x, xg, d_all = cloud("uniform", 257)
    before = knn.stats["calls"]
    got = model.k_nearest_neighbors(xg, 4)
    assert got.is_cuda and torch.equal(got, knn.knn(xg, k=4))
    assert torch.equal(geometry.nearest_neighbors(xg, 3), knn.nearest_neighbors(xg, 3))
    assert torch.equal(model.nearest_neighbor_dist_cpuKD(xg), knn.nearest_neighbor_dist(xg))
    assert torch.equal(model.nearest_neighbor_dist_cpuKD(xg, xg[:9] + 1.0), knn.nearest_neighbor_dist(xg, xg[:9] + 1.0))
    assert calls == [] and knn.stats["calls"] == before + 8
    model.k_nearest_neighbors(x, 4)                                              # the CPU cloud still goes to the original
    assert calls == [("k_nearest_neighbors", 4)]
