"""Exact k nearest neighbours in 3-D on the MI355X: what the reference's initialisation takes from `sklearn.neighbors`
(threedgrut/model/geometry.py), backed by csrc/knn.hip.  There is no CPU fallback in this module.

    knn(points, queries=None, k=4, exclude_self=False, return_indices=False)   the validated wrapper of grut_knn
    k_nearest_neighbors(x, K=4)                   geometry.py:42: [N,K] distances in x's dtype, column 0 the point itself (0)
    nearest_neighbors(pts_src, k=2)               geometry.py:52: [N,k-1] int64 indices of the nearest OTHER points
    nearest_neighbor_dist(pts_src, pts_target=None)   geometry.py:76 (nearest_neighbor_dist_cpuKD): differentiable distance to the
                                                  nearest other point, or to the nearest target
    install_gpu_knn()    opt-in: rebinds the three functions on threedgrut.model.geometry and the two names threedgrut.model.model imported

Selection is by the fp32 squared distance with ties broken by the lower index; the reported distance is recomputed in double from the
fp32 coordinates and rounded once, which is the number sklearn's float64 search returns after the reference's cast back.  The result
is bitwise reproducible and does not depend on the order of the rows beyond the tie rule.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _abi

MAX_K = 16
MAX_POINTS = 2 ** 31 - 1
stats = {"calls": 0}   # plain counter of kernel calls (tests: the hook fell through / did not)


def _check_cloud(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor (there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype})")
    if t.dim() != 2 or t.shape[1] != 3:
        raise RuntimeError(f"{name} must be [N, 3] (got {list(t.shape)})")
    if t.shape[0] > MAX_POINTS:
        raise RuntimeError(f"{name} must have fewer than 2^31 rows (got {t.shape[0]})")


def knn(points: torch.Tensor, queries: torch.Tensor | None = None, k: int = 4, exclude_self: bool = False, return_indices: bool = False):
    """The k nearest `points` of every query, ascending: [Q,k] fp32 distances, and with return_indices the [Q,k] int64 indices too.
    points: fp32 CUDA [P,3]; queries: fp32 CUDA [Q,3] on the same device, or None for the points themselves.  exclude_self (only without
    queries): a point is not its own neighbour, by INDEX - coincident other points still are.  1 <= k <= 16.
    Raises ValueError when k exceeds the available points or when any coordinate is NaN or infinite (both as sklearn does); the second
    costs the call's one host read.  Non-contiguous inputs are made contiguous.  Nothing here is differentiable."""
    _check_cloud(points, "points")
    if queries is not None:
        _check_cloud(queries, "queries")
        if queries.device != points.device:
            raise RuntimeError("points and queries must be on the same device")
        if exclude_self:
            raise ValueError("exclude_self only applies without queries")
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}] (got {k})")
    p = int(points.shape[0])
    available = p - (1 if exclude_self else 0)
    if k > available:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {max(available, 0)}")
    q = p if queries is None else int(queries.shape[0])
    dev = points.device
    dist = torch.empty((q, k), dtype=torch.float32, device=dev)
    index = torch.empty((q, k), dtype=torch.int32, device=dev) if return_indices else None
    if q:
        lib = _abi.load_library()
        points = points.detach().contiguous()
        queries = None if queries is None else queries.detach().contiguous()
        nbytes = int(lib.grut_knn_scratch_bytes(p, 0 if queries is None else q))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        nonfinite = torch.empty(1, dtype=torch.int32, device=dev)
        null = C.c_void_p(None)
        stats["calls"] += 1
        with torch.cuda.device(dev):
            _abi.check(lib.grut_knn(
                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), p, C.c_void_p(points.data_ptr()), 0 if queries is None else q,
                null if queries is None else C.c_void_p(queries.data_ptr()), k, 1 if exclude_self else 0, C.c_void_p(dist.data_ptr()),
                null if index is None else C.c_void_p(index.data_ptr()), C.c_void_p(scratch.data_ptr()), nbytes,
                C.c_void_p(nonfinite.data_ptr())), "grut_knn")
        if int(nonfinite.item()) != 0:
            raise ValueError("Input contains NaN or infinity.")
    return (dist, index.long()) if return_indices else dist


def k_nearest_neighbors(x: torch.Tensor, K: int = 4) -> torch.Tensor:
    """geometry.py:42-49: [N,K] distances to the K nearest points of x, itself included (column 0 is 0), in x's dtype and on its device."""
    return knn(x, k=K).to(x)


def nearest_neighbors(pts_src: torch.Tensor, k: int = 2) -> torch.Tensor:
    """geometry.py:52-73: [N,k-1] int64 indices of the nearest other points (the reference queries k and masks the point itself out)."""
    return knn(pts_src, k=int(k) - 1, exclude_self=True, return_indices=True)[1]


def nearest_neighbor_dist(pts_src: torch.Tensor, pts_target: torch.Tensor | None = None) -> torch.Tensor:
    """geometry.py:76-117 (nearest_neighbor_dist_cpuKD): with one argument the distance of every point to the nearest OTHER point of the
    set, with two the distance of every source point to the nearest target.  Only the index comes from the kernel; the distance is the
    reference's own torch expression, so it is differentiable and bit-identical whenever the index agrees."""
    if pts_target is None:
        pts_target = pts_src
        idx = knn(pts_src, k=1, exclude_self=True, return_indices=True)[1][:, 0]
    else:
        idx = knn(pts_target, pts_src, k=1, return_indices=True)[1][:, 0]
    return torch.linalg.norm(pts_src - pts_target[idx, :], dim=-1)


def _on_gpu(t, k=1) -> bool:
    """The preconditions of the hook's GPU path; anything else goes to the reference's own function."""
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 3
            and 0 < t.shape[0] <= MAX_POINTS and isinstance(k, int) and 1 <= k <= MAX_K)


def install_gpu_knn():
    """Opt-in: rebind k_nearest_neighbors, nearest_neighbors and nearest_neighbor_dist_cpuKD on threedgrut.model.geometry, and the two
    names threedgrut.model.model imported from it (model.py:33-34, used at :588, :728 and :732), to functions that run the search on the
    GPU.  Each replacement calls the function it replaced whenever a precondition does not hold - an input that is not an fp32 CUDA
    [N,3] tensor with 0 < N < 2^31 rows, K > 16 (k - 1 > 16 for nearest_neighbors), or two clouds on different devices - so CPU tensors
    behave exactly as before.  Non-contiguous inputs are made contiguous.  Call it before the model is initialised.  Returns the dict of
    the replaced (original) functions by name; calling it again changes nothing and returns the same dict."""
    geometry = __import__("threedgrut.model.geometry", fromlist=["k_nearest_neighbors"])
    if getattr(geometry.k_nearest_neighbors, "_grut_gpu_knn", False):
        return geometry.k_nearest_neighbors._grut_originals
    model = __import__("threedgrut.model.model", fromlist=["MixtureOfGaussians"])
    originals = {"k_nearest_neighbors": geometry.k_nearest_neighbors, "nearest_neighbors": geometry.nearest_neighbors,
                 "nearest_neighbor_dist_cpuKD": geometry.nearest_neighbor_dist_cpuKD}

    def gpu_k_nearest_neighbors(x, K=4):
        if not _on_gpu(x, K):
            return originals["k_nearest_neighbors"](x, K)
        return k_nearest_neighbors(x, K)

    def gpu_nearest_neighbors(pts_src, k=2):
        if not (isinstance(k, int) and _on_gpu(pts_src, k - 1)):
            return originals["nearest_neighbors"](pts_src, k)
        return nearest_neighbors(pts_src, k)

    def gpu_nearest_neighbor_dist(pts_src, pts_target=None):
        if not _on_gpu(pts_src) or (pts_target is not None and not (_on_gpu(pts_target) and pts_target.device == pts_src.device)):
            return originals["nearest_neighbor_dist_cpuKD"](pts_src, pts_target)
        return nearest_neighbor_dist(pts_src, pts_target)

    replacements = {"k_nearest_neighbors": gpu_k_nearest_neighbors, "nearest_neighbors": gpu_nearest_neighbors,
                    "nearest_neighbor_dist_cpuKD": gpu_nearest_neighbor_dist}
    for name, fn in replacements.items():
        fn.__name__ = fn.__qualname__ = name
        fn.__doc__ = originals[name].__doc__
        fn._grut_gpu_knn = True
        fn._grut_originals = originals
        setattr(geometry, name, fn)
    for name in ("k_nearest_neighbors", "nearest_neighbor_dist_cpuKD"):
        setattr(model, name, replacements[name])
    return originals
