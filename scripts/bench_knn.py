#!/usr/bin/env python
"""The initialisation's nearest-neighbour searches on the GPU against the host functions they replace (threedgrut/model/geometry.py).

  k_nearest_neighbors(x, 4)        the Gaussians' initial size (model.py:732); host: sklearn.neighbors.NearestNeighbors, as geometry.py:42-49
  nearest_neighbor_dist(x)         distance to the nearest other point (model.py:588); host: sklearn.neighbors.KDTree with k = 2, the self
                                   column masked out and the distance recomputed in torch, as geometry.py:76-117

at 100 k, 1 M and 4 M points of two distributions: uniform in a 10-cube, and clustered (30 Gaussian blobs whose centres have spread 5,
sigma = 0.01 of that spread).  GPU: the public Python function, i.e. including its scratch allocation and its one host read of the
non-finite count; two warm-up calls, then `--repeats` calls timed one by one with device events, median and minimum reported.  Host: the
function being replaced, once, on this box's CPUs with at most 16 threads, when sklearn imports here (`reference: unavailable`
otherwise); skipped at 4 M.  One JSON line per case.

    python scripts/bench_knn.py [--sizes 100000,1000000,4000000] [--repeats 7] [--no-host] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
knn = importlib.import_module("3dgrut_amd.knn")

HOST_MAX_POINTS = 1_000_000


def make_points(dist, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dist == "uniform":
        return torch.rand((n, 3), generator=g) * 10.0
    spread = 5.0
    centres = torch.randn((30, 3), generator=g) * spread
    return centres[torch.randint(0, 30, (n,), generator=g)] + torch.randn((n, 3), generator=g) * (0.01 * spread)


def host_functions():
    """The two host functions as the reference has them, or None without sklearn."""
    try:
        import numpy as np
        import sklearn.neighbors
    except ImportError:
        return None

    def k_nearest_neighbors(x, K=4):
        x_np = x.cpu().numpy()
        distances, _ = sklearn.neighbors.NearestNeighbors(n_neighbors=K, metric="euclidean").fit(x_np).kneighbors(x_np)
        return torch.from_numpy(distances).to(x)

    def nearest_neighbor_dist(x):
        x_np = x.cpu().numpy()
        _, neighbors = sklearn.neighbors.KDTree(x_np).query(x_np, k=2)
        mask = neighbors != np.arange(neighbors.shape[0])[:, None]
        mask[mask.sum(axis=1) == 2, -1] = False
        index = torch.from_numpy(neighbors[mask]).to(x.device)
        return torch.linalg.norm(x - x[index, :], dim=-1)

    return {"k_nearest_neighbors": k_nearest_neighbors, "nearest_neighbor_dist": nearest_neighbor_dist}


def time_gpu(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,4000000")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn.py measures on the GPU; none is available")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    host = None if args.no_host else host_functions()
    if host is None:
        print("reference: unavailable", flush=True)
    gpu = {"k_nearest_neighbors": lambda x: knn.k_nearest_neighbors(x, 4), "nearest_neighbor_dist": lambda x: knn.nearest_neighbor_dist(x)}
    lines = []
    for n in [int(s) for s in args.sizes.split(",")]:
        for dist in ("uniform", "clustered"):
            x = make_points(dist, n)
            xg = x.cuda()
            for name, fn in gpu.items():
                med, lo, hi = time_gpu(lambda: fn(xg), args.repeats)
                entry = {"function": name, "points": n, "distribution": dist, "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
                         "gpu_ms_median": round(med, 3), "gpu_ms_min": round(lo, 3), "gpu_ms_max": round(hi, 3), "host_s": None, "speedup": None}
                if host is not None and n <= HOST_MAX_POINTS:
                    t0 = time.perf_counter()
                    want = host[name](x)
                    entry["host_s"] = round(time.perf_counter() - t0, 3)
                    entry["speedup"] = round(entry["host_s"] * 1e3 / med, 1)
                    got = fn(xg).cpu()
                    entry["rows_bit_equal_to_host"] = round(float((got == want).reshape(n, -1).all(dim=1).float().mean()), 6)
                line = json.dumps({"knn": entry})
                print(line, flush=True)
                lines.append(line)
            del xg
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
