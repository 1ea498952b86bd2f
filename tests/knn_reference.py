"""Float64 brute-force restatement of the nearest-neighbour search, in torch on the CPU: what tests/test_knn_gpu.py trusts and what
tests/test_knn_cpu.py pins to the reference's sklearn functions.  Chunked over the queries so that a 10 k x 10 k problem never holds
more than about 200 MB of distances.  Also the six input distributions the two test files share."""
import torch

CHUNK_ELEMS = 4_000_000   # float64 squared distances held at once (32 MB; the temporaries of a chunk are about six times that)


def _sq_dist(q, p):
    """[Q,P] float64 squared distances, (dx^2 + dy^2) + dz^2 with separately rounded products and sums."""
    d = q[:, None, :] - p[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _k_smallest(d2, k):
    """The k smallest entries of every row of d2 as (values, indices), ascending, equal values in the order of their indices - what a
    stable full sort gives, without sorting the rows: everything below the k-th value, then the lowest indices among its equals."""
    kth = torch.topk(d2, k, dim=1, largest=False).values.max(dim=1, keepdim=True).values
    below, equal = d2 < kth, d2 == kth
    need = k - below.sum(dim=1, keepdim=True)
    chosen = below | (equal & (torch.cumsum(equal, dim=1) <= need))
    index = chosen.nonzero()[:, 1].reshape(d2.shape[0], k)          # exactly k per row, in index order
    order = torch.sort(torch.gather(d2, 1, index), dim=1, stable=True)
    return order.values, torch.gather(index, 1, order.indices)


def brute_force(points, queries=None, k=4, exclude_self=False):
    """-> (dist [Q,k] float64 ascending, index [Q,k] int64).  Selection by the float64 squared distance, ties to the lower index;
    exclude_self removes the query's own index (self queries only)."""
    p = points.detach().cpu().double()
    q = p if queries is None else queries.detach().cpu().double()
    assert not (exclude_self and queries is not None)
    n_q, n_p = q.shape[0], p.shape[0]
    dist = torch.empty((n_q, k), dtype=torch.float64)
    index = torch.empty((n_q, k), dtype=torch.int64)
    rows = max(1, CHUNK_ELEMS // max(n_p, 1))
    for s in range(0, n_q, rows):
        e = min(n_q, s + rows)
        d2 = _sq_dist(q[s:e], p)
        if exclude_self:
            d2[torch.arange(e - s), torch.arange(s, e)] = float("inf")
        values, index[s:e] = _k_smallest(d2, k)
        dist[s:e] = values.sqrt()
    return dist, index


def recomputed_distance(points, index, queries=None):
    """float64 distance of every (query row, points[index]) pair from the fp32 coordinates: differences, squares and sum in double, one
    square root.  Rounded to fp32 it is the number the kernel must report for the neighbour it selected."""
    p = points.detach().cpu().double()
    q = p if queries is None else queries.detach().cpu().double()
    d = q[:, None, :] - p[index.cpu()]
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).sqrt()


# ---- input distributions (fp32 [n,3], |x| <= 1e4, distinct points at least 1e-6 apart) ----------------------------------------------
def uniform(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, 3), generator=g) * 10.0


def clustered(n, seed=1):
    """30 blobs at spread 5, sigma 0.01; 50 rows duplicated once and one point repeated 20 times (as far as n allows)."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn((30, 3), generator=g) * 5.0
    x = centres[torch.randint(0, 30, (n,), generator=g)] + torch.randn((n, 3), generator=g) * 0.01
    dup = min(50, n // 4)
    x[2 * dup:3 * dup] = x[:dup]
    rep = min(20, n // 4)
    x[n - rep:] = x[n // 2]
    return x.contiguous()


def lattice(n, seed=2):
    """the first n points of a cubic lattice of spacing 0.1 in a shuffled order: massive exact ties"""
    side = 1
    while side ** 3 < n:
        side += 1
    a = torch.arange(side, dtype=torch.float32) * 0.1
    x = torch.stack(torch.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    g = torch.Generator().manual_seed(seed)
    return x[torch.randperm(x.shape[0], generator=g)[:n]].contiguous()


def collinear(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros((n, 3))
    x[:, 0] = torch.rand((n,), generator=g) * 100.0
    x[:, 1], x[:, 2] = 2.5, -7.0
    return x


def identical(n, seed=4):
    return torch.tensor([[1.25, -3.5, 1000.0]]).repeat(n, 1)


def two_clusters_and_outlier(n, seed=5):
    """two tight clusters 1e4 apart and one outlier: the quantisation puts nearly everything into one cell"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, 3), generator=g) * 0.01
    x[n // 2:, 0] += 1.0e4
    if n >= 3:
        x[n // 3] = torch.tensor([5.0e3, 5.0e3, -5.0e3])
    return x.contiguous()


DISTRIBUTIONS = {"uniform": uniform, "clustered": clustered, "lattice": lattice, "collinear": collinear, "identical": identical,
                 "two_clusters": two_clusters_and_outlier}
