"""CPU: the pruning slack of the custom primitives (csrc/grt_kernels.hip: grt_proxy_kernel) is conservative - as mathematics, in float64.

render.primitive_type = custom offers a particle to every ray that touches its WORLD box and reports the distance t* of maximum response,
the minimiser of |W (o + t d - mu)| with W = diag(1 / kscl) R^T (intersectCustomParticle, gaussianParticles.cuh:407-441).  The tree walk
prunes a node when `box entry - slack > k-th best distance so far`: sound only if t* >= entry - slack for every ray through the box.  The
bounds in use: slack = kmax |s|, s_i = sum_j |W_ij| h_j (h = the box's half extents) for every ray, and 3 max scl + half diagonal for the
candidates the program can accept (the kernel takes the smaller); the Euclidean half diagonal that preceded them fails
for anisotropic particles - shown here too, so that the test would have caught the defect the 1 M-particle parity run found in round 5."""
import numpy as np


def _rot(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def test_custom_primitive_slack_bounds_the_reported_distance_for_every_ray_through_the_world_box():
    rng = np.random.default_rng(11)
    worst_new, worst_old, worst_acc, n_rays, n_accepted = 0.0, 0.0, 0.0, 0, 0
    for _ in range(400):
        R = _rot(rng.normal(size=4))
        k = np.exp(rng.uniform(np.log(0.01), np.log(1.0), size=3))          # kscl: anisotropy up to 100
        mu = rng.normal(size=3)
        W = np.diag(1.0 / k) @ R.T
        h = np.abs(R) @ k                                                   # half extents of the world box of the oriented box (particlePrimitives.cu:498-541)
        slack_new = k.max() * np.linalg.norm(np.abs(W) @ h)
        slack_old = np.linalg.norm(h)
        for _ in range(200):
            p = mu + rng.uniform(-1, 1, size=3) * h                         # a point of the box the ray passes through
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            o = p - rng.uniform(0.5, 5.0) * d
            j = 1.0 / d
            a0, a1 = (mu - h - o) * j, (mu + h - o) * j
            tnear, tfar = np.minimum(a0, a1).max(), np.maximum(a0, a1).min()
            assert tnear <= tfar + 1e-12
            po, pd = W @ (o - mu), W @ d
            t_star = -(po @ pd) / (pd @ pd)
            worst_new = max(worst_new, (tnear - t_star) / slack_new, (t_star - tfar) / slack_new)
            worst_old = max(worst_old, (tnear - t_star) / slack_old)
            # the second bound holds for the candidates the program can ACCEPT (|W (x* - mu)| ks < 3; the kernel uses the smaller of the two)
            for ks in (1.5, 3.0, 4.5):                                       # kernelScale of dense ... faint particles (kscl = ks * scl)
                slack_acc = 3.0 * k.max() / ks + np.linalg.norm(h)
                if np.linalg.norm(po + t_star * pd) * ks < 3.0:
                    worst_acc = max(worst_acc, (tnear - t_star) / slack_acc, (t_star - tfar) / slack_acc)
                    n_accepted += 1
            n_rays += 1
    assert worst_new <= 1.0, f"t* precedes the box entry by {worst_new:.3f} x the slack"
    assert worst_acc <= 1.0 and n_accepted > 5000, (worst_acc, n_accepted)
    assert worst_old > 1.5, "the Euclidean half diagonal was expected to fail on anisotropic particles"   # (the defect this test guards against)
    assert n_rays == 80000


def test_custom_primitive_bounds_hold_for_the_unsigned_distance_of_the_slang_pipeline():
    """render.pipeline_type referenceSlang (and neural harmonic features): the candidate's distance is |t*| (RayW::absdist; particleDensityHitCustom,
    gaussianParticles.slang:489-523), and the ray origin may lie inside or beyond the world box, so t* < 0 occurs.  What the kernels rely on:
      tree walk - a node is pruned when `max(box entry, 0) - slack > k-th best distance`: needs |t*| >= entry - slack for every ray whose t >= 0 part
        meets the box.  From the signed bound t_p - slack <= t* <= t_p + slack for every point p = o + t_p d of the ray in the box: t* >= 0 is the
        signed case; t* < 0 gives entry <= t_p <= t* + slack < slack + |t*|.
      packet lists (bin_particle, load_list_entry) - an ACCEPTED hit has |x* - mu| < Rt = 3 kmax / ks, and |t*| |d| = |x* - o| is a Euclidean length:
        by the triangle inequality |v| - Rt <= |t*| |d| <= |v| + Rt with v = mu - o, whatever the sign of t*.  The key max(|v| - Rt, 0) / dmax
        and the upper bound (|v| + Rt) / dmin therefore hold unchanged (dmin <= |d| <= dmax).
    Checked here as mathematics in float64, on rays of which a large share has t* < 0, with unnormalised directions."""
    rng = np.random.default_rng(12)
    worst_walk, worst_lo, worst_hi, n_neg, n_neg_accepted, n_rays = 0.0, 0.0, 0.0, 0, 0, 0
    for _ in range(400):
        R = _rot(rng.normal(size=4))
        k = np.exp(rng.uniform(np.log(0.01), np.log(1.0), size=3))
        mu = rng.normal(size=3)
        W = np.diag(1.0 / k) @ R.T
        h = np.abs(R) @ k
        for ks in (1.5, 3.0, 4.5):
            slack = min(k.max() * np.linalg.norm(np.abs(W) @ h), 3.0 * k.max() / ks + np.linalg.norm(h))   # grt_proxy_kernel takes the smaller
            Rt = 3.0 * k.max() / ks
            for _ in range(70):
                p = mu + rng.uniform(-1, 1, size=3) * h                     # a point of the box the ray passes through, at t_p >= 0
                d = rng.normal(size=3)
                d *= rng.uniform(0.4, 2.5) / np.linalg.norm(d)
                o = p - rng.uniform(0.0, 0.6) * np.linalg.norm(h) * d / np.linalg.norm(d)   # origins inside the box or just in front of it
                j = 1.0 / d
                a0, a1 = (mu - h - o) * j, (mu + h - o) * j
                tnear, tfar = np.minimum(a0, a1).max(), np.maximum(a0, a1).min()
                assert tnear <= tfar + 1e-12 and tfar >= -1e-12
                po, pd = W @ (o - mu), W @ d
                t_star = -(po @ pd) / (pd @ pd)
                n_rays += 1
                n_neg += t_star < 0
                if not np.linalg.norm(po + t_star * pd) * ks < 3.0:          # (the program rejects it: pruning may lose it)
                    continue
                n_neg_accepted += t_star < 0
                dist = abs(t_star)
                # (the slack is a world length for unit directions: the kernels' rays are what the test scales by |d|)
                worst_walk = max(worst_walk, (max(tnear, 0.0) * np.linalg.norm(d) - dist * np.linalg.norm(d)) / slack)
                v = np.linalg.norm(mu - o)
                for dmin, dmax in ((np.linalg.norm(d), np.linalg.norm(d)), (0.4, 2.5)):
                    worst_lo = max(worst_lo, max(v - Rt, 0.0) / dmax - dist)
                    worst_hi = max(worst_hi, dist - (v + Rt) / dmin)
    assert n_rays == 84000 and n_neg > 0.2 * n_rays and n_neg_accepted > 2000, (n_rays, n_neg, n_neg_accepted)
    assert worst_walk <= 1.0, f"|t*| precedes the box entry by {worst_walk:.3f} x the slack"
    assert worst_lo <= 1e-12 and worst_hi <= 1e-12, (worst_lo, worst_hi)
