"""The per-row gradient bound of tests/row_budget.py, established on the CPU: the reference alone (f32 against f64 oracle on identical
hit lists) meets the conditions on every configuration the GPU test runs, stays inside the recorded constants, and the row check
built from them notices seeded faults at least as often as the tensor metric the rest of the suite uses.

`python tests/row_budget.py` repeats the measurement and rewrites profiles/row_budget_constants.txt."""
import numpy as np
import pytest

import oracle
import row_budget as rb


@pytest.mark.parametrize("name", ["s3000_depth", "k4", "nht"])
def test_budget_mode_leaves_the_gradients_bit_identical(name):
    """The budgets are a by-product: with them the three backward entry points return what they return without.  Both builds add
    their per-hit terms as doubles in the threads' order, so two runs of ONE entry point agree to the last few bits of a double only:
    in the f64 build that is what is asserted, in the f32 build the rounded sums may differ by one f32 ulp where the two double sums
    straddle a rounding boundary.  (With the mode off the entry points run the code they ran before: every budget statement sits
    behind `if (bud)`.)"""
    pair = rb.oracle_pair(name)
    conf, scene = pair["conf"], pair["scene"]
    cfg = rb.oracle_config(conf)
    for dtype, fwd, (g, _, _) in ((np.float32, pair["f32"], pair["g32"][:3]), (np.float64, pair["f64"], pair["g64"][:3])):
        if conf.nht:
            feats = rb.nht_features(len(scene["density12"]))
            gd, gf = oracle.gut_backward_nht(cfg, scene["cam"], scene["pose_start"], scene["pose_end"], scene["density12"], feats, *scene["rays"], fwd,
                                             pair["g_fd"], None, dtype=dtype)
            second = {"features": gf}
        else:
            gd, gsph, grgb = oracle.gut_backward(cfg, scene["cam"], 3, fwd, pair["g_fd"], pair["g_dist"], dtype=dtype)
            second = {"sph": gsph, "rgb": grgb}
        assert np.abs(gd).max() > 0
        got = dict({k: gd[:, sl] for k, sl in rb.ROWS.items()}, **second)
        for k, a in got.items():
            if dtype == np.float32:   # (the double sums of two runs can straddle one f32 rounding boundary)
                assert np.all(np.abs(a.astype(np.float64) - g[k]) <= np.spacing(np.abs(g[k]).astype(np.float32))), (name, k)
            else:
                assert np.abs(a - g[k]).max() <= 1e-13 * np.abs(g[k]).max(), (name, k)


@pytest.mark.parametrize("name", [c.name for c in rb.CONFIGS])
def test_reference_stays_inside_the_recorded_constant(name):
    """Per configuration: the two oracles disagree on few enough hit counts for the scene to be usable; every row of the f32 oracle lies
    within C * eps * B_T of the f64 oracle (no row is an outlier that would need the borderline exemption of the GPU test: the scene
    itself sits on no threshold); a row without budget has no gradient; the budgets are ordered B_T >= B_1 >= |gradient| (up to the
    rounding of their double sums)."""
    pair = rb.oracle_pair(name)
    conf = pair["conf"]
    assert pair["flips"] <= rb.FLIP_CAP(pair["pixels"]), f"the oracles disagree on {pair['flips']} hit counts: change the scene's seed or scale"
    (g32, _, _, _), (g64, b1, bT, hits) = pair["g32"], pair["g64"]
    for k, r in rb.row_errors(pair).items():
        print(f"{name} {k}: rows {r.size}, largest r {r.max():.2f} (C[{conf.family}] = {rb.C[conf.family]:g})")
        assert r.size > 100, f"{k}: the configuration exercises too few rows"
        assert r.max() <= rb.C[conf.family], f"{k}: f32 against f64 oracle {r.max():.2f} eps B_T, recorded {rb.C[conf.family]:g}"
    for k in g64:
        dead = bT[k] == 0
        assert np.all(g32[k][dead] == 0) and np.all(g64[k][dead] == 0), f"{k}: a row without budget has a gradient"
        assert np.all(b1[k][dead] == 0)
        if k == "geometry":
            assert np.all(hits[~dead] >= 1) and np.all(hits <= 256 * pair["tiles_count"])   # (a hit in a masked pixel counts, with zero terms)
        # (T <= 1, so B_T >= B_1 term by term; the two are summed by separate atomics in the threads' order, and for a particle hit
        # only at T == 1 they are the same terms in two orders: equal up to the rounding of a double sum)
        assert np.all(bT[k] >= b1[k] * (1 - 1e-12)), k
        if k != "position":   # (the position's budget bounds the direction term by its norm, its elements by more than their own size)
            assert np.all(np.abs(g64[k]).max(1) <= b1[k] * (1 + 1e-12)), k
        else:
            assert np.all(np.abs(g64[k]).max(1) <= b1[k] * (1 + 1e-9) + 1e-300), k


@pytest.mark.parametrize("family", list(rb.C))
def test_recorded_constant_is_the_measured_one(family):
    """The recorded constant is the family's measurement rounded up, not a looser number: some configuration reaches 9 / 10 of it."""
    worst = max(max(float(r.max()) for r in rb.row_errors(rb.oracle_pair(c.name)).values()) for c in rb.CONFIGS if c.family == family)
    print(f"C[{family}]: measured {worst:.2f}, recorded {rb.C[family]:g}")
    assert 0.9 * rb.C[family] <= worst <= rb.C[family]


@pytest.mark.parametrize("family", list(rb.C))
def test_row_check_notices_seeded_faults(family):
    """The test tests itself: a tile entry lost by the backward alone.  No fixed detection rate is asserted (the figures are recorded in
    profiles/row_budget_constants.txt); the row check at the GPU bound must not notice fewer than the tensor metric at 1e-3."""
    counted, by_row, by_tensor = rb.seeded_faults(family)
    print(f"{family}: {counted} removals changed the victim's row; row check flagged {by_row}, tensor metric {by_tensor}")
    assert counted >= 30
    assert by_row >= by_tensor


def test_borderline_lookup_finds_the_decisions_rounding_decides():
    """The exemption's lookup, which no GPU case has needed so far: for an accept decision within 1e-3 of its threshold (searched in
    the oracle's own traces) it returns that pixel and margin, and nothing once the pixel is masked.  It reads the accept margins from
    the SH trace for the feature path too: the accept test is a function of ray and particle alone, and the feature trace
    (orc_gut_pixel_trace_nht) reports the same margins and alphas entry by entry."""
    pair = rb.oracle_pair("nht")
    conf, scene = pair["conf"], pair["scene"]
    cfg = rb.oracle_config(conf)
    lists = rb.lists_of(conf, pair["f32"])
    w, h = scene["W"], scene["H"]
    fwd = rb.trace_input(scene, lists, np.float32)
    fwd_nht = dict(fwd, nht_features=rb.nht_features(len(scene["density12"])))
    found = None
    for pix in range(0, w * h, 7):
        tr = oracle.gut_pixel_trace(cfg, scene["cam"], fwd, pix)
        if pix % 49 == 0:
            trn = oracle.gut_pixel_trace_nht(cfg, scene["cam"], fwd_nht, pix)
            assert np.array_equal(tr["idx"], trn["idx"]) and np.array_equal(tr["margin"], trn["margin"]) and np.array_equal(tr["alpha"], trn["alpha"])
        near = np.flatnonzero((np.abs(tr["margin"]) < rb.BORDERLINE) & (tr["alpha"] > 0))
        if near.size:
            found = (pix, int(tr["idx"][near[0]]), float(tr["margin"][near[0]]))
            break
    assert found is not None, "no borderline decision in the scene: choose another for this test"
    pix, particle, margin = found
    nothing_masked = np.zeros((h, w), bool)
    assert (pix, margin) in rb.borderline_entries(conf, scene, lists, particle, nothing_masked)
    masked = nothing_masked.copy()
    masked.reshape(-1)[pix] = True
    assert all(p != pix for p, _ in rb.borderline_entries(conf, scene, lists, particle, masked))
