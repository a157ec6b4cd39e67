"""The fate scan's rule as lane masks: the places where the branch-free trip, its wave-uniform choice between
the body with the two bounds on j and the body without, and the queue's portions and list batches can go wrong.  Every case runs
with fate_scan forced to 1, asserts through isx_fate_scan_launches that the scan ran, and is compared with fate_scan 0, the oracle
and -- for the rule itself -- the numpy restatement (tests/fatescan_np.py)."""
import numpy as np
import pytest

import fatescan_np as fs

pytestmark = pytest.mark.gpu

SEED = 0x5EED0001
WRAP = 2 ** 32 - 1000
CENSUS = ("launched", "exited", "counted_below_z", "absorbed", "suspended", "bin_increments", "wall_hits")
DEFAULTS = (("fate_scan", -1), ("grid_blocks", 0))


def _census(st):
    return tuple(int(getattr(st, f)) for f in CENSUS)


def _cfg(mod, **kw):
    c = mod.default_config()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _flux_three_ways(isx, orc, kw, n, first=0, opts=()):
    """isx_fluxmap with the scan (which must have run, once) == without it == the oracle: histogram and all seven census fields"""
    try:
        for k, v in opts:
            isx.set_option(k, v)
        isx.set_option("fate_scan", 1)
        k0 = isx.fate_scan_launches()
        h1, s1 = isx.fluxmap(_cfg(isx, **kw), n, SEED, first)
        k1 = isx.fate_scan_launches()
        isx.set_option("fate_scan", 0)
        h0, s0 = isx.fluxmap(_cfg(isx, **kw), n, SEED, first)
        k2 = isx.fate_scan_launches()
    finally:
        for k, v in DEFAULTS:
            isx.set_option(k, v)
    assert (k1 - k0, k2 - k1) == (1, 0), (k0, k1, k2)
    assert _census(s1) == _census(s0), (_census(s1), _census(s0))
    assert np.array_equal(h1, h0)
    oh, ost = orc.fluxmap(_cfg(orc, **kw), n, SEED, first)
    assert _census(s1) == _census(ost), (_census(s1), _census(ost))
    assert np.array_equal(h1, oh)
    assert _census(s1)[0] == n   # launched: a ray settled twice, or neither settled nor listed, shows here
    return _census(s1)


def _rule_equals_numpy(isx, orc, kw, n, first=0):
    fate, order = isx.fate_scan(_cfg(isx, **kw), n, SEED, first)
    want_fate, want_order, _ = fs.fate_scan_np(_cfg(orc, **kw), n, SEED, first)
    assert np.array_equal(fate, want_fate)
    assert np.array_equal(order, want_order)
    return fate, order


# ------------------------------------------------------------------ a bound on j at every position of a trip
BOUND_CASES = [(2, 0), (4, 0), (5, 0), (9, 0), (10, 0), (11, 0), (17, 0), (18, 0), (10, WRAP)]


@pytest.mark.parametrize("max_points,first", BOUND_CASES)
def test_bounce_limit_at_every_position_of_a_trip(isx, orc, max_points, first):
    n, kw = 20_000, {"max_points": max_points}
    fate, order = _rule_equals_numpy(isx, orc, kw, n, first)
    settled = fate == fs.ABSORBED
    assert settled.any() and (~settled).any()
    assert set(np.unique(order[~settled])) == set(range(max_points))   # left at every order 0 ... max_points - 1
    cen = _flux_three_ways(isx, orc, kw, n, first)
    assert cen[CENSUS.index("absorbed")] >= int(settled.sum())


# ------------------------------------------------------------------ J_CAP reached
@pytest.mark.parametrize("rho,first,absorbed,at_cap", [(0.999, 0, 1280, 160), (1.0, 0, 0, 521), (0.999, WRAP, None, None)])
def test_j_cap_is_reached(isx, orc, rho, first, absorbed, at_cap):
    n, kw = 4000, {"reflectance": rho, "theta_max_deg": 175.0, "max_points": 5000}
    fate, order = _rule_equals_numpy(isx, orc, kw, n, first)
    assert (order[fate == fs.TRACE] == fs.J_CAP).any() and order.max() == fs.J_CAP
    if absorbed is not None:
        assert int((fate == fs.ABSORBED).sum()) == absorbed
        assert int((order == fs.J_CAP).sum()) == at_cap
    _flux_three_ways(isx, orc, kw, n, first)


# ------------------------------------------------------------------ portions off the queue, batches onto the list
@pytest.mark.parametrize("n,first", [(1, 0), (63, 0), (64, 0), (65, 0), (255, 0), (256, 0), (257, 0), (1023, 0), (1024, 0), (1025, 0),
                                     (70_001, 0), (257, WRAP)])
def test_portion_and_batch_edges(isx, orc, n, first):
    _flux_three_ways(isx, orc, {}, n, first)


def test_one_workgroup_takes_every_portion(isx, orc):
    _flux_three_ways(isx, orc, {}, 5000, opts=(("grid_blocks", 1),))


@pytest.mark.parametrize("opts", [(), (("grid_blocks", 1),)], ids=["default_grid", "one_workgroup"])
def test_every_ray_goes_to_the_list(isx, orc, opts):
    """rho 1: no ray is settled.  On the default grid a wave's share is below a batch and goes out in the flush at the end; one
    workgroup fills and flushes its waves' batches many times"""
    cen = _flux_three_ways(isx, orc, {"reflectance": 1.0, "max_points": 64}, 70_001, opts=opts)
    assert cen[CENSUS.index("absorbed")] == 0
