"""isx_exit_lines_kernel without the generic search: the box point comes from the three slab quotients, the
bounds from reciprocal-root estimates rounded up.  The accept rule is the one tests/exitscan_np.py states -- no test dropped, none
loosened -- and where the trimmed arithmetic is stressed (largest j and eps, the geometry scaled, ray indices past 2^32) histogram and
census with the path are those without it, and the oracle's.  Tier 1 of the binning kernel takes one bound per region, the largest
eps of the region's lines, from the region's word: checked where a wave closes more than one region and with every eps scaled."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED0001
CENSUS = ("launched", "exited", "counted_below_z", "absorbed", "suspended", "bin_increments", "wall_hits")


def _census(st):
    return tuple(int(getattr(st, f)) for f in CENSUS)


def _scaled(cfg, s):
    c = cfg.copy()
    c.r_in *= s; c.r_out *= s; c.box_half *= s
    c.det_diameter *= s; c.det_distance *= s; c.exit_port_z *= s
    for k in range(3):
        c.src[k] *= s
    return c


def _mod(cfg, **kw):
    c = cfg.copy()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _on_off(isx, cfg, n, first=0, scale=1):
    """-> (hist, census, (accepted, list B, redo entries)) with exit_scan 1, after asserting that exit_scan 0 gives the same"""
    try:
        isx.set_option("exit_eps_scale", scale)
        isx.set_option("exit_scan", 1)
        k0 = isx.exit_scan_counts()
        h1, s1 = isx.fluxmap(cfg, n, SEED, first)
        k1 = isx.exit_scan_counts()
        isx.set_option("exit_scan", 0)
        h0, s0 = isx.fluxmap(cfg, n, SEED, first)
        assert isx.exit_scan_counts() == k1
    finally:
        isx.set_option("exit_scan", -1)
        isx.set_option("exit_eps_scale", 1)
    assert np.array_equal(h1, h0)
    assert _census(s1) == _census(s0)
    return h1, _census(s1), tuple(b - a for a, b in zip(k0, k1))


def test_accept_rule_is_the_cpu_restatements(isx):
    """Default configuration, 400 000 rays from ray 0.  tests/exitscan_np.py (exit_lines_np, which takes the box point from the slab
    quotients and runs no search) lists 172 173 rays and accepts 163 011; of the 9 162 it rejects 6 975 clip the rim with or
    without the margins, 1 992 fail the word rule and 195 the chord and direction floors.  A dropped or loosened accept test moves
    the first number up, a tightened one down."""
    try:
        isx.set_option("exit_scan", 1)
        k0 = isx.exit_scan_counts()
        isx.fluxmap(isx.default_config(), 400_000, SEED, 0)
        k1 = isx.exit_scan_counts()
    finally:
        isx.set_option("exit_scan", -1)
    d = tuple(b - a for a, b in zip(k0, k1))
    print(f"accepted {d[0]}, list B {d[1]}, redo entries {d[2]}")
    assert d[:2] == (163_011, 9_162), d


STRESS = {
    "long_rays": (lambda c: _mod(c, reflectance=0.999, theta_max_deg=175.0, max_points=5000), 4000, 0),   # largest j, largest eps
    "scale100": (lambda c: _scaled(c, 100.0), 20_000, 0),      # the bounds' scaling
    "scale0.01": (lambda c: _scaled(c, 0.01), 20_000, 0),
    "first_wrap": (lambda c: c, 20_000, 2 ** 32 - 1000),
}


@pytest.mark.parametrize("name", list(STRESS))
def test_on_is_off_is_the_oracle_where_the_bounds_are_stressed(isx, orc, name):
    make, n, first = STRESS[name]
    h, cen, d = _on_off(isx, make(isx.default_config()), n, first)
    print(f"{name}: accepted {d[0]}, list B {d[1]}, redo entries {d[2]}")
    assert d[0] > 0.5 * cen[CENSUS.index("counted_below_z")], (d, cen)
    oh, ost = orc.fluxmap(make(orc.default_config()), n, SEED, first)
    assert np.array_equal(h, oh)
    assert cen == _census(ost)


@pytest.mark.parametrize("scale", [1, 1_000_000])
def test_a_wave_that_closes_two_regions_gives_each_its_own_bound(isx, orc, scale):
    """The exit kernel writes a region's largest eps into the region's word when it closes the region, and tier 1 of the binning
    kernel forms its band from that bound.  The launch plan gives a call this small one wave per 512 rays, so no wave fills a
    region (1024 lines); with grid_blocks 1 the kernel has four waves, and n = 10 400 rays is the smallest round number at which
    they accept more than 4 x 1024 lines (0.4075 of the rays are accepted: 4238), so that at least one wave closes a full region
    in its loop and a second one at its end."""
    n = 10_400
    try:
        isx.set_option("grid_blocks", 1)
        h, cen, d = _on_off(isx, isx.default_config(), n, 0, scale=scale)
    finally:
        isx.set_option("grid_blocks", 0)
    print(f"exit_eps_scale {scale}: accepted {d[0]}, list B {d[1]}, redo entries {d[2]}")
    assert d[0] > 4 * 1024, d
    oh, ost = orc.fluxmap(orc.default_config(), n, SEED, 0)
    assert np.array_equal(h, oh)
    assert cen == _census(ost)


def test_scaled_bounds_send_no_fewer_candidates_to_the_redo_kernel(isx, orc):
    """exit_eps_scale 1, 1e3, 1e6 at 2e4 rays: map and census stay the oracle's, and a larger bound never leaves fewer candidates
    undecided (with every line's own eps in tier 1 and exact reciprocal roots in the bounds: 6 redo entries at 1e3, 41 477 at 1e6)."""
    n = 20_000
    oh, ost = orc.fluxmap(orc.default_config(), n, SEED, 0)
    redo = []
    for scale in (1, 1000, 1_000_000):
        h, cen, d = _on_off(isx, isx.default_config(), n, 0, scale=scale)
        print(f"exit_eps_scale {scale}: accepted {d[0]}, list B {d[1]}, redo entries {d[2]}")
        assert np.array_equal(h, oh)
        assert cen == _census(ost)
        redo.append(d[2])
    assert redo[0] <= redo[1] <= redo[2] and redo[2] > 0, redo
