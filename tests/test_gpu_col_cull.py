"""The tilt cull of isx_bin_cols_kernel's column producer (col_cull) on the GPU: it removes candidates, never
a hit.  Histogram and census of isx_fluxmap equal the oracle's and those of bin_mode 0 (every bin of every line: no pre-selection
at all), with the exit-line path on and off; the constructed lines at the cull's own edge (tests/colcull_np.py: edge_family) and
the families of tests/edge_lines.py go through isx_bin_injected_lines against the oracle's isxo_bin_lines, bit for bit."""
import numpy as np
import pytest

import colcull_np as CC
import edge_lines as EL

pytestmark = pytest.mark.gpu

SEED = 0x5EED0001
N = 20000
CENSUS = ("launched", "exited", "counted_below_z", "absorbed", "suspended", "bin_increments", "wall_hits")
DEFAULTS = (("exit_scan", -1), ("bin_mode", 1), ("bin_cols", 1), ("bin_slots", 1), ("pipeline", 1))

# (n_theta, n_phi, diameter, distance), first
CASES = {
    "default": ((180, 90, 40.0, 100.0), 0),
    "45x20_10cm": ((45, 20, 10.0, 100.0), 0),
    "80cm": ((180, 90, 80.0, 100.0), 0),
    "R60": ((180, 90, 40.0, 60.0), 0),
    "2x3": ((2, 3, 40.0, 100.0), 0),
    "3x2": ((3, 2, 40.0, 100.0), 0),
    "first_wrap": ((180, 90, 40.0, 100.0), 2 ** 32 - 1000),
}


@pytest.fixture(autouse=True)
def _default_options(isx):
    for k, v in DEFAULTS:
        isx.set_option(k, v)
    yield
    for k, v in DEFAULTS:
        isx.set_option(k, v)


def _cfg(mod, grid):
    c = mod.default_config()
    c.n_theta, c.n_phi, c.det_diameter, c.det_distance = grid
    return c


def _census(st):
    return tuple(int(getattr(st, f)) for f in CENSUS)


_ORACLE = {}


def _oracle(orc, name):
    if name not in _ORACLE:
        grid, first = CASES[name]
        h, st = orc.fluxmap(_cfg(orc, grid), N, SEED, first)
        h.setflags(write=False)
        _ORACLE[name] = (h, _census(st))
    return _ORACLE[name]


@pytest.mark.parametrize("exit_scan", [1, 0])
@pytest.mark.parametrize("name", list(CASES))
def test_fluxmap_is_the_oracles_and_the_brute_force_binners(isx, orc, name, exit_scan):
    grid, first = CASES[name]
    want, want_census = _oracle(orc, name)
    assert int(want.sum()) > 0
    isx.set_option("exit_scan", exit_scan)
    h, st = isx.fluxmap(_cfg(isx, grid), N, SEED, first)
    assert isx.last_kernel_ms()[2] > 0, "a binning kernel ran"
    assert np.array_equal(h, want), (name, np.argwhere(h != want)[:8].tolist())
    assert _census(st) == want_census
    isx.set_option("bin_mode", 0)
    hb, sb = isx.fluxmap(_cfg(isx, grid), N, SEED, first)
    assert np.array_equal(h, hb) and _census(st) == _census(sb)


SCALES = (0.01, 1.0, 100.0)


@pytest.mark.parametrize("f", SCALES)
def test_constructed_edge_lines_against_the_oracle(isx, orc, f):
    """lines through the disc point farthest from the meridian plane, along it, shifted by 1e-9 cm and a few ulp (the whole
    geometry at three scales: the cull's slack terms are all relative)"""
    co = CC.scaled(_cfg(orc, EL.DEFAULT), f)
    P, V, B, S = CC.edge_family(co, per_bin=3, extra=6)
    want = orc.bin_lines(co, P, V)
    inward = orc.bin_lines(co, P[S < 0], V[S < 0])
    assert int(inward.sum()) >= int((S < 0).sum()), "the lines shifted inwards hit"
    c = _cfg(isx, EL.DEFAULT)
    c.det_distance, c.det_diameter, c.exit_port_z = co.det_distance, co.det_diameter, co.exit_port_z
    c.box_half = max(c.box_half, co.box_half)       # (the world box stays outside the sphere; it bounds the lines' points only)
    hits, _, _, inc = isx.bin_injected_lines(c, isx.INJECT_FLUX, P, V)
    assert isx.last_kernel_ms()[2] > 0
    assert np.array_equal(hits, want), (f, np.argwhere(hits != want)[:8].tolist())
    assert inc == int(want.sum())


@pytest.mark.parametrize("grid", [EL.DEFAULT, (45, 20, 10.0, 100.0), (2, 3, 30.0, 25.0), (7, 3, 60.0, 80.0)], ids=lambda g: "%dx%d_d%g_R%g" % g)
def test_edge_line_families_against_the_oracle(isx, orc, grid):
    fam = EL.families(_cfg(orc, grid))
    P = np.concatenate([fam[k][0] for k in EL.FAMILIES]); V = np.concatenate([fam[k][1] for k in EL.FAMILIES])
    want = orc.bin_lines(_cfg(orc, grid), P, V)
    hits, _, _, inc = isx.bin_injected_lines(_cfg(isx, grid), isx.INJECT_FLUX, P, V)
    assert np.array_equal(hits, want), (grid, np.argwhere(hits != want)[:8].tolist())
    assert inc == int(want.sum()) > 0
