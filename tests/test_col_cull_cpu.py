"""The tilt cull of isx_bin_cols_kernel's column producer, restated in numpy binary32 (tests/colcull_np.py),
against the oracle's own detector test: no reference hit may lie outside the slots the cull leaves, for either variant (column
test only; column test + row trim), and no bin may be handed out twice.  No GPU.

Mutation check (run once in a scratch copy, docs/LOG.md section 32.2): with every slack term of the cull halved (slack = 0.5)
test_edge_family_survives_the_cull fails -- 10 reference hits lost at each of the three scales -- so the family does sit at the
cull's edge; with slack = 1.0 it passes.  test_edge_family_bites_without_slack keeps the slack = 0 half of that in the suite."""
import numpy as np
import pytest

import bandwin_np as BW
import colcull_np as CC
import edge_lines as EL
from boxwin_np import acos_cull, random_lines

SEED = 0x5EED0001


def _cfg(orc, n_theta=180, n_phi=90, diameter=40.0, distance=100.0):
    c = orc.default_config()
    c.n_theta, c.n_phi, c.det_diameter, c.det_distance = n_theta, n_phi, diameter, distance
    return c


def _no_hit_lost(orc, c, P, V, variants=(1, 2)):
    """every reference hit of every line inside the slots of every variant, no bin twice -> (hits, candidates per variant, caps lines)"""
    hits, cand, caps = 0, {v: 0 for v in variants}, 0
    for p, v in zip(P, V):
        h = CC.reference_hits(c, p, v)
        hits += int(h.sum())
        for var in variants:
            kind, slots = CC.line_slots(p, v, c, var)
            cov = np.zeros((c.n_theta, c.n_phi), int)
            for j, i, n in slots:
                cov[i:i + n, j] += 1
            assert not (h & (cov == 0)).any(), ("hit lost", var, kind, p.tolist(), v.tolist(), np.argwhere(h & (cov == 0))[:4].tolist())
            assert not (cov > 1).any(), ("bin twice", var, kind, p.tolist(), v.tolist())
            cand[var] += int(cov.sum())
        caps += kind == "caps"
    return hits, cand, caps


def _traced_lines(orc, c, n_lines):
    """the first n_lines counted exit lines of the oracle's trace, seed 0x5EED0001"""
    n = 3 * n_lines
    st, _, lp, d = orc.trace_endstates(c, n, SEED)
    keep = (st == 1) & (lp[:, 2] < c.exit_port_z)
    assert keep.sum() >= n_lines
    return lp[keep][:n_lines], d[keep][:n_lines]


# the five configurations of the issue's table, at its line counts
CONFIGS = {"default": ((180, 90, 40.0, 100.0), 3000), "45x20_10cm": ((45, 20, 10.0, 100.0), 2000), "80cm": ((180, 90, 80.0, 100.0), 500),
           "90x180": ((90, 180, 40.0, 100.0), 500), "R60": ((180, 90, 40.0, 60.0), 500)}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_traced_lines_lose_no_hit(orc, name):
    grid, n_lines = CONFIGS[name]
    c = _cfg(orc, *grid)
    P, V = _traced_lines(orc, c, n_lines)
    hits, cand, caps = _no_hit_lost(orc, c, P, V)
    assert hits > 0 and caps > 0.9 * n_lines, "the lines are lines with caps: the cull is what is tested"
    assert cand[2] <= cand[1]
    if name == "default":   # the cull does cull: variant 0 (no cull) hands on 1.59 candidates per hit on these lines
        assert cand[1] / hits < 1.53 and cand[2] / hits < 1.46, (cand, hits)


def test_variant_0_is_bandwin(orc):
    c = _cfg(orc)
    P, V = EL.bulk_lines(c, m=80, near=40)
    for p, v in zip(P, V):
        assert CC.line_slots(p, v, c, 0) == BW.line_slots(p, v, c)


@pytest.mark.parametrize("grid", [EL.DEFAULT] + EL.GRIDS, ids=lambda g: "%dx%d_d%g_R%g" % g)
def test_edge_line_families_lose_no_hit(orc, grid):
    c = _cfg(orc, *grid)
    for name, (P, V) in EL.families(c).items():
        step = 4 if name == "tangent" else 1            # (1400 tangent lines: every fourth, all seven eps)
        _no_hit_lost(orc, c, P[::step], V[::step], variants=(2,))


@pytest.mark.parametrize("grid", [(2, 3), (3, 2), (2, 90), (3, 180), (2, 1), (3, 1)], ids=lambda g: "%dx%d" % g)
def test_two_and_three_row_grids(orc, grid):
    """where tools/soak_cull.py found the overlap of the two caps' row ranges"""
    for diameter, distance in ((40.0, 100.0), (30.0, 25.0), (10.0, 100.0)):
        c = _cfg(orc, grid[0], grid[1], diameter, distance)
        P, V = EL.bulk_lines(c, m=60, near=60)
        _no_hit_lost(orc, c, P, V)


def test_random_geometries(orc):
    """60 geometries in the ranges tools/soak_cull.py draws from, 40 lines each (general position, aimed at the shell, near O)"""
    rng = np.random.default_rng(2024)
    caps = 0
    for k in range(60):
        c = orc.default_config()
        c.n_theta, c.n_phi = int(rng.integers(1, 200)), int(rng.integers(1, 180))
        if c.n_theta * c.n_phi > 36000:
            c.n_phi = 36000 // c.n_theta
        c.det_distance = float(rng.choice([30.0, 60.0, 100.0, 180.0]))
        c.det_diameter = float(c.det_distance * 2 * rng.choice([0.005, 0.05, 0.2, 0.3, 0.45, 0.55, 0.67, 0.8, 0.95, 1.05, 1.5, 3.0]))
        c.exit_port_z = float(rng.choice([-100.0, -120.0, -99.0]))
        c.box_half = float(rng.choice([200.0, 300.0]))
        P, V = EL.bulk_lines(c, seed=3000 + k, m=16, near=24)
        caps += _no_hit_lost(orc, c, P, V)[2]
    assert caps > 300, "enough of the lines have caps"


def test_acos_cull_underestimates_by_less_than_the_angle_slack():
    """ANGLE = 8e-5 rests on this: over every 4e-6-th of [0, 1] acos_cull falls short of acos by at most 6.8e-5"""
    x = np.linspace(0, 1, 2000001).astype(np.float32)
    short = np.arccos(x.astype(np.float64)) - acos_cull(x).astype(np.float64)
    assert short.max() < 6.8e-5 < float(CC.ANGLE)


SCALES = (0.01, 1.0, 100.0)
_EDGE = {}


def _edge(orc, f):
    if f not in _EDGE:
        c = CC.scaled(_cfg(orc), f)
        _EDGE[f] = (c,) + CC.edge_family(c, per_bin=3, extra=6)
    return _EDGE[f]


@pytest.mark.parametrize("f", SCALES)
def test_edge_family_survives_the_cull(orc, f):
    c, P, V, B, S = _edge(orc, f)
    inward = 0
    for p, v, b, s in zip(P, V, B, S):
        h = CC.reference_hits(c, p, v)
        inward += bool(s < 0 and h.reshape(-1)[b])
        for var in (1, 2):
            kind, slots = CC.line_slots(p, v, c, var)
            cov = np.zeros((c.n_theta, c.n_phi), bool)
            for j, i, n in slots:
                cov[i:i + n, j] = True
            assert not (h & ~cov).any(), ("hit lost", f, var, kind, int(b), p.tolist(), v.tolist())
    assert inward > 0.95 * (S < 0).sum(), "the lines shifted inwards hit the bin they were built on"


@pytest.mark.parametrize("f", SCALES)
def test_edge_family_bites_without_slack(orc, f):
    """the same lines through the restatement with its slack terms at 0: hits ARE lost (at 0.5 as well: module docstring)"""
    c, P, V, B, S = _edge(orc, f)
    lost = 0
    for p, v, b, s in zip(P, V, B, S):
        if s > 0:
            continue
        kind, slots = CC.line_slots(p, v, c, 2, slack=0.0)
        h = CC.reference_hits(c, p, v)
        cov = np.zeros((c.n_theta, c.n_phi), bool)
        for j, i, n in slots:
            cov[i:i + n, j] = True
        lost += int((h & ~cov).sum())
    assert lost > 0
