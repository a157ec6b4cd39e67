"""The exit-line rule (tests/exitscan_np.py) against the CPU oracle -- no GPU needed.

1. Every ray the rule accepts is EXITED in oracle.trace_endstates with n_points = j + 3, its direction lies within eps_V of the
   oracle's and the point of its line nearest to O within eps of the oracle's line's -- over the default configuration and the
   configurations that move a threshold (port angle, reflectance, bounce limit, scale, a ray range that crosses 2^32), and with j
   forced large (rho 0.999, port 175 deg: the drift has hundreds of steps to grow).
2. The reference test on the approximate lines gives the histogram it gives on the oracle's lines, against all detectors; a bin
   where the two differ is looked at line by line, and every difference must lie inside the band decide_approx leaves undecided."""
import numpy as np
import pytest

import exitscan_np as ex
import fatescan_np as fs

SEED = 0x5EED0001
EXITED = 1


def _scaled(cfg, s):
    c = cfg.copy()
    c.r_in *= s; c.r_out *= s; c.box_half *= s
    c.det_diameter *= s; c.det_distance *= s; c.exit_port_z *= s
    for k in range(3):
        c.src[k] *= s
    return c


def _cases(orc):
    d = orc.default_config()

    def mod(**kw):
        c = d.copy()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    return {
        "default": (d, 1_000_000, 0),
        "port160": (mod(theta_max_deg=160.0), 200_000, 0),
        "rho0.9": (mod(reflectance=0.9), 200_000, 0),
        "max_points3": (mod(max_points=3), 200_000, 0),
        "max_points8": (mod(max_points=8), 200_000, 0),
        "scale0.01": (_scaled(d, 0.01), 200_000, 0),
        "scale100": (_scaled(d, 100.0), 200_000, 0),
        "first_wrap": (d, 200_000, 2 ** 32 - 1000),
        "long_rays": (mod(reflectance=0.999, theta_max_deg=175.0, max_points=5000), 4000, 0),
    }


_memo = {}


def _run(orc, name):
    """the rule and the oracle's end states of a case, computed once"""
    if name not in _memo:
        cfg, n, first = _cases(orc)[name]
        _memo[name] = (cfg, ex.exit_lines_np(cfg, orc, n, SEED, first), orc.trace_endstates(cfg, n, SEED, first))
    return _memo[name]


@pytest.mark.parametrize("name", ["default", "port160", "rho0.9", "max_points3", "max_points8", "scale0.01", "scale100", "first_wrap",
                                  "long_rays"])
def test_accepted_rays_exit_in_the_oracle_along_the_same_line_within_the_bound(orc, name):
    cfg, a, (status, npts, lp, dr) = _run(orc, name)
    idx = a["idx"]
    assert idx.size > 0, name
    wrong = status[idx] != EXITED
    assert not wrong.any(), (name, int(wrong.sum()), idx[wrong][:5])
    assert np.array_equal(npts[idx], a["n_points"]), name
    assert (lp[idx, 2] < cfg.exit_port_z).all(), name
    o = np.array([0.0, 0.0, cfg.exit_port_z])
    dV = np.linalg.norm(dr[idx] - a["V"], axis=1)
    dQ = np.linalg.norm(ex.nearest_to(o, lp[idx], dr[idx]) - ex.nearest_to(o, a["P"], a["V"]), axis=1)
    reach = (a["eps"] - a["eps_p"] - a["eps_ref"] - 4e-15 * cfg.box_half) / a["eps_V"]     # (the kernel's lever of a direction error)
    exits = int((status == EXITED).sum())
    print(f"{name}: accepted {idx.size} of {a['listed']} listed rays, {idx.size / max(exits, 1):.4f} of the oracle's exits; j up to "
          f"{int(a['j'].max())}; max |dV| {dV.max():.3g} (bound {a['eps_V'][dV.argmax()]:.3g}, least bound / measured "
          f"{(a['eps_V'] / np.maximum(dV, 1e-300)).min():.3g}); max |dQ| {dQ.max():.3g} r_in {cfg.r_in:g} (eps {a['eps'][dQ.argmax()]:.3g}, "
          f"least eps / measured {(a['eps'] / np.maximum(dQ, 1e-300)).min():.3g})")
    assert (dV <= a["eps_V"]).all(), (name, float((dV / a["eps_V"]).max()))
    assert (dQ <= a["eps"]).all(), (name, float((dQ / a["eps"]).max()))
    assert (dV * reach / 2.1 <= a["eps"]).all(), name
    if name in ("default", "first_wrap"):
        assert idx.size >= 0.9 * exits, (idx.size, exits)


@pytest.mark.parametrize("name,sample", [("default", 100_000), ("long_rays", 4000)])
def test_reference_decisions_on_the_approximate_lines_differ_only_inside_the_band(orc, name, sample):
    cfg, a, (status, npts, lp, dr) = _run(orc, name)
    keep = a["idx"] < sample
    idx, P, V, eps = a["idx"][keep], a["P"][keep], a["V"][keep], a["eps"][keep]
    h_approx = orc.bin_lines(cfg, P, V).ravel()
    h_exact = orc.bin_lines(cfg, lp[idx], dr[idx]).ravel()
    table = orc.detector_table(cfg)
    outside = flagged = differ = 0
    for b in np.flatnonzero(h_approx != h_exact):
        d_a = np.array([orc.check_intersection(table[b], cfg.det_diameter, p, v) for p, v in zip(P, V)])
        d_e = np.array([orc.check_intersection(table[b], cfg.det_diameter, p, v) for p, v in zip(lp[idx], dr[idx])])
        g, band = ex.decide_approx_np(cfg, table[b], P, V, eps)
        bad = d_a != d_e
        differ += int(bad.sum())
        outside += int((bad & (np.abs(g) > band)).sum())
    # the flagged share per line, on a stride of the detectors (every detector of every 97th bin)
    for b in range(0, table.shape[0], 97):
        g, band = ex.decide_approx_np(cfg, table[b], P, V, eps)
        flagged += int((np.abs(g) <= band).sum())
    share = flagged * 97.0 / max(idx.size, 1)
    print(f"{name}: {idx.size} lines x {table.shape[0]} detectors: {differ} decisions differ, {outside} of them outside the band; "
          f"flagged candidates per line ~{share:.3g}")
    assert outside == 0
    assert share <= 1e-2, share
