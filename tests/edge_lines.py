"""Deterministic exit lines at the edges of the binning kernels -- TEST INFRASTRUCTURE (pure numpy, fixed seeds).

Traced rays leave through the port and pass near O = (0, 0, exit_port_z); in a test-sized run they never land on a detector's rim
to within rounding, on the |n.V| < 1e-10 parallel cut, on the pole row or the phi seam on purpose, or on the thresholds of the
float32 cull (the far skip dO - rho > 1.001 R, the a1 < 0.999 R and 4 (R^2 - dO^2) > 4.04 ch^2 switches of prep_record).  The
families below are built to.  families(cfg) -> {name: (P[k, 3], V[k, 3])} with unit V (| |V| - 1 | <= 1e-12, |P| <= sqrt(3) box_half: the
domain of isx_bin_injected_lines' flux sink); tangent_lines / parallel_lines also say which bin each line was aimed at.
exit_edge_lines(spec) is the hand-made edge family of the exit maps and the light field (those sinks only: it holds NaN and inf).
"""
import numpy as np

import boxwin_np

# the grids (n_theta, n_phi, diameter, distance) and families of tests/test_gpu_injected_lines.py and tests/test_injected_lines_cpu.py.
# The last grid is beyond the slot kernels' limits (n_theta > 256), so that the plan's fallback to isx_bin_lines_kernel is what runs;
# on (17, 4, 195, 100) and (180, 90, 176, 100) no line has caps: every line is a band line
DEFAULT = (180, 90, 40.0, 100.0)
GRIDS = [(45, 20, 10.0, 100.0), (7, 3, 60.0, 80.0), (1, 1, 40.0, 100.0), (2, 3, 30.0, 25.0), (17, 4, 195.0, 100.0),
         (180, 90, 176.0, 100.0), (300, 8, 20.0, 100.0)]
FAMILIES = ("tangent", "parallel", "through_O", "axis", "seam", "shell", "bulk")

TANGENT_EPS = (0.0, -1e-15, 1e-15, -1e-12, 1e-12, -1e-7, 1e-7)
PARALLEL_DELTA = (0.0, 5e-11, -5e-11, 1e-10 * (1 - 1e-6), -1e-10 * (1 - 1e-6), 1e-10 * (1 + 1e-6), -1e-10 * (1 + 1e-6),
                  2e-10, -2e-10, 1e-8, -1e-8)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1)[..., None]


def _random_units(rng, m):
    return _unit(rng.standard_normal((m, 3)))


def _perp(rng, V):
    """a random unit vector perpendicular to every V[k]"""
    a = rng.standard_normal(V.shape)
    a -= np.einsum("ij,ij->i", a, V)[:, None] * V
    return _unit(a)


def detector_table(cfg):
    """Detector::setPosition as the library builds it (isx_detector_table is host code: no GPU, and no oracle, needed) --
    centres c[k, 3], normals n[k, 3]; restated in numpy so that this module stands alone."""
    th = np.deg2rad((np.arange(cfg.n_theta) + 0.5) * 90.0 / cfg.n_theta)
    ph = np.deg2rad((np.arange(cfg.n_phi) + 0.5) * 360.0 / cfg.n_phi)
    T, F = np.meshgrid(th, ph, indexing="ij")
    R, pz = cfg.det_distance, cfg.exit_port_z
    c = np.stack([R * np.sin(T) * np.cos(F), R * np.sin(T) * np.sin(F), pz - R * np.cos(T)], axis=-1).reshape(-1, 3)
    d = c - np.array([0.0, 0.0, pz])
    mag = np.linalg.norm(d, axis=1)
    n = np.stack([-d[:, 1] / mag, d[:, 0] / mag, d[:, 2] / mag], axis=1)
    return c, n


def target_bins(cfg, rng, extra=4):
    """bins lines are aimed at: the four corners of the grid (rows 0 and n_theta - 1, columns 0 and n_phi - 1) and a few others"""
    nt, nph = cfg.n_theta, cfg.n_phi
    bins = {0, nph - 1, (nt - 1) * nph, nt * nph - 1}
    for _ in range(extra):
        bins.add(int(rng.integers(nt)) * nph + int(rng.integers(nph)))
    return sorted(bins)


def _plane_basis(n):
    """two unit vectors spanning the plane with unit normal n[k]"""
    t = np.zeros_like(n)
    t[np.arange(len(n)), np.argmin(np.abs(n), axis=1)] = 1.0
    e1 = _unit(t - np.einsum("ij,ij->i", t, n)[:, None] * n)
    return e1, np.cross(n, e1)


def tangent_lines(cfg, per_eps=200, seed=101):
    """Lines through a point of a target detector's plane at rho_d (1 + eps) from its centre: -> (P, V, target bin, eps).
    eps = 0 lines are decided by rounding alone.  (|V.n| >= 0.1, so that the test's own rounding, ~1e-16 |P| / |V.n| / rho_d,
    stays below the 1e-12 offsets, which must decide.)"""
    rng = np.random.default_rng(seed)
    c, n = detector_table(cfg)
    bins = target_bins(cfg, rng)
    rho = cfg.det_diameter / 2
    P, V, tgt, eps = [], [], [], []
    for e in TANGENT_EPS:
        k = np.array([bins[i % len(bins)] for i in range(per_eps)])
        e1, e2 = _plane_basis(n[k])
        az = rng.uniform(0, 2 * np.pi, per_eps)
        X = c[k] + (rho * (1.0 + e)) * (np.cos(az)[:, None] * e1 + np.sin(az)[:, None] * e2)
        v = _random_units(rng, per_eps)
        for _ in range(64):
            bad = np.abs(np.einsum("ij,ij->i", v, n[k])) < 0.1
            if not bad.any():
                break
            v[bad] = _random_units(rng, int(bad.sum()))
        s = rng.uniform(50, 200, per_eps)
        P.append(X - s[:, None] * v); V.append(v); tgt.append(k); eps.append(np.full(per_eps, e))
    return np.concatenate(P), np.concatenate(V), np.concatenate(tgt), np.concatenate(eps)


def parallel_lines(cfg, seed=202, azimuths=4):
    """Lines from a point of a target detector's plane (rho_d / 2 from its centre) along unit(e + delta n), e in the plane:
    n.V = delta / sqrt(1 + delta^2) spans the reference's |dot| < 1e-10 cut.  -> (P, V, target bin, delta)."""
    rng = np.random.default_rng(seed)
    c, n = detector_table(cfg)
    bins = target_bins(cfg, rng)
    rho = cfg.det_diameter / 2
    if len(bins) < 4:
        azimuths *= 2          # (a grid of one or two bins: still at least 20 lines on either side of the cut)
    P, V, tgt, dl = [], [], [], []
    for k in bins:
        e1, e2 = _plane_basis(n[k:k + 1])
        for _ in range(azimuths):
            a, b = rng.uniform(0, 2 * np.pi, 2)
            p = c[k] + 0.5 * rho * (np.cos(a) * e1[0] + np.sin(a) * e2[0])
            e = np.cos(b) * e1[0] + np.sin(b) * e2[0]
            for d in PARALLEL_DELTA:
                P.append(p); V.append(_unit(e + d * n[k])); tgt.append(k); dl.append(d)
    return np.array(P), np.array(V), np.array(tgt), np.array(dl)


def _through(rng, O, dist, V, s=120.0):
    """lines along V[k] whose foot of O lies at distance dist[k] from O"""
    u = _perp(rng, V)
    return O + np.asarray(dist)[:, None] * u - s * V


def through_O_lines(cfg, seed=303, per=24):
    rng = np.random.default_rng(seed)
    R = cfg.det_distance
    O = np.array([0.0, 0.0, cfg.exit_port_z])
    P, V = [], []
    for off in (0.0, 1e-9 * R, 1e-3 * R * (1 - 1e-3), 1e-3 * R * (1 + 1e-3)):
        v = _random_units(rng, per)
        v[0] = (0.0, 0.0, -1.0); v[1] = (0.0, 0.0, 1.0); v[2] = (1.0, 0.0, 0.0); v[3] = (0.0, -1.0, 0.0)
        P.append(_through(rng, O, np.full(per, off), v)); V.append(v)
    return np.concatenate(P), np.concatenate(V)


def axis_lines(cfg, seed=404):
    """Exactly vertical lines on and near the axis (the pole: every column of a row), exactly horizontal ones, and directions at
    the cull's own switches: |V_xy| ~ 1e-7 and 1e-5 (1 +- 1e-3) (box_line: vxy2 > 1e-10), |V.z| = 1e-3 (1 +- 1e-3) (avz > 1e-3)."""
    rng = np.random.default_rng(seed)
    R, rho, pz = cfg.det_distance, cfg.det_diameter / 2, cfg.exit_port_z
    P, V = [], []
    for x in (0.0, 1e-9, 1e-3 * R, 0.5 * rho, rho, rho * (1 + 1e-9), 2.0 * rho, 0.7 * R):
        for sgn in (-1.0, 1.0):
            a = rng.uniform(0, 2 * np.pi)
            P.append((x * np.cos(a), x * np.sin(a), pz - sgn * 150.0)); V.append((0.0, 0.0, sgn))
    P.append((0.0, 0.0, pz + 50.0)); V.append((0.0, 0.0, -1.0))
    c, _ = detector_table(cfg)
    aim = np.concatenate([c[rng.integers(len(c), size=12)], np.array([[0.0, 0.0, pz]]) + rng.standard_normal((6, 3)) * 0.2 * R])
    for t in aim:
        a = rng.uniform(0, 2 * np.pi)
        ca, sa = np.cos(a), np.sin(a)
        dirs = [(ca, sa, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]
        dirs += [_unit((w * ca, w * sa, -1.0)) for w in (1e-7, 1e-5 * (1 - 1e-3), 1e-5 * (1 + 1e-3))]
        dirs += [_unit((ca, sa, z)) for z in (1e-3 * (1 - 1e-3), -1e-3 * (1 + 1e-3), 1e-3, -1e-3)]
        for v in dirs:
            v = np.asarray(v, dtype=np.float64)
            P.append(t - 130.0 * v); V.append(v)
    return np.array(P, dtype=np.float64), np.array(V, dtype=np.float64)


def seam_lines(cfg, seed=505, per=6):
    """Aimed at the centres of columns 0 and n_phi - 1, at phi = 0 between them, and at the first and last rows."""
    rng = np.random.default_rng(seed)
    nt, nph, R, pz = cfg.n_theta, cfg.n_phi, cfg.det_distance, cfg.exit_port_z
    c, _ = detector_table(cfg)
    rows = sorted({0, nt // 3, nt // 2, nt - 1})
    tgt = [c[i * nph + j] for i in rows for j in sorted({0, nph - 1})]
    th = np.deg2rad((np.array(rows) + 0.5) * 90.0 / nt)
    tgt += [np.array([R * np.sin(t), 0.0, pz - R * np.cos(t)]) for t in th]                       # phi = 0 exactly
    tgt += [c[i * nph + int(j)] for i in sorted({0, nt - 1}) for j in rng.integers(nph, size=3)]   # first and last rows
    tgt = np.repeat(np.array(tgt), per, axis=0)
    v = _random_units(rng, len(tgt))
    return tgt - 150.0 * v, v


def shell_lines(cfg, seed=606, per=10):
    """Lines at the distances from O where the cull switches: (R + rho_d) (1 +- 1e-6 / 1e-3) (the last hit), 1.001 R + rho_d (the
    far skip), (R - rho_d) (1 +- 1e-3) and 0.999 R - rho_d (the fast path's switches; left out where rho_d > R)."""
    rng = np.random.default_rng(seed)
    R, rho = cfg.det_distance, cfg.det_diameter / 2
    O = np.array([0.0, 0.0, cfg.exit_port_z])
    dist = [(R + rho) * f for f in (1 - 1e-6, 1 + 1e-6, 1 - 1e-3, 1 + 1e-3)]
    dist += [(1.001 * R + rho) * f for f in (1 - 1e-6, 1.0, 1 + 1e-6)]
    dist += [d for d in ((R - rho) * (1 - 1e-3), (R - rho) * (1 + 1e-3), 0.999 * R - rho, (0.999 * R - rho) * (1 - 1e-6),
                         (0.999 * R - rho) * (1 + 1e-6)) if d > 0]
    dist = np.repeat(np.array(dist), per)
    v = _random_units(rng, len(dist))
    s = rng.uniform(50, 200, len(dist))
    u = _perp(rng, v)
    return O + dist[:, None] * u - s[:, None] * v, v


def bulk_lines(cfg, seed=707, m=160, near=80):
    """boxwin_np.random_lines (general position + horizontal, vertical, nearly horizontal, aimed at the shell) and lines through the
    neighbourhood of O, where a line has two low caps (tests/test_cull_math.py: test_column_slots_contain_every_hit)."""
    rng = np.random.default_rng(seed)
    P, V = boxwin_np.random_lines(cfg, m, seed=seed)
    tgt = np.array([0.0, 0.0, cfg.exit_port_z]) + rng.standard_normal((near, 3)) * cfg.det_distance * 0.4
    v = _random_units(rng, near)
    return np.concatenate([P, tgt - 120.0 * v]), np.concatenate([V, v])


def families(cfg):
    """{name: (P, V)}: every family of the flux binners, unit V"""
    tp, tv, _, _ = tangent_lines(cfg)
    pp, pv, _, _ = parallel_lines(cfg)
    out = {"tangent": (tp, tv), "parallel": (pp, pv), "through_O": through_O_lines(cfg), "axis": axis_lines(cfg),
           "seam": seam_lines(cfg), "shell": shell_lines(cfg), "bulk": bulk_lines(cfg)}
    for name, (P, V) in out.items():
        assert np.isfinite(P).all() and np.isfinite(V).all(), name
        assert np.abs(np.linalg.norm(V, axis=1) - 1.0).max() <= 1e-12 and np.linalg.norm(P, axis=1).max() <= np.sqrt(3.0) * cfg.box_half, name
    return out


def exit_edge_lines(spec):
    """The hand-made edge family of the exit maps / the light field for `spec` (n_u, n_v, n_x, n_y >= 0, plane_z, half_extent):
    direction components exactly -1 and +1 and exactly on bin edges 2k/n - 1, V.z in {-0.0, +0.0, -1e-300, -1e-17}, crossing points
    exactly at +-half_extent and on interior bin edges, NaN and +-inf in any single coordinate.  -> (P, V); V is not always unit."""
    h, pz = float(spec.half_extent), float(spec.plane_z)
    P, V = [], []

    def add(p, v):
        P.append(tuple(float(x) for x in p)); V.append(tuple(float(x) for x in v))
    base_p = (0.25 * h, -0.125 * h, pz + 3.0)
    for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (1, 1, -1), (-1, -1, -1), (-1, 1, -0.5)):
        add(base_p, v)
    nu, nv = max(spec.n_u, 1), max(spec.n_v, 1)
    for k in sorted({0, 1, nu // 2, nu - 1, nu}):
        for m in sorted({0, 1, nv // 2, nv - 1, nv}):
            add(base_p, (2.0 * k / nu - 1.0, 2.0 * m / nv - 1.0, -0.5))
    for vz in (-0.0, 0.0, -1e-300, -1e-17):
        add(base_p, (0.3, -0.2, vz))
        add((0.0, 0.0, pz), (0.3, -0.2, vz))
    nx, ny = max(spec.n_x, 1), max(spec.n_y, 1)
    xs = [-h, h, np.nextafter(-h, -np.inf), np.nextafter(h, 0.0)] + [-h + 2.0 * h * k / nx for k in sorted({1, nx // 2, nx - 1})]
    ys = [-h, h, np.nextafter(h, np.inf), np.nextafter(-h, 0.0)] + [-h + 2.0 * h * k / ny for k in sorted({1, ny // 2, ny - 1})]
    for x in xs:
        for y in ys:
            add((x, y, pz), (0.1, 0.2, -1.0))          # on the plane: t = 0, the crossing point is (x, y) exactly
            add((x, y, pz + 1.0), (0.0, 0.0, -1.0))    # t = 1 exactly, nothing added
    for k in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            l = [0.25 * h, -0.125 * h, pz + 3.0, 0.3, -0.2, -0.6]
            l[k] = bad
            add(l[:3], l[3:])
    return np.array(P, dtype=np.float64), np.array(V, dtype=np.float64)
