"""isx_wall_map without a GPU: the numpy restatement of the contract (tests/wallmap_np.py), its two sources of wall points
against each other, the flatness of the diffuse wall irradiance, and the parts of the ABI that need no device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import wallmap_np as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_limit_sweep_equals_replay(orc):
    """Two independent readings of the oracle give the same interactions, bit for bit (300 rays, M = 5: 1445 points)."""
    c = orc.default_config()
    n, M = 300, 5
    rp = W.replay(c, n, 7)
    keep = rp[1] < M
    a = W.sort_points(tuple(x[keep] for x in rp))
    b = W.sort_points(W.limit_sweep(orc, c, n, 7, M))
    print("points: replay %d (j < %d: %d), limit sweep %d" % (rp[0].size, M, a[0].size, b[0].size))
    assert a[0].size == b[0].size == 1445
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64))
    # ... and with an offset first ray
    rp = W.replay(c, 100, 7, first=1000)
    a = W.sort_points(tuple(x[rp[1] < 3] for x in rp))
    b = W.sort_points(W.limit_sweep(orc, c, 100, 7, 3, first=1000))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64))


def test_projection_properties(orc):
    c = orc.default_config()
    # the pole, the equator, the antipode
    r = c.r_in
    X, Y = W.project([[0, 0, r], [r, 0, 0], [0, -r, 0]], r)
    assert (X[0], Y[0]) == (0.0, 0.0)
    assert X[1] == pytest.approx(np.sqrt(0.5), abs=1e-15) and Y[2] == pytest.approx(-np.sqrt(0.5), abs=1e-15)
    # (a radius whose reciprocal is exact, so that c == -1.0 exactly: 0.5 / 0 = inf, 0 * inf = NaN -> outside; the same for NaN input)
    X, Y = W.project([[0, 0, -128.0]], 128.0)
    assert np.isnan(X[0]) and np.isnan(Y[0])
    _, _, ok = W.bins([[0, 0, -128.0], [0, 0, 128.0], [float("nan"), 0, 1.0], [3.0, 0, -128.0]], 128.0, 8, 8)
    assert list(ok) == [False, True, False, False]                            # (the last: 3/128 * inf = inf)
    # equal area: X^2 + Y^2 = (1 - cos(theta)) / 2 = sin^2(theta / 2)
    th = np.linspace(0.01, 3.0, 50)
    q = np.stack([r * np.sin(th) * np.cos(1.0), r * np.sin(th) * np.sin(1.0), r * np.cos(th)], axis=1)
    X, Y = W.project(q, r)
    assert np.allclose(X * X + Y * Y, np.sin(th / 2) ** 2, rtol=1e-13)
    # every inner point of the default configuration lies in the wall disc (observed: |X| <= 0.9961 = sin 85 deg)
    pts = W.replay(c, 2000, 11)
    inner = pts[2]
    assert inner.sum() > 50_000 and (~inner).sum() > 0
    X, Y = W.project(pts[3][inner], r)
    lim = np.sin(np.deg2rad(c.theta_max_deg) / 2.0) ** 2
    print("max X^2 + Y^2 = %.6f (wall disc %.6f), max |X| = %.4f" % ((X * X + Y * Y).max(), lim, np.abs(X).max()))
    assert (X * X + Y * Y).max() <= lim + 1e-12
    # a bin edge opens the bin above; n_x is a power of two, so the edges and the formula are exact
    m, k = W.wall_map_np((np.zeros(1, np.int64), np.zeros(1, np.int64), np.ones(1, bool), np.array([[0.0, 0.0, r]])), r, 16, 4, 0)
    assert m[2, 8] == 1 and k == {"binned": 1, "outside": 0, "skipped": 0, "other_surface": 0}


def test_classification_and_identities(orc):
    c = orc.default_config()
    pts = W.replay(c, 3000, 5)
    total = pts[0].size
    for first_order, nx, ny in ((0, 64, 64), (1, 96, 40), (3, 1, 1), (10 ** 6, 8, 8)):
        m, k = W.wall_map_np(pts, c.r_in, nx, ny, first_order)
        assert m.shape == (ny, nx) and int(m.sum()) == k["binned"]
        assert sum(k.values()) == total
        assert k["other_surface"] == int((~pts[2]).sum())
        assert k["skipped"] == int((pts[2] & (pts[1] < first_order)).sum())
    assert k["binned"] == 0                                                   # (first_order beyond every ray)
    m0, k0 = W.wall_map_np(pts, c.r_in, 32, 32, 0)
    m1, k1 = W.wall_map_np(pts, c.r_in, 32, 32, 1)
    d = m0.astype(np.int64) - m1.astype(np.int64)
    assert (d != 0).sum() == 1 and d.max() == 3000 == k1["skipped"]           # the first strike of the pencil source: one bin


def test_flatness_of_the_diffuse_wall_irradiance(orc):
    """first_order 1, 16 x 16, 4e4 replayed rays: chi2 against a flat expectation over the bins whose four corners lie within
    0.9 sin(theta_max / 2) must be <= dof + 5 sqrt(2 dof).  (The chord identity makes the diffuse wall irradiance uniform.)"""
    c = orc.default_config()
    pts = W.replay(c, 40_000, 7)
    m, k = W.wall_map_np(pts, c.r_in, 16, 16, 1)
    chi2, dof = W.flatness_chi2(m, c.theta_max_deg)
    print("chi2 %.1f for %d dof (bound %.1f), binned %d" % (chi2, dof, dof + 5 * np.sqrt(2 * dof), k["binned"]))
    assert dof > 100 and k["binned"] > 2_000_000
    assert chi2 <= dof + 5 * np.sqrt(2 * dof)


def test_binding_structs_and_default_spec():
    import altair_raytracing_amd as isx
    assert C.sizeof(isx.WallMapSpec) == 24 and C.sizeof(isx.WallMapCounts) == 32
    cfg = isx.default_config()
    s = isx.default_wall_map_spec(cfg)
    assert s.struct_size == C.sizeof(isx.WallMapSpec) and s.reserved0 == 0 and s.reserved1 == 0
    assert (s.n_x, s.n_y, s.first_order) == (64, 64, 0)
    t = s.copy(); t.n_x = 5
    assert s.n_x == 64 and t.n_x == 5
    assert isx.abi.WALL_MAP_MAX_BINS == 8192


def test_the_library_exports_what_the_header_declares():
    import altair_raytracing_amd as isx
    header = open(os.path.join(ROOT, "include", "isx.h")).read()
    for name in ("isx_default_wall_map_spec", "isx_wall_map", "isx_wall_map_device"):
        assert name + "(" in header and name in isx.EXPORTS and hasattr(isx.load(), name)
    assert "#define ISX_WALL_MAP_MAX_BINS 8192" in header
    out = subprocess.run(["nm", "-D", "--defined-only", isx.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("isx_")}
    declared = set(isx.EXPORTS)
    assert {"isx_default_wall_map_spec", "isx_wall_map", "isx_wall_map_device"} <= exported
    assert exported - declared <= {"isx_diag_read"}, exported - declared


def test_entry_points_without_a_device():
    """Without a HIP device both entry points answer ISX_ERR_NO_DEVICE (there is no CPU path); where a device is present, a
    process that never called isx_init() gets ISX_ERR_NOT_INIT from both."""
    code = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import altair_raytracing_amd as isx
lib = isx.load()
have = lib.isx_init(0) == 0
if have:
    lib.isx_shutdown()
cfg = isx.default_config()
spec = isx.default_wall_map_spec(cfg)
got = []
try:
    isx.wall_map(cfg, 10, 1)
    got.append(0)
except isx.IsxError as e:
    got.append(e.status)
try:
    isx.wall_map_device(cfg, spec, 10, 1, 0, 4096, 8192)
    got.append(0)
except isx.IsxError as e:
    got.append(e.status)
print("have" if have else "none", got[0], got[1])
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    have, a, b = r.stdout.split()
    import altair_raytracing_amd as isx
    want = isx.abi.ERR_NOT_INIT if have == "have" else isx.abi.ERR_NO_DEVICE
    assert (int(a), int(b)) == (want, want), r.stdout


def test_wall_map_sharded_single_rank():
    """one rank, no process group: the tracer's result passes through untouched"""
    import altair_raytracing_amd as isx

    class K:
        binned, outside, skipped, other_surface = 5, 1, 2, 3

    class S:
        launched, exited, counted_below_z, absorbed, suspended, bin_increments, wall_hits = 4, 1, 1, 3, 0, 5, 11

    seen = {}

    def trace(cfg, count, seed, spec, first):
        seen["args"] = (count, seed, first)
        return np.arange(6, dtype=np.uint64).reshape(2, 3), K, S

    m, k, cen = isx.wall_map_sharded(trace, None, None, 100, 9, first_ray=50)
    assert seen["args"] == (100, 9, 50) and m.shape == (2, 3) and int(m.sum()) == 15
    assert k == {"binned": 5, "outside": 1, "skipped": 2, "other_surface": 3} and cen["wall_hits"] == 11
