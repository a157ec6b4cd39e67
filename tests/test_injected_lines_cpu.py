"""What tests/test_gpu_injected_lines.py rests on, checked without a GPU, on the reference alone:

  * decisiveness -- the edge families (tests/edge_lines.py) do land on the edges: rim lines at eps = 0 split, |eps| >= 1e-12
    decides, the parallel family hits iff the oracle's own |dot| >= 1e-10, both ways;
  * the cull domain -- both numpy restatements of the binners' pre-selection (boxwin_np, bandwin_np) hold every hit of every
    family on every grid the GPU file uses, and hand no bin out twice;
  * isxo_bin_lines -- the oracle entry the GPU file compares against equals isxo_fluxmap on the counted rays of a trace;
  * the refusals of isx_bin_injected_lines, all answered before a device is asked for;
  * exitmap_np / lightfield_np against the header's contract, written out per line in plain Python, on the hand-made edge family.

Conditions, not measurements: the decisiveness bounds come from the issue that asked for these tests (between 1/4 and 3/4 at
eps = 0, all one way from 1e-12 on, at least 20 of either outcome on the parallel cut); the seeds of edge_lines.py are chosen so that
the oracle alone meets them.  The counts are printed (pytest -s)."""
import ctypes as C
import math

import numpy as np
import pytest

import bandwin_np
import boxwin_np
import edge_lines as EL
import exitmap_np as XM
import lightfield_np as LF
from edge_lines import DEFAULT, GRIDS, FAMILIES

ALL_GRIDS = [DEFAULT] + GRIDS
_ids = lambda g: "%dx%d_d%g_R%g" % g


def _cfg(mod, grid):
    c = mod.default_config()
    c.n_theta, c.n_phi, c.det_diameter, c.det_distance = grid
    return c


def _target_hits(orc, c, P, V, tgt):
    tab = orc.detector_table(c)
    return np.array([orc.check_intersection(tab[k], c.det_diameter, p, v) for p, v, k in zip(P, V, tgt)], dtype=bool), tab


# ------------------------------------------------------------------ decisiveness

@pytest.mark.parametrize("grid", ALL_GRIDS, ids=_ids)
def test_rim_lines_split_at_zero_offset_and_are_decided_from_1e12_on(orc, grid):
    c = _cfg(orc, grid)
    P, V, tgt, eps = EL.tangent_lines(c)
    hit, _ = _target_hits(orc, c, P, V, tgt)
    counts = {e: (int(hit[eps == e].sum()), int((eps == e).sum())) for e in EL.TANGENT_EPS}
    print("tangent", grid, "target-bin hits (of lines) by eps:", counts)
    nt, nph = grid[0], grid[1]
    assert {0, nph - 1, (nt - 1) * nph, nt * nph - 1} <= set(tgt.tolist()), "rows 0, n_theta - 1 and columns 0, n_phi - 1 are targets"
    for e, (h, n) in counts.items():
        assert n >= 200
        if e == 0.0:
            assert n / 4 <= h <= 3 * n / 4, "eps = 0 is decided by rounding alone"
        elif abs(e) >= 1e-12:
            assert h == (n if e < 0 else 0), e


@pytest.mark.parametrize("grid", ALL_GRIDS, ids=_ids)
def test_parallel_lines_hit_iff_the_oracles_own_dot_passes_the_cut(orc, grid):
    c = _cfg(orc, grid)
    P, V, tgt, delta = EL.parallel_lines(c)
    hit, tab = _target_hits(orc, c, P, V, tgt)
    n = tab[tgt, 3:]
    dot = V[:, 0] * n[:, 0] + V[:, 1] * n[:, 1] + V[:, 2] * n[:, 2]      # isxo_check_intersection's own expression, left to right
    want = np.abs(dot) >= 1e-10
    print("parallel", grid, "lines", len(P), "hit", int(hit.sum()), "cut", int((~want).sum()),
          "by delta:", {d: int(hit[delta == d].sum()) for d in EL.PARALLEL_DELTA})
    assert np.array_equal(hit, want)
    assert hit.sum() >= 20 and (~hit).sum() >= 20
    # (within 1e-6 of the cut the rounding of the oracle's own dot product decides: both outcomes occur on either side)
    near = np.isin(delta, (1e-10 * (1 - 1e-6), -1e-10 * (1 - 1e-6), 1e-10 * (1 + 1e-6), -1e-10 * (1 + 1e-6)))
    assert near.sum() >= 16 and not hit[np.abs(delta) <= 5e-11].any() and hit[np.abs(delta) >= 2e-10].all()


# ------------------------------------------------------------------ the claimed cull domain

@pytest.mark.parametrize("grid", ALL_GRIDS, ids=_ids)
def test_every_family_lies_in_the_cull_domain_of_both_restatements(orc, grid):
    c = _cfg(orc, grid)
    fam = EL.families(c)
    assert sorted(fam) == sorted(FAMILIES)
    for name, (P, V) in fam.items():
        box, band = boxwin_np.check(c, P, V), bandwin_np.check(c, P, V)
        print("cull", grid, name, "lines", len(P), "hits", box["hits"], "box missed/twice", box["missed"], box["twice"],
              "band missed/twice", band["missed"], band["twice"], "kinds", {k: v["lines"] for k, v in band["by_kind"].items()})
        assert box["missed"] == 0 and box["twice"] == 0, (grid, name, "box windows")
        assert band["missed"] == 0 and band["twice"] == 0, (grid, name, "column slots")


def test_cap_rows_of_a_meridian_perpendicular_to_a_wide_caps_axis(orc):
    """What the injected families found (docs/LOG.md): cap_rows gave a column NO rows when the cap's axis is perpendicular to the
    plane of the column's meridian (rho2 = a^2 + b^2 <= 1e-12) -- right for a cap narrower than a hemisphere, every point of the
    meridian being at 90 degrees from the axis, wrong for the wide cap about h^ of a grazing line (cos w <= 0), which holds the
    whole meridian.  Seen with exactly vertical lines through O on a band grid (the stand-in for h^ is e_x: the columns at 90 and
    270 degrees) and with nearly vertical lines whose foot lies in the azimuth of a column of a 4-column grid."""
    f32 = np.float32
    c32, s32 = np.array([6.1e-17, 1.0, 0.70710678], f32), np.array([1.0, 0.0, 0.70710678], f32)
    for cosw, want in ((f32(-1.0), 17), (f32(-0.5), 17), (f32(0.0), 17), (f32(0.5), 0)):
        ilo, cnt = bandwin_np.cap_rows(f32(1.0), f32(0.0), f32(0.0), cosw, c32, s32, f32(17 * 0.63661977237), 17)
        assert cnt[0] == want and (want == 0 or ilo[0] == 0), (cosw, ilo, cnt)
        assert cnt[1] > 0                                                                      # the column the axis lies in
    # the lines themselves, against the exact test: a band grid, the exactly vertical line through O
    c = _cfg(orc, (180, 90, 176.0, 100.0))
    r = bandwin_np.check(c, np.array([[0.0, 0.0, c.exit_port_z + 120.0]]), np.array([[0.0, 0.0, -1.0]]))
    assert r["by_kind"]["band"]["lines"] == 1 and r["hits"] > 10000 and r["missed"] == 0 and r["twice"] == 0


# ------------------------------------------------------------------ isxo_bin_lines

def _pin_case(orc, kind):
    c = orc.default_config()
    if kind == "brdf":
        c.source_model = 1
    elif kind == "compat":
        c.hit_line_mode = 1
    elif kind == "coarse":
        c.n_theta, c.n_phi, c.det_diameter = 7, 3, 60.0
    return c


@pytest.mark.parametrize("kind", ["default", "brdf", "compat", "coarse"])
def test_oracle_bin_lines_equals_the_flux_map_on_the_counted_rays_of_a_trace(orc, kind):
    c = _pin_case(orc, kind)
    n, seed = 4000, 21
    st, _, lp, d = orc.trace_endstates(c, n, seed)
    sel = (st == 1) & (lp[:, 2] < c.exit_port_z)
    want, stats = orc.fluxmap(c, n, seed)
    assert sel.sum() == stats.counted_below_z > 500
    got = orc.bin_lines(c, lp[sel], d[sel])
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert int(got.sum()) == stats.bin_increments > 0
    assert np.array_equal(orc.bin_lines(c, lp[sel], d[sel], nthreads=1), want)
    # the traced lines are in the injected entry's flux domain (unit directions, points inside the world box)
    assert np.abs(np.linalg.norm(d[sel], axis=1) - 1.0).max() <= 1e-12 and np.linalg.norm(lp[sel], axis=1).max() <= np.sqrt(3.0) * c.box_half


# ------------------------------------------------------------------ the entry's refusals, without a device

@pytest.fixture(scope="module")
def mod():
    import altair_raytracing_amd as m
    m.load()
    return m


def _call(mod, cfg, sink, lines, n=None, spec=None, counts=None, n_regions=None, unit=-1, out_a=True, out_b=True, k=True):
    u64, dbl = C.c_uint64, C.c_double
    lines = None if lines is None else np.ascontiguousarray(lines, dtype=np.float64)
    a = np.zeros(1 << 16, dtype=np.uint64); b = np.zeros(1 << 16, dtype=np.uint64); kk = np.zeros(8, dtype=np.uint64)
    rc_arr = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
    inc = u64(0)
    p = lambda x, t: x.ctypes.data_as(C.POINTER(t))
    return mod.load().isx_bin_injected_lines(
        C.byref(cfg) if cfg is not None else None, sink, C.byref(spec) if spec is not None else None,
        p(lines, dbl) if lines is not None else None, len(lines) if n is None else n,
        p(rc_arr, C.c_uint32) if rc_arr is not None else None, (0 if rc_arr is None else rc_arr.size) if n_regions is None else n_regions,
        unit, p(a, u64) if out_a else None, p(b, u64) if out_b else None, p(kk, u64) if k else None, C.byref(inc))


def test_entry_refusals_need_no_device(mod):
    A = mod.abi
    c = mod.default_config()
    good = np.array([[0.0, 0.0, -50.0, 0.0, 0.0, -1.0], [10.0, 0.0, -60.0, 0.6, 0.0, -0.8]])
    spec = mod.default_exit_map_spec(c)
    passed = (A.OK, A.ERR_NO_DEVICE, A.ERR_NOT_INIT)      # every refusal is behind us: the device is asked for next
    assert _call(mod, c, A.INJECT_FLUX, good) in passed
    assert _call(mod, c, A.INJECT_FLUX, good, counts=[1, 0, 1]) in passed
    assert _call(mod, c, A.INJECT_EXIT_MAPS, good, spec=spec) in passed
    assert _call(mod, c, A.INJECT_LIGHT_FIELD, good, spec=mod.default_light_field_spec(c)) in passed
    # NULL pointers
    assert _call(mod, None, A.INJECT_FLUX, good) == A.ERR_BAD_ARG
    assert _call(mod, c, A.INJECT_FLUX, None, n=2) == A.ERR_BAD_ARG
    assert _call(mod, c, A.INJECT_FLUX, good, out_a=False) == A.ERR_BAD_ARG
    assert _call(mod, c, A.INJECT_EXIT_MAPS, good, spec=None) == A.ERR_BAD_ARG
    assert _call(mod, c, A.INJECT_EXIT_MAPS, good, spec=spec, k=False) == A.ERR_BAD_ARG
    assert _call(mod, c, A.INJECT_EXIT_MAPS, good, spec=spec, out_b=False) == A.ERR_BAD_ARG
    assert _call(mod, c, A.INJECT_LIGHT_FIELD, good, spec=mod.default_light_field_spec(c), out_a=False) == A.ERR_BAD_ARG
    # sink, unit, n
    for sink in (-1, 3):
        assert _call(mod, c, sink, good) == A.ERR_BAD_ARG
    for unit in (-2, 1, 3):
        assert _call(mod, c, A.INJECT_FLUX, good, unit=unit) == A.ERR_BAD_ARG
    assert _call(mod, c, A.INJECT_FLUX, good, n=A.INJECT_MAX_LINES + 1) == A.ERR_TOO_LARGE
    # region layouts: a count above a region, counts that do not sum to n, region numbers out of range
    assert _call(mod, c, A.INJECT_FLUX, good, counts=[2, 1025], n=2) == A.ERR_BAD_ARG
    assert _call(mod, c, A.INJECT_FLUX, good, counts=[1, 2]) == A.ERR_BAD_ARG
    assert _call(mod, c, A.INJECT_FLUX, good, counts=[1]) == A.ERR_BAD_ARG
    assert _call(mod, c, A.INJECT_FLUX, good, counts=[1, 1], n_regions=0) == A.ERR_BAD_ARG
    assert _call(mod, c, A.INJECT_FLUX, good, counts=[1, 1], n_regions=A.INJECT_MAX_REGIONS + 1) == A.ERR_BAD_ARG
    assert _call(mod, c, A.INJECT_FLUX, good, counts=None, n_regions=2) == A.ERR_BAD_ARG
    # config and spec
    bad = c.copy(); bad.struct_size = 0
    assert _call(mod, bad, A.INJECT_FLUX, good) == A.ERR_BAD_CONFIG
    bad = c.copy(); bad.n_theta = 0
    assert _call(mod, bad, A.INJECT_FLUX, good) == A.ERR_BAD_CONFIG
    bad = c.copy(); bad.n_theta, bad.n_phi = 400, 400
    assert _call(mod, bad, A.INJECT_FLUX, good) == A.ERR_BAD_CONFIG
    s = spec.copy(); s.n_u = 2000
    assert _call(mod, c, A.INJECT_EXIT_MAPS, good, spec=s) == A.ERR_BAD_CONFIG
    s = spec.copy(); s.half_extent = 0.0
    assert _call(mod, c, A.INJECT_EXIT_MAPS, good, spec=s) == A.ERR_BAD_CONFIG
    s = mod.default_light_field_spec(c); s.n_x = 0
    assert _call(mod, c, A.INJECT_LIGHT_FIELD, good, spec=s) == A.ERR_BAD_CONFIG
    # the flux sink's domain: finite coordinates, unit directions, points within the world box's reach, sqrt(3) box_half
    for k in range(6):
        for v in (np.nan, np.inf, -np.inf):
            l = good.copy(); l[1, k] = v
            assert _call(mod, c, A.INJECT_FLUX, l) == A.ERR_BAD_ARG, (k, v)
    for scale in (1 + 1e-11, 1 - 1e-11, 0.0, 2.0):
        l = good.copy(); l[1, 3:] *= scale
        assert _call(mod, c, A.INJECT_FLUX, l) == A.ERR_BAD_ARG, scale
    l = good.copy(); l[1, 3:] *= 1 + 2e-13
    assert _call(mod, c, A.INJECT_FLUX, l) in passed
    l = good.copy(); l[0, :3] = (0.0, math.sqrt(3.0) * c.box_half * (1 + 1e-9), 0.0)
    assert _call(mod, c, A.INJECT_FLUX, l) == A.ERR_BAD_ARG
    l = good.copy(); l[0, :3] = (0.0, math.sqrt(3.0) * c.box_half * 0.999, 0.0)
    assert _call(mod, c, A.INJECT_FLUX, l) in passed
    # ... which the exit-map and light-field sinks do not have: NaN and inf are "outside" by their contract
    l = good.copy(); l[0, 0] = np.nan; l[1, 5] = -np.inf
    assert _call(mod, c, A.INJECT_EXIT_MAPS, l, spec=spec) in passed
    assert _call(mod, c, A.INJECT_LIGHT_FIELD, l, spec=mod.default_light_field_spec(c)) in passed


# ------------------------------------------------------------------ the restatements against the header, line by line

def _floor_bin(f, n):
    """(int)floor(f) where 0 <= . < n, else None (NaN and inf included)"""
    if f != f or f in (math.inf, -math.inf):
        return None
    i = math.floor(f)
    return i if 0 <= i < n else None


def _div(a, b):
    """IEEE a / b for b != 0 or not (Python raises where C gives inf / NaN)"""
    return float(np.float64(a) / np.float64(b))


def _header_exit_maps(P, V, n_u, n_v, n_x, n_y, plane_z, half):
    """include/isx.h, isx_exit_maps, as written: one line at a time, Python floats (IEEE double, no fma)"""
    dmap, pmap = np.zeros((n_v, n_u), np.uint64), np.zeros((n_y, n_x), np.uint64)
    k = dict.fromkeys(XM.COUNT_FIELDS, 0)
    with np.errstate(all="ignore"):
        for p, v in zip(P.tolist(), V.tolist()):
            if n_u:
                iu, iv = _floor_bin((v[0] + 1.0) * 0.5 * n_u, n_u), _floor_bin((v[1] + 1.0) * 0.5 * n_v, n_v)
                if iu is not None and iv is not None:
                    dmap[iv, iu] += 1; k["dir_binned"] += 1
                else:
                    k["dir_outside"] += 1
            if n_x:
                if not v[2] < 0.0:
                    k["upward"] += 1
                    continue
                t = _div(plane_z - p[2], v[2])
                x, y = p[0] + t * v[0], p[1] + t * v[1]
                ix, iy = _floor_bin(_div(x + half, 2.0 * half) * n_x, n_x), _floor_bin(_div(y + half, 2.0 * half) * n_y, n_y)
                if ix is not None and iy is not None:
                    pmap[iy, ix] += 1; k["pos_binned"] += 1
                else:
                    k["pos_outside"] += 1
    return dmap, pmap, k


def _header_light_field(P, V, n_u, n_v, n_x, n_y, plane_z, half):
    field = np.zeros((n_y, n_x, n_v, n_u), np.uint64)
    k = dict.fromkeys(LF.COUNT_FIELDS, 0)
    with np.errstate(all="ignore"):
        for p, v in zip(P.tolist(), V.tolist()):
            if not v[2] < 0.0:
                k["upward"] += 1
                continue
            t = _div(plane_z - p[2], v[2])
            x, y = p[0] + t * v[0], p[1] + t * v[1]
            ix, iy = _floor_bin(_div(x + half, 2.0 * half) * n_x, n_x), _floor_bin(_div(y + half, 2.0 * half) * n_y, n_y)
            if ix is None or iy is None:
                k["pos_outside"] += 1
                continue
            iu, iv = _floor_bin((v[0] + 1.0) * 0.5 * n_u, n_u), _floor_bin((v[1] + 1.0) * 0.5 * n_v, n_v)
            if iu is None or iv is None:
                k["dir_outside"] += 1
                continue
            field[iy, ix, iv, iu] += 1; k["binned"] += 1
    return field, k


class _Spec:
    def __init__(self, n_u, n_v, n_x, n_y, plane_z=-100.0, half_extent=20.0):
        self.n_u, self.n_v, self.n_x, self.n_y, self.plane_z, self.half_extent = n_u, n_v, n_x, n_y, plane_z, half_extent


@pytest.mark.parametrize("axes", [(8, 6, 5, 7), (1, 1, 1, 1), (128, 128, 64, 64), (3, 5, 1024, 2)])
def test_restatements_agree_with_the_header_on_the_edge_family(axes):
    s = _Spec(*axes)
    P, V = EL.exit_edge_lines(s)
    n = len(P)
    dmap, pmap, k = _header_exit_maps(P, V, s.n_u, s.n_v, s.n_x, s.n_y, s.plane_z, s.half_extent)
    d, db, do = XM.direction_map(V, s.n_u, s.n_v)
    pm, pb, po, up = XM.plane_map(P, V, s.n_x, s.n_y, s.plane_z, s.half_extent)
    assert np.array_equal(d, dmap) and np.array_equal(pm, pmap)
    assert (db, do, pb, po, up) == tuple(k[f] for f in XM.COUNT_FIELDS)
    assert db + do == n == pb + po + up
    field, kf = _header_light_field(P, V, s.n_u, s.n_v, s.n_x, s.n_y, s.plane_z, s.half_extent)
    f, kk = LF.light_field(P, V, s.n_u, s.n_v, s.n_x, s.n_y, s.plane_z, s.half_extent)
    assert np.array_equal(f, field) and kk == kf and sum(kk.values()) == n
    # the family does what it is for: every class of the contract occurs
    assert do >= 4 and po >= 10 and up >= 6 and db > 0 and pb > 0 and kf["dir_outside"] > 0 and kf["binned"] > 0
    # exactly -1 is bin 0, exactly +1 is outside; an exact edge opens the bin above (8 and 4 bins: the edges are exact in binary)
    e = np.array([[-1.0, -1.0, -0.5], [1.0, 0.0, -0.5], [-0.75, -0.5, -0.5], [0.75, 0.5, -0.5]])
    m, b, o = XM.direction_map(e, 8, 4)
    assert (b, o) == (3, 1) and m[0, 0] == 1 and m[1, 1] == 1 and m[3, 7] == 1
    # -0.0, +0.0 are upward; -1e-300 and -1e-17 point down (their crossing is far outside or, from the plane itself, the point)
    z = np.array([[0.3, -0.2, -0.0], [0.3, -0.2, 0.0], [0.3, -0.2, -1e-300], [0.3, -0.2, -1e-17]])
    on_plane = np.tile([0.0, 0.0, s.plane_z], (4, 1))
    _, b, o, u = XM.plane_map(on_plane, z, s.n_x, s.n_y, s.plane_z, s.half_extent)
    assert (b, o, u) == (2, 0, 2)
