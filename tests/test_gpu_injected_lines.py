"""The binning kernels alone, on exit lines built to land where traced rays do not (include/isx.h: isx_bin_injected_lines;
tests/edge_lines.py): a detector's rim to within rounding, the |n.V| < 1e-10 parallel cut, the pole row and the phi seam, the
thresholds of the float32 cull, the +-1 ends and the exact bin edges of the exit maps' axes.

Every comparison is bit-exact (np.array_equal on uint64).  The reference of the flux binners is the oracle's own C test
(isxo_bin_lines: isxo_check_intersection on every bin) -- a numpy brute force disagrees with it on lines decided by rounding
(tests/test_injected_lines_cpu.py) --, that of the exit maps and the light field the numpy restatement of their contract.
References are computed once per (grid, family) and shared.  What the families must show on the reference alone (rim lines that
split, a parallel cut with both outcomes, the claimed cull domain) is checked without a GPU in tests/test_injected_lines_cpu.py."""
import numpy as np
import pytest

import edge_lines as EL
import exitmap_np as XM
import lightfield_np as LF

pytestmark = pytest.mark.gpu

DEFAULT, GRIDS, FAMILIES = EL.DEFAULT, EL.GRIDS, EL.FAMILIES
# 36 000 bins, 32 n_theta + 64 n_phi = 18 560 B of tables: the fused kernel's LDS block fits the 160 KiB of gfx950, that of
# isx_bin_lines_kernel (4 KiB of per-wave lists more) does not -- isx_fluxmap answers with the fused kernel
LDS_MISFIT = (180, 200, 40.0, 100.0)
KERNELS = {  # the three flux binners through the options that select them
    "cols": {},
    "slots": {"bin_cols": 0},
    "lines256": {"bin_slots": 0, "bin_block": 256},
    "lines512": {"bin_slots": 0, "bin_block": 512},
    "lines1024": {"bin_slots": 0, "bin_block": 1024},
}
OPTION_DEFAULTS = (("bin_cols", 1), ("bin_slots", 1), ("bin_block", 512), ("bin_blocks_per_cu", 0), ("grid_blocks", 0),
                   ("lf_global", 0), ("bin_mode", 1), ("pipeline", 1), ("assist", 1), ("surface_pipeline", 1), ("overlap", 0))


@pytest.fixture(autouse=True)
def _default_options(isx):
    for k, v in OPTION_DEFAULTS:
        isx.set_option(k, v)
    yield
    for k, v in OPTION_DEFAULTS:
        isx.set_option(k, v)


def _cfg(mod, grid, kind="default"):
    c = mod.default_config()
    c.n_theta, c.n_phi, c.det_diameter, c.det_distance = grid
    if kind == "brdf":
        c.source_model = 1
    elif kind == "compat":
        c.hit_line_mode = 1
    return c


_FAM, _REF = {}, {}


def _family(orc, grid, name):
    if grid not in _FAM:
        fam = EL.families(_cfg(orc, grid))
        for P, V in fam.values():
            P.setflags(write=False); V.setflags(write=False)
        _FAM[grid] = fam
    return _FAM[grid][name]


def _oracle(orc, grid, key, P, V, kind="default"):
    """isxo_bin_lines of the lines, once per (grid, key)"""
    k = (grid, key, kind)
    if k not in _REF:
        h = orc.bin_lines(_cfg(orc, grid, kind), P, V)
        h.setflags(write=False)
        _REF[k] = h
    return _REF[k]


def _flux(isx, grid, P, V, kind="default", **kw):
    hits, _, _, inc = isx.bin_injected_lines(_cfg(isx, grid, kind), isx.INJECT_FLUX, P, V, **kw)
    return hits, inc


def _check_family(isx, orc, grid, name):
    P, V = _family(orc, grid, name)
    ref = _oracle(orc, grid, name, P, V)
    hits, inc = _flux(isx, grid, P, V)
    assert int(ref.sum()) > 0 or grid[:2] == (1, 1), "the reference side of the comparison is not empty"
    diff = np.argwhere(hits != ref)
    assert np.array_equal(hits, ref), (grid, name, len(P), "bins that differ (row, column):", diff[:8].tolist(),
                                       "gpu", hits[hits != ref][:8].tolist(), "oracle", ref[hits != ref][:8].tolist())
    assert inc == int(ref.sum())


# ------------------------------------------------------------------ (a) flux parity: every family, every kernel, every grid

@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_flux_parity_default_grid(isx, orc, kernel, family):
    for k, v in KERNELS[kernel].items():
        isx.set_option(k, v)
    _check_family(isx, orc, DEFAULT, family)
    assert isx.last_kernel_ms()[2] > 0 and isx.last_kernel_ms()[1] == 0, "a binning kernel ran, no trace kernel"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d_d%g_R%g" % g)
def test_flux_parity_further_grids(isx, orc, grid, family):
    _check_family(isx, orc, grid, family)


def test_grid_whose_histogram_does_not_fit_the_binners_lds_is_refused(isx, orc):
    """isx.h: where the plan has no binning kernel for the call -- here the fused kernel answers isx_fluxmap -- the entry
    refuses with ISX_ERR_BAD_CONFIG; it never routes to another kernel."""
    P, V = _family(orc, DEFAULT, "through_O")
    with pytest.raises(isx.IsxError) as e:
        _flux(isx, LDS_MISFIT, P, V)
    assert e.value.status == isx.abi.ERR_BAD_CONFIG
    hits, st = isx.fluxmap(_cfg(isx, LDS_MISFIT), 2000, 3)
    single, trace, binning = isx.last_kernel_ms()
    assert single > 0 and trace == 0 and binning == 0, "isx_fluxmap of this grid is the fused kernel's"
    assert int(hits.sum()) == st.bin_increments > 0
    for key in ("pipeline", "bin_mode"):          # ... and so do the switches that take the pipeline away
        isx.set_option(key, 0)
        with pytest.raises(isx.IsxError) as e:
            _flux(isx, DEFAULT, P, V)
        assert e.value.status == isx.abi.ERR_BAD_CONFIG
        isx.set_option(key, 1)


# ------------------------------------------------------------------ (b) work-unit logic

LAYOUTS = {"1": [1], "63": [63], "64": [64], "65": [65], "255_256_257": [255, 256, 257], "1023": [1023], "1024_1": [1024, 1],
           "0_5_0": [0, 5, 0], "random40": None}


def _mixed(orc):
    """bulk + tangent lines of the default grid in one fixed shuffled order"""
    if "mixed" not in _FAM:
        (bp, bv), (tp, tv) = _family(orc, DEFAULT, "bulk"), _family(orc, DEFAULT, "tangent")
        P, V = np.concatenate([bp, tp]), np.concatenate([bv, tv])
        order = np.random.default_rng(808).permutation(len(P))
        P, V = P[order], V[order]
        P.setflags(write=False); V.setflags(write=False)
        _FAM["mixed"] = (P, V)
    return _FAM["mixed"]


def _layout(name, n_max):
    if LAYOUTS[name] is not None:
        return LAYOUTS[name]
    counts = np.random.default_rng(909).integers(0, 70, size=40)
    counts[[3, 17]] = 0
    assert counts.sum() <= n_max
    return counts.tolist()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("kernel", ["cols", "slots", "lines512"])
def test_result_does_not_depend_on_region_layout_or_unit_size(isx, orc, kernel, layout):
    for k, v in KERNELS[kernel].items():
        isx.set_option(k, v)
    P, V = _mixed(orc)
    counts = _layout(layout, len(P))
    n = int(np.sum(counts))
    ref = _oracle(orc, DEFAULT, ("mixed", n), P[:n], V[:n])
    for unit in (0, 2, isx.INJECT_UNIT_AUTO):
        hits, inc = _flux(isx, DEFAULT, P[:n], V[:n], region_counts=counts, unit=unit)
        assert np.array_equal(hits, ref), (kernel, layout, unit, int(hits.sum()), int(ref.sum()))
        assert inc == int(ref.sum())


@pytest.mark.parametrize("kernel", ["cols", "slots", "lines512"])
def test_result_does_not_depend_on_line_order_or_grid_and_two_calls_accumulate(isx, orc, kernel):
    for k, v in KERNELS[kernel].items():
        isx.set_option(k, v)
    P, V = _mixed(orc)
    ref = _oracle(orc, DEFAULT, ("mixed", len(P)), P, V)
    for unit in (0, 2):
        hits, inc = _flux(isx, DEFAULT, P, V, unit=unit)
        assert np.array_equal(hits, ref) and inc == int(ref.sum()), unit
    perm = np.random.default_rng(1010).permutation(len(P))
    hits, _ = _flux(isx, DEFAULT, P[perm], V[perm])
    assert np.array_equal(hits, ref)
    isx.set_option("grid_blocks", 1)
    hits, _ = _flux(isx, DEFAULT, P, V)
    isx.set_option("grid_blocks", 0)
    assert np.array_equal(hits, ref)
    # two calls accumulate into the caller's histogram; bin_increments is each call's own
    half = len(P) // 2
    acc = np.zeros_like(ref)
    _, _, _, inc1 = isx.bin_injected_lines(_cfg(isx, DEFAULT), isx.INJECT_FLUX, P[:half], V[:half], into=(acc, None, None))
    first = acc.copy()
    _, _, _, inc2 = isx.bin_injected_lines(_cfg(isx, DEFAULT), isx.INJECT_FLUX, P[half:], V[half:], into=(acc, None, None))
    assert np.array_equal(acc, ref)
    assert inc1 == int(first.sum()) and inc1 + inc2 == int(ref.sum())


# ------------------------------------------------------------------ (c) the same code as production

N_TRACED, SEED = 20000, 11
_TRACED = {}


def _traced(isx, kind):
    """the counted lines of the GPU's own trace_endstates, once per configuration"""
    if kind not in _TRACED:
        c = _cfg(isx, DEFAULT, kind)
        st, _, lp, d = isx.trace_endstates(c, N_TRACED, SEED)
        sel = (st == isx.abi.RAY_EXITED) & (lp[:, 2] < c.exit_port_z)
        P, V = lp[sel].copy(), d[sel].copy()
        P.setflags(write=False); V.setflags(write=False)
        _TRACED[kind] = (P, V)
    return _TRACED[kind]


@pytest.mark.parametrize("kind", ["default", "brdf", "compat"])
def test_injected_traced_lines_give_the_flux_map_of_the_same_rays(isx, kind):
    P, V = _traced(isx, kind)
    c = _cfg(isx, DEFAULT, kind)
    want, st = isx.fluxmap(c, N_TRACED, SEED)
    assert len(P) == st.counted_below_z > 1000
    hits, inc = _flux(isx, DEFAULT, P, V, kind=kind)
    assert np.array_equal(hits, want)
    assert inc == st.bin_increments == int(want.sum())


def _map_spec(isx, n_u, n_v, n_x, n_y, plane_z=-100.0, half=20.0):
    s = isx.default_exit_map_spec(isx.default_config())
    s.n_u, s.n_v, s.n_x, s.n_y, s.plane_z, s.half_extent = n_u, n_v, n_x, n_y, plane_z, half
    return s


@pytest.mark.parametrize("kind", ["default", "brdf", "compat"])
def test_injected_traced_lines_give_the_exit_maps_and_the_light_field_of_the_same_rays(isx, kind):
    P, V = _traced(isx, kind)
    c = _cfg(isx, DEFAULT, kind)
    spec = _map_spec(isx, 32, 24, 16, 20)
    dmap, pmap, k, st = isx.exit_maps(c, N_TRACED, SEED, spec)
    a, b, cnt, inc = isx.bin_injected_lines(c, isx.INJECT_EXIT_MAPS, P, V, spec=spec)
    assert np.array_equal(a, dmap) and np.array_equal(b, pmap)
    assert cnt.tolist() == [getattr(k, f) for f in XM.COUNT_FIELDS]
    assert inc == st.bin_increments == k.dir_binned + k.pos_binned
    spec = _map_spec(isx, 8, 6, 5, 7)
    field, k, st = isx.light_field(c, N_TRACED, SEED, spec)
    a, _, cnt, inc = isx.bin_injected_lines(c, isx.INJECT_LIGHT_FIELD, P, V, spec=spec)
    assert np.array_equal(a, field)
    assert cnt.tolist() == [getattr(k, f) for f in LF.COUNT_FIELDS]
    assert inc == st.bin_increments == k.binned


# ------------------------------------------------------------------ (d) exit maps and light field at their edges

def _edge_and_bulk(orc, spec):
    """the hand-made edge family of the spec + the bulk lines (any doubles: these sinks define NaN and inf as outside)"""
    ep, ev = EL.exit_edge_lines(spec)
    bp, bv = _family(orc, DEFAULT, "bulk")
    return np.concatenate([ep, bp]), np.concatenate([ev, bv])


# (n_u, n_v, n_x, n_y): both maps; the plane map alone and the direction map alone (0 x 0 = not wanted); one-bin axes
EXIT_SPECS = [(8, 6, 5, 7), (0, 0, 5, 7), (8, 6, 0, 0), (1, 1, 1, 1), (128, 128, 64, 64)]


@pytest.mark.parametrize("axes", EXIT_SPECS, ids=lambda a: "%dx%d_%dx%d" % a)
def test_exit_maps_at_the_edges_against_the_restatement(isx, orc, axes):
    spec = _map_spec(isx, *axes)
    P, V = _edge_and_bulk(orc, spec)
    n = len(P)
    rng = np.random.default_rng(1111)
    for counts in (None, rng.multinomial(n, np.ones(12) / 12).tolist()):
        a, b, cnt, inc = isx.bin_injected_lines(isx.default_config(), isx.INJECT_EXIT_MAPS, P, V, spec=spec, region_counts=counts)
        want = dict.fromkeys(XM.COUNT_FIELDS, 0)
        if spec.n_u:
            dmap, want["dir_binned"], want["dir_outside"] = XM.direction_map(V, spec.n_u, spec.n_v)
            assert np.array_equal(a, dmap)
            assert want["dir_binned"] + want["dir_outside"] == n and want["dir_outside"] > 0
        if spec.n_x:
            pmap, want["pos_binned"], want["pos_outside"], want["upward"] = XM.plane_map(P, V, spec.n_x, spec.n_y, spec.plane_z,
                                                                                           spec.half_extent)
            assert np.array_equal(b, pmap)
            assert want["pos_binned"] + want["pos_outside"] + want["upward"] == n
            assert want["pos_outside"] > 0 and want["upward"] > 0
        assert cnt.tolist() == [want[f] for f in XM.COUNT_FIELDS]
        assert inc == want["dir_binned"] + want["pos_binned"]


# (n_u, n_v, n_x, n_y), lf_global: the LDS form, the global form of the same field, a field too large for the LDS
FIELD_CASES = [((8, 6, 5, 7), 0), ((8, 6, 5, 7), 1), ((1, 1, 1, 1), 0), ((16, 16, 16, 16), 0)]


@pytest.mark.parametrize("axes,lf_global", FIELD_CASES, ids=lambda a: str(a).replace(" ", ""))
def test_light_field_at_the_edges_against_the_restatement(isx, orc, axes, lf_global):
    isx.set_option("lf_global", lf_global)
    spec = _map_spec(isx, *axes)
    P, V = _edge_and_bulk(orc, spec)
    want, k = LF.light_field(P, V, spec.n_u, spec.n_v, spec.n_x, spec.n_y, spec.plane_z, spec.half_extent)
    assert sum(k.values()) == len(P) and k["upward"] > 0 and k["pos_outside"] > 0 and k["binned"] > 0
    field, _, cnt, inc = isx.bin_injected_lines(isx.default_config(), isx.INJECT_LIGHT_FIELD, P, V, spec=spec)
    assert np.array_equal(field, want)
    assert cnt.tolist() == [k[f] for f in LF.COUNT_FIELDS]
    assert int(cnt.sum()) == len(P) and inc == k["binned"]
