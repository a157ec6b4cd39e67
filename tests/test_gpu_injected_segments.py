"""The disc sweep's binning kernel alone (isx_bin_discs_kernel), on exit segments built to land where traced rays do not
(include/isx.h: isx_bin_injected_segments; tests/edge_segments.py): a disc's rim to 1e-9 cm, the edge of a cluster's ball, the
tube's ends, the ties of the exact test, a pair list that overflows inside the cluster loop -- on cluster shapes from one disc to
4096, staged in LDS (up to 1024 discs) and read from global memory (above).

Every comparison is bit-exact (np.array_equal on uint64).  The reference is the oracle's own C test on every (segment, disc) pair,
brute force (isxo_bin_segments: no cull, no cluster); where a family claims a truth by construction, single-disc calls are held
against that as well.  References are computed once per (list, family) and shared.  What the families must show on the reference
alone -- decisiveness, the culls' edges, the pair counts -- is checked without a GPU in tests/test_injected_segments_cpu.py."""
import numpy as np
import pytest

import disccull_np as DC
import edge_segments as ES

pytestmark = pytest.mark.gpu

OPTION_DEFAULTS = (("disc_pipeline", 1), ("pipeline", 1), ("assist", 1), ("grid_blocks", 0), ("overlap", 0))


@pytest.fixture(autouse=True)
def _default_options(isx):
    for k, v in OPTION_DEFAULTS:
        isx.set_option(k, v)
    yield
    for k, v in OPTION_DEFAULTS:
        isx.set_option(k, v)


_REF = {}


def _oracle(orc, key, ca, r, h, seg):
    """isxo_bin_segments, once per key"""
    if key not in _REF:
        ref = orc.bin_segments(ca, r, h, seg)
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _inject(isx, ca, r, h, seg, **kw):
    return isx.bin_injected_segments(isx.default_config(), ca, r, h, seg, **kw)


def _only_the_binning_kernel_ran(isx):
    single, trace, binning = isx.last_kernel_ms()
    assert binning > 0 and trace == 0 and single == 0, (single, trace, binning)


def _check(isx, orc, key, ca, r, h, seg, **kw):
    ref = _oracle(orc, key, ca, r, h, seg)
    hits, inc = _inject(isx, ca, r, h, seg, **kw)
    bad = np.nonzero(hits != ref)[0]
    assert np.array_equal(hits, ref), (key, len(seg), "discs that differ:", bad[:8].tolist(), "gpu", hits[bad][:8].tolist(),
                                       "oracle", ref[bad][:8].tolist())
    assert inc == int(ref.sum())
    return ref


# ------------------------------------------------------------------ (a) every family on every disc list

@pytest.mark.parametrize("family", ES.FAMILIES)
@pytest.mark.parametrize("lst", ES.LISTS)
def test_parity_with_the_oracle_and_with_the_constructed_truth(isx, orc, lst, family):
    ca, r, h = ES.disc_list(lst)
    seg, tgt, truth = ES.family(lst, family)
    ref = _check(isx, orc, (lst, family), ca, r, h, seg)
    _only_the_binning_kernel_ran(isx)
    assert int(ref.sum()) >= int(truth.sum()) > 0, "the reference side of the comparison is not empty"
    # the constructed truth, pair by pair: a target disc ALONE against the segments aimed at it (first, last and ten between)
    t = np.unique(tgt)
    for k in t[np.unique(np.linspace(0, len(t) - 1, 12).astype(int))]:
        sel = tgt == k
        hits, inc = _inject(isx, ca[k:k + 1], r, h, seg[sel])
        assert int(hits[0]) == inc == int(truth[sel].sum()), (lst, family, int(k), int(hits[0]), int(truth[sel].sum()), int(sel.sum()))


@pytest.mark.parametrize("among", [1, 9])
def test_ties_equal_the_oracle_segment_by_segment(isx, orc, among):
    """No truth is claimed on a tie: a multiply-add contracted on one side and not on the other would show here."""
    ca, r, h, seg = ES.ties() if among == 1 else ES.ties_among(among)
    ref = _check(isx, orc, ("ties", among), ca, r, h, seg)
    assert 0 < int(ref[-1]) < len(seg)
    for k, s in enumerate(seg):
        want = orc.bin_segments(ca, r, h, s[None, :])
        hits, _ = _inject(isx, ca, r, h, s[None, :])
        assert np.array_equal(hits, want), (among, k, s.tolist(), hits.tolist(), want.tolist())


def test_column_overflows_the_pair_list_inside_the_cluster_loop(isx, orc):
    """64 segments x 5 clusters = 320 pairs per batch against a list of 256 that is flushed above 192: the flush inside the loop
    runs in every full batch, and in the batches of 2 to 63 segments that end a region it does not."""
    ca, r, h, seg, counts = ES.column()
    every = np.full(len(ca), len(seg), dtype=np.uint64)
    for kw in ({"region_counts": counts}, {}, {"region_counts": counts, "unit": 0}):
        hits, inc = _inject(isx, ca, r, h, seg, **kw)
        assert np.array_equal(hits, every), (kw, hits.tolist())
        assert inc == len(ca) * len(seg)
    assert np.array_equal(_oracle(orc, "column", ca, r, h, seg), every)


# ------------------------------------------------------------------ (b) staged and unstaged forms

def test_staged_and_unstaged_forms_agree_on_a_shared_prefix(isx, orc):
    """1024 discs are staged in LDS, 1025 are read from global memory; the first 1024 discs are the same discs"""
    ca4, r, h = ES.disc_list("n1024")
    ca5, _, _ = ES.disc_list("n1025")
    seg = np.concatenate([ES.family("n1024", f)[0] for f in ES.FAMILIES])
    a, inc_a = _inject(isx, ca4, r, h, seg)
    b, inc_b = _inject(isx, ca5, r, h, seg)
    assert np.array_equal(a, b[:1024]) and inc_b - inc_a == int(b[1024])
    assert np.array_equal(b, _oracle(orc, "prefix", ca5, r, h, seg)) and int(a.sum()) > 10000


# ------------------------------------------------------------------ (c) work-unit logic

LAYOUTS = {"1": [1], "63": [63], "64": [64], "65": [65], "255_256_257": [255, 256, 257], "1023": [1023], "1024_1": [1024, 1],
           "0_5_0": [0, 5, 0], "one_per_region": [1] * 40, "random40": None}
_MIXED = {}


def _mixed(lst):
    """rim + short segments of a list in one fixed shuffled order"""
    if lst not in _MIXED:
        seg = np.concatenate([ES.family(lst, "rim")[0], ES.family(lst, "short")[0]])
        seg = np.ascontiguousarray(seg[np.random.default_rng(808).permutation(len(seg))][:20000])
        seg.setflags(write=False)
        _MIXED[lst] = seg
    return _MIXED[lst]


def _layout(name):
    if LAYOUTS[name] is not None:
        return LAYOUTS[name]
    counts = np.random.default_rng(909).integers(0, 70, size=40)
    counts[[3, 17]] = 0
    return counts.tolist()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("lst", ["placement", "n1025"])
def test_result_does_not_depend_on_region_layout_or_unit_size(isx, orc, lst, layout):
    ca, r, h = ES.disc_list(lst)
    counts = _layout(layout)
    n = int(np.sum(counts))
    seg = _mixed(lst)[:n]
    for unit in (0, 2, isx.INJECT_UNIT_AUTO):
        _check(isx, orc, (lst, "mixed", n), ca, r, h, seg, region_counts=counts, unit=unit)


@pytest.mark.parametrize("lst", ["placement", "n1025"])
def test_result_does_not_depend_on_segment_order_or_grid_and_two_calls_accumulate(isx, orc, lst):
    ca, r, h = ES.disc_list(lst)
    seg = _mixed(lst)
    ref = _oracle(orc, (lst, "mixed", len(seg)), ca, r, h, seg)
    for unit in (0, 2):
        _check(isx, orc, (lst, "mixed", len(seg)), ca, r, h, seg, unit=unit)
    perm = np.random.default_rng(1010).permutation(len(seg))
    hits, _ = _inject(isx, ca, r, h, seg[perm])
    assert np.array_equal(hits, ref)
    for blocks in (1, 3):
        isx.set_option("grid_blocks", blocks)
        hits, _ = _inject(isx, ca, r, h, seg)
        isx.set_option("grid_blocks", 0)
        assert np.array_equal(hits, ref), blocks
    # two calls accumulate into the caller's histogram; bin_increments is each call's own
    half = len(seg) // 2
    acc = np.zeros_like(ref)
    _, inc1 = _inject(isx, ca, r, h, seg[:half], into=acc)
    first = acc.copy()
    _, inc2 = _inject(isx, ca, r, h, seg[half:], into=acc)
    assert np.array_equal(acc, ref)
    assert inc1 == int(first.sum()) and inc1 + inc2 == int(ref.sum())


@pytest.mark.parametrize("lst", ["placement", "n1025", "coincident"])
def test_kernel_does_not_read_past_a_regions_count(isx, orc, lst):
    """The slots behind a region's count hold a segment through disc 0 along its axis: segments that miss disc 0, in regions that
    are mostly filler, must leave hits[0] at 0."""
    ca, r, h = ES.disc_list(lst)
    seg, tgt, truth = ES.family(lst, "rim")
    miss = seg[~truth]
    miss = miss[::max(1, len(miss) // 400)]                            # the misses of the rim family, from all over the list ...
    seg = miss[~DC.tube_interval(miss, np.broadcast_to(ca[0], (len(miss), 6)), r, h)[2]][:200]   # ... that miss disc 0 too
    assert len(seg) == 200 and int(orc.bin_segments(ca[:1], r, h, seg)[0]) == 0
    for counts in ([1] * len(seg), [63, 0, 65, 2, len(seg) - 130], [len(seg)]):
        for unit in (0, 2):
            hits, inc = _inject(isx, ca, r, h, seg, region_counts=counts, unit=unit)
            assert hits[0] == 0, (lst, counts[:5], unit, int(hits[0]))
            assert np.array_equal(hits, _oracle(orc, (lst, "no_disc0"), ca, r, h, seg))
    # ... and the filler is as loud as the header says: a segment through disc 0 along its axis counts
    loud = np.concatenate([ca[0, :3] - ca[0, 3:], ca[0, 3:], [2.0]])[None, :]
    hits, _ = _inject(isx, ca, r, h, loud)
    assert hits[0] == 1


# ------------------------------------------------------------------ (d) the same code as production

def _sweep_cfg(mod):
    """integratingSphereDetectorSweep.C's sphere (tests/test_gpu_round2.py::_disc_cfg)"""
    c = mod.default_config()
    c.r_out = 105.0; c.reflectance = 1.0; c.roughness_rad = 0.0; c.max_points = 10000
    c.box_half = 200.0; c.src[2] = -80
    return c


@pytest.mark.parametrize("kind", ["default", "sweep"])
def test_injected_traced_segments_give_the_disc_sweep_of_the_same_rays(isx, orc, kind):
    """Status, last point and direction are isx_trace_endstates' own; the start of the last segment, which that call does not
    report, is the oracle's for the same ray -- after the rest of the end state has been seen to be the same, bit for bit."""
    cfg = (lambda m: m.default_config()) if kind == "default" else _sweep_cfg
    n, seed = 20000, 11
    ca = ES.disc_positions()
    status, _, lp, d = isx.trace_endstates(cfg(isx), n, seed)
    ostatus, seg = orc.exit_segments(cfg(orc), n, seed)
    ex = status == isx.abi.RAY_EXITED
    assert np.array_equal(status, ostatus) and np.array_equal(d[ex].view(np.uint64), np.ascontiguousarray(seg[ex, 3:6]).view(np.uint64))
    assert np.abs(seg[ex, :3] + seg[ex, 6:7] * seg[ex, 3:6] - lp[ex]).max() < 1e-9
    want, st = isx.disc_sweep(cfg(isx), ca, ES.R_REF, ES.H_REF, n, seed)
    single, trace, binning = isx.last_kernel_ms()
    assert trace > 0 and binning > 0 and single == 0, "the sweep took the two-kernel route"
    assert ex.sum() == st.exited > 1000
    hits, inc = isx.bin_injected_segments(cfg(isx), ca, ES.R_REF, ES.H_REF, seg[ex])
    assert np.array_equal(hits, want)
    assert inc == st.bin_increments == int(want.sum()) > 0


@pytest.mark.parametrize("lst", ["one", "seven", "nine", "coincident", "n1024", "n1025", "cap4096"])
def test_public_sweep_at_the_cluster_shapes(isx, orc, lst):
    ca, r, h = ES.disc_list(lst)
    n, seed = 30000, 17
    want, ost = orc.disc_sweep(_sweep_cfg(orc), ca, r, h, n, seed)
    hits, st = isx.disc_sweep(_sweep_cfg(isx), ca, r, h, n, seed)
    single, trace, binning = isx.last_kernel_ms()
    assert trace > 0 and binning > 0 and single == 0, ("the sweep took the two-kernel route", single, trace, binning)
    assert np.array_equal(hits, want) and st.bin_increments == ost.bin_increments == int(want.sum()) > 0
    assert st.exited == ost.exited
    isx.set_option("disc_pipeline", 0)
    fused, fst = isx.disc_sweep(_sweep_cfg(isx), ca, r, h, n, seed)
    single, trace, binning = isx.last_kernel_ms()
    isx.set_option("disc_pipeline", 1)
    assert single > 0 and trace == 0 and binning == 0, "... and disc_pipeline = 0 the fused kernel"
    assert np.array_equal(fused, want) and fst.bin_increments == st.bin_increments


# ------------------------------------------------------------------ (e) refusals with a device

def test_entry_refuses_where_the_plan_does_not_choose_the_two_kernel_route(isx, orc):
    ca, r, h = ES.disc_list("nine")
    seg, _, _ = ES.family("nine", "short")
    for key in ("disc_pipeline", "pipeline", "assist"):
        isx.set_option(key, 0)
        with pytest.raises(isx.IsxError) as e:
            _inject(isx, ca, r, h, seg)
        assert e.value.status == isx.abi.ERR_BAD_CONFIG, key
        isx.set_option(key, 1)
    # a list whose tables do not fit the LDS -- 4 B of histogram and 2 B of cluster table per disc beside 18 KiB of per-wave lists:
    # 30 000 discs need 194 KiB of the 160 --: isx_disc_sweep answers with the fused kernel, the entry refuses
    big = ES.cap_discs(30000, 7)
    with pytest.raises(isx.IsxError) as e:
        _inject(isx, big, r, h, seg)
    assert e.value.status == isx.abi.ERR_BAD_CONFIG
    # a border the route does not serve
    c = isx.default_config()
    c.lambertian = 0
    with pytest.raises(isx.IsxError) as e:
        isx.bin_injected_segments(c, ca, r, h, seg)
    assert e.value.status == isx.abi.ERR_BAD_CONFIG
    # ... and the next call is served as if nothing had happened; an empty call is fine
    _check(isx, orc, ("nine", "short"), ca, r, h, seg)
    hits, inc = _inject(isx, ca, r, h, seg[:0])
    assert inc == 0 and not hits.any()
