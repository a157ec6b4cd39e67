"""What tests/test_gpu_injected_segments.py rests on, checked without a GPU, on the reference alone:

  * decisiveness -- the rim and short families (tests/edge_segments.py) are decided by the oracle as constructed, for every
    segment at every listed offset: delta > 0 a hit, delta < 0 a miss, down to 1e-9 cm; a cut 1e-6 cm before the tube a miss, one
    1e-6 cm inside it a hit;
  * the families reach the culls' edges -- with the kernel's margins neither numpy restatement (tests/disccull_np.py) of the
    binary32 pre-selection and of the binary64 cull drops a hit of any family on any disc list; with the binary32 margins taken
    away (1.0 and 0.0) the pre-selection drops at least 100 hits of cluster_rim on a placement of the sweep's kind;
  * isxo_bin_segments -- the oracle entry the GPU file compares against equals isxo_disc_sweep on the exit segments of a trace;
  * the refusals of isx_bin_injected_segments, all answered before a device is asked for;
  * the numpy cluster table against its properties.

Conditions, not measurements: the bounds come from the issue that asked for these tests and from the construction; the seeds of
edge_segments.py are such that the oracle alone meets them.  The counts are printed (pytest -s)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import disccull_np as DC
import edge_segments as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _per_target_hits(orc, ca, r, h, seg, tgt):
    """hits of (seg[k], disc tgt[k]) summed per target disc -- one single-disc call of the oracle per target -- and the
    segments aimed at it"""
    got, aimed = {}, {}
    for k in np.unique(tgt):
        sel = tgt == k
        got[int(k)] = int(orc.bin_segments(ca[k:k + 1], r, h, seg[sel])[0])
        aimed[int(k)] = sel
    return got, aimed


# ------------------------------------------------------------------ decisiveness

@pytest.mark.parametrize("lst", ES.LISTS)
def test_rim_segments_are_decided_as_constructed_at_every_offset(orc, lst):
    ca, r, h = ES.disc_list(lst)
    seg, tgt, truth = ES.family(lst, "rim")
    delta = np.tile(np.array(ES.RIM_DELTA), len(seg) // len(ES.RIM_DELTA))
    assert np.array_equal(delta > 0, truth)
    counts = {}
    for d in ES.RIM_DELTA:
        sel = delta == d
        got, aimed = _per_target_hits(orc, ca, r, h, seg[sel], tgt[sel])
        want = {k: int(a.sum()) if d > 0 else 0 for k, a in aimed.items()}
        counts[d] = (sum(got.values()), int(sel.sum()))
        assert got == want, (lst, d, [(k, got[k], want[k]) for k in got if got[k] != want[k]][:8])
    print("rim", lst, "discs", len(ca), "segments", len(seg), "target hits (of segments) by delta:", counts)
    assert len(seg) == len(ES.targets(ca)) * ES.PER_DISC * len(ES.RIM_DELTA)


@pytest.mark.parametrize("lst", ES.LISTS)
def test_short_and_cluster_rim_segments_are_decided_as_constructed(orc, lst):
    ca, r, h = ES.disc_list(lst)
    for fam in ("short", "cluster_rim"):
        seg, tgt, truth = ES.family(lst, fam)
        for want_hit in (True, False):
            sel = truth == want_hit
            if not sel.any():
                assert fam == "cluster_rim" and not want_hit
                continue
            got, aimed = _per_target_hits(orc, ca, r, h, seg[sel], tgt[sel])
            want = {k: int(a.sum()) if want_hit else 0 for k, a in aimed.items()}
            assert got == want, (lst, fam, want_hit, [(k, got[k], want[k]) for k in got if got[k] != want[k]][:8])
        print(fam, lst, "segments", len(seg), "constructed hits", int(truth.sum()), "misses", int((~truth).sum()))
    seg, _, _ = ES.family(lst, "short")
    assert (seg[:, 6] == 0.0).sum() > 0 and (seg[:, 6] == 1e-300).sum() > 0


def test_every_family_lies_in_the_entrys_domain():
    box_half = 300.0
    everything = [ES.family(l, f)[0] for l in ES.LISTS for f in ES.FAMILIES] + [ES.ties()[3], ES.column()[3]]
    for seg in everything:
        assert np.isfinite(seg).all()
        assert (np.einsum("ij,ij->i", seg[:, :3], seg[:, :3]) <= 3.0 * box_half ** 2).all()
        assert (np.abs(np.linalg.norm(seg[:, 3:6], axis=1) - 1.0) <= 1e-12).all()
        assert (seg[:, 6] >= 0.0).all() and (seg[:, 6] <= 2.0 * math.sqrt(3.0) * box_half).all()
    for ca in [ES.disc_list(l)[0] for l in ES.LISTS] + [ES.ties()[0], ES.ties_among()[0], ES.column()[0]]:
        assert (np.abs(np.linalg.norm(ca[:, 3:], axis=1) - 1.0) <= 1e-12).all()
        assert (np.einsum("ij,ij->i", ca[:, :3], ca[:, :3]) <= 3.0 * box_half ** 2).all()


def test_the_placement_is_the_sweeps_own():
    import test_gpu_round2
    assert np.array_equal(ES.disc_positions(), test_gpu_round2._disc_positions())
    assert np.array_equal(ES.disc_positions(dtheta=5.0), test_gpu_round2._disc_positions(dtheta=5.0))
    assert [len(ES.disc_list(l)[0]) for l in ES.LISTS] == [362, 362, 1, 7, 8, 9, 16, 1024, 1025, 4096, 38]
    assert np.array_equal(ES.disc_list("n1024")[0], ES.disc_list("n1025")[0][:1024])


# ------------------------------------------------------------------ the culls' edges

@pytest.mark.parametrize("lst", ES.LISTS)
def test_neither_cull_drops_a_hit_of_any_family_with_the_kernels_margins(orc, lst):
    ca, r, h = ES.disc_list(lst)
    for fam in ES.FAMILIES:
        seg, tgt, truth = ES.family(lst, fam)
        i, j = DC.hit_pairs(seg, ca, r, h)
        # the restated exact test is the oracle's on these families (they are decided by margins far above its rounding)
        assert np.array_equal(np.bincount(j, minlength=len(ca)).astype(np.uint64), orc.bin_segments(ca, r, h, seg)), (lst, fam)
        res = DC.check(seg, ca, r, h, pairs=(i, j))
        print("culls", lst, fam, "segments", len(seg), "hits", res["hits"], "dropped by the binary32 pre-selection",
              res["dropped32"], "by the binary64 cull", res["dropped64"], "pairs per batch: max",
              int(res["pairs_per_batch"].max()), "batches above", DC.PAIR_FLUSH, ":", int((res["pairs_per_batch"] > DC.PAIR_FLUSH).sum()))
        assert res["hits"] >= int(truth.sum()) > 0
        assert res["dropped32"] == 0 and res["dropped64"] == 0, (lst, fam)


def test_special_families_against_the_culls_and_the_columns_pair_count(orc):
    for name, (ca, r, h, seg) in {"ties": ES.ties(), "ties_among": ES.ties_among(), "column": ES.column()[:4]}.items():
        res = DC.check(seg, ca, r, h)
        print("culls", name, "segments", len(seg), "hits", res["hits"], "dropped", res["dropped32"], res["dropped64"],
              "pairs per batch: max", int(res["pairs_per_batch"].max()))
        assert res["hits"] > 0 and res["dropped32"] == 0 and res["dropped64"] == 0
    ca, r, h, seg, counts = ES.column()
    # every segment passes every cluster: 64 x 5 = 320 pairs in a full batch, more than the list's flush threshold
    assert (res["pairs_per_batch"][:-1] == 320).all() and 320 > DC.PAIR_FLUSH
    assert np.array_equal(orc.bin_segments(ca, r, h, seg), np.full(len(ca), len(seg), dtype=np.uint64))
    assert sum(counts) == len(seg) and sorted(c % 64 for c in counts)[-1] == 63 and 2 in [c % 64 for c in counts]
    # the ties: both outcomes occur, and the one-ulp neighbours of a tie are decided both ways
    ca, r, h, seg = ES.ties()
    per = np.array([int(orc.bin_segments(ca, r, h, s[None, :])[0]) for s in seg])
    print("ties: segments", len(seg), "hits", int(per.sum()))
    assert 20 <= per.sum() <= len(seg) - 20


def _bare_drops(lst):
    """cluster_rim on a list with the binary32 margins taken away (1.0 and 0.0): (all hits, hits dropped, hits dropped with the
    kernel's margins, {delta: (target pairs dropped, segments)})"""
    ca, r, h = ES.disc_list(lst)
    seg, tgt, _ = ES.family(lst, "cluster_rim")
    pairs = DC.hit_pairs(seg, ca, r, h)
    bare = DC.check(seg, ca, r, h, f32_margins=(1.0, 0.0), pairs=pairs, count_pairs=False)
    kept = DC.check(seg, ca, r, h, pairs=pairs, count_pairs=False)
    perm, cluster_of, centres = DC.cluster_table(ca)
    cw = DC.cluster_radius(ca, r, h, perm, centres)
    delta = np.tile(np.repeat(np.array(ES.CLUSTER_RIM_DELTA), ES.PER_DISC), len(seg) // (ES.PER_DISC * len(ES.CLUSTER_RIM_DELTA)))
    k = cluster_of[tgt]
    near = DC.preselect(seg, centres[k], cw[k], (1.0, 0.0))
    by_delta = {d: (int((~near[delta == d]).sum()), int((delta == d).sum())) for d in ES.CLUSTER_RIM_DELTA}
    return bare["hits"], bare["dropped32"], kept["dropped32"], by_delta


def test_the_binary32_margins_are_what_holds_the_cluster_rim_hits():
    """The condition: without its two margins the restated pre-selection drops at least 100 hits of cluster_rim on a placement of
    _disc_positions' kind.  Where a hit can lie ON a cluster's ball is a matter of geometry: the table's radius is
    max |c - centre| + ball, which a tube reaches only if the direction from the cluster's centre to the disc's points at the
    tube's corner (1.15 degrees out of the disc's plane for r 5, h 0.1), and only the cluster's farthest disc can.  In the 362-disc
    sweep placement (steps of 0.5 degrees, 1.75 cm) two discs do -- 160 of the 28 960 segments lie within 1e-2 cm^2 of the ball, 63
    hits are dropped --; in the same placement in steps of 0.05 degrees (list "fine", also 362 discs) most clusters hold one, and
    about 1300 are.  The bound is asserted on the latter; the former has to show the effect at all."""
    hits, dropped, with_margins, by_delta = _bare_drops("placement")
    print("cluster_rim on the placement: hits", hits, "dropped without the binary32 margins", dropped,
          "target pairs dropped (of segments) by delta:", by_delta, "with the margins", with_margins)
    assert with_margins == 0 and dropped > 0
    hits, dropped, with_margins, by_delta = _bare_drops("fine")
    print("cluster_rim on the fine placement: hits", hits, "dropped without the binary32 margins", dropped,
          "target pairs dropped (of segments) by delta:", by_delta, "with the margins", with_margins)
    assert with_margins == 0
    assert dropped >= 100
    assert all(n >= 100 for n, _ in by_delta.values())


# ------------------------------------------------------------------ isxo_bin_segments

def _sweep_cfg(mod):
    c = mod.default_config()
    c.r_out = 105.0; c.reflectance = 1.0; c.roughness_rad = 0.0; c.max_points = 10000
    c.box_half = 200.0; c.src[2] = -80
    return c


@pytest.mark.parametrize("kind", ["default", "sweep"])
def test_oracle_bin_segments_equals_the_disc_sweep_on_the_exit_segments_of_a_trace(orc, kind):
    c = orc.default_config() if kind == "default" else _sweep_cfg(orc)
    ca = ES.disc_positions(dtheta=5.0)
    n, seed = 4000, 21
    want, stats = orc.disc_sweep(c, ca, ES.R_REF, ES.H_REF, n, seed)
    status, seg = orc.exit_segments(c, n, seed)
    st2, _, lp, d = orc.trace_endstates(c, n, seed)
    assert np.array_equal(status, st2)
    ex = status == 1
    assert ex.sum() == stats.exited > 500
    assert np.array_equal(seg[ex, 3:6], d[ex]) and (seg[~ex] == 0).all()
    # tmax is (p - start).v: the segment ends at the reported last point
    assert np.abs(seg[ex, :3] + seg[ex, 6:7] * seg[ex, 3:6] - lp[ex]).max() < 1e-9
    got = orc.bin_segments(ca, ES.R_REF, ES.H_REF, seg[ex])
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert int(got.sum()) == stats.bin_increments > 0
    assert np.array_equal(orc.bin_segments(ca, ES.R_REF, ES.H_REF, seg[ex], nthreads=1), want)
    # the traced segments are in the injected entry's domain
    assert np.abs(np.linalg.norm(seg[ex, 3:6], axis=1) - 1.0).max() <= 1e-12
    assert np.linalg.norm(seg[ex, :3], axis=1).max() <= math.sqrt(3.0) * c.box_half
    assert seg[ex, 6].min() >= 0.0 and seg[ex, 6].max() <= 2.0 * math.sqrt(3.0) * c.box_half


def test_the_oracle_addition_is_clean_under_the_sanitizers(orc, tmp_path):
    """isx_oracle.c + tests/native/bin_segments_main.c compiled with AddressSanitizer and UBSan and run as a child process
    (nothing is preloaded): exit status 0 -- the brute force equals isxo_disc_sweep there too -- and the counts it prints are the
    library's"""
    exe = str(tmp_path / "bin_segments_main")
    src = [os.path.join(ROOT, "oracle", "isx_oracle.c"), os.path.join(ROOT, "tests", "native", "bin_segments_main.c")]
    # (gcc by name: the flags that link the sanitizers' runtimes statically are gcc's, whatever CC says)
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-ffp-contract=off", "-mfma", "-msse4.1", "-fopenmp", "-D_GNU_SOURCE",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "oracle"), "-o", exe] + src + ["-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    t = np.deg2rad((np.arange(19) - 9) * 5.0)
    ca = np.stack([200.0 * np.sin(t), 0 * t, -200.0 * np.cos(t), np.sin(t), 0 * t, -np.cos(t)], axis=1)
    want, st = orc.disc_sweep(orc.default_config(), ca, 5.0, 0.1, 2000, 21)
    assert r.stdout.splitlines() == ["threads %d: segments %d hits %d" % (nt, st.exited, int(want.sum())) for nt in (1, 4)] + \
        ["one disc: hits %d" % int(want[9])], r.stdout
    assert int(want.sum()) > 0


# ------------------------------------------------------------------ the entry's refusals, without a device

@pytest.fixture(scope="module")
def mod():
    import altair_raytracing_amd as m
    m.load()
    return m


def _call(mod, cfg, ca, seg, r=5.0, h=0.1, n=None, n_disc=None, counts=None, n_regions=None, unit=-1, hits=True):
    u64, dbl = C.c_uint64, C.c_double
    ca = None if ca is None else np.ascontiguousarray(ca, dtype=np.float64)
    seg = None if seg is None else np.ascontiguousarray(seg, dtype=np.float64)
    out = np.zeros(1 << 16, dtype=np.uint64)
    rc_arr = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
    inc = u64(0)
    p = lambda x, t: x.ctypes.data_as(C.POINTER(t))
    return mod.load().isx_bin_injected_segments(
        C.byref(cfg) if cfg is not None else None, p(ca, dbl) if ca is not None else None,
        (len(ca) if ca is not None else 1) if n_disc is None else n_disc, r, h,
        p(seg, dbl) if seg is not None else None, (len(seg) if seg is not None else 0) if n is None else n,
        p(rc_arr, C.c_uint32) if rc_arr is not None else None, (0 if rc_arr is None else rc_arr.size) if n_regions is None else n_regions,
        unit, p(out, u64) if hits else None, C.byref(inc))


def test_entry_refusals_need_no_device(mod):
    A = mod.abi
    c = mod.default_config()
    ca = ES.disc_positions(dtheta=5.0)[:3]
    good = np.array([[0.0, 0.0, -50.0, 0.0, 0.0, -1.0, 200.0], [10.0, 0.0, -60.0, 0.6, 0.0, -0.8, 0.0]])
    passed = (A.OK, A.ERR_NO_DEVICE, A.ERR_NOT_INIT)      # every refusal is behind us: the device is asked for next
    assert _call(mod, c, ca, good) in passed
    assert _call(mod, c, ca, good, counts=[1, 0, 1]) in passed
    assert _call(mod, c, ca, good[:0], n=0) in passed
    for unit in (0, 2):
        assert _call(mod, c, ca, good, unit=unit) in passed
    # NULL pointers
    assert _call(mod, None, ca, good) == A.ERR_BAD_ARG
    assert _call(mod, c, None, good, n_disc=3) == A.ERR_BAD_ARG
    assert _call(mod, c, ca, None, n=2) == A.ERR_BAD_ARG
    assert _call(mod, c, ca, good, hits=False) == A.ERR_BAD_ARG
    # the disc list
    for n_disc in (0, -1, 36001):
        assert _call(mod, c, ca, good, n_disc=n_disc) == A.ERR_BAD_ARG
    for r, h in ((0.0, 0.1), (-1.0, 0.1), (5.0, 0.0), (5.0, -0.1), (np.nan, 0.1), (5.0, np.nan), (np.inf, 0.1)):
        assert _call(mod, c, ca, good, r=r, h=h) == A.ERR_BAD_ARG, (r, h)
    # unit, n
    for unit in (-2, 1, 3):
        assert _call(mod, c, ca, good, unit=unit) == A.ERR_BAD_ARG
    assert _call(mod, c, ca, good, n=A.INJECT_MAX_LINES + 1) == A.ERR_TOO_LARGE
    # region layouts: a count above a region, counts that do not sum to n, region numbers out of range
    assert _call(mod, c, ca, good, counts=[2, 1025], n=2) == A.ERR_BAD_ARG
    assert _call(mod, c, ca, good, counts=[1, 2]) == A.ERR_BAD_ARG
    assert _call(mod, c, ca, good, counts=[1]) == A.ERR_BAD_ARG
    assert _call(mod, c, ca, good, counts=[1, 1], n_regions=0) == A.ERR_BAD_ARG
    assert _call(mod, c, ca, good, counts=[1, 1], n_regions=A.INJECT_MAX_REGIONS + 1) == A.ERR_BAD_ARG
    assert _call(mod, c, ca, good, counts=None, n_regions=2) == A.ERR_BAD_ARG
    # a config the public call refuses
    bad = c.copy(); bad.struct_size = 0
    assert _call(mod, bad, ca, good) == A.ERR_BAD_CONFIG
    bad = c.copy(); bad.r_out = bad.r_in
    assert _call(mod, bad, ca, good) == A.ERR_BAD_CONFIG
    bad = c.copy(); bad.source_model = A.SOURCE_BRDF
    assert _call(mod, bad, ca, good) == A.ERR_BAD_CONFIG
    # the domain of the segments: finite coordinates, unit directions, starts within sqrt(3) box_half, 0 <= tmax <= 2 sqrt(3) box_half
    for k in range(7):
        for v in (np.nan, np.inf, -np.inf):
            s = good.copy(); s[1, k] = v
            assert _call(mod, c, ca, s) == A.ERR_BAD_ARG, (k, v)
    for scale in (1 + 1e-11, 1 - 1e-11, 0.0, 2.0):
        s = good.copy(); s[1, 3:6] *= scale
        assert _call(mod, c, ca, s) == A.ERR_BAD_ARG, scale
    s = good.copy(); s[1, 3:6] *= 1 + 2e-13
    assert _call(mod, c, ca, s) in passed
    reach = math.sqrt(3.0) * c.box_half
    s = good.copy(); s[0, :3] = (0.0, reach * (1 + 1e-9), 0.0)
    assert _call(mod, c, ca, s) == A.ERR_BAD_ARG
    s = good.copy(); s[0, :3] = (0.0, reach * 0.999, 0.0)
    assert _call(mod, c, ca, s) in passed
    for tmax, ok in ((-1e-300, False), (-1.0, False), (2 * reach * (1 + 1e-9), False), (2 * reach * 0.999, True), (-0.0, True), (1e-300, True)):
        s = good.copy(); s[0, 6] = tmax
        assert (_call(mod, c, ca, s) in passed) == ok and (ok or _call(mod, c, ca, s) == A.ERR_BAD_ARG), tmax
    # ... and of the discs: finite, unit axes, centres within the same reach
    for k in range(6):
        for v in (np.nan, np.inf):
            d = ca.copy(); d[2, k] = v
            assert _call(mod, c, d, good) == A.ERR_BAD_ARG, (k, v)
    for scale in (1 + 1e-11, 1 - 1e-11, 0.0):
        d = ca.copy(); d[1, 3:] *= scale
        assert _call(mod, c, d, good) == A.ERR_BAD_ARG, scale
    d = ca.copy(); d[0, :3] = (reach * (1 + 1e-9), 0.0, 0.0)
    assert _call(mod, c, d, good) == A.ERR_BAD_ARG
    d = ca.copy(); d[0, :3] = (reach * 0.999, 0.0, 0.0)
    assert _call(mod, c, d, good) in passed


# ------------------------------------------------------------------ the numpy cluster table

@pytest.mark.parametrize("lst", ES.LISTS)
def test_cluster_table_is_a_permutation_into_clusters_that_hold_their_discs(lst):
    ca, r, h = ES.disc_list(lst)
    n = len(ca)
    perm, cluster_of, centres = DC.cluster_table(ca)
    cw = DC.cluster_radius(ca, r, h, perm, centres)
    assert sorted(perm.tolist()) == list(range(n))
    assert len(centres) == len(cw) == (n + 7) // 8 and centres.dtype == np.float32 and cw.dtype == np.float32
    assert np.array_equal(cluster_of[perm], np.arange(n) // 8)
    # every disc's bounding ball lies inside its cluster's ball
    ball = math.sqrt(r * r + h * h)
    dist = np.linalg.norm(ca[:, :3] - centres[cluster_of].astype(np.float64), axis=1)
    assert (dist + ball <= cw[cluster_of].astype(np.float64)).all()
    assert (cw.astype(np.float64) <= (dist.max() + ball) * (1 + 3e-6)).all()
    if lst == "coincident":
        assert np.array_equal(perm, np.arange(n)), "equal Morton codes keep the caller's order"
