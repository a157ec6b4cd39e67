"""The scene path histograms on the GPU: isx_scene_path_hist bit for bit against the restatements of include/isx.h
(tests/scenepath_np.py: the Python restatement for the small shapes, the C walk of tests/native/scene_path_walk.c for the rest) --
the histograms, the 21 overflow counters, the 21 checksums, the 36 scene counters and the census -- with the low bins in the
workgroup's LDS (automatic and capped) and with every bin in global memory, across 2^32 inside one launch, with long rays, under
every cut and launch shape; against isx_scene_response and isx_fluxmap_scene; the device form and the sharded call.

The checksum is the instrument for the carried double: a hand-over or a park that loses or mixes up one ray's L changes the sum
of the bit patterns, whatever the bin width.  The conditions on the walks are asserted on the restatements alone before the
library is looked at.  Every walk is computed once per key, shared, never changed."""
import os
import subprocess
import sys

import numpy as np
import pytest

import response_np as R
import scene_np as SC
import scenepath_np as SP
import test_gpu_baffle as TB
from test_gpu_scene import _case
from test_gpu_scene_response import FILLED, N_SIDE, _side, _side_walk
from test_gpu_scene_walk import CROSSING, LONG, N, _row_case, _scene_row
from test_scene_path_cpu import EDGES, edge_expect, edge_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
CENSUS = SC.CENSUS_FIELDS
CAP = 8             # "spath_lds_bins" of the capped form: bins 0..7 in the LDS, the rest global
BIN = 25.0

_kept = {}


def _reset(isx):
    TB._reset(isx)
    isx.set_option("spath_lds_bins", -1)


def _side_replay(orc):
    """side_photometer, 2e4 rays: the Python restatement (once), with the counters and the census of the oracle's own walk, which
    the restatement's per-ray end states are asserted to equal"""
    if "side" not in _kept:
        oc, spec = _side(orc)
        p = SP.replay(oc, SC.spec_of(spec), N_SIDE, SEED, 0)
        w = _side_walk(orc)
        for k in ("status", "n_points", "last_point", "direction", "last_baffle", "last_class"):
            assert np.array_equal(p[k], w[k]), k
        q = dict(w)
        q["path_cm"] = p["path_cm"]
        _kept["side"] = q
    return _kept["side"]


def _c_walk(orc, key, oc, spec, n, first=0, base=None):
    """the C walk of a scene (once per key), with the counters and the census of the oracle's own walk `base` (or a fresh one)"""
    if key not in _kept:
        sd = SC.spec_of(spec)
        c = SP.walk(orc, oc, sd, n, SEED, first, nthreads=16)
        w = base if base is not None else orc.scene_walk(oc, sd, n, SEED, first, nthreads=16)
        for k in ("status", "n_points", "last_point", "direction", "last_baffle", "last_class"):
            assert np.array_equal(c[k], w[k]), k
        q = dict(w)
        q["path_cm"] = c["path_cm"]
        _kept[key] = q
    return _kept[key]


def _side_conditions(orc):
    """on the restatement alone: at least 40 rays in every slot the scene can fill; with 4 bins (100 cm) at least one ray overflows
    in every slot the scene can fill but 19 -- a ray that leaves otherwise gets no tail and has only its legs inside the cavity's
    lower part behind it: the restatement has none of them above 100 cm, so that slot's overflow is asserted to be 0 -- and so in
    each form of the sink (the parametrised test asserts the library's overflow per form); at least 40 rays lie on either side of
    bin CAP"""
    oc, _ = _side(orc)
    w = _side_replay(orc)
    hist, over, _ = SP.from_walk(w, oc, 64, BIN)
    rows = hist.sum(axis=1) + over
    _, over4, _ = SP.from_walk(w, oc, 4, BIN)
    ib = (w["path_cm"] / BIN).astype(np.int64)
    print("side_photometer fates:", rows.tolist(), "overflow of 4 bins:", over4.tolist(), "bins < 8:", int((ib < CAP).sum()),
          ">= 8:", int((ib >= CAP).sum()), "largest L", float(w["path_cm"].max()))
    assert all(int(rows[f]) >= 40 for f in FILLED), rows.tolist()
    assert not rows[4:10].any() and not rows[14:18].any()
    assert all(int(over4[f]) >= 1 for f in FILLED if f != SP.EXITED_OTHER) and int(over4[SP.EXITED_OTHER]) == 0
    assert int((ib < CAP).sum()) >= 40 and int((ib >= CAP).sum()) >= 40
    return w


def _equal(got, w, oc, n_bins, bin_cm):
    hist, pc, cnt, st = got
    want, over, cks = SP.from_walk(w, oc, n_bins, bin_cm)
    assert hist.dtype == np.uint64 and hist.shape == want.shape == (21, n_bins)
    assert np.array_equal(hist, want)
    assert np.array_equal(pc.words()[:21], over)
    assert np.array_equal(pc.words()[21:], cks), "the checksums: a path length was lost, mixed up or rounded otherwise"
    assert np.array_equal(cnt.words(), SC.counter_words(w))
    for f in CENSUS:
        assert getattr(st, f) == w["census"][f], f
    _identities(hist, pc, cnt, st)


def _identities(hist, pc, cnt, st):
    pa, pb, ba, bb = cnt.arrays()
    over = pc.words()[:21]
    rows = hist.sum(axis=1) + over
    assert np.array_equal(rows[:10], pb) and np.array_equal(rows[10:18], bb.reshape(-1))
    assert rows[18] == st.counted_below_z and rows[18] + rows[19] == st.exited and rows[20] == st.suspended
    assert int(rows.sum()) == st.launched and int(hist.sum()) == st.bin_increments
    assert int(pa.sum()) + int(ba.sum()) == st.wall_hits and int(pb.sum()) + int(bb.sum()) == st.absorbed
    assert st.exited + st.absorbed + st.suspended == st.launched


# ---------------------------------------------------------------- 1. small shapes: the Python restatement, every form
@pytest.mark.parametrize("lds_bins", [-1, 0, CAP], ids=["automatic", "global", "cap-8"])
@pytest.mark.parametrize("n_bins", [1, 4, 29, 64, 4096])
def test_side_photometer_equals_the_restatement(isx, orc, n_bins, lds_bins):
    """20 000 rays of at most 30 points, bins of 25 cm: 1 and 4 bins overflow, 4096 hold everything"""
    w = _side_conditions(orc)
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    try:
        isx.set_option("spath_lds_bins", lds_bins)
        got = isx.scene_path_hist(cfg, spec, isx.scene_path_spec(n_bins, BIN), N_SIDE, SEED)
        assert bool(got[1].words()[:21].any()) == (n_bins < 4096)
        _equal(got, w, oc, n_bins, BIN)
    finally:
        _reset(isx)


# ---------------------------------------------------------------- 2. 1e6 rays: long rays, and a ray index that passes 2^32
@pytest.mark.parametrize("lds_bins", [-1, 0], ids=["automatic", "global"])
@pytest.mark.parametrize("name,rho,first,theta", [LONG, ("photometer", 0.95, CROSSING, 170.0)], ids=["led_first_in-long-rays", "photometer-across-2^32"])
def test_a_million_rays_equal_the_c_walk(isx, orc, name, rho, first, theta, lds_bins):
    """the rows of test_gpu_scene_walk.py (their oracle walks are shared with it), 65536 bins of 25 cm.  The row of the long rays
    (rays above 1000 points: L above 1e5 cm, bins far beyond any B a launch can have) hands every ray over many times."""
    base = _scene_row(orc, name, rho, first, theta)
    oc, ospec = _row_case(orc, name, rho, theta)
    w = _c_walk(orc, ("row", name, rho, first, theta), oc, ospec, N, first, base)
    ib = (w["path_cm"] / BIN).astype(np.int64)
    print("largest L", float(w["path_cm"].max()), "rays above bin 4096:", int((ib >= 4096).sum()))
    if (name, rho, first, theta) == LONG:
        assert int(w["n_points"].max()) > 1000 and int((ib >= 4096).sum()) >= 40 and int(ib.max()) < 65536
    _reset(isx)
    cfg, spec = _row_case(isx, name, rho, theta)
    try:
        isx.set_option("spath_lds_bins", lds_bins)
        got = isx.scene_path_hist(cfg, spec, isx.scene_path_spec(65536, BIN), N, SEED, first_ray=first)
        assert not got[1].words()[:21].any()
        _equal(got, w, oc, 65536, BIN)
    finally:
        _reset(isx)


# ---------------------------------------------------------------- 3. queues and parks: the hazards of the carried double
N_Q = 200_000


@pytest.mark.parametrize("shape", [{"grid_blocks": 1}, {"assist_block": 256}, {"assist_block": 768}, {"pipeline_chunk": 4096}, {"ray_sub": 64}],
                         ids=lambda s: "%s=%d" % next(iter(s.items())))
@pytest.mark.parametrize("lds_bins", [-1, CAP], ids=["automatic", "cap-8"])
def test_queues_and_parks_keep_every_path_length(isx, orc, lds_bins, shape):
    """2e5 rays of `photometer`: one workgroup with full rings, other workgroup sizes (other park counts), launches of 4096 rays,
    sub-ranges of 64 rays (a park per refill) -- the checksums are the walk's"""
    oc, ospec = _case(orc, "photometer", 0.95)
    w = _c_walk(orc, ("photometer", N_Q), oc, ospec, N_Q)
    _reset(isx)
    cfg, spec = _case(isx, "photometer", 0.95)
    try:
        for k, v in shape.items():
            isx.set_option(k, v)
        isx.set_option("spath_lds_bins", lds_bins)
        _equal(isx.scene_path_hist(cfg, spec, isx.scene_path_spec(1024, BIN), N_Q, SEED), w, oc, 1024, BIN)
    finally:
        _reset(isx)


# ---------------------------------------------------------------- 4. partition invariance, the device form
@pytest.mark.parametrize("lds_bins", [-1, 0, CAP], ids=["automatic", "global", "cap-8"])
def test_partition_invariance(isx, orc, lds_bins):
    """20 000 rays as 7 001 + 1 + 12 998: histograms, overflow, checksums (modulo 2^64), counters and census add up to the whole"""
    w = _side_conditions(orc)
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    ps = isx.scene_path_spec(16, BIN)
    try:
        isx.set_option("spath_lds_bins", lds_bins)
        whole = isx.scene_path_hist(cfg, spec, ps, N_SIDE, SEED)
        parts = [isx.scene_path_hist(cfg, spec, ps, n, SEED, first_ray=first) for first, n in ((0, 7001), (7001, 1), (7002, 12998))]
    finally:
        _reset(isx)
    _equal(whole, w, oc, 16, BIN)
    assert [p[3].launched for p in parts] == [7001, 1, 12998]
    assert np.array_equal(sum(p[0] for p in parts), whole[0])
    with np.errstate(over="ignore"):
        assert np.array_equal(sum(p[1].words() for p in parts), whole[1].words()) and whole[1].words()[:21].any()
    assert np.array_equal(sum(p[2].words() for p in parts), whole[2].words())
    for f in CENSUS + ("bin_increments",):
        assert sum(getattr(p[3], f) for p in parts) == getattr(whole[3], f), f
    for part in parts:
        _identities(*part)


def test_device_form_accumulates():
    """isx_scene_path_hist_device twice into one set of buffers == twice the blocking result on top of what was there (the
    checksums modulo 2^64), and isx_take_stats adds up (a process of its own: torch owns the tensors)."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import altair_raytracing_amd as isx
from test_gpu_scene_response import _side
isx.load(); isx.init(0)
cfg, spec = _side(isx)
SEED = 12345
for n_bins, cap in ((16, -1), (64, 8), (4096, 0)):
    isx.set_option("spath_lds_bins", cap)
    ps = isx.scene_path_spec(n_bins, 25.0)
    nw = 21 * n_bins
    d_hist = torch.arange(5, 5 + nw, dtype=torch.int64, device="cuda:0")
    d_pc = torch.arange(50, 92, dtype=torch.int64, device="cuda:0")
    d_cnt = torch.arange(100, 136, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):
        isx.scene_path_hist_device(cfg, spec, ps, 20000, SEED, 0, d_hist.data_ptr(), d_pc.data_ptr(), d_cnt.data_ptr())
    isx.sync()
    st = isx.take_stats()
    hist, pc, cnt, bst = isx.scene_path_hist(cfg, spec, ps, 20000, SEED)
    torch.cuda.synchronize()
    assert np.array_equal(d_hist.cpu().numpy() - np.arange(5, 5 + nw), 2 * hist.reshape(-1).astype(np.int64))
    with np.errstate(over="ignore"):
        want = np.arange(50, 92).astype(np.uint64) + np.uint64(2) * pc.words()
    assert np.array_equal(d_pc.cpu().numpy().astype(np.uint64), want)
    assert np.array_equal(d_cnt.cpu().numpy() - np.arange(100, 136), 2 * cnt.words().astype(np.int64))
    for f in ("launched", "exited", "counted_below_z", "absorbed", "suspended", "wall_hits", "bin_increments"):
        assert getattr(st, f) == 2 * getattr(bst, f), f
    assert int(hist.sum()) + int(pc.words()[:21].sum()) == 20000 and bool(pc.words()[:21].any()) == (n_bins != 4096)
    assert pc.words()[21:].any()
for ptrs in ((0, d_pc.data_ptr(), d_cnt.data_ptr()), (d_hist.data_ptr(), 0, d_cnt.data_ptr()), (d_hist.data_ptr(), d_pc.data_ptr(), 0)):
    try:
        isx.scene_path_hist_device(cfg, spec, ps, 10, SEED, 0, *ptrs)
        raise SystemExit("a NULL pointer was accepted")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_BAD_ARG
isx.shutdown()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]


# ---------------------------------------------------------------- 5. ray counts
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_ray_counts(isx, orc, n):
    _reset(isx)
    cfg, spec = _side(isx)
    oc, ospec = _side(orc)
    got = isx.scene_path_hist(cfg, spec, isx.scene_path_spec(16, BIN), n, SEED)
    if n == 0:
        hist, pc, cnt, st = got
        assert not hist.any() and not pc.words().any() and not cnt.words().any()
        assert st.launched == 0 and st.bin_increments == 0 and st.wall_hits == 0
        return
    _equal(got, _c_walk(orc, ("side", n), oc, ospec, n), oc, 16, BIN)


# ---------------------------------------------------------------- 6. hand-made rays through the library
@pytest.mark.parametrize("which", EDGES)
def test_hand_made_rays(isx, orc, which):
    """64 and 20 000 copies of one ray whose path length is known by hand (tests/test_scene_path_cpu.py: edge_scene)"""
    _reset(isx)
    cfg, spec, n_bins, bin_cm = edge_scene(isx, which)
    oc, _, _, _ = edge_scene(orc, which)
    fate, L = edge_expect(oc, which)
    word = int(SP.bits(np.array([L]))[0])
    for n in (64, 20000):
        hist, pc, cnt, st = isx.scene_path_hist(cfg, spec, isx.scene_path_spec(n_bins, bin_cm), n, SEED)
        want = np.zeros((21, n_bins), dtype=np.uint64)
        want[fate, int(L / bin_cm)] = n
        assert np.array_equal(hist, want) and not pc.words()[:21].any()
        assert int(pc.words()[21 + fate]) == (n * word) % (1 << 64) and int((pc.words()[21:] != 0).sum()) == (1 if word else 0)
        _identities(hist, pc, cnt, st)
    if which == "first_strike":        # fb == n_bins is overflow
        hist, pc, _, _ = isx.scene_path_hist(cfg, spec, isx.scene_path_spec(4, bin_cm), 64, SEED)
        assert not hist.any() and pc.words()[fate] == 64 and int(pc.words()[:21].sum()) == 64


# ---------------------------------------------------------------- 7. against the library itself
@pytest.mark.parametrize("name,rho,n", [("photometer", 0.95, 100_000), ("led_first_in", 0.95, 100_000), ("full", 0.95, 100_000)])
def test_rows_counters_and_census_are_the_librarys(isx, name, rho, n):
    """GPU against GPU: rows plus overflow are isx_scene_response's row sums with spec (1, 1, 1, 1); the 36 counters and every
    field of the census but bin_increments are isx_fluxmap_scene's; one bin of 1e300 cm is the response's row itself; the
    detector grid and the hit line play no part"""
    _reset(isx)
    cfg, spec = _case(isx, name, rho)
    _, fcnt, fst = isx.fluxmap_scene(cfg, spec, n, SEED)
    resp, _, _ = isx.scene_response(cfg, spec, isx.response_spec(1, 1, 1, 1), n, SEED)
    sums = []
    for n_bins, bin_cm in ((1, 1e300), (8, BIN), (1024, cfg.r_in / 4)):
        hist, pc, cnt, st = isx.scene_path_hist(cfg, spec, isx.scene_path_spec(n_bins, bin_cm), n, SEED)
        over = pc.words()[:21]
        assert np.array_equal(hist.sum(axis=1) + over, resp[:, 0])
        assert bool(over.any()) == (n_bins == 8)
        if n_bins == 1:
            assert np.array_equal(hist[:, 0], resp[:, 0])
        assert np.array_equal(cnt.words(), fcnt.words())
        for f in CENSUS:
            assert getattr(st, f) == getattr(fst, f), f
        assert st.launched == n and st.counted_below_z > 100
        _identities(hist, pc, cnt, st)
        sums.append(pc.words()[21:])
    assert np.array_equal(sums[0], sums[1]) and np.array_equal(sums[0], sums[2])      # the checksums do not depend on the bins
    odd = cfg.copy(); odd.n_theta, odd.n_phi, odd.hit_line_mode = 36000, 36000, 1
    hist2, pc2, cnt2, st2 = isx.scene_path_hist(odd, spec, isx.scene_path_spec(1024, cfg.r_in / 4), n, SEED)
    assert np.array_equal(hist2, hist) and np.array_equal(pc2.words(), pc.words()) and np.array_equal(cnt2.words(), cnt.words())


def test_the_default_scene_goes_through(isx, orc):
    """the pencil as the degenerate beam, no baffle, no patch, the default spec: the C walk's result"""
    _reset(isx)
    cfg, spec = _case(isx, "empty", 0.99)
    oc, ospec = _case(orc, "empty", 0.99)
    n = 100_000
    w = _c_walk(orc, ("empty", n), oc, ospec, n)
    ps = isx.default_scene_path_spec(cfg)
    got = isx.scene_path_hist(cfg, spec, ps, n, SEED)
    _equal(got, w, oc, ps.n_bins, ps.bin_cm)
    assert not got[0][2:18].any() and got[0][18].sum() > 1000


# ---------------------------------------------------------------- 8. the sharded call
def test_scene_path_hist_sharded_one_rank_equals_scene_path_hist(isx):
    _reset(isx)
    cfg, spec = _side(isx)
    ps = isx.scene_path_spec(16, BIN)
    hist, pc, cnt, st = isx.scene_path_hist(cfg, spec, ps, N_SIDE, SEED)
    shist, sover, scks, pa, pb, ba, bb, sc = isx.scene_path_hist_sharded(isx.scene_path_hist, cfg, spec, ps, N_SIDE, SEED)
    assert np.array_equal(shist, hist) and np.array_equal(sover, pc.words()[:21]) and np.array_equal(scks, pc.words()[21:])
    assert int(hist.sum()) + int(sover.sum()) == N_SIDE and scks.any()
    for got, want in zip((pa, pb, ba, bb), cnt.arrays()):
        assert np.array_equal(got, want)
    for f in CENSUS + ("bin_increments",):
        assert sc[f] == getattr(st, f), f


# ---------------------------------------------------------------- 9. refusals with a device present
def test_refusals_with_a_device(isx):
    """a refused spec, a refused scene and a NULL pointer are answered as without a device, and nothing is written"""
    import ctypes as C
    from test_scene_path_cpu import path_specs
    _reset(isx)
    cfg, spec = _side(isx)
    lib = isx.load()
    buf = np.full(21 * 16, 7, dtype=np.uint64)
    hp = buf.ctypes.data_as(C.POINTER(C.c_uint64))
    pc, cnt = isx.ScenePathCounts(), isx.SceneCounts()
    bad, _ = path_specs(isx)
    for what, ps in bad:
        st = isx.Stats(); st.launched = 77
        assert lib.isx_scene_path_hist(C.byref(cfg), C.byref(spec), C.byref(ps), 10, 1, 0, hp, C.byref(pc), C.byref(cnt), C.byref(st)) == isx.abi.ERR_BAD_CONFIG, what
        assert st.launched == 77
    ps = isx.scene_path_spec(16, BIN)
    broken = spec.copy(); broken.beam.struct_size = 0
    assert lib.isx_scene_path_hist(C.byref(cfg), C.byref(broken), C.byref(ps), 10, 1, 0, hp, None, None, None) == isx.abi.ERR_BAD_CONFIG
    for k in range(4):
        a = [C.byref(cfg), C.byref(spec), C.byref(ps), hp]
        a[k] = None
        assert lib.isx_scene_path_hist(a[0], a[1], a[2], 10, 1, 0, a[3], None, None, None) == isx.abi.ERR_BAD_ARG, k
    assert (buf == 7).all() and not pc.words().any() and not cnt.words().any()
    hist, pc2, _, st = isx.scene_path_hist(cfg, spec, ps, 10, 1)      # (and the library goes on serving)
    assert st.launched == 10 and int(hist.sum()) + int(pc2.words()[:21].sum()) == 10
