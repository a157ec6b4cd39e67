"""The scene response on the GPU: isx_scene_response bit for bit against the restatement of include/isx.h on the oracle's native
scene walk (tests/response_np.py on isxo_scene_walk) -- response, the 36 counters and the census -- in both forms of the kernel
(the workgroup's LDS block and the global adds), across 2^32 inside one launch, under every cut and launch shape; against
isx_fluxmap_scene for counts and census; the device form and the sharded call.

The conditions on the walk -- every slot the scene can fill is filled -- are asserted on the oracle alone before the library is
looked at.  Every walk is computed once per key, shared, never changed."""
import os
import subprocess
import sys

import numpy as np
import pytest

import response_np as R
import scene_np as SC
import test_gpu_baffle as TB
from test_gpu_scene import _case
from test_gpu_scene_walk import CROSSING, N, _scene_row

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
CENSUS = SC.CENSUS_FIELDS
N_SIDE = 20000
SIDE_SPEC = (3, 5, 7, 11)
SMALL_SPEC = (2, 1, 3, 2)       # 12 bins x 11 slots: fits the workgroup's LDS at every launch shape


def _reset(isx):
    TB._reset(isx)
    isx.set_option("resp_global", 0)


def _side(mod, max_points=30):
    """`side_photometer`: the beam `side` of test_gpu_beam.py with photometer's baffles and patches, wall reflectance 0.95, at most
    30 points per ray -- rays end in every slot a scene with two baffles and two patches can fill"""
    import altair_raytracing_amd as isx
    c, ph = _case(mod, "photometer", 0.95, max_points=max_points)
    ic = isx.default_config()
    side = isx.beam_cone(ic, (-60, 0, -75), (1, 0, 0), 10.0, 20.0, isx.BEAM_UNIFORM)
    s = ph.copy()
    s.beam = side
    return c, s


_walks = {}


def _side_walk(orc, n=N_SIDE, first=0):
    key = (n, first)
    if key not in _walks:
        oc, spec = _side(orc)
        _walks[key] = orc.scene_walk(oc, SC.spec_of(spec), n, SEED, first, nthreads=16)
    return _walks[key]


FILLED = (0, 1, 2, 3, 10, 11, 12, 13, 18, 19, 20)


def _side_conditions(orc, isx):
    """on the walk alone: at least 40 rays in every slot the scene can fill"""
    oc, _ = _side(orc)
    w = _side_walk(orc)
    one = R.from_walk(w, oc, isx.response_spec(1, 1, 1, 1), SEED, 0)[:, 0]
    print("side_photometer fates:", one.tolist())
    assert all(int(one[f]) >= 40 for f in FILLED), one.tolist()
    assert not one[4:10].any() and not one[14:18].any()
    return w


def _equal(got, w, oc, rs, first=0, seed=SEED):
    resp, cnt, st = got
    want = R.from_walk(w, oc, rs, seed, first)
    assert resp.dtype == np.uint64 and resp.shape == want.shape == (21, rs.bins)
    assert np.array_equal(resp, want)
    assert np.array_equal(cnt.words(), SC.counter_words(w))
    for f in CENSUS:
        assert getattr(st, f) == w["census"][f], f
    _identities(resp, cnt, st)


def _identities(resp, cnt, st):
    pa, pb, ba, bb = cnt.arrays()
    rows = resp.sum(axis=1)
    assert np.array_equal(rows[:10], pb) and np.array_equal(rows[10:18], bb.reshape(-1))
    assert rows[18] == st.counted_below_z and rows[18] + rows[19] == st.exited and rows[20] == st.suspended
    assert int(resp.sum()) == st.launched == st.bin_increments
    assert int(pa.sum()) + int(ba.sum()) == st.wall_hits and int(pb.sum()) + int(bb.sum()) == st.absorbed
    assert st.exited + st.absorbed + st.suspended == st.launched


# ---------------------------------------------------------------- parity with the walk, both forms
@pytest.mark.parametrize("resp_global", [0, 1], ids=["default-form", "global-form"])
@pytest.mark.parametrize("axes", [SIDE_SPEC, SMALL_SPEC, (1, 1, 1, 1), (4, 1, 1, 1024)], ids=["3x5x7x11", "2x1x3x2", "B=1", "B=4096"])
def test_side_photometer_equals_the_walk(isx, orc, axes, resp_global):
    w = _side_conditions(orc, isx)
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    rs = isx.response_spec(*axes)
    try:
        isx.set_option("resp_global", resp_global)
        _equal(isx.scene_response(cfg, spec, rs, N_SIDE, SEED), w, oc, rs)
    finally:
        _reset(isx)


@pytest.mark.parametrize("resp_global", [0, 1], ids=["default-form", "global-form"])
@pytest.mark.parametrize("first", [0, CROSSING], ids=["first-0", "across-2^32"])
def test_photometer_at_1e6_rays_equals_the_walk(isx, orc, first, resp_global):
    """rspec (1, 1, 6, 12); with first_ray 2^32 - 500 000 the high word of the stream-3 counter changes inside one launch"""
    w = _scene_row(orc, "photometer", 0.95, first, 170.0)
    _reset(isx)
    cfg, spec = _case(isx, "photometer", 0.95)
    oc, _ = _case(orc, "photometer", 0.95)
    rs = isx.default_response_spec(cfg)
    assert list(rs.n) == [1, 1, 6, 12]
    want = R.from_walk(w, oc, rs, SEED, first)
    cols, det = want.sum(axis=0), want[0]
    print("launches per bin", int(cols.min()), int(cols.max()), "on the detector", int(det.min()), int(det.max()))
    assert int(cols.min()) > 13000 and int(det.min()) > 300
    try:
        isx.set_option("resp_global", resp_global)
        _equal(isx.scene_response(cfg, spec, rs, N, SEED, first_ray=first), w, oc, rs, first)
    finally:
        _reset(isx)


@pytest.mark.parametrize("axes", [(1, 1, 16, 16), (1, 1, 16, 17)], ids=["2816-words", "2992-words"])
def test_photometer_at_the_lds_forms_limit(isx, orc, axes):
    """the threshold between the two forms for a 640-thread workgroup (two of them share a CU's 160 KiB; about 2860 words are
    free in each): 256 bins x 11 slots is the largest block of this scene that fits, 272 x 11 takes the global adds"""
    w = _scene_row(orc, "photometer", 0.95, 0, 170.0)
    _reset(isx)
    cfg, spec = _case(isx, "photometer", 0.95)
    oc, _ = _case(orc, "photometer", 0.95)
    rs = isx.response_spec(*axes)
    _equal(isx.scene_response(cfg, spec, rs, N, SEED), w, oc, rs)


# ---------------------------------------------------------------- invariance
def test_partition_invariance(isx, orc):
    """20 000 rays as 7 001 + 12 999: the response, the counters and the census add up to the whole, which is the walk's"""
    w = _side_conditions(orc, isx)
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    rs = isx.response_spec(*SIDE_SPEC)
    a = isx.scene_response(cfg, spec, rs, 7001, SEED, first_ray=0)
    b = isx.scene_response(cfg, spec, rs, 12999, SEED, first_ray=7001)
    assert a[2].launched == 7001 and b[2].launched == 12999
    assert np.array_equal(a[0] + b[0], R.from_walk(w, oc, rs, SEED, 0))
    assert np.array_equal(a[1].words() + b[1].words(), SC.counter_words(w))
    for f in CENSUS:
        assert getattr(a[2], f) + getattr(b[2], f) == w["census"][f], f
    for part in (a, b):
        _identities(*part)


@pytest.mark.parametrize("shape", [{"grid_blocks": 1}, {"assist_block": 256}, {"assist_block": 768}, {"pipeline_chunk": 4096},
                                   {"ray_sub": 64}, {"rays_per_lane": 1}, {"assist": 0}, {"pipeline": 0}, {"bin_mode": 0}],
                         ids=lambda s: "%s=%d" % next(iter(s.items())))
@pytest.mark.parametrize("axes", [SIDE_SPEC, SMALL_SPEC], ids=["3x5x7x11", "2x1x3x2"])
def test_launch_shape_invariance(isx, orc, axes, shape):
    """one workgroup, other workgroup sizes, launches of 4096 rays, and the switches that select routes elsewhere: one route,
    the walk's result"""
    w = _side_conditions(orc, isx)
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    rs = isx.response_spec(*axes)
    try:
        for k, v in shape.items():
            isx.set_option(k, v)
        _equal(isx.scene_response(cfg, spec, rs, N_SIDE, SEED), w, oc, rs)
    finally:
        _reset(isx)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_ray_counts(isx, orc, n):
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    rs = isx.response_spec(*SIDE_SPEC)
    resp, cnt, st = isx.scene_response(cfg, spec, rs, n, SEED)
    if n == 0:
        assert not resp.any() and not cnt.words().any() and st.launched == 0 and st.bin_increments == 0 and st.wall_hits == 0
        return
    _equal((resp, cnt, st), _side_walk(orc, n), oc, rs)
    # ... and they are the first n rays of the 20 000
    big = _side_walk(orc)
    assert np.array_equal(np.nonzero(resp.reshape(-1))[0],
                          np.unique(R.fates(big, oc)[:n] * rs.bins + R.bins(rs, SEED, 0, N_SIDE)[:n]))


# ---------------------------------------------------------------- against isx_fluxmap_scene
@pytest.mark.parametrize("name,rho,n", [("empty", 0.99, 200_000), ("photometer", 0.95, 100_000), ("led_first_in", 0.95, 100_000),
                                        ("full", 0.95, 100_000), ("only_patches", 0.99, 100_000)],
                         ids=["default-scene", "photometer", "led_first_in", "full", "only_patches"])
def test_counts_and_census_are_the_flux_maps(isx, name, rho, n):
    """GPU against GPU: the 36 counters and every field of the census but bin_increments are isx_fluxmap_scene's for the same
    call -- the default scene (the pencil as the degenerate beam, nothing in the cavity) among them -- and the identities hold"""
    _reset(isx)
    cfg, spec = _case(isx, name, rho)
    rs = isx.default_response_spec(cfg)
    _, fcnt, fst = isx.fluxmap_scene(cfg, spec, n, SEED)
    resp, cnt, st = isx.scene_response(cfg, spec, rs, n, SEED)
    assert np.array_equal(cnt.words(), fcnt.words())
    for f in CENSUS:
        assert getattr(st, f) == getattr(fst, f), f
    assert st.launched == n and st.counted_below_z > 100
    _identities(resp, cnt, st)
    P, nb = spec.patches.n_patches, spec.baffles.n_baffles
    rows = resp.sum(axis=1)
    assert not rows[P + 2:10].any() and not rows[10 + 2 * nb:18].any()
    # the bins are the source's sample space whatever the beam makes of it: every bin gets its share of the launches
    cols = resp.sum(axis=0).astype(np.float64)
    assert np.abs(cols - n / 72.0).max() < 6.0 * np.sqrt(n / 72.0)
    # the detector grid and the hit line play no part
    odd = cfg.copy(); odd.n_theta, odd.n_phi, odd.hit_line_mode = 36000, 36000, 1
    resp2, cnt2, st2 = isx.scene_response(odd, spec, rs, n, SEED)
    assert np.array_equal(resp2, resp) and np.array_equal(cnt2.words(), cnt.words()) and st2.wall_hits == st.wall_hits


# ---------------------------------------------------------------- the device form, the sharded call
def test_device_form_accumulates():
    """isx_scene_response_device twice into one buffer == twice the blocking result on top of what was there, and
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
for axes, g in (((3, 5, 7, 11), 0), ((2, 1, 3, 2), 0), ((2, 1, 3, 2), 1)):
    isx.set_option("resp_global", g)
    rs = isx.response_spec(*axes)
    nw = 21 * rs.bins
    d_resp = torch.arange(5, 5 + nw, dtype=torch.int64, device="cuda:0")
    d_cnt = torch.arange(100, 136, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):
        isx.scene_response_device(cfg, spec, rs, 20000, SEED, 0, d_resp.data_ptr(), d_cnt.data_ptr())
    isx.sync()
    st = isx.take_stats()
    resp, cnt, bst = isx.scene_response(cfg, spec, rs, 20000, SEED)
    torch.cuda.synchronize()
    assert np.array_equal(d_resp.cpu().numpy() - np.arange(5, 5 + nw), 2 * resp.reshape(-1).astype(np.int64))
    assert np.array_equal(d_cnt.cpu().numpy() - np.arange(100, 136), 2 * cnt.words().astype(np.int64))
    for f in ("launched", "exited", "counted_below_z", "absorbed", "suspended", "wall_hits", "bin_increments"):
        assert getattr(st, f) == 2 * getattr(bst, f), f
    assert int(resp.sum()) == 20000 and resp.sum(axis=1)[[0, 1, 2, 3, 10, 11, 12, 13, 18, 19, 20]].min() >= 40
for rp, cp in ((0, d_cnt.data_ptr()), (d_resp.data_ptr(), 0)):
    try:
        isx.scene_response_device(cfg, spec, rs, 10, SEED, 0, rp, cp)
        raise SystemExit("a NULL pointer was accepted")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_BAD_ARG
isx.shutdown()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]


def test_scene_response_sharded_one_rank_equals_scene_response(isx):
    _reset(isx)
    cfg, spec = _side(isx)
    rs = isx.response_spec(*SIDE_SPEC)
    resp, cnt, st = isx.scene_response(cfg, spec, rs, N_SIDE, SEED)
    sresp, pa, pb, ba, bb, sc = isx.scene_response_sharded(isx.scene_response, cfg, spec, rs, N_SIDE, SEED)
    assert np.array_equal(sresp, resp) and int(resp.sum()) == N_SIDE
    for got, want in zip((pa, pb, ba, bb), cnt.arrays()):
        assert np.array_equal(got, want)
    for f in CENSUS + ("bin_increments",):
        assert sc[f] == getattr(st, f), f
