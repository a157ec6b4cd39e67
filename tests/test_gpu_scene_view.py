"""The scene view on the GPU: isx_scene_view bit for bit against the restatement of include/isx.h on the oracle's native scene
walk (tests/view_np.py on isxo_scene_walk) -- the map, its four counters, the 36 scene counters and the census -- in both forms of
the kernel (the workgroup's LDS map and the global adds), across 2^32 inside one launch, under every cut and launch shape; against
isx_fluxmap_scene for counts and census; the device form and the sharded call.

The conditions on the walk -- the detector of `photometer` sees no direct light and that of `lamp_open` does, rays arrive from
behind a wide cap, half the directions lie outside a map of half extent 0.5, un-normalised chords and unit vectors are both among
the directions -- are asserted on the oracle alone before the library is looked at.  Every walk is computed once per key, shared,
never changed."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scene_np as SC
import test_gpu_baffle as TB
import view_np as V
from test_gpu_scene import _case
from test_gpu_scene_response import N_SIDE, _side, _side_walk
from test_gpu_scene_walk import CROSSING, LONG, N, _row_case, _scene_row, _walked
from test_scene_cpu import parts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
CENSUS = SC.CENSUS_FIELDS
FORMS = pytest.mark.parametrize("view_global", [0, 1], ids=["default-form", "global-form"])


def _reset(isx):
    TB._reset(isx)
    isx.set_option("view_global", 0)


def _wide_cap(mod, rho=0.95):
    """the lamp and `screen` with a wide cap (60 degrees about +y, reflectance 0.5) as patch 0, then `det`"""
    import altair_raytracing_amd as isx
    c = mod.default_config()
    c.reflectance = rho
    ic = isx.default_config()
    p = parts(isx, ic)
    return c, isx.scene_spec(ic, p["lamp"], [p["screen"]], [isx.wall_patch_cap(ic, (0, 1, 0), 60.0, 0.5), p["det"]])


def _row(mod, name):
    return _wide_cap(mod) if name == "wide_cap" else _case(mod, name, 0.95)


def _row_walk(orc, name, first=0):
    if name in ("photometer", "full"):      # (shared with test_gpu_scene_walk.py and test_gpu_scene_response.py)
        return _scene_row(orc, name, 0.95, first, 170.0)
    oc, spec = _row(orc, name)
    return _walked(orc, ("view", name, first), oc, SC.spec_of(spec), N, SEED, first)


def _counts_of(w, oc, spec, patch, h):
    import altair_raytracing_amd as isx
    vs = isx.view_frame(isx.default_config(), spec, patch, 32, 32, h)
    return V.from_walk(w, oc, vs)


# (scene, patch): the rows of the proposal's table
ROWS = [("photometer", 0), ("photometer", 1), ("lamp_open", 0), ("led_first_in", 1), ("wide_cap", 0)]
ROW_IDS = ["photometer-det", "photometer-sample", "lamp_open-det", "led_first_in-sample", "wide_cap"]
_conditions_done = set()


def _row_conditions(orc, name, patch):
    """on the walk alone (1e6 rays, seed 12345, wall 0.95), with the frame of isx_view_frame on a 32 x 32 map"""
    w = _row_walk(orc, name)
    if (name, patch) in _conditions_done:
        return w
    oc, spec = _row(orc, name)
    view1, c1 = _counts_of(w, oc, spec, patch, 1.0)
    _, c5 = _counts_of(w, oc, spec, patch, 0.5)
    sel = int(c1.sum())
    print(name, "patch", patch, "absorbed", sel, "binned / outside / behind / direct at h = 1", c1.tolist(), "at h = 0.5", c5.tolist(),
          "fullest bin", int(view1.max()))
    assert c1[V.OUTSIDE] == 0 and c5[V.DIRECT] == c1[V.DIRECT] and c5[V.BEHIND] == c1[V.BEHIND]
    if (name, patch) == ("photometer", 0):
        assert sel >= 20000 and c1[V.DIRECT] == 0
    if (name, patch) == ("lamp_open", 0):
        assert c1[V.DIRECT] >= 1000
    if (name, patch) == ("photometer", 1):
        assert c1[V.DIRECT] >= 1000 and c1[V.BEHIND] >= 50 and c5[V.OUTSIDE] >= 10000
        # both the tracers' un-normalised chords and the assist wave's unit vectors are among the binned directions
        import altair_raytracing_amd as isx
        vs = isx.view_frame(isx.default_config(), spec, patch, 32, 32, 1.0)
        s = V.selected(w, oc, vs)
        branch, _ = V.classify(vs, w["n_points"][s], w["direction"][s])
        mag = np.sqrt((w["direction"][s][branch == V.BINNED] ** 2).sum(axis=1))
        off = np.abs(mag - 1.0) > 1e-9
        print("binned directions: |d| from", float(mag.min()), "to", float(mag.max()), "; unit to 1e-9:", int((~off).sum()))
        assert off.any() and (~off).any()
    if name == "wide_cap":
        assert c1[V.BEHIND] >= 10000
    _conditions_done.add((name, patch))
    return w


def _equal(got, w, oc, vs):
    view, vc, cnt, st = got
    want_view, want_counts = V.from_walk(w, oc, vs)
    assert view.dtype == np.uint64 and view.shape == want_view.shape == (vs.n_v, vs.n_u)
    assert np.array_equal(vc.words(), want_counts), (vc.words().tolist(), want_counts.tolist())
    assert np.array_equal(view, want_view)
    assert np.array_equal(cnt.words(), SC.counter_words(w))
    for f in CENSUS:
        assert getattr(st, f) == w["census"][f], f
    _identities(view, vc, cnt, st, vs.patch)


def _identities(view, vc, cnt, st, patch):
    pa, pb, ba, bb = cnt.arrays()
    assert vc.binned + vc.outside + vc.behind + vc.direct == int(pb[patch])
    assert int(view.sum()) == vc.binned == st.bin_increments
    assert int(pa.sum()) + int(ba.sum()) == st.wall_hits and int(pb.sum()) + int(bb.sum()) == st.absorbed
    assert st.exited + st.absorbed + st.suspended == st.launched


# ---------------------------------------------------------------- parity with the walk, both forms
@FORMS
@pytest.mark.parametrize("h", [1.0, 0.5], ids=["h=1", "h=0.5"])
@pytest.mark.parametrize("name,patch", ROWS, ids=ROW_IDS)
def test_rows_at_1e6_rays_equal_the_walk(isx, orc, name, patch, h, view_global):
    w = _row_conditions(orc, name, patch)
    _reset(isx)
    cfg, spec = _row(isx, name)
    oc, _ = _row(orc, name)
    vs = isx.view_frame(cfg, spec, patch, 32, 32, h)
    try:
        isx.set_option("view_global", view_global)
        _equal(isx.scene_view(cfg, spec, vs, N, SEED), w, oc, vs)
    finally:
        _reset(isx)


@FORMS
def test_photometer_across_2_32_equals_the_walk(isx, orc, view_global):
    """first_ray 2^32 - 500 000: the high word of the ray index changes inside one launch"""
    w = _scene_row(orc, "photometer", 0.95, CROSSING, 170.0)
    _reset(isx)
    cfg, spec = _case(isx, "photometer", 0.95)
    oc, _ = _case(orc, "photometer", 0.95)
    vs = isx.view_frame(cfg, spec, 0, 32, 32)
    assert int(w["patch_absorbed"][0]) >= 20000
    try:
        isx.set_option("view_global", view_global)
        _equal(isx.scene_view(cfg, spec, vs, N, SEED, first_ray=CROSSING), w, oc, vs)
    finally:
        _reset(isx)


@FORMS
@pytest.mark.parametrize("n_u,n_v", [(1, 1), (32, 32), (7, 13), (256, 256)], ids=["1x1", "32x32", "7x13", "256x256"])
@pytest.mark.parametrize("patch", [0, 1])
def test_side_photometer_equals_the_walk(isx, orc, patch, n_u, n_v, view_global):
    """`side_photometer` of test_gpu_scene_response.py (20 000 rays, at most 30 points per ray: rays end in every slot); a map of
    one bin, an odd one, and one that only the global form holds"""
    w = _side_walk(orc)
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    vs = isx.view_frame(cfg, spec, patch, n_u, n_v)
    assert int(w["patch_absorbed"][patch]) >= 40 and w["census"]["suspended"] >= 40
    try:
        isx.set_option("view_global", view_global)
        _equal(isx.scene_view(cfg, spec, vs, N_SIDE, SEED), w, oc, vs)
    finally:
        _reset(isx)


@pytest.mark.parametrize("patch", [7, 0])
def test_full_equals_the_walk(isx, orc, patch):
    """8 patches + 4 baffles: the last class (reflectance 1: it absorbs nothing) and the first (reflectance 0)"""
    w = _scene_row(orc, "full", 0.95, 0, 170.0)
    _reset(isx)
    cfg, spec = _case(isx, "full", 0.95)
    oc, _ = _case(orc, "full", 0.95)
    vs = isx.view_frame(cfg, spec, patch, 32, 32)
    assert int(w["patch_arrivals"][patch]) >= 1000 and (int(w["patch_absorbed"][patch]) >= 1000 if patch == 0 else int(w["patch_absorbed"][patch]) == 0)
    _equal(isx.scene_view(cfg, spec, vs, N, SEED), w, oc, vs)


# ---------------------------------------------------------------- edges
N_EDGE = 100_000


def _lamp_with(mod, caps, rho=0.95):
    import altair_raytracing_amd as isx
    c = mod.default_config()
    c.reflectance = rho
    ic = isx.default_config()
    return c, isx.scene_spec(ic, parts(isx, ic)["lamp"], [], [isx.wall_patch_cap(ic, *cap) for cap in caps])


@FORMS
def test_an_overlapped_cap_sees_nothing(isx, orc, view_global):
    """two identical caps: every arrival is the lower index's, the higher one selected has all four counters 0"""
    caps = [((0, 1, 0), 20.0, 0.3), ((0, 1, 0), 20.0, 0.3)]
    oc, spec = _lamp_with(orc, caps)
    w = _walked(orc, ("view", "twin_caps"), oc, SC.spec_of(spec), N_EDGE, SEED)
    assert int(w["patch_absorbed"][0]) >= 1000 and int(w["patch_absorbed"][1]) == 0 and int(w["patch_arrivals"][1]) == 0
    _reset(isx)
    cfg, spec = _lamp_with(isx, caps)
    try:
        isx.set_option("view_global", view_global)
        for patch in (1, 0):
            vs = isx.view_frame(cfg, spec, patch, 32, 32)
            got = isx.scene_view(cfg, spec, vs, N_EDGE, SEED)
            _equal(got, w, oc, vs)
            if patch == 1:
                assert not got[0].any() and not got[1].words().any() and got[3].bin_increments == 0
    finally:
        _reset(isx)


def test_a_white_patch_sees_nothing(isx, orc):
    """a selected patch of reflectance 1 absorbs no ray: all 0"""
    caps = [((0, 1, 0), 20.0, 1.0), ((1, 0, 0), 5.0, 0.0)]
    oc, spec = _lamp_with(orc, caps)
    w = _walked(orc, ("view", "white_cap"), oc, SC.spec_of(spec), N_EDGE, SEED)
    assert int(w["patch_arrivals"][0]) >= 1000 and int(w["patch_absorbed"][0]) == 0
    _reset(isx)
    cfg, spec = _lamp_with(isx, caps)
    vs = isx.view_frame(cfg, spec, 0, 32, 32)
    got = isx.scene_view(cfg, spec, vs, N_EDGE, SEED)
    _equal(got, w, oc, vs)
    assert not got[0].any() and not got[1].words().any()


@FORMS
def test_black_every_selected_ray_is_direct(isx, orc, view_global):
    """`black` of test_gpu_scene.py: every reflectance 0, every ray ends at its first interaction"""
    oc, spec = _case(orc, "black")
    w = _walked(orc, ("view", "black"), oc, SC.spec_of(spec), N_EDGE, SEED)
    assert int(w["n_points"].max()) == 2 and int(w["patch_absorbed"][1]) >= 100
    _reset(isx)
    cfg, spec = _case(isx, "black")
    try:
        isx.set_option("view_global", view_global)
        for patch in (1, 0):      # (the screen shadows patch 0: nothing at all)
            vs = isx.view_frame(cfg, spec, patch, 32, 32)
            got = isx.scene_view(cfg, spec, vs, N_EDGE, SEED)
            _equal(got, w, oc, vs)
            assert got[1].direct == int(w["patch_absorbed"][patch]) and got[1].binned == got[1].outside == got[1].behind == 0
    finally:
        _reset(isx)


@pytest.mark.parametrize("n_u,n_v", [(44, 64), (52, 55), (53, 54), (44, 68)], ids=["2816-words", "2860-words", "2862-words", "2992-words"])
def test_photometer_at_the_lds_forms_limit(isx, orc, n_u, n_v):
    """the threshold between the two forms for a 640-thread workgroup (two of them share a CU's 160 KiB; 80 KiB less the scene's
    70 464 B and the four counters leave 2860 words): 52 x 55 is the largest map that fits, 53 x 54 (2864 words once rounded to
    16 B) takes the global adds; and the pair the response's test uses, clear of the limit on either side"""
    w = _scene_row(orc, "photometer", 0.95, 0, 170.0)
    _reset(isx)
    cfg, spec = _case(isx, "photometer", 0.95)
    oc, _ = _case(orc, "photometer", 0.95)
    vs = isx.view_frame(cfg, spec, 1, n_u, n_v)
    _equal(isx.scene_view(cfg, spec, vs, N, SEED), w, oc, vs)


# ---------------------------------------------------------------- invariance
def test_one_workgroup_with_full_rings_equals_the_walk(isx, orc):
    """the row of the long rays of test_gpu_scene_walk.py through ONE workgroup (`grid_blocks` 1)"""
    w = _scene_row(orc, *LONG)
    name, rho, first, theta = LONG
    _reset(isx)
    cfg, spec = _row_case(isx, name, rho, theta)
    oc, _ = _row_case(orc, name, rho, theta)
    vs = isx.view_frame(cfg, spec, 1, 32, 32)
    assert int(w["patch_absorbed"][1]) >= 1000
    try:
        isx.set_option("grid_blocks", 1)
        _equal(isx.scene_view(cfg, spec, vs, N, SEED), w, oc, vs)
    finally:
        _reset(isx)


@pytest.mark.parametrize("shape", TB.SHAPES, ids=lambda s: "%s=%d" % next(iter(s.items())))
def test_launch_shape_invariance(isx, orc, shape):
    """other workgroup sizes, launches of 4096 rays, and the switches that select routes elsewhere: one route, the walk's
    result, in both forms"""
    w = _side_walk(orc)
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    vs = isx.view_frame(cfg, spec, 1, 32, 32)
    try:
        for g in (0, 1):
            for k, v in shape.items():
                isx.set_option(k, v)
            isx.set_option("view_global", g)
            _equal(isx.scene_view(cfg, spec, vs, N_SIDE, SEED), w, oc, vs)
    finally:
        _reset(isx)


def test_partition_invariance(isx, orc):
    """20 000 rays cut in three, and in launches of 4096 rays (`pipeline_chunk`): the map, the counters and the census add up to
    the whole, which is the walk's"""
    w = _side_walk(orc)
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    vs = isx.view_frame(cfg, spec, 1, 7, 13, 0.5)
    want_view, want_counts = V.from_walk(w, oc, vs)
    assert want_counts[V.BINNED] >= 100 and want_counts[V.OUTSIDE] >= 100
    cuts = [(0, 7001), (7001, 63), (7064, N_SIDE - 7064)]
    got = [isx.scene_view(cfg, spec, vs, n, SEED, first_ray=first) for first, n in cuts]
    assert [g[3].launched for g in got] == [n for _, n in cuts]
    assert np.array_equal(sum(g[0] for g in got), want_view)
    assert np.array_equal(sum(g[1].words() for g in got), want_counts)
    assert np.array_equal(sum(g[2].words() for g in got), SC.counter_words(w))
    for f in CENSUS:
        assert sum(getattr(g[3], f) for g in got) == w["census"][f], f
    for g in got:
        _identities(g[0], g[1], g[2], g[3], 1)
    try:
        isx.set_option("pipeline_chunk", 4096)
        _equal(isx.scene_view(cfg, spec, vs, N_SIDE, SEED), w, oc, vs)
    finally:
        _reset(isx)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_ray_counts(isx, orc, n):
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    vs = isx.view_frame(cfg, spec, 1, 32, 32)
    view, vc, cnt, st = isx.scene_view(cfg, spec, vs, n, SEED)
    if n == 0:
        assert not view.any() and not vc.words().any() and not cnt.words().any() and st.launched == 0 and st.bin_increments == 0
        return
    _equal((view, vc, cnt, st), _side_walk(orc, n), oc, vs)


# ---------------------------------------------------------------- against isx_fluxmap_scene
@pytest.mark.parametrize("name,patch,n", [("photometer", 0, 100_000), ("led_first_in", 1, 100_000), ("full", 5, 100_000),
                                          ("only_patches", 1, 100_000)], ids=["photometer", "led_first_in", "full", "only_patches"])
def test_counts_and_census_are_the_flux_maps(isx, name, patch, n):
    """GPU against GPU: the 36 counters and every field of the census but bin_increments are isx_fluxmap_scene's for the same
    call, and the identities hold; the detector grid and the hit line play no part"""
    _reset(isx)
    cfg, spec = _case(isx, name, 0.99 if name == "only_patches" else 0.95)
    vs = isx.view_frame(cfg, spec, patch, 32, 32)
    _, fcnt, fst = isx.fluxmap_scene(cfg, spec, n, SEED)
    view, vc, cnt, st = isx.scene_view(cfg, spec, vs, n, SEED)
    assert np.array_equal(cnt.words(), fcnt.words())
    for f in CENSUS:
        assert getattr(st, f) == getattr(fst, f), f
    assert st.launched == n and vc.binned > 100
    _identities(view, vc, cnt, st, patch)
    odd = cfg.copy(); odd.n_theta, odd.n_phi, odd.hit_line_mode = 36000, 36000, 1
    view2, vc2, cnt2, st2 = isx.scene_view(odd, spec, vs, n, SEED)
    assert np.array_equal(view2, view) and np.array_equal(vc2.words(), vc.words()) and np.array_equal(cnt2.words(), cnt.words())
    assert st2.wall_hits == st.wall_hits


# ---------------------------------------------------------------- the device form, the sharded call
def test_device_form_accumulates():
    """isx_scene_view_device twice into one set of buffers == twice the blocking result on top of what was there, and
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
for (n_u, n_v), g in (((32, 32), 0), ((32, 32), 1), ((256, 256), 0)):
    isx.set_option("view_global", g)
    vs = isx.view_frame(cfg, spec, 1, n_u, n_v)
    nw = n_u * n_v
    d_view = torch.arange(5, 5 + nw, dtype=torch.int64, device="cuda:0")
    d_vc = torch.arange(50, 54, dtype=torch.int64, device="cuda:0")
    d_cnt = torch.arange(100, 136, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):
        isx.scene_view_device(cfg, spec, vs, 20000, SEED, 0, d_view.data_ptr(), d_vc.data_ptr(), d_cnt.data_ptr())
    isx.sync()
    st = isx.take_stats()
    view, vc, cnt, bst = isx.scene_view(cfg, spec, vs, 20000, SEED)
    torch.cuda.synchronize()
    assert np.array_equal(d_view.cpu().numpy() - np.arange(5, 5 + nw), 2 * view.reshape(-1).astype(np.int64))
    assert np.array_equal(d_vc.cpu().numpy() - np.arange(50, 54), 2 * vc.words().astype(np.int64))
    assert np.array_equal(d_cnt.cpu().numpy() - np.arange(100, 136), 2 * cnt.words().astype(np.int64))
    for f in ("launched", "exited", "counted_below_z", "absorbed", "suspended", "wall_hits", "bin_increments"):
        assert getattr(st, f) == 2 * getattr(bst, f), f
    assert int(view.sum()) == vc.binned > 100
for k in range(3):
    p = [d_view.data_ptr(), d_vc.data_ptr(), d_cnt.data_ptr()]
    p[k] = 0
    try:
        isx.scene_view_device(cfg, spec, vs, 10, SEED, 0, *p)
        raise SystemExit("a NULL pointer was accepted")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_BAD_ARG
isx.shutdown()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]


def test_scene_view_sharded_one_rank_equals_scene_view(isx):
    _reset(isx)
    cfg, spec = _side(isx)
    vs = isx.view_frame(cfg, spec, 1, 7, 13, 0.5)
    view, vc, cnt, st = isx.scene_view(cfg, spec, vs, N_SIDE, SEED)
    sview, svc, pa, pb, ba, bb, sc = isx.scene_view_sharded(isx.scene_view, cfg, spec, vs, N_SIDE, SEED)
    assert np.array_equal(sview, view) and np.array_equal(svc, vc.words()) and int(view.sum()) == vc.binned > 100
    for got, want in zip((pa, pb, ba, bb), cnt.arrays()):
        assert np.array_equal(got, want)
    for f in CENSUS + ("bin_increments",):
        assert sc[f] == getattr(st, f), f
