"""The scene patch field on the GPU: isx_scene_patch_field bit for bit against the restatement of include/isx.h on the oracle's
native scene walk (tests/field_np.py on isxo_scene_walk) -- the field, its five counters, the 36 scene counters and the census --
in both forms of the kernel (the workgroup's LDS field and the global adds), across 2^32 inside one launch, under every cut and
launch shape; against isx_scene_view and the position marginal, GPU against GPU; against isx_fluxmap_scene for counts and census;
the device form and the sharded call.

The conditions on the walk -- how many rays the two patches of `photometer` absorb, that the helper's scale keeps every position
inside the unit disc and twice that scale puts many outside, that rays arrive from behind a wide cap -- are asserted on the oracle
alone before the library is looked at.  Every walk is computed once per key, shared, never changed (the fixtures of
test_gpu_scene_view.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import field_np as F
import scene_np as SC
import test_gpu_baffle as TB
from test_gpu_scene import _case
from test_gpu_scene_response import N_SIDE, _side, _side_walk
from test_gpu_scene_view import ROWS, ROW_IDS, _row, _row_walk
from test_gpu_scene_walk import CROSSING, LONG, N, _row_case, _scene_row

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
CENSUS = SC.CENSUS_FIELDS
FORMS = pytest.mark.parametrize("field_global", [0, 1], ids=["default-form", "global-form"])
AXES = [(8, 8, 16, 16), (3, 5, 7, 2)]
AXES_IDS = ["8x8x16x16", "3x5x7x2"]


def _reset(isx):
    TB._reset(isx)
    isx.set_option("field_global", 0)
    isx.set_option("view_global", 0)


def _frame(patch, spec, axes, h=1.0, scale=1.0):
    """isx_patch_field_frame's spec (host only) with its pos_scale times `scale`"""
    import altair_raytracing_amd as isx
    fs = isx.patch_field_frame(isx.default_config(), spec, patch, *axes, h)
    fs.pos_scale = fs.pos_scale * scale
    return fs


_conditions_done = set()


def _row_conditions(orc, name, patch):
    """on the walk alone (1e6 rays, seed 12345, wall 0.95), at (8, 8, 16, 16) with the helper's scale and twice it"""
    w = _row_walk(orc, name)
    if (name, patch) in _conditions_done:
        return w
    oc, spec = _row(orc, name)
    f1 = _frame(patch, spec, AXES[0])
    f2 = _frame(patch, spec, AXES[0], 1.0, 2.0)
    _, c1 = F.from_walk(w, oc, f1)
    _, c2 = F.from_walk(w, oc, f2)
    sel = F.selected(w, oc, f1)
    X, Y = F.position(f1, oc.r_in, w["last_point"][sel])
    rmax = float(np.sqrt(X * X + Y * Y).max()) if sel.any() else 0.0
    print(name, "patch", patch, "selected", int(sel.sum()), "binned / pos_outside / dir_outside / behind / direct", c1.tolist(),
          "at twice the scale", c2.tolist(), "largest radius", rmax)
    assert c1[F.POS_OUTSIDE] == 0 and rmax <= 1.0 and c2[F.DIRECT] == c1[F.DIRECT] and c2[F.BEHIND] == c1[F.BEHIND]
    if (name, patch) == ("photometer", 0):
        assert int(sel.sum()) == 28228 and c1[F.DIRECT] == 0 and c1[F.BEHIND] == 0 and 0.999 <= rmax < 1.0
        assert c2[F.POS_OUTSIDE] >= 10000
    if (name, patch) == ("photometer", 1):
        assert int(sel.sum()) == 60110 and c1[F.DIRECT] == 3513
        assert c2[F.POS_OUTSIDE] >= 10000
    if name == "wide_cap":
        assert c1[F.BEHIND] >= 10000
    _conditions_done.add((name, patch))
    return w


def _equal(got, w, oc, fs):
    field, fc, cnt, st = got
    want_field, want_counts = F.from_walk(w, oc, fs)
    assert field.dtype == np.uint64 and field.shape == want_field.shape == (fs.n_y, fs.n_x, fs.n_v, fs.n_u)
    assert np.array_equal(fc.words(), want_counts), (fc.words().tolist(), want_counts.tolist())
    assert np.array_equal(field, want_field)
    assert np.array_equal(cnt.words(), SC.counter_words(w))
    for f in CENSUS:
        assert getattr(st, f) == w["census"][f], f
    _identities(field, fc, cnt, st, fs.patch)


def _identities(field, fc, cnt, st, patch):
    pa, pb, ba, bb = cnt.arrays()
    assert fc.binned + fc.pos_outside + fc.dir_outside + fc.behind + fc.direct == int(pb[patch])
    assert int(field.sum()) == fc.binned == st.bin_increments
    assert int(pa.sum()) + int(ba.sum()) == st.wall_hits and int(pb.sum()) + int(bb.sum()) == st.absorbed
    assert st.exited + st.absorbed + st.suspended == st.launched


# ---------------------------------------------------------------- parity with the walk, both forms
@FORMS
@pytest.mark.parametrize("axes", AXES, ids=AXES_IDS)
@pytest.mark.parametrize("name,patch", ROWS, ids=ROW_IDS)
def test_rows_at_1e6_rays_equal_the_walk(isx, orc, name, patch, axes, field_global):
    """the five rows of the view's table, at h = 1 and 0.5, with the helper's scale and twice it"""
    w = _row_conditions(orc, name, patch)
    _reset(isx)
    cfg, spec = _row(isx, name)
    oc, _ = _row(orc, name)
    try:
        isx.set_option("field_global", field_global)
        for h in (1.0, 0.5):
            for scale in (1.0, 2.0):
                fs = _frame(patch, spec, axes, h, scale)
                _equal(isx.scene_patch_field(cfg, spec, fs, N, SEED), w, oc, fs)
    finally:
        _reset(isx)


@pytest.mark.parametrize("axes", [(2, 2, 353, 2), (2, 3, 157, 3)], ids=["2824-words", "2826-words"])
def test_photometer_at_the_lds_forms_limit(isx, orc, axes):
    """the threshold between the two forms for a 640-thread workgroup: two of them share a CU's 160 KiB, so each has 81 920 B;
    the scene's rings, tables and parks take 70 464 B and the field's head (the frame's 16 doubles and 8 counter words) 160 B:
    11 296 B = 2824 words are left.  2 x 2 x 353 x 2 = 2824 is the largest field that fits; 2 x 3 x 157 x 3 = 2826 (2828 words once
    rounded to 16 B) takes the global adds"""
    w = _scene_row(orc, "photometer", 0.95, 0, 170.0)
    _reset(isx)
    cfg, spec = _case(isx, "photometer", 0.95)
    oc, _ = _case(orc, "photometer", 0.95)
    fs = _frame(1, spec, axes, 1.0, 1.5)
    _equal(isx.scene_patch_field(cfg, spec, fs, N, SEED), w, oc, fs)


def test_a_field_of_2_22_bins(isx, orc):
    """64 x 64 x 32 x 32: the largest field, the global form"""
    w = _scene_row(orc, "photometer", 0.95, 0, 170.0)
    _reset(isx)
    cfg, spec = _case(isx, "photometer", 0.95)
    oc, _ = _case(orc, "photometer", 0.95)
    fs = _frame(1, spec, (64, 64, 32, 32))
    assert fs.bins == 1 << 22
    got = isx.scene_patch_field(cfg, spec, fs, N, SEED)
    _equal(got, w, oc, fs)
    assert got[1].binned >= 50000


@FORMS
def test_one_position_bin_is_the_scene_view(isx, field_global):
    """GPU against GPU: (1, 1, 32, 32) with pos_scale halved -- every position in range -- is isx_scene_view's map, dir_outside
    its `outside`, behind and direct its own; and at the helper's (8, 8, 32, 32) the direction marginal is that map"""
    _reset(isx)
    try:
        isx.set_option("field_global", field_global)
        for name, patch, h in (("photometer", 1, 1.0), ("photometer", 1, 0.5), ("wide_cap", 0, 1.0)):
            cfg, spec = _row(isx, name)
            vs = isx.view_frame(cfg, spec, patch, 32, 32, h)
            view, vc, vcnt, vst = isx.scene_view(cfg, spec, vs, N, SEED)
            fs = _frame(patch, spec, (1, 1, 32, 32), h, 0.5)
            field, fc, cnt, st = isx.scene_patch_field(cfg, spec, fs, N, SEED)
            assert fc.pos_outside == 0 and fc.binned > 10000
            assert np.array_equal(field.reshape(32, 32), view)
            assert (fc.binned, fc.dir_outside, fc.behind, fc.direct) == (vc.binned, vc.outside, vc.behind, vc.direct)
            assert np.array_equal(cnt.words(), vcnt.words()) and st.bin_increments == vst.bin_increments
            fs = _frame(patch, spec, (8, 8, 32, 32), h)
            field, fc, cnt, st = isx.scene_patch_field(cfg, spec, fs, N, SEED)
            pos, dr = isx.patch_field_marginals(fs, field)
            assert fc.pos_outside == 0 and np.array_equal(dr, view) and (fc.behind, fc.direct) == (vc.behind, vc.direct)
    finally:
        _reset(isx)


@FORMS
def test_one_direction_bin_is_the_position_marginal(isx, orc, field_global):
    """(8, 8, 1, 1) against the position marginal of (8, 8, 16, 16), GPU against GPU, and against the walk"""
    w = _row_walk(orc, "photometer")
    _reset(isx)
    cfg, spec = _row(isx, "photometer")
    oc, _ = _row(orc, "photometer")
    try:
        isx.set_option("field_global", field_global)
        for patch in (0, 1):
            fs1 = _frame(patch, spec, (8, 8, 1, 1))
            got = isx.scene_patch_field(cfg, spec, fs1, N, SEED)
            _equal(got, w, oc, fs1)
            fs = _frame(patch, spec, (8, 8, 16, 16))
            field, fc, _, _ = isx.scene_patch_field(cfg, spec, fs, N, SEED)
            pos, dr = isx.patch_field_marginals(fs, field)
            assert fc.dir_outside == 0 and got[1].dir_outside == 0      # (h = 1: every direction from the front is in the map)
            assert np.array_equal(got[0].reshape(8, 8), pos) and got[1].binned == fc.binned > 10000
    finally:
        _reset(isx)


@FORMS
def test_photometer_across_2_32_equals_the_walk(isx, orc, field_global):
    """first_ray 2^32 - 500 000: the high word of the ray index changes inside one launch"""
    w = _scene_row(orc, "photometer", 0.95, CROSSING, 170.0)
    _reset(isx)
    cfg, spec = _case(isx, "photometer", 0.95)
    oc, _ = _case(orc, "photometer", 0.95)
    fs = _frame(0, spec, AXES[0])
    assert int(w["patch_absorbed"][0]) >= 20000
    try:
        isx.set_option("field_global", field_global)
        _equal(isx.scene_patch_field(cfg, spec, fs, N, SEED, first_ray=CROSSING), w, oc, fs)
    finally:
        _reset(isx)


@FORMS
@pytest.mark.parametrize("axes", AXES + [(1, 1, 1, 1)], ids=AXES_IDS + ["1x1x1x1"])
@pytest.mark.parametrize("patch", [0, 1])
def test_side_photometer_equals_the_walk(isx, orc, patch, axes, field_global):
    """`side_photometer` of test_gpu_scene_response.py (20 000 rays, at most 30 points per ray: rays end in every slot)"""
    w = _side_walk(orc)
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    fs = _frame(patch, spec, axes, 0.75, 1.5)
    assert int(w["patch_absorbed"][patch]) >= 40 and w["census"]["suspended"] >= 40
    try:
        isx.set_option("field_global", field_global)
        _equal(isx.scene_patch_field(cfg, spec, fs, N_SIDE, SEED), w, oc, fs)
    finally:
        _reset(isx)


@pytest.mark.parametrize("patch", [7, 0])
def test_full_equals_the_walk(isx, orc, patch):
    """8 patches + 4 baffles: the last class (reflectance 1: it absorbs nothing, all zero) and the first (reflectance 0)"""
    w = _scene_row(orc, "full", 0.95, 0, 170.0)
    _reset(isx)
    cfg, spec = _case(isx, "full", 0.95)
    oc, _ = _case(orc, "full", 0.95)
    fs = _frame(patch, spec, AXES[0])
    assert int(w["patch_arrivals"][patch]) >= 1000 and (int(w["patch_absorbed"][patch]) >= 1000 if patch == 0 else int(w["patch_absorbed"][patch]) == 0)
    got = isx.scene_patch_field(cfg, spec, fs, N, SEED)
    _equal(got, w, oc, fs)
    if patch == 7:
        assert not got[0].any() and not got[1].words().any() and got[3].bin_increments == 0


@FORMS
def test_a_frame_that_is_not_the_patchs_own_is_used_as_given(isx, orc, field_global):
    """the frame and the scale of `det` on patch `sample`: positions far from the frame's axis, many rays from behind its plane"""
    w = _row_walk(orc, "photometer")
    _reset(isx)
    cfg, spec = _row(isx, "photometer")
    oc, _ = _row(orc, "photometer")
    fs = _frame(0, spec, AXES[1])
    fs.patch = 1
    _, want = F.from_walk(w, oc, fs)
    print("det's frame on sample: binned / pos_outside / dir_outside / behind / direct", want.tolist())
    assert want[F.DIRECT] == 3513 and want[F.BEHIND] + want[F.POS_OUTSIDE] >= 10000
    try:
        isx.set_option("field_global", field_global)
        _equal(isx.scene_patch_field(cfg, spec, fs, N, SEED), w, oc, fs)
    finally:
        _reset(isx)


# ---------------------------------------------------------------- invariance
def test_one_workgroup_with_full_rings_equals_the_walk(isx, orc):
    """the row of the long rays of test_gpu_scene_walk.py through ONE workgroup (`grid_blocks` 1)"""
    w = _scene_row(orc, *LONG)
    name, rho, first, theta = LONG
    _reset(isx)
    cfg, spec = _row_case(isx, name, rho, theta)
    oc, _ = _row_case(orc, name, rho, theta)
    fs = _frame(1, spec, AXES[0])
    assert int(w["patch_absorbed"][1]) >= 1000
    try:
        isx.set_option("grid_blocks", 1)
        _equal(isx.scene_patch_field(cfg, spec, fs, N, SEED), w, oc, fs)
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
    fs = _frame(1, spec, AXES[0], 0.75, 1.5)
    try:
        for g in (0, 1):
            for k, v in shape.items():
                isx.set_option(k, v)
            isx.set_option("field_global", g)
            _equal(isx.scene_patch_field(cfg, spec, fs, N_SIDE, SEED), w, oc, fs)
    finally:
        _reset(isx)


def test_partition_invariance(isx, orc):
    """20 000 rays cut in three, and in launches of 4096 rays (`pipeline_chunk`): the field, the counters and the census add up to
    the whole, which is the walk's"""
    w = _side_walk(orc)
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    fs = _frame(1, spec, AXES[1], 0.5, 1.5)
    want_field, want_counts = F.from_walk(w, oc, fs)
    assert want_counts[F.BINNED] >= 50 and want_counts[F.POS_OUTSIDE] >= 50 and want_counts[F.DIR_OUTSIDE] >= 50
    cuts = [(0, 7001), (7001, 63), (7064, N_SIDE - 7064)]
    got = [isx.scene_patch_field(cfg, spec, fs, n, SEED, first_ray=first) for first, n in cuts]
    assert [g[3].launched for g in got] == [n for _, n in cuts]
    assert np.array_equal(sum(g[0] for g in got), want_field)
    assert np.array_equal(sum(g[1].words() for g in got), want_counts)
    assert np.array_equal(sum(g[2].words() for g in got), SC.counter_words(w))
    for f in CENSUS:
        assert sum(getattr(g[3], f) for g in got) == w["census"][f], f
    for g in got:
        _identities(g[0], g[1], g[2], g[3], 1)
    try:
        isx.set_option("pipeline_chunk", 4096)
        _equal(isx.scene_patch_field(cfg, spec, fs, N_SIDE, SEED), w, oc, fs)
    finally:
        _reset(isx)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_ray_counts(isx, orc, n):
    _reset(isx)
    cfg, spec = _side(isx)
    oc, _ = _side(orc)
    fs = _frame(1, spec, AXES[0])
    field, fc, cnt, st = isx.scene_patch_field(cfg, spec, fs, n, SEED)
    if n == 0:
        assert not field.any() and not fc.words().any() and not cnt.words().any() and st.launched == 0 and st.bin_increments == 0
        return
    _equal((field, fc, cnt, st), _side_walk(orc, n), oc, fs)


# ---------------------------------------------------------------- against isx_fluxmap_scene
@pytest.mark.parametrize("name,patch,n", [("photometer", 0, 100_000), ("led_first_in", 1, 100_000), ("full", 5, 100_000),
                                          ("only_patches", 1, 100_000)], ids=["photometer", "led_first_in", "full", "only_patches"])
def test_counts_and_census_are_the_flux_maps(isx, name, patch, n):
    """GPU against GPU: the 36 counters and every field of the census but bin_increments are isx_fluxmap_scene's for the same
    call, and the identities hold; the detector grid and the hit line play no part"""
    _reset(isx)
    cfg, spec = _case(isx, name, 0.99 if name == "only_patches" else 0.95)
    fs = _frame(patch, spec, AXES[0])
    _, fcnt, fst = isx.fluxmap_scene(cfg, spec, n, SEED)
    field, fc, cnt, st = isx.scene_patch_field(cfg, spec, fs, n, SEED)
    assert np.array_equal(cnt.words(), fcnt.words())
    for f in CENSUS:
        assert getattr(st, f) == getattr(fst, f), f
    assert st.launched == n and fc.binned > 100
    _identities(field, fc, cnt, st, patch)
    odd = cfg.copy(); odd.n_theta, odd.n_phi, odd.hit_line_mode = 36000, 36000, 1
    field2, fc2, cnt2, st2 = isx.scene_patch_field(odd, spec, fs, n, SEED)
    assert np.array_equal(field2, field) and np.array_equal(fc2.words(), fc.words()) and np.array_equal(cnt2.words(), cnt.words())
    assert st2.wall_hits == st.wall_hits


# ---------------------------------------------------------------- the device form, the sharded call
def test_device_form_accumulates():
    """isx_scene_patch_field_device twice into one set of buffers == twice the blocking result on top of what was there, and
    isx_take_stats adds up; every NULL pointer is refused (a process of its own: torch owns the tensors, the library's stream does
    the work)."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import altair_raytracing_amd as isx
from test_gpu_scene_response import _side
isx.load(); isx.init(0)
cfg, spec = _side(isx)
SEED = 12345
for axes, g in (((8, 8, 16, 16), 0), ((8, 8, 16, 16), 1), ((3, 5, 7, 2), 0)):
    isx.set_option("field_global", g)
    fs = isx.patch_field_frame(cfg, spec, 1, *axes, 0.75)
    fs.pos_scale = fs.pos_scale * 1.5
    nw = fs.bins
    d_field = torch.arange(5, 5 + nw, dtype=torch.int64, device="cuda:0")
    d_fc = torch.arange(50, 55, dtype=torch.int64, device="cuda:0")
    d_cnt = torch.arange(100, 136, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):
        isx.scene_patch_field_device(cfg, spec, fs, 20000, SEED, 0, d_field.data_ptr(), d_fc.data_ptr(), d_cnt.data_ptr())
    isx.sync()
    st = isx.take_stats()
    field, fc, cnt, bst = isx.scene_patch_field(cfg, spec, fs, 20000, SEED)
    torch.cuda.synchronize()
    assert np.array_equal(d_field.cpu().numpy() - np.arange(5, 5 + nw), 2 * field.reshape(-1).astype(np.int64))
    assert np.array_equal(d_fc.cpu().numpy() - np.arange(50, 55), 2 * fc.words().astype(np.int64))
    assert np.array_equal(d_cnt.cpu().numpy() - np.arange(100, 136), 2 * cnt.words().astype(np.int64))
    for f in ("launched", "exited", "counted_below_z", "absorbed", "suspended", "wall_hits", "bin_increments"):
        assert getattr(st, f) == 2 * getattr(bst, f), f
    assert int(field.sum()) == fc.binned > 50 and fc.pos_outside > 50 and fc.dir_outside > 20
for k in range(3):
    p = [d_field.data_ptr(), d_fc.data_ptr(), d_cnt.data_ptr()]
    p[k] = 0
    try:
        isx.scene_patch_field_device(cfg, spec, fs, 10, SEED, 0, *p)
        raise SystemExit("a NULL pointer was accepted")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_BAD_ARG
isx.shutdown()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]


def test_null_pointers_of_the_blocking_form(isx):
    import ctypes as C
    _reset(isx)
    cfg, spec = _side(isx)
    fs = _frame(1, spec, AXES[1])
    lib = isx.load()
    buf = np.full(fs.bins, 7, dtype=np.uint64)
    hp = buf.ctypes.data_as(C.POINTER(C.c_uint64))
    for k in range(4):      # cfg, scene, fspec, field
        a = [C.byref(cfg), C.byref(spec), C.byref(fs), hp]
        a[k] = None
        assert lib.isx_scene_patch_field(a[0], a[1], a[2], 10, 1, 0, a[3], None, None, None) == isx.abi.ERR_BAD_ARG, k
    assert (buf == 7).all()
    # field_counts, scene_counts and stats may be NULL: the field alone, zeroed by the callee and filled
    assert lib.isx_scene_patch_field(C.byref(cfg), C.byref(spec), C.byref(fs), N_SIDE, SEED, 0, hp, None, None, None) == 0
    field, fc, _, _ = isx.scene_patch_field(cfg, spec, fs, N_SIDE, SEED)
    assert np.array_equal(buf, field.reshape(-1)) and int(buf.sum()) == fc.binned > 50


def test_scene_patch_field_sharded_one_rank_equals_scene_patch_field(isx):
    _reset(isx)
    cfg, spec = _side(isx)
    fs = _frame(1, spec, AXES[1], 0.5, 1.5)
    field, fc, cnt, st = isx.scene_patch_field(cfg, spec, fs, N_SIDE, SEED)
    sfield, sfc, pa, pb, ba, bb, sc = isx.scene_patch_field_sharded(isx.scene_patch_field, cfg, spec, fs, N_SIDE, SEED)
    assert np.array_equal(sfield, field) and np.array_equal(sfc, fc.words()) and int(field.sum()) == fc.binned > 50
    for got, want in zip((pa, pb, ba, bb), cnt.arrays()):
        assert np.array_equal(got, want)
    for f in CENSUS + ("bin_increments",):
        assert sc[f] == getattr(st, f), f
