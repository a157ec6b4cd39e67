"""The scene calls on the GPU: isx_scene_endstates and isx_fluxmap_scene bit for bit against the replay of the composed contract
on the oracle (tests/scene_np.py); the scenes that hold only one of the three parts against the library's own specialised
kernels; the edges; partition and launch-shape invariance; one workgroup with full rings; the device form, the sharded call and
the host driver.

The replays' counters are asserted first in every parity test (a condition on the replay, not on the library): a test cannot pass
without baffle interactions and patch arrivals."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scene_np as SC
from test_gpu_baffle import FIXTURES as BAFFLE_FIXTURES, SHAPES, _reset
from test_scene_cpu import SCENES, parts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "altair-raytracing_amd", "host", "isx_macro")
SEED = 12345
CENSUS = SC.CENSUS_FIELDS


def _spec(name):
    """the SceneSpec of a scene of this module"""
    import altair_raytracing_amd as isx
    ic = isx.default_config()
    p = parts(isx, ic)
    if name in SCENES:
        beam, baffles, patches = SCENES[name]
        return isx.scene_spec(ic, p[beam], [p[b] for b in baffles], [p[w] for w in patches])
    if name == "empty":
        return isx.default_scene_spec(ic)
    if name == "only_two":
        return isx.scene_spec(ic, None, [isx.baffle_disc(ic, *b) for b in BAFFLE_FIXTURES["two"]], [])
    if name == "only_led":
        return isx.scene_spec(ic, p["led"], [], [])
    if name == "only_patches":
        return isx.scene_spec(ic, None, [], [p["det"], p["sample"]])
    if name in ("black", "white"):      # every reflectance 0 / 1 (the wall's is the configuration's: _case)
        rho = 0.0 if name == "black" else 1.0
        return isx.scene_spec(ic, p["lamp"], [isx.baffle_disc(ic, (35, 0, 13), (1, 0, 0), 10.0, rho), isx.baffle_disc(ic, (0, 0, -40), (0, 0, 1), 12.0, rho)],
                              [isx.wall_patch_cap(ic, (1, 0, 0), 5.0, rho), isx.wall_patch_cap(ic, (0, 1, 0), 10.0, rho)])
    if name == "black_spot":            # a patch of reflectance 0 under the LED's first-strike spot (66.3, 0, -75)
        return isx.scene_spec(ic, p["led"], [], [isx.wall_patch_cap(ic, (66.3, 0, -75), 5.0, 0.0), p["sample"]])
    if name == "in_plane":              # the lamp's start point lies in the baffle's plane z = 20: s_p == 0, no crossing
        return isx.scene_spec(ic, p["lamp"], [isx.baffle_disc(ic, (10, 0, 20), (0, 0, 1), 30.0, 0.9)], [p["det"]])
    if name == "full":                  # 8 patches + 4 baffles at once
        caps = [isx.wall_patch_cap(ic, (k - 3.5, 1, 2), 10.0 + k, k / 7.0) for k in range(8)]
        return isx.scene_spec(ic, p["lamp"], [p["screen"], p["shield_port"], p["shield"], p["first_in"]], caps)
    raise KeyError(name)


def _case(mod, name, rho=0.95, compat=False, max_points=None):
    """(cfg, SceneSpec) of a scene; mod: a module with default_config() (the library or the oracle: same layout)"""
    c = mod.default_config()
    c.reflectance = {"black": 0.0, "white": 1.0}.get(name, rho)
    if compat:
        c.hit_line_mode = 1
    if max_points is not None:
        c.max_points = max_points
    return c, _spec(name)


_replays = {}


def _replayed(orc, name, n, seed=SEED, first=0, rho=0.95, max_points=None):
    """the replay of a scene: computed once, shared, never changed (the hit line plays no part in it)"""
    key = (name, n, seed, first, rho, max_points)
    if key not in _replays:
        oc, spec = _case(orc, name, rho, max_points=max_points)
        _replays[key] = SC.replay(oc, SC.spec_of(spec), n, seed, first, workers=None if n >= 2000 else 1)
    return _replays[key]


def _say(name, rep):
    print(name, "patch arrivals", rep["patch_arrivals"].tolist(), "absorbed", rep["patch_absorbed"].tolist(), "baffle arrivals",
          rep["baffle_arrivals"].tolist(), "absorbed", rep["baffle_absorbed"].tolist(), rep["census"])


def _endstates_equal(got, rep, sel=slice(None)):
    st, npts, lp, d, sp, sd, lb, lc = got
    assert np.array_equal(st, rep["status"][sel]) and np.array_equal(npts, rep["n_points"][sel])
    assert np.array_equal(lp, rep["last_point"][sel]), "last point"
    assert np.array_equal(d, rep["direction"][sel]), "direction"
    assert np.array_equal(sp, rep["start_point"][sel]) and np.array_equal(sd, rep["start_dir"][sel]), "start"
    assert np.array_equal(lb, rep["last_baffle"][sel]), "last baffle"
    assert np.array_equal(lc, rep["last_class"][sel]), "last class"


def _identities(cnt, st, hits):
    pa, pb, ba, bb = cnt.arrays()
    assert int(pa.sum()) + int(ba.sum()) == st.wall_hits
    assert int(pb.sum()) + int(bb.sum()) == st.absorbed
    assert st.bin_increments == int(hits.sum())
    assert st.exited + st.absorbed + st.suspended == st.launched


def _fluxmap_equal(orc, oc, got, rep):
    hits, cnt, st = got
    P, V = SC.counted_lines(oc, rep)
    want = orc.bin_lines(oc, P, V)
    assert hits.dtype == np.uint64 and hits.shape == want.shape
    assert np.array_equal(hits, want)
    for f in CENSUS:
        assert getattr(st, f) == rep["census"][f], f
    assert np.array_equal(cnt.words(), SC.counter_words(rep))
    _identities(cnt, st, hits)
    return P.shape[0]


# (scene, rays, wall reflectance, first ray)
PARITY = [("photometer", 20000, 0.95, 0), ("led_shield", 20000, 0.95, 0), ("led_first_in", 20000, 0.95, 0), ("lamp_open", 5000, 0.95, 0),
          ("photometer", 20000, 0.95, (1 << 32) + 7), ("photometer", 4000, 0.99, 0)]
PARITY_IDS = ["photometer", "led_shield", "led_first_in", "lamp_open", "photometer-first-ray", "photometer-rho0.99"]


def _replay_is_a_scene(name, rep):
    """a condition on the replay: the parts of the scene all take part"""
    _, baffles, patches = SCENES[name]
    assert rep["baffle_arrivals"].shape[0] == max(len(baffles), 1) and rep["patch_arrivals"].size == len(patches) + 2
    if baffles:
        assert int(rep["baffle_arrivals"].min()) >= 100, rep["baffle_arrivals"].tolist()
    assert int(rep["patch_arrivals"][:len(patches)].min()) >= 50, rep["patch_arrivals"].tolist()
    assert len(set(rep["status"].tolist())) >= 2        # exited and absorbed rays both


@pytest.mark.parametrize("name,n,rho,first", PARITY, ids=PARITY_IDS)
def test_scene_endstates_equal_the_replay(isx, orc, name, n, rho, first):
    _reset(isx)
    cfg, spec = _case(isx, name, rho)
    rep = _replayed(orc, name, n, SEED, first, rho)
    _say(name, rep)
    _replay_is_a_scene(name, rep)
    _endstates_equal(isx.scene_endstates(cfg, spec, n, SEED, first_ray=first), rep)


@pytest.mark.parametrize("compat", [False, True], ids=["last-segment", "origin-compat"])
@pytest.mark.parametrize("name,n,rho,first", PARITY, ids=PARITY_IDS)
def test_fluxmap_scene_equals_the_replay(isx, orc, name, n, rho, first, compat):
    _reset(isx)
    cfg, spec = _case(isx, name, rho, compat)
    oc, _ = _case(orc, name, rho, compat)
    rep = _replayed(orc, name, n, SEED, first, rho)
    _replay_is_a_scene(name, rep)
    lines = _fluxmap_equal(orc, oc, isx.fluxmap_scene(cfg, spec, n, SEED, first_ray=first), rep)
    print(name, "lines through the port:", lines)
    assert lines >= 100


def test_the_photometer_is_shadowed(isx, orc):
    """the pins of the issue on the GPU's own answer: with the two baffles 0 rays whose only interaction is on the detector, 0 rays
    straight through the port; the bare lamp has both"""
    _reset(isx)
    for name, n in (("photometer", 20000), ("lamp_open", 5000)):
        cfg, spec = _case(isx, name)
        st, npts, lp, d, sp, sd, lb, lc = isx.scene_endstates(cfg, spec, n, SEED)
        straight = int(((st == 1) & (npts == 2)).sum())
        first_on_det = int(((npts == 2) & (st == 2) & (lc == 0)).sum())      # (the detector is black: a first arrival there ends the ray)
        rep = _replayed(orc, name, n)
        assert first_on_det == int((rep["first_class"] == 0).sum()) and straight == int(((rep["status"] == 1) & (rep["n_points"] == 2)).sum())
        if name == "photometer":
            assert (first_on_det, straight) == (0, 0)
        else:
            assert first_on_det > 0 and straight > 0


# ---------------------------------------------------------------- one part only: against the library's own specialised kernels
N_DEG = 200_000


def _census_equal(a, b, fields=CENSUS + ("bin_increments",)):
    for f in fields:
        assert getattr(a, f) == getattr(b, f), f


def test_the_empty_scene_is_the_flux_map(isx):
    """the default spec at 2e5 rays: histogram and census are isx_fluxmap's (fate_scan 0), the end states isx_trace_endstates'; the
    fate scan's launch counter does not move, whatever the option says"""
    _reset(isx)
    cfg = isx.default_config()
    spec = isx.default_scene_spec(cfg)
    try:
        isx.set_option("fate_scan", 0)
        want = isx.fluxmap(cfg, N_DEG, SEED)
        for fs in (-1, 1, 0):
            isx.set_option("fate_scan", fs)
            before = isx.fate_scan_launches()
            hits, cnt, st = isx.fluxmap_scene(cfg, spec, N_DEG, SEED)
            assert isx.fate_scan_launches() == before
            assert np.array_equal(hits, want[0])
            _census_equal(st, want[1])
            w = cnt.words()
            assert w[0] + w[1] == st.wall_hits and w[10] + w[11] == st.absorbed and not w[2:10].any() and not w[12:].any()
    finally:
        _reset(isx)
    assert int(want[0].sum()) > 1000
    st, npts, lp, d, sp, sd, lb, lc = isx.scene_endstates(cfg, spec, N_DEG, SEED)
    wst, wnp, wlp, wd = isx.trace_endstates(cfg, N_DEG, SEED)
    assert np.array_equal(st, wst) and np.array_equal(npts, wnp) and np.array_equal(lp, wlp) and np.array_equal(d, wd)
    assert (lb == -1).all() and set(np.unique(lc).tolist()) <= {-1, 0, 1}
    assert np.array_equal(sp, np.tile(np.array(cfg.src[:]), (N_DEG, 1)))


def test_only_baffles_is_the_baffle_call(isx):
    """`two` of the baffle tests and nothing else: isx_fluxmap_baffle's histogram, census and 16 counters, isx_baffle_endstates'
    end states"""
    _reset(isx)
    cfg, spec = _case(isx, "only_two")
    before = isx.fate_scan_launches()
    want = isx.fluxmap_baffle(cfg, spec.baffles, N_DEG, SEED)
    hits, cnt, st = isx.fluxmap_scene(cfg, spec, N_DEG, SEED)
    assert isx.fate_scan_launches() == before
    assert np.array_equal(hits, want[0]) and int(hits.sum()) > 1000
    _census_equal(st, want[2])
    pa, pb, ba, bb = cnt.arrays()
    assert np.array_equal(ba, want[1].arrays()[0]) and np.array_equal(bb, want[1].arrays()[1]) and int(ba[:2].min()) > 1000
    _identities(cnt, st, hits)
    got = isx.scene_endstates(cfg, spec, N_DEG, SEED)
    ref = isx.baffle_endstates(cfg, spec.baffles, N_DEG, SEED)
    for k, j in ((0, 0), (1, 1), (2, 2), (3, 3), (6, 4)):
        assert np.array_equal(got[k], ref[j]), k


def test_only_a_beam_is_the_beam_call(isx):
    _reset(isx)
    cfg, spec = _case(isx, "only_led")
    before = isx.fate_scan_launches()
    want = isx.fluxmap_beam(cfg, spec.beam, N_DEG, SEED)
    hits, cnt, st = isx.fluxmap_scene(cfg, spec, N_DEG, SEED)
    assert isx.fate_scan_launches() == before
    assert np.array_equal(hits, want[0]) and int(hits.sum()) > 1000
    _census_equal(st, want[1])
    _identities(cnt, st, hits)
    got = isx.scene_endstates(cfg, spec, N_DEG, SEED)
    ref = isx.beam_endstates(cfg, spec.beam, N_DEG, SEED)
    for k in range(6):
        assert np.array_equal(got[k], ref[k]), k
    assert (got[6] == -1).all()


def test_only_patches_is_the_patch_call(isx):
    """[det, sample] and nothing else: isx_wall_patches' arrivals, absorbed and census (its bin_increments is another quantity)"""
    _reset(isx)
    cfg, spec = _case(isx, "only_patches")
    before = isx.fate_scan_launches()
    arr, ab, wst = isx.wall_patches(cfg, N_DEG, SEED, spec.patches)
    hits, cnt, st = isx.fluxmap_scene(cfg, spec, N_DEG, SEED)
    assert isx.fate_scan_launches() == before
    pa, pb, ba, bb = cnt.arrays()
    assert np.array_equal(pa[:4], arr) and np.array_equal(pb[:4], ab) and not pa[4:].any() and not ba.any()
    assert int(arr[:2].min()) > 100
    _census_equal(st, wst, CENSUS)
    _identities(cnt, st, hits)


# ---------------------------------------------------------------- edges
N_EDGE = 5000


@pytest.mark.parametrize("name,max_points", [("led_first_in", 4), ("led_first_in", 7), ("black", None), ("white", None),
                                             ("black_spot", None), ("in_plane", None), ("full", None)])
def test_edges_equal_the_replay(isx, orc, name, max_points):
    """a bounce limit that suspends rays right after a baffle and right after a patch; every reflectance 0 and every reflectance 1;
    a black patch under the LED's first-strike spot; the lamp's start point in a baffle's plane; 8 patches and 4 baffles at once"""
    _reset(isx)
    cfg, spec = _case(isx, name, max_points=max_points)
    oc, _ = _case(orc, name, max_points=max_points)
    rep = _replayed(orc, name, N_EDGE, max_points=max_points)
    _say(name, rep)
    print("suspended after a baffle", rep["suspended_after_baffle"], "after a patch", rep["suspended_after_patch"])
    pa, pb, ba, bb = (rep[k] for k in SC.COUNTERS)
    if max_points is not None:
        assert rep["suspended_after_baffle"] >= 1 and rep["suspended_after_patch"] >= 1
    if name == "black":      # every ray ends at its first interaction, wherever that is
        assert np.array_equal(pa, pb) and np.array_equal(ba, bb) and int(ba.sum()) > 100 and int(pa[1:3].min()) > 0 and pa[0] == 0      # (the screen shadows the detector)
        assert rep["census"]["wall_hits"] == rep["census"]["absorbed"]
    if name == "white":
        assert not pb.any() and not bb.any() and rep["census"]["absorbed"] == 0 and int(pa[:2].min()) > 0 and int(ba.min()) > 0
    if name == "black_spot":
        assert pa[0] == pb[0] > N_EDGE // 2      # most rays end on their first strike
    if name == "in_plane":
        assert (rep["first_kind"] != -2).all() and int(ba.min()) > 100      # no ray's first segment is struck; later ones are
    if name == "full":
        assert ba.shape == (4, 2) and int(ba.sum(axis=1).min()) > 0 and int((pa[:8] > 0).sum()) >= 6
    _endstates_equal(isx.scene_endstates(cfg, spec, N_EDGE, SEED), rep)
    _fluxmap_equal(orc, oc, isx.fluxmap_scene(cfg, spec, N_EDGE, SEED), rep)


# ---------------------------------------------------------------- how the job is cut and launched
def _same(a, b):
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].words(), b[1].words())
    _census_equal(a[2], b[2])


def test_partition_invariance(isx):
    """photometer: 3e5 rays in one call == three calls of 1e5 at consecutive first_ray"""
    _reset(isx)
    cfg, spec = _case(isx, "photometer")
    n = 300_000
    whole = isx.fluxmap_scene(cfg, spec, n, SEED)
    cut = [isx.fluxmap_scene(cfg, spec, 100_000, SEED, first_ray=100_000 * k) for k in range(3)]
    assert np.array_equal(sum(p[0] for p in cut), whole[0])
    assert np.array_equal(sum(p[1].words() for p in cut), whole[1].words())
    for f in CENSUS + ("bin_increments",):
        assert sum(getattr(p[2], f) for p in cut) == getattr(whole[2], f), f
    assert whole[2].launched == n and int(whole[0].sum()) > 1000
    _identities(whole[1], whole[2], whole[0])


def test_launch_shape_invariance(isx):
    """the thirteen shapes and switches of the baffle tests on led_first_in, 1e5 rays"""
    _reset(isx)
    cfg, spec = _case(isx, "led_first_in")
    n = 100_000
    base = isx.fluxmap_scene(cfg, spec, n, SEED)
    assert base[2].launched == n and int(base[0].sum()) > 1000
    assert len(SHAPES) == 13
    try:
        for opts in SHAPES:
            _reset(isx)
            for key, v in opts.items():
                isx.set_option(key, v)
            _same(isx.fluxmap_scene(cfg, spec, n, SEED), base)
    finally:
        _reset(isx)


@pytest.mark.parametrize("name", ["led_first_in", "photometer"])
def test_one_workgroup_with_full_rings(isx, name):
    """1e5 rays at wall reflectance 0.99 through ONE workgroup (`grid_blocks` 1): its tracer lanes, the pending ring and the resume
    ring all fill with rays that want the assist wave or come back from it, and the result is that of the default launch.  (The
    assist wave never waits for room in the resume ring, with the beam's parked rays as without: docs/LOG.md sections 18.4, 19.2.)"""
    _reset(isx)
    cfg, spec = _case(isx, name, rho=0.99)
    n = 100_000
    base = isx.fluxmap_scene(cfg, spec, n, SEED)
    assert int(base[1].arrays()[2].sum()) > n // 2 and int(base[0].sum()) > 1000
    try:
        isx.set_option("grid_blocks", 1)
        _same(isx.fluxmap_scene(cfg, spec, n, SEED), base)
    finally:
        _reset(isx)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 769])
def test_ray_counts(isx, orc, n):
    """the smallest launches of photometer against the first rays of its replay"""
    _reset(isx)
    cfg, spec = _case(isx, "photometer")
    oc, _ = _case(orc, "photometer")
    rep = _replayed(orc, "photometer", 20000)
    part = {k: rep[k][:n] for k in SC.PER_RAY}
    _endstates_equal(isx.scene_endstates(cfg, spec, n, SEED), part)
    hits, cnt, st = isx.fluxmap_scene(cfg, spec, n, SEED)
    P, V = SC.counted_lines(oc, part)
    assert np.array_equal(hits, orc.bin_lines(oc, P, V))
    assert st.launched == n and st.wall_hits == int((part["n_points"] - 1 - (part["status"] == 1)).sum())
    assert st.absorbed == int((part["status"] == 2).sum()) and st.exited == int((part["status"] == 1).sum())
    _identities(cnt, st, hits)


def test_no_rays(isx):
    _reset(isx)
    cfg, spec = _case(isx, "photometer")
    hits, cnt, st = isx.fluxmap_scene(cfg, spec, 0, SEED)
    assert int(hits.sum()) == 0 and st.launched == 0 and st.wall_hits == 0 and not cnt.words().any()
    out = isx.scene_endstates(cfg, spec, 0, SEED)
    assert all(a.shape[0] == 0 for a in out)


@pytest.mark.parametrize("nt,nph", [(36000, 1), (190, 189)])
def test_a_grid_whose_tables_do_not_fit_the_lds_is_refused(isx, nt, nph):
    """ISX_ERR_BAD_CONFIG from the blocking call with hits, counts and census untouched and nothing launched; the same grid is no
    obstacle to isx_scene_endstates, and a grid that fits (185 x 185) is served"""
    import ctypes as C
    _reset(isx)
    cfg, spec = _case(isx, "photometer")
    cfg.n_theta, cfg.n_phi = nt, nph
    lib = isx.load()
    isx.sync()
    isx.take_stats()
    buf = np.full(nt * nph, 7, dtype=np.uint64)
    cnt, st = isx.SceneCounts(), isx.Stats()
    st.launched = 77
    cnt.patch_arrivals[0] = 5
    rc = lib.isx_fluxmap_scene(C.byref(cfg), C.byref(spec), 1000, SEED, 0, buf.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(cnt), C.byref(st))
    assert rc == isx.abi.ERR_BAD_CONFIG
    assert (buf == 7).all() and st.launched == 77 and int(cnt.words().sum()) == 5
    left = isx.take_stats()
    assert (left.launched, left.wall_hits, left.bin_increments) == (0, 0, 0)
    out = isx.scene_endstates(cfg, spec, 100, SEED)
    assert out[0].shape == (100,)
    cfg.n_theta, cfg.n_phi = 185, 185
    hits, cnt2, st2 = isx.fluxmap_scene(cfg, spec, 20000, SEED)
    assert st2.launched == 20000 and hits.shape == (185, 185)
    _identities(cnt2, st2, hits)


def test_device_form_accumulates():
    """isx_fluxmap_scene_device twice into caller-owned, pre-filled tensors == the sum of the blocking calls on top of what was
    there, and isx_take_stats adds up (a process of its own: torch owns the tensors, the library's stream does the work)."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import altair_raytracing_amd as isx
from test_gpu_scene import _case
isx.load(); isx.init(0)
cfg, spec = _case(isx, "photometer")
SEED = 12345
nb = cfg.n_theta * cfg.n_phi
d_hits = torch.arange(5, 5 + nb, dtype=torch.int64, device="cuda:0")
d_cnt = torch.arange(100, 136, dtype=torch.int64, device="cuda:0")
torch.cuda.synchronize()
cut = [(0, 100001), (100001, 99999)]
for first, n in cut:
    isx.fluxmap_scene_device(cfg, spec, n, SEED, first, d_hits.data_ptr(), d_cnt.data_ptr())
isx.sync()
st = isx.take_stats()
blocking = [isx.fluxmap_scene(cfg, spec, n, SEED, first) for first, n in cut]
torch.cuda.synchronize()
hits = sum(b[0] for b in blocking)
assert np.array_equal(d_hits.cpu().numpy() - np.arange(5, 5 + nb), hits.reshape(-1).astype(np.int64))
want_cnt = sum(b[1].words() for b in blocking)
assert np.array_equal(d_cnt.cpu().numpy() - np.arange(100, 136), want_cnt.astype(np.int64))
for f in ("launched", "exited", "counted_below_z", "absorbed", "suspended", "wall_hits", "bin_increments"):
    assert getattr(st, f) == sum(getattr(b[2], f) for b in blocking), f
assert int(hits.sum()) > 1000 and want_cnt[:4].min() > 100 and want_cnt[20:24].min() > 1000
for hp, cp in ((0, d_cnt.data_ptr()), (d_hits.data_ptr(), 0)):
    try:
        isx.fluxmap_scene_device(cfg, spec, 10, SEED, 0, hp, cp)
        raise SystemExit("a NULL pointer was accepted")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_BAD_ARG
isx.shutdown()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]


def test_fluxmap_scene_sharded_one_rank_equals_fluxmap_scene(isx):
    _reset(isx)
    cfg, spec = _case(isx, "photometer")
    hits, cnt, st = isx.fluxmap_scene(cfg, spec, 100_000, SEED)
    shits, pa, pb, ba, bb, sc = isx.fluxmap_scene_sharded(isx.fluxmap_scene, cfg, spec, 100_000, SEED)
    assert np.array_equal(shits, hits)
    for got, want in zip((pa, pb, ba, bb), cnt.arrays()):
        assert np.array_equal(got, want)
    for f in CENSUS + ("bin_increments",):
        assert sc[f] == getattr(st, f), f


def test_host_driver_scene_flux(isx, tmp_path):
    """isx_macro sceneFlux for photometer: the CSV in the flux maps' format parsed back == fluxmap_scene with the same scene, seed
    and ray range; the scene and all counters stand in the metadata"""
    _reset(isx)
    env = dict(os.environ, ISX_QUIET="1")
    env.pop("ISX_RAYS", None); env.pop("ISX_SEED", None)
    n = 100_000      # (fractions are multiples of 1e-5: the six decimals of the format hold them)
    args = ["--origin", "0,0,20", "--axis", "0,0,1", "--half-angle", "180", "--law", "uniform",
            "--centre", "35,0,13", "--normal", "1,0,0", "--radius", "10", "--reflectance", "0.9",
            "--centre", "0,0,-40", "--normal", "0,0,1", "--radius", "12", "--reflectance", "0.9",
            "--patch-dir", "1,0,0", "--patch-half-angle", "5", "--patch-reflectance", "0",
            "--patch-dir", "0,1,0", "--patch-half-angle", "10", "--patch-reflectance", "0.5"]
    r = subprocess.run([CLI, "sceneFlux", "--rays", str(n)] + args, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    found = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs if f.startswith("scene_flux") and f.endswith(".csv")]
    assert len(found) == 1, found
    lines = open(found[0]).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    meta = {l[2:].split(":")[0]: l.split(":", 1)[1].strip() for l in head if ":" in l}
    assert meta["Baffles"] == "2" and meta["Baffle 0 radius"] == "10cm" and meta["Wall patches"] == "2"
    assert meta["Patch 1 reflectance"] == "0.5" and meta["Beam origin (x,y,z)"] == "0cm, 0cm, 20cm"
    body = [l for l in lines if not l.startswith("#")]
    cfg = isx.default_config()      # (the macro's sphere: the default configuration, wall reflectance 0.99)
    assert body[0] == "theta,phi,fraction" and len(body) == 1 + cfg.n_theta * cfg.n_phi
    spec = _spec("photometer")
    hits, cnt, st = isx.fluxmap_scene(cfg, spec, n, int(meta["Seed"]), int(meta["First ray"]))
    got = np.array([round(float(l.split(",")[2]) * n) for l in body[1:]], dtype=np.uint64).reshape(cfg.n_theta, cfg.n_phi)
    assert np.array_equal(got, hits) and int(hits.sum()) > 1000
    pa, pb, ba, bb = cnt.arrays()
    for k in (0, 1):
        assert meta["Baffle %d arrivals (side 0, side 1)" % k] == "%d, %d" % (ba[k, 0], ba[k, 1])
        assert meta["Baffle %d absorbed (side 0, side 1)" % k] == "%d, %d" % (bb[k, 0], bb[k, 1])
    assert meta["Class arrivals"] == ", ".join(str(int(x)) for x in pa[:4])
    assert meta["Class absorbed"] == ", ".join(str(int(x)) for x in pb[:4])
    assert int(ba[:2].min()) > 100 and int(pa[:2].min()) > 100
    assert (int(meta["Launched"]), int(meta["Exited"]), int(meta["Absorbed"]), int(meta["Suspended"]), int(meta["Wall hits"]),
            int(meta["Detector hits"])) == (st.launched, st.exited, st.absorbed, st.suspended, st.wall_hits, st.bin_increments)
    assert meta["Total rays exiting port"] == "%d out of %d" % (st.counted_below_z, n)
    # a scene the library refuses is an error, not a run; so is a patch short of an option
    for bad in (["--centre", "30,0,-85", "--normal", "-66.3,0,-23.6", "--radius", "12", "--reflectance", "0.9"],
                ["--patch-dir", "1,0,0", "--patch-half-angle", "5"],
                ["--patch-dir", "1,x,0", "--patch-half-angle", "5", "--patch-reflectance", "0.5"],
                ["--origin", "0,0,200"]):
        r = subprocess.run([CLI, "sceneFlux", "--rays", "1000"] + bad + ["folder=bad"], cwd=tmp_path, env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode != 0, bad
