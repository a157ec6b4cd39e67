"""The scene calls (isx_fluxmap_scene, isx_scene_endstates) without a GPU: the refusals of the three component contracts reached
through the scene, the bindings, the sharded call, and the replay of the composed contract on the oracle (scene_np) -- against the
three replays it is composed of, against the oracle's own trace for the empty scene, and the numbers of the photometer scene."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import baffle_np
import beam_np
import scene_np as SC
import wallpatch_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
RHO = 0.95
NORMAL = (-66.3, 0.0, -23.6)


# ---------------------------------------------------------------- the fixtures (made with the library's own helpers)
def parts(isx, cfg):
    """the pieces the scenes are made of"""
    return {
        "lamp": isx.beam_cone(cfg, (0, 0, 20), (0, 0, 1), 0.0, 180.0, isx.BEAM_UNIFORM),
        "led": isx.beam_cone(cfg, (-60, 0, -75), (1, 0, 0), 2.0, 3.0, isx.BEAM_LAMBERT),
        "screen": isx.baffle_disc(cfg, (35, 0, 13), (1, 0, 0), 10.0, 0.9),
        "shield_port": isx.baffle_disc(cfg, (0, 0, -40), (0, 0, 1), 12.0, 0.9),
        "shield": isx.baffle_disc(cfg, (30, 0, -85), NORMAL, 8.0, 0.9),
        "first_in": isx.baffle_disc(cfg, (30, 0, -80), NORMAL, 12.0, 0.9),
        "det": isx.wall_patch_cap(cfg, (1, 0, 0), 5.0, 0.0),
        "sample": isx.wall_patch_cap(cfg, (0, 1, 0), 10.0, 0.5),
    }


SCENES = {"photometer": ("lamp", ("screen", "shield_port"), ("det", "sample")),
          "lamp_open": ("lamp", (), ("det", "sample")),
          "led_shield": ("led", ("shield",), ("det",)),
          "led_first_in": ("led", ("first_in",), ("det", "sample"))}


def scene(isx, cfg, name):
    """the SceneSpec of one of the four scenes"""
    p = parts(isx, cfg)
    beam, baffles, patches = SCENES[name]
    return isx.scene_spec(cfg, p[beam], [p[b] for b in baffles], [p[w] for w in patches])


# ---------------------------------------------------------------- bindings
def test_binding_structs_and_default_spec():
    import altair_raytracing_amd as isx
    assert C.sizeof(isx.SceneSpec) == 8 + C.sizeof(isx.BeamSpec) + C.sizeof(isx.BaffleSpec) + C.sizeof(isx.WallPatchSpec) == 744
    assert C.sizeof(isx.SceneCounts) == 36 * 8 and isx.SCENE_COUNT_WORDS == 36
    assert isx.SceneSpec.beam.offset == 8 and isx.SceneSpec.baffles.offset == 136 and isx.SceneSpec.patches.offset == 408
    assert isx.SceneCounts.patch_absorbed.offset == 80 and isx.SceneCounts.baffle.offset == 160
    cfg = isx.default_config()
    s = isx.default_scene_spec(cfg)
    assert s.struct_size == C.sizeof(isx.SceneSpec) and s.reserved0 == 0
    for part, default in ((s.beam, isx.default_beam_spec(cfg)), (s.baffles, isx.default_baffle_spec(cfg)),
                          (s.patches, isx.default_wall_patch_spec(cfg))):
        assert bytes(part) == bytes(default)
    assert list(s.beam.origin) == list(cfg.src) and s.beam.radius == 0.0 and s.beam.cos_min == 1.0
    assert s.baffles.n_baffles == 0 and s.patches.n_patches == 0
    isx.load().isx_default_scene_spec(C.byref(cfg), None)      # (a NULL spec is left alone)
    ph = scene(isx, cfg, "photometer")
    assert ph.baffles.n_baffles == 2 and ph.patches.n_patches == 2 and ph.struct_size == 744
    assert list(ph.beam.e1) == [1.0, 0.0, 0.0] and list(ph.beam.e2) == [0.0, 1.0, 0.0] and ph.beam.cos_min == -1.0
    assert bytes(isx.scene_spec(cfg)) == bytes(s)
    pa, pb, ba, bb = isx.SceneCounts().arrays()
    assert pa.shape == (10,) and pb.shape == (10,) and ba.shape == (4, 2) and bb.shape == (4, 2)
    cnt = isx.SceneCounts()
    cnt.patch_arrivals[9] = 3; cnt.patch_absorbed[0] = 4; cnt.baffle.arrivals[3][1] = 5; cnt.baffle.absorbed[0][0] = 6
    w = cnt.words()
    assert w.size == 36 and w[9] == 3 and w[10] == 4 and w[27] == 5 and w[28] == 6 and int(w.sum()) == 18
    with pytest.raises(ValueError):
        isx.scene_spec(cfg, baffles=[parts(isx, cfg)["shield"]] * 5)
    with pytest.raises(ValueError):
        isx.scene_spec(cfg, patches=[parts(isx, cfg)["det"]] * 9)


def refused_scenes(isx):
    """([(what, cfg, SceneSpec)] that isx.h refuses with ISX_ERR_BAD_CONFIG, [(cfg, SceneSpec)] that get past the checks): every
    refusal of the three component calls' own lists (their tests' refused_calls), each inside an otherwise good scene, and the
    outer struct_size"""
    import test_baffle_cpu
    import test_beam_cpu
    import test_wall_patches_cpu
    cfg = isx.default_config()
    good = scene(isx, cfg, "photometer")

    def with_part(field, part):
        s = good.copy()
        C.memmove(C.byref(getattr(s, field)), C.byref(part), C.sizeof(part))
        return s

    bad, served = [], [(cfg, good), (cfg, isx.default_scene_spec(cfg))]
    for field, mod in (("beam", test_beam_cpu), ("baffles", test_baffle_cpu), ("patches", test_wall_patches_cpu)):
        _, _, b, ok = mod.refused_calls(isx)
        for what, c, part in b:
            bad.append(("%s: %s" % (field, what), c, with_part(field, part)))
        for c, part in ok:
            served.append((c, with_part(field, part)))
    for size in (0, C.sizeof(isx.SceneSpec) - 8, C.sizeof(isx.SceneSpec) + 8, C.sizeof(isx.BeamSpec)):
        s = good.copy(); s.struct_size = size
        bad.append(("scene struct_size %d" % size, cfg, s))
    # at the limits: 8 patches and 4 baffles at once
    p = parts(isx, cfg)
    caps = [isx.wall_patch_cap(cfg, (k - 3.5, 1, 2), 10.0 + k, k / 7.0) for k in range(8)]
    served.append((cfg, isx.scene_spec(cfg, p["led"], [p["screen"], p["shield_port"], p["shield"], p["first_in"]], caps)))
    return cfg, good, bad, served


def test_refusals_and_null_arguments_need_no_device():
    """Every refusal of the three component contracts is ISX_ERR_BAD_CONFIG through the three scene entry points, a wrong nested or
    outer struct_size included, and a NULL pointer ISX_ERR_BAD_ARG, before anything asks for a device (this process never keeps
    isx_init); scenes at the limits (8 patches, 4 baffles) get past the checks; so does a grid check (check_baffle_grid)."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ctypes as C
import numpy as np
import altair_raytracing_amd as isx
from test_scene_cpu import refused_scenes
from test_baffle_cpu import big_grids
lib = isx.load()
have = lib.isx_init(0) == 0
if have:
    lib.isx_shutdown()
past = isx.abi.ERR_NOT_INIT if have else isx.abi.ERR_NO_DEVICE
buf = np.full(36000, 7, dtype=np.uint64)
hp = buf.ctypes.data_as(C.POINTER(C.c_uint64))
ip = np.zeros(16, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
dp = np.zeros(48, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
cnt = isx.SceneCounts()
cfg, good, bad, served = refused_scenes(isx)
dev = C.c_void_p(4096)
BAD_CONFIG, BAD_ARG = isx.abi.ERR_BAD_CONFIG, isx.abi.ERR_BAD_ARG
for what, c, s in bad:
    assert lib.isx_fluxmap_scene(C.byref(c), C.byref(s), 10, 1, 0, hp, C.byref(cnt), None) == BAD_CONFIG, what
    assert lib.isx_fluxmap_scene_device(C.byref(c), C.byref(s), 10, 1, 0, dev, dev) == BAD_CONFIG, what
    assert lib.isx_scene_endstates(C.byref(c), C.byref(s), 10, 1, 0, ip, ip, dp, dp, dp, dp, ip, ip) == BAD_CONFIG, what
for k, (c, s) in enumerate(served):
    assert lib.isx_fluxmap_scene(C.byref(c), C.byref(s), 10, 1, 0, hp, None, None) == past, k
    assert lib.isx_fluxmap_scene_device(C.byref(c), C.byref(s), 10, 1, 0, dev, dev) == past, k
    assert lib.isx_scene_endstates(C.byref(c), C.byref(s), 10, 1, 0, ip, ip, dp, dp, None, None, None, None) == past, k
g, cf = C.byref(good), C.byref(cfg)
assert lib.isx_fluxmap_scene(None, g, 10, 1, 0, hp, None, None) == BAD_ARG
assert lib.isx_fluxmap_scene(cf, None, 10, 1, 0, hp, None, None) == BAD_ARG
assert lib.isx_fluxmap_scene(cf, g, 10, 1, 0, None, None, None) == BAD_ARG
assert lib.isx_fluxmap_scene_device(None, g, 10, 1, 0, dev, dev) == BAD_ARG
assert lib.isx_fluxmap_scene_device(cf, None, 10, 1, 0, dev, dev) == BAD_ARG
assert lib.isx_fluxmap_scene_device(cf, g, 10, 1, 0, None, dev) == BAD_ARG
assert lib.isx_fluxmap_scene_device(cf, g, 10, 1, 0, dev, None) == BAD_ARG
for k in range(6):      # cfg, spec, status, n_points, last_point, direction
    a = [cf, g, ip, ip, dp, dp]
    a[k] = None
    assert lib.isx_scene_endstates(a[0], a[1], 10, 1, 0, a[2], a[3], a[4], a[5], dp, dp, ip, ip) == BAD_ARG, k
# the detector grid of the two flux-map calls (check_baffle_grid): refused without a device, nothing written
grids, fits = big_grids(isx)
for what, c in grids:
    st = isx.Stats(); st.launched = 77
    assert lib.isx_fluxmap_scene(C.byref(c), g, 10, 1, 0, hp, C.byref(cnt), C.byref(st)) == BAD_CONFIG, what
    assert lib.isx_fluxmap_scene_device(C.byref(c), g, 10, 1, 0, dev, dev) == BAD_CONFIG, what
    assert lib.isx_scene_endstates(C.byref(c), g, 10, 1, 0, ip, ip, dp, dp, None, None, None, None) == past, what
    assert (buf == 7).all() and st.launched == 77 and not cnt.words().any()
for c in fits:
    assert lib.isx_fluxmap_scene(C.byref(c), g, 10, 1, 0, hp, None, None) == past, (c.n_theta, c.n_phi)
try:
    isx.fluxmap_scene(bad[0][1], bad[0][2], 10, 1)
    print("no error")
except isx.IsxError as e:
    print("ok", e.status, len(bad), len(served), len(grids), len(fits))
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    # 46 beam + 68 baffle + 28 patch refusals + 4 outer sizes; 2 + 7 + 8 + 4 + 1 served
    assert r.stdout.split() == ["ok", "-2", "146", "22", "4", "5"], r.stdout


def test_no_device_on_a_machine_without_one():
    """where the library can initialise no HIP device, a valid scene call is ISX_ERR_NO_DEVICE (a process of its own)"""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import altair_raytracing_amd as isx
from test_scene_cpu import scene
lib = isx.load()
if lib.isx_init(0) == 0:
    lib.isx_shutdown()
    print("device")      # (test_refusals_and_null_arguments_need_no_device covers the machine with a device)
    raise SystemExit(0)
cfg = isx.default_config()
spec = scene(isx, cfg, "photometer")
for call in (lambda: isx.fluxmap_scene(cfg, spec, 10, 1), lambda: isx.scene_endstates(cfg, spec, 10, 1),
             lambda: isx.fluxmap_scene_device(cfg, spec, 10, 1, 0, 4096, 8192)):
    try:
        call()
        raise SystemExit("no error")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_NO_DEVICE, e.status
print("no device")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() in (["device"], ["no", "device"]), r.stdout + r.stderr[-2000:]


# ---------------------------------------------------------------- the replay against what it is composed of
N_PART = 2000


def _ocfg(orc, rho=RHO):
    c = orc.default_config()
    c.reflectance = rho
    return c


def test_replay_of_the_empty_scene_is_the_oracles_trace(orc):
    """no beam, no baffle, no patch: status, n_points, last point and direction of every ray are oracle.trace_endstates', the
    census oracle.fluxmap's -- with the pencil as the configuration states it and as the degenerate beam of the default spec"""
    import altair_raytracing_amd as isx
    cfg = _ocfg(orc)
    st, npts, lp, d = orc.trace_endstates(cfg, N_PART, SEED, 0)
    _, ost = orc.fluxmap(cfg, N_PART, SEED)
    empty = SC.spec_of(isx.default_scene_spec(isx.default_config()))
    assert empty["baffles"] == [] and empty["patches"] == []
    for sc in ({"beam": None, "baffles": [], "patches": []}, empty):
        rep = SC.replay(cfg, sc, N_PART, SEED)
        assert np.array_equal(rep["status"], st) and np.array_equal(rep["n_points"], npts)
        assert np.array_equal(rep["last_point"], lp)
        ex = st == 1
        assert ex.sum() > 50 and np.array_equal(rep["direction"][ex], d[ex])
        assert (rep["last_baffle"] == -1).all() and not rep["baffle_arrivals"].any()
        assert (rep["last_class"][rep["n_points"] > 2] >= 0).all() and rep["patch_arrivals"].size == 2
        for f in SC.CENSUS_FIELDS:
            assert rep["census"][f] == getattr(ost, f), f
    assert len(set(st.tolist())) >= 2
    part = SC.replay(cfg, empty, 40, SEED, first=100, workers=1)
    assert np.array_equal(part["status"], st[100:140]) and np.array_equal(part["last_point"], lp[100:140])


def test_replay_with_only_baffles_is_the_baffle_replay(orc):
    import altair_raytracing_amd as isx
    icfg = isx.default_config()
    p = parts(isx, icfg)
    two = baffle_np.spec_of(isx.baffle_spec(icfg, [p["shield"], isx.baffle_disc(icfg, (0, 0, 0), (0, 0, 1), 25.0, 0.5)]))
    cfg = _ocfg(orc)
    ref = baffle_np.replay(cfg, two, N_PART, SEED)
    rep = SC.replay(cfg, {"beam": None, "baffles": two, "patches": []}, N_PART, SEED)
    for k in baffle_np.PER_RAY:
        assert np.array_equal(rep[k], ref[k]), k
    assert np.array_equal(rep["baffle_arrivals"], ref["arrivals"]) and np.array_equal(rep["baffle_absorbed"], ref["absorbed"])
    assert rep["census"] == ref["census"] and rep["suspended_after_baffle"] == ref["suspended_after_baffle"]
    assert int(ref["arrivals"].sum()) > 100


def test_replay_with_only_patches_is_the_patch_replay(orc):
    import altair_raytracing_amd as isx
    icfg = isx.default_config()
    p = parts(isx, icfg)
    patches = wallpatch_np.spec_of(isx.wall_patch_spec(icfg, [p["det"], p["sample"]]))
    cfg = _ocfg(orc)
    arr, ab, census, status, npts = wallpatch_np.replay(cfg, patches, N_PART, SEED)
    rep = SC.replay(cfg, {"beam": None, "baffles": [], "patches": patches}, N_PART, SEED)
    assert np.array_equal(rep["patch_arrivals"], arr) and np.array_equal(rep["patch_absorbed"], ab)
    assert rep["census"] == census and np.array_equal(rep["status"], status) and np.array_equal(rep["n_points"], npts)
    assert arr[:2].all()


def test_replay_with_only_a_beam_is_the_beam_replay(orc):
    import altair_raytracing_amd as isx
    icfg = isx.default_config()
    cfg = _ocfg(orc)
    for name in ("led", "lamp"):
        beam = beam_np.spec_of(parts(isx, icfg)[name])
        sp, sv, status, npts, lp, d, kind0, census = beam_np.replay(cfg, beam, N_PART, SEED)
        rep = SC.replay(cfg, {"beam": beam, "baffles": [], "patches": []}, N_PART, SEED)
        for key, ref in (("start_point", sp), ("start_dir", sv), ("status", status), ("n_points", npts), ("last_point", lp),
                         ("direction", d), ("first_kind", kind0)):
            assert np.array_equal(rep[key], ref), (name, key)
        assert rep["census"] == census


# ---------------------------------------------------------------- the photometer
N_PHOT = 20000


@pytest.fixture(scope="module")
def photometer(orc):
    """the replay of `photometer` at 2e4 rays: computed once, shared, never changed"""
    import altair_raytracing_amd as isx
    return SC.replay(_ocfg(orc), SC.spec_of(scene(isx, isx.default_config(), "photometer")), N_PHOT, SEED)


@pytest.fixture(scope="module")
def lamp_open(orc):
    import altair_raytracing_amd as isx
    return SC.replay(_ocfg(orc), SC.spec_of(scene(isx, isx.default_config(), "lamp_open")), N_PHOT, SEED)


def direct(rep, det_class=0):
    """(rays whose first interaction is on the detector patch, rays that leave through the port with no interaction)"""
    on_det = int((rep["first_class"] == det_class).sum())
    straight = int(((rep["status"] == 1) & (rep["n_points"] == 2)).sum())
    return on_det, straight


def test_photometer_counts(photometer):
    """the numbers of the composed contract for lamp + [screen, shield_port] + [det, sample], 2e4 rays, seed 12345, with the caps'
    min_dot and the lamp's cos_min as the library's helpers make them"""
    r = photometer
    assert r["patch_arrivals"].tolist() == [554, 2375, 309842, 99]
    assert r["patch_absorbed"].tolist() == [554, 1200, 15633, 2]
    assert r["baffle_arrivals"].tolist() == [[761, 1111], [1239, 913]]
    assert r["baffle_absorbed"].tolist() == [[93, 119], [118, 98]]
    c = r["census"]
    assert c["exited"] == c["counted_below_z"] == 2183 and c["absorbed"] == 17817 and c["suspended"] == 0
    assert c["wall_hits"] == 316894 and c["launched"] == N_PHOT
    # ... and the workers cut the range without changing a ray
    import altair_raytracing_amd as isx
    import oracle
    part = SC.replay(_ocfg(oracle), SC.spec_of(scene(isx, isx.default_config(), "photometer")), 60, SEED, first=500, workers=1)
    for k in SC.PER_RAY:
        assert np.array_equal(part[k], r[k][500:560]), k


def test_the_baffles_shadow_detector_and_port(photometer, lamp_open):
    """what the arrangement is for: with the two baffles no ray reaches the detector cap as its first interaction and none leaves
    through the port without one; the bare lamp does both"""
    assert direct(photometer) == (0, 0)
    assert direct(lamp_open) == (38, 100)
    assert lamp_open["census"]["counted_below_z"] == 2331
    assert not lamp_open["baffle_arrivals"].any() and (lamp_open["last_baffle"] == -1).all()


@pytest.mark.parametrize("which", ["photometer", "lamp_open"])
def test_identities(which, photometer, lamp_open):
    """sum(patch_arrivals) + sum(baffle arrivals) == wall_hits; sum(patch_absorbed) + sum(baffle absorbed) == absorbed; the
    per-ray outputs say the same"""
    r = photometer if which == "photometer" else lamp_open
    c = r["census"]
    assert int(r["patch_arrivals"].sum()) + int(r["baffle_arrivals"].sum()) == c["wall_hits"]
    assert int(r["patch_absorbed"].sum()) + int(r["baffle_absorbed"].sum()) == c["absorbed"]
    assert c["exited"] + c["absorbed"] + c["suspended"] == c["launched"] == N_PHOT
    st, npts = r["status"], r["n_points"]
    assert int((npts - 1 - (st == 1)).sum()) == c["wall_hits"]
    assert (r["first_class"][r["last_class"] == -1] < 0).all()      # (no wall interaction at all: the first was none, or a baffle's)
    # a ray with no interaction has neither a class nor a baffle
    none = npts == 2
    assert ((r["last_class"][none & (st == 1)] == -1) & (r["last_baffle"][none & (st == 1)] == -1)).all()
    assert np.abs(np.sqrt((r["start_dir"] ** 2).sum(axis=1)) - 1.0).max() < 1e-15
    assert np.array_equal(r["start_point"], np.tile([0.0, 0.0, 20.0], (N_PHOT, 1)))


def test_led_scenes(orc):
    """the two LED scenes at 2e4 rays: in led_first_in all but three fresh rays meet the disc first"""
    import altair_raytracing_amd as isx
    icfg = isx.default_config()
    sh = SC.replay(_ocfg(orc), SC.spec_of(scene(isx, icfg, "led_shield")), N_PHOT, SEED)
    fi = SC.replay(_ocfg(orc), SC.spec_of(scene(isx, icfg, "led_first_in")), N_PHOT, SEED)
    print("led_shield", sh["baffle_arrivals"].tolist(), sh["census"], "led_first_in", fi["baffle_arrivals"].tolist(), fi["census"])
    assert sh["baffle_arrivals"].tolist() == [[3516, 804]] and sh["census"]["counted_below_z"] == 2579
    assert fi["baffle_arrivals"].tolist() == [[21229, 816]] and fi["census"]["counted_below_z"] == 4023
    # (all but three: rays 14670, 16001 and 19327 start at the top of the LED's disc, 3 degrees upwards, and pass over the rim)
    assert int((fi["first_class"] == -2).sum()) == int((fi["first_kind"] == -2).sum()) == N_PHOT - 3
    for r in (sh, fi):
        assert int(r["patch_arrivals"].sum()) + int(r["baffle_arrivals"].sum()) == r["census"]["wall_hits"]
        assert int(r["patch_absorbed"].sum()) + int(r["baffle_absorbed"].sum()) == r["census"]["absorbed"]


# ---------------------------------------------------------------- the sharded call
def replay_trace(isx, orc):
    """a stand-in tracer for fluxmap_scene_sharded: the replay and the oracle's binning"""
    def trace(c, sp, count, seed, first):
        rep = SC.replay(c, SC.spec_of(sp), count, seed, first, workers=1)
        P, V = SC.counted_lines(c, rep)
        st = orc.Stats()
        for f, val in rep["census"].items():
            setattr(st, f, val)
        cnt = isx.SceneCounts()
        C.memmove(C.byref(cnt), SC.counter_words(rep).tobytes(), C.sizeof(cnt))
        return orc.bin_lines(c, P, V), cnt, st
    return trace


def test_sharded_with_one_rank_is_the_plain_call(orc):
    """fluxmap_scene_sharded without a process group hands the whole range to the tracer and returns its histogram, the 36
    counters and the census"""
    import altair_raytracing_amd as isx
    cfg = _ocfg(orc)
    spec = scene(isx, isx.default_config(), "led_first_in")
    seen = []
    inner = replay_trace(isx, orc)

    def trace(c, sp, count, seed, first):
        seen.append((count, seed, first, sp is spec))
        return inner(c, sp, count, seed, first)

    hits, pa, pb, ba, bb, census = isx.fluxmap_scene_sharded(trace, cfg, spec, 200, SEED, first_ray=1000)
    assert seen == [(200, SEED, 1000, True)]
    assert hits.shape == (cfg.n_theta, cfg.n_phi) and census["launched"] == 200
    assert census["exited"] + census["absorbed"] + census["suspended"] == 200
    assert pa.shape == (10,) and pb.shape == (10,) and ba.shape == (4, 2) and bb.shape == (4, 2)
    assert ba[0].sum() >= 200 and not ba[1:].any() and (bb <= ba).all() and (pb <= pa).all() and not pa[4:].any()
    assert int(pa.sum()) + int(ba.sum()) == census["wall_hits"] and int(pb.sum()) + int(bb.sum()) == census["absorbed"]
    ref = SC.replay(cfg, SC.spec_of(spec), 200, SEED, 1000, workers=1)
    assert np.array_equal(np.concatenate([pa, pb, ba.reshape(-1), bb.reshape(-1)]), SC.counter_words(ref))


N_SHARDED, FIRST_SHARDED = 301, 1000


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import oracle
    import altair_raytracing_amd as isx

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    cfg = _ocfg(oracle)
    spec = scene(isx, isx.default_config(), "led_first_in")
    out = isx.fluxmap_scene_sharded(replay_trace(isx, oracle), cfg, spec, N_SHARDED, SEED, first_ray=FIRST_SHARDED)
    q.put((rank,) + out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_allreduce_equals_single_rank(orc):
    """two ranks over gloo: histogram, the 36 counters and the census of every rank are those of the job in one piece"""
    import socket
    import altair_raytracing_amd as isx
    import torch.multiprocessing as mp

    cfg = _ocfg(orc)
    spec = scene(isx, isx.default_config(), "led_first_in")
    whole = isx.fluxmap_scene_sharded(replay_trace(isx, orc), cfg, spec, N_SHARDED, SEED, first_ray=FIRST_SHARDED)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert whole[5]["launched"] == N_SHARDED and int(whole[3].sum()) >= N_SHARDED
    for out in got:
        rank, parts_ = out[0], out[1:]
        for a, w in zip(parts_[:5], whole[:5]):
            assert a.dtype == np.uint64 and a.shape == w.shape and np.array_equal(a, w), rank
        assert parts_[5] == whole[5], rank
