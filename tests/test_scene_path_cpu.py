"""The scene path histograms (isx_scene_path_hist, isx_scene_path_moments, isx_scene_path_decay) without a GPU: the bindings,
every refusal, the two host helpers against their formulas bit for bit, the C walk of tests/native/scene_path_walk.c against the
oracle's own scene walk and against the Python restatement (tests/scenepath_np.py), hand-made rays whose path length is known by
hand, the contract's identities, the decay constant against the unbinned estimate, and the C walk as a stand-alone program under
AddressSanitizer / UBSan (nothing is preloaded)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import response_np as R
import scene_np as SC
import scenepath_np as SP
from test_scene_cpu import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
RHO = 0.95


def _ocfg(orc, rho=RHO, max_points=None):
    c = orc.default_config()
    c.reflectance = rho
    if max_points is not None:
        c.max_points = max_points
    return c


def side_photometer(isx):
    """`photometer` with the beam `side` of the GPU tests: a 10 cm disc at (-60, 0, -75) that shines a 20 degree cone along +x"""
    cfg = isx.default_config()
    s = scene(isx, cfg, "photometer")
    s.beam = isx.beam_cone(cfg, (-60, 0, -75), (1, 0, 0), 10.0, 20.0, isx.BEAM_UNIFORM)
    return s


# ---------------------------------------------------------------- bindings
def test_binding_structs_and_default_spec():
    import altair_raytracing_amd as isx
    S = isx.ScenePathSpec
    assert C.sizeof(S) == 24 and S.n_bins.offset == 8 and S.reserved1.offset == 12 and S.bin_cm.offset == 16
    assert C.sizeof(isx.ScenePathCounts) == 42 * 8 and isx.ScenePathCounts.checksum.offset == 21 * 8
    assert isx.SCENE_PATH_MAX_BINS == 65536 and SP.FATES == isx.RESPONSE_FATES == 21 and isx.LIGHT_CM_PER_NS == 29.9792458
    cfg = isx.default_config()
    s = isx.default_scene_path_spec(cfg)
    assert (s.struct_size, s.reserved0, s.n_bins, s.reserved1, s.bin_cm) == (24, 0, 1024, 0, cfg.r_in / 4)
    isx.load().isx_default_scene_path_spec(C.byref(cfg), None)      # (a NULL spec is left alone)
    assert bytes(isx.scene_path_spec(1024, cfg.r_in / 4)) == bytes(s)
    pc = isx.ScenePathCounts()
    pc.overflow[20] = 7
    pc.checksum[0] = (1 << 64) - 1
    assert pc.words().tolist() == [0] * 20 + [7] + [(1 << 64) - 1] + [0] * 20
    for name in ("isx_default_scene_path_spec", "isx_scene_path_hist", "isx_scene_path_hist_device", "isx_scene_path_moments",
                 "isx_scene_path_decay"):
        assert name in isx.EXPORTS and hasattr(isx.load(), name)
    for name in ("ScenePathSpec", "ScenePathCounts", "default_scene_path_spec", "scene_path_spec", "scene_path_hist",
                 "scene_path_hist_device", "scene_path_moments", "scene_path_decay", "scene_path_hist_sharded"):
        assert name in isx.__all__ and hasattr(isx, name)
    lib = isx.load()
    for v, rc in ((-1, 0), (0, 0), (8, 0), (65536, 0), (-2, isx.abi.ERR_BAD_ARG), (65537, isx.abi.ERR_BAD_ARG)):
        assert lib.isx_set_option(b"spath_lds_bins", v) == rc, v
    assert lib.isx_set_option(b"spath_lds_bins", -1) == 0


def path_specs(isx):
    """([(what, ScenePathSpec)] that isx.h refuses with ISX_ERR_BAD_CONFIG, [ScenePathSpec] that get past the checks)"""
    bad = []
    for size in (0, 16, 32):
        s = isx.scene_path_spec(512, 25.0); s.struct_size = size
        bad.append(("struct_size %d" % size, s))
    s = isx.scene_path_spec(512, 25.0); s.reserved0 = 1
    bad.append(("reserved0", s))
    s = isx.scene_path_spec(512, 25.0); s.reserved1 = -1
    bad.append(("reserved1", s))
    for v in (0, -1, 65537, 1 << 30, -(1 << 31)):
        bad.append(("n_bins %d" % v, isx.scene_path_spec(v, 25.0)))
    for v in (0.0, -0.0, -1.0, math.inf, -math.inf, math.nan):
        bad.append(("bin_cm %r" % v, isx.scene_path_spec(512, v)))
    return bad, [isx.scene_path_spec(n, b) for n, b in ((1, 1e300), (2, 25.0), (1024, 5e-324), (4096, 0.5), (65536, 1.0))]


def test_refusals_and_null_arguments_need_no_device():
    """Everything isx_scene_endstates refuses of cfg and scene is refused here with its code -- every refusal of each nested spec
    among them; a wrong path spec is ISX_ERR_BAD_CONFIG and a NULL pointer ISX_ERR_BAD_ARG, before anything asks for a device (this
    process never keeps isx_init).  The detector grid and the hit line are no reason for refusal."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ctypes as C
import numpy as np
import altair_raytracing_amd as isx
from test_scene_cpu import refused_scenes
from test_scene_path_cpu import path_specs
from test_baffle_cpu import big_grids
lib = isx.load()
have = lib.isx_init(0) == 0
if have:
    lib.isx_shutdown()
past = isx.abi.ERR_NOT_INIT if have else isx.abi.ERR_NO_DEVICE
buf = np.full(21 * 65536, 7, dtype=np.uint64)
hp = buf.ctypes.data_as(C.POINTER(C.c_uint64))
pd = C.POINTER(C.c_double)
cnt = isx.SceneCounts()
pcnt = isx.ScenePathCounts()
zero = np.zeros(21 * 65536, dtype=np.uint64)
zp = zero.ctypes.data_as(C.POINTER(C.c_uint64))
fr = np.zeros(21)
tau, sig = C.c_double(7.0), C.c_double(7.0)
cfg, good, bad, served = refused_scenes(isx)
pbad, pgood = path_specs(isx)
ps = C.byref(isx.default_scene_path_spec(cfg))
dev = C.c_void_p(4096)
BAD_CONFIG, BAD_ARG = isx.abi.ERR_BAD_CONFIG, isx.abi.ERR_BAD_ARG
nested = set()
for what, c, s in bad:
    assert lib.isx_scene_path_hist(C.byref(c), C.byref(s), ps, 10, 1, 0, hp, C.byref(pcnt), C.byref(cnt), None) == BAD_CONFIG, what
    assert lib.isx_scene_path_hist_device(C.byref(c), C.byref(s), ps, 10, 1, 0, dev, dev, dev) == BAD_CONFIG, what
    nested.add(what.split(":")[0])
assert {"beam", "baffles", "patches"} <= nested
for k, (c, s) in enumerate(served):
    assert lib.isx_scene_path_hist(C.byref(c), C.byref(s), ps, 10, 1, 0, hp, None, None, None) == past, k
    assert lib.isx_scene_path_hist_device(C.byref(c), C.byref(s), ps, 10, 1, 0, dev, dev, dev) == past, k
g, cf = C.byref(good), C.byref(cfg)
for what, o in pbad:
    st = isx.Stats(); st.launched = 77
    assert lib.isx_scene_path_hist(cf, g, C.byref(o), 10, 1, 0, hp, C.byref(pcnt), C.byref(cnt), C.byref(st)) == BAD_CONFIG, what
    assert lib.isx_scene_path_hist_device(cf, g, C.byref(o), 10, 1, 0, dev, dev, dev) == BAD_CONFIG, what
    assert st.launched == 77
    assert lib.isx_scene_path_hist(C.byref(bad[0][1]), C.byref(bad[0][2]), C.byref(o), 10, 1, 0, hp, None, None, None) == BAD_CONFIG, what
    assert lib.isx_scene_path_moments(C.byref(o), zp, C.byref(pcnt), fr.ctypes.data_as(pd), None) == BAD_CONFIG, what
    assert lib.isx_scene_path_decay(C.byref(o), zp, C.byref(pcnt), 18, 0, C.byref(tau), C.byref(sig)) == BAD_CONFIG, what
for o in pgood:
    assert lib.isx_scene_path_hist(cf, g, C.byref(o), 10, 1, 0, hp, None, None, None) == past, o.n_bins
    assert lib.isx_scene_path_hist_device(cf, g, C.byref(o), 10, 1, 0, dev, dev, dev) == past, o.n_bins
    assert lib.isx_scene_path_moments(C.byref(o), zp, C.byref(pcnt), fr.ctypes.data_as(pd), None) == 0, o.n_bins
for k in range(4):      # cfg, scene, pspec, hist
    a = [cf, g, ps, hp]
    a[k] = None
    assert lib.isx_scene_path_hist(a[0], a[1], a[2], 10, 1, 0, a[3], None, None, None) == BAD_ARG, k
for k in range(6):      # cfg, scene, pspec, d_hist, d_path_counts, d_scene_counts
    a = [cf, g, ps, dev, dev, dev]
    a[k] = None
    assert lib.isx_scene_path_hist_device(a[0], a[1], a[2], 10, 1, 0, a[3], a[4], a[5]) == BAD_ARG, k
grids, fits = big_grids(isx)
for what, c in grids:
    assert lib.isx_fluxmap_scene(C.byref(c), g, 10, 1, 0, hp, None, None) == BAD_CONFIG, what
    assert lib.isx_scene_path_hist(C.byref(c), g, ps, 10, 1, 0, hp, None, None, None) == past, what
    assert lib.isx_scene_path_hist_device(C.byref(c), g, ps, 10, 1, 0, dev, dev, dev) == past, what
for nt, nph, mode in ((0, 0, 0), (-5, 7, 1), (1 << 20, 1 << 20, 1)):
    c = cfg.copy(); c.n_theta, c.n_phi, c.hit_line_mode = nt, nph, mode
    assert lib.isx_scene_path_hist(C.byref(c), g, ps, 10, 1, 0, hp, None, None, None) == past, (nt, nph, mode)
assert (buf == 7).all() and not cnt.words().any() and not pcnt.words().any() and tau.value == 7.0 and sig.value == 7.0
try:
    isx.scene_path_hist(cfg, good, pbad[0][1], 10, 1)
    print("no error")
except isx.IsxError as e:
    print("ok", e.status, len(bad), len(served), len(pbad), len(pgood), len(grids))
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["ok", "-2", "146", "22", "16", "5", "4"], r.stdout


def test_no_device_on_a_machine_without_one():
    """where the library can initialise no HIP device, a valid call is ISX_ERR_NO_DEVICE (a process of its own)"""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import altair_raytracing_amd as isx
from test_scene_cpu import scene
lib = isx.load()
if lib.isx_init(0) == 0:
    lib.isx_shutdown()
    print("device")
    raise SystemExit(0)
cfg = isx.default_config()
spec = scene(isx, cfg, "photometer")
ps = isx.default_scene_path_spec(cfg)
for call in (lambda: isx.scene_path_hist(cfg, spec, ps, 10, 1), lambda: isx.scene_path_hist_device(cfg, spec, ps, 10, 1, 0, 4096, 8192, 12288)):
    try:
        call()
        raise SystemExit("no error")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_NO_DEVICE, e.status
print("no device")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() in (["device"], ["no", "device"]), r.stdout + r.stderr[-2000:]


# ---------------------------------------------------------------- the two host helpers
def _rows(rng, n_bins):
    hist = np.zeros((21, n_bins), dtype=np.uint64)
    hist[0] = rng.integers(0, 1000, n_bins)
    hist[3, n_bins // 2] = 17                                 # one bin only: sd 0
    hist[18] = (1e6 * np.exp(-np.arange(n_bins) / 9.0)).astype(np.uint64)
    hist[19, :3] = np.array([5, 0, 1 << 40], dtype=np.uint64)[:n_bins]
    hist[20] = rng.integers(0, 3, n_bins)
    return hist


@pytest.mark.parametrize("n_bins,bin_cm", [(1, 1e300), (64, 25.025), (1000, 0.1)])
def test_moments_equal_the_formulas_bit_for_bit(n_bins, bin_cm):
    import altair_raytracing_amd as isx
    hist = _rows(np.random.default_rng(5), n_bins)
    over = np.zeros(42, dtype=np.uint64)
    over[20] = 1                                              # an overflowed row: NaN
    ps = isx.scene_path_spec(n_bins, bin_cm)
    mean, sd = isx.scene_path_moments(ps, hist, over)
    wm, ws = SP.moments(hist, over[:21], bin_cm)
    assert np.array_equal(mean.view(np.uint64)[~np.isnan(wm)], wm.view(np.uint64)[~np.isnan(wm)])
    assert np.array_equal(sd.view(np.uint64)[~np.isnan(ws)], ws.view(np.uint64)[~np.isnan(ws)])
    assert np.array_equal(np.isnan(mean), np.isnan(wm)) and np.array_equal(np.isnan(sd), np.isnan(ws))
    assert np.isnan(mean[1]) and np.isnan(mean[20]) and np.isnan(sd[20]) and not np.isnan(mean[0])      # empty row, overflowed row
    if n_bins > 1:
        assert sd[3] == 0.0 and mean[3] == (n_bins // 2 + 0.5) * bin_cm
    lib = isx.load()
    pc = isx.ScenePathCounts()
    h = np.ascontiguousarray(hist.reshape(-1))
    hp = h.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.isx_scene_path_moments(C.byref(ps), hp, C.byref(pc), None, None) == 0                    # (either output may be NULL)
    for a in ((None, hp, C.byref(pc)), (C.byref(ps), None, C.byref(pc)), (C.byref(ps), hp, None)):
        assert lib.isx_scene_path_moments(a[0], a[1], a[2], None, None) == isx.abi.ERR_BAD_ARG


def test_decay_equals_the_formulas_bit_for_bit_and_refuses():
    import altair_raytracing_amd as isx
    n_bins, bin_cm = 200, 25.025
    hist = _rows(np.random.default_rng(6), n_bins)
    zero = np.zeros(42, dtype=np.uint64)
    ps = isx.scene_path_spec(n_bins, bin_cm)
    for f, lo in ((18, 0), (18, 7), (18, 100), (0, 0), (0, 199 - 1), (20, 3), (19, 0)):
        got = isx.scene_path_decay(ps, hist, zero, f, lo)
        want = SP.decay(hist, f, lo, bin_cm)
        assert want is not None and np.array_equal(np.array(got).view(np.uint64), np.array(want).view(np.uint64)), (f, lo)
    tau, _ = isx.scene_path_decay(ps, hist, zero, 18, 5)
    assert abs(tau / bin_cm - 9.0) < 0.05                      # (the row was made with a decay of 9 bins)
    BAD_CONFIG, BAD_ARG = isx.abi.ERR_BAD_CONFIG, isx.abi.ERR_BAD_ARG

    def status(*a, **k):
        try:
            isx.scene_path_decay(*a, **k)
            return 0
        except isx.IsxError as e:
            return e.status
    over = zero.copy(); over[18] = 1
    assert status(ps, hist, over, 18, 0) == BAD_CONFIG and status(ps, hist, over, 0, 0) == 0            # an overflowed row
    assert status(ps, hist, zero, 1, 0) == BAD_CONFIG                                                   # N == 0
    assert status(ps, hist, zero, 3, n_bins // 2) == BAD_CONFIG and SP.decay(hist, 3, n_bins // 2, bin_cm) is None     # m == 0
    assert status(ps, hist, zero, 3, n_bins // 2 + 1) == BAD_CONFIG                                     # N == 0 from lo_bin on
    assert status(ps, hist, zero, 0, n_bins - 1) == BAD_CONFIG                                          # the last bin alone: m == 0
    for f, lo in ((-1, 0), (21, 0), (18, -1), (18, n_bins)):
        assert status(ps, hist, zero, f, lo) == BAD_ARG, (f, lo)
    lib = isx.load()
    pc = isx.ScenePathCounts()
    h = np.ascontiguousarray(hist.reshape(-1))
    hp = h.ctypes.data_as(C.POINTER(C.c_uint64))
    t, s = C.c_double(0), C.c_double(0)
    full = [C.byref(ps), hp, C.byref(pc), C.byref(t), C.byref(s)]
    assert lib.isx_scene_path_decay(full[0], full[1], full[2], 18, 0, full[3], full[4]) == 0
    for k in range(5):
        a = list(full)
        a[k] = None
        assert lib.isx_scene_path_decay(a[0], a[1], a[2], 18, 0, a[3], a[4]) == BAD_ARG, k


# ---------------------------------------------------------------- the C walk against the oracle and against Python
PINNED = ("status", "n_points", "last_point", "direction", "start_point", "last_baffle", "last_class")


def _scene_of(orc, name):
    import altair_raytracing_amd as isx
    if name == "side_photometer":
        return _ocfg(orc, max_points=30), SC.spec_of(side_photometer(isx))
    cfg = isx.default_config()
    return _ocfg(orc), SC.spec_of(scene(isx, cfg, name))


_cwalks = {}


def c_walk(orc, name, n):
    if (name, n) not in _cwalks:
        oc, sd = _scene_of(orc, name)
        _cwalks[(name, n)] = SP.walk(orc, oc, sd, n, SEED, 0, nthreads=4)
    return _cwalks[(name, n)]


@pytest.mark.parametrize("name", ["side_photometer", "photometer"])
def test_c_walk_equals_the_oracles_walk(orc, name):
    """2e4 rays: status, n_points, last point, direction, start, last_baffle and last_class are isxo_scene_walk's bit for bit"""
    oc, sd = _scene_of(orc, name)
    w = orc.scene_walk(oc, sd, 20000, SEED, 0, nthreads=4)
    c = c_walk(orc, name, 20000)
    for k in PINNED:
        assert c[k].dtype == w[k].dtype and np.array_equal(c[k].view(np.uint64 if c[k].dtype == np.float64 else np.int32),
                                                          w[k].view(np.uint64 if w[k].dtype == np.float64 else np.int32)), k
    assert np.isfinite(c["path_cm"]).all() and (c["path_cm"] >= 0).all()
    # (any thread count, any cut of the range)
    oc2, _ = _scene_of(orc, name)
    part = SP.walk(orc, oc2, sd, 777, SEED, 5000, nthreads=1)
    assert np.array_equal(SP.bits(part["path_cm"]), SP.bits(c["path_cm"][5000:5777]))


@pytest.mark.parametrize("name", ["side_photometer", "photometer"])
def test_c_walk_path_equals_the_python_restatement(orc, name):
    """2000 rays: L of the C walk is the Python restatement's bit for bit, and so is everything else the two report"""
    oc, sd = _scene_of(orc, name)
    p = SP.replay(oc, sd, 2000, SEED, 0)
    c = c_walk(orc, name, 20000)
    assert np.array_equal(SP.bits(p["path_cm"]), SP.bits(c["path_cm"][:2000]))
    for k in PINNED:
        assert np.array_equal(p[k], c[k][:2000]), k
    f = R.fates(p, oc)
    print(name, "fates of 2000 rays:", np.bincount(f, minlength=21).tolist(), "mean L", float(p["path_cm"].mean()))


def test_the_c_walk_is_clean_under_the_sanitizers(orc, tmp_path):
    """scene_path_walk.c (-DSPW_MAIN) + isx_oracle.c under AddressSanitizer and UBSan as a child process, nothing preloaded: exit
    status 0, and the checksum and the census it prints for 2000 rays of `photometer` at 1 and 4 threads are the library build's"""
    exe = str(tmp_path / "scene_path_walk_main")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-ffp-contract=off", "-mfma", "-msse4.1", "-fopenmp", "-D_GNU_SOURCE", "-DSPW_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "oracle"), "-o", exe, SP.WALK_C, SP.ORACLE_C, "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    c = c_walk(orc, "photometer", 20000)
    b = SP.bits(c["path_cm"][:2000])
    with np.errstate(over="ignore"):
        cks = int(np.add.reduce(b, dtype=np.uint64))
    st = c["status"][:2000]
    want = ["threads %d: checksum %d exited %d absorbed %d suspended %d" % (nt, cks, (st == 1).sum(), (st == 2).sum(), (st == 3).sum())
            for nt in (1, 4)]
    assert r.stdout.splitlines() == want, r.stdout


# ---------------------------------------------------------------- hand-made rays
def edge_scene(mod, which):
    """(cfg, SceneSpec, n_bins, bin_cm) of a scene whose every ray is the same ray, with a path length known by hand.  `mod`: the
    library or the oracle (one layout).
      first_strike   from (0, 0, 0) along +x onto a black wall: absorbed at the first strike, L == r_in
      port           from (0, 0, 0) along -z through the port to the world box: no interaction, L is the tail to the port plane
      other_exit     the same ray with the port plane below the world box: slot 19, no tail, L == 0
      baffle         from (0, 0, 0) along +x onto a black disc at x = 35: one leg
    """
    import altair_raytracing_amd as isx
    c = mod.default_config()
    ic = isx.default_config()
    c.reflectance = 0.0
    direction = (0, 0, -1) if which in ("port", "other_exit") else (1, 0, 0)
    beam = isx.beam_cone(ic, (0, 0, 0), direction, 0.0, 0.0, isx.BEAM_UNIFORM)
    baffles = [isx.baffle_disc(ic, (35, 0, 0), (1, 0, 0), 10.0, 0.0)] if which == "baffle" else []
    if which == "other_exit":
        c.exit_port_z = -2.0 * c.box_half
    return c, isx.scene_spec(ic, beam, baffles, []), 8, c.r_in / 4


def edge_expect(cfg, which):
    """(fate slot, L) by hand, in the contract's arithmetic"""
    f64 = np.float64
    if which == "first_strike":
        return 0, f64(cfg.r_in)                    # (no patch: the wall's class P = 0)
    if which == "port":
        s = f64(cfg.box_half)
        f = (f64(cfg.exit_port_z) - f64(0.0)) / (f64(-cfg.box_half) - f64(0.0))
        assert 0.0 < f <= 1.0
        return SP.PORT, f64(0.0) + s * f
    if which == "other_exit":
        return SP.EXITED_OTHER, f64(0.0)
    # baffle: sp = (0 - 35) * 1, sq = (r_in - 35) * 1, f = sp / (sp - sq), x = 0 + f * (r_in - 0)
    sp, sq = f64(0.0) - f64(35.0), f64(cfg.r_in) - f64(35.0)
    f = sp / (sp - sq)
    x = f64(0.0) + f * (f64(cfg.r_in) - f64(0.0))
    return SP.BAFFLE0 + 1, np.sqrt((x * x + f64(0.0)) + f64(0.0))      # (struck from the side the normal does not point to)


EDGES = ["first_strike", "port", "other_exit", "baffle"]


@pytest.mark.parametrize("which", EDGES)
def test_hand_made_rays(orc, which):
    oc, spec, n_bins, bin_cm = edge_scene(orc, which)
    sd = SC.spec_of(spec)
    fate, L = edge_expect(oc, which)
    for w in (SP.walk(orc, oc, sd, 64, SEED, 0, nthreads=2), SP.replay(oc, sd, 64, SEED, 0, workers=1)):
        assert np.array_equal(SP.bits(w["path_cm"]), np.full(64, SP.bits(np.array([L]))[0])), (which, w["path_cm"][:3], L)
        assert (R.fates(w, oc) == fate).all(), (which, R.fates(w, oc)[:3])
        hist, over, cks = SP.from_walk(w, oc, n_bins, bin_cm)
        want = np.zeros((21, n_bins), dtype=np.uint64)
        want[fate, int(L / bin_cm)] = 64
        assert np.array_equal(hist, want) and not over.any()
        assert int(cks[fate]) == (64 * int(SP.bits(np.array([L]))[0])) % (1 << 64) and not np.delete(cks, fate).any()
    if which == "first_strike":        # L == r_in exactly: bin 4 of 8, and with 4 bins it is overflow (fb == n_bins)
        assert L == oc.r_in and int(L / bin_cm) == 4 and L / bin_cm == 4.0
        hist, over, _ = SP.from_walk(w, oc, 4, bin_cm)
        assert not hist.any() and over[fate] == 64
    if which == "port":
        assert 0.0 < L < oc.box_half and w["n_points"].max() == 2
    if which == "baffle":
        assert abs(L - 35.0) < 1e-12 and (w["last_baffle"] == 1).all()


# ---------------------------------------------------------------- identities
def test_identities_rows_and_split_invariance(orc):
    """rows plus overflow are the response's rows (response_np on the oracle's own walk); n_bins 1 with bin_cm 1e300 is the response's
    row itself; the checksums of a split of the ray range add up modulo 2^64"""
    import altair_raytracing_amd as isx
    oc, sd = _scene_of(orc, "side_photometer")
    c = c_walk(orc, "side_photometer", 20000)
    w = orc.scene_walk(oc, sd, 20000, SEED, 0, nthreads=4)
    resp = R.from_walk(w, oc, isx.response_spec(1, 1, 1, 1), SEED, 0)[:, 0]
    for n_bins, bin_cm in ((1, 1e300), (4, 25.0), (29, 25.0), (4096, 0.5)):
        hist, over, cks = SP.from_walk(c, oc, n_bins, bin_cm)
        assert np.array_equal(hist.sum(axis=1) + over, resp), (n_bins, bin_cm)
        if n_bins == 1:
            assert np.array_equal(hist[:, 0], resp) and not over.any()
        if n_bins == 4:
            assert over.any()
    whole = SP.from_walk(c, oc, 29, 25.0)
    parts = []
    for first, n in ((0, 7001), (7001, 1), (7002, 12998)):
        p = SP.walk(orc, oc, sd, n, SEED, first, nthreads=3)
        parts.append(SP.from_walk(p, oc, 29, 25.0))
    with np.errstate(over="ignore"):
        for k in range(3):
            assert np.array_equal(sum(p[k] for p in parts), whole[k]), k
    assert (whole[2][list((0, 1, 2, 3, 10, 11, 12, 13, 18, 19, 20))] != 0).all()


# ---------------------------------------------------------------- the decay constant
def test_decay_constant_against_the_unbinned_estimate(orc):
    """The port row of the bare default sphere (the default scene: the pencil as the degenerate beam; reflectance 0.99), 2e5 rays of
    the C walk: isx_scene_path_decay from bin lo_bin on against the unbinned mean-excess estimate mean(L - x0 | L >= x0),
    x0 = lo_bin * bin_cm, from the per-ray L.  Bound: |z| < 4 with the helper's sigma -- the project's bound for its statistical
    checks."""
    import altair_raytracing_amd as isx
    cfg = isx.default_config()
    oc = orc.default_config()
    sd = SC.spec_of(isx.default_scene_spec(cfg))
    n = 200_000
    w = SP.walk(orc, oc, sd, n, SEED, 0, nthreads=8)
    f = R.fates(w, oc)
    n_bins, bin_cm, lo_bin = 65536, cfg.r_in / 4, 64
    hist, over, _ = SP.from_rays(w["path_cm"], f, n_bins, bin_cm)
    assert not over.any()
    tau, sigma = isx.scene_path_decay(isx.scene_path_spec(n_bins, bin_cm), hist, np.zeros(42, dtype=np.uint64), SP.PORT, lo_bin)
    assert (tau, sigma) == SP.decay(hist, SP.PORT, lo_bin, bin_cm)
    L = w["path_cm"][f == SP.PORT]
    x0 = lo_bin * bin_cm
    tail = L[L >= x0]
    direct = float((tail - x0).mean())
    z = (tau - direct) / sigma
    print("port rays %d, in the tail %d; tau binned %.2f cm (%.2f ns), unbinned %.2f cm, sigma %.2f cm, z %.3f" % (
        L.size, tail.size, tau, tau / SP.LIGHT_CM_PER_NS, direct, sigma, z))
    assert tail.size > 10_000 and abs(z) < 4.0
