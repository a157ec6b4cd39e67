"""The scene order histograms (isx_scene_order_hist, isx_scene_order_reweight, isx_scene_order_moments) without a GPU: the
bindings, every refusal, the restatement of the contract on the oracle's walk (sceneorder_np) against a plain per-ray loop, the two
host-side helpers against their formulas operation for operation, the reweighted histograms against direct walks of the aged
scene, and the sharded call."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import response_np as R
import scene_np as SC
import sceneorder_np as SO
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
    assert C.sizeof(isx.SceneOrderSpec) == 16 and isx.SceneOrderSpec.n_orders.offset == 8 and isx.SceneOrderSpec.reserved1.offset == 12
    assert C.sizeof(isx.SceneOrderCounts) == 21 * 8 and isx.SCENE_ORDER_MAX_ORDERS == 65536 and SO.FATES == isx.RESPONSE_FATES == 21
    cfg = isx.default_config()
    s = isx.default_scene_order_spec(cfg)
    assert (s.struct_size, s.reserved0, s.n_orders, s.reserved1) == (16, 0, 512, 0)
    isx.load().isx_default_scene_order_spec(C.byref(cfg), None)      # (a NULL spec is left alone)
    assert bytes(isx.scene_order_spec(512)) == bytes(s)
    t = isx.scene_order_spec(29)
    assert (t.struct_size, t.n_orders) == (16, 29)
    oc = isx.SceneOrderCounts()
    oc.overflow[20] = 7
    assert oc.words().tolist() == [0] * 20 + [7]
    for name in ("isx_default_scene_order_spec", "isx_scene_order_hist", "isx_scene_order_hist_device", "isx_scene_order_reweight",
                 "isx_scene_order_moments"):
        assert name in isx.EXPORTS and hasattr(isx.load(), name)
    for name in ("SceneOrderSpec", "SceneOrderCounts", "default_scene_order_spec", "scene_order_spec", "scene_order_hist",
                 "scene_order_hist_device", "scene_order_reweight", "scene_order_moments", "scene_order_hist_sharded"):
        assert name in isx.__all__ and hasattr(isx, name)
    # the switch is known with and without a device, and keeps to its range
    lib = isx.load()
    for v, rc in ((-1, 0), (0, 0), (8, 0), (65536, 0), (-2, isx.abi.ERR_BAD_ARG), (65537, isx.abi.ERR_BAD_ARG)):
        assert lib.isx_set_option(b"sorder_lds_orders", v) == rc, v
    assert lib.isx_set_option(b"sorder_lds_orders", -1) == 0


def order_specs(isx):
    """([(what, SceneOrderSpec)] that isx.h refuses with ISX_ERR_BAD_CONFIG, [SceneOrderSpec] that get past the checks)"""
    bad = []
    for size in (0, 8, 24):
        s = isx.scene_order_spec(512); s.struct_size = size
        bad.append(("struct_size %d" % size, s))
    s = isx.scene_order_spec(512); s.reserved0 = 1
    bad.append(("reserved0", s))
    s = isx.scene_order_spec(512); s.reserved1 = -1
    bad.append(("reserved1", s))
    for v in (0, -1, 65537, 1 << 30, -(1 << 31)):
        bad.append(("n_orders %d" % v, isx.scene_order_spec(v)))
    return bad, [isx.scene_order_spec(v) for v in (1, 2, 512, 4096, 65536)]


def test_refusals_and_null_arguments_need_no_device():
    """Everything isx_scene_endstates refuses of cfg and scene is refused here with its code; a wrong order spec is
    ISX_ERR_BAD_CONFIG and a NULL pointer ISX_ERR_BAD_ARG, before anything asks for a device (this process never keeps isx_init).
    The detector grid and the hit line are no reason for refusal.  The reweighting refuses the same scenes and specs."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ctypes as C
import numpy as np
import altair_raytracing_amd as isx
from test_scene_cpu import refused_scenes
from test_scene_order_cpu import order_specs
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
ocnt = isx.SceneOrderCounts()
zero = np.zeros(21 * 65536, dtype=np.uint64)
zp = zero.ctypes.data_as(C.POINTER(C.c_uint64))
one, fr = np.ones(1), np.zeros(21)
cfg, good, bad, served = refused_scenes(isx)
obad, ogood = order_specs(isx)
os_ = C.byref(isx.default_scene_order_spec(cfg))
dev = C.c_void_p(4096)
BAD_CONFIG, BAD_ARG = isx.abi.ERR_BAD_CONFIG, isx.abi.ERR_BAD_ARG
def reweight(c, s, o):
    return lib.isx_scene_order_reweight(c, s, o, zp, C.byref(ocnt), 10, one.ctypes.data_as(pd), 1, fr.ctypes.data_as(pd), None)
for what, c, s in bad:
    assert lib.isx_scene_order_hist(C.byref(c), C.byref(s), os_, 10, 1, 0, hp, C.byref(ocnt), C.byref(cnt), None) == BAD_CONFIG, what
    assert lib.isx_scene_order_hist_device(C.byref(c), C.byref(s), os_, 10, 1, 0, dev, dev, dev) == BAD_CONFIG, what
    assert reweight(C.byref(c), C.byref(s), os_) == BAD_CONFIG, what
for k, (c, s) in enumerate(served):
    assert lib.isx_scene_order_hist(C.byref(c), C.byref(s), os_, 10, 1, 0, hp, None, None, None) == past, k
    assert lib.isx_scene_order_hist_device(C.byref(c), C.byref(s), os_, 10, 1, 0, dev, dev, dev) == past, k
    assert reweight(C.byref(c), C.byref(s), os_) == 0, k
g, cf = C.byref(good), C.byref(cfg)
for what, o in obad:
    st = isx.Stats(); st.launched = 77
    assert lib.isx_scene_order_hist(cf, g, C.byref(o), 10, 1, 0, hp, C.byref(ocnt), C.byref(cnt), C.byref(st)) == BAD_CONFIG, what
    assert lib.isx_scene_order_hist_device(cf, g, C.byref(o), 10, 1, 0, dev, dev, dev) == BAD_CONFIG, what
    assert st.launched == 77
    # (a refused scene with a refused spec is refused all the same)
    assert lib.isx_scene_order_hist(C.byref(bad[0][1]), C.byref(bad[0][2]), C.byref(o), 10, 1, 0, hp, None, None, None) == BAD_CONFIG, what
    assert reweight(cf, g, C.byref(o)) == BAD_CONFIG, what
    assert lib.isx_scene_order_moments(C.byref(o), zp, C.byref(ocnt), fr.ctypes.data_as(pd), None) == BAD_CONFIG, what
for o in ogood:
    assert lib.isx_scene_order_hist(cf, g, C.byref(o), 10, 1, 0, hp, None, None, None) == past, o.n_orders
    assert lib.isx_scene_order_hist_device(cf, g, C.byref(o), 10, 1, 0, dev, dev, dev) == past, o.n_orders
    assert reweight(cf, g, C.byref(o)) == 0, o.n_orders
    assert lib.isx_scene_order_moments(C.byref(o), zp, C.byref(ocnt), fr.ctypes.data_as(pd), None) == 0, o.n_orders
for k in range(4):      # cfg, scene, ospec, hist
    a = [cf, g, os_, hp]
    a[k] = None
    assert lib.isx_scene_order_hist(a[0], a[1], a[2], 10, 1, 0, a[3], None, None, None) == BAD_ARG, k
for k in range(6):      # cfg, scene, ospec, d_hist, d_order_counts, d_scene_counts
    a = [cf, g, os_, dev, dev, dev]
    a[k] = None
    assert lib.isx_scene_order_hist_device(a[0], a[1], a[2], 10, 1, 0, a[3], a[4], a[5]) == BAD_ARG, k
# the detector grid and the hit line are ignored: what isx_fluxmap_scene refuses for its grid gets past the checks here
grids, fits = big_grids(isx)
for what, c in grids:
    assert lib.isx_fluxmap_scene(C.byref(c), g, 10, 1, 0, hp, None, None) == BAD_CONFIG, what
    assert lib.isx_scene_order_hist(C.byref(c), g, os_, 10, 1, 0, hp, None, None, None) == past, what
    assert lib.isx_scene_order_hist_device(C.byref(c), g, os_, 10, 1, 0, dev, dev, dev) == past, what
for nt, nph, mode in ((0, 0, 0), (-5, 7, 1), (1 << 20, 1 << 20, 1)):
    c = cfg.copy(); c.n_theta, c.n_phi, c.hit_line_mode = nt, nph, mode
    assert lib.isx_scene_order_hist(C.byref(c), g, os_, 10, 1, 0, hp, None, None, None) == past, (nt, nph, mode)
assert (buf == 7).all() and not cnt.words().any() and not ocnt.words().any()
try:
    isx.scene_order_hist(cfg, good, obad[0][1], 10, 1)
    print("no error")
except isx.IsxError as e:
    print("ok", e.status, len(bad), len(served), len(obad), len(ogood), len(grids))
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["ok", "-2", "146", "22", "10", "5", "4"], r.stdout


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
    print("device")      # (test_refusals_and_null_arguments_need_no_device covers the machine with a device)
    raise SystemExit(0)
cfg = isx.default_config()
spec = scene(isx, cfg, "photometer")
os_ = isx.default_scene_order_spec(cfg)
for call in (lambda: isx.scene_order_hist(cfg, spec, os_, 10, 1), lambda: isx.scene_order_hist_device(cfg, spec, os_, 10, 1, 0, 4096, 8192, 12288)):
    try:
        call()
        raise SystemExit("no error")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_NO_DEVICE, e.status
print("no device")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() in (["device"], ["no", "device"]), r.stdout + r.stderr[-2000:]


# ---------------------------------------------------------------- the restatement: sceneorder_np on the oracle
def test_restatement_against_a_per_ray_loop(orc):
    """2000 rays of side_photometer with at most 30 points, 16 orders: from_walk against the contract read ray by ray"""
    import altair_raytracing_amd as isx
    cfg = _ocfg(orc, max_points=30)
    w = orc.scene_walk(cfg, SC.spec_of(side_photometer(isx)), 2000, SEED, 0, nthreads=2)
    n_orders = 16
    hist, over = SO.from_walk(w, cfg, n_orders)
    want, wover, ksum = np.zeros((21, n_orders), dtype=np.uint64), np.zeros(21, dtype=np.uint64), 0
    fate = R.fates(w, cfg)
    for i in range(2000):
        status, npts = int(w["status"][i]), int(w["n_points"][i])
        k = npts - 2 if status == R.EXITED else npts - 1
        ksum += k
        if k >= n_orders:
            wover[fate[i]] += np.uint64(1)
        else:
            want[fate[i], k] += np.uint64(1)
    assert np.array_equal(hist, want) and np.array_equal(over, wover) and ksum == w["census"]["wall_hits"]
    assert hist.dtype == np.uint64 and int(hist.sum()) + int(over.sum()) == 2000
    # every kind of row takes part, on both sides of the limit
    assert over[20] == w["census"]["suspended"] > 0 and not hist[20].any()      # (a suspended ray has k = 29)
    assert hist[18].sum() > 0 and hist[2].sum() > 0 and over[2] > 0 and hist[10:14].sum() > 0
    # with room for every order nothing overflows, and the orders weigh wall_hits (asserted inside from_walk)
    full, none = SO.from_walk(w, cfg, 64)
    assert not none.any() and np.array_equal(full[:, :n_orders], hist) and np.array_equal(full[:, n_orders:].sum(axis=1), over)
    # a part of the range: the same rays
    part = orc.scene_walk(cfg, SC.spec_of(side_photometer(isx)), 300, SEED, 1000, nthreads=2)
    ph, po = SO.from_walk(part, cfg, n_orders)
    k = SO.orders(w)[1000:1300]
    f = fate[1000:1300]
    assert np.array_equal(ph, np.bincount(f[k < n_orders] * n_orders + k[k < n_orders], minlength=21 * n_orders).reshape(21, n_orders))
    assert np.array_equal(po, np.bincount(f[k >= n_orders], minlength=21))


# ---------------------------------------------------------------- the helpers against their formulas
def _random_hist(rng, K, P=2, nb=2):
    hist = rng.integers(0, 5000, size=(21, K)).astype(np.uint64)
    hist[P + 2:10] = 0
    hist[10 + 2 * nb:18] = 0
    hist[:18, 0] = 0
    return hist


def test_reweight_against_the_formulas():
    import altair_raytracing_amd as isx
    rng = np.random.default_rng(11)
    cfg = isx.default_config()
    cfg.reflectance = RHO
    sc = scene(isx, cfg, "photometer")      # det 0.0, sample 0.5, two baffles of 0.9, the wall 0.95
    rho = SO.surface_rho(cfg, sc)
    assert rho[:4] == [0.0, 0.5, RHO, RHO] and rho[10:14] == [0.9] * 4 and all(r < 0 for r in rho[4:10] + rho[14:18])
    none = np.zeros(21, dtype=np.uint64)
    for K in (1, 2, 29, 512):
        hist = _random_hist(rng, K)
        launched = int(hist.sum()) + 17
        scale = [1.0, 0.95, 0.9, 0.5, 0.0, 1.0 / RHO]
        frac, sig = isx.scene_order_reweight(cfg, sc, isx.scene_order_spec(K), hist, none, launched, scale)
        wf, ws = SO.reweight(hist, launched, scale, rho)
        assert frac.shape == sig.shape == (6, 21)
        assert np.array_equal(frac, wf) and np.array_equal(sig, ws)
        # t == 1: the row sums over launched exactly as the division gives it
        assert np.array_equal(frac[0], hist.sum(axis=1).astype(np.float64) / float(launched))
        # t == 0: what ends at its first interaction, and the rays that never interact
        if K >= 2:
            assert np.array_equal(frac[4, 18:], hist[18:, 0] / float(launched))
            assert np.array_equal(frac[4, 1], (1.0 / (1.0 - 0.5)) * hist[1, 1] / float(launched))
        assert not frac[:, 4:10].any() and not frac[:, 14:18].any() and not sig[:, 4:10].any()
        # sigma may be NULL, n_scale may be 0
        lib, fr = isx.load(), np.zeros(21)
        t1 = np.ones(1)
        pu, pd = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
        oc = isx.SceneOrderCounts()
        os_ = isx.scene_order_spec(K)
        assert lib.isx_scene_order_reweight(C.byref(cfg), C.byref(sc), C.byref(os_), hist.ctypes.data_as(pu), C.byref(oc), launched,
                                            t1.ctypes.data_as(pd), 1, fr.ctypes.data_as(pd), None) == 0
        assert np.array_equal(fr, frac[0])
        assert lib.isx_scene_order_reweight(C.byref(cfg), C.byref(sc), C.byref(os_), hist.ctypes.data_as(pu), C.byref(oc), launched,
                                            None, 0, None, None) == 0


def test_reweight_of_a_perfect_mirror_row_is_nan():
    """a surface of reflectance 1 absorbs nothing: its rows are empty by construction, NaN for t != 1 and 0 for t == 1"""
    import altair_raytracing_amd as isx
    cfg = isx.default_config()
    cfg.reflectance = 0.9
    sc = isx.scene_spec(cfg, None, [isx.baffle_disc(cfg, (35, 0, 13), (1, 0, 0), 10.0, 1.0)], [isx.wall_patch_cap(cfg, (1, 0, 0), 5.0, 1.0)])
    K = 8
    hist = np.zeros((21, K), dtype=np.uint64)
    hist[1, 1:] = 5; hist[2, 3] = 7; hist[18, 2] = 9
    frac, sig = isx.scene_order_reweight(cfg, sc, isx.scene_order_spec(K), hist, np.zeros(21, dtype=np.uint64), 100, [1.0, 0.5])
    wf, ws = SO.reweight(hist, 100, [1.0, 0.5], SO.surface_rho(cfg, sc))
    assert np.array_equal(frac, wf, equal_nan=True) and np.array_equal(sig, ws, equal_nan=True)
    for f in (0, 10, 11):
        assert frac[0, f] == 0.0 and sig[0, f] == 0.0 and math.isnan(frac[1, f]) and math.isnan(sig[1, f])
    assert np.isfinite(frac[:, [1, 2, 18]]).all() and frac[1, 18] == 9 * 0.25 / 100.0


def test_reweight_refusals():
    import altair_raytracing_amd as isx
    lib = isx.load()
    cfg = isx.default_config()
    cfg.reflectance = RHO
    sc = scene(isx, cfg, "photometer")
    K = 6
    os_ = isx.scene_order_spec(K)
    hist = _random_hist(np.random.default_rng(5), K)
    oc = isx.SceneOrderCounts()
    t, fr, sg = np.array([1.0, 0.9]), np.zeros(42), np.zeros(42)
    pu, pd = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    args = [C.byref(cfg), C.byref(sc), C.byref(os_), hist.ctypes.data_as(pu), C.byref(oc), 10 ** 6, t.ctypes.data_as(pd), 2,
            fr.ctypes.data_as(pd)]
    assert lib.isx_scene_order_reweight(*args, sg.ctypes.data_as(pd)) == 0
    for k in (0, 1, 2, 3, 4, 6, 8):      # cfg, scene, ospec, hist, counts, scale, fraction
        a = list(args); a[k] = None
        assert lib.isx_scene_order_reweight(*a, None) == isx.abi.ERR_BAD_ARG, k
    a = list(args); a[7] = -1
    assert lib.isx_scene_order_reweight(*a, None) == isx.abi.ERR_BAD_ARG
    none = np.zeros(21, dtype=np.uint64)
    for v in (-1.0, -1e-300, np.nan, np.inf, -np.inf, 1.0 / RHO * (1 + 1e-12), 1.06, 2.0):      # (t * 0.95 above 1: the wall)
        with pytest.raises(isx.IsxError) as e:
            isx.scene_order_reweight(cfg, sc, os_, hist, none, 10 ** 6, [1.0, v])
        assert e.value.status == isx.abi.ERR_BAD_ARG, v
    isx.scene_order_reweight(cfg, sc, os_, hist, none, 10 ** 6, [1.0 / RHO])      # (t * rho == 1 exactly at most: allowed)
    # a surface brighter than the wall sets the limit
    bright = isx.scene_spec(cfg, None, [], [isx.wall_patch_cap(cfg, (1, 0, 0), 5.0, 0.99)])
    with pytest.raises(isx.IsxError) as e:
        isx.scene_order_reweight(cfg, bright, os_, hist, none, 10 ** 6, [1.02])
    assert e.value.status == isx.abi.ERR_BAD_ARG
    for f in (0, 18, 20, 7):      # any overflow, even of a slot the scene cannot fill
        over = none.copy(); over[f] = 1
        with pytest.raises(isx.IsxError) as e:
            isx.scene_order_reweight(cfg, sc, os_, hist, over, 10 ** 6, [1.0])
        assert e.value.status == isx.abi.ERR_BAD_CONFIG, f
    with pytest.raises(isx.IsxError) as e:
        isx.scene_order_reweight(cfg, sc, os_, hist, none, 0, [1.0])
    assert e.value.status == isx.abi.ERR_BAD_CONFIG
    with pytest.raises(ValueError):
        isx.scene_order_reweight(cfg, sc, os_, hist.reshape(-1)[:10], none, 10, [1.0])


def test_moments_against_the_formulas():
    import altair_raytracing_amd as isx
    rng = np.random.default_rng(13)
    lib = isx.load()
    for K in (1, 2, 29, 512):
        hist = _random_hist(rng, K)
        over = np.zeros(21, dtype=np.uint64)
        over[1] = 3
        mean, sd = isx.scene_order_moments(isx.scene_order_spec(K), hist, over)
        wm, ws = SO.moments(hist, over)
        assert np.array_equal(mean, wm, equal_nan=True) and np.array_equal(sd, ws, equal_nan=True)
        empty = [f for f in range(21) if not hist[f].any()]
        assert all(math.isnan(mean[f]) and math.isnan(sd[f]) for f in empty + [1]) and len(empty) >= 10
        full = [f for f in range(21) if hist[f].any() and f != 1]
        assert np.isfinite(mean[full]).all() and np.isfinite(sd[full]).all()
        k = np.arange(K, dtype=np.float64)
        for f in full:
            h = hist[f].astype(np.float64)
            assert abs(mean[f] - (k * h).sum() / h.sum()) <= 1e-12 * max(1.0, mean[f])
    # one order only: the mean is that order, the deviation 0; either output may be NULL
    hist = np.zeros((21, 8), dtype=np.uint64)
    hist[18, 5] = 9
    mean, sd = isx.scene_order_moments(isx.scene_order_spec(8), hist, np.zeros(21, dtype=np.uint64))
    assert mean[18] == 5.0 and sd[18] == 0.0
    os_, oc, out = isx.scene_order_spec(8), isx.SceneOrderCounts(), np.zeros(21)
    pu, pd = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    assert lib.isx_scene_order_moments(C.byref(os_), hist.ctypes.data_as(pu), C.byref(oc), None, out.ctypes.data_as(pd)) == 0 and out[18] == 0.0
    assert lib.isx_scene_order_moments(C.byref(os_), hist.ctypes.data_as(pu), C.byref(oc), out.ctypes.data_as(pd), None) == 0 and out[18] == 5.0
    for k in range(3):
        a = [C.byref(os_), hist.ctypes.data_as(pu), C.byref(oc)]
        a[k] = None
        assert lib.isx_scene_order_moments(*a, out.ctypes.data_as(pd), None) == isx.abi.ERR_BAD_ARG, k


# ---------------------------------------------------------------- the reweighting against direct walks of the aged scene
N_Z = 200_000


@pytest.fixture(scope="module")
def side_walk(orc):
    """side_photometer at wall reflectance 0.95, 2e5 rays, seed 12345: computed once, shared, never changed"""
    import altair_raytracing_amd as isx
    return orc.scene_walk(_ocfg(orc), SC.spec_of(side_photometer(isx)), N_Z, SEED, 0, nthreads=16)


def _aged(isx, orc, t):
    """the configuration and the scene with every reflectance multiplied by t"""
    c = _ocfg(orc, RHO * t)
    s = side_photometer(isx)
    for p in range(s.patches.n_patches):
        s.patches.patch[p].reflectance *= t
    for b in range(s.baffles.n_baffles):
        s.baffles.baffle[b].reflectance *= t
    return c, s


def test_reweighted_histograms_are_the_aged_scene(orc, side_walk):
    """One walk of side_photometer reweighted to t = 0.95 and t = 0.90 against direct walks, with other seeds, of the scene with
    every reflectance -- the wall's 0.95, the detector's 0, the sample's 0.5, the baffles' 0.9 -- multiplied by t: two independent
    estimates of the same fractions.  z per slot that holds at least 100 rays in both walks, from the reweighting's sigma and the
    direct walk's binomial error; |z| <= 4.  Found at 2e5 rays (docs/LOG.md section 26): t = 0.95: z -0.95 .. +1.23 over ten
    slots; t = 0.90: z -2.76 (the detector) .. +1.68."""
    import altair_raytracing_amd as isx
    cfg = _ocfg(orc)
    icfg = isx.default_config()
    icfg.reflectance = RHO
    sc = side_photometer(isx)
    K = 1024
    hist, over = SO.from_walk(side_walk, cfg, K)
    rows = hist.sum(axis=1)
    print("fates of side_photometer at 2e5 rays:", rows.tolist(), "largest k", int(SO.orders(side_walk).max()))
    assert not over.any()
    # the slots the test is about pass the cap: the detector patch, the port, and wall class P
    assert rows[0] >= 100 and rows[18] >= 100 and rows[2] >= 100
    scale = [0.95, 0.90]
    frac, sig = isx.scene_order_reweight(icfg, sc, isx.scene_order_spec(K), hist, over, N_Z, scale)
    for i, t in enumerate(scale):
        c2, s2 = _aged(isx, orc, t)
        d = orc.scene_walk(c2, SC.spec_of(s2), N_Z, 778 + i, 0, nthreads=16)
        dh, dov = SO.from_walk(d, c2, K)
        direct = (dh.sum(axis=1) + dov).astype(np.float64)
        fd = direct / N_Z
        sd = np.sqrt(fd * (1.0 - fd) / N_Z)
        slots = [f for f in range(21) if direct[f] >= 100 and rows[f] >= 100]
        z = {f: float((frac[i, f] - fd[f]) / np.sqrt(sig[i, f] ** 2 + sd[f] ** 2)) for f in slots}
        print("t", t, "slots", slots, "reweighted", [round(float(frac[i, f]), 5) for f in slots], "direct",
              [round(float(fd[f]), 5) for f in slots], "z", {f: round(v, 2) for f, v in z.items()})
        assert 0 in slots and 2 in slots and 18 in slots and len(slots) >= 8
        assert max(abs(v) for v in z.values()) <= 4.0, z
    # the time response of the same walk: the port's light has fewer interactions behind it than what the wall absorbs
    mean, sd = isx.scene_order_moments(isx.scene_order_spec(K), hist, over)
    k, f = SO.orders(side_walk), R.fates(side_walk, cfg)
    for slot in (0, 2, 18):
        assert abs(mean[slot] - k[f == slot].mean()) < 1e-9 and abs(sd[slot] - k[f == slot].std()) < 1e-9
    print("mean k: detector %.2f, wall %.2f, port %.2f" % (mean[0], mean[2], mean[18]))


# ---------------------------------------------------------------- the sharded call
def walk_trace(isx, orc):
    """a stand-in tracer for scene_order_hist_sharded: the oracle's walk and the restatement"""
    def trace(c, sp, os_, count, seed, first):
        w = orc.scene_walk(c, SC.spec_of(sp), count, seed, first, nthreads=2)
        st = orc.Stats()
        for f, val in w["census"].items():
            setattr(st, f, val)
        hist, over = SO.from_walk(w, c, os_.n_orders)
        st.bin_increments = int(hist.sum())
        cnt = isx.SceneCounts()
        C.memmove(C.byref(cnt), SC.counter_words(w).tobytes(), C.sizeof(cnt))
        oc = isx.SceneOrderCounts()
        C.memmove(C.byref(oc), over.tobytes(), C.sizeof(oc))
        return hist, oc, cnt, st
    return trace


N_SHARDED, FIRST_SHARDED = 3001, 1000


def test_sharded_with_one_rank_is_the_plain_call(orc):
    import altair_raytracing_amd as isx
    cfg = _ocfg(orc)
    spec = scene(isx, isx.default_config(), "photometer")
    os_ = isx.scene_order_spec(12)
    seen = []
    inner = walk_trace(isx, orc)

    def trace(c, sp, o, count, seed, first):
        seen.append((count, seed, first, sp is spec, o is os_))
        return inner(c, sp, o, count, seed, first)

    hist, over, pa, pb, ba, bb, census = isx.scene_order_hist_sharded(trace, cfg, spec, os_, N_SHARDED, SEED, first_ray=FIRST_SHARDED)
    assert seen == [(N_SHARDED, SEED, FIRST_SHARDED, True, True)]
    assert hist.shape == (21, 12) and hist.dtype == np.uint64 and over.shape == (21,) and over.any()
    assert int(hist.sum()) + int(over.sum()) == N_SHARDED == census["launched"] and int(hist.sum()) == census["bin_increments"]
    rows = hist.sum(axis=1) + over
    assert np.array_equal(rows[:10], pb) and np.array_equal(rows[10:18], bb.reshape(-1))
    assert rows[18] == census["counted_below_z"] and rows[18] + rows[19] == census["exited"] and rows[20] == census["suspended"]
    assert pa.shape == (10,) and ba.shape == (4, 2) and int(pa.sum()) + int(ba.sum()) == census["wall_hits"]


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import oracle
    import altair_raytracing_amd as isx

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    cfg = _ocfg(oracle)
    spec = scene(isx, isx.default_config(), "photometer")
    out = isx.scene_order_hist_sharded(walk_trace(isx, oracle), cfg, spec, isx.scene_order_spec(12), N_SHARDED, SEED,
                                       first_ray=FIRST_SHARDED)
    q.put((rank,) + out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_allreduce_equals_single_rank(orc):
    """two ranks over gloo: the histograms, the overflow, the 36 counters and the census of every rank are those of the job in one
    piece"""
    import socket
    import altair_raytracing_amd as isx
    import torch.multiprocessing as mp

    cfg = _ocfg(orc)
    spec = scene(isx, isx.default_config(), "photometer")
    whole = isx.scene_order_hist_sharded(walk_trace(isx, orc), cfg, spec, isx.scene_order_spec(12), N_SHARDED, SEED,
                                         first_ray=FIRST_SHARDED)
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
    assert whole[6]["launched"] == N_SHARDED and int(whole[0].sum()) + int(whole[1].sum()) == N_SHARDED
    for out in got:
        rank, parts_ = out[0], out[1:]
        for a, w in zip(parts_[:6], whole[:6]):
            assert a.dtype == np.uint64 and a.shape == w.shape and np.array_equal(a, w), rank
        assert parts_[6] == whole[6], rank
