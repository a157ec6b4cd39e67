"""The scene response (isx_scene_response, isx_response_reweight) without a GPU: the bindings, every refusal, the host-side
reweighting against its formulas in numpy, the restatement of the contract on the oracle's walk (response_np) -- its Philox against
the oracle's, its rows against the walk's totals -- the reweighted response against a direct walk of the narrower lamp, and the
sharded call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import response_np as R
import scene_np as SC
from test_scene_cpu import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
RHO = 0.95


# ---------------------------------------------------------------- bindings
def test_binding_struct_and_default_spec():
    import altair_raytracing_amd as isx
    assert C.sizeof(isx.ResponseSpec) == 24 and isx.ResponseSpec.n.offset == 8
    assert isx.RESPONSE_FATES == R.FATES == 21 and isx.abi.RESPONSE_MAX_AXIS == 1024 and isx.abi.RESPONSE_MAX_BINS == 4096
    assert (isx.abi.RESPONSE_BAFFLE0, isx.abi.RESPONSE_PORT, isx.abi.RESPONSE_EXITED_OTHER, isx.abi.RESPONSE_SUSPENDED) == (10, 18, 19, 20)
    cfg = isx.default_config()
    s = isx.default_response_spec(cfg)
    assert s.struct_size == 24 and s.reserved0 == 0 and list(s.n) == [1, 1, 6, 12] and s.bins == 72
    isx.load().isx_default_response_spec(C.byref(cfg), None)      # (a NULL spec is left alone)
    t = isx.response_spec(3, 5, 7, 11)
    assert t.struct_size == 24 and list(t.n) == [3, 5, 7, 11] and t.bins == 1155
    assert bytes(isx.response_spec(1, 1, 6, 12)) == bytes(s)
    for name in ("isx_default_response_spec", "isx_scene_response", "isx_scene_response_device", "isx_response_reweight"):
        assert name in isx.EXPORTS and hasattr(isx.load(), name)
    for name in ("ResponseSpec", "response_spec", "default_response_spec", "scene_response", "scene_response_device",
                 "response_reweight", "scene_response_sharded"):
        assert name in isx.__all__ and hasattr(isx, name)


def response_specs(isx):
    """([(what, ResponseSpec)] that isx.h refuses with ISX_ERR_BAD_CONFIG, [ResponseSpec] that get past the checks)"""
    bad = []
    for size in (0, 16, 32):
        s = isx.response_spec(1, 1, 6, 12); s.struct_size = size
        bad.append(("struct_size %d" % size, s))
    s = isx.response_spec(1, 1, 6, 12); s.reserved0 = 1
    bad.append(("reserved0", s))
    for a in range(4):
        for v in (0, -1, 1025, 1 << 30, -(1 << 31)):
            n = [1, 1, 1, 1]; n[a] = v
            bad.append(("axis %d = %d" % (a, v), isx.response_spec(*n)))
    for n in ((4097 // 17 + 1, 17, 1, 1), (64, 65, 1, 1), (1, 8, 513, 1), (1024, 1024, 1024, 1024), (2, 1024, 1, 3), (16, 16, 16, 17)):
        bad.append(("B of %r" % (n,), isx.response_spec(*n)))
    good = [isx.response_spec(*n) for n in ((1, 1, 1, 1), (1, 1, 6, 12), (3, 5, 7, 11), (4, 1, 1, 1024), (1024, 4, 1, 1), (8, 8, 8, 8),
                                            (1, 1024, 2, 2), (64, 64, 1, 1))]
    return bad, good


def test_refusals_and_null_arguments_need_no_device():
    """Everything isx_scene_endstates refuses of cfg and scene is refused here with its code; a wrong response spec is
    ISX_ERR_BAD_CONFIG and a NULL pointer ISX_ERR_BAD_ARG, before anything asks for a device (this process never keeps isx_init).
    The detector grid and the hit line are no reason for refusal: grids that isx_fluxmap_scene refuses get past the checks."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ctypes as C
import numpy as np
import altair_raytracing_amd as isx
from test_scene_cpu import refused_scenes
from test_scene_response_cpu import response_specs
from test_baffle_cpu import big_grids
lib = isx.load()
have = lib.isx_init(0) == 0
if have:
    lib.isx_shutdown()
past = isx.abi.ERR_NOT_INIT if have else isx.abi.ERR_NO_DEVICE
buf = np.full(21 * 4096, 7, dtype=np.uint64)
hp = buf.ctypes.data_as(C.POINTER(C.c_uint64))
cnt = isx.SceneCounts()
cfg, good, bad, served = refused_scenes(isx)
rbad, rgood = response_specs(isx)
rs = C.byref(isx.default_response_spec(cfg))
dev = C.c_void_p(4096)
BAD_CONFIG, BAD_ARG = isx.abi.ERR_BAD_CONFIG, isx.abi.ERR_BAD_ARG
for what, c, s in bad:
    assert lib.isx_scene_response(C.byref(c), C.byref(s), rs, 10, 1, 0, hp, C.byref(cnt), None) == BAD_CONFIG, what
    assert lib.isx_scene_response_device(C.byref(c), C.byref(s), rs, 10, 1, 0, dev, dev) == BAD_CONFIG, what
for k, (c, s) in enumerate(served):
    assert lib.isx_scene_response(C.byref(c), C.byref(s), rs, 10, 1, 0, hp, None, None) == past, k
    assert lib.isx_scene_response_device(C.byref(c), C.byref(s), rs, 10, 1, 0, dev, dev) == past, k
g, cf = C.byref(good), C.byref(cfg)
for what, r in rbad:
    st = isx.Stats(); st.launched = 77
    assert lib.isx_scene_response(cf, g, C.byref(r), 10, 1, 0, hp, C.byref(cnt), C.byref(st)) == BAD_CONFIG, what
    assert lib.isx_scene_response_device(cf, g, C.byref(r), 10, 1, 0, dev, dev) == BAD_CONFIG, what
    assert st.launched == 77
    # (a refused scene with a refused spec is refused all the same)
    assert lib.isx_scene_response(C.byref(bad[0][1]), C.byref(bad[0][2]), C.byref(r), 10, 1, 0, hp, None, None) == BAD_CONFIG, what
    w = np.ones(4096); f = np.zeros(21)
    assert lib.isx_response_reweight(C.byref(r), hp, w.ctypes.data_as(C.POINTER(C.c_double)), f.ctypes.data_as(C.POINTER(C.c_double)), None) == BAD_CONFIG, what
for r in rgood:
    assert lib.isx_scene_response(cf, g, C.byref(r), 10, 1, 0, hp, None, None) == past, list(r.n)
    assert lib.isx_scene_response_device(cf, g, C.byref(r), 10, 1, 0, dev, dev) == past, list(r.n)
for k in range(4):      # cfg, scene, rspec, response
    a = [cf, g, rs, hp]
    a[k] = None
    assert lib.isx_scene_response(a[0], a[1], a[2], 10, 1, 0, a[3], None, None) == BAD_ARG, k
for k in range(5):      # cfg, scene, rspec, d_response, d_counts
    a = [cf, g, rs, dev, dev]
    a[k] = None
    assert lib.isx_scene_response_device(a[0], a[1], a[2], 10, 1, 0, a[3], a[4]) == BAD_ARG, k
# the detector grid and the hit line are ignored: what isx_fluxmap_scene refuses for its grid gets past the checks here
grids, fits = big_grids(isx)
for what, c in grids:
    assert lib.isx_fluxmap_scene(C.byref(c), g, 10, 1, 0, hp, None, None) == BAD_CONFIG, what
    assert lib.isx_scene_response(C.byref(c), g, rs, 10, 1, 0, hp, None, None) == past, what
    assert lib.isx_scene_response_device(C.byref(c), g, rs, 10, 1, 0, dev, dev) == past, what
for nt, nph, mode in ((0, 0, 0), (-5, 7, 1), (1 << 20, 1 << 20, 1)):
    c = cfg.copy(); c.n_theta, c.n_phi, c.hit_line_mode = nt, nph, mode
    assert lib.isx_scene_response(C.byref(c), g, rs, 10, 1, 0, hp, None, None) == past, (nt, nph, mode)
assert (buf == 7).all() and not cnt.words().any()
try:
    isx.scene_response(cfg, good, rbad[0][1], 10, 1)
    print("no error")
except isx.IsxError as e:
    print("ok", e.status, len(bad), len(served), len(rbad), len(rgood), len(grids))
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["ok", "-2", "146", "22", "30", "8", "4"], r.stdout


def test_no_device_on_a_machine_without_one():
    """where the library can initialise no HIP device, a valid response call is ISX_ERR_NO_DEVICE (a process of its own)"""
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
rs = isx.default_response_spec(cfg)
for call in (lambda: isx.scene_response(cfg, spec, rs, 10, 1), lambda: isx.scene_response_device(cfg, spec, rs, 10, 1, 0, 4096, 8192)):
    try:
        call()
        raise SystemExit("no error")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_NO_DEVICE, e.status
print("no device")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() in (["device"], ["no", "device"]), r.stdout + r.stderr[-2000:]


# ---------------------------------------------------------------- isx_response_reweight
def reweight_np(resp, w):
    """isx.h's formulas, the sums in increasing b"""
    resp = np.asarray(resp, dtype=np.uint64)
    nb = resp.sum(axis=0).astype(np.float64)
    L = 0.0
    for b in range(w.size):
        L += w[b] * nb[b]
    frac, sig = np.zeros(R.FATES), np.zeros(R.FATES)
    for f in range(R.FATES):
        s = 0.0
        for b in range(w.size):
            s += w[b] * float(resp[f, b])
        F = s / L
        v = 0.0
        for b in range(w.size):
            h = float(resp[f, b])
            v += w[b] * w[b] * (h * (1.0 - F) * (1.0 - F) + (nb[b] - h) * F * F)
        frac[f], sig[f] = F, np.sqrt(v) / L
    return frac, sig


def test_reweight_against_the_formulas():
    import altair_raytracing_amd as isx
    rng = np.random.default_rng(7)
    for n in ((1, 1, 1, 1), (1, 1, 6, 12), (3, 5, 7, 11), (2, 3, 1, 4)):
        rs = isx.response_spec(*n)
        B = rs.bins
        resp = rng.integers(0, 5000, size=(R.FATES, B)).astype(np.uint64)
        resp[4:10] = 0; resp[14:18] = 0
        launched = int(resp.sum())
        # unit weights: the row sums over launched exactly as the division gives it, and the binomial error
        frac, sig = isx.response_reweight(rs, resp, np.ones(B))
        rows = resp.sum(axis=1)
        assert np.array_equal(frac, rows.astype(np.float64) / float(launched))
        binom = np.sqrt(frac * (1.0 - frac) / launched)
        assert np.allclose(sig, binom, rtol=1e-12, atol=0.0) and (sig[rows > 0] > 0).all() and not sig[rows == 0].any()
        assert abs(frac.sum() - 1.0) < 1e-14
        # any weights: the formulas, to the rounding of two sums taken in the same order
        for w in (rng.random(B) * 3.0, (np.arange(B) % 3 == 0).astype(np.float64), np.full(B, 1e-3)):
            frac, sig = isx.response_reweight(rs, resp, w)
            wf, ws = reweight_np(resp, w)
            assert np.allclose(frac, wf, rtol=1e-14, atol=0.0) and np.allclose(sig, ws, rtol=1e-13, atol=0.0)
            assert abs(frac.sum() - 1.0) < 1e-13
        # a scaled weight is the same lamp
        f1, s1 = isx.response_reweight(rs, resp, np.full(B, 4.0))
        f0, s0 = isx.response_reweight(rs, resp, np.ones(B))
        assert np.allclose(f1, f0, rtol=1e-15) and np.allclose(s1, s0, rtol=1e-14)
        # sigma may be NULL
        lib, fr = isx.load(), np.zeros(R.FATES)
        w = np.ones(B)
        assert lib.isx_response_reweight(C.byref(rs), resp.ctypes.data_as(C.POINTER(C.c_uint64)), w.ctypes.data_as(C.POINTER(C.c_double)),
                                         fr.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
        assert np.array_equal(fr, f0)


def test_reweight_refusals():
    import altair_raytracing_amd as isx
    lib = isx.load()
    rs = isx.response_spec(1, 1, 2, 3)
    resp = np.arange(R.FATES * 6, dtype=np.uint64)
    w, fr, sg = np.ones(6), np.zeros(R.FATES), np.zeros(R.FATES)
    pu, pd = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    args = [C.byref(rs), resp.ctypes.data_as(pu), w.ctypes.data_as(pd), fr.ctypes.data_as(pd)]
    assert lib.isx_response_reweight(*args, sg.ctypes.data_as(pd)) == 0
    for k in range(4):
        a = list(args); a[k] = None
        assert lib.isx_response_reweight(*a, None) == isx.abi.ERR_BAD_ARG, k
    for v in (-1.0, -1e-300, np.nan, np.inf, -np.inf):
        for at in (0, 5):
            bad = np.ones(6); bad[at] = v
            with pytest.raises(isx.IsxError) as e:
                isx.response_reweight(rs, resp, bad)
            assert e.value.status == isx.abi.ERR_BAD_ARG, (v, at)
    for what, zero_w, zero_resp in (("all weights 0", True, False), ("an empty response", False, True)):
        with pytest.raises(isx.IsxError) as e:
            isx.response_reweight(rs, np.zeros_like(resp) if zero_resp else resp, np.zeros(6) if zero_w else w)
        assert e.value.status == isx.abi.ERR_BAD_CONFIG, what
    # weights only where nothing was launched: L == 0
    hole = resp.reshape(R.FATES, 6).copy(); hole[:, 2] = 0
    with pytest.raises(isx.IsxError) as e:
        isx.response_reweight(rs, hole, np.array([0, 0, 1.0, 0, 0, 0]))
    assert e.value.status == isx.abi.ERR_BAD_CONFIG
    with pytest.raises(ValueError):
        isx.response_reweight(rs, resp[:10], w)


# ---------------------------------------------------------------- the restatement: response_np on the oracle
def test_numpy_philox_is_the_oracles(orc):
    """about 1000 counters, ray indices on both sides of 2^32 and of 2^63 among them, several seeds and streams"""
    rng = np.random.default_rng(3)
    ids = np.concatenate([np.arange(0, 40, dtype=np.uint64), np.uint64((1 << 32) - 20) + np.arange(40, dtype=np.uint64),
                          np.uint64((1 << 63) - 5) + np.arange(10, dtype=np.uint64), np.uint64((1 << 64) - 10) + np.arange(10, dtype=np.uint64),
                          rng.integers(0, 1 << 63, size=100, dtype=np.uint64)])
    checked = 0
    for seed in (0, 1, SEED, 777, (1 << 64) - 1, 0x5EED00010000F00D):
        for block, stream in ((0, 3), (0, 0), (7, 2), (0xFFFFFFFF, 3)):
            if (block, stream) != (0, 3) and seed not in (SEED, (1 << 64) - 1):
                continue
            got = R.philox4x32_10(ids & np.uint64(0xFFFFFFFF), ids >> np.uint64(32), block, stream, seed & 0xFFFFFFFF, seed >> 32)
            for k, rid in enumerate(ids.tolist()):
                want = orc.philox([rid & 0xFFFFFFFF, rid >> 32, block, stream], [seed & 0xFFFFFFFF, seed >> 32])
                assert [int(g[k]) for g in got] == want, (seed, block, stream, rid)
                checked += 1
    assert checked >= 1000
    w = R.start_words(SEED, (1 << 32) - 3, 6)
    for k in range(6):
        rid = (1 << 32) - 3 + k
        assert [int(x[k]) for x in w] == orc.philox([rid & 0xFFFFFFFF, rid >> 32, 0, 3], [SEED, 0])


def test_the_integer_bin_rule_is_not_floor_of_u01():
    """isx.h states the rule on the words: for an n that is no power of two floor(u01(w) n) differs at some words"""
    import altair_raytracing_amd as isx
    w = np.array([0x55555555, 0xAAAAAAAA, 0, 0xFFFFFFFF, 0x80000000], dtype=np.uint64)
    n = np.uint64(3)
    rule = (w * n) >> np.uint64(32)
    assert rule.tolist() == [0, 1, 0, 2, 1]
    u = (w.astype(np.float64) + 0.5) * 2.0 ** -32
    assert np.floor(u * 3.0).astype(np.int64).tolist() == [1, 1, 0, 2, 1]      # (0x55555555: 3 (w + 1/2) = 2^32 + 1/2)
    # bins() of every axis alone and of all four together, against the words
    rs = isx.response_spec(3, 5, 7, 11)
    ws = R.start_words(SEED, 100, 5000)
    i = [(x * np.uint64(m)) >> np.uint64(32) for x, m in zip(ws, (3, 5, 7, 11))]
    assert np.array_equal(R.bins(rs, SEED, 100, 5000), (((i[0] * 5 + i[1]) * 7 + i[2]) * 11 + i[3]).astype(np.int64))
    for a, m in enumerate((3, 5, 7, 11)):
        n4 = [1, 1, 1, 1]; n4[a] = m
        assert np.array_equal(R.bins(isx.response_spec(*n4), SEED, 100, 5000), i[a].astype(np.int64))
        assert np.bincount(i[a].astype(np.int64), minlength=m).min() > 5000 / m * 0.8


N_Z = 200_000


def _ocfg(orc, rho=RHO):
    c = orc.default_config()
    c.reflectance = rho
    return c


@pytest.fixture(scope="module")
def photometer_walk(orc):
    """`photometer` at 2e5 rays, seed 12345: computed once, shared, never changed"""
    import altair_raytracing_amd as isx
    sc = SC.spec_of(scene(isx, isx.default_config(), "photometer"))
    return sc, orc.scene_walk(_ocfg(orc), sc, N_Z, SEED, 0, nthreads=16)


def test_from_walk_identities(orc, photometer_walk):
    """the rows are the walk's totals (asserted inside from_walk), the columns the launches per bin, for three specs"""
    import altair_raytracing_amd as isx
    _, w = photometer_walk
    cfg = _ocfg(orc)
    for n in ((1, 1, 6, 12), (3, 5, 7, 11), (1, 1, 1, 1)):
        rs = isx.response_spec(*n)
        resp = R.from_walk(w, cfg, rs, SEED, 0)
        assert resp.shape == (21, rs.bins) and resp.dtype == np.uint64
        cols = resp.sum(axis=0)
        assert np.array_equal(cols, np.bincount(R.bins(rs, SEED, 0, N_Z), minlength=rs.bins).astype(np.uint64))
        expect = N_Z / rs.bins
        assert abs(cols.astype(np.float64) - expect).max() < 6.0 * np.sqrt(expect)      # (every bin: the same expected launches)
    one = R.from_walk(w, cfg, isx.response_spec(1, 1, 1, 1), SEED, 0)[:, 0]
    print("fates of photometer at 2e5 rays:", one.tolist())
    assert one[:4].min() > 0 and one[10:14].min() > 0 and one[18] > 0 and not one[4:10].any() and not one[14:18].any()
    # a part of the range: the same rays
    part = orc.scene_walk(cfg, photometer_walk[0], 300, SEED, 1000, nthreads=2)
    rs = isx.response_spec(1, 1, 6, 12)
    want = np.bincount(R.fates(w, cfg)[1000:1300] * 72 + R.bins(rs, SEED, 0, N_Z)[1000:1300], minlength=21 * 72).reshape(21, 72)
    assert np.array_equal(R.from_walk(part, cfg, rs, SEED, 1000), want.astype(np.uint64))


def test_reweighted_polar_band_is_the_cone_lamp(orc, photometer_walk):
    """The response of the isotropic lamp in 4 polar bands, reweighted to band 0 alone (ct > 0.5: a cone of 60 degrees), against
    a direct walk of that cone lamp with another seed: two independent estimates of the same fractions.  z per slot with at least
    500 rays in the direct walk, from the reweighting's sigma and the direct walk's binomial error; |z| <= 4.
    Found at 2e5 rays: see the printed values (docs/LOG.md section 21)."""
    import altair_raytracing_amd as isx
    sc, w = photometer_walk
    cfg = _ocfg(orc)
    rs = isx.response_spec(1, 1, 4, 1)
    resp = R.from_walk(w, cfg, rs, SEED, 0)
    frac, sig = isx.response_reweight(rs, resp, np.array([1.0, 0.0, 0.0, 0.0]))
    cone = dict(sc, beam=dict(sc["beam"], cos_min=0.5))
    d = orc.scene_walk(cfg, cone, N_Z, 777, 0, nthreads=16)
    assert float(d["start_dir"][:, 2].min()) >= 0.5 and float(w["start_dir"][:, 2].min()) < -0.99      # (the lamp's axis is +z)
    direct = R.from_walk(d, cfg, isx.response_spec(1, 1, 1, 1), 777, 0)[:, 0].astype(np.float64)
    fd = direct / N_Z
    sd = np.sqrt(fd * (1.0 - fd) / N_Z)
    slots = [f for f in range(R.FATES) if direct[f] >= 500]
    z = {f: float((frac[f] - fd[f]) / np.sqrt(sig[f] ** 2 + sd[f] ** 2)) for f in slots}
    print("slots", slots, "reweighted", [round(float(frac[f]), 5) for f in slots], "direct", [round(float(fd[f]), 5) for f in slots],
          "z", {f: round(v, 2) for f, v in z.items()})
    assert len(slots) >= 6 and 0 in slots and 18 in slots
    assert max(abs(v) for v in z.values()) <= 4.0, z
    # the launches of band 0 are a quarter of the whole, and the reweighted fractions are band 0's own
    n0 = int(resp[:, 0].sum())
    assert abs(n0 - N_Z / 4) < 6 * np.sqrt(N_Z * 0.25 * 0.75)
    assert np.array_equal(frac, resp[:, 0].astype(np.float64) / float(n0))


# ---------------------------------------------------------------- the sharded call
def walk_trace(isx, orc):
    """a stand-in tracer for scene_response_sharded: the oracle's walk and the restatement"""
    def trace(c, sp, rs, count, seed, first):
        w = orc.scene_walk(c, SC.spec_of(sp), count, seed, first, nthreads=2)
        st = orc.Stats()
        for f, val in w["census"].items():
            setattr(st, f, val)
        st.bin_increments = count
        cnt = isx.SceneCounts()
        C.memmove(C.byref(cnt), SC.counter_words(w).tobytes(), C.sizeof(cnt))
        return R.from_walk(w, c, rs, seed, first), cnt, st
    return trace


N_SHARDED, FIRST_SHARDED = 3001, 1000


def test_sharded_with_one_rank_is_the_plain_call(orc):
    import altair_raytracing_amd as isx
    cfg = _ocfg(orc)
    spec = scene(isx, isx.default_config(), "photometer")
    rs = isx.response_spec(2, 1, 3, 4)
    seen = []
    inner = walk_trace(isx, orc)

    def trace(c, sp, r, count, seed, first):
        seen.append((count, seed, first, sp is spec, r is rs))
        return inner(c, sp, r, count, seed, first)

    resp, pa, pb, ba, bb, census = isx.scene_response_sharded(trace, cfg, spec, rs, N_SHARDED, SEED, first_ray=FIRST_SHARDED)
    assert seen == [(N_SHARDED, SEED, FIRST_SHARDED, True, True)]
    assert resp.shape == (21, 24) and resp.dtype == np.uint64 and int(resp.sum()) == N_SHARDED == census["launched"] == census["bin_increments"]
    rows = resp.sum(axis=1)
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
    out = isx.scene_response_sharded(walk_trace(isx, oracle), cfg, spec, isx.response_spec(2, 1, 3, 4), N_SHARDED, SEED,
                                     first_ray=FIRST_SHARDED)
    q.put((rank,) + out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_allreduce_equals_single_rank(orc):
    """two ranks over gloo: the response, the 36 counters and the census of every rank are those of the job in one piece"""
    import socket
    import altair_raytracing_amd as isx
    import torch.multiprocessing as mp

    cfg = _ocfg(orc)
    spec = scene(isx, isx.default_config(), "photometer")
    whole = isx.scene_response_sharded(walk_trace(isx, orc), cfg, spec, isx.response_spec(2, 1, 3, 4), N_SHARDED, SEED,
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
    assert whole[5]["launched"] == N_SHARDED and int(whole[0].sum()) == N_SHARDED
    for out in got:
        rank, parts_ = out[0], out[1:]
        for a, w in zip(parts_[:5], whole[:5]):
            assert a.dtype == np.uint64 and a.shape == w.shape and np.array_equal(a, w), rank
        assert parts_[5] == whole[5], rank
