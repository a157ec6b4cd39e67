"""The beam source (isx_fluxmap_beam, isx_beam_endstates) without a GPU: the refusals of isx.h, isx_beam_cone, the replay on the
oracle (beam_np) against the oracle's own pencil trace for the degenerate beam, and the sampling law."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import beam_np as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11


def side_beam(isx, cfg):
    return isx.beam_cone(cfg, (-60, 0, -75), (1, 0, 0), 10.0, 20.0, isx.BEAM_UNIFORM)


def refused_calls(isx):
    """(cfg, a good spec, [(what, cfg, spec)] that isx.h refuses with ISX_ERR_BAD_CONFIG, [(cfg, spec)] that get past the checks)"""
    cfg = isx.default_config()
    good = side_beam(isx, cfg)
    bad = []
    for what, field, v in (("BRDF source", "source_model", 1), ("lobe border", "surface_model", 1), ("rough-specular border", "lambertian", 0),
                           ("chord mode", "trace_mode", 1)):
        c = cfg.copy(); setattr(c, field, v)
        bad.append((what, c, good))
    c = cfg.copy(); c.struct_size += 8
    bad.append(("config struct_size", c, good))
    for size in (0, C.sizeof(isx.BeamSpec) - 8, C.sizeof(isx.BeamSpec) + 8):
        s = good.copy(); s.struct_size = size
        bad.append(("struct_size %d" % size, cfg, s))
    for field in ("origin", "axis", "e1", "e2"):
        for i, v in ((0, np.nan), (1, np.inf), (2, -np.inf)):
            s = good.copy(); getattr(s, field)[i] = v
            bad.append(("%s[%d] %r" % (field, i, v), cfg, s))
    for field in ("radius", "cos_min"):
        for v in (np.nan, np.inf, -np.inf):
            s = good.copy(); setattr(s, field, v)
            bad.append(("%s %r" % (field, v), cfg, s))
    s = good.copy(); s.radius = -1e-9
    bad.append(("radius < 0", cfg, s))
    for v in (-1.0 - 1e-9, 1.0 + 1e-9, 2.0):
        s = good.copy(); s.cos_min = v
        bad.append(("cos_min %r" % v, cfg, s))
    for v in (-1e-9, -1.0, 1.0 + 1e-9):
        s = good.copy(); s.angular_law = isx.BEAM_LAMBERT; s.cos_min = v
        bad.append(("lambert cos_min %r" % v, cfg, s))
    for v in (-1, 2, 1 << 20):
        s = good.copy(); s.angular_law = v
        bad.append(("law %d" % v, cfg, s))
    # not orthonormal: a length, then each mutual dot product
    for field in ("axis", "e1", "e2"):
        s = good.copy()
        for i in range(3):
            getattr(s, field)[i] *= 1.0 + 1e-9
        bad.append(("|%s| off by 1e-9" % field, cfg, s))
    s = good.copy(); s.axis[:] = [1.0, 0.0, 0.0]; s.e1[:] = [1e-9, 1.0, 0.0]; s.e2[:] = [0.0, 0.0, 1.0]
    bad.append(("axis . e1", cfg, s))
    s = good.copy(); s.axis[:] = [1.0, 0.0, 0.0]; s.e1[:] = [0.0, 1.0, 0.0]; s.e2[:] = [0.0, 1e-9, 1.0]
    bad.append(("e1 . e2", cfg, s))
    s = good.copy(); s.axis[:] = [1.0, 0.0, 0.0]; s.e1[:] = [0.0, 1.0, 0.0]; s.e2[:] = [1e-9, 0.0, 1.0]
    bad.append(("e2 . axis", cfg, s))
    # the disc's centre must lie strictly inside the inner sphere, every start point strictly inside the world box
    s = good.copy(); s.origin[:] = [cfg.r_in, 0.0, 0.0]; s.radius = 0.0
    bad.append(("origin on the wall", cfg, s))
    s = good.copy(); s.origin[:] = [0.0, 0.0, 100.5]
    bad.append(("origin inside the wall shell", cfg, s))
    s = good.copy(); s.origin[:] = [0.0, -200.0, 0.0]
    bad.append(("origin outside the sphere", cfg, s))
    s = good.copy(); s.origin[:] = [0.0, 0.0, 95.0]; s.radius = 205.0
    bad.append(("|origin| + radius = box_half", cfg, s))
    served = [(cfg, good), (cfg, isx.default_beam_spec(cfg))]
    s = good.copy(); s.origin[:] = [0.0, 0.0, 100.0]; s.radius = 199.9    # centre inside r_in = 100.1, 299.9 < box_half = 300
    served.append((cfg, s))
    s = isx.beam_cone(cfg, (0, 0, 0), (0, 0, 1), 0.0, 180.0)              # the lamp
    served.append((cfg, s))
    s = isx.beam_cone(cfg, (0, 0, -90), (0, 0, -1), 8.0, 90.0, isx.BEAM_LAMBERT)
    served.append((cfg, s))
    s = good.copy(); s.e1[0] += 5e-13                                     # (within 1e-12)
    served.append((cfg, s))
    c = cfg.copy(); c.hit_line_mode = 1
    served.append((c, good))
    return cfg, good, bad, served


def test_refusals_and_null_arguments_need_no_device():
    """Every refusal of isx.h is ISX_ERR_BAD_CONFIG and a NULL pointer ISX_ERR_BAD_ARG from the three compute entry points, before
    anything asks for a device (this process never keeps isx_init); specs at the limits get past the checks."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ctypes as C
import numpy as np
import altair_raytracing_amd as isx
from test_beam_cpu import refused_calls
lib = isx.load()
have = lib.isx_init(0) == 0
if have:
    lib.isx_shutdown()
past = isx.abi.ERR_NOT_INIT if have else isx.abi.ERR_NO_DEVICE
buf = np.zeros(180 * 90, dtype=np.uint64)
hp = buf.ctypes.data_as(C.POINTER(C.c_uint64))
ibuf = np.zeros(16, dtype=np.int32)
ip = ibuf.ctypes.data_as(C.POINTER(C.c_int32))
dbuf = np.zeros(48, dtype=np.float64)
dp = dbuf.ctypes.data_as(C.POINTER(C.c_double))
cfg, good, bad, served = refused_calls(isx)
dev = C.c_void_p(4096)
BAD_CONFIG, BAD_ARG = isx.abi.ERR_BAD_CONFIG, isx.abi.ERR_BAD_ARG
for what, c, s in bad:
    assert lib.isx_fluxmap_beam(C.byref(c), C.byref(s), 10, 1, 0, hp, None) == BAD_CONFIG, what
    assert lib.isx_fluxmap_beam_device(C.byref(c), C.byref(s), 10, 1, 0, dev) == BAD_CONFIG, what
    assert lib.isx_beam_endstates(C.byref(c), C.byref(s), 10, 1, 0, ip, ip, dp, dp, dp, dp) == BAD_CONFIG, what
for k, (c, s) in enumerate(served):
    assert lib.isx_fluxmap_beam(C.byref(c), C.byref(s), 10, 1, 0, hp, None) == past, k
    assert lib.isx_fluxmap_beam_device(C.byref(c), C.byref(s), 10, 1, 0, dev) == past, k
    assert lib.isx_beam_endstates(C.byref(c), C.byref(s), 10, 1, 0, ip, ip, dp, dp, None, None) == past, k
g, cf = C.byref(good), C.byref(cfg)
assert lib.isx_fluxmap_beam(None, g, 10, 1, 0, hp, None) == BAD_ARG
assert lib.isx_fluxmap_beam(cf, None, 10, 1, 0, hp, None) == BAD_ARG
assert lib.isx_fluxmap_beam(cf, g, 10, 1, 0, None, None) == BAD_ARG
assert lib.isx_fluxmap_beam_device(None, g, 10, 1, 0, dev) == BAD_ARG
assert lib.isx_fluxmap_beam_device(cf, None, 10, 1, 0, dev) == BAD_ARG
assert lib.isx_fluxmap_beam_device(cf, g, 10, 1, 0, None) == BAD_ARG
assert lib.isx_beam_endstates(None, g, 10, 1, 0, ip, ip, dp, dp, dp, dp) == BAD_ARG
assert lib.isx_beam_endstates(cf, None, 10, 1, 0, ip, ip, dp, dp, dp, dp) == BAD_ARG
assert lib.isx_beam_endstates(cf, g, 10, 1, 0, None, ip, dp, dp, dp, dp) == BAD_ARG
assert lib.isx_beam_endstates(cf, g, 10, 1, 0, ip, None, dp, dp, dp, dp) == BAD_ARG
assert lib.isx_beam_endstates(cf, g, 10, 1, 0, ip, ip, None, dp, dp, dp) == BAD_ARG
assert lib.isx_beam_endstates(cf, g, 10, 1, 0, ip, ip, dp, None, dp, dp) == BAD_ARG
lib.isx_default_beam_spec(cf, None)      # (a NULL spec is left alone)
try:
    isx.fluxmap_beam(bad[0][1], bad[0][2], 10, 1)
    print("no error")
except isx.IsxError as e:
    print("ok", e.status, len(bad), len(served))
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["ok", "-2", "46", "7"], r.stdout


def test_no_device_on_a_machine_without_one():
    """where the library can initialise no HIP device, a valid compute call is ISX_ERR_NO_DEVICE (a process of its own: whether
    there is a device is the library's own answer, and this process may hold an initialised one)"""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import altair_raytracing_amd as isx
from test_beam_cpu import side_beam
lib = isx.load()
if lib.isx_init(0) == 0:
    lib.isx_shutdown()
    print("device")      # (test_refusals_and_null_arguments_need_no_device covers the machine with a device)
    raise SystemExit(0)
cfg = isx.default_config()
spec = side_beam(isx, cfg)
for call in (lambda: isx.fluxmap_beam(cfg, spec, 10, 1), lambda: isx.beam_endstates(cfg, spec, 10, 1),
             lambda: isx.fluxmap_beam_device(cfg, spec, 10, 1, 0, 4096)):
    try:
        call()
        raise SystemExit("no error")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_NO_DEVICE, e.status
print("no device")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() in (["device"], ["no", "device"]), r.stdout + r.stderr[-2000:]


def test_binding_struct_and_default_spec():
    import altair_raytracing_amd as isx
    assert C.sizeof(isx.BeamSpec) == 8 + 14 * 8 + 8
    cfg = isx.default_config()
    s = isx.default_beam_spec(cfg)
    assert s.struct_size == C.sizeof(isx.BeamSpec) and s.reserved0 == 0 and s.reserved1 == 0
    assert list(s.origin) == [cfg.src[0], cfg.src[1], cfg.src[2]] == [-60.0, 0.0, -75.0]
    assert list(s.axis) == [1.0, 0.0, 0.0] and s.radius == 0.0 and s.cos_min == 1.0 and s.angular_law == isx.BEAM_UNIFORM
    assert list(s.e1) == [0.0, 1.0, 0.0] and list(s.e2) == [0.0, 0.0, 1.0]     # (the header's frame rule)


@pytest.mark.parametrize("direction", [(1, 0, 0), (0, 0, -1), (0, -3, 0), (1, 1, 1), (3, -4, 12), (-1e-3, 2.5, -7), (66.3, 0, -75),
                                       (1e-100, 1e-100, 1e-80), (-5, 5, 5e-9), (0.3, 0.3, 0.3000001)])
def test_beam_cone_frame(direction):
    """axis = dir / |dir| bit for bit (the same IEEE operations in numpy); the frame is orthonormal to 1e-15 and right-handed"""
    import altair_raytracing_amd as isx
    cfg = isx.default_config()
    s = isx.beam_cone(cfg, (1, 2, 3), direction, 4.0, 33.0, isx.BEAM_UNIFORM)
    d = np.array(direction, dtype=np.float64)
    mag = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    a, e1, e2 = np.array(s.axis[:]), np.array(s.e1[:]), np.array(s.e2[:])
    assert list(a) == list(d / mag)
    for x in (a, e1, e2):
        assert abs(np.sqrt(x @ x) - 1.0) <= 1e-15
    for x, y in ((a, e1), (e1, e2), (e2, a)):
        assert abs(x @ y) <= 1e-15
    assert np.abs(np.cross(e1, e2) - a).max() <= 2e-15
    assert np.linalg.det(np.stack([e1, e2, a])) > 0.999
    assert list(s.origin) == [1.0, 2.0, 3.0] and s.radius == 4.0 and s.angular_law == isx.BEAM_UNIFORM
    assert s.struct_size == C.sizeof(isx.BeamSpec)


def test_beam_cone_cos_min_and_refusals():
    import altair_raytracing_amd as isx
    lib = isx.load()
    cfg = isx.default_config()
    for deg, want in ((0.0, 1.0), (90.0, 0.0), (180.0, -1.0)):
        assert isx.beam_cone(cfg, (0, 0, 0), (0, 0, 1), 0.0, deg).cos_min == want
    assert isx.beam_cone(cfg, (0, 0, 0), (0, 0, 1), 0.0, 90.0, isx.BEAM_LAMBERT).cos_min == 0.0
    # elsewhere cos(deg * pi / 180): the library's libm and numpy's are each within an ulp of the true cosine
    for deg in (20.0, 30.0, 60.0, 123.4):
        assert abs(isx.beam_cone(cfg, (0, 0, 0), (0, 0, 1), 0.0, deg).cos_min - np.cos(np.float64(deg) * np.pi / 180.0)) <= 2.0 ** -51
    out = isx.BeamSpec()
    o, d = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(0, 0, 1)
    BAD_ARG, BAD_CONFIG = isx.abi.ERR_BAD_ARG, isx.abi.ERR_BAD_CONFIG
    assert lib.isx_beam_cone(None, o, d, 1.0, 10.0, 0, C.byref(out)) == BAD_ARG
    assert lib.isx_beam_cone(C.byref(cfg), None, d, 1.0, 10.0, 0, C.byref(out)) == BAD_ARG
    assert lib.isx_beam_cone(C.byref(cfg), o, None, 1.0, 10.0, 0, C.byref(out)) == BAD_ARG
    assert lib.isx_beam_cone(C.byref(cfg), o, d, 1.0, 10.0, 0, None) == BAD_ARG
    for oo, dd, radius, half, law in (((0, 0, 0), (0, 0, 0), 1, 10, 0), ((0, 0, 0), (np.nan, 0, 1), 1, 10, 0), ((0, 0, 0), (np.inf, 0, 1), 1, 10, 0),
                                      ((np.nan, 0, 0), (0, 0, 1), 1, 10, 0), ((0, np.inf, 0), (0, 0, 1), 1, 10, 0),
                                      ((0, 0, 0), (0, 0, 1), -1e-9, 10, 0), ((0, 0, 0), (0, 0, 1), np.nan, 10, 0), ((0, 0, 0), (0, 0, 1), np.inf, 10, 0),
                                      ((0, 0, 0), (0, 0, 1), 1, -1, 0), ((0, 0, 0), (0, 0, 1), 1, 180.5, 0), ((0, 0, 0), (0, 0, 1), 1, np.nan, 0),
                                      ((0, 0, 0), (0, 0, 1), 1, 90.5, 1), ((0, 0, 0), (0, 0, 1), 1, 10, 2), ((0, 0, 0), (0, 0, 1), 1, 10, -1)):
        with pytest.raises(isx.IsxError) as e:
            isx.beam_cone(cfg, oo, dd, radius, half, law)
        assert e.value.status == BAD_CONFIG, (oo, dd, radius, half, law)
    c2 = cfg.copy(); c2.struct_size += 8
    assert lib.isx_beam_cone(C.byref(c2), o, d, 1.0, 10.0, 0, C.byref(out)) == BAD_CONFIG


def test_degenerate_beam_replays_the_oracles_pencil(orc):
    """radius 0, cos_min 1 about the default (5, 0, 0): mag == 1.0 and v == axis, so the replay from the sampled start is
    oracle.trace_endstates bit for bit, and its census oracle.fluxmap's"""
    import altair_raytracing_amd as isx
    cfg = orc.default_config()
    spec = B.spec_of(isx.default_beam_spec(isx.default_config()))
    n = 300
    sp, sv, status, npts, lp, d, kind0, census = B.replay(cfg, spec, n, SEED, workers=1)
    assert np.array_equal(sp, np.tile([-60.0, 0.0, -75.0], (n, 1))) and np.array_equal(sv, np.tile([1.0, 0.0, 0.0], (n, 1)))
    st, np_, olp, od = orc.trace_endstates(cfg, n, SEED, 0)
    assert np.array_equal(status, st) and np.array_equal(npts, np_) and np.array_equal(lp, olp)
    ex = st == 1
    assert ex.sum() > 10 and np.array_equal(d[ex], od[ex])
    assert (kind0 == B.K_INNER).all()
    _, ost = orc.fluxmap(cfg, n, SEED)
    for f in B.CENSUS_FIELDS:
        assert census[f] == getattr(ost, f), f
    # ... and the workers cut the range without changing a ray
    part = B.replay(cfg, spec, 40, SEED, first=100, workers=1)
    assert np.array_equal(part[2], status[100:140]) and np.array_equal(part[4], lp[100:140])


N_LAW = 100000


@pytest.fixture(scope="module")
def law_uniforms(orc):
    """the words of 1e5 rays, drawn once for both laws"""
    return B.uniforms(N_LAW, SEED, 5)


def _sample_with(monkeypatch, spec, uni):
    monkeypatch.setattr(B, "uniforms", lambda n, seed, first=0: uni)
    return B.sample(spec, N_LAW, SEED, 5)


@pytest.mark.parametrize("law,half", [(B.UNIFORM, 20.0), (B.UNIFORM, 130.0), (B.LAMBERT, 90.0), (B.LAMBERT, 35.0)])
def test_sampling_law(orc, law_uniforms, monkeypatch, law, half):
    """r^2 / radius^2, the polar variable of the law (cos theta on [cos_min, 1]; sin^2 theta on [0, 1 - cos_min^2]) and both
    azimuths are uniform: chi2 over 20 bins, p > 1e-4 each; the direction is a unit vector to 4e-16"""
    import altair_raytracing_amd as isx
    cfg = isx.default_config()
    bs = isx.beam_cone(cfg, (-20, 10, -40), (3, -4, 12), 7.5, half, law)
    spec = B.spec_of(bs)
    p, v = _sample_with(monkeypatch, spec, law_uniforms)
    o, a, e1, e2 = (np.array(spec[k]) for k in ("origin", "axis", "e1", "e2"))
    assert np.abs(np.sqrt((v * v).sum(axis=1)) - 1.0).max() <= 4e-16
    dp = p - o
    assert np.abs(dp @ a).max() < 1e-12                      # the start points lie in the disc's plane
    r2 = (dp * dp).sum(axis=1) / spec["radius"] ** 2
    assert r2.max() <= 1.0 + 1e-12
    ps = {"r2": B.uniform_chi2_p(np.minimum(r2, 1.0))}
    ps["disc azimuth"] = B.uniform_chi2_p(np.mod(np.arctan2(dp @ e2, dp @ e1) / (2 * np.pi), 1.0))
    ct = v @ a
    cm = spec["cos_min"]
    assert ct.min() >= cm - 1e-12
    if law == B.UNIFORM:
        ps["cos theta"] = B.uniform_chi2_p(np.clip((1.0 - ct) / (1.0 - cm), 0.0, 1.0))
    else:
        ps["sin2 theta"] = B.uniform_chi2_p(np.clip((1.0 - ct * ct) / (1.0 - cm * cm), 0.0, 1.0))
    ps["cone azimuth"] = B.uniform_chi2_p(np.mod(np.arctan2(v @ e2, v @ e1) / (2 * np.pi), 1.0))
    for k, pv in ps.items():
        assert pv > 1e-4, (k, pv, ps)


def test_chi2_sf_against_known_quantiles():
    """A self-check of the test helper beam_np.chi2_sf, not of the feature (it passes without the beam source): the 19-dof
    quantiles of the chi2 law (tables), P(X >= 30.1435) = 0.05, P(X >= 43.8202) = 0.001"""
    assert abs(B.chi2_sf(30.1435, 19) - 0.05) < 1e-5 and abs(B.chi2_sf(43.8202, 19) - 0.001) < 1e-6
    assert B.chi2_sf(0.0, 19) == 1.0 and B.chi2_sf(400.0, 19) < 1e-50 + 1e-12
    assert B.uniform_chi2_p(np.linspace(0, 1, 2000, endpoint=False)) > 0.999
    assert B.uniform_chi2_p(np.linspace(0, 1, 2000, endpoint=False) ** 2) < 1e-4


def test_sharded_with_one_rank_is_the_plain_call(orc):
    """fluxmap_beam_sharded without a process group hands the whole range to the tracer and returns its histogram and census"""
    import altair_raytracing_amd as isx
    cfg = orc.default_config()
    bs = side_beam(isx, isx.default_config())
    seen = []

    def trace(c, spec, count, seed, first):
        seen.append((count, seed, first, spec is bs))
        rep = B.replay(c, B.spec_of(spec), count, seed, first, workers=1)
        P, V = B.counted_lines(c, rep)
        st = orc.Stats()
        for f, val in rep[7].items():
            setattr(st, f, val)
        return orc.bin_lines(c, P, V), st

    hits, census = isx.fluxmap_beam_sharded(trace, cfg, bs, 200, SEED, first_ray=1000)
    assert seen == [(200, SEED, 1000, True)]
    assert hits.shape == (cfg.n_theta, cfg.n_phi) and census["launched"] == 200
    assert census["exited"] + census["absorbed"] + census["suspended"] == 200
