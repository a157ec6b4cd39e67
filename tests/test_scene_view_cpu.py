"""The scene view (isx_scene_view, isx_view_frame, isx_view_reweight, isx_view_weight_fov) without a GPU: the bindings and the
frame helper, every refusal, the two host-side helpers against their formulas written out in Python, the restatement of the
contract on the oracle's walk (view_np) against an independent per-ray loop and on hand-made rays that fix the sign convention
and every branch, and the sharded call."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import scene_np as SC
import view_np as V
from test_scene_cpu import parts, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
RHO = 0.95


def wide_cap(isx, cfg):
    """the lamp and `screen` with a wide cap -- 60 degrees about +y, reflectance 0.5 -- as patch 0 and `det` as patch 1: most rays
    end on patch 0, many of them from behind the plane of its frame"""
    p = parts(isx, cfg)
    return isx.scene_spec(cfg, p["lamp"], [p["screen"]], [isx.wall_patch_cap(cfg, (0, 1, 0), 60.0, 0.5), p["det"]])


# ---------------------------------------------------------------- bindings, the frame
def test_binding_structs_and_view_frame():
    import altair_raytracing_amd as isx
    S = isx.ViewSpec
    assert C.sizeof(S) == 104 and C.sizeof(isx.ViewCounts) == 32
    assert (S.struct_size.offset, S.reserved0.offset, S.patch.offset, S.n_u.offset, S.n_v.offset, S.reserved1.offset) == (0, 4, 8, 12, 16, 20)
    assert (S.axis.offset, S.e1.offset, S.e2.offset, S.half_extent.offset) == (24, 48, 72, 96)
    assert [f[0] for f in isx.ViewCounts._fields_] == ["binned", "outside", "behind", "direct"]
    assert isx.abi.VIEW_MAX_AXIS == 1024 and isx.abi.VIEW_MAX_BINS == 65536
    for name in ("isx_view_frame", "isx_scene_view", "isx_scene_view_device", "isx_view_reweight", "isx_view_weight_fov"):
        assert name in isx.EXPORTS and hasattr(isx.load(), name)
    for name in ("ViewSpec", "ViewCounts", "view_frame", "scene_view", "scene_view_device", "view_reweight", "view_weight_fov",
                 "scene_view_sharded"):
        assert name in isx.__all__ and hasattr(isx, name)
    cfg = isx.default_config()
    ph = scene(isx, cfg, "photometer")
    v = isx.view_frame(cfg, ph, 0, 32, 32)
    assert v.struct_size == 104 and v.reserved0 == 0 and v.reserved1 == 0 and (v.patch, v.n_u, v.n_v, v.half_extent) == (0, 32, 32, 1.0)
    assert list(v.axis) == [1.0, 0.0, 0.0] and list(v.e1) == [0.0, 1.0, 0.0] and list(v.e2) == [0.0, 0.0, 1.0]
    v = isx.view_frame(cfg, ph, 1, 7, 13, 0.5)
    assert (v.patch, v.n_u, v.n_v, v.half_extent, v.bins) == (1, 7, 13, 0.5, 91)
    # the patch's axis bit for bit, the frame of beam_cone about it, right-handed and orthonormal to rounding: 8 oblique caps
    caps = [isx.wall_patch_cap(cfg, (k - 3.5, 1 - 0.3 * k, 2.0 - k), 10.0 + k, k / 7.0) for k in range(8)]
    sc = isx.scene_spec(cfg, parts(isx, cfg)["lamp"], [], caps)
    for k in range(8):
        v = isx.view_frame(cfg, sc, k, 4, 5, 0.25)
        ax = sc.patches.patch[k].axis
        assert bytes(v.axis) == bytes(ax)
        beam = isx.beam_cone(cfg, (0, 0, 0), tuple(ax), 0.0, 10.0, isx.BEAM_UNIFORM)
        assert bytes(v.e1) == bytes(beam.e1) and bytes(v.e2) == bytes(beam.e2)
        a, e1, e2 = (np.array(list(x)) for x in (v.axis, v.e1, v.e2))
        for x, y in ((a, e1), (e1, e2), (e2, a)):
            assert abs(np.linalg.norm(x) - 1.0) < 1e-14 and abs(x @ y) < 1e-14
        assert np.abs(np.cross(a, e1) - e2).max() < 1e-14
    # refusals of the helper itself
    lib = isx.load()
    out = isx.ViewSpec()
    for k in range(3):
        a = [C.byref(cfg), C.byref(ph), C.byref(out)]
        a[k] = None
        assert lib.isx_view_frame(a[0], a[1], 0, 4, 4, 1.0, a[2]) == isx.abi.ERR_BAD_ARG
    for args in ((2, 4, 4, 1.0), (-1, 4, 4, 1.0), (0, 0, 4, 1.0), (0, 4, 1025, 1.0), (0, 257, 256, 1.0), (0, 4, 4, 0.0), (0, 4, 4, 1.5),
                 (0, 4, 4, float("nan")), (0, 4, 4, -0.5), (0, 4, 4, float("inf"))):
        with pytest.raises(isx.IsxError) as e:
            isx.view_frame(cfg, ph, *args)
        assert e.value.status == isx.abi.ERR_BAD_CONFIG, args
    with pytest.raises(isx.IsxError) as e:
        isx.view_frame(cfg, isx.default_scene_spec(cfg), 0, 4, 4)      # (a scene without patches)
    assert e.value.status == isx.abi.ERR_BAD_CONFIG
    assert not bytes(out).strip(b"\0")      # (a refused call writes nothing)


def view_specs(isx):
    """([(what, ViewSpec)] that isx.h refuses with ISX_ERR_BAD_CONFIG whatever the scene, [ViewSpec] that get past the checks for
    a scene with at least two patches)"""
    cfg = isx.default_config()
    ph = scene(isx, cfg, "photometer")
    base = isx.view_frame(cfg, ph, 0, 32, 32)

    def made(**kw):
        s = base.copy()
        for k, val in kw.items():
            if isinstance(val, tuple):
                name, i = k.split("_at_")
                getattr(s, name)[int(i)] = val[0]
            else:
                setattr(s, k, val)
        return s

    bad = [("struct_size %d" % n, made(struct_size=n)) for n in (0, 96, 112, 24)]
    bad += [("reserved0", made(reserved0=1)), ("reserved1", made(reserved1=-1)), ("reserved1 = 7", made(reserved1=7))]
    bad += [("patch %d" % k, made(patch=k)) for k in (-1, 2, 8, 1 << 30, -(1 << 31))]
    for ax in ("n_u", "n_v"):
        bad += [("%s = %d" % (ax, n), made(**{ax: n})) for n in (0, -1, 1025, 1 << 30, -(1 << 31))]
    bad += [("bins %d x %d" % n, made(n_u=n[0], n_v=n[1])) for n in ((257, 256), (1024, 65), (1024, 1024), (65, 1024))]
    bad += [("half_extent %r" % h, made(half_extent=h)) for h in (0.0, -0.0, -0.5, 1.0000000000000002, 2.0, float("nan"), float("inf"),
                                                                  -float("inf"))]
    for name in ("axis", "e1", "e2"):
        for i in range(3):
            for val in (float("nan"), float("inf"), -float("inf")):
                bad.append(("%s[%d] = %r" % (name, i, val), made(**{"%s_at_%d" % (name, i): (val,)})))
    # not orthonormal: a length off by 1e-11, a pair 1e-11 from a right angle, two axes the same, a zero vector
    bad.append(("|axis| = 1 + 1e-11", made(axis_at_0=(1.0 + 1e-11,))))
    bad.append(("|e1| = 1 - 1e-11", made(e1_at_1=(1.0 - 1e-11,))))
    bad.append(("|e2| = 2", made(e2_at_2=(2.0,))))
    bad.append(("axis . e1 = 1e-11", made(axis_at_1=(1e-11,))))
    bad.append(("e1 . e2 = 1e-11", made(e1_at_2=(1e-11,))))
    bad.append(("e2 . axis = 1e-11", made(e2_at_0=(1e-11,))))
    s = base.copy(); s.e2[1], s.e2[2] = 1.0, 0.0
    bad.append(("e2 == e1", s))
    s = base.copy(); s.e1[1] = 0.0
    bad.append(("e1 == 0", s))
    good = [base, made(patch=1), made(n_u=1, n_v=1), made(n_u=256, n_v=256), made(n_u=1024, n_v=64), made(n_u=64, n_v=1024),
            made(n_u=7, n_v=13, half_extent=0.5), made(half_extent=5e-324), made(axis_at_1=(5e-13,)),
            # a left-handed frame and one that is not the patch's own are used as given
            made(e2_at_2=(-1.0,))]
    s = base.copy()
    s.axis[0], s.axis[2], s.e2[0], s.e2[2] = 0.0, 1.0, -1.0, 0.0
    good.append(s)
    return bad, good


def test_refusals_and_null_arguments_need_no_device():
    """Everything isx_scene_endstates refuses of cfg and scene is refused here with its code; a wrong view spec is
    ISX_ERR_BAD_CONFIG and a NULL pointer ISX_ERR_BAD_ARG, before anything asks for a device (this process never keeps isx_init).
    The detector grid and the hit line are no reason for refusal."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ctypes as C
import numpy as np
import altair_raytracing_amd as isx
from test_scene_cpu import refused_scenes
from test_scene_view_cpu import view_specs
from test_baffle_cpu import big_grids
lib = isx.load()
have = lib.isx_init(0) == 0
if have:
    lib.isx_shutdown()
past = isx.abi.ERR_NOT_INIT if have else isx.abi.ERR_NO_DEVICE
buf = np.full(65536, 7, dtype=np.uint64)
hp = buf.ctypes.data_as(C.POINTER(C.c_uint64))
cnt, vc = isx.SceneCounts(), isx.ViewCounts()
cfg, good, bad, served = refused_scenes(isx)
vbad, vgood = view_specs(isx)
vs = C.byref(vgood[0])
dev = C.c_void_p(4096)
BAD_CONFIG, BAD_ARG = isx.abi.ERR_BAD_CONFIG, isx.abi.ERR_BAD_ARG
for what, c, s in bad:
    assert lib.isx_scene_view(C.byref(c), C.byref(s), vs, 10, 1, 0, hp, C.byref(vc), C.byref(cnt), None) == BAD_CONFIG, what
    assert lib.isx_scene_view_device(C.byref(c), C.byref(s), vs, 10, 1, 0, dev, dev, dev) == BAD_CONFIG, what
    assert lib.isx_view_frame(C.byref(c), C.byref(s), 0, 32, 32, 1.0, C.byref(isx.ViewSpec())) == BAD_CONFIG, what
n_past = 0
for k, (c, s) in enumerate(served):      # (a served scene without patches has no detector: refused)
    want = past if s.patches.n_patches >= 1 else BAD_CONFIG
    n_past += want == past
    assert lib.isx_scene_view(C.byref(c), C.byref(s), vs, 10, 1, 0, hp, None, None, None) == want, k
    assert lib.isx_scene_view_device(C.byref(c), C.byref(s), vs, 10, 1, 0, dev, dev, dev) == want, k
g, cf = C.byref(good), C.byref(cfg)
w = np.ones(65536); sig = C.c_double(0.0)
wp = w.ctypes.data_as(C.POINTER(C.c_double))
for what, r in vbad:
    st = isx.Stats(); st.launched = 77
    assert lib.isx_scene_view(cf, g, C.byref(r), 10, 1, 0, hp, C.byref(vc), C.byref(cnt), C.byref(st)) == BAD_CONFIG, what
    assert lib.isx_scene_view_device(cf, g, C.byref(r), 10, 1, 0, dev, dev, dev) == BAD_CONFIG, what
    assert st.launched == 77
    # (a refused scene with a refused spec is refused all the same)
    assert lib.isx_scene_view(C.byref(bad[0][1]), C.byref(bad[0][2]), C.byref(r), 10, 1, 0, hp, None, None, None) == BAD_CONFIG, what
    if not what.startswith("patch"):      # (the host-side helpers have no scene: the patch index is not looked at)
        assert lib.isx_view_reweight(C.byref(r), hp, C.byref(vc), 10, wp, 1.0, C.byref(sig), None) == BAD_CONFIG, what
        assert lib.isx_view_weight_fov(C.byref(r), 45.0, wp) == BAD_CONFIG, what
for r in vgood:
    assert lib.isx_scene_view(cf, g, C.byref(r), 10, 1, 0, hp, None, None, None) == past, bytes(r)
    assert lib.isx_scene_view_device(cf, g, C.byref(r), 10, 1, 0, dev, dev, dev) == past, bytes(r)
for k in range(4):      # cfg, scene, vspec, view
    a = [cf, g, vs, hp]
    a[k] = None
    assert lib.isx_scene_view(a[0], a[1], a[2], 10, 1, 0, a[3], None, None, None) == BAD_ARG, k
for k in range(6):      # cfg, scene, vspec, d_view, d_view_counts, d_scene_counts
    a = [cf, g, vs, dev, dev, dev]
    a[k] = None
    assert lib.isx_scene_view_device(a[0], a[1], a[2], 10, 1, 0, a[3], a[4], a[5]) == BAD_ARG, k
# the detector grid and the hit line are ignored: what isx_fluxmap_scene refuses for its grid gets past the checks here
grids, fits = big_grids(isx)
for what, c in grids:
    assert lib.isx_fluxmap_scene(C.byref(c), g, 10, 1, 0, hp, None, None) == BAD_CONFIG, what
    assert lib.isx_scene_view(C.byref(c), g, vs, 10, 1, 0, hp, None, None, None) == past, what
    assert lib.isx_scene_view_device(C.byref(c), g, vs, 10, 1, 0, dev, dev, dev) == past, what
for nt, nph, mode in ((0, 0, 0), (-5, 7, 1), (1 << 20, 1 << 20, 1)):
    c = cfg.copy(); c.n_theta, c.n_phi, c.hit_line_mode = nt, nph, mode
    assert lib.isx_scene_view(C.byref(c), g, vs, 10, 1, 0, hp, None, None, None) == past, (nt, nph, mode)
assert (buf == 7).all() and not cnt.words().any() and not vc.words().any()
try:
    isx.scene_view(cfg, good, vbad[0][1], 10, 1)
    print("no error")
except isx.IsxError as e:
    print("ok", e.status, len(bad), len(served), n_past, len(vbad), len(vgood), len(grids))
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    # (146 refused scenes; 22 served ones, 20 of them with a patch 0; 69 refused view specs, 11 past the checks; 4 refused grids)
    assert r.stdout.split() == ["ok", "-2", "146", "22", "20", "69", "11", "4"], r.stdout


def test_no_device_on_a_machine_without_one():
    """where the library can initialise no HIP device, a valid view call is ISX_ERR_NO_DEVICE (a process of its own)"""
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
vs = isx.view_frame(cfg, spec, 0, 32, 32)
for call in (lambda: isx.scene_view(cfg, spec, vs, 10, 1), lambda: isx.scene_view_device(cfg, spec, vs, 10, 1, 0, 4096, 8192, 12288)):
    try:
        call()
        raise SystemExit("no error")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_NO_DEVICE, e.status
print("no device")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() in (["device"], ["no", "device"]), r.stdout + r.stderr[-2000:]


# ---------------------------------------------------------------- isx_view_reweight, isx_view_weight_fov
def _spec(isx, n_u, n_v, h=1.0, patch=0):
    cfg = isx.default_config()
    return isx.view_frame(cfg, scene(isx, cfg, "photometer"), patch, n_u, n_v, h)


def reweight_py(view, direct, launched, w, dw):
    """isx.h's formulas, the sums in increasing b"""
    s1 = s2 = 0.0
    for b in range(w.size):
        s1 += float(w[b]) * float(view[b])
        s2 += float(w[b]) * float(w[b]) * float(view[b])
    s1 += dw * float(direct)
    s2 += dw * dw * float(direct)
    var = s2 - s1 * s1 / float(launched)
    return s1 / float(launched), math.sqrt(var if var > 0 else 0.0) / float(launched)


def test_view_reweight_against_the_formulas():
    import altair_raytracing_amd as isx
    rng = np.random.default_rng(11)
    for n_u, n_v in ((1, 1), (32, 32), (7, 13), (256, 256)):
        vs = _spec(isx, n_u, n_v)
        B = n_u * n_v
        view = rng.integers(0, 3000, size=(n_v, n_u)).astype(np.uint64)
        vc = isx.ViewCounts()
        vc.binned, vc.outside, vc.behind, vc.direct = int(view.sum()), 17, 5, 1234
        launched = int(view.sum()) * 3 + 99991
        # unit weights: (binned + direct) / launched exactly as the division gives it
        sig, sd = isx.view_reweight(vs, view, vc, launched, np.ones(B), 1.0)
        assert sig == float(int(view.sum()) + 1234) / float(launched)
        p = sig
        assert sd == pytest.approx(math.sqrt(p * (1.0 - p) / launched), rel=1e-12)
        # without the direct light
        sig0, _ = isx.view_reweight(vs, view, vc, launched, np.ones((n_v, n_u)))
        assert sig0 == float(int(view.sum())) / float(launched)
        # any weights: the formulas, to the rounding of two sums taken in the same order
        for w, dw in ((rng.random(B) * 3.0, 0.7), ((np.arange(B) % 3 == 0).astype(np.float64), 0.0), (np.full(B, 1e-3), 2.5)):
            got = isx.view_reweight(vs, view, vc, launched, w, dw)
            want = reweight_py(view.reshape(-1), 1234, launched, w, dw)
            assert got[0] == pytest.approx(want[0], rel=1e-14) and got[1] == pytest.approx(want[1], rel=1e-12)
        # the other counters are not read; sigma may be NULL
        vc2 = isx.ViewCounts(); vc2.direct = 1234; vc2.outside = 1 << 60
        assert isx.view_reweight(vs, view, vc2, launched, np.ones(B), 1.0) == (sig, sd)
        lib, s = isx.load(), C.c_double(0.0)
        w = np.ones(B)
        assert lib.isx_view_reweight(C.byref(vs), view.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(vc), launched,
                                     w.ctypes.data_as(C.POINTER(C.c_double)), 1.0, C.byref(s), None) == 0
        assert s.value == sig
    # one ray launched, one binned with weight 1: signal 1, variance 0
    vs = _spec(isx, 2, 1)
    assert isx.view_reweight(vs, np.array([1, 0], dtype=np.uint64), isx.ViewCounts(), 1, np.ones(2)) == (1.0, 0.0)


def test_view_reweight_refusals():
    import altair_raytracing_amd as isx
    lib = isx.load()
    vs = _spec(isx, 3, 2)
    view = np.arange(6, dtype=np.uint64)
    vc = isx.ViewCounts()
    w, s, sd = np.ones(6), C.c_double(0.0), C.c_double(0.0)
    pu, pd = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    args = [C.byref(vs), view.ctypes.data_as(pu), C.byref(vc), 100, w.ctypes.data_as(pd), 1.0, C.byref(s)]
    assert lib.isx_view_reweight(*args, C.byref(sd)) == 0
    for k in (0, 1, 2, 4, 6):
        a = list(args); a[k] = None
        assert lib.isx_view_reweight(*a, None) == isx.abi.ERR_BAD_ARG, k
    for val in (-1.0, -1e-300, np.nan, np.inf, -np.inf):
        for at in (0, 5):
            bad = np.ones(6); bad[at] = val
            with pytest.raises(isx.IsxError) as e:
                isx.view_reweight(vs, view, vc, 100, bad)
            assert e.value.status == isx.abi.ERR_BAD_ARG, (val, at)
        with pytest.raises(isx.IsxError) as e:
            isx.view_reweight(vs, view, vc, 100, w, val)
        assert e.value.status == isx.abi.ERR_BAD_ARG, val
    with pytest.raises(isx.IsxError) as e:
        isx.view_reweight(vs, view, vc, 0, w)
    assert e.value.status == isx.abi.ERR_BAD_CONFIG
    with pytest.raises(ValueError):
        isx.view_reweight(vs, view[:4], vc, 100, w)


def test_view_weight_fov():
    import altair_raytracing_amd as isx
    for n_u, n_v, h in ((32, 32, 1.0), (7, 13, 0.5), (1, 1, 1.0), (64, 3, 0.9)):
        vs = _spec(isx, n_u, n_v, h)
        uc = -h + (np.arange(n_u) + 0.5) * (2.0 * h / n_u)
        vcen = -h + (np.arange(n_v) + 0.5) * (2.0 * h / n_v)
        r2 = vcen[:, None] ** 2 + uc[None, :] ** 2
        # 90 degrees: exactly the centres inside the unit disc; 0 degrees: a centre at the origin alone
        w90 = isx.view_weight_fov(vs, 90.0)
        assert w90.shape == (n_v, n_u) and np.array_equal(w90, (r2 <= 1.0).astype(np.float64))
        assert np.array_equal(isx.view_weight_fov(vs, 0.0), (r2 <= 0.0).astype(np.float64))
        for deg in (10.0, 30.0, 45.0, 89.0):
            s = math.sin(deg * math.pi / 180.0)
            edge = np.abs(r2 - s * s) < 1e-12      # (a centre on the stop's edge to rounding: either answer)
            assert np.array_equal(isx.view_weight_fov(vs, deg)[~edge], (r2 <= s * s).astype(np.float64)[~edge]), deg
    # 32 x 32 at h = 1: centres at (2 i + 1) / 32; those in the unit disc by the integer test (2 i + 1)^2 + (2 j + 1)^2 <= 32^2
    # (no sum of two odd squares is 1024, so no centre lies on the circle)
    i = 2 * np.arange(-16, 16) + 1
    inside = int(((i[:, None] ** 2 + i[None, :] ** 2) <= 32 * 32).sum())
    vs = _spec(isx, 32, 32)
    assert int(isx.view_weight_fov(vs, 90.0).sum()) == inside and abs(inside - math.pi * 256) < 16
    # by hand: a 4 x 4 map at h = 1 has centres at +-0.25 and +-0.75; at 30 degrees (s = 0.5) only the four inner centres
    # (r^2 = 0.125) pass, at 53 degrees (s^2 = 0.638) the eight with r^2 = 0.625 as well, the corners (r^2 = 1.125) never
    vs = _spec(isx, 4, 4)
    inner = np.zeros((4, 4)); inner[1:3, 1:3] = 1.0
    cross = np.ones((4, 4)); cross[0, 0] = cross[0, 3] = cross[3, 0] = cross[3, 3] = 0.0
    assert np.array_equal(isx.view_weight_fov(vs, 30.0), inner)
    assert np.array_equal(isx.view_weight_fov(vs, 53.0), cross) and np.array_equal(isx.view_weight_fov(vs, 90.0), cross)
    assert np.array_equal(isx.view_weight_fov(vs, 52.0), inner)      # (sin^2 52 = 0.621 < 0.625)
    lib = isx.load()
    w = np.zeros(16)
    wp = w.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.isx_view_weight_fov(None, 45.0, wp) == isx.abi.ERR_BAD_ARG and lib.isx_view_weight_fov(C.byref(vs), 45.0, None) == isx.abi.ERR_BAD_ARG
    for deg in (-1e-9, 90.00000001, 180.0, float("nan"), float("inf")):
        with pytest.raises(isx.IsxError) as e:
            isx.view_weight_fov(vs, deg)
        assert e.value.status == isx.abi.ERR_BAD_CONFIG, deg


# ---------------------------------------------------------------- the restatement: view_np
def rule_py(vspec, n_points, d):
    """one ray by the contract, in Python floats: -> ("direct" | "behind" | "outside", None) or ("binned", bin)"""
    _, n_u, n_v, h, ax, e1, e2 = V.frame(vspec)
    if n_points == 2:
        return "direct", None
    c = (d[0] * ax[0] + d[1] * ax[1]) + d[2] * ax[2]
    if not c > 0.0:
        return "behind", None
    s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    mag = math.sqrt(s) if s == s and s != math.inf else s
    a = (d[0] * e1[0] + d[1] * e1[1]) + d[2] * e1[2]
    b = (d[0] * e2[0] + d[1] * e2[1]) + d[2] * e2[2]
    try:
        U, W = -(a / mag), -(b / mag)
    except ZeroDivisionError:
        return "outside", None
    fu = (U + h) / (2.0 * h) * n_u
    fv = (W + h) / (2.0 * h) * n_v
    if fu != fu or fv != fv or math.isinf(fu) or math.isinf(fv):
        return "outside", None
    iu, iv = math.floor(fu), math.floor(fv)
    if 0 <= iu < n_u and 0 <= iv < n_v:
        return "binned", iv * n_u + iu
    return "outside", None


NAMES = {"binned": V.BINNED, "outside": V.OUTSIDE, "behind": V.BEHIND, "direct": V.DIRECT}


def _ocfg(orc, rho=RHO):
    c = orc.default_config()
    c.reflectance = rho
    return c


@pytest.mark.parametrize("which,patch,h,n_u,n_v", [("wide_cap", 0, 1.0, 32, 32), ("wide_cap", 0, 0.5, 7, 13), ("lamp_open", 1, 1.0, 32, 32),
                                                   ("lamp_open", 0, 0.5, 5, 3)])
def test_view_np_against_a_per_ray_loop(orc, which, patch, h, n_u, n_v):
    """2 000 rays of the oracle's walk: the vectorised restatement against the contract applied ray by ray in Python floats, with
    the selection made from the walk's own arrays a second way (status, last class, and no baffle at the end: neither scene has a
    baffle that absorbs where a wall could)"""
    import altair_raytracing_amd as isx
    cfg = isx.default_config()
    spec = wide_cap(isx, cfg) if which == "wide_cap" else scene(isx, cfg, which)
    vs = isx.view_frame(cfg, spec, patch, n_u, n_v, h)
    oc = _ocfg(orc)
    w = orc.scene_walk(oc, SC.spec_of(spec), 2000, SEED, 0, nthreads=4)
    view, counts = V.from_walk(w, oc, vs)
    want_view, want_counts = np.zeros(n_u * n_v, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    r_last = np.sqrt((w["last_point"] ** 2).sum(axis=1))
    for i in range(2000):
        on_wall = w["last_baffle"][i] < 0 or r_last[i] >= oc.r_in - 1e-9
        if w["status"][i] != 2 or not on_wall or w["last_class"][i] != patch:
            continue
        kind, b = rule_py(vs, int(w["n_points"][i]), [float(x) for x in w["direction"][i]])
        want_counts[NAMES[kind]] += np.uint64(1)
        if b is not None:
            want_view[b] += np.uint64(1)
    print(which, "patch", patch, "h", h, "binned / outside / behind / direct", want_counts.tolist())
    assert np.array_equal(counts, want_counts) and np.array_equal(view.reshape(-1), want_view)
    assert int(want_counts.sum()) == int(w["patch_absorbed"][patch]) >= 40
    if which == "wide_cap" and h == 1.0:
        assert want_counts[V.BEHIND] > 20 and want_counts[V.DIRECT] > 100 and want_counts[V.OUTSIDE] == 0
    if h == 0.5:
        assert want_counts[V.OUTSIDE] > 10


def test_view_np_on_hand_made_rays():
    """the frame of `det` -- axis +x, e1 +y, e2 +z -- on a 4 x 4 map: the sign convention and every branch"""
    import altair_raytracing_amd as isx
    vs = _spec(isx, 4, 4)
    assert list(vs.axis) == [1.0, 0.0, 0.0] and list(vs.e1) == [0.0, 1.0, 0.0] and list(vs.e2) == [0.0, 0.0, 1.0]
    nan, inf = float("nan"), float("inf")
    rays = [
        # (n_points, d, branch, bin)
        (5, (0.6, -0.8, 0.0), V.BINNED, 2 * 4 + 3),        # travelling towards -e1: the light came from the +e1 side, U = +0.8
        (5, (0.6, 0.0, 0.8), V.BINNED, 0 * 4 + 2),         # travelling towards +e2: V = -0.8, U = -0 -> fu = 2
        (3, (0.0, -1.0, 0.0), V.BEHIND, None),             # d = -e1 itself grazes: c = 0 is not > 0
        (3, (-0.5, 0.1, 0.1), V.BEHIND, None),             # from behind
        (7, (nan, nan, nan), V.BEHIND, None),              # a NaN direction: c > 0 is false
        (2, (nan, 0.3, 0.1), V.DIRECT, None),              # absorbed at its first interaction, whatever the direction says
        (2, (0.6, -0.8, 0.0), V.DIRECT, None),
        (9, (120.0, 160.0, 0.0), V.BINNED, 2 * 4 + 0),     # |d| = 200, the un-normalised chord: U = -0.8
        (4, (1e-200, -1.0, 0.0), V.OUTSIDE, None),         # U = +1 exactly: fu = n_u, the map's far edge is outside
        (4, (1e-200, 1.0, 0.0), V.BINNED, 2 * 4 + 0),      # U = -1 exactly: fu = 0, the near edge is inside
        (4, (inf, 0.0, 0.0), V.OUTSIDE, None),             # c = inf, a = inf * 0: NaN
        (4, (5e-324, 0.0, 0.0), V.OUTSIDE, None),          # c > 0, |d|^2 underflows to 0: 0 / 0
    ]
    branch, bins = V.classify(vs, [r[0] for r in rays], [r[1] for r in rays])
    for k, (npts, d, want, b) in enumerate(rays):
        assert branch[k] == want, (k, d)
        if b is not None:
            assert bins[k] == b, (k, d)
        kind, pb = rule_py(vs, npts, list(d))
        assert NAMES[kind] == want and pb == b, (k, d, kind, pb)
    # h = 0.5: U = +0.8 lies outside, U = -0.2 in column floor((0.3 / 1.0) * 4) = 1
    half = _spec(isx, 4, 4, 0.5)
    branch, bins = V.classify(half, [5, 5], [(0.6, -0.8, 0.0), (math.sqrt(1.0 - 0.04), 0.2, 0.0)])
    assert branch.tolist() == [V.OUTSIDE, V.BINNED] and bins[1] == 2 * 4 + 1
    # n_u != n_v: the row is iv, the column iu
    wide = _spec(isx, 8, 2)
    branch, bins = V.classify(wide, [5], [(0.6, -0.8, 0.0)])      # fu = 0.9 * 8 = 7.2, fv = 0.5 * 2 = 1
    assert branch.tolist() == [V.BINNED] and bins[0] == 1 * 8 + 7


# ---------------------------------------------------------------- the sharded call
def walk_trace(isx, orc):
    """a stand-in tracer for scene_view_sharded: the oracle's walk and the restatement"""
    def trace(c, sp, vs, count, seed, first):
        w = orc.scene_walk(c, SC.spec_of(sp), count, seed, first, nthreads=2)
        st = orc.Stats()
        for f, val in w["census"].items():
            setattr(st, f, val)
        view, counts = V.from_walk(w, c, vs)
        st.bin_increments = int(counts[V.BINNED])
        cnt, vc = isx.SceneCounts(), isx.ViewCounts()
        C.memmove(C.byref(cnt), SC.counter_words(w).tobytes(), C.sizeof(cnt))
        C.memmove(C.byref(vc), counts.tobytes(), C.sizeof(vc))
        return view, vc, cnt, st
    return trace


N_SHARDED, FIRST_SHARDED = 3001, 1000


def _sharded_case(isx):
    cfg = isx.default_config()
    spec = wide_cap(isx, cfg)
    return spec, isx.view_frame(cfg, spec, 0, 5, 3, 0.75)


def test_sharded_with_one_rank_is_the_plain_call(orc):
    import altair_raytracing_amd as isx
    cfg = _ocfg(orc)
    spec, vs = _sharded_case(isx)
    seen = []
    inner = walk_trace(isx, orc)

    def trace(c, sp, r, count, seed, first):
        seen.append((count, seed, first, sp is spec, r is vs))
        return inner(c, sp, r, count, seed, first)

    view, vc, pa, pb, ba, bb, census = isx.scene_view_sharded(trace, cfg, spec, vs, N_SHARDED, SEED, first_ray=FIRST_SHARDED)
    assert seen == [(N_SHARDED, SEED, FIRST_SHARDED, True, True)]
    plain = inner(cfg, spec, vs, N_SHARDED, SEED, FIRST_SHARDED)
    assert view.shape == (3, 5) and view.dtype == np.uint64 and np.array_equal(view, plain[0])
    assert vc.shape == (4,) and vc.dtype == np.uint64 and np.array_equal(vc, plain[1].words())
    assert int(view.sum()) == int(vc[0]) == census["bin_increments"] > 500 and int(vc.sum()) == int(pb[0])
    assert vc[1] > 100 and vc[2] > 20 and vc[3] > 100
    assert census["launched"] == N_SHARDED
    assert pa.shape == (10,) and ba.shape == (4, 2) and int(pa.sum()) + int(ba.sum()) == census["wall_hits"]


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import oracle
    import altair_raytracing_amd as isx

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    spec, vs = _sharded_case(isx)
    out = isx.scene_view_sharded(walk_trace(isx, oracle), _ocfg(oracle), spec, vs, N_SHARDED, SEED, first_ray=FIRST_SHARDED)
    q.put((rank,) + out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_allreduce_equals_single_rank(orc):
    """two ranks over gloo: the map, its four counters, the 36 scene counters and the census of every rank are those of the job
    in one piece"""
    import socket
    import altair_raytracing_amd as isx
    import torch.multiprocessing as mp

    spec, vs = _sharded_case(isx)
    whole = isx.scene_view_sharded(walk_trace(isx, orc), _ocfg(orc), spec, vs, N_SHARDED, SEED, first_ray=FIRST_SHARDED)
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
    assert whole[6]["launched"] == N_SHARDED and int(whole[0].sum()) == int(whole[1][0])
    for out in got:
        rank, parts_ = out[0], out[1:]
        for a, w in zip(parts_[:6], whole[:6]):
            assert a.dtype == np.uint64 and a.shape == w.shape and np.array_equal(a, w), rank
        assert parts_[6] == whole[6], rank
