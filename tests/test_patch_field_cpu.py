"""The scene patch field (isx_scene_patch_field, isx_patch_field_frame, isx_patch_field_marginals) without a GPU: the bindings and
the frame helper, every refusal, the marginals against numpy sums, the restatement of the contract on the oracle's walk
(field_np) against an independent per-ray loop and on hand-made rays that fix every branch and the index order, its reduction to
the scene view, and the sharded call."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import field_np as F
import scene_np as SC
import view_np as V
from test_scene_cpu import parts, scene
from test_scene_view_cpu import wide_cap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
RHO = 0.95


# ---------------------------------------------------------------- bindings, the frame
def test_binding_structs_and_patch_field_frame():
    import altair_raytracing_amd as isx
    S = isx.PatchFieldSpec
    assert C.sizeof(S) == 120 and C.sizeof(isx.PatchFieldCounts) == 40
    assert (S.struct_size.offset, S.reserved0.offset, S.patch.offset, S.n_x.offset, S.n_y.offset, S.n_u.offset, S.n_v.offset,
            S.reserved1.offset) == (0, 4, 8, 12, 16, 20, 24, 28)
    assert (S.axis.offset, S.e1.offset, S.e2.offset, S.half_extent.offset, S.pos_scale.offset) == (32, 56, 80, 104, 112)
    K = isx.PatchFieldCounts
    assert [f[0] for f in K._fields_] == ["binned", "pos_outside", "dir_outside", "behind", "direct"]
    assert [getattr(K, f[0]).offset for f in K._fields_] == [0, 8, 16, 24, 32]
    assert isx.abi.PATCH_FIELD_MAX_AXIS == 1024 and isx.abi.PATCH_FIELD_MAX_BINS == 1 << 22
    for name in ("isx_patch_field_frame", "isx_scene_patch_field", "isx_scene_patch_field_device", "isx_patch_field_marginals"):
        assert name in isx.EXPORTS and hasattr(isx.load(), name)
    for name in ("PatchFieldSpec", "PatchFieldCounts", "patch_field_frame", "scene_patch_field", "scene_patch_field_device",
                 "patch_field_marginals", "scene_patch_field_sharded"):
        assert name in isx.__all__ and hasattr(isx, name)
    cfg = isx.default_config()
    ph = scene(isx, cfg, "photometer")
    f = isx.patch_field_frame(cfg, ph, 0, 8, 8, 16, 16)
    assert f.struct_size == 120 and f.reserved0 == 0 and f.reserved1 == 0
    assert (f.patch, f.n_x, f.n_y, f.n_u, f.n_v, f.half_extent, f.bins) == (0, 8, 8, 16, 16, 1.0, 16384)
    # `det`: the frame of isx_view_frame, the scale by the formula in Python floats
    v = isx.view_frame(cfg, ph, 0, 16, 16)
    assert list(f.axis) == [1.0, 0.0, 0.0] and list(f.e1) == [0.0, 1.0, 0.0] and list(f.e2) == [0.0, 0.0, 1.0]
    assert bytes(f.axis) == bytes(v.axis) and bytes(f.e1) == bytes(v.e1) and bytes(f.e2) == bytes(v.e2)
    for k in (0, 1):
        f = isx.patch_field_frame(cfg, ph, k, 3, 5, 7, 2, 0.5)
        md = float(ph.patches.patch[k].min_dot)
        assert f.pos_scale == 1.0 / math.sqrt(0.5 * (1.0 - md / float(cfg.r_in)))
        assert (f.patch, f.n_x, f.n_y, f.n_u, f.n_v, f.half_extent, f.bins) == (k, 3, 5, 7, 2, 0.5, 210)
    # oblique caps: the patch's axis bit for bit, isx_view_frame's e1 / e2 bit for bit, s = 1 / sin(alpha / 2) to rounding
    caps = [isx.wall_patch_cap(cfg, (k - 3.5, 1 - 0.3 * k, 2.0 - k), 10.0 + k, k / 7.0) for k in range(8)]
    sc = isx.scene_spec(cfg, parts(isx, cfg)["lamp"], [], caps)
    for k in range(8):
        f = isx.patch_field_frame(cfg, sc, k, 4, 5, 6, 7, 0.25)
        v = isx.view_frame(cfg, sc, k, 6, 7, 0.25)
        assert bytes(f.axis) == bytes(sc.patches.patch[k].axis) == bytes(v.axis)
        assert bytes(f.e1) == bytes(v.e1) and bytes(f.e2) == bytes(v.e2)
        assert f.pos_scale == 1.0 / math.sqrt(0.5 * (1.0 - float(sc.patches.patch[k].min_dot) / float(cfg.r_in)))
        assert f.pos_scale == pytest.approx(1.0 / math.sin(math.radians(10.0 + k) / 2.0), rel=1e-12)
    # refusals of the helper itself
    lib = isx.load()
    out = isx.PatchFieldSpec()
    for k in range(3):
        a = [C.byref(cfg), C.byref(ph), C.byref(out)]
        a[k] = None
        assert lib.isx_patch_field_frame(a[0], a[1], 0, 4, 4, 4, 4, 1.0, a[2]) == isx.abi.ERR_BAD_ARG
    for args in ((2, 4, 4, 4, 4, 1.0), (-1, 4, 4, 4, 4, 1.0), (0, 0, 4, 4, 4, 1.0), (0, 4, 1025, 4, 4, 1.0), (0, 4, 4, -1, 4, 1.0),
                 (0, 4, 4, 4, 0, 1.0), (0, 64, 64, 32, 33, 1.0), (0, 4, 4, 4, 4, 0.0), (0, 4, 4, 4, 4, 1.5),
                 (0, 4, 4, 4, 4, float("nan")), (0, 4, 4, 4, 4, -0.5), (0, 4, 4, 4, 4, float("inf"))):
        with pytest.raises(isx.IsxError) as e:
            isx.patch_field_frame(cfg, ph, *args)
        assert e.value.status == isx.abi.ERR_BAD_CONFIG, args
    with pytest.raises(isx.IsxError) as e:
        isx.patch_field_frame(cfg, isx.default_scene_spec(cfg), 0, 4, 4, 4, 4)      # (a scene without patches)
    assert e.value.status == isx.abi.ERR_BAD_CONFIG
    # a cap of zero angle has no scale: 1 / sqrt(0) is not finite
    zero = isx.scene_spec(cfg, parts(isx, cfg)["lamp"], [], [isx.wall_patch_cap(cfg, (0, 1, 0), 0.0, 0.5)])
    assert float(zero.patches.patch[0].min_dot) == float(cfg.r_in)
    with pytest.raises(isx.IsxError) as e:
        isx.patch_field_frame(cfg, zero, 0, 4, 4, 4, 4)
    assert e.value.status == isx.abi.ERR_BAD_CONFIG
    assert not bytes(out).strip(b"\0")      # (a refused call writes nothing)


def field_specs(isx):
    """([(what, PatchFieldSpec)] that isx.h refuses with ISX_ERR_BAD_CONFIG whatever the scene, [PatchFieldSpec] that get past
    the checks for a scene with at least two patches)"""
    cfg = isx.default_config()
    ph = scene(isx, cfg, "photometer")
    base = isx.patch_field_frame(cfg, ph, 0, 8, 8, 16, 16)

    def made(**kw):
        s = base.copy()
        for k, val in kw.items():
            if isinstance(val, tuple):
                name, i = k.split("_at_")
                getattr(s, name)[int(i)] = val[0]
            else:
                setattr(s, k, val)
        return s

    nan, inf = float("nan"), float("inf")
    bad = [("struct_size %d" % n, made(struct_size=n)) for n in (0, 104, 112, 128, 32)]
    bad += [("reserved0", made(reserved0=1)), ("reserved1", made(reserved1=-1)), ("reserved1 = 7", made(reserved1=7))]
    bad += [("patch %d" % k, made(patch=k)) for k in (-1, 2, 8, 1 << 30, -(1 << 31))]
    for ax in ("n_x", "n_y", "n_u", "n_v"):
        bad += [("%s = %d" % (ax, n), made(**{ax: n})) for n in (0, -1, 1025, 1 << 30, -(1 << 31))]
    bad += [("bins %d x %d x %d x %d" % n, made(n_x=n[0], n_y=n[1], n_u=n[2], n_v=n[3]))
            for n in ((64, 64, 32, 33), (1024, 1024, 4, 2), (1024, 1024, 1024, 1024), (1, 4097, 1024, 1), (65, 64, 32, 32))]
    bad += [("half_extent %r" % h, made(half_extent=h)) for h in (0.0, -0.0, -0.5, 1.0000000000000002, 2.0, nan, inf, -inf)]
    bad += [("pos_scale %r" % s, made(pos_scale=s)) for s in (0.0, -0.0, -1.0, -5e-324, nan, inf, -inf)]
    for name in ("axis", "e1", "e2"):
        for i in range(3):
            for val in (nan, inf, -inf):
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
    good = [base, made(patch=1), made(n_x=1, n_y=1, n_u=1, n_v=1), made(n_x=64, n_y=64, n_u=32, n_v=32),
            made(n_x=1024, n_y=1, n_u=1, n_v=1), made(n_x=1, n_y=1024, n_u=4, n_v=1024), made(n_x=4, n_y=1, n_u=1024, n_v=1024),
            made(n_x=3, n_y=5, n_u=7, n_v=2, half_extent=0.5), made(half_extent=5e-324), made(pos_scale=5e-324),
            made(pos_scale=1e300), made(axis_at_1=(5e-13,)),
            # a left-handed frame and one that is not the patch's own are used as given
            made(e2_at_2=(-1.0,))]
    s = base.copy()
    s.axis[0], s.axis[2], s.e2[0], s.e2[2] = 0.0, 1.0, -1.0, 0.0
    good.append(s)
    return bad, good


def test_refusals_and_null_arguments_need_no_device():
    """Everything isx_scene_endstates refuses of cfg and scene is refused here with its code; a wrong field spec is
    ISX_ERR_BAD_CONFIG and a NULL pointer ISX_ERR_BAD_ARG, before anything asks for a device (this process never keeps isx_init).
    The detector grid and the hit line are no reason for refusal."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ctypes as C
import numpy as np
import altair_raytracing_amd as isx
from test_scene_cpu import refused_scenes
from test_patch_field_cpu import field_specs
from test_baffle_cpu import big_grids
lib = isx.load()
have = lib.isx_init(0) == 0
if have:
    lib.isx_shutdown()
past = isx.abi.ERR_NOT_INIT if have else isx.abi.ERR_NO_DEVICE
buf = np.full(1 << 22, 7, dtype=np.uint64)
hp = buf.ctypes.data_as(C.POINTER(C.c_uint64))
cnt, fc = isx.SceneCounts(), isx.PatchFieldCounts()
cfg, good, bad, served = refused_scenes(isx)
fbad, fgood = field_specs(isx)
fs = C.byref(fgood[0])
dev = C.c_void_p(4096)
BAD_CONFIG, BAD_ARG = isx.abi.ERR_BAD_CONFIG, isx.abi.ERR_BAD_ARG
for what, c, s in bad:
    assert lib.isx_scene_patch_field(C.byref(c), C.byref(s), fs, 10, 1, 0, hp, C.byref(fc), C.byref(cnt), None) == BAD_CONFIG, what
    assert lib.isx_scene_patch_field_device(C.byref(c), C.byref(s), fs, 10, 1, 0, dev, dev, dev) == BAD_CONFIG, what
    assert lib.isx_patch_field_frame(C.byref(c), C.byref(s), 0, 8, 8, 16, 16, 1.0, C.byref(isx.PatchFieldSpec())) == BAD_CONFIG, what
n_past = 0
for k, (c, s) in enumerate(served):      # (a served scene without patches has no patch to select: refused)
    want = past if s.patches.n_patches >= 1 else BAD_CONFIG
    n_past += want == past
    assert lib.isx_scene_patch_field(C.byref(c), C.byref(s), fs, 10, 1, 0, hp, None, None, None) == want, k
    assert lib.isx_scene_patch_field_device(C.byref(c), C.byref(s), fs, 10, 1, 0, dev, dev, dev) == want, k
g, cf = C.byref(good), C.byref(cfg)
for what, r in fbad:
    st = isx.Stats(); st.launched = 77
    assert lib.isx_scene_patch_field(cf, g, C.byref(r), 10, 1, 0, hp, C.byref(fc), C.byref(cnt), C.byref(st)) == BAD_CONFIG, what
    assert lib.isx_scene_patch_field_device(cf, g, C.byref(r), 10, 1, 0, dev, dev, dev) == BAD_CONFIG, what
    assert st.launched == 77
    # (a refused scene with a refused spec is refused all the same)
    assert lib.isx_scene_patch_field(C.byref(bad[0][1]), C.byref(bad[0][2]), C.byref(r), 10, 1, 0, hp, None, None, None) == BAD_CONFIG, what
    if not what.startswith("patch"):      # (the host-side helper has no scene: the patch index is not looked at)
        assert lib.isx_patch_field_marginals(C.byref(r), hp, hp, hp) == BAD_CONFIG, what
for r in fgood:
    assert lib.isx_scene_patch_field(cf, g, C.byref(r), 10, 1, 0, hp, None, None, None) == past, bytes(r)
    assert lib.isx_scene_patch_field_device(cf, g, C.byref(r), 10, 1, 0, dev, dev, dev) == past, bytes(r)
for k in range(4):      # cfg, scene, fspec, field
    a = [cf, g, fs, hp]
    a[k] = None
    assert lib.isx_scene_patch_field(a[0], a[1], a[2], 10, 1, 0, a[3], None, None, None) == BAD_ARG, k
for k in range(6):      # cfg, scene, fspec, d_field, d_field_counts, d_scene_counts
    a = [cf, g, fs, dev, dev, dev]
    a[k] = None
    assert lib.isx_scene_patch_field_device(a[0], a[1], a[2], 10, 1, 0, a[3], a[4], a[5]) == BAD_ARG, k
assert lib.isx_patch_field_marginals(None, hp, None, None) == BAD_ARG and lib.isx_patch_field_marginals(fs, None, None, None) == BAD_ARG
# the detector grid and the hit line are ignored: what isx_fluxmap_scene refuses for its grid gets past the checks here
grids, fits = big_grids(isx)
for what, c in grids:
    assert lib.isx_fluxmap_scene(C.byref(c), g, 10, 1, 0, hp, None, None) == BAD_CONFIG, what
    assert lib.isx_scene_patch_field(C.byref(c), g, fs, 10, 1, 0, hp, None, None, None) == past, what
    assert lib.isx_scene_patch_field_device(C.byref(c), g, fs, 10, 1, 0, dev, dev, dev) == past, what
for nt, nph, mode in ((0, 0, 0), (-5, 7, 1), (1 << 20, 1 << 20, 1)):
    c = cfg.copy(); c.n_theta, c.n_phi, c.hit_line_mode = nt, nph, mode
    assert lib.isx_scene_patch_field(C.byref(c), g, fs, 10, 1, 0, hp, None, None, None) == past, (nt, nph, mode)
assert (buf == 7).all() and not cnt.words().any() and not fc.words().any()
try:
    isx.scene_patch_field(cfg, good, fbad[0][1], 10, 1)
    print("no error")
except isx.IsxError as e:
    print("ok", e.status, len(bad), len(served), n_past, len(fbad), len(fgood), len(grids))
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    # (146 refused scenes; 22 served ones, 20 of them with a patch 0; 88 refused field specs, 14 past the checks; 4 refused grids)
    assert r.stdout.split() == ["ok", "-2", "146", "22", "20", "88", "14", "4"], r.stdout


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
fs = isx.patch_field_frame(cfg, spec, 0, 8, 8, 16, 16)
for call in (lambda: isx.scene_patch_field(cfg, spec, fs, 10, 1),
             lambda: isx.scene_patch_field_device(cfg, spec, fs, 10, 1, 0, 4096, 8192, 12288)):
    try:
        call()
        raise SystemExit("no error")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_NO_DEVICE, e.status
print("no device")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() in (["device"], ["no", "device"]), r.stdout + r.stderr[-2000:]


# ---------------------------------------------------------------- isx_patch_field_marginals
def _spec(isx, n_x, n_y, n_u, n_v, h=1.0, patch=0):
    cfg = isx.default_config()
    return isx.patch_field_frame(cfg, scene(isx, cfg, "photometer"), patch, n_x, n_y, n_u, n_v, h)


def test_marginals_against_numpy_sums():
    import altair_raytracing_amd as isx
    rng = np.random.default_rng(7)
    lib = isx.load()
    pu = C.POINTER(C.c_uint64)
    for n_x, n_y, n_u, n_v in ((3, 5, 7, 2), (1, 1, 1, 1), (8, 8, 16, 16), (1, 1, 32, 32), (8, 8, 1, 1), (2, 1024, 1, 3)):
        fs = _spec(isx, n_x, n_y, n_u, n_v)
        field = rng.integers(0, 1 << 40, size=(n_y, n_x, n_v, n_u)).astype(np.uint64)
        pos, dr = isx.patch_field_marginals(fs, field)
        assert pos.shape == (n_y, n_x) and dr.shape == (n_v, n_u) and pos.dtype == dr.dtype == np.uint64
        assert np.array_equal(pos, field.sum(axis=(2, 3), dtype=np.uint64)) and np.array_equal(dr, field.sum(axis=(0, 1), dtype=np.uint64))
        # either output may be NULL; the other is written all the same, over what was there
        p2 = np.full(n_y * n_x, 9, dtype=np.uint64)
        d2 = np.full(n_v * n_u, 9, dtype=np.uint64)
        assert lib.isx_patch_field_marginals(C.byref(fs), field.ctypes.data_as(pu), p2.ctypes.data_as(pu), None) == 0
        assert lib.isx_patch_field_marginals(C.byref(fs), field.ctypes.data_as(pu), None, d2.ctypes.data_as(pu)) == 0
        assert np.array_equal(p2, pos.reshape(-1)) and np.array_equal(d2, dr.reshape(-1))
    with pytest.raises(ValueError):
        isx.patch_field_marginals(_spec(isx, 3, 5, 7, 2), np.zeros(209, dtype=np.uint64))


# ---------------------------------------------------------------- the restatement: field_np
def rule_py(fspec, r_in, n_points, q, d):
    """one ray by the contract, in Python floats: -> (branch name, bin or None)"""
    _, (n_x, n_y, n_u, n_v), h, s, ax, e1, e2 = F.frame(fspec)

    def div(a, b):      # IEEE division where Python raises
        if b != 0.0 or a != a:
            return a / b
        if a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)

    def sqrt(x):
        return math.nan if x != x or x < 0.0 else (x if x == math.inf else math.sqrt(x))

    def cell(f, n):
        if f != f or math.isinf(f):
            return None
        i = math.floor(f)
        return i if 0 <= i < n else None

    if n_points == 2:
        return "direct", None
    cd = (d[0] * ax[0] + d[1] * ax[1]) + d[2] * ax[2]
    if not cd > 0.0:
        return "behind", None
    inv = 1.0 / r_in
    c = ((q[0] * ax[0] + q[1] * ax[1]) + q[2] * ax[2]) * inv
    w = sqrt(div(0.5, 1.0 + c))
    a = (q[0] * e1[0] + q[1] * e1[1]) + q[2] * e1[2]
    b = (q[0] * e2[0] + q[1] * e2[1]) + q[2] * e2[2]
    X, Y = ((a * inv) * w) * s, ((b * inv) * w) * s
    ix, iy = cell((X + 1.0) * 0.5 * n_x, n_x), cell((Y + 1.0) * 0.5 * n_y, n_y)
    if ix is None or iy is None:
        return "pos_outside", None
    mag = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    a = (d[0] * e1[0] + d[1] * e1[1]) + d[2] * e1[2]
    b = (d[0] * e2[0] + d[1] * e2[1]) + d[2] * e2[2]
    U, W = -div(a, mag), -div(b, mag)
    iu, iv = cell(div(U + h, 2.0 * h) * n_u, n_u), cell(div(W + h, 2.0 * h) * n_v, n_v)
    if iu is None or iv is None:
        return "dir_outside", None
    return "binned", ((iy * n_x + ix) * n_v + iv) * n_u + iu


NAMES = {"binned": F.BINNED, "pos_outside": F.POS_OUTSIDE, "dir_outside": F.DIR_OUTSIDE, "behind": F.BEHIND, "direct": F.DIRECT}


def _ocfg(orc, rho=RHO):
    c = orc.default_config()
    c.reflectance = rho
    return c


@pytest.mark.parametrize("which,patch,h,scale,axes", [("wide_cap", 0, 1.0, 1.0, (8, 8, 16, 16)), ("wide_cap", 0, 0.5, 2.0, (3, 5, 7, 2)),
                                                      ("lamp_open", 1, 1.0, 1.0, (8, 8, 16, 16)), ("lamp_open", 0, 0.5, 2.0, (5, 3, 2, 7))])
def test_field_np_against_a_per_ray_loop(orc, which, patch, h, scale, axes):
    """2 000 rays of the oracle's walk: the vectorised restatement against the contract applied ray by ray in Python floats, with
    the selection made from the walk's own arrays a second way (status, last class, and no baffle at the end)"""
    import altair_raytracing_amd as isx
    cfg = isx.default_config()
    spec = wide_cap(isx, cfg) if which == "wide_cap" else scene(isx, cfg, which)
    fs = isx.patch_field_frame(cfg, spec, patch, *axes, h)
    fs.pos_scale = fs.pos_scale * scale
    oc = _ocfg(orc)
    w = orc.scene_walk(oc, SC.spec_of(spec), 2000, SEED, 0, nthreads=4)
    field, counts = F.from_walk(w, oc, fs)
    want_field, want_counts = np.zeros(fs.bins, dtype=np.uint64), np.zeros(5, dtype=np.uint64)
    r_last = np.sqrt((w["last_point"] ** 2).sum(axis=1))
    for i in range(2000):
        on_wall = w["last_baffle"][i] < 0 or r_last[i] >= oc.r_in - 1e-9
        if w["status"][i] != 2 or not on_wall or w["last_class"][i] != patch:
            continue
        kind, b = rule_py(fs, float(oc.r_in), int(w["n_points"][i]), [float(x) for x in w["last_point"][i]],
                          [float(x) for x in w["direction"][i]])
        want_counts[NAMES[kind]] += np.uint64(1)
        if b is not None:
            want_field[b] += np.uint64(1)
    print(which, "patch", patch, "h", h, "scale x", scale, "binned / pos_outside / dir_outside / behind / direct", want_counts.tolist())
    assert np.array_equal(counts, want_counts) and np.array_equal(field.reshape(-1), want_field)
    assert int(want_counts.sum()) == int(w["patch_absorbed"][patch]) >= 40
    if scale == 1.0:
        assert want_counts[F.POS_OUTSIDE] == 0 and want_counts[F.DIR_OUTSIDE] == 0
    else:
        assert want_counts[F.POS_OUTSIDE] > 10 and want_counts[F.DIR_OUTSIDE] > 5
    if which == "wide_cap":
        assert want_counts[F.BEHIND] > 20 and want_counts[F.DIRECT] > 100


def test_field_np_on_hand_made_rays():
    """the frame of `det` -- axis +x, e1 +y, e2 +z -- with pos_scale 1 (the whole sphere but the antipode lies in the unit disc)
    on a (4, 4, 4, 4) field: every branch in the contract's order"""
    import altair_raytracing_amd as isx
    fs = _spec(isx, 4, 4, 4, 4)
    fs.pos_scale = 1.0
    assert list(fs.axis) == [1.0, 0.0, 0.0] and list(fs.e1) == [0.0, 1.0, 0.0] and list(fs.e2) == [0.0, 0.0, 1.0]
    R = float(isx.default_config().r_in)
    nan = float("nan")
    # the antipode of the rule is c = -1 exactly; inv is the rounded 1 / r_in, so the x with x * inv == 1 is R to within an ulp or two
    inv = 1.0 / R
    xa = next(x for x in (R, math.nextafter(R, 0.0), math.nextafter(R, 2 * R), math.nextafter(math.nextafter(R, 0.0), 0.0),
                          math.nextafter(math.nextafter(R, 2 * R), 2 * R)) if x * inv == 1.0)
    pole, anti = (R, 0.0, 0.0), (-xa, 0.0, 0.0)
    ok_d = (0.6, -0.8, 0.0)                 # U = +0.8, V = -0: iu = 3, iv = 2
    rays = [
        # (n_points, q, d, branch, bin)
        (5, pole, ok_d, F.BINNED, ((2 * 4 + 2) * 4 + 2) * 4 + 3),          # the pole: X = Y = 0 -> ix = iy = 2
        (2, pole, ok_d, F.DIRECT, None),                                   # n_points 2 is direct whatever else holds:
        (2, anti, (nan, nan, nan), F.DIRECT, None),                        #   the antipode with a NaN direction
        (2, (nan, nan, nan), (-1.0, 0.0, 0.0), F.DIRECT, None),            #   a NaN position, from behind
        (3, pole, (0.0, -1.0, 0.0), F.BEHIND, None),                       # cd == 0 is not > 0
        (3, anti, (0.0, -1.0, 0.0), F.BEHIND, None),                       #   ... before the position is looked at
        (7, pole, (nan, nan, nan), F.BEHIND, None),                        # a NaN direction: cd > 0 is false
        (7, pole, (-0.5, 0.1, 0.1), F.BEHIND, None),
        (4, anti, ok_d, F.POS_OUTSIDE, None),                              # c = -1: 0.5 / 0 = inf, a = 0: 0 * inf = NaN
        (4, (-xa, 1e-9, 0.0), ok_d, F.POS_OUTSIDE, None),                  #   ... and beside it: X = inf
        (4, (-R * 1.000001, 0.0, 0.0), ok_d, F.POS_OUTSIDE, None),         #   ... and past it: the root of a negative number
        (4, (nan, 0.0, 0.0), ok_d, F.POS_OUTSIDE, None),
        (4, (0.0, R, 0.0), ok_d, F.BINNED, ((2 * 4 + 3) * 4 + 2) * 4 + 3),     # 90 degrees towards +e1: X = sqrt(0.5)
        (4, (0.0, 0.0, -R), ok_d, F.BINNED, ((0 * 4 + 2) * 4 + 2) * 4 + 3),    # towards -e2: Y = -sqrt(0.5) -> iy = 0
        (4, pole, (1e-200, -1.0, 0.0), F.DIR_OUTSIDE, None),               # a position in range with U = +1 exactly
        (4, pole, (1e-200, 1.0, 0.0), F.BINNED, ((2 * 4 + 2) * 4 + 2) * 4 + 0),    # U = -1 exactly is inside
        (4, pole, (5e-324, 0.0, 0.0), F.DIR_OUTSIDE, None),                # |d|^2 underflows: 0 / 0
        (9, pole, (120.0, 160.0, 0.0), F.BINNED, ((2 * 4 + 2) * 4 + 2) * 4 + 0),   # |d| = 200, the un-normalised chord
    ]
    branch, bins = F.classify(fs, R, [r[0] for r in rays], [r[1] for r in rays], [r[2] for r in rays])
    for k, (npts, q, d, want, b) in enumerate(rays):
        assert branch[k] == want, (k, q, d)
        if b is not None:
            assert bins[k] == b, (k, q, d)
        kind, pb = rule_py(fs, R, npts, list(q), list(d))
        assert NAMES[kind] == want and pb == b, (k, q, d, kind, pb)
    # X = +1 exactly is outside and X = -1 inside: q at 90 degrees has a * inv = 1 and w = sqrt(0.5), and sqrt(0.5) * sqrt(2)
    # rounds to 1.0000000000000002; q = (0, R, 0) with pos_scale = 1 / sqrt(0.5) computed so that the product is exactly 1
    half = math.sqrt(0.5)
    s1 = next(s for s in (1.0 / half, math.nextafter(1.0 / half, 0.0), math.nextafter(1.0 / half, 2.0)) if half * s == 1.0)
    fs.pos_scale = s1
    # (xa: the radius with xa * inv == 1 exactly, as above)
    edge = [(0.0, xa, 0.0), (0.0, -xa, 0.0), (0.0, 0.0, xa), (0.0, 0.0, -xa)]
    X, Y = F.position(fs, R, edge)
    assert X.tolist() == [1.0, -1.0, 0.0, 0.0] and Y.tolist() == [0.0, 0.0, 1.0, -1.0]
    branch, bins = F.classify(fs, R, [4] * 4, edge, [ok_d] * 4)
    assert branch.tolist() == [F.POS_OUTSIDE, F.BINNED, F.POS_OUTSIDE, F.BINNED]
    assert bins[1] == ((2 * 4 + 0) * 4 + 2) * 4 + 3 and bins[3] == ((0 * 4 + 2) * 4 + 2) * 4 + 3
    for q, want in ((edge[0], "pos_outside"), (edge[1], "binned")):
        assert rule_py(fs, R, 4, list(q), list(ok_d))[0] == want


def test_field_np_index_order_on_asymmetric_axes():
    """(n_x, n_y, n_u, n_v) = (3, 5, 7, 2): field[iy][ix][iv][iu], one ray in a cell whose four indices all differ"""
    import altair_raytracing_amd as isx
    fs = _spec(isx, 3, 5, 7, 2)
    fs.pos_scale = 1.0
    R = float(isx.default_config().r_in)
    # q at polar angle t from +x, azimuth from +y towards +z: X = sin(t / 2) * cos(az) * ... the Lambert radius is sin(t / 2)
    # (with s = 1): t = 120 degrees, towards (e1, e2) = (0.6, -0.8): rho = sin 60 = 0.866 -> X = 0.5196, Y = -0.6928
    t, ux, uy = math.radians(120.0), 0.6, -0.8
    q = (R * math.cos(t), R * math.sin(t) * ux, R * math.sin(t) * uy)
    X, Y = F.position(fs, R, [q])
    assert X[0] == pytest.approx(math.sin(t / 2) * ux, abs=1e-12) and Y[0] == pytest.approx(math.sin(t / 2) * uy, abs=1e-12)
    ix, iy = math.floor((X[0] + 1.0) * 0.5 * 3), math.floor((Y[0] + 1.0) * 0.5 * 5)
    assert (ix, iy) == (2, 0)
    d = (0.6, 0.48, -0.64)      # U = -0.48 -> fu = 0.26 * 7 = 1.82; V = +0.64 -> fv = 0.82 * 2 = 1.64
    branch, bins = F.classify(fs, R, [5], [q], [d])
    assert branch.tolist() == [F.BINNED] and bins[0] == ((0 * 3 + 2) * 2 + 1) * 7 + 1
    w = {"n_points": np.array([5]), "last_point": np.array([q]), "direction": np.array([d])}
    kind, b = rule_py(fs, R, 5, list(q), list(d))
    assert (kind, b) == ("binned", int(bins[0]))
    field = np.bincount(bins, minlength=210).reshape(5, 3, 2, 7)
    assert field[0, 2, 1, 1] == 1 and field.sum() == 1
    pos, dr = isx.patch_field_marginals(fs, field.astype(np.uint64))
    assert pos[0, 2] == 1 and dr[1, 1] == 1 and pos.sum() == dr.sum() == 1
    del w


@pytest.mark.parametrize("which,patch,h", [("wide_cap", 0, 1.0), ("wide_cap", 0, 0.5), ("photometer", 1, 1.0)])
def test_one_position_bin_is_the_scene_view(orc, which, patch, h):
    """n_x = n_y = 1 with pos_scale halved -- the cap then fills the disc of radius 1/2: every position in range -- is
    view_np.from_walk: the map, dir_outside = outside, behind, direct"""
    import altair_raytracing_amd as isx
    cfg = isx.default_config()
    spec = wide_cap(isx, cfg) if which == "wide_cap" else scene(isx, cfg, which)
    fs = isx.patch_field_frame(cfg, spec, patch, 1, 1, 32, 32, h)
    fs.pos_scale = fs.pos_scale * 0.5
    vs = isx.view_frame(cfg, spec, patch, 32, 32, h)
    oc = _ocfg(orc)
    w = orc.scene_walk(oc, SC.spec_of(spec), 20000, SEED, 0, nthreads=4)
    field, fc = F.from_walk(w, oc, fs)
    view, vc = V.from_walk(w, oc, vs)
    assert fc[F.POS_OUTSIDE] == 0 and vc[V.BINNED] > 200
    assert np.array_equal(field.reshape(32, 32), view)
    assert (fc[F.BINNED], fc[F.DIR_OUTSIDE], fc[F.BEHIND], fc[F.DIRECT]) == (vc[V.BINNED], vc[V.OUTSIDE], vc[V.BEHIND], vc[V.DIRECT])
    # and at any position grid, behind and direct are the view's and the direction marginal is below the view's map
    fs2 = isx.patch_field_frame(cfg, spec, patch, 3, 5, 32, 32, h)
    field2, fc2 = F.from_walk(w, oc, fs2)
    assert fc2[F.BEHIND] == vc[V.BEHIND] and fc2[F.DIRECT] == vc[V.DIRECT]
    assert np.array_equal(field2.sum(axis=(0, 1)), view) and fc2[F.POS_OUTSIDE] == 0      # (the helper's scale: the cap fills the disc)


# ---------------------------------------------------------------- the sharded call
def walk_trace(isx, orc):
    """a stand-in tracer for scene_patch_field_sharded: the oracle's walk and the restatement"""
    def trace(c, sp, fs, count, seed, first):
        w = orc.scene_walk(c, SC.spec_of(sp), count, seed, first, nthreads=2)
        st = orc.Stats()
        for f, val in w["census"].items():
            setattr(st, f, val)
        field, counts = F.from_walk(w, c, fs)
        st.bin_increments = int(counts[F.BINNED])
        cnt, fc = isx.SceneCounts(), isx.PatchFieldCounts()
        C.memmove(C.byref(cnt), SC.counter_words(w).tobytes(), C.sizeof(cnt))
        C.memmove(C.byref(fc), counts.tobytes(), C.sizeof(fc))
        return field, fc, cnt, st
    return trace


N_SHARDED, FIRST_SHARDED = 3001, 1000


def _sharded_case(isx):
    cfg = isx.default_config()
    spec = wide_cap(isx, cfg)
    fs = isx.patch_field_frame(cfg, spec, 0, 3, 2, 5, 3, 0.75)
    fs.pos_scale = fs.pos_scale * 1.5
    return spec, fs


def test_sharded_with_one_rank_is_the_plain_call(orc):
    import altair_raytracing_amd as isx
    cfg = _ocfg(orc)
    spec, fs = _sharded_case(isx)
    seen = []
    inner = walk_trace(isx, orc)

    def trace(c, sp, r, count, seed, first):
        seen.append((count, seed, first, sp is spec, r is fs))
        return inner(c, sp, r, count, seed, first)

    field, fc, pa, pb, ba, bb, census = isx.scene_patch_field_sharded(trace, cfg, spec, fs, N_SHARDED, SEED, first_ray=FIRST_SHARDED)
    assert seen == [(N_SHARDED, SEED, FIRST_SHARDED, True, True)]
    plain = inner(cfg, spec, fs, N_SHARDED, SEED, FIRST_SHARDED)
    assert field.shape == (2, 3, 3, 5) and field.dtype == np.uint64 and np.array_equal(field, plain[0])
    assert fc.shape == (5,) and fc.dtype == np.uint64 and np.array_equal(fc, plain[1].words())
    assert int(field.sum()) == int(fc[0]) == census["bin_increments"] > 200 and int(fc.sum()) == int(pb[0])
    assert fc[1] > 100 and fc[2] > 50 and fc[3] > 20 and fc[4] > 100
    assert census["launched"] == N_SHARDED
    assert pa.shape == (10,) and ba.shape == (4, 2) and int(pa.sum()) + int(ba.sum()) == census["wall_hits"]


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import oracle
    import altair_raytracing_amd as isx

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    spec, fs = _sharded_case(isx)
    out = isx.scene_patch_field_sharded(walk_trace(isx, oracle), _ocfg(oracle), spec, fs, N_SHARDED, SEED, first_ray=FIRST_SHARDED)
    q.put((rank,) + out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_allreduce_equals_single_rank(orc):
    """two ranks over gloo: the field, its five counters, the 36 scene counters and the census of every rank are those of the job
    in one piece"""
    import socket
    import altair_raytracing_amd as isx
    import torch.multiprocessing as mp

    spec, fs = _sharded_case(isx)
    whole = isx.scene_patch_field_sharded(walk_trace(isx, orc), _ocfg(orc), spec, fs, N_SHARDED, SEED, first_ray=FIRST_SHARDED)
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
