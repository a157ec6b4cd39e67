"""The trace kernels of the last four features -- wall patches, beam source, baffles, the scene call -- at 1e6 rays against the
oracle's native scene walk (isxo_scene_walk: the composed contract of include/isx.h restated in C, itself held against the Python
replays by tests/test_scene_walk_cpu.py), and the contract's ties (test_scene_walk_cpu.tie_cases) on the GPU.

Every comparison is bit for bit.  Each test does one walk (computed once per key, shared, never changed) and a few GPU calls.
The conditions on the walk -- enough arrivals on every baffle side, every patch and the rim / outer sphere, enough counted lines,
a ray of more than 1000 points in the rows of the long rays -- are asserted on the oracle alone before anything of the library is looked at.

A case that cannot be built: "s_q == 0" with the crossing inside a disc (a disc lies strictly inside the cavity, q on the wall);
see test_scene_walk_cpu.py.
"""
import ctypes as C

import numpy as np
import pytest

import scene_np as SC
import test_gpu_baffle as TB
import test_gpu_beam as TBM
import test_gpu_wall_patches as TW
from test_gpu_scene import _case, _endstates_equal, _fluxmap_equal
from test_scene_walk_cpu import COPLANAR, TIE_COUNTS, TIES, coplanar, expect_tie, tie_cases

pytestmark = pytest.mark.gpu

SEED = 12345
N = 1_000_000
CROSSING = (1 << 32) - 500_000      # the ray index passes 2^32 in the middle of one launch
_reset = TB._reset                  # (the longest list of switches: the fate scan's too)

_walks = {}


def _walked(orc, key, cfg, scene, n, seed, first=0):
    """the walk of a scene: computed once, shared, never changed (the hit line plays no part in it)"""
    if key not in _walks:
        _walks[key] = orc.scene_walk(cfg, scene, n, seed, first, nthreads=16)
    return _walks[key]


def walk_conditions(w, nb, P, long_rays):
    """conditions on the walk alone: every part of the scene takes part, often"""
    pa, ba = w["patch_arrivals"], w["baffle_arrivals"]
    print("patch arrivals", pa.tolist(), "absorbed", w["patch_absorbed"].tolist(), "baffle arrivals", ba.tolist(), "absorbed",
          w["baffle_absorbed"].tolist(), w["census"], "longest ray", int(w["n_points"].max()))
    assert pa.size == P + 2 and ba.shape[0] == max(nb, 1)
    if nb:
        assert int(ba.min()) >= 1000, ba.tolist()
    if P:
        assert int(pa[:P].min()) >= 1000, pa.tolist()
    assert int(pa[P + 1]) >= 100
    assert w["census"]["counted_below_z"] >= 1000
    if long_rays:
        assert int(w["n_points"].max()) > 1000
    assert int(pa.sum()) + int(ba.sum()) == w["census"]["wall_hits"]


# (scene, wall reflectance, first ray, theta_max_deg).  A ray of more than 1000 points among 1e6 needs a loss per bounce below
# ln(1e6) / 1000 = 1.4 %; the default port (theta_max 170 degrees: 0.76 % of the sphere) and a wall of 0.99 lose 1.76 % before any
# patch or baffle.  The row of the long rays therefore narrows the port to 3 degrees (0.07 %) and, led_first_in's two patches and
# its baffle taking another 0.7 %, raises the wall to 0.997: the walk then has 48 rays above 1000 points, the longest 1249.
ROWS = [("photometer", 0.95, 0, 170.0), ("photometer", 0.95, CROSSING, 170.0), ("led_first_in", 0.997, 0, 177.0), ("full", 0.95, 0, 170.0)]
ROW_IDS = ["photometer", "photometer-across-2^32", "led_first_in-long-rays", "full"]
LONG = ("led_first_in", 0.997, 0, 177.0)


def _row_case(mod, name, rho, theta, compat=False):
    c, spec = _case(mod, name, rho, compat)
    c.theta_max_deg = theta
    return c, spec


class _Binned:
    """the oracle with the binning of a walk's counted lines kept: computed once per (walk, hit-line mode), on 16 threads"""
    _kept = {}

    def __init__(self, orc, key):
        self.orc, self.key = orc, key

    def bin_lines(self, oc, P, V):
        k = (self.key, oc.hit_line_mode)
        if k not in self._kept:
            self._kept[k] = self.orc.bin_lines(oc, P, V, nthreads=16)
        return self._kept[k]


def _scene_row(orc, name, rho, first, theta):
    oc, spec = _row_case(orc, name, rho, theta)
    w = _walked(orc, ("scene", name, rho, first, theta), oc, SC.spec_of(spec), N, SEED, first)
    walk_conditions(w, spec.baffles.n_baffles, spec.patches.n_patches, theta != 170.0)
    return w


@pytest.mark.parametrize("name,rho,first,theta", ROWS, ids=ROW_IDS)
def test_scene_endstates_equal_the_walk(isx, orc, name, rho, first, theta):
    w = _scene_row(orc, name, rho, first, theta)
    _reset(isx)
    cfg, spec = _row_case(isx, name, rho, theta)
    _endstates_equal(isx.scene_endstates(cfg, spec, N, SEED, first_ray=first), w)


@pytest.mark.parametrize("compat", [False, True], ids=["last-segment", "origin-compat"])
@pytest.mark.parametrize("name,rho,first,theta", ROWS, ids=ROW_IDS)
def test_fluxmap_scene_equals_the_walk(isx, orc, name, rho, first, theta, compat):
    w = _scene_row(orc, name, rho, first, theta)
    _reset(isx)
    cfg, spec = _row_case(isx, name, rho, theta, compat)
    oc, _ = _row_case(orc, name, rho, theta, compat)
    _fluxmap_equal(_Binned(orc, ("scene", name, rho, first, theta)), oc, isx.fluxmap_scene(cfg, spec, N, SEED, first_ray=first), w)


def test_fluxmap_scene_one_workgroup_equals_the_walk(isx, orc):
    """the row of the long rays through ONE workgroup (`grid_blocks` 1): the state with full rings, held against the independent
    statement and not only against the default launch"""
    w = _scene_row(orc, *LONG)
    name, rho, first, theta = LONG
    _reset(isx)
    cfg, spec = _row_case(isx, name, rho, theta)
    oc, _ = _row_case(orc, name, rho, theta)
    try:
        isx.set_option("grid_blocks", 1)
        _fluxmap_equal(_Binned(orc, ("scene",) + LONG), oc, isx.fluxmap_scene(cfg, spec, N, SEED), w)
    finally:
        _reset(isx)


# ---------------------------------------------------------------- the specialised calls
def _as_baffle_replay(w):
    """the walk's result under the names of baffle_np.replay"""
    return dict(w, arrivals=w["baffle_arrivals"], absorbed=w["baffle_absorbed"])


def _as_beam_replay(w):
    """the walk's result as the tuple of beam_np.replay"""
    return (w["start_point"], w["start_dir"], w["status"], w["n_points"], w["last_point"], w["direction"], w["first_kind"], w["census"])


@pytest.mark.parametrize("compat", [False, True], ids=["last-segment", "origin-compat"])
def test_the_baffle_calls_equal_the_walk(isx, orc, compat):
    """`two` of test_gpu_baffle.FIXTURES: isx_baffle_endstates in its five arrays, isx_fluxmap_baffle in histogram, census and the
    16 words"""
    oc, spec = TB._case(orc, "two", 0.95, compat)
    w = _walked(orc, ("baffle", "two"), oc, {"beam": None, "baffles": TB.BF.spec_of(spec), "patches": []}, N, TB.SEED)
    walk_conditions(w, 2, 0, False)
    _reset(isx)
    cfg, spec = TB._case(isx, "two", 0.95, compat)
    rep = _as_baffle_replay(w)
    if not compat:      # (the end states do not depend on the hit line)
        TB._endstates_equal(isx.baffle_endstates(cfg, spec, N, TB.SEED), rep)
    TB._fluxmap_equal(_Binned(orc, ("baffle", "two")), oc, isx.fluxmap_baffle(cfg, spec, N, TB.SEED), rep)


def test_the_beam_calls_equal_the_walk(isx, orc):
    """`side` of test_gpu_beam at reflectance 0.99, the port narrowed to 3 degrees for the long rays (ROWS): isx_beam_endstates in
    its six arrays, isx_fluxmap_beam in histogram and census"""
    oc, spec = TBM._case(orc, "side", rho=0.99)
    oc.theta_max_deg = 177.0
    w = _walked(orc, ("beam", "side"), oc, {"beam": TBM.B.spec_of(spec), "baffles": [], "patches": []}, N, TBM.SEED)
    walk_conditions(w, 0, 0, True)
    k0 = np.bincount(w["first_kind"], minlength=5)
    assert k0[SC.K_INNER] > 100_000 and k0[SC.K_OUTER] >= 100 and k0[SC.K_CONE] >= 100 and k0[SC.K_BOX] >= 100, k0.tolist()
    TBM._reset(isx)
    cfg, spec = TBM._case(isx, "side", rho=0.99)
    cfg.theta_max_deg = 177.0
    st, npts, lp, d, sp, sd = isx.beam_endstates(cfg, spec, N, TBM.SEED)
    assert np.array_equal(sp, w["start_point"]) and np.array_equal(sd, w["start_dir"]), "start"
    assert np.array_equal(st, w["status"]) and np.array_equal(npts, w["n_points"])
    assert np.array_equal(lp, w["last_point"]), "last point"
    assert np.array_equal(d, w["direction"]), "direction"
    TBM._fluxmap_equal(_Binned(orc, ("beam", "side")), oc, isx.fluxmap_beam(cfg, spec, N, TBM.SEED), _as_beam_replay(w))


def test_the_wall_patches_equal_the_walk(isx, orc):
    """`eight`, the largest fixture of test_gpu_wall_patches.py, at its own reflectance (the default's 0.99): arrivals and absorbed
    of the ten classes, the census and the identities"""
    oc, spec = TW._case(orc, "eight")
    w = _walked(orc, ("patches", "eight"), oc, {"beam": None, "baffles": [], "patches": TW.W.spec_of(spec)}, N, TW.SEED)
    walk_conditions(w, 0, 8, False)
    TW._reset(isx)
    cfg, spec = TW._case(isx, "eight")
    TW._equal_to_replay(isx, isx.wall_patches(cfg, N, TW.SEED, spec), (w["patch_arrivals"], w["patch_absorbed"], w["census"]), 8)


# ---------------------------------------------------------------- the contract's ties
def library_case(isx, cfg, scene):
    """(isx.Config, SceneSpec) of a case of test_scene_walk_cpu: every number of the scene dict goes into the structs as given"""
    c = isx.Config.from_buffer_copy(bytes(cfg))
    s = isx.default_scene_spec(c)      # (the pencil of cfg as the degenerate beam)
    if scene["beam"] is not None:
        b = scene["beam"]
        for k in ("origin", "axis", "e1", "e2"):
            setattr(s.beam, k, (C.c_double * 3)(*b[k]))
        s.beam.radius, s.beam.cos_min, s.beam.angular_law = b["radius"], b["cos_min"], b["law"]
    s.baffles.n_baffles = len(scene["baffles"])
    for k, (centre, normal, radius, rho) in enumerate(scene["baffles"]):
        s.baffles.baffle[k].centre, s.baffles.baffle[k].normal = (C.c_double * 3)(*centre), (C.c_double * 3)(*normal)
        s.baffles.baffle[k].radius, s.baffles.baffle[k].reflectance = radius, rho
    s.patches.n_patches = len(scene["patches"])
    for k, (axis, min_dot, rho) in enumerate(scene["patches"]):
        s.patches.patch[k].axis = (C.c_double * 3)(*axis)
        s.patches.patch[k].min_dot, s.patches.patch[k].reflectance = min_dot, rho
    return c, s


def _compat(c):
    c = c.copy()
    c.hit_line_mode = 1
    return c


@pytest.mark.parametrize("n", TIE_COUNTS)
@pytest.mark.parametrize("name", TIES)
def test_ties_equal_the_walk(isx, orc, name, n):
    """every tie through isx_scene_endstates and isx_fluxmap_scene (whose first segment takes the parked path) and, where the
    source is the pencil of the configuration, through the specialised calls (there the first boundary is the per-workgroup one)"""
    oc, scene, pencil = tie_cases(orc)[name]
    w = _walked(orc, ("tie", name, n), oc, scene, n, SEED)
    expect_tie(name, w, n)
    _reset(isx)
    cfg, spec = library_case(isx, oc, scene)
    _endstates_equal(isx.scene_endstates(cfg, spec, n, SEED), w)
    _fluxmap_equal(orc, oc, isx.fluxmap_scene(cfg, spec, n, SEED), w)
    _fluxmap_equal(orc, _compat(oc), isx.fluxmap_scene(_compat(cfg), spec, n, SEED), w)
    if pencil and scene["baffles"]:
        rep = _as_baffle_replay(w)
        TB._endstates_equal(isx.baffle_endstates(cfg, spec.baffles, n, SEED), rep)
        TB._fluxmap_equal(orc, oc, isx.fluxmap_baffle(cfg, spec.baffles, n, SEED), rep)
    if pencil and scene["patches"]:
        P = len(scene["patches"])
        TW._equal_to_replay(isx, isx.wall_patches(cfg, n, SEED, spec.patches), (w["patch_arrivals"], w["patch_absorbed"], w["census"]), P)


N_COPLANAR = 200_000


@pytest.mark.parametrize("variant", COPLANAR)
def test_coplanar_discs_equal_the_walk(isx, orc, variant):
    """two discs in one plane at 2e5 rays: whether a ray re-emitted from one disc "crosses" the other at f ~ 1e-17 is the sign of
    a rounding error of s_p -- one contracted multiply-add in the kernel's segment test would flip it"""
    oc, scene = coplanar(orc, variant)
    w = _walked(orc, ("coplanar", variant), oc, scene, N_COPLANAR, SEED)
    print("rays from disc to disc:", w["rays_baffle_to_baffle"])
    assert w["rays_baffle_to_baffle"] >= 100
    walk_conditions(w, 2, 0, False)
    _reset(isx)
    cfg, spec = library_case(isx, oc, scene)
    _endstates_equal(isx.scene_endstates(cfg, spec, N_COPLANAR, SEED), w)
    _fluxmap_equal(orc, oc, isx.fluxmap_scene(cfg, spec, N_COPLANAR, SEED), w)
