"""The oracle's native scene walk (isxo_scene_walk, tests/oracle.py: scene_walk) without a GPU.

The walk restates the composed contract of include/isx.h (scene section, steps 1-6) in C, so that the GPU suites can hold the
kernels against an independent statement at 1e6 rays (tests/test_gpu_scene_walk.py).  Here the walk itself is checked: bit for
bit against the Python replays (scene_np, and baffle_np / beam_np / wallpatch_np for the scenes with one part only) at the sizes
the GPU suites replay, against the oracle's own trace for the empty scene, for any thread count and any cut of the range, and
under AddressSanitizer / UBSan as a stand-alone program (tests/native/scene_walk_main.c; nothing is preloaded).

The contract's ties -- clauses a random trace never meets -- are built here (tie_cases) from the oracle's own first segment and
the degenerate beam, each with its premise asserted in float64 numpy, evaluated with the contract's own expression:
  rim, inclusive        "hit iff ... <= r2":  the pencil's first segment crosses a disc's plane exactly on its rim
  equal f, lowest k     two discs struck at bitwise the same f
  cap bound, inclusive  ">= min_dot":  the first strike lies exactly on a cap's bound; and the overlap rule on that point
  coplanar discs        a ray re-emitted from one disc starts within a rounding error of the other's plane: the sign of s_p is
                        rounding noise, and decides whether the next segment "crosses" at f ~ 1e-17 (a parity scene)

A case that cannot be built: "s_q == 0" with the crossing inside a disc.  A disc must lie strictly inside the cavity and q lies
on the wall (or the world box), so q is never in a served disc's plane within its radius.  Nobody needs to look for it again.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import baffle_np
import beam_np
import scene_np as SC
import wallpatch_np
from test_gpu_scene import PARITY, PARITY_IDS, _case, _replayed
from test_scene_cpu import parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345
f64 = np.float64


def same(a, b):
    """two results of replay() / scene_walk(): every key of b, bit for bit"""
    for k, v in b.items():
        if isinstance(v, np.ndarray):
            assert a[k].dtype == v.dtype and a[k].shape == v.shape and np.array_equal(a[k], v), k
        else:
            assert a[k] == v, k


# ---------------------------------------------------------------- the walk against the replay of the composed contract
EDGES = [("led_first_in", 4), ("led_first_in", 7), ("black", None), ("white", None), ("black_spot", None), ("in_plane", None),
         ("full", None)]
N_EDGE = 5000


@pytest.mark.parametrize("name,n,rho,first", PARITY, ids=PARITY_IDS)
def test_walk_equals_the_replay(orc, name, n, rho, first):
    """every scene of SCENES, the first_ray = 2^32 + 7 case and reflectance 0.99, at the sizes of test_gpu_scene.py"""
    oc, spec = _case(orc, name, rho)
    rep = _replayed(orc, name, n, SEED, first, rho)
    w = orc.scene_walk(oc, SC.spec_of(spec), n, SEED, first)
    same(w, rep)
    assert int(rep["baffle_arrivals"].sum()) + int(rep["patch_arrivals"].sum()) == rep["census"]["wall_hits"] > n


@pytest.mark.parametrize("name,max_points", EDGES)
def test_walk_equals_the_replay_at_the_edges(orc, name, max_points):
    oc, spec = _case(orc, name, max_points=max_points)
    rep = _replayed(orc, name, N_EDGE, max_points=max_points)
    same(orc.scene_walk(oc, SC.spec_of(spec), N_EDGE, SEED), rep)
    if max_points is not None:
        assert rep["suspended_after_baffle"] >= 1 and rep["suspended_after_patch"] >= 1


# ---------------------------------------------------------------- one part only: the replay of that part
N_PART = 2000


def _ocfg(orc, rho=0.95):
    c = orc.default_config()
    c.reflectance = rho
    return c


def test_walk_with_only_baffles_is_the_baffle_replay(orc):
    import altair_raytracing_amd as isx
    icfg = isx.default_config()
    two = baffle_np.spec_of(isx.baffle_spec(icfg, [parts(isx, icfg)["shield"], isx.baffle_disc(icfg, (0, 0, 0), (0, 0, 1), 25.0, 0.5)]))
    cfg = _ocfg(orc)
    ref = baffle_np.replay(cfg, two, N_PART, SEED)
    w = orc.scene_walk(cfg, {"beam": None, "baffles": two, "patches": []}, N_PART, SEED)
    for k in baffle_np.PER_RAY:
        assert np.array_equal(w[k], ref[k]), k
    assert np.array_equal(w["baffle_arrivals"], ref["arrivals"]) and np.array_equal(w["baffle_absorbed"], ref["absorbed"])
    assert w["census"] == ref["census"] and w["suspended_after_baffle"] == ref["suspended_after_baffle"]
    assert int(ref["arrivals"].sum()) > 100


def test_walk_with_only_patches_is_the_patch_replay(orc):
    import altair_raytracing_amd as isx
    icfg = isx.default_config()
    p = parts(isx, icfg)
    patches = wallpatch_np.spec_of(isx.wall_patch_spec(icfg, [p["det"], p["sample"]]))
    cfg = _ocfg(orc)
    arr, ab, census, status, npts = wallpatch_np.replay(cfg, patches, N_PART, SEED)
    w = orc.scene_walk(cfg, {"beam": None, "baffles": [], "patches": patches}, N_PART, SEED)
    assert np.array_equal(w["patch_arrivals"], arr) and np.array_equal(w["patch_absorbed"], ab)
    assert w["census"] == census and np.array_equal(w["status"], status) and np.array_equal(w["n_points"], npts)
    assert arr[:2].all()


@pytest.mark.parametrize("name", ["led", "lamp"])
def test_walk_with_only_a_beam_is_the_beam_replay(orc, name):
    import altair_raytracing_amd as isx
    beam = beam_np.spec_of(parts(isx, isx.default_config())[name])
    cfg = _ocfg(orc)
    sp, sv, status, npts, lp, d, kind0, census = beam_np.replay(cfg, beam, N_PART, SEED)
    w = orc.scene_walk(cfg, {"beam": beam, "baffles": [], "patches": []}, N_PART, SEED)
    for key, ref in (("start_point", sp), ("start_dir", sv), ("status", status), ("n_points", npts), ("last_point", lp),
                     ("direction", d), ("first_kind", kind0)):
        assert np.array_equal(w[key], ref), key
    assert w["census"] == census


# ---------------------------------------------------------------- the empty scene, threads, cuts
N_BIG = 100_000


@pytest.fixture(scope="module")
def photometer_big(orc):
    """`photometer` walked at 1e5 rays on 16 threads: computed once, shared, never changed"""
    oc, spec = _case(orc, "photometer")
    return orc.scene_walk(oc, SC.spec_of(spec), N_BIG, SEED, nthreads=16)


def test_the_default_scene_is_the_oracles_trace(orc):
    """no baffle, no patch, the pencil (as the configuration states it and as the degenerate beam of the default spec) at 1e5
    rays: isxo_trace_endstates' four arrays and isxo_fluxmap's census"""
    import altair_raytracing_amd as isx
    cfg = _ocfg(orc)
    st, npts, lp, d = orc.trace_endstates(cfg, N_BIG, SEED)
    _, ost = orc.fluxmap(cfg, N_BIG, SEED, nthreads=16)
    empty = SC.spec_of(isx.default_scene_spec(isx.default_config()))
    for sc in ({"beam": None, "baffles": [], "patches": []}, empty):
        w = orc.scene_walk(cfg, sc, N_BIG, SEED)
        assert np.array_equal(w["status"], st) and np.array_equal(w["n_points"], npts)
        assert np.array_equal(w["last_point"], lp) and np.array_equal(w["direction"], d)
        assert (w["last_baffle"] == -1).all() and not w["baffle_arrivals"].any() and w["rays_baffle_to_baffle"] == 0
        assert np.array_equal(w["start_point"], np.tile([-60.0, 0.0, -75.0], (N_BIG, 1)))
        assert np.array_equal(w["start_dir"], np.tile([1.0, 0.0, 0.0], (N_BIG, 1)))
        for f in SC.CENSUS_FIELDS:
            assert w["census"][f] == getattr(ost, f), f
        assert int(w["patch_arrivals"].sum()) == ost.wall_hits and int(w["patch_absorbed"].sum()) == ost.absorbed
    assert len(set(st.tolist())) >= 2 and ost.counted_below_z > 1000


def test_one_thread_is_sixteen(orc, photometer_big):
    oc, spec = _case(orc, "photometer")
    same(orc.scene_walk(oc, SC.spec_of(spec), N_BIG, SEED, nthreads=1), photometer_big)
    assert photometer_big["census"]["launched"] == N_BIG


def test_a_range_cut_in_three_is_the_whole(orc, photometer_big):
    """three walks at consecutive first_ray: the per-ray arrays concatenate and every total adds up"""
    oc, spec = _case(orc, "photometer")
    cuts = [(0, 33_333), (33_333, 40_001), (73_334, 26_666)]
    part = [orc.scene_walk(oc, SC.spec_of(spec), n, SEED, first) for first, n in cuts]
    for k in SC.PER_RAY:
        assert np.array_equal(np.concatenate([p[k] for p in part]), photometer_big[k]), k
    for k in SC.COUNTERS:
        assert np.array_equal(sum(p[k] for p in part), photometer_big[k]), k
    for f in SC.CENSUS_FIELDS:
        assert sum(p["census"][f] for p in part) == photometer_big["census"][f], f
    for k in ("suspended_after_baffle", "suspended_after_patch", "rays_baffle_to_baffle"):
        assert sum(p[k] for p in part) == photometer_big[k], k


def test_outside_the_replays_scope_is_an_error(orc):
    """the chord mode, the other borders and the BRDF source are not walked: an error code, as isxo_* return them"""
    for field, value in (("trace_mode", 1), ("lambertian", 0), ("surface_model", 1), ("source_model", 1)):
        c = _ocfg(orc)
        setattr(c, field, value)
        rc = orc.lib().isxo_scene_walk(C.byref(c), None, None, None, 10, SEED, 0, None, None, 1)
        assert rc == -2, field
    assert orc.lib().isxo_scene_walk(C.byref(_ocfg(orc)), None, None, None, 10, SEED, 0, None, None, 1) == 0


# ---------------------------------------------------------------- the contract's ties
TIE_COUNTS = (64, 769)
N_COPLANAR = 5000
LAMP = {"origin": (0.0, 0.0, 20.0), "axis": (0.0, 0.0, 1.0), "e1": (1.0, 0.0, 0.0), "e2": (0.0, 1.0, 0.0), "radius": 0.0,
        "cos_min": -1.0, "law": 0}


def seg(p, q, disc):
    """the contract's expressions for one disc on the segment p -> q in float64 numpy, left to right: (s_p, s_q, f, x, |d|^2, r2)"""
    c, m, radius, _ = disc
    p, q, c, m = (np.array(a, dtype=f64) for a in (p, q, c, m))
    sp = ((p[0] - c[0]) * m[0] + (p[1] - c[1]) * m[1]) + (p[2] - c[2]) * m[2]
    sq = ((q[0] - c[0]) * m[0] + (q[1] - c[1]) * m[1]) + (q[2] - c[2]) * m[2]
    f = sp / (sp - sq)
    x = np.array([p[k] + f * (q[k] - p[k]) for k in range(3)])
    d = x - c
    return sp, sq, f, x, (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], f64(radius) * f64(radius)


def cap_dot(q, axis):
    return (f64(q[0]) * f64(axis[0]) + f64(q[1]) * f64(axis[1])) + f64(q[2]) * f64(axis[2])


def tie_cases(orc):
    """name -> (cfg, scene, pencil): the oracle's configuration, the scene dict, and whether the source is the pencil of cfg (then
    the specialised calls take the case too).  Every premise is asserted here, on the oracle's own first segment."""
    out = {}
    # --- the default pencil (-60, 0, -75) along +x; q0 its first strike
    c = orc.default_config()
    c.reflectance = 0.95
    p0 = (-60.0, 0.0, -75.0)
    kind, q0 = orc.next_boundary(c, p0, (1.0, 0.0, 0.0), 0)
    assert kind == SC.K_INNER and q0[1] == 0.0 and q0[2] == -75.0
    # (the pencil comes from the side the normal (1, 0, 0) points away from: s_p = -60 < 0, side 1 by the header's rule; rim_facing
    # is the same disc with the normal turned towards the source, struck on side 0)
    for name, radius, mx in (("rim", 8.0, 1.0), ("rim_short", float(np.nextafter(8.0, 0.0)), 1.0), ("rim_facing", 8.0, -1.0)):
        disc = ((0.0, 0.0, -67.0), (mx, 0.0, 0.0), radius, 0.0)
        sp, sq, f, x, dd, r2 = seg(p0, q0, disc)
        assert sp * mx < 0 < sq * mx and dd == 64.0, (sp, sq, dd)
        assert (r2 < 64.0 and not dd <= r2) if name == "rim_short" else (r2 == 64.0 and dd <= r2)
        out[name] = (c, {"beam": None, "baffles": [disc], "patches": []}, True)
    qx = float(q0[0])
    assert cap_dot(q0, (1.0, 0.0, 0.0)) == qx      # dq == min_dot: (q.x * 1 + 0 * 0) + q.z * 0 is q.x
    up = float(np.nextafter(qx, np.inf))
    assert not cap_dot(q0, (1.0, 0.0, 0.0)) >= up
    out["cap"] = (c, {"beam": None, "baffles": [], "patches": [((1.0, 0.0, 0.0), qx, 0.0)]}, True)
    out["cap_short"] = (c, {"beam": None, "baffles": [], "patches": [((1.0, 0.0, 0.0), up, 0.0)]}, True)
    # the overlap rule on the same point: both caps hold q0 (the second, about (0.6, 0, -0.8), well inside its bound)
    other = (0.6, 0.0, -0.8)
    assert cap_dot(q0, other) >= 90.0
    out["cap_black_first"] = (c, {"beam": None, "baffles": [], "patches": [((1.0, 0.0, 0.0), qx, 0.0), (other, 90.0, 1.0)]}, True)
    out["cap_white_first"] = (c, {"beam": None, "baffles": [], "patches": [(other, 90.0, 1.0), ((1.0, 0.0, 0.0), qx, 0.0)]}, True)
    # --- a pencil along -z from (0, 0, 20) through the common centre of two discs: the wall is black, so that no ray comes back
    cz = orc.default_config()
    cz.reflectance = 0.0
    cz.src[0], cz.src[1], cz.src[2] = 0.0, 0.0, 20.0
    cz.dir[0], cz.dir[1], cz.dir[2] = 0.0, 0.0, -1.0
    down = {"origin": (0.0, 0.0, 20.0), "axis": (0.0, 0.0, -1.0), "e1": (1.0, 0.0, 0.0), "e2": (0.0, -1.0, 0.0), "radius": 0.0,
            "cos_min": 1.0, "law": 0}
    sp_, sv_ = beam_np.sample(down, 3, SEED)
    assert np.array_equal(sp_, np.tile([0.0, 0.0, 20.0], (3, 1))) and np.array_equal(sv_, np.tile([0.0, 0.0, -1.0], (3, 1)))
    _, qz = orc.next_boundary(cz, (0.0, 0.0, 20.0), (0.0, 0.0, -1.0), 0)
    black = ((0.0, 0.0, -10.0), (0.6, 0.0, 0.8), 10.0, 0.0)
    white = ((0.0, 0.0, -10.0), (-0.6, 0.0, 0.8), 10.0, 1.0)
    a, b = seg((0.0, 0.0, 20.0), qz, black), seg((0.0, 0.0, 20.0), qz, white)
    assert a[0] > 0 > a[1] and b[0] > 0 > b[1] and a[4] <= a[5] and b[4] <= b[5]
    assert a[2].tobytes() == b[2].tobytes(), (a[2], b[2])      # f_0 == f_1, bitwise
    for name, discs in (("equal_f", [black, white]), ("equal_f_swapped", [white, black])):
        out[name] = (cz, {"beam": None, "baffles": discs, "patches": []}, True)
        out[name + "_beam"] = (cz, {"beam": down, "baffles": discs, "patches": []}, False)
    return out


COPLANAR = ["same-normal", "negated-normal", "tilted"]


def coplanar(orc, variant):
    """(cfg, scene): two discs in one plane about one centre, radii 10 and 25, under the lamp.  same-normal: the plane z = 0.1,
    normal (0, 0, 1); negated-normal: disc 1's normal negated; tilted: both normals (0.6, 0, 0.8) about (0.1, 0, 0.1) -- with an
    axis-aligned normal the products of s_p are exact and a contracted multiply-add changes nothing; here it changes the sign of
    the rounding error.  (In the plane z = 0 the crossing below happens too, for 11 rays in 5000; z = 0.1 is not representable.)"""
    c = orc.default_config()
    c.reflectance = 0.95
    m0 = (0.6, 0.0, 0.8) if variant == "tilted" else (0.0, 0.0, 1.0)
    m1 = (0.0, 0.0, -1.0) if variant == "negated-normal" else m0
    centre = (0.1, 0.0, 0.1) if variant == "tilted" else (0.0, 0.0, 0.1)
    return c, {"beam": dict(LAMP), "baffles": [(centre, m0, 10.0, 0.9), (centre, m1, 25.0, 0.5)], "patches": []}


def expect_tie(name, w, n):
    """what the contract says of a tie case, on a result of the walk (or anything equal to it)"""
    st, npts, ba, bb, pa, pb = (w[k] for k in ("status", "n_points", "baffle_arrivals", "baffle_absorbed", "patch_arrivals",
                                              "patch_absorbed"))
    name = name[:-5] if name.endswith("_beam") else name
    if name in ("rim", "rim_facing", "equal_f"):      # every ray is absorbed on disc 0 at its first interaction
        side = 1 if name == "rim" else 0
        assert (st == 2).all() and (npts == 2).all() and (w["last_baffle"] == side).all() and (w["first_kind"] == -2).all()
        assert ba[0, side] == bb[0, side] == n and int(ba.sum()) == n
    elif name == "rim_short":           # the radius one ulp short: no ray's first interaction is on the disc
        assert (w["first_kind"] != -2).all() and (w["first_class"] != -2).all()
    elif name == "equal_f_swapped":     # the white disc is struck, absorbs nothing and, the wall being black, is never met again
        assert (w["first_kind"] == -2).all() and ba[0, 0] == n and ba[0, 1] == 0 and not bb[0].any()
    elif name in ("cap", "cap_black_first"):
        assert (st == 2).all() and (npts == 2).all() and (w["last_class"] == 0).all() and pa[0] == pb[0] == n
    elif name == "cap_short":           # the bound one ulp above q.x: class 0 has no arrival from a first segment
        assert (w["first_class"] != 0).all() and (w["first_class"] == 1).all()
    elif name == "cap_white_first":     # the lowest index wins: the white cap takes every first strike and absorbs nothing
        assert (w["first_class"] == 0).all() and pa[0] >= n and pb[0] == 0
    else:
        raise KeyError(name)


TIES = ["rim", "rim_short", "rim_facing", "cap", "cap_short", "cap_black_first", "cap_white_first", "equal_f", "equal_f_swapped", "equal_f_beam",
        "equal_f_swapped_beam"]


@pytest.mark.parametrize("n", TIE_COUNTS)
@pytest.mark.parametrize("name", TIES)
def test_ties_walk_equals_the_replay(orc, name, n):
    cfg, scene, _ = tie_cases(orc)[name]
    w = orc.scene_walk(cfg, scene, n, SEED)
    expect_tie(name, w, n)
    same(w, SC.replay(cfg, scene, n, SEED, workers=1))


@pytest.mark.parametrize("variant", COPLANAR)
def test_coplanar_discs_walk_equals_the_replay(orc, variant):
    """the rounding-sign crossing: at least 100 rays whose interaction on one disc directly follows one on the other"""
    cfg, scene = coplanar(orc, variant)
    w = orc.scene_walk(cfg, scene, N_COPLANAR, SEED)
    print("coplanar,", variant, "rays from disc to disc:", w["rays_baffle_to_baffle"], "arrivals", w["baffle_arrivals"].tolist())
    assert w["rays_baffle_to_baffle"] >= 100 and int(w["baffle_arrivals"].min()) >= 100
    same(w, SC.replay(cfg, scene, N_COPLANAR, SEED))


# ---------------------------------------------------------------- the stand-alone program under the sanitizers
def test_the_walk_is_clean_under_the_sanitizers(orc, tmp_path):
    """isx_oracle.c + tests/native/scene_walk_main.c compiled with AddressSanitizer and UBSan and run as a child process: exit
    status 0, and the census it prints for `photometer` and the coplanar scene (2000 rays, 1 and 4 threads) is the library's"""
    exe = str(tmp_path / "scene_walk_main")
    src = [os.path.join(ROOT, "oracle", "isx_oracle.c"), os.path.join(ROOT, "tests", "native", "scene_walk_main.c")]
    # (gcc by name: the flags that link the sanitizers' runtimes statically are gcc's, whatever CC says)
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-ffp-contract=off", "-mfma", "-msse4.1", "-fopenmp", "-D_GNU_SOURCE",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "oracle"),
                           "-o", exe] + src + ["-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    oc, spec = _case(orc, "photometer")
    want = []
    for name, (cfg, scene) in (("photometer", (oc, SC.spec_of(spec))), ("coplanar", coplanar(orc, "same-normal"))):
        w = orc.scene_walk(cfg, scene, 2000, SEED)
        for nt in (1, 4):
            want.append("%s threads %d: " % (name, nt) + " ".join("%s %d" % (f, w["census"][f]) for f in SC.CENSUS_FIELDS)
                        + " counters %d baffle_to_baffle %d" % (int(SC.counter_words(w).sum()), w["rays_baffle_to_baffle"]))
    assert r.stdout.splitlines() == want, r.stdout
