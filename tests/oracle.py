"""ctypes binding of the CPU oracle (oracle/libisx_oracle.so) — TEST INFRASTRUCTURE.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this
module.  The product package never does.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(_HERE), "oracle")
ORACLE_SO = os.path.join(ORACLE_DIR, "libisx_oracle.so")


class Config(C.Structure):
    """Same layout as isx_config (include/isx.h) and isxo_config (oracle/isx_oracle.h)."""

    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved0", C.c_uint32),
        ("r_in", C.c_double), ("r_out", C.c_double), ("theta_max_deg", C.c_double),
        ("reflectance", C.c_double), ("roughness_rad", C.c_double), ("box_half", C.c_double),
        ("lambertian", C.c_int32), ("max_points", C.c_int32),
        ("src", C.c_double * 3), ("dir", C.c_double * 3),
        ("n_theta", C.c_int32), ("n_phi", C.c_int32),
        ("det_diameter", C.c_double), ("det_distance", C.c_double), ("exit_port_z", C.c_double),
        ("source_model", C.c_int32), ("surface_model", C.c_int32),
        ("brdf", C.c_double * 3),
        ("hit_line_mode", C.c_int32), ("trace_mode", C.c_int32),
    ]

    def copy(self):
        c = Config()
        C.memmove(C.byref(c), C.byref(self), C.sizeof(Config))
        return c


class Stats(C.Structure):
    _fields_ = [
        ("launched", C.c_uint64), ("exited", C.c_uint64), ("counted_below_z", C.c_uint64),
        ("absorbed", C.c_uint64), ("suspended", C.c_uint64), ("bin_increments", C.c_uint64),
        ("wall_hits", C.c_uint64), ("t_kernel_ms", C.c_double),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BeamSpec(C.Structure):
    """Layout twins of isx_beam_spec, isx_baffle_spec, isx_wall_patch_spec and isx_scene_counts (isxo_* in oracle/isx_oracle.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("origin", C.c_double * 3), ("axis", C.c_double * 3),
                ("e1", C.c_double * 3), ("e2", C.c_double * 3), ("radius", C.c_double), ("cos_min", C.c_double),
                ("angular_law", C.c_int32), ("reserved1", C.c_int32)]


class Baffle(C.Structure):
    _fields_ = [("centre", C.c_double * 3), ("normal", C.c_double * 3), ("radius", C.c_double), ("reflectance", C.c_double)]


class BaffleSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("n_baffles", C.c_int32), ("reserved1", C.c_int32),
                ("baffle", Baffle * 4)]


class WallPatch(C.Structure):
    _fields_ = [("axis", C.c_double * 3), ("min_dot", C.c_double), ("reflectance", C.c_double)]


class WallPatchSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("n_patches", C.c_int32), ("reserved1", C.c_int32),
                ("patch", WallPatch * 8)]


class SceneRays(C.Structure):
    _fields_ = [("status", C.POINTER(C.c_int32)), ("n_points", C.POINTER(C.c_int32)),
                ("last_point", C.POINTER(C.c_double)), ("direction", C.POINTER(C.c_double)),
                ("start_point", C.POINTER(C.c_double)), ("start_dir", C.POINTER(C.c_double)),
                ("last_baffle", C.POINTER(C.c_int32)), ("last_class", C.POINTER(C.c_int32)),
                ("first_class", C.POINTER(C.c_int32)), ("first_kind", C.POINTER(C.c_int32))]


class SceneTotals(C.Structure):
    _fields_ = [("patch_arrivals", C.c_uint64 * 10), ("patch_absorbed", C.c_uint64 * 10),
                ("baffle_arrivals", (C.c_uint64 * 2) * 4), ("baffle_absorbed", (C.c_uint64 * 2) * 4),
                ("census", Stats), ("suspended_after_baffle", C.c_uint64), ("suspended_after_patch", C.c_uint64),
                ("rays_baffle_to_baffle", C.c_uint64)]


_lib = None


def build():
    subprocess.check_call(["make", "-s", "-C", ORACLE_DIR])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(ORACLE_SO) or os.path.getmtime(ORACLE_SO) < os.path.getmtime(
            os.path.join(ORACLE_DIR, "isx_oracle.c")
        ):
            build()
        L = C.CDLL(ORACLE_SO)
        u64, i32, dbl = C.c_uint64, C.c_int32, C.c_double
        P = C.POINTER
        L.isxo_default_config.argtypes = [P(Config)]
        L.isxo_default_config.restype = None
        L.isxo_philox4x32_10.argtypes = [P(C.c_uint32), P(C.c_uint32), P(C.c_uint32)]
        L.isxo_philox4x32_10.restype = None
        L.isxo_u01.argtypes = [C.c_uint32]
        L.isxo_u01.restype = dbl
        L.isxo_log.argtypes = [dbl]
        L.isxo_log.restype = dbl
        L.isxo_sincos2pi.argtypes = [dbl, P(dbl), P(dbl)]
        L.isxo_sincos2pi.restype = None
        L.isxo_circle_point.argtypes = [dbl, P(dbl), P(dbl)]
        L.isxo_circle_point.restype = None
        L.isxo_sincos.argtypes = [dbl, P(dbl), P(dbl)]
        L.isxo_sincos.restype = None
        L.isxo_detector_table.argtypes = [P(Config), P(dbl)]
        L.isxo_check_intersection.argtypes = [P(dbl), dbl, P(dbl), P(dbl)]
        L.isxo_trace_endstates.argtypes = [P(Config), u64, u64, u64, P(i32), P(i32), P(dbl), P(dbl)]
        L.isxo_fluxmap.argtypes = [P(Config), u64, u64, u64, P(u64), P(Stats), C.c_int]
        L.isxo_bin_lines.argtypes = [P(Config), P(dbl), u64, P(u64), C.c_int]
        L.isxo_disc_sweep.argtypes = [P(Config), P(dbl), i32, dbl, dbl, u64, u64, u64, P(u64), P(Stats), C.c_int]
        L.isxo_bin_segments.argtypes = [P(dbl), i32, dbl, dbl, P(dbl), u64, P(u64), C.c_int]
        L.isxo_exit_segments.argtypes = [P(Config), u64, u64, u64, P(i32), P(dbl)]
        L.isxo_disc_sweep_per_position.argtypes = [P(Config), P(dbl), i32, dbl, dbl, u64, u64, u64, P(u64), P(Stats), C.c_int]
        L.isxo_exit_dz_hist.argtypes = [P(Config), u64, u64, u64, i32, P(u64), P(Stats), C.c_int]
        L.isxo_fluxmap_per_position.argtypes = [P(Config), u64, i32, u64, u64, u64, u64, P(u64), P(Stats), C.c_int]
        L.isxo_trace_rays_detector.argtypes = [P(Config), P(dbl), dbl, u64, u64, u64, P(u64), P(Stats)]
        L.isxo_exit_directions.argtypes = [P(Config), u64, u64, u64, u64, P(u64), P(dbl), P(u64)]
        L.isxo_max_threads.restype = C.c_int
        L.isxo_next_boundary.argtypes = [P(Config), P(dbl), P(dbl), C.c_int, P(dbl), P(dbl)]
        L.isxo_surface_normal.argtypes = [P(Config), C.c_int, P(dbl), P(dbl)]
        L.isxo_cosine_emission.argtypes = [P(Config), C.c_int, P(dbl), C.c_uint32, C.c_uint32, P(dbl)]
        L.isxo_scene_walk.argtypes = [P(Config), P(BeamSpec), P(BaffleSpec), P(WallPatchSpec), u64, u64, u64, P(SceneRays),
                                      P(SceneTotals), C.c_int]
        _lib = L
    return _lib


def default_config():
    c = Config()
    lib().isxo_default_config(C.byref(c))
    return c


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def philox(ctr, key):
    c = (C.c_uint32 * 4)(*ctr)
    k = (C.c_uint32 * 2)(*key)
    o = (C.c_uint32 * 4)()
    lib().isxo_philox4x32_10(c, k, o)
    return list(o)


def sincos2pi(u):
    s, c = C.c_double(), C.c_double()
    lib().isxo_sincos2pi(u, C.byref(s), C.byref(c))
    return s.value, c.value


def circle_point(u):
    c, s = C.c_double(), C.c_double()
    lib().isxo_circle_point(u, C.byref(c), C.byref(s))
    return c.value, s.value


def sincos(x):
    s, c = C.c_double(), C.c_double()
    lib().isxo_sincos(x, C.byref(s), C.byref(c))
    return s.value, c.value


def next_boundary(cfg, p, v, on, with_direction=False):
    """(kind, point) of the next boundary from p along v for a ray sitting on boundary `on` (isxo_next_boundary);
    with_direction: also the direction the step was taken along (the unit vector of v once the ray leaves rule S1')."""
    P3, V3, Q3, W3 = (C.c_double * 3)(*p), (C.c_double * 3)(*v), (C.c_double * 3)(), (C.c_double * 3)()
    kind = lib().isxo_next_boundary(C.byref(cfg), P3, V3, int(on), Q3, W3)
    if with_direction:
        return kind, np.array(Q3[:]), np.array(W3[:])
    return kind, np.array(Q3[:])


def surface_normal(cfg, kind, q):
    Q3, N3 = (C.c_double * 3)(*q), (C.c_double * 3)()
    assert lib().isxo_surface_normal(C.byref(cfg), int(kind), Q3, N3) == 0
    return np.array(N3[:])


def cosine_emission(cfg, kind, q, wa, wb):
    """interact()'s cosine emission from surface point q for the two Philox words of an interaction (r_in s - q, un-normalised,
    on the inner sphere, kind 1; the unit vector of n + s elsewhere)"""
    Q3, W3 = (C.c_double * 3)(*q), (C.c_double * 3)()
    assert lib().isxo_cosine_emission(C.byref(cfg), int(kind), Q3, int(wa), int(wb), W3) == 0
    return np.array(W3[:])


def check_intersection(det, width, last_point, direction):
    D6, L3, V3 = (C.c_double * 6)(*det), (C.c_double * 3)(*last_point), (C.c_double * 3)(*direction)
    return int(lib().isxo_check_intersection(D6, float(width), L3, V3))


def detector_table(cfg):
    out = np.zeros((cfg.n_theta * cfg.n_phi, 6), dtype=np.float64)
    rc = lib().isxo_detector_table(C.byref(cfg), _p(out, C.c_double))
    assert rc == 0, rc
    return out


def trace_endstates(cfg, n, seed, first=0):
    status = np.zeros(n, dtype=np.int32)
    npts = np.zeros(n, dtype=np.int32)
    lp = np.zeros((n, 3), dtype=np.float64)
    d = np.zeros((n, 3), dtype=np.float64)
    rc = lib().isxo_trace_endstates(C.byref(cfg), n, seed, first, _p(status, C.c_int32), _p(npts, C.c_int32),
                                    _p(lp, C.c_double), _p(d, C.c_double))
    assert rc == 0, rc
    return status, npts, lp, d


def fluxmap(cfg, n, seed, first=0, nthreads=0):
    hits = np.zeros(cfg.n_theta * cfg.n_phi, dtype=np.uint64)
    st = Stats()
    rc = lib().isxo_fluxmap(C.byref(cfg), n, seed, first, _p(hits, C.c_uint64), C.byref(st), nthreads)
    assert rc == 0, rc
    return hits.reshape(cfg.n_theta, cfg.n_phi), st


def bin_lines(cfg, P, V, nthreads=0):
    """-> hits[n_theta, n_phi]: isxo_check_intersection of the lines (P[k], V[k]) against every bin, in table order."""
    lines = np.ascontiguousarray(np.concatenate([np.asarray(P, dtype=np.float64).reshape(-1, 3),
                                                 np.asarray(V, dtype=np.float64).reshape(-1, 3)], axis=1))
    hits = np.zeros(cfg.n_theta * cfg.n_phi, dtype=np.uint64)
    rc = lib().isxo_bin_lines(C.byref(cfg), _p(lines, C.c_double), lines.shape[0], _p(hits, C.c_uint64), nthreads)
    assert rc == 0, rc
    return hits.reshape(cfg.n_theta, cfg.n_phi)


def disc_sweep(cfg, centers_axes, radius, half_thick, n, seed, first=0, nthreads=0):
    ca = np.ascontiguousarray(centers_axes, dtype=np.float64)
    nd = ca.shape[0]
    hits = np.zeros(nd, dtype=np.uint64)
    st = Stats()
    rc = lib().isxo_disc_sweep(C.byref(cfg), _p(ca, C.c_double), nd, radius, half_thick, n, seed, first,
                               _p(hits, C.c_uint64), C.byref(st), nthreads)
    assert rc == 0, rc
    return hits, st


def bin_segments(centers_axes, radius, half_thick, segments, nthreads=0):
    """-> hits[n_disc]: the sweep's own segment_hits_tube of every segment[7] (start, direction, tmax) against every disc."""
    ca = np.ascontiguousarray(centers_axes, dtype=np.float64).reshape(-1, 6)
    seg = np.ascontiguousarray(segments, dtype=np.float64).reshape(-1, 7)
    hits = np.zeros(ca.shape[0], dtype=np.uint64)
    if nthreads <= 0 and seg.shape[0] * ca.shape[0] <= 1 << 16:
        nthreads = 1                                            # (a handful of tests: not worth a team of threads)
    rc = lib().isxo_bin_segments(_p(ca, C.c_double), ca.shape[0], radius, half_thick, _p(seg, C.c_double), seg.shape[0],
                                 _p(hits, C.c_uint64), nthreads)
    assert rc == 0, rc
    return hits


def exit_segments(cfg, n, seed, first=0):
    """-> (status[n], segments[n, 7]): what isxo_disc_sweep tests of every ray (zeros where the ray did not exit)"""
    status = np.zeros(n, dtype=np.int32)
    seg = np.zeros((n, 7), dtype=np.float64)
    rc = lib().isxo_exit_segments(C.byref(cfg), n, seed, first, _p(status, C.c_int32), _p(seg, C.c_double))
    assert rc == 0, rc
    return status, seg


def disc_sweep_per_position(cfg, centers_axes, radius, half_thick, rpp, seed, first=0, nthreads=0):
    ca = np.ascontiguousarray(centers_axes, dtype=np.float64)
    nd = ca.shape[0]
    hits = np.zeros(nd, dtype=np.uint64)
    st = Stats()
    rc = lib().isxo_disc_sweep_per_position(C.byref(cfg), _p(ca, C.c_double), nd, radius, half_thick, rpp, seed, first,
                                            _p(hits, C.c_uint64), C.byref(st), nthreads)
    assert rc == 0, rc
    return hits, st


def exit_dz_hist(cfg, n, seed, nbins=100, first=0, nthreads=0):
    hist = np.zeros(nbins, dtype=np.uint64)
    st = Stats()
    rc = lib().isxo_exit_dz_hist(C.byref(cfg), n, seed, first, nbins, _p(hist, C.c_uint64), C.byref(st), nthreads)
    assert rc == 0, rc
    return hist, st


def fluxmap_per_position(cfg, rays_per_position, seed, fold=1, first_group=0, n_groups=None, first=0, nthreads=0):
    nb = cfg.n_theta * cfg.n_phi
    if n_groups is None:
        n_groups = nb // fold - first_group
    hits = np.zeros(nb, dtype=np.uint64)
    st = Stats()
    rc = lib().isxo_fluxmap_per_position(C.byref(cfg), rays_per_position, fold, first_group, n_groups, seed, first,
                                         _p(hits, C.c_uint64), C.byref(st), nthreads)
    assert rc == 0, rc
    return hits.reshape(cfg.n_theta, cfg.n_phi), st


def trace_rays_detector(cfg, detector, width, n, seed, first=0):
    det = np.ascontiguousarray(detector, dtype=np.float64).reshape(6)
    h = C.c_uint64(0)
    st = Stats()
    rc = lib().isxo_trace_rays_detector(C.byref(cfg), _p(det, C.c_double), width, n, seed, first, C.byref(h), C.byref(st))
    assert rc == 0, rc
    return int(h.value), st


def exit_directions(cfg, n, seed, first=0, capacity=None):
    cap = capacity or n
    ids = np.zeros(cap, dtype=np.uint64)
    d = np.zeros((cap, 3), dtype=np.float64)
    cnt = C.c_uint64(0)
    rc = lib().isxo_exit_directions(C.byref(cfg), n, seed, first, cap, _p(ids, C.c_uint64), _p(d, C.c_double), C.byref(cnt))
    assert rc == 0, rc
    k = min(int(cnt.value), cap)
    return ids[:k], d[:k], int(cnt.value)


WALK_THREADS = 16      # (the walk's default: a fixed number, not the machine's core count)


def scene_walk(cfg, scene, n, seed, first=0, nthreads=None):
    """The scene of scene_np.spec_of() -- {"beam": a beam_np spec or None (the pencil of cfg), "baffles": [(centre, normal,
    radius, reflectance)], "patches": [(axis, min_dot, reflectance)]} -- walked natively by isxo_scene_walk.  -> the dict of
    scene_np.replay(): the per-ray arrays, patch_arrivals / patch_absorbed [P + 2], baffle_arrivals / baffle_absorbed [K, 2]
    (K = max(len(baffles), 1)), the census dict, suspended_after_baffle / suspended_after_patch; and one key more,
    rays_baffle_to_baffle: the rays with a baffle interaction that directly follows one on ANOTHER baffle."""
    beam, baffles, patches = scene.get("beam"), list(scene.get("baffles") or ()), list(scene.get("patches") or ())
    assert len(baffles) <= 4 and len(patches) <= 8
    bs = None
    if beam is not None:
        bs = BeamSpec()
        bs.struct_size = C.sizeof(BeamSpec)
        for k in ("origin", "axis", "e1", "e2"):
            setattr(bs, k, (C.c_double * 3)(*[float(x) for x in beam[k]]))
        bs.radius, bs.cos_min, bs.angular_law = float(beam["radius"]), float(beam["cos_min"]), int(beam["law"])
    fs = BaffleSpec()
    fs.struct_size, fs.n_baffles = C.sizeof(BaffleSpec), len(baffles)
    for k, (centre, normal, radius, rho) in enumerate(baffles):
        fs.baffle[k].centre = (C.c_double * 3)(*[float(x) for x in centre])
        fs.baffle[k].normal = (C.c_double * 3)(*[float(x) for x in normal])
        fs.baffle[k].radius, fs.baffle[k].reflectance = float(radius), float(rho)
    ws = WallPatchSpec()
    ws.struct_size, ws.n_patches = C.sizeof(WallPatchSpec), len(patches)
    for k, (axis, min_dot, rho) in enumerate(patches):
        ws.patch[k].axis = (C.c_double * 3)(*[float(x) for x in axis])
        ws.patch[k].min_dot, ws.patch[k].reflectance = float(min_dot), float(rho)
    out = {k: np.zeros(n, dtype=np.int32) for k in ("status", "n_points", "last_baffle", "last_class", "first_class", "first_kind")}
    out.update({k: np.zeros((n, 3), dtype=np.float64) for k in ("last_point", "direction", "start_point", "start_dir")})
    rays = SceneRays()
    for k, a in out.items():
        setattr(rays, k, _p(a, C.c_double if a.dtype == np.float64 else C.c_int32))
    tot = SceneTotals()
    rc = lib().isxo_scene_walk(C.byref(cfg), None if bs is None else C.byref(bs), C.byref(fs), C.byref(ws), n, seed, first,
                               C.byref(rays), C.byref(tot), WALK_THREADS if nthreads is None else nthreads)
    assert rc == 0, rc
    P, K = len(patches), max(len(baffles), 1)
    out["patch_arrivals"] = np.array(tot.patch_arrivals[:P + 2], dtype=np.uint64)
    out["patch_absorbed"] = np.array(tot.patch_absorbed[:P + 2], dtype=np.uint64)
    out["baffle_arrivals"] = np.array([list(r) for r in tot.baffle_arrivals], dtype=np.uint64)[:K]
    out["baffle_absorbed"] = np.array([list(r) for r in tot.baffle_absorbed], dtype=np.uint64)[:K]
    out["census"] = {k: int(getattr(tot.census, k)) for k in ("launched", "exited", "counted_below_z", "absorbed", "suspended",
                                                              "wall_hits")}
    out["suspended_after_baffle"] = int(tot.suspended_after_baffle)
    out["suspended_after_patch"] = int(tot.suspended_after_patch)
    out["rays_baffle_to_baffle"] = int(tot.rays_baffle_to_baffle)
    return out
