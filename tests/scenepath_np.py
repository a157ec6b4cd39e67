"""The scene path histograms of include/isx.h (isx_scene_path_hist) restated -- TEST INFRASTRUCTURE.

Three pieces:
  replay()      the contract in Python: the walk of scene_np._replay_range (the same calls in the same order: beam_np.sample,
                oracle.next_boundary, baffle_np.segment, wallpatch_np.classify, oracle.philox, oracle.cosine_emission) with every
                track point kept, and from the track points the path length L of every ray by the contract's own expressions in
                numpy float64 -- per segment sqrt((d.x*d.x + d.y*d.y) + d.z*d.z), summed in order, the leg to the world box left
                out, the tail up to the port plane for a ray counted below z.  The fate slot is response_np.fates.
  walk()        the same in C (tests/native/scene_path_walk.c on the oracle's exported primitives), compiled on first use with
                gcc and the flags of oracle/Makefile, linked with oracle/isx_oracle.c, into tests/native/build/ (git-ignored).
                The 1e6-ray tests need it.
  from_rays()   (L, fate) -> hist, overflow, checksum; moments() and decay() are the two host helpers' formulas.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import baffle_np
import beam_np
import response_np as R
import scene_np as SC
import wallpatch_np

FATES, BAFFLE0, PORT, EXITED_OTHER, SUSPENDED = R.FATES, R.BAFFLE0, R.PORT, R.EXITED_OTHER, R.SUSPENDED
LIGHT_CM_PER_NS = 29.9792458
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
BUILD = os.path.join(NATIVE, "build")
WALK_C = os.path.join(NATIVE, "scene_path_walk.c")
ORACLE_C = os.path.join(ROOT, "oracle", "isx_oracle.c")
WALK_SO = os.path.join(BUILD, "libscene_path_walk.so")
# oracle/Makefile's CFLAGS
CFLAGS = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-mfma", "-msse4.1", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter",
          "-D_GNU_SOURCE"]
f64 = np.float64


# ---------------------------------------------------------------- the contract's arithmetic
def seg_len(a, b):
    """s = sqrt((d.x*d.x + d.y*d.y) + d.z*d.z), d = b - a componentwise, in IEEE double"""
    dx, dy, dz = f64(b[0]) - f64(a[0]), f64(b[1]) - f64(a[1]), f64(b[2]) - f64(a[2])
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def path_of(points, status, exit_port_z):
    """L of a ray from its track points X_0 .. X_{n-1} and its status"""
    L = f64(0.0)
    last = len(points) - 1 if status != R.EXITED else len(points) - 2
    for i in range(1, last + 1):
        L = L + seg_len(points[i - 1], points[i])
    if status == R.EXITED and f64(points[-1][2]) < f64(exit_port_z):   # slot 18: the leg up to the port plane
        p, q = points[-2], points[-1]
        s = seg_len(p, q)
        with np.errstate(all="ignore"):
            f = (f64(exit_port_z) - f64(p[2])) / (f64(q[2]) - f64(p[2]))
        L = L + (s * f if (f > 0.0 and f <= 1.0) else f64(0.0))
    return L


def _replay_range(cfg_bytes, scene, lo, hi, seed, first):
    """rays [lo, hi) of a call: scene_np._replay_range's walk with the track points kept -> the per-ray arrays and L"""
    import oracle
    c = oracle.Config()
    C.memmove(C.byref(c), cfg_bytes, C.sizeof(oracle.Config))
    assert c.lambertian == 1 and c.surface_model == 0 and c.source_model == 0 and c.trace_mode == 0
    assert scene["beam"] is not None, "the path contract starts at the beam contract's start point"
    baffles, patches = scene["baffles"], scene["patches"]
    nb, P = len(baffles), len(patches)
    n = hi - lo
    sp, sv = beam_np.sample(scene["beam"], n, seed, first + lo)
    cfgs, thrs = [], []
    for k in range(P + 2):
        ck = c.copy()
        if k < P:
            ck.reflectance = patches[k][2]
        cfgs.append(ck)
        thrs.append(SC.rho_thr(ck.reflectance))
    bcfg, bthr, brm = [], [], []
    for (_, m, _, rho) in baffles:
        ck = c.copy()
        ck.reflectance = rho
        bcfg.append(ck)
        bthr.append(SC.rho_thr(rho))
        brm.append(tuple(f64(c.r_in) * f64(m[i]) for i in range(3)))
    status, n_points, last_baffle, last_class = (np.zeros(n, dtype=np.int32) for _ in range(4))
    lps, dirs, path = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    zero = (0.0, 0.0, 0.0)
    for i in range(n):
        rid = first + lo + i
        p, v = sp[i].copy(), sv[i].copy()
        track = [p.copy()]
        on, j, st, skip, lb, lc = SC.K_NONE, 0, 0, -1, -1, -1
        while True:
            kind, q, v = oracle.next_boundary(c, p, v, on, with_direction=True)
            k, side, x = baffle_np.segment(baffles, p, q, skip) if nb else (-1, 0, None)
            w = oracle.philox([rid & 0xffffffff, rid >> 32, j >> 1, 0], [seed & 0xffffffff, seed >> 32])
            wa, wb = w[2 * (j & 1)], w[2 * (j & 1) + 1]
            if k >= 0:
                p = np.array(x, dtype=np.float64)
                track.append(p.copy())
                lb = 2 * k + side
                on, skip = SC.K_NONE, k
                j += 1
                if not wb < bthr[k]:
                    st = 2
                    break
                S = oracle.cosine_emission(bcfg[k], SC.K_INNER, zero, wa, wb)
                rm = brm[k]
                if side == 0:
                    wv = (rm[0] + f64(S[0]), rm[1] + f64(S[1]), rm[2] + f64(S[2]))
                else:
                    wv = ((-rm[0]) + f64(S[0]), (-rm[1]) + f64(S[1]), (-rm[2]) + f64(S[2]))
                mag = np.sqrt((wv[0] * wv[0] + wv[1] * wv[1]) + wv[2] * wv[2])
                v = np.array([wv[0] / mag, wv[1] / mag, wv[2] / mag])
                if len(track) > c.max_points:
                    st = 3
                    break
                continue
            skip = -1
            p = np.array(q, dtype=np.float64)
            track.append(p.copy())
            if kind == SC.K_BOX:
                st = 1
                break
            on = kind
            cls = wallpatch_np.classify(patches, kind == SC.K_INNER, p)
            lc = cls
            j += 1
            if not wb < thrs[cls]:
                st = 2
                break
            v = np.asarray(oracle.cosine_emission(cfgs[cls], kind, p, wa, wb), dtype=np.float64)
            if len(track) > c.max_points:
                st = 3
                break
        status[i], n_points[i], lps[i], dirs[i], last_baffle[i], last_class[i] = st, len(track), p, v, lb, lc
        path[i] = path_of(track, st, c.exit_port_z)
    return {"status": status, "n_points": n_points, "last_point": lps, "direction": dirs, "start_point": np.asarray(sp, dtype=np.float64),
            "last_baffle": last_baffle, "last_class": last_class, "path_cm": path}


PER_RAY = ("status", "n_points", "last_point", "direction", "start_point", "last_baffle", "last_class", "path_cm")


def replay(cfg, scene, n, seed, first=0, workers=None):
    """-> dict of per-ray arrays (PER_RAY) of rays first .. first + n - 1; path_cm is L.  A few spawned processes, as
    scene_np.replay."""
    raw = bytes(C.string_at(C.addressof(cfg), C.sizeof(cfg)))
    scene = {"beam": None if scene.get("beam") is None else dict(scene["beam"]),
             "baffles": [(tuple(float(x) for x in c), tuple(float(x) for x in m), float(r), float(rho))
                         for c, m, r, rho in scene.get("baffles", ())],
             "patches": [(tuple(float(x) for x in a), float(md), float(rho)) for a, md, rho in scene.get("patches", ())]}
    if workers is None:
        workers = max(1, min(8, (os.cpu_count() or 1)))
    if workers == 1 or n < 2000:
        return _replay_range(raw, scene, 0, n, seed, first)
    import multiprocessing as mp
    step = (n + 4 * workers - 1) // (4 * workers)
    jobs = [(raw, scene, lo, min(lo + step, n), seed, first) for lo in range(0, n, step)]
    with mp.get_context("spawn").Pool(workers) as pool:
        parts = pool.starmap(_replay_range, jobs)
    return {k: np.concatenate([p[k] for p in parts]) for k in PER_RAY}


# ---------------------------------------------------------------- the C walk
class _Rays(C.Structure):
    _fields_ = [("status", C.POINTER(C.c_int32)), ("n_points", C.POINTER(C.c_int32)), ("last_point", C.POINTER(C.c_double)),
                ("direction", C.POINTER(C.c_double)), ("start_point", C.POINTER(C.c_double)), ("last_baffle", C.POINTER(C.c_int32)),
                ("last_class", C.POINTER(C.c_int32)), ("path_cm", C.POINTER(C.c_double))]


_lib = None


def build_walk(out=WALK_SO, extra=()):
    """gcc, oracle/Makefile's flags: scene_path_walk.c + isx_oracle.c -> a shared library (or, with -DSPW_MAIN in extra, a program)"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    shared = [] if "-DSPW_MAIN" in extra else ["-shared"]
    flags = [f for f in CFLAGS if not (f == "-fPIC" and not shared)]
    subprocess.check_call(["gcc"] + flags + list(extra) + shared + ["-I", os.path.join(ROOT, "oracle"), "-o", out, WALK_C, ORACLE_C, "-lm"])
    return out


def walk_lib():
    global _lib
    if _lib is None:
        newest = max(os.path.getmtime(WALK_C), os.path.getmtime(ORACLE_C))
        if not os.path.exists(WALK_SO) or os.path.getmtime(WALK_SO) < newest:
            build_walk()
        _lib = C.CDLL(WALK_SO)
    return _lib


def walk(orc, cfg, scene, n, seed, first=0, nthreads=16):
    """the C walk of a scene_np scene dict (orc: tests/oracle.py, for its ctypes twins of the specs) -> dict of PER_RAY arrays"""
    beam, baffles, patches = scene.get("beam"), list(scene.get("baffles") or ()), list(scene.get("patches") or ())
    assert beam is not None and len(baffles) <= 4 and len(patches) <= 8
    bs = orc.BeamSpec()
    bs.struct_size = C.sizeof(orc.BeamSpec)
    for k in ("origin", "axis", "e1", "e2"):
        setattr(bs, k, (C.c_double * 3)(*[float(x) for x in beam[k]]))
    bs.radius, bs.cos_min, bs.angular_law = float(beam["radius"]), float(beam["cos_min"]), int(beam["law"])
    fs = orc.BaffleSpec()
    fs.struct_size, fs.n_baffles = C.sizeof(orc.BaffleSpec), len(baffles)
    for k, (centre, normal, radius, rho) in enumerate(baffles):
        fs.baffle[k].centre = (C.c_double * 3)(*[float(x) for x in centre])
        fs.baffle[k].normal = (C.c_double * 3)(*[float(x) for x in normal])
        fs.baffle[k].radius, fs.baffle[k].reflectance = float(radius), float(rho)
    ws = orc.WallPatchSpec()
    ws.struct_size, ws.n_patches = C.sizeof(orc.WallPatchSpec), len(patches)
    for k, (axis, min_dot, rho) in enumerate(patches):
        ws.patch[k].axis = (C.c_double * 3)(*[float(x) for x in axis])
        ws.patch[k].min_dot, ws.patch[k].reflectance = float(min_dot), float(rho)
    out = {k: np.zeros(n, dtype=np.int32) for k in ("status", "n_points", "last_baffle", "last_class")}
    out.update({k: np.zeros((n, 3), dtype=np.float64) for k in ("last_point", "direction", "start_point")})
    out["path_cm"] = np.zeros(n, dtype=np.float64)
    rays = _Rays()
    for k, a in out.items():
        setattr(rays, k, a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == np.float64 else C.c_int32)))
    fn = walk_lib().spw_scene_path_walk
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(_Rays), C.c_int]
    rc = fn(C.addressof(cfg), C.addressof(bs), C.addressof(fs), C.addressof(ws), int(n), int(seed), int(first), C.byref(rays), int(nthreads))
    assert rc == 0, rc
    return out


# ---------------------------------------------------------------- histograms, overflow, checksum
def bits(L):
    return np.ascontiguousarray(np.asarray(L, dtype=np.float64)).view(np.uint64)


def from_rays(L, fate, n_bins, bin_cm):
    """(hist[21, n_bins], overflow[21], checksum[21]) uint64 of rays with path lengths L and fate slots `fate`"""
    L = np.asarray(L, dtype=np.float64)
    fate = np.asarray(fate, dtype=np.int64)
    n_bins = int(n_bins)
    with np.errstate(all="ignore"):
        fb = L / f64(bin_cm)
        inside = fb < f64(n_bins)      # (false for a NaN)
    ib = np.zeros(L.size, dtype=np.int64)
    ib[inside] = fb[inside].astype(np.int64)   # (int)fb: truncation
    hist = np.bincount(fate[inside] * n_bins + ib[inside], minlength=FATES * n_bins).astype(np.uint64).reshape(FATES, n_bins)
    overflow = np.bincount(fate[~inside], minlength=FATES).astype(np.uint64)
    checksum = np.zeros(FATES, dtype=np.uint64)
    b = bits(L)
    with np.errstate(over="ignore"):
        for f in range(FATES):
            checksum[f] = np.add.reduce(b[fate == f], dtype=np.uint64) if (fate == f).any() else np.uint64(0)
    return hist, overflow, checksum


def from_walk(w, cfg, n_bins, bin_cm):
    """from_rays on a walk's (or a replay's) per-ray arrays, the fate slots by response_np.fates"""
    return from_rays(w["path_cm"], R.fates(w, cfg), n_bins, bin_cm)


# ---------------------------------------------------------------- the two host helpers' formulas
def moments(hist, overflow, bin_cm):
    """isx_scene_path_moments' formulas, operation for operation -> (mean_cm[21], sd_cm[21])"""
    hist = np.asarray(hist, dtype=np.uint64)
    mean, sd = np.full(FATES, np.nan), np.full(FATES, np.nan)
    for f in range(FATES):
        N = A = B = 0.0
        for k in range(hist.shape[1]):
            h, x = float(hist[f, k]), (float(k) + 0.5) * float(bin_cm)
            N += h
            A += x * h
            B += x * x * h
        if N > 0 and int(overflow[f]) == 0:
            m = A / N
            var = B / N - m * m
            mean[f], sd[f] = m, math.sqrt(var if var > 0 else 0.0)
    return mean, sd


def decay(hist, f, lo_bin, bin_cm):
    """isx_scene_path_decay's formulas, operation for operation -> (tau_cm, sigma_cm), or None where the call refuses (N == 0, m == 0)"""
    row = np.asarray(hist, dtype=np.uint64)[f]
    N = S = 0.0
    for ib in range(lo_bin, row.size):
        h = float(row[ib])
        S += float(ib - lo_bin) * h
        N += h
    if not N > 0:
        return None
    m = S / N
    if not m > 0:
        return None
    r = m / (1.0 + m)
    lr = math.log(r)
    return -float(bin_cm) / lr, float(bin_cm) / (lr * lr) / math.sqrt(N * m * (1.0 + m))
