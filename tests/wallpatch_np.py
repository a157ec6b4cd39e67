"""The wall patches of include/isx.h (isx_wall_patches) replayed on the unchanged CPU oracle -- TEST INFRASTRUCTURE.

replay() walks the oracle's own trace loop bounce by bounce, as wallmap_np.replay does (oracle.next_boundary / philox /
cosine_emission), with the header's classification at every mirror interaction: the class of the point, the class's reflectance
rho_eff for the absorb test (threshold ceil(ldexp(rho_eff, 32) - 0.5), clamped to [0, 2^32]) and, through a configuration copy
with reflectance rho_eff, for the oracle's cosine emission.  The dot product is numpy's binary64 multiply and add, left to right
as the header writes it (no fma).  Valid for the Lambertian border, the pencil source and explicit bounces -- the call's scope.

A spec is a sequence of patches (axis[3], min_dot, reflectance); spec_of() makes one from the library's WallPatchSpec.
"""
import ctypes as C
import math
import os

import numpy as np

K_NONE, K_INNER, K_OUTER, K_CONE, K_BOX = 0, 1, 2, 3, 4
CENSUS_FIELDS = ("launched", "exited", "counted_below_z", "absorbed", "suspended", "wall_hits")


def rho_thr(rho):
    """the absorb test's threshold on the raw word: b survives iff b < rho_thr"""
    x = math.ceil(math.ldexp(float(rho), 32) - 0.5)
    return min(max(int(x), 0), 1 << 32)


def spec_of(spec):
    """[(axis, min_dot, reflectance)] of a WallPatchSpec"""
    return [((float(p.axis[0]), float(p.axis[1]), float(p.axis[2])), float(p.min_dot), float(p.reflectance))
            for p in list(spec.patch)[:spec.n_patches]]


def classify(patches, inner, q):
    """the class of an interaction at q: P + 1 off the inner sphere, else the lowest patch that holds q, else P"""
    P = len(patches)
    if not inner:
        return P + 1
    qx, qy, qz = np.float64(q[0]), np.float64(q[1]), np.float64(q[2])
    for k, (a, md, _) in enumerate(patches):
        if (qx * np.float64(a[0]) + qy * np.float64(a[1])) + qz * np.float64(a[2]) >= np.float64(md):
            return k
    return P


def _replay_range(cfg_bytes, patches, lo, hi, seed, first):
    """rays [lo, hi) of a call (seed, first) -> (arrivals, absorbed, census, status, n_points)"""
    import oracle
    c = oracle.Config()
    C.memmove(C.byref(c), cfg_bytes, C.sizeof(oracle.Config))
    assert c.lambertian == 1 and c.surface_model == 0 and c.source_model == 0 and c.trace_mode == 0, "replay(): Lambertian border, pencil source, explicit bounces"
    P = len(patches)
    cfgs, thrs = [], []
    for k in range(P + 2):
        ck = c.copy()
        if k < P:
            ck.reflectance = patches[k][2]
        cfgs.append(ck)
        thrs.append(rho_thr(ck.reflectance))
    arrivals = np.zeros(P + 2, dtype=np.uint64)
    absorbed = np.zeros(P + 2, dtype=np.uint64)
    census = dict.fromkeys(CENSUS_FIELDS, 0)
    n = hi - lo
    status, n_points = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    src = np.array([c.src[0], c.src[1], c.src[2]])
    d0 = np.array([c.dir[0], c.dir[1], c.dir[2]])
    d0 = d0 / np.linalg.norm(d0)
    for i in range(n):
        rid = first + lo + i
        p, v = src.copy(), d0.copy()
        on, j, npoints, st = K_NONE, 0, 1, 0
        while True:
            kind, q, v = oracle.next_boundary(c, p, v, on, with_direction=True)
            p = q
            npoints += 1
            if kind == K_BOX:
                st = 1
                break
            on = kind
            cls = classify(patches, kind == K_INNER, p)
            arrivals[cls] += np.uint64(1)
            w = oracle.philox([rid & 0xffffffff, rid >> 32, j >> 1, 0], [seed & 0xffffffff, seed >> 32])
            wa, wb = w[2 * (j & 1)], w[2 * (j & 1) + 1]
            j += 1
            if not wb < thrs[cls]:
                absorbed[cls] += np.uint64(1)
                st = 2
                break
            v = oracle.cosine_emission(cfgs[cls], kind, p, wa, wb)
            if npoints > c.max_points:
                st = 3
                break
        status[i], n_points[i] = st, npoints
        census["launched"] += 1
        census["wall_hits"] += j
        if st == 1:
            census["exited"] += 1
            if p[2] < c.exit_port_z:
                census["counted_below_z"] += 1
        elif st == 2:
            census["absorbed"] += 1
        else:
            census["suspended"] += 1
    return arrivals, absorbed, census, status, n_points


def replay(cfg, patches, n, seed, first=0, workers=None):
    """-> (arrivals[P + 2], absorbed[P + 2], census dict, status[n], n_points[n]) of rays [first, first + n).  The rays are
    independent: they are walked by a few fresh processes (spawned, so that nothing of the caller's process is inherited)."""
    raw = bytes(C.string_at(C.addressof(cfg), C.sizeof(cfg)))
    patches = [(tuple(float(x) for x in a), float(md), float(rho)) for a, md, rho in patches]
    if workers is None:
        workers = max(1, min(8, (os.cpu_count() or 1)))
    if workers == 1 or n < 2000:
        return _replay_range(raw, patches, 0, n, seed, first)
    import multiprocessing as mp
    step = (n + 4 * workers - 1) // (4 * workers)
    jobs = [(raw, patches, lo, min(lo + step, n), seed, first) for lo in range(0, n, step)]
    with mp.get_context("spawn").Pool(workers) as pool:
        parts = pool.starmap(_replay_range, jobs)
    arrivals = sum(p[0] for p in parts)
    absorbed = sum(p[1] for p in parts)
    census = {k: sum(p[2][k] for p in parts) for k in CENSUS_FIELDS}
    return arrivals, absorbed, census, np.concatenate([p[3] for p in parts]), np.concatenate([p[4] for p in parts])


def binomial_z(arrivals, absorbed, rho):
    """z of `absorbed` against Binomial(arrivals, 1 - rho_thr(rho) / 2^32): the law is exact, one fresh word per arrival"""
    pa = 1.0 - rho_thr(rho) / 4294967296.0
    n = float(arrivals)
    sd = math.sqrt(n * pa * (1.0 - pa))
    return (float(absorbed) - n * pa) / sd if sd > 0 else 0.0
