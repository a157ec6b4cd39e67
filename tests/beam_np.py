"""The beam source of include/isx.h (isx_fluxmap_beam, isx_beam_endstates) on the unchanged CPU oracle -- TEST INFRASTRUCTURE.

sample() is the header's per-ray sampling in numpy binary64: the words are oracle.philox's (block 0 of stream 3 of the ray), u01
and sincos2pi the oracle's own (isxo_u01 / isxo_sincos2pi), everything else numpy's multiply, add, divide and sqrt -- the IEEE
operations, correctly rounded, no fma -- evaluated left to right as the header writes them.

replay() walks the oracle's trace loop bounce by bounce from the sampled (p, v), as wallpatch_np._replay_range does from the
pencil's (oracle.next_boundary with on = 0 / philox stream 0 / cosine_emission).  Valid for the Lambertian border and explicit
bounces -- the call's scope.

A spec is a dict (origin, axis, e1, e2: 3-tuples; radius, cos_min: floats; law: 0 / 1); spec_of() makes one from the library's
BeamSpec.
"""
import ctypes as C
import math
import os

import numpy as np

K_NONE, K_INNER, K_OUTER, K_CONE, K_BOX = 0, 1, 2, 3, 4
UNIFORM, LAMBERT = 0, 1
CENSUS_FIELDS = ("launched", "exited", "counted_below_z", "absorbed", "suspended", "wall_hits")


def spec_of(bs):
    """the dict of a BeamSpec"""
    return {"origin": tuple(float(x) for x in bs.origin), "axis": tuple(float(x) for x in bs.axis),
            "e1": tuple(float(x) for x in bs.e1), "e2": tuple(float(x) for x in bs.e2),
            "radius": float(bs.radius), "cos_min": float(bs.cos_min), "law": int(bs.angular_law)}


def rho_thr(rho):
    """the absorb test's threshold on the raw word: b survives iff b < rho_thr"""
    x = math.ceil(math.ldexp(float(rho), 32) - 0.5)
    return min(max(int(x), 0), 1 << 32)


def uniforms(n, seed, first=0):
    """-> u[n, 4], (s1, c1)[n], (s3, c3)[n]: u01 of block 0 of stream 3 of rays [first, first + n) and the two sincos2pi"""
    import oracle
    L = oracle.lib()
    u = np.zeros((n, 4), dtype=np.float64)
    sc1 = np.zeros((n, 2), dtype=np.float64)
    sc3 = np.zeros((n, 2), dtype=np.float64)
    key = [seed & 0xffffffff, seed >> 32]
    for i in range(n):
        rid = first + i
        w = oracle.philox([rid & 0xffffffff, rid >> 32, 0, 3], key)
        u[i] = [L.isxo_u01(w[0]), L.isxo_u01(w[1]), L.isxo_u01(w[2]), L.isxo_u01(w[3])]
        sc1[i] = oracle.sincos2pi(u[i, 1])
        sc3[i] = oracle.sincos2pi(u[i, 3])
    return u, sc1, sc3


def sample(spec, n, seed, first=0):
    """-> (p[n, 3], v[n, 3]): the start of rays [first, first + n), the header's expressions in their order"""
    u, sc1, sc3 = uniforms(n, seed, first)
    f = np.float64
    origin, axis, e1, e2 = (tuple(f(x) for x in spec[k]) for k in ("origin", "axis", "e1", "e2"))
    radius, cos_min = f(spec["radius"]), f(spec["cos_min"])
    rr = radius * np.sqrt(u[:, 0])
    s1, c1 = sc1[:, 0], sc1[:, 1]
    a = rr * c1
    b = rr * s1
    p = np.stack([(origin[k] + a * e1[k]) + b * e2[k] for k in range(3)], axis=1)
    if spec["law"] == LAMBERT:
        s2 = u[:, 2] * (f(1.0) - cos_min * cos_min)
        st = np.sqrt(s2)
        ct = np.sqrt(f(1.0) - s2)
    else:
        ct = f(1.0) - u[:, 2] * (f(1.0) - cos_min)
        st = np.sqrt(f(1.0) - ct * ct)
    s3, c3 = sc3[:, 0], sc3[:, 1]
    k1 = st * c3
    k2 = st * s3
    d = [(ct * axis[k] + k1 * e1[k]) + k2 * e2[k] for k in range(3)]
    mag = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    v = np.stack([d[0] / mag, d[1] / mag, d[2] / mag], axis=1)
    return p, v


def _replay_range(cfg_bytes, spec, lo, hi, seed, first):
    """rays [lo, hi) of a call (seed, first) -> (start p, start v, status, n_points, last point, direction, first kind, census)"""
    import oracle
    c = oracle.Config()
    C.memmove(C.byref(c), cfg_bytes, C.sizeof(oracle.Config))
    assert c.lambertian == 1 and c.surface_model == 0 and c.source_model == 0 and c.trace_mode == 0, "replay(): Lambertian border, explicit bounces"
    thr = rho_thr(c.reflectance)
    n = hi - lo
    sp, sv = sample(spec, n, seed, first + lo)
    status, n_points, kind0 = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    lps, dirs = np.zeros((n, 3)), np.zeros((n, 3))
    census = dict.fromkeys(CENSUS_FIELDS, 0)
    for i in range(n):
        rid = first + lo + i
        p, v = sp[i].copy(), sv[i].copy()
        on, j, npoints, st = K_NONE, 0, 1, 0
        while True:
            kind, q, v = oracle.next_boundary(c, p, v, on, with_direction=True)
            if npoints == 1:
                kind0[i] = kind
            p = q
            npoints += 1
            if kind == K_BOX:
                st = 1
                break
            on = kind
            w = oracle.philox([rid & 0xffffffff, rid >> 32, j >> 1, 0], [seed & 0xffffffff, seed >> 32])
            wa, wb = w[2 * (j & 1)], w[2 * (j & 1) + 1]
            j += 1
            if not wb < thr:
                st = 2
                break
            v = oracle.cosine_emission(c, kind, p, wa, wb)
            if npoints > c.max_points:
                st = 3
                break
        status[i], n_points[i], lps[i], dirs[i] = st, npoints, p, v
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
    return sp, sv, status, n_points, lps, dirs, kind0, census


def replay(cfg, spec, n, seed, first=0, workers=None):
    """-> (start_point[n, 3], start_dir[n, 3], status[n], n_points[n], last_point[n, 3], direction[n, 3], first_kind[n], census
    dict) of rays [first, first + n); first_kind is the boundary of every ray's first segment.  The rays are independent: they
    are walked by a few fresh processes (spawned, so that nothing of the caller's process is inherited)."""
    raw = bytes(C.string_at(C.addressof(cfg), C.sizeof(cfg)))
    spec = dict(spec)
    if workers is None:
        workers = max(1, min(8, (os.cpu_count() or 1)))
    if workers == 1 or n < 2000:
        return _replay_range(raw, spec, 0, n, seed, first)
    import multiprocessing as mp
    step = (n + 4 * workers - 1) // (4 * workers)
    jobs = [(raw, spec, lo, min(lo + step, n), seed, first) for lo in range(0, n, step)]
    with mp.get_context("spawn").Pool(workers) as pool:
        parts = pool.starmap(_replay_range, jobs)
    census = {k: sum(p[7][k] for p in parts) for k in CENSUS_FIELDS}
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(7)) + (census,)


def counted_lines(cfg, rep):
    """(P, V) of the replay's rays that left through the port: exited with the last point below exit_port_z"""
    _, _, status, _, lp, d, _, _ = rep
    sel = (status == 1) & (lp[:, 2] < cfg.exit_port_z)
    return lp[sel], d[sel]


def chi2_sf(x, dof):
    """P(chi2_dof >= x): the regularised upper incomplete gamma function Q(dof / 2, x / 2) by its series"""
    a, z = 0.5 * dof, 0.5 * x
    if z <= 0:
        return 1.0
    term = 1.0 / a
    total = term
    k = 0
    while abs(term) > 1e-17 * abs(total) and k < 10000:
        k += 1
        term *= z / (a + k)
        total += term
    p_lower = total * math.exp(-z + a * math.log(z) - math.lgamma(a))
    return max(0.0, 1.0 - p_lower)


def uniform_chi2_p(x, bins=20):
    """p-value of the chi2 of x (values in [0, 1]) over `bins` equal bins against the uniform law"""
    x = np.asarray(x, dtype=np.float64)
    idx = np.minimum((x * bins).astype(np.int64), bins - 1)
    assert idx.min() >= 0
    obs = np.bincount(idx, minlength=bins).astype(np.float64)
    e = x.size / bins
    return chi2_sf(float(((obs - e) ** 2 / e).sum()), bins - 1)
