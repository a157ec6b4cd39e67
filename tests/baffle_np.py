"""The baffles of include/isx.h (isx_fluxmap_baffle, isx_baffle_endstates) replayed on the unchanged CPU oracle -- TEST INFRASTRUCTURE.

replay() walks the oracle's own trace loop bounce by bounce, as wallpatch_np._replay_range and beam_np._replay_range do
(oracle.next_boundary / philox / cosine_emission), with the header's segment test between every point p and the next boundary
point q: numpy's binary64 subtract, multiply, add and divide, left to right as the header writes them (no fma).  A struck
baffle takes the interaction of the ray's index j: the absorb test on the raw word against the threshold of the baffle's
reflectance, then the cosine emission about the struck side's normal from the oracle's own sphere point --
isxo_cosine_emission of kind 1 at q = (0, 0, 0) with the baffle's reflectance in the configuration -- plus or minus
rm = r_in * normal, normalised with numpy's sqrt and divide.  The ray goes on from the struck point on no surface (on = 0), with
that baffle skipped for one segment.  Valid for the Lambertian border, the pencil source and explicit bounces -- the call's scope.

A spec is a sequence of baffles (centre[3], normal[3], radius, reflectance); spec_of() makes one from the library's BaffleSpec.
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
    """[(centre, normal, radius, reflectance)] of a BaffleSpec"""
    return [(tuple(float(x) for x in b.centre), tuple(float(x) for x in b.normal), float(b.radius), float(b.reflectance))
            for b in list(spec.baffle)[:spec.n_baffles]]


def disc(centre, direction, radius, reflectance):
    """isx_baffle_disc in numpy: normal = direction / |direction| (mag = sqrt(dx*dx + dy*dy + dz*dz), three divisions)"""
    d = [np.float64(x) for x in direction]
    mag = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return (tuple(float(x) for x in centre), tuple(float(x / mag) for x in d), float(radius), float(reflectance))


def segment(baffles, p, q, skip):
    """the header's segment test -> (k, side, x) of the struck baffle, or (-1, 0, None)"""
    f64 = np.float64
    best, bf, bx, bside = -1, None, None, 0
    px, py, pz = f64(p[0]), f64(p[1]), f64(p[2])
    qx, qy, qz = f64(q[0]), f64(q[1]), f64(q[2])
    for k, (c, m, radius, _) in enumerate(baffles):
        if k == skip:
            continue
        cx, cy, cz = f64(c[0]), f64(c[1]), f64(c[2])
        mx, my, mz = f64(m[0]), f64(m[1]), f64(m[2])
        sp = ((px - cx) * mx + (py - cy) * my) + (pz - cz) * mz
        sq = ((qx - cx) * mx + (qy - cy) * my) + (qz - cz) * mz
        if not ((sp > 0 and sq < 0) or (sp < 0 and sq > 0)):
            continue
        f = sp / (sp - sq)
        x = (px + f * (qx - px), py + f * (qy - py), pz + f * (qz - pz))
        dx, dy, dz = x[0] - cx, x[1] - cy, x[2] - cz
        r2 = f64(radius) * f64(radius)
        if (dx * dx + dy * dy) + dz * dz <= r2 and (best < 0 or f < bf):
            best, bf, bx, bside = k, f, x, (0 if sp > 0 else 1)
    return best, bside, (None if bx is None else np.array(bx, dtype=np.float64))


def _replay_range(cfg_bytes, baffles, lo, hi, seed, first):
    """rays [lo, hi) of a call (seed, first) -> dict of per-ray arrays, counters and the census"""
    import oracle
    c = oracle.Config()
    C.memmove(C.byref(c), cfg_bytes, C.sizeof(oracle.Config))
    assert c.lambertian == 1 and c.surface_model == 0 and c.source_model == 0 and c.trace_mode == 0, "replay(): Lambertian border, pencil source, explicit bounces"
    f64 = np.float64
    nb = len(baffles)
    thr = rho_thr(c.reflectance)
    bcfg, bthr, brm = [], [], []
    for (_, m, _, rho) in baffles:
        ck = c.copy()
        ck.reflectance = rho
        bcfg.append(ck)
        bthr.append(rho_thr(rho))
        brm.append(tuple(f64(c.r_in) * f64(m[i]) for i in range(3)))
    arrivals = np.zeros((max(nb, 1), 2), dtype=np.uint64)
    absorbed = np.zeros((max(nb, 1), 2), dtype=np.uint64)
    census = dict.fromkeys(CENSUS_FIELDS, 0)
    n = hi - lo
    status, n_points, last_baffle = (np.zeros(n, dtype=np.int32) for _ in range(3))
    lps, dirs = np.zeros((n, 3)), np.zeros((n, 3))
    emitted = []          # (2 k + side, v) of every re-emission from a baffle
    after_baffle = 0      # rays suspended right after a baffle interaction
    src = np.array([c.src[0], c.src[1], c.src[2]])
    d0 = np.array([c.dir[0], c.dir[1], c.dir[2]])
    d0 = d0 / np.linalg.norm(d0)
    zero = (0.0, 0.0, 0.0)
    for i in range(n):
        rid = first + lo + i
        p, v = src.copy(), d0.copy()
        on, j, npoints, st, skip, lb = K_NONE, 0, 1, 0, -1, -1
        while True:
            kind, q, v = oracle.next_boundary(c, p, v, on, with_direction=True)
            k, side, x = segment(baffles, p, q, skip) if nb else (-1, 0, None)
            npoints += 1
            if k >= 0:
                p = x
                arrivals[k, side] += np.uint64(1)
                lb = 2 * k + side
                on, skip = K_NONE, k
                w = oracle.philox([rid & 0xffffffff, rid >> 32, j >> 1, 0], [seed & 0xffffffff, seed >> 32])
                wa, wb = w[2 * (j & 1)], w[2 * (j & 1) + 1]
                j += 1
                if not wb < bthr[k]:
                    absorbed[k, side] += np.uint64(1)
                    st = 2
                    break
                S = oracle.cosine_emission(bcfg[k], K_INNER, zero, wa, wb)
                rm = brm[k]
                if side == 0:
                    wv = (rm[0] + f64(S[0]), rm[1] + f64(S[1]), rm[2] + f64(S[2]))
                else:
                    wv = ((-rm[0]) + f64(S[0]), (-rm[1]) + f64(S[1]), (-rm[2]) + f64(S[2]))
                mag = np.sqrt((wv[0] * wv[0] + wv[1] * wv[1]) + wv[2] * wv[2])
                v = np.array([wv[0] / mag, wv[1] / mag, wv[2] / mag])
                emitted.append((lb, v.copy()))
                if npoints > c.max_points:
                    st = 3
                    after_baffle += 1
                    break
                continue
            skip = -1
            p = q
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
        status[i], n_points[i], lps[i], dirs[i], last_baffle[i] = st, npoints, p, v, lb
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
    return {"status": status, "n_points": n_points, "last_point": lps, "direction": dirs, "last_baffle": last_baffle,
            "arrivals": arrivals, "absorbed": absorbed, "census": census,
            "emit_side": np.array([e[0] for e in emitted], dtype=np.int32),
            "emit_dir": np.array([e[1] for e in emitted], dtype=np.float64).reshape(-1, 3),
            "suspended_after_baffle": after_baffle}


PER_RAY = ("status", "n_points", "last_point", "direction", "last_baffle")


def replay(cfg, baffles, n, seed, first=0, workers=None):
    """-> dict: status[n], n_points[n], last_point[n, 3], direction[n, 3], last_baffle[n] (-1 or 2 k + side), arrivals[K, 2],
    absorbed[K, 2] (K = max(len(baffles), 1)), census dict, and of every re-emission from a baffle emit_side (2 k + side) and
    emit_dir; suspended_after_baffle counts the rays the bounce limit stopped right after a baffle interaction.  The rays are
    independent: they are walked by a few fresh processes (spawned, so that nothing of the caller's process is inherited)."""
    raw = bytes(C.string_at(C.addressof(cfg), C.sizeof(cfg)))
    baffles = [(tuple(float(x) for x in c), tuple(float(x) for x in m), float(r), float(rho)) for c, m, r, rho in baffles]
    if workers is None:
        workers = max(1, min(8, (os.cpu_count() or 1)))
    if workers == 1 or n < 2000:
        return _replay_range(raw, baffles, 0, n, seed, first)
    import multiprocessing as mp
    step = (n + 4 * workers - 1) // (4 * workers)
    jobs = [(raw, baffles, lo, min(lo + step, n), seed, first) for lo in range(0, n, step)]
    with mp.get_context("spawn").Pool(workers) as pool:
        parts = pool.starmap(_replay_range, jobs)
    out = {k: np.concatenate([p[k] for p in parts]) for k in PER_RAY + ("emit_side", "emit_dir")}
    out["arrivals"] = sum(p["arrivals"] for p in parts)
    out["absorbed"] = sum(p["absorbed"] for p in parts)
    out["census"] = {k: sum(p["census"][k] for p in parts) for k in CENSUS_FIELDS}
    out["suspended_after_baffle"] = sum(p["suspended_after_baffle"] for p in parts)
    return out


def counted_lines(cfg, rep):
    """(P, V) of the replay's rays that left through the port: exited with the last point below exit_port_z"""
    sel = (rep["status"] == 1) & (rep["last_point"][:, 2] < cfg.exit_port_z)
    return rep["last_point"][sel], rep["direction"][sel]
