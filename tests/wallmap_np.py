"""The wall map of include/isx.h (isx_wall_map) restated in numpy, and two independent sources of wall points -- TEST INFRASTRUCTURE.

The bin arithmetic is the header's, operation for operation: numpy's binary64 multiply, add, divide and sqrt are the IEEE
operations (correctly rounded, no fma), evaluated left to right as written.

Wall points come from the unchanged CPU oracle in two ways:
  replay()       walks the oracle's own trace loop bounce by bounce (oracle.next_boundary / philox / cosine_emission, exactly as
                 robast_dump.write_synthetic does) and checks every end state against oracle.trace_endstates.  Valid for the
                 Lambertian border, the pencil source and explicit bounces.
  limit_sweep()  runs oracle.trace_endstates with max_points = m for m = 1..M: a ray that is absorbed or suspended with
                 n_points == m + 1 ended AT its interaction m - 1, so its last point is q_{m-1}.  Valid for every border and
                 trace mode; the kind of surface is told by |q| (inner sphere: | |q| - r_in | < 1e-9).
Both return the interactions as arrays (ray, j, inner, q).
"""
import ctypes as C
import os

import numpy as np

K_NONE, K_INNER, K_OUTER, K_CONE, K_BOX = 0, 1, 2, 3, 4
COUNT_FIELDS = ("binned", "outside", "skipped", "other_surface")


def project(q, r_in):
    """(X, Y) of isx.h for points q[N, 3]"""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    inv = 1.0 / np.float64(r_in)
    with np.errstate(all="ignore"):
        c = q[:, 2] * inv
        w = np.sqrt(0.5 / (1.0 + c))
        X = (q[:, 0] * inv) * w
        Y = (q[:, 1] * inv) * w
    return X, Y


def bins(q, r_in, n_x, n_y):
    """-> (ix, iy, ok): the bin of every point, ok False = outside (NaN / inf included)"""
    X, Y = project(q, r_in)
    with np.errstate(all="ignore"):
        fx = (X + 1.0) * 0.5 * np.float64(n_x)
        fy = (Y + 1.0) * 0.5 * np.float64(n_y)
        fl_x, fl_y = np.floor(fx), np.floor(fy)
        ok = (fl_x >= 0) & (fl_x < n_x) & (fl_y >= 0) & (fl_y < n_y)     # (a NaN compares false)
    ix = np.where(ok, fl_x, 0).astype(np.int64)
    iy = np.where(ok, fl_y, 0).astype(np.int64)
    return ix, iy, ok


def wall_map_np(points, r_in, n_x, n_y, first_order):
    """points = (ray, j, inner, q) -> (wall_map[n_y, n_x] uint64, counts dict): the classification of isx.h, in its order"""
    _, j, inner, q = points
    other = ~inner
    skipped = inner & (j < first_order)
    cand = inner & ~skipped
    ix, iy, ok = bins(q[cand], r_in, n_x, n_y)
    m = np.zeros((n_y, n_x), dtype=np.uint64)
    np.add.at(m, (iy[ok], ix[ok]), np.uint64(1))
    counts = {"binned": int(ok.sum()), "outside": int((~ok).sum()), "skipped": int(skipped.sum()), "other_surface": int(other.sum())}
    return m, counts


def wall_map_of_spec(points, cfg, spec):
    return wall_map_np(points, cfg.r_in, spec.n_x, spec.n_y, spec.first_order)


def _pack(rows):
    if not rows:
        return (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, bool), np.zeros((0, 3)))
    ray = np.array([r[0] for r in rows], dtype=np.int64)
    j = np.array([r[1] for r in rows], dtype=np.int64)
    inner = np.array([r[2] for r in rows], dtype=bool)
    q = np.array([r[3] for r in rows], dtype=np.float64).reshape(-1, 3)
    return ray, j, inner, q


def _replay_range(cfg_bytes, lo, hi, seed, first):
    """the interactions of rays [lo, hi) of a call (seed, first): robast_dump.write_synthetic's loop"""
    import oracle
    c = oracle.Config()
    C.memmove(C.byref(c), cfg_bytes, C.sizeof(oracle.Config))
    assert c.lambertian == 1 and c.surface_model == 0 and c.source_model == 0 and c.trace_mode == 0, "replay(): Lambertian border, pencil source, explicit bounces"
    n = hi - lo
    st, npts, lps, dirs = oracle.trace_endstates(c, n, seed, first + lo)
    rho_thr = int(np.ceil(c.reflectance * 2.0 ** 32 - 0.5))
    src = np.array([c.src[0], c.src[1], c.src[2]])
    d0 = np.array([c.dir[0], c.dir[1], c.dir[2]])
    d0 = d0 / np.linalg.norm(d0)
    rows = []
    for i in range(n):
        rid = first + lo + i
        p, v = src.copy(), d0.copy()
        on, j, npoints, status = K_NONE, 0, 1, 0
        while True:
            kind, q, v = oracle.next_boundary(c, p, v, on, with_direction=True)
            p = q
            npoints += 1
            if kind == K_BOX:
                status = 1
                break
            on = kind
            rows.append((lo + i, j, kind == K_INNER, p.copy()))
            w = oracle.philox([rid & 0xffffffff, rid >> 32, j >> 1, 0], [seed & 0xffffffff, seed >> 32])
            wa, wb = w[2 * (j & 1)], w[2 * (j & 1) + 1]
            j += 1
            if not wb < rho_thr:
                status = 2
                break
            v = oracle.cosine_emission(c, kind, p, wa, wb)
            if npoints > c.max_points:
                status = 3
                break
        assert status == int(st[i]) and npoints == npts[i] and np.array_equal(p, lps[i]), (rid, status, int(st[i]), npoints, int(npts[i]))
        if status == 1:
            assert np.array_equal(v, dirs[i]), rid
    return rows


def replay(cfg, n, seed, first=0, workers=None):
    """The interactions of rays [first, first + n), every end state checked against oracle.trace_endstates.  The rays are
    independent: they are walked by a few fresh processes (spawned, so that nothing of the caller's process is inherited)."""
    raw = bytes(C.string_at(C.addressof(cfg), C.sizeof(cfg)))
    if workers is None:
        workers = max(1, min(8, (os.cpu_count() or 1)))
    if workers == 1 or n < 2000:
        return _pack(_replay_range(raw, 0, n, seed, first))
    import multiprocessing as mp
    step = (n + 4 * workers - 1) // (4 * workers)
    jobs = [(raw, lo, min(lo + step, n), seed, first) for lo in range(0, n, step)]
    with mp.get_context("spawn").Pool(workers) as pool:
        parts = pool.starmap(_replay_range, jobs)
    return _pack([r for part in parts for r in part])


def limit_sweep(orc, cfg, n, seed, M, first=0):
    """The interactions j < M of rays [first, first + n): see the module docstring."""
    ray, jj, inner, qq = [], [], [], []
    for m in range(1, M + 1):
        c = cfg.copy()
        c.max_points = m
        st, npts, lp, _ = orc.trace_endstates(c, n, seed, first)
        sel = ((st == 2) | (st == 3)) & (npts == m + 1)
        idx = np.nonzero(sel)[0]
        q = lp[idx]
        ray.append(idx.astype(np.int64))
        jj.append(np.full(idx.size, m - 1, dtype=np.int64))
        inner.append(np.abs(np.sqrt((q * q).sum(axis=1)) - cfg.r_in) < 1e-9)
        qq.append(q)
    return np.concatenate(ray), np.concatenate(jj), np.concatenate(inner), np.concatenate(qq).reshape(-1, 3)


def sort_points(points):
    """by (ray, j): the order in which two sources can be compared"""
    ray, j, inner, q = points
    o = np.lexsort((j, ray))
    return ray[o], j[o], inner[o], q[o]


def flatness_chi2(wmap, theta_max_deg, frac=0.9):
    """chi2 of the bins whose four corners lie within frac * sin(theta_max / 2) of the map's centre against a flat expectation
    (their mean: one fitted parameter) -> (chi2, dof).  The chord identity makes the diffuse irradiance of the wall uniform,
    and the projection is equal-area."""
    n_y, n_x = wmap.shape
    rw = frac * np.sin(np.deg2rad(theta_max_deg) / 2.0)
    x0 = -1.0 + np.arange(n_x) * (2.0 / n_x)
    y0 = -1.0 + np.arange(n_y) * (2.0 / n_y)
    ax = np.maximum(np.abs(x0), np.abs(x0 + 2.0 / n_x))
    ay = np.maximum(np.abs(y0), np.abs(y0 + 2.0 / n_y))
    inside = (ax[None, :] ** 2 + ay[:, None] ** 2) <= rw * rw
    obs = wmap[inside].astype(np.float64)
    e = obs.mean()
    return float(((obs - e) ** 2 / e).sum()), int(obs.size - 1)
