"""numpy restatement of the exit maps' numeric contract (include/isx.h, isx_exit_maps) over end-state arrays --
TEST INFRASTRUCTURE: the reference every exit-map test compares against, fed from the oracle's trace_endstates().

IEEE double, evaluated left to right as the header writes it; numpy never fuses a multiply and an add."""
import numpy as np

EXITED = 1
COUNT_FIELDS = ("dir_binned", "dir_outside", "pos_binned", "pos_outside", "upward")


def _axis_bin(f, n):
    """(int)floor(f) where that is a bin of [0, n); -1 otherwise (NaN and +-inf have no bin)."""
    with np.errstate(invalid="ignore"):
        fl = np.floor(f)
        ok = np.isfinite(fl) & (fl >= 0) & (fl < n)
    out = np.full(f.shape, -1, dtype=np.int64)
    out[ok] = fl[ok].astype(np.int64)
    return out


def direction_map(v, n_u, n_v):
    """v[k, 3]: final directions of counted rays -> (dir_map[n_v, n_u] uint64, binned, outside)."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    iu = _axis_bin((v[:, 0] + 1.0) * 0.5 * n_u, n_u)
    iv = _axis_bin((v[:, 1] + 1.0) * 0.5 * n_v, n_v)
    ok = (iu >= 0) & (iv >= 0)
    m = np.bincount(iv[ok] * n_u + iu[ok], minlength=n_u * n_v).astype(np.uint64).reshape(n_v, n_u)
    return m, int(ok.sum()), int((~ok).sum())


def plane_map(p, v, n_x, n_y, plane_z, half_extent):
    """p[k, 3], v[k, 3]: last points and final directions of counted rays -> (pos_map[n_y, n_x], binned, outside, upward)."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    down = v[:, 2] < 0.0                       # -0.0, +0.0 and NaN are "upward"
    p, v = p[down], v[down]
    with np.errstate(all="ignore"):
        t = (np.float64(plane_z) - p[:, 2]) / v[:, 2]
        x = p[:, 0] + t * v[:, 0]
        y = p[:, 1] + t * v[:, 1]
        h = np.float64(half_extent)
        ix = _axis_bin((x + h) / (2.0 * h) * n_x, n_x)
        iy = _axis_bin((y + h) / (2.0 * h) * n_y, n_y)
    ok = (ix >= 0) & (iy >= 0)
    m = np.bincount(iy[ok] * n_x + ix[ok], minlength=n_x * n_y).astype(np.uint64).reshape(n_y, n_x)
    return m, int(ok.sum()), int((~ok).sum()), int((~down).sum())


def exitmap_np(endstates, exit_port_z, n_u, n_v, n_x, n_y, plane_z, half_extent):
    """endstates = (status, n_points, last_point[n, 3], direction[n, 3]) as trace_endstates() returns them.
    -> (dir_map[n_v, n_u], pos_map[n_y, n_x], counts dict, counted).  A map with 0 x 0 bins is not wanted: shape (0, 0),
    its counters 0."""
    status, _, lp, d = endstates
    sel = (np.asarray(status) == EXITED) & (lp[:, 2] < exit_port_z)
    p, v = lp[sel], d[sel]
    counts = dict.fromkeys(COUNT_FIELDS, 0)
    dmap = np.zeros((0, 0), dtype=np.uint64)
    pmap = np.zeros((0, 0), dtype=np.uint64)
    if n_u > 0 and n_v > 0:
        dmap, counts["dir_binned"], counts["dir_outside"] = direction_map(v, n_u, n_v)
    if n_x > 0 and n_y > 0:
        pmap, counts["pos_binned"], counts["pos_outside"], counts["upward"] = plane_map(p, v, n_x, n_y, plane_z, half_extent)
    return dmap, pmap, counts, int(sel.sum())


def exitmap_of_spec(endstates, cfg, spec):
    return exitmap_np(endstates, cfg.exit_port_z, spec.n_u, spec.n_v, spec.n_x, spec.n_y, spec.plane_z, spec.half_extent)
