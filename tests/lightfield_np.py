"""numpy restatement of the port light field's contract (include/isx.h, isx_light_field) over end-state arrays --
TEST INFRASTRUCTURE: the reference every light-field test compares against, fed from the oracle's trace_endstates().

Built on exitmap_np._axis_bin and the same left-to-right expressions as the exit maps' restatement (IEEE double; numpy never
fuses a multiply and an add).  The classification is in the header's order: upward, position bin, direction bin."""
import numpy as np

from exitmap_np import EXITED, _axis_bin

COUNT_FIELDS = ("binned", "pos_outside", "dir_outside", "upward")


def light_field(p, v, n_u, n_v, n_x, n_y, plane_z, half_extent):
    """p[k, 3], v[k, 3]: last points and final directions of counted rays -> (field[n_y, n_x, n_v, n_u] uint64, counts dict)."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    down = v[:, 2] < 0.0                       # -0.0, +0.0 and NaN are "upward"
    upward = int((~down).sum())
    p, v = p[down], v[down]
    with np.errstate(all="ignore"):
        t = (np.float64(plane_z) - p[:, 2]) / v[:, 2]
        x = p[:, 0] + t * v[:, 0]
        y = p[:, 1] + t * v[:, 1]
        h = np.float64(half_extent)
        ix = _axis_bin((x + h) / (2.0 * h) * n_x, n_x)
        iy = _axis_bin((y + h) / (2.0 * h) * n_y, n_y)
    pos = (ix >= 0) & (iy >= 0)
    pos_outside = int((~pos).sum())
    ix, iy, v = ix[pos], iy[pos], v[pos]
    iu = _axis_bin((v[:, 0] + 1.0) * 0.5 * n_u, n_u)
    iv = _axis_bin((v[:, 1] + 1.0) * 0.5 * n_v, n_v)
    ok = (iu >= 0) & (iv >= 0)
    word = ((iy[ok] * n_x + ix[ok]) * n_v + iv[ok]) * n_u + iu[ok]
    field = np.bincount(word, minlength=n_x * n_y * n_u * n_v).astype(np.uint64).reshape(n_y, n_x, n_v, n_u)
    return field, {"binned": int(ok.sum()), "pos_outside": pos_outside, "dir_outside": int((~ok).sum()), "upward": upward}


def light_field_np(endstates, exit_port_z, n_u, n_v, n_x, n_y, plane_z, half_extent):
    """endstates = (status, n_points, last_point[n, 3], direction[n, 3]) as trace_endstates() returns them.
    -> (field[n_y, n_x, n_v, n_u], counts dict, counted)."""
    status, _, lp, d = endstates
    sel = (np.asarray(status) == EXITED) & (lp[:, 2] < exit_port_z)
    field, counts = light_field(lp[sel], d[sel], n_u, n_v, n_x, n_y, plane_z, half_extent)
    return field, counts, int(sel.sum())


def light_field_of_spec(endstates, cfg, spec):
    return light_field_np(endstates, cfg.exit_port_z, spec.n_u, spec.n_v, spec.n_x, spec.n_y, spec.plane_z, spec.half_extent)
