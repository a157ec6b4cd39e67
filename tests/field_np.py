"""The scene patch field of include/isx.h (isx_scene_patch_field) restated on a walk's per-ray arrays -- TEST INFRASTRUCTURE.

A ray is selected if its fate slot (response_np.fates: what isxo_scene_walk reports per ray -- status, last point, last class,
last baffle) equals the spec's patch; the rule of the contract is then applied to n_points, last_point and direction as the walk
reports them, vectorised in numpy float64 with every expression in the contract's order (numpy's multiply, add, divide and sqrt
are the correctly rounded IEEE operations, and it fuses nothing).  from_walk() asserts the contract's identities against the
walk's own patch_absorbed.  tests/test_patch_field_cpu.py holds it against an independent per-ray loop in Python floats.
"""
import numpy as np

import response_np as R

BINNED, POS_OUTSIDE, DIR_OUTSIDE, BEHIND, DIRECT = 0, 1, 2, 3, 4


def frame(fspec):
    """(patch, (n_x, n_y, n_u, n_v), h, s, axis, e1, e2) of a PatchFieldSpec, as Python numbers"""
    return (int(fspec.patch), (int(fspec.n_x), int(fspec.n_y), int(fspec.n_u), int(fspec.n_v)), float(fspec.half_extent),
            float(fspec.pos_scale), [float(x) for x in fspec.axis], [float(x) for x in fspec.e1], [float(x) for x in fspec.e2])


def position(fspec, r_in, last_point):
    """(X, Y) of the contract for an array of points, in its order of operations"""
    _, _, _, s, ax, e1, e2 = frame(fspec)
    q = np.asarray(last_point, dtype=np.float64).reshape(-1, 3)
    qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
    inv = 1.0 / float(r_in)
    with np.errstate(all="ignore"):
        c = ((qx * ax[0] + qy * ax[1]) + qz * ax[2]) * inv
        w = np.sqrt(0.5 / (1.0 + c))
        a = (qx * e1[0] + qy * e1[1]) + qz * e1[2]
        b = (qx * e2[0] + qy * e2[1]) + qz * e2[2]
        X = ((a * inv) * w) * s
        Y = ((b * inv) * w) * s
    return X, Y


def classify(fspec, r_in, n_points, last_point, direction):
    """the rule on the selected rays' arrays -> (branch[n] in {BINNED, POS_OUTSIDE, DIR_OUTSIDE, BEHIND, DIRECT}, bin[n] (valid
    where BINNED))"""
    _, (n_x, n_y, n_u, n_v), h, _, ax, e1, e2 = frame(fspec)
    d = np.asarray(direction, dtype=np.float64).reshape(-1, 3)
    npts = np.asarray(n_points).reshape(-1)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    X, Y = position(fspec, r_in, last_point)
    with np.errstate(all="ignore"):
        cd = (dx * ax[0] + dy * ax[1]) + dz * ax[2]
        fx = (X + 1.0) * 0.5 * n_x
        fy = (Y + 1.0) * 0.5 * n_y
        ix, iy = np.floor(fx), np.floor(fy)
        pos_in = (ix >= 0) & (ix < n_x) & (iy >= 0) & (iy < n_y)      # (NaN and inf compare false)
        mag = np.sqrt((dx * dx + dy * dy) + dz * dz)
        a = (dx * e1[0] + dy * e1[1]) + dz * e1[2]
        b = (dx * e2[0] + dy * e2[1]) + dz * e2[2]
        U = -(a / mag)
        V = -(b / mag)
        fu = (U + h) / (2.0 * h) * n_u
        fv = (V + h) / (2.0 * h) * n_v
        iu, iv = np.floor(fu), np.floor(fv)
        dir_in = (iu >= 0) & (iu < n_u) & (iv >= 0) & (iv < n_v)
    direct = npts == 2
    behind = ~direct & ~(cd > 0.0)
    pos_out = ~direct & ~behind & ~pos_in
    dir_out = ~direct & ~behind & pos_in & ~dir_in
    binned = ~direct & ~behind & pos_in & dir_in
    branch = np.where(direct, DIRECT, np.where(behind, BEHIND, np.where(pos_out, POS_OUTSIDE, np.where(dir_out, DIR_OUTSIDE, BINNED))))

    def z(v):
        return np.where(binned, v, 0).astype(np.int64)

    bins = ((z(iy) * n_x + z(ix)) * n_v + z(iv)) * n_u + z(iu)
    return branch.astype(np.int64), bins


def selected(w, cfg, fspec):
    """the rays of a walk that the spec's patch absorbed"""
    return R.fates(w, cfg) == int(fspec.patch)


def from_walk(w, cfg, fspec):
    """(field[n_y, n_x, n_v, n_u] uint64, counts[5] uint64: binned, pos_outside, dir_outside, behind, direct) of the rays of
    oracle.scene_walk(cfg, scene, ...)"""
    patch, (n_x, n_y, n_u, n_v) = frame(fspec)[:2]
    sel = selected(w, cfg, fspec)
    branch, bins = classify(fspec, cfg.r_in, w["n_points"][sel], w["last_point"][sel], w["direction"][sel])
    counts = np.bincount(branch, minlength=5).astype(np.uint64)
    field = np.bincount(bins[branch == BINNED], minlength=n_x * n_y * n_u * n_v).astype(np.uint64).reshape(n_y, n_x, n_v, n_u)
    assert 0 <= patch < w["patch_absorbed"].size - 2, "the patch is one of the scene's"
    assert int(counts.sum()) == int(sel.sum()) == int(w["patch_absorbed"][patch]), \
        "binned + pos_outside + dir_outside + behind + direct == patch_absorbed[patch]"
    assert int(field.sum()) == int(counts[BINNED]), "field sums to binned"
    return field, counts
