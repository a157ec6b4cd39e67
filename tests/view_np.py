"""The scene view of include/isx.h (isx_scene_view) restated on a walk's per-ray arrays -- TEST INFRASTRUCTURE.

A ray is selected if its fate slot (response_np.fates: what isxo_scene_walk reports per ray -- status, last point, last class,
last baffle) equals the spec's patch; the rule of the contract is then applied to n_points and direction as the walk reports
them, vectorised in numpy float64 with every expression in the contract's order (numpy's multiply, add, divide and sqrt are the
correctly rounded IEEE operations, and it fuses nothing).  from_walk() asserts the contract's identities against the walk's own
patch_absorbed.  tests/test_scene_view_cpu.py holds it against an independent per-ray loop in Python floats.
"""
import numpy as np

import response_np as R

BINNED, OUTSIDE, BEHIND, DIRECT = 0, 1, 2, 3


def frame(vspec):
    """(patch, n_u, n_v, h, axis, e1, e2) of a ViewSpec, as Python numbers"""
    return (int(vspec.patch), int(vspec.n_u), int(vspec.n_v), float(vspec.half_extent), [float(x) for x in vspec.axis],
            [float(x) for x in vspec.e1], [float(x) for x in vspec.e2])


def classify(vspec, n_points, direction):
    """the rule on the selected rays' arrays -> (branch[n] in {BINNED, OUTSIDE, BEHIND, DIRECT}, bin[n] (valid where BINNED))"""
    _, n_u, n_v, h, ax, e1, e2 = frame(vspec)
    d = np.asarray(direction, dtype=np.float64).reshape(-1, 3)
    npts = np.asarray(n_points).reshape(-1)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        c = (dx * ax[0] + dy * ax[1]) + dz * ax[2]
        mag = np.sqrt((dx * dx + dy * dy) + dz * dz)
        a = (dx * e1[0] + dy * e1[1]) + dz * e1[2]
        b = (dx * e2[0] + dy * e2[1]) + dz * e2[2]
        U = -(a / mag)
        V = -(b / mag)
        fu = (U + h) / (2.0 * h) * n_u
        fv = (V + h) / (2.0 * h) * n_v
        iu, iv = np.floor(fu), np.floor(fv)
        inside = (iu >= 0) & (iu < n_u) & (iv >= 0) & (iv < n_v)      # (NaN and inf compare false)
    direct = npts == 2
    behind = ~direct & ~(c > 0.0)
    binned = ~direct & ~behind & inside
    branch = np.where(direct, DIRECT, np.where(behind, BEHIND, np.where(binned, BINNED, OUTSIDE))).astype(np.int64)
    bins = np.where(binned, np.where(binned, iv, 0) * n_u + np.where(binned, iu, 0), 0).astype(np.int64)
    return branch, bins


def selected(w, cfg, vspec):
    """the rays of a walk that the spec's patch absorbed"""
    return R.fates(w, cfg) == int(vspec.patch)


def from_walk(w, cfg, vspec):
    """(view[n_v, n_u] uint64, counts[4] uint64: binned, outside, behind, direct) of the rays of oracle.scene_walk(cfg, scene, ...)"""
    patch, n_u, n_v = int(vspec.patch), int(vspec.n_u), int(vspec.n_v)
    sel = selected(w, cfg, vspec)
    branch, bins = classify(vspec, w["n_points"][sel], w["direction"][sel])
    counts = np.bincount(branch, minlength=4).astype(np.uint64)
    view = np.bincount(bins[branch == BINNED], minlength=n_u * n_v).astype(np.uint64).reshape(n_v, n_u)
    assert 0 <= patch < w["patch_absorbed"].size - 2, "the patch is one of the scene's"
    assert int(counts.sum()) == int(sel.sum()) == int(w["patch_absorbed"][patch]), "binned + outside + behind + direct == patch_absorbed[patch]"
    assert int(view.sum()) == int(counts[BINNED]), "view sums to binned"
    return view, counts
