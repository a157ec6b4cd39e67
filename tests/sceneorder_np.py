"""The scene order histograms of include/isx.h (isx_scene_order_hist) restated on a walk's per-ray arrays -- TEST INFRASTRUCTURE.

The fate slot of a ray is the scene response's (tests/response_np.py: fates, from status, last point, last class and last baffle
as isxo_scene_walk reports them); its order is isx_order_hist's rule on status and n_points; the histograms are one bincount over
fate * n_orders + k, the rays with k >= n_orders counted per fate apart.  from_walk() asserts the contract's row identities against
the walk's own counters -- patch_absorbed, baffle_absorbed, the census -- and that the orders sum to the walk's wall_hits.
"""
import numpy as np

import response_np as R

FATES, BAFFLE0, PORT, EXITED_OTHER, SUSPENDED = R.FATES, R.BAFFLE0, R.PORT, R.EXITED_OTHER, R.SUSPENDED


def orders(w):
    """k of every ray: n_points - 2 for a ray that exited (its last point is no interaction), else n_points - 1"""
    npts = w["n_points"].astype(np.int64)
    k = np.where(w["status"] == R.EXITED, npts - 2, npts - 1)
    assert k.size == 0 or int(k.min()) >= 0
    return k


def from_walk(w, cfg, n_orders):
    """(hist[21, n_orders], overflow[21]) of the rays of oracle.scene_walk(cfg, scene, n, seed, first)"""
    n_orders = int(n_orders)
    f, k = R.fates(w, cfg), orders(w)
    assert int(k.sum()) == w["census"]["wall_hits"], "the orders sum to wall_hits"
    over = k >= n_orders
    hist = np.bincount(f[~over] * n_orders + k[~over], minlength=FATES * n_orders).astype(np.uint64).reshape(FATES, n_orders)
    overflow = np.bincount(f[over], minlength=FATES).astype(np.uint64)
    rows = hist.sum(axis=1) + overflow
    P = w["patch_absorbed"].size - 2
    assert np.array_equal(rows[:P + 2], w["patch_absorbed"]) and not rows[P + 2:BAFFLE0].any(), "rows 0..9 are patch_absorbed"
    ba = np.zeros(8, dtype=np.uint64)
    ba[:w["baffle_absorbed"].size] = w["baffle_absorbed"].reshape(-1)
    assert np.array_equal(rows[BAFFLE0:PORT], ba), "rows 10..17 are baffle_absorbed"
    c = w["census"]
    assert rows[PORT] == c["counted_below_z"] and rows[PORT] + rows[EXITED_OTHER] == c["exited"] and rows[SUSPENDED] == c["suspended"]
    assert int(rows.sum()) == c["launched"] == k.size
    assert not hist[:PORT, 0].any(), "an absorbed ray has at least one interaction"
    if not overflow.any():
        assert int((hist * np.arange(n_orders, dtype=np.uint64)).sum()) == c["wall_hits"]
    return hist, overflow


def reweight(hist, launched, scale, rho):
    """isx_scene_order_reweight's formulas, operation for operation: rho[f] the reflectance of the surface slot f < 18 absorbs on,
    a negative value for a slot the scene cannot fill -> (fraction[n_scale, 21], sigma[n_scale, 21])"""
    import math
    hist = np.asarray(hist, dtype=np.uint64)
    K = hist.shape[1]
    n = float(launched)
    frac, sig = np.zeros((len(scale), FATES)), np.zeros((len(scale), FATES))
    for i, t in enumerate(float(x) for x in scale):
        for f in range(FATES):
            s1 = s2 = 0.0
            if f >= PORT:
                for k in range(K):
                    wk, h = math.pow(t, float(k)), float(hist[f, k])
                    s1 += h * wk
                    s2 += h * wk * wk
            elif rho[f] < 0:
                pass
            elif rho[f] == 1.0:
                s1 = s2 = 0.0 if t == 1.0 else math.nan
            else:
                a = (1.0 - t * rho[f]) / (1.0 - rho[f])
                for k in range(1, K):
                    wk, h = a * math.pow(t, float(k) - 1.0), float(hist[f, k])
                    s1 += h * wk
                    s2 += h * wk * wk
            frac[i, f] = s1 / n
            var = s2 - s1 * s1 / n
            sig[i, f] = var if math.isnan(var) else math.sqrt(var if var > 0 else 0.0) / n
    return frac, sig


def moments(hist, overflow):
    """isx_scene_order_moments' formulas, operation for operation -> (mean[21], sd[21])"""
    import math
    hist = np.asarray(hist, dtype=np.uint64)
    mean, sd = np.full(FATES, np.nan), np.full(FATES, np.nan)
    for f in range(FATES):
        N = A = B = 0.0
        for k in range(hist.shape[1]):
            h, x = float(hist[f, k]), float(k)
            N += h
            A += x * h
            B += x * x * h
        if N > 0 and int(overflow[f]) == 0:
            m = A / N
            var = B / N - m * m
            mean[f], sd[f] = m, math.sqrt(var if var > 0 else 0.0)
    return mean, sd


def surface_rho(cfg, scene):
    """rho[f] for the slots 0..17 of a scene (a ctypes SceneSpec): the patches', the wall's for the classes P and P + 1, each
    baffle's for its two sides; -1 where the scene has nothing"""
    rho = [-1.0] * PORT
    P, nb = int(scene.patches.n_patches), int(scene.baffles.n_baffles)
    for f in range(P):
        rho[f] = float(scene.patches.patch[f].reflectance)
    rho[P] = rho[P + 1] = float(cfg.reflectance)
    for b in range(nb):
        rho[BAFFLE0 + 2 * b] = rho[BAFFLE0 + 2 * b + 1] = float(scene.baffles.baffle[b].reflectance)
    return rho
