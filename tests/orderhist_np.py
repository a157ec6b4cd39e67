"""numpy restatement of the bounce-order histograms' contract (include/isx.h, isx_order_hist) over end-state arrays, and of the
reweighting formula (isx_order_reweight) -- TEST INFRASTRUCTURE: the reference every order-histogram test compares against, fed
from the oracle's trace_endstates().

Nothing is replayed: status and n_points of a ray say its class and its order, its final direction the dz bin."""
import numpy as np

EXITED, ABSORBED, SUSPENDED = 1, 2, 3
CLASSES = ("port", "exited_other", "absorbed", "suspended")


def classify(endstates, exit_port_z):
    """-> (k, c) per ray: the order (n_points - 2 if EXITED else n_points - 1) and the class (0 counted below z, 1 exited
    otherwise, 2 absorbed, 3 suspended)."""
    status, npts, lp, _ = endstates
    status = np.asarray(status)
    npts = np.asarray(npts, dtype=np.int64)
    assert np.isin(status, (EXITED, ABSORBED, SUSPENDED)).all()
    exited = status == EXITED
    k = np.where(exited, npts - 2, npts - 1)
    c = np.where(exited, np.where(lp[:, 2] < exit_port_z, 0, 1), np.where(status == ABSORBED, 2, 3))
    return k, c


def order_hist_np(endstates, exit_port_z, n_orders, n_dz):
    """endstates = (status, n_points, last_point[n, 3], direction[n, 3]) as trace_endstates() returns them.
    -> (hist[4, n_orders] uint64, port_dz[n_orders, n_dz] uint64, {"overflow": [4], "dz_outside": int})."""
    k, c = classify(endstates, exit_port_z)
    assert (k >= 0).all()
    inside = k < n_orders
    overflow = [int(((c == cl) & ~inside).sum()) for cl in range(4)]
    hist = np.bincount(c[inside] * n_orders + k[inside], minlength=4 * n_orders).astype(np.uint64).reshape(4, n_orders)
    port_dz = np.zeros((n_orders, n_dz), dtype=np.uint64)
    dz_outside = 0
    if n_dz > 0:
        sel = inside & (c == 0)
        vz = np.asarray(endstates[3], dtype=np.float64)[sel, 2]
        with np.errstate(all="ignore"):
            f = (vz + 1.0) * 0.5 * n_dz          # IEEE double, left to right
            fl = np.floor(f)
        ok = (fl >= 0) & (fl < n_dz)             # (NaN and inf compare false)
        b = fl[ok].astype(np.int64)
        port_dz = np.bincount(k[sel][ok] * n_dz + b, minlength=n_orders * n_dz).astype(np.uint64).reshape(n_orders, n_dz)
        dz_outside = int((~ok).sum())
    return hist, port_dz, {"overflow": overflow, "dz_outside": dz_outside}


def order_hist_of_spec(endstates, cfg, spec):
    return order_hist_np(endstates, cfg.exit_port_z, spec.n_orders, spec.n_dz)


def census_np(endstates, exit_port_z):
    """the census fields the end states determine"""
    status, _, lp, _ = endstates
    status = np.asarray(status)
    return {"launched": int(status.size), "exited": int((status == EXITED).sum()),
            "counted_below_z": int(((status == EXITED) & (lp[:, 2] < exit_port_z)).sum()),
            "absorbed": int((status == ABSORBED).sum()), "suspended": int((status == SUSPENDED).sum())}


def check_identities(hist, port_dz, counts, census, n_dz):
    """the identities of include/isx.h that hold per call (census: dict or a Stats)"""
    get = census.get if isinstance(census, dict) else (lambda f: getattr(census, f))
    ov = counts["overflow"]
    s = [int(hist[c].sum()) for c in range(4)]
    assert s[0] + ov[0] == get("counted_below_z")
    assert s[1] + ov[1] == get("exited") - get("counted_below_z")
    assert s[2] + ov[2] == get("absorbed")
    assert s[3] + ov[3] == get("suspended")
    assert sum(s) + sum(ov) == get("launched")
    if n_dz > 0:
        assert int(port_dz.sum()) + counts["dz_outside"] == s[0]
        if counts["dz_outside"] == 0:
            assert np.array_equal(port_dz.sum(axis=1), hist[0])
    else:
        assert port_dz.size == 0 and counts["dz_outside"] == 0


def reweight_np(port_hist, launched, rho0, rho):
    """isx_order_reweight: -> (fraction, sigma) for one rho; the sums in increasing k."""
    h = np.asarray(port_hist, dtype=np.float64)
    w = np.power(np.float64(rho) / np.float64(rho0), np.arange(h.size, dtype=np.float64))
    s1 = s2 = 0.0
    for hk, wk in zip(h, w):
        s1 += hk * wk
        s2 += hk * wk * wk
    n = float(launched)
    var = s2 - s1 * s1 / n
    return s1 / n, np.sqrt(max(var, 0.0)) / n
