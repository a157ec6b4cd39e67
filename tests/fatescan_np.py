"""numpy restatement of the fate scan (csrc/isx_device.hpp: fate_step) -- TEST INFRASTRUCTURE.

The scan walks the interactions j = 0, 1, ... of a ray over its Philox words (block j/2 of stream 0, words 2(j&1) and 2(j&1)+1) and
either SETTLES the ray as absorbed at j or leaves it to the trace kernel at j:

    j >= J_CAP                      -> TRACE
    wb_j >= rho_thr                 -> ABSORBED (final; n_points = j + 2)
    j + 2 > max_points              -> TRACE   (the bounce limit ends the ray here)
    wa_j > w_leave                  -> TRACE   (w_leave = floor(W_leave - MARG))
    |wa_j - wa_{j-1}| < SEP         -> TRACE   (wa_{-1} = the word equivalent of the first strike's z)
    else on to j + 1

Philox4x32-10 is vectorised here and checked against the oracle's isxo_philox4x32_10 in tests/test_fate_scan_cpu.py; the
thresholds are computed with the expressions of isx_api.hip (prepare_geom, fate_consts)."""
import math

import numpy as np

MARG, SEP, J_CAP = 1 << 16, 1 << 17, 1024
ABSORBED, TRACE = 2, 0
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """counter words (arrays or scalars, values < 2^32) and the two key words -> the four output words, uint64 arrays < 2^32"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LO for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = _M0 * c0          # (32 x 32 bits: fits 64)
        p1 = _M1 * c2
        n0 = (p1 >> _S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> _S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & _LO, n2, p0 & _LO
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def draw_block(seed, ray, block, stream=0):
    """the words of Philox block `block` of ray index array `ray` (uint64): counter (ray lo, ray hi, block, stream), key = seed"""
    ray = np.asarray(ray, dtype=np.uint64)
    return philox4x32_10(ray & _LO, ray >> _S32, np.uint64(block), np.uint64(stream), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def sphere_z(w):
    """1 - 2 (w + 1/2) 2^-32, exact in binary64"""
    return 1.0 - 2.0 ** -32 - np.asarray(w, dtype=np.float64) * 2.0 ** -31


def thresholds(cfg):
    """-> dict(rho_thr, w_leave, w_q0, sep, j_cap, limit, ok): prepare_geom's and fate_consts' expressions, operation for operation"""
    r_in = cfg.r_in
    th = cfg.theta_max_deg * math.pi / 180.0
    zcut_in = r_in * math.cos(th)
    rin2 = r_in * r_in
    x = math.ldexp(cfg.reflectance, 32) - 0.5
    rho_thr = 0 if not x > 0.0 else (1 << 32 if x >= 4294967296.0 else int(math.ceil(x)))
    dx, dy, dz = cfg.dir[0], cfg.dir[1], cfg.dir[2]
    mag = math.sqrt(dx * dx + dy * dy + dz * dz)
    vx, vy, vz = dx / mag, dy / mag, dz / mag
    px, py, pz = cfg.src[0], cfg.src[1], cfg.src[2]
    w_leave = (1.0 - 2.0 ** -32 - zcut_in / r_in) * 2.0 ** 31 - float(MARG)
    b = px * vx + py * vy + pz * vz
    ci = (px * px + py * py + pz * pz) - rin2
    di = b * b - ci
    ok = (cfg.source_model == 0 and cfg.surface_model == 0 and cfg.lambertian != 0 and cfg.trace_mode == 0 and
          0.0 <= w_leave < 4294967296.0 and ci < -1e-9 * rin2 and di >= 0.0)
    out = {"rho_thr": rho_thr, "sep": SEP, "j_cap": J_CAP, "limit": int(cfg.max_points), "w_leave": 0, "w_q0": 0, "ok": False,
           "zcut_in": zcut_in}
    if ok:
        out["w_leave"] = int(math.floor(w_leave))
        q0z = pz + (math.sqrt(di) - b) * vz
        wq = math.floor((1.0 - 2.0 ** -32 - q0z / r_in) * 2.0 ** 31 + 0.5)
        ok = 0.0 <= wq <= float(out["w_leave"])
        if ok:
            out["w_q0"] = int(wq)
    out["ok"] = bool(ok)
    return out


def fate_scan_np(cfg, n, seed, first=0):
    """-> (fate int32[n], order int32[n], scanned): fate ABSORBED (2) settled at interaction order, or TRACE (0) given up at
    interaction order; scanned = interactions whose words the scan looked at, over all rays"""
    t = thresholds(cfg)
    assert t["ok"], "the scan does not serve this configuration"
    fate = np.full(n, -1, dtype=np.int32)
    order = np.zeros(n, dtype=np.int32)
    idx = np.arange(n, dtype=np.int64)                         # rays still undecided
    ray = np.uint64(first) + np.arange(n, dtype=np.uint64)
    wprev = np.full(n, t["w_q0"], dtype=np.int64)
    scanned = 0
    j = 0
    while idx.size:
        w = draw_block(seed, ray[idx], j >> 1)
        for half in (0, 1):
            if not idx.size:
                break
            wa = w[2 * half].astype(np.int64)
            wb = w[2 * half + 1].astype(np.int64)
            if j >= t["j_cap"]:
                fate[idx] = TRACE
                order[idx] = j
                idx = idx[:0]
                break
            scanned += idx.size
            absorbed = wb >= t["rho_thr"]
            if j + 2 > t["limit"]:
                trace = ~absorbed
            else:
                trace = ~absorbed & ((wa > t["w_leave"]) | (np.abs(wa - wprev[idx]) < t["sep"]))
            done = absorbed | trace
            fate[idx[absorbed]] = ABSORBED
            fate[idx[trace]] = TRACE
            order[idx[done]] = j
            go = ~done
            wprev[idx[go]] = wa[go]
            idx = idx[go]
            w = tuple(x[go] for x in w)
            j += 1
    assert (fate >= 0).all()
    return fate, order, scanned
