"""numpy restatement of the exit-line rule (csrc/isx_kernels.hpp: isx_exit_lines_kernel, decide_approx) --
TEST INFRASTRUCTURE.

A ray that the fate scan (tests/fatescan_np.py) leaves at interaction j has provably reached the mirror patch j + 1 times.  It is
ACCEPTED -- its exit line formed from its words -- if at j

    j < J_CAP, wb_j < rho_thr, j + 2 <= max_points, wa_j >= w_exit          (w_exit = w_leave + 2 MARG + 2 >= W_leave + MARG)
    |r_in s_j - p'| >= CHORD r_in and |p' - p''| >= CHORD r_in               (p' = r_in s_{j-1}, p'' = r_in s_{j-2}; q0 below 0)
    p'.V' < -1e-3 r_in, V'.z <= -MIN_DZ                                       (V' = unit(r_in s_j - p'))
    on the planes z = zcut_in (1 - 1e-6), zcut_out, zcut_out (1 + 1e-6) the line lies within the rim cone's radius there (the
    middle one: the outer sphere's, less 1e-6) by more than 2.5 (eps_p + t eps_V) / |V'.z| + 1e-9 of the radius
    the box point lies below exit_port_z by more than 2.5 (eps_p + 4 H eps_V) + 1e-9 H

with eps_p = ((j + 2) 32 u + 4e-15) r_in^2 1.001 / |p' - p''| + 1e-14 r_in and eps_V = 2.1 eps_p / |r_in s_j - p'| + 2e-14.  The
bound the binning kernel gets is eps = eps_p + reach eps_V + 4e-15 H + eps_ref (the kernel's expressions).  The azimuth's cosine
and sine come from numpy here, from circle_point_psi's polynomials on the device: 1e-16, far below every bound."""
import math

import numpy as np

import fatescan_np as fs

CHORD, MIN_DZ = 0.05, 0.02
STEP = 32.0 * 2.0 ** -53


def _words(seed, ray, j):
    """(wa_j, wb_j) of interaction j (an int64 array, >= 0) of the rays"""
    w = fs.philox4x32_10(ray & fs._LO, ray >> fs._S32, (j >> 1).astype(np.uint64), np.uint64(0), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    odd = (j & 1) == 1
    return np.where(odd, w[2], w[0]).astype(np.int64), np.where(odd, w[3], w[1]).astype(np.int64)


def _wall_point(cfg, t, wa, wb):
    zz = fs.sphere_z(wa)
    s2 = np.sqrt(1.0 - zz * zz)
    inv_thr = 1.0 / t["rho_thr"]
    psi = wb.astype(np.float64) * (inv_thr * (math.pi / 2)) + (0.5 * inv_thr - 0.5) * (math.pi / 2)
    return np.stack([cfg.r_in * s2 * np.cos(4.0 * psi), cfg.r_in * s2 * np.sin(4.0 * psi), cfg.r_in * zz], axis=1)


def exit_lines_np(cfg, orc, n, seed, first=0):
    """-> dict: idx (rays accepted, indices into the range), j, P, V (the approximate line: box point, unit direction), eps_p,
    eps_V, eps (the bound handed to the binning kernel), listed (rays the scan left), n_points (= j + 3)"""
    t = fs.thresholds(cfg)
    assert t["ok"] and t["rho_thr"] > 0
    fate, order, _ = fs.fate_scan_np(cfg, n, seed, first)
    cand = np.flatnonzero(fate == fs.TRACE)
    j = order[cand].astype(np.int64)
    ray = np.uint64(first) + cand.astype(np.uint64)
    r_in, H = cfg.r_in, cfg.box_half
    th = cfg.theta_max_deg * math.pi / 180.0
    zcut_in, zcut_out, tanc = r_in * math.cos(th), cfg.r_out * math.cos(th), abs(math.tan(th))
    d = np.array(cfg.dir[:])
    kind0, q0 = orc.next_boundary(cfg, np.array(cfg.src[:]), d / np.sqrt(d @ d), 0)
    assert kind0 == 1
    wa, wb = _words(seed, ray, j)
    w_exit = t["w_leave"] + 2 * fs.MARG + 2
    ok = (j < t["j_cap"]) & (wb < t["rho_thr"]) & (j + 2 <= t["limit"]) & (wa >= w_exit)
    cand, j, ray, wa, wb = cand[ok], j[ok], ray[ok], wa[ok], wb[ok]
    p = np.repeat(q0[None, :], j.size, axis=0)
    pp = np.repeat(q0[None, :], j.size, axis=0)
    m1 = j >= 1
    p[m1] = _wall_point(cfg, t, *_words(seed, ray[m1], j[m1] - 1))
    m2 = j >= 2
    pp[m2] = _wall_point(cfg, t, *_words(seed, ray[m2], j[m2] - 2))
    prev = np.where(m1, np.linalg.norm(p - pp, axis=1), r_in)
    v = _wall_point(cfg, t, wa, wb) - p
    chord = np.linalg.norm(v, axis=1)
    V = v / chord[:, None]
    ok = (prev >= CHORD * r_in) & (chord >= CHORD * r_in) & (np.einsum("ij,ij->i", p, V) < -1e-3 * r_in) & (V[:, 2] <= -MIN_DZ)
    eps_p = ((j + 2) * STEP + 4e-15) * (r_in * r_in) * 1.001 / np.maximum(prev, 1e-300) + 1e-14 * r_in
    eps_V = 2.1 * eps_p / np.maximum(chord, 1e-300) + 2e-14
    with np.errstate(divide="ignore", invalid="ignore"):
        iz = 1.0 / V[:, 2]
        for zp, rho in ((zcut_in * (1 - 1e-6), tanc * abs(zcut_in * (1 - 1e-6))),
                        (zcut_out, math.sqrt(max(cfg.r_out ** 2 - zcut_out ** 2, 0.0)) * (1 - 1e-6)),
                        (zcut_out * (1 + 1e-6), tanc * abs(zcut_out * (1 + 1e-6)))):
            tt = (zp - p[:, 2]) * iz
            x, y = p[:, 0] + tt * V[:, 0], p[:, 1] + tt * V[:, 1]
            lim = rho * (1 - 1e-9) - 2.5 * (eps_p + tt * eps_V) * (-iz)
            ok &= (tt > 0) & (lim > 0) & (x * x + y * y < lim * lim)
        # the box (next_hit_generic's last lines)
        tb = np.full(j.size, np.inf)
        for k in range(3):
            tk = np.where(V[:, k] > 0, (H - p[:, k]) / V[:, k], np.where(V[:, k] < 0, (-H - p[:, k]) / V[:, k], np.inf))
            tb = np.minimum(tb, tk)
    P = p + tb[:, None] * V
    ok &= P[:, 2] < cfg.exit_port_z - (2.5 * (eps_p + 4.0 * H * eps_V) + 1e-9 * H)
    R = cfg.det_distance
    reach = 2.1 * (1.001 * r_in + abs(cfg.exit_port_z) + R + cfg.det_diameter / 2)
    wz = P[:, 2] - cfg.exit_port_z
    eps_ref = 1e-14 * (4.0 * (P[:, 0] ** 2 + P[:, 1] ** 2 + wz ** 2 + R * R) + (cfg.det_diameter / 2) ** 2) / R
    eps = eps_p + reach * eps_V + 4e-15 * H + eps_ref
    return {"idx": cand[ok], "j": j[ok], "P": P[ok], "V": V[ok], "eps_p": eps_p[ok], "eps_V": eps_V[ok], "eps": eps[ok],
            "eps_ref": eps_ref[ok], "listed": int((fate == fs.TRACE).sum()), "n_points": j[ok] + 3}


def nearest_to(o, P, V):
    """the point of each line (P, unit V) nearest to the point o"""
    w = P - o
    return P - np.einsum("ij,ij->i", w, V)[:, None] * V


def decide_approx_np(cfg, det, P, V, eps):
    """decide_approx for one detector entry (x, y, z, nx, ny, nz) and arrays of lines: -> (g, band): the candidate is decided by the
    sign of g iff |g| > band (and the |dot| cut is clear); plain numpy on the detector table's own centre and normal"""
    c, nrm = det[:3], det[3:]
    o = np.array([0.0, 0.0, cfg.exit_port_z])
    R, hw2 = cfg.det_distance, (cfg.det_diameter / 2) ** 2
    Q = nearest_to(o, P, V)
    dot = V @ nrm
    num = (Q - c) @ nrm
    mdv = -2.0 * np.einsum("ij,ij->i", Q - c, V)
    D2 = np.einsum("ij,ij->i", Q - c, Q - c)
    ddw = D2 - hw2
    g = dot * (dot * ddw + num * mdv) + num * num
    e = eps
    a_dot, a_num, a_mdv = np.abs(dot) + e / R, np.abs(num) + e, np.abs(mdv) + 4 * e
    Dq = np.sqrt(D2) + e
    a_ddw = np.abs(ddw) + 2 * Dq * e
    dg = 2 * a_dot * (e / R * a_ddw + a_dot * Dq * e) + (e / R * a_num + a_dot * e) * a_mdv + 4 * e * a_dot * a_num + 2 * a_num * e
    Pc = P - c
    scale_p = 2.0 * np.einsum("ij,ij->i", Pc, Pc) + hw2
    band = 1.25 * dg + 1e-13 * scale_p
    cut = np.abs(dot) < 1.000001e-10 + (e / R + 1e-14)
    return g, np.where(cut, np.inf, band)
