"""numpy float32 restatement of the TILT cull of isx_bin_cols_kernel's column producer (isx_kernels.hpp: prep_shared's slo / shi,
prep_cols' interval ends, col_cull behind cap_rows -- same formulas, same slack terms; DESIGN.md section 4.4, "the tilt of the
discs").  The detector of bin (i, j) is tilted: its disc reaches only rho_d cos(theta_i) out of the meridian plane of column j.
A hit needs a point x of the line with |phi^_j . (x - O)| <= rho_d cos(theta_i) whose parameter lies in the interval of the pass's
side; dmin_j, the least magnitude of the affine form over that interval, drops a (line, column) slot or trims its high-theta end.

  line_slots(P, V, cfg, variant)   variant 0: the slots of bandwin_np (no cull), 1: column test only, 2: column test + row trim
  edge_family(cfg)                 constructed lines AT the cull's edge: through the disc point c +- rho_d u2, in the plane
                                   perpendicular to phi^_j (dmin_j = rho_d cos(theta_i) exactly), shifted along phi^_j
  python tests/colcull_np.py [n_rays]      candidates per hit and slots per line of the default configuration, per variant

Lines without caps (band lines, far lines) keep bandwin_np's slots.  Test infrastructure only (imports the oracle)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import oracle as orc
import bandwin_np as BW
from boxwin_np import acos_cull, exact_hits

f32 = np.float32

# the slack terms of col_cull (isx_kernels.hpp), all scale-free: the end points are handed over in units of rho_d
REL = f32(4e-6)        # relative, on dmin_j / rho_d: rho_d and 1 / rho_d in binary32
ABS = f32(5e-7)        # times |xa| + |ya| + |xb| + |yb| (units of rho_d): the roundings of the two forms
ANGLE = f32(8e-5)      # rad: acos_cull underestimates by at most 6.8e-5 (every binary32 in [0, 1]; tests/test_col_cull_cpu.py)
ROWS = f32(1e-3)       # rows: the rounding of theta * inv_dth
S2 = f32(1e-6)         # times R^2, on slo^2 and shi^2: the cancellation in (R -+ rho)^2 - dO^2
SREL_LO, SREL_HI = f32(0.9999), f32(1.0001)
FALLBACK = f32(1.001)  # slo <= 1.001 rho: the interval starts at -1.001 rho (the hit may lie on the other side of the foot)


def interval(dO2, R, rho):
    """prep_shared: [slo, shi], the parameter interval (from the foot of O) of side 0; side 1 is its mirror image"""
    R2 = f32(R * R)
    rm, rp = f32(R - rho), f32(R + rho)
    slo = f32(np.sqrt(max(f32(0), f32(f32(rm * rm - dO2) - f32(S2 * R2)))) * SREL_LO)
    shi = f32(np.sqrt(f32(f32(rp * rp - dO2) + f32(S2 * R2))) * SREL_HI)
    if not slo > f32(FALLBACK * rho):
        slo = f32(-FALLBACK * rho)
    return slo, shi


def col_cull(xa, ya, xb, yb, cs, c32, s32, inv_dth, ilo, cnt, variant, slack=1.0):
    """the rows [ilo, ilo + cnt) of the columns (arrays) after the cull; (xa, ya), (xb, yb): interval ends / rho_d"""
    fa = (c32 * ya - s32 * xa).astype(f32)
    fb = (c32 * yb - s32 * xb).astype(f32)
    dm = np.minimum(np.abs(fa), np.abs(fb)).astype(f32)
    t = (dm * f32(f32(1) - f32(slack) * REL) - cs).astype(f32)
    act = ((fa * fb).astype(f32) > 0) & (t > 0) & (cnt > 0)
    th = (acos_cull(np.minimum(t, f32(1))) + f32(slack) * ANGLE).astype(f32)
    rows = f32(slack) * ROWS
    cnt = cnt.copy()
    if variant == 1:
        drop = act & (ilo.astype(f32) > (th * inv_dth + rows).astype(f32))      # the lower edge of the first row lies beyond
        cnt[drop] = 0
    elif variant == 2:
        hi = np.floor((th * inv_dth - f32(0.5) + rows).astype(f32)).astype(int)
        cnt = np.where(act, np.clip(hi - ilo + 1, 0, cnt), cnt)
    return cnt


def line_slots(P, V, cfg, variant=2, slack=1.0):
    """-> (kind, [(column, first row, rows)]) for ONE line as isx_bin_cols_kernel produces them (bandwin_np.line_slots + the cull).
    slack: multiplies the cull's own slack terms (1.0 is the kernel; the mutation check of the tests runs 0.5)"""
    n_phi, n_theta = cfg.n_phi, cfg.n_theta
    R, rho, portz = f32(cfg.det_distance), f32(cfg.det_diameter / 2), f32(cfg.exit_port_z)
    inv_dphi = f32(f32(n_phi) * f32(0.15915494309)); inv_dth = f32(f32(n_theta) * f32(0.63661977237))
    phi = (np.arange(n_phi) + 0.5) * 360.0 / n_phi * np.pi / 180
    c32, s32 = np.cos(phi).astype(f32), np.sin(phi).astype(f32)
    # ---- prep_shared (as in bandwin_np)
    wz = P[2] - float(portz)
    wv = P[0] * V[0] + P[1] * V[1] + wz * V[2]
    hx, hy, hz = P[0] - wv * V[0], P[1] - wv * V[1], wz - wv * V[2]
    dO2 = f32(hx * hx + hy * hy + hz * hz)
    R2 = f32(R * R)
    dO = BW.sqrt_cull(dO2)
    a1 = f32(dO + rho)
    if dO - rho > f32(1.001) * R or not a1 < f32(0.999) * R:
        return BW.line_slots(P, V, cfg)
    am = f32(dO - rho)
    smin = BW.sqrt_cull(R2 - a1 * a1)
    smx = BW.sqrt_cull(R2 - am * am)
    sM = f32(f32(0.5) * f32(smin + smx))
    ds = f32(smx - smin)
    d2 = f32(f32(f32(4.0) * rho * rho + ds * ds) * f32(1.0001) + f32(4e-3))
    s2w = f32(f32(0.25) * d2 / R2)
    cosw = f32(BW.sqrt_cull(max(f32(0), f32(1) - s2w)) - f32(2e-6))
    iL = f32(1) / BW.sqrt_cull(f32(dO2 + sM * sM))
    sinw = BW.sqrt_cull(max(f32(0), f32(1) - cosw * cosw))
    if not (cosw > f32(0.5) and sM * iL > sinw * f32(1.01) + f32(1e-3)):
        return BW.line_slots(P, V, cfg)
    ch = BW.sqrt_cull(f32(f32(2.0) * R2 * f32(f32(1) - cosw)))
    slo, shi = interval(dO2, R, rho)

    def side(s):
        s0 = (float(sM) - wv) if s == 0 else (-float(sM) - wv)
        return s0, f32(f32(f32(wz + s0 * V[2]) * iL) * R)
    low2 = not (side(1)[1] - ch > 0)
    touch = not (cosw > f32(0.05) and sM * iL > sinw * f32(1.0001) + f32(8e-3))
    if low2 and touch:
        return BW.line_slots(P, V, cfg)                                 # the whole line as a grazing line
    ir = f32(1) / rho
    slots = []
    for s in ((0, 1) if low2 else (0,)):
        s0, Gz = side(s)
        if Gz - ch > 0:
            continue
        fx, fy = f32(f32(P[0] + s0 * V[0]) * iL), f32(f32(P[1] + s0 * V[1]) * iL)
        a = f32(-f32(wz + s0 * V[2]) * iL)
        jlo, ncol = BW.col_range(fx, fy, cosw, inv_dphi, n_phi, False)
        js = (jlo + np.arange(ncol)) % n_phi
        ilo, cnt = BW.cap_rows(fx, fy, a, cosw, c32[js], s32[js], inv_dth, n_theta)
        if variant:
            sg = 1.0 if s == 0 else -1.0
            sa, sb = sg * float(slo) - wv, sg * float(shi) - wv
            xa, ya = f32(f32(P[0] + sa * V[0]) * ir), f32(f32(P[1] + sa * V[1]) * ir)
            xb, yb = f32(f32(P[0] + sb * V[0]) * ir), f32(f32(P[1] + sb * V[1]) * ir)
            cs = f32(f32(slack) * ABS * f32(f32(abs(xa) + abs(ya)) + f32(abs(xb) + abs(yb))))
            cnt = col_cull(xa, ya, xb, yb, cs, c32[js], s32[js], inv_dth, ilo, cnt, variant, slack)
        slots += [(int(j), int(i), int(n)) for j, i, n in zip(js, ilo, cnt) if n > 0]
    return "caps", slots


def reference_hits(c, P, V, tab=None):
    """bool[n_theta, n_phi]: the oracle's own isxo_check_intersection of ONE line on every bin (tab given: the numpy formula)"""
    if tab is not None:
        return exact_hits(P, V, tab, c.det_diameter).reshape(c.n_theta, c.n_phi)
    return orc.bin_lines(c, P[None, :], V[None, :], nthreads=1) > 0


def check(c, lp, d, variant=2, slack=1.0, tab=None):
    """-> dict(lines, hits, candidates, slots, missed, twice): the slots of every line against the reference formula"""
    out = dict(lines=0, hits=0, candidates=0, slots=0, missed=0, twice=0, caps=0)
    for P, V in zip(lp, d):
        h = reference_hits(c, P, V, tab)
        kind, slots = line_slots(P, V, c, variant, slack)
        cov = np.zeros((c.n_theta, c.n_phi), int)
        for j, i, n in slots:
            cov[i:i + n, j] += 1
        out["missed"] += int((h & (cov == 0)).sum()); out["twice"] += int((cov > 1).sum())
        out["candidates"] += int(cov.sum()); out["hits"] += int(h.sum()); out["lines"] += 1; out["slots"] += len(slots)
        out["caps"] += kind == "caps"
    return out


def edge_family(cfg, seed=1212, per_bin=6, extra=10):
    """Lines at the cull's own edge.  For chosen bins (i, j) the disc point X = c +- rho_d u2 (alpha = 0, |beta| = rho_d: the point
    of the disc farthest from the meridian plane, at rho_d cos(theta_i) exactly) and lines through it along directions IN the plane
    perpendicular to phi^_j -- phi^_j . (x - O) is then the same all along the line, dmin_j = rho_d cos(theta_i) -- shifted along
    phi^_j by +-1e-9 cm and by +-4 ulp of the coordinates' size (inwards: a hit of bin (i, j) in the reference; outwards: not one).
    -> (P, V, bin, shift sign: -1 inwards, +1 outwards)"""
    rng = np.random.default_rng(seed)
    nt, nph, R, pz = cfg.n_theta, cfg.n_phi, cfg.det_distance, cfg.exit_port_z
    rho = cfg.det_diameter / 2
    rows = sorted({0, nt // 4, nt // 2, (3 * nt) // 4, nt - 1} | set(int(x) for x in rng.integers(nt, size=extra)))
    P, V, B, S = [], [], [], []
    for i in rows:
        for j in sorted({0, nph - 1, int(rng.integers(nph))}):
            th = np.deg2rad((i + 0.5) * 90.0 / nt); ph = np.deg2rad((j + 0.5) * 360.0 / nph)
            Sn, Cs, cp, sp = np.sin(th), np.cos(th), np.cos(ph), np.sin(ph)
            c = np.array([R * Sn * cp, R * Sn * sp, pz - R * Cs])
            rh, ph_hat, zh = np.array([cp, sp, 0.0]), np.array([-sp, cp, 0.0]), np.array([0.0, 0.0, 1.0])
            u2 = Cs * ph_hat + Sn * zh
            for sgn in (1.0, -1.0):
                X = c + sgn * rho * u2
                out = sgn * ph_hat                                   # away from the meridian plane
                for _ in range(per_bin):
                    a = rng.uniform(np.pi / 6, 5 * np.pi / 6) * rng.choice([-1.0, 1.0])
                    v = np.cos(a) * rh + np.sin(a) * zh              # perpendicular to phi^_j: n . v = -sin(a) cos(theta_i)
                    if abs(np.sin(a) * Cs) < 1e-3:                   # (the reference's own rounding, ~1e-16 |P| / |n . v|, stays small)
                        continue
                    for sh in (1e-9, 4 * np.spacing(abs(X).max())):
                        for io in (-1.0, 1.0):
                            p = X + io * sh * out
                            P.append(p - rng.uniform(50, 150) * R / 100.0 * v); V.append(v); B.append(i * nph + j); S.append(io)
    return np.array(P), np.array(V), np.array(B), np.array(S)


def scaled(cfg, f):
    """the configuration with every length multiplied by f"""
    c = cfg.copy()
    for name in ("det_distance", "det_diameter", "exit_port_z", "box_half"):
        setattr(c, name, getattr(cfg, name) * f)
    return c


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
    c = orc.default_config()
    st, _, lp, d = orc.trace_endstates(c, n, 0x5EED0001)
    keep = (st == 1) & (lp[:, 2] < c.exit_port_z)
    for variant in (0, 1, 2):
        r = check(c, lp[keep], d[keep], variant)
        print(f"variant {variant}: lines {r['lines']}, candidates/hit {r['candidates'] / r['hits']:.3f}, slots/line "
              f"{r['slots'] / r['lines']:.2f}, missed {r['missed']}, twice {r['twice']}")


if __name__ == "__main__":
    main()
