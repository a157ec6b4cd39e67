"""Deterministic exit segments at the edges of the disc sweep's binning kernel -- TEST INFRASTRUCTURE (pure numpy, fixed seeds).

isx_bin_discs_kernel decides a hit in two steps: a binary32 pre-selection of the segment's line against the ball of a cluster of
eight discs, then the exact binary64 test behind a bounding-ball cull of its own.  Traced rays never graze a rim to 1e-9 cm, never
end at a tube, never sit on the ties of the exact test.  The families below do.  A segment is seg[7] = start, unit direction,
tmax; every start lies within sqrt(3) * 300 cm of the origin BY CONSTRUCTION (discs within 205 cm, along-line distances of at
most 300 cm: 505 < 519.6) and 0 <= tmax <= 350 -- the domain of isx_bin_injected_segments for the default box_half of 300.

  rim          through a point X shifted by delta from a disc's rim circle along the disc's bounding-ball normal, in a direction of
               the ball's tangent plane there: delta > 0 puts X inside the tube (a hit), delta < 0 keeps the whole line outside
               the ball (a miss)
  cluster_rim  through the rim point farthest from the cluster's rounded centre (shifted inward), perpendicular to the direction
               from that centre: hits at the largest line-to-centre distance a hit of the cluster can have
  short        segments that end 1e-6 cm before the tube (miss) or 1e-6 cm inside it (hit); start points inside a tube with tmax
               0 and 1e-300 (hits)
  ties         hand-made, exactly representable: |ws| == h with vs == 0, A <= 0 at radial distance r, D == 0, t0 == t1, tmax == 0,
               -0.0 -- no truth claimed, the GPU has to equal the oracle
  column       40 coaxial discs 1 cm apart and segments straight down their axis: every segment passes all five clusters, 320
               pairs per 64-segment batch, so the kernel's pair list is flushed inside its cluster loop
"""
import math

import numpy as np

import disccull_np as DC

R_REF, H_REF = 5.0, 0.1                       # integratingSphereDetectorSweep.C's disc
RIM_DELTA = (1e-9, -1e-9, 1e-7, -1e-7, 1e-5, -1e-5, 1e-3)
CLUSTER_RIM_DELTA = (1e-9, 1e-6)
PER_DISC = 40                                 # rim points (rim), lines (cluster_rim) per disc and offset
FAMILIES = ("rim", "cluster_rim", "short")    # the families that are built for any disc list
LISTS = ("placement", "fine", "one", "seven", "eight", "nine", "coincident", "n1024", "n1025", "cap4096", "thin")


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1)[..., None]


def _plane_basis(n):
    """two unit vectors spanning the plane with unit normal n[..., 3]"""
    flat = n.reshape(-1, 3)
    t = np.zeros_like(flat)
    t[np.arange(len(flat)), np.argmin(np.abs(flat), axis=1)] = 1.0
    e1 = _unit(t - np.einsum("ij,ij->i", t, flat)[:, None] * flat)
    e2 = np.cross(flat, e1)
    return e1.reshape(n.shape), e2.reshape(n.shape)


def disc_positions(dtheta=0.5, theta_max=45.0):
    """the placement of tests/test_gpu_round2.py::_disc_positions (rootMacros::detectorDiskPlacement), restated so that this module
    stands alone (tests/test_injected_segments_cpu.py holds the two together)"""
    out = []
    for th in np.arange(-theta_max, theta_max + 1e-9, dtheta):
        for ph in (0.0, 180.0):
            t, p = math.radians(th), math.radians(ph)
            x, y, z = 200 * math.sin(t) * math.cos(p), 200 * math.sin(t) * math.sin(p), -200 * math.cos(t)
            dx, dy, dz = 0 - x, 0 - y, -100 - z
            rot = -math.atan2(math.sqrt(dx * dx + dy * dy), dz)
            out.append([x, y, z, math.sin(rot), 0.0, math.cos(rot)])
    return np.array(out)


def cap_discs(n, seed):
    """n discs at 200 cm, random over the cap theta <= 0.8 rad, facing the origin (tests/test_gpu_round4.py's recipe)"""
    rng = np.random.default_rng(seed)
    th = rng.uniform(0.0, 0.8, n); ph = rng.uniform(0.0, 2 * np.pi, n)
    axes = _unit(np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)], axis=1))
    return np.concatenate([200.0 * axes, axes], axis=1).astype(np.float64)


def coincident_discs(n=16):
    """n discs at one point with different axes: every Morton span is 0"""
    k = np.arange(n)
    th, ph = 0.05 * k, 2.4 * k
    axes = _unit(np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1))
    return np.concatenate([np.tile([0.0, 0.0, -200.0], (n, 1)), axes], axis=1)


_LISTS = {}


def disc_list(name):
    """-> (ca[n, 6], radius, half_thick), read-only.  n1024 is the first 1024 discs of n1025 (the kernel keeps up to 1024 discs in
    LDS: one list on either side of that threshold, sharing a prefix)."""
    if name not in _LISTS:
        r, h = R_REF, H_REF
        if name == "placement":
            ca = disc_positions()
        elif name == "fine":
            ca = disc_positions(dtheta=0.05, theta_max=4.5)      # the same placement in steps of 1.75 mm: most clusters hold
        elif name == "one":                                      # a disc whose farthest rim point lies ON the cluster's ball
            ca = disc_positions()[180:181]                       # theta = 0
        elif name in ("seven", "eight", "nine"):
            ca = disc_positions(dtheta=5.0)[:{"seven": 7, "eight": 8, "nine": 9}[name]]
        elif name == "coincident":
            ca = coincident_discs()
        elif name in ("n1024", "n1025"):
            ca = cap_discs(1025, 1025)[:int(name[1:])]
        elif name == "cap4096":
            ca = cap_discs(4096, 7)
        elif name == "thin":
            ca, r, h = disc_positions(dtheta=5.0), 0.5, 0.01
        else:
            raise KeyError(name)
        ca = np.ascontiguousarray(ca, dtype=np.float64)
        ca.setflags(write=False)
        _LISTS[name] = (ca, r, h)
    return _LISTS[name]


def targets(ca, seed=5):
    """the discs the families aim at: all of a short list; of a long one 256 -- the first, the last, the last cluster, the rest
    drawn -- so that the largest case stays near 1e5 segments"""
    n = len(ca)
    if n <= 400:
        return np.arange(n)
    perm, _, _ = DC.cluster_table(ca)
    keep = {0, n - 1} | set(perm[8 * ((n - 1) // 8):].tolist())
    rest = np.random.default_rng(seed).permutation(n)
    for k in rest:
        if len(keep) >= 256:
            break
        keep.add(int(k))
    return np.array(sorted(keep))


def _through(X, u, rng, past=50.0):
    """segments through the points X[m, 3] along u[m, 3]: the start 50 to 300 cm before X, tmax 50 cm past it"""
    L = rng.uniform(50.0, 300.0, len(X))
    return np.concatenate([X - L[:, None] * u, u, (L + past)[:, None]], axis=1)


def _rim_points(ca, r, h, tgt, phi, sign, delta):
    """X = Q - delta n for Q = c + r e(phi) + sign h a on the rim circles of discs tgt, n the bounding-ball normal at Q"""
    c, a = ca[tgt, :3], ca[tgt, 3:]
    e1, e2 = _plane_basis(a)
    q = r * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2) + (sign * h)[:, None] * a      # Q - c, |.| = ball
    n = _unit(q)
    return c + q - delta[:, None] * n, n


def rim(ca, r, h, seed=101):
    """-> (seg[m, 7], tgt[m], delta[m]); truth of (seg[k], disc tgt[k]): hit iff delta[k] > 0"""
    rng = np.random.default_rng(seed)
    t = targets(ca)
    m = len(t) * PER_DISC
    tgt = np.repeat(t, PER_DISC)
    phi, sign = rng.uniform(0.0, 2 * np.pi, m), np.where(rng.integers(0, 2, m) == 1, 1.0, -1.0)
    nd = len(RIM_DELTA)
    tgt, phi, sign = np.repeat(tgt, nd), np.repeat(phi, nd), np.repeat(sign, nd)
    delta = np.tile(np.array(RIM_DELTA), m)
    X, n = _rim_points(ca, r, h, tgt, phi, sign, delta)
    e1, e2 = _plane_basis(n)
    al = rng.uniform(0.0, 2 * np.pi, len(X))
    u = _unit(np.cos(al)[:, None] * e1 + np.sin(al)[:, None] * e2)
    return _through(X, u, rng), tgt, delta


def cluster_rim(ca, r, h, seed=202):
    """-> (seg[m, 7], tgt[m], delta[m]); every (seg[k], disc tgt[k]) is a hit: X lies inside the tube, on the segment"""
    rng = np.random.default_rng(seed)
    t = targets(ca)
    _, cluster_of, centres = DC.cluster_table(ca)
    c, a = ca[t, :3], ca[t, 3:]
    d = c - centres[cluster_of[t]].astype(np.float64)                  # from the rounded centre the kernel uses
    dp = d - np.einsum("ij,ij->i", d, a)[:, None] * a                  # its part in the disc's plane
    e1, _ = _plane_basis(a)
    small = np.linalg.norm(dp, axis=1) < 1e-9
    e = _unit(np.where(small[:, None], e1, dp))
    sign = np.where(np.einsum("ij,ij->i", d, a) < 0, -1.0, 1.0)
    q = r * e + (sign * h)[:, None] * a                                # the farthest rim point, from the disc's centre
    nd = len(CLUSTER_RIM_DELTA)
    reps = PER_DISC * nd
    tgt = np.repeat(t, reps)
    delta = np.tile(np.repeat(np.array(CLUSTER_RIM_DELTA), PER_DISC), len(t))
    qq, cc, dd = np.repeat(q, reps, axis=0), np.repeat(c, reps, axis=0), np.repeat(d, reps, axis=0)
    X = cc + qq - delta[:, None] * _unit(qq)
    g = _unit(dd + (X - cc))                                           # from the cluster's centre to X
    e1, e2 = _plane_basis(g)
    al = rng.uniform(0.0, 2 * np.pi, len(X))
    u = _unit(np.cos(al)[:, None] * e1 + np.sin(al)[:, None] * e2)
    return _through(X, u, rng), tgt, delta


def short(ca, r, h, seed=303, per_disc=8):
    """-> (seg[m, 7], tgt[m], truth[m]): the hit of (seg[k], disc tgt[k]).  Rim lines at delta = 1e-3 and lines through the
    centre, cut 1e-6 cm before the tube (miss) and 1e-6 cm inside it (hit: X lies at least 2e-5 cm deep, so the chord is longer);
    starts inside the tube with tmax 0 and 1e-300 (hits)."""
    rng = np.random.default_rng(seed)
    t = targets(ca)
    tgt = np.repeat(t, per_disc)
    m = len(tgt)
    phi, sign = rng.uniform(0.0, 2 * np.pi, m), np.where(rng.integers(0, 2, m) == 1, 1.0, -1.0)
    X, n = _rim_points(ca, r, h, tgt, phi, sign, np.full(m, 1e-3))
    e1, e2 = _plane_basis(n)
    al = rng.uniform(0.0, 2 * np.pi, m)
    u_rim = _unit(np.cos(al)[:, None] * e1 + np.sin(al)[:, None] * e2)
    u_ctr = _unit(rng.standard_normal((m, 3)))
    long_ = np.concatenate([_through(X, u_rim, rng), _through(ca[tgt, :3], u_ctr, rng)])
    tg2 = np.concatenate([tgt, tgt])
    t_in, _, hit = DC.tube_interval(long_, ca[tg2], r, h)
    assert hit.all() and (t_in >= 50.0 - 2.0 * math.hypot(r, h) - 1e-6).all(), "the uncut segments enter the tube a chord before X at the most"
    before, inside = long_.copy(), long_.copy()
    before[:, 6] = t_in - 1e-6
    inside[:, 6] = t_in + 1e-6
    # starts inside the tube
    k = np.repeat(t, 2)
    e1, e2 = _plane_basis(ca[k, 3:])
    rho, ang, ax = rng.uniform(0.0, 0.5 * r, len(k)), rng.uniform(0.0, 2 * np.pi, len(k)), rng.uniform(-0.5 * h, 0.5 * h, len(k))
    P = ca[k, :3] + rho[:, None] * (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2) + ax[:, None] * ca[k, 3:]
    u = _unit(rng.standard_normal((len(k), 3)))
    zero = np.concatenate([P, u, np.zeros((len(k), 1))], axis=1)
    tiny = np.concatenate([P, u, np.full((len(k), 1), 1e-300)], axis=1)
    seg = np.concatenate([before, inside, zero, tiny])
    tgt_all = np.concatenate([tg2, tg2, k, k])
    truth = np.concatenate([np.zeros(len(before), bool), np.ones(len(inside) + 2 * len(k), bool)])
    return seg, tgt_all, truth


_FAM = {}


def family(list_name, name):
    """-> (seg, tgt, truth) of a family of FAMILIES on a list of LISTS, built once, read-only"""
    key = (list_name, name)
    if key not in _FAM:
        ca, r, h = disc_list(list_name)
        if name == "rim":
            seg, tgt, delta = rim(ca, r, h)
            truth = delta > 0
        elif name == "cluster_rim":
            seg, tgt, delta = cluster_rim(ca, r, h)
            truth = np.ones(len(seg), bool)
        else:
            seg, tgt, truth = short(ca, r, h)
        seg = np.ascontiguousarray(seg)
        for x in (seg, tgt, truth):
            x.setflags(write=False)
        _FAM[key] = (seg, tgt, truth)
    return _FAM[key]


# ------------------------------------------------------------------ ties

TIE_DISC = (np.array([[0.0, 0.0, -200.0, 0.0, 0.0, 1.0]]), 5.0, 0.125)


def ties():
    """-> (ca[1, 6], r, h, seg[m, 7]): the disc with axis (0, 0, 1), r = 5, h = 0.125 about (0, 0, -200), and segments whose
    every number is exactly representable (w = start - centre is exact too)"""
    up, dn = lambda x: float(np.nextafter(x, np.inf)), lambda x: float(np.nextafter(x, -np.inf))
    cz, r, h = -200.0, 5.0, 0.125
    s = []
    # vs == 0: direction exactly perpendicular to the axis, |ws| == h and one ulp (of the coordinate) either side, on both faces
    for z in (cz + h, up(cz + h), dn(cz + h), cz - h, up(cz - h), dn(cz - h)):
        for y in (0.0, 3.0, 5.0, up(5.0)):
            s.append([-10.0, y, z, 1.0, 0.0, 0.0, 20.0])
            s.append([y, 10.0, z, 0.0, -1.0, 0.0, 20.0])
    # A <= 0: direction exactly along the axis, at radial distance exactly r and one ulp either side
    for x, y in ((5.0, 0.0), (up(5.0), 0.0), (dn(5.0), 0.0), (3.0, 4.0), (-4.0, 3.0), (up(3.0), 4.0), (dn(3.0), 4.0), (0.0, -5.0)):
        s.append([x, y, cz - 10.0, 0.0, 0.0, 1.0, 20.0])
        s.append([x, y, cz + 10.0, 0.0, 0.0, -1.0, 20.0])
    # D == 0: w = (-10, 5, 0), V = (1, 0, 0) touches the cylinder at t = 10 -- with tmax exactly there, an ulp short, an ulp past
    for tmax in (10.0, dn(10.0), up(10.0), 20.0):
        s.append([-10.0, 5.0, cz, 1.0, 0.0, 0.0, tmax])
        s.append([-10.0, -5.0, cz + 0.0625, 1.0, 0.0, 0.0, tmax])
        s.append([5.0, 10.0, cz, 0.0, -1.0, 0.0, tmax])
    # the slab's interval and the cylinder's meet in one point: through the tube's corner circle from outside, in the x-z plane
    for vx, vz in ((0.6, 0.8), (0.8, 0.6), (0.6, -0.8), (0.28, 0.96)):
        for corner_z in (h, -h):
            k = 8.0
            s.append([-5.0 - k * vx, 0.0, cz + corner_z - k * vz, vx, 0.0, vz, 30.0])
            s.append([5.0 + k * vx, 0.0, cz + corner_z - k * vz, -vx, 0.0, vz, 30.0])
    # t0 == t1: the start on the surface looking away, and looking in; tmax == 0 on the surface, inside and outside
    for p in ((5.0, 0.0, cz), (0.0, 5.0, cz + h), (3.0, 4.0, cz - h), (0.0, 0.0, cz + h), (0.0, 0.0, cz)):
        for v in ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0)):
            for tmax in (0.0, 1e-300, 1.0):
                s.append([*p, *v, tmax])
    for p in ((up(5.0), 0.0, cz), (dn(5.0), 0.0, cz), (0.0, 0.0, up(cz + h)), (0.0, 0.0, dn(cz + h))):
        s.append([*p, 0.0, 1.0, 0.0, 0.0])
    # -0.0 components, tmax -0.0 included (the domain's 0 <= tmax holds for it)
    s.append([-10.0, -0.0, cz, 1.0, -0.0, -0.0, 20.0])
    s.append([-0.0, -0.0, cz - 10.0, -0.0, -0.0, 1.0, 20.0])
    s.append([-0.0, 0.0, cz, -0.0, 1.0, -0.0, -0.0])
    s.append([5.0, -0.0, cz + h, -0.0, -0.0, -1.0, -0.0])
    ca, r, h = TIE_DISC
    return ca.copy(), r, h, np.array(s, dtype=np.float64)


def ties_among(n=9):
    """the same segments on a list that holds the tie disc as its last: n - 1 discs of the placement in front of it"""
    ca, r, h, seg = ties()
    return np.concatenate([disc_positions(dtheta=5.0)[:n - 1], ca]), r, h, seg


# ------------------------------------------------------------------ column

COLUMN_DISCS = 40


def column(seed=404):
    """-> (ca[40, 6], r, h, seg[m, 7], region_counts): 40 coaxial discs 1 cm apart (five clusters along z) and segments straight
    down their axis from 100 cm above, within 3 cm of it: every segment hits every disc.  The layout holds full 64-segment batches
    and regions whose last batch has 2 to 63 segments."""
    rng = np.random.default_rng(seed)
    ca = np.array([[0.0, 0.0, -160.0 - k, 0.0, 0.0, 1.0] for k in range(COLUMN_DISCS)])
    counts = [64, 1024, 128 + 2, 64 + 63, 3 * 64 + 17, 64 + 33, 2, 63, 256 + 40]
    m = int(np.sum(counts))
    rho, ang = rng.uniform(0.0, 3.0, m), rng.uniform(0.0, 2 * np.pi, m)
    P = np.stack([rho * np.cos(ang), rho * np.sin(ang), np.full(m, -60.0)], axis=1)
    seg = np.concatenate([P, np.tile([0.0, 0.0, -1.0], (m, 1)), np.full((m, 1), 200.0)], axis=1)
    return ca, R_REF, H_REF, seg, counts
