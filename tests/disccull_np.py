"""numpy restatements of what the disc sweep's binning kernel does around its exact test -- TEST INFRASTRUCTURE.

  cluster_table     upload_discs_clustered (isx_api.hip): Morton order, eight discs to a cluster, the ball about the ROUNDED centre
  preselect         step 1 of isx_bin_discs_kernel: the segment's line against a cluster's ball in binary32, with its two margins
  ball_cull         the binary64 cull at the head of the kernel's segment_hits_tube
  tube_interval     the exact test, segment_hits_tube of the oracle, as the interval [t0, t1] it ends with
  hit_pairs         every (segment, disc) pair that tube_interval calls a hit

The binary32 fused multiply-adds are taken in binary64 and rounded once more (a product of two binary32 numbers is exact in
binary64; the sum is rounded twice, which differs from fmaf in the last bit of rare cases); the binary64 ones are written
unfused.  Both differ from the kernel by an ulp of the quantity compared, against margins of 1e-6 relative and more: these
restatements say whether a MARGIN covers a hit, they are not the reference of any parity test (that is isxo_bin_segments).
"""
import numpy as np

F32_MARGINS = (1.002, 4e-6)      # isx_bin_discs_kernel: on the radius^2, and on the two cancelling terms
F64_MARGINS = (1.000001, 1e-9)   # segment_hits_tube (kernel): relative, absolute
PAIR_FLUSH = 256 - 64            # kPairCap - 64: a pair list longer than this is flushed inside the kernel's cluster loop


def cluster_table(ca):
    """-> (perm[n], cluster_of[n], clusters[ncl, 3] float32).  perm[j]: the caller's index of the j-th disc in cluster order;
    cluster_of[k]: the cluster of the caller's disc k; clusters[c]: the rounded centre (the radius: cluster_radius)."""
    ca = np.asarray(ca, dtype=np.float64).reshape(-1, 6)
    n = len(ca)
    lo, hi = ca[:, :3].min(axis=0), ca[:, :3].max(axis=0)
    code = np.zeros(n, dtype=np.uint64)
    for a in range(3):
        span = hi[a] - lo[a]
        if span > 0:
            q = np.minimum(1023.0, np.floor((ca[:, a] - lo[a]) / span * 1024.0)).astype(np.uint64)
        else:
            q = np.zeros(n, dtype=np.uint64)
        for bit in range(10):
            code |= ((q >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + a)
    perm = np.lexsort((np.arange(n), code))                 # (code, index) pairs in order: the kernel's stable sort
    ncl = (n + 7) // 8
    centres = np.zeros((ncl, 3), dtype=np.float32)
    cluster_of = np.zeros(n, dtype=np.int64)
    for c in range(ncl):
        idx = perm[8 * c:8 * c + 8]
        ctr = np.zeros(3)
        for j in idx:                                       # (a sum of quotients, in cluster order, as the host writes it)
            ctr += ca[j, :3] / float(len(idx))
        centres[c] = ctr.astype(np.float32)
        cluster_of[idx] = c
    return perm, cluster_of, centres


def cluster_radius(ca, radius, half_thick, perm, centres):
    """the table's fourth float: nextafter(float32((max |c - rounded centre| + ball) (1 + 1e-6)), inf)"""
    ca = np.asarray(ca, dtype=np.float64).reshape(-1, 6)
    ball = np.sqrt(radius * radius + half_thick * half_thick)
    out = np.zeros(len(centres), dtype=np.float32)
    for c in range(len(centres)):
        d = ca[perm[8 * c:8 * c + 8], :3] - centres[c].astype(np.float64)
        r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).max()
        out[c] = np.nextafter(np.float32((r + ball) * (1.0 + 1e-6)), np.float32(np.inf))
    return out


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def preselect(seg, centres, cw, margins=F32_MARGINS):
    """near[k]: the kernel's `!(lhs > rhs)` of segment seg[k] against the cluster (centres[k], cw[k]) -- pairs, not a matrix"""
    f32 = np.float32
    p, v = seg[:, :3].astype(f32), seg[:, 3:6].astype(f32)
    c, cw = np.asarray(centres, dtype=f32), np.asarray(cw, dtype=f32)
    m1, m2 = f32(margins[0]), f32(margins[1])
    vv = _fma32(v[:, 0], v[:, 0], _fma32(v[:, 1], v[:, 1], v[:, 2] * v[:, 2]))
    w = p - c
    wv = _fma32(w[:, 0], v[:, 0], _fma32(w[:, 1], v[:, 1], w[:, 2] * v[:, 2]))
    ww = _fma32(w[:, 0], w[:, 0], _fma32(w[:, 1], w[:, 1], w[:, 2] * w[:, 2]))
    lhs = _fma32(ww, vv, -(wv * wv))
    rhs = _fma32(cw * cw * m1, vv, m2 * _fma32(ww, vv, wv * wv))
    return ~(lhs > rhs)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + (a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2])


def ball_cull(seg, ca, radius, half_thick, margins=F64_MARGINS):
    """culled[k]: the kernel's binary64 cull of segment seg[k] against disc ca[k] -- pairs"""
    w, v = seg[:, :3] - ca[:, :3], seg[:, 3:6]
    wv, ww, vv = _dot(w, v), _dot(w, w), _dot(v, v)
    return ww * vv - wv * wv > (radius * radius + half_thick * half_thick) * vv * margins[0] + margins[1]


def tube_interval(seg, ca, radius, half_thick):
    """(t0, t1, hit) of segment seg[k] against disc ca[k] -- pairs: the oracle's segment_hits_tube, unfused.  t0 of a hit is
    where the segment enters the tube."""
    with np.errstate(all="ignore"):
        w, v, a, tmax = seg[:, :3] - ca[:, :3], seg[:, 3:6], ca[:, 3:], seg[:, 6]
        ws, vs = _dot(w, a), _dot(v, a)
        t0, t1 = np.zeros(len(seg)), tmax.copy()
        ta, tb = (-half_thick - ws) / vs, (half_thick - ws) / vs
        lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
        moving = vs != 0.0
        t0 = np.where(moving & (lo > t0), lo, t0)
        t1 = np.where(moving & (hi < t1), hi, t1)
        miss = (~moving & (np.abs(ws) > half_thick)) | (t0 > t1)
        A = _dot(v, v) - vs * vs
        B = _dot(w, v) - ws * vs
        Cq = _dot(w, w) - ws * ws - radius * radius
        D = B * B - A * Cq
        sD = np.sqrt(np.where(D < 0, 0.0, D))
        ra, rb = (-B - sD) / A, (-B + sD) / A
        axial = A <= 0.0
        r0 = np.where(~axial & (ra > t0), ra, t0)
        r1 = np.where(~axial & (rb < t1), rb, t1)
        hit = np.where(axial, Cq <= 0.0, (D >= 0.0) & (r0 <= r1)) & ~miss
    return r0, r1, hit


def hit_pairs(seg, ca, radius, half_thick, chunk=4096):
    """-> (i[m], j[m]): the pairs (segment i, disc j) that tube_interval calls a hit.  Candidates first: discs whose centre the
    segment's line passes within twice the bounding ball (no margin question: the tube lies inside the ball)."""
    seg = np.asarray(seg, dtype=np.float64).reshape(-1, 7)
    ca = np.asarray(ca, dtype=np.float64).reshape(-1, 6)
    reach2 = 4.0 * (radius * radius + half_thick * half_thick) + 1.0
    ii, jj = [], []
    c, cc = ca[:, :3], (ca[:, :3] * ca[:, :3]).sum(axis=1)
    for s0 in range(0, len(seg), chunk):
        s = seg[s0:s0 + chunk]
        p, v = s[:, :3], s[:, 3:6]
        # |w|^2 - (w.v)^2 for w = p - c, as matrix products (rounding ~1e-10 cm^2 against a reach of twice the ball)
        wv = (p * v).sum(axis=1)[:, None] - v @ c.T
        d2 = (p * p).sum(axis=1)[:, None] + cc[None, :] - 2.0 * (p @ c.T) - wv * wv
        i, j = np.nonzero(d2 <= reach2)
        _, _, hit = tube_interval(s[i], ca[j], radius, half_thick)
        ii.append(i[hit] + s0); jj.append(j[hit])
    if not ii:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(ii), np.concatenate(jj)


def check(seg, ca, radius, half_thick, f32_margins=F32_MARGINS, f64_margins=F64_MARGINS, pairs=None, count_pairs=True):
    """What the two culls do to the hits of `seg` on the list `ca`: {"hits", "dropped32", "dropped64", "pairs_per_batch"}.
    pairs_per_batch: the (segment, cluster) pairs step 1 keeps of each 64 consecutive segments (what the kernel's pair list sees
    when the segments lie in full regions)."""
    seg = np.asarray(seg, dtype=np.float64).reshape(-1, 7)
    ca = np.asarray(ca, dtype=np.float64).reshape(-1, 6)
    perm, cluster_of, centres = cluster_table(ca)
    cw = cluster_radius(ca, radius, half_thick, perm, centres)
    i, j = hit_pairs(seg, ca, radius, half_thick) if pairs is None else pairs
    k = cluster_of[j]
    near = preselect(seg[i], centres[k], cw[k], f32_margins)
    culled = ball_cull(seg[i], ca[j], radius, half_thick, f64_margins)
    out = {"hits": int(len(i)), "dropped32": int((~near).sum()), "dropped64": int(culled.sum())}
    per_batch = np.zeros((len(seg) + 63) // 64, dtype=np.int64)
    for c in range(len(centres) if count_pairs else 0):
        n = preselect(seg, np.broadcast_to(centres[c], (len(seg), 3)), np.broadcast_to(cw[c], (len(seg),)), f32_margins)
        np.add.at(per_batch, np.nonzero(n)[0] // 64, 1)
    out["pairs_per_batch"] = per_batch
    return out
