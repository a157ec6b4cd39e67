"""The scene of include/isx.h (isx_fluxmap_scene, isx_scene_endstates) replayed on the unchanged CPU oracle -- TEST INFRASTRUCTURE.

Nothing is stated here: replay() composes the three replays that exist.  A ray starts by beam_np.sample (the beam contract); every
segment p -> q of the oracle's own trace loop (oracle.next_boundary / philox / cosine_emission) is tested by baffle_np.segment (the
baffle contract), and a struck baffle takes the interaction exactly as baffle_np._replay_range runs it; a wall arrival is
classified by wallpatch_np.classify and interacts with the class's reflectance exactly as wallpatch_np._replay_range runs it.
Valid for the Lambertian border and explicit bounces -- the calls' scope.

A scene is a dict: "beam" a beam_np spec (None: the pencil of the configuration as the degenerate beam), "baffles" a baffle_np
spec, "patches" a wallpatch_np spec; spec_of() makes one from the library's SceneSpec.
"""
import ctypes as C
import os

import numpy as np

import baffle_np
import beam_np
import wallpatch_np

K_NONE, K_INNER, K_OUTER, K_CONE, K_BOX = 0, 1, 2, 3, 4
CENSUS_FIELDS = baffle_np.CENSUS_FIELDS
rho_thr = baffle_np.rho_thr


def spec_of(spec):
    """the dict of a SceneSpec"""
    return {"beam": beam_np.spec_of(spec.beam), "baffles": baffle_np.spec_of(spec.baffles),
            "patches": wallpatch_np.spec_of(spec.patches)}


def _replay_range(cfg_bytes, scene, lo, hi, seed, first):
    """rays [lo, hi) of a call (seed, first) -> dict of per-ray arrays, counters and the census"""
    import oracle
    c = oracle.Config()
    C.memmove(C.byref(c), cfg_bytes, C.sizeof(oracle.Config))
    assert c.lambertian == 1 and c.surface_model == 0 and c.source_model == 0 and c.trace_mode == 0, "replay(): Lambertian border, explicit bounces"
    f64 = np.float64
    baffles, patches = scene["baffles"], scene["patches"]
    nb, P = len(baffles), len(patches)
    n = hi - lo
    if scene["beam"] is None:   # the pencil, as the replays of the pencil's calls start it
        src = np.array([c.src[0], c.src[1], c.src[2]])
        d0 = np.array([c.dir[0], c.dir[1], c.dir[2]])
        d0 = d0 / np.linalg.norm(d0)
        sp, sv = np.tile(src, (n, 1)), np.tile(d0, (n, 1))
    else:
        sp, sv = beam_np.sample(scene["beam"], n, seed, first + lo)
    # per wall class: the configuration with the class's reflectance and its threshold (wallpatch_np._replay_range)
    cfgs, thrs = [], []
    for k in range(P + 2):
        ck = c.copy()
        if k < P:
            ck.reflectance = patches[k][2]
        cfgs.append(ck)
        thrs.append(rho_thr(ck.reflectance))
    # per baffle: the same, and rm = r_in * normal (baffle_np._replay_range)
    bcfg, bthr, brm = [], [], []
    for (_, m, _, rho) in baffles:
        ck = c.copy()
        ck.reflectance = rho
        bcfg.append(ck)
        bthr.append(rho_thr(rho))
        brm.append(tuple(f64(c.r_in) * f64(m[i]) for i in range(3)))
    p_arr, p_abs = np.zeros(P + 2, dtype=np.uint64), np.zeros(P + 2, dtype=np.uint64)
    b_arr, b_abs = np.zeros((max(nb, 1), 2), dtype=np.uint64), np.zeros((max(nb, 1), 2), dtype=np.uint64)
    census = dict.fromkeys(CENSUS_FIELDS, 0)
    status, n_points, last_baffle, last_class, first_class, first_kind = (np.zeros(n, dtype=np.int32) for _ in range(6))
    lps, dirs = np.zeros((n, 3)), np.zeros((n, 3))
    after_baffle = after_patch = 0   # rays the bounce limit stopped right after a baffle / right after a patch (class < P)
    zero = (0.0, 0.0, 0.0)
    for i in range(n):
        rid = first + lo + i
        p, v = sp[i].copy(), sv[i].copy()
        on, j, npoints, st, skip, lb, lc = K_NONE, 0, 1, 0, -1, -1, -1
        fc, fk = -1, -1   # the ray's first interaction: class of a wall arrival (-2: a baffle), and the kind of its first segment's end
        while True:
            kind, q, v = oracle.next_boundary(c, p, v, on, with_direction=True)
            k, side, x = baffle_np.segment(baffles, p, q, skip) if nb else (-1, 0, None)
            if npoints == 1:
                fk = -2 if k >= 0 else kind
            npoints += 1
            if k >= 0:
                p = x
                b_arr[k, side] += np.uint64(1)
                lb = 2 * k + side
                if j == 0:
                    fc = -2
                on, skip = K_NONE, k
                w = oracle.philox([rid & 0xffffffff, rid >> 32, j >> 1, 0], [seed & 0xffffffff, seed >> 32])
                wa, wb = w[2 * (j & 1)], w[2 * (j & 1) + 1]
                j += 1
                if not wb < bthr[k]:
                    b_abs[k, side] += np.uint64(1)
                    st = 2
                    break
                S = oracle.cosine_emission(bcfg[k], K_INNER, zero, wa, wb)
                rm = brm[k]
                if side == 0:
                    wv = (rm[0] + f64(S[0]), rm[1] + f64(S[1]), rm[2] + f64(S[2]))
                else:
                    wv = ((-rm[0]) + f64(S[0]), (-rm[1]) + f64(S[1]), (-rm[2]) + f64(S[2]))
                mag = np.sqrt((wv[0] * wv[0] + wv[1] * wv[1]) + wv[2] * wv[2])
                v = np.array([wv[0] / mag, wv[1] / mag, wv[2] / mag])
                if npoints > c.max_points:
                    st = 3
                    after_baffle += 1
                    break
                continue
            skip = -1
            p = q
            if kind == K_BOX:
                st = 1
                break
            on = kind
            cls = wallpatch_np.classify(patches, kind == K_INNER, p)
            p_arr[cls] += np.uint64(1)
            lc = cls
            if j == 0:
                fc = cls
            w = oracle.philox([rid & 0xffffffff, rid >> 32, j >> 1, 0], [seed & 0xffffffff, seed >> 32])
            wa, wb = w[2 * (j & 1)], w[2 * (j & 1) + 1]
            j += 1
            if not wb < thrs[cls]:
                p_abs[cls] += np.uint64(1)
                st = 2
                break
            v = oracle.cosine_emission(cfgs[cls], kind, p, wa, wb)
            if npoints > c.max_points:
                st = 3
                if cls < P:
                    after_patch += 1
                break
        status[i], n_points[i], lps[i], dirs[i], last_baffle[i], last_class[i] = st, npoints, p, v, lb, lc
        first_class[i], first_kind[i] = fc, fk
        census["launched"] += 1
        census["wall_hits"] += j
        if st == 1:
            census["exited"] += 1
            if p[2] < c.exit_port_z:
                census["counted_below_z"] += 1
        elif st == 2:
            census["absorbed"] += 1
        else:
            census["suspended"] += 1
    return {"start_point": sp, "start_dir": sv, "status": status, "n_points": n_points, "last_point": lps, "direction": dirs,
            "last_baffle": last_baffle, "last_class": last_class, "first_class": first_class, "first_kind": first_kind,
            "patch_arrivals": p_arr, "patch_absorbed": p_abs, "baffle_arrivals": b_arr, "baffle_absorbed": b_abs,
            "census": census, "suspended_after_baffle": after_baffle, "suspended_after_patch": after_patch}


PER_RAY = ("start_point", "start_dir", "status", "n_points", "last_point", "direction", "last_baffle", "last_class", "first_class",
           "first_kind")
COUNTERS = ("patch_arrivals", "patch_absorbed", "baffle_arrivals", "baffle_absorbed")


def replay(cfg, scene, n, seed, first=0, workers=None):
    """-> dict: per ray start_point, start_dir, status, n_points, last_point, direction, last_baffle (-1 or 2 k + side),
    last_class (-1 or the class of the last mirror interaction), first_class (the class of the ray's FIRST interaction if that
    was a wall's, -2 if a baffle's, -1 if it had none) and first_kind (the boundary its first segment ends on, -2: on a baffle);
    patch_arrivals[P + 2], patch_absorbed[P + 2], baffle_arrivals[K, 2], baffle_absorbed[K, 2] (K = max(len(baffles), 1)); the
    census dict; suspended_after_baffle / suspended_after_patch.  The rays are independent: they are walked by a few fresh
    processes (spawned, so that nothing of the caller's process is inherited)."""
    raw = bytes(C.string_at(C.addressof(cfg), C.sizeof(cfg)))
    scene = {"beam": None if scene.get("beam") is None else dict(scene["beam"]),
             "baffles": [(tuple(float(x) for x in c), tuple(float(x) for x in m), float(r), float(rho))
                         for c, m, r, rho in scene.get("baffles", ())],
             "patches": [(tuple(float(x) for x in a), float(md), float(rho)) for a, md, rho in scene.get("patches", ())]}
    if workers is None:
        workers = max(1, min(8, (os.cpu_count() or 1)))
    if workers == 1 or n < 2000:
        return _replay_range(raw, scene, 0, n, seed, first)
    import multiprocessing as mp
    step = (n + 4 * workers - 1) // (4 * workers)
    jobs = [(raw, scene, lo, min(lo + step, n), seed, first) for lo in range(0, n, step)]
    with mp.get_context("spawn").Pool(workers) as pool:
        parts = pool.starmap(_replay_range, jobs)
    out = {k: np.concatenate([p[k] for p in parts]) for k in PER_RAY}
    for k in COUNTERS:
        out[k] = sum(p[k] for p in parts)
    out["census"] = {k: sum(p["census"][k] for p in parts) for k in CENSUS_FIELDS}
    out["suspended_after_baffle"] = sum(p["suspended_after_baffle"] for p in parts)
    out["suspended_after_patch"] = sum(p["suspended_after_patch"] for p in parts)
    return out


def counted_lines(cfg, rep):
    """(P, V) of the replay's rays that left through the port: exited with the last point below exit_port_z"""
    sel = (rep["status"] == 1) & (rep["last_point"][:, 2] < cfg.exit_port_z)
    return rep["last_point"][sel], rep["direction"][sel]


def counter_words(rep, max_patches=8, max_baffles=4):
    """the 36 words of isx_scene_counts of a replay, in the struct's order"""
    P = rep["patch_arrivals"].size - 2
    pa, pb = np.zeros(max_patches + 2, dtype=np.uint64), np.zeros(max_patches + 2, dtype=np.uint64)
    pa[:P + 2], pb[:P + 2] = rep["patch_arrivals"], rep["patch_absorbed"]
    ba, bb = np.zeros((max_baffles, 2), dtype=np.uint64), np.zeros((max_baffles, 2), dtype=np.uint64)
    K = rep["baffle_arrivals"].shape[0]
    ba[:K], bb[:K] = rep["baffle_arrivals"], rep["baffle_absorbed"]
    return np.concatenate([pa, pb, ba.reshape(-1), bb.reshape(-1)])
