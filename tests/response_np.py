"""The scene response of include/isx.h (isx_scene_response) restated on a walk's per-ray arrays -- TEST INFRASTRUCTURE.

Two independent pieces: the bin of a ray from a vectorised numpy Philox4x32-10 (held against the oracle's isxo_philox4x32_10 by
tests/test_scene_response_cpu.py) and the integer rule of the contract; the fate slot from what isxo_scene_walk reports per ray --
status, last point, last class, last baffle.  The walk does not say on what a ray was absorbed: a baffle lies strictly inside the
cavity, so an absorbed ray whose last point lies inside the inner sphere ended on the baffle it touched last, and one on the wall
on the class of its last mirror interaction.  from_walk() asserts that the distinction is clear -- no absorbed ray that touched a baffle
ends in the last 1e-6 inside r_in unless it lies on the sphere itself (to 1e-9; a wall point is there to rounding) -- and that the
rows it makes are the walk's own patch_absorbed / baffle_absorbed, which no misjudged ray would leave standing.
"""
import numpy as np

FATES, BAFFLE0, PORT, EXITED_OTHER, SUSPENDED = 21, 10, 18, 19, 20
EXITED, ABSORBED, SUSPENDED_STATUS = 1, 2, 3
_M = np.uint64(0xFFFFFFFF)
_S = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counters (c0..c3) under one key (k0, k1) -> four uint64 arrays of 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & _M for x in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> _S) ^ c1 ^ k0, p1 & _M, (p0 >> _S) ^ c3 ^ k1, p0 & _M
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M, (k1 + np.uint64(0xBB67AE85)) & _M
    return c0, c1, c2, c3


def start_words(seed, first, count):
    """w[0..3] of the beam contract for rays first .. first + count - 1: block 0 of stream 3"""
    ids = np.uint64(int(first)) + np.arange(int(count), dtype=np.uint64)
    return philox4x32_10(ids & _M, ids >> _S, 0, 3, int(seed) & 0xFFFFFFFF, int(seed) >> 32)


def axes(rspec):
    return [int(v) for v in rspec.n]


def bins(rspec, seed, first, count):
    """the bin of every ray: i_a = (w[a] * n[a]) >> 32, b = ((i_0 n_1 + i_1) n_2 + i_2) n_3 + i_3"""
    n = axes(rspec)
    i = [(w * np.uint64(n[a])) >> _S for a, w in enumerate(start_words(seed, first, count))]
    return (((i[0] * np.uint64(n[1]) + i[1]) * np.uint64(n[2]) + i[2]) * np.uint64(n[3]) + i[3]).astype(np.int64)


def fates(w, cfg):
    """the fate slot of every ray of a walk"""
    st, lp, lb, lc = w["status"], w["last_point"], w["last_baffle"], w["last_class"]
    r = np.sqrt((lp * lp).sum(axis=1))
    touched = (st == ABSORBED) & (lb >= 0)
    # (a wall point lies on the inner sphere to rounding, ~1e-14, or beyond it; a baffle point clearly inside: nothing in between)
    unclear = touched & (r >= cfg.r_in - 1e-6) & (r < cfg.r_in - 1e-9)
    assert not unclear.any(), "an absorbed ray that touched a baffle ends within 1e-6 inside r_in, and not on the sphere"
    on_baffle = touched & (r < cfg.r_in - 1e-6)
    f = np.where(st == SUSPENDED_STATUS, SUSPENDED,
                 np.where(st == EXITED, np.where(lp[:, 2] < cfg.exit_port_z, PORT, EXITED_OTHER),
                          np.where(on_baffle, BAFFLE0 + lb, lc))).astype(np.int64)
    assert ((st >= EXITED) & (st <= SUSPENDED_STATUS)).all() and (f >= 0).all() and (f < FATES).all()
    return f


def from_walk(w, cfg, rspec, seed, first):
    """response[21, B] of the rays of oracle.scene_walk(cfg, scene, n, seed, first)"""
    n = w["status"].size
    n_ax = axes(rspec)
    B = n_ax[0] * n_ax[1] * n_ax[2] * n_ax[3]
    f, b = fates(w, cfg), bins(rspec, seed, first, n)
    assert n == 0 or (0 <= int(b.min()) and int(b.max()) < B)
    resp = np.bincount(f * B + b, minlength=FATES * B).astype(np.uint64).reshape(FATES, B)
    rows = resp.sum(axis=1)
    P = w["patch_absorbed"].size - 2
    assert np.array_equal(rows[:P + 2], w["patch_absorbed"]) and not rows[P + 2:BAFFLE0].any(), "rows 0..9 are patch_absorbed"
    ba = np.zeros(8, dtype=np.uint64)
    ba[:w["baffle_absorbed"].size] = w["baffle_absorbed"].reshape(-1)
    assert np.array_equal(rows[BAFFLE0:PORT], ba), "rows 10..17 are baffle_absorbed"
    c = w["census"]
    assert rows[PORT] == c["counted_below_z"] and rows[PORT] + rows[EXITED_OTHER] == c["exited"] and rows[SUSPENDED] == c["suspended"]
    assert int(resp.sum()) == c["launched"] == n
    return resp
