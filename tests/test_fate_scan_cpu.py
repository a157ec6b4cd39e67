"""The fate scan's rule (tests/fatescan_np.py) against the CPU oracle -- no GPU needed.

1. The vectorised Philox is the oracle's isxo_philox4x32_10.
2. Every ray the rule settles is ABSORBED in oracle.trace_endstates, with n_points = j + 2 -- over the default configuration and the
   configurations that move a threshold (port angle, reflectance, scale, bounce limit, a ray range that crosses 2^32).
3. A replay of explicit bounces on the oracle's own primitives (isxo_cosine_emission, isxo_next_boundary) lands within MARG / 100
   words of r_in sphere_z(wa): the margin the rule keeps from the port's edge has its 100x headroom."""
import numpy as np
import pytest

import fatescan_np as fs

SEED = 0x5EED0001
K_NONE, K_INNER = 0, 1


def _scaled(cfg, s):
    c = cfg.copy()
    c.r_in *= s; c.r_out *= s; c.box_half *= s
    c.det_diameter *= s; c.det_distance *= s; c.exit_port_z *= s
    for k in range(3):
        c.src[k] *= s
    return c


def _cases(orc):
    d = orc.default_config()

    def mod(**kw):
        c = d.copy()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    return {
        "default": (d, 1_000_000, 0),
        "port160": (mod(theta_max_deg=160.0), 200_000, 0),
        "rho0.9": (mod(reflectance=0.9), 200_000, 0),
        "rho0.5": (mod(reflectance=0.5), 200_000, 0),
        "scale0.01": (_scaled(d, 0.01), 200_000, 0),
        "scale100": (_scaled(d, 100.0), 200_000, 0),
        "max_points3": (mod(max_points=3), 200_000, 0),
        "max_points8": (mod(max_points=8), 200_000, 0),
        "first_wrap": (d, 200_000, 2 ** 32 - 1000),
    }


def test_vectorised_philox_is_the_oracles(orc):
    rng = np.random.default_rng(7)
    ctr = rng.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64)
    ctr[0] = 0
    ctr[1] = 0xFFFFFFFF
    for key in ((0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (SEED & 0xFFFFFFFF, SEED >> 32), (0xA4093822, 0x299F31D0)):
        got = np.stack(fs.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[0], key[1]), axis=1)
        for row, c in zip(got, ctr):
            assert [int(x) for x in row] == orc.philox([int(x) for x in c], list(key))
    # draw_block's counter layout: (ray lo, ray hi, block, stream), key = seed
    ray = np.array([5, 2 ** 32 - 1, 2 ** 32 + 3], dtype=np.uint64)
    w = np.stack(fs.draw_block(SEED, ray, 9), axis=1)
    for row, r in zip(w, ray):
        assert [int(x) for x in row] == orc.philox([int(r) & 0xFFFFFFFF, int(r) >> 32, 9, 0], [SEED & 0xFFFFFFFF, SEED >> 32])


@pytest.mark.parametrize("name", ["default", "port160", "rho0.9", "rho0.5", "scale0.01", "scale100", "max_points3", "max_points8",
                                  "first_wrap"])
def test_settled_rays_are_the_oracles_absorbed_rays(orc, name):
    cfg, n, first = _cases(orc)[name]
    fate, order, scanned = fs.fate_scan_np(cfg, n, SEED, first)
    status, npts, _, _ = orc.trace_endstates(cfg, n, SEED, first)
    settled = fate == fs.ABSORBED
    wrong = settled & (status != 2)
    assert not wrong.any(), (name, int(wrong.sum()), np.flatnonzero(wrong)[:5])
    assert np.array_equal(npts[settled], order[settled] + 2), name
    share, oracle_share = settled.mean(), (status == 2).mean()
    print(f"{name}: settled {share:.4f} of the rays, the oracle absorbs {oracle_share:.4f}; scanned {scanned / n:.2f} "
          f"interactions per ray, left to trace {1 - share:.4f}")
    if name == "default":
        assert share >= 0.95 * oracle_share, (share, oracle_share)
    else:
        assert settled.sum() > 0, name


def test_replayed_bounces_land_within_a_hundredth_of_the_margin(orc):
    """>= 2e5 explicit bounces on the oracle's primitives: |q.z - r_in sphere_z(wa)|, in words, times 100 stays below MARG."""
    cfg = orc.default_config()
    t = fs.thresholds(cfg)
    r_in = cfg.r_in
    d = np.array(cfg.dir[:])
    d = d / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])          # (rule S1 of the oracle takes a unit vector)
    kind0, q0 = orc.next_boundary(cfg, np.array(cfg.src[:]), d, K_NONE)
    assert kind0 == K_INNER
    to_words = 2.0 ** 31 / r_in
    assert abs((1.0 - 2.0 ** -32 - q0[2] / r_in) * 2.0 ** 31 - t["w_q0"]) <= 1.0   # the host's first strike is the oracle's
    worst, worst_r2, bounces, ray = 0.0, 0.0, 0, 0
    while bounces < 200_000:
        q, j = q0, 0
        while True:
            w = [int(x[0]) for x in fs.draw_block(SEED, np.array([ray], dtype=np.uint64), j >> 1)]
            wa, wb = w[2 * (j & 1)], w[2 * (j & 1) + 1]
            if wb >= t["rho_thr"]:
                break
            v = orc.cosine_emission(cfg, K_INNER, q, wa, wb)
            kind, q = orc.next_boundary(cfg, q, v, K_INNER)
            if kind != K_INNER:
                break
            bounces += 1
            worst = max(worst, abs(q[2] - r_in * float(fs.sphere_z(wa))) * to_words)
            worst_r2 = max(worst_r2, abs(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] - r_in * r_in))
            j += 1
        ray += 1
    print(f"{bounces} bounces of {ray} rays: max |q.z - r_in sphere_z(wa)| = {worst:.3g} words, max ||q|^2 - r_in^2| = {worst_r2:.3g}")
    assert worst * 100.0 < fs.MARG, worst
