"""Exit maps (include/isx.h: isx_exit_maps), the part that needs no GPU: the numpy restatement of the contract on hand-made end
states, the oracle-side figures the GPU tests lean on, the reference's 3dRayLog.txt as a 16 x 16 direction map against the oracle,
the sharded all-reduce over gloo, and the entry points' behaviour without a device."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import exitmap_np as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SEED = 6000, 77


def _states(p, v, status=None):
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    st = np.full(len(p), X.EXITED, dtype=np.int32) if status is None else np.asarray(status, dtype=np.int32)
    return st, np.ones(len(p), dtype=np.int32), p, v


# ------------------------------------------------------------------ the restatement itself, on hand-made end states

def test_direction_components_exactly_one_are_outside_and_minus_one_is_bin_zero():
    v = [[-1.0, 0.0, -0.0], [1.0, 0.0, -0.0], [0.0, -1.0, -0.0], [0.0, 1.0, -0.0], [-1.0, -1.0, -1.0]]
    m, binned, outside = X.direction_map(v, 8, 4)
    assert (binned, outside) == (3, 2)                       # +1 -> f == n: no bin
    assert m[2, 0] == 1 and m[0, 4] == 1 and m[0, 0] == 1 and m.sum() == 3


def test_direction_bin_edges_open_the_bin_above():
    n = 16                                                    # a power of two: the edges k * 2 / n - 1 and the formula are exact
    edges = np.array([k * 2.0 / n - 1.0 for k in range(n)])
    assert np.array_equal((edges + 1.0) * 0.5 * n, np.arange(n, dtype=float))
    v = np.stack([edges, np.zeros(n), -np.ones(n)], axis=1)
    m, binned, outside = X.direction_map(v, n, 1)
    assert binned == n and outside == 0 and np.array_equal(m[0], np.ones(n, dtype=np.uint64))      # edge k belongs to bin k
    below = edges[1:] - 1e-9                                  # under edge k (by more than the rounding of "+ 1.0"): bin k - 1
    m2, b2, _ = X.direction_map(np.stack([below, np.zeros(n - 1), -np.ones(n - 1)], axis=1), n, 1)
    assert b2 == n - 1 and np.array_equal(m2[0, :n - 1], np.ones(n - 1, dtype=np.uint64)) and m2[0, n - 1] == 0
    # any n: the bin is the floor of the formula as written, whatever k * 2 / n - 1 rounds to
    for n in (10, 37, 101):
        e = np.array([k * 2.0 / n - 1.0 for k in range(n)])
        want = np.floor((e + 1.0) * 0.5 * n).astype(int)
        assert (np.abs(want - np.arange(n)) <= 1).all()
        m3, _, _ = X.direction_map(np.stack([np.zeros(n), e, -np.ones(n)], axis=1), 1, n)
        assert np.array_equal(m3[:, 0], np.bincount(want, minlength=n).astype(np.uint64))


def test_plane_map_zero_and_denormal_vz():
    p = [[0.0, 0.0, -100.5]] * 5
    tiny = 5e-324
    v = [[0.0, 0.0, -0.0], [0.0, 0.0, 0.0], [0.6, 0.0, 0.8], [1.0, 0.0, -tiny], [0.0, 0.0, -1.0]]
    m, binned, outside, upward = X.plane_map(p, v, 4, 4, -101.0, 10.0)
    assert upward == 3                                        # -0.0, +0.0 and a positive dz: "v.z < 0.0 is false"
    assert outside == 1                                       # the denormal: t = 0.5 / 5e-324 = inf, x = inf
    assert binned == 1 and m[2, 2] == 1                       # straight down through (0, 0): f = 2.0 -> bin 2
    # a denormal dz with dx = 0: t = inf, x = 0 + inf * 0 = NaN -> outside as well
    _, b2, o2, u2 = X.plane_map([[0.0, 0.0, -100.5]], [[0.0, 0.0, -tiny]], 4, 4, -101.0, 10.0)
    assert (b2, o2, u2) == (0, 1, 0)


def test_plane_map_last_point_on_the_plane_and_crossings_at_the_extent():
    h = 8.0
    # p.z == plane_z: t = 0 / v.z = -0.0, the crossing is the last point itself
    m, binned, outside, upward = X.plane_map([[3.0, -5.0, -100.0]], [[0.6, 0.0, -0.8]], 4, 4, -100.0, h)
    assert (binned, outside, upward) == (1, 0, 0) and m[0, 2] == 1      # x = 3 -> f = 2.75, y = -5 -> f = 0.75
    # a crossing exactly at -half_extent is bin 0, exactly at +half_extent is outside
    p = [[-h, 0.0, -99.0], [h, 0.0, -99.0], [0.0, -h, -99.0], [0.0, h, -99.0]]
    v = [[0.0, 0.0, -1.0]] * 4
    m, binned, outside, upward = X.plane_map(p, v, 4, 4, -100.0, h)
    assert (binned, outside, upward) == (2, 2, 0) and m[2, 0] == 1 and m[0, 2] == 1


def test_nan_input_is_counted_outside_never_binned():
    nan = float("nan")
    es = _states([[nan, 0.0, -101.0], [0.0, 0.0, -101.0], [0.0, 0.0, -101.0]],
                 [[0.0, 0.0, -1.0], [nan, 0.0, -1.0], [0.0, 0.0, nan]])
    d, p, c, counted = X.exitmap_np(es, -100.0, 4, 4, 4, 4, -102.0, 5.0)
    assert counted == 3
    assert c == {"dir_binned": 2, "dir_outside": 1, "pos_binned": 0, "pos_outside": 2, "upward": 1}
    assert d.sum() == 2 and p.sum() == 0


def test_selection_and_identities_on_mixed_states():
    rng = np.random.default_rng(5)
    n = 4000
    v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1)[:, None]
    p = rng.uniform(-30, 30, size=(n, 3)); p[:, 2] = rng.uniform(-103.0, -97.0, size=n)
    status = rng.integers(1, 4, size=n)
    es = _states(p, v, status)
    d, pm, c, counted = X.exitmap_np(es, -100.0, 37, 101, 200, 5, -150.0, 40.0)
    assert counted == int(((status == 1) & (p[:, 2] < -100.0)).sum()) and 0 < counted < n
    assert d.shape == (101, 37) and pm.shape == (5, 200)
    assert c["dir_binned"] + c["dir_outside"] == counted == c["pos_binned"] + c["pos_outside"] + c["upward"]
    assert int(d.sum()) == c["dir_binned"] and int(pm.sum()) == c["pos_binned"] and c["upward"] > 0 and c["pos_outside"] > 0
    # one map only: that map of the two-map call, the other's counters 0
    d1, p1, c1, _ = X.exitmap_np(es, -100.0, 37, 101, 0, 0, 0.0, 0.0)
    assert np.array_equal(d1, d) and p1.shape == (0, 0) and c1["pos_binned"] == c1["pos_outside"] == c1["upward"] == 0


# ------------------------------------------------------------------ the oracle-side figures of the GPU comparisons

def test_oracle_side_figures(orc):
    """What the GPU tests compare against is not empty: the figures of the issue, exact (the oracle is deterministic)."""
    c = orc.default_config()
    d, p, k, counted = X.exitmap_np(orc.trace_endstates(c, 200_000, 7), c.exit_port_z, 128, 128, 64, 64, -100.0, 20.0)
    assert (counted, k["pos_outside"], k["upward"]) == (85163, 104, 0)
    assert (int((d > 0).sum()), int((p > 0).sum())) == (12938, 3089)
    b = c.copy(); b.source_model = 1
    es = orc.trace_endstates(b, 100_000, 7)
    d, p, k, counted = X.exitmap_np(es, b.exit_port_z, 128, 128, 64, 64, -100.0, 20.0)
    assert (counted, k["upward"], k["pos_binned"]) == (61930, 9189, 5262)
    sel = (es[0] == 1) & (es[2][:, 2] < b.exit_port_z)
    assert 0.9999 < es[3][sel][:, 2].max() < 1.0
    d, p, k, counted = X.exitmap_np(orc.trace_endstates(c, 100_000, 7), c.exit_port_z, 128, 128, 64, 64, -200.0, 150.0)
    assert (counted, k["pos_outside"]) == (42440, 11508)


# ------------------------------------------------------------------ against the reference's data

def raylog_chi2(dir_map, n_rays):
    """Two-sample chi2 of a 16 x 16 direction map against the reference's 3dRayLog.txt as such a map, over the cells whose pooled
    expectation in the log is >= 20.  -> (chi2, dof, share of the log's rays in the cells used)."""
    with open(os.path.join(ROOT, "tests", "golden", "raylog_dxdy_16x16.json")) as f:
        g = json.load(f)
    assert g["n"] == 100000 and g["binned"] == 100000 and g["outside"] == 0 and g["n_u"] == g["n_v"] == 16
    Hr = np.array(g["dir_map"], dtype=float)
    Ho = np.asarray(dir_map, dtype=float)
    assert Hr.shape == Ho.shape == (16, 16) and Hr.sum() == g["n"] and Ho.sum() == n_rays
    p = (Hr + Ho) / (Hr.sum() + Ho.sum())
    use = p * Hr.sum() >= 20
    chi2 = (((Hr / Hr.sum() - Ho / Ho.sum()) ** 2)[use] / (p * (1 / Hr.sum() + 1 / Ho.sum()))[use]).sum()
    return float(chi2), int(use.sum()) - 1, float(Hr[use].sum() / Hr.sum())


def raylog_config(mod):
    c = mod.default_config()
    c.src[2] = -80.0; c.reflectance = 1.0; c.roughness_rad = 0.0; c.max_points = 10000; c.box_half = 200.0
    return c


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_reference_ray_log_as_direction_map_against_the_oracle(orc, seed):
    """Measured: chi2 210.7 / 223.0 / 226.8 for 215 dof (p 0.57 / 0.34 / 0.28); the cells used hold 99.875 % of the log."""
    from scipy import stats
    c = raylog_config(orc)
    n = 1_000_000
    d, _, k, counted = X.exitmap_np(orc.trace_endstates(c, n, seed), c.exit_port_z, 16, 16, 0, 0, 0.0, 0.0)
    # rho = 1: every ray leaves through the port, but for the few that reach max_points first
    assert n - 100 < counted <= n and k["dir_binned"] == counted and k["dir_outside"] == 0
    chi2, dof, share = raylog_chi2(d, counted)
    print("seed %d: chi2 %.1f for %d dof, p %.3f, cells used hold %.3f %% of the log" % (seed, chi2, dof, stats.chi2.sf(chi2, dof), 100 * share))
    assert share >= 0.99
    assert stats.chi2.sf(chi2, dof) > 1e-4, (chi2, dof)


# ------------------------------------------------------------------ sharding over gloo

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Counts:
    def __init__(self, d):
        self.__dict__.update(d)


def _oracle_exit_maps(oracle, c, count, seed, spec, first):
    """The tracer a GPU box takes from altair_raytracing_amd.exit_maps, made of the oracle + the restatement."""
    es = oracle.trace_endstates(c, count, seed, first)
    d, p, k, counted = X.exitmap_of_spec(es, c, spec)
    st = oracle.Stats()
    st.launched = count; st.counted_below_z = counted; st.exited = int((es[0] == 1).sum()); st.absorbed = int((es[0] == 2).sum())
    st.suspended = int((es[0] == 3).sum()); st.bin_increments = k["dir_binned"] + k["pos_binned"]
    return d, p, _Counts(k), st


def _spec(isx, cfg):
    s = isx.default_exit_map_spec(cfg)
    s.n_u, s.n_v, s.n_x, s.n_y = 24, 20, 12, 16
    return s


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import oracle
    import altair_raytracing_amd as isx

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    cfg = oracle.default_config()
    spec = _spec(isx, isx.default_config())
    out = isx.exit_maps_sharded(lambda c, count, seed, sp, first: _oracle_exit_maps(oracle, c, count, seed, sp, first),
                                cfg, spec, N, SEED, first_ray=1000)
    q.put((rank,) + out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_exit_maps_sharded_allreduce_equals_single_rank(world, orc):
    import torch.multiprocessing as mp
    import altair_raytracing_amd as isx

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    cfg = orc.default_config()
    spec = _spec(isx, isx.default_config())
    wd, wp, wk, wst = _oracle_exit_maps(orc, cfg, N, SEED, spec, 1000)
    # one rank, no process group: the same function is the plain call
    sd, sp_, sk, sc = isx.exit_maps_sharded(lambda c, count, seed, s, first: _oracle_exit_maps(orc, c, count, seed, s, first),
                                            cfg, spec, N, SEED, first_ray=1000)
    assert np.array_equal(sd, wd) and np.array_equal(sp_, wp) and sk == wk.__dict__
    assert wd.sum() > 1000 and wp.sum() > 1000
    for rank, d, p, k, census in got:
        assert d.shape == (20, 24) and p.shape == (16, 12) and d.dtype == np.uint64
        assert np.array_equal(d, wd) and np.array_equal(p, wp), rank
        assert k == wk.__dict__, rank
        assert census["launched"] == N and census["counted_below_z"] == wst.counted_below_z
        assert census["bin_increments"] == k["dir_binned"] + k["pos_binned"]


# ------------------------------------------------------------------ the boundary without a device

def test_binding_structs_and_default_spec():
    import altair_raytracing_amd as isx
    assert C.sizeof(isx.ExitMapSpec) == 8 + 16 + 16 and C.sizeof(isx.ExitMapCounts) == 40
    cfg = isx.default_config()
    s = isx.default_exit_map_spec(cfg)
    assert s.struct_size == C.sizeof(isx.ExitMapSpec) and s.reserved0 == 0
    assert (s.n_u, s.n_v, s.n_x, s.n_y) == (128, 128, 64, 64) and s.plane_z == cfg.exit_port_z == -100.0
    assert s.half_extent == pytest.approx(1.25 * 100.1 * np.sin(np.deg2rad(170.0)), rel=1e-15)
    cfg.theta_max_deg = 160.0; cfg.exit_port_z = -94.0
    s = isx.default_exit_map_spec(cfg)
    assert s.plane_z == -94.0 and s.half_extent == pytest.approx(1.25 * 100.1 * np.sin(np.deg2rad(160.0)), rel=1e-15)
    for name in ("isx_default_exit_map_spec", "isx_exit_maps", "isx_exit_maps_device"):
        assert name in isx.EXPORTS and hasattr(isx.load(), name)


def test_entry_points_need_isx_init():
    """A process that never called isx_init(): both entry points answer ISX_ERR_NOT_INIT (whether or not a GPU is there)."""
    code = r"""
import sys
sys.path.insert(0, %r)
import altair_raytracing_amd as isx
cfg = isx.default_config()
spec = isx.default_exit_map_spec(cfg)
try:
    isx.exit_maps(cfg, 10, 1)
    print("no error")
except isx.IsxError as e:
    print("blocking", e.status)
try:
    isx.exit_maps_device(cfg, spec, 10, 1, 0, 4096, 4096, 4096)
    print("no error")
except isx.IsxError as e:
    print("device", e.status)
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["blocking", "-5", "device", "-5"], r.stdout
