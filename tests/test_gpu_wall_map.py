"""isx_wall_map on the GPU: map and four counters bit for bit against the oracle's wall points (tests/wallmap_np.py), route and
partition invariance, the identities of include/isx.h, the flatness of the diffuse wall irradiance, the host driver.

The BRDF source has no per-bounce oracle (the replay and the limit sweep walk the pencil source's trace): it is covered by the
identities, the census of isx_fluxmap and route / partition invariance."""
import os
import subprocess

import numpy as np
import pytest

import wallmap_np as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "altair-raytracing_amd", "host", "isx_macro")
SEED = 7
CENSUS = ("launched", "exited", "counted_below_z", "absorbed", "suspended", "wall_hits")


def _reset(isx):
    for k, v in (("assist", 1), ("assist_block", 0), ("pipeline", 1), ("ray_sub", 0), ("grid_blocks", 0), ("overlap", 0),
                 ("trace_block", 512), ("trace_blocks_per_cu", 0), ("bin_mode", 1), ("pipeline_chunk", 1 << 26),
                 ("surface_pipeline", 1), ("rays_per_lane", 0)):
        isx.set_option(k, v)


def _config(mod, kind):
    c = mod.default_config()
    if kind == "brdf":
        c.source_model = 1
    elif kind == "lobe":
        c.surface_model = 1
    elif kind == "rough":
        c.lambertian = 0; c.roughness_rad = 0.5
    elif kind == "chord":
        c.trace_mode = 1
    elif kind == "compat":
        c.hit_line_mode = 1
    elif kind == "port160":
        c.theta_max_deg = 160.0
    elif kind == "brdf_chord":
        c.source_model = 1; c.trace_mode = 1
    elif kind == "source2":          # another source point and direction
        c.src[0], c.src[1], c.src[2] = 10.0, -35.0, 20.0
        c.dir[0], c.dir[1], c.dir[2] = -1.0, 2.0, 3.0
    elif kind == "rho09":
        c.reflectance = 0.9
    elif kind != "default":
        raise ValueError(kind)
    return c


def _spec(isx, n_x=64, n_y=64, first_order=0):
    s = isx.default_wall_map_spec(isx.default_config())
    s.n_x, s.n_y, s.first_order = n_x, n_y, first_order
    return s


def _check_identities(m, k, st):
    assert int(m.sum()) == k.binned == st.bin_increments
    assert k.binned + k.outside + k.skipped + k.other_surface == st.wall_hits


def _equal(a, b):
    """two results of wall_map: the map, the four counters, the census"""
    assert np.array_equal(a[0], b[0])
    assert a[1].as_dict() == b[1].as_dict()
    for f in CENSUS + ("bin_increments",):
        assert getattr(a[2], f) == getattr(b[2], f), f


def _census_equals_fluxmap(isx, cfg, n, seed, st, first=0):
    _, fs = isx.fluxmap(cfg, n, seed, first)
    for f in CENSUS:
        assert getattr(st, f) == getattr(fs, f), f


# ------------------------------------------------------------------ bit for bit against the replay

_replays = {}


def _replayed(orc, kind, n):
    if (kind, n) not in _replays:
        _replays[(kind, n)] = W.replay(_config(orc, kind), n, SEED)
    return _replays[(kind, n)]


REPLAY_CASES = [
    # name, config, rays, spec
    ("default", "default", 20_000, {}),
    ("port160", "port160", 20_000, {}),
    ("source2", "source2", 20_000, {}),
    ("rho09", "rho09", 40_000, {}),
    ("first_order_1", "default", 20_000, {"first_order": 1}),
    ("first_order_3", "default", 20_000, {"first_order": 3}),
    ("non_square", "default", 20_000, {"n_x": 96, "n_y": 40}),
    ("one_bin", "default", 20_000, {"n_x": 1, "n_y": 1, "first_order": 1}),
    ("bin_limit", "default", 20_000, {"n_x": 128, "n_y": 64}),
    ("bin_limit_tall", "source2", 20_000, {"n_x": 16, "n_y": 512, "first_order": 1}),
]


@pytest.mark.parametrize("name,kind,n,spec_kw", REPLAY_CASES, ids=[c[0] for c in REPLAY_CASES])
def test_wall_map_equals_the_replay(isx, orc, name, kind, n, spec_kw):
    _reset(isx)
    spec = _spec(isx, **spec_kw)
    oc = _config(orc, kind)
    pts = _replayed(orc, kind, n)
    om, ok = W.wall_map_of_spec(pts, oc, spec)
    # the replay side first: no comparison of empty branches (the rim and the outer sphere are hit a few times in 1e4 interactions)
    print(name, ok, "interactions", pts[0].size)
    assert ok["binned"] > 100_000 and ok["other_surface"] > 0
    assert (ok["skipped"] > 0) == (spec.first_order > 0)
    if spec.first_order == 1 and kind == "default":
        assert ok["skipped"] == n
    # the library
    cfg = _config(isx, kind)
    m, k, st = isx.wall_map(cfg, n, SEED, spec)
    assert m.shape == (spec.n_y, spec.n_x) and m.dtype == np.uint64
    assert k.as_dict() == ok, name
    assert np.array_equal(m, om), name
    assert st.launched == n and st.wall_hits == pts[0].size
    _check_identities(m, k, st)
    _census_equals_fluxmap(isx, cfg, n, SEED, st)


# ------------------------------------------------------------------ bit for bit against the limit sweep

@pytest.mark.parametrize("kind", ["default", "chord", "lobe", "rough", "compat"])
def test_wall_map_equals_the_limit_sweep(isx, orc, kind):
    _reset(isx)
    n, M = 200_000, 6
    oc = _config(orc, kind)
    pts = W.limit_sweep(orc, oc, n, SEED, M)
    cfg = _config(isx, kind)
    cfg.max_points = M
    for spec in (_spec(isx), _spec(isx, 37, 101, 2)):
        om, ok = W.wall_map_of_spec(pts, oc, spec)
        print(kind, ok)
        assert ok["binned"] > 500_000 and (ok["skipped"] > 0) == (spec.first_order > 0)
        m, k, st = isx.wall_map(cfg, n, SEED, spec)
        assert k.as_dict() == ok, kind
        assert np.array_equal(m, om), kind
        assert st.wall_hits == pts[0].size
        _check_identities(m, k, st)
        _census_equals_fluxmap(isx, cfg, n, SEED, st)
    if kind == "compat":   # hit_line_mode is ignored
        d = _config(isx, "default"); d.max_points = M
        _equal((m, k, st), isx.wall_map(d, n, SEED, spec))


# ------------------------------------------------------------------ routes

ROUTES = [{"assist": 0}, {"pipeline": 0}, {"surface_pipeline": 0}, {"assist_block": 256}, {"assist_block": 512},
          {"rays_per_lane": 1}, {"rays_per_lane": 16}, {"grid_blocks": 1}, {"grid_blocks": 7}, {"ray_sub": 64}]


@pytest.mark.parametrize("kind", ["default", "chord", "brdf", "brdf_chord", "lobe", "rough", "port160"])
def test_route_invariance(isx, kind):
    _reset(isx)
    cfg, n = _config(isx, kind), 200_000
    spec = _spec(isx, 96, 40, 1)
    base = isx.wall_map(cfg, n, SEED, spec)
    _check_identities(*base)
    _census_equals_fluxmap(isx, cfg, n, SEED, base[2])
    assert base[1].binned > 1_000_000 and base[1].skipped > 0
    if kind.startswith("brdf"):   # j restarts for the scattered trace: more than one skipped interaction per launched ray
        assert base[1].skipped > n
    try:
        for opts in ROUTES:
            _reset(isx)
            for key, v in opts.items():
                isx.set_option(key, v)
            got = isx.wall_map(cfg, n, SEED, spec)
            _equal(got, base)
    finally:
        _reset(isx)


# ------------------------------------------------------------------ partitions

def test_partition_invariance(isx):
    """one 2e7-ray call == 4 calls with offset first_ray"""
    _reset(isx)
    cfg, n = isx.default_config(), 20_000_000
    spec = _spec(isx, 64, 64, 1)
    whole = isx.wall_map(cfg, n, SEED, spec)
    _check_identities(*whole)
    _census_equals_fluxmap(isx, cfg, n, SEED, whole[2])
    parts = [isx.wall_map(cfg, n // 4, SEED, spec, first_ray=i * (n // 4)) for i in range(4)]
    assert np.array_equal(sum(p[0] for p in parts), whole[0])
    for f in W.COUNT_FIELDS:
        assert sum(getattr(p[1], f) for p in parts) == getattr(whole[1], f), f
    for f in CENSUS + ("bin_increments",):
        assert sum(getattr(p[2], f) for p in parts) == getattr(whole[2], f), f


def test_device_form_accumulates_the_same_partition():
    """isx_wall_map_device for the same four quarters into caller-owned tensors == the one 2e7-ray call (a process of its own, as
    the flux map's device form: torch owns the tensors, the library's stream does the work)."""
    import sys
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import altair_raytracing_amd as isx
import wallmap_np as W
isx.load(); isx.init(0)
cfg = isx.default_config()
spec = isx.default_wall_map_spec(cfg)
spec.first_order = 1
n, SEED = 20000000, 7
d_map = torch.zeros(spec.n_x * spec.n_y, dtype=torch.int64, device="cuda:0")
d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda:0")
torch.cuda.synchronize()
for i in range(4):
    isx.wall_map_device(cfg, spec, n // 4, SEED, i * (n // 4), d_map.data_ptr(), d_cnt.data_ptr())
isx.sync()
st = isx.take_stats()
whole = isx.wall_map(cfg, n, SEED, spec)
torch.cuda.synchronize()
assert np.array_equal(d_map.cpu().numpy().astype(np.uint64).reshape(whole[0].shape), whole[0])
assert d_cnt.cpu().numpy().tolist() == [getattr(whole[1], f) for f in W.COUNT_FIELDS]
for f in ("launched", "exited", "counted_below_z", "absorbed", "suspended", "wall_hits", "bin_increments"):
    assert getattr(st, f) == getattr(whole[2], f), f
assert whole[1].binned > 10**9 and whole[1].skipped == n
# a missing pointer is refused before anything is enqueued
for args in ((0, d_cnt.data_ptr()), (d_map.data_ptr(), 0)):
    try:
        isx.wall_map_device(cfg, spec, 10, SEED, 0, *args)
        raise SystemExit("a NULL pointer was accepted")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_BAD_ARG
isx.shutdown()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]


def test_a_call_above_one_launch(isx):
    """1.5e8 rays in one call == 3 x 5e7"""
    _reset(isx)
    cfg = isx.default_config()
    spec = _spec(isx)
    whole = isx.wall_map(cfg, 150_000_000, SEED, spec)
    _check_identities(*whole)
    parts = [isx.wall_map(cfg, 50_000_000, SEED, spec, first_ray=i * 50_000_000) for i in range(3)]
    assert np.array_equal(sum(p[0] for p in parts), whole[0])
    for f in W.COUNT_FIELDS:
        assert sum(getattr(p[1], f) for p in parts) == getattr(whole[1], f), f
    assert sum(p[2].wall_hits for p in parts) == whole[2].wall_hits and whole[2].launched == 150_000_000


# ------------------------------------------------------------------ physics

def test_first_strike_is_one_bin(isx):
    _reset(isx)
    cfg, n = isx.default_config(), 1_000_000
    a = isx.wall_map(cfg, n, SEED, _spec(isx, 64, 64, 0))
    b = isx.wall_map(cfg, n, SEED, _spec(isx, 64, 64, 1))
    d = a[0].astype(np.int64) - b[0].astype(np.int64)
    assert int((d != 0).sum()) == 1 and int(d.max()) == a[2].launched == n
    assert b[1].skipped == n and a[1].skipped == 0


def test_flatness_on_the_gpu(isx):
    """2e6 rays, 32 x 32, first_order 1: the statistic and bound of the CPU test.  (The rim's non-uniform re-emission is expected
    to add less than 40 to chi2, against a 5 sigma margin of about 200.)"""
    _reset(isx)
    cfg = isx.default_config()
    m, k, st = isx.wall_map(cfg, 2_000_000, SEED, _spec(isx, 32, 32, 1))
    chi2, dof = W.flatness_chi2(m, cfg.theta_max_deg)
    print("chi2 %.1f for %d dof (bound %.1f), binned %d" % (chi2, dof, dof + 5 * np.sqrt(2 * dof), k.binned))
    assert dof > 400 and k.binned > 100_000_000
    assert chi2 <= dof + 5 * np.sqrt(2 * dof)


# ------------------------------------------------------------------ the ABI's refusals

def test_refused_specs(isx):
    _reset(isx)
    cfg = isx.default_config()
    bad = [_spec(isx, 0, 64), _spec(isx, 64, 0), _spec(isx, 513, 1), _spec(isx, 1, 513), _spec(isx, 128, 65), _spec(isx, 512, 17),
           _spec(isx, 64, 64, -1)]
    wrong = _spec(isx); wrong.struct_size = 20
    bad.append(wrong)
    for s in bad:
        with pytest.raises(isx.IsxError) as e:
            isx.wall_map(cfg, 1000, SEED, s)
        assert e.value.status == isx.abi.ERR_BAD_CONFIG, (s.n_x, s.n_y, s.first_order, s.struct_size)
    m, k, st = isx.wall_map(cfg, 1000, SEED, _spec(isx, 512, 16))   # the limit itself is served
    _check_identities(m, k, st)
    m, k, st = isx.wall_map(cfg, 0, SEED)                            # no rays: zeroed results
    assert int(m.sum()) == 0 and sum(k.as_dict().values()) == 0 and st.launched == 0


def test_single_kernel_time_is_reported(isx):
    _reset(isx)
    isx.wall_map(isx.default_config(), 2_000_000, SEED)
    single, trace, binning = isx.last_kernel_ms()
    assert single > 0 and trace == 0 and binning == 0


# ------------------------------------------------------------------ host driver, sharding

def test_host_driver_wall_map(isx, tmp_path):
    """isx_macro wallMap: the CSV's count column == wall_map with the same configuration, seed and ray range; the footer == the counters."""
    _reset(isx)
    env = dict(os.environ, ISX_QUIET="1")
    env.pop("ISX_RAYS", None); env.pop("ISX_SEED", None)
    r = subprocess.run([CLI, "wallMap", "--rays", "200000", "--bins", "32"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    found = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs if f.startswith("wall_map") and f.endswith(".csv")]
    assert len(found) == 1, found
    lines = open(found[0]).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    seed = int([l for l in head if l.startswith("# Seed:")][0].split(":")[1])
    body = [l for l in lines if not l.startswith("#")]
    assert body[0] == "ix,iy,X,Y,count" and len(body) == 1 + 32 * 32
    rows = np.array([[float(x) for x in l.split(",")] for l in body[1:]])
    m, k, st = isx.wall_map(isx.default_config(), 200_000, seed, _spec(isx, 32, 32, 0), 0)
    assert np.array_equal(rows[:, 4].astype(np.uint64).reshape(32, 32), m)
    assert np.array_equal(rows[:, 0].reshape(32, 32)[0], np.arange(32)) and np.allclose(rows[:, 2].reshape(32, 32)[0], -1 + (np.arange(32) + 0.5) / 16)
    foot = {l[2:].split(":")[0]: l.split(":")[1].strip() for l in head if ":" in l}
    assert (int(foot["Binned"]), int(foot["Outside"]), int(foot["Skipped"]), int(foot["Other surface"])) == \
           (k.binned, k.outside, k.skipped, k.other_surface)
    lo, mean, hi = (float(x) for x in foot["Count over those bins (min mean max)"].split())
    ax = np.maximum(np.abs(-1 + np.arange(32) / 16), np.abs(-1 + (np.arange(32) + 1) / 16))
    inside = (ax[None, :] ** 2 + ax[:, None] ** 2) <= np.sin(np.deg2rad(170.0) / 2) ** 2
    assert int(foot["Bins inside the wall disc"]) == int(inside.sum())
    assert (lo, hi) == (float(m[inside].min()), float(m[inside].max())) and mean == pytest.approx(m[inside].mean(), rel=1e-12)
    # --first-order reaches the spec
    r = subprocess.run([CLI, "wallMap", "--rays", "50000", "--bins", "8", "--first-order", "1", "folder=fo"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr


def test_wall_map_sharded_one_rank_equals_wall_map(isx):
    _reset(isx)
    cfg, spec = isx.default_config(), _spec(isx, 48, 48, 1)
    m, k, st = isx.wall_map(cfg, 300_000, SEED, spec)
    sm, sk, sc = isx.wall_map_sharded(isx.wall_map, cfg, spec, 300_000, SEED)
    assert np.array_equal(sm, m) and sk == k.as_dict()
    for f in CENSUS + ("bin_increments",):
        assert sc[f] == getattr(st, f), f
