"""isx_wall_patches on the GPU: arrivals, absorbed and the census bit for bit against the replay on the oracle
(tests/wallpatch_np.py), ray counts, partition and launch-shape invariance, the device form, the identities of include/isx.h,
the binomial law of the absorbed counts, the host driver."""
import os
import subprocess
import sys

import numpy as np
import pytest

import wallpatch_np as W
from test_wall_patches_cpu import first_strike, three_patches

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "altair-raytracing_amd", "host", "isx_macro")
SEED = 7
CENSUS = W.CENSUS_FIELDS


def _reset(isx):
    for k, v in (("assist", 1), ("assist_block", 0), ("pipeline", 1), ("ray_sub", 0), ("grid_blocks", 0), ("overlap", 0),
                 ("trace_block", 512), ("trace_blocks_per_cu", 0), ("bin_mode", 1), ("pipeline_chunk", 1 << 26),
                 ("surface_pipeline", 1), ("rays_per_lane", 0)):
        isx.set_option(k, v)


# ------------------------------------------------------------------ the cases of the comparison with the replay

def _rotated_y(v, deg):
    a = np.deg2rad(deg)
    return np.array([v[0] * np.cos(a) + v[2] * np.sin(a), v[1], -v[0] * np.sin(a) + v[2] * np.cos(a)])


def _case(mod, name):
    """(cfg, WallPatchSpec) of a case; mod: a module with default_config() (the library or the oracle: same layout)"""
    import altair_raytracing_amd as isx
    c = mod.default_config()
    ic = isx.default_config()      # (isx_wall_patch_cap reads r_in alone)
    cap = lambda d, half, rho: isx.wall_patch_cap(ic, d, half, rho)
    if name in ("three", "three_150", "three_160"):
        if name != "three":
            c.theta_max_deg = float(name[-3:])
        return c, three_patches(isx, ic)
    q0 = first_strike(ic)
    if name == "rho1_limit12":            # a wall that absorbs nothing, a short bounce limit: suspended rays
        c.reflectance = 1.0; c.max_points = 12
        return c, isx.wall_patch_spec(ic, [cap((0, 0, 1), 25.0, 0.5), cap(q0, 10.0, 0.9)])
    if name == "all_in_front":            # patch 0 holds every point of the inner sphere: the others stay empty
        s = isx.wall_patch_spec(ic, [cap((1, 0, 0), 20.0, 0.9), cap((0, 0, 1), 30.0, 0.0), cap(q0, 15.0, 0.5)])
        s.patch[0].min_dot = -1e300
        return c, s
    if name == "none_in_front":           # patch 0 holds no point
        s = isx.wall_patch_spec(ic, [cap((1, 0, 0), 20.0, 0.0), cap((0, 0, 1), 30.0, 0.6), cap(q0, 15.0, 0.5)])
        s.patch[0].min_dot = 1e300
        return c, s
    if name == "twice":                   # two identical patches: the second stays empty
        p = cap((0, 1, 1), 35.0, 0.8)
        return c, isx.wall_patch_spec(ic, [p, p, cap(q0, 15.0, 0.5)])
    if name == "rho_one":                 # a patch that absorbs nothing on a wall that does: the 2^32 threshold
        return c, isx.wall_patch_spec(ic, [cap((0, 0, 1), 60.0, 1.0), cap(q0, 15.0, 1.0)])
    if name == "eight":
        dirs = [(0, 0, 1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (1, 1, 1), (-1, -1, 0.5), q0]
        return c, isx.wall_patch_spec(ic, [cap(d, 12.0 + 3 * k, (0.0, 0.3, 0.5, 0.7, 0.9, 0.95, 0.99, 1.0)[k]) for k, d in enumerate(dirs)])
    if name == "on_first_strike":         # a 5 degree cap round the first-strike point ...
        return c, isx.wall_patch_spec(ic, [cap(q0, 5.0, 0.5)])
    if name == "off_first_strike":        # ... and the same cap moved just off it
        return c, isx.wall_patch_spec(ic, [cap(_rotated_y(q0, 5.001), 5.0, 0.5)])
    if name == "source_outside":          # rule S1 does not find the first strike (Geom::q0_ok = 0): the source lies outside the
        c.src[0], c.src[1], c.src[2] = 0.0, 0.0, -150.0      # ball and shines in through the port
        c.dir[0], c.dir[1], c.dir[2] = 0.05, 0.02, 1.0
        return c, isx.wall_patch_spec(ic, [cap((0, 0, 1), 20.0, 0.5), cap((1, 0, 0), 40.0, 0.9)])
    if name == "source_at_rim":           # ... or the first segment crosses the port opening and meets the rim cone
        rim = np.array([100.5 * np.sin(np.deg2rad(10.0)), 0.0, -100.5 * np.cos(np.deg2rad(10.0))])
        s0 = np.array([c.src[0], c.src[1], c.src[2]])
        c.dir[0], c.dir[1], c.dir[2] = (float(x) for x in rim - s0)
        return c, isx.wall_patch_spec(ic, [cap((0, 0, 1), 40.0, 0.5), cap((1, 0, 0), 40.0, 0.9)])
    raise ValueError(name)


# name, rays (at most 6000 per replayed case)
CASES = [("three", 6000), ("three_150", 6000), ("three_160", 3000), ("rho1_limit12", 3000), ("all_in_front", 2000), ("none_in_front", 3000),
         ("twice", 3000), ("rho_one", 2000), ("eight", 3000), ("on_first_strike", 3000), ("off_first_strike", 3000),
         ("source_outside", 3000), ("source_at_rim", 3000)]
_replays = {}


def _replayed(orc, name, n):
    """the replay of a case: computed once, shared, never changed"""
    if (name, n) not in _replays:
        oc, spec = _case(orc, name)
        _replays[(name, n)] = W.replay(oc, W.spec_of(spec), n, SEED)
    return _replays[(name, n)]


def _equal_to_replay(isx, got, want, P):
    arr, ab, st = got
    warr, wab, wcensus = want[:3]
    assert arr.dtype == ab.dtype == np.uint64 and arr.shape == ab.shape == (P + 2,)
    assert np.array_equal(arr, warr), (arr, warr)
    assert np.array_equal(ab, wab), (ab, wab)
    for f in CENSUS:
        assert getattr(st, f) == wcensus[f], f
    _check_identities(arr, ab, st, P)


def _check_identities(arr, ab, st, P):
    assert int(arr.sum()) == st.wall_hits and int(ab.sum()) == st.absorbed
    assert st.bin_increments == int(arr[:P].sum())
    assert st.launched == st.exited + st.absorbed + st.suspended


@pytest.mark.parametrize("name,n", CASES, ids=[c[0] for c in CASES])
def test_wall_patches_equal_the_replay(isx, orc, name, n):
    _reset(isx)
    cfg, spec = _case(isx, name)
    P = spec.n_patches
    want = _replayed(orc, name, n)
    warr, wab, wcensus = want[:3]
    # the replay side first: no comparison of empty branches
    print(name, "arrivals", warr.tolist(), "absorbed", wab.tolist(), wcensus)
    assert int(warr[:P].max()) >= 100, name
    if name == "rho1_limit12":
        assert wcensus["suspended"] > 100 and wab[P] == 0
    if name == "all_in_front":
        assert warr[1] == warr[2] == warr[P] == 0 and warr[0] > 1000
    if name == "none_in_front":
        assert warr[0] == 0 and warr[1] > 100
    if name == "twice":
        assert warr[1] == 0 and warr[0] > 100
    if name == "rho_one":
        assert wab[0] == wab[1] == 0 and warr[0] > 1000 and wab[P] > 0
    if name == "eight":
        assert P == 8 and int((warr[:8] > 0).sum()) == 8
    if name == "on_first_strike":
        assert warr[0] >= n
    if name == "off_first_strike":
        assert 0 < warr[0] < n // 2
    if name.startswith("source_"):
        assert wcensus["wall_hits"] > 5 * n            # the rays still bounce
    got = isx.wall_patches(cfg, n, SEED, spec)
    _equal_to_replay(isx, got, want, P)


def test_the_replayed_cases_reach_the_other_surfaces(orc):
    """the rim cone and the outer sphere (class P + 1) are rare: across the cases of the comparison above there are enough"""
    total = 0
    for name, n in CASES:
        _, spec = _case(orc, name)
        total += int(_replayed(orc, name, n)[0][spec.n_patches + 1])
    print("other-surface arrivals across the cases:", total)
    assert total >= 20


@pytest.mark.parametrize("n", [1, 63, 64, 65, 6000])
def test_ray_counts(isx, orc, n):
    _reset(isx)
    cfg, spec = _case(isx, "three")
    want = _replayed(orc, "three", n)
    _equal_to_replay(isx, isx.wall_patches(cfg, n, SEED, spec), want, spec.n_patches)
    if n < 6000:   # the same rays further along the index range
        oc, _ = _case(orc, "three")
        want = W.replay(oc, W.spec_of(spec), n, SEED, first=12345, workers=1)
        _equal_to_replay(isx, isx.wall_patches(cfg, n, SEED, spec, first_ray=12345), want, spec.n_patches)


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for f in CENSUS + ("bin_increments",):
        assert getattr(a[2], f) == getattr(b[2], f), f


def test_no_rays(isx):
    _reset(isx)
    cfg, spec = _case(isx, "three")
    arr, ab, st = isx.wall_patches(cfg, 0, SEED, spec)
    assert int(arr.sum()) == 0 and int(ab.sum()) == 0 and st.launched == 0


def test_partition_invariance(isx):
    """three unequal calls == one call; a small pipeline_chunk (many launches per call) changes nothing"""
    _reset(isx)
    cfg, spec = _case(isx, "eight")
    n = 300_000
    whole = isx.wall_patches(cfg, n, SEED, spec)
    _check_identities(*whole, spec.n_patches)
    assert int(whole[0][:8].min()) > 1000
    cuts = [0, 1, 100_001, n]
    parts = [isx.wall_patches(cfg, cuts[i + 1] - cuts[i], SEED, spec, first_ray=cuts[i]) for i in range(3)]
    assert np.array_equal(sum(p[0] for p in parts), whole[0]) and np.array_equal(sum(p[1] for p in parts), whole[1])
    for f in CENSUS + ("bin_increments",):
        assert sum(getattr(p[2], f) for p in parts) == getattr(whole[2], f), f
    try:
        isx.set_option("pipeline_chunk", 4096)
        _same(isx.wall_patches(cfg, n, SEED, spec), whole)
    finally:
        _reset(isx)


SHAPES = [{"assist_block": 128}, {"assist_block": 256}, {"assist_block": 768}, {"rays_per_lane": 1}, {"rays_per_lane": 4}, {"ray_sub": 64},
          # the switches that select routes elsewhere select none here
          {"assist": 0}, {"pipeline": 0}, {"surface_pipeline": 0}]


@pytest.mark.parametrize("name", ["three", "source_at_rim"])
def test_launch_shape_invariance(isx, name):
    _reset(isx)
    cfg, spec = _case(isx, name)
    n = 200_000
    base = isx.wall_patches(cfg, n, SEED, spec)
    _check_identities(*base, spec.n_patches)
    try:
        for opts in SHAPES:
            _reset(isx)
            for key, v in opts.items():
                isx.set_option(key, v)
            _same(isx.wall_patches(cfg, n, SEED, spec), base)
    finally:
        _reset(isx)


def test_device_form_accumulates_into_prefilled_tensors():
    """isx_wall_patches_device for three unequal parts into caller-owned, pre-filled tensors == the one call on top of what was
    there (a process of its own, as the wall map's device form: torch owns the tensors, the library's stream does the work)."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import altair_raytracing_amd as isx
from test_gpu_wall_patches import _case
isx.load(); isx.init(0)
cfg, spec = _case(isx, "three")
P, n, SEED = spec.n_patches, 300000, 7
d_arr = torch.arange(100, 100 + P + 2, dtype=torch.int64, device="cuda:0")
d_ab = torch.full((P + 2,), 7, dtype=torch.int64, device="cuda:0")
torch.cuda.synchronize()
cuts = [0, 17, 100001, n]
for i in range(3):
    isx.wall_patches_device(cfg, spec, cuts[i + 1] - cuts[i], SEED, cuts[i], d_arr.data_ptr(), d_ab.data_ptr())
isx.sync()
st = isx.take_stats()
whole = isx.wall_patches(cfg, n, SEED, spec)
torch.cuda.synchronize()
assert np.array_equal(d_arr.cpu().numpy() - np.arange(100, 100 + P + 2), whole[0].astype(np.int64))
assert np.array_equal(d_ab.cpu().numpy() - 7, whole[1].astype(np.int64))
for f in ("launched", "exited", "counted_below_z", "absorbed", "suspended", "wall_hits", "bin_increments"):
    assert getattr(st, f) == getattr(whole[2], f), f
assert whole[0][1] >= n and whole[1][0] == whole[0][0] > 1000
# a missing pointer is refused before anything is enqueued
for args in ((0, d_ab.data_ptr()), (d_arr.data_ptr(), 0)):
    try:
        isx.wall_patches_device(cfg, spec, 10, SEED, 0, *args)
        raise SystemExit("a NULL pointer was accepted")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_BAD_ARG
isx.shutdown()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]


@pytest.mark.parametrize("kind", ["default", "port160", "rho1_limit12"])
def test_no_patches_and_same_rho_patches_leave_the_census_of_fluxmap(isx, kind):
    _reset(isx)
    cfg = isx.default_config()
    if kind == "port160":
        cfg.theta_max_deg = 160.0
    elif kind == "rho1_limit12":
        cfg.reflectance = 1.0; cfg.max_points = 12
    n = 2_000_000
    _, fs = isx.fluxmap(cfg, n, SEED)
    arr0, ab0, st0 = isx.wall_patches(cfg, n, SEED)
    assert arr0.shape == (2,) and st0.bin_increments == 0
    _check_identities(arr0, ab0, st0, 0)
    spec = three_patches(isx, isx.default_config())
    for k in range(spec.n_patches):
        spec.patch[k].reflectance = cfg.reflectance
    arr, ab, st = isx.wall_patches(cfg, n, SEED, spec)
    _check_identities(arr, ab, st, spec.n_patches)
    for f in CENSUS:
        assert getattr(st0, f) == getattr(fs, f), f
        assert getattr(st, f) == getattr(fs, f), f
    assert int(arr[:3].min()) > 10_000 and arr[4] == arr0[1] and int(arr[:4].sum()) == arr0[0]
    assert ab[4] == ab0[1] and int(ab[:4].sum()) == ab0[0]


def test_absorbed_counts_follow_the_binomial_law(isx):
    """absorbed[k] ~ Binomial(arrivals[k], 1 - rho_thr_k / 2^32) exactly (one fresh word per arrival): |z| < 5 per patch, a false
    failure about once in 2e6.  (The same statistic on the replay, at its own size: docs/LOG.md section 13.)"""
    _reset(isx)
    cfg = isx.default_config()
    q0 = first_strike(cfg)
    rhos = (0.5, 0.9, 0.99)
    spec = isx.wall_patch_spec(cfg, [isx.wall_patch_cap(cfg, (0, 0, 1), 20.0, rhos[0]), isx.wall_patch_cap(cfg, q0, 10.0, rhos[1]),
                                     isx.wall_patch_cap(cfg, (-1, 0, 0), 30.0, rhos[2])])
    arr, ab, st = isx.wall_patches(cfg, 2_000_000, SEED, spec)
    _check_identities(arr, ab, st, 3)
    for k, rho in enumerate(rhos):
        z = W.binomial_z(arr[k], ab[k], rho)
        print("patch %d rho %.2f: arrivals %d absorbed %d z %+.2f" % (k, rho, arr[k], ab[k], z))
        assert arr[k] > 1_000_000 and abs(z) < 5, (k, z)
    assert abs(W.binomial_z(arr[3], ab[3], cfg.reflectance)) < 5


def test_patches_change_the_port_fraction(isx):
    """a detector patch and a sample of lower reflectance take light from the port"""
    _reset(isx)
    cfg, spec = _case(isx, "three")
    n = 1_000_000
    _, _, plain = isx.wall_patches(cfg, n, SEED)
    arr, ab, st = isx.wall_patches(cfg, n, SEED, spec)
    assert st.counted_below_z < 0.5 * plain.counted_below_z and ab[0] == arr[0] > 10_000


def test_wall_patches_sharded_one_rank_equals_wall_patches(isx):
    _reset(isx)
    cfg, spec = _case(isx, "three")
    arr, ab, st = isx.wall_patches(cfg, 300_000, SEED, spec)
    sarr, sab, sc = isx.wall_patches_sharded(isx.wall_patches, cfg, spec, 300_000, SEED)
    assert np.array_equal(sarr, arr) and np.array_equal(sab, ab)
    for f in CENSUS + ("bin_increments",):
        assert sc[f] == getattr(st, f), f


def test_host_driver_wall_patches(isx, tmp_path):
    """isx_macro wallPatches: the CSV parsed back == wall_patches with the same caps, seed and ray range; the footer == the census."""
    _reset(isx)
    env = dict(os.environ, ISX_QUIET="1")
    env.pop("ISX_RAYS", None); env.pop("ISX_SEED", None)
    caps = [((0.0, 0.0, 1.0), 10.0, 0.0), ((66.0, 0.0, -75.0), 5.0, 0.5), ((66.0, 0.0, -75.0), 15.0, 0.9)]
    args = []
    for d, half, rho in caps:
        args += ["--patch", "%r,%r,%r,%r,%r" % (d[0], d[1], d[2], half, rho)]
    r = subprocess.run([CLI, "wallPatches", "--rays", "200000"] + args, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    found = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs if f.startswith("wall_patches") and f.endswith(".csv")]
    assert len(found) == 1, found
    lines = open(found[0]).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    seed = int([l for l in head if l.startswith("# Seed:")][0].split(":")[1])
    body = [l for l in lines if not l.startswith("#")]
    assert body[0] == "class,arrivals,absorbed,arrivals_per_sr" and len(body) == 1 + 5
    rows = [l.split(",") for l in body[1:]]
    cfg = isx.default_config()
    spec = isx.wall_patch_spec(cfg, [isx.wall_patch_cap(cfg, d, half, rho) for d, half, rho in caps])
    arr, ab, st = isx.wall_patches(cfg, 200_000, seed, spec, 0)
    assert [int(x[0]) for x in rows] == list(range(5))
    assert [int(x[1]) for x in rows] == arr.tolist() and [int(x[2]) for x in rows] == ab.tolist()
    for k, (d, half, rho) in enumerate(caps):
        sr = 2 * np.pi * (1 - np.cos(np.deg2rad(half)))
        assert float(rows[k][3]) == pytest.approx(int(arr[k]) / sr, rel=1e-9)
    assert rows[3][3] == "" and rows[4][3] == ""
    foot = {l[2:].split(":")[0]: l.split(":")[1].strip() for l in head if ":" in l}
    assert (int(foot["Launched"]), int(foot["Exited"]), int(foot["Counted below z"]), int(foot["Absorbed"]), int(foot["Suspended"]),
            int(foot["Wall hits"])) == (st.launched, st.exited, st.counted_below_z, st.absorbed, st.suspended, st.wall_hits)
    assert float(foot["Port fraction"]) == pytest.approx(st.counted_below_z / st.launched, rel=1e-12)
    # a refused cap is an error, not a run
    r = subprocess.run([CLI, "wallPatches", "--rays", "1000", "--patch", "0,0,0,10,0.5", "folder=bad"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
