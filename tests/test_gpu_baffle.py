"""Baffles on the GPU: isx_baffle_endstates and isx_fluxmap_baffle bit for bit against the replay on the oracle
(tests/baffle_np.py), the call without a baffle against isx_fluxmap, the edges of the interaction, partition and launch-shape
invariance, the device form.

The replays' arrival counts are asserted first in every parity test (a condition on the replay, not on the library): a test
cannot pass without baffle interactions.  Measured with the replay: shield 2e4 rays (403, 897); two (316, 767) and (3747, 4501);
first 1500 rays (1585, 53); shield at wall reflectance 0.99, seed 7, 4000 rays (292, 422) with 217 809 wall hits.

The fixture `first` as first proposed -- the shield with radius 12 about (30, 0, -85) -- does not lie inside the cavity:
|c| + radius = 90.14 + 12 = 102.14 > r_in = 100.1, and its rim at (34.0, 0, -96.3) is 102.1 from the centre, outside the wall.
isx.h refuses such a disc (ISX_ERR_BAD_CONFIG), so no call can be compared with its replay; the replay, which checks nothing,
still gives the quoted (1585, 53).  What the fixture is for -- the pencil's first strike lies on the baffle, so that the launch's
shared first segment is struck and every fresh ray starts its life in the assist wave -- is checked with `first_in`: the same
disc (radius 12, same normal and reflectance) 5 cm higher, about (30, 0, -80), |c| + radius = 97.4; 1500 rays, replay arrivals
(1586, 53), at least 40 per side asserted.  test_the_fixture_first_is_refused pins the refusal."""
import os
import subprocess
import sys

import numpy as np
import pytest

import baffle_np as BF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "altair-raytracing_amd", "host", "isx_macro")
SEED = 12345
CENSUS = BF.CENSUS_FIELDS
NORMAL = (-66.3, 0.0, -23.6)


def _reset(isx):
    for k, v in (("assist", 1), ("assist_block", 0), ("pipeline", 1), ("ray_sub", 0), ("grid_blocks", 0), ("overlap", 0),
                 ("trace_block", 512), ("trace_blocks_per_cu", 0), ("bin_mode", 1), ("pipeline_chunk", 1 << 26),
                 ("surface_pipeline", 1), ("rays_per_lane", 0), ("bin_cols", 1), ("bin_slots", 1), ("fate_scan", -1)):
        isx.set_option(k, v)


# name -> [(centre, direction, radius, reflectance)]
FIXTURES = {
    "none": [],
    "shield": [((30, 0, -85), NORMAL, 8.0, 0.9)],
    "first": [((30, 0, -85), NORMAL, 12.0, 0.9)],        # overhangs the wall: refused (the module's docstring)
    "first_in": [((30, 0, -80), NORMAL, 12.0, 0.9)],     # the pencil's first strike lies on the baffle
    "two": [((30, 0, -85), NORMAL, 8.0, 0.9), ((0, 0, 0), (0, 0, 1), 25.0, 0.5)],
    "black": [((30, 0, -85), NORMAL, 8.0, 0.0), ((0, 0, 0), (0, 0, 1), 25.0, 0.0)],
    "white": [((30, 0, -85), NORMAL, 8.0, 1.0), ((0, 0, 0), (0, 0, 1), 25.0, 1.0)],
    # the second of `two` tilted and moved so that it cuts the shield (its plane passes 2.8 cm from the shield's centre)
    "crossing": [((30, 0, -85), NORMAL, 8.0, 0.9), ((28, 0, -80), (0.6, 0, 0.8), 12.0, 0.5)],
    # met only on the way from the wall through the port to the box (the port's rim lies at z = -98.6)
    "port": [((0, 0, -95), (0, 0, 1), 3.0, 0.9)],
}


def _case(mod, name, rho=0.95, compat=False, max_points=None):
    """(cfg, BaffleSpec) of a fixture; mod: a module with default_config() (the library or the oracle: same layout)"""
    import altair_raytracing_amd as isx
    c = mod.default_config()
    c.reflectance = rho
    if compat:
        c.hit_line_mode = 1
    if max_points is not None:
        c.max_points = max_points
    ic = isx.default_config()
    return c, isx.baffle_spec(ic, [isx.baffle_disc(ic, *b) for b in FIXTURES[name]])


_replays = {}


def _replayed(orc, name, n, seed=SEED, first=0, rho=0.95, max_points=None):
    """the replay of a fixture: computed once, shared, never changed (the hit line plays no part in it)"""
    key = (name, n, seed, first, rho, max_points)
    if key not in _replays:
        oc, spec = _case(orc, name, rho, max_points=max_points)
        _replays[key] = BF.replay(oc, BF.spec_of(spec), n, seed, first, workers=None if n >= 2000 else 1)
    return _replays[key]


# (fixture, rays, wall reflectance, seed, first ray, least arrivals per side)
PARITY = [("shield", 20000, 0.95, SEED, 0, 200), ("first_in", 1500, 0.95, SEED, 0, 40), ("two", 20000, 0.95, SEED, 0, 200),
          ("shield", 4000, 0.99, 7, 0, 200), ("shield", 20000, 0.95, SEED, (1 << 32) + 7, 200)]
PARITY_IDS = ["shield", "first_in", "two", "shield-rho0.99", "shield-first-ray"]


def _arrivals_ok(rep, nb, least):
    arr = rep["arrivals"]
    print("replay arrivals", arr.tolist(), "absorbed", rep["absorbed"].tolist(), rep["census"])
    assert arr.shape[0] == nb and int(arr.min()) >= least, arr.tolist()


def _endstates_equal(got, rep):
    st, npts, lp, d, lb = got
    assert np.array_equal(st, rep["status"]) and np.array_equal(npts, rep["n_points"])
    assert np.array_equal(lp, rep["last_point"]), "last point"
    assert np.array_equal(d, rep["direction"]), "direction"
    assert np.array_equal(lb, rep["last_baffle"]), "last baffle"


def _counts_equal(cnt, rep):
    arr, ab = cnt.arrays()
    nb = rep["arrivals"].shape[0]
    assert np.array_equal(arr[:nb], rep["arrivals"]) and np.array_equal(ab[:nb], rep["absorbed"])
    assert not arr[nb:].any() and not ab[nb:].any()


def _fluxmap_equal(orc, oc, got, rep):
    hits, cnt, st = got
    P, V = BF.counted_lines(oc, rep)
    want = orc.bin_lines(oc, P, V)
    assert hits.dtype == np.uint64 and hits.shape == want.shape
    assert np.array_equal(hits, want)
    for f in CENSUS:
        assert getattr(st, f) == rep["census"][f], f
    assert st.bin_increments == int(want.sum())
    _counts_equal(cnt, rep)
    arr, ab = cnt.arrays()
    assert int(ab.sum()) <= st.absorbed and int(arr.sum()) <= st.wall_hits
    return P.shape[0]


def test_the_issues_replay_counts(orc):
    """the replay reproduces the arrival counts measured with the prototype"""
    assert _replayed(orc, "shield", 20000)["arrivals"].tolist() == [[403, 897]]
    assert _replayed(orc, "two", 20000)["arrivals"].tolist() == [[316, 767], [3747, 4501]]
    assert _replayed(orc, "first", 1500)["arrivals"].tolist() == [[1585, 53]]
    r = _replayed(orc, "shield", 4000, seed=7, rho=0.99)
    assert r["arrivals"].tolist() == [[292, 422]] and r["census"]["wall_hits"] == 217809
    assert _replayed(orc, "first_in", 1500)["arrivals"].tolist() == [[1586, 53]]


def test_the_fixture_first_is_refused(isx):
    """the shield with radius 12 reaches through the wall (the module's docstring): both compute calls refuse it, as isx.h says"""
    _reset(isx)
    cfg, spec = _case(isx, "first")
    c, r = np.array(spec.baffle[0].centre[:]), spec.baffle[0].radius
    assert np.sqrt(c @ c) + r > cfg.r_in
    for call in (lambda: isx.baffle_endstates(cfg, spec, 10, SEED), lambda: isx.fluxmap_baffle(cfg, spec, 10, SEED)):
        with pytest.raises(isx.IsxError) as e:
            call()
        assert e.value.status == isx.abi.ERR_BAD_CONFIG


@pytest.mark.parametrize("name,n,rho,seed,first,least", PARITY, ids=PARITY_IDS)
def test_baffle_endstates_equal_the_replay(isx, orc, name, n, rho, seed, first, least):
    _reset(isx)
    cfg, spec = _case(isx, name, rho)
    rep = _replayed(orc, name, n, seed, first, rho)
    _arrivals_ok(rep, spec.n_baffles, least)
    assert len(set(rep["status"].tolist())) >= 2        # exited and absorbed rays both
    _endstates_equal(isx.baffle_endstates(cfg, spec, n, seed, first_ray=first), rep)


@pytest.mark.parametrize("compat", [False, True], ids=["last-segment", "origin-compat"])
@pytest.mark.parametrize("name,n,rho,seed,first,least", PARITY, ids=PARITY_IDS)
def test_fluxmap_baffle_equals_the_replay(isx, orc, name, n, rho, seed, first, least, compat):
    _reset(isx)
    cfg, spec = _case(isx, name, rho, compat)
    oc, _ = _case(orc, name, rho, compat)
    rep = _replayed(orc, name, n, seed, first, rho)
    _arrivals_ok(rep, spec.n_baffles, least)
    lines = _fluxmap_equal(orc, oc, isx.fluxmap_baffle(cfg, spec, n, seed, first_ray=first), rep)
    print(name, "lines through the port:", lines)
    assert lines >= 100


def _same(a, b):
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].arrays()[0], b[1].arrays()[0]) and np.array_equal(a[1].arrays()[1], b[1].arrays()[1])
    for f in CENSUS + ("bin_increments",):
        assert getattr(a[2], f) == getattr(b[2], f), f


def test_no_baffle_is_the_flux_map(isx):
    """n_baffles == 0 at 2e5 rays: histogram and census are isx_fluxmap's, the end states isx_trace_endstates', bit for bit; the
    call takes its own kernels: the fate scan's launch counter does not move, whatever the option says"""
    _reset(isx)
    cfg = isx.default_config()
    spec = isx.default_baffle_spec(cfg)
    n = 200_000
    want = isx.fluxmap(cfg, n, SEED)
    try:
        for fs in (-1, 1):
            isx.set_option("fate_scan", fs)
            before = isx.fate_scan_launches()
            hits, cnt, st = isx.fluxmap_baffle(cfg, spec, n, SEED)
            assert isx.fate_scan_launches() == before
            assert np.array_equal(hits, want[0])
            for f in CENSUS + ("bin_increments",):
                assert getattr(st, f) == getattr(want[1], f), f
            assert not cnt.arrays()[0].any() and not cnt.arrays()[1].any()
    finally:
        _reset(isx)
    assert int(want[0].sum()) > 1000
    st, npts, lp, d, lb = isx.baffle_endstates(cfg, spec, n, SEED)
    wst, wnp, wlp, wd = isx.trace_endstates(cfg, n, SEED)
    assert np.array_equal(st, wst) and np.array_equal(npts, wnp) and np.array_equal(lp, wlp) and np.array_equal(d, wd)
    assert (lb == -1).all()


N_EDGE = 5000


@pytest.mark.parametrize("name,max_points", [("two", 4), ("two", 7), ("black", None), ("white", None), ("crossing", None), ("port", None)])
def test_edges_equal_the_replay(isx, orc, name, max_points):
    """a bounce limit that suspends rays right after a baffle interaction; reflectance 0 and 1; two baffles that cross each other;
    a baffle the rays meet only between the wall and the world box"""
    _reset(isx)
    cfg, spec = _case(isx, name, max_points=max_points)
    oc, _ = _case(orc, name, max_points=max_points)
    rep = _replayed(orc, name, N_EDGE, max_points=max_points)
    arr, ab = rep["arrivals"], rep["absorbed"]
    print(name, max_points, "replay arrivals", arr.tolist(), "absorbed", ab.tolist(), "suspended after a baffle",
          rep["suspended_after_baffle"], rep["census"])
    assert int(arr.sum()) > 0
    if max_points is not None:
        assert rep["suspended_after_baffle"] >= 1 and rep["census"]["suspended"] > rep["suspended_after_baffle"]
    if name == "black":
        assert np.array_equal(arr, ab) and int(arr.min()) > 0
    if name == "white":
        assert not ab.any() and int(arr.min()) > 0
    if name == "crossing":
        assert int(arr.min()) > 0
    if name == "port":      # (nearly) every arrival comes from above, on the way out
        assert arr[0, 0] >= 10 and arr[0, 0] > 5 * arr[0, 1]
    _endstates_equal(isx.baffle_endstates(cfg, spec, N_EDGE, SEED), rep)
    _fluxmap_equal(orc, oc, isx.fluxmap_baffle(cfg, spec, N_EDGE, SEED), rep)


def test_partition_invariance(isx):
    """`two`: 3e5 rays in one call == three calls of 1e5 at consecutive first_ray"""
    _reset(isx)
    cfg, spec = _case(isx, "two")
    n = 300_000
    whole = isx.fluxmap_baffle(cfg, spec, n, SEED)
    parts = [isx.fluxmap_baffle(cfg, spec, 100_000, SEED, first_ray=100_000 * k) for k in range(3)]
    assert np.array_equal(sum(p[0] for p in parts), whole[0])
    for i in (0, 1):
        assert np.array_equal(sum(p[1].arrays()[i] for p in parts), whole[1].arrays()[i])
    for f in CENSUS + ("bin_increments",):
        assert sum(getattr(p[2], f) for p in parts) == getattr(whole[2], f), f
    assert whole[2].launched == n and int(whole[0].sum()) > 1000 and int(whole[1].arrays()[0][:2].min()) > 1000


SHAPES = [{"assist_block": 128}, {"assist_block": 256}, {"assist_block": 768}, {"rays_per_lane": 1}, {"rays_per_lane": 4}, {"ray_sub": 64},
          {"pipeline_chunk": 4096}, {"bin_mode": 0}, {"bin_cols": 0},
          # the switches that select routes elsewhere change nothing here
          {"assist": 0}, {"pipeline": 0}, {"bin_mode": 2}, {"fate_scan": 1}]


def test_launch_shape_invariance(isx):
    _reset(isx)
    cfg, spec = _case(isx, "two")
    n = 300_000
    base = isx.fluxmap_baffle(cfg, spec, n, SEED)
    assert base[2].launched == n and int(base[0].sum()) > 1000
    try:
        for opts in SHAPES:
            _reset(isx)
            for key, v in opts.items():
                isx.set_option(key, v)
            _same(isx.fluxmap_baffle(cfg, spec, n, SEED), base)
    finally:
        _reset(isx)


@pytest.mark.parametrize("name", ["two", "first_in"])
def test_one_workgroup_with_full_rings(isx, name):
    """1e5 rays at wall reflectance 0.99 through ONE workgroup (`grid_blocks` 1): its 704 tracer lanes, the pending ring (512) and the
    resume ring (128) all fill with rays that want the assist wave or come back from it -- the state every workgroup of a large call
    is in -- and the result is that of the default launch.  (The assist wave must not wait for room in the resume ring there:
    docs/LOG.md section 18.)"""
    _reset(isx)
    cfg, spec = _case(isx, name, rho=0.99)
    n = 100_000
    base = isx.fluxmap_baffle(cfg, spec, n, SEED)
    assert int(base[1].arrays()[0].sum()) > n // 2 and int(base[0].sum()) > 1000
    try:
        isx.set_option("grid_blocks", 1)
        _same(isx.fluxmap_baffle(cfg, spec, n, SEED), base)
    finally:
        _reset(isx)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 769])
def test_ray_counts(isx, orc, n):
    """the trace kernel against the end-state kernel's own replay-checked answer at the smallest launches"""
    _reset(isx)
    cfg, spec = _case(isx, "two")
    oc, _ = _case(orc, "two")
    rep = _replayed(orc, "two", 769)
    part = {k: rep[k][:n] for k in BF.PER_RAY}
    _endstates_equal(isx.baffle_endstates(cfg, spec, n, SEED), part)
    hits, cnt, st = isx.fluxmap_baffle(cfg, spec, n, SEED)
    P, V = BF.counted_lines(oc, part)
    assert np.array_equal(hits, orc.bin_lines(oc, P, V))
    assert st.launched == n and st.wall_hits == int((part["n_points"] - 1 - (part["status"] == 1)).sum())
    assert st.absorbed == int((part["status"] == 2).sum()) and st.exited == int((part["status"] == 1).sum())


@pytest.mark.parametrize("nt,nph", [(36000, 1), (1, 36000), (190, 189)])
def test_a_grid_whose_tables_do_not_fit_the_lds_is_refused(isx, nt, nph):
    """within isx_fluxmap's 36000 bins, but the binning kernels' tables (4 B per bin, 32 B per row, 64 B per column) do not fit the
    160 KiB of a workgroup: ISX_ERR_BAD_CONFIG from the blocking call with hits, counts and census untouched and nothing launched;
    the same grid is no obstacle to isx_baffle_endstates, and a grid that fits (185 x 185) is served"""
    import ctypes as C
    _reset(isx)
    cfg, spec = _case(isx, "two")
    cfg.n_theta, cfg.n_phi = nt, nph
    lib = isx.load()
    isx.sync()
    isx.take_stats()
    buf = np.full(nt * nph, 7, dtype=np.uint64)
    cnt, st = isx.BaffleCounts(), isx.Stats()
    st.launched = 77
    cnt.arrivals[0][0] = 5
    rc = lib.isx_fluxmap_baffle(C.byref(cfg), C.byref(spec), 1000, SEED, 0, buf.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(cnt), C.byref(st))
    assert rc == isx.abi.ERR_BAD_CONFIG
    assert (buf == 7).all() and st.launched == 77 and cnt.arrivals[0][0] == 5 and int(cnt.arrays()[0].sum()) == 5
    left = isx.take_stats()
    assert (left.launched, left.wall_hits, left.bin_increments) == (0, 0, 0)
    out = isx.baffle_endstates(cfg, spec, 100, SEED)
    assert out[0].shape == (100,) and len(set(out[0].tolist())) >= 1
    cfg.n_theta, cfg.n_phi = 185, 185
    hits, cnt2, st2 = isx.fluxmap_baffle(cfg, spec, 20000, SEED)
    assert st2.launched == 20000 and hits.shape == (185, 185) and int(cnt2.arrays()[0][:2].min()) > 100


def test_no_rays(isx):
    _reset(isx)
    cfg, spec = _case(isx, "two")
    hits, cnt, st = isx.fluxmap_baffle(cfg, spec, 0, SEED)
    assert int(hits.sum()) == 0 and st.launched == 0 and st.wall_hits == 0 and not cnt.arrays()[0].any()
    out = isx.baffle_endstates(cfg, spec, 0, SEED)
    assert all(a.shape[0] == 0 for a in out)


def test_device_form_accumulates():
    """isx_fluxmap_baffle_device twice into caller-owned, pre-filled tensors == the sum of the blocking calls on top of what was
    there, and isx_take_stats adds up (a process of its own: torch owns the tensors, the library's stream does the work)."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import altair_raytracing_amd as isx
from test_gpu_baffle import _case
isx.load(); isx.init(0)
cfg, spec = _case(isx, "two")
SEED = 12345
nb = cfg.n_theta * cfg.n_phi
d_hits = torch.arange(5, 5 + nb, dtype=torch.int64, device="cuda:0")
d_cnt = torch.arange(100, 116, dtype=torch.int64, device="cuda:0")
torch.cuda.synchronize()
parts = [(0, 100001), (100001, 199999)]
for first, n in parts:
    isx.fluxmap_baffle_device(cfg, spec, n, SEED, first, d_hits.data_ptr(), d_cnt.data_ptr())
isx.sync()
st = isx.take_stats()
blocking = [isx.fluxmap_baffle(cfg, spec, n, SEED, first) for first, n in parts]
torch.cuda.synchronize()
hits = sum(b[0] for b in blocking)
assert np.array_equal(d_hits.cpu().numpy() - np.arange(5, 5 + nb), hits.reshape(-1).astype(np.int64))
want_cnt = np.concatenate([sum(b[1].arrays()[0] for b in blocking).reshape(-1), sum(b[1].arrays()[1] for b in blocking).reshape(-1)])
assert np.array_equal(d_cnt.cpu().numpy() - np.arange(100, 116), want_cnt.astype(np.int64))
for f in ("launched", "exited", "counted_below_z", "absorbed", "suspended", "wall_hits", "bin_increments"):
    assert getattr(st, f) == sum(getattr(b[2], f) for b in blocking), f
assert int(hits.sum()) > 1000 and want_cnt[:4].min() > 1000
# a grid whose tables do not fit the binning kernels' LDS: refused, nothing enqueued, the tensors as they were
big = cfg.copy(); big.n_theta, big.n_phi = 36000, 1
d_big = torch.full((36000,), 9, dtype=torch.int64, device="cuda:0")
cnt_before = d_cnt.clone()
torch.cuda.synchronize()
try:
    isx.fluxmap_baffle_device(big, spec, 1000, SEED, 0, d_big.data_ptr(), d_cnt.data_ptr())
    raise SystemExit("a grid that does not fit was accepted")
except isx.IsxError as e:
    assert e.status == isx.abi.ERR_BAD_CONFIG
isx.sync()
left = isx.take_stats()
torch.cuda.synchronize()
assert (left.launched, left.wall_hits, left.bin_increments) == (0, 0, 0)
assert bool((d_big == 9).all()) and bool((d_cnt == cnt_before).all())
for hp, cp in ((0, d_cnt.data_ptr()), (d_hits.data_ptr(), 0)):
    try:
        isx.fluxmap_baffle_device(cfg, spec, 10, SEED, 0, hp, cp)
        raise SystemExit("a NULL pointer was accepted")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_BAD_ARG
isx.shutdown()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]


def test_fluxmap_baffle_sharded_one_rank_equals_fluxmap_baffle(isx):
    _reset(isx)
    cfg, spec = _case(isx, "two")
    hits, cnt, st = isx.fluxmap_baffle(cfg, spec, 100_000, SEED)
    shits, arr, ab, sc = isx.fluxmap_baffle_sharded(isx.fluxmap_baffle, cfg, spec, 100_000, SEED)
    assert np.array_equal(shits, hits) and np.array_equal(arr, cnt.arrays()[0]) and np.array_equal(ab, cnt.arrays()[1])
    for f in CENSUS + ("bin_increments",):
        assert sc[f] == getattr(st, f), f


def test_host_driver_baffle_flux(isx, tmp_path):
    """isx_macro baffleFlux: the CSV in the flux maps' format parsed back == fluxmap_baffle with the same baffles, seed and ray
    range; the baffles and their counters stand in the metadata"""
    _reset(isx)
    env = dict(os.environ, ISX_QUIET="1")
    env.pop("ISX_RAYS", None); env.pop("ISX_SEED", None)
    n = 100_000      # (fractions are multiples of 1e-5: the six decimals of the format hold them)
    r = subprocess.run([CLI, "baffleFlux", "--rays", str(n), "--centre", "30,0,-85", "--normal", "-66.3,0,-23.6", "--radius", "8",
                        "--reflectance", "0.9", "--centre", "0,0,0", "--normal", "0,0,1", "--radius", "25", "--reflectance", "0.5"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    found = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs if f.startswith("baffle_flux") and f.endswith(".csv")]
    assert len(found) == 1, found
    lines = open(found[0]).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    meta = {l[2:].split(":")[0]: l.split(":", 1)[1].strip() for l in head if ":" in l}
    assert meta["Baffles"] == "2" and meta["Baffle 0 radius"] == "8cm" and meta["Baffle 1 reflectance"] == "0.5"
    assert meta["Baffle 0 centre (x,y,z)"] == "30cm, 0cm, -85cm" and meta["Baffle 1 normal (x,y,z)"] == "0, 0, 1"
    body = [l for l in lines if not l.startswith("#")]
    cfg = isx.default_config()      # (the macro's sphere: the default configuration, wall reflectance 0.99)
    assert body[0] == "theta,phi,fraction" and len(body) == 1 + cfg.n_theta * cfg.n_phi
    spec = _case(isx, "two")[1]
    hits, cnt, st = isx.fluxmap_baffle(cfg, spec, n, int(meta["Seed"]), int(meta["First ray"]))
    got = np.array([round(float(l.split(",")[2]) * n) for l in body[1:]], dtype=np.uint64).reshape(cfg.n_theta, cfg.n_phi)
    assert np.array_equal(got, hits) and int(hits.sum()) > 1000
    arr, ab = cnt.arrays()
    for k in (0, 1):
        assert meta["Baffle %d arrivals (side 0, side 1)" % k] == "%d, %d" % (arr[k, 0], arr[k, 1])
        assert meta["Baffle %d absorbed (side 0, side 1)" % k] == "%d, %d" % (ab[k, 0], ab[k, 1])
    assert int(arr[:2].min()) > 100
    assert (int(meta["Launched"]), int(meta["Exited"]), int(meta["Absorbed"]), int(meta["Suspended"]), int(meta["Wall hits"]),
            int(meta["Detector hits"])) == (st.launched, st.exited, st.absorbed, st.suspended, st.wall_hits, st.bin_increments)
    assert meta["Total rays exiting port"] == "%d out of %d" % (st.counted_below_z, n)
    # a baffle the library refuses is an error, not a run; so are a baffle short of an option and an argument that is no number
    for bad in (["--centre", "30,0,-85", "--normal", "-66.3,0,-23.6", "--radius", "12", "--reflectance", "0.9"],
                ["--centre", "0,0,0", "--normal", "0,0,1", "--radius", "25"],
                ["--centre", "0,x,0", "--normal", "0,0,1", "--radius", "25", "--reflectance", "0.5"],
                ["--centre", "0,0,0", "--normal", "0,0", "--radius", "25", "--reflectance", "0.5"],
                ["--centre", "0,0,0", "--normal", "0,0,1", "--radius", "25", "--reflectance", "half"]):
        r = subprocess.run([CLI, "baffleFlux", "--rays", "1000"] + bad + ["folder=bad"], cwd=tmp_path, env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode != 0, bad
