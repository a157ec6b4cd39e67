"""Exit maps on the GPU (include/isx.h: isx_exit_maps): bit for bit against the CPU oracle + the numpy restatement for every source /
border / trace mode, the same maps on every route and for every partition of a job, against the library's own exit log, against
the reference's 3dRayLog.txt, the refused specs, and the host driver's `exitMaps` entry."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import exitmap_np as X
from test_exit_maps_cpu import raylog_chi2, raylog_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "altair-raytracing_amd", "host", "isx_macro")
SEED = 7
CENSUS = ("launched", "exited", "counted_below_z", "absorbed", "suspended")   # (the oracle's end states carry no wall-hit count)


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
    elif kind != "default":
        raise ValueError(kind)
    return c


def _spec(isx, n_u=128, n_v=128, n_x=64, n_y=64, plane_z=-100.0, half=20.0):
    s = isx.default_exit_map_spec(isx.default_config())
    s.n_u, s.n_v, s.n_x, s.n_y, s.plane_z, s.half_extent = n_u, n_v, n_x, n_y, plane_z, half
    return s


def _check_identities(d, p, k, st, both=True):
    assert int(d.sum()) == k.dir_binned and int(p.sum()) == k.pos_binned
    assert st.bin_increments == k.dir_binned + k.pos_binned
    if both or d.size:
        assert k.dir_binned + k.dir_outside == st.counted_below_z
    if both or p.size:
        assert k.pos_binned + k.pos_outside + k.upward == st.counted_below_z


def _equal(a, b):
    """two results of exit_maps: maps, the five counters, the census"""
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2].as_dict() == b[2].as_dict()
    for f in CENSUS + ("bin_increments", "wall_hits"):
        assert getattr(a[3], f) == getattr(b[3], f), f


def _sum(parts):
    d = sum(x[0].astype(np.uint64) for x in parts)
    p = sum(x[1].astype(np.uint64) for x in parts)
    k = {f: sum(x[2].as_dict()[f] for x in parts) for f in X.COUNT_FIELDS}
    return d, p, k


# ------------------------------------------------------------------ bit for bit against the oracle

ORACLE_CASES = [
    # name, config, rays, spec, what the ORACLE side must show so that the comparison is not one of empty branches
    ("default", "default", 200_000, {}, {"counted": 85163, "pos_outside": 104, "upward": 0, "dir_occupied": 12938, "pos_occupied": 3089}),
    ("brdf", "brdf", 100_000, {}, {"counted": 61930, "upward": 9189, "pos_binned": 5262}),
    ("lobe", "lobe", 100_000, {}, {}),
    ("rough", "rough", 100_000, {}, {}),
    ("chord", "chord", 100_000, {}, {}),
    ("compat", "compat", 100_000, {}, {}),
    ("port160", "port160", 100_000, {"half": 40.0}, {}),
    ("screen", "default", 100_000, {"plane_z": -200.0, "half": 150.0}, {"counted": 42440, "pos_outside": 11508}),
    ("asymmetric", "default", 100_000, {"n_u": 37, "n_v": 101, "n_x": 200, "n_y": 5}, {}),
]


@pytest.mark.parametrize("name,kind,n,spec_kw,want", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_exit_maps_equal_the_oracle(isx, orc, name, kind, n, spec_kw, want):
    _reset(isx)
    spec = _spec(isx, **spec_kw)
    oc = _config(orc, kind)
    es = orc.trace_endstates(oc, n, SEED)
    od, op, ok, counted = X.exitmap_of_spec(es, oc, spec)
    # the oracle side first
    seen = dict(ok, counted=counted, dir_occupied=int((od > 0).sum()), pos_occupied=int((op > 0).sum()))
    for key, val in want.items():
        assert seen[key] == val, (key, seen[key], val)
    assert counted > 10_000 and ok["dir_binned"] > 10_000 and ok["pos_binned"] > 1_000
    if name == "brdf":
        sel = (es[0] == 1) & (es[2][:, 2] < oc.exit_port_z)
        assert es[3][sel][:, 2].max() > 0.9999
    # the library
    d, p, k, st = isx.exit_maps(_config(isx, kind), n, SEED, spec)
    assert d.shape == (spec.n_v, spec.n_u) and p.shape == (spec.n_y, spec.n_x) and d.dtype == p.dtype == np.uint64
    assert np.array_equal(d, od), name
    assert np.array_equal(p, op), name
    assert k.as_dict() == ok, name
    assert st.launched == n and st.counted_below_z == counted
    assert st.exited == int((es[0] == 1).sum()) and st.absorbed == int((es[0] == 2).sum()) and st.suspended == int((es[0] == 3).sum())
    _check_identities(d, p, k, st)
    if name == "compat":   # hit_line_mode is ignored: the maps of the last segment
        _equal((d, p, k, st), isx.exit_maps(_config(isx, "default"), n, SEED, spec))


def test_default_spec_is_the_spec_of_a_call_without_one(isx):
    _reset(isx)
    cfg = isx.default_config()
    a = isx.exit_maps(cfg, 50_000, SEED)
    b = isx.exit_maps(cfg, 50_000, SEED, isx.default_exit_map_spec(cfg))
    _equal(a, b)
    assert a[0].shape == (128, 128) and a[1].shape == (64, 64) and a[2].pos_binned > 10_000


# ------------------------------------------------------------------ routes and partitions

@pytest.mark.parametrize("kind", ["default", "lobe"])
def test_route_and_partition_invariance(isx, kind):
    _reset(isx)
    n = 3_000_000
    cfg, spec = _config(isx, kind), _spec(isx)
    try:
        one = isx.exit_maps(cfg, n, SEED, spec, 5)
        single, trace, binning = isx.last_kernel_ms()
        assert trace > 0 and binning > 0 and single == 0, "the two-kernel pipeline ran"
        _check_identities(*one)
        assert one[2].dir_binned > 1_000_000 and one[2].pos_binned > 1_000_000
        thirds = [isx.exit_maps(cfg, 1_000_000, SEED, spec, 5 + i * 1_000_000) for i in range(3)]
        d, p, k = _sum(thirds)
        assert np.array_equal(d, one[0]) and np.array_equal(p, one[1]) and k == one[2].as_dict()
        assert sum(t[3].counted_below_z for t in thirds) == one[3].counted_below_z
        assert sum(t[3].wall_hits for t in thirds) == one[3].wall_hits
        for key, val in (("pipeline_chunk", 1 << 18), ("pipeline", 0), ("assist", 0), ("surface_pipeline", 0)):
            _reset(isx)
            isx.set_option(key, val)
            other = isx.exit_maps(cfg, n, SEED, spec, 5)
            kinds = isx.last_kernel_ms()
            if key == "pipeline" or (kind == "lobe" and key != "pipeline_chunk"):
                assert kinds[0] > 0 and kinds[1] == 0, (key, "the fused kernel ran")
            else:
                assert kinds[1] > 0 and kinds[2] > 0 and kinds[0] == 0, (key, "the pipeline ran")
            _equal(one, other)
    finally:
        _reset(isx)


@pytest.mark.parametrize("kind", ["brdf", "brdf_chord", "rough", "chord", "compat"])
def test_fused_fallback_equals_the_pipeline(isx, kind):
    """The BRDF source in chord mode has no pipeline kernel (fused at once); the others: pipeline == pipeline 0 == assist 0."""
    _reset(isx)
    n = 400_000
    cfg, spec = _config(isx, kind), _spec(isx, n_u=64, n_v=48, n_x=40, n_y=56, half=25.0)
    try:
        one = isx.exit_maps(cfg, n, SEED, spec)
        assert (isx.last_kernel_ms()[0] > 0) == (kind == "brdf_chord")
        _check_identities(*one)
        for key in ("pipeline", "assist"):
            _reset(isx)
            isx.set_option(key, 0)
            _equal(one, isx.exit_maps(cfg, n, SEED, spec))
    finally:
        _reset(isx)


def test_device_form_accumulates():
    """isx_exit_maps_device twice into the same caller-owned tensors == the sum of the two blocking calls (a process of its own,
    as the flux map's device form: torch owns the tensors, the library's stream does the work)."""
    import sys
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import altair_raytracing_amd as isx
import exitmap_np as X
isx.load(); isx.init(0)
cfg = isx.default_config()
spec = isx.default_exit_map_spec(cfg)
spec.half_extent = 20.0
n, SEED = 1000000, 7
d_dir = torch.zeros(spec.n_u * spec.n_v, dtype=torch.int64, device="cuda:0")
d_pos = torch.zeros(spec.n_x * spec.n_y, dtype=torch.int64, device="cuda:0")
d_cnt = torch.zeros(5, dtype=torch.int64, device="cuda:0")
torch.cuda.synchronize()
isx.exit_maps_device(cfg, spec, n, SEED, 0, d_dir.data_ptr(), d_pos.data_ptr(), d_cnt.data_ptr())
isx.exit_maps_device(cfg, spec, n, SEED, n, d_dir.data_ptr(), d_pos.data_ptr(), d_cnt.data_ptr())
isx.sync()
st = isx.take_stats()
a, b = isx.exit_maps(cfg, n, SEED, spec, 0), isx.exit_maps(cfg, n, SEED, spec, n)
torch.cuda.synchronize()
assert np.array_equal(d_dir.cpu().numpy().astype(np.uint64).reshape(a[0].shape), a[0] + b[0])
assert np.array_equal(d_pos.cpu().numpy().astype(np.uint64).reshape(a[1].shape), a[1] + b[1])
k = [a[2].as_dict()[f] + b[2].as_dict()[f] for f in X.COUNT_FIELDS]
assert d_cnt.cpu().numpy().tolist() == k and k[0] > 800000 and k[2] > 800000
assert st.launched == 2 * n and st.counted_below_z == a[3].counted_below_z + b[3].counted_below_z
assert st.bin_increments == k[0] + k[2] and st.wall_hits == a[3].wall_hits + b[3].wall_hits
# only the direction map wanted: the plane map's pointer may be NULL
spec.n_x = spec.n_y = 0
d_dir.zero_(); d_cnt.zero_(); torch.cuda.synchronize()
isx.exit_maps_device(cfg, spec, n, SEED, 0, d_dir.data_ptr(), 0, d_cnt.data_ptr())
isx.sync(); isx.take_stats()
assert np.array_equal(d_dir.cpu().numpy().astype(np.uint64).reshape(a[0].shape), a[0])
assert d_cnt.cpu().numpy().tolist() == [a[2].dir_binned, a[2].dir_outside, 0, 0, 0]
isx.shutdown()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]


def test_one_map_only(isx):
    _reset(isx)
    cfg, n = _config(isx, "brdf"), 300_000
    both = isx.exit_maps(cfg, n, SEED, _spec(isx))
    d_only = isx.exit_maps(cfg, n, SEED, _spec(isx, n_x=0, n_y=0))
    p_only = isx.exit_maps(cfg, n, SEED, _spec(isx, n_u=0, n_v=0))
    assert np.array_equal(d_only[0], both[0]) and d_only[1].shape == (0, 0)
    assert np.array_equal(p_only[1], both[1]) and p_only[0].shape == (0, 0)
    kb = both[2]
    assert d_only[2].as_dict() == {"dir_binned": kb.dir_binned, "dir_outside": kb.dir_outside, "pos_binned": 0, "pos_outside": 0, "upward": 0}
    assert p_only[2].as_dict() == {"dir_binned": 0, "dir_outside": 0, "pos_binned": kb.pos_binned, "pos_outside": kb.pos_outside,
                                   "upward": kb.upward}
    assert kb.upward > 1000
    _check_identities(*d_only, both=False)
    _check_identities(*p_only, both=False)


def test_more_than_one_chunk_in_one_call(isx):
    """1.5e8 rays: three 2^26-ray chunks in one call == the sum of its two halves."""
    _reset(isx)
    cfg, spec = isx.default_config(), _spec(isx)
    n = 150_000_000
    one = isx.exit_maps(cfg, n, SEED, spec)
    _check_identities(*one)
    assert one[3].launched == n and one[2].dir_binned > 60_000_000
    halves = [isx.exit_maps(cfg, n // 2, SEED, spec, i * (n // 2)) for i in range(2)]
    d, p, k = _sum(halves)
    assert np.array_equal(d, one[0]) and np.array_equal(p, one[1]) and k == one[2].as_dict()
    assert sum(h[3].counted_below_z for h in halves) == one[3].counted_below_z


# ------------------------------------------------------------------ inside the library, and against the reference's data

def test_direction_map_is_the_map_of_the_exit_log(isx):
    _reset(isx)
    cfg, n = isx.default_config(), 1_000_000
    spec = _spec(isx)
    d, p, k, st = isx.exit_maps(cfg, n, SEED, spec)
    ids, dirs, count, lst = isx.exit_directions(cfg, n, SEED)
    want, binned, outside = X.direction_map(dirs, spec.n_u, spec.n_v)
    assert np.array_equal(d, want) and (binned, outside) == (k.dir_binned, k.dir_outside)
    assert k.dir_binned + k.dir_outside == st.counted_below_z == count == len(ids) and count > 400_000


def test_direction_map_against_the_reference_ray_log(isx):
    """3dRayLog.txt as a 16 x 16 direction map against 1e6 rays of the library: two-sample chi2 over the cells whose pooled
    expectation in the log is >= 20 (they must hold >= 99 % of the log), p > 1e-4."""
    from scipy import stats
    _reset(isx)
    cfg, n = raylog_config(isx), 1_000_000
    d, _, k, st = isx.exit_maps(cfg, n, 11, _spec(isx, n_u=16, n_v=16, n_x=0, n_y=0))
    assert n - 100 < st.counted_below_z <= n and k.dir_binned == st.counted_below_z
    chi2, dof, share = raylog_chi2(d, k.dir_binned)
    print("chi2 %.1f for %d dof, p %.3f, cells used hold %.3f %% of the log" % (chi2, dof, stats.chi2.sf(chi2, dof), 100 * share))
    assert share >= 0.99
    assert stats.chi2.sf(chi2, dof) > 1e-4, (chi2, dof)


# ------------------------------------------------------------------ the boundary

def test_bad_specs_are_refused(isx):
    _reset(isx)
    cfg = isx.default_config()
    lib = isx.load()
    dmap = np.zeros(1 << 21, dtype=np.uint64)
    pmap = np.zeros(1 << 21, dtype=np.uint64)

    def call(spec):
        return lib.isx_exit_maps(C.byref(cfg), C.byref(spec), 1000, 1, 0, dmap.ctypes.data_as(C.POINTER(C.c_uint64)),
                                 pmap.ctypes.data_as(C.POINTER(C.c_uint64)), None, None)

    def call_device(spec):   # (a refused spec is refused before anything looks at the accumulators)
        return lib.isx_exit_maps_device(C.byref(cfg), C.byref(spec), 1000, 1, 0, C.c_void_p(4096), C.c_void_p(4096), C.c_void_p(4096))

    good = _spec(isx)
    assert call(good) == 0
    bad = []
    for delta in (-8, 8):
        s = good.copy(); s.struct_size += delta; bad.append(("struct_size", s))
    s = good.copy(); s.n_u = s.n_v = s.n_x = s.n_y = 0; bad.append(("no map", s))
    s = good.copy(); s.n_u = 129; bad.append(("129 x 128", s))
    s = good.copy(); s.n_x, s.n_y = 129, 128; bad.append(("plane 129 x 128", s))
    s = good.copy(); s.n_u, s.n_v = 1025, 1; bad.append(("axis 1025", s))
    s = good.copy(); s.n_u = 0; bad.append(("0 x 128", s))
    s = good.copy(); s.n_y = -1; bad.append(("negative", s))
    for h in (0.0, -1.0, float("nan"), float("inf")):
        s = good.copy(); s.half_extent = h; bad.append(("half %r" % h, s))
    s = good.copy(); s.plane_z = float("nan"); bad.append(("plane_z nan", s))
    for what, s in bad:
        assert call(s) == isx.abi.ERR_BAD_CONFIG, what
        assert call_device(s) == isx.abi.ERR_BAD_CONFIG, what
    # the limits themselves are served: 16 384 bins per map, an axis of 1024
    big = isx.exit_maps(cfg, 100_000, SEED, _spec(isx, n_u=1024, n_v=16, n_x=16, n_y=1024))
    _check_identities(*big)
    assert big[0].shape == (16, 1024) and big[1].shape == (1024, 16) and big[2].pos_binned > 10_000
    # a plane map that is not wanted does not look at plane_z / half_extent
    s = _spec(isx, n_x=0, n_y=0); s.half_extent = 0.0
    assert call(s) == 0
    isx.take_stats()


def test_host_driver_exit_maps(isx, tmp_path):
    """isx_macro exitMaps: both CSVs, their count columns == exit_maps with the same geometry, seed and ray range."""
    _reset(isx)
    env = dict(os.environ, ISX_QUIET="1")
    env.pop("ISX_RAYS", None); env.pop("ISX_SEED", None)
    r = subprocess.run([CLI, "exitMaps", "--rays", "200000", "--seed", "3"], cwd=tmp_path, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    cfg = isx.default_config()     # rootMacros' geometry (distributionSphereDetectorSweep.C)
    cfg.max_points = 10000; cfg.box_half = 200.0; cfg.reflectance = 1.0; cfg.roughness_rad = 0.0; cfg.src[2] = -80.0
    spec = isx.default_exit_map_spec(cfg)
    d, p, k, st = isx.exit_maps(cfg, 200_000, 3, spec, 0)

    def read(name):
        meta, rows = {}, []
        lines = (tmp_path / name).read_text().splitlines()
        for ln in lines:
            if ln.startswith("# "):
                key, _, val = ln[2:].partition(": ")
                meta[key] = val
        body = [ln for ln in lines if not ln.startswith("#")]
        return meta, body[0], np.array([[float(x) for x in ln.split(",")] for ln in body[1:]])

    meta, head, rows = read("exit_direction_map.csv")
    assert head == "u,v,count,intensity_per_sr"
    assert np.array_equal(rows[:, 2].astype(np.uint64).reshape(spec.n_v, spec.n_u), d) and d.sum() > 190_000
    du = 2.0 / spec.n_u
    assert rows[0, 0] == -1.0 + 0.5 * du and rows[1, 0] == -1.0 + 1.5 * du and rows[spec.n_u, 1] == -1.0 + 1.5 * (2.0 / spec.n_v)
    w2 = 1.0 - rows[:, 0] ** 2 - rows[:, 1] ** 2
    inside = w2 > 0
    assert (rows[~inside, 3] == 0).all()
    np.testing.assert_allclose(rows[inside, 3], rows[inside, 2] / (200_000 * du * (2.0 / spec.n_v) / np.sqrt(w2[inside])), rtol=1e-12)
    for m in (meta, read("exit_plane_map.csv")[0]):
        assert m["Number of rays"] == "200000" and m["Seed"] == "3" and m["First ray"] == "0"
        assert m["Direction bins (u x v)"] == "128 x 128" and m["Plane bins (x x y)"] == "64 x 64"
        assert float(m["Plane z"].rstrip("cm")) == spec.plane_z and float(m["Plane half extent"].rstrip("cm")) == spec.half_extent
        assert [int(m[key]) for key in ("Direction binned", "Direction outside", "Plane binned", "Plane outside", "Upward")] == \
            [k.dir_binned, k.dir_outside, k.pos_binned, k.pos_outside, k.upward]
        assert int(m["Rays through the exit port"]) == st.counted_below_z
    meta, head, rows = read("exit_plane_map.csv")
    assert head == "x_cm,y_cm,count,fraction_per_cm2"
    assert np.array_equal(rows[:, 2].astype(np.uint64).reshape(spec.n_y, spec.n_x), p) and p.sum() > 100_000
    dx = 2.0 * spec.half_extent / spec.n_x
    np.testing.assert_allclose(rows[:, 3], rows[:, 2] / (200_000 * dx * dx), rtol=1e-12)
    np.testing.assert_allclose(rows[:spec.n_x, 0], -spec.half_extent + (np.arange(spec.n_x) + 0.5) * dx, rtol=1e-14)
