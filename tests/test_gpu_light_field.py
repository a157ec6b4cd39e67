"""Port light field on the GPU (include/isx.h: isx_light_field): field, four counters and census bit for bit against the CPU
oracle + the numpy restatement (tests/lightfield_np.py) in both forms of the binning kernel, the seam between the forms, the same
field on every route and for every partition of a job, the device form, the marginals against isx_exit_maps, the refused specs,
the host driver's `lightField` entry and the sharded call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lightfield_np as LF
from test_light_field_cpu import refused_specs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "altair-raytracing_amd", "host", "isx_macro")
SEED = 7
CENSUS = ("launched", "exited", "counted_below_z", "absorbed", "suspended")   # (the oracle's end states carry no wall-hit count)
LDS_LIMIT = 32768                                                              # words of the largest field binned in LDS


def _reset(isx):
    for k, v in (("assist", 1), ("assist_block", 0), ("pipeline", 1), ("ray_sub", 0), ("grid_blocks", 0), ("overlap", 0),
                 ("trace_block", 512), ("trace_blocks_per_cu", 0), ("bin_mode", 1), ("pipeline_chunk", 1 << 26),
                 ("surface_pipeline", 1), ("rays_per_lane", 0), ("lf_global", 0)):
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


def _spec(isx, n_x, n_y, n_u, n_v, plane_z=-100.0, half=20.0):
    s = isx.default_light_field_spec(isx.default_config())
    s.n_u, s.n_v, s.n_x, s.n_y, s.plane_z, s.half_extent = n_u, n_v, n_x, n_y, plane_z, half
    return s


def _check_identities(f, k, st):
    assert int(f.sum()) == k.binned == st.bin_increments
    assert k.binned + k.pos_outside + k.dir_outside + k.upward == st.counted_below_z


def _equal(a, b):
    """two results of light_field: the field, the four counters, the census"""
    assert np.array_equal(a[0], b[0])
    assert a[1].as_dict() == b[1].as_dict()
    for f in CENSUS + ("bin_increments", "wall_hits"):
        assert getattr(a[2], f) == getattr(b[2], f), f


def _ran(isx, route):
    single, trace, binning = isx.last_kernel_ms()
    if route == "pipeline":
        assert trace > 0 and binning > 0 and single == 0, "the two-kernel pipeline ran"
    else:
        assert single > 0 and trace == 0 and binning == 0, "the fused kernel ran"


_ENDSTATES = {}


def _endstates(orc, kind, n):
    """the oracle's end states of a case: traced once, shared by the field sizes, never written"""
    key = (kind, n)
    if key not in _ENDSTATES:
        es = orc.trace_endstates(_config(orc, kind), n, SEED)
        for a in es:
            a.setflags(write=False)
        _ENDSTATES[key] = es
    return _ENDSTATES[key]


# ------------------------------------------------------------------ (a) bit for bit against the oracle, both forms

SMALL, LARGE = (4, 4, 16, 16), (16, 16, 16, 16)      # (n_x, n_y, n_u, n_v): 4 096 words -> LDS form, 65 536 -> global form
ASYM = (5, 3, 37, 11)                                 # 6 105 words: LDS form, and the global form through lf_global
ORACLE_CASES = [
    # name, config, rays, plane_z, half, what the ORACLE side must show (so that no comparison is one of empty branches),
    # occupied words of the field as observed on the oracle side: (SMALL, LARGE) -- for "asymmetric" the one spec
    ("default", "default", 200_000, -100.0, 20.0, {"counted": 85163, "pos_outside": 104, "upward": 0}, (3431, 31224)),
    ("brdf", "brdf", 100_000, -100.0, 20.0, {"counted": 61930, "upward": 9189}, (2396, 4893)),
    ("lobe", "lobe", 100_000, -100.0, 20.0, {}, (2689, 17258)),
    ("rough", "rough", 100_000, -100.0, 20.0, {}, (3342, 23213)),
    ("chord", "chord", 100_000, -100.0, 20.0, {}, (3285, 23836)),
    ("compat", "compat", 100_000, -100.0, 20.0, {}, (3285, 23836)),
    ("port160", "port160", 100_000, -100.0, 40.0, {}, (3116, 28790)),
    ("brdf_chord", "brdf_chord", 100_000, -100.0, 20.0, {}, (2396, 4893)),
    ("screen", "default", 100_000, -200.0, 150.0, {"counted": 42440, "pos_outside": 11508}, (413, 1750)),
    ("asymmetric", "default", 100_000, -100.0, 20.0, {}, (4825, 4825)),
]


@pytest.mark.parametrize("form", ["lds", "global"])
@pytest.mark.parametrize("name,kind,n,plane_z,half,want,occupied", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_light_field_equals_the_oracle(isx, orc, name, kind, n, plane_z, half, want, occupied, form):
    _reset(isx)
    axes = ASYM if name == "asymmetric" else SMALL if form == "lds" else LARGE
    spec = _spec(isx, *axes, plane_z=plane_z, half=half)
    words = int(np.prod(axes))
    assert (words <= LDS_LIMIT) == (form == "lds" or name == "asymmetric")
    oc = _config(orc, kind)
    es = _endstates(orc, kind, n)
    of, ok, counted = LF.light_field_of_spec(es, oc, spec)
    # the oracle side first
    seen = dict(ok, counted=counted)
    for key, val in want.items():
        assert seen[key] == val, (key, seen[key], val)
    assert counted > 10_000 and ok["binned"] > 1_000
    assert int((of > 0).sum()) == occupied[0 if form == "lds" or name == "asymmetric" else 1]
    if name == "brdf":
        sel = (es[0] == 1) & (es[2][:, 2] < oc.exit_port_z)
        assert es[3][sel][:, 2].max() > 0.9999
    # the library
    try:
        if name == "asymmetric" and form == "global":
            isx.set_option("lf_global", 1)
        f, k, st = isx.light_field(_config(isx, kind), n, SEED, spec)
        _ran(isx, "fused" if kind == "brdf_chord" else "pipeline")
    finally:
        _reset(isx)
    assert f.shape == (spec.n_y, spec.n_x, spec.n_v, spec.n_u) and f.dtype == np.uint64
    assert np.array_equal(f, of), name
    assert k.as_dict() == ok, name
    assert st.launched == n and st.counted_below_z == counted
    assert st.exited == int((es[0] == 1).sum()) and st.absorbed == int((es[0] == 2).sum()) and st.suspended == int((es[0] == 3).sum())
    _check_identities(f, k, st)
    # every other field of the census is the flux map's; upward and pos_outside are the exit maps'
    cfg = _config(isx, kind)
    _, fst = isx.fluxmap(cfg, n, SEED)
    for fld in CENSUS + ("wall_hits",):
        assert getattr(st, fld) == getattr(fst, fld), fld
    if form == "lds":
        e = isx.default_exit_map_spec(cfg)
        e.n_u, e.n_v, e.n_x, e.n_y, e.plane_z, e.half_extent = spec.n_u, spec.n_v, spec.n_x, spec.n_y, plane_z, half
        _, pm, ek, _ = isx.exit_maps(cfg, n, SEED, e)
        assert (k.upward, k.pos_outside) == (ek.upward, ek.pos_outside)
        assert np.array_equal(f.sum(axis=(2, 3)), pm) and k.dir_outside == 0
    if name == "compat":   # hit_line_mode is ignored: the field of the last segment
        _equal((f, k, st), isx.light_field(_config(isx, "default"), n, SEED, spec))


def test_default_spec_is_the_spec_of_a_call_without_one(isx):
    _reset(isx)
    cfg = isx.default_config()
    a = isx.light_field(cfg, 50_000, SEED)
    b = isx.light_field(cfg, 50_000, SEED, isx.default_light_field_spec(cfg))
    _equal(a, b)
    assert a[0].shape == (32, 32, 32, 32) and a[1].binned > 10_000
    _check_identities(*a)


# ------------------------------------------------------------------ (b) the seam between the two forms

@pytest.mark.parametrize("axes,option", [((8, 8, 32, 16), 0), ((8, 8, 32, 17), 0), ((4, 4, 8, 8), 1)],
                         ids=["limit", "limit_plus_one_step", "lf_global"])
def test_the_seam_between_the_forms(isx, orc, axes, option):
    """A field of exactly the LDS form's limit, one axis step above it, and the global form forced on a field that fits: all
    equal the oracle + numpy."""
    _reset(isx)
    assert (int(np.prod(axes)) <= LDS_LIMIT) == (axes != (8, 8, 32, 17)) and 8 * 8 * 32 * 16 == LDS_LIMIT
    n = 200_000
    spec = _spec(isx, *axes)
    oc = _config(orc, "default")
    of, ok, counted = LF.light_field_of_spec(_endstates(orc, "default", n), oc, spec)
    assert ok["binned"] > 80_000 and int((of > 0).sum()) > 500
    try:
        isx.set_option("lf_global", option)
        f, k, st = isx.light_field(_config(isx, "default"), n, SEED, spec)
        _ran(isx, "pipeline")
    finally:
        _reset(isx)
    assert np.array_equal(f, of) and k.as_dict() == ok and st.counted_below_z == counted
    _check_identities(f, k, st)


# ------------------------------------------------------------------ (c) routes, (d) partitions

@pytest.mark.parametrize("axes", [SMALL, LARGE], ids=["lds", "global"])
@pytest.mark.parametrize("kind", ["default", "lobe"])
def test_route_invariance(isx, kind, axes):
    _reset(isx)
    n = 300_000
    cfg, spec = _config(isx, kind), _spec(isx, *axes)
    try:
        one = isx.light_field(cfg, n, SEED, spec, 5)
        _ran(isx, "pipeline")
        _check_identities(*one)
        assert one[1].binned > 100_000
        for key in ("pipeline", "assist", "surface_pipeline"):
            _reset(isx)
            isx.set_option(key, 0)
            other = isx.light_field(cfg, n, SEED, spec, 5)
            _ran(isx, "fused" if key == "pipeline" or kind == "lobe" else "pipeline")
            _equal(one, other)
    finally:
        _reset(isx)


@pytest.mark.parametrize("axes", [SMALL, LARGE], ids=["lds", "global"])
def test_partition_invariance(isx, axes):
    """One call == the sum of three unequal calls over the same index range == the same call cut into five chunks."""
    _reset(isx)
    n, first = 300_000, 11
    cfg, spec = isx.default_config(), _spec(isx, *axes)
    try:
        one = isx.light_field(cfg, n, SEED, spec, first)
        _check_identities(*one)
        cuts = [0, 70_001, 199_999, n]
        parts = [isx.light_field(cfg, cuts[i + 1] - cuts[i], SEED, spec, first + cuts[i]) for i in range(3)]
        assert np.array_equal(sum(p[0] for p in parts), one[0])
        assert {f: sum(p[1].as_dict()[f] for p in parts) for f in LF.COUNT_FIELDS} == one[1].as_dict()
        for fld in CENSUS + ("bin_increments", "wall_hits"):
            assert sum(getattr(p[2], fld) for p in parts) == getattr(one[2], fld), fld
        isx.set_option("pipeline_chunk", 1 << 16)      # 300 000 rays: five trace / binning pairs
        _equal(one, isx.light_field(cfg, n, SEED, spec, first))
        _ran(isx, "pipeline")
    finally:
        _reset(isx)


def test_more_than_one_chunk_in_one_call(isx):
    """1.5e8 rays (three 2^26-ray chunks) in one call == the sum of three calls of 5e7, global form."""
    _reset(isx)
    cfg, spec = isx.default_config(), _spec(isx, *LARGE)
    n = 150_000_000
    one = isx.light_field(cfg, n, SEED, spec)
    _check_identities(*one)
    assert one[2].launched == n and one[1].binned > 60_000_000
    parts = [isx.light_field(cfg, n // 3, SEED, spec, i * (n // 3)) for i in range(3)]
    for p in parts:
        _check_identities(*p)
    assert np.array_equal(sum(p[0] for p in parts), one[0])
    assert {f: sum(p[1].as_dict()[f] for p in parts) for f in LF.COUNT_FIELDS} == one[1].as_dict()
    assert sum(p[2].counted_below_z for p in parts) == one[2].counted_below_z
    assert sum(p[2].wall_hits for p in parts) == one[2].wall_hits


# ------------------------------------------------------------------ (e) the device form

def test_device_form_accumulates():
    """isx_light_field_device twice into the same caller-owned, pre-filled tensors adds the two blocking calls to what was there, in
    both forms (a process of its own, as the other sinks' device forms: torch owns the tensors, the library's stream does the work)."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import altair_raytracing_amd as isx
import lightfield_np as LF
isx.load(); isx.init(0)
cfg = isx.default_config()
n, SEED = 500000, 7
for axes in ((4, 4, 16, 16), (16, 16, 16, 16)):
    spec = isx.default_light_field_spec(cfg)
    spec.n_x, spec.n_y, spec.n_u, spec.n_v = axes
    spec.half_extent = 20.0
    words = int(np.prod(axes))
    d_field = (torch.arange(words, dtype=torch.int64, device="cuda:0") %% 7) + 1
    d_cnt = torch.tensor([11, 22, 33, 44], dtype=torch.int64, device="cuda:0")
    before = d_field.cpu().numpy().astype(np.uint64)
    torch.cuda.synchronize()
    isx.light_field_device(cfg, spec, n, SEED, 0, d_field.data_ptr(), d_cnt.data_ptr())
    isx.light_field_device(cfg, spec, n, SEED, n, d_field.data_ptr(), d_cnt.data_ptr())
    isx.sync()
    st = isx.take_stats()
    a, b = isx.light_field(cfg, n, SEED, spec, 0), isx.light_field(cfg, n, SEED, spec, n)
    torch.cuda.synchronize()
    got = d_field.cpu().numpy().astype(np.uint64)
    assert np.array_equal(got, before + a[0].reshape(-1) + b[0].reshape(-1)), axes
    k = [a[1].as_dict()[f] + b[1].as_dict()[f] for f in LF.COUNT_FIELDS]
    assert d_cnt.cpu().numpy().tolist() == [11 + k[0], 22 + k[1], 33 + k[2], 44 + k[3]] and k[0] > 400000 and k[1] > 0
    assert st.launched == 2 * n and st.counted_below_z == a[2].counted_below_z + b[2].counted_below_z
    assert st.bin_increments == k[0] and st.wall_hits == a[2].wall_hits + b[2].wall_hits
isx.shutdown()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]


# ------------------------------------------------------------------ (f) the marginals against isx_exit_maps

def _exit_spec(isx, cfg, spec):
    e = isx.default_exit_map_spec(cfg)
    e.n_u, e.n_v, e.n_x, e.n_y, e.plane_z, e.half_extent = spec.n_u, spec.n_v, spec.n_x, spec.n_y, spec.plane_z, spec.half_extent
    return e


def test_marginals_are_the_exit_maps(isx, orc):
    """A plane that catches every ray (half_extent 1000): summed over the directions the field is the plane map, summed over the
    plane it is the direction map -- the exit maps of the same call, exactly."""
    _reset(isx)
    n = 200_000
    cfg, spec = isx.default_config(), _spec(isx, *LARGE, half=1000.0)
    of, ok, counted = LF.light_field_of_spec(_endstates(orc, "default", n), _config(orc, "default"), spec)
    assert ok == {"binned": counted, "pos_outside": 0, "dir_outside": 0, "upward": 0} and counted == 85163
    f, k, st = isx.light_field(cfg, n, SEED, spec)
    assert np.array_equal(f, of) and k.as_dict() == ok
    d, p, ek, est = isx.exit_maps(cfg, n, SEED, _exit_spec(isx, cfg, spec))
    assert np.array_equal(f.sum(axis=(2, 3)), p) and np.array_equal(f.sum(axis=(0, 1)), d)
    assert ek.pos_binned == ek.dir_binned == k.binned == est.counted_below_z == st.counted_below_z


def test_marginals_at_the_largest_field(isx):
    """64 x 64 x 32 x 32 = 2^22 words (32 MiB), 5e6 rays."""
    _reset(isx)
    n = 5_000_000
    cfg, spec = isx.default_config(), _spec(isx, 64, 64, 32, 32, half=1000.0)
    assert spec.n_x * spec.n_y * spec.n_u * spec.n_v == isx.abi.LIGHT_FIELD_MAX_BINS
    f, k, st = isx.light_field(cfg, n, SEED, spec)
    _ran(isx, "pipeline")
    _check_identities(f, k, st)
    assert f.shape == (64, 64, 32, 32) and k.binned == st.counted_below_z > 2_000_000
    d, p, ek, est = isx.exit_maps(cfg, n, SEED, _exit_spec(isx, cfg, spec))
    assert np.array_equal(f.sum(axis=(2, 3)), p) and np.array_equal(f.sum(axis=(0, 1)), d)
    assert (ek.pos_outside, ek.upward, ek.dir_outside) == (0, 0, 0) and ek.pos_binned == k.binned


# ------------------------------------------------------------------ (g) the boundary, the host driver, the sharded call

def test_bad_specs_are_refused(isx):
    _reset(isx)
    cfg = isx.default_config()
    lib = isx.load()
    field = np.zeros(1 << 20, dtype=np.uint64)
    fp = field.ctypes.data_as(C.POINTER(C.c_uint64))
    good, bad = refused_specs(isx)
    assert lib.isx_light_field(C.byref(cfg), C.byref(good), 1000, 1, 0, fp, None, None) == 0
    for what, s in bad:
        assert lib.isx_light_field(C.byref(cfg), C.byref(s), 1000, 1, 0, fp, None, None) == isx.abi.ERR_BAD_CONFIG, what
        # (a refused spec is refused before anything looks at the accumulators)
        assert lib.isx_light_field_device(C.byref(cfg), C.byref(s), 1000, 1, 0, C.c_void_p(4096), C.c_void_p(4096)) == isx.abi.ERR_BAD_CONFIG, what
    assert lib.isx_light_field(C.byref(cfg), None, 1000, 1, 0, fp, None, None) == isx.abi.ERR_BAD_ARG
    assert lib.isx_light_field(C.byref(cfg), C.byref(good), 1000, 1, 0, None, None, None) == isx.abi.ERR_BAD_ARG
    # the limits themselves are served: an axis of 1024, and every axis 1
    big = isx.light_field(cfg, 100_000, SEED, _spec(isx, 1024, 2, 1, 64))
    _check_identities(*big)
    assert big[0].shape == (2, 1024, 64, 1) and big[1].binned > 10_000
    one = isx.light_field(cfg, 100_000, SEED, _spec(isx, 1, 1, 1, 1))
    _check_identities(*one)
    assert one[0].shape == (1, 1, 1, 1) and int(one[0][0, 0, 0, 0]) == one[1].binned > 10_000
    isx.take_stats()


def test_host_driver_light_field(isx, tmp_path):
    """isx_macro lightField: the sparse CSV parsed back == light_field with the same configuration, seed and ray range."""
    _reset(isx)
    env = dict(os.environ, ISX_QUIET="1")
    env.pop("ISX_RAYS", None); env.pop("ISX_SEED", None)
    r = subprocess.run([CLI, "lightField", "--rays", "200000", "--seed", "3"], cwd=tmp_path, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    cfg = isx.default_config()
    spec = isx.default_light_field_spec(cfg)
    f, k, st = isx.light_field(cfg, 200_000, 3, spec, 0)
    lines = (tmp_path / "light_field.csv").read_text().splitlines()
    meta = {}
    for ln in lines:
        if ln.startswith("# "):
            key, _, val = ln[2:].partition(": ")
            meta[key] = val
    body = [ln for ln in lines if not ln.startswith("#")]
    assert body[0] == "ix,iy,iu,iv,count"
    rows = np.array([[int(x) for x in ln.split(",")] for ln in body[1:]], dtype=np.int64)
    assert (rows[:, 4] > 0).all() and len(rows) == int((f > 0).sum()) > 10_000
    word = ((rows[:, 1] * spec.n_x + rows[:, 0]) * spec.n_v + rows[:, 3]) * spec.n_u + rows[:, 2]
    assert (np.diff(word) > 0).all()                                   # the non-zero bins in index order
    back = np.zeros(f.size, dtype=np.uint64)
    back[word] = rows[:, 4].astype(np.uint64)
    assert np.array_equal(back.reshape(f.shape), f)
    assert meta["Number of rays"] == "200000" and meta["Seed"] == "3" and meta["First ray"] == "0"
    assert meta["Position bins (x x y)"] == "32 x 32" and meta["Direction bins (u x v)"] == "32 x 32"
    assert float(meta["Plane z"].rstrip("cm")) == spec.plane_z and float(meta["Plane half extent"].rstrip("cm")) == spec.half_extent
    assert [int(meta[key]) for key in ("Binned", "Position outside", "Direction outside", "Upward")] == \
        [k.binned, k.pos_outside, k.dir_outside, k.upward]
    assert int(meta["Rays through the exit port"]) == st.counted_below_z
    dx = 2.0 * spec.half_extent / 32
    norm = float(meta["Radiance normalisation (count / N dx dy du dv), N dx dy du dv"])
    assert norm == pytest.approx(200_000 * dx * dx * (2.0 / 32) * (2.0 / 32), rel=1e-14)


def test_light_field_sharded_one_rank_equals_light_field(isx):
    _reset(isx)
    cfg, spec = isx.default_config(), _spec(isx, *LARGE)
    f, k, st = isx.light_field(cfg, 300_000, SEED, spec)
    sf, sk, sc = isx.light_field_sharded(isx.light_field, cfg, spec, 300_000, SEED)
    assert np.array_equal(sf, f) and sk == k.as_dict()
    assert sc["counted_below_z"] == st.counted_below_z and sc["bin_increments"] == k.binned and sc["wall_hits"] == st.wall_hits
