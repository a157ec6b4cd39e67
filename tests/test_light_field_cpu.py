"""Port light field (include/isx.h: isx_light_field), the part that needs no GPU: the numpy restatement of the contract on
hand-made end states and on 20 000 rays of the oracle (identities, marginals against the exit maps' restatement), the binding's
structs and defaults, every refused spec, the entry points' status without a device, and the sharded all-reduce over gloo."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import exitmap_np as X
import lightfield_np as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SEED = 20_000, 7


@pytest.fixture(scope="module")
def endstates(orc):
    """20 000 rays of the default configuration: traced once, read by every test that needs them."""
    c = orc.default_config()
    es = orc.trace_endstates(c, N, SEED)
    for a in es:
        a.setflags(write=False)
    return c, es


# ------------------------------------------------------------------ the restatement on hand-made end states

def test_classification_order_on_hand_made_states():
    nan, tiny = float("nan"), 5e-324
    p = [[0.0, 0.0, -100.5]] * 7
    v = [[0.0, 0.0, -1.0],       # straight down through (0, 0): binned
         [0.0, 0.0, -0.0],       # upward (v.z < 0.0 is false)
         [1.0, 0.0, 0.5],        # upward comes first: its direction bin does not exist either
         [0.9, 0.0, -tiny],      # t = inf: pos_outside
         [1.0, 0.0, -1e6],       # a position bin, fu == n_u: dir_outside
         [nan, 0.0, -1.0],       # x = NaN: pos_outside (never dir_outside: the position comes first)
         [0.0, 0.0, nan]]        # NaN < 0.0 is false: upward
    f, k = LF.light_field(p, v, 4, 4, 4, 4, -101.0, 10.0)
    assert k == {"binned": 1, "pos_outside": 2, "dir_outside": 1, "upward": 3}
    assert f.shape == (4, 4, 4, 4) and f.sum() == 1 and f[2, 2, 2, 2] == 1
    # the layout: field[iy, ix, iv, iu], word ((iy n_x + ix) n_v + iv) n_u + iu
    f, k = LF.light_field([[3.0, -5.0, -100.0]], [[0.6, 0.0, -0.8]], 5, 3, 4, 2, -100.0, 8.0)
    assert k["binned"] == 1 and f.shape == (2, 4, 3, 5)
    iy, ix, iv, iu = (int(a[0]) for a in np.nonzero(f))
    assert (ix, iy, iu, iv) == (2, 0, 4, 1)     # fx = 11/16*4 = 2.75, fy = 3/16*2 = 0.375, fu = 1.6*0.5*5 = 4.0, fv = 1.5
    assert f.reshape(-1)[((iy * 4 + ix) * 3 + iv) * 5 + iu] == 1


def test_marginal_is_short_by_exactly_the_dir_outside_rays():
    rng = np.random.default_rng(11)
    n = 3000
    v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1)[:, None]
    p = rng.uniform(-15, 15, size=(n, 3)); p[:, 2] = rng.uniform(-103.0, -100.0, size=n)
    edge = rng.random(n) < 0.1
    v[edge, 0] = 1.0                                    # fu == n_u: no direction bin
    f, k = LF.light_field(p, v, 6, 7, 9, 5, -110.0, 30.0)
    pm, binned, outside, upward = X.plane_map(p, v, 9, 5, -110.0, 30.0)
    assert k["dir_outside"] > 50 and k["pos_outside"] > 50 and k["upward"] > 500 and k["binned"] > 500
    assert (k["upward"], k["pos_outside"]) == (upward, outside)
    assert k["binned"] + k["dir_outside"] == binned and sum(k.values()) == n
    short = pm.astype(np.int64) - f.sum(axis=(2, 3)).astype(np.int64)
    assert (short >= 0).all() and short.sum() == k["dir_outside"]
    # ... and those rays are the ones with the edge direction, bin by bin
    pe, _, _, _ = X.plane_map(p[edge], v[edge], 9, 5, -110.0, 30.0)
    assert np.array_equal(short, pe.astype(np.int64))


# ------------------------------------------------------------------ 20 000 rays of the oracle

@pytest.mark.parametrize("n_u,n_v,n_x,n_y,plane_z,half", [(16, 16, 4, 4, -100.0, 20.0), (37, 11, 5, 3, -100.0, 20.0),
                                                          (8, 8, 16, 16, -200.0, 150.0), (1, 1, 1, 1, -100.0, 1000.0)])
def test_identities_and_marginals_on_oracle_rays(endstates, n_u, n_v, n_x, n_y, plane_z, half):
    c, es = endstates
    f, k, counted = LF.light_field_np(es, c.exit_port_z, n_u, n_v, n_x, n_y, plane_z, half)
    assert counted > 8000 and k["binned"] > 5000
    assert f.shape == (n_y, n_x, n_v, n_u) and f.dtype == np.uint64
    assert sum(k.values()) == counted and int(f.sum()) == k["binned"]
    d, p, ek, ecounted = X.exitmap_np(es, c.exit_port_z, n_u, n_v, n_x, n_y, plane_z, half)
    assert ecounted == counted and (k["upward"], k["pos_outside"]) == (ek["upward"], ek["pos_outside"])
    assert k["dir_outside"] == 0                                       # (real unit directions below the port: |dx|, |dy| < 1)
    assert np.array_equal(f.sum(axis=(2, 3)), p)
    if k["pos_outside"] == 0 and k["upward"] == 0:
        assert np.array_equal(f.sum(axis=(0, 1)), d)
    else:                                                              # the direction marginal lacks the rays without a position
        lack = d.astype(np.int64) - f.sum(axis=(0, 1)).astype(np.int64)
        assert (lack >= 0).all() and lack.sum() == k["pos_outside"] + k["upward"]


def test_the_field_of_a_brdf_source_has_upward_rays(orc):
    c = orc.default_config(); c.source_model = 1
    es = orc.trace_endstates(c, N, SEED)
    f, k, counted = LF.light_field_np(es, c.exit_port_z, 8, 8, 8, 8, -100.0, 20.0)
    assert k["upward"] > 1000 and k["binned"] > 500 and sum(k.values()) == counted


# ------------------------------------------------------------------ the binding and the boundary without a device

NEW = ("isx_default_light_field_spec", "isx_light_field", "isx_light_field_device")


def test_binding_structs_and_default_spec():
    import altair_raytracing_amd as isx
    assert C.sizeof(isx.LightFieldCounts) == 32 and C.sizeof(isx.ExitMapSpec) == 40
    assert [n for n, _ in isx.LightFieldCounts._fields_] == list(LF.COUNT_FIELDS)
    cfg = isx.default_config()
    s = isx.default_light_field_spec(cfg)
    e = isx.default_exit_map_spec(cfg)
    assert s.struct_size == C.sizeof(isx.ExitMapSpec) and s.reserved0 == 0
    assert (s.n_u, s.n_v, s.n_x, s.n_y) == (32, 32, 32, 32)
    assert s.plane_z == cfg.exit_port_z == -100.0 and s.half_extent == e.half_extent
    cfg.theta_max_deg = 160.0; cfg.exit_port_z = -94.0
    s = isx.default_light_field_spec(cfg)
    assert s.plane_z == -94.0 and s.half_extent == isx.default_exit_map_spec(cfg).half_extent
    assert (isx.abi.LIGHT_FIELD_MAX_BINS, isx.abi.LIGHT_FIELD_MAX_AXIS) == (1 << 22, 1024)
    k = isx.LightFieldCounts(1, 2, 3, 4)
    assert k.as_dict() == {"binned": 1, "pos_outside": 2, "dir_outside": 3, "upward": 4}


def test_the_library_exports_what_the_header_declares():
    import altair_raytracing_amd as isx
    header = open(os.path.join(ROOT, "include", "isx.h")).read()
    for name in NEW:
        assert name + "(" in header and name in isx.EXPORTS and hasattr(isx.load(), name)
    assert "#define ISX_LIGHT_FIELD_MAX_BINS (1 << 22)" in header and "#define ISX_LIGHT_FIELD_MAX_AXIS 1024" in header
    out = subprocess.run(["nm", "-D", "--defined-only", isx.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("isx_")}
    assert set(NEW) <= exported
    assert exported - set(isx.EXPORTS) <= {"isx_diag_read"}, exported - set(isx.EXPORTS)
    assert set(isx.EXPORTS) <= exported


def refused_specs(isx):
    """(what, spec) for every spec include/isx.h refuses with ISX_ERR_BAD_CONFIG -- shared with tests/test_gpu_light_field.py"""
    good = isx.default_light_field_spec(isx.default_config())
    bad = []
    for delta in (-8, 8):
        s = good.copy(); s.struct_size += delta; bad.append(("struct_size %+d" % delta, s))
    for axis in ("n_u", "n_v", "n_x", "n_y"):
        for val in (0, -1, 1025):
            s = good.copy(); s.n_u = s.n_v = s.n_x = s.n_y = 1; setattr(s, axis, val); bad.append(("%s = %d" % (axis, val), s))
    s = good.copy(); s.n_u, s.n_v, s.n_x, s.n_y = 64, 64, 32, 33; bad.append(("2^22 + 2^17 bins", s))
    s = good.copy(); s.n_u, s.n_v, s.n_x, s.n_y = 1024, 1024, 1024, 1024; bad.append(("2^40 bins", s))
    s = good.copy(); s.n_u, s.n_v, s.n_x, s.n_y = 1024, 1024, 4, 2; bad.append(("2^23 bins", s))
    for h in (0.0, -1.0, float("nan"), float("inf")):
        s = good.copy(); s.half_extent = h; bad.append(("half %r" % h, s))
    for z in (float("nan"), float("-inf")):
        s = good.copy(); s.plane_z = z; bad.append(("plane_z %r" % z, s))
    return good, bad


def test_refused_specs_and_null_arguments_need_no_device():
    """A refused spec is ISX_ERR_BAD_CONFIG and a NULL spec / field ISX_ERR_BAD_ARG from both entry points, before anything asks
    for a device (this process never calls isx_init)."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ctypes as C
import numpy as np
import altair_raytracing_amd as isx
from test_light_field_cpu import refused_specs
lib = isx.load()
cfg = isx.default_config()
field = np.zeros(16, dtype=np.uint64)
fp = field.ctypes.data_as(C.POINTER(C.c_uint64))
good, bad = refused_specs(isx)
assert len(bad) >= 20
for what, s in bad:
    assert lib.isx_light_field(C.byref(cfg), C.byref(s), 10, 1, 0, fp, None, None) == isx.abi.ERR_BAD_CONFIG, what
    assert lib.isx_light_field_device(C.byref(cfg), C.byref(s), 10, 1, 0, C.c_void_p(4096), C.c_void_p(4096)) == isx.abi.ERR_BAD_CONFIG, what
assert lib.isx_light_field(C.byref(cfg), None, 10, 1, 0, fp, None, None) == isx.abi.ERR_BAD_ARG
assert lib.isx_light_field(C.byref(cfg), C.byref(good), 10, 1, 0, None, None, None) == isx.abi.ERR_BAD_ARG
assert lib.isx_light_field_device(C.byref(cfg), None, 10, 1, 0, C.c_void_p(4096), C.c_void_p(4096)) == isx.abi.ERR_BAD_ARG
assert lib.isx_light_field_device(C.byref(cfg), C.byref(good), 10, 1, 0, None, C.c_void_p(4096)) == isx.abi.ERR_BAD_ARG
wrong = cfg.copy(); wrong.struct_size += 8
assert lib.isx_light_field(C.byref(wrong), C.byref(good), 10, 1, 0, fp, None, None) == isx.abi.ERR_BAD_CONFIG
# the Python wrapper hands a refused spec to the library and raises its status
try:
    isx.light_field(cfg, 10, 1, bad[-1][1])
    print("no error")
except isx.IsxError as e:
    print("ok", e.status)
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["ok", "-2"], r.stdout


def test_entry_points_without_a_device():
    """Without a HIP device both entry points answer ISX_ERR_NO_DEVICE (there is no CPU path); where a device is present, a
    process that never called isx_init() gets ISX_ERR_NOT_INIT from both -- the status of isx_wall_map in the same process."""
    code = r"""
import sys
sys.path.insert(0, %r)
import altair_raytracing_amd as isx
lib = isx.load()
have = lib.isx_init(0) == 0
if have:
    lib.isx_shutdown()
cfg = isx.default_config()
spec = isx.default_light_field_spec(cfg)
got = []
for call in (lambda: isx.light_field(cfg, 10, 1), lambda: isx.light_field_device(cfg, spec, 10, 1, 0, 4096, 8192),
             lambda: isx.wall_map(cfg, 10, 1)):
    try:
        call()
        got.append(0)
    except isx.IsxError as e:
        got.append(e.status)
print("have" if have else "none", *got)
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    have, a, b, wall = r.stdout.split()
    import altair_raytracing_amd as isx
    want = isx.abi.ERR_NOT_INIT if have == "have" else isx.abi.ERR_NO_DEVICE
    assert (int(a), int(b), int(wall)) == (want, want, want), r.stdout


# ------------------------------------------------------------------ sharding

class _Counts:
    def __init__(self, d):
        self.__dict__.update(d)


def _oracle_light_field(oracle, c, count, seed, spec, first):
    """The tracer a GPU box takes from altair_raytracing_amd.light_field, made of the oracle + the restatement."""
    es = oracle.trace_endstates(c, count, seed, first)
    f, k, counted = LF.light_field_of_spec(es, c, spec)
    st = oracle.Stats()
    st.launched = count; st.counted_below_z = counted; st.exited = int((es[0] == 1).sum()); st.absorbed = int((es[0] == 2).sum())
    st.suspended = int((es[0] == 3).sum()); st.bin_increments = k["binned"]
    return f, _Counts(k), st


def _spec(isx, cfg):
    s = isx.default_light_field_spec(cfg)
    s.n_u, s.n_v, s.n_x, s.n_y = 6, 5, 4, 3
    return s


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import oracle
    import altair_raytracing_amd as isx

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    cfg = oracle.default_config()
    spec = _spec(isx, isx.default_config())
    out = isx.light_field_sharded(lambda c, count, seed, sp, first: _oracle_light_field(oracle, c, count, seed, sp, first),
                                  cfg, spec, 6000, 77, first_ray=1000)
    q.put((rank,) + out)
    dist.barrier()
    dist.destroy_process_group()


def test_light_field_sharded_allreduce_equals_single_rank(orc):
    import torch.multiprocessing as mp
    import altair_raytracing_amd as isx

    world = 3
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
    wf, wk, wst = _oracle_light_field(orc, cfg, 6000, 77, spec, 1000)
    # one rank, no process group: the same function is the plain call
    sf, sk, sc = isx.light_field_sharded(lambda c, count, seed, s, first: _oracle_light_field(orc, c, count, seed, s, first),
                                         cfg, spec, 6000, 77, first_ray=1000)
    assert np.array_equal(sf, wf) and sk == wk.__dict__ and wf.sum() > 1000
    for rank, f, k, census in got:
        assert f.shape == (3, 4, 5, 6) and f.dtype == np.uint64
        assert np.array_equal(f, wf), rank
        assert k == wk.__dict__, rank
        assert census["launched"] == 6000 and census["counted_below_z"] == wst.counted_below_z
        assert census["bin_increments"] == k["binned"]
