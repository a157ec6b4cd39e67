"""isx_order_hist without a GPU: the numpy restatement of the contract (tests/orderhist_np.py) on oracle end states, the ABI's
structs and defaults, every refused spec, the entry points' status without a device, isx_order_reweight (host code) against
numpy, and the sharded all-reduce over gloo."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import orderhist_np as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7


def config(mod, kind):
    """the configurations of the order-histogram tests (mod: the oracle binding or the product package)"""
    c = mod.default_config()
    if kind == "brdf":
        c.source_model = 1
    elif kind == "brdf_chord":
        c.source_model = 1; c.trace_mode = 1
    elif kind == "lobe":
        c.surface_model = 1
    elif kind == "rough":
        c.lambertian = 0; c.roughness_rad = 0.5
    elif kind == "chord":
        c.trace_mode = 1
    elif kind == "port160":
        c.theta_max_deg = 160.0
    elif kind == "source2":          # another source point and direction
        c.src[0], c.src[1], c.src[2] = 10.0, -35.0, 20.0
        c.dir[0], c.dir[1], c.dir[2] = -1.0, 2.0, 3.0
    elif kind == "rho09":
        c.reflectance = 0.9
    elif kind == "rho1":             # no absorbed rays
        c.reflectance = 1.0
    elif kind == "limit6":           # class 3 is populated, k sits at the limit
        c.max_points = 6
    elif kind == "cut150":           # a cut below the port plane: rays that leave sideways are exited, not counted (class 1)
        c.exit_port_z = -150.0
    elif kind != "default":
        raise ValueError(kind)
    return c


_endstates = {}


def endstates(orc, kind, n, seed=SEED, first=0):
    """oracle end states, computed once per (configuration, n, seed, first) and shared; never modified"""
    key = (kind, n, seed, first)
    if key not in _endstates:
        _endstates[key] = orc.trace_endstates(config(orc, kind), n, seed, first)
    return _endstates[key]


# ------------------------------------------------------------------ the restatement on oracle rays

@pytest.mark.parametrize("kind", ["default", "chord", "lobe", "rough", "brdf", "rho1", "limit6", "cut150"])
def test_identities_on_oracle_rays(orc, kind):
    c = config(orc, kind)
    n = 20_000
    es = endstates(orc, kind, n)
    cen = H.census_np(es, c.exit_port_z)
    k, cl = H.classify(es, c.exit_port_z)
    for n_orders, n_dz in ((512, 8), (40, 8), (2048, 0), (1, 0), (128, 60), (64, 1)):
        hist, dz, cnt = H.order_hist_np(es, c.exit_port_z, n_orders, n_dz)
        assert hist.shape == (4, n_orders) and dz.shape == (n_orders, n_dz) and hist.dtype == dz.dtype == np.uint64
        H.check_identities(hist, dz, cnt, cen, n_dz)
        assert sum(cnt["overflow"]) == int((k >= n_orders).sum())
    print(kind, cen, "k max", int(k.max()))
    # the branch the configuration is here for
    if kind == "rho1":
        assert cen["absorbed"] == 0 and cen["suspended"] == 0
    if kind == "limit6":
        # (a ray is suspended when its next point would be one too many: it has max_points interactions behind it)
        assert cen["suspended"] > 10_000 and int(k[cl == 3].min()) == int(k.max()) == c.max_points
    if kind == "cut150":
        assert cen["exited"] - cen["counted_below_z"] > 100
        d = config(orc, "default")
        assert cen["exited"] == H.census_np(endstates(orc, "default", n), d.exit_port_z)["exited"]
    if kind == "brdf":
        assert cen["exited"] - cen["counted_below_z"] > 1000
    # a unit direction never falls outside [-1, 1): only v.z == 1.0 would, and such a ray does not leave downwards
    assert H.order_hist_np(es, c.exit_port_z, 512, 8)[2]["dz_outside"] == 0


def test_dz_bin_on_hand_made_states():
    """the dz word: floor((v.z + 1) / 2 * n_dz), v.z == 1.0 and NaN outside, nothing for the other classes or an overflowing ray"""
    st = np.array([1, 1, 1, 1, 1, 2, 3, 1], dtype=np.int32)
    npts = np.array([2, 3, 4, 5, 6, 3, 4, 50], dtype=np.int32)          # k = 0, 1, 2, 3, 4 | 2 | 3 | 48
    lp = np.zeros((8, 3)); lp[:, 2] = -300.0; lp[4, 2] = 10.0             # ray 4 leaves above the cut: class 1
    d = np.zeros((8, 3)); d[:, 2] = [-1.0, -0.5, 1.0, float("nan"), -0.2, 0.0, 0.0, -0.9]
    hist, dz, cnt = H.order_hist_np((st, npts, lp, d), -100.0, 8, 4)
    assert hist[0].tolist() == [1, 1, 1, 1, 0, 0, 0, 0] and hist[1].tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    assert hist[2].tolist() == [0, 0, 1, 0, 0, 0, 0, 0] and hist[3].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert cnt == {"overflow": [1, 0, 0, 0], "dz_outside": 2}
    assert dz[0].tolist() == [1, 0, 0, 0] and dz[1].tolist() == [0, 1, 0, 0] and int(dz.sum()) == 2


@pytest.mark.parametrize("kind", ["default", "chord", "port160", "limit6"])
def test_pencil_source_orders_add_up_to_wall_hits(orc, kind):
    """sum of k * hist == stats.wall_hits of the oracle's own census (pencil source, no overflow)"""
    c = config(orc, kind)
    n = 20_000
    hist, _, cnt = H.order_hist_np(endstates(orc, kind, n), c.exit_port_z, 2048, 0)
    assert sum(cnt["overflow"]) == 0
    _, st = orc.fluxmap(c, n, SEED)
    assert int((hist.astype(np.int64) * np.arange(2048)[None, :]).sum()) == st.wall_hits > n
    assert int(hist[0].sum()) == st.counted_below_z and int(hist[2].sum()) == st.absorbed and int(hist[3].sum()) == st.suspended


# ------------------------------------------------------------------ the ABI without a device

def test_binding_structs_and_default_spec():
    import altair_raytracing_amd as isx
    assert C.sizeof(isx.OrderHistSpec) == 16 and C.sizeof(isx.OrderHistCounts) == 40
    cfg = isx.default_config()
    s = isx.default_order_hist_spec(cfg)
    assert s.struct_size == C.sizeof(isx.OrderHistSpec) and s.reserved0 == 0
    assert (s.n_orders, s.n_dz) == (512, 8)
    t = s.copy(); t.n_orders = 5
    assert s.n_orders == 512 and t.n_orders == 5
    assert (isx.abi.ORDER_HIST_MAX_ORDERS, isx.abi.ORDER_HIST_MAX_WORDS) == (2048, 8192)
    k = isx.OrderHistCounts()
    assert k.as_dict() == {"overflow": [0, 0, 0, 0], "dz_outside": 0}


def test_the_library_exports_what_the_header_declares():
    import altair_raytracing_amd as isx
    header = open(os.path.join(ROOT, "include", "isx.h")).read()
    names = ("isx_default_order_hist_spec", "isx_order_hist", "isx_order_hist_device", "isx_order_reweight")
    for name in names:
        assert name + "(" in header and name in isx.EXPORTS and hasattr(isx.load(), name)
    assert "#define ISX_ORDER_HIST_MAX_ORDERS 2048" in header and "#define ISX_ORDER_HIST_MAX_WORDS  8192" in header
    out = subprocess.run(["nm", "-D", "--defined-only", isx.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("isx_")}
    assert set(names) <= exported
    assert exported - set(isx.EXPORTS) <= {"isx_diag_read"}, exported - set(isx.EXPORTS)


def refused_specs(isx):
    """(a good spec, [(what, spec)] that isx.h refuses with ISX_ERR_BAD_CONFIG); (served: specs at the limits)"""
    good = isx.default_order_hist_spec(isx.default_config())
    bad = []
    for what, no, nz in (("n_orders 0", 0, 8), ("n_orders -1", -1, 0), ("n_orders 2049", 2049, 0), ("n_dz -1", 512, -1),
                         ("n_dz 65", 64, 65), ("10240 words", 2048, 1), ("8196 words", 683, 8), ("8256 words", 129, 60),
                         ("n_orders 2^30", 1 << 30, 4)):
        s = good.copy(); s.n_orders, s.n_dz = no, nz
        bad.append((what, s))
    for size in (0, 12, 20):
        s = good.copy(); s.struct_size = size
        bad.append(("struct_size %d" % size, s))
    served = []
    for no, nz in ((1, 0), (2048, 0), (128, 60), (1, 64), (682, 8), (512, 8)):
        s = good.copy(); s.n_orders, s.n_dz = no, nz
        served.append(s)
    return good, bad, served


def test_refused_specs_and_null_arguments_need_no_device():
    """A refused spec is ISX_ERR_BAD_CONFIG and a NULL cfg / spec / hist (or port_dz with n_dz > 0) ISX_ERR_BAD_ARG from both entry
    points, before anything asks for a device (this process never calls isx_init); a spec at the limits gets past the checks."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import ctypes as C
import numpy as np
import altair_raytracing_amd as isx
from test_order_hist_cpu import refused_specs
lib = isx.load()
have = lib.isx_init(0) == 0
if have:
    lib.isx_shutdown()
past = isx.abi.ERR_NOT_INIT if have else isx.abi.ERR_NO_DEVICE
cfg = isx.default_config()
buf = np.zeros(8192 + 8, dtype=np.uint64)
hp = buf.ctypes.data_as(C.POINTER(C.c_uint64))
good, bad, served = refused_specs(isx)
dev = C.c_void_p(4096)
for what, s in bad:
    assert lib.isx_order_hist(C.byref(cfg), C.byref(s), 10, 1, 0, hp, hp, None, None) == isx.abi.ERR_BAD_CONFIG, what
    assert lib.isx_order_hist_device(C.byref(cfg), C.byref(s), 10, 1, 0, dev, dev, dev) == isx.abi.ERR_BAD_CONFIG, what
for s in served:
    assert lib.isx_order_hist(C.byref(cfg), C.byref(s), 10, 1, 0, hp, hp, None, None) == past, (s.n_orders, s.n_dz)
    assert lib.isx_order_hist_device(C.byref(cfg), C.byref(s), 10, 1, 0, dev, dev, dev) == past, (s.n_orders, s.n_dz)
BAD_ARG = isx.abi.ERR_BAD_ARG
assert lib.isx_order_hist(None, C.byref(good), 10, 1, 0, hp, hp, None, None) == BAD_ARG
assert lib.isx_order_hist(C.byref(cfg), None, 10, 1, 0, hp, hp, None, None) == BAD_ARG
assert lib.isx_order_hist(C.byref(cfg), C.byref(good), 10, 1, 0, None, hp, None, None) == BAD_ARG
assert lib.isx_order_hist(C.byref(cfg), C.byref(good), 10, 1, 0, hp, None, None, None) == BAD_ARG       # n_dz = 8
assert lib.isx_order_hist_device(None, C.byref(good), 10, 1, 0, dev, dev, dev) == BAD_ARG
assert lib.isx_order_hist_device(C.byref(cfg), None, 10, 1, 0, dev, dev, dev) == BAD_ARG
assert lib.isx_order_hist_device(C.byref(cfg), C.byref(good), 10, 1, 0, None, dev, dev) == BAD_ARG
assert lib.isx_order_hist_device(C.byref(cfg), C.byref(good), 10, 1, 0, dev, None, dev) == BAD_ARG
assert lib.isx_order_hist_device(C.byref(cfg), C.byref(good), 10, 1, 0, dev, dev, None) == BAD_ARG
nodz = good.copy(); nodz.n_dz = 0                                                                       # port_dz may be NULL iff n_dz == 0
assert lib.isx_order_hist(C.byref(cfg), C.byref(nodz), 10, 1, 0, hp, None, None, None) == past
assert lib.isx_order_hist_device(C.byref(cfg), C.byref(nodz), 10, 1, 0, dev, None, dev) == past
wrong = cfg.copy(); wrong.struct_size += 8
assert lib.isx_order_hist(C.byref(wrong), C.byref(good), 10, 1, 0, hp, hp, None, None) == isx.abi.ERR_BAD_CONFIG
# the Python wrapper hands a refused spec to the library and raises its status
try:
    isx.order_hist(cfg, 10, 1, bad[0][1])
    print("no error")
except isx.IsxError as e:
    print("ok", e.status, len(bad))
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["ok", "-2", "12"], r.stdout


def test_entry_points_without_a_device():
    """Without a HIP device both entry points answer ISX_ERR_NO_DEVICE (there is no CPU path); where a device is present, a
    process that never called isx_init() gets ISX_ERR_NOT_INIT from both -- the status of isx_light_field in the same process."""
    code = r"""
import sys
sys.path.insert(0, %r)
import altair_raytracing_amd as isx
lib = isx.load()
have = lib.isx_init(0) == 0
if have:
    lib.isx_shutdown()
cfg = isx.default_config()
spec = isx.default_order_hist_spec(cfg)
got = []
for call in (lambda: isx.order_hist(cfg, 10, 1), lambda: isx.order_hist_device(cfg, spec, 10, 1, 0, 4096, 8192, 12288),
             lambda: isx.light_field(cfg, 10, 1)):
    try:
        call()
        got.append(0)
    except isx.IsxError as e:
        got.append(e.status)
print("have" if have else "none", *got)
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    have, a, b, field = r.stdout.split()
    import altair_raytracing_amd as isx
    want = isx.abi.ERR_NOT_INIT if have == "have" else isx.abi.ERR_NO_DEVICE
    assert (int(a), int(b), int(field)) == (want, want, want), r.stdout


def test_no_device_on_a_machine_without_one():
    """where no HIP device can be initialised, a valid call is ISX_ERR_NO_DEVICE"""
    import altair_raytracing_amd as isx
    import torch
    if torch.cuda.is_available():
        return   # (test_entry_points_without_a_device covers the machine with a device)
    with pytest.raises(isx.IsxError) as e:
        isx.order_hist(isx.default_config(), 10, 1)
    assert e.value.status == isx.abi.ERR_NO_DEVICE


# ------------------------------------------------------------------ isx_order_reweight (host code)

def _counts(isx, overflow=(0, 0, 0, 0), dz_outside=0):
    k = isx.OrderHistCounts()
    for i, v in enumerate(overflow):
        k.overflow[i] = v
    k.dz_outside = dz_outside
    return k


def _oracle_hist(isx, orc, kind, n, n_orders, n_dz=0):
    c = config(orc, kind)
    hist, dz, cnt = H.order_hist_np(endstates(orc, kind, n), c.exit_port_z, n_orders, n_dz)
    spec = isx.default_order_hist_spec(isx.default_config())
    spec.n_orders, spec.n_dz = n_orders, n_dz
    return hist, _counts(isx, cnt["overflow"], cnt["dz_outside"]), spec


@pytest.mark.parametrize("kind,n_orders", [("default", 2048), ("default", 1024), ("rho09", 128), ("port160", 512), ("limit6", 8)])
def test_reweight_equals_numpy(orc, kind, n_orders):
    """rtol 1e-12: at most 2048 terms, each a few ulp from pow (and S2 - S1^2 / N loses nothing: S1^2 / N is far below S2)"""
    import altair_raytracing_amd as isx
    n = 20_000
    hist, cnt, spec = _oracle_hist(isx, orc, kind, n, n_orders)
    assert cnt.overflow[0] == 0 and int(hist[0].sum()) > 500
    cfg = config(isx, kind)
    rho = np.array([cfg.reflectance, 0.95 * cfg.reflectance, 0.9, 0.5, 0.0, 1e-3, min(1.0, cfg.reflectance * 1.005)])
    frac, sig = isx.order_reweight(cfg, spec, hist, cnt, n, rho)
    for i, r in enumerate(rho):
        f, s = H.reweight_np(hist[0], n, cfg.reflectance, r)
        assert frac[i] == pytest.approx(f, rel=1e-12, abs=0) and sig[i] == pytest.approx(s, rel=1e-12, abs=0), (kind, r)
    # rho = rho0: every weight is 1.0 exactly
    assert frac[0] == int(hist[0].sum()) / n
    p = int(hist[0].sum()) / n
    assert sig[0] == pytest.approx(np.sqrt(p * (1 - p) / n), rel=1e-12)
    # rho = 0: only the rays of order 0 are left (pow(0, 0) == 1)
    assert frac[4] == int(hist[0][0]) / n
    # fewer histories survive a darker wall
    assert frac[0] > frac[1] > frac[3] >= frac[4]
    # one value, a scalar; no value at all
    f1, s1 = isx.order_reweight(cfg, spec, hist, cnt, n, 0.9)
    assert (f1[0], s1[0]) == (frac[2], sig[2])
    f0, s0 = isx.order_reweight(cfg, spec, hist, cnt, n, np.zeros(0))
    assert f0.size == 0 and s0.size == 0


def test_reweight_refusals(orc):
    import altair_raytracing_amd as isx
    n = 20_000
    hist, cnt, spec = _oracle_hist(isx, orc, "default", n, 1024)
    cfg = isx.default_config()
    ok = lambda **kw: isx.order_reweight(kw.get("cfg", cfg), kw.get("spec", spec), hist, kw.get("cnt", cnt), kw.get("n", n), kw.get("rho", [0.9]))
    ok()

    def status(**kw):
        with pytest.raises(isx.IsxError) as e:
            ok(**kw)
        return e.value.status

    BAD_CONFIG, BAD_ARG = isx.abi.ERR_BAD_CONFIG, isx.abi.ERR_BAD_ARG
    brdf = isx.default_config(); brdf.source_model = 1
    assert status(cfg=brdf) == BAD_CONFIG                                   # the primary's interactions are not in k
    assert status(cnt=_counts(isx, (1, 0, 0, 0))) == BAD_CONFIG             # the tail is lost
    ok(cnt=_counts(isx, (0, 5, 7, 9), 3))                                   # (the other classes' tails do not matter)
    for r0 in (0.0, -0.5):
        dark = isx.default_config(); dark.reflectance = r0
        assert status(cfg=dark) == BAD_CONFIG
    assert status(n=0) == BAD_CONFIG
    bad_spec = spec.copy(); bad_spec.n_orders = 0
    assert status(spec=bad_spec) == BAD_CONFIG
    for r in (-0.1, float("nan"), float("inf")):
        assert status(rho=[0.9, r]) == BAD_ARG
    # rho > rho0 is accepted
    f, s = ok(rho=[1.0])
    assert f[0] > int(hist[0].sum()) / n and s[0] > 0
    # NULL arguments
    lib = isx.load()
    h = np.ascontiguousarray(hist.reshape(-1))
    hp = h.ctypes.data_as(C.POINTER(C.c_uint64))
    rho = (C.c_double * 1)(0.9); out = (C.c_double * 1)()
    assert lib.isx_order_reweight(C.byref(cfg), C.byref(spec), hp, C.byref(cnt), n, rho, 1, out, None) == 0     # sigma may be NULL
    assert lib.isx_order_reweight(None, C.byref(spec), hp, C.byref(cnt), n, rho, 1, out, out) == BAD_ARG
    assert lib.isx_order_reweight(C.byref(cfg), None, hp, C.byref(cnt), n, rho, 1, out, out) == BAD_ARG
    assert lib.isx_order_reweight(C.byref(cfg), C.byref(spec), None, C.byref(cnt), n, rho, 1, out, out) == BAD_ARG
    assert lib.isx_order_reweight(C.byref(cfg), C.byref(spec), hp, None, n, rho, 1, out, out) == BAD_ARG
    assert lib.isx_order_reweight(C.byref(cfg), C.byref(spec), hp, C.byref(cnt), n, None, 1, out, out) == BAD_ARG
    assert lib.isx_order_reweight(C.byref(cfg), C.byref(spec), hp, C.byref(cnt), n, rho, 1, None, out) == BAD_ARG
    assert lib.isx_order_reweight(C.byref(cfg), C.byref(spec), hp, C.byref(cnt), n, rho, -1, out, out) == BAD_ARG


def test_reweighted_oracle_rays_agree_with_a_direct_oracle_trace(orc):
    """The statistic of the GPU physics test on the reference itself, 2e5 rays: histories traced at rho0 = 0.99 (seed 7),
    reweighted to 0.95 and 0.90, against direct traces at those reflectances with another seed (11):
    |f_rw - f_direct| <= 5 sqrt(sigma_rw^2 + f (1 - f) / N)."""
    import altair_raytracing_amd as isx
    n = 200_000
    c = orc.default_config()
    assert c.reflectance == 0.99
    es = orc.trace_endstates(c, n, 7)
    hist, _, cnt = H.order_hist_np(es, c.exit_port_z, 2048, 0)
    assert cnt["overflow"][0] == 0
    spec = isx.default_order_hist_spec(isx.default_config()); spec.n_orders, spec.n_dz = 2048, 0
    for rho in (0.95, 0.90):
        f_rw, s_rw = (x[0] for x in isx.order_reweight(isx.default_config(), spec, hist, _counts(isx, cnt["overflow"]), n, rho))
        d = orc.default_config(); d.reflectance = rho
        _, st = orc.fluxmap(d, n, 11)
        f = st.counted_below_z / n
        z = (f_rw - f) / np.sqrt(s_rw ** 2 + f * (1 - f) / n)
        print("rho %.2f: reweighted %.6f +- %.6f, direct %.6f, z = %+.2f" % (rho, f_rw, s_rw, f, z))
        assert abs(z) <= 5


# ------------------------------------------------------------------ sharding

class _Counts:
    def __init__(self, d):
        self.overflow = list(d["overflow"]); self.dz_outside = d["dz_outside"]


def _oracle_order_hist(oracle, c, count, seed, spec, first):
    """The tracer a GPU box takes from altair_raytracing_amd.order_hist, made of the oracle + the restatement."""
    es = oracle.trace_endstates(c, count, seed, first)
    hist, dz, k = H.order_hist_of_spec(es, c, spec)
    st = oracle.Stats()
    for f, v in H.census_np(es, c.exit_port_z).items():
        setattr(st, f, v)
    st.bin_increments = int(hist.sum())
    st.wall_hits = int(H.classify(es, c.exit_port_z)[0].sum())
    return hist, dz, _Counts(k), st


def _spec(isx):
    s = isx.default_order_hist_spec(isx.default_config())
    s.n_orders, s.n_dz = 48, 5
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
    out = isx.order_hist_sharded(lambda c, count, seed, sp, first: _oracle_order_hist(oracle, c, count, seed, sp, first),
                                 cfg, _spec(isx), 6001, 77, first_ray=1000)
    q.put((rank,) + out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_order_hist_sharded_allreduce_equals_single_rank(orc, world):
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
    spec = _spec(isx)
    wh, wd, wk, wst = _oracle_order_hist(orc, cfg, 6001, 77, spec, 1000)
    want_counts = dict(zip(isx.sharding.ORDER_COUNT_FIELDS, wk.overflow + [wk.dz_outside]))
    assert wk.overflow[0] > 0 and wk.overflow[2] > 0 and wh[0].sum() > 500
    # one rank, no process group: the same function is the plain call
    sh, sd, sk, sc = isx.order_hist_sharded(lambda c, count, seed, s, first: _oracle_order_hist(orc, c, count, seed, s, first),
                                            cfg, spec, 6001, 77, first_ray=1000)
    assert np.array_equal(sh, wh) and np.array_equal(sd, wd) and sk == want_counts
    for rank, h, d, k, census in got:
        assert h.shape == (4, 48) and d.shape == (48, 5) and h.dtype == d.dtype == np.uint64
        assert np.array_equal(h, wh) and np.array_equal(d, wd), rank
        assert k == want_counts, rank
        assert census["launched"] == 6001 and census["counted_below_z"] == wst.counted_below_z
        assert census["bin_increments"] == int(wh.sum()) and census["wall_hits"] == wst.wall_hits
