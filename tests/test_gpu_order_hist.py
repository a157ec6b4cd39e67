"""isx_order_hist on the GPU: histograms, the port's dz array, the five counters and the census bit for bit against the oracle's
end states (tests/orderhist_np.py) -- every border model, source and trace mode: nothing is replayed, so the BRDF source is covered
too --, route, shape and partition invariance, the device form, the reweighted port fraction against direct traces, the host driver."""
import os
import subprocess
import sys

import numpy as np
import pytest

import orderhist_np as H
from test_order_hist_cpu import config, endstates

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


def _spec(isx, n_orders=512, n_dz=8):
    s = isx.default_order_hist_spec(isx.default_config())
    s.n_orders, s.n_dz = n_orders, n_dz
    return s


def _check_identities(res):
    hist, dz, k, st = res
    H.check_identities(hist, dz, k.as_dict(), st, dz.shape[1])
    assert st.bin_increments == int(hist.sum())


def _equal(a, b):
    """two results of order_hist: both arrays, the five counters, the census"""
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2].as_dict() == b[2].as_dict()
    for f in CENSUS + ("bin_increments",):
        assert getattr(a[3], f) == getattr(b[3], f), f


def _census_equals_fluxmap(isx, cfg, n, seed, st, first=0):
    _, fs = isx.fluxmap(cfg, n, seed, first)
    for f in CENSUS:
        assert getattr(st, f) == getattr(fs, f), f


def _equals_the_oracle(isx, orc, kind, n, spec):
    """one comparison: the oracle side first (returned for the caller's preconditions), then the library"""
    oc = config(orc, kind)
    es = endstates(orc, kind, n)
    oh, od, ok = H.order_hist_of_spec(es, oc, spec)
    ocen = H.census_np(es, oc.exit_port_z)
    cfg = config(isx, kind)
    hist, dz, k, st = isx.order_hist(cfg, n, SEED, spec)
    print(kind, (spec.n_orders, spec.n_dz), "oracle", [int(x.sum()) for x in oh], ok, "gpu", [int(x.sum()) for x in hist], k.as_dict())
    assert hist.shape == (4, spec.n_orders) and dz.shape == (spec.n_orders, spec.n_dz) and hist.dtype == dz.dtype == np.uint64
    assert k.as_dict() == ok, kind
    assert np.array_equal(hist, oh), kind
    assert np.array_equal(dz, od), kind
    for f, v in ocen.items():
        assert getattr(st, f) == v, f
    _check_identities((hist, dz, k, st))
    _census_equals_fluxmap(isx, cfg, n, SEED, st)
    return oh, od, ok, ocen, st


# ------------------------------------------------------------------ bit for bit against the oracle

@pytest.mark.parametrize("kind", ["default", "port160", "source2", "rho09", "chord", "lobe", "rough", "brdf", "brdf_chord",
                                  "rho1", "limit6", "cut150"])
def test_order_hist_equals_the_oracle(isx, orc, kind):
    _reset(isx)
    n = 40_000 if kind == "rho09" else 20_000
    spec = _spec(isx)
    oc = config(orc, kind)
    # the oracle side first: no comparison of empty branches
    oh, od, ok = H.order_hist_of_spec(endstates(orc, kind, n), oc, spec)
    assert int(oh[0].sum()) > 500 and int(od.sum()) == int(oh[0].sum()) and int((od.sum(axis=0) > 0).sum()) >= 3
    if kind == "rho1":
        assert int(oh[2].sum()) == 0 and ok["overflow"][0] > 0           # no absorbed rays; the port's tail overflows
    elif kind == "limit6":
        assert int(oh[3].sum()) > 10_000 and int(oh[3][oc.max_points]) == int(oh[3].sum())   # class 3, all of it at the limit
        assert int(oh[2].sum()) > 500
    else:
        assert int(oh[2].sum()) > 1000
    if kind in ("cut150", "brdf", "brdf_chord"):
        assert int(oh[1].sum()) > 100                                     # class 1
    *_, st = _equals_the_oracle(isx, orc, kind, n, spec)
    if oc.source_model == 0 and sum(ok["overflow"]) == 0:                 # pencil source, nothing lost: the orders are the wall hits
        assert int((oh.astype(np.int64) * np.arange(spec.n_orders)[None, :]).sum()) == st.wall_hits


EDGE_SPECS = [(1, 0), (40, 8), (2048, 0), (128, 60), (64, 1)]


@pytest.mark.parametrize("n_orders,n_dz", EDGE_SPECS, ids=["%dx%d" % s for s in EDGE_SPECS])
@pytest.mark.parametrize("kind", ["default", "brdf"])
def test_edge_specs(isx, orc, kind, n_orders, n_dz):
    _reset(isx)
    n = 20_000
    spec = _spec(isx, n_orders, n_dz)
    oh, od, ok = H.order_hist_of_spec(endstates(orc, kind, n), config(orc, kind), spec)
    if n_orders == 1:      # everything but k = 0 overflows
        assert sum(ok["overflow"]) + int(oh[:, 0].sum()) == n and sum(ok["overflow"]) > n // 2
        if kind == "brdf":   # (a pencil ray never ends without an interaction; a scattered one does: the one word is in use)
            assert int(oh[0, 0]) > 1000 and int(oh[1, 0]) > 100
    if n_orders == 40:
        assert ok["overflow"][0] > 0 and ok["overflow"][2] > 0 and int(oh[0].sum()) > 0 and int(oh[2].sum()) > 0
    if n_orders == 2048:
        assert sum(ok["overflow"]) == 0
    if (n_orders, n_dz) == (128, 60):
        assert 4 * n_orders + n_orders * n_dz == isx.abi.ORDER_HIST_MAX_WORDS and int(od.sum()) > 1000
        assert int((od.sum(axis=0) > 0).sum()) > 10 and int(od[n_orders - 1].sum()) > 0    # many dz words; the array's last row
    if n_dz == 1:
        assert np.array_equal(od[:, 0], oh[0]) and int(od.sum()) > 1000
    _equals_the_oracle(isx, orc, kind, n, spec)


def test_offset_first_ray_and_no_rays(isx, orc):
    _reset(isx)
    spec = _spec(isx, 300, 4)
    oc = orc.default_config()
    es = endstates(orc, "default", 20_000, SEED, 123_456_789_012)
    oh, od, ok = H.order_hist_of_spec(es, oc, spec)
    assert ok["overflow"][0] + ok["overflow"][2] > 0
    hist, dz, k, st = isx.order_hist(isx.default_config(), 20_000, SEED, spec, first_ray=123_456_789_012)
    assert np.array_equal(hist, oh) and np.array_equal(dz, od) and k.as_dict() == ok
    hist, dz, k, st = isx.order_hist(isx.default_config(), 0, SEED, spec)
    assert int(hist.sum()) == 0 and int(dz.sum()) == 0 and k.as_dict() == {"overflow": [0] * 4, "dz_outside": 0} and st.launched == 0


def test_hit_line_mode_and_grid_are_ignored(isx):
    _reset(isx)
    spec = _spec(isx, 256, 8)
    base = isx.order_hist(isx.default_config(), 100_000, SEED, spec)
    c = isx.default_config(); c.hit_line_mode = 1; c.n_theta = 7; c.n_phi = 3; c.det_diameter = 1.0
    _equal(isx.order_hist(c, 100_000, SEED, spec), base)


# ------------------------------------------------------------------ routes and shapes

ROUTES = [{"assist": 0}, {"pipeline": 0}, {"surface_pipeline": 0}, {"assist_block": 128}, {"assist_block": 512}, {"assist_block": 768},
          {"rays_per_lane": 1}, {"rays_per_lane": 4}, {"ray_sub": 32}]


@pytest.mark.parametrize("kind", ["default", "chord", "brdf", "brdf_chord", "lobe", "rough", "cut150"])
def test_route_and_shape_invariance(isx, kind):
    _reset(isx)
    cfg, n = config(isx, kind), 200_000
    spec = _spec(isx, 300, 8)                     # (the tail overflows: the counters take part)
    base = isx.order_hist(cfg, n, SEED, spec)
    _check_identities(base)
    _census_equals_fluxmap(isx, cfg, n, SEED, base[3])
    assert int(base[0][0].sum()) > 10_000 and int(base[0][2].sum()) > 5_000 and sum(base[2].overflow) > 0
    try:
        for opts in ROUTES:
            _reset(isx)
            for key, v in opts.items():
                isx.set_option(key, v)
            _equal(isx.order_hist(cfg, n, SEED, spec), base)
    finally:
        _reset(isx)


# ------------------------------------------------------------------ partitions, the device form

def test_partition_invariance(isx):
    """one 2e6-ray call (the default 768-thread shape) == 8 calls of 2.5e5 with offset first_ray"""
    _reset(isx)
    cfg, n = isx.default_config(), 2_000_000
    spec = _spec(isx)
    whole = isx.order_hist(cfg, n, SEED, spec)
    _check_identities(whole)
    _census_equals_fluxmap(isx, cfg, n, SEED, whole[3])
    parts = [isx.order_hist(cfg, n // 8, SEED, spec, first_ray=i * (n // 8)) for i in range(8)]
    assert np.array_equal(sum(p[0] for p in parts), whole[0]) and np.array_equal(sum(p[1] for p in parts), whole[1])
    assert [sum(p[2].overflow[c] for p in parts) for c in range(4)] == list(whole[2].overflow)
    assert sum(p[2].dz_outside for p in parts) == whole[2].dz_outside
    for f in CENSUS + ("bin_increments",):
        assert sum(getattr(p[3], f) for p in parts) == getattr(whole[3], f), f
    assert whole[2].overflow[0] > 0 and whole[2].overflow[2] > 0


def test_device_form_accumulates_and_leaves_foreign_words_alone():
    """isx_order_hist_device twice into caller-owned tensors == the blocking call over both ranges; the words around the three
    arrays keep their pattern (a process of its own: torch owns the tensors, the library's stream does the work)."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import altair_raytracing_amd as isx
isx.load(); isx.init(0)
cfg = isx.default_config()
spec = isx.default_order_hist_spec(cfg)
spec.n_orders, spec.n_dz = 200, 6
n, SEED, PAD, MARK = 300000, 7, 64, 0x5A5A5A5A5A5A5A5A
nh, nd = 4 * spec.n_orders, spec.n_orders * spec.n_dz
buf = torch.full((PAD + nh + PAD + nd + PAD + 5 + PAD,), MARK, dtype=torch.int64, device="cuda:0")
o_h, o_d, o_c = PAD, PAD + nh + PAD, PAD + nh + PAD + nd + PAD
buf[o_h:o_h + nh] = 0; buf[o_d:o_d + nd] = 0; buf[o_c:o_c + 5] = 0
torch.cuda.synchronize()
base = buf.data_ptr()
for i in range(2):
    isx.order_hist_device(cfg, spec, n // 2, SEED, i * (n // 2), base + 8 * o_h, base + 8 * o_d, base + 8 * o_c)
isx.sync()
st = isx.take_stats()
whole = isx.order_hist(cfg, n, SEED, spec)
torch.cuda.synchronize()
got = buf.cpu().numpy()
assert np.array_equal(got[o_h:o_h + nh].astype(np.uint64).reshape(4, -1), whole[0])
assert np.array_equal(got[o_d:o_d + nd].astype(np.uint64).reshape(spec.n_orders, -1), whole[1])
assert got[o_c:o_c + 5].tolist() == list(whole[2].overflow) + [whole[2].dz_outside]
keep = np.ones(got.size, bool)
for o, m in ((o_h, nh), (o_d, nd), (o_c, 5)):
    keep[o:o + m] = False
assert (got[keep] == MARK).all() and int(keep.sum()) == 4 * PAD
for f in ("launched", "exited", "counted_below_z", "absorbed", "suspended", "wall_hits", "bin_increments"):
    assert getattr(st, f) == getattr(whole[3], f), f
assert whole[2].overflow[0] > 0 and whole[2].overflow[2] > 0 and int(whole[1].sum()) > 50000
# n_dz = 0: no port_dz pointer is needed, none is written through
spec0 = spec.copy(); spec0.n_dz = 0
buf[o_h:o_h + nh] = 0; buf[o_c:o_c + 5] = 0
torch.cuda.synchronize()
isx.order_hist_device(cfg, spec0, n, SEED, 0, base + 8 * o_h, 0, base + 8 * o_c)
isx.sync(); isx.take_stats()
torch.cuda.synchronize()
got0 = buf.cpu().numpy()
assert np.array_equal(got0[o_h:o_h + nh].astype(np.uint64).reshape(4, -1), whole[0]) and np.array_equal(got0[o_d:o_d + nd], got[o_d:o_d + nd])
assert got0[o_c + 4] == 0 and (got0[keep] == MARK).all()
# a missing pointer is refused before anything is enqueued
for args in ((0, base, base), (base, 0, base), (base, base, 0)):
    try:
        isx.order_hist_device(cfg, spec, 10, SEED, 0, *args)
        raise SystemExit("a NULL pointer was accepted")
    except isx.IsxError as e:
        assert e.status == isx.abi.ERR_BAD_ARG
isx.shutdown()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]


# ------------------------------------------------------------------ physics

def test_reweighted_port_fraction_agrees_with_direct_traces(isx):
    """2e6 rays at rho0 = 0.99 (seed 7), n_orders 2048, reweighted to 0.95 and 0.90, against direct traces at those reflectances
    with seed 11 and the same ray count: |f_rw - f_direct| <= 5 sqrt(sigma_rw^2 + f (1 - f) / N).  The same statistic on the oracle
    alone at 2e5 rays (tests/test_order_hist_cpu.py) gives z = +1.39 and -0.12."""
    _reset(isx)
    n = 2_000_000
    cfg = isx.default_config()
    assert cfg.reflectance == 0.99
    spec = _spec(isx, 2048, 0)
    hist, _, k, st = isx.order_hist(cfg, n, 7, spec)
    assert k.overflow[0] == 0 and st.launched == n
    frac, sig = isx.order_reweight(cfg, spec, hist, k, st.launched, [0.99, 0.95, 0.90])
    assert frac[0] == st.counted_below_z / n
    for i, rho in ((1, 0.95), (2, 0.90)):
        d = isx.default_config(); d.reflectance = rho
        _, ds = isx.fluxmap(d, n, 11)
        f = ds.counted_below_z / n
        z = (frac[i] - f) / np.sqrt(sig[i] ** 2 + f * (1 - f) / n)
        print("rho %.2f: reweighted %.6f +- %.6f, direct %.6f, z = %+.2f" % (rho, frac[i], sig[i], f, z))
        assert abs(frac[i] - f) <= 5 * np.sqrt(sig[i] ** 2 + f * (1 - f) / n)


def test_single_kernel_time_is_reported(isx):
    _reset(isx)
    isx.order_hist(isx.default_config(), 2_000_000, SEED)
    single, trace, binning = isx.last_kernel_ms()
    assert single > 0 and trace == 0 and binning == 0


# ------------------------------------------------------------------ host driver, sharding

def test_host_driver_order_hist(isx, orc, tmp_path):
    """isx_macro orderHist: the CSV's rows == order_hist with the same configuration, seed and ray range; the footer == the counters;
    order_reweight.csv == order_reweight.  1024 orders x (4 + 4 dz) words is the whole LDS block (ISX_ORDER_HIST_MAX_WORDS)."""
    _reset(isx)
    assert 4 * 1024 + 1024 * 4 == isx.abi.ORDER_HIST_MAX_WORDS
    # the oracle side first: with the driver's default seed no port ray reaches order 1024, so the reweighting is not refused
    k_o, cl_o = H.classify(endstates(orc, "default", 200_000, 0x5EED0001), orc.default_config().exit_port_z)
    assert 512 < int(k_o[cl_o == 0].max()) < 1024
    env = dict(os.environ, ISX_QUIET="1")
    env.pop("ISX_RAYS", None); env.pop("ISX_SEED", None)
    r = subprocess.run([CLI, "orderHist", "--rays", "200000", "--orders", "1024", "--dz", "4", "--reflectances", "0.99,0.95,0.9"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    found = {f: os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs if f.startswith("order_") and f.endswith(".csv")}
    assert sorted(found) == ["order_hist.csv", "order_reweight.csv"], found
    lines = open(found["order_hist.csv"]).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    seed = int([l for l in head if l.startswith("# Seed:")][0].split(":")[1])
    body = [l for l in lines if not l.startswith("#")]
    assert body[0] == "k,port,exited_other,absorbed,suspended,dz_0,dz_1,dz_2,dz_3" and len(body) == 1 + 1024
    rows = np.array([[int(x) for x in l.split(",")] for l in body[1:]], dtype=np.uint64)
    spec = _spec(isx, 1024, 4)
    hist, dz, k, st = isx.order_hist(isx.default_config(), 200_000, seed, spec, 0)
    assert np.array_equal(rows[:, 0], np.arange(1024, dtype=np.uint64))
    assert np.array_equal(rows[:, 1:5].T, hist) and np.array_equal(rows[:, 5:], dz) and int(hist[0].sum()) > 50_000
    foot = {l[2:].split(":")[0]: l.split(":")[1].strip() for l in head if ":" in l}
    assert [int(foot[f]) for f in ("Overflow port", "Overflow exited other", "Overflow absorbed", "Overflow suspended", "dz outside")] == \
           list(k.overflow) + [k.dz_outside]
    assert int(foot["Launched"]) == st.launched == 200_000 and seed == 0x5EED0001
    rw = [l for l in open(found["order_reweight.csv"]).read().splitlines() if not l.startswith("#")]
    assert rw[0] == "rho,fraction,sigma" and len(rw) == 4
    frac, sig = isx.order_reweight(isx.default_config(), spec, hist, k, st.launched, [0.99, 0.95, 0.9])
    for i, l in enumerate(rw[1:]):
        rho, f, s = (float(x) for x in l.split(","))
        assert (rho, f, s) == ([0.99, 0.95, 0.9][i], frac[i], sig[i])
    # without --reflectances only the histogram is written; a refused spec is an error of the entry point
    plain = tmp_path / "plain"
    plain.mkdir()
    r = subprocess.run([CLI, "orderHist", "--rays", "50000", "--orders", "64", "--dz", "0"], cwd=plain, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert [f for _, _, fs in os.walk(plain) for f in fs] == ["order_hist.csv"]
    r = subprocess.run([CLI, "orderHist", "--rays", "50000", "--orders", "4096"], cwd=plain, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "isx_order_hist" in r.stderr + r.stdout


def test_order_hist_sharded_one_rank_equals_order_hist(isx):
    _reset(isx)
    cfg, spec = isx.default_config(), _spec(isx, 100, 3)
    hist, dz, k, st = isx.order_hist(cfg, 300_000, SEED, spec)
    sh, sd, sk, sc = isx.order_hist_sharded(isx.order_hist, cfg, spec, 300_000, SEED)
    assert np.array_equal(sh, hist) and np.array_equal(sd, dz)
    assert list(sk.values()) == list(k.overflow) + [k.dz_outside] and sum(sk.values()) > 0
    for f in CENSUS + ("bin_increments",):
        assert sc[f] == getattr(st, f), f
