"""Call overlap ("call_overlap"): an enqueued flux map (isx_fluxmap_device) puts its fate scan and trace kernel
on a trace stream and only its binning kernel on isx_stream(), so that the next call's scan and trace run under this call's launch
tails.  A scheduling option: every histogram and every census of an enqueued sequence is that of blocking isx_fluxmap calls of the
same (n, seed, first), and the oracle's.

The sequences need torch (device memory, and a zeroing enqueued on isx_stream() through torch.cuda.ExternalStream as bench.py
does), and torch's HIP runtime has to come up before libisx's: ONE child process runs them all and leaves what it read back in an
.npz; the tests compare.  The seven calls of a sequence walk over FOUR ray ranges (call s takes range s mod 4) while the library
rotates over three workspaces (s mod 3): two calls that share a workspace never share a range, and the oracle runs four times."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0001
CENSUS = ("launched", "exited", "counted_below_z", "absorbed", "suspended", "bin_increments", "wall_hits")
N = 300_000
PARTS = [(i * N, N) for i in range(4)]                      # (first, n)
SEVEN = [s % 4 for s in range(7)]                           # call s of a sequence -> its range
SMALL = [(7, 1), (7, 63), (7, 64), (7, 65)]
CHUNKED = [(2 * N - 60_000, 60_000), PARTS[2], (3 * N, 50_000)]   # one chunk, five chunks of 65 536, one chunk

WORKER = r"""
import sys, traceback, numpy as np, torch
sys.path.insert(0, %(root)r)
torch.cuda.init(); torch.zeros(1, device="cuda:0")
import altair_raytracing_amd as isx
isx.load(); isx.init(0)
SEED, N = %(seed)d, %(n)d
PARTS, SEVEN, SMALL, CHUNKED = %(parts)r, %(seven)r, %(small)r, %(chunked)r
F = %(census)r
c = isx.default_config()
nb = c.n_theta * c.n_phi
ext = torch.cuda.ExternalStream(isx.load().isx_stream(), device="cuda:0")
res = {}

def cen(st):
    return np.array([int(getattr(st, f)) for f in F], dtype=np.uint64)

def dev(rows):
    t = torch.zeros((rows, nb), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    return t

def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().astype(np.uint64)

def options(**kw):
    o = dict(fate_scan=1, call_overlap=1, call_overlap_streams=2, overlap=0, pipeline_chunk=1 << 26)
    o.update(kw)
    for k, v in o.items():
        isx.set_option(k, v)

def blocking(key, cfg, parts):
    for i, (first, n) in enumerate(parts):
        h, st = isx.fluxmap(cfg, n, SEED, first)
        res["%%s_h%%d" %% (key, i)] = h.reshape(-1)
        res["%%s_c%%d" %% (key, i)] = cen(st)

def scenario(fn):
    try:
        options()
        isx.take_stats()
        fn()
        res["ok_" + fn.__name__] = np.array([1])
    except Exception:
        res["err_" + fn.__name__] = np.array(traceback.format_exc())
        try:
            isx.take_stats()
        except Exception:
            pass

def seven_hists(key, **kw):
    options(**kw)
    d = dev(7)
    k0 = isx.fate_scan_launches()
    for s, r in enumerate(SEVEN):
        isx.fluxmap_device(c, PARTS[r][1], SEED, PARTS[r][0], d[s].data_ptr())
    st = isx.take_stats()
    res[key + "_scans"] = np.array([isx.fate_scan_launches() - k0])
    res[key + "_h"], res[key + "_c"] = host(d), cen(st)

def refs():
    blocking("blk", c, PARTS)
    blocking("small", c, SMALL)
    options(pipeline_chunk=65536)
    blocking("chunk", c, CHUNKED)

def seven_on(): seven_hists("seven_on", call_overlap=1)
def seven_off(): seven_hists("seven_off", call_overlap=0)
def seven_one_stream(): seven_hists("seven_one", call_overlap=1, call_overlap_streams=1)

def one_hist():
    for key, zero in (("one_zeroed", True), ("one_summed", False)):
        d = dev(1)
        for r in SEVEN:
            if zero:
                with torch.cuda.stream(ext):
                    d.zero_()
            isx.fluxmap_device(c, PARTS[r][1], SEED, PARTS[r][0], d.data_ptr())
        st = isx.take_stats()
        res[key + "_h"], res[key + "_c"] = host(d), cen(st)

def five_chunks():
    options(pipeline_chunk=65536)
    d = dev(3)
    k0 = isx.fate_scan_launches()
    for i, (first, n) in enumerate(CHUNKED):
        isx.fluxmap_device(c, n, SEED, first, d[i].data_ptr())
    st = isx.take_stats()
    res["chunks_scans"] = np.array([isx.fate_scan_launches() - k0])
    res["chunks_h"], res["chunks_c"] = host(d), cen(st)

def mixed_sizes():
    seq = [("blk", 0), ("small", 0), ("blk", 1), ("small", 1), ("blk", 2), ("small", 2), ("small", 3), ("blk", 3)]
    parts = {"blk": PARTS, "small": SMALL}
    d = dev(len(seq))
    for i, (kind, j) in enumerate(seq):
        first, n = parts[kind][j]
        isx.fluxmap_device(c, n, SEED, first, d[i].data_ptr())
    st = isx.take_stats()
    res["mixed_h"], res["mixed_c"] = host(d), cen(st)
    # reflectance 0 (every ray settled by the scan: the list is empty) between two ordinary calls
    c0 = isx.default_config(); c0.reflectance = 0.0
    h, s = isx.fluxmap(c0, N, SEED, 0)
    res["rho0_blk_h"], res["rho0_blk_c"] = h.reshape(-1), cen(s)
    d = dev(3)
    for i, (cfg, r) in enumerate(((c, 0), (c0, 0), (c, 1))):
        isx.fluxmap_device(cfg, PARTS[r][1], SEED, PARTS[r][0], d[i].data_ptr())
    st = isx.take_stats()
    res["rho0_h"], res["rho0_c"] = host(d), cen(st)
    # without the scan: the plain trace kernel on the trace stream
    options(fate_scan=0)
    d = dev(4)
    k0 = isx.fate_scan_launches()
    for s in range(4):
        isx.fluxmap_device(c, PARTS[s][1], SEED, PARTS[s][0], d[s].data_ptr())
    st = isx.take_stats()
    res["noscan_scans"] = np.array([isx.fate_scan_launches() - k0])
    res["noscan_h"], res["noscan_c"] = host(d), cen(st)

def other_routes():
    beam = isx.beam_cone(c, (-60.0, 0.0, -75.0), (1.0, 0.0, 0.0), 2.0, 5.0)
    # (detector discs 200 cm from the origin, every 5 degrees on both sides, their axes towards the port)
    th = np.radians(np.arange(-45.0, 45.0 + 1e-9, 5.0))
    x, z = 200 * np.sin(th), -200 * np.cos(th)
    rot = -np.arctan2(np.abs(x), -100 - z)
    discs = np.concatenate([np.stack([s * x, 0 * x, z, np.sin(rot), 0 * x, np.cos(rot)], axis=1) for s in (1.0, -1.0)])
    bh, bs = isx.fluxmap_beam(c, beam, 150_000, SEED, 0)
    dh, ds = isx.disc_sweep(c, discs, 5.0, 0.1, 100_000, SEED)
    res["beam_alone_h"], res["beam_alone_c"] = bh.reshape(-1), cen(bs)
    res["disc_alone_h"], res["disc_alone_c"] = dh.reshape(-1), cen(ds)
    d = dev(6)
    isx.fluxmap_device(c, PARTS[0][1], SEED, PARTS[0][0], d[0].data_ptr())
    isx.fluxmap_device(c, PARTS[1][1], SEED, PARTS[1][0], d[1].data_ptr())
    bh, bs = isx.fluxmap_beam(c, beam, 150_000, SEED, 0)        # (a blocking call drops the census enqueued before it)
    isx.fluxmap_device(c, PARTS[2][1], SEED, PARTS[2][0], d[2].data_ptr())
    isx.fluxmap_device(c, PARTS[3][1], SEED, PARTS[3][0], d[3].data_ptr())
    dh, ds = isx.disc_sweep(c, discs, 5.0, 0.1, 100_000, SEED)
    isx.fluxmap_device(c, PARTS[0][1], SEED, PARTS[0][0], d[4].data_ptr())
    isx.fluxmap_device(c, PARTS[1][1], SEED, PARTS[1][0], d[5].data_ptr())
    st = isx.take_stats()
    res["beam_mid_h"], res["beam_mid_c"] = bh.reshape(-1), cen(bs)
    res["disc_mid_h"], res["disc_mid_c"] = dh.reshape(-1), cen(ds)
    res["routes_h"], res["routes_c"] = host(d), cen(st)

def lifecycle():
    d = dev(4)
    isx.fluxmap_device(c, PARTS[0][1], SEED, PARTS[0][0], d[0].data_ptr())
    isx.set_option("call_overlap", 1)
    isx.fluxmap_device(c, PARTS[1][1], SEED, PARTS[1][0], d[1].data_ptr())
    isx.sync()
    res["life_after_sync_h"] = d[:2].cpu().numpy().astype(np.uint64)     # (isx_sync alone has completed both)
    isx.fluxmap_device(c, PARTS[2][1], SEED, PARTS[2][0], d[2].data_ptr())
    isx.set_option("fate_scan", 0)
    isx.fluxmap_device(c, PARTS[3][1], SEED, PARTS[3][0], d[3].data_ptr())
    st = isx.take_stats()
    res["life_h"], res["life_c"] = host(d), cen(st)
    # shutdown with a sequence in flight and no take_stats; then a fresh library
    options()
    d = dev(4)
    for s in range(3):
        isx.fluxmap_device(c, PARTS[s][1], SEED, PARTS[s][0], d[s].data_ptr())
    isx.shutdown()
    res["shutdown_h"] = d[:3].cpu().numpy().astype(np.uint64)
    isx.init(0)
    options()
    isx.fluxmap_device(c, PARTS[3][1], SEED, PARTS[3][0], d[3].data_ptr())
    st = isx.take_stats()
    res["reinit_h"], res["reinit_c"] = host(d)[3], cen(st)

def not_eligible():
    cc = isx.default_config(); cc.trace_mode = 1
    for key, cfg, kw in (("chord", cc, {}), ("overlap2", c, {"overlap": 2})):
        for co in (0, 1):
            options(call_overlap=co, **kw)
            d = dev(3)
            for s in range(3):
                isx.fluxmap_device(cfg, PARTS[s][1], SEED, PARTS[s][0], d[s].data_ptr())
            st = isx.take_stats()
            res["%%s_%%d_h" %% (key, co)], res["%%s_%%d_c" %% (key, co)] = host(d), cen(st)
        options(call_overlap=0, **kw)
        blocking(key + "_blk", cfg, PARTS[:3])

for fn in (refs, seven_on, seven_off, seven_one_stream, one_hist, five_chunks, mixed_sizes, other_routes, lifecycle, not_eligible):
    scenario(fn)
isx.shutdown()
np.savez(sys.argv[1], **res)
print("ok")
"""


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("call_overlap") / "res.npz")
    code = WORKER % dict(root=ROOT, seed=SEED, n=N, parts=PARTS, seven=SEVEN, small=SMALL, chunked=CHUNKED, census=CENSUS)
    r = subprocess.run([sys.executable, "-c", code, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
    return dict(np.load(out))


@pytest.fixture(scope="module")
def ora(orc):
    """oracle (histogram, census) of a range of the default configuration (reflectance given), computed once per range"""
    cache = {}

    def get(first, n, reflectance=None, trace_mode=0):
        key = (first, n, reflectance, trace_mode)
        if key not in cache:
            c = orc.default_config()
            if reflectance is not None:
                c.reflectance = reflectance
            c.trace_mode = trace_mode
            h, st = orc.fluxmap(c, n, SEED, first)
            cache[key] = (h.reshape(-1), np.array([int(getattr(st, f)) for f in CENSUS], dtype=np.uint64))
        return cache[key]
    return get


def _ok(run, name):
    assert "err_" + name not in run, str(run["err_" + name])
    assert "ok_" + name in run


def _blk(run, key, i):
    return run["%s_h%d" % (key, i)], run["%s_c%d" % (key, i)]


def _sum_c(cs):
    return np.sum(np.stack(cs), axis=0, dtype=np.uint64)


REFS = [("blk", i, p) for i, p in enumerate(PARTS)] + [("small", i, p) for i, p in enumerate(SMALL)] + \
       [("chunk", i, p) for i, p in enumerate(CHUNKED)]


@pytest.mark.parametrize("key,i,part", REFS, ids=["%s%d" % (k, i) for k, i, _ in REFS])
def test_blocking_references_are_the_oracles(run, ora, key, i, part):
    """what every sequence below is held against: the blocking calls equal the oracle, range by range"""
    _ok(run, "refs")
    h, c = _blk(run, key, i)
    oh, oc = ora(*part)
    assert np.array_equal(h, oh), (key, i)
    assert np.array_equal(c, oc), (key, i, c, oc)


@pytest.mark.parametrize("key", ["seven_on", "seven_off", "seven_one"])
def test_seven_calls_into_seven_histograms(run, key):
    """more calls in flight than workspaces; with the option on (two trace streams, the default, and one) and off"""
    _ok(run, {"seven_one": "seven_one_stream"}.get(key, key))
    assert int(run[key + "_scans"][0]) == 7
    for s, r in enumerate(SEVEN):
        assert np.array_equal(run[key + "_h"][s], _blk(run, "blk", r)[0]), (key, s)
    assert np.array_equal(run[key + "_c"], _sum_c([_blk(run, "blk", r)[1] for r in SEVEN]))


def test_seven_calls_into_one_histogram_zeroed_on_the_stream_in_between(run):
    _ok(run, "one_hist")
    assert np.array_equal(run["one_zeroed_h"][0], _blk(run, "blk", SEVEN[-1])[0])
    assert np.array_equal(run["one_zeroed_c"], _sum_c([_blk(run, "blk", r)[1] for r in SEVEN]))


def test_seven_calls_into_one_histogram_sum(run):
    _ok(run, "one_hist")
    want = np.sum(np.stack([_blk(run, "blk", r)[0] for r in SEVEN]), axis=0, dtype=np.uint64)
    assert np.array_equal(run["one_summed_h"][0], want)
    assert np.array_equal(run["one_summed_c"], _sum_c([_blk(run, "blk", r)[1] for r in SEVEN]))


def test_five_chunks_between_two_single_chunk_calls(run):
    _ok(run, "five_chunks")
    assert int(run["chunks_scans"][0]) == 7
    for i in range(3):
        assert np.array_equal(run["chunks_h"][i], _blk(run, "chunk", i)[0]), i
    assert np.array_equal(run["chunks_c"], _sum_c([_blk(run, "chunk", i)[1] for i in range(3)]))


def test_mixed_call_sizes(run, ora):
    _ok(run, "mixed_sizes")
    seq = [("blk", 0), ("small", 0), ("blk", 1), ("small", 1), ("blk", 2), ("small", 2), ("small", 3), ("blk", 3)]
    for i, (kind, j) in enumerate(seq):
        assert np.array_equal(run["mixed_h"][i], _blk(run, kind, j)[0]), (i, kind, j)
    assert np.array_equal(run["mixed_c"], _sum_c([_blk(run, kind, j)[1] for kind, j in seq]))
    # reflectance 0
    oh, oc = ora(0, N, reflectance=0.0)
    assert np.array_equal(run["rho0_blk_h"], oh) and np.array_equal(run["rho0_blk_c"], oc)
    assert int(oc[CENSUS.index("absorbed")]) == N
    for i, want in enumerate((_blk(run, "blk", 0)[0], run["rho0_blk_h"], _blk(run, "blk", 1)[0])):
        assert np.array_equal(run["rho0_h"][i], want), i
    assert np.array_equal(run["rho0_c"], _sum_c([_blk(run, "blk", 0)[1], run["rho0_blk_c"], _blk(run, "blk", 1)[1]]))
    # fate_scan 0
    assert int(run["noscan_scans"][0]) == 0
    for s in range(4):
        assert np.array_equal(run["noscan_h"][s], _blk(run, "blk", s)[0]), s
    assert np.array_equal(run["noscan_c"], _sum_c([_blk(run, "blk", s)[1] for s in range(4)]))


def test_blocking_calls_of_other_routes_in_the_middle(run):
    _ok(run, "other_routes")
    for i, r in enumerate((0, 1, 2, 3, 0, 1)):
        assert np.array_equal(run["routes_h"][i], _blk(run, "blk", r)[0]), i
    for k in ("beam", "disc"):
        assert np.array_equal(run[k + "_mid_h"], run[k + "_alone_h"]), k
        assert np.array_equal(run[k + "_mid_c"], run[k + "_alone_c"]), k
        assert int(run[k + "_alone_c"][0]) == (150_000 if k == "beam" else 100_000)
    # (a blocking call collects and drops what was enqueued before it: the last two calls are what is left)
    assert np.array_equal(run["routes_c"], _sum_c([_blk(run, "blk", 0)[1], _blk(run, "blk", 1)[1]]))


def test_lifecycle_calls_in_the_middle(run):
    _ok(run, "lifecycle")
    for s in range(2):
        assert np.array_equal(run["life_after_sync_h"][s], _blk(run, "blk", s)[0]), s
    for s in range(4):
        assert np.array_equal(run["life_h"][s], _blk(run, "blk", s)[0]), s
    assert np.array_equal(run["life_c"], _sum_c([_blk(run, "blk", s)[1] for s in range(4)]))
    for s in range(3):
        assert np.array_equal(run["shutdown_h"][s], _blk(run, "blk", s)[0]), s
    assert np.array_equal(run["reinit_h"], _blk(run, "blk", 3)[0])
    assert np.array_equal(run["reinit_c"], _blk(run, "blk", 3)[1])


@pytest.mark.parametrize("key", ["chord", "overlap2"])
def test_chord_mode_and_overlap_2_ignore_the_option(run, ora, key):
    _ok(run, "not_eligible")
    for s in range(3):
        bh, bc = _blk(run, key + "_blk", s)
        if key == "overlap2" or s == 0:   # (the chord oracle of one range: the others are held against the blocking calls)
            oh, oc = ora(PARTS[s][0], PARTS[s][1], trace_mode=1 if key == "chord" else 0)
            assert np.array_equal(bh, oh) and np.array_equal(bc, oc), (key, s)
        for co in (0, 1):
            assert np.array_equal(run["%s_%d_h" % (key, co)][s], bh), (key, co, s)
    for co in (0, 1):
        assert np.array_equal(run["%s_%d_c" % (key, co)], _sum_c([_blk(run, key + "_blk", s)[1] for s in range(3)])), (key, co)
