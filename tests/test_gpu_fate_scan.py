"""The fate scan on the device ("fate_scan"): isx_fate_scan_kernel settles the rays the inner wall absorbs from
their Philox words, isx_trace_assist_list_kernel traces the rest.  A scheduling option: histogram and census with the scan are
those without it, and the oracle's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fatescan_np as fs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0001
CENSUS = ("launched", "exited", "counted_below_z", "absorbed", "suspended", "bin_increments", "wall_hits")
DEFAULTS = (("fate_scan", -1), ("assist", 1), ("overlap", 0), ("pipeline_chunk", 1 << 26), ("grid_blocks", 0))


def _reset(isx):
    for k, v in DEFAULTS:
        isx.set_option(k, v)


def _census(st):
    return tuple(int(getattr(st, f)) for f in CENSUS)


def _cfg(mod, **kw):
    c = mod.default_config()
    for k, v in kw.items():
        if k in ("src", "dir"):
            for i in range(3):
                getattr(c, k)[i] = v[i]
        else:
            setattr(c, k, v)
    return c


def _on_off(isx, make, n, first=0, call=None, scans=1):
    """-> (hist, census) with fate_scan 1, after asserting that fate_scan 0 gives the same -- and that the call with 1 took the
    scan for `scans` chunks (isx_fate_scan_launches), the call with 0 for none"""
    call = call or (lambda c: isx.fluxmap(c, n, SEED, first))
    try:
        isx.set_option("fate_scan", 1)
        k0 = isx.fate_scan_launches()
        h1, s1 = call(make(isx))
        k1 = isx.fate_scan_launches()
        isx.set_option("fate_scan", 0)
        h0, s0 = call(make(isx))
        k2 = isx.fate_scan_launches()
    finally:
        isx.set_option("fate_scan", -1)
    assert (k1 - k0, k2 - k1) == (scans, 0), (k0, k1, k2)
    assert np.array_equal(h1, h0)
    assert _census(s1) == _census(s0)
    return h1, _census(s1)


# ------------------------------------------------------------------ the rule on the device is the numpy restatement
@pytest.mark.parametrize("name,kw,first", [("default", {}, 0), ("first_wrap", {}, 2 ** 32 - 1000), ("max_points3", {"max_points": 3}, 0)])
def test_device_fates_equal_the_numpy_restatement(isx, orc, name, kw, first):
    n = 200_000
    fate, order = isx.fate_scan(_cfg(isx, **kw), n, SEED, first)
    want_fate, want_order, _ = fs.fate_scan_np(_cfg(orc, **kw), n, SEED, first)
    assert np.array_equal(fate, want_fate), name
    assert np.array_equal(order, want_order), name
    assert (fate == fs.ABSORBED).any() and (fate == fs.TRACE).any()


# ------------------------------------------------------------------ scan on == scan off == the oracle
FLUX_CASES = {
    "default": ({}, 0, ()),
    "first_wrap": ({}, 2 ** 32 - 1000, ()),
    "rho0_every_ray_settled": ({"reflectance": 0.0}, 0, ()),
    "rho1_no_ray_settled": ({"reflectance": 1.0, "max_points": 64}, 0, ()),
    "max_points3": ({"max_points": 3}, 0, ()),
    "max_points8": ({"max_points": 8}, 0, ()),
    "five_chunks": ({}, 0, (("pipeline_chunk", 65536),)),
    "port160": ({"theta_max_deg": 160.0}, 0, ()),
    "origin_compat": ({"hit_line_mode": 1}, 0, ()),
}


@pytest.mark.parametrize("name", list(FLUX_CASES))
def test_fluxmap_with_the_scan_is_the_fluxmap_without_and_the_oracles(isx, orc, name):
    kw, first, opts = FLUX_CASES[name]
    n = 300_000
    try:
        for k, v in opts:
            isx.set_option(k, v)
        h, cen = _on_off(isx, lambda m: _cfg(m, **kw), n, first, scans=5 if name == "five_chunks" else 1)
    finally:
        _reset(isx)
    oh, ost = orc.fluxmap(_cfg(orc, **kw), n, SEED, first)
    assert np.array_equal(h, oh), name
    assert cen == _census(ost), (name, cen, _census(ost))
    if name == "rho0_every_ray_settled":
        assert cen[CENSUS.index("absorbed")] == n and cen[CENSUS.index("wall_hits")] == n
    if name == "rho1_no_ray_settled":
        assert cen[CENSUS.index("absorbed")] == 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_small_launches(isx, orc, n):
    h, cen = _on_off(isx, lambda m: m.default_config(), n, 7)
    oh, ost = orc.fluxmap(orc.default_config(), n, SEED, 7)
    assert np.array_equal(h, oh)
    assert cen == _census(ost)


def test_automatic_mode_leaves_small_calls_alone(isx):
    """fate_scan -1: a call of 3e5 rays is far below the rule's ray count and takes the kernels it took before"""
    _reset(isx)
    k0 = isx.fate_scan_launches()
    isx.fluxmap(isx.default_config(), 300_000, SEED, 0)
    assert isx.fate_scan_launches() == k0


def test_two_halves_of_a_range_sum_to_the_whole(isx):
    c = isx.default_config()
    try:
        isx.set_option("fate_scan", 1)
        whole, sw = isx.fluxmap(c, 300_000, SEED, 11)
        a, sa = isx.fluxmap(c, 123_457, SEED, 11)
        b, sb = isx.fluxmap(c, 300_000 - 123_457, SEED, 11 + 123_457)
    finally:
        _reset(isx)
    assert np.array_equal(a + b, whole)
    assert tuple(x + y for x, y in zip(_census(sa), _census(sb))) == _census(sw)


def test_three_enqueued_device_calls_equal_three_blocking_calls():
    """isx_fluxmap_device three times without a synchronisation in between (list, count word and counters of the launches are
    reused on the stream) against three blocking calls.  Own process: torch's HIP runtime has to come up before libisx's."""
    code = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
torch.cuda.init(); torch.zeros(1, device="cuda:0")
import altair_raytracing_amd as isx
isx.load(); isx.init(0)
SEED = 0x5EED0001
F = ("launched", "exited", "counted_below_z", "absorbed", "suspended", "bin_increments", "wall_hits")
c = isx.default_config()
nb = c.n_theta * c.n_phi
isx.set_option("fate_scan", 1)
parts = [(0, 70001), (70001, 110000), (180001, 120000)]    # (growing: the list is enlarged with launches enqueued)
d = torch.zeros(nb, dtype=torch.int64, device="cuda:0")
torch.cuda.synchronize()
for first, n in parts:
    isx.fluxmap_device(c, n, SEED, first, d.data_ptr())
isx.sync()
assert isx.fate_scan_launches() == 3
st = isx.take_stats()
torch.cuda.synchronize()
got = d.cpu().numpy().astype(np.uint64).reshape(c.n_theta, c.n_phi)
want = np.zeros_like(got)
cen = [0] * len(F)
for first, n in parts:
    h, s = isx.fluxmap(c, n, SEED, first)
    want += h
    cen = [a + int(getattr(s, f)) for a, f in zip(cen, F)]
assert np.array_equal(got, want)
assert [int(getattr(st, f)) for f in F] == cen, ([int(getattr(st, f)) for f in F], cen)
isx.set_option("fate_scan", 0)
h0, s0 = isx.fluxmap(c, 300001, SEED, 0)
assert np.array_equal(h0, want) and [int(getattr(s0, f)) for f in F] == cen
isx.shutdown()
print("ok", int(want.sum()))
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.stdout[-500:], r.stderr[-2000:])


# ------------------------------------------------------------------ what the scan does not serve takes the kernels it took before
INELIGIBLE = {
    "pencil_into_the_port": ({"dir": (60.0, 0.0, -25.0)}, ()),
    "brdf_source": ({"source_model": 1}, ()),
    "lobe": ({"surface_model": 1}, ()),
    "rough_specular": ({"lambertian": 0}, ()),
    "chord": ({"trace_mode": 1}, ()),
    "assist0": ({}, (("assist", 0),)),
    "overlap2": ({}, (("overlap", 2),)),
}


@pytest.mark.parametrize("name", list(INELIGIBLE))
def test_forced_scan_changes_nothing_where_it_is_not_eligible(isx, name):
    kw, opts = INELIGIBLE[name]
    try:
        for k, v in opts:
            isx.set_option(k, v)
        h, cen = _on_off(isx, lambda m: _cfg(m, **kw), 150_000, scans=0)
    finally:
        _reset(isx)
    assert cen[0] == 150_000


def test_forced_scan_changes_nothing_for_the_beam_source(isx):
    c = isx.default_config()
    spec = isx.beam_cone(c, (-60.0, 0.0, -75.0), (1.0, 0.0, 0.0), 2.0, 5.0)
    _, cen = _on_off(isx, lambda m: c, 150_000, call=lambda cc: isx.fluxmap_beam(cc, spec, 150_000, SEED, 0), scans=0)
    assert cen[0] == 150_000
