"""Exit lines from the words on the device ("exit_scan"): behind the fate scan isx_exit_lines_kernel forms the
exit line of every ray that leaves cleanly through the port from the ray's Philox words, with a proven bound on its deviation;
isx_trace_assist_list_kernel traces the rest; isx_bin_cols_kernel decides a candidate of such a line only where every line within the
bound agrees, and isx_redo_kernel traces the rays of the candidates that are left.  The option changes no result: histogram and
census with it are those without it, and the oracle's."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0001
CENSUS = ("launched", "exited", "counted_below_z", "absorbed", "suspended", "bin_increments", "wall_hits")
DEFAULTS = (("exit_scan", -1), ("exit_eps_scale", 1), ("fate_scan", -1), ("assist", 1), ("overlap", 0), ("pipeline_chunk", 1 << 26),
            ("grid_blocks", 0))


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


def _on_off(isx, make, n, first=0, call=None, ran=True, scale=1):
    """-> (hist, census, counts) with exit_scan 1, after asserting that exit_scan 0 gives the same -- and through
    isx_exit_scan_counts that the call with 1 took the path (`ran`: every ray the scan lists is accepted or sent on to list B) or
    did not, and that the call with 0 did not"""
    call = call or (lambda c: isx.fluxmap(c, n, SEED, first))
    try:
        isx.set_option("exit_eps_scale", scale)
        isx.set_option("exit_scan", 1)
        k0 = isx.exit_scan_counts()
        h1, s1 = call(make(isx))
        k1 = isx.exit_scan_counts()
        isx.set_option("exit_scan", 0)
        h0, s0 = call(make(isx))
        k2 = isx.exit_scan_counts()
    finally:
        isx.set_option("exit_scan", -1)
        isx.set_option("exit_eps_scale", 1)
    d = tuple(b - a for a, b in zip(k0, k1))
    assert k2 == k1, (k1, k2)
    if ran:
        assert d[0] + d[1] > 0 or _census(s1)[CENSUS.index("exited")] == 0, d
        assert d[0] <= _census(s1)[CENSUS.index("counted_below_z")]
    else:
        assert d == (0, 0, 0), d
    assert np.array_equal(h1, h0)
    assert _census(s1) == _census(s0)
    return h1, _census(s1), d


# ------------------------------------------------------------------ path on == path off == the oracle
FLUX_CASES = {
    "default": ({}, 0, ()),
    "first_wrap": ({}, 2 ** 32 - 1000, ()),
    "rho0": ({"reflectance": 0.0}, 0, ()),
    "rho1_max_points64": ({"reflectance": 1.0, "max_points": 64}, 0, ()),
    "max_points3": ({"max_points": 3}, 0, ()),
    "max_points8": ({"max_points": 8}, 0, ()),
    "five_chunks": ({}, 0, (("pipeline_chunk", 65536),)),
    "port160": ({"theta_max_deg": 160.0}, 0, ()),
    "grid_blocks1": ({}, 0, (("grid_blocks", 1),)),
}


@pytest.mark.parametrize("name", list(FLUX_CASES))
def test_fluxmap_with_exit_lines_is_the_fluxmap_without_and_the_oracles(isx, orc, name):
    kw, first, opts = FLUX_CASES[name]
    n = 300_000
    try:
        for k, v in opts:
            isx.set_option(k, v)
        h, cen, d = _on_off(isx, lambda m: _cfg(m, **kw), n, first)
    finally:
        _reset(isx)
    oh, ost = orc.fluxmap(_cfg(orc, **kw), n, SEED, first)
    assert np.array_equal(h, oh), name
    assert cen == _census(ost), (name, cen, _census(ost))
    if name == "rho0":
        assert d == (0, 0, 0)          # every ray is absorbed at its first strike: the scan lists none
    elif name != "max_points3":        # (three track points: a ray can leave at interactions 0 and 1 only)
        assert d[0] > 0.5 * cen[CENSUS.index("counted_below_z")], (name, d, cen)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513])
def test_small_launches(isx, orc, n):
    h, cen, _ = _on_off(isx, lambda m: m.default_config(), n, 7)
    oh, ost = orc.fluxmap(orc.default_config(), n, SEED, 7)
    assert np.array_equal(h, oh)
    assert cen == _census(ost)


def test_two_halves_of_a_range_sum_to_the_whole(isx):
    c = isx.default_config()
    try:
        isx.set_option("exit_scan", 1)
        k0 = isx.exit_scan_counts()
        whole, sw = isx.fluxmap(c, 300_000, SEED, 11)
        k1 = isx.exit_scan_counts()
        a, sa = isx.fluxmap(c, 123_457, SEED, 11)
        b, sb = isx.fluxmap(c, 300_000 - 123_457, SEED, 11 + 123_457)
        k2 = isx.exit_scan_counts()
    finally:
        _reset(isx)
    assert np.array_equal(a + b, whole)
    assert tuple(x + y for x, y in zip(_census(sa), _census(sb))) == _census(sw)
    assert k1[0] > k0[0] and tuple(y - x for x, y in zip(k1, k2))[:2] == tuple(y - x for x, y in zip(k0, k1))[:2]


def test_three_enqueued_device_calls_equal_three_blocking_calls():
    """isx_fluxmap_device three times without a synchronisation in between (lists, side entries, redo lists and counters rotate with the
    workspaces) against three blocking calls.  Own process: torch's HIP runtime has to come up before libisx's."""
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
isx.set_option("exit_scan", 1)
parts = [(0, 70001), (70001, 110000), (180001, 120000)]    # (growing: the workspaces are enlarged with launches enqueued)
d = torch.zeros(nb, dtype=torch.int64, device="cuda:0")
torch.cuda.synchronize()
for first, n in parts:
    isx.fluxmap_device(c, n, SEED, first, d.data_ptr())
isx.sync()
acc, lb, redo = isx.exit_scan_counts()
st = isx.take_stats()
torch.cuda.synchronize()
assert acc > 0.9 * int(st.counted_below_z) and acc + lb > 0, (acc, lb, int(st.counted_below_z))
got = d.cpu().numpy().astype(np.uint64).reshape(c.n_theta, c.n_phi)
isx.set_option("exit_scan", 0)
want = np.zeros_like(got)
cen = [0] * len(F)
for first, n in parts:
    h, s = isx.fluxmap(c, n, SEED, first)
    want += h
    cen = [a + int(getattr(s, f)) for a, f in zip(cen, F)]
assert isx.exit_scan_counts()[:2] == (acc, lb)
assert np.array_equal(got, want)
assert [int(getattr(st, f)) for f in F] == cen, ([int(getattr(st, f)) for f in F], cen)
isx.shutdown()
print("ok", int(want.sum()))
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.stdout[-500:], r.stderr[-2000:])


# ------------------------------------------------------------------ the redo path: every bound multiplied
@pytest.mark.parametrize("scale", [1000, 1000000])
def test_scaled_bounds_reach_the_redo_kernel_and_change_nothing(isx, orc, scale):
    n = 20_000
    h, cen, d = _on_off(isx, lambda m: m.default_config(), n, 0, scale=scale)
    print(f"exit_eps_scale {scale}: accepted {d[0]}, list B {d[1]}, redo entries {d[2]}")
    assert d[2] > 0, d
    oh, ost = orc.fluxmap(orc.default_config(), n, SEED, 0)
    assert np.array_equal(h, oh)
    assert cen == _census(ost)


def test_a_bound_cannot_be_made_narrower(isx):
    with pytest.raises(isx.IsxError):
        isx.set_option("exit_eps_scale", 0)
    isx.set_option("exit_eps_scale", 1)


# ------------------------------------------------------------------ what the path does not serve takes the kernels it took before
INELIGIBLE = {
    "origin_compat": ({"hit_line_mode": 1}, ()),
    "brdf_source": ({"source_model": 1}, ()),
    "lobe": ({"surface_model": 1}, ()),
    "rough_specular": ({"lambertian": 0}, ()),
    "chord": ({"trace_mode": 1}, ()),
    "assist0": ({}, (("assist", 0),)),
}


@pytest.mark.parametrize("name", list(INELIGIBLE))
def test_forced_path_changes_nothing_where_it_is_not_eligible(isx, name):
    kw, opts = INELIGIBLE[name]
    try:
        for k, v in opts:
            isx.set_option(k, v)
        h, cen, _ = _on_off(isx, lambda m: _cfg(m, **kw), 150_000, ran=False)
    finally:
        _reset(isx)
    assert cen[0] == 150_000


def test_forced_path_changes_nothing_for_the_beam_source(isx):
    c = isx.default_config()
    spec = isx.beam_cone(c, (-60.0, 0.0, -75.0), (1.0, 0.0, 0.0), 2.0, 5.0)
    _, cen, _ = _on_off(isx, lambda m: c, 150_000, call=lambda cc: isx.fluxmap_beam(cc, spec, 150_000, SEED, 0), ran=False)
    assert cen[0] == 150_000
