#!/usr/bin/env python3
"""Times the exit maps (isx_exit_maps, default spec) against the nearest sink an older build has: isx_exit_dz_hist (100 bins).

usage: tools/time_exit_maps.py [--rays N] [--calls K] [--warmup W] [--baseline-lib PATH/libisx.so]

For the default, BRDF-source and cos^2-lobe configurations, per leg the median of K calls after W warm-ups of
stats.t_kernel_ms and of the trace / binning split of isx_last_kernel_ms:
  dz_hist    isx_exit_dz_hist, 100 bins                     (the yardstick: exit_maps must not be slower)
  fluxmap    isx_fluxmap, twice                             (same trace kernel and launch plan as exit_maps; the two runs
                                                             give the run-to-run noise band of trace_ms)
  exit_maps  isx_exit_maps, 128 x 128 + 64 x 64 bins
--baseline-lib: the dz_hist and fluxmap legs again, in a process of their own, on that library (e.g. the parent commit's
build, which has no isx_exit_maps), so that both builds are measured in one session.  Prints one JSON object.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def configs(mod):
    out = {}
    for name in ("default", "brdf", "lobe"):
        c = mod.default_config()
        if name == "brdf":
            c.source_model = 1
        elif name == "lobe":
            c.surface_model = 1
        out[name] = c
    return out


def median_of(call, kinds, calls, warmup):
    """call() -> t_kernel_ms; kinds() -> (single, trace, bin) of that call"""
    rows = []
    for i in range(warmup + calls):
        t = call()
        if i >= warmup:
            rows.append((t,) + tuple(kinds()))
    med = [statistics.median(r[k] for r in rows) for k in range(4)]
    return {"t_kernel_ms": med[0], "single_ms": med[1], "trace_ms": med[2], "bin_ms": med[3],
            "min_ms": min(r[0] for r in rows), "max_ms": max(r[0] for r in rows)}


def legs(lib_path, rays, calls, warmup, with_exit_maps):
    """Through the package's structs and a plain ctypes handle of `lib_path` (an older build lacks the newer symbols the
    package binds at load time)."""
    import numpy as np
    import altair_raytracing_amd as isx
    abi = isx.abi
    L = C.CDLL(lib_path)
    u64, P = C.c_uint64, C.POINTER
    L.isx_default_config.restype = None
    L.isx_exit_dz_hist.argtypes = [P(abi.Config), u64, u64, u64, C.c_int32, P(u64), P(abi.Stats)]
    L.isx_fluxmap.argtypes = [P(abi.Config), u64, u64, u64, P(u64), P(abi.Stats)]
    L.isx_last_kernel_ms.argtypes = [P(C.c_double)] * 3
    if L.isx_init(0) != 0:
        raise SystemExit("no GPU: nothing to time")

    class Raw:
        @staticmethod
        def default_config():
            c = abi.Config()
            L.isx_default_config(C.byref(c))
            return c

    def kinds():
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        L.isx_last_kernel_ms(C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    out = {}
    seed = 0x5EED0001
    for name, cfg in configs(Raw).items():
        hist = np.zeros(100, dtype=np.uint64)
        hits = np.zeros(cfg.n_theta * cfg.n_phi, dtype=np.uint64)
        st = abi.Stats()

        def dz():
            rc = L.isx_exit_dz_hist(C.byref(cfg), rays, seed, 0, 100, hist.ctypes.data_as(P(u64)), C.byref(st))
            assert rc == 0, rc
            return st.t_kernel_ms

        def flux():
            rc = L.isx_fluxmap(C.byref(cfg), rays, seed, 0, hits.ctypes.data_as(P(u64)), C.byref(st))
            assert rc == 0, rc
            return st.t_kernel_ms

        row = {"dz_hist": median_of(dz, kinds, calls, warmup), "counted_below_z": int(st.counted_below_z),
               "fluxmap": median_of(flux, kinds, calls, warmup), "fluxmap_again": median_of(flux, kinds, calls, warmup)}
        if with_exit_maps:
            assert os.path.realpath(isx.LIB_PATH) == os.path.realpath(lib_path)
            isx.init(0)
            spec = isx.default_exit_map_spec(cfg)

            def maps():
                return isx.exit_maps(cfg, rays, seed, spec)[3].t_kernel_ms

            row["exit_maps"] = median_of(maps, kinds, calls, warmup)
            row["exit_maps"]["mrays_per_s"] = rays / row["exit_maps"]["t_kernel_ms"] / 1e3
        row["dz_hist"]["mrays_per_s"] = rays / row["dz_hist"]["t_kernel_ms"] / 1e3
        out[name] = row
    L.isx_shutdown()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=float, default=5e7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-lib")
    ap.add_argument("--only-older-legs", help=argparse.SUPPRESS)
    a = ap.parse_args()
    rays = int(a.rays)
    if a.only_older_legs:
        print(json.dumps(legs(a.only_older_legs, rays, a.calls, a.warmup, False)))
        return
    result = {"rays": rays, "calls": a.calls, "warmup": a.warmup}
    if a.baseline_lib:   # first, and in its own process: one library per process
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rays", str(rays), "--calls", str(a.calls), "--warmup",
                            str(a.warmup), "--only-older-legs", os.path.abspath(a.baseline_lib)], capture_output=True, text=True,
                           timeout=900)
        if r.returncode != 0:
            raise SystemExit("baseline leg failed: " + r.stderr[-2000:])
        result["baseline"] = json.loads(r.stdout.strip().splitlines()[-1])
    import altair_raytracing_amd as isx
    result["this_build"] = legs(isx.LIB_PATH, rays, a.calls, a.warmup, True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
