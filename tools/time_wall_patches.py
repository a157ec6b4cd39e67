#!/usr/bin/env python3
"""Times the wall patches (isx_wall_patches) against the trace kernel of the flux map for the same call.

usage: tools/time_wall_patches.py [--rays N] [--calls K] [--warmup W] [--parent-lib PATH] [--limit SECONDS]

Two legs, each in a fresh child process with its own time limit:
  patches   this build: isx_wall_patches for the headline call with 0, 1, 4 and 8 patches at the WALL'S reflectance -- the
            histories are then those of the flux map, so what differs between the rows is the cost of the patch test alone;
            single_ms of isx_last_kernel_ms
  fluxmap   trace_ms of isx_fluxmap for the same call, through the library at PATH -- a build of the parent commit -- or, without
            --parent-lib, through this build (the flux map's trace kernel is the parent's: tools/isa_stats.py shows the same
            code before and after).  Bound with plain ctypes, so that a library without the new symbols loads.
Per row: median [min, max] of K calls after W warm-ups.  Prints one JSON object.
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
SEED = 0x5EED0001


def summary(rows):
    return {"median": statistics.median(rows), "min": min(rows), "max": max(rows)}


def leg_patches(rays, calls, warmup):
    import altair_raytracing_amd as isx
    isx.init(0)
    cfg = isx.default_config()
    dirs = [(0, 0, 1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (1, 1, 1), (-1, -1, 0.5), (66.3, 0, -75)]
    out = {"device": isx.device_info()[0]}
    for P in (0, 1, 4, 8):
        spec = isx.wall_patch_spec(cfg, [isx.wall_patch_cap(cfg, d, 20.0, cfg.reflectance) for d in dirs[:P]])
        rows, st = [], None
        for i in range(warmup + calls):
            arr, ab, st = isx.wall_patches(cfg, rays, SEED, spec)
            if i >= warmup:
                rows.append(isx.last_kernel_ms()[0])
        row = summary(rows)
        row["arrivals_on_patches_per_ray"] = st.bin_increments / rays
        row["wall_hits_per_ray"] = st.wall_hits / rays
        out["patches_%d" % P] = row
    isx.shutdown()
    return out


def leg_fluxmap(rays, calls, warmup, lib_path):
    from importlib import import_module
    abi = import_module("altair-raytracing_amd._abi")      # (the struct layouts; nothing is loaded)
    L = C.CDLL(lib_path or abi.LIB_PATH)
    u64, P = C.c_uint64, C.POINTER
    L.isx_default_config.argtypes = [P(abi.Config)]
    L.isx_default_config.restype = None
    L.isx_fluxmap.argtypes = [P(abi.Config), u64, u64, u64, P(u64), P(abi.Stats)]
    L.isx_last_kernel_ms.argtypes = [P(C.c_double)] * 3
    L.isx_shutdown.restype = None
    cfg = abi.Config()
    L.isx_default_config(C.byref(cfg))
    if L.isx_init(0) != 0:
        raise SystemExit("isx_init failed")
    hits = (u64 * (cfg.n_theta * cfg.n_phi))()
    st = abi.Stats()
    rows = []
    for i in range(warmup + calls):
        if L.isx_fluxmap(C.byref(cfg), rays, SEED, 0, hits, C.byref(st)) != 0:
            raise SystemExit("isx_fluxmap failed")
        ms = [C.c_double(), C.c_double(), C.c_double()]
        L.isx_last_kernel_ms(*[C.byref(m) for m in ms])
        if i >= warmup:
            rows.append(ms[1].value)
    L.isx_shutdown()
    out = {"library": "parent build" if lib_path else "this build", "trace_ms": summary(rows), "wall_hits_per_ray": st.wall_hits / rays}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=float, default=5e7)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--limit", type=int, default=240, help="time limit of each leg, seconds")
    ap.add_argument("--leg", default="", help="(internal) run one leg in this process")
    a = ap.parse_args()
    rays = int(a.rays)
    if a.leg == "patches":
        print(json.dumps(leg_patches(rays, a.calls, a.warmup)))
        return
    if a.leg == "fluxmap":
        print(json.dumps(leg_fluxmap(rays, a.calls, a.warmup, a.parent_lib)))
        return
    out = {"rays": rays, "calls": a.calls, "warmup": a.warmup}
    for leg in ("fluxmap", "patches"):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--rays", str(rays), "--calls", str(a.calls), "--warmup", str(a.warmup)]
        if a.parent_lib:
            cmd += ["--parent-lib", a.parent_lib]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:      # (nothing more is started on the device once a leg has failed)
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("leg %s failed with status %d" % (leg, r.returncode))
        out[leg] = json.loads(r.stdout.strip().splitlines()[-1])
    yard = out["fluxmap"]["trace_ms"]["median"]
    for k, row in out["patches"].items():
        if isinstance(row, dict):
            row["minus_fluxmap_trace_ms"] = row["median"] - yard
            row["ratio_to_fluxmap_trace"] = row["median"] / yard
    print(json.dumps(out))


if __name__ == "__main__":
    main()
