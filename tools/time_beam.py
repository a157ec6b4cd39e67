#!/usr/bin/env python3
"""Times the beam-source flux map (isx_fluxmap_beam) against the flux map of the pencil for the same call.

usage: tools/time_beam.py [--rays N] [--calls K] [--warmup W] [--parent-lib PATH] [--limit SECONDS]

Two legs, each in a fresh child process with its own time limit, on the default configuration:
  beam      this build: trace_ms / bin_ms of isx_fluxmap_beam for the degenerate beam (isx_default_beam_spec: the pencil's own ray
            histories, so what differs from the flux map is the sampled start alone) and for "side" (a 10 cm disc at the pencil's
            source, 20 degree cone: other histories -- reported, not compared)
  fluxmap   trace_ms / bin_ms of isx_fluxmap for the same call, through the library at PATH -- a build of the parent commit -- or,
            without --parent-lib, through this build (the flux map's trace kernel is the parent's: tools/isa_stats.py shows the
            same code before and after).  Bound with plain ctypes, so that a library without the new symbols loads.
Per row: median [min, max] of K calls after W warm-ups.  Prints one JSON object; "degenerate_over_parent_trace" is the ratio the
acceptance bounds at 1.10 (docs/LOG.md, "Beam source").
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


def leg_beam(rays, calls, warmup):
    import altair_raytracing_amd as isx
    isx.init(0)
    cfg = isx.default_config()
    beams = {"degenerate": isx.default_beam_spec(cfg),
             "side": isx.beam_cone(cfg, (-60, 0, -75), (1, 0, 0), 10.0, 20.0, isx.BEAM_UNIFORM)}
    out = {"device": isx.device_info()[0]}
    for name, spec in beams.items():
        trace, binning, st = [], [], None
        for i in range(warmup + calls):
            _, st = isx.fluxmap_beam(cfg, spec, rays, SEED)
            if i >= warmup:
                ms = isx.last_kernel_ms()
                trace.append(ms[1])
                binning.append(ms[2])
        out[name] = {"trace_ms": summary(trace), "bin_ms": summary(binning), "wall_hits_per_ray": st.wall_hits / rays,
                     "port_fraction": st.counted_below_z / rays}
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
    trace, binning = [], []
    for i in range(warmup + calls):
        if L.isx_fluxmap(C.byref(cfg), rays, SEED, 0, hits, C.byref(st)) != 0:
            raise SystemExit("isx_fluxmap failed")
        ms = [C.c_double(), C.c_double(), C.c_double()]
        L.isx_last_kernel_ms(*[C.byref(m) for m in ms])
        if i >= warmup:
            trace.append(ms[1].value)
            binning.append(ms[2].value)
    L.isx_shutdown()
    return {"library": "parent build" if lib_path else "this build", "trace_ms": summary(trace), "bin_ms": summary(binning),
            "wall_hits_per_ray": st.wall_hits / rays}


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
    if a.leg == "beam":
        print(json.dumps(leg_beam(rays, a.calls, a.warmup)))
        return
    if a.leg == "fluxmap":
        print(json.dumps(leg_fluxmap(rays, a.calls, a.warmup, a.parent_lib)))
        return
    out = {"rays": rays, "calls": a.calls, "warmup": a.warmup}
    for leg in ("fluxmap", "beam"):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--rays", str(rays), "--calls", str(a.calls), "--warmup", str(a.warmup)]
        if a.parent_lib:
            cmd += ["--parent-lib", a.parent_lib]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:      # (nothing more is started on the device once a leg has failed)
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("leg %s failed with status %d" % (leg, r.returncode))
        out[leg] = json.loads(r.stdout.strip().splitlines()[-1])
    out["degenerate_over_parent_trace"] = out["beam"]["degenerate"]["trace_ms"]["median"] / out["fluxmap"]["trace_ms"]["median"]
    out["side_over_parent_trace"] = out["beam"]["side"]["trace_ms"]["median"] / out["fluxmap"]["trace_ms"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
