#!/usr/bin/env python3
"""Times the flux map with baffles (isx_fluxmap_baffle) against the flux map without the feature for the same call.

usage: tools/time_baffle.py [--rays N] [--calls K] [--warmup W] [--rounds R] [--parent-lib PATH] [--limit SECONDS]

Two legs, run alternately R times (default 3) in one session, on the default configuration; the flux map and every baffle case run
in a fresh child process of their own, each with its own time limit (a case that fails or runs out of time ends the session):
  fluxmap   (a) trace_ms / bin_ms of isx_fluxmap with "fate_scan" 0 -- the trace kernel the baffle kernel is derived from --
            through the library at PATH (a build of the parent commit) or, without --parent-lib, through this build.  Bound
            with plain ctypes, so that a library without the new symbols loads.
  baffle    this build: isx_fluxmap_baffle with (b) no baffle, (c) "shield" (a disc of radius 8 between the first-strike spot and
            the port), (d) "two" (the shield and a disc of radius 25 about the centre), (e) "first_in" (a disc of radius 12 in the
            pencil's way: every ray starts its life in the assist wave).  The issue's own "first" (the shield with radius 12)
            overhangs the wall and is refused; the row says so.
Per row: median [min, max] of K calls after W warm-ups, over all rounds.  Prints one JSON object; "ratios" are the medians of
trace_ms over (a)'s.
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
NORMAL = (-66.3, 0.0, -23.6)
BAFFLES = {
    "none": [],
    "shield": [((30, 0, -85), NORMAL, 8.0, 0.9)],
    "two": [((30, 0, -85), NORMAL, 8.0, 0.9), ((0, 0, 0), (0, 0, 1), 25.0, 0.5)],
    "first": [((30, 0, -85), NORMAL, 12.0, 0.9)],
    "first_in": [((30, 0, -80), NORMAL, 12.0, 0.9)],
}


def summary(rows):
    return {"median": statistics.median(rows), "min": min(rows), "max": max(rows), "n": len(rows)}


def leg_baffle(rays, calls, warmup, case):
    import altair_raytracing_amd as isx
    isx.init(0)
    cfg = isx.default_config()
    out = {"device": isx.device_info()[0]}
    for name, discs in ((case, BAFFLES[case]),):
        spec = isx.baffle_spec(cfg, [isx.baffle_disc(cfg, *d) for d in discs])
        trace, binning, st, cnt = [], [], None, None
        try:
            for i in range(warmup + calls):
                _, cnt, st = isx.fluxmap_baffle(cfg, spec, rays, SEED)
                if i >= warmup:
                    ms = isx.last_kernel_ms()
                    trace.append(ms[1])
                    binning.append(ms[2])
        except isx.IsxError as e:
            if e.status != isx.abi.ERR_BAD_CONFIG:
                raise
            out[name] = {"refused": e.status}
            continue
        out[name] = {"trace_ms": trace, "bin_ms": binning, "wall_hits_per_ray": st.wall_hits / rays,
                     "port_fraction": st.counted_below_z / rays, "baffle_arrivals_per_ray": float(cnt.arrays()[0].sum()) / rays}
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
    L.isx_set_option.argtypes = [C.c_char_p, C.c_int64]
    L.isx_shutdown.restype = None
    cfg = abi.Config()
    L.isx_default_config(C.byref(cfg))
    if L.isx_init(0) != 0:
        raise SystemExit("isx_init failed")
    if L.isx_set_option(b"fate_scan", 0) != 0:
        raise SystemExit("isx_set_option(fate_scan) failed")
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
    return {"library": "parent build" if lib_path else "this build", "trace_ms": trace, "bin_ms": binning,
            "wall_hits_per_ray": st.wall_hits / rays, "port_fraction": st.counted_below_z / rays}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=float, default=5e7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--limit", type=int, default=240, help="time limit of each leg, seconds")
    ap.add_argument("--leg", default="", help="(internal) run one leg in this process")
    a = ap.parse_args()
    rays = int(a.rays)
    if a.leg.startswith("baffle:"):
        print(json.dumps(leg_baffle(rays, a.calls, a.warmup, a.leg.split(":", 1)[1])))
        return
    if a.leg == "fluxmap":
        print(json.dumps(leg_fluxmap(rays, a.calls, a.warmup, a.parent_lib)))
        return
    out = {"rays": rays, "calls": a.calls, "warmup": a.warmup, "rounds": a.rounds}
    rows = {}
    for _ in range(a.rounds):
        for leg in ["fluxmap"] + ["baffle:" + name for name in BAFFLES]:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--rays", str(rays), "--calls", str(a.calls), "--warmup", str(a.warmup)]
            if a.parent_lib:
                cmd += ["--parent-lib", a.parent_lib]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            if r.returncode != 0:      # (nothing more is started on the device once a leg has failed)
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit("leg %s failed with status %d" % (leg, r.returncode))
            got = json.loads(r.stdout.strip().splitlines()[-1])
            cases = {"fluxmap": got} if leg == "fluxmap" else {k: v for k, v in got.items() if isinstance(v, dict)}
            if leg != "fluxmap":
                out["device"] = got["device"]
            sys.stderr.write("%s done\n" % leg)
            sys.stderr.flush()
            for name, row in cases.items():
                acc = rows.setdefault(name, {"trace_ms": [], "bin_ms": []})
                if "refused" in row:
                    acc["refused"] = row["refused"]
                    continue
                acc["trace_ms"] += row["trace_ms"]
                acc["bin_ms"] += row["bin_ms"]
                for k, v in row.items():
                    if k not in ("trace_ms", "bin_ms"):
                        acc[k] = v
    for name, acc in rows.items():
        if "refused" in acc:
            out[name] = {"refused": acc["refused"]}
        else:
            out[name] = dict(acc, trace_ms=summary(acc["trace_ms"]), bin_ms=summary(acc["bin_ms"]))
    base = out["fluxmap"]["trace_ms"]["median"]
    out["ratios"] = {name: out[name]["trace_ms"]["median"] / base for name in BAFFLES if "trace_ms" in out[name]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
