#!/usr/bin/env python3
"""Times the scene path histograms (isx_scene_path_hist) against the scene's flux map (isx_fluxmap_scene) for the same call.

usage: tools/time_scene_path.py [--rays N] [--reflectance R] [--calls K] [--warmup W] [--rounds R] [--limit SECONDS]
                                [--parent-lib PATH]

Every case runs in a fresh child process of its own with its own time limit (a case that fails or runs out of time ends the
session); the whole set is run R times (default 3) in one session, the cases in alternation.  The scene is `photometer` of
tools/time_scene.py at wall reflectance 0.95 (about 16 interactions per ray):
  scene          isx_fluxmap_scene: trace_ms of its trace kernel (its binning kernel is reported as bin_ms).  With --parent-lib
                 it is taken from that libisx.so -- a build of the parent commit -- through the C ABI alone, so that the ratios
                 are over the parent's trace in the same session
  path:1024      isx_scene_path_hist with the default spec (1024 bins of r_in / 4) in the form the plan picks: the low bins of
                 every slot in the workgroup's LDS, the rest by global adds
  path:1024:g    the same spec with "spath_lds_bins" 0: one global u64 add per ended ray
  path:65536     the largest spec
isx_scene_path_hist is one kernel: its trace_ms is the call's single_ms.  Per row: median [min, max] of K calls after W warm-ups,
over all rounds.  Prints one JSON object; "ratios" are the medians of trace_ms of a path leg over the scene's; the path legs
report the mean and the decay constant of the detector's row (slot 0) and the port's (slot 18) in cm and ns.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
SEED = 12345
CASES = ["scene", "path:1024", "path:1024:g", "path:65536"]


def summary(rows):
    return {"median": statistics.median(rows), "min": min(rows), "max": max(rows), "n": len(rows)}


def parent_leg(path, rays, rho, calls, warmup):
    """isx_fluxmap_scene of another libisx.so (the parent commit's), through the C ABI alone: this package's structs, that library's
    code.  This package's own library only builds the scene (host code); it is never initialised here."""
    import numpy as np
    import altair_raytracing_amd as isx
    from time_scene import scene
    A = isx.abi
    cfg = isx.default_config()
    cfg.reflectance = rho
    spec = scene(isx, cfg, "photometer")
    L = C.CDLL(path)
    P, u64, dbl = C.POINTER, C.c_uint64, C.c_double
    L.isx_fluxmap_scene.argtypes = [P(A.Config), P(A.SceneSpec), u64, u64, u64, P(u64), P(A.SceneCounts), P(A.Stats)]
    L.isx_last_kernel_ms.argtypes = [P(dbl), P(dbl), P(dbl)]
    assert L.isx_init(0) == 0
    hits = np.zeros(cfg.n_theta * cfg.n_phi, dtype=np.uint64)
    cnt, st = A.SceneCounts(), A.Stats()
    trace, binning = [], []
    for i in range(warmup + calls):
        rc = L.isx_fluxmap_scene(C.byref(cfg), C.byref(spec), rays, SEED, 0, hits.ctypes.data_as(P(u64)), C.byref(cnt), C.byref(st))
        assert rc == 0, rc
        if i >= warmup:
            a, b, c = dbl(0), dbl(0), dbl(0)
            L.isx_last_kernel_ms(C.byref(a), C.byref(b), C.byref(c))
            trace.append(b.value)
            binning.append(c.value)
    L.isx_shutdown()
    return {"device": "", "trace_ms": trace, "bin_ms": binning, "wall_hits_per_ray": st.wall_hits / rays,
            "port_fraction": st.counted_below_z / rays, "bin_increments": st.bin_increments, "library": path}


def leg(rays, rho, calls, warmup, case):
    import altair_raytracing_amd as isx
    from time_scene import scene
    isx.init(0)
    cfg = isx.default_config()
    cfg.reflectance = rho
    spec = scene(isx, cfg, "photometer")
    extra = {}
    if case == "scene":
        call = lambda: isx.fluxmap_scene(cfg, spec, rays, SEED)
    else:
        parts = case.split(":")
        ps = isx.scene_path_spec(int(parts[1]), cfg.r_in / 4)
        isx.set_option("spath_lds_bins", 0 if parts[-1] == "g" else -1)
        call = lambda: isx.scene_path_hist(cfg, spec, ps, rays, SEED)
    trace, binning, got = [], [], None
    for i in range(warmup + calls):
        got = call()
        if i >= warmup:
            ms = isx.last_kernel_ms()
            trace.append(ms[1] if case == "scene" else ms[0])
            binning.append(ms[2])
    st = got[-1]
    if case != "scene":
        hist, pc = got[0], got[1]
        over = pc.words()[:21]
        mean, sd = isx.scene_path_moments(ps, hist, pc)
        ns = isx.LIGHT_CM_PER_NS
        extra = {"overflow": int(over.sum()), "mean_cm": {"detector": mean[0], "port": mean[18]},
                 "mean_ns": {"detector": mean[0] / ns, "port": mean[18] / ns}, "sd_cm": {"detector": sd[0], "port": sd[18]}}
        for name, f in (("detector", 0), ("port", 18)):
            if not over[f]:
                lo = int(2 * mean[f] / ps.bin_cm)      # (the tail: from twice the mean on)
                try:
                    tau, sig = isx.scene_path_decay(ps, hist, pc, f, min(lo, ps.n_bins - 1))
                    extra.setdefault("tau_cm", {})[name] = [tau, sig]
                    extra.setdefault("tau_ns", {})[name] = [tau / ns, sig / ns]
                except isx.IsxError:
                    pass
    out = {"device": isx.device_info()[0], "trace_ms": trace, "bin_ms": binning, "wall_hits_per_ray": st.wall_hits / rays,
           "port_fraction": st.counted_below_z / rays, "bin_increments": st.bin_increments, **extra}
    isx.shutdown()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=float, default=5e7)
    ap.add_argument("--reflectance", type=float, default=0.95)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="time limit of each case, seconds")
    ap.add_argument("--parent-lib", default="", help="a libisx.so of the parent commit: the `scene` case is timed on it")
    ap.add_argument("--leg", default="", help="(internal) run one case in this process")
    a = ap.parse_args()
    rays = int(a.rays)
    if a.leg:
        if a.leg == "scene" and a.parent_lib:
            print(json.dumps(parent_leg(os.path.abspath(a.parent_lib), rays, a.reflectance, a.calls, a.warmup)))
        else:
            print(json.dumps(leg(rays, a.reflectance, a.calls, a.warmup, a.leg)))
        return
    out = {"rays": rays, "reflectance": a.reflectance, "calls": a.calls, "warmup": a.warmup, "rounds": a.rounds,
           "scene_library": a.parent_lib or "this build"}
    rows = {}
    for _ in range(a.rounds):
        for case in CASES:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", case, "--rays", str(rays), "--reflectance", str(a.reflectance),
                   "--calls", str(a.calls), "--warmup", str(a.warmup)]
            if a.parent_lib:
                cmd += ["--parent-lib", a.parent_lib]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            if r.returncode != 0:      # (nothing more is started on the device once a case has failed)
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit("case %s failed with status %d" % (case, r.returncode))
            got = json.loads(r.stdout.strip().splitlines()[-1])
            out["device"] = got.pop("device") or out.get("device", "")
            sys.stderr.write("%s done\n" % case)
            sys.stderr.flush()
            acc = rows.setdefault(case, {"trace_ms": [], "bin_ms": []})
            acc["trace_ms"] += got.pop("trace_ms")
            acc["bin_ms"] += got.pop("bin_ms")
            acc.update(got)
    for case, acc in rows.items():
        out[case] = dict(acc, trace_ms=summary(acc["trace_ms"]), bin_ms=summary(acc["bin_ms"]))
    out["ratios"] = {c: out[c]["trace_ms"]["median"] / out["scene"]["trace_ms"]["median"] for c in CASES[1:]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
