#!/usr/bin/env python3
"""Times the scene order histograms (isx_scene_order_hist) against the scene's flux map (isx_fluxmap_scene) for the same call.

usage: tools/time_scene_order.py [--rays N] [--reflectance R] [--calls K] [--warmup W] [--rounds R] [--limit SECONDS]

Every case runs in a fresh child process of its own with its own time limit (a case that fails or runs out of time ends the
session); the whole set is run R times (default 3) in one session, the cases in alternation.  The scene is `photometer` of
tools/time_scene.py at wall reflectance 0.95 (about 16 interactions per ray):
  scene          isx_fluxmap_scene: trace_ms of its trace kernel (its binning kernel is reported as bin_ms)
  order:512      isx_scene_order_hist with the default spec in the form plan_launch picks: the low orders of every slot in the
                 workgroup's LDS, the rest by global adds
  order:512:g    the same spec with "sorder_lds_orders" 0: one global u64 add per ended ray -- why the LDS block exists
  order:65536    the largest spec: as many low orders in the LDS as for 512, 21 x 65536 words of global memory behind them
isx_scene_order_hist is one kernel: its trace_ms is the call's single_ms.  Per row: median [min, max] of K calls after W warm-ups,
over all rounds.  Prints one JSON object; "ratios" are the medians of trace_ms of an order leg over the scene's.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SEED = 12345
CASES = ["scene", "order:512", "order:512:g", "order:65536"]


def summary(rows):
    return {"median": statistics.median(rows), "min": min(rows), "max": max(rows), "n": len(rows)}


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
        os_ = isx.scene_order_spec(int(parts[1]))
        isx.set_option("sorder_lds_orders", 0 if parts[-1] == "g" else -1)
        call = lambda: isx.scene_order_hist(cfg, spec, os_, rays, SEED)
    trace, binning, got = [], [], None
    for i in range(warmup + calls):
        got = call()
        if i >= warmup:
            ms = isx.last_kernel_ms()
            trace.append(ms[1] if case == "scene" else ms[0])
            binning.append(ms[2])
    st = got[-1]
    if case != "scene":
        hist, over = got[0], got[1].words()
        mean, sd = isx.scene_order_moments(os_, hist, over)
        extra = {"overflow": int(over.sum()), "largest_order": int(max(0, *[int(hist[f].nonzero()[0].max()) for f in range(21) if hist[f].any()])),
                 "mean_order": {"detector": mean[0], "port": mean[18]}, "sd_order": {"detector": sd[0], "port": sd[18]}}
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
    ap.add_argument("--leg", default="", help="(internal) run one case in this process")
    a = ap.parse_args()
    rays = int(a.rays)
    if a.leg:
        print(json.dumps(leg(rays, a.reflectance, a.calls, a.warmup, a.leg)))
        return
    out = {"rays": rays, "reflectance": a.reflectance, "calls": a.calls, "warmup": a.warmup, "rounds": a.rounds}
    rows = {}
    for _ in range(a.rounds):
        for case in CASES:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", case, "--rays", str(rays), "--reflectance", str(a.reflectance),
                   "--calls", str(a.calls), "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            if r.returncode != 0:      # (nothing more is started on the device once a case has failed)
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit("case %s failed with status %d" % (case, r.returncode))
            got = json.loads(r.stdout.strip().splitlines()[-1])
            out["device"] = got.pop("device")
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
