#!/usr/bin/env python3
"""Times the scene call (isx_fluxmap_scene) against the specialised calls for the same content.

usage: tools/time_scene.py [--rays N] [--calls K] [--warmup W] [--rounds R] [--limit SECONDS]

Every case runs in a fresh child process of its own with its own time limit (a case that fails or runs out of time ends the
session); the whole set is run R times (default 3) in one session, on the default configuration (wall reflectance 0.99).  Each leg
is a specialised call and the scene restricted to the same content:
  fluxmap    isx_fluxmap with "fate_scan" 0        | scene:empty     the default scene spec
  baffle     isx_fluxmap_baffle with `shield`      | scene:shield    the scene with only `shield`
  beam       isx_fluxmap_beam with `led`           | scene:led       the scene with only `led`
  patches    isx_wall_patches with [det, sample]   | scene:patches   the scene with only the patches  (trace_ms only: the
             (no binning kernel)                   |                 specialised call bins nothing)
and then the two scenes that have no specialised counterpart: scene:photometer and scene:led_first_in.
Per row: median [min, max] of K calls after W warm-ups, over all rounds.  Prints one JSON object; "ratios" are the medians of
trace_ms of a scene leg over its specialised call's.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 0x5EED0001
NORMAL = (-66.3, 0.0, -23.6)
PAIRS = [("fluxmap", "scene:empty"), ("baffle", "scene:shield"), ("beam", "scene:led"), ("patches", "scene:patches")]
ALONE = ["scene:photometer", "scene:led_first_in"]


def summary(rows):
    return {"median": statistics.median(rows), "min": min(rows), "max": max(rows), "n": len(rows)}


def parts(isx, cfg):
    return {
        "lamp": isx.beam_cone(cfg, (0, 0, 20), (0, 0, 1), 0.0, 180.0, isx.BEAM_UNIFORM),
        "led": isx.beam_cone(cfg, (-60, 0, -75), (1, 0, 0), 2.0, 3.0, isx.BEAM_LAMBERT),
        "screen": isx.baffle_disc(cfg, (35, 0, 13), (1, 0, 0), 10.0, 0.9),
        "shield_port": isx.baffle_disc(cfg, (0, 0, -40), (0, 0, 1), 12.0, 0.9),
        "shield": isx.baffle_disc(cfg, (30, 0, -85), NORMAL, 8.0, 0.9),
        "first_in": isx.baffle_disc(cfg, (30, 0, -80), NORMAL, 12.0, 0.9),
        "det": isx.wall_patch_cap(cfg, (1, 0, 0), 5.0, 0.0),
        "sample": isx.wall_patch_cap(cfg, (0, 1, 0), 10.0, 0.5),
    }


def scene(isx, cfg, name):
    p = parts(isx, cfg)
    beam, baffles, patches = {"empty": (None, (), ()), "shield": (None, ("shield",), ()), "led": ("led", (), ()),
                              "patches": (None, (), ("det", "sample")),
                              "photometer": ("lamp", ("screen", "shield_port"), ("det", "sample")),
                              "led_first_in": ("led", ("first_in",), ("det", "sample"))}[name]
    return isx.scene_spec(cfg, p[beam] if beam else None, [p[b] for b in baffles], [p[w] for w in patches])


def leg(rays, calls, warmup, case):
    import altair_raytracing_amd as isx
    isx.init(0)
    cfg = isx.default_config()
    p = parts(isx, cfg)
    if case == "fluxmap":
        isx.set_option("fate_scan", 0)
        call = lambda: isx.fluxmap(cfg, rays, SEED)[-1]
    elif case == "baffle":
        spec = isx.baffle_spec(cfg, [p["shield"]])
        call = lambda: isx.fluxmap_baffle(cfg, spec, rays, SEED)[-1]
    elif case == "beam":
        call = lambda: isx.fluxmap_beam(cfg, p["led"], rays, SEED)[-1]
    elif case == "patches":
        spec = isx.wall_patch_spec(cfg, [p["det"], p["sample"]])
        call = lambda: isx.wall_patches(cfg, rays, SEED, spec)[-1]
    else:
        spec = scene(isx, cfg, case.split(":", 1)[1])
        call = lambda: isx.fluxmap_scene(cfg, spec, rays, SEED)[-1]
    trace, binning, st = [], [], None
    for i in range(warmup + calls):
        st = call()
        if i >= warmup:
            ms = isx.last_kernel_ms()
            trace.append(ms[0] if case == "patches" else ms[1])      # (isx_wall_patches is one kernel: single_ms)
            binning.append(ms[2])
    out = {"device": isx.device_info()[0], "trace_ms": trace, "bin_ms": binning, "wall_hits_per_ray": st.wall_hits / rays,
           "port_fraction": st.counted_below_z / rays}
    isx.shutdown()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=float, default=5e7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="time limit of each case, seconds")
    ap.add_argument("--leg", default="", help="(internal) run one case in this process")
    a = ap.parse_args()
    rays = int(a.rays)
    if a.leg:
        print(json.dumps(leg(rays, a.calls, a.warmup, a.leg)))
        return
    out = {"rays": rays, "calls": a.calls, "warmup": a.warmup, "rounds": a.rounds}
    rows = {}
    cases = [c for pair in PAIRS for c in pair] + ALONE
    for _ in range(a.rounds):
        for case in cases:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", case, "--rays", str(rays), "--calls", str(a.calls), "--warmup", str(a.warmup)]
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
    out["ratios"] = {s: out[s]["trace_ms"]["median"] / out[b]["trace_ms"]["median"] for b, s in PAIRS}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
