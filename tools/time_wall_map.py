#!/usr/bin/env python3
"""Times the wall map (isx_wall_map, 64 x 64) against the trace kernel of the flux map for the same call.

usage: tools/time_wall_map.py [--rays N] [--calls K] [--warmup W] [--configs default,chord,brdf[,lobe,rough]]

For each configuration, in one session, the median of K calls after W warm-ups:
  fluxmap        isx_fluxmap: trace_ms of isx_last_kernel_ms -- the yardstick.  The flux map's trace kernels are not touched by
                 the wall map (tools/isa_stats.py shows the same code before and after), so this is the parent's kernel.
  fluxmap_again  the same once more: the run-to-run noise band of trace_ms
  wall_assist_0 / wall_assist_1    isx_wall_map on the assist-wave route (the default), first_order 0 and 1: single_ms
  wall_fused_0 / wall_fused_1      the same on the fused route (isx_set_option("assist", 0))
and the ratio wall map / flux-map trace time of every leg.  Prints one JSON object.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def config(isx, name):
    c = isx.default_config()
    if name == "brdf":
        c.source_model = 1
    elif name == "chord":
        c.trace_mode = 1
    elif name == "lobe":
        c.surface_model = 1
    elif name == "rough":
        c.lambertian = 0; c.roughness_rad = 0.5
    elif name != "default":
        raise SystemExit("unknown configuration " + name)
    return c


def median_of(isx, call, calls, warmup):
    rows = []
    for i in range(warmup + calls):
        call()
        if i >= warmup:
            rows.append(isx.last_kernel_ms())
    return {k: statistics.median(r[i] for r in rows) for i, k in enumerate(("single_ms", "trace_ms", "bin_ms"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=float, default=5e7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", default="default,chord,brdf")
    a = ap.parse_args()
    rays = int(a.rays)
    import altair_raytracing_amd as isx
    isx.init(0)
    seed = 0x5EED0001
    out = {"rays": rays, "calls": a.calls, "warmup": a.warmup, "device": isx.device_info()[0]}
    for name in a.configs.split(","):
        cfg = config(isx, name)
        row = {}
        isx.set_option("assist", 1)
        for leg in ("fluxmap", "fluxmap_again"):
            row[leg] = median_of(isx, lambda: isx.fluxmap(cfg, rays, seed), a.calls, a.warmup)
        yard = row["fluxmap"]["trace_ms"] or row["fluxmap"]["single_ms"]   # (a configuration the flux pipeline does not serve: its one kernel)
        for route, assist in (("assist", 1), ("fused", 0)):
            isx.set_option("assist", assist)
            for first_order in (0, 1):
                spec = isx.default_wall_map_spec(cfg)
                spec.first_order = first_order
                res = {}

                def call():
                    res["r"] = isx.wall_map(cfg, rays, seed, spec)

                leg = median_of(isx, call, a.calls, a.warmup)
                _, k, st = res["r"]
                leg["ratio_to_fluxmap_trace"] = leg["single_ms"] / yard
                leg["increments_per_ray"] = k.binned / rays
                leg["g_increments_per_s"] = k.binned / leg["single_ms"] / 1e6
                row["wall_%s_%d" % (route, first_order)] = leg
                row["wall_hits"] = int(st.wall_hits)
        isx.set_option("assist", 1)
        out[name] = row
    isx.shutdown()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
