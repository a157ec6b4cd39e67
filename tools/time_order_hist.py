#!/usr/bin/env python3
"""Times the bounce-order histograms (isx_order_hist) against the trace kernel of the flux map for the same call.

usage: tools/time_order_hist.py [--rays N] [--calls K] [--warmup W] [--configs default[,chord,brdf,lobe,rough]]

For each configuration, in one session, the median of K calls after W warm-ups:
  fluxmap        isx_fluxmap: trace_ms of isx_last_kernel_ms -- the yardstick.  The flux map's trace kernels are not touched by
                 the order histograms (tools/isa_stats.py shows the same code before and after), so this is the parent's kernel.
  fluxmap_again  the same once more: the run-to-run noise band of trace_ms
  order_assist / order_assist_2048x0 / order_assist_128x60   isx_order_hist on the assist-wave route (the default) with the
                 default spec (512 x 8), 2048 orders without dz, and the largest LDS block (8192 words): single_ms
  order_fused    the default spec on the fused route (isx_set_option("assist", 0))
and the ratio order histogram / flux-map trace time of every leg.  On a build without isx_order_hist (the parent commit) only the
two flux-map legs are timed.  Prints one JSON object.
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
    ap.add_argument("--configs", default="default")
    a = ap.parse_args()
    rays = int(a.rays)
    import altair_raytracing_amd as isx
    isx.init(0)
    seed = 0x5EED0001
    have = hasattr(isx, "order_hist")
    out = {"rays": rays, "calls": a.calls, "warmup": a.warmup, "device": isx.device_info()[0], "order_hist": have}
    for name in a.configs.split(","):
        cfg = config(isx, name)
        row = {}
        isx.set_option("assist", 1)
        for leg in ("fluxmap", "fluxmap_again"):
            row[leg] = median_of(isx, lambda: isx.fluxmap(cfg, rays, seed), a.calls, a.warmup)
        yard = row["fluxmap"]["trace_ms"] or row["fluxmap"]["single_ms"]   # (a configuration the flux pipeline does not serve: its one kernel)
        legs = (("order_assist", 1, 512, 8), ("order_assist_2048x0", 1, 2048, 0), ("order_assist_128x60", 1, 128, 60),
                ("order_fused", 0, 512, 8)) if have else ()
        for leg_name, assist, n_orders, n_dz in legs:
            isx.set_option("assist", assist)
            spec = isx.default_order_hist_spec(cfg)
            spec.n_orders, spec.n_dz = n_orders, n_dz
            res = {}

            def call():
                res["r"] = isx.order_hist(cfg, rays, seed, spec)

            leg = median_of(isx, call, a.calls, a.warmup)
            st = res["r"][3]
            leg["ratio_to_fluxmap_trace"] = leg["single_ms"] / yard
            leg["minus_fluxmap_trace_ms"] = leg["single_ms"] - yard
            leg["increments_per_ray"] = st.bin_increments / rays
            row[leg_name] = leg
            row["wall_hits_per_ray"] = st.wall_hits / rays
        isx.set_option("assist", 1)
        out[name] = row
    isx.shutdown()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
