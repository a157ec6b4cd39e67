#!/usr/bin/env python3
"""Times the port light field (isx_light_field) against the exit maps (isx_exit_maps, default spec: the yardstick -- the same
trace kernels, the binning kernel the light field's was modelled on).

usage: tools/time_light_field.py [--rays N] [--calls K] [--warmup W]

Headline configuration, one process, the legs interleaved round by round (every round runs each leg once), per leg the median,
minimum and maximum over K rounds after W warm-up rounds of stats.t_kernel_ms and of the trace / binning split of
isx_last_kernel_ms:
  exit_maps        isx_exit_maps, 128 x 128 + 64 x 64 bins
  lf_lds_2^14      isx_light_field, 8 x 8 x 16 x 16: the LDS form
  lf_global_2^16   isx_light_field, 16 x 16 x 16 x 16: the global form (one global u64 atomic add per binned ray)
  lf_global_2^20   32 x 32 x 32 x 32
  lf_global_2^22   64 x 64 x 32 x 32
and, for the global form, the atomic adds per second of the binning kernel (binned / bin_ms).  Prints one JSON object.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=float, default=5e7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    rays = int(a.rays)
    import altair_raytracing_amd as isx
    isx.load()
    isx.init(0)
    cfg = isx.default_config()
    seed = 0x5EED0001
    legs = {}

    def field_leg(n_x, n_y, n_u, n_v):
        s = isx.default_light_field_spec(cfg)
        s.n_x, s.n_y, s.n_u, s.n_v = n_x, n_y, n_u, n_v

        def run():
            _, k, st = isx.light_field(cfg, rays, seed, s)
            return st.t_kernel_ms, k.binned
        return run

    espec = isx.default_exit_map_spec(cfg)

    def exit_leg():
        _, _, k, st = isx.exit_maps(cfg, rays, seed, espec)
        return st.t_kernel_ms, k.dir_binned + k.pos_binned

    legs["exit_maps"] = exit_leg
    legs["lf_lds_2^14"] = field_leg(8, 8, 16, 16)
    legs["lf_global_2^16"] = field_leg(16, 16, 16, 16)
    legs["lf_global_2^20"] = field_leg(32, 32, 32, 32)
    legs["lf_global_2^22"] = field_leg(64, 64, 32, 32)
    rows = {name: [] for name in legs}
    for i in range(a.warmup + a.calls):
        for name, run in legs.items():
            t, binned = run()
            single, trace, binning = isx.last_kernel_ms()
            if i >= a.warmup:
                rows[name].append((t, trace, binning, binned, single))
    out = {"rays": rays, "calls": a.calls, "warmup": a.warmup, "device": isx.device_info()[0]}
    for name, r in rows.items():
        def col(k):
            v = [x[k] for x in r]
            return {"median": statistics.median(v), "min": min(v), "max": max(v)}
        leg = {"t_kernel_ms": col(0), "trace_ms": col(1), "bin_ms": col(2), "single_ms": col(4)["median"],
               "increments": r[0][3], "mrays_per_s": rays / col(0)["median"] / 1e3}
        if name.startswith("lf_global"):
            leg["atomics_per_s"] = r[0][3] / (col(2)["median"] * 1e-3)
        out[name] = leg
    isx.shutdown()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
