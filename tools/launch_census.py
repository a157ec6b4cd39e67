"""One call of every ray-launching entry point, in a fixed order, for a kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/launch_census.py
    python tools/launch_census.py --summarize DIR > launches.txt

(kernel trace alone: no counters, no other tracing).  The summary is the sequence of (kernel, grid, workgroup, LDS bytes) in
dispatch order per queue; two builds of the library that plan their launches alike give the same file, whatever the clock says.
Only the public Python API is used, so the same file runs against any build.  The trace's LDS column holds the static LDS only
(0 for this library); the dynamic LDS of every launch is in the HIP runtime's own log: run the script under AMD_LOG_LEVEL=3,
without the profiler, and compare the `hipLaunchKernel ( ... )` lines with their pointers masked.

pipeline_chunk is 65536 and every call has 200 000 rays, so every call is cut into four launches (pairs of launches on the
pipelines).  The flux map is called again under each overlap setting and with the fate scan forced on; every scene-map call
again in its global form.
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SEED, CHUNK = 200000, 12345, 65536


def census():
    import torch   # (before the library: one HIP runtime in the process, as in bench.py)
    sys.path.insert(0, ROOT)
    import altair_raytracing_amd as isx

    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    isx.load()
    isx.init(0)
    isx.set_option("pipeline_chunk", CHUNK)
    cfg = isx.default_config()
    nb = cfg.n_theta * cfg.n_phi
    buf = [torch.zeros(1 << 20, dtype=torch.int64, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    a, b, c = (t.data_ptr() for t in buf)

    def done():
        isx.sync()
        isx.take_stats()

    # ---- the flux map: blocking, enqueued (the call overlap), the overlap settings, the fate scan forced on
    isx.fluxmap(cfg, N, SEED)
    isx.fluxmap_device(cfg, N, SEED, 0, a)
    isx.fluxmap_device(cfg, N, SEED, N, a)
    done()
    for key, values in (("call_overlap", (0, 1)), ("call_overlap_streams", (1, 2)), ("overlap", (2, 3, 0)),
                        ("overlap_trace_streams", (2, 1))):
        for v in values:
            isx.set_option(key, v)
            if key == "overlap_trace_streams":
                isx.set_option("overlap", 2)
            isx.fluxmap(cfg, N, SEED)
            isx.fluxmap_device(cfg, N, SEED, 0, a)
            done()
    isx.set_option("overlap", 0)
    isx.set_option("call_overlap", -1)
    isx.set_option("fate_scan", 1)
    isx.fluxmap(cfg, N, SEED)
    isx.fluxmap_device(cfg, N, SEED, 0, a)
    done()
    isx.set_option("fate_scan", -1)
    chord = cfg.copy()
    chord.trace_mode = 1
    isx.fluxmap(chord, N, SEED)
    brdf = cfg.copy()
    brdf.source_model = isx.SOURCE_BRDF
    isx.fluxmap(brdf, N, SEED)
    lobe = cfg.copy()
    lobe.surface_model = 1
    isx.fluxmap(lobe, N, SEED)
    rough = cfg.copy()
    rough.lambertian = 0
    isx.fluxmap(rough, N, SEED)
    compat = cfg.copy()
    compat.hit_line_mode = 1
    isx.fluxmap(compat, N, SEED)
    isx.fluxmap_series([cfg, chord], N, SEED)

    # ---- the older sinks
    discs = [[10.0 * k - 50.0, 0.0, -120.0, 0.0, 0.0, 1.0] for k in range(11)]
    isx.disc_sweep(cfg, discs, 4.0, 0.5, N, SEED)
    isx.disc_sweep_per_position(cfg, discs, 4.0, 0.5, N // len(discs), SEED)
    isx.exit_dz_hist(cfg, N, SEED)
    small = cfg.copy()
    small.n_theta, small.n_phi = 10, 10
    isx.fluxmap_per_position(small, N // 100, SEED)
    isx.fluxmap_per_position(small, N // 50, SEED, fold=2)
    isx.trace_rays_detector(cfg, [0.0, 0.0, -200.0, 0.0, 0.0, 1.0], 40.0, N, SEED)
    isx.exit_directions(cfg, N, SEED, capacity=1024)
    isx.trace_endstates(cfg, N, SEED)
    isx.fate_scan(cfg, N, SEED)

    # ---- the sinks with a spec: blocking and enqueued
    xm = isx.default_exit_map_spec(cfg)
    isx.exit_maps(cfg, N, SEED, xm)
    isx.exit_maps_device(cfg, xm, N, SEED, 0, a, b, c)
    wm = isx.default_wall_map_spec(cfg)
    isx.wall_map(cfg, N, SEED, wm)
    isx.wall_map_device(cfg, wm, N, SEED, 0, a, b)
    lf = isx.default_light_field_spec(cfg)
    isx.light_field(cfg, N, SEED, lf)
    isx.light_field_device(cfg, lf, N, SEED, 0, a, b)
    isx.set_option("lf_global", 1)
    isx.light_field(cfg, N, SEED, lf)
    isx.set_option("lf_global", 0)
    oh = isx.default_order_hist_spec(cfg)
    isx.order_hist(cfg, N, SEED, oh)
    isx.order_hist_device(cfg, oh, N, SEED, 0, a, b, c)
    done()

    patches = [isx.wall_patch_cap(cfg, (1, 0, 0), 5.0, 0.0), isx.wall_patch_cap(cfg, (0, 1, 0), 10.0, 0.5)]
    wp = isx.wall_patch_spec(cfg, patches)
    isx.wall_patches(cfg, N, SEED, wp)
    isx.wall_patches_device(cfg, wp, N, SEED, 0, a, b)
    beam = isx.beam_cone(cfg, (0, 0, 20), (0, 0, 1), 0.0, 180.0, isx.BEAM_UNIFORM)
    isx.beam_endstates(cfg, beam, N, SEED)
    isx.fluxmap_beam(cfg, beam, N, SEED)
    isx.fluxmap_beam_device(cfg, beam, N, SEED, 0, a)
    baffles = [isx.baffle_disc(cfg, (35, 0, 13), (1, 0, 0), 10.0, 0.9), isx.baffle_disc(cfg, (0, 0, -40), (0, 0, 1), 12.0, 0.9)]
    bf = isx.baffle_spec(cfg, baffles)
    isx.baffle_endstates(cfg, bf, N, SEED)
    isx.fluxmap_baffle(cfg, bf, N, SEED)
    isx.fluxmap_baffle_device(cfg, bf, N, SEED, 0, a, b)
    scene = isx.scene_spec(cfg, beam, baffles, patches)
    isx.scene_endstates(cfg, scene, N, SEED)
    isx.fluxmap_scene(cfg, scene, N, SEED)
    isx.fluxmap_scene_device(cfg, scene, N, SEED, 0, a, b)
    done()

    # ---- the scene maps: blocking and enqueued, then once more in the global form
    rs = isx.default_response_spec(cfg)
    vs = isx.view_frame(cfg, scene, 0, 32, 32, 1.0)
    fs = isx.patch_field_frame(cfg, scene, 1, 8, 8, 8, 8, 1.0)
    big = isx.patch_field_frame(cfg, scene, 1, 16, 16, 16, 16, 1.0)   # (a field no workgroup's LDS holds)
    os_ = isx.scene_order_spec(512)
    for form in (0, 1):
        isx.set_option("resp_global", form)
        isx.set_option("view_global", form)
        isx.set_option("field_global", form)
        isx.set_option("sorder_lds_orders", 0 if form else -1)
        isx.scene_response(cfg, scene, rs, N, SEED)
        isx.scene_response_device(cfg, scene, rs, N, SEED, 0, a, b)
        isx.scene_view(cfg, scene, vs, N, SEED)
        isx.scene_view_device(cfg, scene, vs, N, SEED, 0, a, b, c)
        isx.scene_patch_field(cfg, scene, fs, N, SEED)
        isx.scene_patch_field_device(cfg, scene, fs, N, SEED, 0, a, b, c)
        isx.scene_patch_field(cfg, scene, big, N, SEED)
        isx.scene_order_hist(cfg, scene, os_, N, SEED)
        isx.scene_order_hist_device(cfg, scene, os_, N, SEED, 0, a, b, c)
        done()
    isx.set_option("sorder_lds_orders", 7)
    isx.scene_order_hist(cfg, scene, os_, N, SEED)
    isx.set_option("sorder_lds_orders", -1)
    isx.shutdown()
    print("launch census done")


def summarize(path):
    files = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit("no *kernel_trace.csv under " + path)
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    lds = [k for k in rows[0] if "LDS" in k.upper()]
    queue = "Queue_Id" if "Queue_Id" in rows[0] else None
    rows = [r for r in rows if r["Kernel_Name"].startswith("isx_") or "isx::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: (int(r[queue]) if queue else 0, int(r["Dispatch_Id"])))
    queues = {}
    for r in rows:
        q = queues.setdefault(r[queue] if queue else "0", len(queues))   # (queue ids differ between runs: number them as met)
        name = r["Kernel_Name"].split("(")[0]
        print("q%d %s grid %s wg %s lds %s" % (q, name, r["Grid_Size_X"], r["Workgroup_Size_X"], "/".join(r[k] for k in lds)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        census()
