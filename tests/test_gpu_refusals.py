"""What every device-touching entry of libisx answers to an empty or a refused call: a characterisation table.

Each row is one call through the ctypes wrappers and the status it comes back with.  The expected statuses are literals recorded
from the library as it stood before its launch path was put behind one call descriptor (`python tests/test_gpu_refusals.py`
prints the table as the loaded library answers it); they pin, above all, the ORDER of the checks -- which status wins when two
things are wrong at once.  An empty call (n_rays = 0) is ISX_OK and leaves every output zero; nothing here launches more than
64 rays.

Device forms get their pointers from one hipMalloc'ed, zeroed block (through the HIP runtime libisx itself has mapped); no call of
the table may write to it, which is checked at the end.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK = 0                        # (the others: ISX_ERR_BAD_CONFIG -2, ISX_ERR_BAD_ARG -3, ISX_ERR_TOO_LARGE -6)
MAX_RAYS = 1 << 40            # ISX_MAX_RAYS_PER_CALL
MAX_ENDSTATES = 1 << 28       # the endstates / fate-scan entries' own limit
TOP = (1 << 64) - 1           # first_ray = TOP with n_rays >= 1: first + n is not representable
SEED = 7
DEV_WORDS = 1 << 16

# The statuses of the rows below that carry no literal of their own, as the library answered them before the change.
EXPECTED = {
    "fluxmap-fine-grid": -2, "fluxmap_device-fine-grid": -2, "fluxmap_device-fine-grid-and-overflow": -3,
    "fluxmap_device-fine-grid-and-too-large": -6, "fluxmap_beam-fine-grid-empty": -2, "fluxmap_beam-fine-grid": -2,
    "fluxmap_beam-fine-grid-and-bad-beam": -2, "fluxmap_beam_device-fine-grid-empty": -2, "fluxmap_beam_device-fine-grid": -2,
    "fluxmap_beam_device-fine-grid-and-bad-beam": -2, "fluxmap_beam_device-fine-grid-and-overflow": -3,
    "fluxmap_baffle-fine-grid-empty": -2, "fluxmap_baffle_device-fine-grid-and-bad-baffle": -2,
    "fluxmap_scene-fine-grid-empty": -2, "fluxmap_scene_device-fine-grid-and-overflow": -2, "scene_view-fine-grid-empty": 0,
    "fluxmap-full-grid": 0, "fluxmap_device-full-grid": 0, "fluxmap_device-full-grid-and-overflow": -3,
    "fluxmap_device-full-grid-and-too-large": -6, "fluxmap_beam-full-grid-empty": 0, "fluxmap_beam-full-grid": -2,
    "fluxmap_beam-full-grid-and-bad-beam": -2, "fluxmap_beam_device-full-grid-empty": 0, "fluxmap_beam_device-full-grid": -2,
    "fluxmap_beam_device-full-grid-and-bad-beam": -2, "fluxmap_beam_device-full-grid-and-overflow": -3,
    "fluxmap_baffle-full-grid-empty": -2, "fluxmap_baffle_device-full-grid-and-bad-baffle": -2,
    "fluxmap_scene-full-grid-empty": -2, "fluxmap_scene_device-full-grid-and-overflow": -2, "scene_view-full-grid-empty": 0,
    "fluxmap_beam-bad-beam-and-too-large": -2, "fluxmap_beam_device-bad-beam-and-null": -3, "fluxmap_beam-chord-mode": -2,
    "fluxmap_scene-bad-baffle-and-bad-patch": -2, "fluxmap_scene-bad-patch-and-overflow": -2,
    "fluxmap_scene-all-three-bad-and-too-large": -2, "fluxmap_scene_device-bad-baffle-and-bad-patch": -2,
    "fluxmap_scene_device-bad-patch-and-overflow": -2, "fluxmap_scene_device-all-three-bad-and-too-large": -2,
    "scene_endstates-bad-baffle-and-bad-patch": -2, "scene_endstates-bad-patch-and-overflow": -2,
    "scene_endstates-all-three-bad-and-too-large": -2, "scene_response-bad-baffle-and-bad-patch": -2,
    "scene_response-bad-patch-and-overflow": -2, "scene_response-all-three-bad-and-too-large": -2,
    "scene_view_device-bad-baffle-and-bad-patch": -2, "scene_view_device-bad-patch-and-overflow": -2,
    "scene_view_device-all-three-bad-and-too-large": -2, "scene_patch_field-bad-baffle-and-bad-patch": -2,
    "scene_patch_field-bad-patch-and-overflow": -2, "scene_patch_field-all-three-bad-and-too-large": -2,
    "scene_order_hist_device-bad-baffle-and-bad-patch": -2, "scene_order_hist_device-bad-patch-and-overflow": -2,
    "scene_order_hist_device-all-three-bad-and-too-large": -2, "scene_view-patch-past-the-end": -2,
    "scene_view-patch-past-the-end-and-overflow": -2, "scene_view_device-patch-past-the-end": -2,
    "scene_view_device-patch-past-the-end-and-null": -3, "scene_view-last-patch": 0,
    "scene_view-patch-past-the-end-and-bad-patch": -2, "scene_patch_field-patch-past-the-end": -2,
    "scene_patch_field-patch-past-the-end-and-too-large": -2, "scene_patch_field_device-patch-past-the-end": -2,
    "scene_patch_field_device-patch-past-the-end-and-null": -3, "scene_patch_field-last-patch": 0,
    "scene_view-skewed-frame": -2, "scene_patch_field-skewed-frame": -2, "scene_response-bad-spec-and-bad-patch": -2,
    "scene_order_hist-no-orders-and-overflow": -2, "fluxmap_per_position-fold2-odd-phi-empty": -2,
    "fluxmap_per_position-fold2-odd-phi": -2, "fluxmap_per_position-fold2-odd-phi-and-overflow": -3,
    "fluxmap_per_position-fold2-odd-phi-and-too-large": -6, "fluxmap_per_position-fold3-and-fine-grid": -2,
    "fluxmap_per_position-fold3": -3, "fluxmap_per_position-groups-past-the-end": -3, "fluxmap-bad-config-and-too-large": -2,
    "fluxmap_device-bad-config-and-overflow": -2, "fluxmap_device-null-and-bad-config": -3,
    "exit_dz_hist-too-many-bins-empty": -3, "exit_dz_hist-too-many-bins-and-too-large": -6,
    "exit_dz_hist-too-many-bins-and-bad-config": -2, "disc_sweep-too-many-discs-empty": -3,
    "disc_sweep-too-many-discs-and-overflow": -3, "disc_sweep-brdf-source-and-bad-radius": -2,
    "disc_sweep_per_position-too-many-discs": -3, "trace_rays_detector-no-width-and-bad-config": -3,
    "trace_rays_detector-bad-config-empty": -2, "exit_directions-no-room-and-bad-config": -2,
    "exit_directions-too-many-records": -6, "fluxmap_series-grids-differ-and-too-large": -2,
    "fluxmap_series-second-config-bad": -2, "exit_maps-bad-spec-and-too-large": -2, "exit_maps_device-bad-spec-empty": -2,
    "exit_maps_device-bad-spec-and-overflow": -3, "exit_maps_device-bad-spec-and-too-large": -6,
    "exit_maps_device-no-dir-map-empty": -3, "exit_maps_device-no-dir-map-and-bad-config": -2,
    "wall_map-bad-spec-and-bad-config": -2, "wall_map_device-bad-spec-empty": -2, "wall_map_device-bad-spec-and-overflow": -3,
    "wall_map_device-bad-spec-and-too-large": -6, "light_field_device-bad-spec-and-null": -3,
    "light_field_device-bad-spec-and-overflow": -2, "light_field-bad-config-and-overflow": -2,
    "order_hist_device-no-dz-array-and-bad-config": -3, "order_hist_device-bad-spec-and-overflow": -2,
    "order_hist-bad-config-and-too-large": -2, "wall_patches-bad-patch-and-too-large": -2,
    "wall_patches_device-chord-mode-and-overflow": -2, "wall_patches-zero-direction-and-overflow": -2,
    "fluxmap_baffle-bad-baffle-and-too-large": -2, "fluxmap_baffle_device-zero-direction-and-overflow": -2,
    "fluxmap_scene_device-zero-direction-empty": 0,
}


class _Ctx:
    """the library, small specs shared by the rows, and the zeroed device block"""

    def __init__(self, isx):
        self.isx = isx
        self.abi = isx.abi
        self.lib = isx.abi.load()
        # (the options a refusal looks at, at their defaults: the binning kernels' LDS next to a grid, the routes)
        for k, v in (("pipeline", 1), ("assist", 1), ("bin_mode", 1), ("bin_block", 512), ("disc_pipeline", 1),
                     ("surface_pipeline", 1), ("pipeline_chunk", 1 << 26), ("overlap", 0)):
            isx.set_option(k, v)
        with open("/proc/self/maps") as f:
            image = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})[0]
        self.hip = C.CDLL(image)
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), DEV_WORDS * 8) == 0
        assert self.hip.hipMemset(p, 0, DEV_WORDS * 8) == 0
        self.base = p.value

        self.cfg = self.config()
        c = self.cfg
        self.xm = isx.default_exit_map_spec(c)
        self.xm.n_u = self.xm.n_v = self.xm.n_x = self.xm.n_y = 8
        self.wm = isx.default_wall_map_spec(c)
        self.wm.n_x = self.wm.n_y = 8
        self.lf = isx.default_light_field_spec(c)
        self.lf.n_u = self.lf.n_v = self.lf.n_x = self.lf.n_y = 4
        self.oh = isx.default_order_hist_spec(c)
        self.oh.n_orders, self.oh.n_dz = 16, 2
        self.patches = [isx.wall_patch_cap(c, (1, 0, 0), 5.0, 0.0), isx.wall_patch_cap(c, (0, 1, 0), 10.0, 0.5)]
        self.wp = isx.wall_patch_spec(c, self.patches)
        self.beam = isx.beam_cone(c, (0, 0, 20), (0, 0, 1), 0.0, 180.0, isx.BEAM_UNIFORM)
        self.baffles = [isx.baffle_disc(c, (35, 0, 13), (1, 0, 0), 10.0, 0.9)]
        self.bf = isx.baffle_spec(c, self.baffles)
        self.scene = isx.scene_spec(c, self.beam, self.baffles, self.patches)
        self.rs = isx.response_spec(1, 1, 2, 3)
        self.vs = isx.view_frame(c, self.scene, 0, 4, 4, 1.0)
        self.fs = isx.patch_field_frame(c, self.scene, 0, 2, 2, 2, 2, 1.0)
        self.os = isx.scene_order_spec(8)
        self.discs = np.array([[0, 0, -120, 0, 0, 1], [10, 0, -120, 0, 0, 1]], dtype=np.float64)
        self.det = np.array([0, 0, -200, 0, 0, 1], dtype=np.float64)

    def config(self, **kw):
        c = self.isx.default_config()
        c.n_theta, c.n_phi = 6, 4
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def d(self, k):
        """device pointer k: 4096 words apart"""
        return self.base + k * 4096 * 8

    def device_words(self):
        out = np.empty(DEV_WORDS, dtype=np.uint64)
        self.isx.sync()
        assert self.hip.hipMemcpy(out.ctypes.data, self.base, DEV_WORDS * 8, 2) == 0
        return out

    def close(self):
        self.hip.hipFree(self.base)

    # specs with one thing wrong
    def bad_beam(self):
        b = self.beam.copy()
        b.axis[0] = 2.0
        return b

    def bad_baffles(self):
        b = self.bf.copy()
        b.baffle[0].radius = -1.0
        return b

    def bad_patches(self):
        p = self.wp.copy()
        p.patch[1].reflectance = 2.0
        return p

    def scene_with(self, beam=None, baffles=None, patches=None):
        s = self.scene.copy()
        for dst, src in ((s.beam, beam), (s.baffles, baffles), (s.patches, patches)):
            if src is not None:
                C.memmove(C.byref(dst), C.byref(src), C.sizeof(src))
        return s

    def view(self, patch):
        v = self.vs.copy()
        v.patch = patch
        return v

    def field(self, patch):
        f = self.fs.copy()
        f.patch = patch
        return f


def _endstates_raw(x, entry, spec, n, first):
    """the endstates entries with n beyond what a wrapper could allocate: refused before anything is written"""
    i4, f8 = (C.c_int32 * 4)(), (C.c_double * 12)()
    args = [C.byref(x.cfg)] + ([C.byref(spec)] if spec is not None else []) + [n, SEED, first, i4, i4, f8, f8]
    extra = {"isx_trace_endstates": [], "isx_beam_endstates": [f8, f8], "isx_baffle_endstates": [i4],
             "isx_scene_endstates": [f8, f8, i4, i4]}[entry]
    rc = getattr(x.lib, entry)(*(args + extra))
    if rc:
        raise x.abi.IsxError(rc, entry)


def _fate_raw(x, n, first):
    i4 = (C.c_int32 * 4)()
    rc = x.lib.isx_fate_scan(C.byref(x.cfg), n, SEED, first, i4, i4)
    if rc:
        raise x.abi.IsxError(rc, "isx_fate_scan")


def _rows():
    """(id, expected status, call).  call(x) -> the outputs of the call (checked to be zero for the rows named -empty)."""
    R = []

    def row(name, expected, fn):
        R.append((name, EXPECTED[name] if expected is None else expected, fn))

    def trio(name, ok, fn, too_large=MAX_RAYS + 1, first=TOP):
        """the four rows every entry has: fn(x, n_rays, first_ray); ok: their statuses"""
        row(name + "-empty", ok[0], lambda x: fn(x, 0, 0))
        row(name + "-too-large", ok[1], lambda x: fn(x, too_large, 0))
        row(name + "-first-overflow", ok[2], lambda x: fn(x, 8, first))
        row(name + "-too-large-and-overflow", ok[3], lambda x: fn(x, too_large, first))

    # ---- the flux map and the sinks without a spec
    trio("fluxmap", (0, -6, -3, -6), lambda x, n, f: x.isx.fluxmap(x.cfg, n, SEED, f))
    trio("fluxmap_device", (0, -6, -3, -6), lambda x, n, f: x.isx.fluxmap_device(x.cfg, n, SEED, f, x.d(0)))
    trio("fluxmap_series", (0, -6, -3, -6), lambda x, n, f: x.isx.fluxmap_series([x.cfg, x.cfg], n, SEED, f))
    trio("exit_dz_hist", (0, -6, -3, -6), lambda x, n, f: x.isx.exit_dz_hist(x.cfg, n, SEED, 10, f))
    trio("disc_sweep", (0, -6, -3, -6), lambda x, n, f: x.isx.disc_sweep(x.cfg, x.discs, 4.0, 0.5, n, SEED, f))
    trio("trace_rays_detector", (0, -6, -3, -6), lambda x, n, f: x.isx.trace_rays_detector(x.cfg, x.det, 40.0, n, SEED, f))
    trio("exit_directions", (0, -6, -3, -6), lambda x, n, f: x.isx.exit_directions(x.cfg, n, SEED, f, capacity=4))
    # (per-position calls: the ray count is groups x rays per position)
    row("fluxmap_per_position-empty", 0, lambda x: x.isx.fluxmap_per_position(x.cfg, 4, SEED, n_groups=0))
    row("fluxmap_per_position-too-large", -6, lambda x: x.isx.fluxmap_per_position(x.cfg, MAX_RAYS, SEED, n_groups=2))
    row("fluxmap_per_position-first-overflow", -3, lambda x: x.isx.fluxmap_per_position(x.cfg, 4, SEED, n_groups=2, first_ray=TOP))
    row("disc_sweep_per_position-no-rays", -3, lambda x: x.isx.disc_sweep_per_position(x.cfg, x.discs, 4.0, 0.5, 0, SEED))
    row("disc_sweep_per_position-too-large", -6, lambda x: x.isx.disc_sweep_per_position(x.cfg, x.discs, 4.0, 0.5, MAX_RAYS, SEED))
    row("disc_sweep_per_position-first-overflow", -3,
        lambda x: x.isx.disc_sweep_per_position(x.cfg, x.discs, 4.0, 0.5, 4, SEED, TOP))
    # ---- the per-ray diagnostics (their own limit of 2^28 rays)
    trio("trace_endstates", (0, -6, 0, -6),   # (this entry has no test of the index range: eight rays wrap round)
         lambda x, n, f: x.isx.trace_endstates(x.cfg, n, SEED, f) if n <= 8 else _endstates_raw(x, "isx_trace_endstates", None, n, f),
         MAX_ENDSTATES + 1)
    trio("fate_scan", (0, -6, -3, -6), lambda x, n, f: x.isx.fate_scan(x.cfg, n, SEED, f) if n <= 8 else _fate_raw(x, n, f),
         MAX_ENDSTATES + 1)
    trio("beam_endstates", (0, -6, -3, -6),
         lambda x, n, f: x.isx.beam_endstates(x.cfg, x.beam, n, SEED, f) if n <= 8 else _endstates_raw(x, "isx_beam_endstates", x.beam, n, f),
         MAX_ENDSTATES + 1)
    trio("baffle_endstates", (0, -6, -3, -6),
         lambda x, n, f: x.isx.baffle_endstates(x.cfg, x.bf, n, SEED, f) if n <= 8 else _endstates_raw(x, "isx_baffle_endstates", x.bf, n, f),
         MAX_ENDSTATES + 1)
    trio("scene_endstates", (0, -6, -3, -6),
         lambda x, n, f: x.isx.scene_endstates(x.cfg, x.scene, n, SEED, f) if n <= 8 else _endstates_raw(x, "isx_scene_endstates", x.scene, n, f),
         MAX_ENDSTATES + 1)
    row("mathprobe-empty", -3, lambda x: x.isx.mathprobe(0, np.zeros(0)))
    # ---- the sinks with a spec, host and device forms
    trio("exit_maps", (0, -6, -3, -6), lambda x, n, f: x.isx.exit_maps(x.cfg, n, SEED, x.xm, f))
    trio("exit_maps_device", (0, -6, -3, -6), lambda x, n, f: x.isx.exit_maps_device(x.cfg, x.xm, n, SEED, f, x.d(0), x.d(1), x.d(2)))
    trio("wall_map", (0, -6, -3, -6), lambda x, n, f: x.isx.wall_map(x.cfg, n, SEED, x.wm, f))
    trio("wall_map_device", (0, -6, -3, -6), lambda x, n, f: x.isx.wall_map_device(x.cfg, x.wm, n, SEED, f, x.d(0), x.d(1)))
    trio("light_field", (0, -6, -3, -6), lambda x, n, f: x.isx.light_field(x.cfg, n, SEED, x.lf, f))
    trio("light_field_device", (0, -6, -3, -6), lambda x, n, f: x.isx.light_field_device(x.cfg, x.lf, n, SEED, f, x.d(0), x.d(1)))
    trio("order_hist", (0, -6, -3, -6), lambda x, n, f: x.isx.order_hist(x.cfg, n, SEED, x.oh, f))
    trio("order_hist_device", (0, -6, -3, -6), lambda x, n, f: x.isx.order_hist_device(x.cfg, x.oh, n, SEED, f, x.d(0), x.d(1), x.d(2)))
    trio("wall_patches", (0, -6, -3, -6), lambda x, n, f: x.isx.wall_patches(x.cfg, n, SEED, x.wp, f))
    trio("wall_patches_device", (0, -6, -3, -6), lambda x, n, f: x.isx.wall_patches_device(x.cfg, x.wp, n, SEED, f, x.d(0), x.d(1)))
    trio("fluxmap_beam", (0, -6, -3, -6), lambda x, n, f: x.isx.fluxmap_beam(x.cfg, x.beam, n, SEED, f))
    trio("fluxmap_beam_device", (0, -6, -3, -6), lambda x, n, f: x.isx.fluxmap_beam_device(x.cfg, x.beam, n, SEED, f, x.d(0)))
    trio("fluxmap_baffle", (0, -6, -3, -6), lambda x, n, f: x.isx.fluxmap_baffle(x.cfg, x.bf, n, SEED, f))
    trio("fluxmap_baffle_device", (0, -6, -3, -6), lambda x, n, f: x.isx.fluxmap_baffle_device(x.cfg, x.bf, n, SEED, f, x.d(0), x.d(1)))
    trio("fluxmap_scene", (0, -6, -3, -6), lambda x, n, f: x.isx.fluxmap_scene(x.cfg, x.scene, n, SEED, f))
    trio("fluxmap_scene_device", (0, -6, -3, -6), lambda x, n, f: x.isx.fluxmap_scene_device(x.cfg, x.scene, n, SEED, f, x.d(0), x.d(1)))
    trio("scene_response", (0, -6, -3, -6), lambda x, n, f: x.isx.scene_response(x.cfg, x.scene, x.rs, n, SEED, f))
    trio("scene_response_device", (0, -6, -3, -6),
         lambda x, n, f: x.isx.scene_response_device(x.cfg, x.scene, x.rs, n, SEED, f, x.d(0), x.d(1)))
    trio("scene_view", (0, -6, -3, -6), lambda x, n, f: x.isx.scene_view(x.cfg, x.scene, x.vs, n, SEED, f))
    trio("scene_view_device", (0, -6, -3, -6),
         lambda x, n, f: x.isx.scene_view_device(x.cfg, x.scene, x.vs, n, SEED, f, x.d(0), x.d(1), x.d(2)))
    trio("scene_patch_field", (0, -6, -3, -6), lambda x, n, f: x.isx.scene_patch_field(x.cfg, x.scene, x.fs, n, SEED, f))
    trio("scene_patch_field_device", (0, -6, -3, -6),
         lambda x, n, f: x.isx.scene_patch_field_device(x.cfg, x.scene, x.fs, n, SEED, f, x.d(0), x.d(1), x.d(2)))
    trio("scene_order_hist", (0, -6, -3, -6), lambda x, n, f: x.isx.scene_order_hist(x.cfg, x.scene, x.os, n, SEED, f))
    trio("scene_order_hist_device", (0, -6, -3, -6),
         lambda x, n, f: x.isx.scene_order_hist_device(x.cfg, x.scene, x.os, n, SEED, f, x.d(0), x.d(1), x.d(2)))
    # ---- the injected-record entries (no ray count: an empty list, and one record too many)
    row("bin_injected_lines-empty", 0, lambda x: x.isx.bin_injected_lines(x.cfg, x.isx.INJECT_FLUX, np.zeros((0, 3)), np.zeros((0, 3))))
    row("bin_injected_lines-maps-empty", 0,
        lambda x: x.isx.bin_injected_lines(x.cfg, x.isx.INJECT_EXIT_MAPS, np.zeros((0, 3)), np.zeros((0, 3)), x.xm))
    row("bin_injected_lines-field-empty", 0,
        lambda x: x.isx.bin_injected_lines(x.cfg, x.isx.INJECT_LIGHT_FIELD, np.zeros((0, 3)), np.zeros((0, 3)), x.lf))
    row("bin_injected_lines-bad-sink-and-bad-unit", -3,
        lambda x: x.isx.bin_injected_lines(x.cfg, 9, np.zeros((0, 3)), np.zeros((0, 3)), x.lf, unit=5))
    row("bin_injected_lines-bad-unit-and-bad-config", -3,
        lambda x: x.isx.bin_injected_lines(x.config(r_out=1.0), x.isx.INJECT_FLUX, np.zeros((0, 3)), np.zeros((0, 3)), unit=5))
    row("bin_injected_lines-bad-spec-and-fine-grid", -2,
        lambda x: x.isx.bin_injected_lines(x.config(n_theta=190, n_phi=190), x.isx.INJECT_EXIT_MAPS, np.zeros((0, 3)), np.zeros((0, 3)),
                                           _with(x.xm, n_u=0)))
    row("bin_injected_segments-empty", 0, lambda x: x.isx.bin_injected_segments(x.cfg, x.discs, 4.0, 0.5, np.zeros((0, 7))))
    row("bin_injected_segments-bad-radius-and-brdf-source", -3,
        lambda x: x.isx.bin_injected_segments(x.config(source_model=x.isx.SOURCE_BRDF), x.discs, -1.0, 0.5, np.zeros((0, 7))))
    row("bin_injected_segments-brdf-source", -2,
        lambda x: x.isx.bin_injected_segments(x.config(source_model=x.isx.SOURCE_BRDF), x.discs, 4.0, 0.5, np.zeros((0, 7))))

    # ---- two things wrong at once: the order of the checks
    fine = dict(n_theta=190, n_phi=190)      # 36100 bins: above the 36000 a workgroup's histogram may have
    full = dict(n_theta=180, n_phi=200)      # 36000 bins: within that limit, the tables next to the histogram are not
    for tag, grid in (("fine-grid", fine), ("full-grid", full)):
        row("fluxmap-%s" % tag, None, lambda x, g=grid: x.isx.fluxmap(x.config(**g), 0, SEED))
        row("fluxmap_device-%s" % tag, None, lambda x, g=grid: x.isx.fluxmap_device(x.config(**g), 0, SEED, 0, x.d(0)))
        row("fluxmap_device-%s-and-overflow" % tag, None, lambda x, g=grid: x.isx.fluxmap_device(x.config(**g), 8, SEED, TOP, x.d(0)))
        row("fluxmap_device-%s-and-too-large" % tag, None,
            lambda x, g=grid: x.isx.fluxmap_device(x.config(**g), MAX_RAYS + 1, SEED, 0, x.d(0)))
        row("fluxmap_beam-%s-empty" % tag, None, lambda x, g=grid: x.isx.fluxmap_beam(x.config(**g), x.beam, 0, SEED))
        row("fluxmap_beam-%s" % tag, None, lambda x, g=grid: x.isx.fluxmap_beam(x.config(**g), x.beam, 8, SEED))
        row("fluxmap_beam-%s-and-bad-beam" % tag, None, lambda x, g=grid: x.isx.fluxmap_beam(x.config(**g), x.bad_beam(), 8, SEED))
        row("fluxmap_beam_device-%s-empty" % tag, None,
            lambda x, g=grid: x.isx.fluxmap_beam_device(x.config(**g), x.beam, 0, SEED, 0, x.d(0)))
        row("fluxmap_beam_device-%s" % tag, None, lambda x, g=grid: x.isx.fluxmap_beam_device(x.config(**g), x.beam, 8, SEED, 0, x.d(0)))
        row("fluxmap_beam_device-%s-and-bad-beam" % tag, None,
            lambda x, g=grid: x.isx.fluxmap_beam_device(x.config(**g), x.bad_beam(), 8, SEED, 0, x.d(0)))
        row("fluxmap_beam_device-%s-and-overflow" % tag, None,
            lambda x, g=grid: x.isx.fluxmap_beam_device(x.config(**g), x.beam, 8, SEED, TOP, x.d(0)))
        row("fluxmap_baffle-%s-empty" % tag, None, lambda x, g=grid: x.isx.fluxmap_baffle(x.config(**g), x.bf, 0, SEED))
        row("fluxmap_baffle_device-%s-and-bad-baffle" % tag, None,
            lambda x, g=grid: x.isx.fluxmap_baffle_device(x.config(**g), x.bad_baffles(), 0, SEED, 0, x.d(0), x.d(1)))
        row("fluxmap_scene-%s-empty" % tag, None, lambda x, g=grid: x.isx.fluxmap_scene(x.config(**g), x.scene, 0, SEED))
        row("fluxmap_scene_device-%s-and-overflow" % tag, None,
            lambda x, g=grid: x.isx.fluxmap_scene_device(x.config(**g), x.scene, 8, SEED, TOP, x.d(0), x.d(1)))
        row("scene_view-%s-empty" % tag, None, lambda x, g=grid: x.isx.scene_view(x.config(**g), x.scene, x.vs, 0, SEED))
    row("fluxmap_beam-bad-beam-and-too-large", None, lambda x: x.isx.fluxmap_beam(x.cfg, x.bad_beam(), MAX_RAYS + 1, SEED))
    row("fluxmap_beam_device-bad-beam-and-null", None, lambda x: x.isx.fluxmap_beam_device(x.cfg, x.bad_beam(), 0, SEED, 0, 0))
    row("fluxmap_beam-chord-mode", None, lambda x: x.isx.fluxmap_beam(x.config(trace_mode=1), x.beam, 0, SEED))
    # a scene with a bad baffle spec and a bad patch spec (and then a bad beam as well)
    for name, call in (
            ("fluxmap_scene", lambda x, s, n, f: x.isx.fluxmap_scene(x.cfg, s, n, SEED, f)),
            ("fluxmap_scene_device", lambda x, s, n, f: x.isx.fluxmap_scene_device(x.cfg, s, n, SEED, f, x.d(0), x.d(1))),
            ("scene_endstates", lambda x, s, n, f: x.isx.scene_endstates(x.cfg, s, n, SEED, f) if n <= 8 else
             _endstates_raw(x, "isx_scene_endstates", s, MAX_ENDSTATES + 1, f)),
            ("scene_response", lambda x, s, n, f: x.isx.scene_response(x.cfg, s, x.rs, n, SEED, f)),
            ("scene_view_device", lambda x, s, n, f: x.isx.scene_view_device(x.cfg, s, x.vs, n, SEED, f, x.d(0), x.d(1), x.d(2))),
            ("scene_patch_field", lambda x, s, n, f: x.isx.scene_patch_field(x.cfg, s, x.fs, n, SEED, f)),
            ("scene_order_hist_device", lambda x, s, n, f: x.isx.scene_order_hist_device(x.cfg, s, x.os, n, SEED, f, x.d(0), x.d(1), x.d(2)))):
        row(name + "-bad-baffle-and-bad-patch", None,
            lambda x, c=call: c(x, x.scene_with(baffles=x.bad_baffles(), patches=x.bad_patches()), 0, 0))
        row(name + "-bad-patch-and-overflow", None, lambda x, c=call: c(x, x.scene_with(patches=x.bad_patches()), 8, TOP))
        row(name + "-all-three-bad-and-too-large", None,
            lambda x, c=call: c(x, x.scene_with(x.bad_beam(), x.bad_baffles(), x.bad_patches()), MAX_RAYS + 1, 0))
    # a view or field patch index equal to n_patches
    row("scene_view-patch-past-the-end", None, lambda x: x.isx.scene_view(x.cfg, x.scene, x.view(2), 0, SEED))
    row("scene_view-patch-past-the-end-and-overflow", None, lambda x: x.isx.scene_view(x.cfg, x.scene, x.view(2), 8, SEED, TOP))
    row("scene_view_device-patch-past-the-end", None,
        lambda x: x.isx.scene_view_device(x.cfg, x.scene, x.view(2), 0, SEED, 0, x.d(0), x.d(1), x.d(2)))
    row("scene_view_device-patch-past-the-end-and-null", None,
        lambda x: x.isx.scene_view_device(x.cfg, x.scene, x.view(2), 0, SEED, 0, x.d(0), 0, x.d(2)))
    row("scene_view-last-patch", None, lambda x: x.isx.scene_view(x.cfg, x.scene, x.view(1), 0, SEED))
    row("scene_view-patch-past-the-end-and-bad-patch", None,
        lambda x: x.isx.scene_view(x.cfg, x.scene_with(patches=x.bad_patches()), x.view(2), 0, SEED))
    row("scene_patch_field-patch-past-the-end", None, lambda x: x.isx.scene_patch_field(x.cfg, x.scene, x.field(2), 0, SEED))
    row("scene_patch_field-patch-past-the-end-and-too-large", None,
        lambda x: x.isx.scene_patch_field(x.cfg, x.scene, x.field(2), MAX_RAYS + 1, SEED))
    row("scene_patch_field_device-patch-past-the-end", None,
        lambda x: x.isx.scene_patch_field_device(x.cfg, x.scene, x.field(2), 0, SEED, 0, x.d(0), x.d(1), x.d(2)))
    row("scene_patch_field_device-patch-past-the-end-and-null", None,
        lambda x: x.isx.scene_patch_field_device(x.cfg, x.scene, x.field(2), 0, SEED, 0, 0, x.d(1), x.d(2)))
    row("scene_patch_field-last-patch", None, lambda x: x.isx.scene_patch_field(x.cfg, x.scene, x.field(1), 0, SEED))
    row("scene_view-skewed-frame", None, lambda x: x.isx.scene_view(x.cfg, x.scene, _with(x.vs, e1=(1.0, 0.0, 0.0)), 0, SEED))
    row("scene_patch_field-skewed-frame", None,
        lambda x: x.isx.scene_patch_field(x.cfg, x.scene, _with(x.fs, e2=(0.0, 0.6, 0.8000001)), 0, SEED))
    row("scene_response-bad-spec-and-bad-patch", None,
        lambda x: x.isx.scene_response(x.cfg, x.scene_with(patches=x.bad_patches()), x.isx.response_spec(0, 1, 1, 1), 0, SEED))
    row("scene_order_hist-no-orders-and-overflow", None,
        lambda x: x.isx.scene_order_hist(x.cfg, x.scene, x.isx.scene_order_spec(0), 8, SEED, TOP))
    # SINK_PERPOS: fold = 2 over an odd number of azimuths
    odd = dict(n_theta=6, n_phi=5)
    row("fluxmap_per_position-fold2-odd-phi-empty", None, lambda x: x.isx.fluxmap_per_position(x.config(**odd), 4, SEED, fold=2, n_groups=0))
    row("fluxmap_per_position-fold2-odd-phi", None, lambda x: x.isx.fluxmap_per_position(x.config(**odd), 4, SEED, fold=2, n_groups=2))
    row("fluxmap_per_position-fold2-odd-phi-and-overflow", None,
        lambda x: x.isx.fluxmap_per_position(x.config(**odd), 4, SEED, fold=2, n_groups=2, first_ray=TOP))
    row("fluxmap_per_position-fold2-odd-phi-and-too-large", None,
        lambda x: x.isx.fluxmap_per_position(x.config(**odd), MAX_RAYS, SEED, fold=2, n_groups=2))
    row("fluxmap_per_position-fold3-and-fine-grid", None, lambda x: x.isx.fluxmap_per_position(x.config(**fine), 4, SEED, fold=3, n_groups=0))
    row("fluxmap_per_position-fold3", None, lambda x: x.isx.fluxmap_per_position(x.cfg, 4, SEED, fold=3, n_groups=0))
    row("fluxmap_per_position-groups-past-the-end", None, lambda x: x.isx.fluxmap_per_position(x.cfg, 4, SEED, first_group=20, n_groups=5))
    # a bad configuration next to a bad count, a bad spec or a bad list
    shell = dict(r_out=1.0)                  # r_out <= r_in: prepare_geom refuses it
    row("fluxmap-bad-config-and-too-large", None, lambda x: x.isx.fluxmap(x.config(**shell), MAX_RAYS + 1, SEED))
    row("fluxmap_device-bad-config-and-overflow", None, lambda x: x.isx.fluxmap_device(x.config(**shell), 8, SEED, TOP, x.d(0)))
    row("fluxmap_device-null-and-bad-config", None, lambda x: x.isx.fluxmap_device(x.config(**shell), 8, SEED, 0, 0))
    row("exit_dz_hist-too-many-bins-empty", None, lambda x: x.isx.exit_dz_hist(x.cfg, 0, SEED, 36001))
    row("exit_dz_hist-too-many-bins-and-too-large", None, lambda x: x.isx.exit_dz_hist(x.cfg, MAX_RAYS + 1, SEED, 36001))
    row("exit_dz_hist-too-many-bins-and-bad-config", None, lambda x: x.isx.exit_dz_hist(x.config(**shell), 0, SEED, 36001))
    row("disc_sweep-too-many-discs-empty", None, lambda x: x.isx.disc_sweep(x.cfg, _many_discs(), 0.01, 0.01, 0, SEED))
    row("disc_sweep-too-many-discs-and-overflow", None, lambda x: x.isx.disc_sweep(x.cfg, _many_discs(), 0.01, 0.01, 8, SEED, TOP))
    row("disc_sweep-brdf-source-and-bad-radius", None,
        lambda x: x.isx.disc_sweep(x.config(source_model=x.isx.SOURCE_BRDF), x.discs, -1.0, 0.5, 0, SEED))
    row("disc_sweep_per_position-too-many-discs", None, lambda x: x.isx.disc_sweep_per_position(x.cfg, _many_discs(), 0.01, 0.01, 1, SEED))
    row("trace_rays_detector-no-width-and-bad-config", None,
        lambda x: x.isx.trace_rays_detector(x.config(**shell), x.det, 0.0, 0, SEED))
    row("trace_rays_detector-bad-config-empty", None, lambda x: x.isx.trace_rays_detector(x.config(**shell), x.det, 40.0, 0, SEED))
    row("exit_directions-no-room-and-bad-config", None, lambda x: x.isx.exit_directions(x.config(**shell), 8, SEED, capacity=0))
    row("exit_directions-too-many-records", None, lambda x: _exit_directions_raw(x, 1 << 29, (1 << 28) + 1))
    row("fluxmap_series-grids-differ-and-too-large", None,
        lambda x: x.isx.fluxmap_series([x.cfg, x.config(n_phi=5)], MAX_RAYS + 1, SEED))
    row("fluxmap_series-second-config-bad", None, lambda x: x.isx.fluxmap_series([x.cfg, x.config(**shell)], 0, SEED))
    row("exit_maps-bad-spec-and-too-large", None, lambda x: x.isx.exit_maps(x.cfg, MAX_RAYS + 1, SEED, _with(x.xm, n_u=-1)))
    row("exit_maps_device-bad-spec-empty", None,
        lambda x: x.isx.exit_maps_device(x.cfg, _with(x.xm, n_u=-1), 0, SEED, 0, x.d(0), x.d(1), x.d(2)))
    row("exit_maps_device-bad-spec-and-overflow", None,
        lambda x: x.isx.exit_maps_device(x.cfg, _with(x.xm, n_u=-1), 8, SEED, TOP, x.d(0), x.d(1), x.d(2)))
    row("exit_maps_device-bad-spec-and-too-large", None,
        lambda x: x.isx.exit_maps_device(x.cfg, _with(x.xm, n_u=-1), MAX_RAYS + 1, SEED, 0, x.d(0), x.d(1), x.d(2)))
    row("exit_maps_device-no-dir-map-empty", None, lambda x: x.isx.exit_maps_device(x.cfg, x.xm, 0, SEED, 0, 0, x.d(1), x.d(2)))
    row("exit_maps_device-no-dir-map-and-bad-config", None,
        lambda x: x.isx.exit_maps_device(x.config(**shell), x.xm, 0, SEED, 0, 0, x.d(1), x.d(2)))
    row("wall_map-bad-spec-and-bad-config", None, lambda x: x.isx.wall_map(x.config(**shell), 0, SEED, _with(x.wm, n_x=0)))
    row("wall_map_device-bad-spec-empty", None, lambda x: x.isx.wall_map_device(x.cfg, _with(x.wm, n_x=0), 0, SEED, 0, x.d(0), x.d(1)))
    row("wall_map_device-bad-spec-and-overflow", None,
        lambda x: x.isx.wall_map_device(x.cfg, _with(x.wm, n_x=0), 8, SEED, TOP, x.d(0), x.d(1)))
    row("wall_map_device-bad-spec-and-too-large", None,
        lambda x: x.isx.wall_map_device(x.cfg, _with(x.wm, n_x=0), MAX_RAYS + 1, SEED, 0, x.d(0), x.d(1)))
    row("light_field_device-bad-spec-and-null", None, lambda x: x.isx.light_field_device(x.cfg, _with(x.lf, n_x=0), 0, SEED, 0, 0, x.d(1)))
    row("light_field_device-bad-spec-and-overflow", None,
        lambda x: x.isx.light_field_device(x.cfg, _with(x.lf, n_x=0), 8, SEED, TOP, x.d(0), x.d(1)))
    row("light_field-bad-config-and-overflow", None, lambda x: x.isx.light_field(x.config(**shell), 8, SEED, x.lf, TOP))
    row("order_hist_device-no-dz-array-and-bad-config", None,
        lambda x: x.isx.order_hist_device(x.config(**shell), x.oh, 0, SEED, 0, x.d(0), 0, x.d(2)))
    row("order_hist_device-bad-spec-and-overflow", None,
        lambda x: x.isx.order_hist_device(x.cfg, _with(x.oh, n_orders=0), 8, SEED, TOP, x.d(0), x.d(1), x.d(2)))
    row("order_hist-bad-config-and-too-large", None, lambda x: x.isx.order_hist(x.config(**shell), MAX_RAYS + 1, SEED, x.oh))
    row("wall_patches-bad-patch-and-too-large", None, lambda x: x.isx.wall_patches(x.cfg, MAX_RAYS + 1, SEED, x.bad_patches()))
    row("wall_patches_device-chord-mode-and-overflow", None,
        lambda x: x.isx.wall_patches_device(x.config(trace_mode=1), x.wp, 8, SEED, TOP, x.d(0), x.d(1)))
    row("wall_patches-zero-direction-and-overflow", None, lambda x: x.isx.wall_patches(x.config(dir=(C.c_double * 3)(0, 0, 0)), 8, SEED, x.wp, TOP))
    row("fluxmap_baffle-bad-baffle-and-too-large", None, lambda x: x.isx.fluxmap_baffle(x.cfg, x.bad_baffles(), MAX_RAYS + 1, SEED))
    row("fluxmap_baffle_device-zero-direction-and-overflow", None,
        lambda x: x.isx.fluxmap_baffle_device(x.config(dir=(C.c_double * 3)(0, 0, 0)), x.bf, 8, SEED, TOP, x.d(0), x.d(1)))
    row("fluxmap_scene_device-zero-direction-empty", None,
        lambda x: x.isx.fluxmap_scene_device(x.config(dir=(C.c_double * 3)(0, 0, 0)), x.scene, 0, SEED, 0, x.d(0), x.d(1)))
    return R


def _with(spec, **kw):
    s = spec.copy()
    for k, v in kw.items():
        if isinstance(v, tuple):
            for i, c in enumerate(v):
                getattr(s, k)[i] = c
        else:
            setattr(s, k, v)
    return s


_MANY = []


def _many_discs():
    """36001 discs: one more than a disc list may have"""
    if not _MANY:
        ca = np.zeros((36001, 6))
        ca[:, 0] = np.arange(36001) * 1e-3
        ca[:, 2], ca[:, 5] = -120.0, 1.0
        _MANY.append(ca)
    return _MANY[0]


def _exit_directions_raw(x, n, capacity):
    """a record capacity beyond what a wrapper could allocate: refused before anything is written"""
    u8, f8, cnt = (C.c_uint64 * 4)(), (C.c_double * 12)(), C.c_uint64(0)
    rc = x.lib.isx_exit_directions(C.byref(x.cfg), n, SEED, 0, capacity, u8, f8, C.byref(cnt), None)
    if rc:
        raise x.abi.IsxError(rc, "isx_exit_directions")


def _all_zero(out):
    if out is None:
        return True
    if isinstance(out, (tuple, list)):
        return all(_all_zero(o) for o in out)
    if isinstance(out, np.ndarray):
        return not out.any()
    if isinstance(out, (C.Structure, C.Array)):
        return not any(bytes(out))
    return out == 0


def _answer(x, fn):
    try:
        out = fn(x)
    except x.abi.IsxError as e:
        return e.status, None
    return OK, out


ROWS = _rows()


@pytest.fixture(scope="module")
def ctx(isx):
    x = _Ctx(isx)
    yield x
    x.close()


def test_row_names_are_unique():
    names = [r[0] for r in ROWS]
    assert len(names) == len(set(names))


def test_table(ctx):
    """every row at once (one library state, one pass: the rows are a few microseconds each)"""
    wrong = []
    for name, expected, fn in ROWS:
        status, out = _answer(ctx, fn)
        if status != expected:
            wrong.append((name, expected, status))
        elif name.endswith("-empty") and not _all_zero(out):
            wrong.append((name, "zero outputs", "something was written"))
    assert not wrong, wrong
    assert not ctx.device_words().any(), "a refused or empty call wrote to device memory"
    # the library still answers: a small flux map after the table
    hits, st = ctx.isx.fluxmap(ctx.cfg, 64, SEED)
    assert st.launched == 64


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import altair_raytracing_amd as m
    m.load()
    m.init(0)
    x = _Ctx(m)
    for name, expected, fn in ROWS:
        try:
            status, out = _answer(x, fn)
        except Exception as e:   # (a row the wrappers themselves cannot make)
            print("%-70s PYTHON %r" % (name, e))
            continue
        print("%-70s %4d %s %s" % (name, status, "" if expected is None or expected == status else "EXPECTED %s" % expected,
                                   "" if status or _all_zero(out) else "NONZERO"))
    print("device block zero:", not x.device_words().any())
    x.close()
    m.shutdown()
