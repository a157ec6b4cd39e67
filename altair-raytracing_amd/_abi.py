"""ctypes binding of libisx.so (include/isx.h) — the only way Python reaches the GPU path.

There is no Python/NumPy compute fallback: if libisx.so is missing or no HIP device is
present, every compute call raises IsxError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("ISX_LIB_PATH") or os.path.join(CSRC, "libisx.so")  # ISX_LIB_PATH: tuning variants

OK = 0
ERR_NO_DEVICE = -1
ERR_BAD_CONFIG = -2
ERR_BAD_ARG = -3
ERR_HIP = -4
ERR_NOT_INIT = -5
ERR_TOO_LARGE = -6

SOURCE_PENCIL = 0
SOURCE_BRDF = 1

RAY_EXITED, RAY_ABSORBED, RAY_SUSPENDED = 1, 2, 3

WALL_MAP_MAX_BINS, WALL_MAP_MAX_AXIS = 8192, 512   # ISX_WALL_MAP_MAX_BINS / ISX_WALL_MAP_MAX_AXIS
LIGHT_FIELD_MAX_BINS, LIGHT_FIELD_MAX_AXIS = 1 << 22, 1024   # ISX_LIGHT_FIELD_MAX_BINS / ISX_LIGHT_FIELD_MAX_AXIS
ORDER_HIST_MAX_ORDERS, ORDER_HIST_MAX_WORDS, ORDER_HIST_MAX_DZ = 2048, 8192, 64   # ISX_ORDER_HIST_MAX_ORDERS / _MAX_WORDS, n_dz <= 64
MAX_WALL_PATCHES = 8   # ISX_MAX_WALL_PATCHES
BEAM_UNIFORM, BEAM_LAMBERT = 0, 1   # ISX_BEAM_UNIFORM / ISX_BEAM_LAMBERT
MAX_BAFFLES = 4   # ISX_MAX_BAFFLES
INJECT_FLUX, INJECT_EXIT_MAPS, INJECT_LIGHT_FIELD = 0, 1, 2   # ISX_INJECT_*: the sink of isx_bin_injected_lines
INJECT_UNIT_AUTO = -1                                          # ISX_INJECT_UNIT_AUTO (else 0: 256-line work units, 2: 64-line units)
INJECT_MAX_LINES, INJECT_MAX_REGIONS = 1 << 20, 1024   # (the flux sink also wants |P| <= sqrt(3) cfg.box_half)

# every symbol include/isx.h declares (tests check the .so exports exactly these)
EXPORTS = [
    "isx_default_config", "isx_init", "isx_shutdown", "isx_strerror", "isx_last_hip_error", "isx_abi_version", "isx_stream_version",
    "isx_device_info", "isx_fluxmap", "isx_fluxmap_device", "isx_sync", "isx_take_stats", "isx_stream",
    "isx_set_option", "isx_mathprobe", "isx_trace_endstates", "isx_fate_scan", "isx_fate_scan_launches", "isx_exit_scan_counts", "isx_disc_sweep", "isx_detector_table",
    "isx_exit_dz_hist", "isx_fluxmap_per_position", "isx_trace_rays_detector", "isx_exit_directions",
    "isx_fluxmap_series", "isx_disc_sweep_per_position", "isx_last_kernel_ms",
    "isx_default_exit_map_spec", "isx_exit_maps", "isx_exit_maps_device",
    "isx_default_wall_map_spec", "isx_wall_map", "isx_wall_map_device",
    "isx_default_light_field_spec", "isx_light_field", "isx_light_field_device", "isx_bin_injected_lines",
    "isx_bin_injected_segments",
    "isx_default_order_hist_spec", "isx_order_hist", "isx_order_hist_device", "isx_order_reweight",
    "isx_default_wall_patch_spec", "isx_wall_patch_cap", "isx_wall_patches", "isx_wall_patches_device",
    "isx_default_beam_spec", "isx_beam_cone", "isx_beam_endstates", "isx_fluxmap_beam", "isx_fluxmap_beam_device",
    "isx_default_baffle_spec", "isx_baffle_disc", "isx_baffle_endstates", "isx_fluxmap_baffle", "isx_fluxmap_baffle_device",
    "isx_default_scene_spec", "isx_scene_endstates", "isx_fluxmap_scene", "isx_fluxmap_scene_device",
    "isx_default_response_spec", "isx_scene_response", "isx_scene_response_device", "isx_response_reweight",
    "isx_view_frame", "isx_scene_view", "isx_scene_view_device", "isx_view_reweight", "isx_view_weight_fov",
    "isx_patch_field_frame", "isx_scene_patch_field", "isx_scene_patch_field_device", "isx_patch_field_marginals",
    "isx_default_scene_order_spec", "isx_scene_order_hist", "isx_scene_order_hist_device", "isx_scene_order_reweight",
    "isx_scene_order_moments",
    "isx_default_scene_path_spec", "isx_scene_path_hist", "isx_scene_path_hist_device", "isx_scene_path_moments",
    "isx_scene_path_decay",
]


class IsxError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = status
        msg = _lib.isx_strerror(status).decode() if _lib is not None else str(status)
        super().__init__(f"libisx {where}: {msg} (status {status})")


class Config(C.Structure):
    """isx_config (include/isx.h)."""

    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved0", C.c_uint32),
        ("r_in", C.c_double), ("r_out", C.c_double), ("theta_max_deg", C.c_double),
        ("reflectance", C.c_double), ("roughness_rad", C.c_double), ("box_half", C.c_double),
        ("lambertian", C.c_int32), ("max_points", C.c_int32),
        ("src", C.c_double * 3), ("dir", C.c_double * 3),
        ("n_theta", C.c_int32), ("n_phi", C.c_int32),
        ("det_diameter", C.c_double), ("det_distance", C.c_double), ("exit_port_z", C.c_double),
        ("source_model", C.c_int32), ("surface_model", C.c_int32),
        ("brdf", C.c_double * 3),
        ("hit_line_mode", C.c_int32), ("trace_mode", C.c_int32),
    ]

    def copy(self):
        c = Config()
        C.memmove(C.byref(c), C.byref(self), C.sizeof(Config))
        return c


class Stats(C.Structure):
    """isx_stats (include/isx.h)."""

    _fields_ = [
        ("launched", C.c_uint64), ("exited", C.c_uint64), ("counted_below_z", C.c_uint64),
        ("absorbed", C.c_uint64), ("suspended", C.c_uint64), ("bin_increments", C.c_uint64),
        ("wall_hits", C.c_uint64), ("t_kernel_ms", C.c_double),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ExitMapSpec(C.Structure):
    """isx_exit_map_spec (include/isx.h)."""

    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved0", C.c_uint32),
        ("n_u", C.c_int32), ("n_v", C.c_int32), ("n_x", C.c_int32), ("n_y", C.c_int32),
        ("plane_z", C.c_double), ("half_extent", C.c_double),
    ]

    def copy(self):
        s = ExitMapSpec()
        C.memmove(C.byref(s), C.byref(self), C.sizeof(ExitMapSpec))
        return s


class ExitMapCounts(C.Structure):
    """isx_exit_map_counts (include/isx.h)."""

    _fields_ = [(n, C.c_uint64) for n in ("dir_binned", "dir_outside", "pos_binned", "pos_outside", "upward")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class WallMapSpec(C.Structure):
    """isx_wall_map_spec (include/isx.h)."""

    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved0", C.c_uint32),
        ("n_x", C.c_int32), ("n_y", C.c_int32), ("first_order", C.c_int32), ("reserved1", C.c_int32),
    ]

    def copy(self):
        s = WallMapSpec()
        C.memmove(C.byref(s), C.byref(self), C.sizeof(WallMapSpec))
        return s


class WallMapCounts(C.Structure):
    """isx_wall_map_counts (include/isx.h)."""

    _fields_ = [(n, C.c_uint64) for n in ("binned", "outside", "skipped", "other_surface")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class LightFieldCounts(C.Structure):
    """isx_light_field_counts (include/isx.h)."""

    _fields_ = [(n, C.c_uint64) for n in ("binned", "pos_outside", "dir_outside", "upward")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class OrderHistSpec(C.Structure):
    """isx_order_hist_spec (include/isx.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("n_orders", C.c_int32), ("n_dz", C.c_int32)]

    def copy(self):
        s = OrderHistSpec()
        C.memmove(C.byref(s), C.byref(self), C.sizeof(OrderHistSpec))
        return s


class OrderHistCounts(C.Structure):
    """isx_order_hist_counts (include/isx.h): overflow per class (port, exited otherwise, absorbed, suspended), dz_outside."""

    _fields_ = [("overflow", C.c_uint64 * 4), ("dz_outside", C.c_uint64)]

    def as_dict(self):
        return {"overflow": [int(x) for x in self.overflow], "dz_outside": int(self.dz_outside)}


class WallPatch(C.Structure):
    """isx_wall_patch (include/isx.h): a cap of the inner wall -- q . axis >= min_dot -- with a reflectance of its own."""

    _fields_ = [("axis", C.c_double * 3), ("min_dot", C.c_double), ("reflectance", C.c_double)]


class WallPatchSpec(C.Structure):
    """isx_wall_patch_spec (include/isx.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("n_patches", C.c_int32), ("reserved1", C.c_int32),
                ("patch", WallPatch * MAX_WALL_PATCHES)]

    def copy(self):
        s = WallPatchSpec()
        C.memmove(C.byref(s), C.byref(self), C.sizeof(WallPatchSpec))
        return s


class BeamSpec(C.Structure):
    """isx_beam_spec (include/isx.h): the emitting disc, the frame (used as given), the cone and the angular law."""

    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("origin", C.c_double * 3), ("axis", C.c_double * 3),
                ("e1", C.c_double * 3), ("e2", C.c_double * 3), ("radius", C.c_double), ("cos_min", C.c_double),
                ("angular_law", C.c_int32), ("reserved1", C.c_int32)]

    def copy(self):
        s = BeamSpec()
        C.memmove(C.byref(s), C.byref(self), C.sizeof(BeamSpec))
        return s


class Baffle(C.Structure):
    """isx_baffle (include/isx.h): a two-sided disc inside the cavity; the normal is used as given, side 0 is the side it points to."""

    _fields_ = [("centre", C.c_double * 3), ("normal", C.c_double * 3), ("radius", C.c_double), ("reflectance", C.c_double)]


class BaffleSpec(C.Structure):
    """isx_baffle_spec (include/isx.h): up to MAX_BAFFLES discs."""

    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("n_baffles", C.c_int32), ("reserved1", C.c_int32),
                ("baffle", Baffle * MAX_BAFFLES)]

    def copy(self):
        s = BaffleSpec()
        C.memmove(C.byref(s), C.byref(self), C.sizeof(BaffleSpec))
        return s


class BaffleCounts(C.Structure):
    """isx_baffle_counts (include/isx.h): arrivals and absorbed rays per [baffle][side]."""

    _fields_ = [("arrivals", (C.c_uint64 * 2) * MAX_BAFFLES), ("absorbed", (C.c_uint64 * 2) * MAX_BAFFLES)]

    def arrays(self):
        """-> (arrivals[MAX_BAFFLES, 2], absorbed[MAX_BAFFLES, 2]) uint64"""
        a = np.array([[self.arrivals[k][s] for s in range(2)] for k in range(MAX_BAFFLES)], dtype=np.uint64)
        b = np.array([[self.absorbed[k][s] for s in range(2)] for k in range(MAX_BAFFLES)], dtype=np.uint64)
        return a, b


class SceneSpec(C.Structure):
    """isx_scene_spec (include/isx.h): the beam source, the baffles and the wall patches of one trace."""

    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("beam", BeamSpec), ("baffles", BaffleSpec),
                ("patches", WallPatchSpec)]

    def copy(self):
        s = SceneSpec()
        C.memmove(C.byref(s), C.byref(self), C.sizeof(SceneSpec))
        return s


class SceneCounts(C.Structure):
    """isx_scene_counts (include/isx.h): arrivals and absorbed rays per wall class and per [baffle][side]; 36 words."""

    _fields_ = [("patch_arrivals", C.c_uint64 * (MAX_WALL_PATCHES + 2)), ("patch_absorbed", C.c_uint64 * (MAX_WALL_PATCHES + 2)),
                ("baffle", BaffleCounts)]

    def arrays(self):
        """-> (patch_arrivals[MAX_WALL_PATCHES + 2], patch_absorbed[...], baffle arrivals[MAX_BAFFLES, 2], baffle absorbed[...]) uint64"""
        pa = np.array(list(self.patch_arrivals), dtype=np.uint64)
        pb = np.array(list(self.patch_absorbed), dtype=np.uint64)
        return (pa, pb) + self.baffle.arrays()

    def words(self):
        """-> the 36 words in the struct's order (the device form's layout)"""
        return np.frombuffer(bytes(self), dtype=np.uint64).copy()


SCENE_COUNT_WORDS = 2 * (MAX_WALL_PATCHES + 2) + 4 * MAX_BAFFLES   # sizeof(isx_scene_counts) / 8

RESPONSE_FATES, RESPONSE_MAX_AXIS, RESPONSE_MAX_BINS = 21, 1024, 4096
# the fate slots of isx_scene_response: wall classes 0 .. P + 1 first, then ...
RESPONSE_BAFFLE0, RESPONSE_PORT, RESPONSE_EXITED_OTHER, RESPONSE_SUSPENDED = 10, 18, 19, 20


class ResponseSpec(C.Structure):
    """isx_response_spec (include/isx.h): bins per axis of the source's sample space -- disc ring, disc azimuth, polar band,
    direction azimuth."""

    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("n", C.c_int32 * 4)]

    @property
    def bins(self):
        return int(self.n[0]) * int(self.n[1]) * int(self.n[2]) * int(self.n[3])


VIEW_MAX_AXIS, VIEW_MAX_BINS = 1024, 65536


class ViewSpec(C.Structure):
    """isx_view_spec (include/isx.h): the selected wall class (the detector), the map's size, the detector's frame -- used as
    given -- and the half extent of the map in direction cosines."""

    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("patch", C.c_int32), ("n_u", C.c_int32), ("n_v", C.c_int32),
                ("reserved1", C.c_int32), ("axis", C.c_double * 3), ("e1", C.c_double * 3), ("e2", C.c_double * 3),
                ("half_extent", C.c_double)]

    @property
    def bins(self):
        return int(self.n_u) * int(self.n_v)

    def copy(self):
        s = ViewSpec()
        C.memmove(C.byref(s), C.byref(self), C.sizeof(ViewSpec))
        return s


class ViewCounts(C.Structure):
    """isx_view_counts (include/isx.h): the selected rays by what became of them."""

    _fields_ = [("binned", C.c_uint64), ("outside", C.c_uint64), ("behind", C.c_uint64), ("direct", C.c_uint64)]

    def words(self):
        """-> the 4 words in the struct's order (the device form's layout)"""
        return np.frombuffer(bytes(self), dtype=np.uint64).copy()


PATCH_FIELD_MAX_AXIS, PATCH_FIELD_MAX_BINS = 1024, 1 << 22


class PatchFieldSpec(C.Structure):
    """isx_patch_field_spec (include/isx.h): the selected wall class, the four axis sizes of the field, the patch's frame and the
    scale of the position part -- both used as given -- and the half extent of the direction part in direction cosines."""

    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("patch", C.c_int32), ("n_x", C.c_int32), ("n_y", C.c_int32),
                ("n_u", C.c_int32), ("n_v", C.c_int32), ("reserved1", C.c_int32), ("axis", C.c_double * 3), ("e1", C.c_double * 3),
                ("e2", C.c_double * 3), ("half_extent", C.c_double), ("pos_scale", C.c_double)]

    @property
    def bins(self):
        return int(self.n_x) * int(self.n_y) * int(self.n_u) * int(self.n_v)

    def copy(self):
        s = PatchFieldSpec()
        C.memmove(C.byref(s), C.byref(self), C.sizeof(PatchFieldSpec))
        return s


class PatchFieldCounts(C.Structure):
    """isx_patch_field_counts (include/isx.h): the selected rays by what became of them."""

    _fields_ = [("binned", C.c_uint64), ("pos_outside", C.c_uint64), ("dir_outside", C.c_uint64), ("behind", C.c_uint64),
                ("direct", C.c_uint64)]

    def words(self):
        """-> the 5 words in the struct's order (the device form's layout)"""
        return np.frombuffer(bytes(self), dtype=np.uint64).copy()


SCENE_ORDER_MAX_ORDERS = 65536


class SceneOrderSpec(C.Structure):
    """isx_scene_order_spec (include/isx.h): orders 0 .. n_orders - 1 per fate slot."""

    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("n_orders", C.c_int32), ("reserved1", C.c_int32)]


class SceneOrderCounts(C.Structure):
    """isx_scene_order_counts (include/isx.h): per fate slot, the rays whose order is n_orders or more."""

    _fields_ = [("overflow", C.c_uint64 * RESPONSE_FATES)]

    def words(self):
        """-> the 21 words (the device form's layout)"""
        return np.frombuffer(bytes(self), dtype=np.uint64).copy()


SCENE_PATH_MAX_BINS = 65536
LIGHT_CM_PER_NS = 29.9792458


class ScenePathSpec(C.Structure):
    """isx_scene_path_spec (include/isx.h): bins 0 .. n_bins - 1 of width bin_cm per fate slot."""

    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("n_bins", C.c_int32), ("reserved1", C.c_int32),
                ("bin_cm", C.c_double)]


class ScenePathCounts(C.Structure):
    """isx_scene_path_counts (include/isx.h): per fate slot, the rays beyond the last bin and the sum of the bit patterns of L
    modulo 2^64."""

    _fields_ = [("overflow", C.c_uint64 * RESPONSE_FATES), ("checksum", C.c_uint64 * RESPONSE_FATES)]

    def words(self):
        """-> the 42 words (the device form's layout)"""
        return np.frombuffer(bytes(self), dtype=np.uint64).copy()


_lib = None


def load():
    """dlopen libisx.so; raises if it was not built (run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run `make -C {CSRC}` (or __graft_entry__.build()); "
                          "there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    u64, i32, i64, dbl, P = C.c_uint64, C.c_int32, C.c_int64, C.c_double, C.POINTER
    L.isx_default_config.argtypes = [P(Config)]
    L.isx_default_config.restype = None
    L.isx_init.argtypes = [C.c_int]
    L.isx_shutdown.restype = None
    L.isx_strerror.argtypes = [C.c_int]
    L.isx_strerror.restype = C.c_char_p
    L.isx_device_info.argtypes = [C.c_char_p, C.c_int]
    L.isx_fluxmap.argtypes = [P(Config), u64, u64, u64, P(u64), P(Stats)]
    L.isx_fluxmap_device.argtypes = [P(Config), u64, u64, u64, C.c_void_p]
    L.isx_take_stats.argtypes = [P(Stats)]
    L.isx_stream.restype = C.c_void_p
    L.isx_set_option.argtypes = [C.c_char_p, i64]
    L.isx_mathprobe.argtypes = [C.c_int, P(dbl), P(dbl), P(dbl), P(dbl), i32]
    L.isx_trace_endstates.argtypes = [P(Config), u64, u64, u64, P(i32), P(i32), P(dbl), P(dbl)]
    L.isx_fate_scan.argtypes = [P(Config), u64, u64, u64, P(i32), P(i32)]
    L.isx_fate_scan_launches.argtypes = [P(u64)]
    L.isx_exit_scan_counts.argtypes = [P(u64), P(u64), P(u64)]
    L.isx_disc_sweep.argtypes = [P(Config), P(dbl), i32, dbl, dbl, u64, u64, u64, P(u64), P(Stats)]
    L.isx_disc_sweep_per_position.argtypes = [P(Config), P(dbl), i32, dbl, dbl, u64, u64, u64, P(u64), P(Stats)]
    L.isx_last_kernel_ms.argtypes = [P(dbl), P(dbl), P(dbl)]
    L.isx_detector_table.argtypes = [P(Config), P(dbl)]
    L.isx_exit_dz_hist.argtypes = [P(Config), u64, u64, u64, i32, P(u64), P(Stats)]
    L.isx_fluxmap_per_position.argtypes = [P(Config), u64, i32, u64, u64, u64, u64, P(u64), P(Stats)]
    L.isx_trace_rays_detector.argtypes = [P(Config), P(dbl), dbl, u64, u64, u64, P(u64), P(Stats)]
    L.isx_exit_directions.argtypes = [P(Config), u64, u64, u64, u64, P(u64), P(dbl), P(u64), P(Stats)]
    L.isx_fluxmap_series.argtypes = [P(Config), i32, u64, u64, u64, P(u64), P(Stats)]
    L.isx_default_exit_map_spec.argtypes = [P(Config), P(ExitMapSpec)]
    L.isx_default_exit_map_spec.restype = None
    L.isx_exit_maps.argtypes = [P(Config), P(ExitMapSpec), u64, u64, u64, P(u64), P(u64), P(ExitMapCounts), P(Stats)]
    L.isx_exit_maps_device.argtypes = [P(Config), P(ExitMapSpec), u64, u64, u64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.isx_default_wall_map_spec.argtypes = [P(Config), P(WallMapSpec)]
    L.isx_default_wall_map_spec.restype = None
    L.isx_wall_map.argtypes = [P(Config), P(WallMapSpec), u64, u64, u64, P(u64), P(WallMapCounts), P(Stats)]
    L.isx_wall_map_device.argtypes = [P(Config), P(WallMapSpec), u64, u64, u64, C.c_void_p, C.c_void_p]
    L.isx_default_light_field_spec.argtypes = [P(Config), P(ExitMapSpec)]
    L.isx_default_light_field_spec.restype = None
    L.isx_light_field.argtypes = [P(Config), P(ExitMapSpec), u64, u64, u64, P(u64), P(LightFieldCounts), P(Stats)]
    L.isx_light_field_device.argtypes = [P(Config), P(ExitMapSpec), u64, u64, u64, C.c_void_p, C.c_void_p]
    L.isx_bin_injected_lines.argtypes = [P(Config), i32, P(ExitMapSpec), P(dbl), u64, P(C.c_uint32), i32, i32, P(u64), P(u64), P(u64),
                                         P(u64)]
    L.isx_bin_injected_segments.argtypes = [P(Config), P(dbl), i32, dbl, dbl, P(dbl), u64, P(C.c_uint32), i32, i32, P(u64), P(u64)]
    L.isx_default_order_hist_spec.argtypes = [P(Config), P(OrderHistSpec)]
    L.isx_default_order_hist_spec.restype = None
    L.isx_order_hist.argtypes = [P(Config), P(OrderHistSpec), u64, u64, u64, P(u64), P(u64), P(OrderHistCounts), P(Stats)]
    L.isx_order_hist_device.argtypes = [P(Config), P(OrderHistSpec), u64, u64, u64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.isx_order_reweight.argtypes = [P(Config), P(OrderHistSpec), P(u64), P(OrderHistCounts), u64, P(C.c_double), C.c_int32,
                                     P(C.c_double), P(C.c_double)]
    L.isx_default_wall_patch_spec.argtypes = [P(Config), P(WallPatchSpec)]
    L.isx_default_wall_patch_spec.restype = None
    L.isx_wall_patch_cap.argtypes = [P(Config), P(dbl), dbl, dbl, P(WallPatch)]
    L.isx_wall_patches.argtypes = [P(Config), P(WallPatchSpec), u64, u64, u64, P(u64), P(u64), P(Stats)]
    L.isx_wall_patches_device.argtypes = [P(Config), P(WallPatchSpec), u64, u64, u64, C.c_void_p, C.c_void_p]
    L.isx_default_beam_spec.argtypes = [P(Config), P(BeamSpec)]
    L.isx_default_beam_spec.restype = None
    L.isx_beam_cone.argtypes = [P(Config), P(dbl), P(dbl), dbl, dbl, i32, P(BeamSpec)]
    L.isx_beam_endstates.argtypes = [P(Config), P(BeamSpec), u64, u64, u64, P(i32), P(i32), P(dbl), P(dbl), P(dbl), P(dbl)]
    L.isx_fluxmap_beam.argtypes = [P(Config), P(BeamSpec), u64, u64, u64, P(u64), P(Stats)]
    L.isx_fluxmap_beam_device.argtypes = [P(Config), P(BeamSpec), u64, u64, u64, C.c_void_p]
    L.isx_default_baffle_spec.argtypes = [P(Config), P(BaffleSpec)]
    L.isx_default_baffle_spec.restype = None
    L.isx_baffle_disc.argtypes = [P(Config), P(dbl), P(dbl), dbl, dbl, P(Baffle)]
    L.isx_baffle_endstates.argtypes = [P(Config), P(BaffleSpec), u64, u64, u64, P(i32), P(i32), P(dbl), P(dbl), P(i32)]
    L.isx_fluxmap_baffle.argtypes = [P(Config), P(BaffleSpec), u64, u64, u64, P(u64), P(BaffleCounts), P(Stats)]
    L.isx_fluxmap_baffle_device.argtypes = [P(Config), P(BaffleSpec), u64, u64, u64, C.c_void_p, C.c_void_p]
    L.isx_default_scene_spec.argtypes = [P(Config), P(SceneSpec)]
    L.isx_default_scene_spec.restype = None
    L.isx_scene_endstates.argtypes = [P(Config), P(SceneSpec), u64, u64, u64, P(i32), P(i32), P(dbl), P(dbl), P(dbl), P(dbl), P(i32),
                                      P(i32)]
    L.isx_fluxmap_scene.argtypes = [P(Config), P(SceneSpec), u64, u64, u64, P(u64), P(SceneCounts), P(Stats)]
    L.isx_fluxmap_scene_device.argtypes = [P(Config), P(SceneSpec), u64, u64, u64, C.c_void_p, C.c_void_p]
    L.isx_default_response_spec.argtypes = [P(Config), P(ResponseSpec)]
    L.isx_default_response_spec.restype = None
    L.isx_scene_response.argtypes = [P(Config), P(SceneSpec), P(ResponseSpec), u64, u64, u64, P(u64), P(SceneCounts), P(Stats)]
    L.isx_scene_response_device.argtypes = [P(Config), P(SceneSpec), P(ResponseSpec), u64, u64, u64, C.c_void_p, C.c_void_p]
    L.isx_response_reweight.argtypes = [P(ResponseSpec), P(u64), P(dbl), P(dbl), P(dbl)]
    L.isx_view_frame.argtypes = [P(Config), P(SceneSpec), i32, i32, i32, dbl, P(ViewSpec)]
    L.isx_scene_view.argtypes = [P(Config), P(SceneSpec), P(ViewSpec), u64, u64, u64, P(u64), P(ViewCounts), P(SceneCounts), P(Stats)]
    L.isx_scene_view_device.argtypes = [P(Config), P(SceneSpec), P(ViewSpec), u64, u64, u64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.isx_view_reweight.argtypes = [P(ViewSpec), P(u64), P(ViewCounts), u64, P(dbl), dbl, P(dbl), P(dbl)]
    L.isx_view_weight_fov.argtypes = [P(ViewSpec), dbl, P(dbl)]
    L.isx_patch_field_frame.argtypes = [P(Config), P(SceneSpec), i32, i32, i32, i32, i32, dbl, P(PatchFieldSpec)]
    L.isx_scene_patch_field.argtypes = [P(Config), P(SceneSpec), P(PatchFieldSpec), u64, u64, u64, P(u64), P(PatchFieldCounts),
                                        P(SceneCounts), P(Stats)]
    L.isx_scene_patch_field_device.argtypes = [P(Config), P(SceneSpec), P(PatchFieldSpec), u64, u64, u64, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
    L.isx_patch_field_marginals.argtypes = [P(PatchFieldSpec), P(u64), P(u64), P(u64)]
    L.isx_default_scene_order_spec.argtypes = [P(Config), P(SceneOrderSpec)]
    L.isx_default_scene_order_spec.restype = None
    L.isx_scene_order_hist.argtypes = [P(Config), P(SceneSpec), P(SceneOrderSpec), u64, u64, u64, P(u64), P(SceneOrderCounts),
                                       P(SceneCounts), P(Stats)]
    L.isx_scene_order_hist_device.argtypes = [P(Config), P(SceneSpec), P(SceneOrderSpec), u64, u64, u64, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
    L.isx_scene_order_reweight.argtypes = [P(Config), P(SceneSpec), P(SceneOrderSpec), P(u64), P(SceneOrderCounts), u64, P(dbl), i32,
                                           P(dbl), P(dbl)]
    L.isx_scene_order_moments.argtypes = [P(SceneOrderSpec), P(u64), P(SceneOrderCounts), P(dbl), P(dbl)]
    L.isx_default_scene_path_spec.argtypes = [P(Config), P(ScenePathSpec)]
    L.isx_default_scene_path_spec.restype = None
    L.isx_scene_path_hist.argtypes = [P(Config), P(SceneSpec), P(ScenePathSpec), u64, u64, u64, P(u64), P(ScenePathCounts),
                                      P(SceneCounts), P(Stats)]
    L.isx_scene_path_hist_device.argtypes = [P(Config), P(SceneSpec), P(ScenePathSpec), u64, u64, u64, C.c_void_p, C.c_void_p,
                                             C.c_void_p]
    L.isx_scene_path_moments.argtypes = [P(ScenePathSpec), P(u64), P(ScenePathCounts), P(dbl), P(dbl)]
    L.isx_scene_path_decay.argtypes = [P(ScenePathSpec), P(u64), P(ScenePathCounts), i32, i32, P(dbl), P(dbl)]
    _lib = L
    return L


def _chk(rc, where):
    if rc != OK:
        raise IsxError(rc, where)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def default_config():
    c = Config()
    load().isx_default_config(C.byref(c))
    return c


def init(device=0):
    _chk(load().isx_init(int(device)), "isx_init")


def shutdown():
    load().isx_shutdown()


def device_info():
    buf = C.create_string_buffer(256)
    cu = load().isx_device_info(buf, 256)
    if cu < 0:
        raise IsxError(cu, "isx_device_info")
    return buf.value.decode(), cu


def set_option(key, value):
    _chk(load().isx_set_option(key.encode(), int(value)), f"isx_set_option({key})")


def fluxmap(cfg, n_rays, seed, first_ray=0):
    """-> (hits[n_theta, n_phi] uint64, Stats).  Host-buffer form of the ABI."""
    hits = np.zeros(cfg.n_theta * cfg.n_phi, dtype=np.uint64)
    st = Stats()
    _chk(load().isx_fluxmap(C.byref(cfg), int(n_rays), int(seed), int(first_ray), _p(hits, C.c_uint64), C.byref(st)),
         "isx_fluxmap")
    return hits.reshape(cfg.n_theta, cfg.n_phi), st


def fluxmap_device(cfg, n_rays, seed, first_ray, d_hits_ptr):
    """Enqueue on the library stream, accumulating into device memory at d_hits_ptr."""
    _chk(load().isx_fluxmap_device(C.byref(cfg), int(n_rays), int(seed), int(first_ray), C.c_void_p(int(d_hits_ptr))),
         "isx_fluxmap_device")


def sync():
    _chk(load().isx_sync(), "isx_sync")


def take_stats():
    st = Stats()
    _chk(load().isx_take_stats(C.byref(st)), "isx_take_stats")
    return st


def trace_endstates(cfg, n, seed, first_ray=0):
    status = np.zeros(n, dtype=np.int32)
    npts = np.zeros(n, dtype=np.int32)
    lp = np.zeros((n, 3), dtype=np.float64)
    d = np.zeros((n, 3), dtype=np.float64)
    _chk(load().isx_trace_endstates(C.byref(cfg), int(n), int(seed), int(first_ray), _p(status, C.c_int32),
                                    _p(npts, C.c_int32), _p(lp, C.c_double), _p(d, C.c_double)), "isx_trace_endstates")
    return status, npts, lp, d


def fate_scan(cfg, n, seed, first_ray=0):
    """-> (fate, order): the "fate_scan" rule per ray (include/isx.h: isx_fate_scan) -- fate 2: settled as absorbed at interaction
    order; fate 0: left to the trace kernel, undecided at interaction order."""
    fate = np.zeros(n, dtype=np.int32)
    order = np.zeros(n, dtype=np.int32)
    _chk(load().isx_fate_scan(C.byref(cfg), int(n), int(seed), int(first_ray), _p(fate, C.c_int32), _p(order, C.c_int32)),
         "isx_fate_scan")
    return fate, order


def fate_scan_launches():
    """chunks that took the fate scan since init() (include/isx.h: isx_fate_scan_launches)"""
    n = C.c_uint64(0)
    _chk(load().isx_fate_scan_launches(C.byref(n)), "isx_fate_scan_launches")
    return int(n.value)


def exit_scan_counts():
    """-> (accepted, list_b, redo) of the "exit_scan" path since init() (include/isx.h: isx_exit_scan_counts)"""
    a, b, r = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _chk(load().isx_exit_scan_counts(C.byref(a), C.byref(b), C.byref(r)), "isx_exit_scan_counts")
    return int(a.value), int(b.value), int(r.value)


def disc_sweep(cfg, centers_axes, radius, half_thick, n_rays, seed, first_ray=0):
    ca = np.ascontiguousarray(centers_axes, dtype=np.float64)
    nd = ca.shape[0]
    hits = np.zeros(nd, dtype=np.uint64)
    st = Stats()
    _chk(load().isx_disc_sweep(C.byref(cfg), _p(ca, C.c_double), nd, float(radius), float(half_thick), int(n_rays),
                               int(seed), int(first_ray), _p(hits, C.c_uint64), C.byref(st)), "isx_disc_sweep")
    return hits, st


def last_kernel_ms():
    """(single, trace, bin) HIP-event milliseconds of the launches collected by the last blocking call / take_stats()."""
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    _chk(load().isx_last_kernel_ms(C.byref(a), C.byref(b), C.byref(c)), "isx_last_kernel_ms")
    return a.value, b.value, c.value


def disc_sweep_per_position(cfg, centers_axes, radius, half_thick, rays_per_position, seed, first_ray=0):
    """One launch for the reference's per-position disc loop: disc k sees only its own rays."""
    ca = np.ascontiguousarray(centers_axes, dtype=np.float64)
    nd = ca.shape[0]
    hits = np.zeros(nd, dtype=np.uint64)
    st = Stats()
    _chk(load().isx_disc_sweep_per_position(C.byref(cfg), _p(ca, C.c_double), nd, float(radius), float(half_thick),
                                            int(rays_per_position), int(seed), int(first_ray), _p(hits, C.c_uint64),
                                            C.byref(st)), "isx_disc_sweep_per_position")
    return hits, st


def exit_dz_hist(cfg, n_rays, seed, nbins=100, first_ray=0):
    hist = np.zeros(nbins, dtype=np.uint64)
    st = Stats()
    _chk(load().isx_exit_dz_hist(C.byref(cfg), int(n_rays), int(seed), int(first_ray), int(nbins),
                                 _p(hist, C.c_uint64), C.byref(st)), "isx_exit_dz_hist")
    return hist, st


def fluxmap_per_position(cfg, rays_per_position, seed, fold=1, first_group=0, n_groups=None, first_ray=0):
    nb = cfg.n_theta * cfg.n_phi
    if n_groups is None:
        n_groups = nb // fold - first_group
    hits = np.zeros(nb, dtype=np.uint64)
    st = Stats()
    _chk(load().isx_fluxmap_per_position(C.byref(cfg), int(rays_per_position), int(fold), int(first_group), int(n_groups),
                                         int(seed), int(first_ray), _p(hits, C.c_uint64), C.byref(st)),
         "isx_fluxmap_per_position")
    return hits.reshape(cfg.n_theta, cfg.n_phi), st


def trace_rays_detector(cfg, detector, width, n_rays, seed, first_ray=0):
    det = np.ascontiguousarray(detector, dtype=np.float64).reshape(6)
    h = C.c_uint64(0)
    st = Stats()
    _chk(load().isx_trace_rays_detector(C.byref(cfg), _p(det, C.c_double), float(width), int(n_rays), int(seed),
                                        int(first_ray), C.byref(h), C.byref(st)), "isx_trace_rays_detector")
    return int(h.value), st


def exit_directions(cfg, n_rays, seed, first_ray=0, capacity=None):
    """-> (ray_ids[k], directions[k,3], total_count, Stats); k = min(total_count, capacity)."""
    cap = int(capacity or n_rays)
    ids = np.zeros(cap, dtype=np.uint64)
    d = np.zeros((cap, 3), dtype=np.float64)
    cnt = C.c_uint64(0)
    st = Stats()
    _chk(load().isx_exit_directions(C.byref(cfg), int(n_rays), int(seed), int(first_ray), cap, _p(ids, C.c_uint64),
                                    _p(d, C.c_double), C.byref(cnt), C.byref(st)), "isx_exit_directions")
    k = min(int(cnt.value), cap)
    return ids[:k], d[:k], int(cnt.value), st


def default_exit_map_spec(cfg):
    """128 x 128 direction bins, 64 x 64 plane bins at the port plane over the port radius + 25 % (no GPU needed)."""
    s = ExitMapSpec()
    load().isx_default_exit_map_spec(C.byref(cfg), C.byref(s))
    return s


def exit_maps(cfg, n_rays, seed, spec=None, first_ray=0):
    """-> (dir_map[n_v, n_u], pos_map[n_y, n_x] uint64, ExitMapCounts, Stats): the 2-D histogram of the exit direction
    (dx, dy) and of the point where the exit line crosses the plane z = spec.plane_z (include/isx.h).  A map the spec
    does not want comes back with shape (0, 0)."""
    if spec is None:
        spec = default_exit_map_spec(cfg)
    dmap = np.zeros(max(spec.n_u * spec.n_v, 0), dtype=np.uint64)
    pmap = np.zeros(max(spec.n_x * spec.n_y, 0), dtype=np.uint64)
    cnt, st = ExitMapCounts(), Stats()
    _chk(load().isx_exit_maps(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray),
                              _p(dmap, C.c_uint64) if dmap.size else None, _p(pmap, C.c_uint64) if pmap.size else None,
                              C.byref(cnt), C.byref(st)), "isx_exit_maps")
    return (dmap.reshape(spec.n_v, spec.n_u) if dmap.size else dmap.reshape(0, 0),
            pmap.reshape(spec.n_y, spec.n_x) if pmap.size else pmap.reshape(0, 0), cnt, st)


def exit_maps_device(cfg, spec, n_rays, seed, first_ray, d_dir_ptr, d_pos_ptr, d_counts_ptr):
    """Enqueue on the library stream, accumulating into device memory: uint64 maps at d_dir_ptr / d_pos_ptr (0 for a map
    the spec does not want) and five uint64 counters at d_counts_ptr (e.g. torch tensors' data_ptr())."""
    _chk(load().isx_exit_maps_device(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray),
                                     C.c_void_p(int(d_dir_ptr) or None), C.c_void_p(int(d_pos_ptr) or None),
                                     C.c_void_p(int(d_counts_ptr))), "isx_exit_maps_device")


def default_wall_map_spec(cfg):
    """64 x 64 bins, first_order 0 (no GPU needed)."""
    s = WallMapSpec()
    load().isx_default_wall_map_spec(C.byref(cfg), C.byref(s))
    return s


def wall_map(cfg, n_rays, seed, spec=None, first_ray=0):
    """-> (wall_map[n_y, n_x] uint64, WallMapCounts, Stats): the equal-area map of every mirror interaction on the inner
    sphere (include/isx.h)."""
    if spec is None:
        spec = default_wall_map_spec(cfg)
    wmap = np.zeros(max(spec.n_x * spec.n_y, 1), dtype=np.uint64)
    cnt, st = WallMapCounts(), Stats()
    _chk(load().isx_wall_map(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray), _p(wmap, C.c_uint64),
                             C.byref(cnt), C.byref(st)), "isx_wall_map")
    return wmap.reshape(spec.n_y, spec.n_x), cnt, st


def wall_map_device(cfg, spec, n_rays, seed, first_ray, d_map_ptr, d_counts_ptr):
    """Enqueue on the library stream, accumulating into device memory: the uint64 map at d_map_ptr and four uint64 counters
    at d_counts_ptr (e.g. torch tensors' data_ptr())."""
    _chk(load().isx_wall_map_device(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray),
                                    C.c_void_p(int(d_map_ptr) or None), C.c_void_p(int(d_counts_ptr) or None)), "isx_wall_map_device")


def default_light_field_spec(cfg):
    """32 x 32 position bins at the port plane over the exit maps' default extent, 32 x 32 direction bins (no GPU needed)."""
    s = ExitMapSpec()
    load().isx_default_light_field_spec(C.byref(cfg), C.byref(s))
    return s


def light_field(cfg, n_rays, seed, spec=None, first_ray=0):
    """-> (field[n_y, n_x, n_v, n_u] uint64, LightFieldCounts, Stats): the 4-D position-direction histogram of the port light
    over the plane z = spec.plane_z (include/isx.h); radiance = count / (N dx dy du dv)."""
    if spec is None:
        spec = default_light_field_spec(cfg)
    axes = (spec.n_y, spec.n_x, spec.n_v, spec.n_u)
    ok = all(1 <= a <= LIGHT_FIELD_MAX_AXIS for a in axes) and int(np.prod(axes, dtype=np.int64)) <= LIGHT_FIELD_MAX_BINS
    field = np.zeros(int(np.prod(axes, dtype=np.int64)) if ok else 1, dtype=np.uint64)   # (a refused spec: the library says so)
    cnt, st = LightFieldCounts(), Stats()
    _chk(load().isx_light_field(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray), _p(field, C.c_uint64),
                                C.byref(cnt), C.byref(st)), "isx_light_field")
    return field.reshape(axes), cnt, st


def light_field_device(cfg, spec, n_rays, seed, first_ray, d_field_ptr, d_counts_ptr):
    """Enqueue on the library stream, accumulating into device memory: the uint64 field at d_field_ptr and four uint64 counters
    at d_counts_ptr (e.g. torch tensors' data_ptr())."""
    _chk(load().isx_light_field_device(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray),
                                       C.c_void_p(int(d_field_ptr) or None), C.c_void_p(int(d_counts_ptr) or None)),
         "isx_light_field_device")


def bin_injected_lines(cfg, sink, P, V, spec=None, region_counts=None, unit=INJECT_UNIT_AUTO, into=None):
    """The binning kernel of `sink` alone on the caller's exit lines (P[k], V[k]) (include/isx.h: isx_bin_injected_lines; parity
    tests).  -> (out_a, out_b, counts, bin_increments): INJECT_FLUX hits[n_theta, n_phi], None, None; INJECT_EXIT_MAPS
    dir_map[n_v, n_u], pos_map[n_y, n_x], counts[5]; INJECT_LIGHT_FIELD field[n_y, n_x, n_v, n_u], None, counts[4].
    region_counts: lines per 1024-slot region of the workspace (None: full regions); into: (out_a, out_b, counts) of an earlier
    call to accumulate into."""
    lines = np.ascontiguousarray(np.concatenate([np.asarray(P, dtype=np.float64).reshape(-1, 3),
                                                 np.asarray(V, dtype=np.float64).reshape(-1, 3)], axis=1))
    n = lines.shape[0]
    if sink == INJECT_FLUX:
        shapes = ((cfg.n_theta, cfg.n_phi), None, 0)
    elif sink == INJECT_EXIT_MAPS:
        shapes = ((spec.n_v, spec.n_u), (spec.n_y, spec.n_x), 5)
    else:
        shapes = ((spec.n_y, spec.n_x, spec.n_v, spec.n_u), None, 4)
    if into is not None:
        a, b, k = into
    else:
        a = np.zeros(shapes[0], dtype=np.uint64)
        b = np.zeros(shapes[1], dtype=np.uint64) if shapes[1] is not None else None
        k = np.zeros(shapes[2], dtype=np.uint64) if shapes[2] else None
    rc_arr = None if region_counts is None else np.ascontiguousarray(region_counts, dtype=np.uint32)
    inc = C.c_uint64(0)
    ptr = lambda x: _p(x, C.c_uint64) if x is not None and x.size else None
    _chk(load().isx_bin_injected_lines(C.byref(cfg), int(sink), C.byref(spec) if spec is not None else None,
                                       _p(lines, C.c_double) if n else None, n,
                                       _p(rc_arr, C.c_uint32) if rc_arr is not None else None,
                                       0 if rc_arr is None else rc_arr.size, int(unit), ptr(a), ptr(b), ptr(k), C.byref(inc)),
         "isx_bin_injected_lines")
    return a, b, k, int(inc.value)


def bin_injected_segments(cfg, centers_axes, radius, half_thick, segments, region_counts=None, unit=INJECT_UNIT_AUTO, into=None):
    """The disc sweep's binning kernel alone on the caller's exit segments[n, 7] (start, direction, tmax) (include/isx.h:
    isx_bin_injected_segments; parity tests).  -> (hits[n_disc], bin_increments).  region_counts: segments per 1024-slot region of
    the workspace (None: full regions); into: the hits of an earlier call to accumulate into."""
    ca = np.ascontiguousarray(centers_axes, dtype=np.float64).reshape(-1, 6)
    seg = np.ascontiguousarray(segments, dtype=np.float64).reshape(-1, 7)
    n = seg.shape[0]
    hits = into if into is not None else np.zeros(ca.shape[0], dtype=np.uint64)
    rc_arr = None if region_counts is None else np.ascontiguousarray(region_counts, dtype=np.uint32)
    inc = C.c_uint64(0)
    _chk(load().isx_bin_injected_segments(C.byref(cfg), _p(ca, C.c_double), ca.shape[0], float(radius), float(half_thick),
                                          _p(seg, C.c_double) if n else None, n,
                                          _p(rc_arr, C.c_uint32) if rc_arr is not None else None,
                                          0 if rc_arr is None else rc_arr.size, int(unit), _p(hits, C.c_uint64), C.byref(inc)),
         "isx_bin_injected_segments")
    return hits, int(inc.value)


def default_order_hist_spec(cfg):
    """512 orders, 8 dz bins (no GPU needed)."""
    s = OrderHistSpec()
    load().isx_default_order_hist_spec(C.byref(cfg), C.byref(s))
    return s


def _order_sizes(spec):
    """(n_orders, n_dz) of the arrays a call may write; (1, 0) for a spec the library refuses (it says so itself)."""
    ok = (1 <= spec.n_orders <= ORDER_HIST_MAX_ORDERS and 0 <= spec.n_dz <= ORDER_HIST_MAX_DZ and
          spec.n_orders * (4 + spec.n_dz) <= ORDER_HIST_MAX_WORDS)
    return (spec.n_orders, spec.n_dz) if ok else (1, 0)


def order_hist(cfg, n_rays, seed, spec=None, first_ray=0):
    """-> (hist[4, n_orders] uint64, port_dz[n_orders, n_dz] uint64, OrderHistCounts, Stats): the bounce order at which every ray
    ended, by class -- 0 counted below z, 1 exited otherwise, 2 absorbed, 3 suspended -- and, for the counted rays, by the z of
    the final direction (include/isx.h)."""
    if spec is None:
        spec = default_order_hist_spec(cfg)
    no, nz = _order_sizes(spec)
    hist = np.zeros(4 * no, dtype=np.uint64)
    dz = np.zeros(max(no * nz, 1), dtype=np.uint64)
    cnt, st = OrderHistCounts(), Stats()
    _chk(load().isx_order_hist(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray), _p(hist, C.c_uint64),
                               _p(dz, C.c_uint64), C.byref(cnt), C.byref(st)), "isx_order_hist")
    return hist.reshape(4, no), dz[:no * nz].reshape(no, nz), cnt, st


def order_hist_device(cfg, spec, n_rays, seed, first_ray, d_hist_ptr, d_port_dz_ptr, d_counts_ptr):
    """Enqueue on the library stream, accumulating into device memory: the uint64 histograms [4][n_orders] at d_hist_ptr, the
    port's [n_orders][n_dz] at d_port_dz_ptr (0 / None where n_dz == 0) and five uint64 counters at d_counts_ptr (e.g. torch
    tensors' data_ptr())."""
    _chk(load().isx_order_hist_device(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray),
                                      C.c_void_p(int(d_hist_ptr or 0) or None), C.c_void_p(int(d_port_dz_ptr or 0) or None),
                                      C.c_void_p(int(d_counts_ptr or 0) or None)), "isx_order_hist_device")


def order_reweight(cfg, spec, hist, counts, launched, rho):
    """-> (fraction[n_rho], sigma[n_rho]): the port fraction at the wall reflectances `rho` from the histories traced at
    cfg.reflectance, each with weight (rho / cfg.reflectance)^k (include/isx.h: isx_order_reweight; host only, no GPU needed)."""
    h = np.ascontiguousarray(np.asarray(hist, dtype=np.uint64).reshape(-1))
    no, _ = _order_sizes(spec)
    if h.size < 4 * no:
        raise ValueError("hist has %d words, the spec wants %d" % (h.size, 4 * no))
    r = np.ascontiguousarray(np.atleast_1d(rho), dtype=np.float64)
    frac, sig = np.zeros(max(r.size, 1)), np.zeros(max(r.size, 1))
    _chk(load().isx_order_reweight(C.byref(cfg), C.byref(spec), _p(h, C.c_uint64), C.byref(counts), int(launched),
                                   _p(r, C.c_double), int(r.size), _p(frac, C.c_double), _p(sig, C.c_double)), "isx_order_reweight")
    return frac[:r.size], sig[:r.size]


def default_wall_patch_spec(cfg):
    """No patches (no GPU needed)."""
    s = WallPatchSpec()
    load().isx_default_wall_patch_spec(C.byref(cfg), C.byref(s))
    return s


def wall_patch_cap(cfg, direction, half_angle_deg, reflectance):
    """-> WallPatch: the cap of half-angle `half_angle_deg` about `direction` (include/isx.h: isx_wall_patch_cap; host only)."""
    d = (C.c_double * 3)(*[float(x) for x in direction])
    out = WallPatch()
    _chk(load().isx_wall_patch_cap(C.byref(cfg), d, float(half_angle_deg), float(reflectance), C.byref(out)), "isx_wall_patch_cap")
    return out


def wall_patch_spec(cfg, patches):
    """-> WallPatchSpec of a list of WallPatch (at most MAX_WALL_PATCHES; where caps overlap the first wins)."""
    patches = list(patches)
    if len(patches) > MAX_WALL_PATCHES:
        raise ValueError("at most %d wall patches" % MAX_WALL_PATCHES)
    s = default_wall_patch_spec(cfg)
    s.n_patches = len(patches)
    for k, p in enumerate(patches):
        C.memmove(C.byref(s.patch[k]), C.byref(p), C.sizeof(WallPatch))
    return s


def _patch_classes(spec):
    """entries of the arrays a call may write; 2 for a spec the library refuses (it says so itself)"""
    return (spec.n_patches if 0 <= spec.n_patches <= MAX_WALL_PATCHES else 0) + 2


def wall_patches(cfg, n_rays, seed, spec=None, first_ray=0):
    """-> (arrivals[P + 2] uint64, absorbed[P + 2] uint64, Stats): the trace with the spec's caps of the inner wall at their own
    reflectance; per class -- the P patches, the rest of the inner sphere, rim and outer sphere -- the interactions that arrived
    and the rays absorbed there (include/isx.h)."""
    if spec is None:
        spec = default_wall_patch_spec(cfg)
    nc = _patch_classes(spec)
    arr, ab = np.zeros(nc, dtype=np.uint64), np.zeros(nc, dtype=np.uint64)
    st = Stats()
    _chk(load().isx_wall_patches(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray), _p(arr, C.c_uint64),
                                 _p(ab, C.c_uint64), C.byref(st)), "isx_wall_patches")
    return arr, ab, st


def wall_patches_device(cfg, spec, n_rays, seed, first_ray, d_arrivals_ptr, d_absorbed_ptr):
    """Enqueue on the library stream, accumulating into device memory: n_patches + 2 uint64 counters each at d_arrivals_ptr and
    d_absorbed_ptr (e.g. torch tensors' data_ptr())."""
    _chk(load().isx_wall_patches_device(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray),
                                        C.c_void_p(int(d_arrivals_ptr or 0) or None), C.c_void_p(int(d_absorbed_ptr or 0) or None)),
         "isx_wall_patches_device")


def default_beam_spec(cfg):
    """The pencil of `cfg` as a beam: origin src, axis dir / |dir|, radius 0, cos_min 1 (no GPU needed)."""
    s = BeamSpec()
    load().isx_default_beam_spec(C.byref(cfg), C.byref(s))
    return s


def beam_cone(cfg, origin, direction, radius, half_angle_deg, law=BEAM_UNIFORM):
    """-> BeamSpec: the disc of `radius` about `origin` emitting into the cone of `half_angle_deg` about `direction`
    (include/isx.h: isx_beam_cone; host only)."""
    o = (C.c_double * 3)(*[float(x) for x in origin])
    d = (C.c_double * 3)(*[float(x) for x in direction])
    out = BeamSpec()
    _chk(load().isx_beam_cone(C.byref(cfg), o, d, float(radius), float(half_angle_deg), int(law), C.byref(out)), "isx_beam_cone")
    return out


def beam_endstates(cfg, spec, n, seed, first_ray=0):
    """-> (status, n_points, last_point, direction, start_point, start_dir): trace_endstates for the beam, with every ray's
    sampled start."""
    n = int(n)
    status = np.zeros(n, dtype=np.int32)
    npts = np.zeros(n, dtype=np.int32)
    lp, d, sp, sd = (np.zeros((n, 3), dtype=np.float64) for _ in range(4))
    _chk(load().isx_beam_endstates(C.byref(cfg), C.byref(spec), n, int(seed), int(first_ray), _p(status, C.c_int32),
                                   _p(npts, C.c_int32), _p(lp, C.c_double), _p(d, C.c_double), _p(sp, C.c_double),
                                   _p(sd, C.c_double)), "isx_beam_endstates")
    return status, npts, lp, d, sp, sd


def fluxmap_beam(cfg, spec, n_rays, seed, first_ray=0):
    """-> (hits[n_theta, n_phi] uint64, Stats): the flux map of the beam source `spec` (include/isx.h: isx_fluxmap_beam)."""
    hits = np.zeros(max(cfg.n_theta, 0) * max(cfg.n_phi, 0), dtype=np.uint64)
    st = Stats()
    _chk(load().isx_fluxmap_beam(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray), _p(hits, C.c_uint64),
                                 C.byref(st)), "isx_fluxmap_beam")
    return hits.reshape(cfg.n_theta, cfg.n_phi), st


def fluxmap_beam_device(cfg, spec, n_rays, seed, first_ray, d_hits_ptr):
    """Enqueue on the library stream, accumulating into device memory at d_hits_ptr ([n_theta * n_phi] uint64)."""
    _chk(load().isx_fluxmap_beam_device(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray),
                                        C.c_void_p(int(d_hits_ptr or 0) or None)), "isx_fluxmap_beam_device")


def default_baffle_spec(cfg):
    """No baffle: n_baffles 0 (no GPU needed)."""
    s = BaffleSpec()
    load().isx_default_baffle_spec(C.byref(cfg), C.byref(s))
    return s


def baffle_disc(cfg, centre, direction, radius, reflectance):
    """-> Baffle: the disc of `radius` about `centre` with normal direction / |direction| (include/isx.h: isx_baffle_disc; host only)."""
    c = (C.c_double * 3)(*[float(x) for x in centre])
    d = (C.c_double * 3)(*[float(x) for x in direction])
    out = Baffle()
    _chk(load().isx_baffle_disc(C.byref(cfg), c, d, float(radius), float(reflectance), C.byref(out)), "isx_baffle_disc")
    return out


def baffle_spec(cfg, baffles):
    """-> BaffleSpec holding the given Baffle objects, in order."""
    s = default_baffle_spec(cfg)
    baffles = list(baffles)
    if len(baffles) > MAX_BAFFLES:
        raise ValueError("at most %d baffles" % MAX_BAFFLES)
    for k, b in enumerate(baffles):
        C.memmove(C.byref(s.baffle[k]), C.byref(b), C.sizeof(Baffle))
    s.n_baffles = len(baffles)
    return s


def baffle_endstates(cfg, spec, n, seed, first_ray=0):
    """-> (status, n_points, last_point, direction, last_baffle): trace_endstates with the baffles; last_baffle is -1 or
    2 k + side of the ray's last baffle interaction."""
    n = int(n)
    status = np.zeros(n, dtype=np.int32)
    npts = np.zeros(n, dtype=np.int32)
    lb = np.zeros(n, dtype=np.int32)
    lp, d = (np.zeros((n, 3), dtype=np.float64) for _ in range(2))
    _chk(load().isx_baffle_endstates(C.byref(cfg), C.byref(spec), n, int(seed), int(first_ray), _p(status, C.c_int32),
                                     _p(npts, C.c_int32), _p(lp, C.c_double), _p(d, C.c_double), _p(lb, C.c_int32)),
         "isx_baffle_endstates")
    return status, npts, lp, d, lb


def fluxmap_baffle(cfg, spec, n_rays, seed, first_ray=0):
    """-> (hits[n_theta, n_phi] uint64, BaffleCounts, Stats): the flux map with the baffles of `spec` in the cavity
    (include/isx.h: isx_fluxmap_baffle)."""
    hits = np.zeros(max(cfg.n_theta, 0) * max(cfg.n_phi, 0), dtype=np.uint64)
    st = Stats()
    cnt = BaffleCounts()
    _chk(load().isx_fluxmap_baffle(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray), _p(hits, C.c_uint64),
                                   C.byref(cnt), C.byref(st)), "isx_fluxmap_baffle")
    return hits.reshape(cfg.n_theta, cfg.n_phi), cnt, st


def fluxmap_baffle_device(cfg, spec, n_rays, seed, first_ray, d_hits_ptr, d_counts_ptr):
    """Enqueue on the library stream, accumulating into device memory at d_hits_ptr ([n_theta * n_phi] uint64) and d_counts_ptr
    ([16] uint64, BaffleCounts' layout)."""
    _chk(load().isx_fluxmap_baffle_device(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray),
                                          C.c_void_p(int(d_hits_ptr or 0) or None), C.c_void_p(int(d_counts_ptr or 0) or None)),
         "isx_fluxmap_baffle_device")


def default_scene_spec(cfg):
    """The empty scene: the pencil of `cfg` as a beam, no baffle, no patch (no GPU needed)."""
    s = SceneSpec()
    load().isx_default_scene_spec(C.byref(cfg), C.byref(s))
    return s


def scene_spec(cfg, beam=None, baffles=(), patches=()):
    """-> SceneSpec: the BeamSpec `beam` (None: the pencil of `cfg`), the Baffle objects and the WallPatch objects, in order."""
    s = default_scene_spec(cfg)
    if beam is not None:
        C.memmove(C.byref(s.beam), C.byref(beam), C.sizeof(BeamSpec))
    bs, ps = baffle_spec(cfg, baffles), wall_patch_spec(cfg, patches)
    C.memmove(C.byref(s.baffles), C.byref(bs), C.sizeof(BaffleSpec))
    C.memmove(C.byref(s.patches), C.byref(ps), C.sizeof(WallPatchSpec))
    return s


def scene_endstates(cfg, spec, n, seed, first_ray=0):
    """-> (status, n_points, last_point, direction, start_point, start_dir, last_baffle, last_class): trace_endstates of the
    scene; last_baffle is -1 or 2 k + side of the ray's last baffle interaction, last_class -1 or the class of its last mirror
    interaction."""
    n = int(n)
    status = np.zeros(n, dtype=np.int32)
    npts = np.zeros(n, dtype=np.int32)
    lb = np.zeros(n, dtype=np.int32)
    lc = np.zeros(n, dtype=np.int32)
    lp, d, sp, sd = (np.zeros((n, 3), dtype=np.float64) for _ in range(4))
    _chk(load().isx_scene_endstates(C.byref(cfg), C.byref(spec), n, int(seed), int(first_ray), _p(status, C.c_int32),
                                    _p(npts, C.c_int32), _p(lp, C.c_double), _p(d, C.c_double), _p(sp, C.c_double),
                                    _p(sd, C.c_double), _p(lb, C.c_int32), _p(lc, C.c_int32)), "isx_scene_endstates")
    return status, npts, lp, d, sp, sd, lb, lc


def fluxmap_scene(cfg, spec, n_rays, seed, first_ray=0):
    """-> (hits[n_theta, n_phi] uint64, SceneCounts, Stats): the flux map of the scene `spec` (include/isx.h: isx_fluxmap_scene)."""
    hits = np.zeros(max(cfg.n_theta, 0) * max(cfg.n_phi, 0), dtype=np.uint64)
    st = Stats()
    cnt = SceneCounts()
    _chk(load().isx_fluxmap_scene(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray), _p(hits, C.c_uint64),
                                  C.byref(cnt), C.byref(st)), "isx_fluxmap_scene")
    return hits.reshape(cfg.n_theta, cfg.n_phi), cnt, st


def fluxmap_scene_device(cfg, spec, n_rays, seed, first_ray, d_hits_ptr, d_counts_ptr):
    """Enqueue on the library stream, accumulating into device memory at d_hits_ptr ([n_theta * n_phi] uint64) and d_counts_ptr
    ([36] uint64, SceneCounts' layout)."""
    _chk(load().isx_fluxmap_scene_device(C.byref(cfg), C.byref(spec), int(n_rays), int(seed), int(first_ray),
                                         C.c_void_p(int(d_hits_ptr or 0) or None), C.c_void_p(int(d_counts_ptr or 0) or None)),
         "isx_fluxmap_scene_device")


def default_response_spec(cfg):
    """n = (1, 1, 6, 12): a point lamp's directions in 6 polar bands x 12 azimuths (no GPU needed)."""
    s = ResponseSpec()
    load().isx_default_response_spec(C.byref(cfg), C.byref(s))
    return s


def response_spec(n0, n1, n2, n3):
    """-> ResponseSpec with n0 disc rings x n1 disc azimuths x n2 polar bands x n3 direction azimuths (checked by the calls)."""
    s = ResponseSpec()
    s.struct_size = C.sizeof(ResponseSpec)
    s.n[0], s.n[1], s.n[2], s.n[3] = int(n0), int(n1), int(n2), int(n3)
    return s


def _response_bins(rspec):
    """B of the arrays a call may touch; 1 for a spec the library refuses (it says so itself)."""
    ok = all(1 <= int(v) <= RESPONSE_MAX_AXIS for v in rspec.n) and rspec.bins <= RESPONSE_MAX_BINS
    return rspec.bins if ok else 1


def scene_response(cfg, scene, rspec, n_rays, seed, first_ray=0):
    """-> (response[21, B] uint64, SceneCounts, Stats): the fate of every ray of the scene -- absorbed by wall class 0 .. P + 1,
    by side s of baffle k (10 + 2 k + s), through the port (18), exited otherwise (19), suspended (20) -- binned over the
    source's sample space (include/isx.h: isx_scene_response)."""
    B = _response_bins(rspec)
    resp = np.zeros(RESPONSE_FATES * B, dtype=np.uint64)
    st = Stats()
    cnt = SceneCounts()
    _chk(load().isx_scene_response(C.byref(cfg), C.byref(scene), C.byref(rspec), int(n_rays), int(seed), int(first_ray),
                                   _p(resp, C.c_uint64), C.byref(cnt), C.byref(st)), "isx_scene_response")
    return resp.reshape(RESPONSE_FATES, B), cnt, st


def scene_response_device(cfg, scene, rspec, n_rays, seed, first_ray, d_response_ptr, d_counts_ptr):
    """Enqueue on the library stream, accumulating into device memory at d_response_ptr ([21 * B] uint64) and d_counts_ptr
    ([36] uint64, SceneCounts' layout)."""
    _chk(load().isx_scene_response_device(C.byref(cfg), C.byref(scene), C.byref(rspec), int(n_rays), int(seed), int(first_ray),
                                          C.c_void_p(int(d_response_ptr or 0) or None), C.c_void_p(int(d_counts_ptr or 0) or None)),
         "isx_scene_response_device")


def response_reweight(rspec, response, weight):
    """-> (fraction[21], sigma[21]): the fate fractions of a lamp whose intensity relative to the traced source is weight[b] in
    bin b, from one scene_response result (include/isx.h: isx_response_reweight; host only, no GPU needed)."""
    B = _response_bins(rspec)
    h = np.ascontiguousarray(np.asarray(response, dtype=np.uint64).reshape(-1))
    w = np.ascontiguousarray(np.asarray(weight, dtype=np.float64).reshape(-1))
    if h.size < RESPONSE_FATES * B or w.size < B:
        raise ValueError("response has %d words and weight %d, the spec wants %d and %d" % (h.size, w.size, RESPONSE_FATES * B, B))
    frac, sig = np.zeros(RESPONSE_FATES), np.zeros(RESPONSE_FATES)
    _chk(load().isx_response_reweight(C.byref(rspec), _p(h, C.c_uint64), _p(w, C.c_double), _p(frac, C.c_double),
                                      _p(sig, C.c_double)), "isx_response_reweight")
    return frac, sig


def view_frame(cfg, scene, patch, n_u, n_v, half_extent=1.0):
    """-> ViewSpec for patch `patch` of the scene: its axis as given, e1 and e2 by beam_cone's frame rule about it, an n_u x n_v
    map over [-half_extent, half_extent]^2 of the direction cosines (include/isx.h: isx_view_frame; no GPU needed)."""
    s = ViewSpec()
    _chk(load().isx_view_frame(C.byref(cfg), C.byref(scene), int(patch), int(n_u), int(n_v), float(half_extent), C.byref(s)),
         "isx_view_frame")
    return s


def _view_bins(vspec):
    """the words of the arrays a call may touch; 1 for a spec the library refuses (it says so itself)"""
    ok = 1 <= int(vspec.n_u) <= VIEW_MAX_AXIS and 1 <= int(vspec.n_v) <= VIEW_MAX_AXIS and vspec.bins <= VIEW_MAX_BINS
    return (int(vspec.n_v), int(vspec.n_u)) if ok else (1, 1)


def scene_view(cfg, scene, vspec, n_rays, seed, first_ray=0):
    """-> (view[n_v, n_u] uint64, ViewCounts, SceneCounts, Stats): the rays wall class vspec.patch of the scene absorbs, binned
    over the direction they arrive from in the frame of vspec (include/isx.h: isx_scene_view)."""
    nv, nu = _view_bins(vspec)
    view = np.zeros(nv * nu, dtype=np.uint64)
    st = Stats()
    vc = ViewCounts()
    cnt = SceneCounts()
    _chk(load().isx_scene_view(C.byref(cfg), C.byref(scene), C.byref(vspec), int(n_rays), int(seed), int(first_ray),
                               _p(view, C.c_uint64), C.byref(vc), C.byref(cnt), C.byref(st)), "isx_scene_view")
    return view.reshape(nv, nu), vc, cnt, st


def scene_view_device(cfg, scene, vspec, n_rays, seed, first_ray, d_view_ptr, d_view_counts_ptr, d_scene_counts_ptr):
    """Enqueue on the library stream, accumulating into device memory at d_view_ptr ([n_v * n_u] uint64), d_view_counts_ptr
    ([4] uint64, ViewCounts' layout) and d_scene_counts_ptr ([36] uint64, SceneCounts' layout)."""
    _chk(load().isx_scene_view_device(C.byref(cfg), C.byref(scene), C.byref(vspec), int(n_rays), int(seed), int(first_ray),
                                      C.c_void_p(int(d_view_ptr or 0) or None), C.c_void_p(int(d_view_counts_ptr or 0) or None),
                                      C.c_void_p(int(d_scene_counts_ptr or 0) or None)), "isx_scene_view_device")


def view_reweight(vspec, view, view_counts, launched, weight, direct_weight=0.0):
    """-> (signal, sigma): the reading per launched ray of a detector whose angular response is weight[iv, iu] over the map and
    direct_weight for the rays straight from the source, from one scene_view result (include/isx.h: isx_view_reweight; host
    only, no GPU needed)."""
    nv, nu = _view_bins(vspec)
    h = np.ascontiguousarray(np.asarray(view, dtype=np.uint64).reshape(-1))
    w = np.ascontiguousarray(np.asarray(weight, dtype=np.float64).reshape(-1))
    if h.size < nv * nu or w.size < nv * nu:
        raise ValueError("view has %d words and weight %d, the spec wants %d" % (h.size, w.size, nv * nu))
    sig, sd = C.c_double(0.0), C.c_double(0.0)
    _chk(load().isx_view_reweight(C.byref(vspec), _p(h, C.c_uint64), C.byref(view_counts), int(launched), _p(w, C.c_double),
                                  float(direct_weight), C.byref(sig), C.byref(sd)), "isx_view_reweight")
    return sig.value, sd.value


def view_weight_fov(vspec, half_angle_deg):
    """-> weight[n_v, n_u]: 1.0 for the bins whose centre lies within half_angle_deg of the detector's normal, else 0.0 -- a
    field-of-view stop (include/isx.h: isx_view_weight_fov; host only, no GPU needed)."""
    nv, nu = _view_bins(vspec)
    w = np.zeros(nv * nu, dtype=np.float64)
    _chk(load().isx_view_weight_fov(C.byref(vspec), float(half_angle_deg), _p(w, C.c_double)), "isx_view_weight_fov")
    return w.reshape(nv, nu)


def patch_field_frame(cfg, scene, patch, n_x, n_y, n_u, n_v, half_extent=1.0):
    """-> PatchFieldSpec for patch `patch` of the scene: the frame by view_frame's rule, pos_scale so that the cap fills the unit
    disc of the position part, an n_y x n_x x n_v x n_u field (include/isx.h: isx_patch_field_frame; no GPU needed)."""
    s = PatchFieldSpec()
    _chk(load().isx_patch_field_frame(C.byref(cfg), C.byref(scene), int(patch), int(n_x), int(n_y), int(n_u), int(n_v),
                                      float(half_extent), C.byref(s)), "isx_patch_field_frame")
    return s


def _patch_field_shape(fspec):
    """the shape of the array a call may touch; (1, 1, 1, 1) for a spec the library refuses (it says so itself)"""
    ax = [int(fspec.n_y), int(fspec.n_x), int(fspec.n_v), int(fspec.n_u)]
    ok = all(1 <= a <= PATCH_FIELD_MAX_AXIS for a in ax) and fspec.bins <= PATCH_FIELD_MAX_BINS
    return tuple(ax) if ok else (1, 1, 1, 1)


def scene_patch_field(cfg, scene, fspec, n_rays, seed, first_ray=0):
    """-> (field[n_y, n_x, n_v, n_u] uint64, PatchFieldCounts, SceneCounts, Stats): the rays wall class fspec.patch of the scene
    absorbs, binned over where on the patch they land and the direction they arrive from, in the frame of fspec (include/isx.h:
    isx_scene_patch_field)."""
    shape = _patch_field_shape(fspec)
    field = np.zeros(int(np.prod(shape)), dtype=np.uint64)
    st = Stats()
    fc = PatchFieldCounts()
    cnt = SceneCounts()
    _chk(load().isx_scene_patch_field(C.byref(cfg), C.byref(scene), C.byref(fspec), int(n_rays), int(seed), int(first_ray),
                                      _p(field, C.c_uint64), C.byref(fc), C.byref(cnt), C.byref(st)), "isx_scene_patch_field")
    return field.reshape(shape), fc, cnt, st


def scene_patch_field_device(cfg, scene, fspec, n_rays, seed, first_ray, d_field_ptr, d_field_counts_ptr, d_scene_counts_ptr):
    """Enqueue on the library stream, accumulating into device memory at d_field_ptr ([n_y * n_x * n_v * n_u] uint64),
    d_field_counts_ptr ([5] uint64, PatchFieldCounts' layout) and d_scene_counts_ptr ([36] uint64, SceneCounts' layout)."""
    _chk(load().isx_scene_patch_field_device(C.byref(cfg), C.byref(scene), C.byref(fspec), int(n_rays), int(seed), int(first_ray),
                                             C.c_void_p(int(d_field_ptr or 0) or None),
                                             C.c_void_p(int(d_field_counts_ptr or 0) or None),
                                             C.c_void_p(int(d_scene_counts_ptr or 0) or None)), "isx_scene_patch_field_device")


def patch_field_marginals(fspec, field):
    """-> (pos_map[n_y, n_x], dir_map[n_v, n_u]) uint64: the two sums of a field; dir_map is what view_reweight takes through a
    view spec with the same frame (include/isx.h: isx_patch_field_marginals; host only, no GPU needed)."""
    ny, nx, nv, nu = _patch_field_shape(fspec)
    f = np.ascontiguousarray(np.asarray(field, dtype=np.uint64).reshape(-1))
    if f.size < ny * nx * nv * nu:
        raise ValueError("field has %d words, the spec wants %d" % (f.size, ny * nx * nv * nu))
    pos = np.zeros(ny * nx, dtype=np.uint64)
    dr = np.zeros(nv * nu, dtype=np.uint64)
    _chk(load().isx_patch_field_marginals(C.byref(fspec), _p(f, C.c_uint64), _p(pos, C.c_uint64), _p(dr, C.c_uint64)),
         "isx_patch_field_marginals")
    return pos.reshape(ny, nx), dr.reshape(nv, nu)


def default_scene_order_spec(cfg):
    """512 orders per fate slot (no GPU needed)."""
    s = SceneOrderSpec()
    load().isx_default_scene_order_spec(C.byref(cfg), C.byref(s))
    return s


def scene_order_spec(n_orders):
    """-> SceneOrderSpec with orders 0 .. n_orders - 1 per fate slot (checked by the calls)."""
    s = SceneOrderSpec()
    s.struct_size = C.sizeof(SceneOrderSpec)
    s.n_orders = int(n_orders)
    return s


def _scene_orders(ospec):
    """n_orders of the arrays a call may touch; 1 for a spec the library refuses (it says so itself)."""
    return int(ospec.n_orders) if 1 <= int(ospec.n_orders) <= SCENE_ORDER_MAX_ORDERS else 1


def scene_order_hist(cfg, scene, ospec, n_rays, seed, first_ray=0):
    """-> (hist[21, n_orders] uint64, SceneOrderCounts, SceneCounts, Stats): the fate of every ray of the scene (scene_response's
    slots) by its interaction count k; a ray with k >= n_orders is counted in overflow[fate] instead (include/isx.h:
    isx_scene_order_hist)."""
    K = _scene_orders(ospec)
    hist = np.zeros(RESPONSE_FATES * K, dtype=np.uint64)
    st = Stats()
    oc = SceneOrderCounts()
    cnt = SceneCounts()
    _chk(load().isx_scene_order_hist(C.byref(cfg), C.byref(scene), C.byref(ospec), int(n_rays), int(seed), int(first_ray),
                                     _p(hist, C.c_uint64), C.byref(oc), C.byref(cnt), C.byref(st)), "isx_scene_order_hist")
    return hist.reshape(RESPONSE_FATES, K), oc, cnt, st


def scene_order_hist_device(cfg, scene, ospec, n_rays, seed, first_ray, d_hist_ptr, d_order_counts_ptr, d_scene_counts_ptr):
    """Enqueue on the library stream, accumulating into device memory at d_hist_ptr ([21 * n_orders] uint64), d_order_counts_ptr
    ([21] uint64, SceneOrderCounts' layout) and d_scene_counts_ptr ([36] uint64, SceneCounts' layout)."""
    _chk(load().isx_scene_order_hist_device(C.byref(cfg), C.byref(scene), C.byref(ospec), int(n_rays), int(seed), int(first_ray),
                                            C.c_void_p(int(d_hist_ptr or 0) or None),
                                            C.c_void_p(int(d_order_counts_ptr or 0) or None),
                                            C.c_void_p(int(d_scene_counts_ptr or 0) or None)), "isx_scene_order_hist_device")


def _scene_order_counts(counts):
    if isinstance(counts, SceneOrderCounts):
        return counts
    oc = SceneOrderCounts()
    w = np.asarray(counts, dtype=np.uint64).reshape(-1)
    for f in range(RESPONSE_FATES):
        oc.overflow[f] = int(w[f])
    return oc


def scene_order_reweight(cfg, scene, ospec, hist, counts, launched, scale):
    """-> (fraction[n_scale, 21], sigma[n_scale, 21]): the fate fractions of the same scene with every reflectance -- the wall's,
    every patch's, every baffle's -- multiplied by scale[i], from one scene_order_hist result (include/isx.h:
    isx_scene_order_reweight; host only, no GPU needed)."""
    K = _scene_orders(ospec)
    h = np.ascontiguousarray(np.asarray(hist, dtype=np.uint64).reshape(-1))
    if h.size < RESPONSE_FATES * K:
        raise ValueError("hist has %d words, the spec wants %d" % (h.size, RESPONSE_FATES * K))
    t = np.ascontiguousarray(np.asarray(scale, dtype=np.float64).reshape(-1))
    oc = _scene_order_counts(counts)
    frac, sig = np.zeros((t.size, RESPONSE_FATES)), np.zeros((t.size, RESPONSE_FATES))
    _chk(load().isx_scene_order_reweight(C.byref(cfg), C.byref(scene), C.byref(ospec), _p(h, C.c_uint64), C.byref(oc), int(launched),
                                         _p(t, C.c_double), int(t.size), _p(frac, C.c_double), _p(sig, C.c_double)),
         "isx_scene_order_reweight")
    return frac, sig


def scene_order_moments(ospec, hist, counts):
    """-> (mean[21], sd[21]) of the interaction count k per fate slot: the time response in interactions; NaN for an empty row and
    for a row with overflow (include/isx.h: isx_scene_order_moments; host only, no GPU needed)."""
    K = _scene_orders(ospec)
    h = np.ascontiguousarray(np.asarray(hist, dtype=np.uint64).reshape(-1))
    if h.size < RESPONSE_FATES * K:
        raise ValueError("hist has %d words, the spec wants %d" % (h.size, RESPONSE_FATES * K))
    oc = _scene_order_counts(counts)
    mean, sd = np.zeros(RESPONSE_FATES), np.zeros(RESPONSE_FATES)
    _chk(load().isx_scene_order_moments(C.byref(ospec), _p(h, C.c_uint64), C.byref(oc), _p(mean, C.c_double), _p(sd, C.c_double)),
         "isx_scene_order_moments")
    return mean, sd


def default_scene_path_spec(cfg):
    """1024 bins of r_in / 4 cm per fate slot (no GPU needed)."""
    s = ScenePathSpec()
    load().isx_default_scene_path_spec(C.byref(cfg), C.byref(s))
    return s


def scene_path_spec(n_bins, bin_cm):
    """-> ScenePathSpec with bins 0 .. n_bins - 1 of width bin_cm per fate slot (checked by the calls)."""
    s = ScenePathSpec()
    s.struct_size = C.sizeof(ScenePathSpec)
    s.n_bins = int(n_bins)
    s.bin_cm = float(bin_cm)
    return s


def _scene_path_bins(pspec):
    """n_bins of the arrays a call may touch; 1 for a spec the library refuses (it says so itself)."""
    return int(pspec.n_bins) if 1 <= int(pspec.n_bins) <= SCENE_PATH_MAX_BINS else 1


def scene_path_hist(cfg, scene, pspec, n_rays, seed, first_ray=0):
    """-> (hist[21, n_bins] uint64, ScenePathCounts, SceneCounts, Stats): the fate of every ray of the scene (scene_response's
    slots) by its path length L in cm, bin (int)(L / bin_cm); a ray beyond the last bin is counted in overflow[fate] instead, and
    checksum[fate] sums the bit patterns of L modulo 2^64 (include/isx.h: isx_scene_path_hist).  Time is L / LIGHT_CM_PER_NS."""
    K = _scene_path_bins(pspec)
    hist = np.zeros(RESPONSE_FATES * K, dtype=np.uint64)
    st = Stats()
    pc = ScenePathCounts()
    cnt = SceneCounts()
    _chk(load().isx_scene_path_hist(C.byref(cfg), C.byref(scene), C.byref(pspec), int(n_rays), int(seed), int(first_ray),
                                    _p(hist, C.c_uint64), C.byref(pc), C.byref(cnt), C.byref(st)), "isx_scene_path_hist")
    return hist.reshape(RESPONSE_FATES, K), pc, cnt, st


def scene_path_hist_device(cfg, scene, pspec, n_rays, seed, first_ray, d_hist_ptr, d_path_counts_ptr, d_scene_counts_ptr):
    """Enqueue on the library stream, accumulating into device memory at d_hist_ptr ([21 * n_bins] uint64), d_path_counts_ptr
    ([42] uint64, ScenePathCounts' layout) and d_scene_counts_ptr ([36] uint64, SceneCounts' layout)."""
    _chk(load().isx_scene_path_hist_device(C.byref(cfg), C.byref(scene), C.byref(pspec), int(n_rays), int(seed), int(first_ray),
                                           C.c_void_p(int(d_hist_ptr or 0) or None),
                                           C.c_void_p(int(d_path_counts_ptr or 0) or None),
                                           C.c_void_p(int(d_scene_counts_ptr or 0) or None)), "isx_scene_path_hist_device")


def _scene_path_counts(counts):
    if isinstance(counts, ScenePathCounts):
        return counts
    pc = ScenePathCounts()
    w = np.asarray(counts, dtype=np.uint64).reshape(-1)
    for f in range(RESPONSE_FATES):
        pc.overflow[f] = int(w[f])
        if w.size >= 2 * RESPONSE_FATES:
            pc.checksum[f] = int(w[RESPONSE_FATES + f])
    return pc


def _scene_path_rows(pspec, hist):
    K = _scene_path_bins(pspec)
    h = np.ascontiguousarray(np.asarray(hist, dtype=np.uint64).reshape(-1))
    if h.size < RESPONSE_FATES * K:
        raise ValueError("hist has %d words, the spec wants %d" % (h.size, RESPONSE_FATES * K))
    return h


def scene_path_moments(pspec, hist, counts):
    """-> (mean_cm[21], sd_cm[21]) of the path length per fate slot, from the bin centres; NaN for an empty row and for a row with
    overflow (include/isx.h: isx_scene_path_moments; host only, no GPU needed)."""
    h = _scene_path_rows(pspec, hist)
    pc = _scene_path_counts(counts)
    mean, sd = np.zeros(RESPONSE_FATES), np.zeros(RESPONSE_FATES)
    _chk(load().isx_scene_path_moments(C.byref(pspec), _p(h, C.c_uint64), C.byref(pc), _p(mean, C.c_double), _p(sd, C.c_double)),
         "isx_scene_path_moments")
    return mean, sd


def scene_path_decay(pspec, hist, counts, fate, lo_bin):
    """-> (tau_cm, sigma_cm): the decay constant of row `fate`'s tail from bin lo_bin on, the maximum-likelihood estimate for a
    geometric law over the bins (include/isx.h: isx_scene_path_decay; host only, no GPU needed)."""
    h = _scene_path_rows(pspec, hist)
    pc = _scene_path_counts(counts)
    tau, sig = C.c_double(0.0), C.c_double(0.0)
    _chk(load().isx_scene_path_decay(C.byref(pspec), _p(h, C.c_uint64), C.byref(pc), int(fate), int(lo_bin), C.byref(tau),
                                     C.byref(sig)), "isx_scene_path_decay")
    return tau.value, sig.value


def fluxmap_series(cfgs, n_rays, seed, first_ray=0):
    """cfgs: list of Config sharing one detector grid -> (hits[n_cfg, n_theta, n_phi], [Stats])."""
    n = len(cfgs)
    arr = (Config * n)(*cfgs)
    nb = cfgs[0].n_theta * cfgs[0].n_phi
    hits = np.zeros(n * nb, dtype=np.uint64)
    st = (Stats * n)()
    _chk(load().isx_fluxmap_series(arr, n, int(n_rays), int(seed), int(first_ray), _p(hits, C.c_uint64), st),
         "isx_fluxmap_series")
    return hits.reshape(n, cfgs[0].n_theta, cfgs[0].n_phi), list(st)


def detector_table(cfg):
    out = np.zeros((cfg.n_theta * cfg.n_phi, 6), dtype=np.float64)
    _chk(load().isx_detector_table(C.byref(cfg), _p(out, C.c_double)), "isx_detector_table")
    return out


def mathprobe(op, a, b=None, c=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = a if b is None else np.ascontiguousarray(b, dtype=np.float64)
    c = a if c is None else np.ascontiguousarray(c, dtype=np.float64)
    out = np.zeros_like(a)
    _chk(load().isx_mathprobe(int(op), _p(a, C.c_double), _p(b, C.c_double), _p(c, C.c_double), _p(out, C.c_double),
                              a.size), "isx_mathprobe")
    return out
