"""altair-raytracing_amd — MI355X-native integrating-sphere ray tracer (hot path only).

The product is libisx.so (csrc/, C ABI in include/isx.h) plus the C++ host driver that
keeps the reference's ROOT-macro entry signatures (host/).  This Python package is a thin
ctypes view of the C ABI used by tests/ and bench.py; it contains no compute of its own and
raises if the HIP library is missing.

Because the directory name carries a hyphen, import it with
    importlib.import_module("altair-raytracing_amd")
or through the `altair_raytracing_amd` shim at the repo root.
"""
from . import _abi as abi  # noqa: F401
from . import sharding  # noqa: F401
from .sharding import shard, step_slice, fluxmap_sharded, disc_sweep_sharded, exit_maps_sharded, wall_map_sharded, light_field_sharded, order_hist_sharded, wall_patches_sharded, fluxmap_beam_sharded, fluxmap_baffle_sharded, fluxmap_scene_sharded, scene_response_sharded, scene_view_sharded, scene_patch_field_sharded, scene_order_hist_sharded, scene_path_hist_sharded  # noqa: F401
from ._abi import (  # noqa: F401
    Config, Stats, IsxError, default_config, init, shutdown, device_info, set_option, fluxmap, fluxmap_device, sync,
    take_stats, last_kernel_ms, trace_endstates, fate_scan, fate_scan_launches, exit_scan_counts, disc_sweep, disc_sweep_per_position, exit_dz_hist, fluxmap_per_position, trace_rays_detector, exit_directions, fluxmap_series, detector_table, mathprobe, load, LIB_PATH, EXPORTS,
    ExitMapSpec, ExitMapCounts, default_exit_map_spec, exit_maps, exit_maps_device,
    WallMapSpec, WallMapCounts, default_wall_map_spec, wall_map, wall_map_device,
    LightFieldCounts, default_light_field_spec, light_field, light_field_device,
    bin_injected_lines, bin_injected_segments, INJECT_FLUX, INJECT_EXIT_MAPS, INJECT_LIGHT_FIELD, INJECT_UNIT_AUTO,
    OrderHistSpec, OrderHistCounts, default_order_hist_spec, order_hist, order_hist_device, order_reweight,
    WallPatch, WallPatchSpec, default_wall_patch_spec, wall_patch_cap, wall_patch_spec, wall_patches, wall_patches_device,
    BeamSpec, default_beam_spec, beam_cone, beam_endstates, fluxmap_beam, fluxmap_beam_device, BEAM_UNIFORM, BEAM_LAMBERT,
    Baffle, BaffleSpec, BaffleCounts, default_baffle_spec, baffle_disc, baffle_spec, baffle_endstates, fluxmap_baffle, fluxmap_baffle_device,
    MAX_BAFFLES,
    SceneSpec, SceneCounts, default_scene_spec, scene_spec, scene_endstates, fluxmap_scene, fluxmap_scene_device, SCENE_COUNT_WORDS,
    ResponseSpec, response_spec, default_response_spec, scene_response, scene_response_device, response_reweight, RESPONSE_FATES,
    ViewSpec, ViewCounts, view_frame, scene_view, scene_view_device, view_reweight, view_weight_fov,
    PatchFieldSpec, PatchFieldCounts, patch_field_frame, scene_patch_field, scene_patch_field_device, patch_field_marginals,
    SceneOrderSpec, SceneOrderCounts, default_scene_order_spec, scene_order_spec, scene_order_hist, scene_order_hist_device,
    scene_order_reweight, scene_order_moments, SCENE_ORDER_MAX_ORDERS,
    ScenePathSpec, ScenePathCounts, default_scene_path_spec, scene_path_spec, scene_path_hist, scene_path_hist_device,
    scene_path_moments, scene_path_decay, SCENE_PATH_MAX_BINS, LIGHT_CM_PER_NS,
    SOURCE_PENCIL, SOURCE_BRDF, RAY_EXITED, RAY_ABSORBED, RAY_SUSPENDED,
)

__all__ = ["abi", "sharding", "shard", "step_slice", "fluxmap_sharded", "disc_sweep_sharded", "exit_maps_sharded", "wall_map_sharded", "light_field_sharded", "order_hist_sharded", "Config", "Stats", "IsxError", "default_config", "init", "shutdown", "device_info", "set_option",
           "fluxmap", "fluxmap_device", "fluxmap_per_position", "trace_rays_detector", "exit_directions", "fluxmap_series", "sync", "take_stats", "last_kernel_ms", "trace_endstates", "fate_scan", "fate_scan_launches", "exit_scan_counts", "disc_sweep", "disc_sweep_per_position", "exit_dz_hist",
           "detector_table", "mathprobe", "load", "LIB_PATH", "EXPORTS",
           "ExitMapSpec", "ExitMapCounts", "default_exit_map_spec", "exit_maps", "exit_maps_device",
           "WallMapSpec", "WallMapCounts", "default_wall_map_spec", "wall_map", "wall_map_device",
           "LightFieldCounts", "default_light_field_spec", "light_field", "light_field_device",
           "bin_injected_lines", "bin_injected_segments", "INJECT_FLUX", "INJECT_EXIT_MAPS", "INJECT_LIGHT_FIELD", "INJECT_UNIT_AUTO",
           "OrderHistSpec", "OrderHistCounts", "default_order_hist_spec", "order_hist", "order_hist_device", "order_reweight",
           "WallPatch", "WallPatchSpec", "default_wall_patch_spec", "wall_patch_cap", "wall_patch_spec", "wall_patches", "wall_patches_device",
           "wall_patches_sharded",
           "BeamSpec", "default_beam_spec", "beam_cone", "beam_endstates", "fluxmap_beam", "fluxmap_beam_device", "BEAM_UNIFORM", "BEAM_LAMBERT",
           "fluxmap_beam_sharded",
           "Baffle", "BaffleSpec", "BaffleCounts", "default_baffle_spec", "baffle_disc", "baffle_spec", "baffle_endstates", "fluxmap_baffle",
           "fluxmap_baffle_device", "MAX_BAFFLES", "fluxmap_baffle_sharded",
           "SceneSpec", "SceneCounts", "default_scene_spec", "scene_spec", "scene_endstates", "fluxmap_scene", "fluxmap_scene_device",
           "SCENE_COUNT_WORDS", "fluxmap_scene_sharded",
           "ResponseSpec", "response_spec", "default_response_spec", "scene_response", "scene_response_device", "response_reweight",
           "RESPONSE_FATES", "scene_response_sharded",
           "ViewSpec", "ViewCounts", "view_frame", "scene_view", "scene_view_device", "view_reweight", "view_weight_fov",
           "scene_view_sharded",
           "PatchFieldSpec", "PatchFieldCounts", "patch_field_frame", "scene_patch_field", "scene_patch_field_device",
           "patch_field_marginals", "scene_patch_field_sharded",
           "SceneOrderSpec", "SceneOrderCounts", "default_scene_order_spec", "scene_order_spec", "scene_order_hist",
           "scene_order_hist_device", "scene_order_reweight", "scene_order_moments", "SCENE_ORDER_MAX_ORDERS",
           "scene_order_hist_sharded",
           "ScenePathSpec", "ScenePathCounts", "default_scene_path_spec", "scene_path_spec", "scene_path_hist",
           "scene_path_hist_device", "scene_path_moments", "scene_path_decay", "SCENE_PATH_MAX_BINS", "LIGHT_CM_PER_NS",
           "scene_path_hist_sharded",
           "SOURCE_PENCIL", "SOURCE_BRDF", "RAY_EXITED", "RAY_ABSORBED", "RAY_SUSPENDED"]
