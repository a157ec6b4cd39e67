"""Ray sharding across ranks (one process per GPU) + the single histogram all-reduce.

Rays are independent and ray i always draws from Philox stream (seed, i), so ANY partition of
the index range gives the same summed histogram.  Rank r of P traces the
contiguous range shard(n, r, P); the only exchange is one SUM all-reduce of the
[n_theta*n_phi] int64 histogram (+ the 7-word census; the exit maps: both maps + five counters + census; the wall map: map + four counters + census; the order histograms: both arrays + five counters + census) — torch.distributed backend "nccl"
(= RCCL over xGMI) on GPUs, "gloo" in the CPU tests.

The tracer itself is injected (`trace(cfg, count, seed, first) -> (hits, stats)`): on a GPU
box that is altair_raytracing_amd.fluxmap; there is no CPU tracer in this package.
"""
from typing import Callable, Tuple

import numpy as np


def shard(n_total: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous split of [0,n_total): returns (first, count); the first n_total%world ranks get one extra ray."""
    if world < 1 or not (0 <= rank < world) or n_total < 0:
        raise ValueError("bad shard request")
    q, r = divmod(n_total, world)
    first = rank * q + min(rank, r)
    return first, q + (1 if rank < r else 0)


def step_slice(step: int, rank: int, world: int, rays_per_rank: int) -> Tuple[int, int]:
    """bench.py's weak-scaling schedule: in step s, rank r traces rays [(s*world + r)*n, +n).  Over `steps` steps and all
    ranks these slices tile [0, steps*world*n) exactly once, and the union over ranks of one step is the contiguous block
    [s*world*n, (s+1)*world*n) -- so the summed histogram of a step does not depend on the number of ranks."""
    if world < 1 or not (0 <= rank < world) or step < 0 or rays_per_rank < 0:
        raise ValueError("bad step slice request")
    return (step * world + rank) * rays_per_rank, rays_per_rank


CENSUS_FIELDS = ("launched", "exited", "counted_below_z", "absorbed", "suspended", "bin_increments", "wall_hits")


def fluxmap_sharded(trace: Callable, cfg, n_total: int, seed: int, first_ray: int = 0, device=None):
    """Trace this rank's shard with `trace`, then all-reduce histogram and census over the default
    process group (if initialised).  Returns (hits[n_theta,n_phi] uint64, census dict) — identical on every rank."""
    import torch
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(), dist.get_world_size()
    else:
        rank, world = 0, 1
    first, count = shard(n_total, rank, world)
    hits, st = trace(cfg, count, seed, first_ray + first)
    census = np.array([getattr(st, k) for k in CENSUS_FIELDS], dtype=np.int64)
    if world > 1:
        buf = torch.from_numpy(np.concatenate([hits.reshape(-1).astype(np.int64), census]))
        if device is not None:
            buf = buf.to(device)
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
        buf = buf.cpu().numpy()
        hits = buf[:-len(CENSUS_FIELDS)].astype(np.uint64).reshape(hits.shape)
        census = buf[-len(CENSUS_FIELDS):]
    return hits, dict(zip(CENSUS_FIELDS, (int(x) for x in census)))


def disc_sweep_sharded(sweep: Callable, cfg, discs, radius: float, half_thick: float, n_total: int, seed: int,
                       first_ray: int = 0, device=None):
    """BASELINE.json configs[3] (integratingSphereDetectorSweep.C ray-sharded): every rank traces its slice of the
    n_total rays against ALL discs with `sweep(cfg, discs, radius, half_thick, count, seed, first) -> (hits, stats)`
    (altair_raytracing_amd.disc_sweep on a GPU box), then the per-disc counts and the census are summed by the same
    single all-reduce as the flux map."""
    return fluxmap_sharded(lambda c, count, s, first: sweep(c, discs, radius, half_thick, count, s, first),
                           cfg, n_total, seed, first_ray, device)


EXIT_COUNT_FIELDS = ("dir_binned", "dir_outside", "pos_binned", "pos_outside", "upward")


def exit_maps_sharded(trace: Callable, cfg, spec, n_total: int, seed: int, first_ray: int = 0, device=None):
    """The exit maps (altair_raytracing_amd.exit_maps) ray-sharded: this rank's contiguous shard through
    `trace(cfg, count, seed, spec, first) -> (dir_map, pos_map, counts, stats)`, then ONE SUM all-reduce that carries both
    maps, the five counters and the census.  Returns (dir_map, pos_map, counts dict, census dict) -- identical on every rank."""
    import torch
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(), dist.get_world_size()
    else:
        rank, world = 0, 1
    first, count = shard(n_total, rank, world)
    dmap, pmap, cnt, st = trace(cfg, count, seed, spec, first_ray + first)
    counts = np.array([getattr(cnt, k) for k in EXIT_COUNT_FIELDS], dtype=np.int64)
    census = np.array([getattr(st, k) for k in CENSUS_FIELDS], dtype=np.int64)
    if world > 1:
        buf = torch.from_numpy(np.concatenate([dmap.reshape(-1).astype(np.int64), pmap.reshape(-1).astype(np.int64), counts, census]))
        if device is not None:
            buf = buf.to(device)
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
        buf = buf.cpu().numpy()
        nd, npos = dmap.size, pmap.size
        dmap = buf[:nd].astype(np.uint64).reshape(dmap.shape)
        pmap = buf[nd:nd + npos].astype(np.uint64).reshape(pmap.shape)
        counts = buf[nd + npos:nd + npos + len(EXIT_COUNT_FIELDS)]
        census = buf[nd + npos + len(EXIT_COUNT_FIELDS):]
    return (dmap, pmap, dict(zip(EXIT_COUNT_FIELDS, (int(x) for x in counts))),
            dict(zip(CENSUS_FIELDS, (int(x) for x in census))))


WALL_COUNT_FIELDS = ("binned", "outside", "skipped", "other_surface")


def wall_map_sharded(trace: Callable, cfg, spec, n_total: int, seed: int, first_ray: int = 0, device=None):
    """The wall map (altair_raytracing_amd.wall_map) ray-sharded: this rank's contiguous shard through
    `trace(cfg, count, seed, spec, first) -> (wall_map, counts, stats)`, then ONE SUM all-reduce that carries the map, the
    four counters and the census.  Returns (wall_map, counts dict, census dict) -- identical on every rank."""
    import torch
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(), dist.get_world_size()
    else:
        rank, world = 0, 1
    first, count = shard(n_total, rank, world)
    wmap, cnt, st = trace(cfg, count, seed, spec, first_ray + first)
    counts = np.array([getattr(cnt, k) for k in WALL_COUNT_FIELDS], dtype=np.int64)
    census = np.array([getattr(st, k) for k in CENSUS_FIELDS], dtype=np.int64)
    if world > 1:
        buf = torch.from_numpy(np.concatenate([wmap.reshape(-1).astype(np.int64), counts, census]))
        if device is not None:
            buf = buf.to(device)
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
        buf = buf.cpu().numpy()
        nm = wmap.size
        wmap = buf[:nm].astype(np.uint64).reshape(wmap.shape)
        counts = buf[nm:nm + len(WALL_COUNT_FIELDS)]
        census = buf[nm + len(WALL_COUNT_FIELDS):]
    return (wmap, dict(zip(WALL_COUNT_FIELDS, (int(x) for x in counts))), dict(zip(CENSUS_FIELDS, (int(x) for x in census))))


FIELD_COUNT_FIELDS = ("binned", "pos_outside", "dir_outside", "upward")


def light_field_sharded(trace: Callable, cfg, spec, n_total: int, seed: int, first_ray: int = 0, device=None):
    """The port light field (altair_raytracing_amd.light_field) ray-sharded: this rank's contiguous shard through
    `trace(cfg, count, seed, spec, first) -> (field, counts, stats)`, then ONE SUM all-reduce that carries the field, the
    four counters and the census.  Returns (field, counts dict, census dict) -- identical on every rank."""
    import torch
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(), dist.get_world_size()
    else:
        rank, world = 0, 1
    first, count = shard(n_total, rank, world)
    field, cnt, st = trace(cfg, count, seed, spec, first_ray + first)
    counts = np.array([getattr(cnt, k) for k in FIELD_COUNT_FIELDS], dtype=np.int64)
    census = np.array([getattr(st, k) for k in CENSUS_FIELDS], dtype=np.int64)
    if world > 1:
        buf = torch.from_numpy(np.concatenate([field.reshape(-1).astype(np.int64), counts, census]))
        if device is not None:
            buf = buf.to(device)
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
        buf = buf.cpu().numpy()
        nf = field.size
        field = buf[:nf].astype(np.uint64).reshape(field.shape)
        counts = buf[nf:nf + len(FIELD_COUNT_FIELDS)]
        census = buf[nf + len(FIELD_COUNT_FIELDS):]
    return (field, dict(zip(FIELD_COUNT_FIELDS, (int(x) for x in counts))), dict(zip(CENSUS_FIELDS, (int(x) for x in census))))


ORDER_COUNT_FIELDS = ("overflow_port", "overflow_exited_other", "overflow_absorbed", "overflow_suspended", "dz_outside")


def order_hist_sharded(trace: Callable, cfg, spec, n_total: int, seed: int, first_ray: int = 0, device=None):
    """The bounce-order histograms (altair_raytracing_amd.order_hist) ray-sharded: this rank's contiguous shard through
    `trace(cfg, count, seed, spec, first) -> (hist, port_dz, counts, stats)`, then ONE SUM all-reduce that carries both arrays,
    the five counters (overflow[0..3], dz_outside) and the census.  Returns (hist, port_dz, counts dict, census dict) --
    identical on every rank."""
    import torch
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(), dist.get_world_size()
    else:
        rank, world = 0, 1
    first, count = shard(n_total, rank, world)
    hist, dz, cnt, st = trace(cfg, count, seed, spec, first_ray + first)
    counts = np.array([int(x) for x in cnt.overflow] + [int(cnt.dz_outside)], dtype=np.int64)
    census = np.array([getattr(st, k) for k in CENSUS_FIELDS], dtype=np.int64)
    if world > 1:
        buf = torch.from_numpy(np.concatenate([hist.reshape(-1).astype(np.int64), dz.reshape(-1).astype(np.int64), counts, census]))
        if device is not None:
            buf = buf.to(device)
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
        buf = buf.cpu().numpy()
        nh, nd, nc = hist.size, dz.size, len(ORDER_COUNT_FIELDS)
        hist = buf[:nh].astype(np.uint64).reshape(hist.shape)
        dz = buf[nh:nh + nd].astype(np.uint64).reshape(dz.shape)
        counts = buf[nh + nd:nh + nd + nc]
        census = buf[nh + nd + nc:]
    return (hist, dz, dict(zip(ORDER_COUNT_FIELDS, (int(x) for x in counts))), dict(zip(CENSUS_FIELDS, (int(x) for x in census))))


def wall_patches_sharded(trace: Callable, cfg, spec, n_total: int, seed: int, first_ray: int = 0, device=None):
    """The wall patches (altair_raytracing_amd.wall_patches) ray-sharded: this rank's contiguous shard through
    `trace(cfg, count, seed, spec, first) -> (arrivals, absorbed, stats)`, then ONE SUM all-reduce that carries the 2 (P + 2)
    counters and the census.  Returns (arrivals, absorbed, census dict) -- identical on every rank."""
    import torch
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(), dist.get_world_size()
    else:
        rank, world = 0, 1
    first, count = shard(n_total, rank, world)
    arr, ab, st = trace(cfg, count, seed, spec, first_ray + first)
    census = np.array([getattr(st, k) for k in CENSUS_FIELDS], dtype=np.int64)
    if world > 1:
        buf = torch.from_numpy(np.concatenate([arr.astype(np.int64), ab.astype(np.int64), census]))
        if device is not None:
            buf = buf.to(device)
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
        buf = buf.cpu().numpy()
        nc = arr.size
        arr = buf[:nc].astype(np.uint64)
        ab = buf[nc:2 * nc].astype(np.uint64)
        census = buf[2 * nc:]
    return arr, ab, dict(zip(CENSUS_FIELDS, (int(x) for x in census)))


def fluxmap_beam_sharded(trace: Callable, cfg, spec, n_total: int, seed: int, first_ray: int = 0, device=None):
    """The beam-source flux map (altair_raytracing_amd.fluxmap_beam) ray-sharded: this rank's contiguous shard through
    `trace(cfg, spec, count, seed, first) -> (hits, stats)`, then the flux map's ONE SUM all-reduce of histogram plus census.
    Returns (hits[n_theta, n_phi] uint64, census dict) -- identical on every rank."""
    return fluxmap_sharded(lambda c, count, s, first: trace(c, spec, count, s, first), cfg, n_total, seed, first_ray, device)


def fluxmap_baffle_sharded(trace: Callable, cfg, spec, n_total: int, seed: int, first_ray: int = 0, device=None):
    """The flux map with baffles (altair_raytracing_amd.fluxmap_baffle) ray-sharded: this rank's contiguous shard through
    `trace(cfg, spec, count, seed, first) -> (hits, counts, stats)`, then ONE SUM all-reduce that carries the histogram, the 16
    baffle counters and the census.  Returns (hits[n_theta, n_phi] uint64, arrivals[4, 2] uint64, absorbed[4, 2] uint64, census
    dict) -- identical on every rank."""
    import torch
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(), dist.get_world_size()
    else:
        rank, world = 0, 1
    first, count = shard(n_total, rank, world)
    hits, cnt, st = trace(cfg, spec, count, seed, first_ray + first)
    arr, ab = cnt.arrays()
    census = np.array([getattr(st, k) for k in CENSUS_FIELDS], dtype=np.int64)
    if world > 1:
        buf = torch.from_numpy(np.concatenate([hits.reshape(-1).astype(np.int64), arr.reshape(-1).astype(np.int64),
                                               ab.reshape(-1).astype(np.int64), census]))
        if device is not None:
            buf = buf.to(device)
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
        buf = buf.cpu().numpy()
        nh, na = hits.size, arr.size
        hits = buf[:nh].astype(np.uint64).reshape(hits.shape)
        arr = buf[nh:nh + na].astype(np.uint64).reshape(arr.shape)
        ab = buf[nh + na:nh + 2 * na].astype(np.uint64).reshape(ab.shape)
        census = buf[nh + 2 * na:]
    return hits, arr, ab, dict(zip(CENSUS_FIELDS, (int(x) for x in census)))


def fluxmap_scene_sharded(trace: Callable, cfg, spec, n_total: int, seed: int, first_ray: int = 0, device=None):
    """The flux map of a scene (altair_raytracing_amd.fluxmap_scene) ray-sharded: this rank's contiguous shard through
    `trace(cfg, spec, count, seed, first) -> (hits, counts, stats)`, then ONE SUM all-reduce that carries the histogram, the 36
    scene counters and the census.  Returns (hits[n_theta, n_phi] uint64, patch_arrivals[10] uint64, patch_absorbed[10] uint64,
    baffle arrivals[4, 2] uint64, baffle absorbed[4, 2] uint64, census dict) -- identical on every rank."""
    import torch
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(), dist.get_world_size()
    else:
        rank, world = 0, 1
    first, count = shard(n_total, rank, world)
    hits, cnt, st = trace(cfg, spec, count, seed, first_ray + first)
    parts = list(cnt.arrays())
    census = np.array([getattr(st, k) for k in CENSUS_FIELDS], dtype=np.int64)
    if world > 1:
        buf = torch.from_numpy(np.concatenate([hits.reshape(-1).astype(np.int64)] + [a.reshape(-1).astype(np.int64) for a in parts] +
                                              [census]))
        if device is not None:
            buf = buf.to(device)
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
        buf = buf.cpu().numpy()
        at = hits.size
        hits = buf[:at].astype(np.uint64).reshape(hits.shape)
        for k, a in enumerate(parts):
            parts[k] = buf[at:at + a.size].astype(np.uint64).reshape(a.shape)
            at += a.size
        census = buf[at:]
    return (hits, *parts, dict(zip(CENSUS_FIELDS, (int(x) for x in census))))


def scene_response_sharded(trace: Callable, cfg, scene, rspec, n_total: int, seed: int, first_ray: int = 0, device=None):
    """The response of a scene (altair_raytracing_amd.scene_response) ray-sharded: this rank's contiguous shard through
    `trace(cfg, scene, rspec, count, seed, first) -> (response, counts, stats)`, then ONE SUM all-reduce that carries the response,
    the 36 scene counters and the census -- fluxmap_scene_sharded with the response in the histogram's place.  Returns
    (response[21, B] uint64, patch_arrivals[10] uint64, patch_absorbed[10] uint64, baffle arrivals[4, 2] uint64, baffle
    absorbed[4, 2] uint64, census dict) -- identical on every rank."""
    return fluxmap_scene_sharded(lambda c, sp, count, sd, first: trace(c, sp, rspec, count, sd, first), cfg, scene, n_total, seed,
                                 first_ray, device)


def scene_view_sharded(trace: Callable, cfg, scene, vspec, n_total: int, seed: int, first_ray: int = 0, device=None):
    """The view of a wall detector of a scene (altair_raytracing_amd.scene_view) ray-sharded: this rank's contiguous shard through
    `trace(cfg, scene, vspec, count, seed, first) -> (view, view_counts, scene_counts, stats)`, then ONE SUM all-reduce that
    carries the map, the 4 view counters, the 36 scene counters and the census -- fluxmap_scene_sharded with the map and its four
    counters in the histogram's place.  Returns (view[n_v, n_u] uint64, view_counts[4] uint64 (binned, outside, behind, direct),
    patch_arrivals[10] uint64, patch_absorbed[10] uint64, baffle arrivals[4, 2] uint64, baffle absorbed[4, 2] uint64, census
    dict) -- identical on every rank."""
    shape = []

    def one(c, sp, count, sd, first):
        view, vc, cnt, st = trace(c, sp, vspec, count, sd, first)
        shape.append(view.shape)
        return np.concatenate([np.asarray(view, dtype=np.uint64).reshape(-1), vc.words()]), cnt, st

    out = fluxmap_scene_sharded(one, cfg, scene, n_total, seed, first_ray, device)
    return (out[0][:-4].reshape(shape[0]), out[0][-4:]) + tuple(out[1:])


def scene_patch_field_sharded(trace: Callable, cfg, scene, fspec, n_total: int, seed: int, first_ray: int = 0, device=None):
    """The patch field of a scene (altair_raytracing_amd.scene_patch_field) ray-sharded: this rank's contiguous shard through
    `trace(cfg, scene, fspec, count, seed, first) -> (field, field_counts, scene_counts, stats)`, then ONE SUM all-reduce that
    carries the field, the 5 field counters, the 36 scene counters and the census -- scene_view_sharded with the field and its
    five counters in the map's place.  Returns (field[n_y, n_x, n_v, n_u] uint64, field_counts[5] uint64 (binned, pos_outside,
    dir_outside, behind, direct), patch_arrivals[10] uint64, patch_absorbed[10] uint64, baffle arrivals[4, 2] uint64, baffle
    absorbed[4, 2] uint64, census dict) -- identical on every rank."""
    shape = []

    def one(c, sp, count, sd, first):
        field, fc, cnt, st = trace(c, sp, fspec, count, sd, first)
        shape.append(field.shape)
        return np.concatenate([np.asarray(field, dtype=np.uint64).reshape(-1), fc.words()]), cnt, st

    out = fluxmap_scene_sharded(one, cfg, scene, n_total, seed, first_ray, device)
    return (out[0][:-5].reshape(shape[0]), out[0][-5:]) + tuple(out[1:])


def scene_order_hist_sharded(trace: Callable, cfg, scene, ospec, n_total: int, seed: int, first_ray: int = 0, device=None):
    """The order histograms of a scene (altair_raytracing_amd.scene_order_hist) ray-sharded: this rank's contiguous shard through
    `trace(cfg, scene, ospec, count, seed, first) -> (hist, order_counts, scene_counts, stats)`, then ONE SUM all-reduce that
    carries the histograms, the 21 overflow counters, the 36 scene counters and the census -- scene_patch_field_sharded with the
    histograms and their overflow counters in the field's place.  Returns (hist[21, n_orders] uint64, overflow[21] uint64,
    patch_arrivals[10] uint64, patch_absorbed[10] uint64, baffle arrivals[4, 2] uint64, baffle absorbed[4, 2] uint64, census
    dict) -- identical on every rank."""
    shape = []

    def one(c, sp, count, sd, first):
        hist, oc, cnt, st = trace(c, sp, ospec, count, sd, first)
        shape.append(hist.shape)
        return np.concatenate([np.asarray(hist, dtype=np.uint64).reshape(-1), oc.words()]), cnt, st

    out = fluxmap_scene_sharded(one, cfg, scene, n_total, seed, first_ray, device)
    return (out[0][:-21].reshape(shape[0]), out[0][-21:]) + tuple(out[1:])


def scene_path_hist_sharded(trace: Callable, cfg, scene, pspec, n_total: int, seed: int, first_ray: int = 0, device=None):
    """The path histograms of a scene (altair_raytracing_amd.scene_path_hist) ray-sharded: this rank's contiguous shard through
    `trace(cfg, scene, pspec, count, seed, first) -> (hist, path_counts, scene_counts, stats)`, then ONE SUM all-reduce that
    carries the histograms, the 21 overflow counters, the 21 checksums, the 36 scene counters and the census --
    scene_order_hist_sharded with the path counts in the order counts' place.  The checksums are sums modulo 2^64: they travel as
    int64 words like the rest, and the all-reduce's wrapping sum is theirs.  Returns (hist[21, n_bins] uint64, overflow[21]
    uint64, checksum[21] uint64, patch_arrivals[10] uint64, patch_absorbed[10] uint64, baffle arrivals[4, 2] uint64, baffle
    absorbed[4, 2] uint64, census dict) -- identical on every rank."""
    shape = []

    def one(c, sp, count, sd, first):
        hist, pc, cnt, st = trace(c, sp, pspec, count, sd, first)
        shape.append(hist.shape)
        return np.concatenate([np.asarray(hist, dtype=np.uint64).reshape(-1), pc.words()]), cnt, st

    out = fluxmap_scene_sharded(one, cfg, scene, n_total, seed, first_ray, device)
    return (out[0][:-42].reshape(shape[0]), out[0][-42:-21], out[0][-21:]) + tuple(out[1:])
