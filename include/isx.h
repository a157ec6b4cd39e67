/*
 * isx.h — C ABI of libisx, the MI355X-native integrating-sphere ray tracer.
 *
 * This is the drop-in boundary for ONE hot path of bdagnillo/altair-raytracing:
 * the per-ray trace loop + port-escape test + detector flux histogram
 * (SURVEY.md §8).  The reference has no FFI of its own; the entry points below
 * are what a maintainer's ROOT-macro (or cgo/ctypes) stub would bind in place of
 *
 *   AOpticsManager::TraceNonSequential(ARay&/ARayArray*)   flux_at_observer/fluxAtObserverOptimize.C:254,295
 *   isRayPassingThroughExitPort()                          flux_at_observer/fluxAtObserver.C:162-166
 *   Detector::setPosition / Detector::checkIntersection    flux_at_observer/fluxAtObserver.C:49-107
 *   hitCount++ / fraction = hit/n                          flux_at_observer/fluxAtObserverOptimize.C:309-312,571
 *   trace-once endpoint binning                            flux_at_observer/fluxAtObserverFast.C:1269-1315
 *   BRDF::SampleDirection + second trace                   flux_at_observer/nonLambertianFlux.C:147-208,253-268
 *   addDetectorDisk / isRayHittingDetector                 integratingSphereDetectorSweep.C:134-172
 *
 * Rules of the boundary: plain C types only, caller owns every host buffer,
 * the library owns device memory between isx_init()/isx_shutdown(), calls are
 * blocking unless they take a stream, no exception ever crosses the ABI, every
 * function returns 0 or a negative isx_status.  There is NO CPU fallback: if no
 * gfx950 device (or the HIP runtime) is available every compute entry point
 * returns ISX_ERR_NO_DEVICE.
 *
 * Process model: the library is a process-wide singleton bound to ONE device by isx_init()
 * (one process per GPU, as the reference is one process per run); it is not re-entrant and
 * not thread-safe.  isx_init() with another device ordinal shuts the first binding down.
 */
#ifndef ISX_H
#define ISX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: isx_config starts with struct_size (a config whose size is not the library's is refused, so a field added by a
 *    later ABI can never be mis-read silently). */
#define ISX_ABI_VERSION 3
/* Results are a pure function of (configuration, seed, ray indices) AND of the random-number layout below; a build with
 * another ISX_STREAM_VERSION gives different (equally valid) histograms for the same seed.
 * 3: Philox4x32-10, counter (ray lo, ray hi, block, stream); interaction j takes words (2(j&1), 2(j&1)+1) of block j/2;
 *    absorption and azimuth share one word; Householder cosine emission.
 * 4: the same generator and word layout; the cosine emission is n + s with s a uniform point of the unit sphere in world
 *    coordinates (first word: its z, second word: its azimuth), left un-normalised on the inner sphere, and the next wall point
 *    is p - 2 (p.v)/(v.v) v.  The explicit and the chord trace mode visit the same wall points since. */
#define ISX_STREAM_VERSION 4

typedef enum isx_status {
  ISX_OK = 0,
  ISX_ERR_NO_DEVICE = -1,   /* HIP runtime/device missing: the product never falls back to the CPU */
  ISX_ERR_BAD_CONFIG = -2,  /* geometry/grid parameters out of the supported domain */
  ISX_ERR_BAD_ARG = -3,     /* null pointer, zero size ... */
  ISX_ERR_HIP = -4,         /* a HIP call failed; isx_last_hip_error() has the code */
  ISX_ERR_NOT_INIT = -5,
  ISX_ERR_TOO_LARGE = -6    /* n_rays per call above ISX_MAX_RAYS_PER_CALL (or records above ISX_MAX_LOG_RECORDS) */
} isx_status;

/* One call may trace at most this many rays (the library cuts a call into launches of at most 2^30 rays: a lane keeps a
 * 31-bit offset from its launch's first ray, a workgroup counts in 32-bit LDS bins).  Split larger jobs over calls.
 * Ray indices are 64-bit; first_ray + n_rays must not exceed 2^64 - 1 (ISX_ERR_BAD_ARG). */
#define ISX_MAX_RAYS_PER_CALL (1ull << 40)
/* isx_exit_directions keeps at most this many 32-byte records per call (8 GiB of device memory) */
#define ISX_MAX_LOG_RECORDS (1ull << 28)

/* source_model */
#define ISX_SOURCE_PENCIL 0 /* fluxAtObserver*.C: identical rays from src along dir            */
#define ISX_SOURCE_BRDF 1   /* nonLambertianFlux.C:235-304: primary trace, BRDF re-scatter, 2nd trace */

/* surface_model */
#define ISX_SURFACE_ROBAST 0 /* ABorderSurfaceCondition: Lambertian if `lambertian`, else rough specular   */
#define ISX_SURFACE_LOBE 1   /* "nonLambertianFlux copy.C":31-70,188-221 NonLambertianSurface: cos^2 lobe
                                within 60 deg of the normal by rejection sampling (the de-facto CustomMirror) */
/* trace_mode: how a Lambertian bounce off the INNER SPHERE finds the next wall point */
#define ISX_TRACE_EXPLICIT 0 /* sample a cosine-law direction, intersect the ray with the sphere              */
#define ISX_TRACE_CHORD 1    /* integrating-sphere identity: for cosine-law emission from a point of a sphere
                                the far intersection is UNIFORM over the sphere's area, so the next wall point
                                is sampled directly (1 sqrt + 1 sincos, no direction, no intersection); the
                                direction is only formed when the point falls in the port opening.  Same
                                distribution, different random history; rim/outer-sphere/non-Lambertian
                                interactions are always explicit. */
/* hit_line_mode: which line Detector::checkIntersection sees */
#define ISX_HITLINE_LAST_SEGMENT 0 /* last point + final direction (fluxAtObserverOptimize.C:309; canonical)   */
#define ISX_HITLINE_ORIGIN_COMPAT 1 /* what fluxAtObserverFast.C:1181-1201,1285-1288 effectively used because
                                       GetPoint(nPoints-2, buf) never fills buf: start (0,0,0), direction
                                       lastPoint/|lastPoint| - reproduces the old fluxmap_traceonce_* files */

/*
 * Geometry + surface + source + detector grid.  Field meaning follows the
 * reference constants: fluxAtObserverOptimize.C:33-41 (THETA_MAX, MAX_REFLECTIONS,
 * INNER/OUTER_RADIUS, REFLECTANCE, ROUGHNESS), :192-230 (setupOpticsManager),
 * :456-461,495 (n, exitPortZ, bins, detector size), fluxAtObserver.C:352-358 (grid).
 * Lengths in cm (AOpticsManager::cm() == 1).
 */
typedef struct isx_config {
  uint32_t struct_size;  /* sizeof(isx_config) of the caller's ABI; set by isx_default_config().  Every entry
                            point refuses (ISX_ERR_BAD_CONFIG) a config whose size is not the library's.  */
  uint32_t reserved0;    /* 0 */
  double r_in;           /* TGeoSphere rmin (100.1)                                   */
  double r_out;          /* TGeoSphere rmax (101)                                     */
  double theta_max_deg;  /* TGeoSphere theta2: shell spans polar angle [0,theta_max]  */
  double reflectance;    /* AMirror::SetReflectance                                   */
  double roughness_rad;  /* ABorderSurfaceCondition::SetGaussianRoughness (sigma)     */
  double box_half;       /* TGeoBBox half edge                                        */
  int32_t lambertian;    /* ABorderSurfaceCondition::EnableLambertian                 */
  int32_t max_points;    /* AOpticsManager::SetLimit                                  */
  double src[3];         /* ARay start point                                          */
  double dir[3];         /* ARay direction (normalised by the library)                */
  int32_t n_theta;       /* detector grid rows: theta_i=(i+.5)*90/n_theta              */
  int32_t n_phi;         /* detector grid cols: phi_j=(j+.5)*360/n_phi                 */
  double det_diameter;   /* Detector::width (used as a DIAMETER, fluxAtObserver.C:106) */
  double det_distance;   /* Detector::setPosition radius (100)                        */
  double exit_port_z;    /* exitPortZ (-100); also the point the detectors face       */
  int32_t source_model;  /* ISX_SOURCE_*                                              */
  int32_t surface_model; /* ISX_SURFACE_*                                             */
  double brdf[3];        /* BRDF(roughness, specular, diffuse) nonLambertianFlux.C:211 */
  int32_t hit_line_mode; /* ISX_HITLINE_*                                             */
  int32_t trace_mode;    /* ISX_TRACE_*                                               */
} isx_config;

/* Ray census of one call (all ranks' census add up). */
typedef struct isx_stats {
  uint64_t launched;
  uint64_t exited;          /* left the world box (ARayArray::GetExited)                  */
  uint64_t counted_below_z; /* exited with lastPoint.z < exit_port_z ("rays exiting port") */
  uint64_t absorbed;
  uint64_t suspended;       /* more than max_points track points                          */
  uint64_t bin_increments;  /* sum of the histogram this call added                        */
  uint64_t wall_hits;       /* mirror interactions (bounces) traced                        */
  double t_kernel_ms;       /* HIP-event time of the kernels of this call, on their stream */
} isx_stats;

/* Fill cfg with the reference's constants for src(-60,0,-75), dir(5,0,0), port 170 deg
 * (fluxAtObserverOptimize.C:33-41,892-896; 180x90 grid, 40 cm detector at 100 cm). */
void isx_default_config(isx_config* cfg);

/* Select device `device` (ordinal as seen by HIP), create stream + workspaces.      */
int isx_init(int device);
void isx_shutdown(void);
const char* isx_strerror(int status);
int isx_last_hip_error(void);
int isx_abi_version(void);
int isx_stream_version(void);
/* Name/arch/CU count of the bound device (buf may be NULL). Returns CU count or <0. */
int isx_device_info(char* buf, int buflen);

/*
 * Trace rays [first_ray, first_ray+n_rays) of stream `seed` and add, for every
 * detector position (i,j), the number of traced rays whose final line hits that
 * detector (Detector::checkIntersection) into hits[i*n_phi+j].
 * Replaces the per-position loop fluxAtObserverOptimize.C:542-579 / the
 * trace-once loops fluxAtObserverFast.C:1143-1315.
 * hits: caller-owned host buffer [n_theta*n_phi], ZEROED by the callee.
 */
int isx_fluxmap(const isx_config* cfg, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                uint64_t* hits, isx_stats* stats);

/*
 * Same, but ACCUMULATES (+=) into a device-resident histogram d_hits
 * [n_theta*n_phi] of uint64 (e.g. a torch tensor the caller will all-reduce
 * over RCCL) on the library's stream; returns after the kernels are enqueued.
 * isx_sync() waits; isx_take_stats() then returns the census + event time of
 * everything enqueued since the previous isx_take_stats().
 * ORDER ("call_overlap", below): the kernel that writes d_hits -- the binning
 * kernel -- runs on isx_stream(), behind whatever the caller enqueued there
 * before this call (a zeroing of d_hits, an all-reduce of the call before).
 * The kernels in front of it touch nothing of the caller's and may run on the
 * library's own streams, ahead of the earlier calls' binning.  Every other
 * entry point, isx_sync(), isx_take_stats(), isx_set_option() and
 * isx_shutdown() first order isx_stream() behind those streams: a caller who
 * knows only isx_stream() sees what a single stream would show.
 */
int isx_fluxmap_device(const isx_config* cfg, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                       uint64_t* d_hits);
int isx_sync(void);
int isx_take_stats(isx_stats* stats);
/* The hipStream_t the library launches on (so callers can order work after it). */
void* isx_stream(void);
/* HIP-event times (ms) of the kernels collected by the last blocking call / isx_take_stats(), by kind: single-kernel
 * launches, the trace kernel of a two-kernel pipeline (flux map, exit maps, disc sweep), its binning kernel.  Any pointer may be NULL.
 * Each kind is summed from its own events.  For enqueued calls under "call_overlap" the spans of consecutive calls overlap, and a
 * span holds the time its kernel spent sharing the machine with the others: the kinds (and isx_stats::t_kernel_ms, their sum) then
 * add up to more than the wall time of the sequence, and only the wall time compares with a build or a setting without the overlap. */
int isx_last_kernel_ms(double* single_ms, double* trace_ms, double* bin_ms);

/* Tuning/diagnostic switches.  None of them changes any result (a ray's history is a function of seed and index).
 *   "bin_mode"     1 (default) culled + classified binning, 0 brute-force reference-order test of every detector position
 *   "pipeline"     1 (default): the lean flux maps (headline, chord mode, BRDF source) run as two kernels -- a trace kernel
 *                  writes the exit lines (48 B per counted ray) to an HBM workspace, a binning kernel reads them; 0: one fused kernel
 *   "pipeline_chunk"  rays per trace / binning pair, default and maximum 2^26.  WORKSPACE: exit lines live in regions of 1024
 *                  slots; a chunk of n rays traced by W waves is given n/961 + W + 1 regions of 48 KB (3.4 GB for 2^26 rays),
 *                  allocated once and kept until isx_shutdown(); "overlap" keeps three of them
 *   "assist"       1 (default): trace kernels with an assist wave per workgroup -- the flux-map pipelines, the
 *                  shared-ray disc sweep and the per-position sinks (isx_fluxmap_per_position, isx_disc_sweep_per_position);
 *                  0: round 2's kernels;
 *                  "assist_block" = their workgroup size (128..768, default 768 = 11 tracer waves + 1 assist wave)
 *   "bin_slots"    1 (default): binning kernels with slot queues by window length (grids up to 256 x 255); 0: round 2's
 *   "bin_cols"     1 (default; 2 is accepted and means the same): (line, COLUMN) slots for every source -- caps of the lines that
 *                  pass near the detector sphere's centre, cap-and-band windows for grazing lines; 0: (line, row) slots
 *   "surface_pipeline"  1 (default, round 5): the cos^2-lobe and rough-specular borders (pencil source) and the origin-compat hit
 *                  line run on the assist-wave pipeline too (isx_trace_assist_lobe_kernel / ..._rough_kernel; the compat lines are
 *                  rewritten by isx_compat_lines_kernel between the trace and the binning kernel); 0: round 1's fused
 *                  isx_trace_bin_full_kernel
 *   "lf_global"    0 (default): isx_light_field bins a field of at most 32 768 words in the workgroup's LDS and a larger one with
 *                  one global atomic add per ray; 1: the global form for every field (a diagnostic)
 *   "resp_global"  0 (default): isx_scene_response keeps a response that fits in the workgroup's LDS there and takes one global
 *                  atomic add per ended ray for a larger one; 1: the global form for every spec (a diagnostic)
 *   "view_global"  0 (default): isx_scene_view keeps a map that fits in the workgroup's LDS there and takes one global atomic
 *                  add per binned ray for a larger one; 1: the global form for every spec (a diagnostic)
 *   "field_global" 0 (default): isx_scene_patch_field keeps a field that fits in the workgroup's LDS there and takes one global
 *                  atomic add per binned ray for a larger one; 1: the global form for every spec (a diagnostic)
 *   "sorder_lds_orders"  how many orders of every fate slot isx_scene_order_hist keeps as u32 words in the workgroup's LDS: -1
 *                  (default) as many as fit without costing a resident workgroup, n > 0 at most n of those, 0 none -- one
 *                  global atomic add per ended ray (a diagnostic).  It changes no result.
 *   "spath_lds_bins"  how many bins of every fate slot isx_scene_path_hist keeps as u32 words in the workgroup's LDS: -1
 *                  (default) as many as fit without costing a resident workgroup, n > 0 at most n of those, 0 none -- one
 *                  global atomic add per ended ray (a diagnostic).  It changes no result.
 *   "bin_block", "bin_blocks_per_cu"  shape of round 2's binning kernel (0 workgroups per CU = what is resident)
 *                  (round 5: "assist_block" 0 = the default again -- 768 threads, 256 for launches below 1e6 rays, 512 for the lobe /
 *                  rough-specular kernels; "rays_per_lane" > 0 sizes every grid for that many rays per tracer lane, 0 = by launch
 *                  size: 1 below 1.5e5 rays, 2 below 3e5, else 4 -- a small launch is bound by its longest ray, not by throughput)
 *   "ray_sub"      rays a wave takes off a launch's ray queue at a time (0 = default: 128)
 *   "fate_scan"    a SCHEDULING option, it changes no result: -1 (default) automatic, 1 on wherever eligible, 0 off.  On the headline
 *                  path of isx_fluxmap / isx_fluxmap_device (pencil source whose first strike lies on the mirror patch, Lambertian
 *                  border, explicit bounces, "assist" 1, no "overlap") isx_fate_scan_kernel first walks every ray of a chunk over
 *                  its Philox words alone and settles the rays the inner wall absorbs -- launched, absorbed and wall_hits are all
 *                  they add to a result; the trace kernel then runs on the list of the others, each from its first interaction
 *                  (DESIGN.md 4.2d).  Automatic: chunks of at least 1e7 rays whose expected settled share
 *                  (1 - rho) / ((1 - rho) + port area fraction) is at least 0.5.  Anything else takes the kernels it took before,
 *                  also with 1.  WORKSPACE: 4 B per ray of the largest chunk, kept until isx_shutdown()
 *   "exit_scan"    changes no result: -1 (default) automatic, 1 on wherever eligible, 0 off.  Behind the fate scan (its
 *                  eligibility; "exit_scan" 1 brings the scan with it unless "fate_scan" is 0), with the last-segment hit line and
 *                  the column-slot binning kernel: isx_exit_lines_kernel forms the exit line of every ray that leaves cleanly
 *                  through the port from the ray's Philox words, with a proven bound on its deviation; the trace kernel runs on
 *                  the rest; the binning kernel decides a candidate of such a line only where every line within the bound gives
 *                  the same answer, and isx_redo_kernel traces the few rays that are left.  Automatic: the fate
 *                  scan's rule.  Anything else takes the kernels it took before, also with 1.  WORKSPACE: 24 B per ray of the
 *                  largest chunk and 8 B per exit-line slot, kept until isx_shutdown().  "exit_eps_scale" (tests; >= 1, default 1)
 *                  multiplies every bound, so that a test-sized run reaches the redo kernel
 *   "call_overlap"  a SCHEDULING option, it changes no result: -1 (default) automatic, 1 on wherever eligible, 0 off.  Eligible are
 *                  isx_fluxmap_device calls that take the two-kernel flux pipeline with explicit bounces, with or without the fate
 *                  scan, and not with "overlap" > 1.  The chunk's counter zeroing, fate scan, trace kernel and
 *                  isx_compat_lines_kernel go to a trace stream of the library's, its binning kernel stays on isx_stream() behind an
 *                  event: the next call's scan and trace run under the launch tails of this one.  Automatic: every
 *                  eligible call (measured faster from 5e4 to 5e7 rays per call).  "call_overlap_streams" 2 (default): consecutive
 *                  chunks alternate between two trace streams; 1: one.  WORKSPACE: three exit-line workspaces and three fate
 *                  lists of the largest chunk instead of one, kept until isx_shutdown()
 *   "overlap", "overlap_trace_streams"  cut a flux-map call into k chunks, binning of chunk i on a second stream while chunk
 *                  i+1 is traced (measured slower on MI355X, default 0)
 *   "disc_pipeline"  1 (default): the shared-ray disc sweep as trace kernel + disc-binning kernel (discs clustered by eight on the
 *                  host, exit segments in HBM); 0: one fused kernel
 *   "blocks_per_cu", "grid_blocks" (0 = auto), "trace_block" (64..1024, default 512), "trace_blocks_per_cu" (0 = resident)
 *                  launch shapes; "sched_mask", "sched_min": batching of the generic boundary search in the kernels without
 *                  an assist wave (every (mask+1)-th loop trip or when `min` lanes wait). */
int isx_set_option(const char* key, int64_t value);

/* Device-side probe of the numeric contract (tests): out[i] = op(a[i],b[i],c[i]) with
 * op 0 sqrt, 1 a/b, 2 fma, 3 log, 4/5 sin/cos(2*pi*a), 6/7 sin/cos(a), 8 the hot loop's sqrt for operands
 * in [2^-33,1], 9 its -1/x for |x| in [1,2] (both must equal the IEEE results),
 * 10/11 cos/sin of the emission azimuth (oracle: isxo_circle_point), 12/13/14 the x/y/z of TVector3(a,b,c).Unit() as the lobe
 * sampler forms it (must equal the plain-operation result). */
int isx_mathprobe(int op, const double* a, const double* b, const double* c, double* out, int32_t n);

/*
 * Per-ray end states, for parity tests against the oracle: status (isx_ray_status),
 * last point, final direction, number of track points.  Host buffers sized n_rays.
 */
typedef enum isx_ray_status { ISX_RAY_EXITED = 1, ISX_RAY_ABSORBED = 2, ISX_RAY_SUSPENDED = 3 } isx_ray_status;
int isx_trace_endstates(const isx_config* cfg, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                        int32_t* status, int32_t* n_points, double* last_point /*[n][3]*/,
                        double* direction /*[n][3]*/);

/*
 * Diagnostic of the "fate_scan" option (tests): the scan's rule per ray, in index order.  fate[i] = ISX_RAY_ABSORBED (2) if the
 * scan settles ray first_ray + i as absorbed at interaction order[i] (isx_trace_endstates then reports ISX_RAY_ABSORBED and
 * n_points = order[i] + 2), or 0 if it leaves the ray to the trace kernel, undecided at interaction order[i].  Host buffers sized
 * n_rays.  ISX_ERR_BAD_CONFIG for a configuration the scan does not serve.
 */
int isx_fate_scan(const isx_config* cfg, uint64_t n_rays, uint64_t seed, uint64_t first_ray, int32_t* fate, int32_t* order);
/* Chunks that took the scan since isx_init (one isx_fate_scan_kernel launch each): shows which path a call took (tests). */
int isx_fate_scan_launches(uint64_t* launches);
/* The "exit_scan" path since isx_init (tests; any pointer may be NULL): rays whose exit line isx_exit_lines_kernel formed from
 * their words, rays it left to the trace kernel, and candidates the binning kernel left to isx_redo_kernel.  Synchronises. */
int isx_exit_scan_counts(uint64_t* accepted, uint64_t* list_b, uint64_t* redo);

/*
 * Physical-disc sweep (integratingSphereDetectorSweep.C:31-105,145-172): n_disc
 * discs (centre[3], unit axis[3]) of radius `radius`, half thickness `half_thick`;
 * hits[k] = number of rays whose forward exit segment enters disc k's volume.
 */
int isx_disc_sweep(const isx_config* cfg, const double* centers_axes /*[n_disc][6]*/, int32_t n_disc,
                   double radius, double half_thick, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                   uint64_t* hits, isx_stats* stats);

/*
 * The same sweep as the reference WRITES it (integratingSphereDetectorSweep.C:54-77): every disc position k gets its
 * own `rays_per_position` fresh rays [first_ray + k*rays_per_position, +rays_per_position) and only those are tested
 * against disc k -- all positions in ONE launch (362 positions x 1e5 rays for the macro's defaults).
 */
int isx_disc_sweep_per_position(const isx_config* cfg, const double* centers_axes /*[n_disc][6]*/, int32_t n_disc,
                                double radius, double half_thick, uint64_t rays_per_position, uint64_t seed,
                                uint64_t first_ray, uint64_t* hits, isx_stats* stats);

/*
 * The reference's PER-POSITION maps: every detector position gets its own
 * `rays_per_position` fresh rays (fluxAtObserverOptimize.C:542-579, n=50000 => 8.1e8 rays
 * for 180x90).  Rays [first_ray + g*rays_per_position, +rays_per_position) belong to
 * detector group g and are tested against that group only.  fold=1: group g is bin g
 * (theta-major).  fold=2 is the "twofold" variant (fluxAtObserverFast.C:336-408,518-865):
 * group g = (i, j<n_phi/2) feeds the two detectors (i,j) and (i,j+n_phi/2).
 * Groups [first_group, first_group+n_groups) are traced (so ranks can split a map);
 * hits: host buffer [n_theta*n_phi], zeroed by the callee.
 */
int isx_fluxmap_per_position(const isx_config* cfg, uint64_t rays_per_position, int32_t fold, uint64_t first_group,
                             uint64_t n_groups, uint64_t seed, uint64_t first_ray, uint64_t* hits, isx_stats* stats);

/*
 * int traceRays(AOpticsManager*, int n, double exitPortZ, Detector&, bool) (fluxAtObserver.C:169,
 * fluxAtObserverOptimize.C:239,281): n rays against ONE detector given as x,y,z,nx,ny,nz
 * (what Detector::setPosition left in the struct) and its width.
 */
int isx_trace_rays_detector(const isx_config* cfg, const double* detector /*[6]*/, double width, uint64_t n_rays,
                            uint64_t seed, uint64_t first_ray, uint64_t* hit_count, isx_stats* stats);

/*
 * Exit-direction by-product (distributionSphereDetectorSweep.C:54,91): histogram of the z
 * component of the final direction of every ray counted below exit_port_z,
 * TH1D(nbins,-1,1) binning.  hist: host buffer [nbins], zeroed by the callee.
 */
int isx_exit_dz_hist(const isx_config* cfg, uint64_t n_rays, uint64_t seed, uint64_t first_ray, int32_t nbins,
                     uint64_t* hist, isx_stats* stats);

/*
 * Un-binned exit log (the committed 3dRayLog.txt, "# dx dy dz"): ray index and final unit
 * direction of every ray counted below exit_port_z, sorted by ray index.  capacity = room in
 * ray_ids[capacity] / directions[capacity][3] (at most ISX_MAX_LOG_RECORDS are kept, more is ISX_ERR_TOO_LARGE;
 * a capacity above n_rays is treated as n_rays); *count = number of such rays (may exceed capacity:
 * the surplus is dropped).  This is the one sink with real HBM output (32 B per exiting ray).
 */
int isx_exit_directions(const isx_config* cfg, uint64_t n_rays, uint64_t seed, uint64_t first_ray, uint64_t capacity,
                        uint64_t* ray_ids, double* directions, uint64_t* count, isx_stats* stats);

/*
 * Exit maps: what an observer FAR from the port sees, and the irradiance over a plane below it.  The flux map tests finite
 * detector discs; the limit "detector -> point at infinity" of that map is the 2-D histogram of the exit direction (radiant
 * intensity), which no finite detector reaches by Monte Carlo.  One call bins, for every traced ray that the census counts as
 * "counted below z" (status EXITED and last_point.z < cfg->exit_port_z -- the rays of isx_exit_dz_hist / isx_exit_directions;
 * for ISX_SOURCE_BRDF the scattered ray), with p = last point and v = final direction as isx_trace_endstates returns them
 * (cfg->hit_line_mode is ignored: the maps always see the real last segment):
 *
 *   direction map (direction-cosine space; a Lambertian port gives a flat map inside the unit disc, radiant intensity per
 *   steradian is count / (N du dv / |dz|)):
 *       fu = (v.x + 1.0) * 0.5 * n_u ;  iu = (int)floor(fu)          (same with v.y, n_v -> iv)
 *       0 <= iu < n_u and 0 <= iv < n_v :  dir_map[iv * n_u + iu] += 1 ,  dir_binned += 1
 *       else                            :  dir_outside += 1           (|component| == 1 exactly)
 *
 *   plane map (where the exit LINE crosses the plane z = plane_z; free space -- the world box is no obstacle, a screen may lie
 *   inside or beyond it):
 *       v.z < 0.0 is false              :  upward += 1 , not binned   (-0.0 and +0.0 are "upward")
 *       t = (plane_z - p.z) / v.z
 *       x = p.x + t * v.x ;  y = p.y + t * v.y                        (a multiply, then an add: no fma)
 *       fx = (x + half_extent) / (2.0 * half_extent) * n_x ;  ix = (int)floor(fx)     (same for y, n_y -> iy)
 *       0 <= ix < n_x and 0 <= iy < n_y :  pos_map[iy * n_x + ix] += 1 ,  pos_binned += 1
 *       else (NaN / inf included)       :  pos_outside += 1
 *
 * All operations are IEEE double, evaluated left to right as written, the division correctly rounded.  For every call and
 * every map that is wanted: dir_binned + dir_outside == stats.counted_below_z == pos_binned + pos_outside + upward,
 * dir_map sums to dir_binned, pos_map to pos_binned, stats.bin_increments == dir_binned + pos_binned.  The counters of a map
 * that is not wanted stay 0.  The result does not depend on any isx_set_option switch nor on how a job is cut into calls.
 *
 * Limits (the two u32 maps of a workgroup live in its LDS): each map at most ISX_EXIT_MAP_MAX_BINS bins, each axis
 * 1..ISX_EXIT_MAP_MAX_AXIS, at least one map wanted, plane_z and half_extent finite, half_extent > 0 -- else ISX_ERR_BAD_CONFIG.
 */
#define ISX_EXIT_MAP_MAX_BINS 16384
#define ISX_EXIT_MAP_MAX_AXIS 1024
typedef struct isx_exit_map_spec {
  uint32_t struct_size;      /* sizeof(isx_exit_map_spec), set by isx_default_exit_map_spec(); a spec of another size is refused */
  uint32_t reserved0;        /* 0 */
  int32_t n_u, n_v;          /* direction map; 0,0 = not wanted (its pointer may then be NULL) */
  int32_t n_x, n_y;          /* plane map;     0,0 = not wanted */
  double plane_z;            /* plane map only */
  double half_extent;        /* plane map only: it covers [-half_extent, half_extent] in x and in y */
} isx_exit_map_spec;
typedef struct isx_exit_map_counts {
  uint64_t dir_binned, dir_outside, pos_binned, pos_outside, upward;
} isx_exit_map_counts;

/* 128 x 128 bins over the direction cosines, 64 x 64 bins at plane_z = cfg->exit_port_z with
 * half_extent = 1.25 * r_in * sin(theta_max) (the port radius + 25 %).  No GPU needed. */
void isx_default_exit_map_spec(const isx_config* cfg, isx_exit_map_spec* spec);

/* Blocking: dir_map[n_v * n_u], pos_map[n_y * n_x], *counts (host, zeroed by the callee; counts and stats may be NULL). */
int isx_exit_maps(const isx_config* cfg, const isx_exit_map_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                  uint64_t* dir_map, uint64_t* pos_map, isx_exit_map_counts* counts, isx_stats* stats);
/* ACCUMULATES (+=) into device-resident maps and five device counters (order of isx_exit_map_counts) on the library's
 * stream and returns after enqueueing; isx_sync() / isx_take_stats() as for isx_fluxmap_device. */
int isx_exit_maps_device(const isx_config* cfg, const isx_exit_map_spec* spec, uint64_t n_rays, uint64_t seed,
                         uint64_t first_ray, uint64_t* d_dir_map, uint64_t* d_pos_map, uint64_t* d_counts /*[5]*/);

/*
 * Wall map: where the light strikes the INSIDE of the sphere.  An integrating sphere exists to produce a spatially uniform
 * irradiance on its wall; this call is the 2-D histogram of every mirror interaction on the inner sphere, in an equal-area
 * projection, so that a uniformly irradiated wall gives a flat map.  For every mirror interaction that the census counts in
 * isx_stats.wall_hits take q, the interaction point (the point isx_trace_endstates would report as last_point if the ray ended
 * there; with ISX_TRACE_CHORD the sampled wall point), j, the ray's interaction count BEFORE this interaction (0-based; it
 * restarts at 0 for the scattered trace of ISX_SOURCE_BRDF), and the kind of surface:
 *
 *       kind is not the inner sphere (rim cone, outer sphere)  :  other_surface += 1
 *       j < spec.first_order                                   :  skipped += 1
 *       inv = 1.0 / cfg->r_in                  (once, on the host)
 *       c  = q.z * inv
 *       w  = sqrt(0.5 / (1.0 + c))
 *       X  = (q.x * inv) * w ;  Y = (q.y * inv) * w
 *       fx = (X + 1.0) * 0.5 * n_x ;  ix = (int)floor(fx)       (same with Y, n_y -> iy)
 *       0 <= ix < n_x and 0 <= iy < n_y  :  wall_map[iy * n_x + ix] += 1 ,  binned += 1
 *       else (NaN / inf included)        :  outside += 1
 *
 * All operations are IEEE double, evaluated left to right as written, no fma, division and square root correctly rounded.
 * (X, Y) is the Lambert azimuthal equal-area projection about +z scaled to the unit disc: the wall is the disc of radius
 * sin(theta_max / 2), the port the ring outside it; equal areas of the sphere are equal areas of the map; the irradiance in
 * rays per unit area is count / (4 pi r_in^2 * (2 / n_x) (2 / n_y) / pi).  first_order = 1 leaves out the first strike of
 * every ray (the bright spot of the pencil source) and shows the diffuse field alone.
 *
 * For every call: binned + outside + skipped + other_surface == stats.wall_hits, wall_map sums to binned,
 * stats.bin_increments == binned, and every other field of stats is what isx_fluxmap reports for the same (cfg, n_rays, seed,
 * first_ray).  The result does not depend on any isx_set_option switch nor on how a job is cut into calls.  cfg->hit_line_mode
 * and the detector-grid fields of cfg are ignored.
 *
 * Limits (a workgroup keeps the u32 map in its LDS next to the rings of its trace kernel): n_x * n_y at most
 * ISX_WALL_MAP_MAX_BINS, each axis 1..ISX_WALL_MAP_MAX_AXIS, first_order >= 0 -- else ISX_ERR_BAD_CONFIG.
 */
#define ISX_WALL_MAP_MAX_BINS 8192
#define ISX_WALL_MAP_MAX_AXIS 512
typedef struct isx_wall_map_spec {
  uint32_t struct_size;      /* sizeof(isx_wall_map_spec), set by isx_default_wall_map_spec(); a spec of another size is refused */
  uint32_t reserved0;        /* 0 */
  int32_t n_x, n_y;
  int32_t first_order;       /* interactions with j < first_order are counted in `skipped`, not binned */
  int32_t reserved1;         /* 0 */
} isx_wall_map_spec;
typedef struct isx_wall_map_counts {
  uint64_t binned, outside, skipped, other_surface;
} isx_wall_map_counts;

/* 64 x 64 bins, first_order 0.  No GPU needed. */
void isx_default_wall_map_spec(const isx_config* cfg, isx_wall_map_spec* spec);

/* Blocking: wall_map[n_y * n_x], *counts (host, zeroed by the callee; counts and stats may be NULL).  Without a HIP device:
 * ISX_ERR_NO_DEVICE; with one but before isx_init(): ISX_ERR_NOT_INIT. */
int isx_wall_map(const isx_config* cfg, const isx_wall_map_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                 uint64_t* wall_map, isx_wall_map_counts* counts, isx_stats* stats);
/* ACCUMULATES (+=) into a device-resident map and four device counters (order of isx_wall_map_counts) on the library's
 * stream and returns after enqueueing; isx_sync() / isx_take_stats() as for isx_fluxmap_device. */
int isx_wall_map_device(const isx_config* cfg, const isx_wall_map_spec* spec, uint64_t n_rays, uint64_t seed,
                        uint64_t first_ray, uint64_t* d_wall_map, uint64_t* d_counts /*[4]*/);

/*
 * Port light field: the radiance of the port as a function of position AND direction.  The exit maps are its two marginals (the
 * direction map summed over the port, the plane map summed over all directions); what says whether the port is a uniform source
 * from every viewing angle, and what any camera or detector in free space would read, is the joint quantity L(x, y, u, v) over
 * the plane z = plane_z.  In direction-cosine space (u, v) = (v.x, v.y) the cos(theta) of the projected area and the solid angle
 * cancel: radiance = count / (N dx dy du dv) with dx = 2 half_extent / n_x, dy = 2 half_extent / n_y, du = 2 / n_u, dv = 2 / n_v,
 * and a Lambertian, uniform port gives a flat 4-D field.
 *
 * The spec is an isx_exit_map_spec: the same six fields with the same meaning, all four axes >= 1.  For every ray the census
 * counts in counted_below_z, with p = last point and v = final direction as isx_trace_endstates returns them
 * (cfg->hit_line_mode is ignored; for ISX_SOURCE_BRDF the scattered ray), in this order:
 *
 *       v.z < 0.0 is false                        :  upward += 1                     (as in the plane map)
 *       (ix, iy) by the plane map's formulas above, operation for operation (t, x, y, fx, fy, floor)
 *       not (0 <= ix < n_x and 0 <= iy < n_y)     :  pos_outside += 1                (NaN / inf included)
 *       (iu, iv) by the direction map's formulas above, operation for operation
 *       not (0 <= iu < n_u and 0 <= iv < n_v)     :  dir_outside += 1                (only rays that have a position bin)
 *       else  field[((iy * n_x + ix) * n_v + iv) * n_u + iu] += 1 ,  binned += 1
 *
 * All operations are IEEE double, evaluated left to right as written, no fma.  For every call:
 * binned + pos_outside + dir_outside + upward == stats.counted_below_z, field sums to binned, stats.bin_increments == binned,
 * every other field of stats is what isx_fluxmap reports for the same (cfg, n_rays, seed, first_ray), and upward and pos_outside
 * equal those of isx_exit_maps for the same (n_x, n_y, plane_z, half_extent).  The result does not depend on any
 * isx_set_option switch nor on how a job is cut into calls.
 *
 * Limits: each axis 1..ISX_LIGHT_FIELD_MAX_AXIS, n_x * n_y * n_u * n_v at most ISX_LIGHT_FIELD_MAX_BINS (32 MiB of uint64),
 * plane_z and half_extent finite, half_extent > 0, struct_size == sizeof(isx_exit_map_spec) -- else ISX_ERR_BAD_CONFIG; a NULL
 * spec or field: ISX_ERR_BAD_ARG.  Both are answered whether or not a device is present.  A field of at most 32 768 words is
 * binned in the workgroups' LDS, a larger one with one global atomic add per binned ray ("lf_global").
 */
#define ISX_LIGHT_FIELD_MAX_BINS (1 << 22)
#define ISX_LIGHT_FIELD_MAX_AXIS 1024
typedef struct isx_light_field_counts {
  uint64_t binned, pos_outside, dir_outside, upward;
} isx_light_field_counts;

/* 32 x 32 position bins at plane_z = cfg->exit_port_z with the exit maps' default half_extent, 32 x 32 direction bins.
 * No GPU needed. */
void isx_default_light_field_spec(const isx_config* cfg, isx_exit_map_spec* spec);

/* Blocking: field[n_y * n_x * n_v * n_u], *counts (host, zeroed by the callee; counts and stats may be NULL).  Without a HIP
 * device: ISX_ERR_NO_DEVICE; with one but before isx_init(): ISX_ERR_NOT_INIT (as isx_wall_map). */
int isx_light_field(const isx_config* cfg, const isx_exit_map_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                    uint64_t* field, isx_light_field_counts* counts, isx_stats* stats);
/* ACCUMULATES (+=) into a device-resident field and four device counters (order of isx_light_field_counts) on the library's
 * stream and returns after enqueueing; isx_sync() / isx_take_stats() as for isx_fluxmap_device. */
int isx_light_field_device(const isx_config* cfg, const isx_exit_map_spec* spec, uint64_t n_rays, uint64_t seed,
                           uint64_t first_ray, uint64_t* d_field, uint64_t* d_counts /*[4]*/);

/*
 * The binning kernels alone, on exit lines the CALLER supplies (parity tests: lines placed on a detector's rim, on the parallel
 * cut, on the thresholds of the cull -- what traced rays do not reach in a test-sized run).  No ray is traced: the lines are
 * laid into the pipeline's workspace exactly as a trace kernel leaves them -- regions of 1024 slots, a line count per region --
 * and the binning kernel that the launch plan selects for (cfg, sink, the current isx_set_option switches) runs on them, with the
 * plan's workgroup shape, LDS and grid ("bin_cols", "bin_slots", "bin_block", "bin_blocks_per_cu", "grid_blocks", "lf_global" keep
 * their meaning); with ISX_HITLINE_ORIGIN_COMPAT and the flux sink the pipeline's line-rewriting kernel runs first.
 *
 *   sink  ISX_INJECT_FLUX         hits of isx_fluxmap:      out_a = hits[n_theta * n_phi], out_b and counts unused (may be NULL)
 *         ISX_INJECT_EXIT_MAPS    maps of isx_exit_maps:    out_a = dir_map[n_v * n_u], out_b = pos_map[n_y * n_x] (NULL for a map
 *                                 that is not wanted), counts[5] in the order of isx_exit_map_counts
 *         ISX_INJECT_LIGHT_FIELD  field of isx_light_field: out_a = field[n_y * n_x * n_v * n_u], counts[4] in the order of
 *                                 isx_light_field_counts
 *   spec  the isx_exit_map_spec of the latter two sinks (ignored, may be NULL, for the flux sink)
 *   lines[n][6]  last point, direction.  Every line counts as "counted below z": no census is taken, cfg's geometry and source
 *         are looked at only where the launch plan does
 *   region_counts[n_regions]  how the lines are laid out: region r holds the next region_counts[r] lines (each 0..1024, their
 *         sum n, n_regions 1..ISX_INJECT_MAX_REGIONS).  NULL with n_regions 0: full regions, the rest in the last.  The slots of a
 *         region that hold no line are filled with one valid line straight down the axis through (0, 0, exit_port_z), which hits
 *         every detector of the rows about the axis: a kernel that reads past a region's count shows up as extra counts
 *   unit  ISX_INJECT_UNIT_AUTO: work units as the pipeline sizes them (64 lines below 1e6 lines, else 256); 0: 256 lines; 2: 64 lines
 *
 * out_a, out_b and counts are HOST arrays and ACCUMULATE (+=); *bin_increments (may be NULL) is set to what this call added.
 * Blocking.  The result does not depend on the layout, the unit, the order of the lines or any switch.
 *
 * Domain of the flux sink: the flux binners are written for unit directions (the foot of the line is h = P - (P.V) V) and for
 * points within the reach of a traced ray -- the world box, |P| <= sqrt(3) cfg->box_half (520 cm for the reference's 300) -- which
 * is what the float32 margins of their cull are written and tested for; their loops must never see anything else.  Refused with ISX_ERR_BAD_ARG, before
 * any device is asked for: a NULL cfg, lines (with n > 0) or accumulator the sink writes; a sink or unit that is none of the
 * above; n above ISX_INJECT_MAX_LINES (ISX_ERR_TOO_LARGE, as is host memory that cannot be had for the staging copy); n_regions or a region count out of range, counts that do not sum to n;
 * and for the flux sink any coordinate that is not finite, a direction with | |V| - 1 | > 1e-12, a point with
 * |P|^2 > 3 cfg->box_half^2.  ISX_ERR_BAD_CONFIG, likewise before the device: a config or spec that the sink's public call
 * refuses.  The exit-map and light-field sinks take any doubles: their contract defines NaN and inf as "outside".
 * With a device, ISX_ERR_BAD_CONFIG as well where the plan has no binning kernel for the call: a flux grid whose histogram and
 * tables do not fit the binning kernels' LDS (isx_fluxmap then runs the fused kernel), "pipeline" 0, "bin_mode" 0 or 2, a border /
 * source combination that the pipeline does not serve.  The disc sweep's binning kernel (8-double segments) is not reachable here:
 * isx_bin_injected_segments below.
 */
#define ISX_INJECT_FLUX 0
#define ISX_INJECT_EXIT_MAPS 1
#define ISX_INJECT_LIGHT_FIELD 2
#define ISX_INJECT_UNIT_AUTO (-1)
/* (a diagnostic entry: the lines are staged once on the host and once on the device, 48 KiB per region -- 48 MiB at the most) */
#define ISX_INJECT_MAX_LINES (1u << 20)
#define ISX_INJECT_MAX_REGIONS 1024
int isx_bin_injected_lines(const isx_config* cfg, int32_t sink, const isx_exit_map_spec* spec, const double* lines /*[n][6]*/,
                           uint64_t n, const uint32_t* region_counts, int32_t n_regions, int32_t unit, uint64_t* out_a,
                           uint64_t* out_b, uint64_t* counts, uint64_t* bin_increments);

/*
 * The same for the shared-ray disc sweep (isx_disc_sweep on its two-kernel route): the sweep's binning kernel alone, on exit
 * SEGMENTS the caller supplies (parity tests: segments that graze a disc's rim, that end at the tube, that sit on the ties of the
 * exact test, that lie at the edge of a cluster's ball -- where the kernel's two culls could drop a hit).  No ray is traced: the
 * segments are laid into the pipeline's workspace exactly as the sweep's trace kernel leaves them -- 8 doubles per slot, the
 * eighth 0, regions of 1024 slots, a count per region -- and the binning kernel runs on them with the plan's workgroup size, LDS
 * and grid ("grid_blocks" keeps its meaning).  The disc list goes the way isx_disc_sweep sends it: into cluster order, with the
 * cluster table.
 *
 *   centers_axes[n_disc][6], radius, half_thick   the discs of isx_disc_sweep
 *   segments[n][7]  start point, direction, length tmax: the forward segment { start + t direction, 0 <= t <= tmax }
 *   region_counts[n_regions], unit   as for isx_bin_injected_lines.  The slots of a region that hold no segment are filled with
 *         one segment through the centre of disc 0 along its axis, from one unit before the centre to one unit behind it: a kernel
 *         that reads past a region's count shows up as extra counts in hits[0]
 *
 * hits[n_disc] is a HOST array and ACCUMULATES (+=); *bin_increments (may be NULL) is set to what this call added.  Blocking.
 * The result does not depend on the layout, the unit, the order of the segments or "grid_blocks".
 *
 * Domain: what the sweep's trace kernel can produce, which is what the binary32 margins of the cluster test are written for --
 * every coordinate finite, directions and disc axes with | |V| - 1 | <= 1e-12, start points and disc centres with
 * |x|^2 <= 3 cfg->box_half^2, 0 <= tmax <= 2 sqrt(3) cfg->box_half.  Refused with ISX_ERR_BAD_ARG, before any device is asked
 * for: a NULL cfg, centers_axes, hits or segments (with n > 0); n_disc < 1 (or above the 36 000 of isx_disc_sweep); radius or
 * half_thick not > 0; anything outside the domain; a unit that is none of the above; n_regions or a region count out of range,
 * counts that do not sum to n; n above ISX_INJECT_MAX_LINES (ISX_ERR_TOO_LARGE, as is host memory that cannot be had for the
 * staging copy).  ISX_ERR_BAD_CONFIG, likewise before the device: a config that isx_disc_sweep refuses.  With a device,
 * ISX_ERR_BAD_CONFIG as well where the plan does not choose the two-kernel route for the sweep: "disc_pipeline", "pipeline" or
 * "assist" 0, a border, source or hit line that the route does not serve, a disc list whose tables do not fit the binning
 * kernel's LDS (isx_disc_sweep then runs the fused kernel).
 */
int isx_bin_injected_segments(const isx_config* cfg, const double* centers_axes /*[n_disc][6]*/, int32_t n_disc, double radius,
                              double half_thick, const double* segments /*[n][7]*/, uint64_t n, const uint32_t* region_counts,
                              int32_t n_regions, int32_t unit, uint64_t* hits /*[n_disc]*/, uint64_t* bin_increments);

/*
 * Bounce-order histograms: how long the light stayed in the sphere before it ended.  A ray that ends after k mirror
 * interactions survived k absorption tests, so the histories traced at reflectance rho0 = cfg->reflectance are the histories at
 * any rho <= rho0 with weight (rho / rho0)^k: one trace gives the port throughput along a whole reflectance curve
 * (isx_order_reweight).  The mean path per bounce is 4 r_in / 3, so the same histogram is the sphere's time response at the
 * resolution of one mean chord; the census reports only its mean, wall_hits / launched.  No path length is measured here (with a
 * scene: isx_scene_path_hist).
 *
 * For every traced ray take status and n_points as isx_trace_endstates reports them for that ray index (for ISX_SOURCE_BRDF
 * the scattered ray, as there) and v, its final direction:
 *
 *       k = n_points - 2 if EXITED, else n_points - 1     (the mirror interactions of the ray: its own count at its end)
 *       c = 0  EXITED and counted below z (the census's counted_below_z)
 *           1  EXITED otherwise
 *           2  ABSORBED
 *           3  SUSPENDED
 *       k >= n_orders                    :  overflow[c] += 1 , nothing else
 *       else                             :  hist[c * n_orders + k] += 1
 *       and for c == 0 with n_dz > 0     :  f = (v.z + 1.0) * 0.5 * n_dz ;  b = (int)floor(f)     (isx_exit_dz_hist's arithmetic)
 *           0 <= b < n_dz                :  port_dz[k * n_dz + b] += 1
 *           else (NaN / inf included)    :  dz_outside += 1
 *
 * For every call: hist[0] sums to counted_below_z - overflow[0], hist[1] to exited - counted_below_z - overflow[1], hist[2] to
 * absorbed - overflow[2], hist[3] to suspended - overflow[3]; with n_dz > 0, port_dz + dz_outside sums to the sum of hist[0];
 * stats.bin_increments == the sum of hist, and every other field of stats is what isx_fluxmap reports for the same (cfg, n_rays,
 * seed, first_ray).  For ISX_SOURCE_PENCIL with all overflow zero, sum over c and k of k * hist[c][k] == stats.wall_hits (with
 * ISX_SOURCE_BRDF wall_hits counts the primaries' interactions as well, k does not).  The result does not depend on any
 * isx_set_option switch nor on how a job is cut into calls.  cfg->hit_line_mode and the detector-grid fields of cfg are ignored.
 *
 * Limits (a workgroup keeps the u32 block [4 * n_orders | n_orders * n_dz | 5 counters] in its LDS next to the rings of its trace
 * kernel, as ISX_WALL_MAP_MAX_BINS): n_orders 1..ISX_ORDER_HIST_MAX_ORDERS, n_dz 0..64, 4 * n_orders + n_orders * n_dz at most
 * ISX_ORDER_HIST_MAX_WORDS, struct_size == sizeof(isx_order_hist_spec) -- else ISX_ERR_BAD_CONFIG; a NULL cfg, spec or hist, or a
 * NULL port_dz with n_dz > 0: ISX_ERR_BAD_ARG.  Both are answered whether or not a device is present.
 */
#define ISX_ORDER_HIST_MAX_ORDERS 2048
#define ISX_ORDER_HIST_MAX_WORDS  8192
typedef struct isx_order_hist_spec {
  uint32_t struct_size;      /* sizeof(isx_order_hist_spec), set by isx_default_order_hist_spec(); a spec of another size is refused */
  uint32_t reserved0;        /* 0 */
  int32_t n_orders;          /* orders 0 .. n_orders - 1; a ray of a higher order is counted in overflow[] */
  int32_t n_dz;              /* bins of the final direction's z over [-1, 1) per order, counted rays only; 0 = not wanted */
} isx_order_hist_spec;
typedef struct isx_order_hist_counts {
  uint64_t overflow[4];      /* per class: rays with k >= n_orders */
  uint64_t dz_outside;
} isx_order_hist_counts;

/* 512 orders, 8 dz bins.  No GPU needed. */
void isx_default_order_hist_spec(const isx_config* cfg, isx_order_hist_spec* spec);

/* Blocking: hist[4 * n_orders], port_dz[n_orders * n_dz] (may be NULL iff n_dz == 0), *counts (host, zeroed by the callee;
 * counts and stats may be NULL).  Without a HIP device: ISX_ERR_NO_DEVICE; with one but before isx_init(): ISX_ERR_NOT_INIT
 * (as isx_light_field). */
int isx_order_hist(const isx_config* cfg, const isx_order_hist_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                   uint64_t* hist, uint64_t* port_dz, isx_order_hist_counts* counts, isx_stats* stats);
/* ACCUMULATES (+=) into device-resident arrays and five device counters (order of isx_order_hist_counts) on the library's
 * stream and returns after enqueueing; isx_sync() / isx_take_stats() as for isx_wall_map_device. */
int isx_order_hist_device(const isx_config* cfg, const isx_order_hist_spec* spec, uint64_t n_rays, uint64_t seed,
                          uint64_t first_ray, uint64_t* d_hist, uint64_t* d_port_dz, uint64_t* d_counts /*[5]*/);

/*
 * The port fraction at other wall reflectances from one isx_order_hist result.  Host only, no GPU needed.  With
 * rho0 = cfg->reflectance and, for each i < n_rho, w_k = pow(rho[i] / rho0, (double)k):
 *
 *       S1 = sum over k of hist[0][k] * w_k ;  S2 = sum over k of hist[0][k] * w_k * w_k      (in increasing k)
 *       fraction[i] = S1 / launched
 *       sigma[i]    = sqrt(S2 - S1 * S1 / launched) / launched       (the standard error of the weighted mean)
 *
 * `launched` is stats.launched of the call(s) that made hist.  At rho[i] == rho0 fraction is counted_below_z / launched exactly.
 * rho > rho0 is accepted, but its weights grow with k, and so does the variance: the estimate is then carried by the few
 * long-lived rays of the tail.  (Only the wall's absorption is reweighted; the histories themselves -- geometry, border model --
 * are those of cfg.)  Refused with ISX_ERR_BAD_CONFIG: a wrong spec, cfg->source_model != ISX_SOURCE_PENCIL (the primary's
 * interactions are not in k), counts->overflow[0] != 0 (the tail is lost), rho0 <= 0, launched == 0.  ISX_ERR_BAD_ARG: a NULL
 * cfg, spec, hist, counts, rho or fraction, n_rho < 0, a rho[i] that is negative or not finite.  sigma may be NULL.
 */
int isx_order_reweight(const isx_config* cfg, const isx_order_hist_spec* spec, const uint64_t* hist,
                       const isx_order_hist_counts* counts, uint64_t launched, const double* rho, int32_t n_rho,
                       double* fraction, double* sigma);

/*
 * Wall patches: up to ISX_MAX_WALL_PATCHES spherical caps of the inner wall with a reflectance of their own -- a wall-mounted
 * detector (reflectance 0: `absorbed` of its cap is its signal), a sample or a reference standard over a port, a patch of aged
 * coating.  Unlike isx_order_reweight and isx_wall_map this CHANGES the ray histories: a ray that arrives on a patch is absorbed
 * or re-emitted at the patch's reflectance.
 *
 * arrivals and absorbed have P + 2 entries, P = spec->n_patches: class k < P is patch k, class P the inner sphere outside every
 * patch, class P + 1 the rim cone and the outer sphere.  For every mirror interaction the census counts in wall_hits, at the
 * point q (the last point isx_trace_endstates would report if the ray ended there), in this order:
 *
 *       class = P + 1 if the surface is not the inner sphere, else the LOWEST k with
 *               (q.x * axis[0] + q.y * axis[1]) + q.z * axis[2] >= min_dot      (IEEE double, left to right, no fma; axis and
 *               min_dot are used as given, nothing is normalised), else P
 *       arrivals[class] += 1
 *       rho_eff = patch[class].reflectance for class < P, else cfg->reflectance
 *       the interaction's word b survives iff b < rho_thr(rho_eff), rho_thr(rho) = ceil(rho * 2^32 - 0.5) clamped to [0, 2^32];
 *               otherwise absorbed[class] += 1 and the ray ends ABSORBED
 *       a surviving ray is re-emitted as the library re-emits at reflectance rho_eff: the azimuth's uniform is
 *               (b + 1/2) / rho_thr(rho_eff); the interaction count and the bounce limit follow as always
 *
 * The random words, their layout and everything else of a ray's history are unchanged.  For every call: arrivals sums to
 * stats.wall_hits, absorbed sums to stats.absorbed, stats.bin_increments == the sum of arrivals[k] over k < P.  With
 * n_patches == 0, or every patch's reflectance equal to cfg->reflectance bit for bit, every other field of stats except
 * t_kernel_ms is what isx_fluxmap reports for the same (cfg, n_rays, seed, first_ray).  The result does not depend on any
 * isx_set_option switch nor on how a job is cut into calls.  The detector-grid fields and hit_line_mode of cfg are ignored.
 *
 * Scope: the pencil source, the Lambertian ROBAST border, explicit bounces.  Refused with ISX_ERR_BAD_CONFIG: n_patches outside
 * 0..ISX_MAX_WALL_PATCHES, struct_size != sizeof(isx_wall_patch_spec), an axis component or min_dot that is not finite, a
 * reflectance that is NaN or outside [0, 1], cfg->source_model != ISX_SOURCE_PENCIL, cfg->surface_model != ISX_SURFACE_ROBAST,
 * cfg->lambertian == 0, cfg->trace_mode != ISX_TRACE_EXPLICIT; with ISX_ERR_BAD_ARG: a NULL cfg, spec, arrivals or absorbed.
 * Both are answered whether or not a device is present.
 */
#define ISX_MAX_WALL_PATCHES 8
typedef struct isx_wall_patch {
  double axis[3];            /* the cap's axis (isx_wall_patch_cap: a unit vector) */
  double min_dot;            /* a point q of the inner sphere lies in the cap iff q . axis >= min_dot */
  double reflectance;        /* in [0, 1] */
} isx_wall_patch;
typedef struct isx_wall_patch_spec {
  uint32_t struct_size;      /* sizeof(isx_wall_patch_spec), set by isx_default_wall_patch_spec(); a spec of another size is refused */
  uint32_t reserved0;        /* 0 */
  int32_t n_patches;         /* 0 .. ISX_MAX_WALL_PATCHES; where caps overlap the lowest index wins */
  int32_t reserved1;         /* 0 */
  isx_wall_patch patch[ISX_MAX_WALL_PATCHES];
} isx_wall_patch_spec;

/* n_patches 0.  No GPU needed. */
void isx_default_wall_patch_spec(const isx_config* cfg, isx_wall_patch_spec* spec);
/* Host only, no GPU needed: the cap of half-angle half_angle_deg (as seen from the sphere's centre) about dir --
 * axis = dir / |dir|, min_dot = cfg->r_in * cos(half_angle_deg * pi / 180), reflectance as given.  ISX_ERR_BAD_ARG: a NULL
 * argument; ISX_ERR_BAD_CONFIG: dir of zero or non-finite length, half_angle_deg not in [0, 180], a reflectance that is NaN or
 * outside [0, 1]. */
int isx_wall_patch_cap(const isx_config* cfg, const double dir[3], double half_angle_deg, double reflectance, isx_wall_patch* out);

/* Blocking: arrivals[n_patches + 2], absorbed[n_patches + 2] (host, zeroed by the callee; stats may be NULL).  Without a HIP
 * device: ISX_ERR_NO_DEVICE; with one but before isx_init(): ISX_ERR_NOT_INIT (as isx_wall_map). */
int isx_wall_patches(const isx_config* cfg, const isx_wall_patch_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                     uint64_t* arrivals, uint64_t* absorbed, isx_stats* stats);
/* ACCUMULATES (+=) into two device-resident arrays of n_patches + 2 counters on the library's stream and returns after
 * enqueueing; isx_sync() / isx_take_stats() as for isx_wall_map_device. */
int isx_wall_patches_device(const isx_config* cfg, const isx_wall_patch_spec* spec, uint64_t n_rays, uint64_t seed,
                            uint64_t first_ray, uint64_t* d_arrivals, uint64_t* d_absorbed);

/*
 * Beam source: a flux map whose rays start on a disc of finite radius and leave inside a cone -- a collimated beam of finite
 * diameter (radius > 0, cos_min = 1), a fibre or an LED with a numerical aperture (ISX_BEAM_UNIFORM / ISX_BEAM_LAMBERT inside
 * the cone of half-angle acos(cos_min)), a lamp inside the sphere (radius 0, cos_min = -1) -- instead of the pencil, whose rays
 * all share one start point and one direction.  cfg->src and cfg->dir are ignored -- they need not even be a valid pencil (the
 * library puts the spec's origin and axis in their place before it looks at cfg); everything else of cfg means what it means for
 * isx_fluxmap.
 *
 * Per ray (index `ray` of stream `seed`), in IEEE double, every expression evaluated left to right as written, no fma; sqrt and
 * / are the correctly rounded ones; sincos2pi(u) = (sin 2 pi u, cos 2 pi u) and u01(w) = (w + 1/2) 2^-32 are the library's own
 * (isx_mathprobe ops 4 / 5; the oracle's isxo_sincos2pi / isxo_u01):
 *
 *       w[0..3] = block 0 of Philox4x32-10 stream 3 of the ray: counter (ray lo, ray hi, 0, 3), key (seed lo, seed hi)
 *       u_i = u01(w[i])
 *       rr = radius * sqrt(u_0);  (s1, c1) = sincos2pi(u_1);  a = rr * c1;  b = rr * s1
 *       p.x = (origin[0] + a * e1[0]) + b * e2[0]                                  (p.y, p.z likewise with [1], [2])
 *       ISX_BEAM_UNIFORM:  ct = 1.0 - u_2 * (1.0 - cos_min);  st = sqrt(1.0 - ct * ct)
 *       ISX_BEAM_LAMBERT:  s2 = u_2 * (1.0 - cos_min * cos_min);  st = sqrt(s2);  ct = sqrt(1.0 - s2)
 *       (s3, c3) = sincos2pi(u_3)
 *       d.x = (ct * axis[0] + (st * c3) * e1[0]) + (st * s3) * e2[0]               (d.y, d.z likewise)
 *       mag = sqrt((d.x * d.x + d.y * d.y) + d.z * d.z);  v = (d.x / mag, d.y / mag, d.z / mag)
 *
 * The ray starts at p along v, on no surface, and is traced from there exactly as a pencil ray is: Philox stream 0 of the ray
 * for its interactions, the same words per interaction, the same bounce limit, the same census.  Stream 3 is used for nothing
 * else.  With the spec of isx_default_beam_spec() on a configuration whose normalised dir is an exact unit vector (the default's
 * (5, 0, 0)), p == src and v == dir / |dir| for every ray: the results are isx_fluxmap's / isx_trace_endstates', bit for bit.
 *
 * Scope: ISX_SOURCE_PENCIL (the source model of cfg is otherwise unused), ISX_SURFACE_ROBAST with `lambertian` set,
 * ISX_TRACE_EXPLICIT, both hit-line modes.  Refused with ISX_ERR_BAD_CONFIG, whether or not a device is present: anything
 * outside that scope; struct_size != sizeof(isx_beam_spec) (or a cfg of the wrong size); any field of origin, axis, e1, e2,
 * radius, cos_min that is not finite; radius < 0; cos_min outside [-1, 1], or outside [0, 1] for ISX_BEAM_LAMBERT; an
 * angular_law that is neither; (axis, e1, e2) not orthonormal to 1e-12 -- | sqrt(x . x) - 1 | <= 1e-12 for each of the three and
 * | x . y | <= 1e-12 for each of the three pairs (plain products summed left to right); unless
 * sqrt(origin . origin) * (1 + 1e-12) < cfg->r_in -- the disc's centre lies strictly inside the inner sphere -- and
 * (sqrt(origin . origin) + radius) * (1 + 1e-12) < cfg->box_half -- every start point lies strictly inside the world box.  The
 * disc MAY overhang the wall, on purpose: a ray that starts inside the inner sphere meets it from the inside (rule S1 of the first
 * segment); one that starts outside it -- the part of a disc that reaches through the wall -- takes the general boundary search, as
 * a pencil placed there does.  A source wholly inside the wall shell or outside the sphere is refused.  With
 * ISX_ERR_BAD_ARG: a NULL pointer (start_point and start_dir of
 * isx_beam_endstates excepted).  The axes are USED AS GIVEN, nothing is normalised or re-orthogonalised.
 */
#define ISX_BEAM_UNIFORM 0   /* directions uniform in solid angle inside the cone (fibre NA; cos_min = -1: isotropic lamp) */
#define ISX_BEAM_LAMBERT 1   /* cosine-weighted inside the cone (flat emitter, LED die); cos_min >= 0 */
typedef struct isx_beam_spec {
  uint32_t struct_size;      /* sizeof(isx_beam_spec), set by isx_default_beam_spec() / isx_beam_cone() */
  uint32_t reserved0;        /* 0 */
  double origin[3];          /* centre of the emitting disc */
  double axis[3], e1[3], e2[3]; /* beam axis and the disc's two in-plane axes: USED AS GIVEN */
  double radius;             /* >= 0: start points uniform over the disc */
  double cos_min;            /* cosine of the cone's half-angle */
  int32_t angular_law;       /* ISX_BEAM_UNIFORM / ISX_BEAM_LAMBERT */
  int32_t reserved1;         /* 0 */
} isx_beam_spec;

/* The pencil as a beam: origin = cfg->src, the frame of isx_beam_cone() about cfg->dir (axis = dir / |dir| as the library
 * normalises the pencil's direction: mag = sqrt(dx*dx + dy*dy + dz*dz), three divisions), radius 0, cos_min 1, ISX_BEAM_UNIFORM.
 * No GPU needed.  (A dir of zero length leaves a zero frame, which every call refuses.) */
void isx_default_beam_spec(const isx_config* cfg, isx_beam_spec* spec);
/* Host only, no GPU needed: the beam from the disc of `radius` about `origin` into the cone of half-angle half_angle_deg about
 * dir.  axis = dir / |dir| (as above).  The frame: t = the coordinate axis k with the smallest |axis[k]| (the lowest k on a tie);
 * u = t - axis[k] * axis;  e1 = u / |u|;  w = axis x e1;  e2 = w / |w| -- right-handed (e1 x e2 = axis), orthonormal to rounding.
 * cos_min = cos(half_angle_deg * pi / 180), with 0 and 180 degrees mapped to exactly 1 and -1 (and 90 to exactly 0).
 * ISX_ERR_BAD_ARG: a NULL argument; ISX_ERR_BAD_CONFIG: a cfg of the wrong size, origin or dir not finite, dir of zero length,
 * radius not finite or < 0, half_angle_deg not in [0, 180] (ISX_BEAM_LAMBERT: [0, 90]), an unknown law.  Whether the beam lies
 * inside the sphere is checked by the calls that trace it. */
int isx_beam_cone(const isx_config* cfg, const double origin[3], const double dir[3], double radius, double half_angle_deg,
                  int32_t law, isx_beam_spec* out);

/* isx_trace_endstates for the beam, plus the sampled start of every ray: start_point / start_dir [n][3] (either may be NULL).
 * Without a HIP device: ISX_ERR_NO_DEVICE; with one but before isx_init(): ISX_ERR_NOT_INIT. */
int isx_beam_endstates(const isx_config* cfg, const isx_beam_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                       int32_t* status, int32_t* n_points, double* last_point /*[n][3]*/, double* direction /*[n][3]*/,
                       double* start_point /*[n][3]*/, double* start_dir /*[n][3]*/);
/* isx_fluxmap / isx_fluxmap_device for the beam: hits [n_theta * n_phi], zeroed by the callee (the device form ACCUMULATES and
 * returns after enqueueing; isx_sync() / isx_take_stats() as for isx_fluxmap_device).  One route whatever the switches say: the
 * assist-wave trace kernel with the sampled start (isx_trace_assist_beam_kernel), then the binning kernels of isx_fluxmap
 * ("pipeline" 0, "assist" 0 and "bin_mode" 2 do not apply; "bin_mode" 0 bins by brute force).  The result does not depend on any
 * isx_set_option switch nor on how a job is cut into calls.  A detector grid whose tables do not fit the binning kernels' LDS
 * is refused with ISX_ERR_BAD_CONFIG (the default 180 x 90 grid fits). */
int isx_fluxmap_beam(const isx_config* cfg, const isx_beam_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                     uint64_t* hits, isx_stats* stats);
int isx_fluxmap_beam_device(const isx_config* cfg, const isx_beam_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                            uint64_t* d_hits);

/*
 * Baffles: up to ISX_MAX_BAFFLES flat two-sided discs inside the cavity that block and scatter rays -- what keeps the first-strike
 * spot, or a lamp, from being seen directly by the port or a detector.  The ray is traced exactly as isx_fluxmap /
 * isx_trace_endstates trace it -- Philox stream 0, the words of interaction j, the bounce limit and the census are unchanged --
 * except that every segment is tested against the baffles before the ray is taken to its next boundary point.
 *
 * A segment runs from the ray's current point p to q, the next boundary point the library finds from p (of any kind, the world
 * box included).  Once per call, on the host: r2 = radius * radius; rm[i] = cfg->r_in * normal[i]; rho_thr, psi_k1, psi_k0 of the
 * baffle's reflectance exactly as the library derives them from cfg->reflectance.  Per segment, in IEEE double, every expression
 * evaluated left to right as written, no fma; / and sqrt are the correctly rounded ones (c = centre, m = normal):
 *
 *       for each baffle k except the one the ray's previous interaction was with:
 *           s_p = ((p.x - c.x) * m.x + (p.y - c.y) * m.y) + (p.z - c.z) * m.z;   s_q = the same with q
 *           crossing iff (s_p > 0 and s_q < 0) or (s_p < 0 and s_q > 0)                     (a NaN: no crossing)
 *           f = s_p / (s_p - s_q);   x.i = p.i + f * (q.i - p.i);   d = x - c
 *           hit iff (d.x * d.x + d.y * d.y) + d.z * d.z <= r2
 *       the baffle with the smallest f is struck; on equal f the lowest k.  No hit: the ray goes to q as always.
 *
 * On a hit the interaction of the ray's index j runs on the baffle, with the words (wa, wb) a wall interaction of that j has:
 *   - side = s_p > 0 ? 0 : 1 (side 0 is the side the normal points to); arrivals[k][side] += 1; the ray's point becomes x;
 *     n_points += 1; j += 1.
 *   - The ray survives iff wb < rho_thr(baffle k).  Otherwise absorbed[k][side] += 1 and the ray ends ISX_RAY_ABSORBED with last
 *     point x; its direction is that of the segment it arrived on, as for a ray the wall absorbs.
 *   - Re-emission by the cosine law about the struck side's normal, from the library's own sphere point:
 *       zs = fma(-2^-31, wa, 1 - 2^-32);  rs = sqrt(fma(-zs, zs, 1));  (cf, sf) = circle_point_psi(fma(wb, psi_k1, psi_k0))
 *       Rrs = r_in * rs;  S = (Rrs * cf, Rrs * sf, r_in * zs)
 *     (bit for bit what the inner sphere's emission gives for q = (0, 0, 0): the oracle's isxo_cosine_emission of kind 1 there,
 *     with the baffle's reflectance in cfg);  w.i = rm[i] + S.i on side 0, (-rm[i]) + S.i on side 1;
 *       mag = sqrt((w.x * w.x + w.y * w.y) + w.z * w.z);  v = (w.x / mag, w.y / mag, w.z / mag)
 *   - The bounce limit is then applied as after a wall interaction.  The ray goes on from x along v on no surface: its next
 *     boundary is searched as for the first segment of a pencil placed at x, with baffle k skipped for that one segment.
 *
 * stats.wall_hits counts baffle interactions too, stats.absorbed the rays a baffle absorbs, stats.bin_increments is the
 * histogram's sum: sum(arrivals) + (wall interactions) == wall_hits and sum(absorbed[k][s]) <= stats.absorbed for every call.
 * With n_baffles == 0 every result is bit for bit that of isx_fluxmap / isx_trace_endstates (through the baffle kernels all the
 * same: one route whatever the switches say, as for the beam; the fate scan does not apply).  No result depends on any
 * isx_set_option switch nor on how a job is cut into calls.
 *
 * Scope: ISX_SOURCE_PENCIL, ISX_SURFACE_ROBAST with `lambertian` set, ISX_TRACE_EXPLICIT, both hit-line modes.  Refused with
 * ISX_ERR_BAD_CONFIG, whether or not a device is present: anything outside that scope; struct_size != sizeof(isx_baffle_spec) (or
 * a cfg of the wrong size); n_baffles outside 0 .. ISX_MAX_BAFFLES; a field of a baffle that is not finite; radius <= 0; a
 * reflectance outside [0, 1]; | sqrt(m . m) - 1 | > 1e-12; a baffle that does not satisfy
 * (sqrt(c . c) + radius) * (1 + 1e-12) < cfg->r_in (plain products summed left to right) -- the disc lies strictly inside the
 * cavity and never touches a wall; and, for the two flux-map calls, a detector grid that isx_fluxmap refuses or whose tables --
 * 4 B per bin, 32 B per row, 64 B per column -- do not fit the binning kernels' LDS (the device's once isx_init() has asked it,
 * 160 KiB before; the default 180 x 90 grid fits).  ISX_ERR_BAD_ARG: a NULL pointer (last_baffle, counts and
 * stats excepted).  Without a HIP device: ISX_ERR_NO_DEVICE; with one but before isx_init(): ISX_ERR_NOT_INIT.
 * Out of scope: baffles for the other sinks (exit maps, wall map, light field, disc sweeps; order histograms with baffles are the
 * scene's: isx_scene_order_hist), and the chord mode.
 * The beam source and the wall patches combine with baffles in the scene calls below (isx_fluxmap_scene).
 */
#define ISX_MAX_BAFFLES 4
typedef struct isx_baffle {
  double centre[3];
  double normal[3];     /* USED AS GIVEN; side 0 is the side the normal points to */
  double radius;        /* > 0 */
  double reflectance;   /* in [0, 1], both sides */
} isx_baffle;
typedef struct isx_baffle_spec {
  uint32_t struct_size;      /* sizeof(isx_baffle_spec), set by isx_default_baffle_spec() */
  uint32_t reserved0;        /* 0 */
  int32_t n_baffles;         /* 0 .. ISX_MAX_BAFFLES */
  int32_t reserved1;         /* 0 */
  isx_baffle baffle[ISX_MAX_BAFFLES];
} isx_baffle_spec;
typedef struct isx_baffle_counts {
  uint64_t arrivals[ISX_MAX_BAFFLES][2];   /* [baffle][side] */
  uint64_t absorbed[ISX_MAX_BAFFLES][2];
} isx_baffle_counts;

/* No baffle: n_baffles 0, everything else zero.  Host only, no GPU needed (cfg is not looked at). */
void isx_default_baffle_spec(const isx_config* cfg, isx_baffle_spec* spec);
/* Host only, no GPU needed: the disc of `radius` about `centre` with normal = dir / |dir| (as isx_beam_cone normalises its axis:
 * mag = sqrt(dx*dx + dy*dy + dz*dz), three divisions).  ISX_ERR_BAD_ARG: a NULL argument; ISX_ERR_BAD_CONFIG: a cfg of the wrong
 * size, centre or dir not finite, dir of zero length, radius not finite or <= 0, reflectance outside [0, 1].  Whether the disc
 * lies inside the cavity is checked by the calls that trace it. */
int isx_baffle_disc(const isx_config* cfg, const double centre[3], const double dir[3], double radius, double reflectance,
                    isx_baffle* out);
/* isx_trace_endstates with the baffles; last_baffle[i] (may be NULL) is -1 if ray i never touched a baffle, else 2 k + side of
 * its last baffle interaction. */
int isx_baffle_endstates(const isx_config* cfg, const isx_baffle_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                         int32_t* status, int32_t* n_points, double* last_point /*[n][3]*/, double* direction /*[n][3]*/,
                         int32_t* last_baffle /*[n]*/);
/* isx_fluxmap / isx_fluxmap_device with the baffles: hits [n_theta * n_phi] and counts, zeroed by the callee (counts and stats
 * may be NULL).  The device form ACCUMULATES into d_hits and d_counts (16 words, isx_baffle_counts' layout; neither may be NULL)
 * and returns after enqueueing; isx_sync() / isx_take_stats() as for isx_fluxmap_device.  The trace kernel is
 * isx_trace_assist_baffle_kernel, the binning kernels are isx_fluxmap's ("pipeline" 0, "assist" 0, "fate_scan" and "bin_mode" 2
 * do not apply; "bin_mode" 0 bins by brute force). */
int isx_fluxmap_baffle(const isx_config* cfg, const isx_baffle_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                       uint64_t* hits, isx_baffle_counts* counts, isx_stats* stats);
int isx_fluxmap_baffle_device(const isx_config* cfg, const isx_baffle_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                              uint64_t* d_hits, uint64_t* d_counts /*[16]*/);

/*
 * Scene: the beam source, the baffles and the wall patches in ONE trace -- a lamp inside the sphere, a screen between lamp and
 * detector, a detector on the wall, a shield over the port.  No rule of its own: per ray the three contracts above, operation for
 * operation as they are stated there.
 *   1. Start: (p, v) by the beam contract (isx_fluxmap_beam: Philox stream 3, block 0); the ray starts on no surface.
 *   2. Segment: q, the next boundary point, as always; the segment p -> q is tested against every baffle except the one of the
 *      ray's previous interaction, by the baffle contract's rule (isx_fluxmap_baffle: smallest f, lowest k on a tie, a NaN or
 *      s_p == 0 is no crossing -- which also covers a start point in a baffle's plane).
 *   3. Baffle struck: the baffle takes the interaction with the ray's index j exactly as in isx_fluxmap_baffle -- counted by side,
 *      absorbed against the baffle's own threshold, re-emitted by the cosine law about the struck side, bounce limit, that baffle
 *      skipped for one segment.
 *   4. Wall arrival (no hit, q on a mirror): classified by the wall-patch rule (isx_wall_patches): the class is the lowest k with
 *      q . axis >= min_dot, else P, and P + 1 off the inner sphere; patch_arrivals[class] += 1; the absorb test and the re-emission
 *      use rho_eff of the class, the azimuth's uniform being (b + 1/2) / rho_thr(rho_eff); an absorbed ray adds to
 *      patch_absorbed[class].
 *   5. Box (no hit, q on the world box): the ray is ISX_RAY_EXITED, as always.
 *   6. last_baffle[i] is as in isx_baffle_endstates; last_class[i] is the class of the ray's last mirror interaction, -1 if none.
 * For every call: sum(patch_arrivals) + sum(baffle.arrivals) == stats.wall_hits; sum(patch_absorbed) + sum(baffle.absorbed) ==
 * stats.absorbed; stats.bin_increments is the histogram's sum.  No result depends on any isx_set_option switch nor on how a job is
 * cut into calls.  One route whatever the switches say, as for the beam and the baffles: the trace kernel is
 * isx_trace_assist_scene_kernel, the binning kernels are isx_fluxmap's ("pipeline" 0, "assist" 0, "fate_scan" and "bin_mode" 2 do
 * not apply; "bin_mode" 0 bins by brute force); a scene never takes one of the specialised kernels, and the specialised calls
 * stay the faster choice for their own cases.  With the default spec (the pencil as the degenerate beam, no baffle, no patch)
 * every result is bit for bit isx_fluxmap's / isx_trace_endstates'.
 *
 * Scope: ISX_SOURCE_PENCIL, ISX_SURFACE_ROBAST with `lambertian` set, ISX_TRACE_EXPLICIT, both hit-line modes.  Refused, with the
 * same codes and whether or not a device is present: everything isx_fluxmap_beam refuses of `beam`, isx_fluxmap_baffle of `baffles`
 * (the detector grid included, for the two flux-map calls) and isx_wall_patches of `patches` -- each nested struct_size must be
 * right as well as the outer one.  ISX_ERR_BAD_ARG: a NULL pointer (start_point, start_dir, last_baffle, last_class, counts and
 * stats excepted).  Out of scope: a scene for the other sinks (exit maps, wall map, light field, disc sweeps; the fates over the
 * source's sample space are isx_scene_response, the directions a wall detector sees isx_scene_view, where on a patch the light
 * lands isx_scene_patch_field, the fates by bounce order isx_scene_order_hist), the chord mode, the other borders and the BRDF
 * source.
 */
typedef struct isx_scene_spec {
  uint32_t struct_size;        /* sizeof(isx_scene_spec), set by isx_default_scene_spec() */
  uint32_t reserved0;          /* 0 */
  isx_beam_spec beam;          /* the source (the pencil is the degenerate beam) */
  isx_baffle_spec baffles;     /* n_baffles 0: none */
  isx_wall_patch_spec patches; /* n_patches 0: none */
} isx_scene_spec;
typedef struct isx_scene_counts {
  uint64_t patch_arrivals[ISX_MAX_WALL_PATCHES + 2];  /* class k < P patch k, P the rest of the inner sphere, P + 1 rim and outer sphere; entries above P + 1 stay 0 */
  uint64_t patch_absorbed[ISX_MAX_WALL_PATCHES + 2];
  isx_baffle_counts baffle;                            /* arrivals[k][side], absorbed[k][side] */
} isx_scene_counts;                                    /* 36 words */

/* isx_default_beam_spec, isx_default_baffle_spec and isx_default_wall_patch_spec into the three parts.  Host only, no GPU needed. */
void isx_default_scene_spec(const isx_config* cfg, isx_scene_spec* spec);
/* isx_trace_endstates of the scene; start_point, start_dir, last_baffle and last_class may be NULL. */
int isx_scene_endstates(const isx_config* cfg, const isx_scene_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                        int32_t* status, int32_t* n_points, double* last_point /*[n][3]*/, double* direction /*[n][3]*/,
                        double* start_point /*[n][3]*/, double* start_dir /*[n][3]*/, int32_t* last_baffle /*[n]*/,
                        int32_t* last_class /*[n]*/);
/* isx_fluxmap / isx_fluxmap_device of the scene: hits [n_theta * n_phi] and counts, zeroed by the callee (counts and stats may be
 * NULL).  The device form ACCUMULATES into d_hits and d_counts (36 words, isx_scene_counts' layout; neither may be NULL) and
 * returns after enqueueing; isx_sync() / isx_take_stats() as for isx_fluxmap_device. */
int isx_fluxmap_scene(const isx_config* cfg, const isx_scene_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                      uint64_t* hits, isx_scene_counts* counts, isx_stats* stats);
int isx_fluxmap_scene_device(const isx_config* cfg, const isx_scene_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                             uint64_t* d_hits, uint64_t* d_counts /*[36]*/);

/*
 * Scene response: the fates of a scene's rays binned over the source's sample space -- how a detector's signal (or any other
 * fate) depends on where the lamp sends its light: the sphere's spatial response.  One trace of a wide source (the isotropic lamp:
 * radius 0, cos_min -1) answers for every lamp whose intensity relative to it is a function of the source sample:
 * isx_response_reweight, a host-side reweighting, as isx_order_reweight answers for every wall reflectance.
 *
 * The ray histories are those of isx_fluxmap_scene / isx_scene_endstates for the same (cfg, scene, seed, ray index): nothing of a
 * history changes.  Every traced ray adds exactly 1 to response[f * B + b], B = n[0] * n[1] * n[2] * n[3]:
 *
 *   b, the bin, from the words w[0..3] of the beam contract (block 0 of Philox4x32-10 stream 3 of the ray: counter (ray lo, ray hi,
 *   0, 3), key (seed lo, seed hi)), in INTEGER arithmetic -- the rule is stated on the words, not on u01(w): for an n that is no
 *   power of two floor(u01(w) * n) differs from it at some words:
 *
 *       i_a = (uint32_t)(((uint64_t)w[a] * (uint64_t)n[a]) >> 32)            a = 0 .. 3
 *       b   = ((i_0 * n[1] + i_1) * n[2] + i_2) * n[3] + i_3
 *
 *   axis 0: equal-area rings of the emitting disc (u_0 = (rr / radius)^2);  axis 1: the disc's azimuth;  axis 2: equal-probability
 *   polar bands of the cone, counted from the axis outward (ISX_BEAM_UNIFORM: bands of equal solid angle, ct = 1 - u_2 (1 - cos_min));
 *   axis 3: the direction's azimuth about the axis in the (e1, e2) frame.  Every bin has the same expected number of launches.
 *
 *   f, the fate slot, from status, last point, last class and last baffle as isx_scene_endstates defines them:
 *
 *       ISX_RAY_SUSPENDED                                                                  20
 *       ISX_RAY_EXITED with last_point.z < cfg->exit_port_z (the census's counted_below_z) 18
 *       ISX_RAY_EXITED otherwise                                                           19
 *       ISX_RAY_ABSORBED by side s of baffle k                                             10 + 2 k + s
 *       ISX_RAY_ABSORBED on a wall: the class of that interaction                          0 .. P + 1, as in isx_scene_counts
 *
 *   Slots the scene cannot fill stay 0.
 *
 * For every call: the slots of a column (bin) sum to the rays launched into that bin; the rows (slots) sum to -- rows 0..9
 * counts.patch_absorbed, rows 10..17 counts.baffle.absorbed, row 18 counted_below_z, rows 18 + 19 exited, row 20 suspended; the whole
 * sums to stats.launched == stats.bin_increments.  `counts` and every other field of stats except t_kernel_ms are
 * isx_fluxmap_scene's for the same arguments.  No result depends on any isx_set_option switch nor on how a job is cut into calls.
 * cfg->hit_line_mode and the detector-grid fields of cfg are ignored and never a reason for refusal (the grid's LDS check of
 * isx_fluxmap_scene does not apply).  One route whatever the switches say: isx_trace_assist_scene_response_kernel -- the scene's
 * trace kernel with one add per ended ray, where the census is taken; it writes no exit lines and no kernel follows it.  A response
 * small enough is kept as u32 words in the workgroup's LDS and flushed once, a larger one (or any, with "resp_global" 1) takes one
 * global u64 add per ended ray.
 *
 * Refused, whether or not a device is present: everything isx_scene_endstates refuses of cfg and scene, with its codes;
 * ISX_ERR_BAD_CONFIG: struct_size != sizeof(isx_response_spec), reserved0 != 0, an axis outside 1..ISX_RESPONSE_MAX_AXIS,
 * B > ISX_RESPONSE_MAX_BINS; ISX_ERR_BAD_ARG: a NULL cfg, scene, rspec or response (device form: d_response, d_counts).  Without a
 * HIP device: ISX_ERR_NO_DEVICE; with one but before isx_init(): ISX_ERR_NOT_INIT (as isx_fluxmap_scene).
 * Out of scope: the isx_macro command line, a binning over the first-strike point on the wall, a response of the other sinks (the
 * fates by bounce order are isx_scene_order_hist).
 */
#define ISX_RESPONSE_FATES 21
#define ISX_RESPONSE_MAX_AXIS 1024
#define ISX_RESPONSE_MAX_BINS 4096
typedef struct isx_response_spec {
  uint32_t struct_size;      /* sizeof(isx_response_spec), set by isx_default_response_spec(); a spec of another size is refused */
  uint32_t reserved0;        /* 0 */
  int32_t n[4];              /* bins per axis: disc ring, disc azimuth, polar band, direction azimuth; each 1..ISX_RESPONSE_MAX_AXIS */
} isx_response_spec;         /* 24 bytes */

/* n = {1, 1, 6, 12}: a point lamp's directions in 6 polar bands x 12 azimuths.  Host only, no GPU needed. */
void isx_default_response_spec(const isx_config* cfg, isx_response_spec* spec);
/* Blocking: response[ISX_RESPONSE_FATES * B] and counts (host, zeroed by the callee; counts and stats may be NULL). */
int isx_scene_response(const isx_config* cfg, const isx_scene_spec* scene, const isx_response_spec* rspec, uint64_t n_rays,
                       uint64_t seed, uint64_t first_ray, uint64_t* response, isx_scene_counts* counts, isx_stats* stats);
/* ACCUMULATES (+=) into d_response [ISX_RESPONSE_FATES * B] and d_counts (36 words, isx_scene_counts' layout; neither may be
 * NULL) on the library's stream and returns after enqueueing; isx_sync() / isx_take_stats() as for isx_fluxmap_scene_device. */
int isx_scene_response_device(const isx_config* cfg, const isx_scene_spec* scene, const isx_response_spec* rspec, uint64_t n_rays,
                              uint64_t seed, uint64_t first_ray, uint64_t* d_response, uint64_t* d_counts /*[36]*/);
/*
 * The fate fractions of another lamp from one isx_scene_response result.  Host only, no GPU needed.  weight[b] is the lamp's
 * intensity in bin b relative to the traced source; with n_b = the column sum of bin b (the rays launched into it), the sums taken
 * in increasing b:
 *
 *       L = sum over b of weight[b] * n_b ;  S_f = sum over b of weight[b] * response[f][b]
 *       fraction[f] = S_f / L
 *       sigma[f]    = sqrt(sum over b of weight[b]^2 * (response[f][b] * (1 - F)^2 + (n_b - response[f][b]) * F^2)) / L ,  F = fraction[f]
 *
 * -- the self-normalised estimator.  With every weight 1, fraction[f] is the row's sum / launched exactly as the division gives
 * it, and sigma[f] the binomial sqrt(F (1 - F) / launched) up to the rounding of the sum.  fraction and sigma have
 * ISX_RESPONSE_FATES entries; sigma may be NULL.  ISX_ERR_BAD_ARG: a NULL rspec, response, weight or fraction, a weight that is
 * negative or not finite; ISX_ERR_BAD_CONFIG: a spec isx_scene_response refuses, L == 0.
 */
int isx_response_reweight(const isx_response_spec* rspec, const uint64_t* response, const double* weight /*[B]*/,
                          double* fraction /*[21]*/, double* sigma /*[21]*/);

/*
 * Scene view: what a wall detector sees -- the rays a wall class of a scene absorbs, binned over the direction they arrive from,
 * in the detector's own frame.  Baffles are placed by this quantity (the detector must not see the lamp nor the first-strike spot,
 * and should see evenly lit wall everywhere else), and the reading of a hooded photodiode or of a detector behind a field-of-view
 * stop is this map weighted by angle of incidence: isx_view_reweight, a host-side reweighting.
 *
 * The ray histories are those of isx_fluxmap_scene / isx_scene_endstates for the same (cfg, scene, seed, ray index): nothing of a
 * history changes.  A ray is SELECTED if and only if its fate slot, as isx_scene_response defines it, equals vspec->patch: it is
 * ISX_RAY_ABSORBED at a wall arrival of that class.  For every selected ray, with n_points and d = direction as
 * isx_scene_endstates reports them (d is NOT a unit vector: the tracers report the un-normalised last chord), h = half_extent,
 * in this order, in IEEE double, every expression left to right as written, no fma, / and sqrt correctly rounded:
 *
 *       n_points == 2                      : direct += 1, nothing else
 *       c = (d.x*axis[0] + d.y*axis[1]) + d.z*axis[2]
 *       c > 0.0 is false                   : behind += 1, nothing else            (NaN included)
 *       mag = sqrt((d.x*d.x + d.y*d.y) + d.z*d.z)
 *       a = (d.x*e1[0] + d.y*e1[1]) + d.z*e1[2] ;  b likewise with e2
 *       U = -(a / mag) ;  V = -(b / mag)           (the direction the light CAME from, seen from the detector)
 *       fu = (U + h) / (2.0 * h) * n_u ; iu = (int)floor(fu)                     (same with V, n_v -> iv)
 *       0 <= iu < n_u and 0 <= iv < n_v    : view[iv * n_u + iu] += 1, binned += 1
 *       else (NaN / inf included)          : outside += 1
 *
 * `direct` is counted and not binned: a ray absorbed at its first interaction came straight from the source, its direction is the
 * source's own sample, known analytically -- and the scene's kernel keeps none for it (a fresh ray parked at its first wall point
 * carries a marker where its direction was; recomputing the start could differ in the last bit where the boundary search
 * re-normalises).  `behind`: a ray that arrives from behind the plane the frame's axis is the normal of (a wide cap, or a frame
 * that is not the patch's own).
 *
 * In direction-cosine space the cos(theta) of the flux and the solid angle cancel, as for the exit maps: an evenly lit Lambertian
 * interior gives a flat map inside the unit disc, and the radiance the detector sees is proportional to
 * count / (N * du * dv), du = 2 h / n_u, dv = 2 h / n_v.
 *
 * For every call: binned + outside + behind + direct == counts.patch_absorbed[patch]; view sums to binned;
 * stats.bin_increments == binned; the 36 scene counters and every other field of stats except t_kernel_ms are isx_fluxmap_scene's
 * for the same arguments.  No result depends on any isx_set_option switch nor on how a job is cut into calls.  cfg->hit_line_mode
 * and the detector-grid fields of cfg are ignored and never a reason for refusal.  One route whatever the switches say:
 * isx_trace_assist_scene_view_kernel -- the scene's trace kernel with one add per binned ray, where the census is taken; it writes
 * no exit lines and no kernel follows it.  A map small enough is kept as u32 words in the workgroup's LDS and flushed once, a larger
 * one (or any, with "view_global" 1) takes one global u64 add per binned ray.
 *
 * Refused, whether or not a device is present: everything isx_scene_endstates refuses of cfg and scene, with its codes;
 * ISX_ERR_BAD_CONFIG: struct_size != sizeof(isx_view_spec), a non-zero reserved field, patch outside 0 .. n_patches - 1 (so a scene
 * without patches), n_u or n_v outside 1..ISX_VIEW_MAX_AXIS, n_u * n_v > ISX_VIEW_MAX_BINS, half_extent not finite or outside
 * (0, 1], a non-finite frame component, (axis, e1, e2) not orthonormal to 1e-12 by the beam contract's test;
 * ISX_ERR_BAD_ARG: a NULL cfg, scene, vspec or view (device form: d_view, d_view_counts, d_scene_counts).  Without a HIP device:
 * ISX_ERR_NO_DEVICE; with one but before isx_init(): ISX_ERR_NOT_INIT (as isx_fluxmap_scene).
 * Out of scope: more than one patch per call, views from baffle sides, the isx_macro command line, scenes for the remaining sinks
 * (the position on the patch, jointly with the direction, is isx_scene_patch_field; the bounce order is isx_scene_order_hist).
 */
#define ISX_VIEW_MAX_AXIS 1024
#define ISX_VIEW_MAX_BINS 65536
typedef struct isx_view_spec {
  uint32_t struct_size;      /* sizeof(isx_view_spec), set by isx_view_frame(); a spec of another size is refused */
  uint32_t reserved0;        /* 0 */
  int32_t patch;             /* 0 .. scene->patches.n_patches - 1: the detector */
  int32_t n_u, n_v;          /* 1 .. ISX_VIEW_MAX_AXIS, n_u * n_v <= ISX_VIEW_MAX_BINS */
  int32_t reserved1;         /* 0 */
  double axis[3], e1[3], e2[3];  /* the detector's outward normal and its two in-plane axes: USED AS GIVEN */
  double half_extent;        /* h in (0, 1]: the map covers [-h, h]^2 of the direction cosines */
} isx_view_spec;             /* 104 bytes */
typedef struct isx_view_counts { uint64_t binned, outside, behind, direct; } isx_view_counts;

/* The spec for a patch of a scene: axis = scene->patches.patch[patch].axis as given, e1 and e2 by isx_beam_cone's frame rule about
 * that axis.  Host only, no GPU needed.  Refuses what isx_scene_view refuses (ISX_ERR_BAD_ARG: a NULL cfg, scene or out). */
int isx_view_frame(const isx_config* cfg, const isx_scene_spec* scene, int32_t patch, int32_t n_u, int32_t n_v, double half_extent,
                   isx_view_spec* out);
/* Blocking: view[n_v * n_u], view_counts and scene_counts (host, zeroed by the callee; view_counts, scene_counts and stats may be
 * NULL). */
int isx_scene_view(const isx_config* cfg, const isx_scene_spec* scene, const isx_view_spec* vspec, uint64_t n_rays, uint64_t seed,
                   uint64_t first_ray, uint64_t* view, isx_view_counts* view_counts, isx_scene_counts* scene_counts, isx_stats* stats);
/* ACCUMULATES (+=) into d_view [n_v * n_u], d_view_counts (4 words, isx_view_counts' layout) and d_scene_counts (36 words,
 * isx_scene_counts' layout; none may be NULL) on the library's stream and returns after enqueueing; isx_sync() / isx_take_stats()
 * as for isx_fluxmap_scene_device. */
int isx_scene_view_device(const isx_config* cfg, const isx_scene_spec* scene, const isx_view_spec* vspec, uint64_t n_rays,
                          uint64_t seed, uint64_t first_ray, uint64_t* d_view, uint64_t* d_view_counts /*[4]*/,
                          uint64_t* d_scene_counts /*[36]*/);
/*
 * The reading of a detector whose angular response is weight[b] in bin b of the map (and direct_weight for the rays that came
 * straight from the source), from one isx_scene_view result of `launched` rays.  Host only, no GPU needed.  The sums in
 * increasing b:
 *
 *       S1 = sum over b of weight[b] * view[b]   + direct_weight * direct
 *       S2 = sum over b of weight[b]^2 * view[b] + direct_weight^2 * direct
 *       signal = S1 / launched
 *       sigma  = sqrt(S2 - S1^2 / launched) / launched
 *
 * -- isx_order_reweight's estimator (a negative rounding residue under the root counts as 0).  With every weight 1, signal is
 * (binned + direct) / launched exactly as the division gives it.  sigma may be NULL; view_counts gives `direct` (its other fields are not read).  ISX_ERR_BAD_ARG: a NULL vspec, view,
 * view_counts, weight or signal, a weight (direct_weight included) that is negative or not finite; ISX_ERR_BAD_CONFIG: a spec
 * isx_scene_view refuses (the patch index is not looked at: no scene is given), launched == 0.
 */
int isx_view_reweight(const isx_view_spec* vspec, const uint64_t* view, const isx_view_counts* view_counts, uint64_t launched,
                      const double* weight /*[n_v * n_u]*/, double direct_weight, double* signal, double* sigma);
/*
 * A field-of-view stop as a weight for isx_view_reweight: weight[iv * n_u + iu] = 1.0 if the bin's centre (Uc, Vc) has
 * Uc^2 + Vc^2 <= s^2, else 0.0; Uc = -h + (iu + 0.5) * (2 h / n_u), Vc = -h + (iv + 0.5) * (2 h / n_v),
 * s = sin(half_angle_deg * pi / 180), with 90 degrees mapped to exactly 1.  Host only, no GPU needed.  ISX_ERR_BAD_ARG: a NULL
 * vspec or weight; ISX_ERR_BAD_CONFIG: a spec isx_scene_view refuses (as above), a half angle outside [0, 90] or not finite.
 */
int isx_view_weight_fov(const isx_view_spec* vspec, double half_angle_deg, double* weight /*[n_v * n_u]*/);

/*
 * Scene patch field: WHERE on a wall patch the light lands and from which direction -- the rays a wall class of a scene absorbs,
 * binned jointly over the position of the arrival on the patch and the direction they arrive from, in the patch's own frame.
 * isx_scene_view sums over the patch's surface; this is the joint 4-D quantity, as isx_light_field is for the port after
 * isx_exit_maps.  What it answers: is the detector's active area (or the sample over a port) evenly lit, does a baffle's shadow edge
 * fall across it, does the angular picture change from one side of the patch to the other.
 *
 * The ray histories are those of isx_fluxmap_scene / isx_scene_endstates for the same (cfg, scene, seed, ray index): nothing of a
 * history changes.  A ray is SELECTED if and only if its fate slot, as isx_scene_response defines it, equals fspec->patch.  For
 * every selected ray, with q = last_point, d = direction and n_points as isx_scene_endstates reports them, inv = 1.0 / cfg->r_in
 * formed once on the host, h = half_extent, s = pos_scale, in this order, in IEEE double, every expression left to right as
 * written, no fma, / and sqrt correctly rounded:
 *
 *       n_points == 2                       : direct += 1, nothing else                      (as isx_scene_view)
 *       cd = (d.x*axis[0] + d.y*axis[1]) + d.z*axis[2]
 *       cd > 0.0 is false                   : behind += 1, nothing else                      (NaN included; as isx_scene_view)
 *       c  = ((q.x*axis[0] + q.y*axis[1]) + q.z*axis[2]) * inv
 *       w  = sqrt(0.5 / (1.0 + c))
 *       a  = (q.x*e1[0] + q.y*e1[1]) + q.z*e1[2] ;  b likewise with e2
 *       X  = ((a * inv) * w) * s ;  Y = ((b * inv) * w) * s
 *       fx = (X + 1.0) * 0.5 * n_x ; ix = (int)floor(fx)                                     (same with Y, n_y -> iy)
 *       not (0 <= ix < n_x and 0 <= iy < n_y) : pos_outside += 1, nothing else               (NaN / inf included)
 *       (iu, iv) from d by isx_scene_view's formulas, operation for operation (mag, a, b, U, V, fu, fv, floor)
 *       not (0 <= iu < n_u and 0 <= iv < n_v) : dir_outside += 1
 *       else  field[((iy * n_x + ix) * n_v + iv) * n_u + iu] += 1 ,  binned += 1
 *
 * (X, Y) is the Lambert azimuthal equal-area projection of the wall about the patch's axis -- the wall map's projection in another
 * frame -- scaled so that a cap of half-angle alpha fills the unit disc when s = 1 / sin(alpha / 2): equal areas of the patch are
 * equal areas of the map.  The antipode of the axis (c = -1) has no image and counts as pos_outside.  The irradiance on the patch
 * is proportional to count / (N dx dy), dx = 2 / n_x, dy = 2 / n_y; the radiance to count / (N dx dy du dv) in direction-cosine
 * space, du = 2 h / n_u, dv = 2 h / n_v.  An evenly lit patch under a Lambertian interior gives a flat field inside the two discs.
 *
 * For every call: binned + pos_outside + dir_outside + behind + direct == scene_counts.patch_absorbed[patch]; field sums to
 * binned; stats.bin_increments == binned; behind and direct equal isx_scene_view's for the same patch and frame; with
 * n_x = n_y = 1 and every position in range the field is isx_scene_view's map and dir_outside its `outside`; the 36 scene counters
 * and every other field of stats except t_kernel_ms are isx_fluxmap_scene's for the same arguments.  No result depends on any
 * isx_set_option switch nor on how a job is cut into calls.  cfg->hit_line_mode and the detector-grid fields of cfg are ignored and
 * never a reason for refusal.  One route whatever the switches say: isx_trace_assist_scene_field_kernel -- the scene's trace
 * kernel with one add per binned ray, where the census is taken; it writes no exit lines and no kernel follows it.  A field small
 * enough is kept as u32 words in the workgroup's LDS and flushed once, a larger one (or any, with "field_global" 1) takes one
 * global u64 add per binned ray.
 *
 * Refused, whether or not a device is present: everything isx_scene_endstates refuses of cfg and scene, with its codes;
 * ISX_ERR_BAD_CONFIG: struct_size != sizeof(isx_patch_field_spec), a non-zero reserved field, patch outside 0 .. n_patches - 1 (so
 * a scene without patches), an axis size outside 1..ISX_PATCH_FIELD_MAX_AXIS, n_x * n_y * n_u * n_v > ISX_PATCH_FIELD_MAX_BINS,
 * half_extent not finite or outside (0, 1], pos_scale not finite or not > 0, a non-finite frame component, (axis, e1, e2) not
 * orthonormal to 1e-12 by the beam contract's test; ISX_ERR_BAD_ARG: a NULL cfg, scene, fspec or field (device form: d_field,
 * d_field_counts, d_scene_counts).  Without a HIP device: ISX_ERR_NO_DEVICE; with one but before isx_init(): ISX_ERR_NOT_INIT (as
 * isx_fluxmap_scene).
 * Out of scope: a position map of the `direct` rays, more than one patch per call, baffle sides, the isx_macro command line, a
 * scene for the remaining sinks (the bounce order is isx_scene_order_hist).
 */
#define ISX_PATCH_FIELD_MAX_AXIS 1024
#define ISX_PATCH_FIELD_MAX_BINS (1 << 22)
typedef struct isx_patch_field_spec {
  uint32_t struct_size;      /* sizeof(isx_patch_field_spec), set by isx_patch_field_frame(); a spec of another size is refused */
  uint32_t reserved0;        /* 0 */
  int32_t patch;             /* 0 .. scene->patches.n_patches - 1 */
  int32_t n_x, n_y;          /* position bins, each 1 .. ISX_PATCH_FIELD_MAX_AXIS */
  int32_t n_u, n_v;          /* direction bins, likewise; n_x * n_y * n_u * n_v <= ISX_PATCH_FIELD_MAX_BINS */
  int32_t reserved1;         /* 0 */
  double axis[3], e1[3], e2[3];  /* the patch's outward normal and its two in-plane axes: USED AS GIVEN */
  double half_extent;        /* h in (0, 1]: the direction part covers [-h, h]^2 of the direction cosines */
  double pos_scale;          /* s > 0: the position part covers [-1, 1]^2 of the scaled projection; USED AS GIVEN */
} isx_patch_field_spec;      /* 120 bytes */
typedef struct isx_patch_field_counts { uint64_t binned, pos_outside, dir_outside, behind, direct; } isx_patch_field_counts;   /* 40 bytes */

/* The spec for a patch of a scene: the frame by isx_view_frame's rule, pos_scale = 1.0 / sqrt(0.5 * (1.0 - min_dot / cfg->r_in))
 * of that patch (the cap fills the unit disc).  Host only, no GPU needed.  ISX_ERR_BAD_CONFIG where that scale is not finite and
 * positive (a cap of zero angle); otherwise refuses what isx_scene_patch_field refuses (ISX_ERR_BAD_ARG: a NULL cfg, scene or
 * out). */
int isx_patch_field_frame(const isx_config* cfg, const isx_scene_spec* scene, int32_t patch, int32_t n_x, int32_t n_y, int32_t n_u,
                          int32_t n_v, double half_extent, isx_patch_field_spec* out);
/* Blocking: field[n_y * n_x * n_v * n_u], field_counts and scene_counts (host, zeroed by the callee; field_counts, scene_counts
 * and stats may be NULL). */
int isx_scene_patch_field(const isx_config* cfg, const isx_scene_spec* scene, const isx_patch_field_spec* fspec, uint64_t n_rays,
                          uint64_t seed, uint64_t first_ray, uint64_t* field, isx_patch_field_counts* field_counts,
                          isx_scene_counts* scene_counts, isx_stats* stats);
/* ACCUMULATES (+=) into d_field [n_y * n_x * n_v * n_u], d_field_counts (5 words, isx_patch_field_counts' layout) and
 * d_scene_counts (36 words, isx_scene_counts' layout; none may be NULL) on the library's stream and returns after enqueueing;
 * isx_sync() / isx_take_stats() as for isx_scene_view_device. */
int isx_scene_patch_field_device(const isx_config* cfg, const isx_scene_spec* scene, const isx_patch_field_spec* fspec, uint64_t n_rays,
                                 uint64_t seed, uint64_t first_ray, uint64_t* d_field, uint64_t* d_field_counts /*[5]*/,
                                 uint64_t* d_scene_counts /*[36]*/);
/* The two marginals of a field: pos_map[iy * n_x + ix] = the sum over (iv, iu), dir_map[iv * n_u + iu] = the sum over (iy, ix);
 * either may be NULL.  dir_map is what isx_view_reweight takes, through a view spec with the same frame.  Host only, no GPU
 * needed.  ISX_ERR_BAD_ARG: a NULL fspec or field; ISX_ERR_BAD_CONFIG: a spec isx_scene_patch_field refuses (the patch index is
 * not looked at: no scene is given). */
int isx_patch_field_marginals(const isx_patch_field_spec* fspec, const uint64_t* field, uint64_t* pos_map /*[n_y * n_x]*/,
                              uint64_t* dir_map /*[n_v * n_u]*/);

/*
 * Scene order histograms: the fates of a scene's rays by bounce order -- after how many interactions the light of a scene ends
 * where it ends.  What isx_order_hist and isx_order_reweight answer for the bare sphere, for a sphere with a lamp, baffles and wall
 * detectors: one trace gives every fate's fraction along a whole ageing curve of the coating (isx_scene_order_reweight: the sphere
 * multiplier against rho) and the time response of every fate in interactions (isx_scene_order_moments).
 *
 * The ray histories are those of isx_fluxmap_scene / isx_scene_endstates for the same (cfg, scene, seed, ray index): nothing of a
 * history changes.  For every traced ray:
 *
 *   f, the fate slot, exactly as isx_scene_response defines it (0 .. 20, ISX_RESPONSE_FATES);
 *   k = n_points - 2 if ISX_RAY_EXITED, else n_points - 1, with n_points as isx_scene_endstates reports it -- isx_order_hist's
 *   rule: the ray's interaction count, interactions with baffles included, so that the sum of k over all rays is stats.wall_hits;
 *   if k >= n_orders: overflow[f] += 1 and nothing else; otherwise hist[f * n_orders + k] += 1.
 *
 * For every call: the sum of row f plus overflow[f] is the row sum isx_scene_response gives for f -- rows 0..9
 * counts.patch_absorbed, rows 10..17 counts.baffle.absorbed, row 18 counted_below_z, rows 18 + 19 exited, row 20 suspended;
 * stats.bin_increments is the sum of hist; with every overflow zero the sum of k * hist[f][k] is stats.wall_hits.  `counts` and
 * every other field of stats except t_kernel_ms are isx_fluxmap_scene's for the same arguments.  No result depends on any
 * isx_set_option switch nor on how a job is cut into calls.  cfg->hit_line_mode and the detector-grid fields of cfg are ignored and
 * never a reason for refusal.  Slots the scene cannot fill stay 0.
 *
 * With isx_default_scene_spec (the pencil, no baffle, no patch) and the same cfg and n_orders: row 18 is isx_order_hist's class 0,
 * row 19 class 1, row 0 + row 1 class 2, row 20 class 3, and the overflows likewise.
 *
 * One route whatever the switches say: isx_trace_assist_scene_order_kernel -- the scene's trace kernel with one add per ended ray,
 * where the census is taken; it draws nothing, writes no exit lines, and no kernel follows it.  An order histogram is peaked at
 * low k: the first L orders of every slot the scene can fill are kept as u32 words in the workgroup's LDS and flushed once, the
 * orders from L on -- rare, spread over many addresses -- take one global u64 add each ("sorder_lds_orders": L).
 *
 * Refused, whether or not a device is present: everything isx_scene_endstates refuses of cfg and scene, with its codes;
 * ISX_ERR_BAD_CONFIG: struct_size != sizeof(isx_scene_order_spec), a non-zero reserved field, n_orders outside
 * 1..ISX_SCENE_ORDER_MAX_ORDERS; ISX_ERR_BAD_ARG: a NULL cfg, scene, ospec or hist (device form: d_hist, d_order_counts,
 * d_scene_counts).  Without a HIP device: ISX_ERR_NO_DEVICE; with one but before isx_init(): ISX_ERR_NOT_INIT (as
 * isx_fluxmap_scene).
 * Out of scope: a reweighting of the wall alone where patches or baffles reflect at another value (it needs a counter per ray),
 * a joint histogram over order and source bin, the isx_macro command line (path lengths in cm are isx_scene_path_hist).
 */
#define ISX_SCENE_ORDER_MAX_ORDERS 65536
typedef struct isx_scene_order_spec {
  uint32_t struct_size;      /* sizeof(isx_scene_order_spec), set by isx_default_scene_order_spec(); a spec of another size is refused */
  uint32_t reserved0;        /* 0 */
  int32_t n_orders;          /* orders 0 .. n_orders - 1 per fate slot; 1..ISX_SCENE_ORDER_MAX_ORDERS */
  int32_t reserved1;         /* 0 */
} isx_scene_order_spec;      /* 16 bytes */
typedef struct isx_scene_order_counts { uint64_t overflow[ISX_RESPONSE_FATES]; } isx_scene_order_counts;   /* 168 bytes */

/* n_orders = 512.  Host only, no GPU needed. */
void isx_default_scene_order_spec(const isx_config* cfg, isx_scene_order_spec* ospec);
/* Blocking: hist[ISX_RESPONSE_FATES * n_orders], order_counts and scene_counts (host, zeroed by the callee; order_counts,
 * scene_counts and stats may be NULL). */
int isx_scene_order_hist(const isx_config* cfg, const isx_scene_spec* scene, const isx_scene_order_spec* ospec, uint64_t n_rays,
                         uint64_t seed, uint64_t first_ray, uint64_t* hist, isx_scene_order_counts* order_counts,
                         isx_scene_counts* scene_counts, isx_stats* stats);
/* ACCUMULATES (+=) into d_hist [ISX_RESPONSE_FATES * n_orders], d_order_counts (21 words, isx_scene_order_counts' layout) and
 * d_scene_counts (36 words, isx_scene_counts' layout; none may be NULL) on the library's stream and returns after enqueueing;
 * isx_sync() / isx_take_stats() as for isx_fluxmap_scene_device. */
int isx_scene_order_hist_device(const isx_config* cfg, const isx_scene_spec* scene, const isx_scene_order_spec* ospec,
                                uint64_t n_rays, uint64_t seed, uint64_t first_ray, uint64_t* d_hist,
                                uint64_t* d_order_counts /*[21]*/, uint64_t* d_scene_counts /*[36]*/);
/*
 * The fate fractions of the same scene with EVERY reflectance multiplied by t = scale[i] -- cfg->reflectance, every patch's and
 * every baffle's: the ageing of the whole interior -- from one isx_scene_order_hist result.  Host only, no GPU needed.  Where all
 * reflecting surfaces carry the wall's coating, t = rho / rho0.  A history that survived s absorption tests keeps the weight t^s;
 * with rho_f the reflectance of the surface slot f absorbs on (patch f for f < P, the wall for the classes P and P + 1, baffle
 * (f - 10) / 2 for the slots 10..17):
 *
 *   rows 18, 19, 20 (every interaction survived):  w_k = pow(t, k)                                       k = 0 .. n_orders - 1
 *   rows 0..17 (absorbed at interaction k):        w_k = a_f * pow(t, k - 1),  a_f = (1 - t * rho_f) / (1 - rho_f)   k = 1 .. n_orders - 1
 *       (an absorbed ray has k >= 1: hist[f][0] is 0 by construction and is not looked at)
 *   S1 = sum over k of hist[f][k] * w_k ;  S2 = sum over k of hist[f][k] * w_k * w_k      (in increasing k)
 *   fraction[i * 21 + f] = S1 / launched
 *   sigma[i * 21 + f]    = sqrt(max(0, S2 - S1 * S1 / launched)) / launched
 *
 * -- isx_order_reweight's estimator.  At t == 1 a fraction is the row's sum / launched exactly.  A row with rho_f == 1 is empty by
 * construction: its fraction and sigma are NaN for t != 1 and 0 for t == 1.  A slot the scene cannot fill (a wall class above
 * P + 1, a baffle the scene does not have) gives 0 and 0.  sigma may be NULL.
 * ISX_ERR_BAD_CONFIG: a spec or a scene isx_scene_order_hist refuses, any overflow[f] != 0, launched == 0; ISX_ERR_BAD_ARG: a NULL
 * cfg, scene, ospec, hist or counts, n_scale < 0, a NULL scale or fraction with n_scale > 0, a t that is negative or not finite,
 * a t for which t * rho is above 1 for any surface of the scene.
 */
int isx_scene_order_reweight(const isx_config* cfg, const isx_scene_spec* scene, const isx_scene_order_spec* ospec,
                             const uint64_t* hist, const isx_scene_order_counts* counts, uint64_t launched, const double* scale,
                             int32_t n_scale, double* fraction /*[n_scale][21]*/, double* sigma /*[n_scale][21]*/);
/*
 * The time response in interactions: mean and standard deviation of k per fate slot.  Host only, no GPU needed.  With
 * N = sum over k of hist[f][k], A = sum of k * hist[f][k], B = sum of k * k * hist[f][k] (as doubles, in increasing k):
 * mean[f] = A / N, sd[f] = sqrt(max(0, B / N - mean[f] * mean[f])).  NaN for an empty row and for a row with overflow[f] != 0.
 * Either output may be NULL.  ISX_ERR_BAD_ARG: a NULL ospec, hist or counts; ISX_ERR_BAD_CONFIG: a spec isx_scene_order_hist refuses.
 */
int isx_scene_order_moments(const isx_scene_order_spec* ospec, const uint64_t* hist, const isx_scene_order_counts* counts,
                            double* mean /*[21]*/, double* sd /*[21]*/);

/*
 * Scene path histograms: the fates of a scene's rays by path length -- how much path, in cm, the light of a scene has travelled
 * where it ends: the temporal impulse response of every fate (time = L / 29.9792458 cm/ns; no call converts).  The bounce order
 * (isx_scene_order_hist) is a time axis only at the resolution of one mean chord and only for a bare sphere; with a lamp, baffles
 * and detector caps the legs run from a few cm to 2 r_in.
 *
 * The ray histories are those of isx_fluxmap_scene / isx_scene_endstates for the same (cfg, scene, seed, ray index): nothing of a
 * history changes.  For every traced ray, f is the fate slot exactly as isx_scene_response defines it (0 .. 20,
 * ISX_RESPONSE_FATES), and L its path length:
 *
 *   Track points.  X_0 is the start point of the beam contract; X_i every point the ray's point becomes -- a baffle crossing x,
 *   the boundary point q of a wall arrival, the world box: the points n_points counts.
 *   Segments (all arithmetic IEEE double, left to right as written, no fma, the correctly rounded sqrt):
 *       d = X_i - X_{i-1} (componentwise) ;  s_i = sqrt((d.x * d.x + d.y * d.y) + d.z * d.z)
 *       L = 0.0, then L = L + s_i in order of i
 *   Which segments count.  ISX_RAY_ABSORBED and ISX_RAY_SUSPENDED: all n_points - 1.  ISX_RAY_EXITED: the n_points - 2 up to the
 *   last interaction point -- the leg to the world box is an artefact of the box.  Slot 18 (counted below z) then adds the leg up
 *   to the port plane: with p = X_{n-2}, q = X_{n-1} and s the length of that leg by the rule above,
 *       f = (cfg->exit_port_z - p.z) / (q.z - p.z) ;  L = L + ((f > 0.0 && f <= 1.0) ? s * f : 0.0)        (a NaN f: 0.0)
 *   so a last interaction point already below the plane adds nothing.  Slot 19 adds nothing.
 *   Binning.  fb = L / bin_cm; if (fb < (double)n_bins) is false (a NaN included): overflow[f] += 1; otherwise
 *   hist[f * n_bins + (int)fb] += 1.  An fb equal to an integer lands in the upper bin; fb == n_bins is overflow.
 *   Checksum.  For every ray, overflowed or not: checksum[f] += the 64 bits of L as an unsigned integer, modulo 2^64 -- the parity
 *   instrument: a histogram cannot see a last-bit difference in L, a modular sum of bit patterns sees every one; it does not
 *   depend on the order of the rays and adds over calls.
 *
 * For every call: the sum of row f plus overflow[f] is the row sum isx_scene_response gives for f; stats.bin_increments is the sum
 * of hist; `scene_counts` and every other field of stats except t_kernel_ms are isx_fluxmap_scene's for the same arguments; with
 * n_bins 1 and bin_cm 1e300 hist[f][0] is the response's row and every overflow 0.  No result, the checksums included, depends on
 * any isx_set_option switch nor on how a job is cut into calls.  cfg->hit_line_mode and the detector-grid fields of cfg are
 * ignored and never a reason for refusal.  Slots the scene cannot fill stay 0.
 *
 * One route whatever the switches say: isx_trace_assist_scene_path_kernel -- the scene's trace kernel with one double more per
 * ray, advanced wherever the ray's point is replaced and handed over with the ray, and one add per ended ray where the census
 * is taken; it draws nothing, writes no exit lines, and no kernel follows it.  The first B bins of every slot the scene can fill
 * are u32 words in the workgroup's LDS, flushed once, with the overflow counters and the checksums; the bins from B on take one
 * global u64 add each ("spath_lds_bins": B).
 *
 * Refused, whether or not a device is present: everything isx_scene_endstates refuses of cfg and scene, with its codes;
 * ISX_ERR_BAD_CONFIG: struct_size != sizeof(isx_scene_path_spec), a non-zero reserved field, n_bins outside
 * 1..ISX_SCENE_PATH_MAX_BINS, a bin_cm that is not finite or not > 0; ISX_ERR_BAD_ARG: a NULL cfg, scene, pspec or hist (device
 * form: d_hist, d_path_counts, d_scene_counts).  Without a HIP device: ISX_ERR_NO_DEVICE; with one but before isx_init():
 * ISX_ERR_NOT_INIT (as isx_fluxmap_scene).
 * Out of scope: path histograms for the bare-sphere calls and the other borders, a joint histogram over path and order or source
 * bin, the convolution with a pulse shape, the isx_macro command line.
 */
#define ISX_SCENE_PATH_MAX_BINS 65536
typedef struct isx_scene_path_spec {
  uint32_t struct_size;      /* sizeof(isx_scene_path_spec), set by isx_default_scene_path_spec(); a spec of another size is refused */
  uint32_t reserved0;        /* 0 */
  int32_t n_bins;            /* bins 0 .. n_bins - 1 per fate slot; 1..ISX_SCENE_PATH_MAX_BINS */
  int32_t reserved1;         /* 0 */
  double bin_cm;             /* width of a bin in cm; finite, > 0 */
} isx_scene_path_spec;       /* 24 bytes */
typedef struct isx_scene_path_counts {
  uint64_t overflow[ISX_RESPONSE_FATES];   /* per fate slot, the rays with L / bin_cm not below n_bins */
  uint64_t checksum[ISX_RESPONSE_FATES];   /* per fate slot, the sum of the bit patterns of L modulo 2^64 */
} isx_scene_path_counts;     /* 336 bytes */

/* n_bins = 1024, bin_cm = cfg->r_in / 4.  Host only, no GPU needed. */
void isx_default_scene_path_spec(const isx_config* cfg, isx_scene_path_spec* pspec);
/* Blocking: hist[ISX_RESPONSE_FATES * n_bins], path_counts and scene_counts (host, zeroed by the callee; path_counts,
 * scene_counts and stats may be NULL). */
int isx_scene_path_hist(const isx_config* cfg, const isx_scene_spec* scene, const isx_scene_path_spec* pspec, uint64_t n_rays,
                        uint64_t seed, uint64_t first_ray, uint64_t* hist, isx_scene_path_counts* path_counts,
                        isx_scene_counts* scene_counts, isx_stats* stats);
/* ACCUMULATES (+=, the checksums modulo 2^64) into d_hist [ISX_RESPONSE_FATES * n_bins], d_path_counts (42 words,
 * isx_scene_path_counts' layout) and d_scene_counts (36 words, isx_scene_counts' layout; none may be NULL) on the library's stream
 * and returns after enqueueing; isx_sync() / isx_take_stats() as for isx_fluxmap_scene_device. */
int isx_scene_path_hist_device(const isx_config* cfg, const isx_scene_spec* scene, const isx_scene_path_spec* pspec,
                               uint64_t n_rays, uint64_t seed, uint64_t first_ray, uint64_t* d_hist,
                               uint64_t* d_path_counts /*[42]*/, uint64_t* d_scene_counts /*[36]*/);
/*
 * Mean and standard deviation of the path length per fate slot, in cm, from the bin centres x_ib = (ib + 0.5) * bin_cm.  Host
 * only, no GPU needed.  With N = sum over ib of hist[f][ib], A = sum of x_ib * hist[f][ib], B = sum of x_ib * x_ib * hist[f][ib]
 * (as doubles, in increasing ib): mean_cm[f] = A / N, sd_cm[f] = sqrt(max(0, B / N - mean_cm[f] * mean_cm[f])) --
 * isx_scene_order_moments' formulas.  NaN for an empty row and for a row with overflow[f] != 0.  Either output may be NULL.
 * ISX_ERR_BAD_ARG: a NULL pspec, hist or counts; ISX_ERR_BAD_CONFIG: a spec isx_scene_path_hist refuses.
 */
int isx_scene_path_moments(const isx_scene_path_spec* pspec, const uint64_t* hist, const isx_scene_path_counts* counts,
                           double* mean_cm /*[21]*/, double* sd_cm /*[21]*/);
/*
 * The decay constant of the tail of row f from bin lo_bin on: the maximum-likelihood estimate for a geometric law over the bins.
 * Host only, no GPU needed.  With N the rays in the bins ib >= lo_bin and m the mean of (ib - lo_bin) over them -- S = sum of
 * (double)(ib - lo_bin) * (double)hist[f][ib] and N = sum of (double)hist[f][ib], in increasing ib, m = S / N:
 *
 *   r        = m / (1.0 + m)
 *   tau_cm   = -bin_cm / log(r)
 *   sigma_cm = bin_cm / (log(r) * log(r)) / sqrt(N * m * (1.0 + m))
 *
 * In time: tau_cm / 29.9792458 ns.  ISX_ERR_BAD_CONFIG: a spec isx_scene_path_hist refuses,
 * overflow[f] != 0, N == 0, m == 0; ISX_ERR_BAD_ARG: f outside 0..20, lo_bin outside 0..n_bins - 1, a NULL pspec, hist, counts,
 * tau_cm or sigma_cm.
 */
int isx_scene_path_decay(const isx_scene_path_spec* pspec, const uint64_t* hist, const isx_scene_path_counts* counts, int32_t f,
                         int32_t lo_bin, double* tau_cm, double* sigma_cm);

/*
 * Series driver (sweepSeries, fluxAtObserverOptimize.C:892-921 / fluxAtObserverFast.C:1641-1673):
 * n_cfg configurations sharing one detector grid, traced back to back on the device with ONE
 * host synchronisation; hits[n_cfg][n_theta*n_phi], stats[n_cfg] (t_kernel_ms = whole series).
 * Configuration k uses ray indices [first_ray + k*n_rays, +n_rays).
 */
int isx_fluxmap_series(const isx_config* cfgs, int32_t n_cfg, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                       uint64_t* hits, isx_stats* stats);

/* Host-side detector table exactly as Detector::setPosition builds it
 * (fluxAtObserver.C:49-68): out[(i*n_phi+j)*6] = x,y,z,nx,ny,nz.  No GPU needed. */
int isx_detector_table(const isx_config* cfg, double* out);

#ifdef __cplusplus
}
#endif
#endif /* ISX_H */
