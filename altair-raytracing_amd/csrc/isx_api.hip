// isx_api.hip — C ABI of libisx (include/isx.h) over the gfx950 kernels.
//
// Host-side "geometry setup" here replaces setupOpticsManager()
// (fluxAtObserverOptimize.C:192-230) and Detector::setPosition (fluxAtObserver.C:49-68):
// it only evaluates closed-form constants and the detector table; all ray work is on the GPU.
// There is no CPU compute path: without a device every entry point returns ISX_ERR_NO_DEVICE.
#include "../../include/isx.h"
#include "isx_kernels.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <limits>
#include <map>
#include <new>
#include <tuple>
#include <variant>
#include <vector>

using namespace isx;

namespace {

struct State {
  bool init = false;
  int device = -1;
  int cu_count = 0;
  size_t lds_limit = 64 * 1024;   // per-workgroup LDS the device grants (160 KiB on gfx950)
  hipStream_t stream = nullptr;
  int last_hip = 0;
  // detector tables (device) + the config they were built for
  isx_config tab_cfg{};
  bool have_tab = false;
  double* d_table = nullptr;
  double* d_rowtab = nullptr;
  double* d_coltab = nullptr;
  size_t cap_bins = 0, cap_rows = 0, cap_cols = 0;
  unsigned long long* d_hist = nullptr;
  size_t cap_hist = 0;
  unsigned long long* d_stats = nullptr;  // [8]
  double* d_aux = nullptr;                // caller-supplied detector / disc lists of the current call (grown, never shrunk)
  size_t cap_aux = 0;
  // two-kernel pipeline of the headline flux map: exit lines in HBM, in regions of kRegion 48-byte slots + lines per region
  static constexpr int kRecBufs = 3;      // workspaces: chunk k uses buffer k mod 3 (the overlapped pipeline keeps up to 3 in flight)
  double* d_rec[kRecBufs] = {};
  uint32_t* d_rec_counts[kRecBufs] = {};
  size_t cap_regions[kRecBufs] = {0, 0, 0};
  // fate scan: the rays of a chunk that the scan leaves to the trace kernel, 4 B per ray of the largest chunk
  // (one list per workspace: the list of chunk k is read by its trace kernel while the scan of a later chunk may already run)
  uint32_t* d_list[kRecBufs] = {};
  size_t cap_list[kRecBufs] = {0, 0, 0};
  unsigned long long fate_launches = 0;   // isx_fate_scan_kernel launches enqueued since isx_init (isx_fate_scan_launches)
  int fate_scan = -1;                     // 0 off, 1 on wherever eligible, -1 (default) automatic: fate_scan_auto()
  // exit lines from the words, behind the fate scan: per workspace the list of the rays isx_exit_lines_kernel
  // leaves to the trace kernel (4 B per ray), the side entry of every line slot (8 B) and the chunk's redo list ([0] count,
  // [1] overflow, [2..] entries); d_list then holds the scan's {offset, j} pairs (8 B per ray)
  int exit_scan = -1;                     // 0 off, 1 on wherever eligible, -1 (default) automatic: where the fate scan's rule says so
  int64_t exit_eps_scale = 1;             // test option: every bound the exit-line kernel hands to the binning kernel is multiplied by it
  uint32_t* d_list_b[kRecBufs] = {};
  uint2* d_side[kRecBufs] = {};
  unsigned long long* d_redo[kRecBufs] = {};
  size_t cap_exit_rays[kRecBufs] = {0, 0, 0}, cap_side[kRecBufs] = {0, 0, 0}, cap_redo[kRecBufs] = {0, 0, 0};
  bool list_pairs[kRecBufs] = {false, false, false};   // d_list[b] has room for pairs
  unsigned long long* d_exit_totals = nullptr;   // [3] accepted, list B, redo entries since isx_init (isx_exit_scan_counts)
  // overlap > 1: a flux-map call is cut into that many chunks and the binning kernel of chunk k runs on a second stream
  // while the trace kernel of chunk k+1 runs on the first
  int overlap = 0;
  int overlap_trace_streams = 1;          // 2: consecutive trace kernels alternate between two streams (chunk k+1 fills the tail of chunk k)
  hipStream_t stream2 = nullptr, stream3 = nullptr;
  // call overlap: an enqueued flux map (isx_fluxmap_device, ROUTE_FLUX_PIPE, explicit bounces) puts its
  // counter zeroing, fate scan and trace kernel on a trace stream (stream2; with call_overlap_streams = 2 consecutive chunks
  // alternate between stream2 and stream3) and only its binning kernel on `stream`, so that the next call's scan and trace fill the
  // launch tails of this one.  Chunk s (counted over calls: call_rot) uses workspace and fate list s mod kRecBufs, and its trace
  // waits for ev_free[s mod kRecBufs], recorded behind the last kernel that read that workspace.  (Its counter block is the
  // ring's next, as everywhere: a block comes round again 256 launches later, behind the same waits.)  trace_open: the trace
  // streams hold work that `stream` has not been joined behind (trace_join()).
  int call_overlap = -1;                  // 0 off, 1 on wherever eligible, -1 (default) automatic: the same
  int call_overlap_streams = 2;
  unsigned call_rot = 0;
  bool trace_open = false;
  hipEvent_t ev_free[kRecBufs] = {};
  bool free_set[kRecBufs] = {false, false, false};
  hipEvent_t ev_join[3] = {};   // [0], [1]: tails of stream2 / stream3; [2]: where `stream` stood when they opened
  int pipeline = 1;                       // 1 (default): trace kernel -> HBM -> binning kernel (lean flux map); 0: fused kernel
  uint64_t pipe_chunk = 1ull << 26;       // rays per trace/bin pair (3.4 GB of exit-line workspace at most)
  // work-queue counters of the launches (Work::ctr): a ring of Q_WORDS-word blocks, one per launch, zeroed on the stream
  // right before its launch
  uint32_t* d_ctr = nullptr;
  size_t ctr_next = 0;
  static constexpr size_t kCtrRing = 256;
  int ray_sub = 0;                        // rays a wave takes off the queue at a time (0: by launch size)
  int bin_block = 512, bin_blocks_per_cu = 0;   // binning kernel: workgroup size, workgroups per CU in the grid (0: what is resident)
  int assist_block = ISX_ASSIST_BLOCK;          // its workgroup size: (assist_block / 64 - 1) tracer waves + 1 assist wave
  bool assist_block_set = false;                // set through isx_set_option: then it holds for small launches too (small_shape)
  int rays_per_lane = 0;                        // 0: by launch size (small_shape); > 0: the grid is sized for this many rays per tracer lane
  int disc_pipeline = 1;                        // 1 (default): the shared-ray disc sweep as assist-wave trace kernel + isx_bin_discs_kernel; 0: fused SINK_DISC kernel
  int assist = 1;                               // 1: trace kernels with an assist wave per workgroup (assist_body)
  int bin_cols = 1;                             // 1 (2: the same): isx_bin_cols_kernel ((line, column) slots) where bin_slots applies; 0: row slots
  int bin_slots = 1;                            // 1: isx_bin_slots_kernel (slot queues by window length) where the grid allows it
  int lf_global = 0;                            // 1: isx_bin_lightfield_kernel's global form for a field that fits the LDS as well (diagnostic)
  int resp_global = 0;                          // 1: isx_trace_assist_scene_response_kernel's global form for a response that fits the LDS as well (diagnostic)
  int field_global = 0;                         // 1: isx_trace_assist_scene_field_kernel's global form for a field that fits the LDS as well (diagnostic)
  int sorder_lds_orders = -1;                   // isx_trace_assist_scene_order_kernel: -1 as many orders in the workgroup's LDS as cost no resident workgroup;
                                                // n > 0: at most n of them; 0: none, one global add per ended ray (diagnostic)
  int spath_lds_bins = -1;                      // isx_trace_assist_scene_path_kernel: -1 as many bins in the workgroup's LDS as cost no resident workgroup;
                                                // n > 0: at most n of them; 0: none, one global add per ended ray (diagnostic)
  int view_global = 0;                          // 1: isx_trace_assist_scene_view_kernel's global form for a map that fits the LDS as well (diagnostic)
  int surface_pipeline = 1;                     // 1 (default): the lobe / rough-specular borders and the origin-compat hit line on the assist-wave
                                                // pipeline (round 5); 0: round 1's fused isx_trace_bin_full_kernel
  // options
  int bin_mode = 1;
  int blocks_per_cu = 1;   // 1024-thread blocks: 16 waves/CU, 4 per SIMD
  int grid_blocks = 0;  // 0 = auto
  int sched_mask = 3, sched_min = 12;   // generic boundary search: every 4th loop trip (24 bounces) or when 12 lanes wait
  // timing of enqueued-but-not-collected launches
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  struct Span { size_t a, b; int kind; };   // kind 0: single-kernel launch, 1: trace kernel of the pipeline, 2: its binning kernel
  std::vector<Span> spans;
  double last_ms[3] = {0, 0, 0};           // per kind, of the launches collected by the last collect_stats()
  // workgroup shape of the kernels that keep no LDS histogram: 512 threads (6 waves per SIMD at <= 80 VGPRs); the grid is what
  // is resident (the waves share one ray queue, so late workgroups have nothing to even out); trace_blocks_per_cu > 0 overrides
  int trace_block = 512, trace_blocks_per_cu = 0;
  // hipFuncSetAttribute(MaxDynamicSharedMemorySize) is made once per kernel and size, not once per launch
  std::map<const void*, size_t> attr_lds;
  // ... and so is the occupancy query (blocks_per_cu): (kernel, workgroup size, LDS bytes) -> workgroups per CU
  std::map<std::tuple<const void*, int, size_t>, int> occ;
  // small calls are bound by host round trips: results and census go through ONE pinned staging buffer
  // (asynchronous copies, one synchronisation per call), and a blocking call that finds nothing enqueued before it skips the
  // census round trip at its start
  unsigned char* h_pin = nullptr;
  size_t cap_pin = 0;
  bool pending = false;                    // launches enqueued since the last collect_stats()
} S;

// Scratch device allocation of one call: freed on every return path.
template <class T>
struct DevBuf {
  T* p = nullptr;
  hipError_t alloc(size_t n) { return hipMalloc(&p, n * sizeof(T)); }
  ~DevBuf() { if (p) (void)hipFree(p); }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

// a HIP status as an isx status (the HIP one is kept for isx_last_hip_error); HIPCHK returns it on failure
int hip_rc(hipError_t e) {
  if (e != hipSuccess) S.last_hip = (int)e;
  return e == hipSuccess ? ISX_OK : ISX_ERR_HIP;
}
#define HIPCHK(expr) do { if (hip_rc(expr)) return ISX_ERR_HIP; } while (0)

// ABI v3: the caller's struct must be the library's (isx.h: struct_size)
bool config_abi_ok(const isx_config* c) { return c->struct_size == (uint32_t)sizeof(isx_config); }

// What the absorb test and the azimuth need of a reflectance (Geom / Hot, and per patch PatchTab): stated once.
struct RhoConsts { unsigned long long rho_thr; double inv_thr, psi_k1, psi_k0; };
RhoConsts reflectance_consts(double rho) {
  RhoConsts k;
  // (w + 0.5) * 2^-32 < rho  <=>  w < rho * 2^32 - 0.5 =: x (both scalings exact)  <=>  w < ceil(x) for integer w
  const double x = std::ldexp(rho, 32) - 0.5;
  k.rho_thr = !(x > 0.0) ? 0ull : (x >= 4294967296.0 ? 4294967296ull : (unsigned long long)std::ceil(x));
  k.inv_thr = k.rho_thr ? 1.0 / (double)k.rho_thr : 0.0;
  k.psi_k1 = k.inv_thr * 1.57079632679489655800e+00;
  k.psi_k0 = (0.5 * k.inv_thr - 0.5) * 1.57079632679489655800e+00;
  return k;
}

// The fate scan's integer thresholds (isx_device.hpp: FateConsts; DESIGN.md section 4.2d has the bound behind MARG and SEP).
//   W_leave = (1 - 2^-32 - zcut_in / r_in) 2^31: r_in sphere_z(wa) >= zcut_in  <=>  wa <= W_leave
//   MARG = 2^16 words: the landing point's z differs from r_in sphere_z(wa) by at most 130 words over J_CAP bounces (worst-case bound, 500x under MARG); measured 9.5e-4
//   SEP  = 2^17 words: consecutive words at least this far apart in z give |v| >= r_in SEP 2^-31 (6e-3 cm at the headline)
// ok = the configuration is served: pencil source inside the ball whose first strike q0 (next_hit_s1<true>'s arithmetic in plain
// operations -- the scan only needs it to a margin) lies on the mirror patch by more than MARG, Lambertian border, explicit bounces.
constexpr uint32_t kFateMarg = 1u << 16, kFateSep = 1u << 17, kFateJCap = 1024u;
FateConsts fate_consts(const isx_config* c, const Geom& g) {
  FateConsts f{};
  f.rho_thr = (uint32_t)g.rho_thr; f.never = g.rho_thr > 0xffffffffull ? 1u : 0u; f.sep = kFateSep; f.j_cap = kFateJCap; f.limit = g.limit;
  const double w_leave = (1.0 - 0x1.0p-32 - g.zcut_in / g.r_in) * 0x1.0p31 - (double)kFateMarg;
  const double px = g.src[0], py = g.src[1], pz = g.src[2], vx = g.dir0[0], vy = g.dir0[1], vz = g.dir0[2];
  const double b = px * vx + py * vy + pz * vz;
  const double ci = (px * px + py * py + pz * pz) - g.rin2;
  const double di = b * b - ci;
  bool ok = c->source_model == ISX_SOURCE_PENCIL && c->surface_model == ISX_SURFACE_ROBAST && c->lambertian != 0 &&
            c->trace_mode == ISX_TRACE_EXPLICIT && w_leave >= 0.0 && w_leave < 4294967296.0 && ci < -1e-9 * g.rin2 && di >= 0.0;
  if (ok) {
    f.w_leave = (uint32_t)std::floor(w_leave);
    const double q0z = pz + (std::sqrt(di) - b) * vz;
    const double wq = std::floor((1.0 - 0x1.0p-32 - q0z / g.r_in) * 0x1.0p31 + 0.5);
    ok = wq >= 0.0 && wq <= (double)f.w_leave;
    if (ok) f.w_q0 = (uint32_t)wq;
  }
  f.ok = ok ? 1 : 0;
  return f;
}

int prepare_geom(const isx_config* c, Geom* g, FateConsts* fate = nullptr) {
  if (!config_abi_ok(c)) return ISX_ERR_BAD_CONFIG;
  if (!(c->r_in > 0) || !(c->r_out > c->r_in)) return ISX_ERR_BAD_CONFIG;
  if (!(c->theta_max_deg > 90.0) || !(c->theta_max_deg < 180.0)) return ISX_ERR_BAD_CONFIG;
  if (!(c->box_half > c->r_out)) return ISX_ERR_BAD_CONFIG;
  if (c->max_points < 1) return ISX_ERR_BAD_CONFIG;
  if (c->source_model != ISX_SOURCE_PENCIL && c->source_model != ISX_SOURCE_BRDF) return ISX_ERR_BAD_CONFIG;
  g->rin2 = c->r_in * c->r_in;
  g->rout2 = c->r_out * c->r_out;
  const double th = c->theta_max_deg * M_PI / 180.0;
  const double ct = std::cos(th);
  const double tt = std::tan(th);
  g->zcut_in = c->r_in * ct;
  g->zcut_out = c->r_out * ct;
  g->k2 = tt * tt;
  g->ninv_rin = -1.0 / c->r_in;
  g->inv_rout = 1.0 / c->r_out;
  g->H = c->box_half;
  g->rho = c->reflectance;
  {
    const RhoConsts k = reflectance_consts(c->reflectance);
    g->rho_thr = k.rho_thr; g->inv_thr = k.inv_thr; g->psi_k1 = k.psi_k1; g->psi_k0 = k.psi_k0;
  }
  g->sigma = c->roughness_rad;
  g->lambertian = c->lambertian;
  g->limit = c->max_points;
  g->source_model = c->source_model;
  if (c->surface_model != ISX_SURFACE_ROBAST && c->surface_model != ISX_SURFACE_LOBE) return ISX_ERR_BAD_CONFIG;
  if (c->hit_line_mode != ISX_HITLINE_LAST_SEGMENT && c->hit_line_mode != ISX_HITLINE_ORIGIN_COMPAT) return ISX_ERR_BAD_CONFIG;
  g->surface_model = c->surface_model;
  if (c->trace_mode != ISX_TRACE_EXPLICIT && c->trace_mode != ISX_TRACE_CHORD) return ISX_ERR_BAD_CONFIG;
  g->chord = c->trace_mode; g->pad2 = 0;
  g->r_in = c->r_in;
  g->sched_mask = S.sched_mask;
  g->sched_min = S.sched_min;
  for (int k = 0; k < 3; ++k) g->src[k] = c->src[k];
  const double dx = c->dir[0], dy = c->dir[1], dz = c->dir[2];
  const double mag = std::sqrt(dx * dx + dy * dy + dz * dz);
  if (!(mag > 0)) return ISX_ERR_BAD_CONFIG;
  g->dir0[0] = dx / mag; g->dir0[1] = dy / mag; g->dir0[2] = dz / mag;
  g->brdf_theta_scale = c->brdf[0] * M_PI / 6;
  const double sum = c->brdf[1] + c->brdf[2];
  g->brdf_spec = sum != 0 ? c->brdf[1] / sum : 0.0;
  if (fate) *fate = fate_consts(c, *g);
  return ISX_OK;
}

// Detector::setPosition, operation for operation (fluxAtObserver.C:49-68)
void det_set_position(double theta, double phi, double radius, double portz, double* d) {
  const double theta_rad = theta * M_PI / 180.0;
  const double phi_rad = phi * M_PI / 180.0;
  // the reference is built by g++ -O2 (ACLiC), which turns sin(a),cos(a) into ONE sincos(a)
  double st, ct, sp, cp;
  ::sincos(theta_rad, &st, &ct);
  ::sincos(phi_rad, &sp, &cp);
  const double x = radius * st * cp;
  const double y = radius * st * sp;
  const double z = portz - radius * ct;
  const double dx = x - 0;
  const double dy = y - 0;
  const double dz = z - (portz);
  const double mag = std::sqrt(dx * dx + dy * dy + dz * dz);
  d[0] = x; d[1] = y; d[2] = z;
  d[3] = -dy / mag; d[4] = dx / mag; d[5] = dz / mag;
}

int check_grid(const isx_config* c) {
  if (!config_abi_ok(c)) return ISX_ERR_BAD_CONFIG;
  if (c->n_theta < 1 || c->n_phi < 1) return ISX_ERR_BAD_CONFIG;
  if ((long long)c->n_theta * c->n_phi > 36000) return ISX_ERR_BAD_CONFIG;  // LDS histogram: 4 B/bin
  if (!(c->det_diameter > 0) || !(c->det_distance > 0)) return ISX_ERR_BAD_CONFIG;
  return ISX_OK;
}

void host_tables(const isx_config* c, std::vector<double>& table, std::vector<double>& rowtab,
                 std::vector<double>& coltab) {
  const int nt = c->n_theta, np = c->n_phi;
  table.resize((size_t)nt * np * 6);
  rowtab.resize((size_t)nt * 4);
  coltab.resize((size_t)np * 2);
  for (int i = 0; i < nt; ++i) {
    const double theta = (i + 0.5) * 90.0 / nt;
    const double theta_rad = theta * M_PI / 180.0;
    double st, ct;
    ::sincos(theta_rad, &st, &ct);
    rowtab[4 * i + 0] = st;
    rowtab[4 * i + 1] = ct;
    rowtab[4 * i + 2] = c->exit_port_z - c->det_distance * ct;
    rowtab[4 * i + 3] = c->det_distance * st;
    for (int j = 0; j < np; ++j) {
      const double phi = (j + 0.5) * 360.0 / np;
      det_set_position(theta, phi, c->det_distance, c->exit_port_z, &table[6 * ((size_t)i * np + j)]);
    }
  }
  for (int j = 0; j < np; ++j) {
    const double phi = (j + 0.5) * 360.0 / np;
    const double phi_rad = phi * M_PI / 180.0;
    ::sincos(phi_rad, &coltab[2 * j + 1], &coltab[2 * j + 0]);
  }
}

bool same_grid(const isx_config& a, const isx_config& b) {
  return a.n_theta == b.n_theta && a.n_phi == b.n_phi && a.det_distance == b.det_distance &&
         a.exit_port_z == b.exit_port_z;
}

int sync_all();   // (below, with the call overlap's other helpers)

int ensure_tables(const isx_config* c) {
  if (S.have_tab && same_grid(S.tab_cfg, *c)) return ISX_OK;
  std::vector<double> table, rowtab, coltab;
  host_tables(c, table, rowtab, coltab);
  if (sync_all()) return ISX_ERR_HIP;
  if (table.size() > S.cap_bins) {
    if (S.d_table) HIPCHK(hipFree(S.d_table));
    HIPCHK(hipMalloc(&S.d_table, table.size() * sizeof(double)));
    S.cap_bins = table.size();
  }
  if (rowtab.size() > S.cap_rows) {
    if (S.d_rowtab) HIPCHK(hipFree(S.d_rowtab));
    HIPCHK(hipMalloc(&S.d_rowtab, rowtab.size() * sizeof(double)));
    S.cap_rows = rowtab.size();
  }
  if (coltab.size() > S.cap_cols) {
    if (S.d_coltab) HIPCHK(hipFree(S.d_coltab));
    HIPCHK(hipMalloc(&S.d_coltab, coltab.size() * sizeof(double)));
    S.cap_cols = coltab.size();
  }
  HIPCHK(hipMemcpy(S.d_table, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(S.d_rowtab, rowtab.data(), rowtab.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(S.d_coltab, coltab.data(), coltab.size() * sizeof(double), hipMemcpyHostToDevice));
  S.tab_cfg = *c;
  S.have_tab = true;
  return ISX_OK;
}

// Launch shape of a SMALL launch (round 5; measured in profiles/r05_small_call_sweep.json).  A launch cannot end before its longest
// ray has -- about ln(n) / 0.0175 bounces, one after the other (620 for 5e4 rays) -- so a small launch is bound by latency, not by
// throughput: few rays per tracer lane (the bulk of the work is then short next to the longest ray) and few waves per SIMD (a
// wave that shares its SIMD with five others takes six times as long per bounce).  5e4 rays per call is the reference's own call
// size (traceRaysParallel, fluxAtObserverOptimize.C:568: 0.82 -> 0.29 ms per call).  From ~1.4e6 rays on the grid is what is resident.
struct Shape { int block; uint64_t rays_per_lane; };
Shape small_shape(uint64_t n, int block_default) {
  Shape sh;
  sh.block = (!S.assist_block_set && n < 1000000ull && block_default > 256) ? 256 : block_default;   // 3 tracer waves + the assist wave: one wave per SIMD
  sh.rays_per_lane = S.rays_per_lane > 0 ? (uint64_t)S.rays_per_lane : (n < 150000ull ? 1ull : n < 300000ull ? 2ull : 4ull);
  return sh;
}

// workgroups per CU of a launch's grid (Plan::per_cu): an option's value if > 0, 0 for blocks_per_cu, kResident for what is
// resident -- workgroups of `fn` (workgroup size `block`, `lds` bytes of dynamic LDS) on one CU at a time (queried once, cached)
constexpr int kResident = -1;
int resident_unless(int option) { return option > 0 ? option : kResident; }
int blocks_per_cu(const void* fn, int block, size_t lds, int per_cu) {
  if (per_cu != kResident) return per_cu;
  const auto key = std::make_tuple(fn, block, lds);
  const auto it = S.occ.find(key);
  if (it != S.occ.end()) return it->second;
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, block, lds) != hipSuccess || nb < 1) nb = 1;
  S.occ[key] = nb;
  return nb;
}

// rays a wave takes off the launch's queue at a time: results never depend on it (a ray's history is a function of its index)
uint32_t pick_sub(uint64_t n) {
  if (S.ray_sub > 0) return (uint32_t)S.ray_sub;
  (void)n;
  return 128u;   // (rays a wave takes off the launch's queue at a time; 512 until the bounce got 20 % shorter: measured at 5e7 rays
                 //  64 / 128 / 192 / 256 / 384 / 512 / 1024: 11.26 / 11.18 / 11.19 / 11.20 / 11.23 / 11.33 / 11.40 ms)
}

// the next block of queue counters, zeroed on `stream` ahead of the launch that uses it
int next_ctr(hipStream_t stream, uint32_t** ctr) {
  uint32_t* c = S.d_ctr + (S.ctr_next++ % State::kCtrRing) * Q_WORDS;
  HIPCHK(hipMemsetAsync(c, 0, Q_WORDS * sizeof(uint32_t), stream));
  *ctr = c;
  S.pending = true;   // (every launch takes a block: from here on the stream holds work whose census has not been collected)
  return ISX_OK;
}

// Call overlap (State::call_overlap).  trace_join(): `stream` waits for what the trace streams hold; every entry but an
// overlapped isx_fluxmap_device begins with it, so that a caller who knows one stream sees what it saw before.  trace_begin(): the
// trace streams wait for what `stream` holds now -- whatever ran before an overlapped sequence (another route through workspace 0,
// the caller's own work) comes first, and with it every earlier user of the workspaces.  sync_all(): nothing is left in flight.
int pooled_event(hipEvent_t* e) {
  if (!*e) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
  return ISX_OK;
}
int trace_join() {
  if (!S.trace_open) return ISX_OK;
  const hipStream_t ts[2] = {S.stream2, S.stream3};
  for (int i = 0; i < 2; ++i) {
    if (!ts[i]) continue;
    if (pooled_event(&S.ev_join[i])) return ISX_ERR_HIP;
    HIPCHK(hipEventRecord(S.ev_join[i], ts[i]));
    HIPCHK(hipStreamWaitEvent(S.stream, S.ev_join[i], 0));
  }
  S.trace_open = false;
  return ISX_OK;
}
int trace_begin() {
  if (S.trace_open) return ISX_OK;
  if (!S.stream2) HIPCHK(hipStreamCreateWithFlags(&S.stream2, hipStreamNonBlocking));
  if (!S.stream3) HIPCHK(hipStreamCreateWithFlags(&S.stream3, hipStreamNonBlocking));
  if (pooled_event(&S.ev_join[2])) return ISX_ERR_HIP;
  HIPCHK(hipEventRecord(S.ev_join[2], S.stream));
  HIPCHK(hipStreamWaitEvent(S.stream2, S.ev_join[2], 0));
  HIPCHK(hipStreamWaitEvent(S.stream3, S.ev_join[2], 0));
  for (int b = 0; b < State::kRecBufs; ++b) S.free_set[b] = false;
  S.trace_open = true;
  return ISX_OK;
}
int sync_all() {
  const int rc = trace_join();
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(S.stream));
  if (S.stream2) HIPCHK(hipStreamSynchronize(S.stream2));
  if (S.stream3) HIPCHK(hipStreamSynchronize(S.stream3));
  return ISX_OK;
}

// pinned staging buffer of at least `bytes` bytes: [0, 64) the census words, [64, ...) a call's result
int ensure_pin(size_t bytes) {
  bytes += 64 + 4096;   // (+ the last 4 KB: upload_aux's slot for a short list)
  if (bytes > S.cap_pin) {
    if (sync_all()) return ISX_ERR_HIP;
    if (S.h_pin) HIPCHK(hipHostFree(S.h_pin));
    S.h_pin = nullptr; S.cap_pin = 0;
    const size_t cap = bytes < (1u << 18) ? (1u << 18) : bytes;
    HIPCHK(hipHostMalloc((void**)&S.h_pin, cap, hipHostMallocDefault));
    S.cap_pin = cap;
  }
  return ISX_OK;
}
// D2H of a call's result: enqueued into the staging buffer (no synchronisation here: collect_stats() has the one of the call);
// fetch_result() copies it out once the stream has been synchronised
int stage_result(const void* dev, size_t bytes) {
  const int rc = ensure_pin(bytes);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(S.h_pin + 64, dev, bytes, hipMemcpyDeviceToHost, S.stream));
  S.pending = true;
  return ISX_OK;
}
void fetch_result(void* host, size_t bytes) { std::memcpy(host, S.h_pin + 64, bytes); }
// D2H of a call's result straight into the caller's memory: complete once collect_stats() has synchronised
int copy_out(void* host, const void* dev, size_t bytes) {
  HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, S.stream));
  S.pending = true;
  return ISX_OK;
}

// one launch addresses its rays by 31-bit offsets from its first ray: larger jobs are cut into launches of this many rays
constexpr uint64_t kLaunchMax = 1ull << 30;

// the disc list of the current isx_disc_sweep call as isx_bin_discs_kernel wants it (upload_discs_clustered below)
struct DiscClusters { size_t n = 0, off_ordered = 0, off_clusters = 0, off_perm = 0; int n_clusters = 0; } g_disc_clusters;

// the call being enqueued is isx_fluxmap_device's: the caller collects later, so the next call's trace can start under this one's tail
bool g_device_call = false;

struct PerPos { uint64_t map_first = 0, rays_per_group = 0; int fold = 1; const double* d_table = nullptr; double width = 0; };
struct LogSink { double* rec = nullptr; unsigned long long* count = nullptr; uint64_t cap = 0; };
// isx_exit_maps: the checked spec and the device accumulators of the call (a map that is not wanted: nullptr)
struct ExitSink { const isx_exit_map_spec* spec = nullptr; unsigned long long *dir = nullptr, *pos = nullptr, *counts = nullptr; };

// isx.h: the limits of an exit-map spec (two u32 maps of at most 64 KiB each in a workgroup's LDS)
int check_exit_spec(const isx_exit_map_spec* s) {
  if (s->struct_size != (uint32_t)sizeof(isx_exit_map_spec)) return ISX_ERR_BAD_CONFIG;
  auto axes = [](int32_t a, int32_t b, bool& wanted) {
    wanted = !(a == 0 && b == 0);
    return !wanted || (a >= 1 && a <= ISX_EXIT_MAP_MAX_AXIS && b >= 1 && b <= ISX_EXIT_MAP_MAX_AXIS &&
                       (long long)a * b <= ISX_EXIT_MAP_MAX_BINS);
  };
  bool dir = false, pos = false;
  if (!axes(s->n_u, s->n_v, dir) || !axes(s->n_x, s->n_y, pos) || !(dir || pos)) return ISX_ERR_BAD_CONFIG;
  if (pos && !(std::isfinite(s->plane_z) && std::isfinite(s->half_extent) && s->half_extent > 0)) return ISX_ERR_BAD_CONFIG;
  return ISX_OK;
}

// isx_wall_map: the checked spec and the device accumulators of the call
struct WallSink { const isx_wall_map_spec* spec = nullptr; unsigned long long *map = nullptr, *counts = nullptr; };

// isx.h: the limits of a wall-map spec (one u32 map of at most 32 KiB in a workgroup's LDS)
int check_wall_spec(const isx_wall_map_spec* s) {
  if (s->struct_size != (uint32_t)sizeof(isx_wall_map_spec)) return ISX_ERR_BAD_CONFIG;
  if (s->n_x < 1 || s->n_x > ISX_WALL_MAP_MAX_AXIS || s->n_y < 1 || s->n_y > ISX_WALL_MAP_MAX_AXIS ||
      (long long)s->n_x * s->n_y > ISX_WALL_MAP_MAX_BINS || s->first_order < 0)
    return ISX_ERR_BAD_CONFIG;
  return ISX_OK;
}

// isx_light_field: the checked spec and the device accumulators of the call
struct FieldSink { const isx_exit_map_spec* spec = nullptr; unsigned long long *field = nullptr, *counts = nullptr; };

// isx.h: the limits of a light-field spec (all four axes wanted; the field lives in global memory, or in LDS if it fits)
int check_field_spec(const isx_exit_map_spec* s) {
  if (s->struct_size != (uint32_t)sizeof(isx_exit_map_spec)) return ISX_ERR_BAD_CONFIG;
  long long words = 1;
  for (int32_t a : {s->n_x, s->n_y, s->n_u, s->n_v}) {
    if (a < 1 || a > ISX_LIGHT_FIELD_MAX_AXIS) return ISX_ERR_BAD_CONFIG;
    words *= a;   // (at most 2^40)
  }
  if (words > ISX_LIGHT_FIELD_MAX_BINS) return ISX_ERR_BAD_CONFIG;
  if (!(std::isfinite(s->plane_z) && std::isfinite(s->half_extent) && s->half_extent > 0)) return ISX_ERR_BAD_CONFIG;
  return ISX_OK;
}

// isx_order_hist: the checked spec and the device accumulators of the call (port_dz: nullptr where n_dz == 0)
struct OrderSink { const isx_order_hist_spec* spec = nullptr; unsigned long long *hist = nullptr, *port_dz = nullptr, *counts = nullptr; };

// isx.h: the limits of an order-histogram spec (one u32 block of at most 32 KiB + the counters in a workgroup's LDS)
int check_order_spec(const isx_order_hist_spec* s) {
  if (s->struct_size != (uint32_t)sizeof(isx_order_hist_spec)) return ISX_ERR_BAD_CONFIG;
  if (s->n_orders < 1 || s->n_orders > ISX_ORDER_HIST_MAX_ORDERS || s->n_dz < 0 || s->n_dz > 64 ||
      4ll * s->n_orders + (long long)s->n_orders * s->n_dz > ISX_ORDER_HIST_MAX_WORDS)
    return ISX_ERR_BAD_CONFIG;
  return ISX_OK;
}

// isx_wall_patches: the checked spec and the device accumulators of the call
struct PatchSink { const isx_wall_patch_spec* spec = nullptr; unsigned long long *arrivals = nullptr, *absorbed = nullptr; };

bool patch_ok(const isx_wall_patch& p) {
  return std::isfinite(p.axis[0]) && std::isfinite(p.axis[1]) && std::isfinite(p.axis[2]) && std::isfinite(p.min_dot) &&
         p.reflectance >= 0.0 && p.reflectance <= 1.0;   // (a NaN compares false)
}
// isx.h: the limits of a wall-patch spec and the scope of the call (the explicit Lambertian lean path)
int check_patch_call(const isx_config* c, const isx_wall_patch_spec* s) {
  if (!config_abi_ok(c) || s->struct_size != (uint32_t)sizeof(isx_wall_patch_spec)) return ISX_ERR_BAD_CONFIG;
  if (s->n_patches < 0 || s->n_patches > ISX_MAX_WALL_PATCHES) return ISX_ERR_BAD_CONFIG;
  for (int k = 0; k < s->n_patches; ++k)
    if (!patch_ok(s->patch[k])) return ISX_ERR_BAD_CONFIG;
  if (c->source_model != ISX_SOURCE_PENCIL || c->surface_model != ISX_SURFACE_ROBAST || c->lambertian == 0 ||
      c->trace_mode != ISX_TRACE_EXPLICIT)
    return ISX_ERR_BAD_CONFIG;
  return ISX_OK;
}
static_assert(ISX_MAX_WALL_PATCHES == kMaxPatches, "isx.h and PatchTab");
// the kernel's table of a checked spec: the caps, and per class the constants of its reflectance (classes P and P + 1: the wall's)
PatchTab patch_table(const isx_config& c, const isx_wall_patch_spec& s) {
  PatchTab t;
  std::memset(&t, 0, sizeof(t));
  t.n = s.n_patches;
  for (int k = 0; k < s.n_patches + 2; ++k) {
    const RhoConsts rc = reflectance_consts(k < s.n_patches ? s.patch[k].reflectance : c.reflectance);
    t.rho_thr[k] = rc.rho_thr; t.psi_k1[k] = rc.psi_k1; t.psi_k0[k] = rc.psi_k0;
    if (k < s.n_patches) {
      const isx_wall_patch& p = s.patch[k];
      t.cap[k][0] = p.axis[0]; t.cap[k][1] = p.axis[1]; t.cap[k][2] = p.axis[2]; t.cap[k][3] = p.min_dot;
    }
  }
  return t;
}
// LDS of the patch kernel's block behind the rings: the table and its 2 (P + 2) u32 counters
size_t patch_lds() { return (sizeof(PatchTab) + 2 * (kMaxPatches + 2) * sizeof(uint32_t) + 15) & ~(size_t)15; }

// isx.h: an orthonormal frame, each length and each dot product to 1e-12 (the beam's, a view's, a patch field's: the one
// statement of the test)
bool check_frame(const double* axis, const double* e1, const double* e2) {
  const double* vec[3] = {axis, e1, e2};
  auto dot = [](const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
  for (int k = 0; k < 3; ++k) {
    if (!(std::fabs(std::sqrt(dot(vec[k], vec[k])) - 1.0) <= 1e-12)) return false;
    if (!(std::fabs(dot(vec[k], vec[(k + 1) % 3])) <= 1e-12)) return false;
  }
  return true;
}

// isx.h: the limits of a beam spec and the scope of the call (the explicit Lambertian lean path, either hit line)
int check_beam_call(const isx_config* c, const isx_beam_spec* s) {
  if (!config_abi_ok(c) || s->struct_size != (uint32_t)sizeof(isx_beam_spec)) return ISX_ERR_BAD_CONFIG;
  if (c->source_model != ISX_SOURCE_PENCIL || c->surface_model != ISX_SURFACE_ROBAST || c->lambertian == 0 ||
      c->trace_mode != ISX_TRACE_EXPLICIT)
    return ISX_ERR_BAD_CONFIG;
  const double* vec[4] = {s->origin, s->axis, s->e1, s->e2};
  for (int k = 0; k < 4; ++k)
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(vec[k][i])) return ISX_ERR_BAD_CONFIG;
  if (!std::isfinite(s->radius) || !std::isfinite(s->cos_min) || s->radius < 0.0) return ISX_ERR_BAD_CONFIG;
  if (s->angular_law != ISX_BEAM_UNIFORM && s->angular_law != ISX_BEAM_LAMBERT) return ISX_ERR_BAD_CONFIG;
  if (s->cos_min > 1.0 || s->cos_min < (s->angular_law == ISX_BEAM_LAMBERT ? 0.0 : -1.0)) return ISX_ERR_BAD_CONFIG;
  if (!check_frame(s->axis, s->e1, s->e2)) return ISX_ERR_BAD_CONFIG;
  auto dot = [](const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
  // (the disc's centre strictly inside the inner sphere, every start point strictly inside the world box; a start outside the
  //  inner sphere -- a disc that overhangs the wall -- takes the generic search, as a pencil there does)
  const double ro = std::sqrt(dot(s->origin, s->origin));
  if (!(ro * (1.0 + 1e-12) < c->r_in) || !((ro + s->radius) * (1.0 + 1e-12) < c->box_half)) return ISX_ERR_BAD_CONFIG;
  return ISX_OK;
}
// the kernels' source of a checked spec
// isx.h: cfg->src and cfg->dir are ignored -- the configuration the beam calls prepare has the spec's origin and axis in their place
isx_config beam_config(const isx_config& c, const isx_beam_spec& s) {
  isx_config b = c;
  for (int i = 0; i < 3; ++i) { b.src[i] = s.origin[i]; b.dir[i] = s.axis[i]; }
  return b;
}
BeamSrc beam_source(const isx_beam_spec& s) {
  BeamSrc b;
  std::memset(&b, 0, sizeof(b));
  for (int i = 0; i < 3; ++i) { b.origin[i] = s.origin[i]; b.axis[i] = s.axis[i]; b.e1[i] = s.e1[i]; b.e2[i] = s.e2[i]; }
  b.radius = s.radius; b.cos_min = s.cos_min; b.law = s.angular_law;
  return b;
}
// LDS of the beam kernel's block behind the rings: the source and the tracer waves' parked starts
size_t beam_lds(int tracers) { return kBeamSrcBytes + (size_t)tracers * kBeamParkBytes; }
// isx_beam_cone's frame about `dir` (isx.h states the rule); false: dir has no length
bool beam_frame(const double dir[3], double axis[3], double e1[3], double e2[3]) {
  const double dx = dir[0], dy = dir[1], dz = dir[2];
  const double mag = std::sqrt(dx * dx + dy * dy + dz * dz);   // (prepare_geom's expression for the pencil)
  if (!(mag > 0) || !std::isfinite(mag)) return false;
  axis[0] = dx / mag; axis[1] = dy / mag; axis[2] = dz / mag;
  int k = 0;
  for (int i = 1; i < 3; ++i)
    if (std::fabs(axis[i]) < std::fabs(axis[k])) k = i;
  double u[3];
  for (int i = 0; i < 3; ++i) u[i] = (i == k ? 1.0 : 0.0) - axis[k] * axis[i];
  const double mu = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (int i = 0; i < 3; ++i) e1[i] = u[i] / mu;
  const double w[3] = {axis[1] * e1[2] - axis[2] * e1[1], axis[2] * e1[0] - axis[0] * e1[2], axis[0] * e1[1] - axis[1] * e1[0]};
  const double mw = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  for (int i = 0; i < 3; ++i) e2[i] = w[i] / mw;
  return true;
}

// isx_fluxmap_baffle: the checked spec and the device counters of the call (isx_baffle_counts' layout)
struct BaffleSink { const isx_baffle_spec* spec = nullptr; unsigned long long* counts = nullptr; };
static_assert(ISX_MAX_BAFFLES == kMaxBaffles, "isx.h and BaffleTab");
static_assert(sizeof(isx_baffle_counts) == 4 * kMaxBaffles * sizeof(uint64_t), "isx.h and the kernels' counters");
// isx.h: the limits of a baffle spec and the scope of the call (the explicit Lambertian lean path, either hit line)
int check_baffle_call(const isx_config* c, const isx_baffle_spec* s) {
  if (!config_abi_ok(c) || s->struct_size != (uint32_t)sizeof(isx_baffle_spec)) return ISX_ERR_BAD_CONFIG;
  if (c->source_model != ISX_SOURCE_PENCIL || c->surface_model != ISX_SURFACE_ROBAST || c->lambertian == 0 ||
      c->trace_mode != ISX_TRACE_EXPLICIT)
    return ISX_ERR_BAD_CONFIG;
  if (s->n_baffles < 0 || s->n_baffles > ISX_MAX_BAFFLES) return ISX_ERR_BAD_CONFIG;
  auto dot = [](const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
  for (int k = 0; k < s->n_baffles; ++k) {
    const isx_baffle& b = s->baffle[k];
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(b.centre[i]) || !std::isfinite(b.normal[i])) return ISX_ERR_BAD_CONFIG;
    if (!std::isfinite(b.radius) || !std::isfinite(b.reflectance)) return ISX_ERR_BAD_CONFIG;
    if (!(b.radius > 0.0) || !(b.reflectance >= 0.0 && b.reflectance <= 1.0)) return ISX_ERR_BAD_CONFIG;
    if (!(std::fabs(std::sqrt(dot(b.normal, b.normal)) - 1.0) <= 1e-12)) return ISX_ERR_BAD_CONFIG;
    // (the disc lies strictly inside the cavity and never touches a wall)
    if (!((std::sqrt(dot(b.centre, b.centre)) + b.radius) * (1.0 + 1e-12) < c->r_in)) return ISX_ERR_BAD_CONFIG;
  }
  return ISX_OK;
}
// isx.h: a detector grid whose tables do not fit the binning kernels' LDS is refused -- answered before a device is asked for.  The
// tables are plan_launch's (histogram, row table, column table, DetGrid); the binning kernel that needs least next to them is
// isx_bin_lines_kernel (128 words per wave), which plan_launch falls back to when the slot kernels do not fit.  The LDS a workgroup
// may have is the device's once isx_init has asked it, and gfx950's 160 KiB -- the one target of this library -- before.
constexpr size_t kGfx950Lds = 160 * 1024;
size_t hist_lds(int nbins);
int check_baffle_grid(const isx_config* c) {
  const int rc = check_grid(c);
  if (rc) return rc;
  const size_t tables = hist_lds(c->n_theta * c->n_phi) + (size_t)(4 * c->n_theta) * 8 + (size_t)(2 * c->n_phi) * sizeof(ColX) + sizeof(DetGrid) + 16;
  const size_t limit = S.init ? S.lds_limit : kGfx950Lds;
  return tables + (size_t)(S.bin_block / 64) * 128 * 4 <= limit ? ISX_OK : ISX_ERR_BAD_CONFIG;
}
// the kernels' table of a checked spec (isx.h: the precomputations of the contract, done once here)
BaffleTab baffle_table(const isx_config& c, const isx_baffle_spec& s, unsigned long long* d_counts) {
  BaffleTab t;
  std::memset(&t, 0, sizeof(t));
  t.n = s.n_baffles;
  t.counts = d_counts;
  for (int k = 0; k < s.n_baffles; ++k) {
    const isx_baffle& b = s.baffle[k];
    const RhoConsts rc = reflectance_consts(b.reflectance);
    t.rho_thr[k] = rc.rho_thr; t.psi_k1[k] = rc.psi_k1; t.psi_k0[k] = rc.psi_k0;
    t.r2[k] = b.radius * b.radius;
    for (int i = 0; i < 3; ++i) { t.centre[k][i] = b.centre[i]; t.normal[k][i] = b.normal[i]; t.rm[k][i] = c.r_in * b.normal[i]; }
  }
  return t;
}

// isx_fluxmap_scene: the checked spec and the device counters of the call (isx_scene_counts' layout: 36 words)
constexpr int kSceneBlock = 640;
struct SceneSink { const isx_scene_spec* spec = nullptr; unsigned long long* counts = nullptr; };
constexpr size_t kSceneWords = sizeof(isx_scene_counts) / sizeof(uint64_t);
static_assert(kSceneWords == 2 * (kMaxPatches + 2) + 4 * kMaxBaffles, "isx.h and the kernels' counters");
static_assert(kPatchLds == (sizeof(PatchTab) + 2 * (kMaxPatches + 2) * sizeof(uint32_t) + 15) / 16 * 16, "SceneLds and patch_lds()");
// isx.h: what the three component calls refuse (the nested struct_size fields are theirs to check), in the order beam, baffles,
// patches; `grid`: the two flux-map calls, whose detector grid has to fit the binning kernels' LDS
int check_scene_call(const isx_config* c, const isx_scene_spec* s, bool grid) {
  if (!config_abi_ok(c) || s->struct_size != (uint32_t)sizeof(isx_scene_spec)) return ISX_ERR_BAD_CONFIG;
  int rc = check_beam_call(c, &s->beam);
  if (rc == ISX_OK) rc = check_baffle_call(c, &s->baffles);
  if (rc == ISX_OK) rc = check_patch_call(c, &s->patches);
  if (rc == ISX_OK && grid) rc = check_baffle_grid(c);
  return rc;
}

// isx_scene_response: the device array of the call is [ISX_RESPONSE_FATES][B] (SceneMap below; the scene travels as SceneSink)
static_assert(ISX_RESPONSE_FATES == kRespFates && kRespBaffle0 == ISX_MAX_WALL_PATCHES + 2 &&
              kRespPort == kRespBaffle0 + 2 * ISX_MAX_BAFFLES && kRespSuspended == kRespPort + 2, "isx.h and MapEnd::fate()'s slots");
// isx.h: the limits of a response spec
int check_response_spec(const isx_response_spec* s) {
  if (s->struct_size != (uint32_t)sizeof(isx_response_spec) || s->reserved0 != 0u) return ISX_ERR_BAD_CONFIG;
  long long bins = 1;
  for (int a = 0; a < 4; ++a) {
    if (s->n[a] < 1 || s->n[a] > ISX_RESPONSE_MAX_AXIS) return ISX_ERR_BAD_CONFIG;
    bins *= s->n[a];   // (at most 2^40)
  }
  return bins <= ISX_RESPONSE_MAX_BINS ? ISX_OK : ISX_ERR_BAD_CONFIG;
}
size_t response_bins(const isx_response_spec& s) { return (size_t)s.n[0] * s.n[1] * s.n[2] * s.n[3]; }

// isx_scene_view: the device arrays of the call are the map [n_v][n_u] and the four words of isx_view_counts
static_assert(sizeof(isx_view_counts) == kViewCounters * sizeof(uint64_t) && offsetof(isx_view_counts, binned) == 8 * kViewBinned &&
              offsetof(isx_view_counts, outside) == 8 * kViewOutside && offsetof(isx_view_counts, behind) == 8 * kViewBehind &&
              offsetof(isx_view_counts, direct) == 8 * kViewDirect, "isx.h and ViewMap's counters");
static_assert(sizeof(isx_view_spec) == 104, "isx.h: isx_view_spec");
// isx.h: the limits of a view spec; n_patches < 0: no scene is at hand (the host-side helpers), the patch index is not looked at
int check_view_spec(const isx_view_spec* s, int n_patches) {
  if (s->struct_size != (uint32_t)sizeof(isx_view_spec) || s->reserved0 != 0u || s->reserved1 != 0) return ISX_ERR_BAD_CONFIG;
  if (n_patches >= 0 && (s->patch < 0 || s->patch >= n_patches)) return ISX_ERR_BAD_CONFIG;
  if (s->n_u < 1 || s->n_u > ISX_VIEW_MAX_AXIS || s->n_v < 1 || s->n_v > ISX_VIEW_MAX_AXIS) return ISX_ERR_BAD_CONFIG;
  if ((long long)s->n_u * s->n_v > ISX_VIEW_MAX_BINS) return ISX_ERR_BAD_CONFIG;
  if (!std::isfinite(s->half_extent) || !(s->half_extent > 0.0 && s->half_extent <= 1.0)) return ISX_ERR_BAD_CONFIG;
  const double* vec[3] = {s->axis, s->e1, s->e2};
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(vec[k][i])) return ISX_ERR_BAD_CONFIG;
  return check_frame(s->axis, s->e1, s->e2) ? ISX_OK : ISX_ERR_BAD_CONFIG;
}
size_t view_bins(const isx_view_spec& s) { return (size_t)s.n_u * (size_t)s.n_v; }

// isx_scene_patch_field: the device arrays of the call are the field [n_y][n_x][n_v][n_u] and the five words of
// isx_patch_field_counts
static_assert(sizeof(isx_patch_field_counts) == kFieldCounters * sizeof(uint64_t) && offsetof(isx_patch_field_counts, binned) == 8 * kFieldBinned &&
              offsetof(isx_patch_field_counts, pos_outside) == 8 * kFieldPosOutside &&
              offsetof(isx_patch_field_counts, dir_outside) == 8 * kFieldDirOutside &&
              offsetof(isx_patch_field_counts, behind) == 8 * kFieldBehind && offsetof(isx_patch_field_counts, direct) == 8 * kFieldDirect,
              "isx.h and PatchFieldMap's counters");
static_assert(sizeof(isx_patch_field_spec) == 120, "isx.h: isx_patch_field_spec");
// isx.h: the limits of a patch-field spec; n_patches < 0: no scene is at hand (the host-side helper), the patch index is not looked at
int check_patch_field_spec(const isx_patch_field_spec* s, int n_patches) {
  if (s->struct_size != (uint32_t)sizeof(isx_patch_field_spec) || s->reserved0 != 0u || s->reserved1 != 0) return ISX_ERR_BAD_CONFIG;
  if (n_patches >= 0 && (s->patch < 0 || s->patch >= n_patches)) return ISX_ERR_BAD_CONFIG;
  const int32_t ax[4] = {s->n_x, s->n_y, s->n_u, s->n_v};
  long long prod = 1;
  for (int a = 0; a < 4; ++a) {
    if (ax[a] < 1 || ax[a] > ISX_PATCH_FIELD_MAX_AXIS) return ISX_ERR_BAD_CONFIG;
    prod *= ax[a];   // (at most 2^40)
  }
  if (prod > ISX_PATCH_FIELD_MAX_BINS) return ISX_ERR_BAD_CONFIG;
  if (!std::isfinite(s->half_extent) || !(s->half_extent > 0.0 && s->half_extent <= 1.0)) return ISX_ERR_BAD_CONFIG;
  if (!std::isfinite(s->pos_scale) || !(s->pos_scale > 0.0)) return ISX_ERR_BAD_CONFIG;
  const double* vec[3] = {s->axis, s->e1, s->e2};
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(vec[k][i])) return ISX_ERR_BAD_CONFIG;
  return check_frame(s->axis, s->e1, s->e2) ? ISX_OK : ISX_ERR_BAD_CONFIG;
}
size_t patch_field_bins(const isx_patch_field_spec& s) { return (size_t)s.n_x * (size_t)s.n_y * (size_t)s.n_u * (size_t)s.n_v; }

// isx_scene_order_hist: the device arrays of the call are the histograms [ISX_RESPONSE_FATES][n_orders] and the 21 words of
// isx_scene_order_counts
static_assert(sizeof(isx_scene_order_spec) == 16 && sizeof(isx_scene_order_counts) == kRespFates * sizeof(uint64_t),
              "isx.h: isx_scene_order_spec, and OrderMap's overflow counters");
// isx.h: the limits of a scene order spec
int check_scene_order_spec(const isx_scene_order_spec* s) {
  if (s->struct_size != (uint32_t)sizeof(isx_scene_order_spec) || s->reserved0 != 0u || s->reserved1 != 0) return ISX_ERR_BAD_CONFIG;
  return s->n_orders >= 1 && s->n_orders <= ISX_SCENE_ORDER_MAX_ORDERS ? ISX_OK : ISX_ERR_BAD_CONFIG;
}

// isx_scene_path_hist: the device arrays of the call are the histograms [ISX_RESPONSE_FATES][n_bins] and the 42 words of
// isx_scene_path_counts
static_assert(sizeof(isx_scene_path_spec) == 24 && sizeof(isx_scene_path_counts) == 2 * kRespFates * sizeof(uint64_t),
              "isx.h: isx_scene_path_spec, and PathMap's overflow counters and checksums");
// isx.h: the limits of a scene path spec
int check_scene_path_spec(const isx_scene_path_spec* s) {
  if (s->struct_size != (uint32_t)sizeof(isx_scene_path_spec) || s->reserved0 != 0u || s->reserved1 != 0) return ISX_ERR_BAD_CONFIG;
  if (!(s->n_bins >= 1 && s->n_bins <= ISX_SCENE_PATH_MAX_BINS)) return ISX_ERR_BAD_CONFIG;
  return std::isfinite(s->bin_cm) && s->bin_cm > 0.0 ? ISX_OK : ISX_ERR_BAD_CONFIG;
}

// The scene-map sink of a call -- isx_scene_response, isx_scene_view, isx_scene_patch_field, isx_scene_order_hist,
// isx_scene_path_hist: which of the five (its SINK_*), its spec (the isx_*_spec of that sink), the device array of the map and
// the device array of its own counters behind it (`tail`: isx_view_counts, isx_patch_field_counts, isx_scene_order_counts,
// isx_scene_path_counts; a response has none).  The scene travels as SceneSink next to it.
struct SceneMap {
  int sink = 0;
  const void* spec = nullptr;
  unsigned long long *out = nullptr, *tail = nullptr;
  const isx_response_spec& response() const { return *static_cast<const isx_response_spec*>(spec); }
  const isx_view_spec& view() const { return *static_cast<const isx_view_spec*>(spec); }
  const isx_patch_field_spec& field() const { return *static_cast<const isx_patch_field_spec*>(spec); }
  const isx_scene_order_spec& order() const { return *static_cast<const isx_scene_order_spec*>(spec); }
  const isx_scene_path_spec& path() const { return *static_cast<const isx_scene_path_spec*>(spec); }
};
// isx.h: the limits of the spec of a scene map in a scene of `n_patches` patches, and the words of its two arrays
int scene_map_shape(const SceneMap& m, int n_patches, size_t& body, size_t& tail) {
  int rc;
  switch (m.sink) {
    case SINK_RESPONSE:
      if ((rc = check_response_spec(&m.response()))) return rc;
      body = (size_t)ISX_RESPONSE_FATES * response_bins(m.response()); tail = 0;
      return ISX_OK;
    case SINK_VIEW:
      if ((rc = check_view_spec(&m.view(), n_patches))) return rc;
      body = view_bins(m.view()); tail = kViewCounters;
      return ISX_OK;
    case SINK_FIELD:
      if ((rc = check_patch_field_spec(&m.field(), n_patches))) return rc;
      body = patch_field_bins(m.field()); tail = kFieldCounters;
      return ISX_OK;
    case SINK_SORDER:
      if ((rc = check_scene_order_spec(&m.order()))) return rc;
      body = (size_t)ISX_RESPONSE_FATES * (size_t)m.order().n_orders; tail = kRespFates;
      return ISX_OK;
    case SINK_SPATH:
      if ((rc = check_scene_path_spec(&m.path()))) return rc;
      body = (size_t)ISX_RESPONSE_FATES * (size_t)m.path().n_bins; tail = 2 * kRespFates;
      return ISX_OK;
  }
  return ISX_ERR_BAD_ARG;
}

// LDS of a workgroup's histogram: 4 B per bin, 16-byte aligned
size_t hist_lds(int nbins) { return ((size_t)nbins * 4 + 15) & ~(size_t)15; }

// One call as the launch path sees it: the sink, the configuration, the rays [first, first + n) of `seed`, where the histogram and
// the census go, and whatever the sink needs besides -- every entry point names the fields it sets (in this order), the rest
// stay empty.
struct Call {
  int sink = SINK_FLUX;
  const isx_config* c = nullptr;
  uint64_t n = 0, seed = 0, first = 0;
  unsigned long long* d_hist = nullptr;    // the histogram (device); nullptr for the sinks that carry their own arrays
  unsigned long long* d_stats = nullptr;   // the census words (device); nullptr: S.d_stats
  int nbins_override = 0;                  // bins of a caller-supplied detector or disc list
  const double* d_discs = nullptr;         // the disc list (device), the discs' radius and half thickness
  double disc_r = 0, disc_h = 0;
  const PerPos* pp = nullptr;              // SINK_PERPOS, SINK_DISCPOS
  const LogSink* lg = nullptr;             // SINK_LOG
  const ExitSink* xm = nullptr;            // SINK_EXITMAP
  const WallSink* wm = nullptr;            // SINK_WALL
  const FieldSink* lf = nullptr;           // SINK_LIGHTFIELD
  const OrderSink* oh = nullptr;           // SINK_ORDER
  const PatchSink* wp = nullptr;           // SINK_PATCH
  const isx_beam_spec* bs = nullptr;       // SINK_FLUX with a beam source (a scene: enqueue sets it)
  const BaffleSink* bf = nullptr;          // SINK_FLUX with baffles (a scene: enqueue sets it)
  const SceneSink* sc = nullptr;           // a scene: isx_fluxmap_scene and the five scene maps
  const SceneMap* map = nullptr;           // SINK_RESPONSE, SINK_VIEW, SINK_FIELD, SINK_SORDER, SINK_SPATH
};
// The DetGrid of a call's sink, checked, and the dynamic LDS of its fused kernel (histogram + tables, census, Geom, DetGrid).
int sink_grid(const Call& k, DetGrid& d, size_t& lds) {
  const int sink = k.sink, nbins_override = k.nbins_override;
  const isx_config* c = k.c;
  const double* d_discs = k.d_discs;
  const double disc_r = k.disc_r, disc_h = k.disc_h;
  const PerPos* pp = k.pp; const LogSink* lg = k.lg; const ExitSink* xm = k.xm; const WallSink* wm = k.wm; const FieldSink* lf = k.lf;
  const OrderSink* oh = k.oh; const PatchSink* wp = k.wp; const isx_beam_spec* bs = k.bs;
  std::memset(&d, 0, sizeof(d));
  d.portz = c->exit_port_z;
  d.hit_line_mode = c->hit_line_mode;
  int rc;
  if (sink == SINK_FLUX) {
    rc = check_grid(c);
    if (rc) return rc;
    rc = ensure_tables(c);
    if (rc) return rc;
    if (bs && (rc = check_beam_call(c, bs))) return rc;
    d.n_theta = c->n_theta; d.n_phi = c->n_phi; d.nbins = c->n_theta * c->n_phi; d.bin_mode = S.bin_mode;
    if (bs && S.bin_mode == 2) d.bin_mode = 1;   // (isx.h: the trace-only diagnostic does not apply to the beam)
    d.half_w2 = (c->det_diameter / 2) * (c->det_diameter / 2);
    d.rho_d = c->det_diameter / 2;
    d.R = c->det_distance;
    d.table = S.d_table; d.rowtab = S.d_rowtab; d.coltab = S.d_coltab;
    lds = hist_lds(d.nbins) + (size_t)(4 * d.n_theta) * 8 + (size_t)(2 * d.n_phi) * sizeof(ColX) + 64 + sizeof(Geom) + sizeof(DetGrid);
  } else if (sink == SINK_PERPOS) {
    if (!pp || pp->rays_per_group < 1 || (pp->fold != 1 && pp->fold != 2)) return ISX_ERR_BAD_ARG;
    if (pp->d_table) {  // caller-supplied detector list (traceRays with one Detector)
      if (nbins_override < 1 || nbins_override > 36000 || pp->fold != 1) return ISX_ERR_BAD_ARG;
      d.n_theta = nbins_override; d.n_phi = 1; d.nbins = nbins_override;
      d.table = pp->d_table;
      d.half_w2 = (pp->width / 2) * (pp->width / 2);
    } else {
      rc = check_grid(c);
      if (rc) return rc;
      if (pp->fold == 2 && (c->n_phi % 2) != 0) return ISX_ERR_BAD_CONFIG;
      rc = ensure_tables(c);
      if (rc) return rc;
      d.n_theta = c->n_theta; d.n_phi = c->n_phi; d.nbins = c->n_theta * c->n_phi;
      d.table = S.d_table;
      d.half_w2 = (c->det_diameter / 2) * (c->det_diameter / 2);
    }
    d.map_first = pp->map_first; d.rays_per_group = pp->rays_per_group; d.fold = pp->fold;
    lds = hist_lds(d.nbins) + 64 + sizeof(Geom) + sizeof(DetGrid);
  } else if (sink == SINK_DISCPOS) {
    if (!pp || pp->rays_per_group < 1 || nbins_override < 1 || nbins_override > 36000) return ISX_ERR_BAD_ARG;
    d.nbins = nbins_override;
    d.discs = d_discs; d.disc_r = disc_r; d.disc_h = disc_h;
    d.map_first = pp->map_first; d.rays_per_group = pp->rays_per_group; d.fold = 1;
    lds = hist_lds(d.nbins) + 64 + sizeof(Geom) + sizeof(DetGrid);
  } else if (sink == SINK_LOG) {
    if (!lg || !lg->rec || !lg->count) return ISX_ERR_BAD_ARG;
    d.nbins = 1;
    d.log_rec = lg->rec; d.log_count = lg->count; d.log_cap = lg->cap;
    lds = 16 + 64 + sizeof(Geom) + sizeof(DetGrid);
  } else if (sink == SINK_EXITMAP) {
    if (!xm || !xm->spec || !xm->counts) return ISX_ERR_BAD_ARG;
    rc = check_exit_spec(xm->spec);
    if (rc) return rc;
    const isx_exit_map_spec& s = *xm->spec;
    if ((s.n_u > 0 && !xm->dir) || (s.n_x > 0 && !xm->pos)) return ISX_ERR_BAD_ARG;
    d.hit_line_mode = ISX_HITLINE_LAST_SEGMENT;   // (isx.h: the maps always see the real last segment)
    d.xm_nu = s.n_u; d.xm_nv = s.n_v; d.xm_nx = s.n_x; d.xm_ny = s.n_y;
    d.xm_plane_z = s.plane_z; d.xm_half = s.half_extent;
    d.xm_dir = xm->dir; d.xm_pos = xm->pos; d.xm_counts = xm->counts;
    d.nbins = s.n_u * s.n_v + s.n_x * s.n_y + 5;   // the workgroup's LDS block: direction map | plane map | the five counters
    lds = hist_lds(d.nbins) + 64 + sizeof(Geom) + sizeof(DetGrid);
  } else if (sink == SINK_LIGHTFIELD) {
    if (!lf || !lf->spec || !lf->field || !lf->counts) return ISX_ERR_BAD_ARG;
    rc = check_field_spec(lf->spec);
    if (rc) return rc;
    const isx_exit_map_spec& s = *lf->spec;
    d.hit_line_mode = ISX_HITLINE_LAST_SEGMENT;   // (isx.h: the field always sees the real last segment)
    // (the spec travels in the exit maps' words of DetGrid: isx_kernels.hpp)
    d.xm_nu = s.n_u; d.xm_nv = s.n_v; d.xm_nx = s.n_x; d.xm_ny = s.n_y;
    d.xm_plane_z = s.plane_z; d.xm_half = s.half_extent;
    d.xm_dir = lf->field; d.xm_counts = lf->counts;
    d.nbins = 4;   // the LDS block of a fused kernel's workgroup: the four counters (the pipeline's binning kernel: plan_launch)
    lds = hist_lds(d.nbins) + 64 + sizeof(Geom) + sizeof(DetGrid);
  } else if (sink == SINK_WALL) {
    if (!wm || !wm->spec || !wm->map || !wm->counts) return ISX_ERR_BAD_ARG;
    rc = check_wall_spec(wm->spec);
    if (rc) return rc;
    const isx_wall_map_spec& s = *wm->spec;
    d.hit_line_mode = ISX_HITLINE_LAST_SEGMENT;   // (isx.h: ignored -- no exit line is looked at)
    // (the spec travels in the exit maps' words of DetGrid: isx_kernels.hpp)
    d.xm_nx = s.n_x; d.xm_ny = s.n_y; d.xm_nu = s.first_order;
    d.xm_plane_z = 1.0 / c->r_in;
    d.xm_pos = wm->map; d.xm_counts = wm->counts;
    d.nbins = s.n_x * s.n_y + 4;   // the workgroup's LDS block: the map | the four counters
    lds = hist_lds(d.nbins) + 64 + sizeof(Geom) + sizeof(DetGrid);
  } else if (sink == SINK_ORDER) {
    if (!oh || !oh->spec || !oh->hist || !oh->counts) return ISX_ERR_BAD_ARG;
    rc = check_order_spec(oh->spec);
    if (rc) return rc;
    const isx_order_hist_spec& s = *oh->spec;
    if (s.n_dz > 0 && !oh->port_dz) return ISX_ERR_BAD_ARG;
    d.hit_line_mode = ISX_HITLINE_LAST_SEGMENT;   // (isx.h: ignored -- no exit line is looked at)
    // (the spec travels in the exit maps' words of DetGrid: isx_kernels.hpp)
    d.xm_nx = s.n_orders; d.xm_ny = s.n_dz;
    d.xm_dir = oh->hist; d.xm_pos = oh->port_dz; d.xm_counts = oh->counts;
    d.nbins = 4 * s.n_orders + s.n_orders * s.n_dz + 5;   // the workgroup's LDS block: the histograms | the port's dz | the five counters
    lds = hist_lds(d.nbins) + 64 + sizeof(Geom) + sizeof(DetGrid);
  } else if (sink == SINK_PATCH) {
    if (!wp || !wp->spec || !wp->arrivals || !wp->absorbed) return ISX_ERR_BAD_ARG;
    rc = check_patch_call(c, wp->spec);
    if (rc) return rc;
    d.hit_line_mode = ISX_HITLINE_LAST_SEGMENT;   // (isx.h: ignored -- no exit line is looked at)
    // (the spec travels in the exit maps' words of DetGrid: isx_kernels.hpp)
    d.xm_nx = wp->spec->n_patches;
    d.xm_dir = wp->arrivals; d.xm_pos = wp->absorbed;
    d.nbins = 2 * (wp->spec->n_patches + 2);
    lds = patch_lds() + 64 + sizeof(Geom) + sizeof(DetGrid);
  } else if (sink == SINK_RESPONSE || sink == SINK_VIEW || sink == SINK_FIELD || sink == SINK_SORDER || sink == SINK_SPATH) {
    // (isx.h: hit_line_mode and the detector grid are ignored -- no exit line is written, no grid is looked at; the scene and the
    //  response spec were checked by the entry, the patches' words are enqueue's)
    d.hit_line_mode = ISX_HITLINE_LAST_SEGMENT;
    d.nbins = 1;
    lds = 16 + 64 + sizeof(Geom) + sizeof(DetGrid);
  } else {
    if (nbins_override < 1 || nbins_override > 36000) return ISX_ERR_BAD_ARG;
    d.nbins = nbins_override;
    d.discs = d_discs; d.disc_r = disc_r; d.disc_h = disc_h;
    lds = hist_lds(d.nbins) + 64 + sizeof(Geom) + sizeof(DetGrid);
  }
  // the per-block histogram (+ tables) must fit the workgroup's LDS: a grid too fine for that is a configuration error
  if (lds > S.lds_limit) return ISX_ERR_BAD_CONFIG;
  if (sink == SINK_FLUX) {
    // room for the per-lane exit-line records of the lean kernels (16 + 4 B per lane) and the long-row list of the column
    // walk (4 B per lane), if the grid leaves it
    const size_t stage = 16 + (size_t)kBlock * 24;
    if (lds + stage <= S.lds_limit) { lds += stage; d.rec_stage = 1; }
  }
  return ISX_OK;
}

// ---- The launch plan of a call: the route, its kernel(s) and their workgroup shapes.
//  ROUTE_FLUX_PIPE  flux maps: per chunk a trace kernel (exit lines -> HBM workspace) and a binning kernel
//  ROUTE_EXIT_PIPE  exit maps: the flux pipeline's trace kernels, workspace and chunking; isx_bin_exitmaps_kernel streams the lines
//  ROUTE_FIELD_PIPE the light field the same way; isx_bin_lightfield_kernel bins into LDS or, a field too large for it, into global memory
//  ROUTE_DISC_PIPE  the shared-ray disc sweep the same way: assist-wave trace kernel (exit segments) -> isx_bin_discs_kernel
//  ROUTE_ASSIST     the per-position sinks: one assist-wave kernel, whose assist wave does the exact test per exiting ray;
//                   the wall map: one assist-wave kernel whose waves bin every interaction into the workgroup's LDS map;
//                   the order histograms: one assist-wave kernel whose waves bin every ray where it ends
//  ROUTE_FUSED      one kernel that traces and bins: everything the routes above do not serve
enum Route { ROUTE_FUSED, ROUTE_ASSIST, ROUTE_FLUX_PIPE, ROUTE_EXIT_PIPE, ROUTE_FIELD_PIPE, ROUTE_DISC_PIPE };
typedef void (*BinFn)(const DetGrid, const Work);
// A trace kernel: its address and what it takes behind (Geom, DetGrid, Work).  The constructors read the tail off the kernel's
// own signature, so a kernel cannot be paired with the wrong arguments; launch_trace() is the one place that passes them.
enum Tail { TAIL_NONE, TAIL_PATCH, TAIL_BEAM, TAIL_LIST, TAIL_BAFFLE, TAIL_SCENE, TAIL_SCENE_MAP };
// the sink of a scene map as its kernel takes it (isx_kernels.hpp: the Arg of the map's policy)
typedef std::variant<std::monostate, RespSink, ViewSink, PatchFieldSink, SOrderSink, SPathSink> MapSink;
struct TraceKernel {
  const void* fn = nullptr;
  Tail tail = TAIL_NONE;
  template <class... A> using Fn = void (*)(const Geom, const DetGrid, const Work, const A...);
  TraceKernel() = default;
  TraceKernel(Fn<> f) : fn((const void*)f), tail(TAIL_NONE) {}
  TraceKernel(Fn<PatchTab> f) : fn((const void*)f), tail(TAIL_PATCH) {}
  TraceKernel(Fn<BeamSrc> f) : fn((const void*)f), tail(TAIL_BEAM) {}
  TraceKernel(Fn<FateList> f) : fn((const void*)f), tail(TAIL_LIST) {}
  TraceKernel(Fn<BaffleTab> f) : fn((const void*)f), tail(TAIL_BAFFLE) {}
  TraceKernel(Fn<PatchTab, BeamSrc, BaffleTab> f) : fn((const void*)f), tail(TAIL_SCENE) {}
  template <class Sink> using MapFn = Fn<PatchTab, BeamSrc, BaffleTab, Sink>;   // (Sink: an alternative of MapSink -- Plan::set_map)
  template <class Sink> TraceKernel(MapFn<Sink> f) : fn((const void*)f), tail(TAIL_SCENE_MAP) {}
};
struct Plan {
  Route route = ROUTE_FUSED;
  TraceKernel fn;               // the kernel (a pipeline's trace kernel); its tail is taken from the members below
  int block = kBlock;           // its workgroup size
  size_t lds = 0;               // its dynamic LDS
  int tracers = 0;              // its tracer waves per workgroup
  uint64_t rays_per_lane = 4;   // rays per tracer lane the grid is sized for
  int per_cu = 0;               // workgroups per CU (blocks_per_cu)
  BinFn bin = nullptr;          // pipelines: the binning kernel, its workgroup size, workgroups per CU and dynamic LDS
  int bblock = 0, bin_per_cu = kResident;
  size_t lds_bin = 0;
  int bin_words = 0;            // ROUTE_FIELD_PIPE: words of the binning workgroup's LDS block (DetGrid::nbins of that kernel)
  bool assist = true;           // the trace kernel has an assist wave (one writing wave per workgroup)
  bool compat_lines = false;    // isx_compat_lines_kernel runs between the two (ISX_HITLINE_ORIGIN_COMPAT)
  bool binning = true;          // false: bin_mode 2, a diagnostic: trace only
  bool overlap = false;         // chunks alternate over two streams (S.overlap)
  bool call_overlap = false;    // the chunks' scans and traces go to a trace stream, ahead of the earlier binning (S.call_overlap)
  size_t slot_doubles = 6;      // doubles per exit record in the workspace
  uint64_t launch_max = 0;      // ROUTE_FUSED / ROUTE_ASSIST: rays per launch (0: kLaunchMax)
  TraceKernel list;             // ROUTE_FLUX_PIPE behind the fate scan: isx_fate_scan_kernel, then this kernel on the rays it left, instead
                                // of fn (which a chunk below the automatic rule's size still takes: launch_pair)
  FateConsts fate{};
  bool fate_auto = false;       // "fate_scan" -1: the rule's ray count is looked at per chunk (launch_pair)
  bool exit_lines = false;      // behind the scan: isx_exit_lines_kernel settles the clean port exits, the list kernel traces the rest,
  uint32_t w_exit = 0;          //   isx_redo_kernel follows the binning kernel; w_exit = ceil(W_leave + MARG)
  // the kernels' trailing arguments (launch_trace): enqueue fills the three tables, plan_scene_map the sink of a scene map
  PatchTab patch_tab{};         // SINK_PATCH; a scene
  BeamSrc beam{};               // isx_fluxmap_beam; a scene
  BaffleTab baffles{};          // isx_fluxmap_baffle; a scene
  MapSink map;                  // the sink of a scene map (its lds_* field: the form of the kernel)
  // a scene map's kernel and its sink, set together: the struct that is filled is the one the kernel's signature names
  template <class Sink> Sink& set_map(TraceKernel::MapFn<Sink> f) { fn = f; return map.emplace<Sink>(); }
};

// The one place a trace kernel is launched: (g, d, w) and the tail its signature names, as hipLaunchKernelGGL would pass them.
// `fl`: the fate scan's list, for TAIL_LIST.  The caller asks hipGetLastError().
void launch_trace(const Plan& p, const TraceKernel& k, int grid, hipStream_t stream, const Geom& g, const DetGrid& d, const Work& w,
                  const FateList* fl = nullptr) {
  const void* args[7] = {&g, &d, &w};
  int na = 3;
  switch (k.tail) {
    case TAIL_NONE: break;
    case TAIL_PATCH: args[na++] = &p.patch_tab; break;
    case TAIL_BEAM: args[na++] = &p.beam; break;
    case TAIL_LIST: args[na++] = fl; break;
    case TAIL_BAFFLE: args[na++] = &p.baffles; break;
    default:   // a scene: its three tables, then the sink of a scene map
      args[na++] = &p.patch_tab; args[na++] = &p.beam; args[na++] = &p.baffles;
      if (k.tail == TAIL_SCENE_MAP) args[na++] = std::visit([](const auto& sink) -> const void* { return &sink; }, p.map);
  }
  (void)hipLaunchKernel(k.fn, dim3(grid), dim3(p.block), const_cast<void**>(args), p.lds, stream);
}

// "fate_scan" = -1: where the scan pays (measured on MI355X, docs/LOG.md section 16.3).  A small launch is bound by its longest
// ray, and a second launch in front of it only adds to that: trace + binning of the default configuration with the scan against
// without, 1.18 / 1.05 ms at 1e6 rays, 2.29 / 2.21 at 5e6, 3.70 / 3.79 at 1e7, 6.65 / 7.01 at 2e7 -- break-even near 7e6.  And
// the scan walks every interaction of every ray to settle the share (1 - rho) / ((1 - rho) + port area fraction) of them -- what
// the wall absorbs of what ends at all: at 1e7 rays it gains at shares 0.87 and 0.57 and loses at 0.40 and below.
constexpr uint64_t kFateMinRays = 10000000ull;
constexpr double kFateMinShare = 0.50;
bool fate_scan_auto(const isx_config* c, uint64_t chunk_rays) {
  const double absorb = 1.0 - c->reflectance;
  const double port = 0.5 * (1.0 + std::cos(c->theta_max_deg * M_PI / 180.0));
  return chunk_rays >= kFateMinRays && absorb > 0.0 && absorb / (absorb + port) >= kFateMinShare;
}

// workgroups of a launch of n rays: enough for p.rays_per_lane rays per tracer lane, no more than `per_cu` per CU
int pick_grid(const Plan& p, uint64_t n, int per_cu) {
  if (S.grid_blocks > 0) return S.grid_blocks;
  const int full = S.cu_count * (per_cu > 0 ? per_cu : S.blocks_per_cu);
  const uint64_t lanes = (uint64_t)p.tracers * 64ull * p.rays_per_lane;
  const uint64_t want = (n + lanes - 1) / lanes;
  if (want < 1) return 1;
  return want < (uint64_t)full ? (int)want : full;
}
// workgroups of a binning launch: a wave per work unit -- the quarter regions of `cnt` exit lines (sixteenths for pad 2) plus
// the open region each of `writers` writing waves of the trace kernel leaves behind -- no more than `per_cu` per CU
int bin_grid(const Plan& p, uint64_t cnt, uint32_t pad, uint64_t writers, int per_cu) {
  if (S.grid_blocks > 0) return S.grid_blocks;
  const uint64_t waves = (uint64_t)(p.bblock / 64);
  const uint64_t want = (cnt / (kRegion >> (2u + pad)) + writers + waves - 1) / waves;
  const int full = S.cu_count * per_cu;
  return want < (uint64_t)full ? (int)want : full;
}

// workgroups of isx_exit_lines_kernel for a chunk of `cnt` rays: its list is at most the chunk, eight entries per lane, four
// workgroups of four waves per CU at most (every wave leaves an open region)
int exit_grid(uint64_t cnt) {
  if (S.grid_blocks > 0) return S.grid_blocks;
  const uint64_t want = (cnt + 8ull * kExitBlock - 1) / (8ull * kExitBlock), full = (uint64_t)S.cu_count * 4ull;
  return (int)std::max<uint64_t>(1, std::min(want, full));
}
// the shape of a trace kernel with or without an assist wave: workgroup, tracer waves, grid, LDS (census, Geom, DetGrid, and
// with an assist wave the queues and rings)
void trace_shape(Plan& p, Shape sh, bool assist, int per_cu) {
  p.block = sh.block; p.rays_per_lane = sh.rays_per_lane;
  p.tracers = sh.block / 64 - (assist ? 1 : 0);
  p.per_cu = per_cu;
  p.lds = 16 + 64 + sizeof(Geom) + sizeof(DetGrid) + (assist ? 16 + sizeof(AssistQueues) + (size_t)(kResumeCap + kPendCap) * 64 : 0);
  p.assist = assist;
}

// The shape and the LDS of a scene map's one kernel.  A scene map (isx_scene_response, isx_scene_view, isx_scene_patch_field,
// isx_scene_order_hist, isx_scene_path_hist) has one route whatever the switches say, as the scene has: the scene's trace kernel `fn` with the map as
// its one sink (check_scene_call: the explicit Lambertian lean path), in the scene's shape, the scene's three blocks behind the
// rings; no exit lines, no second kernel.  Launches are cut at pipeline_chunk as the scene's are.  Behind the parks lie `head`
// bytes the kernel always keeps there (counters, a frame) and then up to `units` units of `unit` u32 words each of the map itself,
// flushed once per workgroup: as many of them as cost no resident workgroup -- as many workgroups as the occupancy query of the
// grid finds without the block still fit the LDS with it.  What does not lie in LDS takes one global u64 add per record.
//   (two 640-thread workgroups: 68.8 KiB each without the block, 80 KiB to be had -- 2864 words; the sum is taken over 2 KiB
//    steps so that the device's allocation granule cannot turn "fits" into one workgroup fewer)
// With cap the largest 2 KiB-rounded size `resident` workgroups can have, a block of w words fits -- the 2 KiB-rounded sum of
// p.lds and the 16-byte-rounded 4 w times the resident count stays within lds_limit -- exactly when w <= room: both roundings are
// to multiples that cap and cap - p.lds rounded down already are.  So one expression serves the maps that lie in LDS whole or not
// at all (one unit: the map) and the order histograms (a unit per order: as many orders as fit).  All sums in size_t: a field has
// up to 2^22 words.  `kept`: the units that went to LDS; p.lds has their bytes.  Returns the kernel's sink, zeroed, to be filled.
template <class Sink>
Sink& plan_scene_map_lds(Plan& p, TraceKernel::MapFn<Sink> fn, uint64_t n, size_t head, size_t unit, size_t units, size_t& kept) {
  p.route = ROUTE_ASSIST;
  Sink& sink = p.set_map(fn);
  p.launch_max = std::min(kLaunchMax, S.pipe_chunk);
  // (the kernel is built for five waves per SIMD: 640 threads -- nine tracer waves and the assist wave -- are what two
  //  workgroups of a CU may have, unless assist_block was set)
  trace_shape(p, small_shape(std::min(n, p.launch_max), S.assist_block_set ? S.assist_block : kSceneBlock), true,
              resident_unless(S.trace_blocks_per_cu));
  p.lds += SceneLds::bytes(p.tracers) + head;
  const size_t resident = (size_t)blocks_per_cu(p.fn.fn, p.block, p.lds, kResident);
  const size_t cap = (S.lds_limit / resident) & ~(size_t)2047;
  const size_t room = cap > p.lds ? ((cap - p.lds) & ~(size_t)15) / 4 : 0;
  kept = std::min(units, room / unit);
  p.lds += (kept * unit * 4 + 15) & ~(size_t)15;
  return sink;
}

// The plan of a scene map and the kernel's sink struct, from the call's SceneMap: per map the kernel, what it keeps behind the
// parks in both forms, the words of the map and the switch that sends all of them to global memory (a diagnostic).
Plan plan_scene_map(const Call& k) {
  const SceneMap& m = *k.map;
  const isx_scene_spec& sc = *k.sc->spec;
  // (the scene's compact slots: P + 2 wall classes, two sides per baffle, port / other exits / suspended)
  const size_t slots = (size_t)((sc.patches.n_patches + 2) + 2 * sc.baffles.n_baffles + 3);
  Plan p;
  size_t kept = 0;
  switch (m.sink) {
    case SINK_RESPONSE: {   // (ResponseMap) the slots times the bins, whole or not at all; "resp_global"
      const isx_response_spec& s = m.response();
      const size_t words = slots * response_bins(s);
      RespSink& r = plan_scene_map_lds(p, isx_trace_assist_scene_response_kernel, k.n, 0, words, S.resp_global ? 0 : 1, kept);
      r.lds_words = (uint32_t)(words * kept);
      r.out = m.out;
      for (int a = 0; a < 4; ++a) r.n[a] = (uint32_t)s.n[a];
      r.B = (uint32_t)response_bins(s);
      break;
    }
    case SINK_VIEW: {   // (ViewMap) behind the four counters the n_u * n_v words of the map, whole or not at all; "view_global"
      const isx_view_spec& v = m.view();
      ViewSink& r = plan_scene_map_lds(p, isx_trace_assist_scene_view_kernel, k.n, kViewCounters * sizeof(uint32_t), view_bins(v),
                                       S.view_global ? 0 : 1, kept);
      r.lds_words = (uint32_t)(view_bins(v) * kept);
      r.out = m.out; r.counts = m.tail;
      for (int i = 0; i < 3; ++i) { r.axis[i] = v.axis[i]; r.e1[i] = v.e1[i]; r.e2[i] = v.e2[i]; }
      r.h = v.half_extent; r.fnu = (double)v.n_u; r.fnv = (double)v.n_v;
      r.patch = v.patch; r.n_u = v.n_u;
      break;
    }
    case SINK_FIELD: {   // (PatchFieldMap) behind the frame's doubles and the five counters (kFieldHead bytes) the n_x * n_y * n_u * n_v
                         // words of the field, whole or not at all; "field_global"
      const isx_patch_field_spec& v = m.field();
      PatchFieldSink& r = plan_scene_map_lds(p, isx_trace_assist_scene_field_kernel, k.n, kFieldHead, patch_field_bins(v),
                                             S.field_global ? 0 : 1, kept);
      r.lds_words = (uint32_t)(patch_field_bins(v) * kept);
      r.out = m.out; r.counts = m.tail;
      PatchFieldFrame& f = r.f;
      for (int i = 0; i < 3; ++i) { f.axis[i] = v.axis[i]; f.e1[i] = v.e1[i]; f.e2[i] = v.e2[i]; }
      f.h = v.half_extent; f.s = v.pos_scale; f.inv = 1.0 / k.c->r_in;   // (isx.h: inv is formed once, here)
      f.fnx = (double)v.n_x; f.fny = (double)v.n_y; f.fnu = (double)v.n_u; f.fnv = (double)v.n_v;
      r.patch = v.patch; r.n_x = v.n_x; r.n_u = v.n_u; r.n_v = v.n_v;
      break;
    }
    case SINK_SORDER: {   // (OrderMap): behind the overflow counters (kSOrderHead words, always) the first L orders of each
                 // slot; the orders from L on take one global u64 add each.  L is as large as fits and at most n_orders;
                 // "sorder_lds_orders" >= 0 caps it (0: every order is global).  L is SOrderSink::lds_orders, nothing else.
      const isx_scene_order_spec& s = m.order();
      size_t orders = (size_t)s.n_orders;
      if (S.sorder_lds_orders >= 0) orders = std::min(orders, (size_t)S.sorder_lds_orders);
      SOrderSink& r = plan_scene_map_lds(p, isx_trace_assist_scene_order_kernel, k.n, kSOrderHead * sizeof(uint32_t), slots, orders, kept);
      r.lds_orders = (uint32_t)kept;
      r.out = m.out; r.overflow = m.tail; r.n_orders = (uint32_t)s.n_orders;
      break;
    }
    default: {   // SINK_SPATH (PathMap): SINK_SORDER's hybrid form.  Behind the side arrays of the two rings, the checksums and the
                 // overflow counters (kSPathHeadBytes, always) the first B bins of each slot; the bins from B on take one global
                 // u64 add each.  B is as large as fits and at most n_bins; "spath_lds_bins" >= 0 caps it (0: every bin is
                 // global).  B is SPathSink::lds_bins, nothing else.
      const isx_scene_path_spec& s = m.path();
      size_t bins = (size_t)s.n_bins;
      if (S.spath_lds_bins >= 0) bins = std::min(bins, (size_t)S.spath_lds_bins);
      SPathSink& r = plan_scene_map_lds(p, isx_trace_assist_scene_path_kernel, k.n, kSPathHeadBytes, slots, bins, kept);
      r.lds_bins = (uint32_t)kept;
      r.out = m.out; r.counts = m.tail; r.bin_cm = s.bin_cm; r.n_bins = (uint32_t)s.n_bins;
    }
  }
  return p;
}

// fate: the fate scan's constants of the call's configuration (nullptr: no trace kernel will run -- the injected-record entries)
Plan plan_launch(const Call& k, const DetGrid& d, size_t lds, const FateConsts* fate = nullptr) {
  if (k.map) return plan_scene_map(k);
  const int sink = k.sink;
  const isx_config* c = k.c;
  const uint64_t n = k.n;
  const bool beam = k.bs != nullptr, baffle = k.bf != nullptr, scene = k.sc != nullptr;
  const bool discs_in_aux = k.d_discs == S.d_aux;   // (the list upload_discs_clustered left there)
  enum { LAMBERT, LOBE, ROUGH } const border =
      c->surface_model == ISX_SURFACE_LOBE ? LOBE : c->lambertian ? LAMBERT : ROUGH;   // (ISX_SURFACE_ROBAST: Lambertian or rough-specular)
  const bool pencil = c->source_model == ISX_SOURCE_PENCIL;   // (else ISX_SOURCE_BRDF)
  const bool chord = c->trace_mode == ISX_TRACE_CHORD;
  const bool compat = c->hit_line_mode != ISX_HITLINE_LAST_SEGMENT;
  const bool sp = S.surface_pipeline != 0;
  // the lean kernels serve the headline border and hit line; every sink has one for the pencil source and the explicit trace
  const bool lean = border == LAMBERT && !compat;
  const bool lean_explicit = lean && pencil && !chord;
  // assist-wave workgroups: the lobe / rough-specular kernels hold 87-93 VGPRs -- four waves per SIMD -- and hand over as often as
  // the lean one at a third of its pace: 512 threads, 7 tracer waves per assist wave and two workgroups per CU, unless assist_block
  // was set (measured 47.1 against 48.3 ms and 33.4 against 34.0 ms for 5e7 rays, profiles/r05_surface_shapes.json)
  const int ablock = (border != LAMBERT && !S.assist_block_set) ? 512 : S.assist_block;
  Plan p;

  // The flux pipeline's trace kernels without an assist wave serve the lean cases (pencil source, either trace mode; BRDF source,
  // explicit trace).  Those with one serve, unless surface_pipeline = 0, the origin-compat hit line as well (the assist wave writes
  // the line the binning kernel is to see) and, with the pencil source, the two other borders -- the chord identity is a property
  // of the Lambertian border, so trace_mode says nothing there.
  const bool flux_served = border == LAMBERT ? (!compat || (sp && S.assist)) && (pencil || !chord) : sp && S.assist && pencil;
  // the trace kernel of a flux-map or exit-map pipeline and its shape
  auto pipe_trace = [&](Route route) {
    p.route = route;
    const bool assist = S.assist != 0;
    if (border == LOBE) p.fn = isx_trace_assist_lobe_kernel;
    else if (border == ROUGH) p.fn = isx_trace_assist_rough_kernel;
    else if (!pencil) p.fn = assist ? isx_trace_assist_brdf_kernel : isx_trace_rec_brdf_kernel;
    else if (chord) p.fn = assist ? isx_trace_assist_chord_kernel : isx_trace_rec_chord_kernel;
    else p.fn = assist ? isx_trace_assist_kernel : isx_trace_rec_kernel;
    trace_shape(p, assist ? small_shape(std::min(n, S.pipe_chunk), ablock) : Shape{S.trace_block, 4}, assist,
                resident_unless(S.trace_blocks_per_cu));
  };
  // The beam source (isx_fluxmap_beam) has one route whatever the switches say: its assist-wave trace kernel (the call is refused
  // outside the explicit Lambertian lean path: check_beam_call), the source behind the rings, and isx_fluxmap's binning kernels
  // (bin_mode 0: the brute-force form of isx_bin_lines_kernel).
  // The baffles (isx_fluxmap_baffle) likewise: their assist-wave trace kernel (check_baffle_call), the table behind the rings.
  // The scene (isx_fluxmap_scene) likewise: its assist-wave trace kernel (check_scene_call), the three blocks behind the rings.
  if (sink == SINK_FLUX && (beam || baffle || (flux_served && S.pipeline && S.bin_mode != 0))) {
    if (scene) {
      p.route = ROUTE_FLUX_PIPE;
      p.fn = isx_trace_assist_scene_kernel;
      // (the kernel is built for five waves per SIMD: 640 threads -- nine tracer waves and the assist wave -- are what two
      //  workgroups of a CU may have, unless assist_block was set)
      trace_shape(p, small_shape(std::min(n, S.pipe_chunk), S.assist_block_set ? S.assist_block : kSceneBlock), true,
                  resident_unless(S.trace_blocks_per_cu));
      p.lds += SceneLds::bytes(p.tracers);
    } else if (beam) {
      p.route = ROUTE_FLUX_PIPE;
      p.fn = isx_trace_assist_beam_kernel;
      trace_shape(p, small_shape(std::min(n, S.pipe_chunk), S.assist_block), true, resident_unless(S.trace_blocks_per_cu));
      p.lds += beam_lds(p.tracers);
    } else if (baffle) {
      p.route = ROUTE_FLUX_PIPE;
      p.fn = isx_trace_assist_baffle_kernel;
      trace_shape(p, small_shape(std::min(n, S.pipe_chunk), S.assist_block), true, resident_unless(S.trace_blocks_per_cu));
      p.lds += kBaffleLds;
    } else
    pipe_trace(ROUTE_FLUX_PIPE);
    // The binning kernel keeps the histogram and the detector tables in LDS.  With slot queues (1024-thread workgroups: 61 KB of
    // queues next to the histogram) if the grid fits their 32-bit slot records and the LDS, and then with COLUMN slots (default
    // for every source since round 4: grazing lines are column slots as well -- prep_band; bin_cols = 0 keeps the row slots of
    // isx_bin_slots_kernel); else the one without.
    const size_t tables = hist_lds(d.nbins) + (size_t)(4 * d.n_theta) * 8 + (size_t)(2 * d.n_phi) * sizeof(ColX) + sizeof(DetGrid) + 16;
    const size_t slots_lds = tables + (size_t)(2 * d.n_phi) * sizeof(ColP) + (size_t)(kBlock / 64) * kSlotWaveWords * 4;
    const size_t cols_lds = tables + (size_t)(d.n_theta + 4) * sizeof(RowX) + (size_t)(kBlock / 64) * kColWaveWords * 4;
    const bool slots = S.bin_slots && d.bin_mode == 1 && d.n_theta <= 256 && d.n_phi <= 255 && slots_lds <= S.lds_limit;
    const bool cols = slots && S.bin_cols && cols_lds <= S.lds_limit;
    p.bin = cols ? isx_bin_cols_kernel : slots ? isx_bin_slots_kernel : isx_bin_lines_kernel;
    p.bblock = slots ? kBlock : S.bin_block;
    p.lds_bin = cols ? cols_lds : slots ? slots_lds : tables + (size_t)(p.bblock / 64) * 128 * 4;
    p.bin_per_cu = resident_unless(S.bin_blocks_per_cu);
    p.compat_lines = compat && d.bin_mode != 2;
    p.binning = d.bin_mode != 2;
    p.overlap = S.overlap > 1 && d.bin_mode == 1 && n >= (uint64_t)S.overlap * 65536;
    // call overlap: scheduling only.  Enqueued plain flux maps with explicit bounces (chord mode keeps the one stream it had: its
    // launch tails have not been measured); never together with `overlap` > 1, whatever the call's size
    p.call_overlap = g_device_call && S.call_overlap != 0 && S.overlap <= 1 && !chord && !beam && !baffle && !scene;
    // the fate scan in front of the headline trace kernel (fate_consts: pencil, Lambertian border, explicit bounces, first strike
    // on the mirror patch): scheduling only -- anything else takes the kernels above whatever the option says
    const bool fate_ok = !beam && fate && fate->ok && p.fn.fn == (const void*)isx_trace_assist_kernel && !p.overlap;
    // exit lines from the words behind the scan: the scan's eligibility, the last-segment hit line, the
    // column-slot binning kernel.  "exit_scan" 1 brings the scan with it (unless "fate_scan" is 0); -1 follows the scan's rule.
    const uint64_t w_exit = fate_ok ? (uint64_t)fate->w_leave + 2ull * kFateMarg + 2ull : ~0ull;
    const bool exit_ok = fate_ok && S.fate_scan != 0 && !compat && cols && p.binning && w_exit <= 0xffffffffull;
    const bool exit_on = exit_ok && (S.exit_scan == 1 || (S.exit_scan < 0 && fate_scan_auto(c, std::min(n, S.pipe_chunk))));
    if (fate_ok && (exit_on || S.fate_scan == 1 || (S.fate_scan < 0 && fate_scan_auto(c, std::min(n, S.pipe_chunk))))) {
      p.list = isx_trace_assist_list_kernel;
      p.fate = *fate;
      p.fate_auto = S.fate_scan < 0 && !(exit_on && S.exit_scan == 1);   // (the largest chunk passes the rule; a shorter last chunk is asked again)
      p.exit_lines = exit_on;
      p.w_exit = exit_on ? (uint32_t)w_exit : 0u;
    }
    if (p.lds_bin <= S.lds_limit || beam || baffle) return p;   // (beam, baffles: enqueue refuses a binning kernel whose LDS does not fit)
    p = Plan();   // (a binning kernel whose LDS does not fit: the fused kernel below)
  }

  // The exit maps take the trace kernels as they are -- every one of them stores last point + final direction, which is the line
  // the maps are defined on whatever hit_line_mode says (the rewrite kernel of the origin-compat line does not run here) -- and bin
  // with isx_bin_exitmaps_kernel: 1024-thread workgroups, the two u32 maps and the five counters in LDS, what is resident.
  const bool exit_served = border == LAMBERT ? (pencil || !chord) : sp && S.assist && pencil;
  if (sink == SINK_EXITMAP && exit_served && S.pipeline) {
    pipe_trace(ROUTE_EXIT_PIPE);
    p.bin = isx_bin_exitmaps_kernel;
    p.bblock = kBlock;
    p.lds_bin = hist_lds(d.nbins);
    if (p.lds_bin <= S.lds_limit) return p;
    p = Plan();
  }

  // The light field goes the same way wherever the exit maps do.  Its binning kernel has two forms (isx_kernels.hpp): a field of at
  // most kLightFieldLdsBins words is a u32 field in the workgroup's LDS; a larger one (or any, with lf_global = 1) takes one global
  // u64 add per binned line, and the LDS holds the four counters only.  The form is the block's size, nothing else.
  if (sink == SINK_LIGHTFIELD && exit_served && S.pipeline) {
    pipe_trace(ROUTE_FIELD_PIPE);
    p.bin = isx_bin_lightfield_kernel;
    p.bblock = kBlock;
    const long long field = (long long)d.xm_nu * d.xm_nv * d.xm_nx * d.xm_ny;
    const bool in_lds = !S.lf_global && field <= kLightFieldLdsBins && hist_lds((int)field + 4) <= S.lds_limit;
    p.bin_words = in_lds ? (int)field + 4 : 4;
    p.lds_bin = hist_lds(p.bin_words);
    return p;
  }

  // The disc pipeline's binning kernel keeps the histogram, the cluster table, the discs (up to kDiscsInLds) and per-wave lists in
  // LDS; above ~16 000 discs on gfx950 they do not fit, and the fused SINK_DISC kernel, which needs the histogram only, takes the sweep.
  const size_t disc_lds = hist_lds(d.nbins) + (size_t)g_disc_clusters.n_clusters * 16 +
                          (d.nbins <= kDiscsInLds ? (size_t)d.nbins * 48 + (size_t)((d.nbins + 1) & ~1) * 4 : 0) +
                          (size_t)(kDiscBinBlock / 64) * (64 * 7 + kPairCap / 2) * sizeof(double);
  if (sink == SINK_DISC && lean_explicit && S.pipeline && S.assist && S.disc_pipeline && g_disc_clusters.n == (size_t)d.nbins &&
      discs_in_aux && disc_lds <= S.lds_limit) {
    p.route = ROUTE_DISC_PIPE;
    p.fn = isx_trace_assist_disc_kernel;
    trace_shape(p, small_shape(std::min(n, S.pipe_chunk), ablock), true, kResident);
    p.bin = isx_bin_discs_kernel; p.bblock = kDiscBinBlock; p.lds_bin = disc_lds;
    p.slot_doubles = 8;   // (exit segments)
    return p;
  }

  // (round 5: the lobe / rough-specular borders as well -- SINK_PERPOS only, last-segment hit line: the assist wave's exact test
  //  takes the line as it is)
  const bool pp_surface = sink == SINK_PERPOS && sp && pencil && border != LAMBERT && !compat;
  if ((sink == SINK_PERPOS || sink == SINK_DISCPOS) && (lean_explicit || pp_surface) && S.pipeline && S.assist) {
    p.route = ROUTE_ASSIST;
    p.fn = sink == SINK_DISCPOS ? isx_trace_assist_discpos_kernel : border == LOBE ? isx_trace_assist_perpos_lobe_kernel :
           border == ROUGH ? isx_trace_assist_perpos_rough_kernel : isx_trace_assist_perpos_kernel;
    trace_shape(p, small_shape(std::min(n, kLaunchMax), ablock), true, resident_unless(S.trace_blocks_per_cu));
    return p;
  }

  // The wall map on the assist-wave kernels: every border with the pencil source, the Lambertian border with the BRDF source and
  // explicit bounces (what those kernels are built for; hit_line_mode plays no part).  The workgroup's u32 map lies behind the rings:
  // at the 8192-bin limit 72.6 KB per workgroup, two 768-thread workgroups per CU.  Should the device not hold two of them (the
  // occupancy query of the grid), the 512-thread shape takes the call.
  const bool wall_served = border == LAMBERT ? (pencil || !chord) : sp && pencil;
  if (sink == SINK_WALL && wall_served && S.pipeline && S.assist) {
    p.route = ROUTE_ASSIST;
    p.fn = border == LOBE ? isx_trace_assist_wall_lobe_kernel : border == ROUGH ? isx_trace_assist_wall_rough_kernel :
           !pencil ? isx_trace_assist_wall_brdf_kernel : chord ? isx_trace_assist_wall_chord_kernel : isx_trace_assist_wall_kernel;
    Shape sh = small_shape(std::min(n, kLaunchMax), ablock);
    trace_shape(p, sh, true, resident_unless(S.trace_blocks_per_cu));
    p.lds += hist_lds(d.nbins);
    if (sh.block > 512 && !S.assist_block_set && blocks_per_cu(p.fn.fn, sh.block, p.lds, kResident) < 2) {
      sh.block = 512;
      trace_shape(p, sh, true, resident_unless(S.trace_blocks_per_cu));
      p.lds += hist_lds(d.nbins);
    }
    return p;
  }

  // The bounce-order histograms go the wall map's way, with its kernels' shapes and its occupancy rule: the workgroup's u32 block
  // (at most 8192 words + the five counters) lies behind the rings.
  if (sink == SINK_ORDER && wall_served && S.pipeline && S.assist) {
    p.route = ROUTE_ASSIST;
    p.fn = border == LOBE ? isx_trace_assist_order_lobe_kernel : border == ROUGH ? isx_trace_assist_order_rough_kernel :
           !pencil ? isx_trace_assist_order_brdf_kernel : chord ? isx_trace_assist_order_chord_kernel : isx_trace_assist_order_kernel;
    Shape sh = small_shape(std::min(n, kLaunchMax), ablock);
    trace_shape(p, sh, true, resident_unless(S.trace_blocks_per_cu));
    p.lds += hist_lds(d.nbins);
    if (sh.block > 512 && !S.assist_block_set && blocks_per_cu(p.fn.fn, sh.block, p.lds, kResident) < 2) {
      sh.block = 512;
      trace_shape(p, sh, true, resident_unless(S.trace_blocks_per_cu));
      p.lds += hist_lds(d.nbins);
    }
    return p;
  }

  // The wall patches have one route whatever the switches say: the assist-wave kernel of the explicit Lambertian lean path (the
  // call is refused for anything else: check_patch_call) in the wall map's shapes, the table and the counters behind the rings.
  // Launches are cut at pipeline_chunk, which bounds what a workgroup's u32 counters can see.
  if (sink == SINK_PATCH) {
    p.route = ROUTE_ASSIST;
    p.fn = isx_trace_assist_patch_kernel;
    p.launch_max = std::min(kLaunchMax, S.pipe_chunk);
    trace_shape(p, small_shape(std::min(n, p.launch_max), S.assist_block), true, resident_unless(S.trace_blocks_per_cu));
    p.lds += patch_lds();
    return p;
  }

  // the fused kernel: the lean build where there is one, the full-featured one for everything else
  switch (sink) {
    case SINK_FLUX: p.fn = lean && pencil ? (chord ? isx_trace_bin_chord_kernel : isx_trace_bin_kernel) :
                           lean && !chord ? isx_trace_bin_brdf_kernel : isx_trace_bin_full_kernel; break;
    case SINK_DZ: p.fn = lean_explicit ? isx_trace_dz_lean_kernel : isx_trace_dz_kernel; break;
    case SINK_EXITMAP: p.fn = border == LAMBERT && pencil && !chord ? isx_trace_exitmap_lean_kernel : isx_trace_exitmap_kernel; break;
    case SINK_WALL: p.fn = border == LAMBERT && pencil && !chord ? isx_trace_wall_lean_kernel : isx_trace_wall_kernel; break;
    case SINK_LIGHTFIELD: p.fn = border == LAMBERT && pencil && !chord ? isx_trace_lightfield_lean_kernel : isx_trace_lightfield_kernel; break;
    case SINK_ORDER: p.fn = border == LAMBERT && pencil && !chord ? isx_trace_order_lean_kernel : isx_trace_order_kernel; break;
    case SINK_DISC: p.fn = lean_explicit ? isx_trace_disc_lean_kernel : isx_trace_disc_kernel; break;
    case SINK_PERPOS: p.fn = lean_explicit ? isx_trace_perpos_lean_kernel : isx_trace_perpos_kernel; break;
    case SINK_DISCPOS: p.fn = lean_explicit ? isx_trace_discpos_lean_kernel : isx_trace_discpos_kernel; break;
    default: p.fn = lean_explicit ? isx_trace_log_lean_kernel : isx_trace_log_kernel; break;
  }
  // Workgroup shape.  The kernels that keep the 64.8 KB LDS histogram run one 1024-thread workgroup per CU (4 waves per SIMD,
  // 128 VGPRs).  The lean trace-only kernels need 75-90 VGPRs and almost no LDS: as 512-thread workgroups (trace_block) they reach
  // 5-6 waves per SIMD (measured: 18.8 -> 17.5 ms for 5e7 rays, 299 -> 282 ms for the 8.1e8-ray per-position map), and their grid is
  // what is resident.
  const bool trace_only = lean_explicit && (sink == SINK_PERPOS || sink == SINK_DISCPOS || sink == SINK_DZ || sink == SINK_LOG);
  p.block = trace_only ? S.trace_block : kBlock;
  p.tracers = p.block / 64;
  p.lds = lds;
  p.per_cu = trace_only ? resident_unless(S.trace_blocks_per_cu) : 0;
  return p;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize): once per kernel and size, not once per launch
int set_lds(const void* fn, size_t bytes) {
  size_t& set = S.attr_lds[fn];
  if (set != bytes) {
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    set = bytes;
  }
  return ISX_OK;
}

// the Work of one launch: rays [wk.first + off, + cnt), a block of queue counters zeroed on `stream`
int launch_work(const Work& wk, uint64_t off, uint64_t cnt, uint32_t pad, hipStream_t stream, Work* w) {
  *w = wk;
  w->first = wk.first + off; w->n = cnt; w->sub = pick_sub(cnt); w->pad = pad;
  return next_ctr(stream, &w->ctr);
}

// Events: mark() records a pooled event on `stream` (*at: its index in S.ev_pool); span() records one on S.stream that ends the
// kernel of `kind` begun at mark *from (kind 0: a whole call, 1: a pipeline's trace kernel, 2: its binning kernel) and moves *from
// on to it, so that consecutive kernels chain.
int mark(hipStream_t stream, size_t* at) {
  if (S.ev_used == S.ev_pool.size()) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    S.ev_pool.push_back(e);
  }
  *at = S.ev_used++;
  return hip_rc(hipEventRecord(S.ev_pool[*at], stream));
}
int span_on(hipStream_t stream, int kind, size_t* from) {   // (... on the stream that holds the kernel and mark *from)
  const size_t a = *from;
  const int rc = mark(stream, from);
  if (rc == ISX_OK) S.spans.push_back({a, *from, kind});
  return rc;
}
int span(int kind, size_t* from) { return span_on(S.stream, kind, from); }

// ROUTE_FUSED and ROUTE_ASSIST: launches of at most kLaunchMax rays, one span
int run_single(const Plan& p, const Geom& g, const DetGrid& d, const Work& wk) {
  int rc = set_lds(p.fn.fn, p.lds); if (rc) return rc;
  const int per_cu = blocks_per_cu(p.fn.fn, p.block, p.lds, p.per_cu);
  const uint64_t launch_max = p.launch_max ? p.launch_max : kLaunchMax;
  size_t t;
  rc = mark(S.stream, &t); if (rc) return rc;
  for (uint64_t off = 0; off < wk.n; off += launch_max) {
    Work w;
    rc = launch_work(wk, off, std::min(wk.n - off, launch_max), 0, S.stream, &w); if (rc) return rc;
    launch_trace(p, p.fn, pick_grid(p, w.n, per_cu), S.stream, g, d, w);
    HIPCHK(hipGetLastError());
  }
  return span(0, &t);
}

// workspace `buf` of the two-kernel pipeline with room for `regions` regions of kRegion 6-double slots and their line counts
int ensure_regions(size_t regions, int buf) {
  if (regions > S.cap_regions[buf]) {
    if (sync_all()) return ISX_ERR_HIP;
    if (S.d_rec[buf]) HIPCHK(hipFree(S.d_rec[buf]));
    if (S.d_rec_counts[buf]) HIPCHK(hipFree(S.d_rec_counts[buf]));
    S.d_rec[buf] = nullptr; S.d_rec_counts[buf] = nullptr; S.cap_regions[buf] = 0;
    HIPCHK(hipMalloc(&S.d_rec[buf], regions * kRegion * 6 * sizeof(double)));
    HIPCHK(hipMalloc(&S.d_rec_counts[buf], regions * sizeof(uint32_t)));
    S.cap_regions[buf] = regions;
  }
  return ISX_OK;
}
// ... for a chunk of `rays` rays traced by `waves` waves: every region but a wave's last is closed with more than kRegion - 64
// lines in it, and a launch cannot have more lines than rays (isx_kernels.hpp: kRegion)
// list: ... and the fate scan's ray list, 4 B per ray of the largest chunk so far (grown, never shrunk)
// exit_waves > 0: ... and what isx_exit_lines_kernel needs: the list as {offset, j} pairs, list B, a side
// entry per line slot, the redo list; its waves leave an open region each, as the trace kernel's writers do
constexpr size_t kRedoMin = 1u << 22;   // entries: what a test-sized chunk can send with its bounds scaled up (exit_eps_scale)
int ensure_pipeline(size_t rays, size_t waves, int buf, size_t slot_doubles, bool list = false, size_t exit_waves = 0) {
  const bool pairs = exit_waves > 0;
  if (list && (rays > S.cap_list[buf] || (pairs && !S.list_pairs[buf]))) {
    if (sync_all()) return ISX_ERR_HIP;
    if (S.d_list[buf]) HIPCHK(hipFree(S.d_list[buf]));
    const size_t cap = std::max(rays, S.cap_list[buf]);
    const bool wide = pairs || S.list_pairs[buf];
    S.d_list[buf] = nullptr; S.cap_list[buf] = 0; S.list_pairs[buf] = false;
    HIPCHK(hipMalloc(&S.d_list[buf], cap * sizeof(uint32_t) * (wide ? 2 : 1)));
    S.cap_list[buf] = cap; S.list_pairs[buf] = wide;
  }
  const size_t regions = (rays / (kRegion - 63) + waves + exit_waves + 1) * slot_doubles / 6 + 1;   // (capacity is counted in 6-double slots)
  int rc = ensure_regions(regions, buf);
  if (rc || !pairs) return rc;
  if (rays > S.cap_exit_rays[buf]) {
    if (sync_all()) return ISX_ERR_HIP;
    if (S.d_list_b[buf]) HIPCHK(hipFree(S.d_list_b[buf]));
    S.d_list_b[buf] = nullptr; S.cap_exit_rays[buf] = 0;
    HIPCHK(hipMalloc(&S.d_list_b[buf], rays * sizeof(uint32_t)));
    S.cap_exit_rays[buf] = rays;
  }
  if (S.cap_regions[buf] > S.cap_side[buf]) {
    if (sync_all()) return ISX_ERR_HIP;
    if (S.d_side[buf]) HIPCHK(hipFree(S.d_side[buf]));
    S.d_side[buf] = nullptr; S.cap_side[buf] = 0;
    HIPCHK(hipMalloc(&S.d_side[buf], S.cap_regions[buf] * kRegion * sizeof(uint2)));
    S.cap_side[buf] = S.cap_regions[buf];
  }
  const size_t redo = std::max(kRedoMin, rays / 4);
  if (redo > S.cap_redo[buf]) {
    if (sync_all()) return ISX_ERR_HIP;
    if (S.d_redo[buf]) HIPCHK(hipFree(S.d_redo[buf]));
    S.d_redo[buf] = nullptr; S.cap_redo[buf] = 0;
    HIPCHK(hipMalloc(&S.d_redo[buf], (redo + 2) * sizeof(unsigned long long)));
    S.cap_redo[buf] = redo;
  }
  if (!S.d_exit_totals) {
    HIPCHK(hipMalloc(&S.d_exit_totals, 3 * sizeof(unsigned long long)));
    HIPCHK(hipMemset(S.d_exit_totals, 0, 3 * sizeof(unsigned long long)));
  }
  return ISX_OK;
}

// what the disc sweep's two kernels see of the list upload_discs_clustered left in the aux buffer: the discs in cluster order
void clustered_discs(DetGrid& d) {
  d.discs = S.d_aux + g_disc_clusters.off_ordered;
  d.clusters = reinterpret_cast<const float*>(S.d_aux + g_disc_clusters.off_clusters);
  d.disc_perm = reinterpret_cast<const int*>(S.d_aux + g_disc_clusters.off_perm);
  d.n_clusters = g_disc_clusters.n_clusters;
}

// ROUTE_FLUX_PIPE, ROUTE_EXIT_PIPE, ROUTE_FIELD_PIPE and ROUTE_DISC_PIPE: a trace launch and a binning launch per chunk of at most pipe_chunk rays
int run_pipeline(const Plan& p, const Geom& g, const DetGrid& d, const Work& wk) {
  // (behind the fate scan the list kernel sizes the grid; a chunk below the automatic rule's size still takes p.fn)
  const TraceKernel& lead = p.list.fn ? p.list : p.fn;
  int rc = set_lds(lead.fn, p.lds);
  if (rc == ISX_OK && p.list.fn) rc = set_lds(p.fn.fn, p.lds);
  if (rc == ISX_OK) rc = set_lds((const void*)p.bin, p.lds_bin);
  if (rc) return rc;
  const int tres = blocks_per_cu(lead.fn, p.block, p.lds, p.per_cu);
  const int bres = blocks_per_cu((const void*)p.bin, p.bblock, p.lds_bin, p.bin_per_cu);
  // what the two kernels see: a flux map's trace kernel keeps no histogram; the disc sweep's kernels walk the discs in cluster order
  DetGrid dt = d, db = d;
  if (p.route != ROUTE_DISC_PIPE) {
    dt.nbins = 1; dt.n_theta = 0; dt.n_phi = 0;
    if (p.route == ROUTE_FIELD_PIPE) db.nbins = p.bin_words;
  } else {
    clustered_discs(db);
    dt = db;
  }
  // one trace launch on `st` and the binning of its `cnt` rays from `off` on `sb`, through workspace `buf`.  t: one stream, each
  // kernel a span of its own from mark *t on; nullptr: an event hands the exit records over from st to sb.  split (call overlap):
  // both -- *t is a mark on st, the trace span and isx_compat_lines_kernel lie on st, the event that ends them hands over to sb, and
  // the binning span lies on sb behind it
  auto launch_pair = [&](uint64_t off, uint64_t cnt, int buf, hipStream_t st, hipStream_t sb, size_t* t, bool split) -> int {
    if (cnt > kLaunchMax) return ISX_ERR_TOO_LARGE;   // (cannot happen: pipeline_chunk <= 2^26)
    // (work units of the binning kernel: quarter regions of 256 exit lines; sixteenths -- 64 lines, one batch -- for a small
    //  launch, whose few thousand lines then spread over as many waves as there are batches)
    Work w;
    int r = launch_work(wk, off, cnt, cnt < 1000000ull ? 2u : 0u, st, &w); if (r) return r;
    dt.rec_lines = db.rec_lines = S.d_rec[buf];
    dt.rec_counts = db.rec_counts = S.d_rec_counts[buf];
    const int tgrid = pick_grid(p, cnt, tres);
    const bool scan = p.list.fn && (!p.fate_auto || cnt >= kFateMinRays);
    const bool exitl = scan && p.exit_lines;
    const int egrid = exitl ? exit_grid(cnt) : 0;
    const FateList fl{exitl ? S.d_list_b[buf] : S.d_list[buf], w.ctr + (exitl ? Q_LISTB : Q_LIST)};
    db.log_rec = exitl ? reinterpret_cast<double*>(S.d_side[buf]) : nullptr;
    db.log_count = exitl ? S.d_redo[buf] : nullptr;
    db.log_cap = exitl ? (uint64_t)S.cap_redo[buf] : 0;
    if (scan) {
      // the scan settles what the wall absorbs and leaves the rest in S.d_list, their number in ctr[Q_LIST] (zeroed with the
      // launch's other counters); the trace kernel's grid is sized from the chunk, an upper bound.  Same stream, no host round
      // trip; both kernels lie in the trace span.
      FateScan fs;
      fs.f = p.fate; fs.seed = w.seed; fs.first = w.first; fs.n = (uint32_t)cnt; fs.pairs = exitl ? 1u : 0u;
      fs.list = S.d_list[buf]; fs.ctr = w.ctr; fs.stats = w.stats;
      const uint64_t want = (cnt + 4ull * kScanBlock - 1) / (4ull * kScanBlock), full = (uint64_t)S.cu_count * 8ull;
      const int sgrid = S.grid_blocks > 0 ? S.grid_blocks : (int)std::max<uint64_t>(1, std::min(want, full));
      hipLaunchKernelGGL(isx_fate_scan_kernel, dim3(sgrid), dim3(kScanBlock), 0, st, fs);
      HIPCHK(hipGetLastError());
      ++S.fate_launches;
    }
    if (exitl) {
      // the clean port exits among them are settled from their words; list B is what the trace kernel takes.  Same stream, inside
      // the trace span.
      ExitScan es;
      es.g = g; es.seed = w.seed; es.first = w.first;
      es.list_a = reinterpret_cast<const uint2*>(S.d_list[buf]); es.list_b = S.d_list_b[buf]; es.ctr = w.ctr; es.stats = w.stats;
      es.totals = S.d_exit_totals; es.rec_lines = S.d_rec[buf]; es.rec_counts = S.d_rec_counts[buf]; es.side = S.d_side[buf];
      es.redo = S.d_redo[buf];
      es.rho_thr = p.fate.rho_thr; es.never = p.fate.never; es.w_exit = p.w_exit; es.j_cap = p.fate.j_cap; es.limit = p.fate.limit; es.pad = 0;
      es.reach = 2.1 * (1.001 * g.r_in + std::fabs(d.portz) + d.R + d.rho_d);
      es.portz = d.portz; es.det_R = d.R; es.half_w2 = d.half_w2; es.eps_scale = (double)S.exit_eps_scale;
      hipLaunchKernelGGL(isx_exit_lines_kernel, dim3(egrid), dim3(kExitBlock), 0, st, es);
      HIPCHK(hipGetLastError());
    }
    launch_trace(p, scan ? p.list : p.fn, tgrid, st, g, dt, w, &fl);
    HIPCHK(hipGetLastError());
    size_t traced;
    if (t) r = span_on(st, 1, t);
    else if ((r = mark(st, &traced)) == ISX_OK) r = hip_rc(hipStreamWaitEvent(sb, S.ev_pool[traced], 0));
    if (r) return r;
    if (p.compat_lines) {   // ISX_HITLINE_ORIGIN_COMPAT: the lines the binning kernel is to see (isx_compat_lines_kernel)
      hipLaunchKernelGGL(isx_compat_lines_kernel, dim3(S.cu_count * 8), dim3(256), 0, split ? st : sb, S.d_rec[buf], S.d_rec_counts[buf], w.ctr);
      HIPCHK(hipGetLastError());
      if (split && (r = span_on(st, 2, t))) return r;
    }
    if (split) {
      HIPCHK(hipStreamWaitEvent(sb, S.ev_pool[*t], 0));
      if (p.binning && (r = mark(sb, t))) return r;
    }
    if (p.binning) {
      // (every writing wave of the trace kernel leaves an open region: one per workgroup with an assist wave)
      const uint64_t writers = (p.assist ? (uint64_t)tgrid : (uint64_t)tgrid * (uint64_t)(p.block / 64)) + (uint64_t)egrid * (kExitBlock / 64);
      hipLaunchKernelGGL(p.bin, dim3(bin_grid(p, cnt, w.pad, writers, bres)), dim3(p.bblock), p.lds_bin, sb, db, w);
      HIPCHK(hipGetLastError());
      if (exitl) {   // what the binning kernel would not decide on an approximate line: the ray traced, the reference's test (inside the binning span)
        hipLaunchKernelGGL(isx_redo_kernel, dim3(S.grid_blocks > 0 ? S.grid_blocks : 64), dim3(256), 0, sb, g, db, w, S.d_exit_totals);
        HIPCHK(hipGetLastError());
      }
      if (t && (r = span_on(sb, 2, t))) return r;
    }
    return ISX_OK;
  };
  const uint64_t n = wk.n;
  if (p.overlap) {
    // ---- overlapped: chunk k is binned on the second stream while chunk k+1 is traced on the first (overlap_trace_streams = 2:
    // odd chunks on a third); chunk k+3 reuses the workspace of chunk k.  (Timing: one wall-clock span around everything; the
    // kernels' own times overlap.)
    if (!S.stream2) HIPCHK(hipStreamCreateWithFlags(&S.stream2, hipStreamNonBlocking));
    if (!S.stream3) HIPCHK(hipStreamCreateWithFlags(&S.stream3, hipStreamNonBlocking));
    const uint64_t per = ((n + (uint64_t)S.overlap - 1) / (uint64_t)S.overlap + 63) & ~63ull;
    const uint64_t chunk = std::min(per, S.pipe_chunk);
    const size_t waves = (size_t)pick_grid(p, chunk, tres) * (p.block / 64);
    for (int b = 0; b < State::kRecBufs && rc == ISX_OK; ++b) rc = ensure_pipeline((size_t)chunk, waves, b, p.slot_doubles);
    size_t t0, t1;
    if (rc == ISX_OK) rc = mark(S.stream, &t0);
    if (rc) return rc;
    HIPCHK(hipStreamWaitEvent(S.stream3, S.ev_pool[t0], 0));   // (what the caller enqueued before this call comes first)
    size_t binned[State::kRecBufs];                            // [k mod kRecBufs]: chunk k is binned, its workspace free
    int k = 0;
    for (uint64_t off = 0; off < n; off += chunk, ++k) {
      const int buf = k % State::kRecBufs;
      const hipStream_t st = (S.overlap_trace_streams == 2 && (k & 1)) ? S.stream3 : S.stream;
      if (k >= State::kRecBufs) HIPCHK(hipStreamWaitEvent(st, S.ev_pool[binned[buf]], 0));
      rc = launch_pair(off, std::min(n - off, chunk), buf, st, S.stream2, nullptr, false);
      if (rc == ISX_OK) rc = mark(S.stream2, &binned[buf]);
      if (rc) return rc;
    }
    HIPCHK(hipStreamWaitEvent(S.stream, S.ev_pool[binned[(k - 1) % State::kRecBufs]], 0));   // the caller's stream sees the finished histogram
    rc = mark(S.stream, &t1); if (rc) return rc;
    S.spans.push_back({t0, t1, 0});
    return ISX_OK;
  }
  const uint64_t chunk = std::min(n, S.pipe_chunk);
  const size_t exit_waves = p.exit_lines ? (size_t)exit_grid(chunk) * (kExitBlock / 64) : 0;   // (the largest chunk's: its grid is the largest)
  if (p.call_overlap) {
    // ---- call overlap: the chunk's counter zeroing, scan, trace (and compat lines) on a trace stream, its binning kernel on the
    // caller's stream behind the event that ends them.  The trace stream does not wait for the binning of the chunk before --
    // the caller's histogram is the binning kernel's alone -- so the scan and trace of the next chunk, of this call or the
    // next, run under the tails of this one's kernels.  All kRecBufs workspaces are sized at once: a workspace that grew in the
    // middle of a sequence would stop it.
    const size_t waves = (size_t)pick_grid(p, chunk, tres) * (p.block / 64);
    for (int b = 0; b < State::kRecBufs && rc == ISX_OK; ++b) rc = ensure_pipeline((size_t)chunk, waves, b, p.slot_doubles, p.list.fn != nullptr, exit_waves);
    if (rc == ISX_OK) rc = trace_begin();
    for (uint64_t off = 0; off < n && rc == ISX_OK; off += chunk, ++S.call_rot) {
      const int buf = (int)(S.call_rot % State::kRecBufs);
      const hipStream_t st = (S.call_overlap_streams == 2 && (S.call_rot & 1)) ? S.stream3 : S.stream2;
      if (S.free_set[buf]) HIPCHK(hipStreamWaitEvent(st, S.ev_free[buf], 0));
      size_t t;
      rc = mark(st, &t);
      if (rc == ISX_OK) rc = launch_pair(off, std::min(n - off, chunk), buf, st, S.stream, &t, true);
      if (rc == ISX_OK) rc = pooled_event(&S.ev_free[buf]);
      if (rc) return rc;
      HIPCHK(hipEventRecord(S.ev_free[buf], p.binning ? S.stream : st));   // (behind the last kernel that reads the workspace)
      S.free_set[buf] = true;
    }
    return rc;
  }
  rc = ensure_pipeline((size_t)chunk, (size_t)pick_grid(p, chunk, tres) * (p.block / 64), 0, p.slot_doubles, p.list.fn != nullptr, exit_waves); if (rc) return rc;
  size_t t;
  rc = mark(S.stream, &t);
  for (uint64_t off = 0; off < n && rc == ISX_OK; off += chunk)
    rc = launch_pair(off, std::min(n - off, chunk), 0, S.stream, S.stream, &t, false);
  return rc;
}

// enqueue one call's launches, accumulating into k.d_hist (device) and S.d_stats (or k.d_stats)
int enqueue(const Call& call) {
  Call k = call;   // (the scene's parts and the beam's configuration are filled in below)
  Geom g;
  FateConsts fate;
  isx_config cb;
  // (a scene is its beam, its baffles -- whose counters are the last 16 of the scene's 36 -- and its patches)
  BaffleSink sc_bf;
  const SceneSink* sc = k.sc;
  if (sc) { k.bs = &sc->spec->beam; sc_bf.spec = &sc->spec->baffles; sc_bf.counts = sc->counts + 2 * (kMaxPatches + 2); k.bf = &sc_bf; }
  if (k.bs && config_abi_ok(k.c) && k.bs->struct_size == (uint32_t)sizeof(isx_beam_spec)) { cb = beam_config(*k.c, *k.bs); k.c = &cb; }
  int rc = prepare_geom(k.c, &g, &fate);
  if (rc) return rc;
  if (k.n > ISX_MAX_RAYS_PER_CALL) return ISX_ERR_TOO_LARGE;
  if (k.first > UINT64_MAX - k.n) return ISX_ERR_BAD_ARG;   // first + n (the exclusive end of the index range) must be representable
  DetGrid d;
  size_t lds = 0;
  rc = sink_grid(k, d, lds);
  if (rc == ISX_OK && k.bf) {
    rc = check_baffle_call(k.c, k.bf->spec);
    if (S.bin_mode == 2) d.bin_mode = 1;   // (isx.h: the trace-only diagnostic does not apply to the baffles)
  }
  if (rc == ISX_OK && sc) {
    rc = check_patch_call(k.c, &sc->spec->patches);
    // (the patches travel in the exit maps' words of DetGrid, as SINK_PATCH's do: a flux map's trace kernel has no other use for them)
    d.xm_nx = sc->spec->patches.n_patches;
    d.xm_dir = sc->counts; d.xm_pos = sc->counts + (kMaxPatches + 2);
  }
  if (rc || k.n == 0) return rc;
  Work wk;
  wk.seed = k.seed; wk.first = k.first; wk.n = k.n; wk.hist = k.d_hist; wk.stats = k.d_stats ? k.d_stats : S.d_stats;
  wk.ctr = nullptr; wk.sub = 0; wk.pad = 0;
  Plan p = plan_launch(k, d, lds, &fate);
  if (k.bf) {
    if (p.lds_bin > S.lds_limit) return ISX_ERR_BAD_CONFIG;   // (isx.h: a grid whose tables do not fit the binning kernels' LDS)
    p.baffles = baffle_table(*k.c, *k.bf->spec, k.bf->counts);
  }
  if (k.sink == SINK_PATCH) p.patch_tab = patch_table(*k.c, *k.wp->spec);
  if (sc) p.patch_tab = patch_table(*k.c, sc->spec->patches);
  if (k.bs) {
    if (p.lds_bin > S.lds_limit) return ISX_ERR_BAD_CONFIG;   // (isx.h: a grid whose tables do not fit the binning kernels' LDS)
    p.beam = beam_source(*k.bs);
  }
  if (!p.call_overlap && (rc = trace_join())) return rc;   // (anything else runs on the caller's stream, behind all of an overlapped sequence)
  return p.route == ROUTE_FUSED || p.route == ROUTE_ASSIST ? run_single(p, g, d, wk) : run_pipeline(p, g, d, wk);
}

// device copy of a caller's detector / disc list in the pooled buffer (no hipMalloc/hipFree per call)
int upload_aux(const double* host, size_t n_doubles) {
  if (trace_join()) return ISX_ERR_HIP;
  if (n_doubles > S.cap_aux) {
    HIPCHK(hipStreamSynchronize(S.stream));
    if (S.d_aux) HIPCHK(hipFree(S.d_aux));
    S.d_aux = nullptr; S.cap_aux = 0;
    const size_t cap = n_doubles < 4096 ? 4096 : n_doubles;
    HIPCHK(hipMalloc(&S.d_aux, cap * sizeof(double)));
    S.cap_aux = cap;
  }
  if (n_doubles * sizeof(double) <= 4096 && ensure_pin(1u << 17) == ISX_OK) {
    // a short list (traceRays' one detector): through the far end of the pinned staging buffer -- the copy engine reads it when the
    // stream gets there, the caller's `host` is free at once, and nothing waits (S.pending: the call ends through collect_stats, or
    // else the next call's opening one synchronises before anything writes the slot again)
    unsigned char* slot = S.h_pin + S.cap_pin - 4096;
    std::memcpy(slot, host, n_doubles * sizeof(double));
    HIPCHK(hipMemcpyAsync(S.d_aux, slot, n_doubles * sizeof(double), hipMemcpyHostToDevice, S.stream));
    S.pending = true;
    return ISX_OK;
  }
  HIPCHK(hipMemcpyAsync(S.d_aux, host, n_doubles * sizeof(double), hipMemcpyHostToDevice, S.stream));
  HIPCHK(hipStreamSynchronize(S.stream));   // `host` may be a temporary of the caller
  return ISX_OK;
}

// The disc list of isx_disc_sweep for isx_bin_discs_kernel: the discs in spatial (Morton) order, eight to a cluster, with the ball
// that holds the bounding balls of a cluster's discs.  Device layout behind the caller's own list (6 n doubles) in the pooled
// aux buffer: ordered discs (6 n doubles) | clusters (4 floats each) | permutation (n ints).

int upload_discs_clustered(const double* ca, size_t n, double radius, double half_thick) {
  g_disc_clusters = DiscClusters();
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (size_t k = 0; k < n; ++k)
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], ca[6 * k + a]); hi[a] = std::max(hi[a], ca[6 * k + a]); }
  std::vector<std::pair<uint32_t, int>> order(n);
  for (size_t k = 0; k < n; ++k) {
    uint32_t code = 0;
    for (int a = 0; a < 3; ++a) {
      const double span = hi[a] - lo[a];
      uint32_t q = span > 0 ? (uint32_t)std::min(1023.0, std::floor((ca[6 * k + a] - lo[a]) / span * 1024.0)) : 0u;
      for (int bit = 0; bit < 10; ++bit) code |= ((q >> bit) & 1u) << (3 * bit + a);   // Morton interleave
    }
    order[k] = {code, (int)k};
  }
  std::stable_sort(order.begin(), order.end());
  const size_t ncl = (n + 7) / 8;
  std::vector<double> ordered(6 * n);
  std::vector<float> clusters(4 * ncl);
  std::vector<int> perm(n);
  const double ball = std::sqrt(radius * radius + half_thick * half_thick);
  for (size_t j = 0; j < n; ++j) {
    perm[j] = order[j].second;
    std::memcpy(&ordered[6 * j], ca + 6 * (size_t)perm[j], 6 * sizeof(double));
  }
  for (size_t c = 0; c < ncl; ++c) {
    const size_t j0 = 8 * c, j1 = std::min(n, j0 + 8);
    double ctr[3] = {0, 0, 0};
    for (size_t j = j0; j < j1; ++j)
      for (int a = 0; a < 3; ++a) ctr[a] += ordered[6 * j + a] / (double)(j1 - j0);
    float cf[3] = {(float)ctr[0], (float)ctr[1], (float)ctr[2]};
    double r = 0;
    for (size_t j = j0; j < j1; ++j) {   // against the ROUNDED centre the kernel will use
      const double dx = ordered[6 * j] - (double)cf[0], dy = ordered[6 * j + 1] - (double)cf[1], dz = ordered[6 * j + 2] - (double)cf[2];
      r = std::max(r, std::sqrt(dx * dx + dy * dy + dz * dz));
    }
    clusters[4 * c + 0] = cf[0]; clusters[4 * c + 1] = cf[1]; clusters[4 * c + 2] = cf[2];
    clusters[4 * c + 3] = std::nextafter((float)((r + ball) * (1.0 + 1e-6)), INFINITY);
  }
  const size_t off_ordered = 6 * n, off_clusters = 12 * n, off_perm = off_clusters + 2 * ncl;
  const size_t total = off_perm + (n + 1) / 2 + 1;
  std::vector<double> blob(total, 0.0);
  std::memcpy(blob.data(), ca, 6 * n * sizeof(double));
  std::memcpy(blob.data() + off_ordered, ordered.data(), 6 * n * sizeof(double));
  std::memcpy(blob.data() + off_clusters, clusters.data(), clusters.size() * sizeof(float));
  std::memcpy(blob.data() + off_perm, perm.data(), n * sizeof(int));
  const int rc = upload_aux(blob.data(), total);
  if (rc) return rc;
  g_disc_clusters.n = n; g_disc_clusters.off_ordered = off_ordered; g_disc_clusters.off_clusters = off_clusters;
  g_disc_clusters.off_perm = off_perm; g_disc_clusters.n_clusters = (int)ncl;
  return ISX_OK;
}

int ensure_hist(size_t nb) {
  if (nb > S.cap_hist) {
    HIPCHK(hipStreamSynchronize(S.stream));
    if (S.d_hist) HIPCHK(hipFree(S.d_hist));
    HIPCHK(hipMalloc(&S.d_hist, nb * sizeof(unsigned long long)));
    S.cap_hist = nb;
  }
  return ISX_OK;
}

int collect_stats(isx_stats* out) {
  // the census through the pinned staging buffer: copy and re-zero enqueued, ONE synchronisation (it also covers a result staged
  // by stage_result()); a call that finds nothing enqueued since the last collection has nothing to wait for
  // (call overlap: the caller's stream is joined behind the trace streams first -- their kernels add to the same census words, and
  //  the words are zeroed behind both)
  if (trace_join()) return ISX_ERR_HIP;
  if (!S.pending && S.spans.empty() && !out) return ISX_OK;
  int rcp = ensure_pin(0);
  if (rcp) return rcp;
  HIPCHK(hipMemcpyAsync(S.h_pin, S.d_stats, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemsetAsync(S.d_stats, 0, 8 * sizeof(unsigned long long), S.stream));   // (ahead of whatever this stream launches next)
  HIPCHK(hipStreamSynchronize(S.stream));
  S.pending = false;
  double ms = 0;
  S.last_ms[0] = S.last_ms[1] = S.last_ms[2] = 0;
  for (const State::Span& sp : S.spans) {
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, S.ev_pool[sp.a], S.ev_pool[sp.b]));
    ms += t;
    S.last_ms[sp.kind] += t;
  }
  S.spans.clear();
  S.ev_used = 0;
  unsigned long long h[8];
  std::memcpy(h, S.h_pin, sizeof(h));
  // stats[7]: a wave of an assist-wave trace kernel gave up a bounded wait (its results are incomplete): never seen, never silent
  if (h[7] != 0) { S.last_hip = (int)hipErrorLaunchFailure; return ISX_ERR_HIP; }
  if (out) {
    out->launched = h[0]; out->exited = h[1]; out->counted_below_z = h[2]; out->absorbed = h[3];
    out->suspended = h[4]; out->bin_increments = h[5]; out->wall_hits = h[6];
    out->t_kernel_ms = ms;
  }
  return ISX_OK;
}

// The lifecycle of every blocking call.  call_open(): room for its histogram (`bins` words), after collecting the census of
// anything enqueued earlier so that it does not leak into this call.  Once call_open() has succeeded the call ends through
// call_close(), on success and on failure alike: the census, with the call's one synchronisation, which also completes its
// uploads, launches and result copies -- nothing of a failed call is left in flight.  The first error is the call's.
int call_open(size_t bins) {
  const int rc = ensure_hist(bins);
  return rc ? rc : collect_stats(nullptr);
}
int zero_hist(size_t bins) { return hip_rc(hipMemsetAsync(S.d_hist, 0, bins * sizeof(unsigned long long), S.stream)); }
int call_close(int rc, isx_stats* stats) { const int rc2 = collect_stats(stats); return rc ? rc : rc2; }
// what an entry point answers before isx_init(): ISX_ERR_NO_DEVICE where no HIP device is to be had, else ISX_ERR_NOT_INIT
int not_initialised() {
  int count = 0;
  return (hipGetDeviceCount(&count) != hipSuccess || count <= 0) ? ISX_ERR_NO_DEVICE : ISX_ERR_NOT_INIT;
}

// The body of the ten scene-map entries.  `k`: the call without its sinks; `m`: the map with the caller's arrays -- device
// arrays for a _device entry, which enqueues and returns; else host arrays (the map's own counters and `scene_counts` may be
// NULL), filled from one device block, one staged result: the map and, behind it, its own counters and the 36 scene counters.
// (What needs no device is answered first: a NULL argument or a refused spec is the same answer with and without one.  isx.h: the
// detector grid is ignored -- isx_scene_endstates' refusals.)
int scene_map_call(Call k, const isx_scene_spec* scene, SceneMap m, uint64_t* scene_counts, bool device, isx_stats* stats) {
  if (!k.c || !scene || !m.spec || !m.out) return ISX_ERR_BAD_ARG;
  if (device && ((m.sink != SINK_RESPONSE && !m.tail) || !scene_counts)) return ISX_ERR_BAD_ARG;
  size_t nb = 0, nt = 0;
  const size_t nc = kSceneWords;
  int rc = check_scene_call(k.c, scene, false);
  if (rc == ISX_OK) rc = scene_map_shape(m, scene->patches.n_patches, nb, nt);
  if (rc) return rc;
  if (!S.init) return not_initialised();
  SceneSink sc{scene, (unsigned long long*)scene_counts};
  k.sc = &sc; k.map = &m;
  if (device) return enqueue(k);
  unsigned long long *body = m.out, *tail = m.tail;
  const size_t bytes = (nb + nt + nc) * sizeof(unsigned long long);
  rc = call_open(nb + nt + nc);
  if (rc) return rc;
  rc = zero_hist(nb + nt + nc);
  m.out = S.d_hist; m.tail = S.d_hist + nb; sc.counts = S.d_hist + nb + nt;
  if (rc == ISX_OK) rc = enqueue(k);
  if (rc == ISX_OK) rc = stage_result(S.d_hist, bytes);
  rc = call_close(rc, stats);
  if (rc == ISX_OK) {
    fetch_result(body, nb * sizeof(unsigned long long));
    const unsigned long long* h = reinterpret_cast<const unsigned long long*>(S.h_pin + 64) + nb;
    if (tail) std::memcpy(tail, h, nt * sizeof(unsigned long long));
    if (scene_counts) std::memcpy(scene_counts, h + nt, nc * sizeof(unsigned long long));
  }
  return rc;
}

// isx_bin_injected_lines / isx_bin_injected_segments: the binning kernel of plan `p` on `n` caller-supplied records laid out as
// `counts` says (one entry per region), through the pipeline's own workspace, queue words and launch helpers -- what
// run_pipeline's launch_pair does after its trace kernel, with the host in the trace kernel's place.  `slot`: doubles per slot of
// the workspace -- 6: exit lines, the caller's rows as they are; 8: exit segments (isx_trace_assist_disc_kernel), the caller's rows
// of 7 doubles and a zero.  The slots of a region that hold no record carry `loud` (a whole slot).
int run_injected(const Plan& p, const DetGrid& d, const double* lines, uint64_t n, const std::vector<uint32_t>& counts,
                 uint32_t pad, const double* loud, size_t slot = 6) {
  const size_t regions = counts.size();
  const size_t row = slot == 8 ? 7 : slot;   // doubles per record of the caller
  int rc = set_lds((const void*)p.bin, p.lds_bin); if (rc) return rc;
  const int bres = blocks_per_cu((const void*)p.bin, p.bblock, p.lds_bin, p.bin_per_cu);
  rc = ensure_regions(slot == 6 ? regions + 1 : (regions + 1) * slot / 6 + 1, 0); if (rc) return rc;   // (capacity is counted in 6-double slots)
  std::vector<double> rec(regions * (size_t)kRegion * slot);
  for (size_t s = 0; s < rec.size(); s += slot) std::memcpy(&rec[s], loud, slot * sizeof(double));
  uint64_t at = 0;
  for (size_t r = 0; r < regions; ++r) {
    double* dst = &rec[r * (size_t)kRegion * slot];
    if (counts[r] && row == slot) std::memcpy(dst, lines + row * at, (size_t)counts[r] * row * sizeof(double));
    else for (uint32_t i = 0; i < counts[r]; ++i) {
      std::memcpy(dst + slot * i, lines + row * (at + i), row * sizeof(double));
      for (size_t k = row; k < slot; ++k) dst[slot * i + k] = 0.0;
    }
    at += counts[r];
  }
  if (at != n) return ISX_ERR_BAD_ARG;
  // (blocking copies from pageable memory: whatever the streams held has completed first)
  if (sync_all()) return ISX_ERR_HIP;
  HIPCHK(hipMemcpy(S.d_rec[0], rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(S.d_rec_counts[0], counts.data(), regions * sizeof(uint32_t), hipMemcpyHostToDevice));
  Work wk;
  wk.seed = 0; wk.first = 0; wk.n = n; wk.hist = S.d_hist; wk.stats = S.d_stats; wk.ctr = nullptr; wk.sub = 0; wk.pad = 0;
  Work w;
  rc = launch_work(wk, 0, n, pad, S.stream, &w); if (rc) return rc;                       // (the queue words, zeroed)
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(w.ctr + Q_REGIONS), (int)regions, 1, S.stream));   // (what the trace kernel would have counted)
  DetGrid db = d;
  if (p.route == ROUTE_FIELD_PIPE) db.nbins = p.bin_words;
  db.rec_lines = S.d_rec[0]; db.rec_counts = S.d_rec_counts[0];
  size_t t;
  rc = mark(S.stream, &t); if (rc) return rc;
  if (p.compat_lines) {
    hipLaunchKernelGGL(isx_compat_lines_kernel, dim3(S.cu_count * 8), dim3(256), 0, S.stream, S.d_rec[0], S.d_rec_counts[0], w.ctr);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(p.bin, dim3(bin_grid(p, n, w.pad, (uint64_t)regions, bres)), dim3(p.bblock), p.lds_bin, S.stream, db, w);
  HIPCHK(hipGetLastError());
  return span(2, &t);
}

}  // namespace

extern "C" {

int isx_abi_version(void) { return ISX_ABI_VERSION; }
int isx_stream_version(void) { return ISX_STREAM_VERSION; }

void isx_default_config(isx_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->struct_size = (uint32_t)sizeof(isx_config);
  // fluxAtObserverOptimize.C:33-41 and sweepSeries() :892-896
  c->r_in = 100.1; c->r_out = 101.0; c->theta_max_deg = 170.0;
  c->reflectance = 0.99; c->roughness_rad = 0.01; c->box_half = 300.0;
  c->lambertian = 1; c->max_points = 50000;
  c->src[0] = -60; c->src[1] = 0; c->src[2] = -75;
  c->dir[0] = 5; c->dir[1] = 0; c->dir[2] = 0;
  c->n_theta = 180; c->n_phi = 90;
  c->det_diameter = 40.0; c->det_distance = 100.0; c->exit_port_z = -100.0;
  c->source_model = ISX_SOURCE_PENCIL;
  c->brdf[0] = 0.3; c->brdf[1] = 0.4; c->brdf[2] = 0.6;  // nonLambertianFlux.C:211
}

const char* isx_strerror(int s) {
  switch (s) {
    case ISX_OK: return "ok";
    case ISX_ERR_NO_DEVICE: return "no HIP device available (libisx has no CPU fallback)";
    case ISX_ERR_BAD_CONFIG: return "configuration outside the supported domain";
    case ISX_ERR_BAD_ARG: return "bad argument";
    case ISX_ERR_HIP: return "HIP runtime error (see isx_last_hip_error)";
    case ISX_ERR_NOT_INIT: return "isx_init() has not been called";
    case ISX_ERR_TOO_LARGE: return "too many rays for one call";
    default: return "unknown status";
  }
}

int isx_last_hip_error(void) { return S.last_hip; }

int isx_init(int device) {
  if (S.init) {
    if (device == S.device) return ISX_OK;
    isx_shutdown();
  }
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) { S.last_hip = (int)e; return ISX_ERR_NO_DEVICE; }
  if (device < 0 || device >= count) return ISX_ERR_BAD_ARG;
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  S.cu_count = prop.multiProcessorCount;
  {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && v > 0) S.lds_limit = (size_t)v;
    if (prop.sharedMemPerBlock > S.lds_limit) S.lds_limit = prop.sharedMemPerBlock;
  }
  // from here on a failure releases what was created (isx_shutdown() works on a partially built state)
  S.device = device;
  S.init = true;
  S.have_tab = false;
  e = hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc(&S.d_stats, 8 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(S.d_stats, 0, 8 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc(&S.d_ctr, State::kCtrRing * Q_WORDS * sizeof(uint32_t));
  if (e != hipSuccess) { isx_shutdown(); S.last_hip = (int)e; return ISX_ERR_HIP; }
  if (const char* m = std::getenv("ISX_BIN_MODE")) {
    const int v = std::atoi(m);
    if (v >= 0 && v <= 2) S.bin_mode = v;   // same domain as isx_set_option("bin_mode")
  }
  return ISX_OK;
}

void isx_shutdown(void) {
  if (!S.init) return;
  (void)trace_join();
  S.trace_open = false;
  if (S.stream) (void)hipStreamSynchronize(S.stream);
  if (S.stream2) { (void)hipStreamSynchronize(S.stream2); (void)hipStreamDestroy(S.stream2); S.stream2 = nullptr; }
  if (S.stream3) { (void)hipStreamSynchronize(S.stream3); (void)hipStreamDestroy(S.stream3); S.stream3 = nullptr; }
  for (hipEvent_t e : S.ev_pool) (void)hipEventDestroy(e);
  S.ev_pool.clear();
  S.ev_used = 0;
  S.spans.clear();
  if (S.d_table) (void)hipFree(S.d_table);
  if (S.d_rowtab) (void)hipFree(S.d_rowtab);
  if (S.d_coltab) (void)hipFree(S.d_coltab);
  if (S.d_hist) (void)hipFree(S.d_hist);
  if (S.d_stats) (void)hipFree(S.d_stats);
  if (S.d_aux) (void)hipFree(S.d_aux);
  S.d_aux = nullptr; S.cap_aux = 0;
  if (S.h_pin) (void)hipHostFree(S.h_pin);
  S.h_pin = nullptr; S.cap_pin = 0; S.pending = false; S.occ.clear();
  for (int b = 0; b < State::kRecBufs; ++b) {
    if (S.d_rec[b]) (void)hipFree(S.d_rec[b]);
    if (S.d_rec_counts[b]) (void)hipFree(S.d_rec_counts[b]);
    S.d_rec[b] = nullptr; S.d_rec_counts[b] = nullptr; S.cap_regions[b] = 0;
  }
  if (S.d_ctr) (void)hipFree(S.d_ctr);
  S.d_ctr = nullptr; S.ctr_next = 0;
  for (int b = 0; b < State::kRecBufs; ++b) {
    if (S.d_list[b]) (void)hipFree(S.d_list[b]);
    S.d_list[b] = nullptr; S.cap_list[b] = 0;
    if (S.d_list_b[b]) (void)hipFree(S.d_list_b[b]);
    if (S.d_side[b]) (void)hipFree(S.d_side[b]);
    if (S.d_redo[b]) (void)hipFree(S.d_redo[b]);
    S.d_list_b[b] = nullptr; S.d_side[b] = nullptr; S.d_redo[b] = nullptr;
    S.cap_exit_rays[b] = S.cap_side[b] = S.cap_redo[b] = 0; S.list_pairs[b] = false;
    if (S.ev_free[b]) (void)hipEventDestroy(S.ev_free[b]);
    S.ev_free[b] = nullptr; S.free_set[b] = false;
  }
  for (hipEvent_t& e : S.ev_join) { if (e) (void)hipEventDestroy(e); e = nullptr; }
  if (S.d_exit_totals) (void)hipFree(S.d_exit_totals);
  S.d_exit_totals = nullptr;
  S.fate_launches = 0; S.call_rot = 0;
  S.attr_lds.clear();
  S.d_table = S.d_rowtab = S.d_coltab = nullptr;
  S.d_hist = S.d_stats = nullptr;
  S.cap_bins = S.cap_rows = S.cap_cols = S.cap_hist = 0;
  if (S.stream) (void)hipStreamDestroy(S.stream);
  S.stream = nullptr;
  S.init = false;
  S.have_tab = false;
}

int isx_device_info(char* buf, int buflen) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, S.device));
  if (buf && buflen > 0) std::snprintf(buf, (size_t)buflen, "%s %s cu=%d", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  return prop.multiProcessorCount;
}

int isx_set_option(const char* key, int64_t value) {
  if (!key) return ISX_ERR_BAD_ARG;
  if (S.init && trace_join()) return ISX_ERR_HIP;   // (an option never changes under an overlapped sequence in flight)
  if (!std::strcmp(key, "bin_mode")) { if (value < 0 || value > 2) return ISX_ERR_BAD_ARG; S.bin_mode = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "blocks_per_cu")) { if (value < 1 || value > 8) return ISX_ERR_BAD_ARG; S.blocks_per_cu = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "sched_mask")) { if (value < 0 || value > 255) return ISX_ERR_BAD_ARG; S.sched_mask = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "sched_min")) { if (value < 1 || value > 65) return ISX_ERR_BAD_ARG; S.sched_min = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "trace_blocks_per_cu")) { if (value < 0 || value > 32) return ISX_ERR_BAD_ARG; S.trace_blocks_per_cu = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "trace_block")) { if (value != 64 && value != 128 && value != 256 && value != 512 && value != 1024) return ISX_ERR_BAD_ARG; S.trace_block = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "bin_blocks_per_cu")) { if (value < 0 || value > 32) return ISX_ERR_BAD_ARG; S.bin_blocks_per_cu = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "bin_block")) { if (value != 256 && value != 512 && value != 1024) return ISX_ERR_BAD_ARG; S.bin_block = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "overlap_trace_streams")) { if (value < 1 || value > 2) return ISX_ERR_BAD_ARG; S.overlap_trace_streams = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "call_overlap")) { if (value < -1 || value > 1) return ISX_ERR_BAD_ARG; S.call_overlap = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "call_overlap_streams")) { if (value < 1 || value > 2) return ISX_ERR_BAD_ARG; S.call_overlap_streams = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "overlap")) { if (value < 0 || value > 64) return ISX_ERR_BAD_ARG; S.overlap = (int)value; return ISX_OK; }
  // ("assist_block" 0: back to the default -- 768 threads, 256 for launches below 1e6 rays)
  if (!std::strcmp(key, "assist_block")) {
    if (value == 0) { S.assist_block = ISX_ASSIST_BLOCK; S.assist_block_set = false; return ISX_OK; }
    if (value < 128 || value > ISX_ASSIST_BLOCK || value % 64) return ISX_ERR_BAD_ARG;
    S.assist_block = (int)value; S.assist_block_set = true; return ISX_OK;
  }
  if (!std::strcmp(key, "rays_per_lane")) { if (value < 0 || value > 4096) return ISX_ERR_BAD_ARG; S.rays_per_lane = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "disc_pipeline")) { if (value < 0 || value > 1) return ISX_ERR_BAD_ARG; S.disc_pipeline = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "assist")) { if (value < 0 || value > 1) return ISX_ERR_BAD_ARG; S.assist = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "bin_cols")) { if (value < 0 || value > 2) return ISX_ERR_BAD_ARG; S.bin_cols = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "bin_slots")) { if (value < 0 || value > 1) return ISX_ERR_BAD_ARG; S.bin_slots = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "lf_global")) { if (value < 0 || value > 1) return ISX_ERR_BAD_ARG; S.lf_global = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "field_global")) { if (value < 0 || value > 1) return ISX_ERR_BAD_ARG; S.field_global = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "sorder_lds_orders")) { if (value < -1 || value > ISX_SCENE_ORDER_MAX_ORDERS) return ISX_ERR_BAD_ARG; S.sorder_lds_orders = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "spath_lds_bins")) { if (value < -1 || value > ISX_SCENE_PATH_MAX_BINS) return ISX_ERR_BAD_ARG; S.spath_lds_bins = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "view_global")) { if (value < 0 || value > 1) return ISX_ERR_BAD_ARG; S.view_global = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "resp_global")) { if (value < 0 || value > 1) return ISX_ERR_BAD_ARG; S.resp_global = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "surface_pipeline")) { if (value < 0 || value > 1) return ISX_ERR_BAD_ARG; S.surface_pipeline = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "ray_sub")) { if (value < 0 || value > (1 << 20)) return ISX_ERR_BAD_ARG; S.ray_sub = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "fate_scan")) { if (value < -1 || value > 1) return ISX_ERR_BAD_ARG; S.fate_scan = (int)value; return ISX_OK; }
  if (!std::strcmp(key, "exit_scan")) { if (value < -1 || value > 1) return ISX_ERR_BAD_ARG; S.exit_scan = (int)value; return ISX_OK; }
  // (test option: a bound can be made wider, never narrower)
  if (!std::strcmp(key, "exit_eps_scale")) { if (value < 1 || value > 1000000000ll) return ISX_ERR_BAD_ARG; S.exit_eps_scale = value; return ISX_OK; }
  if (!std::strcmp(key, "pipeline")) { if (value < 0 || value > 1) return ISX_ERR_BAD_ARG; S.pipeline = (int)value; return ISX_OK; }
  // (a launch addresses its rays by 30-bit offsets -- bits 30 and 31 of Ray::ido are flags in the queue records -- and counts
  //  them in 32 bits: the documented maximum of a chunk is 2^26 rays, 3.4 GB of exit-line workspace)
  if (!std::strcmp(key, "pipeline_chunk")) { if (value < 4096 || value > (1ll << 26)) return ISX_ERR_BAD_ARG; S.pipe_chunk = (uint64_t)value; return ISX_OK; }
  if (!std::strcmp(key, "grid_blocks")) { if (value < 0 || value > 65535) return ISX_ERR_BAD_ARG; S.grid_blocks = (int)value; return ISX_OK; }
  return ISX_ERR_BAD_ARG;
}

void* isx_stream(void) { return (void*)S.stream; }

int isx_last_kernel_ms(double* single_ms, double* trace_ms, double* bin_ms) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (single_ms) *single_ms = S.last_ms[0];
  if (trace_ms) *trace_ms = S.last_ms[1];
  if (bin_ms) *bin_ms = S.last_ms[2];
  return ISX_OK;
}

int isx_sync(void) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  return sync_all();
}

int isx_take_stats(isx_stats* stats) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  return collect_stats(stats);
}

int isx_fluxmap_device(const isx_config* cfg, uint64_t n_rays, uint64_t seed, uint64_t first_ray, uint64_t* d_hits) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (!cfg || !d_hits) return ISX_ERR_BAD_ARG;
  g_device_call = true;
  const int rc = enqueue({.sink = SINK_FLUX, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray,
                         .d_hist = (unsigned long long*)d_hits});
  g_device_call = false;
  return rc;
}

int isx_fluxmap(const isx_config* cfg, uint64_t n_rays, uint64_t seed, uint64_t first_ray, uint64_t* hits,
                isx_stats* stats) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (!cfg || !hits) return ISX_ERR_BAD_ARG;
  int rc = check_grid(cfg);
  if (rc) return rc;
  const size_t nb = (size_t)cfg->n_theta * cfg->n_phi, bytes = nb * sizeof(unsigned long long);
  rc = call_open(nb);
  if (rc) return rc;
  rc = zero_hist(nb);
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_FLUX, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .d_hist = S.d_hist});
  if (rc == ISX_OK) rc = stage_result(S.d_hist, bytes);
  rc = call_close(rc, stats);
  if (rc == ISX_OK) fetch_result(hits, bytes);
  return rc;
}

int isx_trace_endstates(const isx_config* cfg, uint64_t n, uint64_t seed, uint64_t first, int32_t* status,
                        int32_t* n_points, double* last_point, double* direction) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (trace_join()) return ISX_ERR_HIP;   // (behind an overlapped sequence, as every entry but isx_fluxmap_device)
  if (!cfg || !status || !n_points || !last_point || !direction) return ISX_ERR_BAD_ARG;
  if (n == 0) return ISX_OK;
  if (n > (1ull << 28)) return ISX_ERR_TOO_LARGE;
  Geom g;
  int rc = prepare_geom(cfg, &g);
  if (rc) return rc;
  DevBuf<int32_t> b_st, b_np;
  DevBuf<double> b_lp, b_dir;
  HIPCHK(b_st.alloc(n)); HIPCHK(b_np.alloc(n)); HIPCHK(b_lp.alloc(n * 3)); HIPCHK(b_dir.alloc(n * 3));
  int32_t *d_st = b_st.p, *d_np = b_np.p;
  double *d_lp = b_lp.p, *d_dir = b_dir.p;
  const int blk = 256;
  const unsigned grid = (unsigned)((n + blk - 1) / blk);
  hipLaunchKernelGGL(isx_endstates_kernel, dim3(grid), dim3(blk), 0, S.stream, g, seed, first, n, d_st, d_np, d_lp, d_dir);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(status, d_st, n * 4, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemcpyAsync(n_points, d_np, n * 4, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemcpyAsync(last_point, d_lp, n * 24, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemcpyAsync(direction, d_dir, n * 24, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipStreamSynchronize(S.stream));
  return ISX_OK;
}

int isx_fate_scan(const isx_config* cfg, uint64_t n, uint64_t seed, uint64_t first, int32_t* fate, int32_t* order) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (trace_join()) return ISX_ERR_HIP;   // (behind an overlapped sequence, as every entry but isx_fluxmap_device)
  if (!cfg || !fate || !order) return ISX_ERR_BAD_ARG;
  if (n == 0) return ISX_OK;
  if (n > (1ull << 28)) return ISX_ERR_TOO_LARGE;
  if (first > UINT64_MAX - n) return ISX_ERR_BAD_ARG;
  Geom g;
  FateConsts f;
  int rc = prepare_geom(cfg, &g, &f);
  if (rc) return rc;
  if (!f.ok) return ISX_ERR_BAD_CONFIG;   // (a configuration the scan does not serve has no fates to report)
  DevBuf<int32_t> b_ft, b_or;
  HIPCHK(b_ft.alloc(n)); HIPCHK(b_or.alloc(n));
  const int blk = 256;
  const unsigned grid = (unsigned)((n + blk - 1) / blk);
  hipLaunchKernelGGL(isx_fate_diag_kernel, dim3(grid), dim3(blk), 0, S.stream, f, seed, first, n, b_ft.p, b_or.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(fate, b_ft.p, n * 4, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemcpyAsync(order, b_or.p, n * 4, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipStreamSynchronize(S.stream));
  return ISX_OK;
}

int isx_fate_scan_launches(uint64_t* launches) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (!launches) return ISX_ERR_BAD_ARG;
  *launches = S.fate_launches;
  return ISX_OK;
}

int isx_exit_scan_counts(uint64_t* accepted, uint64_t* list_b, uint64_t* redo) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  unsigned long long t[3] = {0, 0, 0};
  if (S.d_exit_totals) {   // (allocated with the first launch that takes the path)
    if (sync_all()) return ISX_ERR_HIP;
    HIPCHK(hipMemcpy(t, S.d_exit_totals, sizeof(t), hipMemcpyDeviceToHost));
  }
  if (accepted) *accepted = t[0];
  if (list_b) *list_b = t[1];
  if (redo) *redo = t[2];
  return ISX_OK;
}

int isx_mathprobe(int op, const double* a, const double* b, const double* c, double* out, int32_t n) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (trace_join()) return ISX_ERR_HIP;   // (behind an overlapped sequence, as every entry but isx_fluxmap_device)
  if (!a || !out || n <= 0) return ISX_ERR_BAD_ARG;
  DevBuf<double> ba, bb, bc, bo;
  const size_t bytes = (size_t)n * 8;
  HIPCHK(ba.alloc(n)); HIPCHK(bb.alloc(n)); HIPCHK(bc.alloc(n)); HIPCHK(bo.alloc(n));
  HIPCHK(hipMemcpy(ba.p, a, bytes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(bb.p, b ? b : a, bytes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(bc.p, c ? c : a, bytes, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(isx_mathprobe_kernel, dim3((n + 255) / 256), dim3(256), 0, S.stream, op, ba.p, bb.p, bc.p, bo.p, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(S.stream));
  HIPCHK(hipMemcpy(out, bo.p, bytes, hipMemcpyDeviceToHost));
  return ISX_OK;
}

int isx_detector_table(const isx_config* cfg, double* out) {
  if (!cfg || !out) return ISX_ERR_BAD_ARG;
  if (!config_abi_ok(cfg) || cfg->n_theta < 1 || cfg->n_phi < 1) return ISX_ERR_BAD_CONFIG;
  for (int i = 0; i < cfg->n_theta; ++i) {
    const double theta = (i + 0.5) * 90.0 / cfg->n_theta;
    for (int j = 0; j < cfg->n_phi; ++j) {
      const double phi = (j + 0.5) * 360.0 / cfg->n_phi;
      det_set_position(theta, phi, cfg->det_distance, cfg->exit_port_z, out + 6 * ((size_t)i * cfg->n_phi + j));
    }
  }
  return ISX_OK;
}

int isx_disc_sweep(const isx_config* cfg, const double* centers_axes, int32_t n_disc, double radius, double half_thick,
                   uint64_t n_rays, uint64_t seed, uint64_t first_ray, uint64_t* hits, isx_stats* stats) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (!cfg || !centers_axes || !hits || n_disc < 1) return ISX_ERR_BAD_ARG;
  if (cfg->source_model != ISX_SOURCE_PENCIL) return ISX_ERR_BAD_CONFIG;
  if (!(radius > 0) || !(half_thick > 0)) return ISX_ERR_BAD_ARG;
  int rc = call_open((size_t)n_disc);
  if (rc) return rc;
  g_disc_clusters = DiscClusters();
  rc = S.disc_pipeline ? upload_discs_clustered(centers_axes, (size_t)n_disc, radius, half_thick) : upload_aux(centers_axes, (size_t)n_disc * 6);
  if (rc == ISX_OK) rc = zero_hist((size_t)n_disc);
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_DISC, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .d_hist = S.d_hist,
                                 .nbins_override = n_disc, .d_discs = S.d_aux, .disc_r = radius, .disc_h = half_thick});
  if (rc == ISX_OK) rc = copy_out(hits, S.d_hist, (size_t)n_disc * sizeof(unsigned long long));
  return call_close(rc, stats);
}

int isx_disc_sweep_per_position(const isx_config* cfg, const double* centers_axes, int32_t n_disc, double radius,
                                double half_thick, uint64_t rays_per_position, uint64_t seed, uint64_t first_ray,
                                uint64_t* hits, isx_stats* stats) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (!cfg || !centers_axes || !hits || n_disc < 1 || rays_per_position < 1) return ISX_ERR_BAD_ARG;
  if (cfg->source_model != ISX_SOURCE_PENCIL) return ISX_ERR_BAD_CONFIG;
  if (!(radius > 0) || !(half_thick > 0)) return ISX_ERR_BAD_ARG;
  if ((uint64_t)n_disc > ISX_MAX_RAYS_PER_CALL / rays_per_position) return ISX_ERR_TOO_LARGE;
  int rc = call_open((size_t)n_disc);
  if (rc) return rc;
  rc = upload_aux(centers_axes, (size_t)n_disc * 6);
  if (rc == ISX_OK) rc = zero_hist((size_t)n_disc);
  const PerPos pp{first_ray, rays_per_position, 1};
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_DISCPOS, .c = cfg, .n = (uint64_t)n_disc * rays_per_position, .seed = seed,
                                 .first = first_ray, .d_hist = S.d_hist, .nbins_override = n_disc, .d_discs = S.d_aux,
                                 .disc_r = radius, .disc_h = half_thick, .pp = &pp});
  if (rc == ISX_OK) rc = copy_out(hits, S.d_hist, (size_t)n_disc * sizeof(unsigned long long));
  return call_close(rc, stats);
}

int isx_fluxmap_per_position(const isx_config* cfg, uint64_t rays_per_position, int32_t fold, uint64_t first_group,
                             uint64_t n_groups, uint64_t seed, uint64_t first_ray, uint64_t* hits, isx_stats* stats) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (!cfg || !hits || rays_per_position < 1) return ISX_ERR_BAD_ARG;
  int rc = check_grid(cfg);
  if (rc) return rc;
  if (fold != 1 && fold != 2) return ISX_ERR_BAD_ARG;
  const size_t nb = (size_t)cfg->n_theta * cfg->n_phi;
  const uint64_t groups_total = nb / (uint64_t)fold;
  if (first_group > groups_total || n_groups > groups_total - first_group) return ISX_ERR_BAD_ARG;
  if (n_groups > ISX_MAX_RAYS_PER_CALL / rays_per_position) return ISX_ERR_TOO_LARGE;
  rc = call_open(nb);
  if (rc) return rc;
  const PerPos pp{first_ray, rays_per_position, fold};
  rc = zero_hist(nb);
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_PERPOS, .c = cfg, .n = n_groups * rays_per_position, .seed = seed,
                                 .first = first_ray + first_group * rays_per_position, .d_hist = S.d_hist, .pp = &pp});
  if (rc == ISX_OK) rc = copy_out(hits, S.d_hist, nb * sizeof(unsigned long long));
  return call_close(rc, stats);
}

int isx_trace_rays_detector(const isx_config* cfg, const double* detector, double width, uint64_t n_rays, uint64_t seed,
                            uint64_t first_ray, uint64_t* hit_count, isx_stats* stats) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (!cfg || !detector || !hit_count || !(width > 0)) return ISX_ERR_BAD_ARG;
  int rc = call_open(1);
  if (rc) return rc;
  rc = upload_aux(detector, 6);
  if (rc == ISX_OK) rc = zero_hist(1);
  const PerPos pp{first_ray, n_rays > 0 ? n_rays : 1, 1, S.d_aux, width};   // (S.d_aux: after the upload, which may move it)
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_PERPOS, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray,
                                 .d_hist = S.d_hist, .nbins_override = 1, .pp = &pp});
  unsigned long long h = 0;
  if (rc == ISX_OK) rc = stage_result(S.d_hist, sizeof(h));
  rc = call_close(rc, stats);
  if (rc == ISX_OK) fetch_result(&h, sizeof(h));
  *hit_count = h;
  return rc;
}

int isx_exit_directions(const isx_config* cfg, uint64_t n_rays, uint64_t seed, uint64_t first_ray, uint64_t capacity,
                        uint64_t* ray_ids, double* directions, uint64_t* count, isx_stats* stats) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (!cfg || !ray_ids || !directions || !count || capacity < 1) return ISX_ERR_BAD_ARG;
  // no more records than rays, and the 32-byte records of one call must stay addressable (ISX_MAX_LOG_RECORDS)
  if (capacity > n_rays && n_rays > 0) capacity = n_rays;
  if (capacity > ISX_MAX_LOG_RECORDS) return ISX_ERR_TOO_LARGE;
  int rc = call_open(1);
  if (rc) return rc;
  DevBuf<double> d_rec;               // 4 doubles per record: ray index (bits), direction
  DevBuf<unsigned long long> d_cnt;
  rc = hip_rc(d_rec.alloc(capacity * 4));
  if (rc == ISX_OK) rc = hip_rc(d_cnt.alloc(1));
  if (rc == ISX_OK) rc = hip_rc(hipMemsetAsync(d_cnt.p, 0, 8, S.stream));
  if (rc == ISX_OK) rc = zero_hist(1);
  const LogSink lg{d_rec.p, d_cnt.p, capacity};
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_LOG, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .d_hist = S.d_hist,
                                 .lg = &lg});
  unsigned long long total = 0;
  if (rc == ISX_OK) rc = hip_rc(hipStreamSynchronize(S.stream));
  if (rc == ISX_OK) rc = hip_rc(hipMemcpy(&total, d_cnt.p, 8, hipMemcpyDeviceToHost));
  const uint64_t kept = total < capacity ? total : capacity;
  std::vector<double> rec(rc == ISX_OK ? kept * 4 : 0);
  if (rc == ISX_OK && kept) rc = hip_rc(hipMemcpy(rec.data(), d_rec.p, kept * 32, hipMemcpyDeviceToHost));
  if (rc == ISX_OK) {
    // slots are handed out in completion order: sort by ray index so the log is reproducible
    std::vector<size_t> order(kept);
    for (size_t k = 0; k < kept; ++k) order[k] = k;
    auto id_of = [&](size_t k) { uint64_t v; std::memcpy(&v, &rec[4 * k], 8); return v; };
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return id_of(a) < id_of(b); });
    for (size_t k = 0; k < kept; ++k) {
      const size_t o = order[k];
      ray_ids[k] = id_of(o);
      directions[3 * k] = rec[4 * (size_t)o + 1]; directions[3 * k + 1] = rec[4 * (size_t)o + 2]; directions[3 * k + 2] = rec[4 * (size_t)o + 3];
    }
  }
  *count = total;
  return call_close(rc, stats);
}

int isx_fluxmap_series(const isx_config* cfgs, int32_t n_cfg, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                       uint64_t* hits, isx_stats* stats) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (!cfgs || !hits || n_cfg < 1 || n_cfg > 4096) return ISX_ERR_BAD_ARG;
  int rc = check_grid(&cfgs[0]);
  if (rc) return rc;
  for (int k = 1; k < n_cfg; ++k)
    if (!same_grid(cfgs[0], cfgs[k]) || cfgs[k].det_diameter != cfgs[0].det_diameter) return ISX_ERR_BAD_CONFIG;
  const size_t nb = (size_t)cfgs[0].n_theta * cfgs[0].n_phi;
  rc = call_open(nb * (size_t)n_cfg);
  if (rc) return rc;
  DevBuf<unsigned long long> d_st;   // the census of each configuration
  rc = hip_rc(d_st.alloc((size_t)n_cfg * 8));
  if (rc == ISX_OK) rc = hip_rc(hipMemsetAsync(d_st.p, 0, (size_t)n_cfg * 64, S.stream));
  if (rc == ISX_OK) rc = zero_hist(nb * (size_t)n_cfg);
  // every configuration is enqueued back to back (no host round trip in between); configuration k
  // uses the ray indices [first_ray + k*n_rays, +n_rays) so the maps are statistically independent
  for (int k = 0; k < n_cfg && rc == ISX_OK; ++k) {
    rc = enqueue({.sink = SINK_FLUX, .c = &cfgs[k], .n = n_rays, .seed = seed, .first = first_ray + (uint64_t)k * n_rays,
                 .d_hist = S.d_hist + (size_t)k * nb, .d_stats = d_st.p + (size_t)k * 8});
  }
  std::vector<unsigned long long> hst((size_t)n_cfg * 8);
  if (rc == ISX_OK) rc = copy_out(hits, S.d_hist, nb * (size_t)n_cfg * sizeof(unsigned long long));
  if (rc == ISX_OK) rc = copy_out(hst.data(), d_st.p, hst.size() * 8);
  isx_stats tot;
  rc = call_close(rc, &tot);   // tot.t_kernel_ms = all launches
  if (rc == ISX_OK && stats) {
    for (int k = 0; k < n_cfg; ++k) {
      const unsigned long long* h = &hst[(size_t)k * 8];
      stats[k].launched = h[0]; stats[k].exited = h[1]; stats[k].counted_below_z = h[2]; stats[k].absorbed = h[3];
      stats[k].suspended = h[4]; stats[k].bin_increments = h[5]; stats[k].wall_hits = h[6];
      stats[k].t_kernel_ms = tot.t_kernel_ms;  // total of the series (launches are not timed separately)
    }
  }
  return rc;
}

int isx_exit_dz_hist(const isx_config* cfg, uint64_t n_rays, uint64_t seed, uint64_t first_ray, int32_t nbins,
                     uint64_t* hist, isx_stats* stats) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (!cfg || !hist || nbins < 1) return ISX_ERR_BAD_ARG;
  int rc = call_open((size_t)nbins);
  if (rc) return rc;
  rc = zero_hist((size_t)nbins);
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_DZ, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .d_hist = S.d_hist,
                                 .nbins_override = nbins});
  if (rc == ISX_OK) rc = copy_out(hist, S.d_hist, (size_t)nbins * sizeof(unsigned long long));
  return call_close(rc, stats);
}

void isx_default_exit_map_spec(const isx_config* cfg, isx_exit_map_spec* spec) {
  if (!spec) return;
  std::memset(spec, 0, sizeof(*spec));
  spec->struct_size = (uint32_t)sizeof(isx_exit_map_spec);
  spec->n_u = 128; spec->n_v = 128; spec->n_x = 64; spec->n_y = 64;
  isx_config dflt;
  if (!cfg) { isx_default_config(&dflt); cfg = &dflt; }
  spec->plane_z = cfg->exit_port_z;
  spec->half_extent = 1.25 * cfg->r_in * std::sin(cfg->theta_max_deg * M_PI / 180.0);   // the port radius + 25 %
}

int isx_exit_maps_device(const isx_config* cfg, const isx_exit_map_spec* spec, uint64_t n_rays, uint64_t seed,
                         uint64_t first_ray, uint64_t* d_dir_map, uint64_t* d_pos_map, uint64_t* d_counts) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (!cfg || !spec || !d_counts) return ISX_ERR_BAD_ARG;
  const ExitSink xm{spec, (unsigned long long*)d_dir_map, (unsigned long long*)d_pos_map, (unsigned long long*)d_counts};
  return enqueue({.sink = SINK_EXITMAP, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .xm = &xm});
}

int isx_exit_maps(const isx_config* cfg, const isx_exit_map_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                  uint64_t* dir_map, uint64_t* pos_map, isx_exit_map_counts* counts, isx_stats* stats) {
  if (!S.init) return ISX_ERR_NOT_INIT;
  if (!cfg || !spec) return ISX_ERR_BAD_ARG;
  if (!config_abi_ok(cfg)) return ISX_ERR_BAD_CONFIG;
  int rc = check_exit_spec(spec);
  if (rc) return rc;
  const size_t ndir = (size_t)spec->n_u * spec->n_v, npos = (size_t)spec->n_x * spec->n_y, words = ndir + npos + 5;
  if ((ndir && !dir_map) || (npos && !pos_map)) return ISX_ERR_BAD_ARG;
  rc = call_open(words);
  if (rc) return rc;
  // the call's accumulators in the pooled histogram: direction map | plane map | the five counters
  const ExitSink xm{spec, ndir ? S.d_hist : nullptr, npos ? S.d_hist + ndir : nullptr, S.d_hist + ndir + npos};
  rc = zero_hist(words);
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_EXITMAP, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .xm = &xm});
  if (rc == ISX_OK) rc = stage_result(S.d_hist, words * sizeof(unsigned long long));
  rc = call_close(rc, stats);
  if (rc == ISX_OK) {
    const unsigned long long* h = reinterpret_cast<const unsigned long long*>(S.h_pin + 64);
    if (ndir) std::memcpy(dir_map, h, ndir * 8);
    if (npos) std::memcpy(pos_map, h + ndir, npos * 8);
    if (counts) {
      const unsigned long long* k = h + ndir + npos;
      counts->dir_binned = k[0]; counts->dir_outside = k[1]; counts->pos_binned = k[2]; counts->pos_outside = k[3]; counts->upward = k[4];
    }
  }
  return rc;
}

void isx_default_wall_map_spec(const isx_config* cfg, isx_wall_map_spec* spec) {
  (void)cfg;   // (the default does not depend on the configuration: the map is scaled to the unit disc)
  if (!spec) return;
  std::memset(spec, 0, sizeof(*spec));
  spec->struct_size = (uint32_t)sizeof(isx_wall_map_spec);
  spec->n_x = 64; spec->n_y = 64; spec->first_order = 0;
}

int isx_wall_map_device(const isx_config* cfg, const isx_wall_map_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                        uint64_t* d_wall_map, uint64_t* d_counts) {
  if (!S.init) return not_initialised();
  if (!cfg || !spec || !d_wall_map || !d_counts) return ISX_ERR_BAD_ARG;
  const WallSink wm{spec, (unsigned long long*)d_wall_map, (unsigned long long*)d_counts};
  return enqueue({.sink = SINK_WALL, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .wm = &wm});
}

int isx_wall_map(const isx_config* cfg, const isx_wall_map_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                 uint64_t* wall_map, isx_wall_map_counts* counts, isx_stats* stats) {
  if (!S.init) return not_initialised();
  if (!cfg || !spec || !wall_map) return ISX_ERR_BAD_ARG;
  if (!config_abi_ok(cfg)) return ISX_ERR_BAD_CONFIG;
  int rc = check_wall_spec(spec);
  if (rc) return rc;
  const size_t nmap = (size_t)spec->n_x * spec->n_y, words = nmap + 4;
  rc = call_open(words);
  if (rc) return rc;
  // the call's accumulators in the pooled histogram: the map | the four counters
  const WallSink wm{spec, S.d_hist, S.d_hist + nmap};
  rc = zero_hist(words);
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_WALL, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .wm = &wm});
  if (rc == ISX_OK) rc = stage_result(S.d_hist, words * sizeof(unsigned long long));
  rc = call_close(rc, stats);
  if (rc == ISX_OK) {
    const unsigned long long* h = reinterpret_cast<const unsigned long long*>(S.h_pin + 64);
    std::memcpy(wall_map, h, nmap * 8);
    if (counts) { counts->binned = h[nmap]; counts->outside = h[nmap + 1]; counts->skipped = h[nmap + 2]; counts->other_surface = h[nmap + 3]; }
  }
  return rc;
}

void isx_default_light_field_spec(const isx_config* cfg, isx_exit_map_spec* spec) {
  if (!spec) return;
  isx_default_exit_map_spec(cfg, spec);   // (plane_z = exit_port_z and the exit maps' half_extent)
  spec->n_u = 32; spec->n_v = 32; spec->n_x = 32; spec->n_y = 32;
}

int isx_light_field_device(const isx_config* cfg, const isx_exit_map_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                           uint64_t* d_field, uint64_t* d_counts) {
  // (what needs no device is answered first: a NULL argument or a refused spec is the same answer with and without one)
  if (!cfg || !spec || !d_field || !d_counts) return ISX_ERR_BAD_ARG;
  const int bad = check_field_spec(spec);
  if (bad) return bad;
  if (!S.init) return not_initialised();
  const FieldSink lf{spec, (unsigned long long*)d_field, (unsigned long long*)d_counts};
  return enqueue({.sink = SINK_LIGHTFIELD, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .lf = &lf});
}

int isx_light_field(const isx_config* cfg, const isx_exit_map_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                    uint64_t* field, isx_light_field_counts* counts, isx_stats* stats) {
  if (!cfg || !spec || !field) return ISX_ERR_BAD_ARG;
  if (!config_abi_ok(cfg)) return ISX_ERR_BAD_CONFIG;
  int rc = check_field_spec(spec);
  if (rc) return rc;
  if (!S.init) return not_initialised();
  const size_t nfield = (size_t)spec->n_x * spec->n_y * spec->n_u * spec->n_v;
  rc = call_open(nfield + 4);   // (the pooled histogram: at most 32 MiB + the counters)
  if (rc) return rc;
  // the call's accumulators in the pooled histogram: the field | the four counters.  The field goes straight into the caller's
  // memory (up to 32 MiB: not through the staging buffer), the counters through the staging buffer.
  const FieldSink lf{spec, S.d_hist, S.d_hist + nfield};
  rc = zero_hist(nfield + 4);
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_LIGHTFIELD, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .lf = &lf});
  if (rc == ISX_OK) rc = copy_out(field, S.d_hist, nfield * sizeof(unsigned long long));
  if (rc == ISX_OK) rc = stage_result(S.d_hist + nfield, 4 * sizeof(unsigned long long));
  rc = call_close(rc, stats);
  if (rc == ISX_OK && counts) {
    const unsigned long long* k = reinterpret_cast<const unsigned long long*>(S.h_pin + 64);
    counts->binned = k[0]; counts->pos_outside = k[1]; counts->dir_outside = k[2]; counts->upward = k[3];
  }
  return rc;
}

// the region layout of an injected call, checked (isx.h): the caller's counts, or full regions with the rest in the last
static int inject_layout(uint64_t n, const uint32_t* region_counts, int32_t n_regions, std::vector<uint32_t>& layout) {
  if (region_counts) {
    if (n_regions < 1 || n_regions > ISX_INJECT_MAX_REGIONS) return ISX_ERR_BAD_ARG;
    uint64_t sum = 0;
    for (int32_t r = 0; r < n_regions; ++r) {
      if (region_counts[r] > kRegion) return ISX_ERR_BAD_ARG;
      sum += region_counts[r];
    }
    if (sum != n) return ISX_ERR_BAD_ARG;
    layout.assign(region_counts, region_counts + n_regions);
  } else {
    if (n_regions != 0) return ISX_ERR_BAD_ARG;
    for (uint64_t left = n; left > 0; left -= layout.back()) layout.push_back((uint32_t)std::min<uint64_t>(left, kRegion));
  }
  return ISX_OK;
}

// (the staging copies are std::vectors: no exception crosses the ABI)
int isx_bin_injected_lines(const isx_config* cfg, int32_t sink, const isx_exit_map_spec* spec, const double* lines, uint64_t n,
                           const uint32_t* region_counts, int32_t n_regions, int32_t unit, uint64_t* out_a, uint64_t* out_b,
                           uint64_t* counts, uint64_t* bin_increments) try {
  // ---- what needs no device (isx.h: the refusals)
  if (!cfg || (n && !lines)) return ISX_ERR_BAD_ARG;
  if (sink != ISX_INJECT_FLUX && sink != ISX_INJECT_EXIT_MAPS && sink != ISX_INJECT_LIGHT_FIELD) return ISX_ERR_BAD_ARG;
  if (unit != ISX_INJECT_UNIT_AUTO && unit != 0 && unit != 2) return ISX_ERR_BAD_ARG;
  if (n > ISX_INJECT_MAX_LINES) return ISX_ERR_TOO_LARGE;
  if (!config_abi_ok(cfg)) return ISX_ERR_BAD_CONFIG;
  std::vector<uint32_t> layout;
  int rc = inject_layout(n, region_counts, n_regions, layout);
  if (rc) return rc;
  size_t na = 0, nb = 0, nc = 0;   // words of out_a, out_b, counts
  {
    Geom g;
    rc = prepare_geom(cfg, &g);   // (the geometry is not used, but a config the public calls refuse is refused here too)
    if (rc) return rc;
  }
  if (sink == ISX_INJECT_FLUX) {
    rc = check_grid(cfg);
    if (rc) return rc;
    if (!out_a) return ISX_ERR_BAD_ARG;
    na = (size_t)cfg->n_theta * cfg->n_phi;
    for (uint64_t i = 0; i < n; ++i) {
      const double* l = lines + 6 * i;
      for (int k = 0; k < 6; ++k) if (!std::isfinite(l[k])) return ISX_ERR_BAD_ARG;
      const double p2 = l[0] * l[0] + l[1] * l[1] + l[2] * l[2];
      if (p2 > 3.0 * cfg->box_half * cfg->box_half) return ISX_ERR_BAD_ARG;   // (beyond the world box: no traced ray ends there)
      const double vn = std::sqrt(l[3] * l[3] + l[4] * l[4] + l[5] * l[5]);
      if (!(std::fabs(vn - 1.0) <= 1e-12)) return ISX_ERR_BAD_ARG;
    }
  } else {
    if (!spec || !counts) return ISX_ERR_BAD_ARG;
    if (sink == ISX_INJECT_EXIT_MAPS) {
      rc = check_exit_spec(spec);
      if (rc) return rc;
      na = (size_t)spec->n_u * spec->n_v; nb = (size_t)spec->n_x * spec->n_y; nc = 5;
      if ((na && !out_a) || (nb && !out_b)) return ISX_ERR_BAD_ARG;
    } else {
      rc = check_field_spec(spec);
      if (rc) return rc;
      na = (size_t)spec->n_x * spec->n_y * spec->n_u * spec->n_v; nc = 4;
      if (!out_a) return ISX_ERR_BAD_ARG;
    }
  }
  if (!S.init) return not_initialised();
  if (bin_increments) *bin_increments = 0;
  if (n == 0) return ISX_OK;
  // ---- the call's accumulators in the pooled histogram (out_a | out_b | counts), its DetGrid and its plan as the sink's public
  // call has them
  const size_t words = na + nb + nc;
  rc = call_open(words);
  if (rc) return rc;
  std::vector<unsigned long long> host(words);
  isx_stats st;
  std::memset(&st, 0, sizeof(st));
  rc = zero_hist(words);
  if (rc == ISX_OK) {
    const int ksink = sink == ISX_INJECT_FLUX ? SINK_FLUX : sink == ISX_INJECT_EXIT_MAPS ? SINK_EXITMAP : SINK_LIGHTFIELD;
    const ExitSink xm{spec, na ? S.d_hist : nullptr, nb ? S.d_hist + na : nullptr, S.d_hist + na + nb};
    const FieldSink lf{spec, S.d_hist, S.d_hist + na};
    const Call call{.sink = ksink, .c = cfg, .n = n, .xm = &xm, .lf = &lf};
    DetGrid d;
    size_t lds = 0;
    rc = sink_grid(call, d, lds);
    if (rc == ISX_OK) {
      const Plan p = plan_launch(call, d, lds);
      const Route want = sink == ISX_INJECT_FLUX ? ROUTE_FLUX_PIPE : sink == ISX_INJECT_EXIT_MAPS ? ROUTE_EXIT_PIPE : ROUTE_FIELD_PIPE;
      if (p.route != want || !p.bin || !p.binning || p.slot_doubles != 6) rc = ISX_ERR_BAD_CONFIG;   // (no binning kernel answers this call)
      else {
        const double loud[6] = {0.0, 0.0, cfg->exit_port_z + 0.5 * cfg->det_distance, 0.0, 0.0, -1.0};
        const uint32_t pad = unit == ISX_INJECT_UNIT_AUTO ? (n < 1000000ull ? 2u : 0u) : (uint32_t)unit;
        rc = run_injected(p, d, lines, n, layout, pad, loud);
      }
    }
  }
  if (rc == ISX_OK) rc = copy_out(host.data(), S.d_hist, words * sizeof(unsigned long long));
  rc = call_close(rc, &st);
  if (rc) return rc;
  for (size_t k = 0; k < na; ++k) out_a[k] += host[k];
  for (size_t k = 0; k < nb; ++k) out_b[k] += host[na + k];
  for (size_t k = 0; k < nc; ++k) counts[k] += host[na + nb + k];
  if (bin_increments) *bin_increments = st.bin_increments;
  return ISX_OK;
} catch (const std::bad_alloc&) {
  return ISX_ERR_TOO_LARGE;
}

// (the staging copies are std::vectors: no exception crosses the ABI)
int isx_bin_injected_segments(const isx_config* cfg, const double* centers_axes, int32_t n_disc, double radius, double half_thick,
                              const double* segments, uint64_t n, const uint32_t* region_counts, int32_t n_regions, int32_t unit,
                              uint64_t* hits, uint64_t* bin_increments) try {
  // ---- what needs no device (isx.h: the refusals)
  if (!cfg || !centers_axes || !hits || (n && !segments)) return ISX_ERR_BAD_ARG;
  if (n_disc < 1 || n_disc > 36000) return ISX_ERR_BAD_ARG;   // (sink_grid's limit for a disc list)
  if (!(radius > 0) || !(half_thick > 0) || !std::isfinite(radius) || !std::isfinite(half_thick)) return ISX_ERR_BAD_ARG;
  if (unit != ISX_INJECT_UNIT_AUTO && unit != 0 && unit != 2) return ISX_ERR_BAD_ARG;
  if (n > ISX_INJECT_MAX_LINES) return ISX_ERR_TOO_LARGE;
  if (!config_abi_ok(cfg)) return ISX_ERR_BAD_CONFIG;
  std::vector<uint32_t> layout;
  int rc = inject_layout(n, region_counts, n_regions, layout);
  if (rc) return rc;
  {
    Geom g;
    rc = prepare_geom(cfg, &g);   // (the geometry is not used, but a config isx_disc_sweep refuses is refused here too)
    if (rc) return rc;
    if (cfg->source_model != ISX_SOURCE_PENCIL) return ISX_ERR_BAD_CONFIG;
  }
  // the domain: what isx_trace_assist_disc_kernel can leave behind, and what the binary32 margins of the cluster test are written for
  const double reach2 = 3.0 * cfg->box_half * cfg->box_half, tmax_max = 2.0 * std::sqrt(3.0) * cfg->box_half;
  auto unit_vec = [](const double* v) { return std::fabs(std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) - 1.0) <= 1e-12; };
  auto in_reach = [&](const double* x) { return x[0] * x[0] + x[1] * x[1] + x[2] * x[2] <= reach2; };
  for (int32_t k = 0; k < n_disc; ++k) {
    const double* ca = centers_axes + 6 * (size_t)k;
    for (int q = 0; q < 6; ++q) if (!std::isfinite(ca[q])) return ISX_ERR_BAD_ARG;
    if (!in_reach(ca) || !unit_vec(ca + 3)) return ISX_ERR_BAD_ARG;
  }
  for (uint64_t i = 0; i < n; ++i) {
    const double* s = segments + 7 * i;
    for (int q = 0; q < 7; ++q) if (!std::isfinite(s[q])) return ISX_ERR_BAD_ARG;
    if (!in_reach(s) || !unit_vec(s + 3) || !(s[6] >= 0.0) || !(s[6] <= tmax_max)) return ISX_ERR_BAD_ARG;
  }
  if (!S.init) return not_initialised();
  if (bin_increments) *bin_increments = 0;
  if (n == 0) return ISX_OK;
  // ---- the call as isx_disc_sweep opens it: its histogram, the clustered disc list, its DetGrid and its plan
  rc = call_open((size_t)n_disc);
  if (rc) return rc;
  std::vector<unsigned long long> host((size_t)n_disc);
  isx_stats st;
  std::memset(&st, 0, sizeof(st));
  g_disc_clusters = DiscClusters();
  rc = S.disc_pipeline ? upload_discs_clustered(centers_axes, (size_t)n_disc, radius, half_thick) : ISX_ERR_BAD_CONFIG;
  if (rc == ISX_OK) rc = zero_hist((size_t)n_disc);
  if (rc == ISX_OK) {
    const Call call{.sink = SINK_DISC, .c = cfg, .n = n, .nbins_override = n_disc, .d_discs = S.d_aux, .disc_r = radius, .disc_h = half_thick};
    DetGrid d;
    size_t lds = 0;
    rc = sink_grid(call, d, lds);
    if (rc == ISX_OK) {
      const Plan p = plan_launch(call, d, lds);
      if (p.route != ROUTE_DISC_PIPE || p.bin != isx_bin_discs_kernel || p.slot_doubles != 8) rc = ISX_ERR_BAD_CONFIG;   // (the fused kernel answers isx_disc_sweep)
      else {
        clustered_discs(d);
        // through the centre of disc 0 along its axis, from one unit before the centre to one unit behind
        const double* c0 = centers_axes;
        const double loud[8] = {c0[0] - c0[3], c0[1] - c0[4], c0[2] - c0[5], c0[3], c0[4], c0[5], 2.0, 0.0};
        const uint32_t pad = unit == ISX_INJECT_UNIT_AUTO ? (n < 1000000ull ? 2u : 0u) : (uint32_t)unit;
        rc = run_injected(p, d, segments, n, layout, pad, loud, 8);
      }
    }
  }
  if (rc == ISX_OK) rc = copy_out(host.data(), S.d_hist, (size_t)n_disc * sizeof(unsigned long long));
  rc = call_close(rc, &st);
  if (rc) return rc;
  for (int32_t k = 0; k < n_disc; ++k) hits[k] += host[(size_t)k];
  if (bin_increments) *bin_increments = st.bin_increments;
  return ISX_OK;
} catch (const std::bad_alloc&) {
  return ISX_ERR_TOO_LARGE;
}

void isx_default_order_hist_spec(const isx_config* cfg, isx_order_hist_spec* spec) {
  (void)cfg;   // (the default does not depend on the configuration: orders are counted, not scaled)
  if (!spec) return;
  std::memset(spec, 0, sizeof(*spec));
  spec->struct_size = (uint32_t)sizeof(isx_order_hist_spec);
  spec->n_orders = 512; spec->n_dz = 8;
}

int isx_order_hist_device(const isx_config* cfg, const isx_order_hist_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                          uint64_t* d_hist, uint64_t* d_port_dz, uint64_t* d_counts) {
  // (what needs no device is answered first: a NULL argument or a refused spec is the same answer with and without one)
  if (!cfg || !spec || !d_hist || !d_counts) return ISX_ERR_BAD_ARG;
  const int bad = check_order_spec(spec);
  if (bad) return bad;
  if (spec->n_dz > 0 && !d_port_dz) return ISX_ERR_BAD_ARG;
  if (!S.init) return not_initialised();
  const OrderSink oh{spec, (unsigned long long*)d_hist, spec->n_dz > 0 ? (unsigned long long*)d_port_dz : nullptr,
                     (unsigned long long*)d_counts};
  return enqueue({.sink = SINK_ORDER, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .oh = &oh});
}

int isx_order_hist(const isx_config* cfg, const isx_order_hist_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                   uint64_t* hist, uint64_t* port_dz, isx_order_hist_counts* counts, isx_stats* stats) {
  if (!cfg || !spec || !hist) return ISX_ERR_BAD_ARG;
  if (!config_abi_ok(cfg)) return ISX_ERR_BAD_CONFIG;
  int rc = check_order_spec(spec);
  if (rc) return rc;
  if (spec->n_dz > 0 && !port_dz) return ISX_ERR_BAD_ARG;
  if (!S.init) return not_initialised();
  const size_t nh = 4 * (size_t)spec->n_orders, nd = (size_t)spec->n_orders * spec->n_dz, words = nh + nd + 5;
  rc = call_open(words);
  if (rc) return rc;
  // the call's accumulators in the pooled histogram: the four histograms | the port's dz | the five counters
  const OrderSink oh{spec, S.d_hist, nd ? S.d_hist + nh : nullptr, S.d_hist + nh + nd};
  rc = zero_hist(words);
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_ORDER, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .oh = &oh});
  if (rc == ISX_OK) rc = stage_result(S.d_hist, words * sizeof(unsigned long long));
  rc = call_close(rc, stats);
  if (rc == ISX_OK) {
    const unsigned long long* h = reinterpret_cast<const unsigned long long*>(S.h_pin + 64);
    std::memcpy(hist, h, nh * 8);
    if (nd) std::memcpy(port_dz, h + nh, nd * 8);
    if (counts) {
      for (int c = 0; c < 4; ++c) counts->overflow[c] = h[nh + nd + c];
      counts->dz_outside = h[nh + nd + 4];
    }
  }
  return rc;
}

int isx_order_reweight(const isx_config* cfg, const isx_order_hist_spec* spec, const uint64_t* hist,
                       const isx_order_hist_counts* counts, uint64_t launched, const double* rho, int32_t n_rho, double* fraction,
                       double* sigma) {
  if (!cfg || !spec || !hist || !counts || n_rho < 0 || (n_rho > 0 && (!rho || !fraction))) return ISX_ERR_BAD_ARG;
  if (!config_abi_ok(cfg)) return ISX_ERR_BAD_CONFIG;
  const int rc = check_order_spec(spec);
  if (rc) return rc;
  const double rho0 = cfg->reflectance;
  if (cfg->source_model != ISX_SOURCE_PENCIL || counts->overflow[0] != 0 || !(rho0 > 0) || launched == 0) return ISX_ERR_BAD_CONFIG;
  for (int32_t i = 0; i < n_rho; ++i)
    if (!(std::isfinite(rho[i]) && rho[i] >= 0)) return ISX_ERR_BAD_ARG;
  const double n = (double)launched;
  for (int32_t i = 0; i < n_rho; ++i) {
    const double q = rho[i] / rho0;
    double s1 = 0, s2 = 0;
    for (int32_t k = 0; k < spec->n_orders; ++k) {
      const double w = std::pow(q, (double)k), h = (double)hist[k];
      s1 += h * w;
      s2 += h * w * w;
    }
    fraction[i] = s1 / n;
    if (sigma) {
      const double var = s2 - s1 * s1 / n;
      sigma[i] = std::sqrt(var > 0 ? var : 0.0) / n;
    }
  }
  return ISX_OK;
}

void isx_default_wall_patch_spec(const isx_config* cfg, isx_wall_patch_spec* spec) {
  (void)cfg;   // (the default does not depend on the configuration: no patches)
  if (!spec) return;
  std::memset(spec, 0, sizeof(*spec));
  spec->struct_size = (uint32_t)sizeof(isx_wall_patch_spec);
}

int isx_wall_patch_cap(const isx_config* cfg, const double dir[3], double half_angle_deg, double reflectance, isx_wall_patch* out) {
  if (!cfg || !dir || !out) return ISX_ERR_BAD_ARG;
  if (!config_abi_ok(cfg)) return ISX_ERR_BAD_CONFIG;
  const double mag = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
  if (!(mag > 0) || !std::isfinite(mag) || !(half_angle_deg >= 0.0 && half_angle_deg <= 180.0) ||
      !(reflectance >= 0.0 && reflectance <= 1.0))
    return ISX_ERR_BAD_CONFIG;
  for (int k = 0; k < 3; ++k) out->axis[k] = dir[k] / mag;
  out->min_dot = cfg->r_in * std::cos(half_angle_deg * M_PI / 180.0);
  out->reflectance = reflectance;
  return ISX_OK;
}

int isx_wall_patches_device(const isx_config* cfg, const isx_wall_patch_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                            uint64_t* d_arrivals, uint64_t* d_absorbed) {
  // (what needs no device is answered first: a NULL argument or a refused spec is the same answer with and without one)
  if (!cfg || !spec || !d_arrivals || !d_absorbed) return ISX_ERR_BAD_ARG;
  const int bad = check_patch_call(cfg, spec);
  if (bad) return bad;
  if (!S.init) return not_initialised();
  const PatchSink wp{spec, (unsigned long long*)d_arrivals, (unsigned long long*)d_absorbed};
  return enqueue({.sink = SINK_PATCH, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .wp = &wp});
}

int isx_wall_patches(const isx_config* cfg, const isx_wall_patch_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                     uint64_t* arrivals, uint64_t* absorbed, isx_stats* stats) {
  if (!cfg || !spec || !arrivals || !absorbed) return ISX_ERR_BAD_ARG;
  int rc = check_patch_call(cfg, spec);
  if (rc) return rc;
  if (!S.init) return not_initialised();
  const size_t nc = (size_t)spec->n_patches + 2, words = 2 * nc;
  rc = call_open(words);
  if (rc) return rc;
  // the call's accumulators in the pooled histogram: arrivals | absorbed
  const PatchSink wp{spec, S.d_hist, S.d_hist + nc};
  rc = zero_hist(words);
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_PATCH, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .wp = &wp});
  if (rc == ISX_OK) rc = stage_result(S.d_hist, words * sizeof(unsigned long long));
  rc = call_close(rc, stats);
  if (rc == ISX_OK) {
    const unsigned long long* h = reinterpret_cast<const unsigned long long*>(S.h_pin + 64);
    std::memcpy(arrivals, h, nc * 8);
    std::memcpy(absorbed, h + nc, nc * 8);
  }
  return rc;
}

void isx_default_beam_spec(const isx_config* cfg, isx_beam_spec* spec) {
  if (!spec) return;
  std::memset(spec, 0, sizeof(*spec));
  spec->struct_size = (uint32_t)sizeof(isx_beam_spec);
  spec->cos_min = 1.0;
  spec->angular_law = ISX_BEAM_UNIFORM;
  if (!cfg) return;
  for (int k = 0; k < 3; ++k) spec->origin[k] = cfg->src[k];
  if (!beam_frame(cfg->dir, spec->axis, spec->e1, spec->e2))
    for (int k = 0; k < 3; ++k) spec->axis[k] = spec->e1[k] = spec->e2[k] = 0.0;
}

int isx_beam_cone(const isx_config* cfg, const double origin[3], const double dir[3], double radius, double half_angle_deg,
                  int32_t law, isx_beam_spec* out) {
  if (!cfg || !origin || !dir || !out) return ISX_ERR_BAD_ARG;
  if (!config_abi_ok(cfg)) return ISX_ERR_BAD_CONFIG;
  if (law != ISX_BEAM_UNIFORM && law != ISX_BEAM_LAMBERT) return ISX_ERR_BAD_CONFIG;
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(origin[k]) || !std::isfinite(dir[k])) return ISX_ERR_BAD_CONFIG;
  if (!std::isfinite(radius) || radius < 0.0) return ISX_ERR_BAD_CONFIG;
  if (!(half_angle_deg >= 0.0 && half_angle_deg <= (law == ISX_BEAM_LAMBERT ? 90.0 : 180.0))) return ISX_ERR_BAD_CONFIG;
  isx_beam_spec s;
  std::memset(&s, 0, sizeof(s));
  s.struct_size = (uint32_t)sizeof(isx_beam_spec);
  if (!beam_frame(dir, s.axis, s.e1, s.e2)) return ISX_ERR_BAD_CONFIG;
  for (int k = 0; k < 3; ++k) s.origin[k] = origin[k];
  s.radius = radius;
  s.cos_min = half_angle_deg == 0.0 ? 1.0 : half_angle_deg == 90.0 ? 0.0 : half_angle_deg == 180.0 ? -1.0 :
              std::cos(half_angle_deg * M_PI / 180.0);
  s.angular_law = law;
  *out = s;
  return ISX_OK;
}

int isx_beam_endstates(const isx_config* cfg, const isx_beam_spec* spec, uint64_t n, uint64_t seed, uint64_t first, int32_t* status,
                       int32_t* n_points, double* last_point, double* direction, double* start_point, double* start_dir) {
  // (what needs no device is answered first: a NULL argument or a refused spec is the same answer with and without one)
  if (!cfg || !spec || !status || !n_points || !last_point || !direction) return ISX_ERR_BAD_ARG;
  int rc = check_beam_call(cfg, spec);
  if (rc) return rc;
  if (!S.init) return not_initialised();
  if (trace_join()) return ISX_ERR_HIP;   // (behind an overlapped sequence, as every entry but isx_fluxmap_device)
  if (n == 0) return ISX_OK;
  if (n > (1ull << 28)) return ISX_ERR_TOO_LARGE;
  if (first > UINT64_MAX - n) return ISX_ERR_BAD_ARG;
  Geom g;
  const isx_config cb = beam_config(*cfg, *spec);
  rc = prepare_geom(&cb, &g);
  if (rc) return rc;
  const BeamSrc b = beam_source(*spec);
  DevBuf<int32_t> b_st, b_np;
  DevBuf<double> b_lp, b_dir, b_sp, b_sd;
  HIPCHK(b_st.alloc(n)); HIPCHK(b_np.alloc(n)); HIPCHK(b_lp.alloc(n * 3)); HIPCHK(b_dir.alloc(n * 3));
  if (start_point) HIPCHK(b_sp.alloc(n * 3));
  if (start_dir) HIPCHK(b_sd.alloc(n * 3));
  const int blk = 256;
  const unsigned grid = (unsigned)((n + blk - 1) / blk);
  hipLaunchKernelGGL(isx_beam_endstates_kernel, dim3(grid), dim3(blk), 0, S.stream, g, b, seed, first, n, b_st.p, b_np.p, b_lp.p,
                     b_dir.p, b_sp.p, b_sd.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(status, b_st.p, n * 4, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemcpyAsync(n_points, b_np.p, n * 4, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemcpyAsync(last_point, b_lp.p, n * 24, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemcpyAsync(direction, b_dir.p, n * 24, hipMemcpyDeviceToHost, S.stream));
  if (start_point) HIPCHK(hipMemcpyAsync(start_point, b_sp.p, n * 24, hipMemcpyDeviceToHost, S.stream));
  if (start_dir) HIPCHK(hipMemcpyAsync(start_dir, b_sd.p, n * 24, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipStreamSynchronize(S.stream));
  return ISX_OK;
}

int isx_fluxmap_beam_device(const isx_config* cfg, const isx_beam_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                            uint64_t* d_hits) {
  if (!cfg || !spec || !d_hits) return ISX_ERR_BAD_ARG;
  const int bad = check_beam_call(cfg, spec);
  if (bad) return bad;
  if (!S.init) return not_initialised();
  return enqueue({.sink = SINK_FLUX, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray,
                 .d_hist = (unsigned long long*)d_hits, .bs = spec});
}

int isx_fluxmap_beam(const isx_config* cfg, const isx_beam_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                     uint64_t* hits, isx_stats* stats) {
  if (!cfg || !spec || !hits) return ISX_ERR_BAD_ARG;
  int rc = check_beam_call(cfg, spec);
  if (rc) return rc;
  if (!S.init) return not_initialised();
  rc = check_grid(cfg);
  if (rc) return rc;
  const size_t nb = (size_t)cfg->n_theta * cfg->n_phi, bytes = nb * sizeof(unsigned long long);
  rc = call_open(nb);
  if (rc) return rc;
  rc = zero_hist(nb);
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_FLUX, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .d_hist = S.d_hist,
                                 .bs = spec});
  if (rc == ISX_OK) rc = stage_result(S.d_hist, bytes);
  rc = call_close(rc, stats);
  if (rc == ISX_OK) fetch_result(hits, bytes);
  return rc;
}

void isx_default_baffle_spec(const isx_config* cfg, isx_baffle_spec* spec) {
  (void)cfg;
  if (!spec) return;
  std::memset(spec, 0, sizeof(*spec));
  spec->struct_size = (uint32_t)sizeof(isx_baffle_spec);
}

int isx_baffle_disc(const isx_config* cfg, const double centre[3], const double dir[3], double radius, double reflectance,
                    isx_baffle* out) {
  if (!cfg || !centre || !dir || !out) return ISX_ERR_BAD_ARG;
  if (!config_abi_ok(cfg)) return ISX_ERR_BAD_CONFIG;
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(centre[k]) || !std::isfinite(dir[k])) return ISX_ERR_BAD_CONFIG;
  if (!std::isfinite(radius) || !(radius > 0.0)) return ISX_ERR_BAD_CONFIG;
  if (!(reflectance >= 0.0 && reflectance <= 1.0)) return ISX_ERR_BAD_CONFIG;
  const double dx = dir[0], dy = dir[1], dz = dir[2];
  const double mag = std::sqrt(dx * dx + dy * dy + dz * dz);   // (prepare_geom's expression for the pencil, as isx_beam_cone)
  if (!(mag > 0) || !std::isfinite(mag)) return ISX_ERR_BAD_CONFIG;
  isx_baffle b;
  std::memset(&b, 0, sizeof(b));
  for (int k = 0; k < 3; ++k) b.centre[k] = centre[k];
  b.normal[0] = dx / mag; b.normal[1] = dy / mag; b.normal[2] = dz / mag;
  b.radius = radius;
  b.reflectance = reflectance;
  *out = b;
  return ISX_OK;
}

int isx_baffle_endstates(const isx_config* cfg, const isx_baffle_spec* spec, uint64_t n, uint64_t seed, uint64_t first,
                         int32_t* status, int32_t* n_points, double* last_point, double* direction, int32_t* last_baffle) {
  // (what needs no device is answered first: a NULL argument or a refused spec is the same answer with and without one)
  if (!cfg || !spec || !status || !n_points || !last_point || !direction) return ISX_ERR_BAD_ARG;
  int rc = check_baffle_call(cfg, spec);
  if (rc) return rc;
  if (!S.init) return not_initialised();
  if (trace_join()) return ISX_ERR_HIP;   // (behind an overlapped sequence, as every entry but isx_fluxmap_device)
  if (n == 0) return ISX_OK;
  if (n > (1ull << 28)) return ISX_ERR_TOO_LARGE;
  if (first > UINT64_MAX - n) return ISX_ERR_BAD_ARG;
  Geom g;
  rc = prepare_geom(cfg, &g);
  if (rc) return rc;
  const BaffleTab t = baffle_table(*cfg, *spec, nullptr);
  DevBuf<int32_t> b_st, b_np, b_lb;
  DevBuf<double> b_lp, b_dir;
  HIPCHK(b_st.alloc(n)); HIPCHK(b_np.alloc(n)); HIPCHK(b_lp.alloc(n * 3)); HIPCHK(b_dir.alloc(n * 3));
  if (last_baffle) HIPCHK(b_lb.alloc(n));
  const int blk = 256;
  const unsigned grid = (unsigned)((n + blk - 1) / blk);
  hipLaunchKernelGGL(isx_baffle_endstates_kernel, dim3(grid), dim3(blk), 0, S.stream, g, t, seed, first, n, b_st.p, b_np.p, b_lp.p,
                     b_dir.p, b_lb.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(status, b_st.p, n * 4, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemcpyAsync(n_points, b_np.p, n * 4, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemcpyAsync(last_point, b_lp.p, n * 24, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemcpyAsync(direction, b_dir.p, n * 24, hipMemcpyDeviceToHost, S.stream));
  if (last_baffle) HIPCHK(hipMemcpyAsync(last_baffle, b_lb.p, n * 4, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipStreamSynchronize(S.stream));
  return ISX_OK;
}

int isx_fluxmap_baffle_device(const isx_config* cfg, const isx_baffle_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                              uint64_t* d_hits, uint64_t* d_counts) {
  if (!cfg || !spec || !d_hits || !d_counts) return ISX_ERR_BAD_ARG;
  int bad = check_baffle_call(cfg, spec);
  if (bad == ISX_OK) bad = check_baffle_grid(cfg);
  if (bad) return bad;
  if (!S.init) return not_initialised();
  const BaffleSink bf{spec, (unsigned long long*)d_counts};
  return enqueue({.sink = SINK_FLUX, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray,
                 .d_hist = (unsigned long long*)d_hits, .bf = &bf});
}

int isx_fluxmap_baffle(const isx_config* cfg, const isx_baffle_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                       uint64_t* hits, isx_baffle_counts* counts, isx_stats* stats) {
  if (!cfg || !spec || !hits) return ISX_ERR_BAD_ARG;
  int rc = check_baffle_call(cfg, spec);
  if (rc == ISX_OK) rc = check_baffle_grid(cfg);
  if (rc) return rc;
  if (!S.init) return not_initialised();
  // the histogram and, behind it, the 16 counters: one device block, one staged result
  const size_t nb = (size_t)cfg->n_theta * cfg->n_phi, nc = 4 * kMaxBaffles, bytes = (nb + nc) * sizeof(unsigned long long);
  rc = call_open(nb + nc);
  if (rc) return rc;
  rc = zero_hist(nb + nc);
  const BaffleSink bf{spec, S.d_hist + nb};
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_FLUX, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .d_hist = S.d_hist,
                                 .bf = &bf});
  if (rc == ISX_OK) rc = stage_result(S.d_hist, bytes);
  rc = call_close(rc, stats);
  if (rc == ISX_OK) {
    fetch_result(hits, nb * sizeof(unsigned long long));
    if (counts) std::memcpy(counts, reinterpret_cast<const unsigned long long*>(S.h_pin + 64) + nb, nc * sizeof(unsigned long long));
  }
  return rc;
}

void isx_default_scene_spec(const isx_config* cfg, isx_scene_spec* spec) {
  if (!spec) return;
  std::memset(spec, 0, sizeof(*spec));
  spec->struct_size = (uint32_t)sizeof(isx_scene_spec);
  isx_default_beam_spec(cfg, &spec->beam);
  isx_default_baffle_spec(cfg, &spec->baffles);
  isx_default_wall_patch_spec(cfg, &spec->patches);
}

int isx_scene_endstates(const isx_config* cfg, const isx_scene_spec* spec, uint64_t n, uint64_t seed, uint64_t first, int32_t* status,
                        int32_t* n_points, double* last_point, double* direction, double* start_point, double* start_dir,
                        int32_t* last_baffle, int32_t* last_class) {
  // (what needs no device is answered first: a NULL argument or a refused spec is the same answer with and without one)
  if (!cfg || !spec || !status || !n_points || !last_point || !direction) return ISX_ERR_BAD_ARG;
  int rc = check_scene_call(cfg, spec, false);
  if (rc) return rc;
  if (!S.init) return not_initialised();
  if (trace_join()) return ISX_ERR_HIP;   // (behind an overlapped sequence, as every entry but isx_fluxmap_device)
  if (n == 0) return ISX_OK;
  if (n > (1ull << 28)) return ISX_ERR_TOO_LARGE;
  if (first > UINT64_MAX - n) return ISX_ERR_BAD_ARG;
  Geom g;
  const isx_config cb = beam_config(*cfg, spec->beam);
  rc = prepare_geom(&cb, &g);
  if (rc) return rc;
  const BeamSrc b = beam_source(spec->beam);
  const BaffleTab t = baffle_table(cb, spec->baffles, nullptr);
  const PatchTab pt = patch_table(cb, spec->patches);
  DevBuf<int32_t> b_st, b_np, b_lb, b_lc;
  DevBuf<double> b_lp, b_dir, b_sp, b_sd;
  HIPCHK(b_st.alloc(n)); HIPCHK(b_np.alloc(n)); HIPCHK(b_lp.alloc(n * 3)); HIPCHK(b_dir.alloc(n * 3));
  if (start_point) HIPCHK(b_sp.alloc(n * 3));
  if (start_dir) HIPCHK(b_sd.alloc(n * 3));
  if (last_baffle) HIPCHK(b_lb.alloc(n));
  if (last_class) HIPCHK(b_lc.alloc(n));
  const int blk = 256;
  const unsigned grid = (unsigned)((n + blk - 1) / blk);
  hipLaunchKernelGGL(isx_scene_endstates_kernel, dim3(grid), dim3(blk), 0, S.stream, g, pt, b, t, seed, first, n, b_st.p, b_np.p,
                     b_lp.p, b_dir.p, b_sp.p, b_sd.p, b_lb.p, b_lc.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(status, b_st.p, n * 4, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemcpyAsync(n_points, b_np.p, n * 4, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemcpyAsync(last_point, b_lp.p, n * 24, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemcpyAsync(direction, b_dir.p, n * 24, hipMemcpyDeviceToHost, S.stream));
  if (start_point) HIPCHK(hipMemcpyAsync(start_point, b_sp.p, n * 24, hipMemcpyDeviceToHost, S.stream));
  if (start_dir) HIPCHK(hipMemcpyAsync(start_dir, b_sd.p, n * 24, hipMemcpyDeviceToHost, S.stream));
  if (last_baffle) HIPCHK(hipMemcpyAsync(last_baffle, b_lb.p, n * 4, hipMemcpyDeviceToHost, S.stream));
  if (last_class) HIPCHK(hipMemcpyAsync(last_class, b_lc.p, n * 4, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipStreamSynchronize(S.stream));
  return ISX_OK;
}

int isx_fluxmap_scene_device(const isx_config* cfg, const isx_scene_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                             uint64_t* d_hits, uint64_t* d_counts) {
  if (!cfg || !spec || !d_hits || !d_counts) return ISX_ERR_BAD_ARG;
  const int bad = check_scene_call(cfg, spec, true);
  if (bad) return bad;
  if (!S.init) return not_initialised();
  const SceneSink sc{spec, (unsigned long long*)d_counts};
  return enqueue({.sink = SINK_FLUX, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray,
                 .d_hist = (unsigned long long*)d_hits, .sc = &sc});
}

int isx_fluxmap_scene(const isx_config* cfg, const isx_scene_spec* spec, uint64_t n_rays, uint64_t seed, uint64_t first_ray,
                      uint64_t* hits, isx_scene_counts* counts, isx_stats* stats) {
  if (!cfg || !spec || !hits) return ISX_ERR_BAD_ARG;
  int rc = check_scene_call(cfg, spec, true);
  if (rc) return rc;
  if (!S.init) return not_initialised();
  // the histogram and, behind it, the 36 counters: one device block, one staged result
  const size_t nb = (size_t)cfg->n_theta * cfg->n_phi, nc = kSceneWords, bytes = (nb + nc) * sizeof(unsigned long long);
  rc = call_open(nb + nc);
  if (rc) return rc;
  rc = zero_hist(nb + nc);
  const SceneSink sc{spec, S.d_hist + nb};
  if (rc == ISX_OK) rc = enqueue({.sink = SINK_FLUX, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray, .d_hist = S.d_hist,
                                 .sc = &sc});
  if (rc == ISX_OK) rc = stage_result(S.d_hist, bytes);
  rc = call_close(rc, stats);
  if (rc == ISX_OK) {
    fetch_result(hits, nb * sizeof(unsigned long long));
    if (counts) std::memcpy(counts, reinterpret_cast<const unsigned long long*>(S.h_pin + 64) + nb, nc * sizeof(unsigned long long));
  }
  return rc;
}

void isx_default_response_spec(const isx_config* cfg, isx_response_spec* spec) {
  (void)cfg;   // (the default does not depend on the configuration: the axes are the source's sample space)
  if (!spec) return;
  std::memset(spec, 0, sizeof(*spec));
  spec->struct_size = (uint32_t)sizeof(isx_response_spec);
  spec->n[0] = 1; spec->n[1] = 1; spec->n[2] = 6; spec->n[3] = 12;
}

int isx_scene_response_device(const isx_config* cfg, const isx_scene_spec* scene, const isx_response_spec* rspec, uint64_t n_rays,
                              uint64_t seed, uint64_t first_ray, uint64_t* d_response, uint64_t* d_counts) {
  return scene_map_call({.sink = SINK_RESPONSE, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray}, scene,
                        SceneMap{SINK_RESPONSE, rspec, (unsigned long long*)d_response, nullptr}, d_counts, true, nullptr);
}

int isx_scene_response(const isx_config* cfg, const isx_scene_spec* scene, const isx_response_spec* rspec, uint64_t n_rays,
                       uint64_t seed, uint64_t first_ray, uint64_t* response, isx_scene_counts* counts, isx_stats* stats) {
  return scene_map_call({.sink = SINK_RESPONSE, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray}, scene,
                        SceneMap{SINK_RESPONSE, rspec, (unsigned long long*)response, nullptr}, (uint64_t*)counts, false, stats);
}

int isx_response_reweight(const isx_response_spec* rspec, const uint64_t* response, const double* weight, double* fraction,
                          double* sigma) {
  if (!rspec || !response || !weight || !fraction) return ISX_ERR_BAD_ARG;
  const int rc = check_response_spec(rspec);
  if (rc) return rc;
  const size_t B = response_bins(*rspec);
  for (size_t b = 0; b < B; ++b)
    if (!(std::isfinite(weight[b]) && weight[b] >= 0)) return ISX_ERR_BAD_ARG;
  std::vector<double> nb(B);
  double L = 0;
  for (size_t b = 0; b < B; ++b) {
    uint64_t col = 0;
    for (int f = 0; f < ISX_RESPONSE_FATES; ++f) col += response[(size_t)f * B + b];
    nb[b] = (double)col;
    L += weight[b] * nb[b];
  }
  if (!(L > 0)) return ISX_ERR_BAD_CONFIG;
  for (int f = 0; f < ISX_RESPONSE_FATES; ++f) {
    const uint64_t* row = response + (size_t)f * B;
    double s = 0;
    for (size_t b = 0; b < B; ++b) s += weight[b] * (double)row[b];
    const double F = s / L;
    fraction[f] = F;
    if (sigma) {
      double v = 0;
      for (size_t b = 0; b < B; ++b) {
        const double h = (double)row[b];
        v += weight[b] * weight[b] * (h * (1.0 - F) * (1.0 - F) + (nb[b] - h) * F * F);
      }
      sigma[f] = std::sqrt(v) / L;
    }
  }
  return ISX_OK;
}

int isx_view_frame(const isx_config* cfg, const isx_scene_spec* scene, int32_t patch, int32_t n_u, int32_t n_v, double half_extent,
                   isx_view_spec* out) {
  if (!cfg || !scene || !out) return ISX_ERR_BAD_ARG;
  int rc = check_scene_call(cfg, scene, false);
  if (rc) return rc;
  if (patch < 0 || patch >= scene->patches.n_patches) return ISX_ERR_BAD_CONFIG;
  isx_view_spec s;
  std::memset(&s, 0, sizeof(s));
  s.struct_size = (uint32_t)sizeof(isx_view_spec);
  s.patch = patch; s.n_u = n_u; s.n_v = n_v; s.half_extent = half_extent;
  const double* a = scene->patches.patch[patch].axis;
  double unit[3];   // (the frame rule normalises its axis; the spec's axis is the patch's, bit for bit)
  if (!beam_frame(a, unit, s.e1, s.e2)) return ISX_ERR_BAD_CONFIG;
  for (int i = 0; i < 3; ++i) s.axis[i] = a[i];
  rc = check_view_spec(&s, scene->patches.n_patches);
  if (rc) return rc;
  *out = s;
  return ISX_OK;
}

int isx_scene_view_device(const isx_config* cfg, const isx_scene_spec* scene, const isx_view_spec* vspec, uint64_t n_rays,
                          uint64_t seed, uint64_t first_ray, uint64_t* d_view, uint64_t* d_view_counts, uint64_t* d_scene_counts) {
  return scene_map_call({.sink = SINK_VIEW, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray}, scene,
                        SceneMap{SINK_VIEW, vspec, (unsigned long long*)d_view, (unsigned long long*)d_view_counts}, d_scene_counts,
                        true, nullptr);
}

int isx_scene_view(const isx_config* cfg, const isx_scene_spec* scene, const isx_view_spec* vspec, uint64_t n_rays, uint64_t seed,
                   uint64_t first_ray, uint64_t* view, isx_view_counts* view_counts, isx_scene_counts* scene_counts, isx_stats* stats) {
  return scene_map_call({.sink = SINK_VIEW, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray}, scene,
                        SceneMap{SINK_VIEW, vspec, (unsigned long long*)view, (unsigned long long*)view_counts},
                        (uint64_t*)scene_counts, false, stats);
}

int isx_view_reweight(const isx_view_spec* vspec, const uint64_t* view, const isx_view_counts* view_counts, uint64_t launched,
                      const double* weight, double direct_weight, double* signal, double* sigma) {
  if (!vspec || !view || !view_counts || !weight || !signal) return ISX_ERR_BAD_ARG;
  const int rc = check_view_spec(vspec, -1);
  if (rc) return rc;
  if (launched == 0) return ISX_ERR_BAD_CONFIG;
  const size_t B = view_bins(*vspec);
  for (size_t b = 0; b < B; ++b)
    if (!(std::isfinite(weight[b]) && weight[b] >= 0)) return ISX_ERR_BAD_ARG;
  if (!(std::isfinite(direct_weight) && direct_weight >= 0)) return ISX_ERR_BAD_ARG;
  double s1 = 0, s2 = 0;
  for (size_t b = 0; b < B; ++b) {
    const double w = weight[b], c = (double)view[b];
    s1 += w * c;
    s2 += w * w * c;
  }
  const double nd = (double)view_counts->direct, nl = (double)launched;
  s1 += direct_weight * nd;
  s2 += direct_weight * direct_weight * nd;
  *signal = s1 / nl;
  if (sigma) {
    const double var = s2 - s1 * s1 / nl;
    *sigma = std::sqrt(var > 0 ? var : 0.0) / nl;
  }
  return ISX_OK;
}

int isx_view_weight_fov(const isx_view_spec* vspec, double half_angle_deg, double* weight) {
  if (!vspec || !weight) return ISX_ERR_BAD_ARG;
  const int rc = check_view_spec(vspec, -1);
  if (rc) return rc;
  if (!std::isfinite(half_angle_deg) || half_angle_deg < 0.0 || half_angle_deg > 90.0) return ISX_ERR_BAD_CONFIG;
  const double s = half_angle_deg == 90.0 ? 1.0 : std::sin(half_angle_deg * 3.14159265358979323846 / 180.0);
  const double h = vspec->half_extent, du = 2.0 * h / (double)vspec->n_u, dv = 2.0 * h / (double)vspec->n_v;
  for (int iv = 0; iv < vspec->n_v; ++iv) {
    const double vc = -h + ((double)iv + 0.5) * dv;
    for (int iu = 0; iu < vspec->n_u; ++iu) {
      const double uc = -h + ((double)iu + 0.5) * du;
      weight[(size_t)iv * vspec->n_u + iu] = uc * uc + vc * vc <= s * s ? 1.0 : 0.0;
    }
  }
  return ISX_OK;
}

int isx_patch_field_frame(const isx_config* cfg, const isx_scene_spec* scene, int32_t patch, int32_t n_x, int32_t n_y, int32_t n_u,
                          int32_t n_v, double half_extent, isx_patch_field_spec* out) {
  if (!cfg || !scene || !out) return ISX_ERR_BAD_ARG;
  int rc = check_scene_call(cfg, scene, false);
  if (rc) return rc;
  if (patch < 0 || patch >= scene->patches.n_patches) return ISX_ERR_BAD_CONFIG;
  isx_patch_field_spec s;
  std::memset(&s, 0, sizeof(s));
  s.struct_size = (uint32_t)sizeof(isx_patch_field_spec);
  s.patch = patch; s.n_x = n_x; s.n_y = n_y; s.n_u = n_u; s.n_v = n_v; s.half_extent = half_extent;
  const double* a = scene->patches.patch[patch].axis;
  double unit[3];   // (isx_view_frame's rule: the spec's axis is the patch's, bit for bit)
  if (!beam_frame(a, unit, s.e1, s.e2)) return ISX_ERR_BAD_CONFIG;
  for (int i = 0; i < 3; ++i) s.axis[i] = a[i];
  // (a cap of half-angle alpha fills the unit disc: 1 / sin(alpha / 2); a cap of zero angle has no scale and is refused below)
  s.pos_scale = 1.0 / std::sqrt(0.5 * (1.0 - scene->patches.patch[patch].min_dot / cfg->r_in));
  rc = check_patch_field_spec(&s, scene->patches.n_patches);
  if (rc) return rc;
  *out = s;
  return ISX_OK;
}

int isx_scene_patch_field_device(const isx_config* cfg, const isx_scene_spec* scene, const isx_patch_field_spec* fspec, uint64_t n_rays,
                                 uint64_t seed, uint64_t first_ray, uint64_t* d_field, uint64_t* d_field_counts,
                                 uint64_t* d_scene_counts) {
  return scene_map_call({.sink = SINK_FIELD, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray}, scene,
                        SceneMap{SINK_FIELD, fspec, (unsigned long long*)d_field, (unsigned long long*)d_field_counts}, d_scene_counts,
                        true, nullptr);
}

int isx_scene_patch_field(const isx_config* cfg, const isx_scene_spec* scene, const isx_patch_field_spec* fspec, uint64_t n_rays,
                          uint64_t seed, uint64_t first_ray, uint64_t* field, isx_patch_field_counts* field_counts,
                          isx_scene_counts* scene_counts, isx_stats* stats) {
  return scene_map_call({.sink = SINK_FIELD, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray}, scene,
                        SceneMap{SINK_FIELD, fspec, (unsigned long long*)field, (unsigned long long*)field_counts},
                        (uint64_t*)scene_counts, false, stats);
}

int isx_patch_field_marginals(const isx_patch_field_spec* fspec, const uint64_t* field, uint64_t* pos_map, uint64_t* dir_map) {
  if (!fspec || !field) return ISX_ERR_BAD_ARG;
  const int rc = check_patch_field_spec(fspec, -1);
  if (rc) return rc;
  const size_t np = (size_t)fspec->n_x * (size_t)fspec->n_y, nd = (size_t)fspec->n_u * (size_t)fspec->n_v;
  if (pos_map) std::memset(pos_map, 0, np * sizeof(uint64_t));
  if (dir_map) std::memset(dir_map, 0, nd * sizeof(uint64_t));
  for (size_t p = 0; p < np; ++p)
    for (size_t k = 0; k < nd; ++k) {
      const uint64_t c = field[p * nd + k];
      if (pos_map) pos_map[p] += c;
      if (dir_map) dir_map[k] += c;
    }
  return ISX_OK;
}

void isx_default_scene_order_spec(const isx_config* cfg, isx_scene_order_spec* ospec) {
  (void)cfg;   // (the default does not depend on the configuration)
  if (!ospec) return;
  std::memset(ospec, 0, sizeof(*ospec));
  ospec->struct_size = (uint32_t)sizeof(isx_scene_order_spec);
  ospec->n_orders = 512;
}

int isx_scene_order_hist_device(const isx_config* cfg, const isx_scene_spec* scene, const isx_scene_order_spec* ospec,
                                uint64_t n_rays, uint64_t seed, uint64_t first_ray, uint64_t* d_hist, uint64_t* d_order_counts,
                                uint64_t* d_scene_counts) {
  return scene_map_call({.sink = SINK_SORDER, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray}, scene,
                        SceneMap{SINK_SORDER, ospec, (unsigned long long*)d_hist, (unsigned long long*)d_order_counts}, d_scene_counts,
                        true, nullptr);
}

int isx_scene_order_hist(const isx_config* cfg, const isx_scene_spec* scene, const isx_scene_order_spec* ospec, uint64_t n_rays,
                         uint64_t seed, uint64_t first_ray, uint64_t* hist, isx_scene_order_counts* order_counts,
                         isx_scene_counts* scene_counts, isx_stats* stats) {
  return scene_map_call({.sink = SINK_SORDER, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray}, scene,
                        SceneMap{SINK_SORDER, ospec, (unsigned long long*)hist, (unsigned long long*)order_counts},
                        (uint64_t*)scene_counts, false, stats);
}

int isx_scene_order_reweight(const isx_config* cfg, const isx_scene_spec* scene, const isx_scene_order_spec* ospec,
                             const uint64_t* hist, const isx_scene_order_counts* counts, uint64_t launched, const double* scale,
                             int32_t n_scale, double* fraction, double* sigma) {
  if (!cfg || !scene || !ospec || !hist || !counts || n_scale < 0 || (n_scale > 0 && (!scale || !fraction))) return ISX_ERR_BAD_ARG;
  int rc = check_scene_call(cfg, scene, false);
  if (rc == ISX_OK) rc = check_scene_order_spec(ospec);
  if (rc) return rc;
  for (int f = 0; f < ISX_RESPONSE_FATES; ++f)
    if (counts->overflow[f] != 0) return ISX_ERR_BAD_CONFIG;
  if (launched == 0) return ISX_ERR_BAD_CONFIG;
  // rho_f per absorbing slot; -1: a slot the scene cannot fill
  const int P = scene->patches.n_patches, nbaf = scene->baffles.n_baffles;
  double rho[kRespPort];
  for (int f = 0; f < kRespPort; ++f) rho[f] = -1.0;
  for (int f = 0; f < P; ++f) rho[f] = scene->patches.patch[f].reflectance;
  rho[P] = rho[P + 1] = cfg->reflectance;
  for (int b = 0; b < nbaf; ++b) rho[kRespBaffle0 + 2 * b] = rho[kRespBaffle0 + 2 * b + 1] = scene->baffles.baffle[b].reflectance;
  for (int32_t i = 0; i < n_scale; ++i) {
    const double t = scale[i];
    if (!(std::isfinite(t) && t >= 0)) return ISX_ERR_BAD_ARG;
    for (int f = 0; f < kRespPort; ++f)
      if (rho[f] >= 0 && t * rho[f] > 1.0) return ISX_ERR_BAD_ARG;
  }
  const double n = (double)launched;
  const size_t K = (size_t)ospec->n_orders;
  for (int32_t i = 0; i < n_scale; ++i) {
    const double t = scale[i];
    for (int f = 0; f < ISX_RESPONSE_FATES; ++f) {
      const uint64_t* row = hist + (size_t)f * K;
      double* frac = fraction + (size_t)i * ISX_RESPONSE_FATES + f;
      double* sig = sigma ? sigma + (size_t)i * ISX_RESPONSE_FATES + f : nullptr;
      double s1 = 0, s2 = 0;
      if (f >= kRespPort) {
        for (size_t k = 0; k < K; ++k) {
          const double w = std::pow(t, (double)k), h = (double)row[k];
          s1 += h * w;
          s2 += h * w * w;
        }
      } else if (rho[f] < 0) {
        // (nothing can be absorbed there)
      } else if (rho[f] == 1.0) {
        s1 = s2 = t == 1.0 ? 0.0 : std::numeric_limits<double>::quiet_NaN();
      } else {
        const double a = (1.0 - t * rho[f]) / (1.0 - rho[f]);
        for (size_t k = 1; k < K; ++k) {
          const double w = a * std::pow(t, (double)k - 1.0), h = (double)row[k];
          s1 += h * w;
          s2 += h * w * w;
        }
      }
      *frac = s1 / n;
      if (sig) {
        const double var = s2 - s1 * s1 / n;
        *sig = std::isnan(var) ? var : std::sqrt(var > 0 ? var : 0.0) / n;
      }
    }
  }
  return ISX_OK;
}

int isx_scene_order_moments(const isx_scene_order_spec* ospec, const uint64_t* hist, const isx_scene_order_counts* counts,
                            double* mean, double* sd) {
  if (!ospec || !hist || !counts) return ISX_ERR_BAD_ARG;
  const int rc = check_scene_order_spec(ospec);
  if (rc) return rc;
  const size_t K = (size_t)ospec->n_orders;
  for (int f = 0; f < ISX_RESPONSE_FATES; ++f) {
    const uint64_t* row = hist + (size_t)f * K;
    double N = 0, A = 0, B = 0;
    for (size_t k = 0; k < K; ++k) {
      const double h = (double)row[k], x = (double)k;
      N += h;
      A += x * h;
      B += x * x * h;
    }
    double m = std::numeric_limits<double>::quiet_NaN(), d = m;
    if (N > 0 && counts->overflow[f] == 0) {
      m = A / N;
      const double var = B / N - m * m;
      d = std::sqrt(var > 0 ? var : 0.0);
    }
    if (mean) mean[f] = m;
    if (sd) sd[f] = d;
  }
  return ISX_OK;
}

void isx_default_scene_path_spec(const isx_config* cfg, isx_scene_path_spec* pspec) {
  if (!pspec) return;
  std::memset(pspec, 0, sizeof(*pspec));
  pspec->struct_size = (uint32_t)sizeof(isx_scene_path_spec);
  pspec->n_bins = 1024;
  pspec->bin_cm = cfg ? cfg->r_in / 4 : 0.0;
}

int isx_scene_path_hist_device(const isx_config* cfg, const isx_scene_spec* scene, const isx_scene_path_spec* pspec, uint64_t n_rays,
                               uint64_t seed, uint64_t first_ray, uint64_t* d_hist, uint64_t* d_path_counts,
                               uint64_t* d_scene_counts) {
  return scene_map_call({.sink = SINK_SPATH, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray}, scene,
                        SceneMap{SINK_SPATH, pspec, (unsigned long long*)d_hist, (unsigned long long*)d_path_counts}, d_scene_counts,
                        true, nullptr);
}

int isx_scene_path_hist(const isx_config* cfg, const isx_scene_spec* scene, const isx_scene_path_spec* pspec, uint64_t n_rays,
                        uint64_t seed, uint64_t first_ray, uint64_t* hist, isx_scene_path_counts* path_counts,
                        isx_scene_counts* scene_counts, isx_stats* stats) {
  return scene_map_call({.sink = SINK_SPATH, .c = cfg, .n = n_rays, .seed = seed, .first = first_ray}, scene,
                        SceneMap{SINK_SPATH, pspec, (unsigned long long*)hist, (unsigned long long*)path_counts},
                        (uint64_t*)scene_counts, false, stats);
}

int isx_scene_path_moments(const isx_scene_path_spec* pspec, const uint64_t* hist, const isx_scene_path_counts* counts,
                           double* mean_cm, double* sd_cm) {
  if (!pspec || !hist || !counts) return ISX_ERR_BAD_ARG;
  const int rc = check_scene_path_spec(pspec);
  if (rc) return rc;
  const size_t K = (size_t)pspec->n_bins;
  for (int f = 0; f < ISX_RESPONSE_FATES; ++f) {
    const uint64_t* row = hist + (size_t)f * K;
    double N = 0, A = 0, B = 0;
    for (size_t k = 0; k < K; ++k) {
      const double h = (double)row[k], x = ((double)k + 0.5) * pspec->bin_cm;
      N += h;
      A += x * h;
      B += x * x * h;
    }
    double m = std::numeric_limits<double>::quiet_NaN(), d = m;
    if (N > 0 && counts->overflow[f] == 0) {
      m = A / N;
      const double var = B / N - m * m;
      d = std::sqrt(var > 0 ? var : 0.0);
    }
    if (mean_cm) mean_cm[f] = m;
    if (sd_cm) sd_cm[f] = d;
  }
  return ISX_OK;
}

int isx_scene_path_decay(const isx_scene_path_spec* pspec, const uint64_t* hist, const isx_scene_path_counts* counts, int32_t f,
                         int32_t lo_bin, double* tau_cm, double* sigma_cm) {
  if (!pspec || !hist || !counts || !tau_cm || !sigma_cm) return ISX_ERR_BAD_ARG;
  const int rc = check_scene_path_spec(pspec);
  if (rc) return rc;
  if (f < 0 || f >= ISX_RESPONSE_FATES || lo_bin < 0 || lo_bin >= pspec->n_bins) return ISX_ERR_BAD_ARG;
  if (counts->overflow[f] != 0) return ISX_ERR_BAD_CONFIG;
  const uint64_t* row = hist + (size_t)f * (size_t)pspec->n_bins;
  double N = 0, Sm = 0;
  for (int32_t ib = lo_bin; ib < pspec->n_bins; ++ib) {
    const double h = (double)row[ib];
    Sm += (double)(ib - lo_bin) * h;
    N += h;
  }
  if (!(N > 0)) return ISX_ERR_BAD_CONFIG;
  const double m = Sm / N;
  if (!(m > 0)) return ISX_ERR_BAD_CONFIG;
  const double r = m / (1.0 + m);
  const double lr = std::log(r);
  *tau_cm = -pspec->bin_cm / lr;
  *sigma_cm = pspec->bin_cm / (lr * lr) / std::sqrt(N * m * (1.0 + m));
  return ISX_OK;
}

#ifdef ISX_DIAG
// tuning builds only (not declared in isx.h): read and clear the binning diagnostics of isx_kernels.hpp
int isx_diag_read(uint64_t* out48) {
  if (!S.init || !out48) return ISX_ERR_BAD_ARG;
  if (trace_join()) return ISX_ERR_HIP;   // (behind an overlapped sequence, as every entry but isx_fluxmap_device)
  HIPCHK(hipStreamSynchronize(S.stream));
  HIPCHK(hipMemcpyFromSymbol(out48, HIP_SYMBOL(isx::g_diag), 48 * sizeof(unsigned long long)));
  unsigned long long z[48] = {0};
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(isx::g_diag), z, sizeof(z)));
  return ISX_OK;
}
#endif

}  // extern "C"
