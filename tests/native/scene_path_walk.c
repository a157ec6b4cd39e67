/* The scene walk with the path length of every ray (TEST INFRASTRUCTURE): include/isx.h's isx_scene_path_hist restated in C on
 * the oracle's exported primitives alone -- isxo_philox4x32_10, isxo_u01, isxo_sincos2pi, isxo_next_boundary,
 * isxo_cosine_emission.  The beam, baffle and patch rules are restated here from include/isx.h; nothing of the oracle's own
 * scene walk is called.  tests/scenepath_np.py compiles this file on first use, together with oracle/isx_oracle.c and with the
 * flags of oracle/Makefile, into a git-ignored build directory, and holds it in three ways (tests/test_scene_path_cpu.py): its
 * per-ray end states equal isxo_scene_walk's bit for bit, its L equals the Python restatement's bit for bit, and it runs once as
 * a stand-alone program under AddressSanitizer and UBSan (-DSPW_MAIN; nothing is preloaded).
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "isx_oracle.h"

enum { K_NONE = 0, K_INNER = 1, K_OUTER = 2, K_CONE = 3, K_BOX = 4 };

/* per-ray outputs, [n] or [n][3]; every pointer may be NULL */
typedef struct spw_rays {
  int32_t *status, *n_points;
  double *last_point, *direction, *start_point;
  int32_t *last_baffle, *last_class;
  double* path_cm;   /* L of the contract */
} spw_rays;

/* the absorb test's threshold on the raw word: b survives iff b < thr (the wall's rule: (b + 0.5) 2^-32 < rho) */
static uint64_t rho_thr(double rho) {
  const double x = ceil(ldexp(rho, 32) - 0.5);
  if (!(x > 0.0)) return 0;
  if (x >= 4294967296.0) return 4294967296ull;
  return (uint64_t)x;
}

static void block(uint64_t seed, uint64_t ray, uint32_t blk, uint32_t stream, uint32_t w[4]) {
  const uint32_t ctr[4] = { (uint32_t)ray, (uint32_t)(ray >> 32), blk, stream };
  const uint32_t key[2] = { (uint32_t)seed, (uint32_t)(seed >> 32) };
  isxo_philox4x32_10(ctr, key, w);
}

/* isx.h, the beam contract: the start of a ray from block 0 of Philox stream 3 */
static void beam_start(const isxo_beam_spec* b, uint64_t seed, uint64_t ray, double p[3], double v[3]) {
  uint32_t w[4];
  block(seed, ray, 0u, 3u, w);
  const double rr = b->radius * sqrt(isxo_u01(w[0]));
  double s1, c1, s3, c3;
  isxo_sincos2pi(isxo_u01(w[1]), &s1, &c1);
  const double a = rr * c1;
  const double bb = rr * s1;
  const double u2 = isxo_u01(w[2]);
  double ct, st;
  if (b->angular_law == 1) {
    const double s2 = u2 * (1.0 - b->cos_min * b->cos_min);
    st = sqrt(s2);
    ct = sqrt(1.0 - s2);
  } else {
    ct = 1.0 - u2 * (1.0 - b->cos_min);
    st = sqrt(1.0 - ct * ct);
  }
  isxo_sincos2pi(isxo_u01(w[3]), &s3, &c3);
  const double k1 = st * c3;
  const double k2 = st * s3;
  double d[3];
  for (int i = 0; i < 3; i++) {
    p[i] = (b->origin[i] + a * b->e1[i]) + bb * b->e2[i];
    d[i] = (ct * b->axis[i] + k1 * b->e1[i]) + k2 * b->e2[i];
  }
  const double mag = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  for (int i = 0; i < 3; i++) v[i] = d[i] / mag;
}

/* isx.h, the baffle contract: the disc the segment p -> q strikes first (smallest f, on equal f the lowest index), or -1 */
static int baffle_segment(const isxo_baffle_spec* bf, const double p[3], const double q[3], int skip, int* side, double x[3]) {
  int best = -1;
  double best_f = 0.0;
  for (int k = 0; k < bf->n_baffles; k++) {
    if (k == skip) continue;
    const double* c = bf->baffle[k].centre;
    const double* m = bf->baffle[k].normal;
    const double sp = ((p[0] - c[0]) * m[0] + (p[1] - c[1]) * m[1]) + (p[2] - c[2]) * m[2];
    const double sq = ((q[0] - c[0]) * m[0] + (q[1] - c[1]) * m[1]) + (q[2] - c[2]) * m[2];
    if (!((sp > 0.0 && sq < 0.0) || (sp < 0.0 && sq > 0.0))) continue;
    const double f = sp / (sp - sq);
    double y[3], d[3];
    for (int i = 0; i < 3; i++) { y[i] = p[i] + f * (q[i] - p[i]); d[i] = y[i] - c[i]; }
    if ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= bf->baffle[k].radius * bf->baffle[k].radius && (best < 0 || f < best_f)) {
      best = k; best_f = f; *side = sp > 0.0 ? 0 : 1;
      x[0] = y[0]; x[1] = y[1]; x[2] = y[2];
    }
  }
  return best;
}

/* isx.h, the path contract: the length of the segment a -> b */
static double segment(const double a[3], const double b[3]) {
  const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

/* -2: outside the walk's scope (no beam, a part count out of range, another border or source); -3: a NULL configuration */
int spw_scene_path_walk(const isxo_config* c, const isxo_beam_spec* beam, const isxo_baffle_spec* baffles,
                        const isxo_wall_patch_spec* patches, uint64_t n, uint64_t seed, uint64_t first, const spw_rays* rays,
                        int nthreads) {
  if (!c) return -3;
  if (!beam || !baffles || !patches || !rays) return -2;
  if (c->lambertian != 1 || c->surface_model != 0 || c->source_model != 0 || c->trace_mode != 0) return -2;
  const int nb = baffles->n_baffles, P = patches->n_patches;
  if (nb < 0 || nb > ISXO_MAX_BAFFLES || P < 0 || P > ISXO_MAX_WALL_PATCHES) return -2;
  if (beam->angular_law != 0 && beam->angular_law != 1) return -2;
  /* per wall class and per baffle: the configuration with that reflectance (the emission's constants), and its threshold */
  isxo_config cc[ISXO_MAX_WALL_PATCHES + 2], bc[ISXO_MAX_BAFFLES];
  uint64_t cthr[ISXO_MAX_WALL_PATCHES + 2], bthr[ISXO_MAX_BAFFLES];
  double rm[ISXO_MAX_BAFFLES][3];
  for (int k = 0; k < P + 2; k++) {
    cc[k] = *c;
    if (k < P) cc[k].reflectance = patches->patch[k].reflectance;
    cthr[k] = rho_thr(cc[k].reflectance);
  }
  for (int k = 0; k < nb; k++) {
    bc[k] = *c;
    bc[k].reflectance = baffles->baffle[k].reflectance;
    bthr[k] = rho_thr(bc[k].reflectance);
    for (int i = 0; i < 3; i++) rm[k][i] = c->r_in * baffles->baffle[k].normal[i];
  }
  const spw_rays R = *rays;
  int bad = 0;
#ifdef _OPENMP
  omp_set_num_threads(nthreads > 0 ? nthreads : omp_get_num_procs());
#else
  (void)nthreads;
#endif
#pragma omp parallel for schedule(dynamic, 256)
  for (int64_t i = 0; i < (int64_t)n; i++) {
    const uint64_t ray = first + (uint64_t)i;
    double p[3], v[3], p0[3];
    beam_start(beam, seed, ray, p, v);
    memcpy(p0, p, sizeof(p0));
    int on = K_NONE, npts = 1, status = 0, skip = -1, lb = -1, lc = -1;
    uint32_t j = 0;
    double L = 0.0;
    for (;;) {
      double q[3], vn[3], x[3];
      int side = 0;
      const int kind = isxo_next_boundary(c, p, v, on, q, vn);
      if (kind < K_INNER || kind > K_BOX) {
#pragma omp atomic write
        bad = 1;
        status = 0;
        break;
      }
      memcpy(v, vn, sizeof(v));
      const int k = nb ? baffle_segment(baffles, p, q, skip, &side, x) : -1;
      npts++;
      uint32_t w[4];
      block(seed, ray, j >> 1, 0u, w);
      const uint32_t wa = w[2u * (j & 1u)], wb = w[2u * (j & 1u) + 1u];
      if (k >= 0) {
        L = L + segment(p, x);
        memcpy(p, x, sizeof(p));
        lb = 2 * k + side;
        on = K_NONE; skip = k;
        j++;
        if (!((uint64_t)wb < bthr[k])) { status = ISXO_ABSORBED; break; }
        const double zero[3] = { 0.0, 0.0, 0.0 };
        double S[3], d[3];
        isxo_cosine_emission(&bc[k], K_INNER, zero, wa, wb, S);
        for (int a = 0; a < 3; a++) d[a] = (side == 0 ? rm[k][a] : -rm[k][a]) + S[a];
        const double mag = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        for (int a = 0; a < 3; a++) v[a] = d[a] / mag;
        if (npts > c->max_points) { status = ISXO_SUSPENDED; break; }
        continue;
      }
      skip = -1;
      if (kind == K_BOX) {
        /* the leg to the world box is not counted; a ray counted below z gets the part of it up to the port plane */
        if (q[2] < c->exit_port_z) {
          const double s = segment(p, q);
          const double f = (c->exit_port_z - p[2]) / (q[2] - p[2]);
          L = L + ((f > 0.0 && f <= 1.0) ? s * f : 0.0);
        }
        memcpy(p, q, sizeof(p));
        status = ISXO_EXITED;
        break;
      }
      L = L + segment(p, q);
      memcpy(p, q, sizeof(p));
      on = kind;
      int cls = P + 1;
      if (kind == K_INNER) {
        cls = P;
        for (int m = 0; m < P; m++) {
          const isxo_wall_patch* wp = &patches->patch[m];
          if ((p[0] * wp->axis[0] + p[1] * wp->axis[1]) + p[2] * wp->axis[2] >= wp->min_dot) { cls = m; break; }
        }
      }
      lc = cls;
      j++;
      if (!((uint64_t)wb < cthr[cls])) { status = ISXO_ABSORBED; break; }
      isxo_cosine_emission(&cc[cls], kind, p, wa, wb, v);
      if (npts > c->max_points) { status = ISXO_SUSPENDED; break; }
    }
    if (R.status) R.status[i] = status;
    if (R.n_points) R.n_points[i] = npts;
    for (int a = 0; a < 3; a++) {
      if (R.last_point) R.last_point[3 * i + a] = p[a];
      if (R.direction) R.direction[3 * i + a] = v[a];
      if (R.start_point) R.start_point[3 * i + a] = p0[a];
    }
    if (R.last_baffle) R.last_baffle[i] = lb;
    if (R.last_class) R.last_class[i] = lc;
    if (R.path_cm) R.path_cm[i] = L;
  }
  int was_bad;
#pragma omp atomic read
  was_bad = bad;
  return was_bad ? -4 : 0;
}

#ifdef SPW_MAIN
/* The stand-alone program: the photometer of tests/native/scene_walk_main.c for 2000 rays of seed 12345, at 1 and 4 threads,
 * every per-ray output in a heap buffer of exactly its size.  Prints the sum of the bit patterns of L modulo 2^64 and the
 * number of rays by status; the test compares the lines with the unsanitised build's. */
#define N 2000
int main(void) {
  isxo_config c;
  isxo_default_config(&c);
  c.reflectance = 0.95;
  isxo_beam_spec b;
  memset(&b, 0, sizeof(b));
  b.origin[2] = 20.0;
  b.axis[2] = 1.0; b.e1[0] = 1.0; b.e2[1] = 1.0;
  b.radius = 0.0; b.cos_min = -1.0; b.angular_law = 0;
  isxo_baffle_spec f;
  memset(&f, 0, sizeof(f));
  f.n_baffles = 2;
  f.baffle[0].centre[0] = 35.0; f.baffle[0].centre[2] = 13.0; f.baffle[0].normal[0] = 1.0; f.baffle[0].radius = 10.0; f.baffle[0].reflectance = 0.9;
  f.baffle[1].centre[2] = -40.0; f.baffle[1].normal[2] = 1.0; f.baffle[1].radius = 12.0; f.baffle[1].reflectance = 0.9;
  isxo_wall_patch_spec w;
  memset(&w, 0, sizeof(w));
  w.n_patches = 2;
  w.patch[0].axis[0] = 1.0; w.patch[0].min_dot = 0x1.8ee058f0a08eap+6; w.patch[0].reflectance = 0.0;
  w.patch[1].axis[1] = 1.0; w.patch[1].min_dot = 0x1.8a51288142af7p+6; w.patch[1].reflectance = 0.5;
  for (int nt = 1; nt <= 4; nt += 3) {
    spw_rays r;
    r.status = malloc(N * sizeof(int32_t)); r.n_points = malloc(N * sizeof(int32_t));
    r.last_baffle = malloc(N * sizeof(int32_t)); r.last_class = malloc(N * sizeof(int32_t));
    r.last_point = malloc(3 * N * sizeof(double)); r.direction = malloc(3 * N * sizeof(double));
    r.start_point = malloc(3 * N * sizeof(double)); r.path_cm = malloc(N * sizeof(double));
    const int rc = spw_scene_path_walk(&c, &b, &f, &w, N, 12345u, 0u, &r, nt);
    if (rc) { fprintf(stderr, "spw_scene_path_walk returned %d\n", rc); return 1; }
    uint64_t sum = 0;
    int by[4] = { 0, 0, 0, 0 };
    for (int i = 0; i < N; i++) {
      uint64_t bits;
      memcpy(&bits, &r.path_cm[i], sizeof(bits));
      sum += bits;
      by[r.status[i] & 3]++;
    }
    printf("threads %d: checksum %llu exited %d absorbed %d suspended %d\n", nt, (unsigned long long)sum, by[1], by[2], by[3]);
    free(r.status); free(r.n_points); free(r.last_baffle); free(r.last_class);
    free(r.last_point); free(r.direction); free(r.start_point); free(r.path_cm);
  }
  return 0;
}
#endif
