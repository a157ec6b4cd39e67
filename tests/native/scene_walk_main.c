/* The oracle's scene walk as a stand-alone program (TEST INFRASTRUCTURE): built by tests/test_scene_walk_cpu.py together with
 * oracle/isx_oracle.c under AddressSanitizer and UBSan and run as a child process.  It walks two scenes for 2000 rays of seed
 * 12345 at 1 and 4 threads with every per-ray output in a heap buffer of exactly the documented size, and prints the census; the
 * test compares the lines with the unsanitised library's.
 *
 *   photometer: the lamp at (0, 0, 20), the two baffles and the two caps of tests/test_scene_cpu.py (the caps' min_dot as
 *               isx_wall_patch_cap makes them for r_in 100.1: r_in cos 5 deg, r_in cos 10 deg), wall reflectance 0.95
 *   coplanar:   two discs in the plane z = 0.1 about one centre, radii 10 and 25, under the same lamp
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "isx_oracle.h"

#define N 2000

static isxo_beam_spec lamp(void) {
  isxo_beam_spec b;
  memset(&b, 0, sizeof(b));
  b.struct_size = (uint32_t)sizeof(b);
  b.origin[2] = 20.0;
  b.axis[2] = 1.0; b.e1[0] = 1.0; b.e2[1] = 1.0;
  b.radius = 0.0; b.cos_min = -1.0; b.angular_law = 0;
  return b;
}

static void disc(isxo_baffle* d, double cx, double cy, double cz, double mx, double my, double mz, double radius, double rho) {
  d->centre[0] = cx; d->centre[1] = cy; d->centre[2] = cz;
  d->normal[0] = mx; d->normal[1] = my; d->normal[2] = mz;
  d->radius = radius; d->reflectance = rho;
}

static int walk(const char* name, const isxo_config* c, const isxo_beam_spec* b, const isxo_baffle_spec* f,
                const isxo_wall_patch_spec* w) {
  for (int nt = 1; nt <= 4; nt += 3) {
    isxo_scene_rays r;
    r.status = malloc(N * sizeof(int32_t)); r.n_points = malloc(N * sizeof(int32_t));
    r.last_baffle = malloc(N * sizeof(int32_t)); r.last_class = malloc(N * sizeof(int32_t));
    r.first_class = malloc(N * sizeof(int32_t)); r.first_kind = malloc(N * sizeof(int32_t));
    r.last_point = malloc(3 * N * sizeof(double)); r.direction = malloc(3 * N * sizeof(double));
    r.start_point = malloc(3 * N * sizeof(double)); r.start_dir = malloc(3 * N * sizeof(double));
    isxo_scene_totals t;
    int rc = isxo_scene_walk(c, b, f, w, N, 12345u, 0u, &r, &t, nt);
    if (rc) { fprintf(stderr, "%s: isxo_scene_walk returned %d\n", name, rc); return 1; }
    /* ... and once more with no per-ray output at all: the totals must not depend on it */
    isxo_scene_totals t2;
    rc = isxo_scene_walk(c, b, f, w, N, 12345u, 0u, NULL, &t2, nt);
    t.census.t_kernel_ms = t2.census.t_kernel_ms = 0.0;
    if (rc || memcmp(&t, &t2, sizeof(t)) != 0) { fprintf(stderr, "%s: the totals depend on the per-ray outputs\n", name); return 1; }
    uint64_t words = 0;
    const uint64_t* cw = (const uint64_t*)&t.counts;
    for (size_t k = 0; k < sizeof(t.counts) / sizeof(uint64_t); k++) words += cw[k];
    long touched = 0;
    for (int i = 0; i < N; i++) touched += r.status[i] + r.n_points[i] + (r.last_point[3 * i + 2] < 0.0) + (r.start_dir[3 * i + 2] < 0.0);
    if (touched <= 0) return 1;
    printf("%s threads %d: launched %llu exited %llu counted_below_z %llu absorbed %llu suspended %llu wall_hits %llu"
           " counters %llu baffle_to_baffle %llu\n", name, nt, (unsigned long long)t.census.launched,
           (unsigned long long)t.census.exited, (unsigned long long)t.census.counted_below_z,
           (unsigned long long)t.census.absorbed, (unsigned long long)t.census.suspended,
           (unsigned long long)t.census.wall_hits, (unsigned long long)words, (unsigned long long)t.rays_baffle_to_baffle);
    free(r.status); free(r.n_points); free(r.last_baffle); free(r.last_class); free(r.first_class); free(r.first_kind);
    free(r.last_point); free(r.direction); free(r.start_point); free(r.start_dir);
  }
  return 0;
}

int main(void) {
  isxo_config c;
  isxo_default_config(&c);
  c.reflectance = 0.95;
  const isxo_beam_spec b = lamp();

  isxo_baffle_spec f;
  memset(&f, 0, sizeof(f));
  f.struct_size = (uint32_t)sizeof(f);
  f.n_baffles = 2;
  disc(&f.baffle[0], 35.0, 0.0, 13.0, 1.0, 0.0, 0.0, 10.0, 0.9);     /* screen */
  disc(&f.baffle[1], 0.0, 0.0, -40.0, 0.0, 0.0, 1.0, 12.0, 0.9);     /* shield over the port */
  isxo_wall_patch_spec w;
  memset(&w, 0, sizeof(w));
  w.struct_size = (uint32_t)sizeof(w);
  w.n_patches = 2;
  w.patch[0].axis[0] = 1.0; w.patch[0].min_dot = 0x1.8ee058f0a08eap+6; w.patch[0].reflectance = 0.0;   /* detector, 5 deg */
  w.patch[1].axis[1] = 1.0; w.patch[1].min_dot = 0x1.8a51288142af7p+6; w.patch[1].reflectance = 0.5;   /* sample, 10 deg */
  if (walk("photometer", &c, &b, &f, &w)) return 1;

  isxo_baffle_spec g;
  memset(&g, 0, sizeof(g));
  g.struct_size = (uint32_t)sizeof(g);
  g.n_baffles = 2;
  disc(&g.baffle[0], 0.0, 0.0, 0.1, 0.0, 0.0, 1.0, 10.0, 0.9);
  disc(&g.baffle[1], 0.0, 0.0, 0.1, 0.0, 0.0, 1.0, 25.0, 0.5);
  if (walk("coplanar", &c, &b, &g, NULL)) return 1;
  return 0;
}
