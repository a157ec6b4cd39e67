/* Stand-alone driver of isxo_exit_segments / isxo_bin_segments for a sanitizer build (tests/test_injected_segments_cpu.py):
 * the exit segments of 2000 rays against 19 discs on an arc at 200 cm, with 1 and 4 threads, must give isxo_disc_sweep's counts;
 * an empty call and a one-disc call run as well.  Prints one line per run; exit status 0 only if everything agrees. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "isx_oracle.h"

#define N_RAYS 2000
#define N_DISC 19

int main(void) {
  isxo_config c;
  isxo_default_config(&c);
  double ca[6 * N_DISC];
  for (int k = 0; k < N_DISC; k++) {
    const double t = (k - 9) * 5.0 * M_PI / 180.0;
    ca[6 * k + 0] = 200.0 * sin(t); ca[6 * k + 1] = 0.0; ca[6 * k + 2] = -200.0 * cos(t);
    ca[6 * k + 3] = sin(t); ca[6 * k + 4] = 0.0; ca[6 * k + 5] = -cos(t);
  }
  int32_t* status = (int32_t*)malloc(N_RAYS * sizeof(int32_t));
  double* seg = (double*)malloc((size_t)N_RAYS * 7 * sizeof(double));
  double* ex = (double*)malloc((size_t)N_RAYS * 7 * sizeof(double));
  if (!status || !seg || !ex) return 2;
  if (isxo_exit_segments(&c, N_RAYS, 21, 0, status, seg)) return 3;
  uint64_t n = 0;
  for (int i = 0; i < N_RAYS; i++)
    if (status[i] == 1) { memcpy(ex + 7 * n, seg + 7 * i, 7 * sizeof(double)); n++; }
  uint64_t want[N_DISC], got[N_DISC];
  isxo_stats st;
  if (isxo_disc_sweep(&c, ca, N_DISC, 5.0, 0.1, N_RAYS, 21, 0, want, &st, 2)) return 4;
  int bad = n != st.exited;
  for (int nt = 1; nt <= 4; nt += 3) {
    if (isxo_bin_segments(ca, N_DISC, 5.0, 0.1, ex, n, got, nt)) return 5;
    uint64_t sum = 0;
    for (int k = 0; k < N_DISC; k++) { sum += got[k]; bad |= got[k] != want[k]; }
    printf("threads %d: segments %llu hits %llu\n", nt, (unsigned long long)n, (unsigned long long)sum);
    bad |= sum != st.bin_increments;
  }
  if (isxo_bin_segments(ca, N_DISC, 5.0, 0.1, NULL, 0, got, 1)) return 6;
  for (int k = 0; k < N_DISC; k++) bad |= got[k] != 0;
  if (isxo_bin_segments(ca + 6 * 9, 1, 5.0, 0.1, ex, n, got, 1)) return 7;
  printf("one disc: hits %llu\n", (unsigned long long)got[0]);
  bad |= got[0] != want[9];
  free(status); free(seg); free(ex);
  return bad ? 1 : 0;
}
