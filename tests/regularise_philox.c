/* The counter-based normals of include/mmf_philox.h on the CPU, for tests/_regularise_cases.py (compiled with gcc,
 * -ffp-contract=off, into the test's tmp_path):
 *     regularise_philox SEED STREAM STEP TRAJ0 N M
 * prints, for every trajectory n < N and particle m < M, the bits of the four normals of
 * mmf_philox_normal4_stream(SEED, STREAM, STEP, TRAJ0 + n, m) as hexadecimal words, one particle per line, and -- after
 * them -- one line "legacy_equal K": K = 1 iff mmf_philox_normal4 gave the same 4 N M words as stream 0 of the same call. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mmf_philox.h"

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const uint64_t seed = strtoull(argv[1], NULL, 10);
  const uint32_t stream = (uint32_t)strtoul(argv[2], NULL, 10), step = (uint32_t)strtoul(argv[3], NULL, 10);
  const uint32_t traj0 = (uint32_t)strtoul(argv[4], NULL, 10);
  const int N = atoi(argv[5]), M = atoi(argv[6]);
  int legacy_equal = 1;
  for (int n = 0; n < N; ++n)
    for (int m = 0; m < M; ++m) {
      float z[4], z0[4], legacy[4];
      uint32_t w[4];
      mmf_philox_normal4_stream(seed, stream, step, traj0 + (uint32_t)n, (uint32_t)m, z);
      mmf_philox_normal4_stream(seed, 0u, step, traj0 + (uint32_t)n, (uint32_t)m, z0);
      mmf_philox_normal4(seed, step, traj0 + (uint32_t)n, (uint32_t)m, legacy);
      if (memcmp(z0, legacy, sizeof z0) != 0) legacy_equal = 0;
      memcpy(w, z, sizeof w);
      printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
    }
  printf("legacy_equal %d\n", legacy_equal);
  return 0;
}
