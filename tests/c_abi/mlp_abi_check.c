/* Plain-C consumer of include/lidar4d_mlp.h: proves that the header is valid C (no C++ or torch types in the boundary),
 * that every declared entry point links against liblidar4d_mlp.so with the declared prototype, and that the version, error
 * and argument checks work without a GPU.  Built and run by tests/test_abi_cpu.py::test_c_abi_from_plain_c[mlp] (gcc). */
#include <stdio.h>
#include <string.h>

#include "lidar4d_mlp.h"

typedef void (*fn_t)(void);

int main(void) {
  const fn_t entry_points[] = {
      (fn_t)&l4dm_last_error,
      (fn_t)&l4dm_mlp_bwd,
      (fn_t)&l4dm_mlp_fwd,
      (fn_t)&l4dm_version,
  };
  const int n = (int)(sizeof(entry_points) / sizeof(entry_points[0]));
  char buf[16];
  float amax = 0.0f;
  for (int i = 0; i < n; ++i)
    if (!entry_points[i]) return 2;
  if (l4dm_version() != L4DM_ABI_VERSION) {
    fprintf(stderr, "ABI mismatch: library %d, header %d\n", l4dm_version(), L4DM_ABI_VERSION);
    return 3;
  }
  /* argument checks run before anything touches a device: width 64 belongs to liblidar4d_hip.so, other shapes to nobody */
  if (l4dm_mlp_fwd(buf, 4, 0, 96, 64, 2, buf, buf, 0, 0, 0) != 1) return 4;
  if (!strstr(l4dm_last_error(), "l4dm_mlp_fwd") || !strstr(l4dm_last_error(), "unsupported shape")) return 5;
  if (l4dm_mlp_fwd(buf, 4, 0, 48, 32, 2, buf, buf, 0, 0, 0) != 1) return 6;
  if (l4dm_mlp_fwd(buf, 4, 0, 96, 32, 4, buf, buf, 0, 0, 0) != 1) return 7;
  if (l4dm_mlp_fwd(buf, 4, 0, 96, 32, 2, buf, 0, 0, 0, 0) != 1) return 8;
  if (!strstr(l4dm_last_error(), "are required")) return 9;
  if (l4dm_mlp_bwd(buf, buf, buf, 4, 0, 96, 64, 2, buf, 0, &amax, 1.0f, 0, 0, 0, 0) != 1) return 10;
  if (!strstr(l4dm_last_error(), "l4dm_mlp_bwd") || !strstr(l4dm_last_error(), "unsupported shape")) return 11;
  if (l4dm_mlp_bwd(buf, 0, buf, 4, 0, 96, 128, 2, buf, 0, &amax, 1.0f, 0, 0, 0, 0) != 1) return 12;
  if (!strstr(l4dm_last_error(), "not recomputed")) return 13;
  if (l4dm_mlp_bwd(buf, buf, buf, 4, 0, 96, 16, 2, buf, 0, &amax, 1.0f, &amax, 0, 16, 0) != 1) return 14; /* dx_absmax without dx */
  if (l4dm_mlp_bwd(buf, buf, buf, 4, 0, 96, 16, 2, buf, buf, &amax, 1.0f, &amax, 8, 32, 0) != 1) return 15;
  if (!strstr(l4dm_last_error(), "dx_absmax needs dx and a column range")) return 16;
  /* zero rows: a valid call that launches nothing */
  if (l4dm_mlp_fwd(buf, 0, 0, 96, 32, 2, buf, buf, 0, 0, 0) != 0) return 17;
  if (l4dm_mlp_bwd(buf, buf, buf, 0, 0, 96, 128, 3, buf, 0, &amax, 1.0f, 0, 0, 0, 0) != 0) return 18;
  printf("%d entry points, ABI v%d, last error: \"%s\"\n", n, l4dm_version(), l4dm_last_error());
  return 0;
}
