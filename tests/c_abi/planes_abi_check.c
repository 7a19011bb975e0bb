/* Plain-C consumer of include/lidar4d_planes.h: proves that the header is valid C (no C++ or torch types in the boundary),
 * that every declared entry point links against liblidar4d_planes.so with the declared prototype, and that the version, error
 * and argument checks work without a GPU.  Built and run by tests/test_abi_cpu.py::test_c_abi_from_plain_c[planes] (gcc). */
#include <stdio.h>
#include <string.h>

#include "lidar4d_planes.h"

typedef void (*fn_t)(void);

int main(void) {
  const fn_t entry_points[] = {
      (fn_t)&l4dh_density_planes_bwd,
      (fn_t)&l4dh_density_planes_fwd,
      (fn_t)&l4dh_last_error,
      (fn_t)&l4dh_planes_bwd,
      (fn_t)&l4dh_planes_fwd,
      (fn_t)&l4dh_version,
  };
  const int n = (int)(sizeof(entry_points) / sizeof(entry_points[0]));
  float buf[16];
  const int64_t off[6 * 9] = {0};
  int32_t res[4 * 9];
  for (int i = 0; i < 4 * 9; ++i) res[i] = 4;
  for (int i = 0; i < n; ++i)
    if (!entry_points[i]) return 2;
  if (l4dh_version() != L4DH_ABI_VERSION) {
    fprintf(stderr, "ABI mismatch: library %d, header %d\n", l4dh_version(), L4DH_ABI_VERSION);
    return 3;
  }
  /* argument checks run before anything touches a device: channel counts other than 4, 8, 16 and more than 8 scales are refused */
  if (l4dh_planes_fwd(buf, off, res, 1, 2, buf, 4, 0, buf, buf, 0) != 1) return 4;
  if (!strstr(l4dh_last_error(), "l4dh_planes_fwd") || !strstr(l4dh_last_error(), "C must be 4, 8 or 16")) return 5;
  if (l4dh_planes_fwd(buf, off, res, 1, 32, buf, 4, 0, buf, buf, 0) != 1) return 6;
  if (l4dh_planes_fwd(buf, off, res, L4DH_MAX_SCALES + 1, 4, buf, 4, 0, buf, buf, 0) != 1) return 7;
  if (l4dh_planes_fwd(buf, off, res, 1, 4, buf, 4, 3, buf, buf, 0) != 1) return 8;
  if (!strstr(l4dh_last_error(), "which outside")) return 9;
  if (l4dh_planes_bwd(buf, off, res, 1, 12, buf, 4, 0, buf, buf, buf, 0, 0) != 1) return 10;
  if (!strstr(l4dh_last_error(), "l4dh_planes_bwd")) return 11;
  if (l4dh_planes_bwd(buf, off, res, L4DH_MAX_SCALES + 1, 16, buf, 4, 0, buf, buf, buf, 0, 0) != 1) return 12;
  if (l4dh_density_planes_fwd(buf, off, res, 1, 2, buf, buf, 6, 0, buf, 4, buf, buf, 0) != 1) return 13;
  if (!strstr(l4dh_last_error(), "l4dh_density_planes_fwd")) return 14;
  if (l4dh_density_planes_fwd(buf, off, res, L4DH_MAX_SCALES + 1, 8, buf, buf, 6, 0, buf, 4, buf, buf, 0) != 1) return 15;
  if (l4dh_density_planes_fwd(buf, off, res, 1, 8, buf, buf, 5, 0, buf, 4, buf, buf, 0) != 1) return 16;
  if (!strstr(l4dh_last_error(), "fewer than 6 columns")) return 17;
  if (l4dh_density_planes_bwd(buf, off, res, 1, 32, buf, buf, 6, 0, buf, 4, buf, buf, buf, buf, 0, 0) != 1) return 18;
  if (!strstr(l4dh_last_error(), "l4dh_density_planes_bwd")) return 19;
  if (l4dh_density_planes_bwd(buf, off, res, 1, 4, buf, buf, 6, 0, buf, 4, buf, buf, 0, buf, 0, 0) != 1) return 20;
  if (!strstr(l4dh_last_error(), "are required")) return 21;
  /* zero samples: a valid call that launches nothing */
  if (l4dh_planes_fwd(buf, off, res, 1, 4, buf, 0, 0, buf, buf, 0) != 0) return 22;
  if (l4dh_planes_bwd(buf, off, res, 1, 16, buf, 0, 0, buf, buf, buf, 0, 0) != 0) return 23;
  if (l4dh_density_planes_fwd(buf, off, res, 3, 4, buf, buf, 6, 0, buf, 0, buf, buf, 0) != 0) return 24;
  if (l4dh_density_planes_bwd(buf, off, res, 3, 16, buf, buf, 16, 1, buf, 0, buf, buf, buf, buf, buf, 0) != 0) return 25;
  printf("%d entry points, ABI v%d, last error: \"%s\"\n", n, l4dh_version(), l4dh_last_error());
  return 0;
}
