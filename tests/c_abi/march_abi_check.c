/* Plain-C consumer of include/lidar4d_march.h: proves that the header is valid C (no C++ or torch types in the boundary),
 * that every declared entry point links against liblidar4d_march.so with the declared prototype, and that the version, error
 * and argument checks work without a GPU.  Built and run by tests/test_abi_cpu.py::test_c_abi_from_plain_c[march] (gcc). */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "lidar4d_march.h"

typedef void (*fn_t)(void);

int main(void) {
  const fn_t entry_points[] = {
      (fn_t)&l4dr_last_error,
      (fn_t)&l4dr_march_init,
      (fn_t)&l4dr_slab_rows,
      (fn_t)&l4dr_slab_update,
      (fn_t)&l4dr_slab_update_workspace,
      (fn_t)&l4dr_version,
  };
  const int n = (int)(sizeof(entry_points) / sizeof(entry_points[0]));
  float buf[16];
  int32_t ibuf[16];
  for (int i = 0; i < n; ++i)
    if (!entry_points[i]) return 2;
  if (l4dr_version() != L4DR_ABI_VERSION) {
    fprintf(stderr, "ABI mismatch: library %d, header %d\n", l4dr_version(), L4DR_ABI_VERSION);
    return 3;
  }
  /* argument checks run before anything touches a device */
  if (l4dr_slab_rows(buf, buf, buf, buf, ibuf, 2, 4, 0, 0, 16, 0.f, 1.f, 1.f, buf, 0) != 1) return 4;
  if (!strstr(l4dr_last_error(), "l4dr_slab_rows") || !strstr(l4dr_last_error(), "T must be at least 1")) return 5;
  if (l4dr_slab_rows(buf, buf, buf, buf, ibuf, 2, 4, 96, 0, 0, 0.f, 1.f, 1.f, buf, 0) != 1) return 6;
  if (!strstr(l4dr_last_error(), "S must be at least 1")) return 7;
  if (l4dr_slab_rows(buf, buf, buf, buf, ibuf, 2, 4, 96, 96, 16, 0.f, 1.f, 1.f, buf, 0) != 1) return 8;
  if (!strstr(l4dr_last_error(), "s0 outside")) return 9;
  if (l4dr_slab_rows(buf, buf, buf, buf, ibuf, 5, 4, 96, 0, 16, 0.f, 1.f, 1.f, buf, 0) != 1) return 10;
  if (!strstr(l4dr_last_error(), "n_live outside")) return 11;
  if (l4dr_slab_update(buf, buf, buf, ibuf, 2, 4, 96, -1, 16, 0.1f, 1.f, 0, 0.f, buf, buf, buf, ibuf, ibuf, ibuf, ibuf, 0) != 1) return 12;
  if (!strstr(l4dr_last_error(), "l4dr_slab_update") || !strstr(l4dr_last_error(), "s0 outside")) return 13;
  if (l4dr_slab_update(buf, buf, buf, ibuf, 2, 4, 96, 0, 16, 0.1f, 1.f, 0, -1e-3f, buf, buf, buf, ibuf, ibuf, ibuf, ibuf, 0) != 1) return 14;
  if (!strstr(l4dr_last_error(), "eps must be a number >= 0")) return 15;
  if (l4dr_slab_update(buf, buf, buf, ibuf, 2, 4, 96, 0, 16, 0.1f, 1.f, 0, (float)NAN, buf, buf, buf, ibuf, ibuf, ibuf, ibuf, 0) != 1) return 16;
  if (l4dr_march_init(-1, buf, ibuf, ibuf, 0) != 1) return 17;
  if (!strstr(l4dr_last_error(), "l4dr_march_init")) return 18;
  /* no rays, or no live rays: valid calls that launch nothing */
  if (l4dr_march_init(0, buf, ibuf, ibuf, 0) != 0) return 19;
  if (l4dr_slab_rows(buf, buf, buf, buf, ibuf, 0, 4, 96, 80, 32, 0.f, 1.f, 1.f, buf, 0) != 0) return 20;
  if (l4dr_slab_update(buf, buf, buf, ibuf, 0, 4, 96, 0, 16, 0.1f, 1.f, 1, 1e-4f, buf, buf, buf, ibuf, ibuf, ibuf, ibuf, 0) != 0) return 21;
  if (l4dr_slab_update_workspace(0) < 4 || l4dr_slab_update_workspace(1000) < 4000) return 22;
  printf("%d entry points, ABI v%d, last error: \"%s\"\n", n, l4dr_version(), l4dr_last_error());
  return 0;
}
