/* Plain-C consumer of include/lidar4d_loss.h: proves that the header is valid C (no C++ or torch types in the boundary),
 * that every declared entry point links against liblidar4d_loss.so with the declared prototype, and that the version and
 * error calls work without a GPU.  Built and run by tests/test_abi_cpu.py::test_c_abi_from_plain_c[loss] (gcc). */
#include <stdio.h>
#include <string.h>

#include "lidar4d_loss.h"

typedef void (*fn_t)(void);

int main(void) {
  const fn_t entry_points[] = {
      (fn_t)&l4dl_last_error,
      (fn_t)&l4dl_los_bwd,
      (fn_t)&l4dl_los_fwd,
      (fn_t)&l4dl_los_workspace,
      (fn_t)&l4dl_version,
  };
  const int n = (int)(sizeof(entry_points) / sizeof(entry_points[0]));
  for (int i = 0; i < n; ++i)
    if (!entry_points[i]) return 2;
  if (l4dl_version() != L4DL_ABI_VERSION) {
    fprintf(stderr, "ABI mismatch: library %d, header %d\n", l4dl_version(), L4DL_ABI_VERSION);
    return 3;
  }
  /* argument checks run before anything touches a device */
  if (l4dl_los_fwd(0, 0, 0, 0, 0, 768, 0, 0, 1000, 0, 0, 0) == 0) return 4;
  if (!strstr(l4dl_last_error(), "l4dl_los_fwd") || !strstr(l4dl_last_error(), "at least 1")) return 5;
  if (l4dl_los_bwd(0, 0, 0, 0, 64, 0, 0, 0, 1000, 0, 0, 0, 0) == 0) return 6;
  if (!strstr(l4dl_last_error(), "l4dl_los_bwd")) return 7;
  if (l4dl_los_workspace(0, 768) != 0 || l4dl_los_workspace(16384, 0) != 0) return 8;
  if (l4dl_los_workspace(16384, 768) <= 0 || l4dl_los_workspace(1, 1) % 8 != 0) return 9;
  printf("%d entry points, ABI v%d, last error: \"%s\"\n", n, l4dl_version(), l4dl_last_error());
  return 0;
}
