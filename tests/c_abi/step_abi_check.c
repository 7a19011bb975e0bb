/* Plain-C consumer of include/lidar4d_step.h: proves that the header is valid C (no C++ or torch types in the boundary),
 * that every declared entry point links against liblidar4d_step.so with the declared prototype, and that the version, error
 * and argument checks work without a GPU.  Built and run by tests/test_abi_cpu.py::test_c_abi_from_plain_c[step] (gcc). */
#include <stdio.h>
#include <string.h>

#include "lidar4d_step.h"

typedef void (*fn_t)(void);

int main(void) {
  const fn_t entry_points[] = {
      (fn_t)&l4ds_last_error,
      (fn_t)&l4ds_primary_losses,
      (fn_t)&l4ds_primary_losses_workspace,
      (fn_t)&l4ds_ray_batch,
      (fn_t)&l4ds_version,
  };
  const int n = (int)(sizeof(entry_points) / sizeof(entry_points[0]));
  for (int i = 0; i < n; ++i)
    if (!entry_points[i]) return 2;
  if (l4ds_version() != L4DS_ABI_VERSION) {
    fprintf(stderr, "ABI mismatch: library %d, header %d\n", l4ds_version(), L4DS_ABI_VERSION);
    return 3;
  }
  /* argument checks run before anything touches a device */
  if (l4ds_primary_losses(0, 0, 0, 0, 0, -1, L4DS_L1, L4DS_MSE, L4DS_MSE, 1.0f, 0.01f, 0.1f, 0.2f, 0.1f, 1.0f, 0, 0, 0, 0, 0, 0, 0) == 0)
    return 4;
  if (!strstr(l4ds_last_error(), "l4ds_primary_losses") || !strstr(l4ds_last_error(), "negative")) return 5;
  if (l4ds_primary_losses(0, 0, 0, 0, 0, 4, L4DS_L1, L4DS_HUBER + 1, L4DS_MSE, 1.0f, 0.01f, 0.1f, 0.2f, 0.1f, 1.0f, 0, 0, 0, 0, 0, 0, 0) == 0)
    return 6;
  if (!strstr(l4ds_last_error(), "unknown criterion")) return 7;
  if (l4ds_ray_batch(0, 0, 4, 0, 8, 0, 2.0f, 26.9f, 8, 32, 0, 0, 0, 0, 0, 0, 0) == 0) return 8;
  if (!strstr(l4ds_last_error(), "l4ds_ray_batch") || !strstr(l4ds_last_error(), "at least 1")) return 9;
  if (l4ds_ray_batch(0, 0, 4, 1, 1, 0, 2.0f, 26.9f, 0, 32, 0, 0, 0, 0, 0, 0, 0) == 0) return 10;
  if (!strstr(l4ds_last_error(), "empty image")) return 11;
  if (l4ds_primary_losses_workspace(-1) != 0 || l4ds_primary_losses_workspace(0) != 4 || l4ds_primary_losses_workspace(257) != 8) return 12;
  printf("%d entry points, ABI v%d, last error: \"%s\"\n", n, l4ds_version(), l4ds_last_error());
  return 0;
}
