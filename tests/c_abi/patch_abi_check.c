/* Plain-C consumer of include/lidar4d_patch.h: proves that the header is valid C (no C++ or torch types in the boundary),
 * that every declared entry point links against liblidar4d_patch.so with the declared prototype, and that the version and
 * error calls work without a GPU.  Built and run by tests/test_abi_cpu.py::test_c_abi_from_plain_c[patch] (gcc). */
#include <stdio.h>
#include <string.h>

#include "lidar4d_patch.h"

typedef void (*fn_t)(void);

int main(void) {
  const fn_t entry_points[] = {
      (fn_t)&l4dg_last_error,
      (fn_t)&l4dg_patch_bwd,
      (fn_t)&l4dg_patch_fwd,
      (fn_t)&l4dg_patch_workspace,
      (fn_t)&l4dg_version,
  };
  const int n = (int)(sizeof(entry_points) / sizeof(entry_points[0]));
  const int flags = L4DG_GRAD_LOSS;
  for (int i = 0; i < n; ++i)
    if (!entry_points[i]) return 2;
  if (l4dg_version() != L4DG_ABI_VERSION) {
    fprintf(stderr, "ABI mismatch: library %d, header %d\n", l4dg_version(), L4DG_ABI_VERSION);
    return 3;
  }
  /* argument checks run before anything touches a device */
  if (l4dg_patch_fwd(0, 0, 0, 0, 4, 33, 32, 1.0f, L4DG_L1, flags, 0.1f, 0.1f, 0.1f, 0.1f, 0, 0, 0, 0) == 0) return 4;
  if (!strstr(l4dg_last_error(), "l4dg_patch_fwd") || !strstr(l4dg_last_error(), "at most 1024")) return 5;
  if (l4dg_patch_fwd(0, 0, 0, 0, 4, 1, 8, 1.0f, L4DG_L1, flags, 0.1f, 0.1f, 0.1f, 0.1f, 0, 0, 0, 0) == 0) return 6;
  if (!strstr(l4dg_last_error(), "at least 2")) return 7;
  if (l4dg_patch_bwd(0, 0, 16, 0, 0) == 0) return 8;
  if (!strstr(l4dg_last_error(), "l4dg_patch_bwd")) return 9;
  if (l4dg_patch_workspace(0, 2, 8) != 0 || l4dg_patch_workspace(4, 1, 8) != 0 || l4dg_patch_workspace(4, 33, 32) != 0) return 10;
  if (l4dg_patch_workspace(1024, 2, 8) <= 0 || l4dg_patch_workspace(1, 32, 32) % 8 != 0) return 11;
  printf("%d entry points, ABI v%d, last error: \"%s\"\n", n, l4dg_version(), l4dg_last_error());
  return 0;
}
