/* Plain-C consumer of include/lidar4d_eval.h: proves that the header is valid C (no C++ or torch types in the boundary),
 * that every declared entry point links against liblidar4d_eval.so with the declared prototype, and that the version and
 * error calls work without a GPU.  Built and run by tests/test_abi_cpu.py::test_c_abi_from_plain_c[eval] (gcc). */
#include <stdio.h>
#include <string.h>

#include "lidar4d_eval.h"

typedef void (*fn_t)(void);

int main(void) {
  const fn_t entry_points[] = {
      (fn_t)&l4de_image_errors,
      (fn_t)&l4de_image_errors_workspace,
      (fn_t)&l4de_last_error,
      (fn_t)&l4de_version,
  };
  const int n = (int)(sizeof(entry_points) / sizeof(entry_points[0]));
  for (int i = 0; i < n; ++i)
    if (!entry_points[i]) return 2;
  if (l4de_version() != L4DE_ABI_VERSION) {
    fprintf(stderr, "ABI mismatch: library %d, header %d\n", l4de_version(), L4DE_ABI_VERSION);
    return 3;
  }
  /* argument checks run before anything touches a device */
  if (l4de_image_errors(0, 0, L4DE_SSIM_WINDOW - 1, 64, 0.0f, 1.0f, 0, 0, 0) == 0) return 4;
  if (!strstr(l4de_last_error(), "at least 7")) return 5;
  if (l4de_image_errors_workspace(L4DE_SSIM_WINDOW - 1, 64) != 0 || l4de_image_errors_workspace(66, 1030) < 66 * 1030 * 4) return 6;
  printf("%d entry points, ABI v%d, last error: \"%s\"\n", n, l4de_version(), l4de_last_error());
  return 0;
}
