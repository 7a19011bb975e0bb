/* Plain-C consumer of include/lidar4d_prep.h: proves that the header is valid C (no C++ or torch types in the boundary),
 * that every declared entry point links against liblidar4d_prep.so with the declared prototype, and that the version and
 * error calls work without a GPU.  Built and run by tests/test_abi_cpu.py::test_c_abi_from_plain_c[prep] (gcc). */
#include <stdio.h>

#include "lidar4d_prep.h"

typedef void (*fn_t)(void);

int main(void) {
  const fn_t entry_points[] = {
      (fn_t)&l4dp_compact_workspace,
      (fn_t)&l4dp_knn_mean_dist,
      (fn_t)&l4dp_knn_workspace,
      (fn_t)&l4dp_last_error,
      (fn_t)&l4dp_outlier_filter,
      (fn_t)&l4dp_plane_mask,
      (fn_t)&l4dp_plane_score,
      (fn_t)&l4dp_range_filter,
      (fn_t)&l4dp_version,
  };
  const int n = (int)(sizeof(entry_points) / sizeof(entry_points[0]));
  for (int i = 0; i < n; ++i)
    if (!entry_points[i]) return 2;
  if (l4dp_version() != L4DP_ABI_VERSION) {
    fprintf(stderr, "ABI mismatch: library %d, header %d\n", l4dp_version(), L4DP_ABI_VERSION);
    return 3;
  }
  /* argument checks run before anything touches a device */
  if (l4dp_knn_mean_dist(0, 8, 65, 0, 0, 0, 0) == 0) return 4;
  if (l4dp_knn_workspace(100) != (128 * 3 + 64 * 6) * 4) return 5; /* 2 batches of 64 points, one group of 64 boxes */
  printf("%d entry points, ABI v%d, last error: \"%s\"\n", n, l4dp_version(), l4dp_last_error());
  return 0;
}
