/*
 * lidar4d_prep.h -- C ABI of the point-cloud preparation kernels (gfx950 / CDNA4): liblidar4d_prep.so.
 *
 * The scene-flow term needs every training frame's cloud split into non-ground and ground points.  The reference
 * makes that split on the CPU (utils/misc.py:116-154, point_removal: range filter, open3d statistical outlier
 * removal, six RANSAC plane fits, outlier removal again); these entry points are its device-side building blocks and
 * lidar4d_amd/pointprep.py assembles them.  A library of its own, next to liblidar4d_hip.so (include/lidar4d_hip.h):
 * start-up work, loaded on first use, and the render path's ABI stays what it is.
 *
 * Conventions as in lidar4d_hip.h: every pointer is a DEVICE pointer unless its comment says "host"; tensors are dense
 * row-major; `stream` is a hipStream_t passed as void*; outputs and workspaces are allocated by the caller; every
 * entry point returns 0 on success or a hipError_t value (l4dp_last_error() gives the text); `*_workspace` return bytes.
 * No entry point synchronises with the host.
 */
#ifndef LIDAR4D_PREP_H
#define LIDAR4D_PREP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L4DP_ABI_VERSION 1
#define L4DP_MAX_NEIGHBORS 64 /* one neighbour per lane of a wavefront */

int l4dp_version(void);
const char* l4dp_last_error(void);

/* Bytes of workspace for an order-preserving compaction of n points (l4dp_range_filter, l4dp_outlier_filter). */
int64_t l4dp_compact_workspace(int64_t n);

/* utils/misc.py:116-125.  Keeps p = points[i] ([n,3] fp32) with dist_min <= |p| <= dist_max (|p| in fp32, like numpy on
 * a float32 cloud), z_min < p.z < z_max and not (|p.x| < 2 and |p.y| < 1 and |p.z| < 2), in input order.
 * out [n,3] (the first *count rows are written), out_index [n] int32 or null (input row of every output row),
 * count [1] int32. */
int l4dp_range_filter(const float* points, int64_t n, float dist_min, float dist_max, float z_min, float z_max, float* out,
                      int32_t* out_index, int32_t* count, void* workspace, void* stream);

/* Mean Euclidean distance of every point to its min(k, n) nearest points of the same cloud, itself included
 * (k <= L4DP_MAX_NEIGHBORS): the statistic of open3d's remove_statistical_outlier.  Exact (every pair is visited) and
 * bit-reproducible from run to run.  order [n] int32 or null: a permutation of the rows; the kernel visits the cloud in
 * that order (neighbours in space should be neighbours in it: the rejection bound tightens early) and still writes
 * avg[i] for input row i. */
int64_t l4dp_knn_workspace(int64_t n);
int l4dp_knn_mean_dist(const float* points, int64_t n, int32_t k, const int32_t* order, float* avg, void* workspace,
                       void* stream);

/* mu = mean(avg), sd = sqrt(sum((avg - mu)^2) / (n - 1)), both in fp64; keeps points[i] with avg[i] < mu + std_ratio * sd,
 * in input order.  out / out_index / count as in l4dp_range_filter; stats [3] fp64: mu, sd, threshold.
 * workspace: l4dp_compact_workspace(n). */
int l4dp_outlier_filter(const float* points, const float* avg, int64_t n, double std_ratio, float* out, int32_t* out_index,
                        int32_t* count, double* stats, void* workspace, void* stream);

/* RANSAC plane hypotheses of utils/misc.py:18-57,81-93, n_hyp at a time.  triples [n_hyp,3] int32: rows of points.
 *   valid  [n_hyp] int32: 0 if the reference redraws the triple (|y0 - y1| < y_gap, a zero component of p1 - p0, the three
 *          ratios (p2 - p0) / (p1 - p0) all equal, or an index outside [0, n)), else 1
 *   coeffs [n_hyp,4] fp32: un-normalised normal (p1 - p0) x (p2 - p0) and d = -(n . p0), separate fp32 multiplies and
 *          subtractions (numpy's arithmetic on a float32 cloud); zeros where valid is 0
 *   counts [n_hyp] int32: points with |n . p + d| / |n| < threshold; 0 where valid is 0 */
int l4dp_plane_score(const float* points, int64_t n, const int32_t* triples, int32_t n_hyp, float y_gap, float threshold,
                     int32_t* valid, float* coeffs, int32_t* counts, void* stream);

/* mask[i] (uint8, [n]) |= 1 if point i lies within threshold of ANY of the n_planes planes coeffs [n_planes,4]. */
int l4dp_plane_mask(const float* points, int64_t n, const float* coeffs, int32_t n_planes, float threshold, uint8_t* mask,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIDAR4D_PREP_H */
