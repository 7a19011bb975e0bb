"""Write tests/golden/point_removal.npz by running the REFERENCE's utils/misc.py (range_filter, estimate_plane, my_ransac).

    python tools/make_golden_pointprep.py --reference /path/to/LiDAR4D

utils/misc.py imports open3d at its top; only the three functions above are called, so an empty stand-in module is registered
under that name.  Nothing of the reference is copied: the fixture holds arrays only -- the input cloud, the rows the
reference's range_filter keeps and, for random.seed(0), (1) and (2), every sample its six my_ransac runs drew (accepted and
rejected), the six inlier sets and models, and random.random() right after the sixth run, on the range-filtered cloud; and the
same six runs (sets, models, random()) on that cloud after the float64 restatement of open3d's statistical outlier removal
(tests/pointprep_ref.py; open3d itself cannot be run), which is where point_removal makes them.
"""
import argparse
import importlib.util
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def load_reference_misc(reference):
    sys.modules.setdefault("open3d", types.ModuleType("open3d"))
    spec = importlib.util.spec_from_file_location("reference_utils_misc", os.path.join(reference, "utils", "misc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "point_removal.npz"))
    args = ap.parse_args()
    misc = load_reference_misc(args.reference)
    import pointprep_ref as ref

    cloud = ref.make_cloud(32, 512)
    kept = misc.range_filter(cloud)
    rf_index = np.flatnonzero(ref.range_filter_mask(cloud)).astype(np.int32)
    assert kept.dtype == np.float32 and np.array_equal(cloud[rf_index], kept)  # stored as rows, checked against the reference's output
    n = len(kept)

    # the band test of tests/test_gpu_pointprep.py assumes that (almost) no point sits at the outlier threshold
    keep, avg, thr = ref.statistical_outlier(kept)
    in_band = int(np.count_nonzero(np.abs(avg - thr) <= 1e-4 * thr))
    assert in_band <= max(1, n // 1000), in_band

    drawn = []
    real_sample = random.sample

    def recording_sample(population, k, **kw):
        s = real_sample(population, k, **kw)
        drawn.append(list(s))
        return s

    def six_runs(data, seeds, record=None):
        """The reference's six my_ransac(0.15) runs on ``data`` per seed -> (inlier masks [S,6,n], models [S,6,4], random() after)."""
        inliers = np.zeros((len(seeds), 6, len(data)), bool)
        models = np.zeros((len(seeds), 6, 4), np.float32)
        rand_after = np.zeros(len(seeds))
        for si, seed in enumerate(seeds):
            random.seed(int(seed))
            for run in range(6):
                del drawn[:]
                random.sample = recording_sample
                try:
                    idx, model = misc.my_ransac(data[:, :3], distance_threshold=0.15)
                finally:
                    random.sample = real_sample
                assert model.dtype == np.float32
                inliers[si, run, idx] = True
                models[si, run] = model
                if record is not None:
                    record(si, run, list(drawn))
            rand_after[si] = random.random()
        return inliers, models, rand_after

    out = {"cloud": cloud, "rf_index": rf_index, "seeds": np.array([0, 1, 2], np.int32)}
    samples, sample_seed, sample_run, sample_valid, sample_model, sample_count = [], [], [], [], [], []

    def record(si, run, run_samples):
        for s3 in run_samples:
            co = None
            if not abs(kept[s3[0], 1] - kept[s3[1], 1]) < 3:
                co = misc.estimate_plane(kept[s3, :], normalize=False)
            samples.append(s3), sample_seed.append(si), sample_run.append(run), sample_valid.append(co is not None)
            sample_model.append(np.zeros(4, np.float32) if co is None else co)
            if co is None:
                sample_count.append(0)
            else:
                r = np.sqrt(co[0] ** 2 + co[1] ** 2 + co[2] ** 2)
                d = np.divide(np.abs(np.matmul(co[:3], kept.T) + co[3]), r)
                sample_count.append(int(np.sum(d < 0.15)))

    inliers, models, rand_after = six_runs(kept, out["seeds"], record)
    # the same runs at their place in point_removal: on the cloud AFTER the first outlier removal.  That step is open3d's in the
    # reference; here it is the float64 restatement (tests/pointprep_ref.py), the RANSAC runs are the reference's own code.
    pipe_inliers, pipe_models, pipe_rand_after = six_runs(kept[keep], out["seeds"])
    out.update(samples=np.array(samples, np.int32), sample_seed=np.array(sample_seed, np.int8), sample_run=np.array(sample_run, np.int8),
               sample_valid=np.array(sample_valid, bool), sample_model=np.stack(sample_model).astype(np.float32),
               sample_count=np.array(sample_count, np.int32), inliers=np.packbits(inliers, axis=-1), n_filtered=np.array(n, np.int64),
               models=models, rand_after=rand_after, pipe_keep=np.packbits(keep), pipe_inliers=np.packbits(pipe_inliers, axis=-1),
               pipe_models=pipe_models, pipe_rand_after=pipe_rand_after)
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {len(cloud)} points, {n} after range_filter, {len(samples)} samples "
          f"({int(np.sum(sample_valid))} accepted), {os.path.getsize(args.out) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
