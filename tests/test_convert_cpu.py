"""CPU tests of the references in tests/convert_cases.py, which tests/test_gpu_convert_edges.py compares the conversion kernels
with: the float32 restatements are oracle/convert_ref.py (itself pinned to the reference project by tests/golden/convert.npz) on
every cloud and image used, the direction bound holds for the restated pixel_dir with a factor two to spare, every cloud keeps its
bin-edge margin, every check body passes against the restatement and fails against it with a fault switched on.  Prints the
measurements that tests/convert_cases.py records."""
import numpy as np
import pytest

import convert_cases as cc
from oracle import convert_ref

F32, F64 = np.float32, np.float64


# ---- pano_to_lidar --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,K", [(64, 2048, cc.KITTI), (3, 5, cc.WIDE), (66, 515, cc.MID), (1, cc.PANO_BIG[1], cc.KITTI)])
def test_direction_bound_holds_for_the_restatement_with_a_factor_two(H, W, K):
    idx = np.arange(H * W)
    err = float(np.abs(cc.pixel_dirs_f32(H, W, K, idx).astype(F64) - cc.pixel_dirs64(H, W, K, idx)).max() / cc.U)
    print(f"direction error {H} x {W} K={K}: {err:.2f} u, DIR_K = {cc.dir_k(K):.2f}, spare factor {cc.dir_k(K) / err:.2f}")
    assert 2.0 * err <= cc.dir_k(K)


def test_dir_k_values_are_the_recorded_ones():
    assert [round(cc.dir_k(K), 2) for K in (cc.KITTI, cc.WIDE, cc.MID)] == [11.49, 12.62, 11.49]


@pytest.mark.parametrize("H,W", [(3, 5), (33, 31), (3, 683)])
def test_pano_restatement_is_the_oracle(H, W):
    for pattern in cc.PATTERNS:
        pano = cc.pano_image(H, W, pattern)
        inten = np.arange(H * W, dtype=F32).reshape(H, W)
        ref = convert_ref.pano_to_lidar_with_intensities(pano, inten, cc.KITTI)
        points, count = np.full((H * W + 1, 4), cc.SENT, F32), np.array([-7], np.int32)
        cc.pano_to_lidar_f32(pano, inten, H, W, cc.KITTI, points, count)
        assert int(count[0]) == ref.shape[0] and np.array_equal(points[:ref.shape[0], 3], ref[:, 3])
        assert cc.same_bits(points[:ref.shape[0]], ref).all(), "the restated pixel_dir is the oracle's arithmetic, bit for bit"


@pytest.mark.parametrize("H,W", cc.pano_shapes() + [(0, 7), (7, 0)])
def test_pano_bodies_pass_against_the_restatement(H, W):
    for pattern in cc.PATTERNS:
        for with_inten in (True, False):
            cc.check_pano_to_lidar(cc.run_pano_f32(), H, W, cc.KITTI, cc.pano_image(H, W, pattern), with_inten)


def test_pano_special_ranges_against_the_restatement():
    for H, W in ((1, 65), (5, 13), (41, 25)):
        cc.check_pano_special(cc.run_pano_f32(), H, W, cc.WIDE)
    kept = np.array([-0.0, 1e-45, np.nan], F32) != 0
    assert kept.tolist() == [False, True, True]  # numpy keeps the subnormal and NaN


def test_pano_fault_prefix_one_sweep_is_caught_only_by_the_large_count():
    """The large image, random 90 %: passes as restated; with a prefix loop that stops after one sweep workgroups 1025 and 1026
    get a base that lacks workgroup 1024's points, and the order check fails.  The small counts cannot see it."""
    H, W = cc.PANO_BIG
    pano = cc.pano_image(H, W, "random90")
    cc.check_pano_to_lidar(cc.run_pano_f32(), H, W, cc.KITTI, pano)
    with pytest.raises(AssertionError, match="count|column 3"):
        cc.check_pano_to_lidar(cc.run_pano_f32("prefix_one_sweep"), H, W, cc.KITTI, pano)
    cc.check_pano_to_lidar(cc.run_pano_f32("prefix_one_sweep"), 1, 2049, cc.KITTI, cc.pano_image(1, 2049, "random90"))


# ---- lidar_to_pano --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,K", cc.CLOUD_SHAPES_CPU)
def test_clouds_keep_their_margin_and_their_own_pixels(H, W, K):
    """The condition of the exact test: every fp32 point is >= 0.2 px from a bin edge in float64, and oracle/convert_ref.py puts
    every point in its own pixel with pano == sqrt_f32((x^2 + y^2) + z^2) bit for bit."""
    seeds = [0] if H * W > 40000 else [0, 20, 30, 40, 50] + list(range(10, 15))
    for seed in seeds:
        pts, pix = cc.cloud(H, W, K, seed=seed)
        margin = cc.cloud_margin(pts, pix, H, W, K)
        if seed == 0:
            print(f"bin-edge margin {H} x {W} K={K}: {margin:.3f} px")
        assert margin >= cc.MARGIN_MIN
        pano, inten = cc.own_pixel_image(pts, pix, H, W)
        rp, ri = convert_ref.lidar_to_pano_with_intensities(pts, H, W, K)
        assert cc.same_bits(rp, pano).all() and cc.same_bits(ri, inten).all()
        p, i = cc.lidar_to_pano_f32(pts, H, W, K, 80.0)
        assert cc.same_bits(p, pano).all() and cc.same_bits(i, inten).all()


def test_lidar_restatement_is_the_oracle_on_contested_and_dropped_clouds():
    for H, W, K in cc.CONTEST_SHAPES:
        for k in cc.CONTEST_K:
            pts, pano, inten = cc.contested(H, W, K, k, k // 2)
            with np.errstate(all="ignore"):
                rp, ri = convert_ref.lidar_to_pano_with_intensities(pts, H, W, K)
            assert cc.same_bits(rp, pano).all() and cc.same_bits(ri, inten).all()
    H, W, K = cc.EDGE_SHAPE
    extra, names = cc.dropped_points(H, W, K)
    assert len(names) == 7 + 15
    with np.errstate(all="ignore"):
        rp, ri = convert_ref.lidar_to_pano_with_intensities(extra, H, W, K)
    assert not rp.any() and not ri.any(), "the oracle drops every one of them"


def test_lidar_bodies_pass_against_the_restatement():
    run = cc.run_lidar_f32()
    for H, W, K in cc.CLOUD_SHAPES:
        cc.check_unambiguous(run, H, W, K)
    for H, W, K in cc.CONTEST_SHAPES:
        for k in cc.CONTEST_K:
            cc.check_contested(run, H, W, K, k)
            cc.check_ties(run, H, W, K, k)
    for md in cc.GATE_DEPTHS:
        cc.check_range_gate(run, md)
    cc.check_dropped(run, *cc.EDGE_SHAPE)
    cc.check_dropped(run, 3, 5, cc.WIDE)
    cc.check_writes(run)
    cc.check_bin_edges(run)


def test_lidar_faults_are_caught():
    """A tie broken by the highest index fails the tie body (and no other); <= at max_depth fails the range gate (and no other)."""
    tie, le = cc.run_lidar_f32("tie_highest"), cc.run_lidar_f32("depth_le")
    for H, W, K in cc.CONTEST_SHAPES:
        with pytest.raises(AssertionError, match="tie of 2"):
            cc.check_ties(tie, H, W, K, 2)
        cc.check_contested(tie, H, W, K, 3)
        cc.check_ties(le, H, W, K, 2)
    for md in cc.GATE_DEPTHS:
        with pytest.raises(AssertionError, match="at max_depth"):
            cc.check_range_gate(le, md)
        cc.check_range_gate(tie, md)
