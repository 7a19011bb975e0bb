"""Edge tests of the range-image conversions on the device (``-m gpu``, MI355X): l4d_pano_to_lidar (ordered compaction: order,
count, what is left alone, special ranges, coordinates against float64) and l4d_lidar_to_pano (exact binning of unambiguous clouds,
competition inside a pixel, the range gate, dropped points, writes, bin edges), through the C ABI with prefilled buffers.

The check bodies, the cases, the references and the bounds are in tests/convert_cases.py; tests/test_convert_cpu.py runs the same
bodies against a float32 restatement of the kernels, with and without faults."""
import numpy as np
import pytest
import torch

import convert_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32


def _ops():
    from lidar4d_amd import ops
    return ops


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def run_pano(pano, inten, H, W, K, points, count):
    from lidar4d_amd import _lib
    ops = _ops()
    p = ops._p
    d_pano, d_inten, d_points, d_count = dev(pano), dev(inten), dev(points), dev(count)
    ws = torch.empty(max(4, _lib.lib().l4d_pano_to_lidar_workspace(H, W)), dtype=torch.uint8, device=DEV)
    ops.call("l4d_pano_to_lidar", p(d_pano), p(d_inten), H, W, float(K[0]), float(K[1]), p(d_points), p(d_count), p(ws), ops._stream())
    torch.cuda.synchronize()
    return host(d_points), host(d_count), host(d_pano).reshape(H, W), None if inten is None else host(d_inten).reshape(H, W)


def run_lidar(points, N, H, W, K, max_depth, pano, inten):
    from lidar4d_amd import _lib
    ops = _ops()
    p = ops._p
    d_points = dev(points) if N else torch.zeros(4, device=DEV)
    d_pano, d_inten = dev(pano), dev(inten)
    ws = torch.empty(max(8, _lib.lib().l4d_lidar_to_pano_workspace(H, W)), dtype=torch.uint8, device=DEV)
    ops.call("l4d_lidar_to_pano", p(d_points), N, H, W, float(K[0]), float(K[1]), float(max_depth), p(d_pano), p(d_inten), p(ws),
             ops._stream())
    torch.cuda.synchronize()
    return host(d_pano), host(d_inten), host(d_points).reshape(-1, 4)[:N] if N else points


# =================================================================================================================================
# 1a. pano_to_lidar
# =================================================================================================================================
@pytest.mark.parametrize("H,W", cc.pano_shapes() + [(0, 7), (7, 0)])
def test_pano_to_lidar_order_count_and_untouched_rows(H, W):
    """Every occupancy pattern, with intensities (= the pixel index: the order, bit for bit) and without (column 3 = +0.0)."""
    worst = 0.0
    for pattern in cc.PATTERNS:
        pano = cc.pano_image(H, W, pattern)
        for with_inten in (True, False):
            worst = max(worst, cc.check_pano_to_lidar(run_pano, H, W, cc.KITTI, pano, with_inten)[2])
    print(f"pano_to_lidar {H} x {W}: largest xyz error {worst:.2f} u |range| (DIR_K = {cc.dir_k(cc.KITTI):.2f})")


@pytest.mark.parametrize("pattern", ["random90", "every_1024th", "full_gap_one", "last", "empty"])
def test_pano_to_lidar_second_sweep_of_the_prefix_loop(pattern):
    """1 x (1024 * 1026 + 5): 1027 workgroups, so workgroups 1025 and 1026 sum the counts in front of them in two sweeps."""
    H, W = cc.PANO_BIG
    worst = cc.check_pano_to_lidar(run_pano, H, W, cc.KITTI, cc.pano_image(H, W, pattern))[2]
    print(f"pano_to_lidar {H} x {W} {pattern}: largest xyz error {worst:.2f} u |range| (DIR_K = {cc.dir_k(cc.KITTI):.2f})")


@pytest.mark.parametrize("H,W,K", [(1, 65, cc.WIDE), (5, 13, cc.WIDE), (41, 25, cc.MID)])
def test_pano_to_lidar_special_ranges(H, W, K):
    """-0.0 is dropped; a negative range, NaN, +inf, the smallest subnormal and 3e38 are kept, with the float64 product's sign,
    NaN or inf."""
    cc.check_pano_special(run_pano, H, W, K)


def test_pano_to_lidar_twice_gives_the_same_bits():
    H, W = 41, 25
    pano = cc.pano_image(H, W, "random90")
    a = cc.check_pano_to_lidar(run_pano, H, W, cc.KITTI, pano)[0]
    b = cc.check_pano_to_lidar(run_pano, H, W, cc.KITTI, pano)[0]
    assert cc.same_bits(a, b).all()


# =================================================================================================================================
# 1b. lidar_to_pano
# =================================================================================================================================
@pytest.mark.parametrize("H,W,K", cc.CLOUD_SHAPES)
def test_lidar_to_pano_unambiguous_cloud_every_pixel_exact(H, W, K):
    cc.check_unambiguous(run_lidar, H, W, K)


@pytest.mark.parametrize("k", cc.CONTEST_K)
@pytest.mark.parametrize("H,W,K", cc.CONTEST_SHAPES)
def test_lidar_to_pano_competition_inside_a_pixel(H, W, K, k):
    """The nearest wins wherever it stands in the array; of equal range bits the lowest index wins, in either direction."""
    cc.check_contested(run_lidar, H, W, K, k)
    cc.check_ties(run_lidar, H, W, K, k)


@pytest.mark.parametrize("max_depth", cc.GATE_DEPTHS)
def test_lidar_to_pano_range_gate(max_depth):
    cc.check_range_gate(run_lidar, max_depth)


@pytest.mark.parametrize("H,W,K", [cc.EDGE_SHAPE, (3, 5, cc.WIDE)])
def test_lidar_to_pano_dropped_points(H, W, K):
    cc.check_dropped(run_lidar, H, W, K)


def test_lidar_to_pano_writes():
    cc.check_writes(run_lidar)


def test_lidar_to_pano_bin_edges():
    cc.check_bin_edges(run_lidar)
