"""The device scan (csrc/mm_scan.hip) and the radix sort (csrc/mm_radix_sort.hip) at their tile boundaries, through
Context.unique_points only.  Rows i of the input are (i // 2, 1, 2): every row occurs twice (the last one once when n is
odd), so the unique rows are (j, 1, 2), j = 0 .. ceil(n / 2) - 1, and the inverse of row i is i // 2 -- no np.unique on
the host.

The order-free form scans n head flags (mm_exclusive_scan_int): its sizes put the scan at 1, 1, 1, 2, 2048 and 2049 tiles;
up to 2048 tiles the last kernel sums the tiles before its own, above that the three-kernel form runs, and at 2049 its
single-workgroup offsets kernel loops more than once over the tile sums.  The ordered form sorts the rows
(mm_radix_sort_pairs, whose every pass scans its [digit][tile] counts): its sizes surround one sort tile, and the largest
one has 513 of them."""
import numpy as np
import pytest

# (these mirror csrc/mm_scan.h: kScanTile items per scan tile, kScanSelfTiles tiles in the two-kernel form; and
# csrc/mm_radix_sort.hip: kTile keys per sort tile)
SCAN_TILE = 1024
SCAN_SELF_TILES = 2048
SORT_TILE = 4096
SCAN_SIZES = [1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, SCAN_TILE * SCAN_SELF_TILES, SCAN_TILE * SCAN_SELF_TILES + 1]
SORT_SIZES = [SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, SCAN_TILE * SCAN_SELF_TILES + 1]


@pytest.fixture(scope="module")
def ctx():
    from multimesh_amd.device import Context

    with Context(0) as c:
        yield c


def _rows(n, dim=3, axis=0):
    """n rows whose coordinate `axis` is i // 2; the other coordinates are constants."""
    pts = np.empty((n, dim), dtype=np.float64)
    pts[:] = [5.0, 1.0, 2.0][:dim]
    pts[:, axis] = np.arange(n) // 2
    return pts


def _check_sorted(ctx, pts, perm):
    """unique_points(pts[perm]) is the rows of pts without their copies, in order, and the inverse undoes perm."""
    n = len(pts)
    uniq, inv = ctx.unique_points(pts[perm])
    assert np.array_equal(uniq.numpy(), pts[::2])
    assert np.array_equal(inv.numpy(), perm // 2)
    assert len(pts[::2]) == (n + 1) // 2


@pytest.mark.gpu
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_tile_boundaries_through_the_order_free_unique(ctx, n):
    pts = _rows(n)
    uniq, inv = ctx.unique_points(pts, ordered=False)
    assert np.array_equal(uniq.numpy(), pts[::2])          # first occurrences are in row order
    assert np.array_equal(inv.numpy(), np.arange(n) // 2)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_tile_boundaries_through_the_ordered_unique(ctx, n):
    _check_sorted(ctx, _rows(n), np.random.default_rng(n).permutation(n))


@pytest.mark.gpu
def test_sort_of_one_dimensional_rows_takes_all_64_key_bits(ctx):
    n = SORT_TILE + 1
    _check_sorted(ctx, _rows(n, dim=1), np.random.default_rng(1).permutation(n))   # (first_shift = 0)


@pytest.mark.gpu
def test_rows_with_one_x_take_the_per_component_sorts(ctx):
    # every x coincides: one run of n rows, so the general path sorts by z, by y and by x in turn
    n = SORT_TILE + 1
    _check_sorted(ctx, _rows(n, axis=1), np.random.default_rng(2).permutation(n))
