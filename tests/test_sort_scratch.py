"""grut_sort_scratch_bytes(n) is an upper bound of what every tile geometry of the three-kernel radix passes needs: the digit-major
histogram matrix (256 rows of one count per workgroup, each row padded to a multiple of 4 words) and the 256 digit totals behind it.
Host arithmetic only: no GPU."""
import pytest

GEOMETRIES = [2048, 4096, 8192, 16384]   # keys per workgroup
SMALL_LIMIT = 2_097_152                  # the host's threshold between the 2048-key tiles and the large arrays' geometry
RADIX = 256


def needed_bytes(n, tile):
    workgroups = (n + tile - 1) // tile
    row = (workgroups + 3) // 4 * 4
    return RADIX * row * 4 + RADIX * 4


def grid():
    ns = {1, 2, 63, 64, 65, 1_000_000, 11_500_000, 17_250_000, 2**31 - 1, 2**31, 2**31 + 1, 2**32 - 2048, 2**32 - 2047, 2**32 - 1}
    for t in GEOMETRIES:
        for m in (1, 2, 3, 4, 5, 1023, 1024):
            ns.update({m * t - 1, m * t, m * t + 1})
    ns.update({SMALL_LIMIT - 1, SMALL_LIMIT, SMALL_LIMIT + 1})
    return sorted(ns)


@pytest.mark.parametrize("n", grid())
def test_scratch_covers_every_geometry(grut_lib, n):
    have = int(grut_lib.grut_sort_scratch_bytes(n))
    for tile in GEOMETRIES:
        assert have >= needed_bytes(n, tile), (n, tile, have, needed_bytes(n, tile))


def test_scratch_is_monotone_over_the_grid(grut_lib):
    """Callers size the scratch for a capacity and sort fewer pairs with it."""
    sizes = [int(grut_lib.grut_sort_scratch_bytes(n)) for n in grid()]
    assert sizes == sorted(sizes)
