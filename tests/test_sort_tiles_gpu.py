"""Every tile geometry of the radix sort's three-kernel passes, forced through grut_debug_sort_pairs_u32_tiled, against the stable numpy
order of tests/sort_reference.py.  Integer work: every comparison is equality, and every word a call must not touch is compared too."""
import ctypes as C

import numpy as np
import pytest

import sort_reference as ref

pytestmark = pytest.mark.gpu

GEOMETRIES = [2048, 4096, 8192, 16384]    # keys per workgroup: 256 x 8, 256 x 16, 512 x 16, 1024 x 16
SMALL_LIMIT = 2_097_152                    # the last size for which the library itself picks 2048-key tiles


def run_sort(lib, tile, keys, begin_bit, end_bit, vals=None, n_dev=None, capacity=None):
    """One forced-geometry call on `capacity` slots whose first len(keys) hold keys / vals (vals None: iota payload, the values buffer
    holds poison) and the rest poison; n_dev None passes a NULL count.  Asserts the live part against the stable order and that every
    other word of the four buffers and their guard words kept what it held."""
    import torch
    live = len(keys)
    n = live if capacity is None else capacity
    assert live == (n if n_dev is None else min(n_dev, n))
    k0 = np.full(n, ref.POISON, dtype=np.uint32)
    k0[:live] = keys
    v0 = np.full(n, ref.POISON, dtype=np.uint32)
    if vals is not None:
        v0[:live] = vals
    before = [ref._padded(k0), ref._padded(v0), np.full(n + ref.PAD, ref.SENTINEL, dtype=np.uint32), np.full(n + ref.PAD, ref.SENTINEL, dtype=np.uint32)]
    k, v, kt, vt = [ref._dev(b) for b in before]
    count = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device="cuda")
    sb = int(lib.grut_sort_scratch_bytes(n))
    scratch = torch.full((sb,), 0x5A, dtype=torch.uint8, device="cuda")
    ok, ov = C.c_void_p(), C.c_void_p()
    status = lib.grut_debug_sort_pairs_u32_tiled(ref._stream(), n, ref._p(count) if count is not None else None, begin_bit, end_bit,
                                                 ref._p(k), ref._p(v), ref._p(kt), ref._p(vt), int(vals is None), tile, ref._p(scratch), sb,
                                                 C.byref(ok), C.byref(ov))
    assert status == 0, lib.grut_last_error()
    torch.cuda.synchronize()
    after = [ref._host(t) for t in (k, v, kt, vt)]
    assert (ok.value, ov.value) in ((k.data_ptr(), v.data_ptr()), (kt.data_ptr(), vt.data_ptr())), "result pointers are not one of the two pairs"
    sk, sv = (after[0], after[1]) if ok.value == k.data_ptr() else (after[2], after[3])
    order = ref.sort_order(k0[:live], begin_bit, end_bit)
    assert np.array_equal(sk[:live], k0[:live][order]), "sorted keys differ"
    payload = np.arange(live, dtype=np.uint32) if vals is None else v0[:live]
    assert np.array_equal(sv[:live], payload[order]), "sorted values differ from the stable order"
    for name, a, b in zip(("keys", "values", "keys_tmp", "values_tmp"), after, before):
        assert np.array_equal(a[live:], b[live:]), f"{name}: words at or beyond the live count changed"


def payload(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def sizes(tile):
    return [1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 3]


@pytest.mark.parametrize("tile,n", [(t, n) for t in GEOMETRIES for n in sizes(t)])
def test_sizes_32_bit_key_in_four_passes(grut_lib, tile, n):
    rng = np.random.default_rng(tile + n)
    run_sort(grut_lib, tile, ref.random_keys(rng, n), 0, 32, vals=payload(rng, n))


# every digit width with a window that does not start at bit 0, and the 13 tile bits of the 1080p frame (two passes: 7 + 6 bits)
LAYOUTS = [(5, 5 + w) for w in range(1, 9)] + [(0, 13)]


@pytest.mark.parametrize("begin,end", LAYOUTS)
@pytest.mark.parametrize("tile", GEOMETRIES)
def test_digit_layouts(grut_lib, tile, begin, end):
    n = 2 * tile + 3
    rng = np.random.default_rng(tile + 100 * end)
    run_sort(grut_lib, tile, ref.random_keys(rng, n), begin, end, vals=payload(rng, n))
    run_sort(grut_lib, tile, ref.random_keys(rng, n), begin, end)   # iota payload


def distribution(name, rng, n, begin, end):
    """Keys whose digits in [begin, end) stress the ranking; the bits outside the window are random and must travel with the key."""
    radix = 1 << min(8, end - begin)
    if name == "equal":
        d = np.full(n, 3 % radix, dtype=np.uint32)
    elif name == "two":
        d = np.where(rng.integers(0, 2, n) == 1, radix - 1, 0).astype(np.uint32)
    elif name == "lane":
        d = ((np.arange(n) % 64) % radix).astype(np.uint32)
    else:
        return ref.random_keys(rng, n)
    window = np.uint32(((1 << (end - begin)) - 1) << begin)
    noise = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & ~window
    return (d << np.uint32(begin)) | noise


@pytest.mark.parametrize("dist", ["equal", "two", "lane", "random"])
@pytest.mark.parametrize("tile", GEOMETRIES)
def test_key_distributions(grut_lib, tile, dist):
    n = 2 * tile + 3
    rng = np.random.default_rng(tile + len(dist))
    for begin, end in ((0, 13), (5, 13), (0, 32)):
        run_sort(grut_lib, tile, distribution(dist, rng, n, begin, end), begin, end, vals=payload(rng, n))


@pytest.mark.parametrize("iota", [False, True])
@pytest.mark.parametrize("which", ["zero", "one", "tile_plus_one", "capacity"])
@pytest.mark.parametrize("tile", GEOMETRIES)
def test_device_count_below_capacity(grut_lib, tile, which, iota):
    """The speculative tail's call: capacity 1.5 x (T + 1) slots, *n_dev live pairs; nothing at or beyond the count may change."""
    capacity = 3 * (tile + 1) // 2
    n_dev = {"zero": 0, "one": 1, "tile_plus_one": tile + 1, "capacity": capacity}[which]
    rng = np.random.default_rng(tile + n_dev)
    run_sort(grut_lib, tile, ref.random_keys(rng, n_dev), 0, 13, vals=None if iota else payload(rng, n_dev), n_dev=n_dev, capacity=capacity)


@pytest.mark.parametrize("begin,end", [(0, 13), (16, 32)])   # 7 + 6 bits, and two 8-bit digits
@pytest.mark.parametrize("n", [SMALL_LIMIT, SMALL_LIMIT + 1])
def test_automatic_choice_on_both_sides_of_the_threshold(grut_lib, n, begin, end):
    """tile_keys = 0: the library picks the geometry - 2048-key tiles up to the limit, the large arrays' tile one key above it."""
    rng = np.random.default_rng(n + end)
    run_sort(grut_lib, 0, ref.random_keys(rng, n), begin, end)


def test_unknown_geometry_is_refused(grut_lib):
    import torch
    n = 5000
    buf = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(4)]
    sb = int(grut_lib.grut_sort_scratch_bytes(n))
    scratch = torch.zeros(sb, dtype=torch.uint8, device="cuda")
    ok, ov = C.c_void_p(), C.c_void_p()
    assert grut_lib.grut_debug_sort_pairs_u32_tiled(ref._stream(), n, None, 0, 32, *[ref._p(b) for b in buf], 0, 1000, ref._p(scratch), sb,
                                                    C.byref(ok), C.byref(ov)) != 0
    assert b"tile_keys" in grut_lib.grut_last_error()
