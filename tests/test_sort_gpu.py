"""Integer stages on the GPU: scan and radix sort must be bit-exact against numpy (stable order)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sort_reference as ref

pytestmark = pytest.mark.gpu


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("n", [1, 63, 64, 2047, 2048, 2049, 100_000, 1_234_567])
def test_inclusive_scan(grut_lib, n):
    import torch
    rng = np.random.default_rng(n)
    x = rng.integers(0, 50, n, dtype=np.uint32)
    d = torch.as_tensor(x.view(np.int32), device="cuda")
    o = torch.zeros_like(d)
    sb = int(grut_lib.grut_scan_scratch_bytes(n))
    scratch = torch.zeros(sb, dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert grut_lib.grut_inclusive_scan_u32(s, n, _p(d), _p(o), _p(scratch), sb) == 0
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy().view(np.uint32), np.cumsum(x, dtype=np.uint64).astype(np.uint32))


@pytest.mark.parametrize("n,bits", [(1, 32), (100, 32), (4096, 32), (4097, 12), (300_000, 13), (1_000_003, 32), (2_000_000, 8)])
def test_sort_pairs_stable(grut_lib, n, bits):
    import torch
    rng = np.random.default_rng(n + bits)
    hi = (1 << bits) - 1
    keys = rng.integers(0, hi + 1, n, dtype=np.uint64).astype(np.uint32)
    if n > 1000:  # many duplicates -> exercises stability
        keys[: n // 2] = keys[: n // 2] & np.uint32(0xFF)
    vals = np.arange(n, dtype=np.uint32)
    k = torch.as_tensor(keys.view(np.int32), device="cuda")
    v = torch.as_tensor(vals.view(np.int32), device="cuda")
    kt, vt = torch.zeros_like(k), torch.zeros_like(v)
    sb = int(grut_lib.grut_sort_scratch_bytes(n))
    scratch = torch.zeros(sb, dtype=torch.uint8, device="cuda")
    ok, ov = C.c_void_p(), C.c_void_p()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert grut_lib.grut_sort_pairs_u32(s, n, 0, bits, _p(k), _p(v), _p(kt), _p(vt), _p(scratch), sb, C.byref(ok), C.byref(ov)) == 0
    torch.cuda.synchronize()
    sk = (k if ok.value == k.data_ptr() else kt).cpu().numpy().view(np.uint32)
    sv = (v if ov.value == v.data_ptr() else vt).cpu().numpy().view(np.uint32)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(sk, keys[order])
    assert np.array_equal(sv, vals[order])


# ---- every path the frames use, through the stage entry points that expose n_dev, vals_iota, gather and the range kernels ----------
# (references and drivers: tests/sort_reference.py; every driver pre-fills what the call may write with a sentinel)
SMALL_LIMIT = 2_097_152   # the last size on the 8-keys-per-lane kernels (2048-key tiles); above it 16 keys per lane (4096-key tiles)
SCAN_FUSED_LIMIT = 16_777_216   # 8192 scan blocks of 2048: the last size whose apply kernel adds up the block sums itself


@pytest.mark.parametrize("n", [2047, 2048, 2049, SMALL_LIMIT, SMALL_LIMIT + 1, SMALL_LIMIT + 4096 + 63])
def test_sort_sizes(grut_lib, n):
    """Tile edges of the small kernels, the switch to the large ones (its last tile holds one key) and a ragged large tile."""
    ref.check_sort(grut_lib, n, 0, 32, seed=n)


@pytest.mark.parametrize("bits", range(1, 33))
def test_sort_every_width(grut_lib, bits):
    ref.check_sort(grut_lib, 5003, 0, bits, seed=bits)   # three tiles: the cross-block prefix takes part


@pytest.mark.parametrize("begin,end", [(16, 32), (0, 30), (3, 20), (31, 32)])
def test_sort_windows(grut_lib, begin, end):
    ref.check_sort(grut_lib, 5003, begin, end, seed=100 + begin)


def test_sort_empty_window_returns_the_input(grut_lib):
    ref.check_sort(grut_lib, 5003, 5, 5, seed=5)


@pytest.mark.parametrize("n,begin,end", [(5003, 0, 32), (5003, 0, 30), (SMALL_LIMIT + 4096 + 63, 0, 13), (SMALL_LIMIT + 1, 16, 32)])
def test_sort_iota_payload(grut_lib, n, begin, end):
    """`vals` holds poison and is never read: the values that come back are the stable argsort itself."""
    ref.check_sort(grut_lib, n, begin, end, seed=n + end, vals_iota=True)


@pytest.mark.parametrize("n,n_dev", [(10_000, m) for m in (0, 1, 2047, 2048, 2049, 10_000, 4_000_000)] + [(SMALL_LIMIT + 1, 5000), (SMALL_LIMIT + 1, SMALL_LIMIT + 1)])
def test_sort_device_count(grut_lib, n, n_dev):
    """Capacity n, *n_dev live pairs (clamped to n), poison behind them: the live part is sorted, every other word of all four buffers
    keeps what it held."""
    ref.check_sort(grut_lib, n, 0, 32, seed=n_dev + 7, n_dev=n_dev)


@pytest.mark.parametrize("n,n_dev,begin,end,iota", [(10_000, 4097, 0, 13, True), (SMALL_LIMIT + 1, 9001, 0, 13, True), (10_000, 4097, 16, 32, False)])
def test_sort_device_count_combined(grut_lib, n, n_dev, begin, end, iota):
    """The legacy tile-sort call (n_dev + iota payload over bits_for(tiles) bits) and n_dev with a window that does not start at bit 0."""
    ref.check_sort(grut_lib, n, begin, end, seed=n_dev + end, n_dev=n_dev, vals_iota=iota)


GATHER_SIZES = [1, 2047, 2048, 2049, 100_000]


@pytest.mark.parametrize("n", GATHER_SIZES)
def test_scan_gather_permutation(grut_lib, n):
    rng = np.random.default_rng(n)
    ref.check_scan(grut_lib, rng.integers(0, 50, n, dtype=np.uint32), rng.permutation(n))


@pytest.mark.parametrize("n", GATHER_SIZES)
def test_scan_gather_repeated_indices(grut_lib, n):
    rng = np.random.default_rng(n + 1)
    src = n // 3 + 1
    ref.check_scan(grut_lib, rng.integers(0, 50, src, dtype=np.uint32), rng.integers(0, src, n))


@pytest.mark.parametrize("n", [SCAN_FUSED_LIMIT, SCAN_FUSED_LIMIT + 1])
def test_scan_fused_limit(grut_lib, n):
    """8192 blocks: the last fused size (32 block sums per thread); one element more: the single-block scan of the sums + plain apply."""
    ref.check_scan(grut_lib, np.random.default_rng(n).integers(0, 50, n, dtype=np.uint32))


@pytest.mark.parametrize("gather", [False, True])
def test_scan_wraps_modulo_2_32(grut_lib, gather):
    n = 100_001
    rng = np.random.default_rng(31)
    x = (np.uint32(1 << 31) - rng.integers(0, 1000, n, dtype=np.uint32)).astype(np.uint32)
    assert int(x[:3].astype(np.uint64).sum()) > 1 << 32
    ref.check_scan(grut_lib, x, rng.permutation(n) if gather else None)


RANGE_SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 70_001]
GUT_TILES, GUT_MASK = 700, 1023    # 10 key bits: tiles 700..1023 can be written in a key and are invalid
GRT_BLOCKS = 700


@pytest.mark.parametrize("scenario", ["sparse", "one", "invalid"])
@pytest.mark.parametrize("n", RANGE_SIZES)
def test_gut_tile_ranges(grut_lib, n, scenario):
    rng = np.random.default_rng(n)
    ref.check_tile_ranges(grut_lib, ref.sorted_tiles(rng, n, GUT_TILES, GUT_MASK, scenario), GUT_MASK, GUT_TILES, seed=n)


@pytest.mark.parametrize("scenario", ["sparse", "one", "invalid"])
@pytest.mark.parametrize("n", RANGE_SIZES)
def test_grt_list_ranges(grut_lib, n, scenario):
    rng = np.random.default_rng(n)
    ref.check_list_ranges(grut_lib, ref.sorted_tiles(rng, n, GRT_BLOCKS, 0xFFFFFFFF, scenario), GRT_BLOCKS, seed=n)


@pytest.mark.parametrize("n_dev", [0, 1, 4, 1025, 33_333, 70_001, 100_000])
def test_ranges_device_count(grut_lib, n_dev):
    """Capacity 70 001, *n_dev live entries (clamped), unsorted valid tiles as poison behind them."""
    n = 70_001
    live = min(n, n_dev)
    rng = np.random.default_rng(n_dev)
    tiles = np.concatenate([ref.sorted_tiles(rng, live, GUT_TILES, GUT_MASK, "invalid") if live else np.zeros(0, np.uint32), np.zeros(n - live, np.uint32)])
    ref.check_tile_ranges(grut_lib, tiles, GUT_MASK, GUT_TILES, seed=n_dev, n_dev=n_dev)
    blocks = np.concatenate([ref.sorted_tiles(rng, live, GRT_BLOCKS, 0xFFFFFFFF, "invalid") if live else np.zeros(0, np.uint32), np.zeros(n - live, np.uint32)])
    ref.check_list_ranges(grut_lib, blocks, GRT_BLOCKS, seed=n_dev, n_dev=n_dev)


def test_checks_notice_a_perturbed_reference(grut_lib):
    """The net has to hold: one case of each family against a slightly wrong reference must fail."""
    def unstable(keys, b, e):    # a valid order of the digits, equal digits reversed
        return len(keys) - 1 - np.argsort(ref.digits(keys, b, e)[::-1], kind="stable")

    def scan_exclusive(x, gather=None):
        r = ref.scan_reference(x, gather)
        return np.concatenate([[0], r[:-1]]).astype(np.uint32)

    def tile_ranges_off_by_one(keys, mask, tiles, seg):
        r, b = ref.tile_ranges_reference(keys, mask, tiles, seg)
        r[r[:, 1] > 0, 1] -= 1
        return r, b

    def boundary_shifted(keys, mask, tiles, seg):
        r, b = ref.tile_ranges_reference(keys, mask, tiles, seg)
        return r, np.roll(b, 1)

    def list_ranges_off_by_one(keys, blocks):
        r = ref.list_ranges_reference(keys, blocks)
        r[r[:, 1] > 0, 0] += 1
        return r

    rng = np.random.default_rng(0)
    tiles = ref.sorted_tiles(rng, 70_001, GUT_TILES, GUT_MASK, "sparse")
    blocks = ref.sorted_tiles(rng, 70_001, GRT_BLOCKS, 0xFFFFFFFF, "sparse")
    perturbed = [
        lambda: ref.check_sort(grut_lib, 5003, 0, 13, seed=1, order_fn=unstable),
        lambda: ref.check_sort(grut_lib, 5003, 0, 13, seed=1, vals_iota=True, n_dev=4097, order_fn=unstable),
        lambda: ref.check_scan(grut_lib, rng.integers(0, 50, 5003, dtype=np.uint32), rng.permutation(5003), scan_fn=scan_exclusive),
        lambda: ref.check_tile_ranges(grut_lib, tiles, GUT_MASK, GUT_TILES, seed=1, ranges_fn=tile_ranges_off_by_one),
        lambda: ref.check_tile_ranges(grut_lib, tiles, GUT_MASK, GUT_TILES, seed=1, ranges_fn=boundary_shifted),
        lambda: ref.check_list_ranges(grut_lib, blocks, GRT_BLOCKS, seed=1, ranges_fn=list_ranges_off_by_one),
    ]
    for call in perturbed:
        with pytest.raises(AssertionError, match="differ"):   # (the comparison itself, not a failed call)
            call()
    # and the unperturbed twins pass
    ref.check_sort(grut_lib, 5003, 0, 13, seed=1)
    ref.check_tile_ranges(grut_lib, tiles, GUT_MASK, GUT_TILES, seed=1)
    ref.check_list_ranges(grut_lib, blocks, GRT_BLOCKS, seed=1)


def test_misaligned_pointers_are_refused(grut_lib):
    """keys / keys_tmp of the sort, in (without gather) / out of the scan and the range kernels' key lists are read or written 16 bytes at
    a time: a pointer 4 bytes off is GRUT_ERR_BAD_INPUT with a message, before anything is launched."""
    import torch
    n = 5000
    buf = [torch.zeros(n + 8, dtype=torch.int32, device="cuda") for _ in range(4)]
    sb = int(grut_lib.grut_sort_scratch_bytes(n))
    scratch = torch.zeros(max(sb, int(grut_lib.grut_scan_scratch_bytes(n))), dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok, ov = C.c_void_p(), C.c_void_p()
    for off_keys, off_tmp in ((4, 0), (0, 4)):
        p = [ref._p(buf[0], off_keys), _p(buf[1]), ref._p(buf[2], off_tmp), _p(buf[3])]
        assert grut_lib.grut_sort_pairs_u32(s, n, 0, 32, *p, _p(scratch), sb, C.byref(ok), C.byref(ov)) != 0
        assert b"16-byte aligned" in grut_lib.grut_last_error()
        assert grut_lib.grut_debug_sort_pairs_u32(s, n, None, 0, 32, *p, 0, _p(scratch), sb, C.byref(ok), C.byref(ov)) != 0
        assert b"16-byte aligned" in grut_lib.grut_last_error()
    for off_in, off_out in ((4, 0), (0, 4)):
        assert grut_lib.grut_inclusive_scan_u32(s, n, ref._p(buf[0], off_in), ref._p(buf[1], off_out), _p(scratch), scratch.numel()) != 0
        assert b"16-byte aligned" in grut_lib.grut_last_error()
    assert grut_lib.grut_debug_scan_gather_u32(s, n, _p(buf[0]), _p(buf[2]), ref._p(buf[1], 4), _p(scratch), scratch.numel()) != 0   # out, with gather
    assert b"16-byte aligned" in grut_lib.grut_last_error()
    seg = C.c_uint32()
    assert grut_lib.gut_debug_tile_ranges(s, n, None, 1023, 700, ref._p(buf[0], 4), _p(buf[1]), _p(buf[2]), C.byref(seg)) != 0
    assert b"16-byte aligned" in grut_lib.grut_last_error()
    assert grut_lib.grt_debug_list_ranges(s, n, None, 700, ref._p(buf[0], 4), _p(buf[1])) != 0
    assert b"16-byte aligned" in grut_lib.grut_last_error()
    torch.cuda.synchronize()
    assert all(int(b.abs().max()) == 0 for b in buf)


def test_onesweep_sort_in_a_fresh_process(grut_lib):
    """GRUT_SORT_ONESWEEP=1 is read once per process: a fresh child repeats a subset of the sort matrix through the same drivers with the
    one-sweep passes (global histogram + decoupled look-back) selected and exits non-zero on the first mismatch.  The look-back spins on
    status words, so the child has a time limit of its own and is killed when it runs out."""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, GRUT_SORT_ONESWEEP="1")
    legacy_bytes = int(grut_lib.grut_sort_scratch_bytes(10_000))   # (this process runs the three-kernel passes: the child's layout must be larger)
    assert not os.environ.get("GRUT_SORT_ONESWEEP")
    r = subprocess.run([sys.executable, os.path.join(tests, "sort_onesweep_child.py"), str(legacy_bytes)], env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "onesweep ok" in r.stdout
