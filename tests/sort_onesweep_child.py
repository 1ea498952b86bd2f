"""Child process of tests/test_sort_gpu.py::test_onesweep_sort_in_a_fresh_process: started with GRUT_SORT_ONESWEEP=1 (the library reads
it once per process), runs a subset of the sort matrix through the drivers of tests/sort_reference.py - which size the scratch with
this process's own grut_sort_scratch_bytes - and ends with a non-zero status on the first mismatch.

    GRUT_SORT_ONESWEEP=1 python tests/sort_onesweep_child.py <grut_sort_scratch_bytes(10000) of a process without the switch>
"""
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import sort_reference as ref  # noqa: E402

SMALL_LIMIT = 2_097_152


def main():
    assert os.environ.get("GRUT_SORT_ONESWEEP") == "1", "start me with GRUT_SORT_ONESWEEP=1"
    lib = importlib.import_module("3dgrut_amd._abi").load_library()
    # the status words of the look-back make the one-sweep scratch layout the larger one: this process has selected it
    assert int(lib.grut_sort_scratch_bytes(10_000)) > int(sys.argv[1]), "the one-sweep passes are not selected"
    cases = [dict(n=n, begin_bit=0, end_bit=32) for n in (2047, 2048, 2049, SMALL_LIMIT, SMALL_LIMIT + 1, SMALL_LIMIT + 4096 + 63)]
    cases += [dict(n=5003, begin_bit=0, end_bit=b) for b in (1, 13, 30, 32)]
    cases += [dict(n=5003, begin_bit=16, end_bit=32)]
    cases += [dict(n=5003, begin_bit=0, end_bit=30, vals_iota=True), dict(n=SMALL_LIMIT + 1, begin_bit=0, end_bit=13, vals_iota=True)]
    cases += [dict(n=10_000, begin_bit=0, end_bit=32, n_dev=m) for m in (0, 1, 2047, 2048, 2049, 10_000, 4_000_000)]
    cases += [dict(n=SMALL_LIMIT + 1, begin_bit=0, end_bit=13, n_dev=9001, vals_iota=True), dict(n=10_000, begin_bit=16, end_bit=32, n_dev=4097)]
    for i, case in enumerate(cases):
        print(case, flush=True)
        ref.check_sort(lib, seed=1000 + i, **case)
    print(f"onesweep ok: {len(cases)} cases")


if __name__ == "__main__":
    main()
