"""Child process of tests/test_split_sh_gpu.py::test_split_two_kernel_finalisation_in_a_fresh_process: started with
GRUT_GUT_UNFUSED_FINALIZE=1 (the library reads it once per process), so every backward here runs the two-kernel finalisation - the gather
and gut_project_bwd_kernel, whose stage-in / stage-out address maps have a split form.  Runs the C-level comparison of every size
against the twin entry points and ends with a non-zero status on the first mismatch.

    GRUT_GUT_UNFUSED_FINALIZE=1 python tests/split_sh_child.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import split_sh_util as u  # noqa: E402


def main():
    assert os.environ.get("GRUT_GUT_UNFUSED_FINALIZE") == "1", "start me with GRUT_GUT_UNFUSED_FINALIZE=1"
    nat = u.native()
    for n in u.SIZES:
        for n_active in range(4):
            u.check_c_level(nat, n, n_active)
        print(n, flush=True)
    for packed, depth in ((True, False), (False, True)):
        u.check_c_level(nat, 129, 3, packed=packed, depth=depth)
    print(f"split unfused ok: {len(u.SIZES)} sizes")


if __name__ == "__main__":
    main()
