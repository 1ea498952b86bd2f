"""The build description (3dgrut_amd/build.py): one object per csrc/*.hip, per-file flags that name real sources, one compile command for
the build and the scripts.  No GPU, nothing is compiled."""
import importlib
import os

build = importlib.import_module("3dgrut_amd.build")
MAX_ILP = "-amdgpu-sched-strategy=max-ilp"


def test_sources_are_the_hip_files_of_csrc():
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    assert set(build.SOURCES) == {f for f in os.listdir(build.CSRC) if f.endswith(".hip")}


def test_every_per_file_flag_names_a_source():
    assert set(build.FILE_FLAGS) <= set(build.SOURCES)


def test_compile_command_carries_the_per_file_flags():
    render, render_k, grt = (build.compile_command(s) for s in ("gut_render.hip", "gut_render_k.hip", "grt_kernels.hip"))
    assert MAX_ILP in render and render[render.index(MAX_ILP) - 1] == "-mllvm"
    assert MAX_ILP not in render_k                      # the sorted hit buffer's kernels lose with it: a source of their own
    assert "-ffp-contract=on" in grt and grt.index("-ffp-contract=on") > grt.index("-ffp-contract=fast")   # (the last one wins)
    for cmd, src in ((render, "gut_render.hip"), (render_k, "gut_render_k.hip"), (grt, "grt_kernels.hip")):
        assert f"--offload-arch={build.ARCH}" in cmd and os.path.join(build.CSRC, src) in cmd
        assert cmd[cmd.index("-o") + 1] == os.path.join(build.CSRC, src.replace(".hip", ".o"))
    assert "-DX=1" in build.compile_command("knn.hip", ["-DX=1"]) and build.compile_command("knn.hip", out="/dev/null")[-1] == "/dev/null"


def test_a_change_of_the_build_description_rebuilds():
    deps = {os.path.realpath(d) for d in build._deps()}
    assert os.path.realpath(build.__file__) in deps
    assert os.path.realpath(os.path.join(build.CSRC, "gut_render_common.inl")) in deps
