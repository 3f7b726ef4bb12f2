"""The split of the triangular inverse into a leading, a trailing and a top part (bobe_amd/csrc/tri_split.hpp) is a pure
function of the block count.  tests/tri_split_check.cpp checks it for nb = 1 ... 70 - the three parts partition every
depth's problem list, their tile ranges are disjoint and cover the level, every block of the inverse is written once,
nb = 1 yields no fork - as a stand-alone host program under -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_split_partitions_every_level(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "tri_split_check")
    # (the sanitizer runtimes linked into the program itself: it needs nothing preloaded and tolerates what is)
    static_rt = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) in ("g++", "c++") else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", *static_rt, "-o", exe, os.path.join(HERE, "tri_split_check.cpp")],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert run.stdout.strip().endswith("ok 1..70")
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
