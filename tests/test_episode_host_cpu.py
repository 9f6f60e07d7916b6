"""csrc/episode_host.hpp (the record layout, scatter and rules words every episode entry shares) without a GPU:
tests/episode_host_check.cpp is built with AddressSanitizer (LeakSanitizer included) and UndefinedBehaviorSanitizer, and runs as a child
process of its own - nothing is loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _compilers():
    found = [c for c in (shutil.which("g++"), CLANG if os.path.exists(CLANG) else None) if c]
    assert found, "no host C++ compiler (g++, or the ROCm clang++)"
    return found


@pytest.mark.parametrize("cxx", _compilers(), ids=os.path.basename)
def test_episode_host_check_under_sanitizers(cxx, tmp_path):
    exe = str(tmp_path / "episode_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "dust_amd", "csrc"), os.path.join(ROOT, "tests", "episode_host_check.cpp"), "-o", exe]
    if os.path.basename(cxx) == "g++":  # the sanitizer runtimes inside the program, as clang++ links them: no library order to mind
        cmd += ["-static-libasan", "-static-libubsan"]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip().endswith("episode_host ok"), run.stdout
