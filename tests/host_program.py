"""Stand-alone host C++ programs of the test-suite: the packed weight forms of sigmarl_amd/csrc/sigmaenv_pack.h against tests/weight_pack_reference.h
(tests/test_weight_load_host.py, tests/test_gradient_check.py).  A program is compiled on its own, linked with nothing of the library, and run as a child process."""
import os
import shutil
import subprocess

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "sigmarl_amd", "csrc")


def compiler():
    return shutil.which("g++") or shutil.which("c++")


def build_and_run(tmp_path, name, source):
    """Writes `source` to tmp_path/name.cpp, compiles it (-std=c++17 -O1 -ffp-contract=off, the library's sources and tests/ on the include path) with AddressSanitizer +
    UBSan where the compiler has them, plainly otherwise, runs it and returns its stdout; a non-zero exit status fails with the end of its output."""
    src, exe = tmp_path / (name + ".cpp"), tmp_path / name
    src.write_text(source)
    base = [compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, "-I", TESTS, str(src), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:  # (a compiler without the sanitizer runtimes: the comparison itself does not need them)
        subprocess.check_call(base)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout[-4000:], run.stderr[-4000:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    return run.stdout
