"""The device-block layout of the host-pointer batched calls (csrc/host_block.hpp, used by
pnol_run_levmarq_batch / pnol_run_simplex_batch / pnol_run_bfgs_batch): tests/cpp/host_block_check.cpp
lays out the array lists those calls pass, with the optional arrays present and absent, and
checks alignment, overlap and the total.  Plain host code, built with AddressSanitizer and
UndefinedBehaviorSanitizer as a stand-alone program; no device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_is_aligned_disjoint_and_sanitizer_clean(tmp_path):
    exe = str(tmp_path / "host_block_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "host_block_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    assert b"host_block_check: clean" in r.stdout
