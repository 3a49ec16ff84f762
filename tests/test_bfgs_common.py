"""The pure helpers of the host BFGS family (csrc/host/bfgs_helpers.hpp: the in-place compaction
of the active-set recursion, the owner / slot arithmetic of the pooled line searches, linspace,
vector_min): tests/cpp/bfgs_common_check.cpp checks them exhaustively at small sizes.  Plain host
code, built with AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program; no
device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_positions_pool_slots_and_helpers_sanitizer_clean(tmp_path):
    exe = str(tmp_path / "bfgs_common_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "bfgs_common_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    assert b"bfgs_common_check: clean" in r.stdout
