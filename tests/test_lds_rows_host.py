"""CPU: the swizzled LDS row tile of the matrix kernels (csrc/lds_rows.h) -- the staging side (the XOR on the LDS-DMA source offset)
against the fragment side (the XOR on the ds_read_b128 address), compiled for the host under AddressSanitizer + UBSan in a
stand-alone program (tests/c_abi/lds_rows_check.cpp).  For tiles of 32, 64, 128 and 256 rows it fills an emulated LDS tile through
every staging map the kernels use (per row, 256- and 512-thread workgroups, the 8-row pieces of one wave) from a source whose element
(row, channel) is row * 32 + channel, then reads every fragment of every row base / lane / group back and expects channels
8 G + 4 hh .. + 3 (32x32x2 form) and 4 q .. + 3 | 16 + 4 q .. + 3 (16x16x4 form); the slot map of a row must be a permutation and
the spellings of the fragment offset the kernels use must agree for all arguments.  A kernel whose two sides disagree still runs and
returns wrong numbers: this is the only place the contract can fail before a GPU run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("lds_rows") / "lds_rows_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "iros20-6d-pose-tracking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "lds_rows_check.cpp"), "-o", out])
    return out


def test_staging_and_fragment_sides_agree(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "lds_rows ok" in out.stdout, (out.returncode, out.stdout[-4000:], out.stderr[-4000:])
