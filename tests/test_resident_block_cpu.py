"""The resident-block type of the map store (dr_slam_amd/csrc/resident_block.h), on the host.

A section that stays behind on the device, or lands at another offset than the view says, only shows in a kernel when that array
happens to decide an output.  tests/native/resident_block.cpp therefore drives one block of five sections (uint8_t, int32_t, float,
double, int32_t) against a fake device, a std::vector<char>, through every kind of edit: the first sync, a sync with nothing
marked, a marked prefix, a tail after the last array shrank, prefix and tail in one sync, a middle array resized with only the last
section marked, growth past the capacity, a middle section of zero elements, assume_current() after stale_all(), single elements,
and a block whose arrays are all empty.  After every step it compares each section of the fake device with the host array at the
offset the view points to, and the copies and bytes with figures worked out by hand from the sizes and the 16-byte alignment.
The header's plan-pack-point part needs no HIP: the program is built with plain g++ and links against nothing.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def block_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resident_block") / "resident_block")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "native", "resident_block.cpp"), "-o", exe], check=True)
    return exe


def test_every_kind_of_edit_reaches_the_fake_device(block_exe):
    p = subprocess.run([block_exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "steps 12 failed 0", p.stdout
