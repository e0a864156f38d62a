"""The granted capacities of the resident-block type (dr_slam_amd/csrc/resident_block.h), on the host.

tests/native/resident_block_capacity.cpp drives one block of three sections against a fake device, a std::vector<char>: no
capacity (today's packed layout, byte for byte), a first grant that moves the section behind it, growth inside the capacity (the
grown tail alone), growth to the last element of the room, a marked section inside its room, one element beyond the capacity (one
new layout, then nothing), a tail a device call wrote itself, an empty section with a capacity and one without.  After every step
it compares each section of the fake device with the host array at the offset the view points to, and the copies and bytes with
figures worked out by hand from the sizes and the 16-byte alignment.  Plain g++, no HIP.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def block_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resident_block_capacity") / "resident_block_capacity")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "native", "resident_block_capacity.cpp"), "-o", exe], check=True)
    return exe


def test_capacities_on_the_fake_device(block_exe):
    p = subprocess.run([block_exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "steps 12 failed 0", p.stdout
