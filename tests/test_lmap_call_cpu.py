"""The parts of the map store's device-call scaffold that need no HIP (dr_slam_amd/csrc/lmap_call.h), on the host.

The failure paths of a device call cannot be provoked on a GPU, and a second-stage copy with a wrong byte count or offset only
shows when that array happens to decide an output.  tests/native/lmap_call.cpp therefore drives LmapFetch against a fake device,
a std::vector<char>: sections of element sizes 1, 4, 8 and 12 at counts 0, 1, 3, 4, 5 and 300 in mixed order, all sections empty,
a single trailing empty section, and one object sized for its fullest chunk and run again at smaller counts, at nothing but its
one-word total, and at the counts it was sized for.  After every run it compares each section of the host block with the fake
device at its source, and the copies (one per non-empty section), their bytes (count x element size), the block's bytes and the
16-aligned offsets with figures worked out by hand.  It drives LmapWrites against ResidentBlocks bound to two small vectors: armed
then done() sends nothing at the next plan, armed then dropped sends the whole block, not armed sends nothing.
The program is built with plain g++ and links against nothing.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def call_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lmap_call") / "lmap_call")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "native", "lmap_call.cpp"), "-o", exe], check=True)
    return exe


def test_fetch_and_guard_against_a_fake_device(call_exe):
    p = subprocess.run([call_exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "steps 10 failed 0", p.stdout
