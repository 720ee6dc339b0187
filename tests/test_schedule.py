"""The one schedule of the step's riders (csrc/vv_schedule.hpp: series rows, scheduled removals of the centre-of-mass motion, trajectory
frames), host side (no GPU): tests/cpp/schedule_check.cpp, a stand-alone program over that header alone, built with the host sanitizers and
run as its own process (never through Python's loader) -- due_in against a plain walk of due() for both kinds and both positions of a
rider, next_due strictly increasing and independent of where it starts -- and vvhip_frames_schedule against the program's walk."""
import importlib
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

# windows: 8 intervals x 2 kinds x 405 starts, and for LOG10 8 intervals x 110 starts around the powers of ten up to 10^15 (0 .. 4, then 7
# each), each with 5 lengths x 2 positions; walks: 16 schedules x 2 501 starts
CASES = (8 * 2 * 405 + 8 * (5 + 15 * 7)) * 5 * 2 + 16 * 2501


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("schedule") / "schedule_check")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "schedule_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_windows_and_walks_under_asan_and_ubsan(program):
    m = re.search(r"SCHEDULE OK cases=(\d+)", _run(program))
    assert m and int(m.group(1)) == CASES, m


@pytest.mark.parametrize("interval,kind,after,n", [(30, 1, 0, 27), (30, 1, 3, 10), (7, 0, 3, 12), (1, 1, 0, 25), (150, 1, 149, 12), (10, 0, 10, 5),
                                                   (64, 1, 99999, 6)])
def test_frames_schedule_is_the_program_s_walk(program, interval, kind, after, n):
    H = importlib.import_module("openmm-velocityverlet_amd").vvhip
    want = [int(x) for x in _run(program, interval, kind, after, n).split()]
    assert len(want) == n and list(H.frames_schedule(interval, after, n, kind == H.FRAMES_LOG10)) == want
    if (interval, kind, after) == (30, 1, 0):      # GroReporter's pattern, as tests/test_frames.py pins it
        assert want == list(range(30, 100, 10)) + list(range(100, 1000, 100)) + list(range(1000, 10000, 1000)) + [10000, 20000]
