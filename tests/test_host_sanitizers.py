"""The host analysis (csrc/vv_host.cpp: analyze() and its passes -- reference-shaped tables, constraint and site plans, wave clusters, arithmetic
layout with its self-check, wave packing, per-lane and riders' tables) under AddressSanitizer and UndefinedBehaviorSanitizer, CPU build (GPU
sanitizers are not available on this pool): tests/cpp/host_sanitize.cpp analyses 2 000 random plans -- repeated molecules with Drude pairs, hydrogen
constraints, rigid water, molecules larger than a wave, Langevin / image subsets, defects, shards -- and four built rounds for the branches those do
not reach (constraints that cannot be fused, a shard that cuts a molecule, a Drude pair across two molecules, in-order packing from 2^20 lanes).
Every plan is digested whole; tests/golden/host_plan_digests.txt holds the digests of the one-function analyze() that the passes replaced."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_analysis_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "host_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "host_sanitize.cpp"), os.path.join(ROOT, "openmm-velocityverlet_amd", "csrc", "vv_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, "300"], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"HOST SANITIZE OK plans=(\d+) periodic=(\d+)", r.stdout)
    assert m and int(m.group(1)) >= 2000 and int(m.group(2)) > 300, r.stdout
    # every table of every plan, bit for bit
    got = [line for line in r.stdout.splitlines() if line.startswith("round ")]
    with open(os.path.join(ROOT, "tests", "golden", "host_plan_digests.txt")) as f:
        want = f.read().splitlines()
    differing = [(g, w) for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not differing, f"{len(got)} lines for {len(want)}; first differing (got, golden): {differing[:3]}"
    # the branches that only the built rounds reach
    props = dict((k, int(v)) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout.split("properties ", 1)[1]))
    for name in ("unfused", "report_unsupported", "report_cross", "in_order"):
        assert props[name] > 0, (name, props)
