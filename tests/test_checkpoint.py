"""Checkpoints and the state digest (include/vvhip.h: "checkpoint"), host side (no GPU): the digest's known answers from the NumPy
statement, vvhip_digest_host against it, the exports, the blob's structs against the header as a C compiler sees them, a blob WRITTEN BY
NUMPY from the documented format through vvhip_checkpoint_inspect, its corruptions refused by name, the refusals that need no device, and
the parser on hostile bytes under the host sanitizers (a stand-alone program, never through Python's loader)."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import checkpoint_cases as K       # noqa: E402
import digest_reference as ref     # noqa: E402


def _H():
    return importlib.import_module("openmm-velocityverlet_amd.vvhip")


KNOWN = [(b"", 0, "0"), (bytes(4), 0, "e220a8397b1dcdaf"), (np.arange(8, dtype="<u4"), 0, "ae98ebd8d59a41c4"),
         (np.arange(8, dtype="<u4"), 5, "bff055141ff009b7"), (np.arange(8, dtype="<u4"), 2 ** 32 - 8, "228ffb44074e6bff"),
         (np.arange(1000, dtype=np.float64) * 0.3 - 3.0, 0, "615ceb7d01ed4ef4")]


@pytest.mark.parametrize("data,base,want", KNOWN)
def test_known_answers(data, base, want):
    assert "%x" % ref.digest(data, base) == want
    assert "%x" % _H().digest_host(data, base) == want


@pytest.mark.parametrize("nwords", [0, 1, 3, 63, 64, 65, 1000])
def test_host_digest_equals_numpy(nwords):
    H = _H()
    buf = np.random.default_rng(nwords).integers(0, 2 ** 32, nwords, dtype=np.uint64).astype("<u4")
    for base in (0, 5, 2 ** 32 - nwords):
        assert H.digest_host(buf, base) == ref.digest(buf, base), (nwords, base)
    # ... and at an address that is no multiple of 4 (a blob may sit anywhere)
    raw = C.create_string_buffer(bytes(1) + buf.tobytes())
    out = C.c_uint64(0)
    assert H.lib.vvhip_digest_host(C.addressof(raw) + 1, 4 * nwords, 5, C.byref(out)) == H.OK and out.value == ref.digest(buf, 5)


def test_host_digest_is_additive_over_shards_and_refuses_what_it_cannot_index():
    H = _H()
    buf = np.random.default_rng(3).integers(0, 2 ** 32, 8 * 100, dtype=np.uint64).astype("<u4")      # 100 particles of 8 words
    whole = H.digest_host(buf, 0)
    for cut in (0, 1, 37, 100):
        assert (H.digest_host(buf[:8 * cut], 0) + H.digest_host(buf[8 * cut:], 8 * cut)) & ref.M64 == whole
    out = C.c_uint64(0)
    assert H.lib.vvhip_digest_host(buf.ctypes.data, 6, 0, C.byref(out)) == H.ERR_INVALID              # no multiple of 4
    assert H.lib.vvhip_digest_host(buf.ctypes.data, 32, 2 ** 32 - 7, C.byref(out)) == H.ERR_INVALID   # a word index of 2^32
    assert H.lib.vvhip_digest_host(buf.ctypes.data, 32, 0, None) == H.ERR_INVALID
    assert H.lib.vvhip_digest_host(None, 32, 0, C.byref(out)) == H.ERR_INVALID


def test_entry_points_are_exported():
    H = _H()
    for name in ("vvhip_digest_host", "vvhip_state_digest", "vvhip_checkpoint_size", "vvhip_checkpoint_save", "vvhip_checkpoint_inspect",
                 "vvhip_checkpoint_error", "vvhip_checkpoint_load"):
        assert name in H.EXPORTS, name


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof and every field offset of the header, cursor and table structs, and the constants, printed by a C program built from
    include/vvhip.h -- against the ctypes binding and against the NumPy statement."""
    H = _H()
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler (the build needs one as well)"
    structs = {"vvhip_checkpoint_header": (H.CheckpointHeader, ref.HEADER), "vvhip_checkpoint_cursor": (H.CheckpointCursor, ref.CURSOR),
               "vvhip_checkpoint_section": (H.CheckpointSection, ref.SECTION), "vvhip_params": (H.Params, ref.PARAMS)}
    lines = []
    for s, (ct, _) in structs.items():
        lines.append(f'    printf("%zu", sizeof({s}));\n' + "".join(f'    printf(" %zu", offsetof({s}, {f[0]}));\n' for f in ct._fields_) + '    printf("\\n");\n')
    lines.append('    printf("%llu %d %d %u %u\\n", (unsigned long long) VVHIP_CKPT_MAGIC, VVHIP_CKPT_VERSION, VVHIP_CKPT_SECTIONS, VVHIP_CKPT_ALL, VVHIP_CKPT_INTEGRATOR);\n')
    lines.append('    printf("%d %d %d %d %d %d %d %d %d\\n", VVHIP_CKPT_POSQ, VVHIP_CKPT_CORRECTION, VVHIP_CKPT_VELM, VVHIP_CKPT_FORCE, VVHIP_CKPT_FORCE_EXTRA, VVHIP_CKPT_RANDOM, VVHIP_CKPT_THERMOSTAT, VVHIP_CKPT_EPOCH, VVHIP_CKPT_CURSOR);\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vvhip.h"\nint main(void) {\n' + "".join(lines) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    rows = [[int(x) for x in line.split()] for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    for row, (s, (ct, dt)) in zip(rows, structs.items()):
        assert row[0] == C.sizeof(ct) == dt.itemsize, s
        assert row[1:] == [getattr(ct, f[0]).offset for f in ct._fields_] == [dt.fields[f[0]][1] for f in ct._fields_], s
    assert rows[0][0] == 272 and rows[2][0] == 40 and rows[1][0] == 32
    assert rows[4] == [H.CKPT_MAGIC, H.CKPT_VERSION, H.CKPT_SECTIONS, H.CKPT_ALL, H.CKPT_INTEGRATOR] == [ref.MAGIC, ref.VERSION, 9, 0x1FF, 0x1F0]
    assert rows[5] == list(range(9)) and H.CKPT_SECTION_NAMES == ref.SECTION_NAMES


def test_a_blob_written_by_numpy_passes_inspect_field_for_field():
    H = _H()
    fields, sections = K.hand_made_fields(), K.hand_made_sections()
    blob = K.hand_made_blob()
    h = H.checkpoint_inspect(blob)
    assert (h.magic, h.version, h.num_sections, h.total_bytes) == (H.CKPT_MAGIC, H.CKPT_VERSION, 9, len(blob))
    for k in ("precision", "num_atoms", "shard_begin", "shard_end", "use_middle_scheme", "num_nh_chains", "random_size"):
        assert getattr(h, k) == fields[k], k
    assert tuple(h.box) == fields["box"] and tuple(h.host_words) == fields["host_words"]
    for k, v in fields["cursor"].items():
        assert getattr(h.cursor, k) == v, k
    for f, _ in H.Params._fields_:
        assert getattr(h.params, f) == fields["params"].get(f, 0), f
    table = H.checkpoint_sections(blob)
    assert list(table) == list(H.CKPT_SECTION_NAMES)
    for name, payload in sections.items():
        s = table[name]
        assert s.bytes == len(payload) and s.offset % 16 == 0 and blob[s.offset:s.offset + s.bytes] == payload
        assert s.digest == ref.digest(payload, 0) == H.digest_host(payload, 0) and s.digest_base == 0
    # a blob without the particle arrays (what an OpenMM adapter stores) is as valid
    small = ref.write_blob(fields, {k: v for k, v in sections.items() if k not in K.PARTICLE_ARRAYS})
    assert H.checkpoint_inspect(small).num_sections == 5


def _refused(blob, *needles):
    H = _H()
    with pytest.raises(H.VVHipError) as e:
        H.checkpoint_inspect(blob)
    assert e.value.code == H.ERR_INVALID
    for n in needles:
        assert n in e.value.message, (n, e.value.message)
    return e.value.message


def test_corrupted_blobs_are_refused_by_name():
    H = _H()
    blob = K.hand_made_blob()
    table = H.checkpoint_sections(blob)
    _refused(b"XVHIPCKP" + blob[8:], "magic")
    _refused(blob[:8] + (2).to_bytes(4, "little") + blob[12:], "version")
    for name, s in table.items():                                   # cut at every section boundary and in the middle of every section
        for cut in (s.offset, s.offset + s.bytes // 2):
            _refused(blob[:cut], "truncated", name)
    _refused(blob[:len(blob) - 16], "truncated")
    _refused(blob[:100], "truncated")
    _refused(blob[:272 + 60], "truncated", "table")
    _refused(blob + bytes(16), "size")
    # an offset past the end, in a table whose digest is right: the parser does not trust the table
    h, _ = ref.read_blob(blob)
    t = np.frombuffer(blob[272:272 + 9 * 40], dtype=ref.SECTION).copy()
    t[3]["offset"] = len(blob) + 16
    hh = h.copy()
    hh["header_digest"] = (ref.digest(hh.tobytes()[:ref.HEADER_DIGESTED]) + ref.digest(t.tobytes(), ref.HEADER_DIGESTED // 4)) & ref.M64
    _refused(hh.tobytes() + t.tobytes() + blob[272 + 360:], "force", "past the end")
    # ... and the same entry without the repaired digest is a corrupted table
    _refused(blob[:272] + t.tobytes() + blob[272 + 360:], "table")
    for name, s in table.items():                                   # one flipped payload byte per section
        at = s.offset + s.bytes // 3
        msg = _refused(blob[:at] + bytes([blob[at] ^ 0x10]) + blob[at + 1:], name)
        assert "corrupted" in msg or "cursor" in msg
    _refused(blob[:20] + bytes([blob[20] ^ 1]) + blob[21:], "header")      # num_atoms: a header byte


def test_refusals_that_need_no_device():
    H = _H()
    I = importlib.import_module("openmm-velocityverlet_amd.integrator")
    blob = K.hand_made_blob()
    L = H.lib
    assert L.vvhip_checkpoint_inspect(None, 100, None) == H.ERR_INVALID and b"null" in L.vvhip_checkpoint_error()
    assert L.vvhip_checkpoint_inspect(blob, len(blob), None) == H.OK and L.vvhip_checkpoint_error() == b""
    assert L.vvhip_checkpoint_load(None, blob, len(blob), None) == H.ERR_INVALID
    assert L.vvhip_state_digest(None, None) == H.ERR_INVALID
    assert L.vvhip_checkpoint_size(None, H.CKPT_ALL, None) == H.ERR_INVALID
    assert L.vvhip_checkpoint_save(None, H.CKPT_ALL, None, None, 0) == H.ERR_INVALID
    it = I.VVIntegrator(333.0, 10.0, 1.0, 40.0, 0.001)
    plan, _, keep = I.create_plan(K.system("D"), it, "mixed")
    try:
        n, out, buf = C.c_size_t(0), (C.c_uint64 * H.CKPT_SECTIONS)(), C.create_string_buffer(64)
        for rc in (L.vvhip_state_digest(plan, C.byref(out)), L.vvhip_checkpoint_size(plan, H.CKPT_ALL, C.byref(n)),
                   L.vvhip_checkpoint_save(plan, H.CKPT_ALL, None, buf, 64), L.vvhip_checkpoint_load(plan, blob, len(blob), None)):
            assert rc == H.ERR_INVALID and "vvhip_bind" in L.vvhip_last_error(plan).decode()
        assert L.vvhip_checkpoint_load(plan, None, 0, None) == H.ERR_INVALID and "null" in L.vvhip_last_error(plan).decode()
        # a broken blob is refused before the plan is looked at, with the parser's text
        assert L.vvhip_checkpoint_load(plan, blob[:300], 300, None) == H.ERR_INVALID and "truncated" in L.vvhip_last_error(plan).decode()
    finally:
        L.vvhip_plan_destroy(plan)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_the_parser_is_clean_under_asan_and_ubsan_on_hostile_bytes(tmp_path):
    """tests/cpp/ckpt_format_sanitize.cpp with csrc/vv_ckpt_format.cpp (no HIP in it), as tests/test_host_sanitizers.py builds its program:
    the intact blob, every truncation, 4 000 single-bit corruptions, hostile table entries."""
    exe = str(tmp_path / "ckpt_format_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "ckpt_format_sanitize.cpp"), os.path.join(ROOT, "openmm-velocityverlet_amd", "csrc", "vv_ckpt_format.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, "4000"], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"CKPT SANITIZE OK truncations=(\d+) rejected=(\d+) padding=(\d+)", r.stdout)
    assert m and int(m.group(1)) > 3000 and int(m.group(2)) > 3900 and int(m.group(2)) + int(m.group(3)) == 4000, r.stdout
