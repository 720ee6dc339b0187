"""The state digest and the checkpoint blob of include/vvhip.h ("checkpoint") restated in NumPy, from the header's text alone: what the
host function, the device kernel and the parser are tested against (tests/test_checkpoint.py, tests/test_gpu_checkpoint.py)."""
import numpy as np

M64 = (1 << 64) - 1
SECTION_NAMES = ("posq", "correction", "velm", "force", "force_extra", "random", "thermostat", "epoch", "cursor")
MAGIC, VERSION = int.from_bytes(b"VVHIPCKP", "little"), 1

PARAMS = np.dtype([("temperature", "<f8"), ("frequency", "<f8"), ("drude_temperature", "<f8"), ("drude_frequency", "<f8"), ("step_size", "<f8"),
                   ("num_nh_chains", "<i4"), ("loops_per_step", "<i4"), ("max_drude_distance", "<f8"), ("friction", "<f8"),
                   ("drude_friction", "<f8"), ("mirror_location", "<f8"), ("electric_field", "<f8"), ("cos_acceleration", "<f8"),
                   ("use_com_temp_group", "<i4"), ("use_middle_scheme", "<i4"), ("auto_set_com_temp_group", "<i4"),
                   ("auto_set_friction", "<i4"), ("constraint_tolerance", "<f8")])
CURSOR = np.dtype([("parity", "<i4"), ("random_pos", "<u4"), ("fextra_dirty", "<i4"), ("fextra_virtual", "<i4"), ("step_count", "<i8"),
                   ("rng_seed", "<u8")])
HEADER = np.dtype([("magic", "<u8"), ("version", "<u4"), ("precision", "<i4"), ("num_atoms", "<i4"), ("shard_begin", "<i4"),
                   ("shard_end", "<i4"), ("use_middle_scheme", "<i4"), ("num_nh_chains", "<i4"), ("random_size", "<u4"), ("box", "<f8", (3,)),
                   ("params", PARAMS), ("cursor", CURSOR), ("host_words", "<u8", (4,)), ("num_sections", "<u4"), ("reserved", "<u4"),
                   ("total_bytes", "<u8"), ("header_digest", "<u8")])
SECTION = np.dtype([("id", "<u4"), ("reserved", "<u4"), ("offset", "<u8"), ("bytes", "<u8"), ("digest_base", "<u8"), ("digest", "<u8")])
assert (PARAMS.itemsize, CURSOR.itemsize, HEADER.itemsize, SECTION.itemsize) == (120, 32, 272, 40)
HEADER_DIGESTED = HEADER.fields["header_digest"][1]      # 264: the header's bytes in front of its own digest


def words(data) -> np.ndarray:
    """A buffer (bytes or an array of any dtype) as its 32-bit little-endian words."""
    b = bytes(data) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data).tobytes()
    assert len(b) % 4 == 0
    return np.frombuffer(b, dtype="<u4")


def digest(data, base: int = 0) -> int:
    w = words(data).astype(np.uint64)
    assert base + w.size <= 1 << 32
    if w.size == 0:
        return 0
    g = np.uint64(base) + np.arange(w.size, dtype=np.uint64)
    z = ((g << np.uint64(32)) | w) + np.uint64(0x9E3779B97F4A7C15)      # (uint64 arrays wrap mod 2^64)
    z ^= z >> np.uint64(30); z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27); z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return int(z.sum(dtype=np.uint64))


def align16(x: int) -> int:
    return (x + 15) // 16 * 16


def write_blob(fields: dict, sections: dict, bases: dict = None) -> bytes:
    """A blob from the documented format: `fields` fills the header (cursor and params as dicts), `sections` = {name: bytes} without
    the cursor section, which is taken from the header's cursor; ascending ids, payloads at 16-byte aligned offsets, zero padding."""
    bases = bases or {}
    h = np.zeros((), dtype=HEADER)
    h["magic"], h["version"] = MAGIC, VERSION
    for k, v in fields.items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                h[k][kk] = vv
        else:
            h[k] = v
    payload = {SECTION_NAMES.index(n): bytes(b) for n, b in sections.items()}
    payload[SECTION_NAMES.index("cursor")] = h["cursor"].tobytes()
    ids = sorted(payload)
    table = np.zeros(len(ids), dtype=SECTION)
    at = align16(HEADER.itemsize + len(ids) * SECTION.itemsize)
    body = bytearray()
    start = at
    for k, i in enumerate(ids):
        base = bases.get(SECTION_NAMES[i], 0)
        table[k] = (i, 0, at, len(payload[i]), base, digest(payload[i], base))
        body += payload[i] + bytes(align16(len(payload[i])) - len(payload[i]))
        at = start + len(body)
    h["num_sections"], h["total_bytes"] = len(ids), at
    h["header_digest"] = (digest(h.tobytes()[:HEADER_DIGESTED], 0) + digest(table.tobytes(), HEADER_DIGESTED // 4)) & M64
    head = h.tobytes() + table.tobytes()
    return head + bytes(start - len(head)) + bytes(body)


def read_blob(blob: bytes):
    """(header record, {name: (table row, payload bytes)}) of a blob, without checks."""
    blob = bytes(blob)
    h = np.frombuffer(blob[:HEADER.itemsize], dtype=HEADER)[0]
    table = np.frombuffer(blob[HEADER.itemsize:HEADER.itemsize + int(h["num_sections"]) * SECTION.itemsize], dtype=SECTION)
    return h, {SECTION_NAMES[int(t["id"])]: (t, blob[int(t["offset"]):int(t["offset"]) + int(t["bytes"])]) for t in table}
