// vv_ckpt_format.cpp -- the checkpoint blob's format (include/vvhip.h: "checkpoint"): the digest on the host and the parser behind
// vvhip_checkpoint_inspect.  Plain C++ with NO HIP dependency: g++ builds this file alone (tests/cpp/ckpt_format_sanitize.cpp runs the
// parser on corrupted blobs under the host sanitizers).  Nothing here trusts a byte of the blob: every offset and size is checked
// against the buffer before it is used, and header and table are copied out (the blob may sit at any alignment).
#include "vv_ckpt_format.hpp"

#include <cstring>

namespace vvckpt {

static_assert(sizeof(vvhip_checkpoint_header) == 272 && kHeaderDigested == 264 && sizeof(vvhip_checkpoint_section) == 40 &&
              sizeof(vvhip_checkpoint_cursor) == 32 && sizeof(vvhip_params) == 120, "blob layout (include/vvhip.h)");

const char* section_name(uint32_t id) {
    static const char* const names[VVHIP_CKPT_SECTIONS] = {"posq", "correction", "velm", "force", "force_extra", "random", "thermostat", "epoch", "cursor"};
    return id < VVHIP_CKPT_SECTIONS ? names[id] : "unknown";
}

static inline uint64_t mix(uint64_t g, uint32_t w) {
    uint64_t z = ((g << 32) | w) + 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

uint64_t digest(const void* data, size_t bytes, uint64_t base) {
    const unsigned char* b = (const unsigned char*) data;
    uint64_t s = 0;
    for (size_t j = 0; j < bytes / 4; j++) {
        // (little-endian words whatever the host's byte order or the buffer's alignment)
        const uint32_t w = (uint32_t) b[4 * j] | (uint32_t) b[4 * j + 1] << 8 | (uint32_t) b[4 * j + 2] << 16 | (uint32_t) b[4 * j + 3] << 24;
        s += mix(base + j, w);
    }
    return s;
}

uint64_t header_digest(const vvhip_checkpoint_header& h, const vvhip_checkpoint_section* table) {
    const size_t n = h.num_sections <= VVHIP_CKPT_SECTIONS ? h.num_sections : 0;
    return digest(&h, kHeaderDigested, 0) + digest(table, n * sizeof(vvhip_checkpoint_section), kHeaderDigested / 4);
}

static int bad(std::string& err, const std::string& msg) {
    err = "checkpoint: " + msg;
    return VVHIP_ERR_INVALID;
}
static std::string sec(uint32_t id) { return "section " + std::to_string(id) + " (" + section_name(id) + ")"; }

int inspect(const void* blob, size_t bytes, vvhip_checkpoint_header* hdr, vvhip_checkpoint_section* table, std::string& err) {
    if (!blob) return bad(err, "null blob");
    const unsigned char* b = (const unsigned char*) blob;
    vvhip_checkpoint_header h;
    if (bytes < sizeof(h)) return bad(err, "truncated: " + std::to_string(bytes) + " bytes are fewer than the header's " + std::to_string(sizeof(h)));
    std::memcpy(&h, b, sizeof(h));
    if (h.magic != VVHIP_CKPT_MAGIC) return bad(err, "wrong magic: not a libvvhip checkpoint");
    if (h.version != VVHIP_CKPT_VERSION) return bad(err, "wrong version " + std::to_string(h.version) + " (this library reads version " + std::to_string(VVHIP_CKPT_VERSION) + ")");
    if (h.num_sections < 1 || h.num_sections > VVHIP_CKPT_SECTIONS) return bad(err, "section count " + std::to_string(h.num_sections) + " out of range");
    const size_t table_end = sizeof(h) + (size_t) h.num_sections * sizeof(vvhip_checkpoint_section);
    if (bytes < table_end) return bad(err, "truncated inside the section table");
    vvhip_checkpoint_section t[VVHIP_CKPT_SECTIONS] = {};
    std::memcpy(t, b + sizeof(h), (size_t) h.num_sections * sizeof(vvhip_checkpoint_section));
    if (header_digest(h, t) != h.header_digest) return bad(err, "header or section table corrupted (header digest mismatch)");
    if (h.precision < VVHIP_SINGLE || h.precision > VVHIP_DOUBLE || h.num_atoms < 0 || h.shard_begin < 0 || h.shard_end < h.shard_begin)
        return bad(err, "header fields out of range");
    uint64_t prev_end = table_end;
    bool cursor_seen = false;
    for (uint32_t k = 0; k < h.num_sections; k++) {
        const vvhip_checkpoint_section& s = t[k];
        if (s.id >= VVHIP_CKPT_SECTIONS || (k > 0 && s.id <= t[k - 1].id)) return bad(err, "table entry " + std::to_string(k) + ": section ids must ascend below " + std::to_string((int) VVHIP_CKPT_SECTIONS));
        if (s.offset % 16 || s.bytes % 4 || s.offset < prev_end) return bad(err, sec(s.id) + ": misplaced payload (offset " + std::to_string(s.offset) + ", " + std::to_string(s.bytes) + " bytes)");
        if (s.offset > bytes || s.bytes > bytes - s.offset)
            return bad(err, sec(s.id) + ": truncated or offset past the end (payload [" + std::to_string(s.offset) + ", +" + std::to_string(s.bytes) + ") of " + std::to_string(bytes) + " bytes)");
        if (s.digest_base > (1ull << 32) || s.bytes / 4 > (1ull << 32) - s.digest_base) return bad(err, sec(s.id) + ": word index beyond 2^32");
        if (digest(b + s.offset, (size_t) s.bytes, s.digest_base) != s.digest) return bad(err, sec(s.id) + ": payload corrupted (digest mismatch)");
        prev_end = s.offset + s.bytes;
        if (s.id == VVHIP_CKPT_CURSOR) {
            if (s.bytes != sizeof(vvhip_checkpoint_cursor) || std::memcmp(b + s.offset, &h.cursor, sizeof(h.cursor)) != 0)
                return bad(err, sec(s.id) + ": does not match the header's cursor");
            cursor_seen = true;
        }
    }
    if (!cursor_seen) return bad(err, sec(VVHIP_CKPT_CURSOR) + ": missing");
    if (h.total_bytes != bytes || align16((size_t) prev_end) != bytes)
        return bad(err, bytes < h.total_bytes ? "truncated: " + std::to_string(bytes) + " of " + std::to_string(h.total_bytes) + " bytes"
                                              : "size mismatch: " + std::to_string(bytes) + " bytes, the header says " + std::to_string(h.total_bytes));
    if (hdr) *hdr = h;
    if (table) std::memcpy(table, t, sizeof(t));
    return VVHIP_OK;
}

}  // namespace vvckpt

static thread_local std::string inspect_error;

extern "C" {

int vvhip_digest_host(const void* data, size_t bytes, uint64_t base, uint64_t* out) {
    if (!out || (!data && bytes) || bytes % 4 || base > (1ull << 32) || bytes / 4 > (1ull << 32) - base) return VVHIP_ERR_INVALID;
    *out = vvckpt::digest(data, bytes, base);
    return VVHIP_OK;
}

int vvhip_checkpoint_inspect(const void* blob, size_t bytes, vvhip_checkpoint_header* out) {
    inspect_error.clear();
    return vvckpt::inspect(blob, bytes, out, nullptr, inspect_error);
}

const char* vvhip_checkpoint_error(void) { return inspect_error.c_str(); }

}  // extern "C"
