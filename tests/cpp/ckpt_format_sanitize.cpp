// The checkpoint parser (csrc/vv_ckpt_format.cpp: vvhip_checkpoint_inspect, vvhip_digest_host) on hostile bytes, built with
// -fsanitize=address,undefined as an ordinary program (tests/test_checkpoint.py): a blob put together here from the structs of
// include/vvhip.h, every truncation of it, and single-byte corruptions at random places (fixed seed).  Every blob sits in a heap block of
// exactly its size, so a read past the end is the sanitizer's to find.  A corrupted blob must be rejected, or -- where the byte fell into
// padding, which no digest covers -- be accepted with every digest unchanged.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vvhip.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_random() {      // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static size_t align16(size_t x) { return (x + 15) & ~(size_t) 15; }
static uint64_t digest(const void* p, size_t n, uint64_t base) {
    uint64_t d = 0;
    if (vvhip_digest_host(p, n, base, &d) != VVHIP_OK) { std::printf("vvhip_digest_host refused %zu bytes\n", n); std::exit(1); }
    return d;
}
// inspect on a heap copy of exactly `n` bytes
static int inspect_copy(const unsigned char* b, size_t n, vvhip_checkpoint_header* out) {
    unsigned char* c = (unsigned char*) std::malloc(n ? n : 1);
    std::memcpy(c, b, n);
    const int rc = vvhip_checkpoint_inspect(n ? c : nullptr, n, out);
    std::free(c);
    return rc;
}

int main(int argc, char** argv) {
    const int corruptions = argc > 1 ? std::atoi(argv[1]) : 4000;
    // sizes that are no multiples of 16 leave padding behind the payloads
    const size_t sizes[VVHIP_CKPT_SECTIONS] = {80, 80, 160, 768, 60, 96, 1408, 8, sizeof(vvhip_checkpoint_cursor)};
    vvhip_checkpoint_header h;
    std::memset(&h, 0, sizeof(h));
    h.magic = VVHIP_CKPT_MAGIC; h.version = VVHIP_CKPT_VERSION; h.precision = VVHIP_MIXED;
    h.num_atoms = 5; h.shard_end = 5; h.use_middle_scheme = 1; h.num_nh_chains = 3; h.random_size = 6;
    h.box[0] = 2.5; h.box[1] = 2.75; h.box[2] = 3.0;
    h.cursor.parity = 1; h.cursor.random_pos = 3; h.cursor.step_count = 23; h.cursor.rng_seed = 0x1234567890ABCDEFull;
    h.host_words[0] = 7; h.num_sections = VVHIP_CKPT_SECTIONS;
    vvhip_checkpoint_section t[VVHIP_CKPT_SECTIONS];
    std::memset(t, 0, sizeof(t));
    size_t at = align16(sizeof(h) + sizeof(t));
    for (int k = 0; k < VVHIP_CKPT_SECTIONS; k++) { t[k].id = (uint32_t) k; t[k].offset = at; t[k].bytes = sizes[k]; at = align16(at + sizes[k]); }
    const size_t total = at;
    std::vector<unsigned char> blob(total, 0);
    std::vector<bool> digested(total, false);
    for (size_t i = 0; i < sizeof(h) + sizeof(t); i++) digested[i] = true;
    for (int k = 0; k < VVHIP_CKPT_SECTIONS; k++) {
        unsigned char* p = blob.data() + t[k].offset;
        if (k == VVHIP_CKPT_CURSOR) std::memcpy(p, &h.cursor, sizeof(h.cursor));
        else for (size_t i = 0; i < sizes[k]; i++) p[i] = (unsigned char) next_random();
        t[k].digest = digest(p, sizes[k], 0);
        for (size_t i = 0; i < sizes[k]; i++) digested[t[k].offset + i] = true;
    }
    h.total_bytes = total;
    h.header_digest = digest(&h, offsetof(vvhip_checkpoint_header, header_digest), 0) + digest(t, sizeof(t), offsetof(vvhip_checkpoint_header, header_digest) / 4);
    std::memcpy(blob.data(), &h, sizeof(h));
    std::memcpy(blob.data() + sizeof(h), t, sizeof(t));

    vvhip_checkpoint_header out;
    if (inspect_copy(blob.data(), total, &out) != VVHIP_OK) { std::printf("the intact blob was refused: %s\n", vvhip_checkpoint_error()); return 1; }
    if (std::memcmp(&out, &h, sizeof(h)) != 0) { std::printf("the header came back changed\n"); return 1; }
    int failures = 0;
    long truncations = 0, rejected = 0, in_padding = 0;
    for (size_t n = 0; n < total; n++, truncations++) {      // every truncation: section boundaries and the middle of each section among them
        if (inspect_copy(blob.data(), n, nullptr) != VVHIP_ERR_INVALID || !*vvhip_checkpoint_error()) { std::printf("a truncation to %zu bytes was not refused\n", n); failures++; }
    }
    std::vector<unsigned char> c(blob);
    for (int i = 0; i < corruptions; i++) {
        const size_t at_byte = (size_t) (next_random() % total);
        const unsigned char flip = (unsigned char) (1u << (next_random() % 8));
        c[at_byte] ^= flip;
        const int rc = inspect_copy(c.data(), total, &out);
        if (rc == VVHIP_ERR_INVALID && *vvhip_checkpoint_error()) rejected++;
        else if (rc == VVHIP_OK && !digested[at_byte]) in_padding++;      // no digested byte changed: header, table and every payload are the intact blob's
        else { std::printf("byte %zu ^ %#x: rc %d, digested %d\n", at_byte, flip, rc, (int) digested[at_byte]); failures++; }
        c[at_byte] ^= flip;
    }
    // a table whose offsets and sizes are hostile but whose header digest is right (the parser must not trust it)
    const uint64_t hostile[][2] = {{total, 16}, {total - 8, 16}, {~0ull - 15, 32}, {16, ~0ull - 3}, {0, 16}, {t[2].offset, sizes[2] + 16}};
    for (const auto& hv : hostile) {
        vvhip_checkpoint_section u[VVHIP_CKPT_SECTIONS];
        std::memcpy(u, t, sizeof(t));
        u[2].offset = hv[0]; u[2].bytes = hv[1];
        vvhip_checkpoint_header g = h;
        g.header_digest = digest(&g, offsetof(vvhip_checkpoint_header, header_digest), 0) + digest(u, sizeof(u), offsetof(vvhip_checkpoint_header, header_digest) / 4);
        std::memcpy(c.data(), &g, sizeof(g));
        std::memcpy(c.data() + sizeof(g), u, sizeof(u));
        if (inspect_copy(c.data(), total, nullptr) != VVHIP_ERR_INVALID) { std::printf("a hostile table entry (%llu, %llu) was accepted\n", (unsigned long long) hv[0], (unsigned long long) hv[1]); failures++; }
    }
    if (failures) return 1;
    std::printf("CKPT SANITIZE OK truncations=%ld rejected=%ld padding=%ld\n", truncations, rejected, in_padding);
    return 0;
}
