// vv_checkpoint.cpp -- a run's complete state as a durable blob (include/vvhip.h: "checkpoint"): the state digest on the device, and
// save / load over the list of items the recovery snapshot keeps (vv_plan.hpp: recovery_items -- the list is stated there once; item k is
// section k), plus the host's cursor and seed as one more section.  The blob's format and its parser are vv_ckpt_format.cpp.
#include "vv_ckpt_format.hpp"
#include "vv_plan.hpp"

namespace {

struct Section { uint32_t id; void* live; size_t bytes; uint64_t base; size_t offset; };

vvhip_checkpoint_cursor cursor_of(const vvhip_plan* p) {
    vvhip_checkpoint_cursor c{};
    c.parity = p->cur.parity; c.random_pos = p->cur.random_pos;
    c.fextra_dirty = p->cur.fextra_dirty ? 1 : 0; c.fextra_virtual = p->cur.fextra_virtual ? 1 : 0;
    c.step_count = p->cur.step_count; c.rng_seed = p->rng_seed;
    return c;
}

// The device sections of the plan as it stands: every item of the shared list, in its order (bytes 0: not in use)
std::vector<Section> device_sections(vvhip_plan* p) {
    const std::vector<RecItem> items = recovery_items(p, nullptr);
    static_assert(VVHIP_CKPT_CURSOR == 8, "the list's items are sections 0 .. 7, the cursor follows");
    std::vector<Section> v;
    for (size_t k = 0; k < items.size() && k < (size_t) VVHIP_CKPT_CURSOR; k++)
        v.push_back({(uint32_t) k, items[k].live, items[k].live ? items[k].bytes : 0, (uint64_t) p->hp.shard_begin * items[k].particle_words, 0});
    return v;
}

// ... and those of a blob with this mask, the cursor section last, with their offsets; returns the blob's size
size_t blob_layout(vvhip_plan* p, uint32_t mask, std::vector<Section>& out) {
    out.clear();
    for (const Section& s : device_sections(p))
        if (s.bytes && (mask >> s.id & 1u)) out.push_back(s);
    out.push_back({VVHIP_CKPT_CURSOR, nullptr, sizeof(vvhip_checkpoint_cursor), 0, 0});
    size_t at = vvckpt::align16(sizeof(vvhip_checkpoint_header) + out.size() * sizeof(vvhip_checkpoint_section));
    for (Section& s : out) { s.offset = at; at = vvckpt::align16(at + s.bytes); }
    return at;
}

bool sharded(const vvhip_plan* p) { return p->hp.shard_begin != 0 || p->hp.shard_end != p->hp.num_atoms; }

}  // namespace

extern "C" {

int vvhip_state_digest(vvhip_plan* p, uint64_t out[VVHIP_CKPT_SECTIONS]) {
    NEED_BOUND(p);
    if (!out) return VVHIP_ERR_INVALID;
    if (p->capturing) return fail(p, VVHIP_ERR_INVALID, "vvhip_state_digest inside a graph capture");
    TRY(settle_recovery(p));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    const size_t bytes = VVHIP_CKPT_SECTIONS * sizeof(unsigned long long);
    HIP_TRY(p, p->d_digest.ensure(bytes));
    if (!p->h_digest) HIP_TRY(p, p->h_digest.alloc(bytes));
    HIP_TRY(p, hipMemsetAsync(p->d_digest.get(), 0, bytes, p->stream));
    for (const Section& s : device_sections(p)) {
        if (!s.bytes) continue;
        if (s.bytes % 4 || s.base + s.bytes / 4 > (1ull << 32)) return fail(p, VVHIP_ERR_UNSUPPORTED, std::string("state digest: section ") + vvckpt::section_name(s.id) + " has words beyond index 2^32");
        const vv::DigestArgs a{(const unsigned int*) s.live, (unsigned long long) (s.bytes / 4), (unsigned long long) s.base, p->d_digest.get() + s.id};
        // 512-thread blocks, eight per CU at most; a forced launch shape (test hooks "block_threads", "grid_cap_a") reaches this kernel too
        HIP_TRY(p, vv::launch_digest(a, p->launch_shape_forced ? p->block_threads : 512, p->launch_shape_forced ? p->grid_cap_a : 8 * p->num_cus, p->stream));
    }
    HIP_TRY(p, hipMemcpyAsync(p->h_digest.get(), p->d_digest.get(), bytes, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    for (int k = 0; k < VVHIP_CKPT_SECTIONS; k++) out[k] = p->h_digest[k];
    const vvhip_checkpoint_cursor c = cursor_of(p);
    out[VVHIP_CKPT_CURSOR] = vvckpt::digest(&c, sizeof(c), 0);
    return VVHIP_OK;
}

int vvhip_checkpoint_size(vvhip_plan* p, uint32_t sections, size_t* bytes) {
    NEED_BOUND(p);
    if (!bytes) return VVHIP_ERR_INVALID;
    if (sections & ~VVHIP_CKPT_ALL) return fail(p, VVHIP_ERR_INVALID, "checkpoint: unknown section bits in the mask");
    std::vector<Section> v;
    *bytes = blob_layout(p, sections, v);
    return VVHIP_OK;
}

int vvhip_checkpoint_save(vvhip_plan* p, uint32_t sections, const uint64_t host_words[4], void* blob, size_t bytes) {
    NEED_BOUND(p);
    if (!blob) return fail(p, VVHIP_ERR_INVALID, "checkpoint: null blob");
    if (sections & ~VVHIP_CKPT_ALL) return fail(p, VVHIP_ERR_INVALID, "checkpoint: unknown section bits in the mask");
    if (p->capturing) return fail(p, VVHIP_ERR_INVALID, "vvhip_checkpoint_save inside a graph capture");
    TRY(vvhip_synchronize(p));      // (a missed rendezvous is repaired here; a sticky word ends the call: a void state is never saved)
    std::vector<Section> v;
    const size_t need = blob_layout(p, sections, v);
    if (bytes < need) return fail(p, VVHIP_ERR_INVALID, "checkpoint: the buffer holds " + std::to_string(bytes) + " bytes, the blob needs " + std::to_string(need) + " (vvhip_checkpoint_size)");
    uint64_t dev[VVHIP_CKPT_SECTIONS];
    TRY(vvhip_state_digest(p, dev));
    unsigned char* b = (unsigned char*) blob;
    vvhip_checkpoint_header h{};
    vvhip_checkpoint_section table[VVHIP_CKPT_SECTIONS] = {};
    h.cursor = cursor_of(p);
    size_t end = vvckpt::align16(sizeof(h) + v.size() * sizeof(vvhip_checkpoint_section));
    std::memset(b + sizeof(h), 0, end - sizeof(h));
    for (size_t k = 0; k < v.size(); k++) {
        const Section& s = v[k];
        if (s.live) HIP_TRY(p, hipMemcpy(b + s.offset, s.live, s.bytes, hipMemcpyDeviceToHost));
        else std::memcpy(b + s.offset, &h.cursor, s.bytes);
        end = vvckpt::align16(s.offset + s.bytes);
        std::memset(b + s.offset + s.bytes, 0, end - (s.offset + s.bytes));
        const uint64_t d = vvckpt::digest(b + s.offset, s.bytes, s.base);
        if (d != dev[s.id])
            return fail(p, VVHIP_ERR_HIP, std::string("checkpoint: section ") + vvckpt::section_name(s.id) + " as downloaded does not have the digest computed on the device (a copy went wrong, or the state moved under the save)");
        table[k] = {s.id, 0, (uint64_t) s.offset, (uint64_t) s.bytes, s.base, d};
    }
    h.magic = VVHIP_CKPT_MAGIC; h.version = VVHIP_CKPT_VERSION; h.precision = p->hp.precision;
    h.num_atoms = p->hp.num_atoms; h.shard_begin = p->hp.shard_begin; h.shard_end = p->hp.shard_end;
    h.use_middle_scheme = p->hp.params.use_middle_scheme ? 1 : 0; h.num_nh_chains = p->hp.params.num_nh_chains;
    h.random_size = p->buf.random_size;
    for (int i = 0; i < 3; i++) h.box[i] = p->box[i];
    std::memcpy(&h.params, &p->hp.params, sizeof(h.params));      // (byte for byte: the header is digested, its padding included)
    for (int i = 0; i < 4; i++) h.host_words[i] = host_words ? host_words[i] : 0;
    h.num_sections = (uint32_t) v.size();
    h.total_bytes = need;
    h.header_digest = vvckpt::header_digest(h, table);
    std::memcpy(b + sizeof(h), table, v.size() * sizeof(vvhip_checkpoint_section));
    std::memcpy(b, &h, sizeof(h));
    return VVHIP_OK;
}

int vvhip_checkpoint_load(vvhip_plan* p, const void* blob, size_t bytes, uint64_t host_words_out[4]) {
    if (!p) return VVHIP_ERR_INVALID;
    if (!blob) return fail(p, VVHIP_ERR_INVALID, "checkpoint: null blob");
    vvhip_checkpoint_header h;
    vvhip_checkpoint_section table[VVHIP_CKPT_SECTIONS];
    std::string err;
    if (vvckpt::inspect(blob, bytes, &h, table, err) != VVHIP_OK) return fail(p, VVHIP_ERR_INVALID, err);
    NEED_BOUND(p);
    if (p->capturing) return fail(p, VVHIP_ERR_INVALID, "vvhip_checkpoint_load inside a graph capture");
    if (p->series.on) return fail(p, VVHIP_ERR_INVALID, "checkpoint: a series is running: stop it, load, start it again (its first row belongs to the old step counter)");
    if (p->frames.on) return fail(p, VVHIP_ERR_INVALID, "checkpoint: a frame recorder is running: stop it, load, start it again (its first frame belongs to the old step counter)");
    if (p->profile.on) return fail(p, VVHIP_ERR_INVALID, "checkpoint: a profile recorder is running: stop it, load, start it again (its first sample belongs to the old step counter)");
    if (p->msd.on) return fail(p, VVHIP_ERR_INVALID, "checkpoint: an MSD recorder is running: stop it, load, start it again (its origins belong to the old positions and step counter)");
    if (p->rdf.on) return fail(p, VVHIP_ERR_INVALID, "checkpoint: an RDF recorder is running: stop it, load, start it again (its first sample belongs to the old step counter)");
    if (p->current.on) return fail(p, VVHIP_ERR_INVALID, "checkpoint: a current recorder is running: stop it, load, start it again (its origins belong to the old positions and step counter)");
    if (p->modes.on) return fail(p, VVHIP_ERR_INVALID, "checkpoint: a density-mode recorder is running: stop it, load, start it again (its origins belong to the old positions and step counter)");
    if (p->contacts.on) return fail(p, VVHIP_ERR_INVALID, "checkpoint: a contact recorder is running: stop it, load, start it again (its origins belong to the old positions and step counter)");
    if (p->acf.on) return fail(p, VVHIP_ERR_INVALID, "checkpoint: an autocorrelation recorder is running: stop it, load, start it again (its origins belong to the old velocities, positions and step counter)");
    if (p->vanhove.on) return fail(p, VVHIP_ERR_INVALID, "checkpoint: a self van Hove recorder is running: stop it, load, start it again (its origins belong to the old positions and step counter)");
    if (p->vhd.on) return fail(p, VVHIP_ERR_INVALID, "checkpoint: a distinct van Hove recorder is running: stop it, load, start it again (its origins belong to the old positions and step counter)");
    if (p->sdf.on) return fail(p, VVHIP_ERR_INVALID, "checkpoint: a spatial distribution recorder is running: stop it, load, start it again (its first sample belongs to the old step counter)");
    if (sharded(p) || p->comm || p->mb_on || p->mb_local)
        return fail(p, VVHIP_ERR_UNSUPPORTED, "checkpoint: loading into a sharded plan or one with a communicator / mailbox is not supported (the peers' exchange counters would have to move together)");
    // ---- the blob's structure against the plan's
    const vv::HostPlan& hp = p->hp;
    auto differs = [&](const char* what, long long in_blob, long long in_plan) {
        return fail(p, VVHIP_ERR_INVALID, std::string("checkpoint: ") + what + " differs: the blob has " + std::to_string(in_blob) + ", the plan " + std::to_string(in_plan));
    };
    if (h.precision != hp.precision) return differs("precision", h.precision, hp.precision);
    if (h.num_atoms != hp.num_atoms) return differs("num_atoms", h.num_atoms, hp.num_atoms);
    if (h.shard_begin != hp.shard_begin || h.shard_end != hp.shard_end) return differs("shard", h.shard_end - h.shard_begin, hp.shard_end - hp.shard_begin);
    if ((h.use_middle_scheme != 0) != (hp.params.use_middle_scheme != 0)) return differs("scheme (use_middle_scheme)", h.use_middle_scheme, hp.params.use_middle_scheme);
    if (h.num_nh_chains != hp.params.num_nh_chains) return differs("num_nh_chains", h.num_nh_chains, hp.params.num_nh_chains);
    if (hp.has_ld && h.random_size != p->buf.random_size) return differs("random_size", h.random_size, p->buf.random_size);
    if (h.cursor.parity != 0 && h.cursor.parity != 1) return fail(p, VVHIP_ERR_INVALID, "checkpoint: section cursor: parity out of range");
    const std::vector<Section> mine = device_sections(p);
    const unsigned char* b = (const unsigned char*) blob;
    for (uint32_t k = 0; k < h.num_sections; k++) {
        const vvhip_checkpoint_section& s = table[k];
        if (s.id == VVHIP_CKPT_CURSOR) continue;
        if (s.bytes != mine[s.id].bytes || s.digest_base != mine[s.id].base)
            return fail(p, VVHIP_ERR_INVALID, std::string("checkpoint: section ") + vvckpt::section_name(s.id) + " differs in size: the blob has " + std::to_string(s.bytes) + " bytes, the plan " + std::to_string(mine[s.id].bytes));
    }
    // ---- from here on the device state changes
    TRY(settle_recovery(p));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    for (uint32_t k = 0; k < h.num_sections; k++) {
        const vvhip_checkpoint_section& s = table[k];
        if (s.id != VVHIP_CKPT_CURSOR) HIP_TRY(p, hipMemcpy(mine[s.id].live, b + s.offset, (size_t) s.bytes, hipMemcpyHostToDevice));
    }
    // both accumulator copies are zero between steps; EVERY rendezvous word goes (both parities, all replicas, the "polled twice" rows, the
    // dead word): a plan that goes back would otherwise meet the words of later steps under a restored tag
    HIP_TRY(p, hipMemsetAsync(p->d_acc.get(), 0, 2 * kAccN * sizeof(unsigned long long), p->stream));
    if (p->d_bigacc) HIP_TRY(p, hipMemsetAsync(p->d_bigacc.get(), 0, p->d_bigacc.bytes(), p->stream));
    if (p->d_rv) HIP_TRY(p, hipMemsetAsync(p->d_rv.get(), 0, (size_t) kRvWords * sizeof(unsigned long long), p->stream));
    p->cur.parity = h.cursor.parity; p->cur.random_pos = h.cursor.random_pos;
    p->cur.fextra_dirty = h.cursor.fextra_dirty != 0; p->cur.fextra_virtual = h.cursor.fextra_virtual != 0;
    p->cur.step_count = h.cursor.step_count;
    p->rng_seed = h.cursor.rng_seed;
    TRY(vvhip_set_box(p, h.box));
    p->mass_tab_valid = false;
    p->rec.valid = false;
    p->rec.runs.clear();
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    drop_graphs(p);
    uint64_t now[VVHIP_CKPT_SECTIONS];
    TRY(vvhip_state_digest(p, now));
    for (uint32_t k = 0; k < h.num_sections; k++)
        if (now[table[k].id] != table[k].digest)
            return fail(p, VVHIP_ERR_HIP, std::string("checkpoint: after the load, section ") + vvckpt::section_name(table[k].id) + " on the device does not have the blob's digest");
    if (host_words_out) for (int i = 0; i < 4; i++) host_words_out[i] = h.host_words[i];
    return VVHIP_OK;
}

}  // extern "C"
