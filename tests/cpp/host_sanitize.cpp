// tests/cpp/host_sanitize.cpp -- the host analysis (csrc/vv_host.cpp: analyze() and its passes -- classify, thermostat_groups, the constraint
// and site plans, the wave clusters, try_periodic, pack_waves, the per-lane tables, the riders' tables) under AddressSanitizer and
// UndefinedBehaviorSanitizer on the CPU (tests/test_host_sanitizers.py builds and runs it with g++ -fsanitize=address,undefined; GPU
// sanitizers are not available on this pool).  Random inventories of repeated molecules -- Drude pairs, hydrogen constraints, rigid water,
// Langevin / image / electrolyte subsets, general constraint clusters, virtual sites, defects, shard cuts on molecule boundaries, molecules
// larger than a wave -- analysed with the arithmetic layout forced on and off; a few invariants are checked so that the optimiser cannot
// drop the work.  Behind the random rounds come four built ones for branches that the random ones do not reach (main()).
//
// Every plan is digested whole (FNV-1a 64 over HostPlan in the declaration order of vv_host.hpp; a refused inventory: error code and text)
// and one line per round is printed: tests/golden/host_plan_digests.txt holds those lines as the analysis gave them before it was split
// into passes, so any change of any table shows.  The draws are plain arithmetic on mt19937's output (specified bit for bit, unlike
// std::uniform_int_distribution), the program is built with -ffp-contract=off: the lines are the same on every toolchain.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <type_traits>
#include <vector>

#include "../../openmm-velocityverlet_amd/csrc/vv_host.hpp"

namespace {
struct Sys {
    std::vector<double> masses, cdist;
    std::vector<int32_t> mol, pairs, cons, ld, img, el, vs;
    std::vector<double> vsp;
    int nmol = 0;
    int cut_begin = 0, cut_end = 0;      // != 0: this shard, wherever it cuts
};

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void* p, size_t n) {
        const unsigned char* b = (const unsigned char*) p;
        for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    }
    template <class T> void scalar(const T& v) { static_assert(std::is_arithmetic<T>::value, "scalars only: a struct has padding"); bytes(&v, sizeof(T)); }
    template <class T, size_t N> void array(const T (&a)[N]) { static_assert(std::is_arithmetic<typename std::remove_all_extents<T>::type>::value, "arrays of scalars only"); bytes(a, sizeof(a)); }
    template <class T> void vec(const std::vector<T>& v) { static_assert(std::is_arithmetic<T>::value, "vectors of scalars only"); scalar((uint64_t) v.size()); if (!v.empty()) bytes(v.data(), v.size() * sizeof(T)); }
    void str(const std::string& s) { scalar((uint64_t) s.size()); bytes(s.data(), s.size()); }
};

void digest(Fnv& f, const vv::HostPlan& hp) {      // the declaration order of vv_host.hpp / vvhip.h
    const vv::PeriodicLayout& q = hp.per;
    f.scalar(q.enabled); f.scalar(q.nreg); f.scalar(q.ncells); f.scalar(q.apc); f.scalar(q.wpc); f.scalar(q.spc); f.scalar(q.magic);
    f.array(q.reg_wave_start); f.array(q.reg_atom_start); f.array(q.reg_atom_end); f.array(q.reg_seg_start); f.array(q.reg_P); f.array(q.reg_spw);
    f.scalar(hp.precision);
    const vvhip_params& p = hp.params;
    f.scalar(p.temperature); f.scalar(p.frequency); f.scalar(p.drude_temperature); f.scalar(p.drude_frequency); f.scalar(p.step_size);
    f.scalar(p.num_nh_chains); f.scalar(p.loops_per_step); f.scalar(p.max_drude_distance); f.scalar(p.friction); f.scalar(p.drude_friction);
    f.scalar(p.mirror_location); f.scalar(p.electric_field); f.scalar(p.cos_acceleration); f.scalar(p.use_com_temp_group); f.scalar(p.use_middle_scheme);
    f.scalar(p.auto_set_com_temp_group); f.scalar(p.auto_set_friction); f.scalar(p.constraint_tolerance);
    const vvhip_plan_info& i = hp.info;
    f.scalar(i.num_particles_nh); f.scalar(i.num_molecules_nh); f.scalar(i.num_normal_nh); f.scalar(i.num_pairs_nh);
    f.scalar(i.num_normal_ld); f.scalar(i.num_pairs_ld); f.scalar(i.num_images); f.scalar(i.num_electrolyte);
    f.scalar(i.num_temp_groups); f.scalar(i.use_com_temp_group); f.scalar(i.friction);
    f.array(i.dof); f.array(i.nkbt); f.array(i.eta_mass); f.scalar(i.inv_mass_total);
    f.scalar(i.num_waves); f.scalar(i.num_slots_used); f.scalar(i.max_cluster); f.scalar(i.num_shake_clusters); f.scalar(i.constraints_fused);
    f.scalar(i.num_settle_clusters); f.scalar(i.periodic_layout); f.scalar(i.num_general_constraints); f.scalar(i.num_virtual_sites);
    f.scalar(i.general_relaxation);
    f.scalar(hp.num_atoms); f.scalar(hp.padded_num_atoms); f.scalar(hp.shard_begin); f.scalar(hp.shard_end);
    f.scalar(hp.has_nh); f.scalar(hp.has_ld); f.scalar(hp.has_ef); f.scalar(hp.has_images); f.scalar(hp.has_pairs);
    f.vec(hp.slots); f.vec(hp.slot_image); f.vec(hp.seg_mass); f.vec(hp.seg_base); f.vec(hp.slot_rand);
    f.vec(hp.slot_shake); f.vec(hp.slot_shake_param); f.scalar(hp.gc_omega); f.scalar(hp.gc_colors);
    f.vec(hp.slot_vsite); f.vec(hp.vsite_params); f.vec(hp.vsite_atom); f.vec(hp.slot_big); f.str(hp.unfused_reason);
    f.scalar(hp.num_big); f.scalar(hp.big_scale); f.vec(hp.image_pairs);
    f.array(hp.report_dof); f.scalar(hp.report_unit_bits); f.scalar(hp.report_frac_bits); f.scalar(hp.report_limit);
    f.vec(hp.report_lane_mol); f.vec(hp.report_lane_mass); f.vec(hp.report_lane_mu); f.vec(hp.report_mol_mass);
    f.vec(hp.report_cross); f.vec(hp.report_cross_mu); f.str(hp.report_unsupported);
    f.scalar(hp.has_cm_motion_remover); f.scalar(hp.cm_total_mass); f.vec(hp.masses);
    f.scalar(hp.therm_massive); f.scalar(hp.therm_massless); f.scalar(hp.therm_pairs); f.vec(hp.therm_laneless);
    f.scalar(hp.baro_frac_bits); f.scalar(hp.baro_num_molecules); f.vec(hp.baro_lane_mol); f.vec(hp.baro_laneless); f.vec(hp.baro_mol_count);
    f.str(hp.baro_unsupported);
    f.vec(hp.particles_nh); f.vec(hp.molecules_nh); f.vec(hp.normal_nh); f.vec(hp.pairs_nh); f.vec(hp.normal_ld); f.vec(hp.pairs_ld);
}

struct Tally {      // plans by property: what the corpus reaches
    int refused = 0, general = 0, sites = 0, big = 0, shake = 0, settle = 0, ld_images = 0;
    int unfused = 0, report_unsupported = 0, report_cross = 0, in_order = 0;
};

struct Tmpl { std::vector<int> units; double heavy; };      // 0 heavy, 1 hydrogen (constrained to the last heavy), 2 Drude pair

void add(Sys& s, const Tmpl& m, int flavour) {
    int last_heavy = -1, hcount = 0;
    const int first = (int) s.masses.size();
    for (int u : m.units) {
        if (u == 2) {
            s.masses.push_back(m.heavy - 0.4); s.masses.push_back(0.4);
            const int n = (int) s.masses.size();
            s.pairs.push_back(n - 1); s.pairs.push_back(n - 2);
            s.mol.push_back(s.nmol); s.mol.push_back(s.nmol);
            last_heavy = n - 2; hcount = 0;
        } else if (u == 1) {
            s.masses.push_back(1.008); s.mol.push_back(s.nmol);
            const int h = (int) s.masses.size() - 1;
            if (flavour >= 1 && flavour != 6 && last_heavy >= 0 && hcount < 3) { s.cons.push_back(h); s.cons.push_back(last_heavy); s.cdist.push_back(flavour == 2 ? 0.1 : 0.109); hcount++; }
        } else {
            s.masses.push_back(m.heavy); s.mol.push_back(s.nmol);
            const int h = (int) s.masses.size() - 1;
            if (flavour == 5 && last_heavy >= first) { s.cons.push_back(h); s.cons.push_back(last_heavy); s.cdist.push_back(0.15); }      // heavy-heavy bonds: general clusters
            last_heavy = h; hcount = 0;
        }
    }
    if (flavour == 2) { s.cons.push_back(first + 1); s.cons.push_back(first + 2); s.cdist.push_back(0.1633); }      // H-H: a rigid triangle
    s.nmol++;
}

Sys build(std::mt19937& rng, int flavour) {
    auto U = [&](int lo, int hi) { return lo + (int) (rng() % (unsigned long) (hi - lo + 1)); };      // (not std::uniform_int_distribution: see above)
    Sys s;
    std::vector<Tmpl> tmpl;
    const int ntmpl = U(1, 3);
    for (int t = 0; t < ntmpl; t++) {
        Tmpl m;
        static const int sizes[] = {1, 2, 3, 4, 7, 10, 19, 27, 33, 64, 70, 130};
        int size = sizes[U(0, flavour == 3 ? 11 : 9)], k = 0;
        while (k < size) {
            const int kind = U(0, 2);
            if (kind == 2 && k + 2 <= size) { m.units.push_back(2); k += 2; }
            else if (kind == 1 && k > 0) { m.units.push_back(1); k += 1; }
            else { m.units.push_back(0); k += 1; }
        }
        m.heavy = 12.0 + U(0, 3);
        tmpl.push_back(m);
    }
    if (flavour == 2) { tmpl.clear(); tmpl.push_back(Tmpl{{0, 1, 1}, 15.9994}); }      // water: rigid triangles below
    const int cells = U(1, 4);
    std::vector<int> counts;
    for (size_t t = 0; t < tmpl.size(); t++) counts.push_back(U(1, 20));
    const int defect_cell = U(0, cells + 1), defect_t = U(0, (int) tmpl.size() - 1);
    for (int c = 0; c < cells; c++)
        for (size_t t = 0; t < tmpl.size(); t++)
            for (int j = 0; j < counts[t]; j++) {
                add(s, tmpl[t], flavour);
                if (c == defect_cell && (int) t == defect_t && j == counts[t] / 2) add(s, Tmpl{{0, 0, 2}, 15.5}, flavour);
            }
    if (flavour == 4) {      // electrode machinery: a few Langevin atoms in front is not possible after the fact, so append them; images of the first molecule
        const int n0 = (int) s.masses.size();
        for (int w = 0; w < 5; w++) { s.masses.push_back(32.06); s.mol.push_back(s.nmol++); s.ld.push_back(n0 + w); }
        int m0 = 0;
        for (int i = 0; i < n0 && s.mol[i] == 0; i++) m0++;
        for (int i = 0; i < m0; i++) { s.masses.push_back(0.0); s.mol.push_back(0); s.img.push_back((int) s.masses.size() - 1); s.img.push_back(i); s.el.push_back(i); }
    }
    if (flavour == 6) {      // virtual sites behind the last particle, each in the molecule of its first parent; now and then a parent from the next molecule
        const int n0 = (int) s.masses.size();
        for (int i = 0; i + 3 < n0; i += U(1, 9)) {
            if (s.masses[i] == 0) continue;
            const int kind = U(0, 3), np = kind == 0 ? 2 : 3;
            int par[3] = {i, -1, -1};
            bool ok = true;
            for (int q = 1; q < np; q++) {
                par[q] = i + q;
                if (s.mol[par[q]] != s.mol[i] && U(0, 3) != 0) ok = false;
            }
            if (!ok) continue;
            s.masses.push_back(0.0); s.mol.push_back(s.mol[i]);
            s.vs.push_back((int) s.masses.size() - 1); s.vs.push_back(kind);
            for (int q = 0; q < 3; q++) s.vs.push_back(par[q]);
            for (int q = 0; q < 12; q++) s.vsp.push_back(0.1 * (q + 1));
        }
    }
    return s;
}

// The built rounds (main(): flavours 7 to 10).
Sys build_chains() {      // heavy chains of 70 and 130 particles, bonds and 1-3 distances constrained in runs of 35: every run fits a wave,
    Sys s;                // but its 67 constraints do not fit the wave's list of 64
    for (int rep = 0; rep < 3; rep++)
        for (int size : {70, 130}) {
            const int first = (int) s.masses.size();
            for (int k = 0; k < size; k++) {
                s.masses.push_back(12.011 + (k % 2)); s.mol.push_back(s.nmol);
                if (k % 35 >= 1) { s.cons.push_back(first + k - 1); s.cons.push_back(first + k); s.cdist.push_back(0.153); }
                if (k % 35 >= 2) { s.cons.push_back(first + k - 2); s.cons.push_back(first + k); s.cdist.push_back(0.252); }
            }
            s.nmol++;
        }
    return s;
}

Sys build_cut_molecule() {      // a shard that ends inside a molecule, between two particles that nothing ties to one wave
    Sys s;
    for (int m = 0; m < 12; m++) add(s, Tmpl{{0, 1, 1, 2, 0, 0, 1}, 14.0}, 1);
    s.cut_begin = 0; s.cut_end = 8 * 5 + 5;      // behind the Drude pair of the sixth molecule
    return s;
}

Sys build_cross_pair() {      // a Drude particle whose parent is the last particle of the molecule before
    Sys s;
    for (int m = 0; m < 9; m++) {
        add(s, Tmpl{{0, 1, 1, 0, 2}, 13.0}, 1);
        if (m % 3 == 1) {      // move the pair's Drude particle (the last particle so far) into the next molecule
            s.mol.back() = s.nmol;
        }
    }
    return s;
}

Sys build_large() {      // just over 2^20 lanes: 14 170 cells of two 27-particle cations and two 10-particle anions
    Sys s;
    const Tmpl cation{{0, 1, 1, 1, 2, 0, 1, 1, 2, 0, 1, 1, 1, 2, 0, 1, 1, 0, 1, 1, 0, 1, 1, 1}, 12.0}, anion{{2, 2, 2, 0, 0, 0, 0}, 14.0};
    for (int c = 0; c < 14170; c++) { add(s, cation, 1); add(s, cation, 1); add(s, anion, 1); add(s, anion, 1); }
    return s;
}

long analyse(const Sys& s, int use_com, int shard_parts, int part, Fnv& f, Tally& t) {
    vvhip_system_desc d;
    std::memset(&d, 0, sizeof(d));
    const int n = (int) s.masses.size();
    d.num_atoms = n; d.padded_num_atoms = (n + 31) / 32 * 32;
    d.masses = s.masses.data(); d.mol_id = s.mol.data(); d.num_molecules = s.nmol;
    d.num_drude_pairs = (int) s.pairs.size() / 2; d.drude_pairs = s.pairs.data();
    d.num_constraints = (int) s.cons.size() / 2; d.constraints = s.cons.data(); d.constraint_distances = s.cdist.empty() ? nullptr : s.cdist.data();
    d.has_cm_motion_remover = 1;
    d.num_particles_ld = (int) s.ld.size(); d.particles_ld = s.ld.data();
    d.num_image_pairs = (int) s.img.size() / 2; d.image_pairs = s.img.data();
    d.num_electrolyte = (int) s.el.size(); d.particles_electrolyte = s.el.data();
    d.num_virtual_sites = (int) s.vs.size() / 5; d.virtual_sites = s.vs.data(); d.virtual_site_params = s.vsp.data();
    if (shard_parts > 1) {      // cut on molecule boundaries
        std::vector<int> starts;
        for (int i = 0; i < n; i++) if (i == 0 || s.mol[i] != s.mol[i - 1]) starts.push_back(i);
        const int per = std::max(1, (int) starts.size() / shard_parts);
        const int b = starts[std::min((size_t) (part * per), starts.size() - 1)];
        const int e = part == shard_parts - 1 ? n : starts[std::min((size_t) ((part + 1) * per), starts.size() - 1)];
        if (e <= b) return 0;
        d.shard_begin = b; d.shard_end = e;
    } else if (s.cut_end != 0) {
        d.shard_begin = s.cut_begin; d.shard_end = s.cut_end;
    }
    vvhip_params p;
    std::memset(&p, 0, sizeof(p));
    p.temperature = 300; p.frequency = 10; p.drude_temperature = 1; p.drude_frequency = 40; p.step_size = 0.001;
    p.num_nh_chains = 3; p.loops_per_step = 1; p.max_drude_distance = 0.02; p.friction = 5; p.drude_friction = 20;
    p.use_com_temp_group = use_com; p.use_middle_scheme = 1; p.auto_set_com_temp_group = 0; p.auto_set_friction = 1; p.constraint_tolerance = 1e-5;
    long check = 0;
    try {
        const vv::HostPlan hp = vv::analyze(d, p, VVHIP_MIXED);
        // every slot points inside the shard, every table has the size the kernels index it with
        const int nloc = hp.shard_end - hp.shard_begin;
        const size_t nslots = (size_t) hp.info.num_waves * 64;
        if (hp.slots.size() != 2 * nslots) { std::fprintf(stderr, "slot table size\n"); std::exit(2); }
        for (size_t i = 0; i < nslots; i++) {
            const int32_t a = hp.slots[2 * i];
            if (a >= nloc) { std::fprintf(stderr, "slot out of shard\n"); std::exit(2); }
            if (a >= 0) check += a + (hp.slots[2 * i + 1] & 0xF);
        }
        if (hp.seg_base.size() != (size_t) hp.info.num_waves + 1 || hp.seg_mass.size() < 2 * (size_t) hp.seg_base.back()) { std::fprintf(stderr, "segment tables\n"); std::exit(2); }
        if (!hp.slot_shake.empty() && (hp.slot_shake.size() != nslots || hp.slot_shake_param.size() != 4 * nslots)) { std::fprintf(stderr, "shake tables\n"); std::exit(2); }
        if (!hp.slot_vsite.empty()) {
            if (hp.slot_vsite.size() != 2 * nslots || hp.vsite_params.size() != 12 * (size_t) hp.info.num_virtual_sites) { std::fprintf(stderr, "site tables\n"); std::exit(2); }
            for (size_t i = 0; i < nslots; i++)
                if ((uint32_t) hp.slot_vsite[2 * i] >> 31) {
                    if (hp.slots[2 * i] < 0 || hp.slot_vsite[2 * i + 1] < 0 || hp.slot_vsite[2 * i + 1] >= hp.info.num_virtual_sites) { std::fprintf(stderr, "site record\n"); std::exit(2); }
                    for (int q = 0; q < 3; q++)
                        if (hp.slots[2 * ((i & ~(size_t) 63) + (((uint32_t) hp.slot_vsite[2 * i] >> (6 * q)) & 63u))] < 0) { std::fprintf(stderr, "site parent lane is empty\n"); std::exit(2); }
                    check += hp.slot_vsite[2 * i + 1];
                }
        }
        check += hp.info.num_general_constraints + hp.info.periodic_layout * 1000003L + hp.info.num_waves;
        digest(f, hp);
        t.general += hp.info.num_general_constraints > 0; t.sites += hp.info.num_virtual_sites > 0; t.big += hp.num_big > 0;
        t.shake += hp.info.num_shake_clusters > 0; t.settle += hp.info.num_settle_clusters > 0; t.ld_images += hp.has_images && hp.has_ld;
        t.unfused += hp.info.constraints_fused == 0 && !hp.unfused_reason.empty();
        t.report_unsupported += !hp.report_unsupported.empty() && !hp.baro_unsupported.empty();
        t.report_cross += !hp.report_cross.empty();
        t.in_order += hp.info.num_slots_used >= (1 << 20) && !hp.info.periodic_layout;
    } catch (const vv::Error& e) {
        check += 7;            // refused inventories (a Drude pair across molecules, ...) are fine: the point is that nothing reads out of bounds
        f.scalar(e.code); f.str(e.what());
        t.refused++;
    }
    return check;
}
}  // namespace

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 300;
    std::mt19937 rng(20241008);
    long total = 0;
    int periodic = 0, plans = 0;
    Tally t;
    for (int r = 0; r < rounds; r++) {
        const int flavour = r % 7;                 // 0 plain, 1 hydrogen constraints, 2 rigid water, 3 big molecules, 4 Langevin + images,
                                                   // 5 bonds between heavy particles as well (general clusters), 6 virtual sites
        const Sys s = build(rng, flavour);
        Fnv f;
        const int before = plans;
        for (int per = 0; per < 2; per++) {
            setenv("VVHIP_PERIODIC", per ? "1" : "0", 1);
            for (int use_com = 0; use_com < 2; use_com++) {
                const long c = analyse(s, use_com, 1, 0, f, t);
                total += c; plans++;
                if (c >= 1000003L) periodic++;
                if (r % 3 == 0) { total += analyse(s, use_com, 2, 0, f, t); total += analyse(s, use_com, 2, 1, f, t); plans += 2; }
            }
        }
        std::printf("round %d flavour %d plans %d digest %016llx\n", r, flavour, plans - before, (unsigned long long) f.h);
    }
    // The built rounds, behind the random ones: 7 bonded heavy chains of 70 and 130 particles with the COM temperature group (constraints
    // that the wave-level sweeps cannot take: not fused, with the reason), 8 no COM group and a shard that cuts a molecule (no report, no
    // barostat), 9 no COM group and Drude pairs across two molecules (the report's cross records), 10 just over 2^20 lanes (in-order packing)
    for (int flavour = 7; flavour <= 10; flavour++) {
        const Sys s = flavour == 7 ? build_chains() : flavour == 8 ? build_cut_molecule() : flavour == 9 ? build_cross_pair() : build_large();
        Fnv f;
        const int before = plans;
        for (int per = 0; per < 2; per++) {
            setenv("VVHIP_PERIODIC", per ? "1" : "0", 1);
            const long c = analyse(s, flavour == 7 || flavour == 10, 1, 0, f, t);
            total += c; plans++;
            if (c >= 1000003L) periodic++;
        }
        std::printf("round %d flavour %d plans %d digest %016llx\n", rounds + flavour - 7, flavour, plans - before, (unsigned long long) f.h);
    }
    std::printf("HOST SANITIZE OK plans=%d periodic=%d checksum=%ld\n", plans, periodic, total);
    std::printf("properties refused=%d general=%d sites=%d big=%d shake=%d settle=%d ld_images=%d unfused=%d report_unsupported=%d report_cross=%d in_order=%d\n",
                t.refused, t.general, t.sites, t.big, t.shake, t.settle, t.ld_images, t.unfused, t.report_unsupported, t.report_cross, t.in_order);
    return 0;
}
