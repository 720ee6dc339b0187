// vv_host.cpp -- see vv_host.hpp.  "API" = openmmapi/src/VVIntegrator.cpp, "HOST" =
// platforms/cuda/src/CudaVVKernels.cpp of the reference.
//
// analyze() at the end of the file is the list of passes; every pass is a function of its own above it and reads what the earlier ones
// returned (Topology, ConstraintPlan, SitePlan, the clusters, PeriodicTry, Packing), never a shared scope.
#include "vv_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>

namespace vv {

namespace {
enum { TG_ATOM = 0, TG_COM = 1, TG_DRUDE = 2 };

void check_index(int i, int n, const char* what) {
    if (i < 0 || i >= n) throw Error(VVHIP_ERR_INVALID, std::string(what) + " index out of range");
}
int num_parents(int kind) { return kind == VVHIP_VSITE_AVERAGE2 ? 2 : 3; }
double reduced_mass(const vvhip_system_desc& sys, int d, int c) {
    const double md = sys.masses[d], mc = sys.masses[c];
    return md > 0 && mc > 0 ? md * mc / (md + mc) : 0.0;
}

struct Shard {
    int begin, end;
    bool has(int i) const { return i >= begin && i < end; }
};

// ---------------------------------------------------------------------------------------------------------------------------------------
// The System as the thermostats see it
// ---------------------------------------------------------------------------------------------------------------------------------------
struct Topology {
    std::vector<char> is_nh, is_ld, is_img, is_el;      // Nose-Hoover / Langevin / image / electrolyte particle
    std::vector<int32_t> image_of;                      // image particle of a parent, or -1
    std::vector<int32_t> partner;                       // the other particle of a Drude pair, or -1
    std::vector<char> in_pair, is_drude;
    std::vector<double> mol_mass;
};

// API:123-155, HOST:509-541, 786-802: validates the description and partitions the particles; fills the reference-shaped tables of hp.
Topology classify(const vvhip_system_desc& sys, HostPlan& hp) {
    const int n = sys.num_atoms, nmol = sys.num_molecules;
    Topology t;
    // ---- API:123-135: molecule masses
    for (int i = 0; i < n; i++)
        if (sys.mol_id[i] < 0 || sys.mol_id[i] >= nmol)
            throw Error(VVHIP_ERR_INVALID, "mol_id out of range");
    t.mol_mass.assign(nmol, 0.0);
    for (int i = 0; i < n; i++) t.mol_mass[sys.mol_id[i]] += sys.masses[i];

    // ---- API:138-151: NH / Langevin / image partition
    t.is_ld.assign(n, 0); t.is_img.assign(n, 0); t.is_el.assign(n, 0);
    for (int k = 0; k < sys.num_particles_ld; k++) { check_index(sys.particles_ld[k], n, "Langevin particle"); t.is_ld[sys.particles_ld[k]] = 1; }
    t.image_of.assign(n, -1);
    for (int k = 0; k < sys.num_image_pairs; k++) {
        int img = sys.image_pairs[2 * k], par = sys.image_pairs[2 * k + 1];
        check_index(img, n, "image particle"); check_index(par, n, "image parent");
        t.is_img[img] = 1;
        if (t.image_of[par] >= 0)
            throw Error(VVHIP_ERR_UNSUPPORTED, "a particle with more than one image particle is not supported");
        t.image_of[par] = img;
    }
    for (int k = 0; k < sys.num_electrolyte; k++) { check_index(sys.particles_electrolyte[k], n, "electrolyte particle"); t.is_el[sys.particles_electrolyte[k]] = 1; }
    t.is_nh.assign(n, 0);
    std::vector<char> mol_is_nh(nmol, 0);
    for (int i = 0; i < n; i++) {
        if (!t.is_ld[i] && !t.is_img[i]) {
            t.is_nh[i] = 1;
            hp.particles_nh.push_back(i);
            if (!mol_is_nh[sys.mol_id[i]]) { mol_is_nh[sys.mol_id[i]] = 1; hp.molecules_nh.push_back(sys.mol_id[i]); }
        }
    }
    for (int i = 0; i < n; i++)
        if (t.is_ld[i] && mol_is_nh[sys.mol_id[i]])
            throw Error(VVHIP_ERR_TOPOLOGY, "NH and Langevin thermostat cannot be applied on the same molecule");
    if (sys.num_particles_ld > 0 && hp.params.cos_acceleration != 0)   // API:154-155
        throw Error(VVHIP_ERR_TOPOLOGY, "Langevin thermostat and periodic perturbation shouldn't be used together");

    // ---- HOST:509-529, 786-792: Drude pairs
    t.partner.assign(n, -1);
    t.is_drude.assign(n, 0); t.in_pair.assign(n, 0);
    std::vector<char> nh_left(t.is_nh.begin(), t.is_nh.end()), ld_left(t.is_ld.begin(), t.is_ld.end());
    for (int k = 0; k < sys.num_drude_pairs; k++) {
        int d = sys.drude_pairs[2 * k], par = sys.drude_pairs[2 * k + 1];
        check_index(d, n, "Drude particle"); check_index(par, n, "Drude parent");
        if (t.in_pair[d] || t.in_pair[par] || d == par)
            throw Error(VVHIP_ERR_UNSUPPORTED, "a particle that belongs to two Drude pairs is not supported");
        t.in_pair[d] = t.in_pair[par] = 1;
        t.is_drude[d] = 1;
        t.partner[d] = par; t.partner[par] = d;
        if (t.is_nh[d] != t.is_nh[par] || t.is_ld[d] != t.is_ld[par])   // HOST:518-519, 786-787
            throw Error(VVHIP_ERR_TOPOLOGY, "Drude particle and its parent atom should be in the same thermostat");
        if (t.is_nh[d]) {
            nh_left[d] = nh_left[par] = 0;
            hp.pairs_nh.push_back(d); hp.pairs_nh.push_back(par);
        }
        if (t.is_ld[d]) {                                                // HOST:788-792
            ld_left[d] = ld_left[par] = 0;
            hp.pairs_ld.push_back(d); hp.pairs_ld.push_back(par);
        }
    }
    for (int i = 0; i < n; i++) {
        if (nh_left[i]) hp.normal_nh.push_back(i);               // std::set order = ascending
        if (ld_left[i]) hp.normal_ld.push_back(i);
    }
    // ---- HOST:531-541, 796-802: constraints
    for (int k = 0; k < sys.num_constraints; k++) {
        int a = sys.constraints[2 * k], b = sys.constraints[2 * k + 1];
        check_index(a, n, "constraint"); check_index(b, n, "constraint");
        if (t.is_nh[a] != t.is_nh[b] || t.is_ld[a] != t.is_ld[b])
            throw Error(VVHIP_ERR_TOPOLOGY, "Constrained particle pair should be in the same thermostat");
    }
    return t;
}

// HOST:496-594, 1028-1031: degrees of freedom of the three temperature groups (summed in the reference's order: particles, then pairs,
// then constraints), chain masses, the counts of hp.info.
void thermostat_groups(const vvhip_system_desc& sys, const Topology& t, HostPlan& hp) {
    const int n = sys.num_atoms;
    const vvhip_params& p = hp.params;
    // ---- HOST:496-541: DOF of the atomic group, NH pairs, constraints
    double dof[3] = {0, 0, 0};
    for (int i = 0; i < n; i++) {
        const double mass = sys.masses[i];
        if (t.is_nh[i] && mass != 0.0) {
            dof[TG_ATOM] += 3;
            if (p.use_com_temp_group) dof[TG_ATOM] -= 3 * mass * (1.0 / t.mol_mass[sys.mol_id[i]]);
        }
    }
    for (size_t k = 0; k < hp.pairs_nh.size() / 2; k++) {
        dof[TG_ATOM] -= 3;
        dof[TG_DRUDE] += 3;
    }
    for (int k = 0; k < sys.num_constraints; k++)
        if (t.is_nh[sys.constraints[2 * k]]) dof[TG_ATOM] -= 1;
    // ---- HOST:547-573
    if (p.use_com_temp_group) dof[TG_COM] = 3.0 * (double) hp.molecules_nh.size();
    if (sys.has_cm_motion_remover) {
        if (p.use_com_temp_group) dof[TG_COM] -= 3;
        else dof[TG_ATOM] -= 3;
    }
    for (double& d : dof) d = std::max(d, 0.0);
    int num_tg = 3;
    if (dof[TG_DRUDE] == 0) {
        num_tg = 2;
        if (dof[TG_COM] == 0) num_tg = 1;
    }
    // ---- HOST:577-594: chain masses
    vvhip_plan_info& info = hp.info;
    std::memset(&info, 0, sizeof(info));
    const double real_kbt = kBoltz * p.temperature, drude_kbt = kBoltz * p.drude_temperature;
    for (int i = 0; i < num_tg; i++) {
        const double kbt = i == TG_DRUDE ? drude_kbt : real_kbt;
        const double tg_mass = i == TG_DRUDE ? drude_kbt / std::pow(p.drude_frequency, 2) : real_kbt / std::pow(p.frequency, 2);
        info.nkbt[i] = dof[i] * kbt;
        info.eta_mass[i][0] = dof[i] * tg_mass;
        for (int c = 1; c < p.num_nh_chains; c++) info.eta_mass[i][c] = tg_mass;
    }
    for (int i = 0; i < 3; i++) info.dof[i] = dof[i];
    double mass_total = 0;                                      // HOST:1028-1031
    for (int i = 0; i < n; i++) mass_total += sys.masses[i];
    info.inv_mass_total = 1.0 / mass_total;
    hp.has_cm_motion_remover = sys.has_cm_motion_remover != 0;
    for (int i = 0; i < n; i++) if (sys.masses[i] > 0) hp.cm_total_mass += sys.masses[i];
    info.num_particles_nh = (int) hp.particles_nh.size();
    info.num_molecules_nh = (int) hp.molecules_nh.size();
    info.num_normal_nh = (int) hp.normal_nh.size();
    info.num_pairs_nh = (int) hp.pairs_nh.size() / 2;
    info.num_normal_ld = (int) hp.normal_ld.size();
    info.num_pairs_ld = (int) hp.pairs_ld.size() / 2;
    info.num_images = sys.num_image_pairs;
    info.num_electrolyte = sys.num_electrolyte;
    info.num_temp_groups = num_tg;
    info.use_com_temp_group = p.use_com_temp_group;
    info.friction = p.friction;
    hp.has_nh = !hp.particles_nh.empty();
    hp.has_ld = sys.num_particles_ld > 0;
    hp.has_ef = sys.num_electrolyte > 0;
    hp.has_images = sys.num_image_pairs > 0;
    hp.has_pairs = sys.num_drude_pairs > 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Constraints and virtual sites: who solves or places what
// ---------------------------------------------------------------------------------------------------------------------------------------
struct Shake { int32_t center; std::vector<int32_t> periph; double d; bool settle = false; double d_pp = 0; };

struct ConstraintPlan {
    std::vector<Shake> shakes;                      // hydrogen-type clusters (SHAKE) and rigid three-site molecules (SETTLE)
    std::vector<int32_t> shake_of;                  // index into shakes, or -1
    bool general = false;                           // every constraint belongs to a general cluster instead
    std::vector<std::vector<int32_t> > gc_adj;      // ... then: constraint partners of a particle
    bool fused = false;                             // the fused steps can take the constraints (general ones: withdrawn if a wave cannot)
};

// rigid three-site molecules (what OpenMM hands to SETTLE): three particles, three mutual constraints and nothing else; the apex is the
// particle whose two distances are equal and whose two partners have equal masses.  Marks their constraints in `used`; false = a triangle
// that fits neither rule.
bool find_settle(const vvhip_system_desc& sys, const std::vector<int>& deg, ConstraintPlan& cp, std::vector<char>& used) {
    const int n = sys.num_atoms;
    std::vector<std::vector<std::pair<int, int> > > adj(n);      // (other particle, constraint index)
    for (int k = 0; k < sys.num_constraints; k++) {
        const int a = sys.constraints[2 * k], b = sys.constraints[2 * k + 1];
        if (deg[a] == 2 && deg[b] == 2) { adj[a].push_back({b, k}); adj[b].push_back({a, k}); }
    }
    for (int a = 0; a < n; a++) {
        if (adj[a].size() != 2 || cp.shake_of[a] >= 0) continue;
        const int b = adj[a][0].first, c = adj[a][1].first;
        if (b == c || adj[b].size() != 2 || adj[c].size() != 2) continue;
        int kbc = -1;
        for (auto& e : adj[b]) if (e.first == c) kbc = e.second;
        if (kbc < 0) continue;                                    // a chain, not a triangle: left to find_shake (which refuses it)
        const int tri[3] = {a, b, c};
        const double dist[3] = {sys.constraint_distances[adj[a][0].second], sys.constraint_distances[adj[a][1].second], sys.constraint_distances[kbc]};   // ab, ac, bc
        // apex candidates: a (ab == ac, m_b == m_c), b (ab == bc, m_a == m_c), c (ac == bc, m_a == m_b)
        int apex = -1;
        if (dist[0] == dist[1] && sys.masses[b] == sys.masses[c]) apex = 0;
        else if (dist[0] == dist[2] && sys.masses[a] == sys.masses[c]) apex = 1;
        else if (dist[1] == dist[2] && sys.masses[a] == sys.masses[b]) apex = 2;
        if (apex < 0 || sys.masses[a] == 0 || sys.masses[b] == 0 || sys.masses[c] == 0) return false;
        Shake st;
        st.settle = true;
        st.center = tri[apex];
        for (int t = 0; t < 3; t++) if (t != apex) st.periph.push_back(tri[t]);
        std::sort(st.periph.begin(), st.periph.end());
        st.d = apex == 0 ? dist[0] : (apex == 1 ? dist[0] : dist[1]);
        st.d_pp = apex == 0 ? dist[2] : (apex == 1 ? dist[1] : dist[0]);
        for (int t = 0; t < 3; t++) cp.shake_of[tri[t]] = (int32_t) cp.shakes.size();
        cp.shakes.push_back(st);
        used[adj[a][0].second] = used[adj[a][1].second] = used[kbc] = 1;
    }
    return true;
}

// everything else must be hydrogen-type clusters (same admission rule as OpenMM's SHAKE kernel: a central particle with one to three
// peripheral particles of identical mass and distance, every peripheral in exactly one constraint)
bool find_shake(const vvhip_system_desc& sys, const std::vector<int>& deg, ConstraintPlan& cp, const std::vector<char>& used) {
    for (int k = 0; k < sys.num_constraints; k++) {
        if (used[k]) continue;
        int a = sys.constraints[2 * k], b = sys.constraints[2 * k + 1];
        const double d = sys.constraint_distances[k];
        // the central particle is the one with several constraints; for an isolated pair, the heavier one
        int ctr = deg[a] > 1 ? a : (deg[b] > 1 ? b : (sys.masses[a] >= sys.masses[b] ? a : b));
        int per = ctr == a ? b : a;
        if (deg[per] != 1 || sys.masses[ctr] == 0 || sys.masses[per] == 0) return false;
        if (cp.shake_of[ctr] < 0) { cp.shake_of[ctr] = (int32_t) cp.shakes.size(); cp.shakes.push_back(Shake{ctr, {}, d}); }
        Shake& s = cp.shakes[cp.shake_of[ctr]];
        if (s.settle || s.center != ctr || s.periph.size() >= 3 || s.d != d || (!s.periph.empty() && sys.masses[s.periph[0]] != sys.masses[per])) return false;
        if (cp.shake_of[per] >= 0) return false;
        s.periph.push_back(per);
        cp.shake_of[per] = cp.shake_of[ctr];
    }
    return true;
}

// Constraint clusters for the in-kernel solvers: SETTLE and SHAKE if every constraint fits them, else GENERAL clusters.
ConstraintPlan classify_constraints(const vvhip_system_desc& sys) {
    const int n = sys.num_atoms;
    ConstraintPlan cp;
    cp.shake_of.assign(n, -1);
    cp.fused = sys.num_constraints == 0;
    if (sys.num_constraints == 0 || !sys.constraint_distances) return cp;
    std::vector<int> deg(n, 0);
    for (int k = 0; k < sys.num_constraints; k++) { deg[sys.constraints[2 * k]]++; deg[sys.constraints[2 * k + 1]]++; }
    std::vector<char> used(sys.num_constraints, 0);
    if (find_settle(sys, deg, cp, used) && find_shake(sys, deg, cp, used)) { cp.fused = true; return cp; }
    cp.shakes.clear();
    std::fill(cp.shake_of.begin(), cp.shake_of.end(), -1);
    // ---- anything else (AllBonds, HAngles: chains, rings, triangles of constraints; examples/ommhelper/oplspsffile.py:948-951) becomes GENERAL
    // clusters: every connected component of the constraint graph must sit in one wave with its particles, and the wave relaxes its constraints
    // by coloured Gauss-Seidel sweeps (vv_device.inc: general_positions / general_velocities).
    for (int k = 0; k < sys.num_constraints; k++) {
        const int a = sys.constraints[2 * k], b = sys.constraints[2 * k + 1];
        if (a == b || sys.masses[a] == 0 || sys.masses[b] == 0 || !(sys.constraint_distances[k] > 0)) return cp;      // (OpenMM refuses massless ones too)
    }
    cp.general = true;
    cp.gc_adj.assign(n, {});
    for (int k = 0; k < sys.num_constraints; k++) {
        cp.gc_adj[sys.constraints[2 * k]].push_back(sys.constraints[2 * k + 1]);
        cp.gc_adj[sys.constraints[2 * k + 1]].push_back(sys.constraints[2 * k]);
    }
    cp.fused = true;          // withdrawn by general_tables if a component does not fit a wave
    return cp;
}

// Virtual sites (vvhip_system_desc.virtual_sites): kernel B places a site from the lane of one of its parents -- the first parent
// that places no other site -- so that sites cost no lanes and the wave layout is the one the System has without them (6 000 sites on the
// headline box as lanes of their own: 2 100 waves instead of 1 752, past what one block per CU holds, -12 % steps/s for the layout alone).
// A site that has an image particle or sits in a Drude pair, or whose parents all place another site already, gets a lane of its own.
struct SitePlan {
    bool enabled = false;                           // sites are given and none hangs on another site
    std::vector<int32_t> vs_of;                     // record of a site particle, or -1
    std::vector<int32_t> vs_host;                   // per record: the particle whose lane places the site
    std::vector<std::vector<int32_t> > vs_adj;      // the lane-bearing particles a particle must share a wave with for that
};

SitePlan plan_sites(const vvhip_system_desc& sys, const Topology& t) {
    const int n = sys.num_atoms;
    SitePlan sp;
    sp.vs_of.assign(n, -1);
    sp.enabled = sys.num_virtual_sites > 0 && sys.virtual_sites && sys.virtual_site_params;
    if (!sp.enabled) return sp;
    for (int k = 0; k < sys.num_virtual_sites; k++) {
        const int32_t* rec = sys.virtual_sites + 5 * (size_t) k;
        const int site = rec[0], kind = rec[1];
        check_index(site, n, "virtual site");
        if (kind < VVHIP_VSITE_AVERAGE2 || kind > VVHIP_VSITE_LOCAL_COORDS) throw Error(VVHIP_ERR_INVALID, "unknown kind of virtual site");
        if (sys.masses[site] != 0.0) throw Error(VVHIP_ERR_INVALID, "a virtual site must have mass 0");
        if (sp.vs_of[site] >= 0) throw Error(VVHIP_ERR_INVALID, "a particle is described as a virtual site twice");
        sp.vs_of[site] = k;
        for (int q = 0; q < num_parents(kind); q++) check_index(rec[2 + q], n, "virtual site parent");
    }
    for (int k = 0; k < sys.num_virtual_sites && sp.enabled; k++) {     // a site that hangs on another site: left to the caller's own kernel
        const int32_t* rec = sys.virtual_sites + 5 * (size_t) k;
        for (int q = 0; q < num_parents(rec[1]); q++)
            if (sp.vs_of[rec[2 + q]] >= 0) sp.enabled = false;
    }
    if (!sp.enabled) return sp;
    sp.vs_adj.assign(n, {});
    sp.vs_host.assign((size_t) sys.num_virtual_sites, -1);
    std::vector<char> hosting(n, 0);
    auto has_lane_anyway = [&](int i) { return sys.masses[i] != 0.0 || t.in_pair[i] || t.image_of[i] >= 0; };
    for (int k = 0; k < sys.num_virtual_sites; k++) {
        const int32_t* rec = sys.virtual_sites + 5 * (size_t) k;
        const int site = rec[0], np = num_parents(rec[1]);
        int host = -1;
        if (t.image_of[site] < 0 && !t.in_pair[site])
            for (int q = 0; q < np && host < 0; q++)
                if (!hosting[rec[2 + q]] && has_lane_anyway(rec[2 + q])) host = rec[2 + q];
        if (host < 0) host = site; else hosting[host] = 1;
        sp.vs_host[(size_t) k] = host;
        std::vector<int32_t> bearers;
        if (host == site) bearers.push_back(site);
        for (int q = 0; q < np; q++) if (has_lane_anyway(rec[2 + q])) bearers.push_back(rec[2 + q]);
        for (size_t b = 1; b < bearers.size(); b++)
            if (bearers[b] != bearers[0]) { sp.vs_adj[bearers[0]].push_back(bearers[b]); sp.vs_adj[bearers[b]].push_back(bearers[0]); }
    }
    return sp;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Clusters: the particles that must share one wave
// ---------------------------------------------------------------------------------------------------------------------------------------
struct Model {      // the description with everything the passes above found out about it
    const vvhip_system_desc& sys;
    const Topology& top;
    const ConstraintPlan& cons;
    const SitePlan& sites;

    bool needs_lane(int i) const {
        if (sys.masses[i] != 0.0) return true;      // anything massive is integrated
        if (sites.enabled && sites.vs_of[i] >= 0 && sites.vs_host[(size_t) sites.vs_of[i]] == i) return true;   // a virtual site that is placed by a lane of its own
        if (top.in_pair[i]) return true;            // massless Drude parent (hard-wall branch K/middle.cu:151-173)
        if (top.image_of[i] >= 0) return true;      // massless image parent: only the mirror copy
        return false;
    }
    // THE rule of who must share a wave with particle j: its Drude partner, its SHAKE / SETTLE cluster, its general-constraint partners,
    // the lane-bearing particles of the virtual sites it takes part in.  (j itself may be among them.)
    template <class F> void for_each_wave_mate(int j, F&& f) const {
        if (top.in_pair[j]) f(top.partner[j]);
        if (cons.shake_of[j] >= 0) {
            const Shake& s = cons.shakes[cons.shake_of[j]];
            f(s.center);
            for (int q : s.periph) f(q);
        }
        if (cons.general) for (int q : cons.gc_adj[j]) f(q);
        if (sites.enabled) for (int q : sites.vs_adj[j]) if (needs_lane(q)) f(q);
    }
    // closure of that rule from `seed` (a handful of particles at most), sorted; claim(q) says whether q is new, or throws
    template <class Claim> std::vector<int32_t> wave_unit(int seed, Claim&& claim) const {
        std::vector<int32_t> unit, todo{seed};
        while (!todo.empty()) {
            const int j = todo.back();
            todo.pop_back();
            unit.push_back(j);
            for_each_wave_mate(j, [&](int q) { if (claim(q)) todo.push_back(q); });
        }
        std::sort(unit.begin(), unit.end());
        return unit;
    }
};

struct Cluster {            // particles that must share one wave
    int32_t first;          // smallest particle index (ordering key)
    std::vector<int32_t> members;
    bool com_segment;       // members form one molecular COM segment
    int32_t big = -1;       // >= 0: chunk of big molecule `big` (a molecule with more than 64 lanes, split over waves)
    bool big_first = false; // first chunk of that molecule
};

// With the COM temperature group a thermostatted molecule is one cluster, everything else the closure of the shared-wave rule.
std::vector<Cluster> build_clusters(const Model& m, const Shard& shard, bool use_com) {
    const vvhip_system_desc& sys = m.sys;
    const int n = sys.num_atoms;
    std::vector<Cluster> clusters;
    std::vector<int32_t> cluster_of_mol(sys.num_molecules, -1);
    std::vector<char> done(n, 0);
    auto claim = [&](int q) {
        if (q < 0 || done[q]) return false;
        if (!shard.has(q)) throw Error(VVHIP_ERR_INVALID, "particle shard cuts a Drude pair or a constraint cluster");
        done[q] = 1;
        return true;
    };
    for (int i = shard.begin; i < shard.end; i++) {
        if (done[i] || !m.needs_lane(i)) continue;
        done[i] = 1;
        if (use_com && m.top.is_nh[i]) {
            const int mol = sys.mol_id[i];
            if (cluster_of_mol[mol] < 0) {
                cluster_of_mol[mol] = (int32_t) clusters.size();
                clusters.push_back(Cluster{i, {}, true});
            }
            clusters[cluster_of_mol[mol]].members.push_back(i);
        } else {
            Cluster c{i, m.wave_unit(i, claim), false};
            c.first = c.members[0];
            clusters.push_back(c);
        }
    }
    // a COM cluster must contain the whole molecule's thermostatted particles: check the shard did not cut it
    if (use_com)
        for (int i = 0; i < n; i++)
            if (m.top.is_nh[i] && m.needs_lane(i) && !shard.has(i) && cluster_of_mol[sys.mol_id[i]] >= 0)
                throw Error(VVHIP_ERR_INVALID, "particle shard cuts a molecule");
    return clusters;
}

// A COM cluster larger than a wave is cut into chunks of <= 64 lanes (the units of the shared-wave rule stay together); the chunks are
// ordinary segments for the wave-level scans, the molecule-level sum goes through a small global accumulator (hp.num_big, hp.big_scale).
void split_big_molecules(const Model& m, std::vector<Cluster>& clusters, HostPlan& hp) {
    std::vector<Cluster> out;
    double max_big_mass = 0;
    auto close = [&](Cluster& chunk) {
        std::sort(chunk.members.begin(), chunk.members.end());
        chunk.first = chunk.members[0];
        out.push_back(chunk);
    };
    for (Cluster& cl : clusters) {
        if (!cl.com_segment || cl.members.size() <= 64) { out.push_back(std::move(cl)); continue; }
        std::sort(cl.members.begin(), cl.members.end());
        const int big = hp.num_big++;
        double mtot = 0;
        for (int i : cl.members) mtot += m.sys.masses[i];
        max_big_mass = std::max(max_big_mass, mtot);
        std::vector<char> taken(cl.members.size(), 0);
        auto claim = [&](int q) {
            auto it = std::lower_bound(cl.members.begin(), cl.members.end(), q);
            if (it == cl.members.end() || *it != q) throw Error(VVHIP_ERR_UNSUPPORTED, "a Drude pair or a constraint cluster spans two molecules");
            const size_t t = (size_t) (it - cl.members.begin());
            if (taken[t]) return false;
            taken[t] = 1;
            return true;
        };
        Cluster chunk{cl.members[0], {}, true, big, true};
        for (size_t k = 0; k < cl.members.size(); k++) {      // the units in index order
            if (taken[k]) continue;
            taken[k] = 1;
            const std::vector<int32_t> u = m.wave_unit(cl.members[k], claim);
            if (chunk.members.size() + u.size() > 64) {
                close(chunk);
                chunk = Cluster{u[0], {}, true, big, false};
            }
            chunk.members.insert(chunk.members.end(), u.begin(), u.end());
        }
        close(chunk);
    }
    clusters.swap(out);
    if (hp.num_big > 0) {       // |sum m v| <= M |v|max with |v|max ~ 50 nm/ps; keep 4x headroom below 2^62
        const double top = std::ldexp(1.0, 62) / (std::max(max_big_mass, 1.0) * 50.0 * 4.0);
        hp.big_scale = std::ldexp(1.0, std::max(0, std::min(40, (int) std::floor(std::log2(top)))));
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Arithmetic ("periodic") layout: runs of identical repeat units, possibly repeated cell after cell (vv_host.hpp: PeriodicLayout)
// ---------------------------------------------------------------------------------------------------------------------------------------
struct Region { uint64_t sig; int p, reps, atoms, segs; };      // unit of p clusters repeated reps times

// region of the cell-local wave wl (unused regions start at INT_MAX)
int region_of_wave(const PeriodicLayout& per, int wl) {
    int r = 0;
    for (int k = 1; k < 4; k++) if (wl >= per.reg_wave_start[k]) r = k;
    return r;
}

struct PeriodicTry {
    bool ok = false;
    std::vector<Region> regions;             // of the whole plan, cell after cell
    int R = 0;                               // regions per cell
    std::vector<int> reg_cluster_start;      // first cluster (cell-local) of region r; [R]: clusters per cell
    PeriodicLayout per;

    // (wave, first lane) of cluster k under the layout: the inverse of region_of_wave and the formula that periodic_matches checks
    void place(const std::vector<Cluster>& clusters, size_t k, int& wave_out, int& lane_out) const {
        const int per_cell = reg_cluster_start[R], cell = (int) (k / (size_t) per_cell), kl = (int) (k % (size_t) per_cell);
        int r = 0;
        while (r + 1 < R && kl >= reg_cluster_start[r + 1]) r++;
        const Region& g = regions[r];
        const int ku = kl - reg_cluster_start[r], unit = ku / g.p, j = ku % g.p, m = 64 / g.atoms;
        int off = 0;
        for (int t = 0; t < j; t++) off += (int) clusters[k - j + t].members.size();
        wave_out = cell * per.wpc + per.reg_wave_start[r] + unit / m;
        lane_out = (unit % m) * g.atoms + off;
    }
};

// What makes two clusters interchangeable for the formula: size, masses, roles, pair and constraint shape relative to the first particle.
// False: the particles are not consecutive.
bool cluster_signature(const Model& m, const Cluster& c, uint64_t& sig) {
    const Topology& t = m.top;
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { for (int b = 0; b < 8; b++) { h ^= (v >> (8 * b)) & 0xff; h *= 1099511628211ull; } };
    mix(c.members.size()); mix(c.com_segment ? 1 : 0);
    for (size_t j = 0; j < c.members.size(); j++) {
        const int i = c.members[j];
        if (i != c.first + (int) j) return false;
        uint64_t mb; std::memcpy(&mb, &m.sys.masses[i], 8);
        mix(mb);
        mix((uint64_t) (t.is_nh[i] ? 1 : 0) | (t.in_pair[i] ? 2 : 0) | (t.is_drude[i] ? 4 : 0) | (t.is_el[i] ? 8 : 0));
        mix(t.in_pair[i] ? (uint64_t) (int64_t) (t.partner[i] - c.first) : 0);
        if (m.cons.shake_of[i] < 0) { mix(0); continue; }
        const Shake& sh = m.cons.shakes[m.cons.shake_of[i]];      // in-kernel constraint cluster: same shape, distances and position inside the unit
        uint64_t db, pb; std::memcpy(&db, &sh.d, 8); std::memcpy(&pb, &sh.d_pp, 8);
        int role = 0;
        for (size_t q = 0; q < sh.periph.size(); q++) if (sh.periph[q] == i) role = 1 + (int) q;
        mix(1 + (uint64_t) role); mix((uint64_t) (int64_t) (sh.center - c.first)); mix(sh.periph.size()); mix(db); mix(pb); mix(sh.settle ? 1 : 0);
    }
    sig = h;
    return true;
}

// greedy decomposition into regions: at each position the unit length (clusters adding up to <= 64 lanes) that covers the most clusters
bool find_regions(const std::vector<Cluster>& clusters, const std::vector<uint64_t>& sig, std::vector<Region>& regions) {
    const size_t K = clusters.size();
    for (size_t i = 0; i < K;) {
        int best_p = 1, best_reps = 1;
        size_t best_cover = 0;
        for (int pp = 1; pp <= 64 && i + pp <= K; pp++) {
            int atoms = 0;
            for (int j = 0; j < pp; j++) atoms += (int) clusters[i + j].members.size();
            if (atoms > 64) break;
            size_t j = i + pp;
            while (j < K && sig[j] == sig[j - pp]) j++;
            const int reps = (int) ((j - i) / pp);
            if (reps < 2 && pp > 1) continue;         // a unit must repeat: 13 anions followed by 4 waters are not one 17-cluster unit
            if ((size_t) reps * pp > best_cover) { best_cover = (size_t) reps * pp; best_p = pp; best_reps = reps; }
        }
        Region r{0, best_p, best_reps, 0, 0};
        uint64_t h = 1469598103934665603ull;
        for (int j = 0; j < best_p; j++) {
            h = (h ^ sig[i + j]) * 1099511628211ull;
            r.atoms += (int) clusters[i + j].members.size();
            r.segs += clusters[i + j].com_segment ? 1 : 0;
        }
        r.sig = h;
        regions.push_back(r);
        i += (size_t) best_p * best_reps;
        if (regions.size() > ((size_t) 1 << 22)) return false;
    }
    return true;
}

// period of the region list (at most four regions per cell) and the layout's constants
bool layout_regions(PeriodicTry& pt) {
    const std::vector<Region>& regions = pt.regions;
    const int L = (int) regions.size();
    int R = 0;
    for (int cand = 1; cand <= 4 && cand <= L && !R; cand++) {
        if (L % cand) continue;
        bool ok = true;
        for (int i = cand; i < L && ok; i++)
            ok = regions[i].sig == regions[i - cand].sig && regions[i].p == regions[i - cand].p && regions[i].reps == regions[i - cand].reps;
        if (ok) R = cand;
    }
    if (!R) return false;
    PeriodicLayout& per = pt.per;
    per.nreg = R;
    per.ncells = L / R;
    pt.reg_cluster_start.assign(R + 1, 0);
    int w = 0, at = 0, sg = 0, cl = 0;
    for (int r = 0; r < R; r++) {
        const Region& g = regions[r];
        const int m = 64 / g.atoms;
        per.reg_wave_start[r] = w; per.reg_atom_start[r] = at; per.reg_seg_start[r] = sg;
        per.reg_P[r] = m * g.atoms; per.reg_spw[r] = m * g.segs;
        pt.reg_cluster_start[r] = cl;
        w += (g.reps + m - 1) / m; at += g.atoms * g.reps; sg += g.segs * g.reps; cl += g.p * g.reps;
        per.reg_atom_end[r] = at;
    }
    pt.reg_cluster_start[R] = cl;
    per.wpc = w; per.apc = at; per.spc = sg;
    pt.R = R;
    const long total_waves = (long) per.wpc * per.ncells;
    if (total_waves > (1l << 26)) return false;
    per.magic = per.ncells > 1 ? (uint32_t) ((1ull << 32) / (uint64_t) per.wpc + 1) : 0u;
    return true;
}

PeriodicTry try_periodic(const Model& m, const std::vector<Cluster>& clusters, const Shard& shard, const HostPlan& hp) {
    // Measured on MI355X (same box, alternating runs): with 8.9 M particles kernel B 305 -> 277 us.  At 111 k particles the block's copy of
    // the pattern rows and its barrier cost more than the slot load did (kernel B 6.0 -> 6.4 us) and best-fit packing needs 13 % fewer
    // waves.  In between (round 4, tools/probes/layout_crossover.py, each layout with its own best launch shape, steps/s best-fit |
    // arithmetic): 222 k particles 66.0 | 57.7 k, 444 k 38.5 | 35.5 k, 666 k 26.8 | 25.0 k, 888 k 18.75 | 18.91 k, 1.33 M 13.6 | 14.1 k,
    // 2.7 M 7.1 | 7.5 k, 4.4 M 4.12 | 4.63 k.  (Round 2 had put the switch at 0.2 M lanes, +3 .. +7 % then: two blocks of 6-7 tile waves
    // per CU, vv_launch.cpp: pick_launch_shape, took the best-fit layout past it.)  With the chain kept inside kernel B up to 2.6 M particles
    // (vv_plan.hpp: split_chain_waves) the two meet a little higher: 888 k particles 20.8 | 20.6 k, 1.33 M 14.3 | 14.5 k, 1.78 M 11.2 | 11.4 k.
    // So: from 1.1 M lanes, unless VVHIP_PERIODIC=1 / 0 says always / never.
    PeriodicTry pt;
    size_t lanes = 0;
    for (const Cluster& c : clusters) lanes += c.members.size();
    bool want = lanes >= 1100000;
    if (const char* e = std::getenv("VVHIP_PERIODIC")) want = std::atoi(e) != 0;
    if (!want) return pt;
    if (hp.has_ld || hp.has_images || hp.num_big > 0 || clusters.empty() || m.cons.general || m.sites.enabled) return pt;
    std::vector<uint64_t> sig(clusters.size());
    int expect = shard.begin;
    for (size_t k = 0; k < clusters.size(); k++) {
        const Cluster& c = clusters[k];
        if (c.first != expect || c.members.size() > 64) return pt;                 // particles must be consecutive, cluster after cluster
        if (!cluster_signature(m, c, sig[k])) return pt;
        expect += (int) c.members.size();
    }
    if (expect != shard.end) return pt;
    if (!find_regions(clusters, sig, pt.regions)) return pt;
    if (std::getenv("VVHIP_PERIODIC_DEBUG"))
        for (size_t r = 0; r < pt.regions.size() && r < 16; r++) std::fprintf(stderr, "  region %zu: unit of %d cluster(s), %d atoms, x%d\n", r, pt.regions[r].p, pt.regions[r].atoms, pt.regions[r].reps);
    pt.ok = layout_regions(pt);
    return pt;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Wave packing and the slot table
// ---------------------------------------------------------------------------------------------------------------------------------------
inline size_t lane_at(int w, int l) { return (size_t) w * 64 + l; }      // index of a lane in the [64*waves] tables

struct Packing {
    std::vector<int32_t> slots;              // becomes HostPlan::slots: (shard-relative particle or -1, role word) per lane
    std::vector<int32_t> lane_of, wave_of;   // of a particle, -1: none
    int nwaves = 0, used = 0;
    std::vector<double> seg_mass;            // become HostPlan::seg_mass, seg_base
    std::vector<int32_t> seg_base;

    int32_t atom(size_t k) const { return slots[2 * k]; }
    int32_t atom(int w, int l) const { return slots[2 * lane_at(w, l)]; }
    uint32_t meta(int w, int l) const { return (uint32_t) slots[2 * lane_at(w, l) + 1]; }
    void put(int w, int l, int32_t atom, uint32_t meta) { slots[2 * lane_at(w, l)] = atom; slots[2 * lane_at(w, l) + 1] = (int32_t) meta; }
};

// The role word (vv_layout.h: ROLE_*, META_*) of member k of cluster c, whose first member sits in first_lane; partner_lane: the lane of
// its Drude partner as far as it is known (fix_partner_lanes)
uint32_t role_word(const Model& m, const Cluster& c, int k, int first_lane, int partner_lane) {
    const Topology& t = m.top;
    const int i = c.members[k], sz = (int) c.members.size(), lane = first_lane + k;
    const bool massive = m.sys.masses[i] != 0.0;
    uint32_t role;
    if (t.is_nh[i] && (massive || t.in_pair[i]))
        role = t.in_pair[i] ? (t.is_drude[i] ? ROLE_NH_DRUDE : ROLE_NH_PARENT) : ROLE_NH_NORMAL;
    else if (t.is_ld[i] && (massive || t.in_pair[i]))
        role = t.in_pair[i] ? (t.is_drude[i] ? ROLE_LD_DRUDE : ROLE_LD_PARENT) : ROLE_LD_NORMAL;
    else
        role = massive ? ROLE_PLAIN : ROLE_NONE;
    uint32_t meta = role;
    meta |= (uint32_t) partner_lane << META_PARTNER_SHIFT;
    const int sf = c.com_segment ? first_lane : lane, sl = c.com_segment ? first_lane + sz - 1 : lane;
    meta |= (uint32_t) sf << META_SEGFIRST_SHIFT;
    meta |= (uint32_t) sl << META_SEGLAST_SHIFT;
    if (t.is_el[i]) meta |= META_EFIELD;
    if (t.image_of[i] >= 0) meta |= META_HAS_IMAGE;
    if (c.com_segment && k == sz - 1) meta |= META_COM_LEADER;      // the LAST lane: its wave-prefix value already ends the segment (kernel A's KE stage)
    if (t.in_pair[i]) meta |= META_PAIR;
    if (t.is_drude[i]) meta |= META_IS_DRUDE;
    if (massive) meta |= META_MASSIVE;
    if (m.cons.shake_of[i] >= 0 || (m.cons.general && !m.cons.gc_adj[i].empty())) meta |= META_SHAKE;
    if (c.big >= 0) meta |= META_BIGMOL;
    if (c.big >= 0 && c.big_first && (meta & META_COM_LEADER)) meta |= META_BIG_FIRST;
    return meta;
}

// partner lanes were only known for the earlier member of each pair: fix them up
void fix_partner_lanes(const Topology& t, const Shard& shard, Packing& pk) {
    for (int w = 0; w < pk.nwaves; w++)
        for (int l = 0; l < 64; l++) {
            const int32_t a = pk.atom(w, l);
            if (a < 0 || !t.in_pair[a + shard.begin]) continue;
            const int partner = t.partner[a + shard.begin];
            if (pk.wave_of[partner] != w)
                throw Error(VVHIP_ERR_UNSUPPORTED, "a Drude particle and its parent are in different molecules");
            pk.put(w, l, a, (pk.meta(w, l) & ~(0x3Fu << META_PARTNER_SHIFT)) | (uint32_t) pk.lane_of[partner] << META_PARTNER_SHIFT);
        }
}

// Compacts the per-segment table (`sparse`: mass and reciprocal at the first lane of every COM segment): segments numbered wave by wave,
// inside a wave by the lane of their leader (what the kernels recompute as seg_base[wave] + popcount of the leader lanes below: one 32-byte
// COM velocity per segment, stored back to back, instead of one at every segment's first-lane position of a 64-entry page per wave)
void compact_segments(const std::vector<double>& sparse, Packing& pk) {
    pk.seg_base.assign((size_t) pk.nwaves + 1, 0);
    for (int w = 0; w < pk.nwaves; w++) {
        pk.seg_base[w] = (int32_t) (pk.seg_mass.size() / 2);
        for (int l = 0; l < 64; l++) {
            if (pk.atom(w, l) < 0 || !(pk.meta(w, l) & META_COM_LEADER)) continue;
            const int first = (pk.meta(w, l) >> META_SEGFIRST_SHIFT) & 63;
            pk.seg_mass.push_back(sparse[2 * lane_at(w, first)]);
            pk.seg_mass.push_back(sparse[2 * lane_at(w, first) + 1]);
        }
    }
    pk.seg_base[pk.nwaves] = (int32_t) (pk.seg_mass.size() / 2);
    // one spare entry: the kernels load table[seg_base[wave] + leaders below the lane] unconditionally, and the lanes behind a
    // wave's last leader point one entry past the wave's segments (the device COM tables are sized from this one)
    pk.seg_mass.push_back(0.0); pk.seg_mass.push_back(0.0);
}

// Clusters are visited in particle order and placed best-fit -- into the open wave whose free lanes they fill most tightly, else into a
// new wave.  Visiting in order keeps neighbouring molecules in neighbouring waves (coalescing, L2 locality); best-fit lets e.g. a
// 10-particle anion complete a wave that two 27-particle cations left at 54 lanes (C3: 87 % -> 99 % lane use, 13 % fewer waves).  O(64)
// per cluster via free-lane buckets.  With a periodic layout the position of every cluster is given by the formula instead.
Packing pack_waves(const Model& m, const std::vector<Cluster>& clusters, const Shard& shard, const PeriodicTry* periodic) {
    const vvhip_system_desc& sys = m.sys;
    Packing pk;
    std::vector<double> sparse;                           // (mass, 1/mass) at the first lane of a COM segment
    std::vector<int32_t> fill;                            // lanes used per wave
    std::vector<std::vector<int32_t> > open_by_free(65);  // waves with exactly f free lanes (stacks)
    // General constraint clusters: a wave's constraint list lives one constraint per LANE, so a wave holds 64 of them whatever its lanes
    // hold -- the packer counts them too (round-4 advisor: HAngles on hydrocarbon-rich molecules, ~1.5 constraints per particle, filled the
    // lanes of a wave with molecules whose constraints did not fit its list, and the whole System lost the fused path).
    std::vector<int32_t> cons_fill;                       // general constraints per wave
    auto cons_of = [&](const Cluster& c) {
        if (!m.cons.general) return 0;
        size_t deg = 0;
        for (int i : c.members) deg += m.cons.gc_adj[i].size();
        return (int) (deg / 2);
    };
    auto new_wave = [&]() {
        const int w = (int) fill.size();
        fill.push_back(0); cons_fill.push_back(0);
        pk.slots.resize((size_t) (w + 1) * 128);
        sparse.resize((size_t) (w + 1) * 128, 0.0);
        for (int l = 0; l < 64; l++) pk.put(w, l, -1, 0);
        return w;
    };
    auto best_fit_wave = [&](int sz, int nc) {
        for (int f = sz; f <= 63; f++) {
            auto& bucket = open_by_free[f];
            for (size_t t = bucket.size(); t-- > 0;)
                if (cons_fill[bucket[t]] + nc <= 64) { const int w = bucket[t]; bucket.erase(bucket.begin() + (long) t); return w; }
        }
        return -1;
    };
    pk.lane_of.assign(sys.num_atoms, -1); pk.wave_of.assign(sys.num_atoms, -1);
    if (periodic) for (long w = 0; w < (long) periodic->per.wpc * periodic->per.ncells; w++) new_wave();
    // Measured on MI355X: best-fit wins while the working set is cache resident (111 k particles: +3 %, 0.9 M: +4 %) and loses
    // once the kernels are HBM bound (8.9 M: -5 %, segments from distant index ranges cost partial cache lines), so very large
    // systems keep plain in-order filling.
    size_t total_lanes = 0;
    for (const Cluster& c : clusters) total_lanes += c.members.size();
    const bool best_fit = total_lanes < ((size_t) 1 << 20);
    int last_wave = -1;
    for (size_t ci = 0; ci < clusters.size(); ci++) {
        const Cluster& c = clusters[ci];
        const int sz = (int) c.members.size(), nc = cons_of(c);
        int wave = -1;
        if (periodic) {
            int lane;
            periodic->place(clusters, ci, wave, lane);
            fill[wave] = lane;
        } else if (best_fit) {
            wave = best_fit_wave(sz, nc);
        } else if (last_wave >= 0 && fill[last_wave] + sz <= 64 && cons_fill[last_wave] + nc <= 64) {
            wave = last_wave;
        }
        if (wave < 0) wave = new_wave();
        cons_fill[wave] += nc;
        last_wave = wave;
        const int first_lane = fill[wave];
        fill[wave] += sz;
        if (!periodic && best_fit && fill[wave] < 64) open_by_free[64 - fill[wave]].push_back(wave);
        for (int k = 0; k < sz; k++) { pk.lane_of[c.members[k]] = first_lane + k; pk.wave_of[c.members[k]] = wave; }
        if (c.com_segment) {
            double mass = 0;
            for (int i : c.members) if (m.top.is_nh[i] && sys.masses[i] != 0.0) mass += sys.masses[i];
            sparse[2 * lane_at(wave, first_lane)] = mass;
            sparse[2 * lane_at(wave, first_lane) + 1] = mass != 0 ? 1.0 / mass : 0.0;
        }
        for (int k = 0; k < sz; k++) {
            const int i = c.members[k], lp = m.top.in_pair[i] ? pk.lane_of[m.top.partner[i]] : -1;
            pk.put(wave, first_lane + k, i - shard.begin, role_word(m, c, k, first_lane, lp >= 0 ? lp : first_lane + k));
            pk.used++;
        }
    }
    if (fill.empty()) new_wave();
    pk.nwaves = (int) fill.size();
    fix_partner_lanes(m.top, shard, pk);
    compact_segments(sparse, pk);
    return pk;
}

// Does the formula reproduce the table?  Particle index, role word (against the pattern wave: the region's first wave of cell 0)
// and segment mass (against the pattern wave's segments) of every lane.
bool periodic_matches(const vvhip_system_desc& sys, const Shard& shard, const PeriodicLayout& per, const Packing& pk) {
    if (pk.nwaves != per.wpc * per.ncells) return false;
    for (int w = 0; w < pk.nwaves; w++) {
        const int cell = per.ncells > 1 ? (int) (((uint64_t) (uint32_t) w * per.magic) >> 32) : 0;
        if (cell != w / per.wpc) return false;
        const int wl = w - cell * per.wpc, r = region_of_wave(per, wl);
        const int wr = wl - per.reg_wave_start[r], a0 = per.reg_atom_start[r] + wr * per.reg_P[r];
        const int count = std::min(per.reg_P[r], per.reg_atom_end[r] - a0);
        const int pw = per.reg_wave_start[r];
        int ord = 0;
        for (int l = 0; l < 64; l++) {
            const int32_t at = pk.atom(w, l);
            const uint32_t meta = pk.meta(w, l);
            if (l >= count) { if (at >= 0) return false; continue; }
            if (at != cell * per.apc + a0 + l) return false;
            if (meta != pk.meta(pw, l)) return false;
            if (sys.masses[at + shard.begin] != sys.masses[pk.atom(pw, l) + shard.begin]) return false;      // (the per-lane mass tables are pattern rows too)
            if (meta & META_COM_LEADER) {
                const size_t here = (size_t) pk.seg_base[w] + ord, pat = (size_t) per.reg_seg_start[r] + ord;
                if ((int) here != cell * per.spc + per.reg_seg_start[r] + wr * per.reg_spw[r] + ord) return false;
                if (std::memcmp(&pk.seg_mass[2 * here], &pk.seg_mass[2 * pat], 16) != 0) return false;
                ord++;
            }
        }
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Per-lane tables
// ---------------------------------------------------------------------------------------------------------------------------------------
void image_table(const vvhip_system_desc& sys, const Topology& t, const Shard& shard, const Packing& pk, HostPlan& hp) {
    hp.slot_image.assign((size_t) pk.nwaves * 64, -1);
    for (int k = 0; k < sys.num_image_pairs; k++) {
        int img = sys.image_pairs[2 * k], par = sys.image_pairs[2 * k + 1];
        if (!shard.has(par)) continue;
        if (!shard.has(img)) throw Error(VVHIP_ERR_UNSUPPORTED, "image particle outside its parent's shard (image charges are single-GPU)");
        hp.image_pairs.push_back(img - shard.begin);
        hp.image_pairs.push_back(par - shard.begin);
    }
    for (size_t k = 0; k < hp.slot_image.size(); k++) {
        const int32_t a = pk.atom(k);
        if (a >= 0 && t.image_of[a + shard.begin] >= 0) hp.slot_image[k] = t.image_of[a + shard.begin] - shard.begin;
    }
}

// Langevin random offsets (K/drudeLangevin.cu:20,30,51-52): normal i -> i, pair i -> Nn + 2 i
void random_table(const Shard& shard, const Packing& pk, HostPlan& hp) {
    std::vector<int32_t> rand_of(hp.num_atoms, -1);
    for (size_t i = 0; i < hp.normal_ld.size(); i++) rand_of[hp.normal_ld[i]] = (int32_t) i;
    for (size_t i = 0; i < hp.pairs_ld.size() / 2; i++)
        rand_of[hp.pairs_ld[2 * i]] = rand_of[hp.pairs_ld[2 * i + 1]] = (int32_t) (hp.normal_ld.size() + 2 * i);
    hp.slot_rand.assign((size_t) pk.nwaves * 64, -1);
    for (size_t k = 0; k < hp.slot_rand.size(); k++)
        if (pk.atom(k) >= 0) hp.slot_rand[k] = rand_of[pk.atom(k) + shard.begin];
}

void big_table(const std::vector<Cluster>& clusters, const Shard& shard, const Packing& pk, HostPlan& hp) {
    std::vector<int32_t> big_of(hp.num_atoms, -1);
    for (const Cluster& cl : clusters)
        if (cl.big >= 0) for (int i : cl.members) big_of[i] = cl.big;
    hp.slot_big.assign((size_t) pk.nwaves * 64, -1);
    for (size_t k = 0; k < hp.slot_big.size(); k++)
        if (pk.atom(k) >= 0) hp.slot_big[k] = big_of[pk.atom(k) + shard.begin];
}

// SHAKE / SETTLE: every member's word lists the whole cluster (vv_host.hpp: SHAKE_WORD_*), every member carries the parameters
void shake_tables(const vvhip_system_desc& sys, const std::vector<Shake>& shakes, const Shard& shard, const Packing& pk, HostPlan& hp) {
    hp.slot_shake.assign((size_t) pk.nwaves * 64, 0);
    hp.slot_shake_param.assign((size_t) pk.nwaves * 64 * 4, 0.0f);
    for (const Shake& s : shakes) {
        if (!shard.has(s.center)) continue;
        const int w = pk.wave_of[s.center], lc = pk.lane_of[s.center];
        uint32_t common = ((uint32_t) s.periph.size() << 2) | ((uint32_t) lc << vv::SHAKE_WORD_CENTRAL_SHIFT) | (s.settle ? vv::SHAKE_WORD_SETTLE : 0u);
        for (size_t k = 0; k < 3; k++) {
            int lane = lc;
            if (k < s.periph.size()) {
                const int q = s.periph[k];
                if (pk.wave_of[q] != w) throw Error(VVHIP_ERR_UNSUPPORTED, "a constraint cluster does not fit into one wave with its molecule");
                lane = pk.lane_of[q];
            }
            common |= (uint32_t) lane << (4 + 6 * k);
        }
        const double imc = 1.0 / sys.masses[s.center], imp = 1.0 / sys.masses[s.periph[0]];
        float prm[4];
        if (s.settle) { prm[0] = (float) s.d; prm[1] = (float) s.d_pp; prm[2] = 0; prm[3] = 0; hp.info.num_settle_clusters++; }   // apex-partner and partner-partner distance
        else { prm[0] = (float) imc; prm[1] = (float) (0.5 / (imc + imp)); prm[2] = (float) (s.d * s.d); prm[3] = (float) imp; hp.info.num_shake_clusters++; }
        hp.slot_shake[lane_at(w, lc)] = (int32_t) (common | 1u);
        std::memcpy(&hp.slot_shake_param[lane_at(w, lc) * 4], prm, sizeof(prm));
        for (size_t k = 0; k < s.periph.size(); k++) {
            const int lq = pk.lane_of[s.periph[k]];
            hp.slot_shake[lane_at(w, lq)] = (int32_t) (common | 2u | ((uint32_t) k << vv::SHAKE_WORD_OWN_SHIFT));
            std::memcpy(&hp.slot_shake_param[lane_at(w, lq) * 4], prm, sizeof(prm));
        }
    }
}

// Virtual sites: word of the placing lane = lanes of the site's parents | kind (| hosted: the lane belongs to a parent and stores the
// site by its particle index, vsite_atom), record = row of vsite_params / vsite_atom.  A site whose parents sit in another wave (another
// molecule, a molecule cut into chunks) or have no lane at all: nothing is placed in-kernel, the caller keeps running its own
// computeVirtualSites.
void site_tables(const vvhip_system_desc& sys, const SitePlan& sites, const Shard& shard, const Packing& pk, HostPlan& hp) {
    std::vector<int32_t> table((size_t) pk.nwaves * 128, 0), atoms;
    std::vector<double> prm;
    int count = 0;
    for (int k = 0; k < sys.num_virtual_sites; k++) {
        const int32_t* rec = sys.virtual_sites + 5 * (size_t) k;
        const int site = rec[0], kind = rec[1], np = num_parents(kind), host = sites.vs_host[(size_t) k];
        bool any = shard.has(site), all = shard.has(site);
        for (int q = 0; q < np; q++) { any = any || shard.has(rec[2 + q]); all = all && shard.has(rec[2 + q]); }
        if (!any) continue;
        // (a shard that holds a site but not its parents, or the reverse, could place it nowhere and no other rank would: refuse it)
        if (!all) throw Error(VVHIP_ERR_INVALID, "particle shard cuts a virtual site from its parents");
        const int w = pk.wave_of[host];
        if (w < 0) return;
        uint32_t word = vv::VS_WORD_VALID | ((uint32_t) kind << 18) | (host != site ? vv::VS_WORD_HOSTED : 0u);
        for (int q = 0; q < 3; q++) {
            const int par = rec[2 + (q < np ? q : 0)];
            if (!shard.has(par) || pk.wave_of[par] != w) return;
            word |= (uint32_t) pk.lane_of[par] << (6 * q);
        }
        table[lane_at(w, pk.lane_of[host]) * 2] = (int32_t) word;
        table[lane_at(w, pk.lane_of[host]) * 2 + 1] = count++;
        atoms.push_back(site - shard.begin);
        prm.insert(prm.end(), sys.virtual_site_params + 12 * (size_t) k, sys.virtual_site_params + 12 * (size_t) k + 12);
    }
    if (count == 0) return;
    hp.slot_vsite.swap(table);
    hp.vsite_params.swap(prm);
    hp.vsite_atom.swap(atoms);
    hp.info.num_virtual_sites = count;
}

// General clusters.  Per wave: its constraints, coloured greedily in System order (two constraints that share a particle get different
// colours: a colour's constraints are relaxed side by side, one per lane), sorted by colour and handed to lanes 0, 1, ... of the wave.
// Word: bit 31 valid | colour << 12 | lane of b << 6 | lane of a; parameters: d^2, 0.5 / (1/m_a + 1/m_b), 1/m_a, 1/m_b (float, as
// OpenMM keeps its SHAKE parameters).  A wave with more than 64 constraints, more than 16 colours, or a constraint across two waves
// (a molecule cut into chunks): not fused (hp.unfused_reason), the split entry points take over as before.
void general_tables(const vvhip_system_desc& sys, const ConstraintPlan& cons, const Shard& shard, const Packing& pk, HostPlan& hp) {
    // relaxation factor of the sweeps (vv_layout.h: GC_OMEGA_*): by whether any three constraints close a triangle
    bool triangles = false;
    for (int k = 0; k < sys.num_constraints && !triangles; k++) {
        const int a = sys.constraints[2 * k], b = sys.constraints[2 * k + 1];
        for (int q : cons.gc_adj[a])
            if (q != b && std::find(cons.gc_adj[b].begin(), cons.gc_adj[b].end(), q) != cons.gc_adj[b].end()) { triangles = true; break; }
    }
    hp.gc_omega = triangles ? vv::GC_OMEGA_TRIANGLES : vv::GC_OMEGA_PLAIN;
    struct GC { int la, lb, colour; float prm[4]; };
    std::vector<std::vector<GC> > per_wave((size_t) pk.nwaves);
    std::vector<uint32_t> used_colours((size_t) pk.nwaves * 64, 0u);
    for (int k = 0; k < sys.num_constraints && hp.unfused_reason.empty(); k++) {
        const int a = sys.constraints[2 * k], b = sys.constraints[2 * k + 1];
        if (!shard.has(a) && !shard.has(b)) continue;
        if (!shard.has(a) || !shard.has(b)) throw Error(VVHIP_ERR_INVALID, "particle shard cuts a Drude pair or a constraint cluster");
        const int w = pk.wave_of[a];
        if (w < 0 || pk.wave_of[b] != w) { hp.unfused_reason = "a constraint connects particles of two waves (a molecule larger than a wave, cut into chunks)"; break; }
        const int la = pk.lane_of[a], lb = pk.lane_of[b];
        const uint32_t taken = used_colours[lane_at(w, la)] | used_colours[lane_at(w, lb)];
        int colour = 0;
        while (colour < 16 && ((taken >> colour) & 1u)) colour++;
        if (colour >= 16) { hp.unfused_reason = "a particle takes part in more constraints than the 16 colours of a wave's sweeps can separate"; break; }
        used_colours[lane_at(w, la)] |= 1u << colour;
        used_colours[lane_at(w, lb)] |= 1u << colour;
        const double ima = 1.0 / sys.masses[a], imb = 1.0 / sys.masses[b], d = sys.constraint_distances[k];
        GC g{la, lb, colour, {(float) (d * d), (float) (0.5 / (ima + imb)), (float) ima, (float) imb}};
        per_wave[(size_t) w].push_back(g);
        if (per_wave[(size_t) w].size() > 64) hp.unfused_reason = "a connected component of the constraint graph holds more than the 64 constraints of a wave's list";
        hp.gc_colors = std::max(hp.gc_colors, colour + 1);
    }
    if (!hp.unfused_reason.empty()) {
        hp.info.constraints_fused = 0;
        hp.gc_colors = 0;
        return;
    }
    hp.info.general_relaxation = hp.gc_omega;
    hp.slot_shake.assign((size_t) pk.nwaves * 64, 0);
    hp.slot_shake_param.assign((size_t) pk.nwaves * 64 * 4, 0.0f);
    for (int w = 0; w < pk.nwaves; w++) {
        auto& list = per_wave[(size_t) w];
        std::stable_sort(list.begin(), list.end(), [](const GC& x, const GC& y) { return x.colour < y.colour; });
        for (size_t l = 0; l < list.size(); l++) {
            const GC& g = list[l];
            hp.slot_shake[lane_at(w, (int) l)] = (int32_t) (vv::GC_WORD_VALID | ((uint32_t) g.colour << 12) | ((uint32_t) g.lb << 6) | (uint32_t) g.la);
            std::memcpy(&hp.slot_shake_param[lane_at(w, (int) l) * 4], g.prm, sizeof(g.prm));
            hp.info.num_general_constraints++;
        }
    }
}

// Under the periodic layout the constraint words and parameters of every wave must be those of its region's pattern wave too
bool periodic_constraints_match(const PeriodicLayout& per, const Packing& pk, const HostPlan& hp) {
    for (int w = 0; w < pk.nwaves; w++) {
        const int pw = per.reg_wave_start[region_of_wave(per, w % per.wpc)];
        for (int l = 0; l < 64; l++) {
            if (pk.atom(w, l) < 0) continue;
            if (hp.slot_shake[lane_at(w, l)] != hp.slot_shake[lane_at(pw, l)] ||
                std::memcmp(&hp.slot_shake_param[lane_at(w, l) * 4], &hp.slot_shake_param[lane_at(pw, l) * 4], 16) != 0) return false;
        }
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The riders' tables
// ---------------------------------------------------------------------------------------------------------------------------------------
// shard-local numbers, by ascending molecule id, of the molecules that `present` marks; -1 for the others
std::vector<int32_t> number_molecules(const std::vector<char>& present) {
    std::vector<int32_t> local(present.size(), -1);
    int32_t next = 0;
    for (size_t m = 0; m < present.size(); m++) if (present[m]) local[m] = next++;
    return local;
}

// which particles of the shard (shard-relative) have a lane
std::vector<char> lanes_of_shard(const Shard& shard, const Packing& pk) {
    std::vector<char> has_lane((size_t) (shard.end - shard.begin), 0);
    for (size_t k = 0; k < (size_t) pk.nwaves * 64; k++) if (pk.atom(k) >= 0) has_lane[(size_t) pk.atom(k)] = 1;
    return has_lane;
}

// Drude temperature report (vv_host.hpp: report_*).  DOFs as examples/ommhelper/reporter/drudetemperaturereporter.py counts them:
// COM 3 n_M (- 3 with a CMMotionRemover), atomic 3 n_m - 3 n_M - n_c - 3 n_p (the remover does not enter), Drude 3 n_p.
void report_tables(const vvhip_system_desc& sys, const Topology& t, const Shard& shard, const Packing& pk, HostPlan& hp) {
    const int n = sys.num_atoms, nmol = sys.num_molecules, npairs = sys.num_drude_pairs;
    int n_massive = 0, n_mol_massive = 0;
    for (int i = 0; i < n; i++) if (sys.masses[i] > 0) n_massive++;
    for (int m = 0; m < nmol; m++) if (t.mol_mass[m] > 0) n_mol_massive++;
    hp.report_dof[0] = 3.0 * n_mol_massive - (sys.has_cm_motion_remover ? 3.0 : 0.0);
    hp.report_dof[1] = 3.0 * n_massive - 3.0 * n_mol_massive - sys.num_constraints - 3.0 * npairs;
    hp.report_dof[2] = 3.0 * npairs;
    // every sum has at most n terms (also over all shards): lo < 2^(61 - bits(n)) and |x| 2^16 < 2^(61 - bits(n)) keep both words' sums
    // inside int64.  The limit on a term (2.7e8 at 0.1 M particles, 2e6 at 9 M: kJ/mol for m|v|^2, Da nm/ps for m v) is far above
    // physical values; a velocity beyond it makes the report fail, never the step.
    int bits = 1;
    while (bits < 40 && ((int64_t) 1 << bits) <= (int64_t) n) bits++;
    hp.report_unit_bits = 16;
    hp.report_frac_bits = 61 - bits;
    hp.report_limit = std::ldexp(1.0, 61 - bits - hp.report_unit_bits);
    std::vector<char> massive_here(nmol, 0);      // the report's molecules: those with a massive particle in the shard
    for (int i = shard.begin; i < shard.end; i++) if (sys.masses[i] > 0) massive_here[sys.mol_id[i]] = 1;
    const std::vector<int32_t> local = number_molecules(massive_here);
    for (int m = 0; m < nmol; m++) if (local[m] >= 0) hp.report_mol_mass.push_back(t.mol_mass[m]);
    for (int i = 0; i < n && hp.report_unsupported.empty(); i++)
        if (!shard.has(i) && sys.masses[i] > 0 && local[sys.mol_id[i]] >= 0)
            hp.report_unsupported = "the particle shard cuts a molecule: its centre-of-mass velocity needs particles of another shard";
    const size_t ns = (size_t) pk.nwaves * 64;
    hp.report_lane_mol.assign(ns, -1);
    hp.report_lane_mass.assign(ns, 0.0);
    hp.report_lane_mu.assign(ns, 0.0);
    for (size_t k = 0; k < ns; k++) {
        if (pk.atom(k) < 0) continue;
        const int i = pk.atom(k) + shard.begin;
        if (sys.masses[i] > 0) { hp.report_lane_mass[k] = sys.masses[i]; hp.report_lane_mol[k] = local[sys.mol_id[i]]; }
        if (t.is_drude[i] && sys.mol_id[t.partner[i]] == sys.mol_id[i]) hp.report_lane_mu[k] = reduced_mass(sys, i, t.partner[i]);
    }
    for (int k = 0; k < npairs; k++) {
        const int d = sys.drude_pairs[2 * k], c = sys.drude_pairs[2 * k + 1];
        if (!shard.has(d) || sys.mol_id[d] == sys.mol_id[c]) continue;
        const int32_t rec[4] = {d - shard.begin, c - shard.begin, local[sys.mol_id[d]], local[sys.mol_id[c]]};
        hp.report_cross.insert(hp.report_cross.end(), rec, rec + 4);
        hp.report_cross_mu.push_back(reduced_mass(sys, d, c));
    }
}

// Maxwell-Boltzmann start velocities (vv_host.hpp: therm_*)
void thermalize_tables(const vvhip_system_desc& sys, const Shard& shard, const std::vector<char>& has_lane, HostPlan& hp) {
    for (int i = shard.begin; i < shard.end; i++) {
        if (sys.masses[i] > 0) { hp.therm_massive++; continue; }
        hp.therm_massless++;
        if (!has_lane[(size_t) (i - shard.begin)]) hp.therm_laneless.push_back(i - shard.begin);
    }
    for (int k = 0; k < sys.num_drude_pairs; k++) {
        const int d = sys.drude_pairs[2 * k], c = sys.drude_pairs[2 * k + 1];
        if (shard.has(d) && shard.has(c) && reduced_mass(sys, d, c) > 0) hp.therm_pairs++;
    }
}

// Monte Carlo barostat (vv_host.hpp: baro_*): EVERY particle of the shard belongs to a molecule, massless ones included, so the
// report's lane table (-1 on massless lanes) does not serve.  The fixed point follows the largest molecule of the WHOLE System:
// |Q| < 2^(22 + F) and n_max <= 2^(40 - F) terms keep a molecule's sum below 2^62 on every shard alike.
void barostat_tables(const vvhip_system_desc& sys, const Shard& shard, const Packing& pk, const std::vector<char>& has_lane, HostPlan& hp) {
    const int n = sys.num_atoms, nmol = sys.num_molecules;
    std::vector<int32_t> mol_count(nmol, 0), here(nmol, 0);
    for (int i = 0; i < n; i++) mol_count[sys.mol_id[i]]++;
    int32_t n_max = 1;
    for (int m = 0; m < nmol; m++) n_max = std::max(n_max, mol_count[m]);
    int lg = 0;
    while (((int64_t) 1 << lg) < (int64_t) n_max) lg++;
    hp.baro_frac_bits = 40 - lg;
    hp.baro_num_molecules = nmol;
    std::vector<char> present(nmol, 0);           // the barostat's molecules: those with any particle in the shard
    for (int i = shard.begin; i < shard.end; i++) { here[sys.mol_id[i]]++; present[sys.mol_id[i]] = 1; }
    const std::vector<int32_t> local = number_molecules(present);
    for (int m = 0; m < nmol; m++) {
        if (!present[m]) continue;
        if (here[m] != mol_count[m] && hp.baro_unsupported.empty())
            hp.baro_unsupported = "the particle shard cuts a molecule: its centre needs particles of another shard";
        hp.baro_mol_count.push_back((double) mol_count[m]);
    }
    hp.baro_lane_mol.assign((size_t) pk.nwaves * 64, -1);
    for (size_t k = 0; k < hp.baro_lane_mol.size(); k++)
        if (pk.atom(k) >= 0) hp.baro_lane_mol[k] = local[sys.mol_id[pk.atom(k) + shard.begin]];
    for (int i = shard.begin; i < shard.end; i++)
        if (!has_lane[(size_t) (i - shard.begin)]) { hp.baro_laneless.push_back(i - shard.begin); hp.baro_laneless.push_back(local[sys.mol_id[i]]); }
}

void check_arguments(const vvhip_system_desc& sys, const vvhip_params& params, int precision) {
    if (precision != VVHIP_SINGLE && precision != VVHIP_MIXED && precision != VVHIP_DOUBLE)
        throw Error(VVHIP_ERR_INVALID, "unknown precision mode");
    if (sys.num_atoms <= 0 || !sys.masses || !sys.mol_id || sys.num_molecules <= 0)
        throw Error(VVHIP_ERR_INVALID, "system description is empty");
    if (sys.padded_num_atoms < sys.num_atoms)
        throw Error(VVHIP_ERR_INVALID, "padded_num_atoms < num_atoms");
    if (params.num_nh_chains < 1 || params.num_nh_chains > VVHIP_MAX_CHAINS)
        throw Error(VVHIP_ERR_UNSUPPORTED, "numNHChains must be between 1 and " + std::to_string(VVHIP_MAX_CHAINS));
    if (params.loops_per_step < 1)
        throw Error(VVHIP_ERR_INVALID, "loopsPerStep must be >= 1");
}
}  // namespace

HostPlan analyze(const vvhip_system_desc& sys, const vvhip_params& params_in, int precision) {
    check_arguments(sys, params_in, precision);
    const bool debug = std::getenv("VVHIP_PERIODIC_DEBUG") != nullptr;
    HostPlan hp;
    hp.precision = precision;
    hp.params = params_in;
    hp.num_atoms = sys.num_atoms;
    hp.padded_num_atoms = sys.padded_num_atoms;
    vvhip_params& p = hp.params;
    vvhip_plan_info& info = hp.info;
    // ---- API:106-121: thermostat defaults depend on whether the System has Drude particles
    if (p.auto_set_com_temp_group) p.use_com_temp_group = sys.num_drude_pairs == 0 ? 0 : 1;
    if (p.auto_set_friction) p.friction = sys.num_drude_pairs == 0 ? 1.0 : 5.0;

    // ---- the System: thermostat partition, constraints, virtual sites
    const Topology top = classify(sys, hp);
    thermostat_groups(sys, top, hp);
    Shard shard{sys.shard_begin, sys.shard_end};
    if (shard.begin == 0 && shard.end == 0) shard.end = sys.num_atoms;
    if (shard.begin < 0 || shard.end > sys.num_atoms || shard.begin >= shard.end) throw Error(VVHIP_ERR_INVALID, "bad particle shard range");
    hp.shard_begin = shard.begin; hp.shard_end = shard.end;
    hp.masses.assign(sys.masses, sys.masses + sys.num_atoms);
    hp.mol_id.assign(sys.mol_id, sys.mol_id + sys.num_atoms);
    const ConstraintPlan cons = classify_constraints(sys);
    const SitePlan sites = plan_sites(sys, top);
    const Model model{sys, top, cons, sites};

    // ---- which particles need a lane, and which must share a wave
    std::vector<Cluster> clusters = build_clusters(model, shard, p.use_com_temp_group != 0);
    split_big_molecules(model, clusters, hp);
    std::stable_sort(clusters.begin(), clusters.end(), [](const Cluster& a, const Cluster& b) { return a.first < b.first; });
    for (auto& c : clusters) {
        std::sort(c.members.begin(), c.members.end());
        info.max_cluster = std::max(info.max_cluster, (int) c.members.size());
    }

    // ---- the waves: by the periodic formula if it reproduces its own table, else packed
    PeriodicTry periodic = try_periodic(model, clusters, shard, hp);
    if (debug) std::fprintf(stderr, "periodic: try=%d regions=%zu R=%d cells=%d wpc=%d apc=%d\n", (int) periodic.ok, periodic.regions.size(), periodic.R, periodic.per.ncells, periodic.per.wpc, periodic.per.apc);
    Packing pk = pack_waves(model, clusters, shard, periodic.ok ? &periodic : nullptr);
    if (periodic.ok && !periodic_matches(sys, shard, periodic.per, pk)) {
        if (debug) std::fprintf(stderr, "periodic: formula does not reproduce the table\n");
        periodic.ok = false;
        pk = pack_waves(model, clusters, shard, nullptr);
    }
    if (periodic.ok) { hp.per = periodic.per; hp.per.enabled = 1; }
    info.num_waves = pk.nwaves;
    info.num_slots_used = pk.used;
    info.periodic_layout = periodic.ok ? 1 : 0;

    // ---- per-lane tables
    if (hp.has_images) image_table(sys, top, shard, pk, hp);
    if (hp.has_ld) random_table(shard, pk, hp);
    info.constraints_fused = cons.fused ? 1 : 0;
    if (!cons.shakes.empty()) shake_tables(sys, cons.shakes, shard, pk, hp);
    if (sites.enabled) site_tables(sys, sites, shard, pk, hp);
    if (cons.general) general_tables(sys, cons, shard, pk, hp);
    if (hp.per.enabled && !cons.shakes.empty() && !periodic_constraints_match(hp.per, pk, hp)) {
        hp.per.enabled = 0;      // the layout stays, the kernels load their slot words
        info.periodic_layout = 0;
    }
    if (hp.num_big > 0) big_table(clusters, shard, pk, hp);

    // ---- the riders' tables
    const std::vector<char> has_lane = lanes_of_shard(shard, pk);
    report_tables(sys, top, shard, pk, hp);
    thermalize_tables(sys, shard, has_lane, hp);
    barostat_tables(sys, shard, pk, has_lane, hp);

    hp.slots = std::move(pk.slots);
    hp.seg_mass = std::move(pk.seg_mass);
    hp.seg_base = std::move(pk.seg_base);
    return hp;
}

}  // namespace vv
