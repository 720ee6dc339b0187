"""The host tables of the seven accumulating recorders (vvhip_profile_* .. vvhip_acf_*), pinned on the CPU: every case calls *_start on an
unbound plan -- which keeps a description that passes the checks and answers ERR_INVALID "vvhip_bind" -- and writes one line: recorder,
case, return code, the whole error text, every field of the *_info layout by name, and vvhip_debug_recorder_digest (FNV-1a 64 over index,
first, weight, items, ... as include/vvhip.h states them).  tests/golden/recorder_tables.txt holds those lines as the builders gave them
before their shared parts were stated once (vv_observe.cpp: "the shared pieces of a start"), so any change of any table, layout field,
refusal order or message shows.  `python tests/test_recorder_tables.py` prints the lines."""
import ctypes as C
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import barostat_cases as K      # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S = pkg.systems
GOLDEN = os.path.join(ROOT, "tests", "golden", "recorder_tables.txt")


def _I():
    return importlib.import_module("openmm-velocityverlet_amd.integrator")


def _ptr(a):
    return None if a is None else a.ctypes.data


def _i8(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int8)


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------ one description per recorder, as the ABI takes it
def _profile(H, n, interval=10, axis=2, nbins=64, mask=1, num_groups=1, group=None, max_samples=1000, limit=(0, 0, 0, 0)):
    g = _i8(group)
    return H.ProfileDesc(interval, axis, nbins, mask, num_groups, 0, _ptr(g), max_samples, (C.c_double * 4)(*limit)), (g,)


def _msd(H, n, interval=10, num_lags=8, origin_every=1, mode=0, num_groups=1, group=None, max_samples=1000, limit=0.0):
    g = _i8(group)
    return H.MsdDesc(interval, num_lags, origin_every, mode, num_groups, 0, _ptr(g), max_samples, limit), (g,)


def _acf(H, n, interval=10, num_lags=8, origin_every=1, mode=0, num_groups=1, group=None, pairs=None, max_samples=1000, limit=0.0, num_pairs=None):
    g = _i8(group)
    pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    return H.AcfDesc(interval, num_lags, origin_every, mode, num_groups, (0 if pr is None else len(pr)) if num_pairs is None else num_pairs,
                     _ptr(g), _ptr(pr), max_samples, limit), (g, pr)


def _rdf(H, n, interval=10, nbins=64, num_groups=1, classes=((0, 0),), exclude=0, group=None, max_samples=1000, r_max=0.5, num_classes=None,
         null_classes=False):
    g = _i8(group)
    cls = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1, 2)
    return H.RdfDesc(interval, nbins, num_groups, len(cls) if num_classes is None else num_classes, exclude, 0, _ptr(g),
                     None if null_classes else cls.ctypes.data, max_samples, r_max), (g, cls)


def _contacts(H, n, interval=10, num_lags=8, origin_every=2, num_groups=1, classes=((0, 0),), r_cut=(0.5,), exclude=0, continuous=1, group=None,
              max_samples=1000, num_classes=None, null_classes=False, null_cut=False):
    g = _i8(group)
    cls = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1, 2)
    cut = np.ascontiguousarray(r_cut, dtype=np.float64)
    return H.ContactsDesc(interval, num_lags, origin_every, num_groups, len(cls) if num_classes is None else num_classes, exclude, continuous, 0,
                          _ptr(g), None if null_classes else cls.ctypes.data, None if null_cut else cut.ctypes.data, max_samples), (g, cls, cut)


def _current(H, n, interval=10, num_lags=8, origin_every=1, num_groups=1, weight="ones", group=None, max_samples=1000, limit_position=0.0,
             limit_velocity=0.0):
    w = np.ones(n) if isinstance(weight, str) else _f64(weight)
    g = _i8(group)
    return H.CurrentDesc(interval, num_lags, origin_every, num_groups, _ptr(w), _ptr(g), max_samples, limit_position, limit_velocity), (w, g)


ONE_MODE = np.array([[1, 0, 0]], dtype=np.int32)


def _modes(H, n, interval=10, num_lags=8, origin_every=1, num_groups=1, weight="ones", group=None, modes=ONE_MODE, num_modes=None, max_samples=1000,
           limit_position=0.0):
    w = np.ones(n) if isinstance(weight, str) else _f64(weight)
    g = _i8(group)
    m = None if modes is None else np.ascontiguousarray(modes, dtype=np.int32).reshape(-1, 3)
    k = num_modes if num_modes is not None else (1 if m is None else m.shape[0])
    return H.ModesDesc(interval, num_lags, origin_every, num_groups, k, _ptr(w), _ptr(g), _ptr(m), max_samples, limit_position), (w, g, m)


DESC = {"profile": _profile, "msd": _msd, "acf": _acf, "rdf": _rdf, "contacts": _contacts, "current": _current, "modes": _modes}
LAYOUT = {"profile": "ProfileLayout", "msd": "MsdLayout", "acf": "AcfLayout", "rdf": "RdfLayout", "contacts": "ContactsLayout",
          "current": "CurrentLayout", "modes": "ModesLayout"}
TUNES = ("rdf_items_target", "contacts_rows_per_tile", "contacts_words_per_item", "current_two_level", "modes_sites_per_thread", "modes_k_tile",
         "modes_block_threads")


def _value(v):
    if hasattr(v, "_length_"):
        return "[" + ",".join(_value(x) for x in v) + "]"
    return repr(v)


class Corpus:
    """The plans (one per system, shard, box and set of knobs) and the lines."""

    def __init__(self):
        self.I = _I()
        self.H = self.I.H
        self.plans = {}
        self.atoms = {}                               # id(plan) -> particles of its System
        self.keep = []
        self.lines = []
        self.systems = {"syn": K.synthetic(), "c3": S.make_config("C3", scale=0.05)}

    def close(self):
        for plan in self.plans.values():
            self.H.lib.vvhip_plan_destroy(plan)
        self.plans = {}

    def plan(self, system, shard=None, box=None, tune=()):
        key = (system, shard, box, tuple(tune))
        if key not in self.plans:
            H = self.H
            it = self.I.VVIntegrator(300.0, 10.0, 1.0, 40.0, 0.001)
            it.setUseCOMTempGroup(False)
            plan, _, keep = self.I.create_plan(self.systems[system], it, "mixed", shard)
            self.keep.append(keep)
            if box is not None:
                assert H.lib.vvhip_set_box(plan, C.byref((C.c_double * 3)(*box))) == H.OK
            for name, value in tune:
                assert name in TUNES and H.lib.vvhip_debug_tune(plan, name.encode(), int(value)) == H.OK, name
            self.plans[key] = plan
            self.atoms[id(plan)] = self.systems[system].num_atoms
        return self.plans[key]

    def case(self, recorder, case, plan, **kw):
        """One start and its line.  Whatever an earlier case left described goes first: a refused start keeps nothing of ITS description."""
        H = self.H
        n = self.atoms[id(plan)]
        assert getattr(H.lib, "vvhip_%s_stop" % recorder)(plan) == H.OK
        desc, alive = DESC[recorder](H, n, **kw)
        rc = getattr(H.lib, "vvhip_%s_start" % recorder)(plan, C.byref(desc))
        err = H.lib.vvhip_last_error(plan).decode() if rc != H.OK else ""
        lay = getattr(H, LAYOUT[recorder])()
        assert getattr(H.lib, "vvhip_%s_info" % recorder)(plan, C.byref(lay)) == H.OK
        digest = C.c_uint64(0)
        assert H.lib.vvhip_debug_recorder_digest(plan, recorder.encode(), C.byref(digest)) == H.OK
        kept = rc == H.ERR_INVALID and err == "vvhip_bind has not been called"
        assert rc != H.OK and (digest.value != 0) == kept, (recorder, case, rc, err)      # (no plan here is bound)
        fields = " ".join("%s=%s" % (f[0], _value(getattr(lay, f[0]))) for f in lay._fields_)
        self.lines.append("%s %s rc=%d err=%r %s digest=%016x" % (recorder, case, rc, err, fields, digest.value))
        del alive
        return rc, err


# ------------------------------------------------------------------------------------------ the accepted descriptions
def _groupings(n, ids):
    """(name, num_groups, group): none; -1, 0, 1 in turn; nothing recorded; more groups than are in use; everything in group 0."""
    third = (np.asarray(ids) % 3 - 1).astype(np.int8)
    return [("none", 1, None), ("third", 2, third), ("nothing", 1, np.full(n, -1, dtype=np.int8)), ("spare", 5, third),
            ("zeros", 1, np.zeros(n, dtype=np.int8))]


def _shards(c, system):
    spec = c.systems[system]
    n = spec.num_atoms
    if system == "syn":
        cut = K.shard_cut(spec)
    else:
        mol = np.asarray(spec.mol_id)
        cut = int(np.nonzero(mol == mol[n // 2])[0].min())
    assert 0 < cut < n
    return [("whole", None), ("front", (0, cut)), ("back", (cut, n))]


def accepted(c):
    for system, spec in c.systems.items():
        n = spec.num_atoms
        mol = np.asarray(spec.mol_id)
        by_particle, by_molecule = _groupings(n, np.arange(n)), _groupings(n, mol)
        # ---- units: msd, acf (particles and molecules), profile
        for sname, shard in _shards(c, system):
            plan = c.plan(system, shard)
            for rec in ("msd", "acf"):
                for mode, groupings in ((0, by_particle), (1, by_molecule)):
                    for gname, G, group in groupings:
                        c.case(rec, "%s-%s-mode%d-%s" % (system, sname, mode, gname), plan, mode=mode, num_lags=7, origin_every=3, num_groups=G, group=group,
                               max_samples=5000, limit=3.0 if gname == "third" else 0.0)
            for mask in (1, 31):
                for gname, G, group in by_particle:
                    c.case("profile", "%s-%s-mask%d-%s" % (system, sname, mask, gname), plan, mask=mask, nbins=17, num_groups=G, group=group,
                           limit=(0, 0, 0, 0) if gname == "none" else (3.0, 0, 1000.0, 8.0))
        if system == "syn":      # the shard that cuts a molecule: particle mode does not mind
            plan = c.plan(system, (0, 3))
            for rec in ("msd", "acf"):
                for gname, G, group in by_particle[:2]:
                    c.case(rec, "syn-cut-mode0-%s" % gname, plan, mode=0, num_groups=G, group=group)
        # ---- acf, orientation: the Drude pairs
        if len(spec.drude_pairs):
            pairs = np.asarray(spec.drude_pairs, dtype=np.int32)[:, :2]
            per_pair = (np.arange(len(pairs)) % 3 - 1).astype(np.int8)
            for sname, shard in _shards(c, system):
                plan = c.plan(system, shard)
                c.case("acf", "%s-%s-orientation-none" % (system, sname), plan, mode=2, pairs=pairs, num_lags=5, origin_every=2)
                c.case("acf", "%s-%s-orientation-third" % (system, sname), plan, mode=2, pairs=pairs[::-1], num_groups=2, group=per_pair, max_samples=1 << 20)
                c.case("acf", "%s-%s-orientation-spare" % (system, sname), plan, mode=2, pairs=pairs, num_groups=4, group=per_pair)
                c.case("acf", "%s-%s-orientation-nopairs" % (system, sname), plan, mode=2, pairs=None, num_pairs=0)
        # ---- sites by group: rdf, contacts
        box = (2.0, 2.0, 2.0)
        lone = np.full(n, -1, dtype=np.int8)
        lone[n // 3] = 0
        lone[5::11] = 1
        three = [(0, 1), (0, 0), (1, 1)]
        site_cases = [("none", dict()), ("nothing", dict(group=by_particle[2][2])),
                      ("third", dict(num_groups=2, group=by_particle[1][2], classes=three)),
                      ("empty-group", dict(num_groups=5, group=by_particle[1][2], classes=[(0, 4), (4, 4), (1, 0)])),
                      ("lone", dict(num_groups=2, group=lone, classes=[(0, 0), (0, 1), (1, 0)]))]
        for tname, tune in (("default", ()), ("target1", (("rdf_items_target", 1),))):
            plan = c.plan(system, None, box, tune)
            for cname, kw in site_cases:
                for exclude in (0, 1):
                    c.case("rdf", "%s-%s-%s-x%d" % (system, tname, cname, exclude), plan, nbins=33, r_max=0.7, exclude=exclude, **kw)
        for tname, tune in (("default", ()), ("rows64", (("contacts_rows_per_tile", 64),)), ("rows128-words1", (("contacts_rows_per_tile", 128), ("contacts_words_per_item", 1)))):
            plan = c.plan(system, None, box, tune)
            for cname, kw in site_cases:
                cuts = [0.3 + 0.1 * k for k in range(len(kw.get("classes", [0])))]
                for exclude, continuous in ((0, 1), (1, 0)) if tname != "default" else ((0, 0), (0, 1), (1, 0), (1, 1)):
                    c.case("contacts", "%s-%s-%s-x%d-c%d" % (system, tname, cname, exclude, continuous), plan, num_lags=5, origin_every=2, r_cut=cuts,
                           exclude=exclude, continuous=continuous, **kw)
        # ---- sites by group with weights: current, modes
        I = c.I
        weights = [("charges", I.current_weights(spec)), ("molecules", I.current_weights(spec, molecules=True))]
        for two in (0, 1):
            plan = c.plan(system, None, None, (("current_two_level", two),))
            for wname, w in weights:
                for gname, G, group in by_particle[:4]:
                    c.case("current", "%s-two%d-%s-%s" % (system, two, wname, gname), plan, num_lags=6, origin_every=4, num_groups=G, group=group, weight=w,
                           limit_velocity=5.0)
        many = np.array([(k % 5 - 2, k // 5 - 3, k % 7) for k in range(33)], dtype=np.int32)
        for tname, tune in (("auto", ()), ("pinned", (("modes_sites_per_thread", 2), ("modes_k_tile", 8), ("modes_block_threads", 128)))):
            plan = c.plan(system, None, None, tune)
            for num_lags in (0, 8):
                for kname, modes in (("k1", ONE_MODE), ("k33", many)):
                    for gname, G, group in by_particle[:4]:
                        c.case("modes", "%s-%s-lags%d-%s-%s" % (system, tname, num_lags, kname, gname), plan, num_lags=num_lags, origin_every=3 if num_lags else 1,
                               num_groups=G, group=group, modes=modes, weight=weights[0][1] * 0.25)


# ------------------------------------------------------------------------------------------ the refusals, rung by rung
def _ladder(c, recorder, name, plan, kw, steps):
    """Everything wrong at once, then one thing put right at a time (tests/test_msd.py, test_acf.py)."""
    kw = dict(kw)
    for k, fix in enumerate(steps):
        c.case(recorder, "%s-%02d" % (name, k), plan, **kw)
        if fix:
            kw.update(fix)
    return kw


def _later(c, recorder, name, plan, later, order):
    """Each rung wrong in its own argument AND in every one behind it (tests/test_rdf.py, test_contacts.py, test_current.py, test_modes.py)."""
    names = [k for k, _ in order]
    for pos, (_, fault) in enumerate(order):
        kw = {k: v for k, v in later.items() if k in names[pos + 1:]}
        kw.update(fault)
        c.case(recorder, "%s-%02d" % (name, pos), plan, **kw)


def refusals(c):
    syn, c3 = c.systems["syn"], c.systems["c3"]
    n = syn.num_atoms
    # ---- msd, acf: the synthetic system under the shard (0, 3), which cuts a molecule
    mixed = (np.arange(n) // 4 % 2).astype(np.int8)
    bad_entry = mixed.copy()
    bad_entry[3] = 5
    plan = c.plan("syn", (0, 3))
    kw = dict(interval=0, num_lags=5000, origin_every=0, mode=7, num_groups=17, group=bad_entry, max_samples=0, limit=-1.0)
    steps = [dict(interval=10), dict(num_lags=4096), dict(origin_every=1), dict(mode=1), dict(num_groups=2), dict(max_samples=1 << 61), dict(limit=0.0),
             dict(group=mixed), dict(group=None), dict(max_samples=1000), dict(origin_every=4), None]
    kw = _ladder(c, "msd", "ladder", plan, kw, steps)
    c.case("msd", "ladder-particles", plan, **dict(kw, mode=0))
    kw = dict(interval=0, num_lags=5000, origin_every=0, mode=7, num_groups=17, group=bad_entry, max_samples=0, limit=-1.0, pairs=[[1, 5]])
    steps = steps[:7] + [dict(pairs=None)] + steps[7:]
    kw = _ladder(c, "acf", "ladder", plan, kw, steps)
    kw.update(mode=2, limit=1.0, pairs=[[1, 5], [2, 2], [0, n], [1, 2], [2, 6]], group=np.array([0, 1, 0, 7, 0], dtype=np.int8))
    steps = [dict(limit=0.0), dict(group=None), dict(pairs=[[1, 5], [0, n], [1, 2], [2, 6]]), dict(pairs=[[1, 5], [1, 2], [2, 6]]), dict(pairs=[[1, 5], [2, 6]]), None]
    kw = _ladder(c, "acf", "ladder-orientation", plan, kw, steps)
    c.case("acf", "ladder-orientation-needs-pairs", plan, **dict(kw, pairs=None, num_pairs=2))
    c.case("acf", "ladder-orientation-bad-pair-in-group-minus-1", plan, **dict(kw, pairs=[[1, 5], [0, n]], group=np.array([0, -1], dtype=np.int8)))
    c.case("acf", "ladder-particles", plan, **dict(kw, mode=0, pairs=None))
    # ---- profile: C3
    n = c3.num_atoms
    plan = c.plan("c3")
    order = [dict(interval=0), dict(axis=3), dict(nbins=0), dict(mask=32 | 1), dict(num_groups=17), dict(max_samples=0), dict(limit=(0, -1.0, 0, 0))]
    for k in range(len(order)):
        kw = {}
        for bad in order[k:]:
            kw.update(bad)
        c.case("profile", "order-%02d" % k, plan, **kw)
    group = np.zeros(n, dtype=np.int8)
    group[5] = 2
    c.case("profile", "group-above", plan, num_groups=2, group=group)
    group[5] = -2
    c.case("profile", "group-below", plan, num_groups=2, group=group)
    c.case("profile", "bits-kinetic", plan, mask=1 | 16, max_samples=1 << 40)
    c.case("profile", "bits-momentum", plan, mask=1 | 2 | 8, max_samples=1 << 20, limit=(0, 0, 2.0 ** 30, 0))
    c.case("profile", "count-alone", plan, mask=1, max_samples=1 << 40)
    # ---- rdf, contacts: C3 in a box of 2 nm
    mol = np.asarray(c3.mol_id)
    cut = int(np.nonzero(mol == mol[n // 2])[0].min())
    bad_group = np.zeros(n, dtype=np.int8)
    bad_group[3] = 2
    plan, front = c.plan("c3", None, (2.0, 2.0, 2.0)), c.plan("c3", (0, cut), (2.0, 2.0, 2.0))
    _later(c, "rdf", "order", plan, dict(r_max=-1.0, nbins=0, num_groups=17, num_classes=33, null_classes=True, max_samples=0),
           [("interval", dict(interval=0)), ("r_max", dict(r_max=float("inf"))), ("nbins", dict(nbins=8193)), ("num_groups", dict(num_groups=0)),
            ("num_classes", dict(num_classes=0)), ("null_classes", dict(null_classes=True)), ("max_samples", dict(max_samples=0))])
    pairs = n * (n - 1) // 2
    for name, kw in [("r_max-zero", dict(r_max=0.0)), ("r_max-nan", dict(r_max=float("nan"))),
                     ("group", dict(num_groups=2, group=bad_group, classes=[(0, 5)], max_samples=1 << 62, r_max=1.5)),
                     ("class", dict(num_groups=2, classes=[(0, 1), (0, 5)], max_samples=1 << 62, r_max=1.5)),
                     ("overflow", dict(max_samples=1 << 62, r_max=1.5)), ("overflow-edge", dict(max_samples=(1 << 62) // pairs + 1, r_max=1.5)),
                     ("box", dict(max_samples=((1 << 62) - 1) // pairs, r_max=1.5)), ("half-box-passes", dict(r_max=1.0))]:
        c.case("rdf", name, plan, **kw)
    c.case("rdf", "shard-box", front, r_max=1.5)
    c.case("rdf", "shard", front, r_max=1.0)
    _later(c, "contacts", "order", plan, dict(num_lags=0, origin_every=0, num_groups=17, num_classes=9, null_classes=True, null_cut=True, max_samples=0),
           [("interval", dict(interval=0)), ("num_lags", dict(num_lags=4097)), ("origin_every", dict(origin_every=9)), ("num_groups", dict(num_groups=0)),
            ("num_classes", dict(num_classes=0)), ("null_classes", dict(null_classes=True)), ("null_cut", dict(null_cut=True)), ("max_samples", dict(max_samples=0))])
    big = dict(num_lags=4096, origin_every=1, max_samples=1 << 62)
    for name, kw in [("group", dict(num_groups=2, group=bad_group, classes=[(0, 5)], r_cut=[-1.0], **big)),
                     ("class", dict(num_groups=2, classes=[(0, 1), (0, 5)], r_cut=[-1.0, 1.0], **big)),
                     ("cut-negative", dict(r_cut=[-1.0], **big)), ("cut-zero", dict(r_cut=[0.0], **big)), ("cut-inf", dict(r_cut=[float("inf")], **big)),
                     ("cut-nan", dict(r_cut=[float("nan")], **big)), ("origins", dict(r_cut=[1.5], **big)),
                     ("overflow", dict(r_cut=[1.5], num_lags=4096, origin_every=4, max_samples=1 << 62)),
                     ("overflow-edge", dict(r_cut=[1.5], max_samples=(1 << 62) // (n * n) + 1)),
                     ("bytes", dict(r_cut=[1.5], num_lags=4096, origin_every=4, max_samples=((1 << 62) - 1) // (n * n))),
                     ("box", dict(r_cut=[1.5])), ("half-box-passes", dict(r_cut=[1.0]))]:
        c.case("contacts", name, plan, **kw)
    c.case("contacts", "shard-box", front, r_cut=[1.5])
    c.case("contacts", "shard", front, r_cut=[1.0])
    # ---- current, modes: C3
    plan, front, back = c.plan("c3"), c.plan("c3", (0, cut)), c.plan("c3", (cut, n))
    bad_weight = np.ones(n)
    bad_weight[5] = np.inf
    nan_weight = np.ones(n)
    nan_weight[n - 1] = np.nan
    _later(c, "current", "order", plan, dict(num_lags=0, origin_every=0, num_groups=9, max_samples=0, limit_position=-1.0, limit_velocity=float("nan"), weight=None),
           [("interval", dict(interval=0)), ("num_lags", dict(num_lags=4097)), ("origin_every", dict(num_lags=8, origin_every=9)), ("num_groups", dict(num_groups=0)),
            ("max_samples", dict(max_samples=0)), ("limit_position", dict(limit_position=float("inf"))), ("limit_velocity", dict(limit_velocity=-2.0)),
            ("weight", dict(weight=None))])
    edge = 62 - int(n).bit_length() - 1 - 8      # (ceil_log2(n + 1) = bit_length(n); W = 2 for weights of 1: the last limit with 8 bits)
    for name, kw in [("group", dict(num_groups=2, group=bad_group, weight=bad_weight, limit_position=2.0 ** 60)), ("weight-inf", dict(weight=bad_weight, limit_position=2.0 ** 60)),
                     ("weight-nan", dict(weight=nan_weight)), ("bits-position", dict(limit_position=2.0 ** 60, limit_velocity=2.0 ** 60)),
                     ("bits-velocity", dict(limit_velocity=2.0 ** 60)), ("bits-edge", dict(limit_position=2.0 ** edge)), ("bits-past-edge", dict(limit_position=2.0 ** (edge + 1)))]:
        c.case("current", name, plan, **kw)
    for sname, shard in (("front", front), ("back", back)):
        c.case("current", "shard-%s-bits" % sname, shard, limit_position=2.0 ** 60)
        c.case("current", "shard-%s" % sname, shard)
    bad_modes = np.array([(1, 0, 0), (0, 4096, 0)], dtype=np.int32)
    _later(c, "modes", "order", plan, dict(num_lags=-1, origin_every=0, num_groups=9, num_modes=0, max_samples=0, limit_position=-1.0, weight=None, modes=None),
           [("interval", dict(interval=0)), ("num_lags", dict(num_lags=4097)), ("origin_every", dict(num_lags=8, origin_every=9)), ("num_groups", dict(num_groups=0)),
            ("num_modes", dict(num_modes=4097)), ("max_samples", dict(max_samples=0)), ("limit_position", dict(limit_position=float("inf"))),
            ("weight", dict(weight=None)), ("modes", dict(modes=None, num_modes=1))])
    heavy = 2.0 ** 23 * np.ones(n)
    wide = np.zeros((4096, 3), dtype=np.int32)
    for name, kw in [("origin-every-without-lags", dict(num_lags=0, origin_every=2)), ("mode", dict(num_groups=2, modes=bad_modes, group=bad_group, weight=bad_weight)),
                     ("mode-negative", dict(modes=np.array([(0, 0, -4096)]))), ("group", dict(num_groups=2, group=bad_group, weight=bad_weight)),
                     ("weight-inf", dict(weight=bad_weight)), ("bits", dict(weight=heavy, num_groups=8, modes=wide, num_lags=255)),
                     ("bits-edge", dict(weight=heavy / 4)), ("bits-past-edge", dict(weight=heavy / 2)), ("table", dict(num_groups=8, modes=wide, num_lags=255)),
                     ("table-edge", dict(num_groups=8, modes=wide, num_lags=254, origin_every=254))]:
        c.case("modes", name, plan, **kw)
    for sname, shard in (("front", front), ("back", back)):
        c.case("modes", "shard-%s-bits" % sname, shard, weight=heavy)
        c.case("modes", "shard-%s" % sname, shard)


def corpus_lines():
    c = Corpus()
    try:
        accepted(c)
        refusals(c)
    finally:
        c.close()
    return c.lines


def test_recorder_tables_equal_the_golden_lines():
    got = corpus_lines()
    want = open(GOLDEN).read().splitlines()
    assert len(set(line.split(" rc=")[0] for line in got)) == len(got)      # every case has a name of its own
    kept = [line for line in got if "err='vvhip_bind has not been called'" in line]
    assert len(kept) >= 400 and len(got) - len(kept) >= 100
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


if __name__ == "__main__":
    print("\n".join(corpus_lines()))
