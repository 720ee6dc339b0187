"""Device-side contact lifetime correlations (include/vvhip.h: vvhip_contacts_*), the host half, no GPU: tests/contacts_reference.py against
a set-of-pairs statement one scalar at a time, an exact lattice with pairs at the cutoff, the table's inequalities, a class of one group
with itself, the exclusion, the ring's corner cases, the layout (an unbound plan's, and vv_layout.h's under the sanitizers in a program of
its own), every refusal of the start in its documented order, the Contacts views, the text writer read back."""
import ctypes as C
import importlib
import io
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contacts_reference as CR      # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S = pkg.systems
R = pkg.reporters

ENTRY_POINTS = ("vvhip_contacts_start", "vvhip_contacts_sample", "vvhip_contacts_read", "vvhip_contacts_stop", "vvhip_contacts_info")


def _I():
    return importlib.import_module("openmm-velocityverlet_amd.integrator")


_SPEC = {}


def _spec():
    if "s" not in _SPEC:
        _SPEC["s"] = S.make_config("C3", scale=0.05)
    return _SPEC["s"]


def _plan(shard=None, box=None):
    I = _I()
    it = I.VVIntegrator(333.0, 10.0, 1.0, 40.0, 0.001)
    plan, _, keep = I.create_plan(_spec(), it, "mixed", shard)
    if box is not None:
        b = (C.c_double * 3)(*box)
        assert I.H.lib.vvhip_set_box(plan, C.byref(b)) == I.H.OK
    return plan, keep


def _describe(plan, interval=10, num_lags=8, origin_every=2, num_groups=1, classes=((0, 0),), r_cut=(0.5,), exclude=0, continuous=1, group=None,
              max_samples=1000, num_classes=None, null_classes=False, null_cut=False):
    """vvhip_contacts_start on an unbound plan: (return code, error text); a description that passes the checks in front of the bind is kept."""
    H = _I().H
    grp = None if group is None else np.ascontiguousarray(group, dtype=np.int8)
    cls = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1, 2)
    cut = np.ascontiguousarray(r_cut, dtype=np.float64)
    desc = H.ContactsDesc(interval, num_lags, origin_every, num_groups, len(cls) if num_classes is None else num_classes, exclude, continuous, 0,
                          None if grp is None else grp.ctypes.data, None if null_classes else cls.ctypes.data, None if null_cut else cut.ctypes.data,
                          max_samples)
    rc = H.lib.vvhip_contacts_start(plan, C.byref(desc))
    return rc, H.lib.vvhip_last_error(plan).decode()


def _info(plan):
    H = _I().H
    lay = H.ContactsLayout()
    assert H.lib.vvhip_contacts_info(plan, C.byref(lay)) == H.OK
    return lay


def test_contacts_entry_points_and_struct_sizes():
    H = _I().H
    header = open(os.path.join(ROOT, "include", "vvhip.h")).read()
    for name in ENTRY_POINTS:
        assert name in H.EXPORTS and hasattr(H.lib, name)
        assert "int %s(" % name in header
    assert C.sizeof(H.ContactsDesc) == 64 and C.sizeof(H.ContactsCounts) == 24 and C.sizeof(H.ContactsLayout) == 432
    assert "#define VVHIP_CONTACTS_MAX_BYTES (1ll << 32)" in header and H.CONTACTS_MAX_BYTES == 1 << 32


# ------------------------------------------------------------------------------------------ the reference against sets of pairs
def _pair_sets(x, box, groups, classes, r_cut, mol_id):
    """Per class the set of (i, j) in contact, one scalar at a time (Python floats are float64; round() is round-half-even), and the NaN pairs."""
    out, invalid = [], 0
    n = len(x)
    for (ga, gb), rc in zip(classes, r_cut):
        pairs = set()
        for i in range(n):
            if groups[i] != ga:
                continue
            for j in range(n):
                if groups[j] != gb or (ga == gb and i == j) or (mol_id is not None and mol_id[i] == mol_id[j]):
                    continue
                d = []
                for a in range(3):
                    t = float(x[i][a]) - float(x[j][a])
                    q = t * (1.0 / box[a])
                    d.append(float("nan") if math.isnan(q) else t - box[a] * float(round(q)))
                r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                if math.isnan(r2):
                    invalid += 1
                elif r2 < rc * rc:
                    pairs.add((i, j))
        out.append(pairs)
    return out, invalid


def _by_origins(sets, num_classes, num_lags, every, continuous=True):
    """The table from the definition of the correlation functions, origin by origin: no ring, no slots."""
    table = np.zeros((num_classes, num_lags, 4), dtype=np.int64)
    for o in range(0, len(sets), every):
        for c in range(num_classes):
            alive = set(sets[o][c])
            for j in range(o, min(len(sets), o + num_lags)):
                alive &= sets[j][c]
                table[c, j - o] += [1, len(sets[o][c]), len(sets[o][c] & sets[j][c]), len(alive) if continuous else 0]
    return table


def _twelve(samples=9, seed=5):
    """Twelve sites in a box of 2 x 2.2 x 2.4 nm doing a small random walk, a third of them starting in other images; groups 0 0 0 0 0 1 1 1
    1 1 -1 -1 by index mod 12 ... as arrays: frames [samples, 12, 3], box, groups, mol_id (pairs of neighbours share a molecule)."""
    rng = np.random.default_rng(seed)
    box = np.array([2.0, 2.2, 2.4])
    x = rng.random((12, 3)) * box * 0.5
    x[::3] += box * np.array([2, -1, 1])
    frames = [x.copy()]
    for _ in range(samples - 1):
        x = x + rng.normal(0, 0.12, (12, 3))
        frames.append(x.copy())
    groups = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1, 1, -1, -1], dtype=np.int8)
    mol = np.arange(12) // 2
    return np.array(frames), box, groups, mol


@pytest.mark.parametrize("exclude", [False, True], ids=["all-pairs", "exclude-same-molecule"])
@pytest.mark.parametrize("num_lags,every", [(4, 1), (5, 2), (1, 1), (9, 3)])
def test_reference_equals_sets_of_pairs(exclude, num_lags, every):
    frames, box, groups, mol = _twelve()
    classes, cut = [(0, 1), (1, 0), (0, 0)], [0.45, 0.45, 0.6]
    m = mol if exclude else None
    sets = [_pair_sets(x, box, groups, classes, cut, m)[0] for x in frames]
    want = _by_origins(sets, 3, num_lags, every)
    got, samples, dropped, invalid = CR.contacts_reference(frames, [box] * len(frames), groups, classes, cut, num_lags, every, m)
    assert (samples, dropped, invalid) == (len(frames), 0, 0)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert want[:, 0, 1].min() > 0 and (num_lags == 1 or np.any(want[:, 1:, 2] < want[:, 1:, 1]))      # contacts exist, and some break
    # the matrices are the sets
    h, bad = CR.contact_matrices(frames[0], box, groups, classes, cut, m)
    ia, ib = CR.sites(groups, 12, 0), CR.sites(groups, 12, 1)
    assert bad == 0 and {(int(ia[i]), int(ib[j])) for i, j in zip(*np.nonzero(h[0]))} == sets[0][0]
    # (1, 0) is the transpose of (0, 1): the same words
    assert np.array_equal(got[0], got[1])


def test_nan_pairs_are_invalid_and_no_contact():
    frames, box, groups, mol = _twelve(samples=2)
    frames[1, 6, 0] = np.nan                                           # one site of group 1
    classes, cut = [(0, 1), (1, 1)], [0.5, 0.5]
    for m in (None, mol):
        got, samples, dropped, invalid = CR.contacts_reference(frames, [box] * 2, groups, classes, cut, 2, 1, m)
        sets = [_pair_sets(x, box, groups, classes, cut, m) for x in frames]
        assert invalid == sets[1][1] == (5 + 2 * 4 if m is None else 5 + 2 * 3)      # five rows of (0, 1); (1, 1) holds each pair twice
        assert np.array_equal(got, _by_origins([s for s, _ in sets], 2, 2, 1))
        assert not any(6 in pr for cls in sets[1][0] for pr in cls)


def _lattice():
    """4 x 4 x 4 sites at multiples of 0.25 nm in a box of 1 nm: every r2 is exact, the nearest neighbours are at r2 = 0.0625 = 0.25^2
    exactly (six each, through the box's faces too), the next at 0.125."""
    g = np.arange(4) * 0.25
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3), np.array([1.0, 1.0, 1.0])


def test_exact_lattice_with_pairs_at_the_cutoff():
    x, box = _lattice()
    r2 = CR.r2_matrix(x, x, box)
    assert set(np.unique(r2)) <= {k * 0.0625 for k in range(13)} and np.count_nonzero(r2 == 0.0625) == 64 * 6
    classes = [(0, 0)] * 3
    cuts = [0.25, np.nextafter(0.25, 1.0), 0.25 * math.sqrt(2.0) + 1e-9]
    assert cuts[0] * cuts[0] == 0.0625 and cuts[1] * cuts[1] > 0.0625
    h, bad = CR.contact_matrices(x, box, None, classes, cuts)
    assert bad == 0
    assert [int(m.sum()) for m in h] == [0, 64 * 6, 64 * 18]           # AT the cutoff is no contact; one ulp above it is; then the 12 diagonals too
    table, samples, _, _ = CR.contacts_reference([x, x, x], [box] * 3, None, classes, cuts, 2, 1)
    assert samples == 3 and np.array_equal(table[0], [[3, 0, 0, 0], [2, 0, 0, 0]])
    assert np.array_equal(table[1], [[3, 3 * 384, 3 * 384, 3 * 384], [2, 2 * 384, 2 * 384, 2 * 384]])


def test_the_words_are_ordered_everywhere():
    frames, box, groups, mol = _twelve(samples=14, seed=11)
    classes, cut = [(0, 1), (0, 0), (1, 1)], [0.5, 0.55, 0.4]
    for num_lags, every in [(6, 1), (6, 4), (14, 5)]:
        t = CR.contacts_reference(frames, [box] * 14, groups, classes, cut, num_lags, every)[0]
        assert np.all(t[..., 3] <= t[..., 2]) and np.all(t[..., 2] <= t[..., 1]) and np.all(t >= 0)
        assert np.array_equal(t[:, 0, 1], t[:, 0, 2]) and np.array_equal(t[:, 0, 2], t[:, 0, 3])      # at the zero lag all three are the origin's contacts
        assert np.any(t[..., 3] < t[..., 2])                           # a pair breaks and re-forms somewhere


def test_a_class_of_one_group_with_itself_counts_each_pair_twice():
    frames, box, groups, mol = _twelve()
    sets, _ = _pair_sets(frames[0], box, groups, [(0, 0)], [0.6], None)
    assert len(sets[0]) > 0 and all((j, i) in sets[0] and i != j for i, j in sets[0])
    h, _ = CR.contact_matrices(frames[0], box, groups, [(0, 0)], [0.6])
    assert np.array_equal(h[0], h[0].T) and not h[0].diagonal().any()
    t = CR.contacts_reference(frames[:1], [box], groups, [(0, 0)], [0.6], 1, 1)[0]
    assert t[0, 0, 1] == 2 * len({frozenset(p) for p in sets[0]})


def test_exclusion_clears_pairs_of_one_molecule():
    frames, box, groups, mol = _twelve()
    groups = np.array([0, 1] * 6, dtype=np.int8)                       # every molecule (i, i + 1) is one pair of class (0, 1)
    frames = frames.copy()
    frames[:, 1::2] = frames[:, 0::2] + 0.01                           # ... and always in contact
    with_, _ = CR.contact_matrices(frames[0], box, groups, [(0, 1)], [0.3])
    without, _ = CR.contact_matrices(frames[0], box, groups, [(0, 1)], [0.3], mol)
    assert with_[0].diagonal().all() and not without[0].diagonal().any()
    off = ~np.eye(6, dtype=bool)
    assert np.array_equal(with_[0][off], without[0][off])


def test_more_slots_than_lags_need():
    """num_lags 5, origin_every 2: R = 3 slots and R E = 6 > 5, so the oldest slot is still held, at l = 5, when it adds nothing."""
    frames, box, groups, mol = _twelve(samples=13)
    classes, cut = [(0, 1)], [0.5]
    rec = CR.Recorder(1, 5, 2)
    assert rec.R == 3
    for k, x in enumerate(frames):
        rec.sample(CR.contact_matrices(x, box, groups, classes, cut)[0])
        if k == 5:
            assert rec.ord == [0, 2, 4]                                # slot 0 holds sample 0 at l = 5 and was skipped
    sets = [_pair_sets(x, box, groups, classes, cut, None)[0] for x in frames]
    assert np.array_equal(rec.words(), _by_origins(sets, 1, 5, 2))
    assert list(rec.words()[0, :, 0]) == [7, 6, 6, 5, 5]


def test_one_lag_and_no_continuous_ring():
    frames, box, groups, mol = _twelve()
    classes, cut = [(0, 1)], [0.5]
    t = CR.contacts_reference(frames, [box] * 9, groups, classes, cut, 1, 1)[0]
    per_sample = [int(CR.contact_matrices(x, box, groups, classes, cut)[0][0].sum()) for x in frames]
    assert t.shape == (1, 1, 4) and list(t[0, 0]) == [9, sum(per_sample), sum(per_sample), sum(per_sample)]
    full = CR.contacts_reference(frames, [box] * 9, groups, classes, cut, 4, 1)[0]
    off = CR.contacts_reference(frames, [box] * 9, groups, classes, cut, 4, 1, continuous=False)[0]
    assert np.array_equal(off[..., :3], full[..., :3]) and not off[..., 3].any() and full[..., 3].any()


def test_max_samples_drops_and_reset_restarts():
    frames, box, groups, mol = _twelve()
    classes, cut = [(0, 1)], [0.5]
    t, samples, dropped, _ = CR.contacts_reference(frames, [box] * 9, groups, classes, cut, 3, 1, max_samples=4)
    assert (samples, dropped) == (4, 5)
    assert np.array_equal(t, CR.contacts_reference(frames[:4], [box] * 4, groups, classes, cut, 3, 1)[0])
    rec = CR.Recorder(1, 3, 1)
    for x in frames[:5]:
        rec.sample(CR.contact_matrices(x, box, groups, classes, cut)[0])
    rec.reset()
    assert rec.ord == [-1] * 3 and rec.samples == 0 and not rec.words().any()
    for x in frames[5:]:
        rec.sample(CR.contact_matrices(x, box, groups, classes, cut)[0])
    assert np.array_equal(rec.words(), CR.contacts_reference(frames[5:], [box] * 4, groups, classes, cut, 3, 1)[0])


# ------------------------------------------------------------------------------------------ the layout
def test_layout_by_hand():
    # 65 rows x 129 columns: 128 padded rows, 3 column words; 1 x 1: 64 and 1; no rows: nothing
    L = CR.layout([65, 1, 0], [129, 1, 7], num_lags=5, origin_every=2, continuous=True, sites_total=200)
    assert L["rows_padded"] == [128, 64, 0] and L["col_words"] == [3, 1, 1] and L["class_words"] == [384, 64, 0] and L["sample_words"] == 448
    assert (L["num_origins"], L["ord_words"], L["table_words"], L["ring_words"]) == (3, 4, 60, 2 * 3 * 448)
    assert L["words_bytes"] == (4 + 60 + 4 + 2688) * 8 and L["scratch_bytes"] == 448 * 8 + 3 * 208 * 8
    assert CR.layout([65], [129], 5, 2, False, 200)["ring_words"] == 3 * 384


def test_layout_of_an_unbound_plan():
    H = _I().H
    n = _spec().num_atoms
    plan, keep = _plan(box=(3.0, 3.2, 3.4))
    try:
        lay = _info(plan)
        assert (lay.active, lay.words, lay.num_lags, lay.total_bytes) == (0, 0, 0, 0)
        groups = (np.arange(n) % 3).astype(np.int8) - 1               # -1, 0, 1
        classes = [(0, 1), (1, 0), (0, 0), (2, 1)]
        rc, text = _describe(plan, interval=7, num_lags=5, origin_every=2, num_groups=3, classes=classes, r_cut=[0.5, 0.6, 1.5, 0.1], group=groups,
                             exclude=1, max_samples=123)
        assert rc == H.ERR_INVALID and "vvhip_bind has not been called" in text
        lay = _info(plan)
        n0, n1 = int(np.count_nonzero(groups == 0)), int(np.count_nonzero(groups == 1))
        assert (lay.active, lay.interval, lay.num_lags, lay.origin_every, lay.num_groups, lay.num_classes, lay.exclude_same_molecule, lay.continuous,
                lay.max_samples, lay.num_origins, lay.words) == (0, 7, 5, 2, 3, 4, 1, 1, 123, 3, 4 * 5 * 4)
        assert list(lay.num_sites[:4]) == [n0, n1, 0, 0] and [tuple(lay.classes[c]) for c in range(4)] == classes
        assert list(lay.rows[:4]) == [n0, n1, n0, 0] and list(lay.cols[:4]) == [n1, n0, n0, n1] and list(lay.r_cut[:4]) == [0.5, 0.6, 1.5, 0.1]
        want = CR.layout(list(lay.rows[:4]), list(lay.cols[:4]), 5, 2, True, n0 + n1)
        assert list(lay.class_words[:4]) == want["class_words"] and want["class_words"][3] == 0 and lay.sample_words == want["sample_words"]
        assert (lay.words_bytes, lay.scratch_bytes, lay.total_bytes) == (want["words_bytes"], want["scratch_bytes"], want["total_bytes"])
        # the defaults of the work lists: tiles of rows x runs of column words; pairs of words in runs of 1024, one item for the empty class
        assert (lay.rows_per_tile, lay.words_per_item, lay.skip_zero_words) == (128, 4, 1)
        tiles = lambda c: -(-want["rows_padded"][c] // lay.rows_per_tile) * -(-want["col_words"][c] // lay.words_per_item)
        assert lay.num_mask_items == sum(tiles(c) for c in range(4))
        assert lay.num_corr_items == sum(max(1, -(-w // 2048)) for w in want["class_words"])
        # continuous = 0: one ring
        assert _describe(plan, num_lags=5, origin_every=2, continuous=0)[0] == H.ERR_INVALID
        lay = _info(plan)
        assert lay.continuous == 0 and lay.words_bytes == CR.layout([n], [n], 5, 2, False, n)["words_bytes"]
        assert H.lib.vvhip_contacts_stop(plan) == H.OK and _info(plan).words == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_layout_and_work_lists_under_the_sanitizers(tmp_path):
    """tests/cpp/contacts_layout_check.cpp, a program of its own built with -fsanitize=address,undefined: it checks that the two work lists
    cover every word exactly once at site counts of 0, 1, 63, 64, 65 and 4 097 and prints the layouts, which are held to layout() here."""
    exe = str(tmp_path / "contacts_layout_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "openmm-velocityverlet_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "contacts_layout_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", (run.stdout[-300:], run.stderr[-2000:])
    lines = [list(map(int, ln.split())) for ln in run.stdout.splitlines()]
    assert len(lines) == 3 * 36
    for na, nb, lags, every, cont, tile, run_, rows_padded0, col_words0, class_words1, sample_words, R_, ord_words, table_words, ring_words, words_bytes, \
            scratch_bytes, total_bytes, nm, nc in lines:
        L = CR.layout([na, nb], [nb, na], lags, every, bool(cont), na + nb)
        assert (rows_padded0, col_words0, class_words1, sample_words, R_, ord_words, table_words, ring_words, words_bytes, scratch_bytes, total_bytes) == \
               (L["rows_padded"][0], L["col_words"][0], L["class_words"][1], L["sample_words"], L["num_origins"], L["ord_words"], L["table_words"],
                L["ring_words"], L["words_bytes"], L["scratch_bytes"], L["total_bytes"])
        assert nm == sum(-(-L["rows_padded"][c] // tile) * -(-L["col_words"][c] // run_) for c in range(2))
        assert nc == sum(max(1, -(-w // 2048)) for w in L["class_words"])
    assert [ln[:2] for ln in lines[:36]] == [[a, b] for a in (0, 1, 63, 64, 65, 4097) for b in (0, 1, 63, 64, 65, 4097)]


# ------------------------------------------------------------------------------------------ the refusals
def test_start_refuses_in_the_documented_order():
    H = _I().H
    n = _spec().num_atoms
    plan, keep = _plan(box=(2.0, 2.0, 2.0))
    try:
        assert H.lib.vvhip_contacts_start(plan, None) == H.ERR_INVALID and "null description" in H.lib.vvhip_last_error(plan).decode()
        bad_group = np.zeros(n, dtype=np.int8)
        bad_group[3] = 2
        # every description carries all the later faults too: the first one in the documented order is the one reported
        later = dict(num_lags=0, origin_every=0, num_groups=17, num_classes=9, null_classes=True, null_cut=True, max_samples=0)
        order = [("interval", dict(interval=0), "interval must be >= 1"),
                 ("num_lags", dict(num_lags=4097), "num_lags must be in [1, 4096]"),
                 ("origin_every", dict(origin_every=9), "origin_every must be in [1, num_lags]"),
                 ("num_groups", dict(num_groups=0), "num_groups must be in [1, 16]"),
                 ("num_classes", dict(num_classes=0), "num_classes must be in [1, 8]"),
                 ("null_classes", dict(null_classes=True), "classes must not be NULL"),
                 ("null_cut", dict(null_cut=True), "r_cut must not be NULL"),
                 ("max_samples", dict(max_samples=0), "max_samples must be >= 1")]
        names = [k for k, _, _ in order]
        for pos, (name, fault, text) in enumerate(order):
            kw = {k: v for k, v in later.items() if k in names[pos + 1:]}
            kw.update(fault)
            rc, err = _describe(plan, **kw)
            assert rc == H.ERR_INVALID and text in err, (name, err)
        # a group entry, a class entry, a cutoff, the slots, the overflow, the cap, the box, then the bind
        big = dict(num_lags=4096, origin_every=1, max_samples=1 << 62)
        rc, err = _describe(plan, num_groups=2, group=bad_group, classes=[(0, 5)], r_cut=[-1.0], **big)
        assert rc == H.ERR_INVALID and "group[3] = 2 is outside [-1, num_groups = 2)" in err
        rc, err = _describe(plan, num_groups=2, classes=[(0, 1), (0, 5)], r_cut=[-1.0, 1.0], **big)
        assert rc == H.ERR_INVALID and "classes[1][1] = 5 is outside [0, num_groups = 2)" in err
        for cut in (-1.0, 0.0, float("inf"), float("nan")):
            rc, err = _describe(plan, r_cut=[cut], **big)
            assert rc == H.ERR_INVALID and "r_cut[0] must be finite and > 0" in err
        rc, err = _describe(plan, r_cut=[1.5], **big)
        assert rc == H.ERR_INVALID and "num_origins" in err and "above 1024" in err
        rc, err = _describe(plan, r_cut=[1.5], num_lags=4096, origin_every=4, max_samples=1 << 62)
        assert rc == H.ERR_INVALID and "reaches 2^62" in err
        assert _describe(plan, r_cut=[1.5], max_samples=(1 << 62) // (n * n) + 1)[1].count("reaches 2^62") == 1
        # R = 1024 slots of n x n bits, twice: above 2^32 bytes as soon as a matrix has 2^18 words
        words = -(-n // 64) * (-(-n // 64) * 64)
        assert 2 * 1024 * words * 8 > 1 << 32
        rc, err = _describe(plan, r_cut=[1.5], num_lags=4096, origin_every=4, max_samples=((1 << 62) - 1) // (n * n))
        assert rc == H.ERR_INVALID and "VVHIP_CONTACTS_MAX_BYTES" in err
        rc, err = _describe(plan, r_cut=[1.5])
        assert rc == H.ERR_INVALID and "above half the shortest edge of the box" in err
        assert _info(plan).words == 0                                # nothing of a refused description is kept
        rc, err = _describe(plan, r_cut=[1.0])                       # exactly min(L) / 2 passes
        assert rc == H.ERR_INVALID and "vvhip_bind has not been called" in err and _info(plan).words == 8 * 4
        assert H.lib.vvhip_contacts_sample(plan) == H.ERR_INVALID and H.lib.vvhip_contacts_read(plan, None, 0, None, 0) == H.ERR_INVALID
    finally:
        H.lib.vvhip_plan_destroy(plan)
    mol = np.asarray(_spec().mol_id)
    cut = int(np.nonzero(mol == mol[n // 2])[0].min())                # a molecule boundary
    assert 0 < cut < n
    plan, keep = _plan(shard=(0, cut), box=(2.0, 2.0, 2.0))
    try:
        rc, err = _describe(plan, r_cut=[1.5])
        assert rc == H.ERR_INVALID and "above half the shortest edge" in err
        rc, err = _describe(plan, r_cut=[1.0])
        assert rc == H.ERR_UNSUPPORTED and "shard" in err and "partial matrix" in err
        assert _info(plan).words == 0 and _info(plan).active == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)


# ------------------------------------------------------------------------------------------ the views and the writer
def _hand_made(continuous=True):
    I = _I()
    # one class of 4 rows x 6 columns, interval 5: 8, 6, 4, 2 origins; C = 1, 0.5, 0.25, 0.125; S = 1, 0.5, 0.125, 0
    words = np.array([[[8, 16, 16, 16], [6, 12, 6, 6], [4, 8, 2, 1], [2, 4, 0, 0]], [[8, 0, 0, 0], [6, 0, 0, 0], [4, 0, 0, 0], [2, 0, 0, 0]]], dtype=np.int64)
    if not continuous:
        words[..., 3] = 0
    return I.Contacts(samples=8, dropped=1, invalid=2, interval=5, origin_every=1, continuous_kept=continuous, classes=np.array([[0, 1], [1, 1]], dtype=np.int32),
                      rows=np.array([4, 6]), cols=np.array([6, 6]), r_cut=np.array([0.5, 0.4]), words=words)


def test_contacts_views():
    con = _hand_made()
    assert list(con.lag_steps) == [0, 5, 10, 15] and list(con.origins) == [8, 6, 4, 2]
    assert list(con.intermittent(0)) == [1.0, 0.5, 0.25, 0.0] and list(con.continuous(0)) == [1.0, 0.5, 0.125, 0.0]
    assert np.all(np.isnan(con.intermittent(1))) and con.mean_contacts(0) == 16 / (8 * 4) and con.mean_contacts(1) == 0.0
    # 0.4 lies between C = 0.5 at 5 steps and 0.25 at 10: 5 + 5 * 0.1 / 0.25 = 7 steps, times dt
    assert con.time_to(0, "intermittent", level=0.4, dt=0.002) == pytest.approx(7 * 0.002, rel=1e-15)
    e = float(np.exp(-1.0))
    assert con.time_to(0, "continuous") == pytest.approx(5 + 5 * (0.5 - e) / 0.375, rel=1e-15) and con.time_to(0) == pytest.approx(5 + 5 * (0.5 - e) / 0.25, rel=1e-15)
    assert math.isnan(con.time_to(0, level=-1.0)) and math.isnan(con.time_to(0, level=2.0)) and math.isnan(con.time_to(1))
    # trapezoids of width 5 dt: (1 + 0.5) / 2 + (0.5 + 0.125) / 2 + 0.125 / 2 = 1.125
    assert con.lifetime(0, "continuous", dt=2.0) == 1.125 * 10.0 and con.lifetime(0, "intermittent", dt=1.0) == (0.75 + 0.375 + 0.125) * 5.0
    with pytest.raises(ValueError):
        con.time_to(0, "neither")
    with pytest.raises(ValueError):
        _hand_made(continuous=False).continuous(0)
    # from the words as the device hands them over
    H = _I().H
    lay, cnt = H.ContactsLayout(), H.ContactsCounts(8, 1, 2)
    lay.num_classes, lay.num_lags, lay.interval, lay.origin_every, lay.continuous = 2, 4, 5, 1, 1
    lay.classes[0][0], lay.classes[0][1], lay.classes[1][0], lay.classes[1][1] = 0, 1, 1, 1
    lay.rows[0], lay.rows[1], lay.cols[0], lay.cols[1], lay.r_cut[0], lay.r_cut[1] = 4, 6, 6, 6, 0.5, 0.4
    back = _I().contacts_from_words(con.words.reshape(-1), lay, cnt)
    assert np.array_equal(back.words, con.words) and (back.samples, back.dropped, back.invalid, back.interval) == (8, 1, 2, 5)
    assert np.array_equal(back.classes, con.classes) and list(back.rows) == [4, 6] and list(back.r_cut) == [0.5, 0.4] and back.continuous_kept


def test_write_contacts_round_trips():
    con = _hand_made()
    buf = io.StringIO()
    R.write_contacts(buf, con, dt=0.001)
    text = buf.getvalue()
    head = text.splitlines()[:2]
    assert head[0] == '#"Samples"\t8\t"Dropped"\t1\t"Invalid"\t2'
    names = [s.strip('"') for s in head[1][1:].split("\t")]
    assert names == ["lag (ps)", "origins"] + ["%s[%s]" % (q, t) for t in ("0-1", "1-1") for q in ("at_origin", "again", "unbroken", "C", "S")]
    data = np.loadtxt(io.StringIO(text), ndmin=2)
    assert data.shape == (4, 12)
    assert np.array_equal(data[:, 0], con.lag_steps * 0.001) and np.array_equal(data[:, 1], [8, 6, 4, 2])
    assert np.array_equal(data[:, 2:5], con.words[0, :, 1:]) and np.array_equal(data[:, 5], con.intermittent(0)) and np.array_equal(data[:, 6], con.continuous(0))
    assert np.all(np.isnan(data[:, 10:]))
    # without the surviving contacts no S column; appended without a header
    buf2 = io.StringIO()
    R.write_contacts(buf2, _hand_made(continuous=False), dt=0.001, header=False)
    assert np.loadtxt(io.StringIO(buf2.getvalue()), ndmin=2).shape == (4, 10)
