"""Device-side spatial distribution functions (include/vvhip.h: vvhip_sdf_*), the host half, no GPU: tests/sdf_reference.py against a
plain loop, the frames' orthonormality and handedness, the layout and the word cap of an unbound plan, every refusal of the start in its
documented order, the struct sizes, the Python views on hand-made counts, both writers read back, the digest of the host tables."""
import ctypes as C
import importlib
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sdf_reference as SR                  # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S = pkg.systems
R = pkg.reporters

ENTRY_POINTS = ("vvhip_sdf_start", "vvhip_sdf_sample", "vvhip_sdf_read", "vvhip_sdf_stop", "vvhip_sdf_info")


def _I():
    return importlib.import_module("openmm-velocityverlet_amd.integrator")


_SPEC = {}


def _spec():
    if "s" not in _SPEC:
        _SPEC["s"] = S.make_config("C3", scale=0.05)
    return _SPEC["s"]


def _frames(spec=None):
    spec = spec or _spec()
    return SR.frames_of_molecules(spec.mol_id, spec.masses, spec.drude_pairs[:, 0])


def _plan(shard=None, box=None):
    I = _I()
    it = I.VVIntegrator(333.0, 10.0, 1.0, 40.0, 0.001)
    plan, _, keep = I.create_plan(_spec(), it, "mixed", shard)
    if box is not None:
        b = (C.c_double * 3)(*box)
        assert I.H.lib.vvhip_set_box(plan, C.byref(b)) == I.H.OK
    return plan, keep


def _describe(plan, interval=10, extent=0.5, nbins=16, frames="default", frame_group=None, site_group=None, classes=((0, 0),), exclude=0,
              max_samples=1000, num_frames=None, num_frame_groups=1, num_site_groups=1, num_classes=None, null_classes=False, null_frames=False):
    """vvhip_sdf_start on an unbound plan: (return code, error text); a description that passes the checks in front of the bind is kept."""
    H = _I().H
    fr = np.ascontiguousarray(_frames() if isinstance(frames, str) else frames, dtype=np.int32).reshape(-1, 3)
    fg = None if frame_group is None else np.ascontiguousarray(frame_group, dtype=np.int8)
    sg = None if site_group is None else np.ascontiguousarray(site_group, dtype=np.int8)
    cls = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1, 2)
    desc = H.SdfDesc(interval, nbins, len(fr) if num_frames is None else num_frames, num_frame_groups, num_site_groups,
                     len(cls) if num_classes is None else num_classes, exclude, 0, None if null_frames or not fr.size else fr.ctypes.data,
                     None if fg is None else fg.ctypes.data, None if sg is None else sg.ctypes.data, None if null_classes else cls.ctypes.data,
                     max_samples, extent)
    rc = H.lib.vvhip_sdf_start(plan, C.byref(desc))
    return rc, H.lib.vvhip_last_error(plan).decode()


def _info(plan):
    H = _I().H
    lay = H.SdfLayout()
    assert H.lib.vvhip_sdf_info(plan, C.byref(lay)) == H.OK
    return lay


def test_entry_points_and_struct_sizes():
    H = _I().H
    header = open(os.path.join(ROOT, "include", "vvhip.h")).read()
    for name in ENTRY_POINTS:
        assert name in H.EXPORTS and hasattr(H.lib, name)
        assert "int %s(" % name in header
    assert C.sizeof(H.SdfDesc) == 8 * 4 + 4 * 8 + 8 + 8 and C.sizeof(H.SdfCounts) == 4 * 8 + 8 + 16 * 8
    assert C.sizeof(H.SdfLayout) == 10 * 4 + 16 * 4 + 16 * 4 + 32 * 4 + 16 * 8 + 4 * 8 + 2 * 8
    assert H.SDF_MAX_WORDS == 1 << 23 and "#define VVHIP_SDF_MAX_WORDS (1ll << 23)" in header
    for cls in ("Sdf", "sdf_from_words"):
        assert hasattr(_I(), cls)
    for method in ("sdf_start", "sdf_sample", "sdf_read", "sdf_stop", "sdf_info"):
        assert hasattr(_I().Context, method)


# ------------------------------------------------------------------------------------------ the reference against a plain loop
def _small_system(rng, nmol=40, per=5, box=(2.5, 3.0, 2.75)):
    """nmol molecules of `per` particles scattered through several images of the box; frames from each molecule's first three."""
    centres = rng.uniform(-4.0, 7.0, size=(nmol, 1, 3))
    x = (centres + rng.normal(0.0, 0.12, size=(nmol, per, 3))).reshape(-1, 3)
    mol = np.repeat(np.arange(nmol), per)
    frames = np.array([[per * m, per * m + 1, per * m + 2] for m in range(nmol)], dtype=np.int32)
    return x, mol, frames, np.array(box)


@pytest.mark.parametrize("exclude", [False, True], ids=["all-sites", "exclude-same-molecule"])
def test_reference_equals_a_plain_loop(exclude):
    rng = np.random.default_rng(3)
    x, mol, frames, box = _small_system(rng)                          # 40 frames, 200 particles
    x[7, 1] = np.nan                                                  # a NaN site (particle 7 is no frame atom of molecule 1: 5, 6, 7 -> it is b)
    x[11] = x[10]                                                     # a on top of o in molecule 2: a bad frame
    x[17] = x[15] + 2.0 * (x[16] - x[15])                             # o, a, b collinear in molecule 3: a bad frame
    x[23, 2] = np.nan                                                 # a NaN site that is no frame atom (molecule 4: 20, 21, 22)
    fg = np.array([0, 1] * 20, dtype=np.int8)
    fg[5] = -1
    sg = (np.arange(len(x)) % 3).astype(np.int8) - 1                  # -1, 0, 1
    classes = [(0, 0), (0, 1), (1, 1), (1, 0)]
    for h, n in ((0.6, 8), (0.35, 3), (0.7, 1)):
        got = SR.sdf_reference(x, box, frames, classes, h, n, fg, sg, mol if exclude else None)
        want = SR.sdf_loop(x, box, frames, classes, h, n, fg, sg, mol if exclude else None)
        assert np.array_equal(got[0], want[0]) and got[0].sum() > 50
        assert got[1] == want[1] and got[1] > 0                       # the NaN site, seen by every good frame of its classes
        assert got[2] == want[2] == 3 and np.array_equal(got[3], want[3]) and got[3].sum() == 39 - 3
    # no groups at all: every frame against every particle
    got = SR.sdf_reference(x, box, frames, [(0, 0)], 0.5, 4, mol_id=mol if exclude else None)
    want = SR.sdf_loop(x, box, frames, [(0, 0)], 0.5, 4, mol_id=mol if exclude else None)
    assert np.array_equal(got[0], want[0]) and got[1:3] == want[1:3] and got[3][0] == 37
    if not exclude:
        assert got[0][0, 2, 2, 2] >= 37                               # every good frame's own origin sits at xi = 0: voxel n / 2 on every axis


# ------------------------------------------------------------------------------------------ the frames
def test_frames_are_orthonormal_and_right_handed():
    rng = np.random.default_rng(9)
    F = 4000
    scale = 2.0 ** rng.integers(-8, 6, size=(F, 1))
    x = np.concatenate([rng.normal(size=(F, 3)) * 5, np.zeros((2 * F, 3))])
    x[F:2 * F] = x[:F] + rng.normal(size=(F, 3)) * scale
    x[2 * F:] = x[:F] + rng.normal(size=(F, 3)) * scale
    frames = np.stack([np.arange(F), np.arange(F) + F, np.arange(F) + 2 * F], axis=1)
    o, E, good = SR.frame_axes(x, frames)
    assert good.all() and np.array_equal(o, x[:F])
    gram = np.einsum("fkc,flc->fkl", E, E)
    # unit length to acf's 2^-49; orthogonality suffers from the cancellation in w = q - t e1 (|q| / |w| of these triplets stays below
    # 2^8), so 2^-40 holds with room
    assert np.abs(gram - np.eye(3)).max() < 2.0 ** -40
    assert np.abs(np.einsum("fkk->fk", gram) - 1.0).max() < 2.0 ** -49
    assert np.all(np.linalg.det(E) > 0.999999)
    # e1 points from o to a, b lies on the positive xi2 side, and a site at X_o + 0.1 (e1 x e2) lands in the upper half of xi3
    p, q = x[F:2 * F] - x[:F], x[2 * F:] - x[:F]
    assert np.all(np.einsum("fc,fc->f", E[:, 0], p) > 0) and np.all(np.einsum("fc,fc->f", E[:, 1], q) > 0)
    box = np.array([40.0, 40.0, 40.0])
    for f in range(0, F, 400):
        site = x[f] + 0.1 * np.cross(E[f, 0], E[f, 1])
        xx = np.concatenate([x, site[None]])
        table, invalid, bad, visits = SR.sdf_reference(xx, box, frames[f:f + 1], [(0, 0)], 0.5, 2,
                                                       site_groups=np.where(np.arange(len(xx)) == len(x), 0, -1))
        # xi = (0, 0, +0.1) up to rounding: xi1 and xi2 are within 2^-40 of 0, on either side, so only xi3's half is asserted
        assert table[0, :, :, 1].sum() == 1 and table.sum() == 1 and (invalid, bad, visits[0]) == (0, 0, 1)
    # bad frames: a on o, collinear, NaN, and an n1 outside [2^-40, 2^40)
    x2 = np.array([[0, 0, 0], [0, 0, 0], [0, 1, 0], [1, 0, 0], [2, 0, 0], [np.nan, 0, 0], [2.0 ** -21, 0, 0], [2.0 ** 20, 0, 0], [0, 1, 0.5]], dtype=np.float64)
    fr2 = [[0, 1, 2], [0, 3, 4], [0, 3, 5], [0, 6, 2], [0, 7, 2], [0, 3, 8], [0, 2, 3]]
    assert list(SR.frame_axes(x2, fr2)[2]) == [False, False, False, False, False, True, True]
    assert np.isnan(SR.frame_axes(x2, fr2)[0][:5]).all()


# ------------------------------------------------------------------------------------------ the layout of an unbound plan
def test_layout_of_an_unbound_plan_and_the_word_cap():
    H = _I().H
    spec = _spec()
    n = spec.num_atoms
    frames = _frames()
    F = len(frames)
    assert F > 20
    plan, keep = _plan(box=(3.0, 3.2, 3.4))
    try:
        lay = _info(plan)
        assert (lay.active, lay.words, lay.nbins, lay.scratch_bytes, lay.num_items) == (0, 0, 0, 0, 0)
        assert H.lib.vvhip_sdf_stop(plan) == H.OK
        fg = (np.arange(F) % 3).astype(np.int8) - 1                   # -1, 0, 1
        sg = (np.arange(n) % 4).astype(np.int8) - 1                   # -1, 0, 1, 2
        classes = [(0, 2), (1, 0), (1, 1), (2, 3)]
        rc, text = _describe(plan, interval=7, extent=0.8, nbins=20, frames=frames, frame_group=fg, site_group=sg, classes=classes, exclude=1,
                             max_samples=123, num_frame_groups=3, num_site_groups=4)
        assert rc == H.ERR_INVALID and "vvhip_bind has not been called" in text
        lay = _info(plan)
        nf = [int(np.count_nonzero(fg == g)) for g in range(3)]
        ns = [int(np.count_nonzero(sg == g)) for g in range(4)]
        assert (lay.active, lay.interval, lay.nbins, lay.num_frame_groups, lay.num_site_groups, lay.num_classes) == (0, 7, 20, 3, 4, 4)
        assert (lay.exclude_same_molecule, lay.max_samples, lay.words) == (1, 123, 4 * 20 ** 3)
        assert list(lay.num_frames[:4]) == nf + [0] and nf[2] == 0 and list(lay.num_sites[:5]) == ns + [0] and ns[3] == 0
        assert [tuple(lay.classes[c]) for c in range(4)] == classes
        assert list(lay.pairs_per_sample[:5]) == [nf[0] * ns[2], nf[1] * ns[0], nf[1] * ns[1], 0, 0]
        assert list(lay.pairs_per_sample[:4]) == list(SR.pairs_per_sample(fg, sg, classes, F, n))
        assert lay.extent == 0.8 and lay.voxel == 2.0 * 0.8 / 20
        stride, fstride = (sum(ns) + 15) // 16 * 16, (sum(nf) + 15) // 16 * 16
        assert lay.scratch_bytes == (3 * stride + 13 * fstride) * 8 and lay.tile >= 64 and lay.tile % 64 == 0
        # a small workload: per i-tile of frames the j-sites in runs of 64; a class with an empty group has no item
        runs = lambda na, nb: -(-na // lay.tile) * -(-nb // 64)
        assert lay.num_items == runs(nf[0], ns[2]) + runs(nf[1], ns[0]) + runs(nf[1], ns[1])
        # no frames at all is a description too
        rc, text = _describe(plan, frames=np.zeros((0, 3), dtype=np.int32))
        assert rc == H.ERR_INVALID and "vvhip_bind has not been called" in text
        lay = _info(plan)
        assert (lay.num_items, lay.words, lay.num_frames[0], lay.num_sites[0], lay.pairs_per_sample[0]) == (0, 16 ** 3, 0, n, 0)
        # the word cap: num_classes * nbins^3 <= 2^23, refused with the count
        rc, text = _describe(plan, nbins=128, classes=[(0, 0)] * 4)
        assert rc == H.ERR_INVALID and "vvhip_bind has not been called" in text and _info(plan).words == 4 * 128 ** 3 == H.SDF_MAX_WORDS
        rc, text = _describe(plan, nbins=128, classes=[(0, 0)] * 5)
        assert rc == H.ERR_INVALID and str(5 * 128 ** 3) in text and "above the cap" in text and "snapshot" in text
        assert _info(plan).words == 4 * 128 ** 3                      # (a refused description leaves the one before it in place)
        assert H.lib.vvhip_sdf_stop(plan) == H.OK and _info(plan).words == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)


# ------------------------------------------------------------------------------------------ the refusals, in their order
def test_start_refuses_in_the_documented_order():
    """Everything wrong at once, then one thing put right at a time: the error names the next one."""
    H = _I().H
    spec = _spec()
    n = spec.num_atoms
    mol = np.asarray(spec.mol_id)
    good = _frames()
    F = len(good)
    other = int(np.nonzero(mol != mol[good[1, 0]])[0][0])            # a particle of another molecule than frame 1's
    outside, twice, spans = good.copy(), good.copy(), good.copy()
    outside[2, 1] = n
    twice[1, 2] = twice[1, 0]
    spans[1, 2] = other
    bad_fg = np.zeros(F, dtype=np.int8)
    bad_fg[4] = 3
    bad_sg = np.zeros(n, dtype=np.int8)
    bad_sg[3] = 2
    pairs = F * n
    plan, keep = _plan(box=(2.0, 2.0, 2.0))
    try:
        assert H.lib.vvhip_sdf_start(plan, None) == H.ERR_INVALID and "null description" in H.lib.vvhip_last_error(plan).decode()
        kw = dict(interval=0, extent=float("nan"), nbins=129, num_frames=-1, num_frame_groups=17, num_site_groups=0, num_classes=17,
                  null_classes=True, null_frames=True, max_samples=0, frame_group=bad_fg, site_group=bad_sg, classes=[(0, 0), (2, 0), (0, 5)],
                  frames=outside)
        steps = [("interval must be >= 1", dict(interval=10)), ("extent must be finite and > 0", dict(extent=float("inf"))),
                 ("extent must be finite and > 0", dict(extent=0.0)), ("extent must be finite and > 0", dict(extent=0.6)),
                 ("nbins must be in [1, 128]", dict(nbins=0)), ("nbins must be in [1, 128]", dict(nbins=128)),
                 ("num_frames must be >= 0", dict(num_frames=None)),
                 ("num_frame_groups must be in [1, 16]", dict(num_frame_groups=2)), ("num_site_groups must be in [1, 16]", dict(num_site_groups=2)),
                 ("num_classes must be in [1, 16]", dict(num_classes=None)), ("classes must not be NULL", dict(null_classes=False)),
                 ("frames must not be NULL with num_frames > 0", dict(null_frames=False)), ("max_samples must be >= 1", dict(max_samples=1 << 62)),
                 ("frame_group[4] = 3 is outside [-1, num_frame_groups = 2)", dict(frame_group=None)),
                 ("site_group[3] = 2 is outside [-1, num_site_groups = 2)", dict(site_group=None)),
                 ("classes[1][0] = 2 is outside [0, num_frame_groups = 2)", dict(classes=[(0, 0), (1, 0), (0, 5)])),
                 ("classes[2][1] = 5 is outside [0, num_site_groups = 2)", dict(classes=[(0, 0)] * 5)),
                 ("frames[2] = {%d, %d, %d} has an index outside the System" % tuple(outside[2]), dict(frames=twice)),
                 ("frames[1] = {%d, %d, %d} names a particle twice" % tuple(twice[1]), dict(frames=spans)),
                 ("frames[1] = {%d, %d, %d} spans molecules" % tuple(spans[1]), dict(frames=good)),
                 ("above the cap", dict(nbins=8)),                    # 5 * 128^3 words
                 ("reaches 2^62", dict(max_samples=(1 << 62) // pairs + 1)),
                 ("reaches 2^62", dict(max_samples=((1 << 62) - 1) // pairs)),
                 ("extent = 0.6", dict(extent=1.0 / np.sqrt(3.0))),   # 3 h^2 must be BELOW (min(L) / 2)^2 = 1 ...
                 ("too large for the box", dict(extent=0.577)),       # ... 0.57735 squared times 3 rounds to 1 or above it
                 ("vvhip_bind has not been called", None)]
        for text, fix in steps:
            rc, err = _describe(plan, **kw)
            assert rc == H.ERR_INVALID and text in err, (text, rc, err)
            if fix:
                assert _info(plan).words == 0                        # nothing of a refused description is kept
                kw.update(fix)
        lay = _info(plan)
        assert lay.words == 5 * 8 ** 3 and lay.active == 0 and lay.pairs_per_sample[0] == pairs and lay.extent == 0.577
        # the rest of the surface on an unbound plan
        assert H.lib.vvhip_sdf_read(plan, None, 0, None, 0) == H.ERR_INVALID
        assert H.lib.vvhip_sdf_sample(plan) == H.ERR_INVALID
        assert H.lib.vvhip_sdf_stop(plan) == H.OK and _info(plan).words == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)
    # a sharded plan: behind the box, in front of the bind
    cut = int(np.nonzero(mol == mol[n // 2])[0].min())                # a molecule boundary
    assert 0 < cut < n
    plan, keep = _plan(shard=(0, cut), box=(2.0, 2.0, 2.0))
    try:
        rc, err = _describe(plan, extent=0.6)
        assert rc == H.ERR_INVALID and "too large for the box" in err
        rc, err = _describe(plan, extent=0.5)
        assert rc == H.ERR_UNSUPPORTED and "shard" in err and "partial table" in err
        assert _info(plan).words == 0 and _info(plan).active == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)


# ------------------------------------------------------------------------------------------ the Python views, the writers
def _hand_made(counts, visits, samples=4, volume=100.0, extent=1.0, classes=((0, 0),), num_sites=(50,), num_frames=(10,)):
    I = _I()
    counts = np.asarray(counts, dtype=np.int64)
    classes = np.asarray(classes, dtype=np.int32).reshape(-1, 2)
    nf, ns = np.asarray(num_frames, dtype=np.int64), np.asarray(num_sites, dtype=np.int64)
    return I.Sdf(samples=samples, dropped=1, invalid=2, bad_frames=3, inv_volume_sum=samples / volume, frame_visits=np.asarray(visits, dtype=np.int64),
                 interval=10, extent=extent, classes=classes, num_frames=nf, num_sites=ns,
                 pairs_per_sample=np.array([nf[a] * ns[b] for a, b in classes], dtype=np.int64), counts=counts)


def test_views_against_their_formulas():
    rng = np.random.default_rng(4)
    counts = rng.integers(0, 50, size=(2, 4, 4, 4))
    s = _hand_made(counts, [40, 0], classes=[(0, 1), (1, 0)], num_sites=(50, 20), num_frames=(10, 5))
    assert s.nbins == 4 and s.voxel == 0.5
    assert np.array_equal(s.edges, [-1.0, -0.5, 0.0, 0.5, 1.0]) and np.array_equal(s.centres, [-0.75, -0.25, 0.25, 0.75])
    rho = s.density(0)
    assert rho.shape == (4, 4, 4) and np.allclose(rho, counts[0] / (40 * 0.125), rtol=1e-15)
    assert np.allclose(s.g(0), rho / (20 * 4 / 100.0 / 4), rtol=1e-15)       # N_sites of group 1 in the mean volume
    assert np.isnan(s.density(1)).all() and np.isnan(s.g(1)).all()           # a frame group without a visit
    # an ideal gas: the expected count of every voxel gives g = 1
    ideal = _hand_made(np.full((1, 4, 4, 4), 40 * 50 / 100.0 * 0.125 * 1e6).astype(np.int64), [40])
    assert np.allclose(ideal.g(0) / 1e6, 1.0, rtol=1e-12)
    # the mirror images
    g = s.g(0)
    sym = s.symmetrized(0, axes=(2,))
    assert np.allclose(sym, 0.5 * (g + g[:, :, ::-1]), rtol=1e-15) and np.array_equal(sym, sym[:, :, ::-1])
    both = s.symmetrized(0, axes=(0, 2))
    assert np.allclose(both, 0.25 * (g + g[::-1] + g[:, :, ::-1] + g[::-1, :, ::-1]), rtol=1e-14)
    assert np.allclose(s.symmetrized(0, axes=(1,), quantity="counts"), 0.5 * (counts[0] + counts[0][:, ::-1]))
    # slabs
    assert np.allclose(s.plane(0, axis=2), 0.5 * (g[:, :, 1] + g[:, :, 2]), rtol=1e-15)                  # the two central layers
    assert np.allclose(s.plane(0, axis=0, lo=0.0, hi=1.0), 0.5 * (g[2] + g[3]), rtol=1e-15)
    assert np.allclose(s.plane(0, axis=1, lo=-0.3, hi=-0.2, quantity="density"), rho[:, 1, :], rtol=1e-15)
    assert s.plane(0, axis=1, lo=0.7).shape == (4, 4)
    with pytest.raises(ValueError):
        s.plane(0, axis=1, lo=0.3, hi=0.4)


def test_from_words_shapes_the_table():
    I = _I()
    H = I.H
    lay, counts = H.SdfLayout(), H.SdfCounts(5, 1, 2, 3, 0.25)
    counts.frame_visits[0], counts.frame_visits[1] = 7, 9
    lay.interval, lay.nbins, lay.num_frame_groups, lay.num_site_groups, lay.num_classes, lay.words, lay.extent = 10, 3, 2, 1, 2, 54, 0.9
    lay.num_frames[0], lay.num_frames[1], lay.num_sites[0] = 3, 4, 11
    lay.classes[1][0] = 1
    lay.pairs_per_sample[0], lay.pairs_per_sample[1] = 33, 44
    words = np.arange(54, dtype=np.int64)
    s = I.sdf_from_words(words, lay, counts)
    assert (s.samples, s.dropped, s.invalid, s.bad_frames, s.inv_volume_sum, s.interval, s.extent) == (5, 1, 2, 3, 0.25, 10, 0.9)
    assert np.array_equal(s.counts, words.reshape(2, 3, 3, 3)) and s.counts[1, 2, 0, 1] == 27 + 18 + 1      # xi1 outermost
    assert np.array_equal(s.classes, [[0, 0], [1, 0]]) and list(s.frame_visits) == [7, 9] and list(s.num_frames) == [3, 4]
    assert list(s.num_sites) == [11] and list(s.pairs_per_sample) == [33, 44]


def test_write_sdf_round_trips_through_loadtxt():
    rng = np.random.default_rng(6)
    counts = rng.integers(0, 3, size=(2, 4, 4, 4)) * rng.integers(0, 2, size=(2, 4, 4, 4))
    s = _hand_made(counts, [40, 8], classes=[(0, 0), (1, 0)], num_frames=(10, 2))
    for c in (0, 1):
        out = io.StringIO()
        R.write_sdf(out, s, c)
        text = out.getvalue()
        head = text.splitlines()[:2]
        assert head[0] == ('#"Samples"\t4\t"Dropped"\t1\t"Invalid"\t2\t"BadFrames"\t3\t"FrameVisits"\t%d\t"InvVolumeSum"\t0.04\t"Extent (nm)"\t1.0\t"Bins"\t4\t"Class"\t"%d-0"'
                           % ((40, 8)[c], c))
        assert head[1] == '#"i1"\t"i2"\t"i3"\t"xi1 (nm)"\t"xi2 (nm)"\t"xi3 (nm)"\t"count"\t"density (nm^-3)"\t"g"'
        back = np.loadtxt(io.StringIO(text)).reshape(-1, 9)
        at = np.argwhere(counts[c] != 0)
        assert len(back) == len(at) > 0 and np.array_equal(back[:, :3], at)
        again = np.zeros((4, 4, 4), dtype=np.int64)
        again[tuple(back[:, :3].astype(int).T)] = back[:, 6].astype(np.int64)
        assert np.array_equal(again, counts[c])
        assert np.array_equal(back[:, 3], s.centres[at[:, 0]]) and np.array_equal(back[:, 5], s.centres[at[:, 2]])
        assert np.array_equal(back[:, 7], s.density(c)[tuple(at.T)]) and np.array_equal(back[:, 8], s.g(c)[tuple(at.T)])
        plain = io.StringIO()
        R.write_sdf(plain, s, c, header=False)
        assert plain.getvalue() == "\n".join(text.splitlines()[2:]) + "\n"


def _read_cube(text):
    """(natoms, origin, voxel vectors [3, 3], counts per axis, atoms, data [n1, n2, n3]) of a Gaussian cube file."""
    lines = text.splitlines()
    first = lines[2].split()
    natoms, origin = int(first[0]), np.array([float(v) for v in first[1:4]])
    shape, vec = [], []
    for a in range(3):
        t = lines[3 + a].split()
        shape.append(int(t[0]))
        vec.append([float(v) for v in t[1:4]])
    atoms = [[float(v) for v in lines[6 + k].split()] for k in range(natoms)]
    data = np.array([float(v) for line in lines[6 + natoms:] for v in line.split()])
    return natoms, origin, np.array(vec), shape, atoms, data.reshape(shape)


@pytest.mark.parametrize("n", [4, 7])
def test_write_sdf_cube_round_trips(n):
    rng = np.random.default_rng(8)
    counts = rng.integers(0, 90, size=(1, n, n, n))
    s = _hand_made(counts, [40], extent=0.7)
    assert R.BOHR_NM == 0.0529177210903
    for quantity, want in (("g", s.g(0)), ("density", s.density(0)), ("counts", counts[0].astype(np.float64))):
        out = io.StringIO()
        R.write_sdf_cube(out, s, 0, quantity=quantity)
        natoms, origin, vec, shape, atoms, data = _read_cube(out.getvalue())
        assert natoms == 1 and shape == [n, n, n] and len(atoms) == 1 and atoms[0][2:] == [0.0, 0.0, 0.0]      # one atom, at the frame's origin
        step = 2 * 0.7 / n / R.BOHR_NM
        assert np.allclose(vec, np.eye(3) * step, atol=1e-6) and np.allclose(origin, (-0.7 / R.BOHR_NM + step / 2), atol=1e-6)
        assert np.allclose(origin + (n - 1) * step, -origin, atol=1e-5)      # the grid is centred on the atom
        assert np.allclose(data, want, rtol=1e-5)                     # C order, xi1 outermost: the table's own
    empty = _hand_made(counts, [0], extent=0.7)
    out = io.StringIO()
    R.write_sdf_cube(out, empty, 0)
    assert not _read_cube(out.getvalue())[5].any()                    # NaN is written as 0


# ------------------------------------------------------------------------------------------ the test hook and the digest of the host tables
def test_hook_is_known_and_checked():
    H = _I().H
    plan, keep = _plan()
    try:
        for value in (1, 2, 4096):
            assert H.lib.vvhip_debug_tune(plan, b"sdf_items_target", value) == H.OK
        for value in (0, -1):
            assert H.lib.vvhip_debug_tune(plan, b"sdf_items_target", value) == H.ERR_INVALID
    finally:
        H.lib.vvhip_plan_destroy(plan)


def test_recorder_digest_answers_for_sdf():
    H = _I().H
    H.lib.vvhip_debug_recorder_digest.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64)]
    plan, keep = _plan(box=(3.0, 3.2, 3.4))
    frames = _frames()
    try:
        def digest(name=b"sdf"):
            out = C.c_uint64(1)
            assert H.lib.vvhip_debug_recorder_digest(plan, name, C.byref(out)) == H.OK
            return out.value

        assert digest() == 0                                         # nothing described
        _describe(plan)
        first = digest()
        assert first != 0 and digest(b"rdf") == 0 and digest(b"vanhove_distinct") == 0
        _describe(plan, interval=77, extent=0.3, nbins=5, max_samples=3)
        assert digest() == first                                     # neither the interval nor the voxels are host tables
        swapped = frames.copy()
        swapped[0, 1], swapped[0, 2] = frames[0, 2], frames[0, 1]
        _describe(plan, frames=swapped)
        assert digest() not in (0, first)                            # the frames are
        _describe(plan, frames=frames[:-1])
        assert digest() not in (0, first)
        _describe(plan, exclude=1)
        assert digest() not in (0, first)                            # ... and the molecule lists of the exclusion
        assert H.lib.vvhip_debug_tune(plan, b"sdf_items_target", 1) == H.OK
        _describe(plan)
        assert digest() not in (0, first)                            # the work list follows the hook that shapes it
        assert H.lib.vvhip_sdf_stop(plan) == H.OK and digest() == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)
