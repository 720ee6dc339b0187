"""Maxwell-Boltzmann start velocities on the device (include/vvhip.h: vvhip_set_velocities_to_temperature), host side (no GPU): the
reference's Philox against known answers, the export, the record's layout against the header as a C compiler sees it, the refusals that
need no device, and the statistical bounds of tests/test_gpu_thermalize.py met by the NumPy statement on the same systems and seeds."""
import ctypes as C
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import thermalize_cases as K            # noqa: E402
import thermalize_reference as ref      # noqa: E402

FIELDS = ("drawn", "pairs_split", "zeroed", "constrained", "cm_removed", "v_removed")


def _I():
    return importlib.import_module("openmm-velocityverlet_amd.integrator")


KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = ref.philox4x32_10(counter, key)
    assert " ".join("%08x" % int(w[0]) for w in got) == want


def test_philox_is_elementwise():
    """An array of counters gives what the counters give one by one (the reference draws all particles at once)."""
    g = np.array([0, 1, 63, 64, 2 ** 31, 2 ** 32 - 1], dtype=np.uint64)
    z = np.zeros_like(g)
    all_at_once = ref.philox4x32_10((g, z, z, z + np.uint64(ref.TAG)), (7, 9))
    for j, gj in enumerate(g):
        one = ref.philox4x32_10((int(gj), 0, 0, ref.TAG), (7, 9))
        assert [int(w[j]) for w in all_at_once] == [int(w[0]) for w in one]


def test_entry_point_is_exported():
    H = _I().H
    assert "vvhip_set_velocities_to_temperature" in H.EXPORTS


def test_record_layout_and_flags_match_the_header(tmp_path):
    """sizeof and every field offset of vvhip_thermalize_record and the two flag values, printed by a C program built from include/vvhip.h."""
    H = _I().H
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler (the build needs one as well)"
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vvhip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(vvhip_thermalize_record));\n'
                   + "".join(f'    printf(" %zu", offsetof(vvhip_thermalize_record, {f}));\n' for f in FIELDS)
                   + '    printf(" %d %d", VVHIP_THERMALIZE_NO_CONSTRAINTS, VVHIP_THERMALIZE_REMOVE_CM);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(H.ThermalizeRecord) == 56
    assert got[1:7] == [getattr(H.ThermalizeRecord, f).offset for f in FIELDS] == [0, 8, 16, 24, 28, 32]
    assert got[7:] == [H.THERMALIZE_NO_CONSTRAINTS, H.THERMALIZE_REMOVE_CM] == [1, 2]


def _plan(spec, shard=None):
    I = _I()
    it = I.VVIntegrator(K.T, 10.0, K.T_DRUDE, 40.0, 0.001)
    plan, _, keep = I.create_plan(spec, it, "mixed", shard)
    return plan, keep


def test_refusals_that_need_no_device():
    """A negative or non-finite temperature, a NaN Drude temperature and unknown flags before anything else; REMOVE_CM on a sharded plan
    with the removal's own error; then the unbound plan."""
    H = _I().H
    spec = K.il()
    plan, _ = _plan(spec)
    call = H.lib.vvhip_set_velocities_to_temperature
    try:
        for bad in (-1.0, float("nan"), float("inf")):
            assert call(plan, bad, -1.0, 1, 0, None) == H.ERR_INVALID
            assert "temperature" in H.lib.vvhip_last_error(plan).decode()
        assert call(plan, 300.0, float("nan"), 1, 0, None) == H.ERR_INVALID
        assert call(plan, 300.0, -1.0, 1, 4, None) == H.ERR_INVALID and "flag" in H.lib.vvhip_last_error(plan).decode()
        assert call(plan, 300.0, -1.0, 1, 0, None) == H.ERR_INVALID and "vvhip_bind" in H.lib.vvhip_last_error(plan).decode()
        assert call(None, 300.0, -1.0, 1, 0, None) == H.ERR_INVALID
    finally:
        H.lib.vvhip_plan_destroy(plan)
    mol = np.asarray(spec.mol_id)
    cut = int(np.nonzero(mol == mol[spec.num_atoms // 2])[0].min())
    plan, _ = _plan(spec, shard=(0, cut))
    try:
        assert call(plan, 300.0, -1.0, 1, H.THERMALIZE_REMOVE_CM, None) == H.ERR_UNSUPPORTED
        assert "shard" in H.lib.vvhip_last_error(plan).decode()
        assert call(plan, 300.0, -1.0, 1, 0, None) == H.ERR_INVALID and "vvhip_bind" in H.lib.vvhip_last_error(plan).decode()
    finally:
        H.lib.vvhip_plan_destroy(plan)


def test_normals_are_standard():
    """Mean, variance and the three cross moments of n(g) over 2^18 particles within five standard deviations, for both seeds."""
    for seed in K.SEEDS:
        n = ref.normals(np.arange(1 << 18), seed)
        N = n.shape[0]
        assert np.isfinite(n).all() and np.abs(n).max() <= 6.7            # sqrt(-2 ln 2^-32) = 6.66
        assert np.abs(n.mean(0)).max() <= 5 / np.sqrt(N)
        assert np.abs((n ** 2).mean(0) - 1).max() <= 5 * np.sqrt(2.0 / N)
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert abs(np.mean(n[:, a] * n[:, b])) <= 5 / np.sqrt(N)


@pytest.mark.parametrize("name", K.STATISTICS)
@pytest.mark.parametrize("seed", K.SEEDS)
def test_the_statement_meets_the_statistical_bounds_of_the_gpu_tests(name, seed):
    """Bounds 3 and 4 of tests/test_gpu_thermalize.py on the reference alone, with the very systems and seeds: conditions the statement
    meets, not hopes."""
    spec = K.SYSTEMS[name]()
    m = np.asarray(spec.masses, dtype=np.float64)
    massive = m > 0
    v = ref.velocities(m, spec.drude_pairs, K.T, seed)
    assert np.all(v[~massive] == 0)
    t = ref.plain_temperature(m, v)
    print(f"{name} seed {seed:#x}: plain T = {t:.3f} K, bound {K.plain_bound(m) * K.T:.3f} K")
    assert abs(t / K.T - 1) <= K.plain_bound(m)
    other = ref.velocities(m, spec.drude_pairs, K.T, seed + 1)
    assert abs(ref.correlation(v[massive] / np.sqrt(ref.R * K.T / m[massive])[:, None],
                               other[massive] / np.sqrt(ref.R * K.T / m[massive])[:, None])) < 5 / np.sqrt(3 * np.count_nonzero(massive))
    if seed == K.SEEDS[0]:                                         # the pair of seeds tests/test_gpu_thermalize.py::test_seeds compares as well
        second = ref.velocities(m, spec.drude_pairs, K.T, K.SEEDS[1])
        assert abs(ref.correlation(v[massive] / np.sqrt(ref.R * K.T / m[massive])[:, None],
                                   second[massive] / np.sqrt(ref.R * K.T / m[massive])[:, None])) < 5 / np.sqrt(3 * np.count_nonzero(massive))
    if name in K.DRUDE:
        pairs = ref.split_pairs(m, spec.drude_pairs)
        vd = ref.velocities(m, spec.drude_pairs, K.T, seed, K.T_DRUDE)
        td = ref.drude_temperature(m, spec.drude_pairs, vd)
        mean, five_sd = K.total_2ke(int(np.count_nonzero(massive)), len(pairs), ref.R)
        print(f"{name} seed {seed:#x}: T_Drude = {td:.4f} K, bound {K.drude_bound(len(pairs)) * K.T_DRUDE:.4f} K; 2KE = {ref.two_ke(m, vd):.2f}, expected {mean:.2f} +- {five_sd:.2f}")
        assert len(pairs) > 300
        assert abs(td / K.T_DRUDE - 1) <= K.drude_bound(len(pairs))
        assert abs(ref.two_ke(m, vd) - mean) <= five_sd
        # outside the pairs the two modes are the same draw
        unpaired = np.ones(m.size, bool)
        unpaired[pairs.ravel()] = False
        assert np.array_equal(v[unpaired], vd[unpaired])


def test_the_cases_have_what_the_gpu_tests_need():
    """More than 8 waves, a partly idle last wave, Drude pairs, massless particles without a lane and a Langevin subset."""
    I = _I()
    for name, make in K.SYSTEMS.items():
        spec = make()
        it = I.VVIntegrator(K.T, 10.0, K.T_DRUDE, 40.0, 0.001)
        info, slots = I.plan_layout(spec, it)
        assert info.num_waves > 8, (name, info.num_waves)
        assert np.count_nonzero(slots[-64:, 0] < 0) > 0, name
    edl = K.edl()
    assert len(edl.particles_ld) > 0 and len(edl.image_pairs) > 0 and np.count_nonzero(np.asarray(edl.masses) == 0) == len(edl.image_pairs)
    info, slots = I.plan_layout(edl, I.VVIntegrator(K.T, 10.0, K.T_DRUDE, 40.0, 0.001))
    assert info.num_slots_used < edl.num_atoms                     # the images have no lane
