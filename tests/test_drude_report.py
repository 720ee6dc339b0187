"""Drude temperature report, host side (no GPU): the report's DOFs (vvhip_drude_report_dof) against a NumPy restatement of the example
reporter's counting, the joining of its fixed-point sums (vvhip_drude_report_combine), and the reporter class."""
import dataclasses
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("openmm-velocityverlet_amd")
S = pkg.systems
R = pkg.reporters


def _I():
    return importlib.import_module("openmm-velocityverlet_amd.integrator")


def reference_dof(spec):
    """examples/ommhelper/reporter/drudetemperaturereporter.py:67-84 in NumPy: COM 3 n_M (- 3 with a CMMotionRemover), atomic
    3 n_m - 3 n_M - n_c - 3 n_p, Drude 3 n_p."""
    m = np.asarray(spec.masses, dtype=np.float64)
    M = np.bincount(spec.mol_id, weights=m, minlength=spec.num_molecules)
    n_M, n_m = np.count_nonzero(M), np.count_nonzero(m > 0)
    n_p, n_c = len(spec.drude_pairs), len(spec.constraints)
    return (3.0 * n_M - (3.0 if spec.has_cm_motion_remover else 0.0), 3.0 * n_m - 3.0 * n_M - n_c - 3.0 * n_p, 3.0 * n_p)


def _integrator(cfg="C3", com=None):
    I = _I()
    it = I.VVIntegrator(300.0 if cfg == "C2" else 333.0, 10.0, 1.0, 40.0, 0.001)
    if com is not None:
        it.setUseCOMTempGroup(com)
    return it


def _systems():
    out = [(c, S.make_config(c)) for c in ("C1", "C2", "C3", "C4", "C5")]
    out.append(("C3+HBonds", S.make_config("C3", hbonds=True)))
    out.append(("C2 rigid", S.make_config("C2", hbonds=True)))
    out.append(("C3 AllBonds", S.constrain_all_bonds(S.make_config("C3", scale=0.05))))
    out.append(("C3 random constraints", S.add_random_constraints(S.make_config("C3", scale=0.05), np.random.default_rng(5))))
    out.append(("C3 sites", S.add_virtual_sites(S.make_config("C3", scale=0.05))))
    return out


SYSTEMS = _systems()


@pytest.mark.parametrize("name,spec", SYSTEMS, ids=[n for n, _ in SYSTEMS])
@pytest.mark.parametrize("cmm", [True, False])
def test_report_dof_matches_the_example_reporter(name, spec, cmm):
    I = _I()
    spec = dataclasses.replace(spec, has_cm_motion_remover=cmm)
    cfg = name.split()[0].split("+")[0]
    want = reference_dof(spec)
    for com in (None, False):                 # the DOFs depend on neither the COM temperature group nor the thermostats
        got = I.drude_report_dof(spec, _integrator(cfg, com))
        assert got == pytest.approx(want, abs=0), (name, com, got, want)


@pytest.mark.parametrize("cfg", ["C1", "C2", "C3"])
@pytest.mark.parametrize("world", [2, 4])
def test_report_dof_of_a_shard_is_the_whole_systems(cfg, world):
    I = _I()
    D = importlib.import_module("openmm-velocityverlet_amd.distributed")
    spec = S.make_config(cfg)
    want = reference_dof(spec)
    for b, e in D.shard_bounds(spec, world):
        assert I.drude_report_dof(spec, _integrator(cfg), shard=(b, e)) == pytest.approx(want, abs=0)


def test_report_combine_joins_the_fixed_point_words():
    """raw = 2KE sums as (hi, lo) word pairs: total, Drude, COM.  KE_Atom = total - COM - Drude, the lo words carry into hi."""
    I = _I()
    H = I.H
    import ctypes as C
    spec = S.make_config("C3", scale=0.05)
    plan, _, _ = I.create_plan(spec, _integrator())
    try:
        dof = (C.c_double * 3)()
        H.check(H.lib.vvhip_drude_report_dof(plan, C.byref(dof)), plan)
        # find the scales: one unit of hi, one unit of lo in the COM words
        ke, t = (C.c_double * 3)(), (C.c_double * 3)()
        unit = []
        for raw in ((C.c_int64 * 6)(0, 0, 0, 0, 1, 0), (C.c_int64 * 6)(0, 0, 0, 0, 0, 1)):
            H.check(H.lib.vvhip_drude_report_combine(plan, C.byref(raw), C.byref(ke), C.byref(t)), plan)
            unit.append(-int(np.log2(2 * ke[0])))
            assert 2.0 ** -unit[-1] == 2 * ke[0]
        U, F = unit[0], unit[1] - unit[0]
        assert 0 <= U <= 20 and 36 <= F <= 60
        one, u = 1 << F, 1 << U
        # total 103.5, Drude 7.25 and COM 20.25 each with one hi unit in their lo words: KE_Atom's lo word is -2 hi units (a negative carry)
        raw = (C.c_int64 * 6)(103 * u + u // 2, 0, 7 * u + u // 4 - 1, one, 20 * u + u // 4 - 1, one)
        H.check(H.lib.vvhip_drude_report_combine(plan, C.byref(raw), C.byref(ke), C.byref(t)), plan)
        assert list(ke) == [10.125, 38.0, 3.625]
        Rgas = 8.31446261815324e-3
        assert list(t) == [2 * k / (d * Rgas) if d > 0 else 0.0 for k, d in zip(ke, dof)]
    finally:
        H.lib.vvhip_plan_destroy(plan)


def test_report_of_an_unbound_integrator_raises():
    I = _I()
    it = _integrator()
    with pytest.raises(I.H.VVHipError, match="not bound"):
        it.getDrudeTemperatures()


# ------------------------------------------------------------------------------------------ the reporter class
class _FakeIntegrator:
    def __init__(self):
        self.calls = 0

    def getDrudeTemperatures(self):
        self.calls += 1
        k = float(self.calls)
        return (1.5 * k, 2.5 * k, 0.125 * k, 300.0 + k, 333.25 + k, 1.0 / k)


class _FakeSimulation:
    def __init__(self):
        self.integrator = _FakeIntegrator()
        self.currentStep = 0


def test_reporter_writes_the_example_reporters_header_and_columns(tmp_path):
    path = tmp_path / "T_drude.txt"
    sim = _FakeSimulation()
    rep = R.DrudeTemperatureReporter(str(path), 1000)
    assert rep.describeNextReport(sim) == (1000, False, False, False, False)      # asks OpenMM for no velocities
    sim.currentStep = 250
    assert rep.describeNextReport(sim)[0] == 750
    for step in (1000, 2000):
        sim.currentStep = step
        rep.report(sim, None)
    rep.close()
    lines = path.read_text().splitlines()
    assert lines[0] == '#"Step"\t"T_COM"\t"T_Atom"\t"T_Drude"\t"KE_COM"\t"KE_Atom"\t"KE_Drude"'
    assert lines[1].split("\t") == ["1000", "301.0", "334.25", "1.0", "1.5", "2.5", "0.125"]
    assert lines[2].split("\t") == ["2000", "302.0", "335.25", "0.5", "3.0", "5.0", "0.25"]
    # what analysis scripts of the example reporter's files do
    data = np.loadtxt(str(path))
    assert data.shape == (2, 7) and data[1, 0] == 2000
    assert sim.integrator.calls == 2


def test_reporter_appends_when_asked(tmp_path):
    path = tmp_path / "T_drude.txt"
    path.write_text("earlier run\n")
    sim = _FakeSimulation()
    sim.currentStep = 10
    rep = R.DrudeTemperatureReporter(str(path), 10, append=True)
    rep.report(sim, None)
    rep.close()
    lines = path.read_text().splitlines()
    assert lines[0] == "earlier run" and lines[1].startswith('#"Step"') and lines[2].startswith("10\t")
    rep = R.DrudeTemperatureReporter(str(path), 10)                   # append=False starts the file afresh
    rep.close()
    assert path.read_text() == ""
