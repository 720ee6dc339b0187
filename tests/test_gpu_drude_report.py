"""Drude temperature report on the GPU (vvhip_drude_temperatures): the six numbers against a float64 NumPy restatement of
examples/ommhelper/reporter/drudetemperaturereporter.py on the downloaded velocities, bit reproducibility, no effect on the run, the
sharded all-reduce."""
import dataclasses
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("openmm-velocityverlet_amd")
S, I = pkg.systems, pkg.integrator
H = I.H

pytestmark = pytest.mark.gpu

RGAS = 8.31446261815324e-3


def reference_report(spec, v):
    """The example reporter's arithmetic in float64 (molecule COM velocities, velocities relative to them, each pair's core replaced by
    the pair's centre of mass): (KE_COM, KE_Atom, KE_Drude, T_COM, T_Atom, T_Drude)."""
    m = np.asarray(spec.masses, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    mol, nmol = np.asarray(spec.mol_id), spec.num_molecules
    M = np.bincount(mol, weights=m, minlength=nmol)
    P = np.stack([np.bincount(mol, weights=m * v[:, k], minlength=nmol) for k in range(3)], 1)
    V = np.zeros_like(P)
    V[M > 0] = P[M > 0] / M[M > 0, None]
    ke_com = 0.5 * (M * (V ** 2).sum(1)).sum()
    u = v - V[mol]
    mm = m.copy()
    pairs = np.asarray(spec.drude_pairs, dtype=np.int64).reshape(-1, 2)
    is_drude = np.zeros(len(m), dtype=bool)
    if len(pairs):
        d, c = pairs[:, 0], pairs[:, 1]
        mt = m[d] + m[c]
        mu = np.where((m[d] > 0) & (m[c] > 0), m[d] * m[c] / np.where(mt > 0, mt, 1), 0.0)
        rel = u[d] - u[c]
        com = (m[d, None] * u[d] + m[c, None] * u[c]) / np.where(mt > 0, mt, 1)[:, None]
        u[d], u[c] = rel, com
        mm[d], mm[c] = mu, mt
        is_drude[d] = True
    mvv = mm * (u ** 2).sum(1)
    ke_atom = 0.5 * mvv[~is_drude].sum()
    ke_drude = 0.5 * mvv[is_drude].sum()
    n_M, n_m, n_p, n_c = np.count_nonzero(M), np.count_nonzero(m > 0), len(pairs), len(spec.constraints)
    dof = (3 * n_M - (3 if spec.has_cm_motion_remover else 0), 3 * n_m - 3 * n_M - n_c - 3 * n_p, 3 * n_p)
    ke = (ke_com, ke_atom, ke_drude)
    return ke + tuple(2 * k / (d * RGAS) if d > 0 else 0.0 for k, d in zip(ke, dof))


def integrator_for(cfg, spec, middle=True):
    it = I.VVIntegrator(300.0 if cfg == "C2" else 333.0, 10.0, 1.0, 40.0, 0.002 if cfg == "C2" else 0.001, 3, 1)
    if cfg not in ("C1", "C2"):
        it.setMaxDrudeDistance(0.02)
    if cfg == "C4":
        it.setCosAcceleration(0.02)
    if cfg == "C5":
        lz = float(spec.box[2])
        it.setMirrorLocation(lz / 2)
        it.setElectricField(2.0 / lz * 2 * 1.602176634e-22)
    it.setUseMiddleScheme(middle)
    return it


def assert_matches(got, want, rel=1e-10, what=""):
    scale = max(abs(x) for x in want[:3])
    for k, (g, w) in enumerate(zip(got, want)):
        tol = rel * abs(w) + (1e-14 * scale if k < 3 else 0.0)
        assert abs(g - w) <= tol, (what, k, g, w, abs(g - w) / max(abs(w), 1e-300))


def report_after(spec, cfg, precision="mixed", steps=50, com=None, **ctx_kw):
    it = integrator_for(cfg, spec)
    if com is not None:
        it.setUseCOMTempGroup(com)
    ctx = I.Context(spec, it, precision=precision, force_provider="tether", **ctx_kw)
    try:
        it.step(steps)
        got = it.getDrudeTemperatures()
        v = ctx.getVelm()[:, :3].astype(np.float64)
        return got, v
    finally:
        ctx.close()


@pytest.mark.parametrize("precision", ["mixed", "double", "single"])
@pytest.mark.parametrize("cfg", ["C1", "C2", "C3", "C4", "C5"])
def test_report_matches_numpy_full_size(cfg, precision):
    spec = S.make_config(cfg)
    got, v = report_after(spec, cfg, precision)
    want = reference_report(spec, v)
    assert_matches(got, want, what=(cfg, precision))
    assert all(np.isfinite(got)) and got[3] > 0 and got[4] > 0
    if cfg in ("C1", "C2"):
        assert got[2] == 0.0 and got[5] == 0.0          # no Drude pairs: T_Drude = 0 (the example reporter fails there)
    else:
        assert got[5] > 0


def _big_molecules(spec, merge=4):
    """Consecutive molecules merged in groups of `merge`: C3's cations of 27 particles become molecules of > 64 lanes."""
    return dataclasses.replace(spec, mol_id=(np.asarray(spec.mol_id) // merge).astype(np.int32))


def _cross_molecule_pairs(spec, every=7):
    """Every `every`-th Drude particle moved into a molecule of its own: pairs across two molecules (taken literally)."""
    mol = np.asarray(spec.mol_id).copy()
    nxt = spec.num_molecules
    for d, _ in np.asarray(spec.drude_pairs)[::every]:
        mol[d] = nxt
        nxt += 1
    return dataclasses.replace(spec, mol_id=mol.astype(np.int32))


LAYOUTS = {
    "C3 COM group off": (lambda: S.make_config("C3", scale=0.1), "C3", False),
    "C5 COM group off": (lambda: S.make_config("C5"), "C5", False),
    "C3 molecules of > 64 lanes": (lambda: _big_molecules(S.make_config("C3", scale=0.1)), "C3", None),
    "C3 molecules of > 64 lanes, COM off": (lambda: _big_molecules(S.make_config("C3", scale=0.1)), "C3", False),
    "C3 pairs across molecules": (lambda: _cross_molecule_pairs(S.make_config("C3", scale=0.1)), "C3", False),
    "C3 + HBonds": (lambda: S.make_config("C3", hbonds=True), "C3", None),
    "C2 rigid water": (lambda: S.make_config("C2", hbonds=True), "C2", None),
    "C3 virtual sites": (lambda: S.add_virtual_sites(S.make_config("C3", scale=0.1)), "C3", None),
    "random constraints, Drude liquid": (lambda: S.add_random_constraints(S.drude_il(cells=(1, 1, 1), pairs_per_cell=12, seed=4001),
                                                                           np.random.default_rng(4001)), "C3", None),
    "random constraints, water": (lambda: S.add_random_constraints(S.spce_water(40, seed=4000), np.random.default_rng(4000)), "C2", None),
    "C3 random sites": (lambda: S.add_random_virtual_sites(S.make_config("C3", scale=0.05), np.random.default_rng(4)), "C3", None),
    "ragged 37 pairs": (lambda: S.drude_il(cells=(1, 1, 1), pairs_per_cell=37, seed=9), "C3", None),
    "ragged 1 pair": (lambda: S.drude_il(cells=(1, 1, 1), pairs_per_cell=1, seed=9), "C3", None),
    "ragged water 5": (lambda: S.spce_water(5), "C2", None),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("precision", ["mixed", "single"])
def test_report_matches_numpy_on_other_layouts(name, precision):
    make, cfg, com = LAYOUTS[name]
    spec = make()
    got, v = report_after(spec, cfg, precision, steps=20, com=com)
    assert_matches(got, reference_report(spec, v), what=(name, precision))


def test_report_bits_do_not_depend_on_calls_or_launch_shape():
    spec = S.make_config("C3")
    it = integrator_for("C3", spec)
    ctx = I.Context(spec, it, precision="mixed", force_provider="tether")
    try:
        it.step(20)
        first = ctx.drude_report_raw()
        six = ctx.getDrudeTemperatures()
        for _ in range(3):
            assert np.array_equal(ctx.drude_report_raw(), first)
            assert ctx.getDrudeTemperatures() == six
        for key, value in (("block_threads", 64), ("grid_cap_a", 3), ("block_threads", 448)):
            H.check(H.lib.vvhip_debug_tune(ctx.plan, key.encode(), value), ctx.plan)
            assert np.array_equal(ctx.drude_report_raw(), first), key
            assert ctx.getDrudeTemperatures() == six
    finally:
        ctx.close()


def _probe(ctx):
    return bytes(memoryview(ctx.getNHState())), ctx.status_words(), ctx.fused_status()


def _run(spec, cfg, middle, steps, report, graph_chunk=None):
    """The run with (report=True) or without a report after every step / graph chunk; both take the same probes of the NH state, the
    status words and fused_status() at the same points, and the report run checks that a report leaves all three as they were."""
    it = integrator_for(cfg, spec, middle)
    ctx = I.Context(spec, it, precision="mixed", force_provider="tether")
    try:
        reports = []
        chunk = graph_chunk or 1
        for _ in range(steps // chunk):
            if graph_chunk is None:
                it.step(1)
            else:
                ctx.run_graph(graph_chunk, graph_chunk)
            before = _probe(ctx)
            if report:
                reports.append(it.getDrudeTemperatures())
                assert _probe(ctx) == before
        ctx.synchronize()
        return ctx.getVelm(), ctx.getPosq(), ctx.getPosqCorrection(), _probe(ctx), reports
    finally:
        ctx.close()


@pytest.mark.parametrize("middle", [True, False], ids=["middle", "classic"])
def test_reports_do_not_disturb_the_run(middle):
    spec = S.make_config("C3")
    a = _run(spec, "C3", middle, 200, report=False)
    b = _run(spec, "C3", middle, 200, report=True)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert a[3] == b[3] and a[3][1] == [0, 0, 0, 0]
    assert len(b[4]) == 200 and all(r[4] > 0 for r in b[4])


def test_reports_between_graph_replays_do_not_disturb_the_run():
    spec = S.make_config("C3")
    a = _run(spec, "C3", True, 200, report=False, graph_chunk=50)
    b = _run(spec, "C3", True, 200, report=True, graph_chunk=50)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert a[3] == b[3] and a[3][1] == [0, 0, 0, 0]
    assert len(b[4]) == 4


def test_sharded_report_equals_single_process_two_ranks_one_gpu():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29561", os.path.join(ROOT, "tests", "drude_report_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "DRUDE REPORT DIST OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


REPORT_DRIVER = os.path.join(ROOT, "lib", "vv_report_driver")


def _read_dump(path):
    out, raw = [], open(path, "rb").read()
    off = 0
    for dt in (np.float64, np.int32, np.int32, np.int32, np.float64):
        n = int(np.frombuffer(raw, dtype=np.int64, count=1, offset=off)[0])
        off += 8
        out.append(np.frombuffer(raw, dtype=dt, count=n, offset=off).copy())
        off += n * np.dtype(dt).itemsize
    return out


def test_cpp_report_through_the_plugin_equals_python_bit_for_bit(tmp_path):
    """VVIntegrator::getDrudeTemperatures() on the HIP plugin (its kernel created on the first call) against Context.getDrudeTemperatures
    of the stand-alone host on the same velocities: the same six doubles."""
    dump = str(tmp_path / "report.bin")
    r = subprocess.run([REPORT_DRIVER, dump, "30"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "REPORT OK" in r.stdout, r.stdout + r.stderr
    got = tuple(float.fromhex(x) for x in next(ln for ln in r.stdout.splitlines() if ln.startswith("REPORT ")).split()[1:])
    masses, mol, pairs, cons, velm = _read_dump(dump)
    n = masses.shape[0]
    v = velm.reshape(n, 4)[:, :3]
    spec = S.SystemSpec(name="cpp driver", masses=masses, charges=np.zeros(n), positions=np.zeros((n, 3)), velocities=v.copy(),
                        box=np.array([3.0, 3.0, 3.0]), mol_id=mol, drude_pairs=pairs.reshape(-1, 2), constraints=cons.reshape(-1, 2),
                        has_cm_motion_remover=True)
    it = I.VVIntegrator(333.0, 10.0, 1.0, 40.0, 0.001)
    ctx = I.Context(spec, it, precision="mixed", force_provider="static")
    try:
        assert np.array_equal(ctx.getVelm()[:, :3], v)
        want = it.getDrudeTemperatures()
    finally:
        ctx.close()
    assert got == want, (got, want)
    assert_matches(got, reference_report(spec, v))
