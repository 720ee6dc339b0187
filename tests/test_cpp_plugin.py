"""The C++ layers a real OpenMM would load: libOpenMMVelocityVerlet (VVIntegrator) and the HIP kernel-factory plugin,
driven by tests/cpp/plugin_driver.cpp through OpenMM-shaped stand-ins (compat/).  CPU tests cover registration, names,
error behaviour, exported plugin symbols and the host chain routine; the GPU test runs VVIntegrator::step() through the
plugin (fused and un-fused call sequences, both schemes) and compares with the oracle on the same dumped system."""
import ctypes
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "lib", "vv_plugin_driver")
PLUGIN = os.path.join(ROOT, "lib", "plugins", "libVelocityVerletPluginHIP.so")
systems = importlib.import_module("openmm-velocityverlet_amd.systems")


def test_plugin_exports_openmm_entry_points():
    lib = ctypes.CDLL(PLUGIN)
    for name in ("registerPlatforms", "registerKernelFactories", "registerHipVVKernelFactories"):
        assert hasattr(lib, name), name          # CudaVVKernelFactory.cpp:37,40,57 with Hip for Cuda


def test_registration_names_and_errors():
    out = subprocess.run([DRIVER, "registry"], capture_output=True, text=True, check=True).stdout
    assert "REGISTRY OK" in out
    for name in ("IntegrateMiddleStep", "IntegrateVVStep", "ModifyDrudeNose", "ModifyLangevin", "ModifyImageCharge",
                 "ModifyElectricField", "ModifyCosineAccelerate"):                       # VVKernels.h:50-248
        assert f"kernel {name}: registered" in out
    assert "This Integrator is not bound to a context!" in out                          # VVIntegrator.cpp:224-225


def test_host_chain_equals_oracle_chain_bitwise():
    vals = [float(x) for x in subprocess.run([DRIVER, "chain"], capture_output=True, text=True, check=True).stdout.split()]
    eta, ed, edd = np.array([0.01, -0.02, 0.03]), np.array([0.5, -1.5, 2.5, 0.0]), np.array([0.1, 0.2, 0.3])
    mass = np.array([4500.0, 0.0277, 0.0277])
    f = O.propagate_nh_chain(eta, ed, edd, mass, 460000.0, 457000.0, 333.0, 0.001, loops_per_step=2)
    assert vals == [f] + eta.tolist() + ed.tolist() + edd.tolist()


def _read(path):
    raw = open(path, "rb").read()
    off = 0
    out = []
    for dt in ("f8", "f8", "i4", "i4", "i4", "f8", "f8", "f8", "f4", "f4", "f8", "f8", "i4", "i4", "i4", "f4", "i4", "f8"):
        if off >= len(raw):
            break
        (n,) = struct.unpack_from("<q", raw, off)
        off += 8
        a = np.frombuffer(raw, dtype=dt, count=n, offset=off).copy()
        off += a.nbytes
        out.append(a)
    return out


def _oracle_for(arrays, middle, cons, cos, nsteps):
    """The oracle stepped on the system the C++ driver dumped (cons == 3: wall atoms with Langevin thermostat, image particles, field)."""
    masses, charges, mol, pairs, cns, pos, vel = arrays[:7]
    cdist = arrays[11]
    n = masses.shape[0]
    spec = systems.SystemSpec(name="cpp", masses=masses, charges=charges, positions=pos.reshape(n, 3), velocities=vel.reshape(n, 3),
                              box=np.array([3.0, 3.0, 3.0]), mol_id=mol, drude_pairs=pairs.reshape(-1, 2),
                              constraints=cns.reshape(-1, 2), has_cm_motion_remover=cons != 3)
    if cons in (2, 4):  # hydrogen-type / general clusters: solved in the fused kernels, and by the oracle (cons == 1: see the driver)
        spec.constraint_distances = cdist
    if cons == 5:       # virtual sites: placed by kernel B, and by the oracle's statement of OpenMM's definitions
        vs, vp = arrays[16].reshape(-1, 5), arrays[17].reshape(-1, 12)
        spec.virtual_sites = [(int(r[0]), int(r[1]), tuple(int(q) for q in r[2:5]), tuple(w)) for r, w in zip(vs, vp)]
    p = O.Params(temperature=333.0, drude_temperature=1.0, max_drude_distance=0.02, cos_acceleration=cos, use_middle_scheme=bool(middle))
    rnd = None
    if cons == 3:
        ld, img, el, normals = arrays[12:16]
        spec.particles_ld = [int(i) for i in ld]
        spec.image_pairs = [(int(a), int(b)) for a, b in img.reshape(-1, 2)]
        spec.particles_electrolyte = [int(i) for i in el]
        p.mirror_location, p.electric_field = 3.5, 2.0 / 3.0 * 1.602176634e-22
        rnd = normals.reshape(-1, 4)
    osys = O.OracleSystem(spec, p, "mixed", random=rnd, force_mode=1)
    osys.step(nsteps)
    return osys


@pytest.mark.gpu
@pytest.mark.parametrize("middle,cons,cos", [(1, 0, 0.0), (1, 1, 0.0), (1, 0, 0.02), (1, 1, 0.02), (0, 0, 0.0), (0, 1, 0.02),
                                             (1, 2, 0.0), (1, 2, 0.02), (0, 2, 0.0), (1, 3, 0.0), (0, 3, 0.0), (1, 4, 0.0), (0, 4, 0.02),
                                             (1, 5, 0.0), (0, 5, 0.02)])
def test_cpp_integrator_through_plugin_matches_oracle(tmp_path, middle, cons, cos):
    nsteps = 12
    dump = str(tmp_path / "run.bin")
    r = subprocess.run([DRIVER, "run", dump, str(middle), str(cons), str(cos), str(nsteps)], capture_output=True, text=True)
    assert r.returncode == 0 and "RUN OK" in r.stdout, r.stdout + r.stderr
    assert f"stepCount={nsteps}" in r.stdout
    # the adapters use the context services the way the reference's CUDA kernels do (platforms/cuda/src/CudaVVKernels.cpp):
    # ContextSelector in every initialize() (:60, 246, 468, ...), initializeContexts + initRandomNumberGenerator once (:61-63), the step
    # size announced once (setNextStepSize, :136-141; the classic kernel uploads (0, dt) itself, :307-319), virtual sites recomputed
    # and atoms reordered after every position update, also on the fused path (:214-216, 374-381)
    import re
    sv = dict(re.findall(r"(\w+)=(\([^)]*\)|\S+)", next(ln for ln in r.stdout.splitlines() if ln.startswith("SERVICES"))))
    nkern = 2 + (1 if cos else 0) + (3 if cons == 3 else 0)      # step kernel + Nose-Hoover (+ cos; + Langevin, image, field) initialize() calls
    assert int(sv["selector"]) == nkern and int(sv["depth"]) == 0 and int(sv["initializeContexts"]) == 1 and int(sv["initRandom"]) == 1
    assert int(sv["setNextStepSize"]) == (1 if middle else 0)
    assert sv["stepSize"] == "(0,0.001)"
    # (cons == 5: the System's virtual sites are described to the plan and placed by kernel B; OpenMM's kernel is not launched)
    assert int(sv["virtualSites"]) == (0 if cons == 5 else nsteps) and int(sv["reorder"]) == nsteps
    assert int(sv["setAsCurrent"]) >= nsteps
    if cons == 1:                                        # constraints the kernels cannot fuse: OpenMM's solver runs between the stages
        assert int(sv["applyConstraints"]) == nsteps and int(sv["applyVelocityConstraints"]) == nsteps
    else:
        assert int(sv["applyConstraints"]) == 0 and int(sv["applyVelocityConstraints"]) == 0
    arrays = _read(dump)
    masses, charges, mol, pairs, cns, pos, vel, velm, posq, corr, vis, cdist = arrays[:12]
    n = masses.shape[0]
    osys = _oracle_for(arrays, middle, cons, cos, nsteps)
    x_g = posq.reshape(n, 4)[:, :3].astype(np.float64) + corr.reshape(n, 4)[:, :3].astype(np.float64)
    v_g = velm.reshape(n, 4)[:, :3]
    massive = masses != 0
    ex = np.abs(x_g - osys.positions()).max() / np.abs(osys.positions()).max()
    ev = np.abs(v_g[massive] - osys.velm[massive, :3]).max() / np.abs(osys.velm[massive, :3]).max()
    assert ex < 1e-5 and ev < 1e-5, (ex, ev)
    if cos != 0:
        assert vis[0] == pytest.approx(osys.viscosity()[0], rel=1e-6, abs=1e-12)
    if cons in (2, 4):
        c = cns.reshape(-1, 2)
        r = np.linalg.norm(x_g[c[:, 0]] - x_g[c[:, 1]], axis=1)
        assert np.abs(r * r - cdist ** 2).max() < 2e-5 * cdist.max() ** 2, np.abs(r - cdist).max()


REF_DRIVER = os.path.join(ROOT, "oracle", "_ref", "refplugin", "vv_plugin_driver")


@pytest.mark.skipif(not os.path.exists(REF_DRIVER), reason="oracle/_ref/refplugin not built (reference sources absent)")
def test_plugin_registers_under_the_reference_api():
    """The HIP plugin compiled against the REFERENCE's own openmmapi headers, next to the reference's own VVIntegrator.cpp compiled in
    place (oracle/Makefile: refplugin): same seven kernel names, same error texts -- from the reference's code this time."""
    out = subprocess.run([REF_DRIVER, "registry"], capture_output=True, text=True, check=True).stdout
    assert "REGISTRY OK" in out and "This Integrator is not bound to a context!" in out
    for name in ("IntegrateMiddleStep", "IntegrateVVStep", "ModifyDrudeNose", "ModifyLangevin", "ModifyImageCharge",
                 "ModifyElectricField", "ModifyCosineAccelerate"):
        assert f"kernel {name}: registered" in out


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_DRIVER), reason="oracle/_ref/refplugin not built (reference sources absent)")
@pytest.mark.parametrize("middle,cons,cos", [(1, 0, 0.0), (1, 1, 0.0), (1, 0, 0.02), (1, 1, 0.02), (0, 0, 0.0), (0, 1, 0.02), (1, 3, 0.0), (0, 3, 0.0)])
def test_reference_integrator_drives_the_hip_kernels(tmp_path, middle, cons, cos):
    """Drop-in at the KernelImpl boundary with the reference on top: the reference's VVIntegrator::step (its own stepMiddle / stepVV,
    compiled in place) calls this repository's seven HIP kernels through the reference's virtuals, stage by stage (it does not know the
    optional fused interface); trajectory against the oracle, and against this repository's own VVIntegrator on the fused path."""
    nsteps = 12
    dump_r, dump_o = str(tmp_path / "ref.bin"), str(tmp_path / "own.bin")
    r = subprocess.run([REF_DRIVER, "run", dump_r, str(middle), str(cons), str(cos), str(nsteps)], capture_output=True, text=True)
    assert r.returncode == 0 and "RUN OK" in r.stdout and f"stepCount={nsteps}" in r.stdout, r.stdout + r.stderr
    # deferred fusion (HipVVKernels.h): the reference's stage-by-stage calls complete the expected sequence once per step (twice in the
    # classic scheme) and each completion launched ONE fused step; with constraints OpenMM's solver must interleave nothing is deferred
    import re
    fused, staged = map(int, re.search(r"DEFER fused=(\d+) staged=(\d+)", r.stdout).groups())
    assert (fused, staged) == ((nsteps if middle else 2 * nsteps, 0) if cons in (0, 3) else (0, 0)), r.stdout
    # ... and the same run with the deferral switched off (every stage its own launch) ends in the same state to rounding
    dump_s = str(tmp_path / "staged.bin")
    st = subprocess.run([REF_DRIVER, "run", dump_s, str(middle), str(cons), str(cos), str(nsteps)], capture_output=True, text=True,
                        env=dict(os.environ, VVHIP_PLUGIN_DEFER="0"))
    assert st.returncode == 0 and "DEFER fused=0" in st.stdout, st.stdout + st.stderr
    staged_run = _read(dump_s)
    o = subprocess.run([DRIVER, "run", dump_o, str(middle), str(cons), str(cos), str(nsteps)], capture_output=True, text=True)
    assert o.returncode == 0 and "RUN OK" in o.stdout, o.stdout + o.stderr
    arrays = _read(dump_r)
    masses, charges, mol, pairs, cns, pos, vel, velm, posq, corr, vis, cdist = arrays[:12]
    own = _read(dump_o)
    n = masses.shape[0]
    osys = _oracle_for(arrays, middle, cons, cos, nsteps)
    x_g = posq.reshape(n, 4)[:, :3].astype(np.float64) + corr.reshape(n, 4)[:, :3].astype(np.float64)
    v_g = velm.reshape(n, 4)[:, :3]
    massive = masses != 0
    ex = np.abs(x_g - osys.positions()).max() / np.abs(osys.positions()).max()
    ev = np.abs(v_g[massive] - osys.velm[massive, :3]).max() / np.abs(osys.velm[massive, :3]).max()
    assert ex < 1e-9 and ev < 1e-9, (ex, ev)
    # the two host classes end in the same state to rounding (different launch granularity, same arithmetic)
    assert np.allclose(velm, own[7], rtol=0, atol=1e-9 * np.abs(velm).max()) and np.allclose(posq, own[8], rtol=0, atol=2e-7 * np.abs(posq).max())
    assert np.allclose(velm, staged_run[7], rtol=0, atol=1e-9 * np.abs(velm).max()) and np.allclose(posq, staged_run[8], rtol=0, atol=2e-7 * np.abs(posq).max())
    if cos != 0:
        assert vis[0] == pytest.approx(osys.viscosity()[0], rel=1e-6, abs=1e-12)


@pytest.mark.gpu
def test_deferred_fusion_only_answers_the_reference_call_order(tmp_path):
    """A host driving the KernelImpl virtuals by hand (tests/cpp/plugin_driver.cpp, hostMode): in the reference's order every step is
    answered with one fused step; with a kinetic-energy query between firstIntegrate and scaleVelocity nothing is fused -- the recorded
    stage runs before the query, the others as they come -- and both end where VVIntegrator::step ends."""
    import re
    nsteps, dumps, counts = 12, {}, {}
    for mode in (0, 1, 2):
        d = str(tmp_path / f"m{mode}.bin")
        r = subprocess.run([DRIVER, "run", d, "1", "0", "0.0", str(nsteps), str(mode)], capture_output=True, text=True)
        assert r.returncode == 0 and "RUN OK" in r.stdout and f"stepCount={nsteps}" in r.stdout, r.stdout + r.stderr
        dumps[mode] = _read(d)
        counts[mode] = tuple(map(int, re.search(r"DEFER fused=(\d+) staged=(\d+)", r.stdout).groups()))
    assert counts[1] == (nsteps, 0), counts
    assert counts[2] == (0, 3 * nsteps), counts
    for mode in (1, 2):
        assert np.allclose(dumps[mode][7], dumps[0][7], rtol=0, atol=1e-9 * np.abs(dumps[0][7]).max())       # velm
        assert np.allclose(dumps[mode][8], dumps[0][8], rtol=0, atol=2e-7 * np.abs(dumps[0][8]).max())       # posq


def _fuzz(driver, tmp_path, middle, cons, cos, nops, seed, hand, defer, **extra_env):
    import re
    d = str(tmp_path / f"fz_{middle}{cons}{seed}{hand}{defer}.bin")
    r = subprocess.run([driver, "fuzz", d, str(middle), str(cons), str(cos), str(nops), str(seed), str(hand)], capture_output=True, text=True,
                       env=dict(os.environ, VVHIP_PLUGIN_DEFER=str(defer), **extra_env))
    assert r.returncode == 0 and "RUN OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    fused, staged = map(int, re.search(r"DEFER fused=(\d+) staged=(\d+)", r.stdout).groups())
    steps, interrupted = map(int, re.search(r"FUZZ steps=(\d+) interrupted=(\d+)", r.stdout).groups())
    count = int(re.search(r"stepCount=(\d+)", r.stdout).group(1))
    return _read(d), fused, staged, steps, interrupted, count


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_DRIVER), reason="oracle/_ref/refplugin not built (reference sources absent)")
@pytest.mark.parametrize("seed", range(1, 7))
@pytest.mark.parametrize("middle,cons,cos", [(1, 0, 0.0), (1, 0, 0.02), (0, 0, 0.0), (0, 0, 0.02), (1, 3, 0.0), (0, 3, 0.0)])
def test_deferred_fusion_fuzz_under_the_reference_integrator(tmp_path, middle, cons, cos, seed):
    """Seeded random sequences of step(k), setStepSize, setTemperature, setCosAcceleration (other values and 0: the cos stages then
    leave the sequence), box changes, kinetic-energy and viscosity queries through the REFERENCE's VVIntegrator.cpp (compiled in
    place) on top of the HIP kernels; with the electrode machinery (Langevin wall atoms, images, field) as well.  The adapters'
    deferred fusion (every completed stage sequence = one fused step) against every stage run as its own launch
    (VVHIP_PLUGIN_DEFER=0): the same bits, and an exact account of what was fused (VVIntegrator.cpp:232-338)."""
    nops = 40
    a, fused, staged, steps, _, count = _fuzz(REF_DRIVER, tmp_path, middle, cons, cos, nops, seed, 0, 1)
    b, fused0, staged0, steps0, _, count0 = _fuzz(REF_DRIVER, tmp_path, middle, cons, cos, nops, seed, 0, 0)
    assert steps == steps0 == count == count0 and steps > 10
    assert (fused, staged) == (steps if middle else 2 * steps, 0), (fused, staged, steps)      # queries only fall between steps here
    assert fused0 == 0
    for k in (7, 8, 9):                                # velm, posq, posqCorrection
        if cos == 0:                                   # bit for bit
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (k, np.abs(a[k] - b[k]).max())
        else:
            # with the cos perturbation the fused step forms the group sums as moments of the still biased velocities:
            # the same algebra in another order of operations, so rounding-level differences (measured 3e-15 .. 6e-15 after 50 steps).
            # This case found a real one first (7e-4): the reference's kick kernels add forceExtra always and the array is only
            # reset in steps that have a source of extra forces, so after setCosAcceleration(0) the last cos force keeps acting
            # (K/middle.cu:11-21, VVIntegrator.cpp:238-240) -- the fused path now does the same (vv_plan.hpp: fextra_virtual).
            assert np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max() <= 1e-12 * max(1.0, np.abs(b[k]).max()), (k, np.abs(a[k] - b[k]).max())
    assert np.isfinite(a[7]).all() and np.isfinite(a[8]).all()


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_DRIVER), reason="oracle/_ref/refplugin not built (reference sources absent)")
@pytest.mark.parametrize("seed", [4, 6])
@pytest.mark.parametrize("rep", range(4))
def test_fuzz_is_insensitive_to_host_stalls(tmp_path, seed, rep):
    """The classic scheme with the cos perturbation again, every kernel compiled at run time (VVHIP_RTC=2): each first launch of a stage set
    stalls the host for about a second while the GPU drains.  Found with exactly this: the reset of both accumulator copies at a switch
    of the cos perturbation (vvhip_set_params) was a plain hipMemset, i.e. enqueued on the null stream, which the plan's non-blocking stream
    does not wait for -- it could land a step later and wipe kernel A's sums (a third to a half of the runs differed by 1e-3; bisected to that one
    fill with per-fill builds, tools/probes/fuzz_flaky.py).  Every fill of a plan buffer is now
    ordered in the plan's stream; fused and staged runs agree to rounding whatever the host's timing."""
    a = _fuzz(REF_DRIVER, tmp_path, 0, 0, 0.02, 40, seed, 0, 1, VVHIP_RTC="2")[0]
    b = _fuzz(REF_DRIVER, tmp_path, 0, 0, 0.02, 40, seed, 0, 0, VVHIP_RTC="2")[0]
    for k in (7, 8, 9):
        assert np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max() <= 1e-12 * max(1.0, np.abs(b[k]).max()), (k, rep)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(1, 13))
def test_deferred_fusion_fuzz_changes_and_queries_between_the_stages(tmp_path, seed):
    """A host that drives the KernelImpl virtuals by hand and changes the step size / temperature / box or asks for the kinetic energy
    at a random place INSIDE a step: a stage that has been recorded belongs to the parameters of the moment it was called, so it runs
    (with them) before the change shows, and the step is not fused; every undisturbed step is.  Same bits as with the deferral off."""
    nops = 60
    a, fused, staged, steps, interrupted, count = _fuzz(DRIVER, tmp_path, 1, 0, 0.0, nops, seed, 1, 1)
    b, fused0, staged0, steps0, interrupted0, count0 = _fuzz(DRIVER, tmp_path, 1, 0, 0.0, nops, seed, 1, 0)
    assert steps == steps0 == count == count0 and interrupted == interrupted0 and steps > 15
    assert fused0 == 0
    # an interrupted step may still be fused when the "change" drew the value that was already set (nothing changed), never the reverse
    assert fused + staged // 3 == steps and staged % 3 == 0 and fused >= steps - interrupted, (fused, staged, steps, interrupted)
    for k in (7, 8, 9):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (k, np.abs(a[k] - b[k]).max())


def test_cmake_build_produces_the_same_plugin(tmp_path):
    """The CMake route (what a maintainer of an OpenMM installation would use) configures and builds the API library, the plugin and
    the driver against the stand-in headers, reusing the in-tree libvvhip.so; the plugin exports the three registration symbols."""
    import shutil
    if not shutil.which("cmake") or not shutil.which("ninja"):
        pytest.skip("cmake / ninja not available")
    lib = os.path.join(ROOT, "openmm-velocityverlet_amd", "lib", "libvvhip.so")
    bdir = str(tmp_path / "b")
    r = subprocess.run(["cmake", "-S", ROOT, "-B", bdir, "-G", "Ninja", f"-DVVHIP_PREBUILT={lib}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run(["cmake", "--build", bdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    plug = os.path.join(bdir, "plugins", "libVelocityVerletPluginHIP.so")
    syms = subprocess.run(["nm", "-D", plug], capture_output=True, text=True).stdout
    for name in ("registerPlatforms", "registerKernelFactories", "registerHipVVKernelFactories"):
        assert f" T {name}" in syms, name
    r = subprocess.run([os.path.join(bdir, "vv_plugin_driver"), "registry"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
