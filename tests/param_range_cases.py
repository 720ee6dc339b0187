"""Small Drude systems at the edges of the integrator's parameter range, for tests/test_param_range.py (CPU: the oracle alone reaches the
regime each case claims and stays finite there) and tests/test_gpu_param_range.py (the fused step against the oracle).  Every other GPU
test runs T = 300-333 K, T_Drude = 1 K, dt = 1-2 fs, thermostat frequencies 10 / 40 per ps, positions inside the box and the masses of
systems.py; the cases here move one of those at a time: the temperatures (the fixed-point scales of the thermostat sums, csrc/vv_launch.cpp:
pick_scale, and the hard wall's sqrt(kB T_D)), dt and the couplings (the chain's masses kT / f^2), the masses (the mass tables), the
start's kinetic energy (the headroom of the sums) and z (cos_kz's fallback to the library cosine beyond |x| = 1024 or next to a
multiple of pi / 2, csrc/vv_dev_wave.inc).  Velocities are rescaled so that every case starts near its own targets.

The synthetic force field (tether springs, a 209 200 kJ/mol/nm^2 spring inside every Drude pair) is sized for dt = 1 fs and a 0.4 u
Drude particle: w dt = 0.72.  With dt = 4 fs (w dt = 2.9), masses / 100 (7.2) or a 0.05 u Drude particle (2.05) velocity Verlet is past
its stability limit of 2: the Drude thermostat's scale factor underflows within four steps and the hard wall of the reference then
divides 0 by 0 (mixed precision, dt = 4 fs, step 4) -- a run that says nothing about the code under test.  Those cases therefore keep
w dt at 0.72: the spring constants go with dt^-2 and with the (reduced) masses.  (Masses x 100 only slow the springs down and keep them.)
Test code only."""
import dataclasses
import importlib
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

from oracle import oracle as O

pkg = importlib.import_module("openmm-velocityverlet_amd")
systems = pkg.systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSTEPS = 10
MAXD = 0.02
# ... of the 5000 K / 50 K case: its Drude displacements are ~ sqrt(kB 50 K / 209 200) = 1.4e-3 nm, the usual wall 14 of those away and
# never met; at 0.002 nm pairs cross it within the first steps
HOT_MAXD = 0.002
BASE_T, BASE_TD = 333.0, 1.0        # what systems.drude_il draws its velocities at
SHIFT_BOXES = 400                   # |2 * 3.1415926 * 400| = 2 513 > 1024
MIXED_WAVE_UNSHIFTED = 40           # particles of the mixed-wave case that stay in the box


def base(which):
    """"small": 444 particles, one block; "large": 2 590 particles, partial last waves, several tiles."""
    if which == "small":
        return systems.drude_il(cells=(1, 1, 1), pairs_per_cell=12, seed=21)
    return systems.drude_il(cells=(1, 1, 1), pairs_per_cell=70, seed=7)


@dataclasses.dataclass
class Case:
    name: str
    spec: object
    regime: str                         # what the case must reach (tests/test_param_range.py asserts it)
    temperature: float = BASE_T
    drude_temperature: float = BASE_TD
    step_size: float = 0.001
    frequency: float = 10.0
    drude_frequency: float = 40.0
    loops_per_step: int = 1
    cos_values: tuple = (0.0, 0.02)     # cos accelerations the trajectories run with
    precisions: tuple = ("mixed",)      # precision modes of the trajectories
    shifted: np.ndarray = None          # bool [N]: particles moved SHIFT_BOXES box lengths along z
    node_particle: int = -1             # particle whose z sits next to pi / 2 in cos_kz's argument
    ke_factor: float = 1.0              # 2KE of the start over the thermostat's total target, roughly
    k_tether: float = 1000.0            # the synthetic force field (Context / OracleSystem defaults)
    k_drude: float = 209200.0
    max_drude_distance: float = MAXD

    def params(self, middle=True, cos=0.0):
        return O.Params(temperature=self.temperature, frequency=self.frequency, drude_temperature=self.drude_temperature,
                        drude_frequency=self.drude_frequency, step_size=self.step_size, loops_per_step=self.loops_per_step,
                        max_drude_distance=self.max_drude_distance, cos_acceleration=cos, use_middle_scheme=middle)

    def integrator(self, middle=True, cos=0.0):
        it = pkg.integrator.VVIntegrator(self.temperature, self.frequency, self.drude_temperature, self.drude_frequency, self.step_size,
                                         3, self.loops_per_step)
        it.setMaxDrudeDistance(self.max_drude_distance)
        it.setCosAcceleration(cos)
        it.setUseMiddleScheme(middle)
        return it


# ---- velocity rescaling
def _split_pairs(spec, v):
    d, p = spec.drude_pairs[:, 0], spec.drude_pairs[:, 1]
    m = spec.masses
    mt = (m[d] + m[p])[:, None]
    return d, p, (m[d, None] * v[d] + m[p, None] * v[p]) / mt, v[d] - v[p]


def retarget(spec, T, Td, masses=None):
    """A copy of `spec` with `masses` (default: its own) whose velocities sit near (T, Td): every velocity times sqrt(m_old / m_new)
    sqrt(T / 333), the relative velocity of a Drude pair times sqrt(mu_old / mu_new) sqrt(Td / 1) around the pair's centre of mass."""
    new = dataclasses.replace(spec, masses=spec.masses.copy() if masses is None else np.asarray(masses, np.float64),
                              positions=spec.positions.copy(), velocities=spec.velocities.copy())
    m0, m1 = spec.masses, new.masses
    d, p, vcm, vrel = _split_pairs(spec, spec.velocities)
    v = spec.velocities * np.sqrt(m0 / m1)[:, None] * math.sqrt(T / BASE_T)
    mt0, mt1 = m0[d] + m0[p], m1[d] + m1[p]
    vcm = vcm * np.sqrt(mt0 / mt1)[:, None] * math.sqrt(T / BASE_T)
    vrel = vrel * np.sqrt((m0[d] * m0[p] / mt0) / (m1[d] * m1[p] / mt1))[:, None] * math.sqrt(Td / BASE_TD)
    v[d] = vcm + vrel * (m1[p] / mt1)[:, None]
    v[p] = vcm - vrel * (m1[d] / mt1)[:, None]
    new.velocities = v
    return new


def shift_z(spec, mask, boxes):
    new = dataclasses.replace(spec, positions=spec.positions.copy())
    new.positions[mask, 2] += boxes * float(spec.box[2])
    return new


# ---- the host build of cos_short_range
_PROBE = None


def have_probe():
    return shutil.which("g++") is not None and " fma " in open("/proc/cpuinfo").read().replace("\n", " ")


def _probe():
    global _PROBE
    if _PROBE is None:
        exe = os.path.join(tempfile.mkdtemp(prefix="cos_ok_probe"), "cos_ok_probe")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-I", os.path.join(ROOT, "openmm-velocityverlet_amd", "csrc"),
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "cos_ok_probe.cpp")], check=True)
        _PROBE = exe
    return _PROBE


def cos_ok(z, inv_box_z):
    """cos_short_range's `ok` for cos_kz's argument of every z (the stored `real` values, and 1 / Lz rounded to `real`)."""
    text = "".join(float(x).hex() + "\n" for x in np.asarray(z).ravel())
    r = subprocess.run([_probe(), "ok", float(inv_box_z).hex()], input=text, capture_output=True, text=True, check=True)
    return np.array(r.stdout.split(), dtype=np.int64).astype(bool)


def node_z(lz):
    """A double z in (Lz / 4, Lz / 4 + 1e-7 Lz) for which cos_short_range sends cos_kz to the library cosine although |x| <= 1024."""
    r = subprocess.run([_probe(), "node", float(lz).hex()], capture_output=True, text=True, check=True)
    return float.fromhex(r.stdout.split()[0])


def real_z(spec, prec):
    """z as the kernels read it (posq.z in `real`) and 1 / Lz as they receive it."""
    R = O.REAL[prec]
    return spec.positions[:, 2].astype(R).astype(np.float64), float(R(1.0 / float(spec.box[2])))


# ---- the cases
TEMPERATURES = [(1.0, 0.01), (30.0, 0.1), (5000.0, 50.0), (333.0, 333.0)]
ALL3 = ("single", "mixed", "double")


def _temperature(T, Td):
    which = "small" if T in (1.0, 5000.0) else "large"
    regime = {1.0: "scale exponent clamped", 30.0: "scale exponent clamped", 5000.0: "hard wall fires", 333.0: "hot Drudes"}[T]
    return Case(f"T{T:g}_Td{Td:g}", retarget(base(which), T, Td), regime, temperature=T, drude_temperature=Td, cos_values=(0.02,),
                precisions=ALL3, max_drude_distance=HOT_MAXD if T == 5000.0 else MAXD)


def _heavy_parent(spec):
    m = spec.masses.copy()
    m[spec.drude_pairs[:, 0]], m[spec.drude_pairs[:, 1]] = 0.05, 200.0
    return m


def _hot(factor, which):
    spec = base(which)
    spec = dataclasses.replace(spec, velocities=spec.velocities * math.sqrt(factor))
    return Case(f"hot{factor:g}", spec, "hot start", precisions=("mixed", "double"), ke_factor=factor)


def _unwrapped(name, which, boxes, keep=0):
    spec = base(which)
    mask = np.arange(spec.num_atoms) >= keep
    return Case(name, shift_z(spec, mask, boxes), "unwrapped", cos_values=(0.02,), precisions=("mixed", "double"), shifted=mask)


def _node():
    spec = base("small")
    spec = dataclasses.replace(spec, positions=spec.positions.copy())
    in_pair = np.zeros(spec.num_atoms, bool)
    in_pair[spec.drude_pairs.reshape(-1)] = True
    i = int(np.nonzero(~in_pair)[0][5])           # a hydrogen: moving it strains no Drude spring
    spec.positions[i, 2] = node_z(float(spec.box[2]))
    return Case("node", spec, "node", cos_values=(0.02,), precisions=("double",), node_particle=i)


_BUILDERS = {
    **{f"T{T:g}_Td{Td:g}": (lambda T=T, Td=Td: _temperature(T, Td)) for T, Td in TEMPERATURES},
    "dt1e-5": lambda: Case("dt1e-5", base("small"), "time step", step_size=1e-5),
    "dt0.004": lambda: Case("dt0.004", base("large"), "time step", step_size=0.004, k_drude=209200.0 / 16),
    "soft": lambda: Case("soft", base("small"), "coupling", frequency=0.1, drude_frequency=0.4),
    "stiff": lambda: Case("stiff", base("large"), "coupling", frequency=200.0, drude_frequency=800.0),
    "stiff_loops3": lambda: Case("stiff_loops3", base("large"), "coupling", frequency=200.0, drude_frequency=800.0, loops_per_step=3),
    "light": lambda: Case("light", retarget(base("small"), BASE_T, BASE_TD, base("small").masses * 0.01), "masses", k_tether=10.0, k_drude=2092.0),
    "heavy": lambda: Case("heavy", retarget(base("large"), BASE_T, BASE_TD, base("large").masses * 100.0), "masses"),
    "heavy_parent": lambda: Case("heavy_parent", retarget(base("small"), BASE_T, BASE_TD, _heavy_parent(base("small"))), "masses",
                                 k_drude=209200.0 * (0.05 * 200.0 / 200.05) / (0.4 * 11.611 / 12.011)),
    "hot30": lambda: _hot(30.0, "large"),
    "hot100": lambda: _hot(100.0, "small"),
    "up400": lambda: _unwrapped("up400", "small", +SHIFT_BOXES),
    "down400": lambda: _unwrapped("down400", "large", -SHIFT_BOXES),
    "mixed_wave": lambda: _unwrapped("mixed_wave", "small", +SHIFT_BOXES, keep=MIXED_WAVE_UNSHIFTED),
    "node": _node,
}
CASES = list(_BUILDERS)
TEMPERATURE_CASES = [f"T{T:g}_Td{Td:g}" for T, Td in TEMPERATURES]
COLD, HOT_THERMOSTAT = TEMPERATURE_CASES[0], TEMPERATURE_CASES[2]
_CACHE = {}


def case(name) -> Case:
    """The named case (built once; nothing steps a case's spec in place)."""
    if name not in _CACHE:
        _CACHE[name] = _BUILDERS[name]()
    return _CACHE[name]


def scale_exponent(nkbt):
    """csrc/vv_launch.cpp: pick_scale(total, 1024) of the three 2KE sums, restated: (exponent before the clamp, exponent used)."""
    top = 2.0 ** 62 / (max(float(sum(nkbt)), 1.0) * 1024.0)
    k = math.floor(math.log2(top))
    return k, max(0, min(k, 40))


# ---- the oracle's side of a trajectory, computed once per (case, scheme, cos, precision) and shared
_ORACLE = {}


def oracle_run(name, middle, cos, prec, steps=NSTEPS, watch=None):
    """The oracle after `steps` steps of the case (force_mode 1 = the tether forces of the product's "tether" provider).  `watch`: called
    with the OracleSystem after every step (such runs are not kept)."""
    key = (name, middle, cos, prec, steps)
    if watch is None and key in _ORACLE:
        return _ORACLE[key]
    c = case(name)
    osys = O.OracleSystem(c.spec, c.params(middle, cos), prec, force_mode=1, k_tether=c.k_tether, k_drude=c.k_drude)
    if watch is None:
        osys.step(steps)
        _ORACLE[key] = osys
    else:
        for _ in range(steps):
            osys.step(1)
            watch(osys)
    return osys


def rel_gap(a, b, mask=None):
    """max |a - b| / max |b| (over the rows of `mask`)."""
    if mask is not None:
        a, b = a[mask], b[mask]
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def single_gap(name, middle, cos=0.02):
    """Gap between the oracle in single and in double precision after the case's steps: positions, velocities of massive particles
    (max |difference| / max |value|) and the groups' 2KE (worst relative difference)."""
    s, d = oracle_run(name, middle, cos, "single"), oracle_run(name, middle, cos, "double")
    m = d.velm[:, 3] != 0
    ntg = d.s.num_tg
    return dict(x=rel_gap(s.positions(), d.positions()), v=rel_gap(s.velm[:, :3].astype(np.float64), d.velm[:, :3], m),
                ke2=float(np.abs(s.ke2()[:ntg] / d.ke2()[:ntg] - 1).max()))
