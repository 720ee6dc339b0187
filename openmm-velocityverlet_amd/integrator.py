"""Host-side mirror of the reference's Python surface for the hot path.

``VVIntegrator`` has the methods of the SWIG class ``velocityverletplugin.VVIntegrator``
(/root/reference/python/velocityverletplugin.i:83-129) with the argument meaning and defaults of the
C++ class (openmmapi/include/openmm/VVIntegrator.h:49-507, openmmapi/src/VVIntegrator.cpp:46-70).
Because neither OpenMM nor its unit package exists here, getters return plain floats in OpenMM's MD
units (K, 1/ps, nm, nm/ps^2, kJ/(nm e)) instead of ``unit.Quantity``.

``Context`` stands in for ``openmm.Context`` just far enough to run the path stand-alone: it owns the
device arrays OpenMM's HipContext would own (velm, posq, posqCorrection, force, random) and a force
provider that plays the part of ``calcForcesAndEnergy``.  Inside a real OpenMM the same C ABI is driven
by the C++ adapters in platforms/hip.  All arithmetic happens in libvvhip.so.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import List, Optional, Tuple

import numpy as np

from . import vvhip as H
from .systems import BOLTZ, SystemSpec


def padded(n: int) -> int:
    return (n + 31) // 32 * 32


class VVIntegrator:
    """Same constructor and method names as the reference's VVIntegrator (velocityverletplugin.i:85-127)."""

    def __init__(self, temperature, frequency, drudeTemperature, drudeFrequency, stepSize, numNHChains=3, loopsPerStep=1):
        # openmmapi/src/VVIntegrator.cpp:46-70
        self._temperature = float(temperature)
        self._frequency = float(frequency)
        self._drudeTemperature = float(drudeTemperature)
        self._drudeFrequency = float(drudeFrequency)
        self._stepSize = float(stepSize)
        self._numNHChains = int(numNHChains)
        self._loopsPerStep = int(loopsPerStep)
        self._constraintTolerance = 1e-5
        self._maxDrudeDistance = 0.0
        self._friction = 5.0
        self._drudeFriction = 20.0
        self._randomNumberSeed = 0
        self._mirrorLocation = 0.0
        self._electricField = 0.0
        self._cosAcceleration = 0.0
        self._useCOMTempGroup = False
        self._useMiddleScheme = True
        self._debugEnabled = False
        self._autoSetCOMTempGroup = True
        self._autoSetFriction = True
        self._particlesLD: List[int] = []
        self._imagePairs: List[Tuple[int, int]] = []
        self._particlesElectrolyte: List[int] = []
        self._context: Optional["Context"] = None

    # ---- plain parameters (VVIntegrator.h:70-431)
    def getTemperature(self): return self._temperature
    def setTemperature(self, temp): self._temperature = float(temp); self._push()
    def getFrequency(self): return self._frequency
    def setFrequency(self, tau): self._frequency = float(tau); self._push()
    def getDrudeTemperature(self): return self._drudeTemperature
    def setDrudeTemperature(self, temp): self._drudeTemperature = float(temp); self._push()
    def getDrudeFrequency(self): return self._drudeFrequency
    def setDrudeFrequency(self, tau): self._drudeFrequency = float(tau); self._push()
    def getStepSize(self): return self._stepSize
    def setStepSize(self, dt): self._stepSize = float(dt); self._push()
    def getConstraintTolerance(self): return self._constraintTolerance
    def setConstraintTolerance(self, tol): self._constraintTolerance = float(tol)
    def getNumNHChains(self): return self._numNHChains
    def setNumNHChains(self, n): self._numNHChains = int(n)
    def getLoopsPerStep(self): return self._loopsPerStep
    def setLoopsPerStep(self, n): self._loopsPerStep = int(n); self._push()
    def getUseCOMTempGroup(self): return self._useCOMTempGroup

    def setUseCOMTempGroup(self, use):                      # VVIntegrator.h:147-150
        self._useCOMTempGroup = bool(use)
        self._autoSetCOMTempGroup = False

    def getUseMiddleScheme(self): return self._useMiddleScheme
    def setUseMiddleScheme(self, use): self._useMiddleScheme = bool(use)
    def getMaxDrudeDistance(self): return self._maxDrudeDistance
    def setMaxDrudeDistance(self, d): self._maxDrudeDistance = float(d); self._push()

    def addParticleLangevin(self, particle):                # VVIntegrator.h:186-189
        self._particlesLD.append(int(particle))
        return len(self._particlesLD)

    def getRandomNumberSeed(self): return self._randomNumberSeed
    def setRandomNumberSeed(self, seed): self._randomNumberSeed = int(seed)
    def getFriction(self): return self._friction

    def setFriction(self, fric):                            # VVIntegrator.h:213-216 (quirk Q7: double, not int)
        self._friction = float(fric)
        self._autoSetFriction = False
        self._push()

    def getDrudeFriction(self): return self._drudeFriction

    def setDrudeFriction(self, fric):
        self._drudeFriction = float(fric)
        self._autoSetFriction = False
        self._push()

    def addImagePair(self, image, parent):                  # VVIntegrator.cpp:76-80
        self._imagePairs.append((int(image), int(parent)))
        return len(self._imagePairs)

    def getImagePairs(self): return list(self._imagePairs)
    def setMirrorLocation(self, z): self._mirrorLocation = float(z); self._push()
    def getMirrorLocation(self): return self._mirrorLocation

    def addParticleElectrolyte(self, particle):
        self._particlesElectrolyte.append(int(particle))
        return len(self._particlesElectrolyte)

    def setElectricField(self, field):
        """kJ/(nm e) per particle, as the C++ API (1 V/nm = 1.602176634e-22 here; quirk Q12)."""
        self._electricField = float(field)
        self._push()

    def getElectricField(self): return self._electricField
    def setCosAcceleration(self, a): self._cosAcceleration = float(a); self._push()
    def getCosAcceleration(self): return self._cosAcceleration
    def getDebugEnabled(self): return self._debugEnabled
    def setDebugEnabled(self, e): self._debugEnabled = bool(e)

    # ---- actions
    def step(self, steps):                                  # VVIntegrator.cpp:223-230
        if self._context is None:
            raise H.VVHipError(H.ERR_INVALID, "This Integrator is not bound to a context!")
        self._context._step(int(steps))

    def getViscosity(self):                                 # VVIntegrator.cpp:378-383 -> (vMax nm/ps, 1/viscosity)
        if self._context is None or self._cosAcceleration == 0:
            return (0.0, 0.0)
        return self._context._viscosity()

    def getDrudeTemperatures(self):
        """(KE_COM, KE_Atom, KE_Drude) in kJ/mol and (T_COM, T_Atom, T_Drude) in K of the current velocities, as one tuple of six
        (vvhip_drude_temperatures: computed on the device, 56 bytes copied back).  Raises when the integrator is not bound."""
        if self._context is None:
            raise H.VVHipError(H.ERR_INVALID, "This Integrator is not bound to a context!")
        return self._context.getDrudeTemperatures()

    # ---- internals
    def _params(self) -> H.Params:
        return H.Params(self._temperature, self._frequency, self._drudeTemperature, self._drudeFrequency, self._stepSize,
                        self._numNHChains, self._loopsPerStep, self._maxDrudeDistance, self._friction, self._drudeFriction,
                        self._mirrorLocation, self._electricField, self._cosAcceleration, int(self._useCOMTempGroup),
                        int(self._useMiddleScheme), int(self._autoSetCOMTempGroup), int(self._autoSetFriction), self._constraintTolerance)

    def _push(self):
        if self._context is not None:
            self._context._set_params()


def create_plan(system: SystemSpec, integrator: "VVIntegrator", precision: str = "mixed", shard=None,
                particles_ld=None, image_pairs=None, electrolyte=None):
    """vvhip_plan_create: host-only analysis (no GPU needed).  Returns (plan handle, PlanInfo, keep-alive arrays)."""
    n = system.num_atoms
    shard = (0, n) if shard is None else shard
    particles_ld = list(system.particles_ld) + list(integrator._particlesLD) if particles_ld is None else particles_ld
    image_pairs = list(system.image_pairs) + list(integrator._imagePairs) if image_pairs is None else image_pairs
    electrolyte = list(system.particles_electrolyte) + list(integrator._particlesElectrolyte) if electrolyte is None else electrolyte
    k = dict(
        masses=np.ascontiguousarray(system.masses, dtype=np.float64),
        mol_id=np.ascontiguousarray(system.mol_id, dtype=np.int32),
        drude=np.ascontiguousarray(system.drude_pairs, dtype=np.int32).reshape(-1),
        cons=np.ascontiguousarray(system.constraints, dtype=np.int32).reshape(-1),
        ld=np.ascontiguousarray(particles_ld, dtype=np.int32),
        img=np.ascontiguousarray(image_pairs, dtype=np.int32).reshape(-1),
        el=np.ascontiguousarray(electrolyte, dtype=np.int32),
        cdist=np.ascontiguousarray(getattr(system, "constraint_distances", None) if getattr(system, "constraint_distances", None) is not None else [], dtype=np.float64))
    if k["cdist"].size not in (0, k["cons"].size // 2):
        raise ValueError("constraint_distances must have one entry per constraint")
    vsites = list(getattr(system, "virtual_sites", None) or [])      # (site, kind, (parents), (params)) per site: System::getVirtualSite
    k["vs"] = np.full((len(vsites), 5), -1, dtype=np.int32)
    k["vsp"] = np.zeros((len(vsites), 12), dtype=np.float64)
    for i, (site, kind, parents, prm) in enumerate(vsites):
        k["vs"][i, 0], k["vs"][i, 1] = site, kind
        k["vs"][i, 2:2 + len(parents)] = parents
        k["vsp"][i, :len(prm)] = prm
    ptr = lambda a: a.ctypes.data if a.size else None
    desc = H.SystemDesc(n, padded(n), ptr(k["masses"]), ptr(k["mol_id"]), system.num_molecules,
                        k["drude"].size // 2, ptr(k["drude"]), k["cons"].size // 2, ptr(k["cons"]),
                        int(system.has_cm_motion_remover), k["ld"].size, ptr(k["ld"]), k["img"].size // 2, ptr(k["img"]),
                        k["el"].size, ptr(k["el"]), int(shard[0]), int(shard[1]), ptr(k["cdist"]),
                        len(vsites), ptr(k["vs"]), ptr(k["vsp"]))
    plan = C.c_void_p()
    err = C.create_string_buffer(512)
    rc = H.lib.vvhip_plan_create(C.byref(desc), C.byref(integrator._params()), H.PRECISION[precision], C.byref(plan), err, 512)
    if rc != H.OK:
        raise H.VVHipError(rc, err.value.decode())
    info = H.PlanInfo()
    H.check(H.lib.vvhip_plan_get_info(plan, C.byref(info)), plan)
    return plan, info, k


def plan_layout(system: SystemSpec, integrator: "VVIntegrator", precision: str = "mixed", shard=None):
    """Host-only: the analysis results and the wave layout [num_waves*64, 2] = (particle, role word)."""
    plan, info, _ = create_plan(system, integrator, precision, shard)
    try:
        nslots = H.lib.vvhip_plan_get_slots(plan, None, 0)
        slots = np.zeros((nslots, 2), dtype=np.int32)
        got = H.lib.vvhip_plan_get_slots(plan, slots.ctypes.data, nslots)
        assert got == nslots
    finally:
        H.lib.vvhip_plan_destroy(plan)
    return info, slots


def drude_report_dof(system: SystemSpec, integrator: "VVIntegrator", precision: str = "mixed", shard=None):
    """Host-only: the degrees of freedom (COM, Atom, Drude) of the Drude temperature report, always those of the whole system."""
    plan, _, _ = create_plan(system, integrator, precision, shard)
    try:
        dof = (C.c_double * 3)()
        H.check(H.lib.vvhip_drude_report_dof(plan, C.byref(dof)), plan)
    finally:
        H.lib.vvhip_plan_destroy(plan)
    return tuple(dof)


def plan_launch_shape(system: SystemSpec, integrator: "VVIntegrator", precision: str = "mixed", shard=None):
    """Host-only: (threads of a block's tile waves, most blocks of kernel A, of kernel B, tile waves per block of the one-launch step or 0) as the
    plan chooses them for a whole MI355X (vvhip_debug_launch_shape)."""
    plan, _, _ = create_plan(system, integrator, precision, shard)
    try:
        shape = (C.c_int32 * 4)()
        H.check(H.lib.vvhip_debug_launch_shape(plan, C.byref(shape)), plan)
    finally:
        H.lib.vvhip_plan_destroy(plan)
    return tuple(shape)


DEFAULT_TUNE: dict = {}      # see Context(tune=...)


@dataclasses.dataclass
class Series:
    """Rows of a device-side series (Context.series_read; include/vvhip.h: vvhip_series_row), one per sampled step.  The Drude fields are
    None without the Drude part, the thermostat and viscosity fields None without the thermostat part."""
    step: np.ndarray                       # int64 [n]: the step after which the row was taken
    dropped: int                           # rows not recorded for want of capacity (their steps follow the last row)
    raw: Optional[np.ndarray] = None       # int64 [n, 6]: the report's raw sums (vvhip_drude_report_raw) of this plan's particles
    ok: Optional[np.ndarray] = None        # bool [n]: the row's fixed-point sums stayed in range (ke / t are NaN where not)
    ke: Optional[np.ndarray] = None        # [n, 3] KE_COM, KE_Atom, KE_Drude (kJ/mol), as getDrudeTemperatures
    t: Optional[np.ndarray] = None         # [n, 3] T_COM, T_Atom, T_Drude (K)
    eta: Optional[np.ndarray] = None       # [n, 3, MAX_CHAINS] ... the fields of getNHState() after the row's step
    eta_dot: Optional[np.ndarray] = None
    eta_dotdot: Optional[np.ndarray] = None
    ke2: Optional[np.ndarray] = None
    vscale: Optional[np.ndarray] = None
    v_bias: Optional[np.ndarray] = None
    box: Optional[np.ndarray] = None       # [n, 3] and [n]: what the row's step ran with
    cos_acceleration: Optional[np.ndarray] = None
    v_max: Optional[np.ndarray] = None     # [n] nm/ps and 1/viscosity as getViscosity() returns them (0 without the cos acceleration)
    inv_viscosity: Optional[np.ndarray] = None

    def __len__(self):
        return len(self.step)


@dataclasses.dataclass
class Frames:
    """Trajectory frames of a device-side recorder (Context.frames_read; include/vvhip.h: vvhip_frames_*), one per recorded step, in nm and
    nm/ps.  The arrays have the recorder's component type (float32, or float64 with frames_start(float64=True))."""
    step: np.ndarray                       # int64 [n]: the step after which the frame was taken
    box: np.ndarray                        # float64 [n, 3]: the periodic box the step ran with
    particles: np.ndarray                  # int32 [m]: global indices of the recorded particles (of this context's shard), in frame order
    positions: Optional[np.ndarray]        # [n, m, 3] as stored: unwrapped, image particles and virtual sites included; None if not recorded
    velocities: Optional[np.ndarray]       # [n, m, 3], or None
    dropped: int                           # frames not recorded for want of capacity (their steps follow the last frame)

    def __len__(self):
        return len(self.step)


@dataclasses.dataclass
class Profile:
    """Sums per bin of one box axis, over the recorded particles and `samples` samples (Context.profile_read; include/vvhip.h:
    vvhip_profile_* states the arithmetic).  `words` is the device's table as it stands, int64 [groups, rows, nbins]; the float64 views are
    word * 2^-frac_bits, None for a quantity that was not recorded."""
    samples: int
    dropped: int                           # samples that were due past max_samples: nothing was added for them
    out_of_range: int                      # particle-samples left out of every row (a term NaN or at / beyond its limit)
    axis: int
    box: np.ndarray                        # float64 [3]: the periodic box at the read
    edges: np.ndarray                      # float64 [nbins + 1]: the bins' edges along the axis, nm
    words: np.ndarray                      # int64 [groups, rows, nbins]
    row_of: tuple                          # first row of (count, charge, mass, momentum, kinetic), -1: not recorded
    frac_bits: tuple
    count: np.ndarray                      # [groups, nbins]
    charge: Optional[np.ndarray] = None    # [groups, nbins] e
    mass: Optional[np.ndarray] = None      # [groups, nbins] Da
    momentum: Optional[np.ndarray] = None  # [groups, 3, nbins] Da nm/ps
    kinetic: Optional[np.ndarray] = None   # [groups, nbins] sum m |v|^2, Da nm^2/ps^2

    @property
    def centres(self) -> np.ndarray:
        return 0.5 * (self.edges[:-1] + self.edges[1:])

    def bin_volume(self) -> float:
        return float(self.box[0] * self.box[1] * self.box[2]) / (len(self.edges) - 1)

    def number_density(self) -> np.ndarray:
        """[groups, nbins] particles per nm^3, averaged over the samples."""
        return self.count / (self.bin_volume() * max(self.samples, 1))

    def charge_density(self) -> np.ndarray:
        """[groups, nbins] e per nm^3, averaged over the samples."""
        if self.charge is None:
            raise ValueError("the charge was not recorded (profile_start(charge=True))")
        return self.charge / (self.bin_volume() * max(self.samples, 1))

    def velocity(self) -> np.ndarray:
        """[groups, 3, nbins] momentum / mass, nm/ps, 0 where a bin holds no mass."""
        if self.momentum is None or self.mass is None:
            raise ValueError("momentum and mass were not both recorded (profile_start(mass=True, momentum=True))")
        m = self.mass[:, None, :]
        return np.where(m > 0, self.momentum / np.where(m > 0, m, 1.0), 0.0)


def profile_from_words(words, layout, counts, box) -> Profile:
    """A Profile from a table's int64 words [groups * rows * nbins], its layout (H.ProfileLayout) and counts."""
    g, rows, nb = layout.num_groups, layout.rows, layout.nbins
    words = np.ascontiguousarray(words, dtype=np.int64).reshape(g, rows, nb)
    box = np.asarray(box, dtype=np.float64)
    row_of, frac = tuple(layout.row_of), tuple(layout.frac_bits)
    return Profile(samples=int(counts.samples), dropped=int(counts.dropped), out_of_range=int(counts.out_of_range), axis=int(layout.axis),
                   box=box, edges=np.arange(nb + 1, dtype=np.float64) * (box[layout.axis] / nb), words=words, row_of=row_of, frac_bits=frac,
                   **profile_views(words, row_of, frac))


def profile_views(words, row_of, frac_bits) -> dict:
    """The float64 views of a table: {quantity: word * 2^-frac_bits, or None where it was not recorded}."""
    def view(q, n=1):
        if row_of[q] < 0:
            return None
        a = words[:, row_of[q]: row_of[q] + n, :].astype(np.float64) * 2.0 ** -frac_bits[q]
        return a[:, 0, :] if n == 1 else a

    return dict(count=view(0), charge=view(1), mass=view(2), momentum=view(3, 3), kinetic=view(4))


@dataclasses.dataclass
class Msd:
    """Mean-squared displacements per group and lag (Context.msd_read; include/vvhip.h: vvhip_msd_* states the units, the schedule and the
    terms).  `words` is the device's table as it stands, int64 [groups, lags, 4]: pairs, then the sums of dx^2, dy^2, dz^2 scaled by
    2^frac_bits."""
    samples: int
    dropped: int                           # samples that were due past max_samples: nothing was added or stored for them
    out_of_range: int                      # unit-pairs left out (a displacement component NaN or at / beyond the limit)
    origin_floor: int                      # origins with an ordinal below it are dead (a barostat move rewrote the positions)
    interval: int
    origin_every: int
    frac_bits: int
    molecules: bool
    words: np.ndarray                      # int64 [groups, lags, 4]

    @property
    def lag_steps(self) -> np.ndarray:
        """int64 [lags]: row l is the lag of (l + 1) * interval steps."""
        return (np.arange(self.words.shape[1], dtype=np.int64) + 1) * self.interval

    @property
    def pairs(self) -> np.ndarray:
        """int64 [groups, lags]: unit-pairs behind every row."""
        return self.words[:, :, 0]

    @property
    def msd(self) -> np.ndarray:
        """float64 [groups, lags, 3]: <dx^2>, <dy^2>, <dz^2> in nm^2 = word * 2^-frac_bits / pairs, NaN where a row has no pairs."""
        n = self.pairs[:, :, None]
        sums = self.words[:, :, 1:].astype(np.float64) * 2.0 ** -self.frac_bits
        return np.where(n > 0, sums / np.where(n > 0, n, 1), np.nan)

    @property
    def total(self) -> np.ndarray:
        """float64 [groups, lags]: <|dr|^2> in nm^2."""
        return self.msd.sum(axis=2)

    def diffusion(self, dt: float, first_lag: int, last_lag: int, axes=(0, 1, 2)) -> np.ndarray:
        """float64 [groups]: the diffusion coefficient in nm^2/ps from rows first_lag .. last_lag (inclusive): the least-squares slope of
        the MSD summed over `axes` against the lag time (lag_steps * dt, dt in ps), divided by 2 * len(axes)."""
        axes = tuple(axes)
        rows = slice(int(first_lag), int(last_lag) + 1)
        t = self.lag_steps[rows].astype(np.float64) * float(dt)
        if t.size < 2:
            raise ValueError("a slope needs at least two lags")
        y = self.msd[:, rows, :][:, :, list(axes)].sum(axis=2)
        tc = t - t.mean()
        slope = ((y - y.mean(axis=1, keepdims=True)) * tc).sum(axis=1) / (tc * tc).sum()
        return slope / (2.0 * len(axes))


def msd_from_words(words, layout, counts) -> Msd:
    """An Msd from a table's int64 words [groups * lags * 4], its layout (H.MsdLayout) and counts (H.MsdCounts)."""
    words = np.ascontiguousarray(words, dtype=np.int64).reshape(layout.num_groups, layout.num_lags, 4)
    return Msd(samples=int(counts.samples), dropped=int(counts.dropped), out_of_range=int(counts.out_of_range),
               origin_floor=int(counts.origin_floor), interval=int(layout.interval), origin_every=int(layout.origin_every),
               frac_bits=int(layout.frac_bits), molecules=layout.mode == H.MSD_MOLECULES, words=words)


ACF_MODES = ("velocity", "molecules", "orientation")      # = H.ACF_VELOCITY_PARTICLES, H.ACF_VELOCITY_MOLECULES, H.ACF_ORIENTATION


@dataclasses.dataclass
class Autocorrelations:
    """Autocorrelations of a per-unit vector per group and lag (Context.acf_read; include/vvhip.h: vvhip_acf_* states the units and their
    vector, the schedule and the terms).  `words` is the device's table as it stands, int64 [groups, lags, 4 or 5]: pairs, then the sums of
    a_x(0) a_x(t), a_y(0) a_y(t), a_z(0) a_z(t) and, in orientation mode, of (u(0).u(t))^2, scaled by 2^frac_bits.  Row 0 is the zero lag."""
    samples: int
    dropped: int                           # samples that were due past max_samples: nothing was added or stored for them
    out_of_range: int                      # unit-pairs left out (a bad vector at either end)
    origin_floor: int                      # origins with an ordinal below it are dead (the velocities were drawn anew)
    interval: int
    origin_every: int
    frac_bits: int
    mode: str                              # "velocity", "molecules" or "orientation"
    words: np.ndarray                      # int64 [groups, lags, 4 | 5]

    @property
    def lag_steps(self) -> np.ndarray:
        """int64 [lags]: row l is the lag of l * interval steps."""
        return np.arange(self.words.shape[1], dtype=np.int64) * self.interval

    @property
    def pairs(self) -> np.ndarray:
        """int64 [groups, lags]: unit-pairs behind every row."""
        return self.words[:, :, 0]

    @property
    def sums(self) -> np.ndarray:
        """float64 [groups, lags, 3]: the sums of a_x(0) a_x(t), a_y(0) a_y(t), a_z(0) a_z(t) = word * 2^-frac_bits."""
        return self.words[:, :, 1:4].astype(np.float64) * 2.0 ** -self.frac_bits

    @property
    def squares(self) -> np.ndarray:
        """float64 [groups, lags]: the sums of (u(0).u(t))^2 (orientation mode)."""
        if self.mode != "orientation":
            raise ValueError("squares are recorded in orientation mode only")
        return self.words[:, :, 4].astype(np.float64) * 2.0 ** -self.frac_bits

    def _per_pair(self, g: int, values: np.ndarray) -> np.ndarray:
        n = self.pairs[int(g)].reshape((-1,) + (1,) * (values.ndim - 1))
        return np.where(n > 0, values / np.where(n > 0, n, 1), np.nan)

    def components(self, g: int) -> np.ndarray:
        """float64 [lags, 3]: <a_x(0) a_x(t)>, <a_y(0) a_y(t)>, <a_z(0) a_z(t)> of group g, NaN where a row has no pairs."""
        return self._per_pair(g, self.sums[int(g)])

    def C(self, g: int) -> np.ndarray:
        """float64 [lags]: <a(0).a(t)> of group g = sum over the components of sums / pairs (velocity modes: nm^2/ps^2)."""
        return self.components(g).sum(axis=1)

    def normalized(self, g: int) -> np.ndarray:
        """float64 [lags]: C(t) / C(0) of group g."""
        c = self.C(g)
        return c / c[0]

    def _velocity_only(self, what):
        if self.mode == "orientation":
            raise ValueError(what + " belongs to the velocity modes")

    def diffusion_green_kubo(self, g: int, dt_ps: float, upto=None) -> float:
        """The Green-Kubo self-diffusion coefficient of group g in nm^2/ps, the unit Msd.diffusion returns: the trapezoid integral of
        C(t) / 3 over the lags 0 .. `upto` (inclusive; None: the whole table), lag time = lag steps x `dt_ps`."""
        self._velocity_only("diffusion_green_kubo")
        last = self.words.shape[1] - 1 if upto is None else int(upto)
        y = self.C(g)[: last + 1] / 3.0
        t = self.lag_steps[: last + 1].astype(np.float64) * float(dt_ps)
        return float(np.sum(0.5 * (y[1:] + y[:-1]) * (t[1:] - t[:-1])))

    def spectrum(self, g: int, dt_ps: float, window: str = "hann"):
        """(frequencies in THz, the cosine transform of C(t) of group g): I(f_m) = 2 h sum'_l w_l C(l h) cos(2 pi f_m l h), h = interval x
        `dt_ps`, the zero lag taken half (the trapezoid of an even function), f_m = m / (2 L h) for m = 0 .. L - 1 with L lags.  `window`:
        "hann" (w_l = cos^2(pi l / (2 L)), one-sided) or None / "none".  The vibrational density of states up to a constant."""
        self._velocity_only("spectrum")
        if window not in ("hann", "none", None):
            raise ValueError("window must be 'hann' or 'none'")
        c = self.C(g)
        L = c.size
        h = float(self.interval) * float(dt_ps)
        l = np.arange(L, dtype=np.float64)
        w = np.cos(np.pi * l / (2.0 * L)) ** 2 if window == "hann" else np.ones(L)
        w[0] *= 0.5
        f = np.arange(L, dtype=np.float64) / (2.0 * L * h)
        return f, 2.0 * h * (np.cos(2.0 * np.pi * np.outer(f, l * h)) * (w * c)).sum(axis=1)

    def P1(self, g: int) -> np.ndarray:
        """float64 [lags]: <u(0).u(t)> of group g (orientation mode)."""
        if self.mode != "orientation":
            raise ValueError("P1 belongs to orientation mode")
        return self.C(g)

    def P2(self, g: int) -> np.ndarray:
        """float64 [lags]: <P2(u(0).u(t))> = (3 squares / pairs - 1) / 2 of group g (orientation mode)."""
        if self.mode != "orientation":
            raise ValueError("P2 belongs to orientation mode")
        return (3.0 * self._per_pair(g, self.squares[int(g)]) - 1.0) / 2.0

    def relaxation_time(self, g: int, l: int, dt: float = 1.0) -> float:
        """The first lag time at which P_l of group g, divided by its zero-lag value, falls below 1 / e, linearly interpolated between
        the two rows around it; NaN if it never does within the table (DensityModes.relaxation_time's time).  `dt`: the step in the unit
        the time is wanted in, as there; the default of 1 gives the time in steps."""
        if int(l) not in (1, 2):
            raise ValueError("l must be 1 or 2")
        y = self.P1(g) if int(l) == 1 else self.P2(g)
        y = y / y[0]
        t = self.lag_steps.astype(np.float64) * float(dt)
        below = np.nonzero(y < np.exp(-1.0))[0]
        if below.size == 0 or below[0] == 0:
            return float("nan")
        i = int(below[0])
        return float(t[i - 1] + (t[i] - t[i - 1]) * (y[i - 1] - np.exp(-1.0)) / (y[i - 1] - y[i]))


def acf_from_words(words, layout, counts) -> Autocorrelations:
    """An Autocorrelations from a table's int64 words [groups * lags * row_words], its layout (H.AcfLayout) and counts (H.AcfCounts)."""
    words = np.ascontiguousarray(words, dtype=np.int64).reshape(int(layout.num_groups), int(layout.num_lags), int(layout.row_words))
    return Autocorrelations(samples=int(counts.samples), dropped=int(counts.dropped), out_of_range=int(counts.out_of_range),
                            origin_floor=int(counts.origin_floor), interval=int(layout.interval), origin_every=int(layout.origin_every),
                            frac_bits=int(layout.frac_bits), mode=ACF_MODES[int(layout.mode)], words=words)


def vanhove_edges(r_max: float, num_bins: int, r_min=None) -> np.ndarray:
    """float64 [num_bins + 1]: bin edges in nm for Context.vanhove_start.  r_min=None: uniform from 0 to r_max, edge k = k * (r_max /
    num_bins); else logarithmic from r_min > 0 to r_max (displacements below r_min are counted in `below`)."""
    if r_min is None:
        return np.arange(int(num_bins) + 1, dtype=np.float64) * (np.float64(r_max) / np.float64(num_bins))
    if not 0 < float(r_min) < float(r_max):
        raise ValueError("logarithmic edges need 0 < r_min < r_max")
    return np.geomspace(np.float64(r_min), np.float64(r_max), int(num_bins) + 1)


@dataclasses.dataclass
class VanHove:
    """The self part of the van Hove function per group and lag (Context.vanhove_read; include/vvhip.h: vvhip_vanhove_* states the units,
    the schedule, the bins and the moments).  `head` and `hist` are the device's table as it stands: int64 [groups, lags, 6] -- pairs,
    below, beyond, sum r2 scaled by 2^frac2_bits, sum r2 r2 as hi and lo -- and int64 [groups, lags, bins]."""
    samples: int
    dropped: int                           # samples that were due past max_samples: nothing was added or stored for them
    out_of_range: int                      # unit-pairs left out (a displacement component NaN or at / beyond the limit)
    origin_floor: int                      # origins with an ordinal below it are dead (a barostat move rewrote the positions)
    interval: int
    origin_every: int
    frac2_bits: int
    r4_hi_bits: int
    r4_lo_bits: int
    molecules: bool
    edges: np.ndarray                      # float64 [bins + 1] nm
    head: np.ndarray                       # int64 [groups, lags, 6]
    hist: np.ndarray                       # int64 [groups, lags, bins]

    @property
    def lag_steps(self) -> np.ndarray:
        """int64 [lags]: row l is the lag of (l + 1) * interval steps."""
        return (np.arange(self.head.shape[1], dtype=np.int64) + 1) * self.interval

    @property
    def pairs(self) -> np.ndarray:
        """int64 [groups, lags]: unit-pairs behind every row = below + hist summed over the bins + beyond."""
        return self.head[:, :, 0]

    @property
    def below(self) -> np.ndarray:
        """int64 [groups, lags]: pairs with r < edges[0]."""
        return self.head[:, :, 1]

    @property
    def beyond(self) -> np.ndarray:
        """int64 [groups, lags]: pairs with r >= edges[-1]."""
        return self.head[:, :, 2]

    def _per_pair(self, values: np.ndarray) -> np.ndarray:
        n = self.pairs.reshape(self.pairs.shape + (1,) * (values.ndim - 2))
        return np.where(n > 0, values / np.where(n > 0, n, 1), np.nan)

    @property
    def P(self) -> np.ndarray:
        """float64 [groups, lags, bins]: the probability of a displacement in every bin = hist / pairs, NaN where a row has no pairs."""
        return self._per_pair(self.hist.astype(np.float64))

    @property
    def G_s(self) -> np.ndarray:
        """float64 [groups, lags, bins]: G_s(r, t) in nm^-3 = P divided by the shell volume 4 pi / 3 (e_{b+1}^3 - e_b^3)."""
        e = self.edges
        return self.P / (4.0 * np.pi / 3.0 * (e[1:] ** 3 - e[:-1] ** 3))

    @property
    def msd(self) -> np.ndarray:
        """float64 [groups, lags]: <r^2> in nm^2 = word * 2^-frac2_bits / pairs (every pair in range, the ones below and beyond too)."""
        return self._per_pair(self.head[:, :, 3].astype(np.float64) * 2.0 ** -self.frac2_bits)

    @property
    def r4(self) -> np.ndarray:
        """float64 [groups, lags]: <r^4> in nm^4 = (hi + lo * 2^-r4_lo_bits) * 2^-r4_hi_bits / pairs."""
        total = (self.head[:, :, 4].astype(np.float64) + self.head[:, :, 5].astype(np.float64) * 2.0 ** -self.r4_lo_bits) * 2.0 ** -self.r4_hi_bits
        return self._per_pair(total)

    @property
    def alpha2(self) -> np.ndarray:
        """float64 [groups, lags]: the non-Gaussian parameter 3 <r^4> / (5 <r^2>^2) - 1 (0 for a Gaussian G_s in three dimensions)."""
        m = self.msd
        return 3.0 * self.r4 / (5.0 * m * m) - 1.0

    def Fs(self, k: float):
        """(F float64 [groups, lags], excluded float64 [groups, lags]): the self-intermediate scattering function at wave number k (nm^-1)
        from the histogram, F = sum_b P_b sin(k r_b) / (k r_b) at the bin midpoints r_b -- limited by the bin width: it is good while
        k * width << 1 --, and the share of the pairs below edges[0] or beyond edges[-1], which are in no bin and not in F."""
        r = 0.5 * (self.edges[1:] + self.edges[:-1])
        F = (self.P * np.sinc(float(k) * r / np.pi)).sum(axis=2)
        return F, self._per_pair((self.below + self.beyond).astype(np.float64))

    def overlap(self, a: float) -> np.ndarray:
        """float64 [groups, lags]: the self-overlap Q_s(t) = the share of the pairs with r < a.  `a` must be one of `edges`: the
        histogram cannot split a bin."""
        at = np.nonzero(self.edges == np.float64(a))[0]
        if at.size == 0:
            raise ValueError(f"overlap: a = {a} is not one of the bin edges")
        inside = self.below + self.hist[:, :, : int(at[0])].sum(axis=2)
        return self._per_pair(inside.astype(np.float64))

    def relaxation_time(self, k: float, level: float = float(np.exp(-1.0)), dt: float = 1.0) -> np.ndarray:
        """float64 [groups]: the first lag time at which Fs(k) falls below `level`, linearly interpolated between the two rows around it
        (the zero lag, where F_s = 1, in front of row 0); NaN if it never does within the table.  `dt`: the step in the unit the time is
        wanted in; the default of 1 gives the time in steps."""
        F, _ = self.Fs(k)
        t = np.concatenate([[0.0], self.lag_steps.astype(np.float64) * float(dt)])
        out = np.full(F.shape[0], np.nan)
        for g in range(F.shape[0]):
            y = np.concatenate([[1.0], F[g]])
            under = np.nonzero(y < level)[0]
            if under.size and under[0] > 0:
                i = int(under[0])
                out[g] = t[i - 1] + (t[i] - t[i - 1]) * (y[i - 1] - level) / (y[i - 1] - y[i])
        return out


def vanhove_from_words(words, layout, counts, edges) -> VanHove:
    """A VanHove from a table's int64 words (head [groups * lags * 6], then hist [groups * lags * bins]), its layout (H.VanHoveLayout),
    counts (H.VanHoveCounts) and the bin edges it was started with."""
    words = np.ascontiguousarray(words, dtype=np.int64)
    G, L, B, hw = int(layout.num_groups), int(layout.num_lags), int(layout.num_bins), int(layout.head_words)
    return VanHove(samples=int(counts.samples), dropped=int(counts.dropped), out_of_range=int(counts.out_of_range),
                   origin_floor=int(counts.origin_floor), interval=int(layout.interval), origin_every=int(layout.origin_every),
                   frac2_bits=int(layout.frac2_bits), r4_hi_bits=int(layout.r4_hi_bits), r4_lo_bits=int(layout.r4_lo_bits),
                   molecules=layout.mode == H.VANHOVE_MOLECULES, edges=np.array(edges, dtype=np.float64),
                   head=words[:hw].reshape(G, L, 6).copy(), hist=words[hw:hw + G * L * B].reshape(G, L, B).copy())


def rdf_edges(r_max: float, nbins: int) -> np.ndarray:
    """float64 [nbins + 1]: the SQUARED bin edges e(k) = ((double) k * dr)^2 with dr = r_max / nbins, as include/vvhip.h defines them."""
    t = np.arange(int(nbins) + 1, dtype=np.float64) * (np.float64(r_max) / np.float64(nbins))
    return t * t


@dataclasses.dataclass
class Rdf:
    """Pair histograms per class and bin (Context.rdf_read; include/vvhip.h: vvhip_rdf_* states the sites, the classes, the arithmetic and
    the bins).  `counts` is the device's table as it stands, int64 [classes, bins]."""
    samples: int
    dropped: int                           # samples that were due past max_samples or in a box too small for r_max: nothing was added
    invalid: int                           # pairs whose squared distance was NaN
    inv_volume_sum: float                  # the counted samples' 1 / V in nm^-3, summed in sample order
    interval: int
    r_max: float
    dr: float
    classes: np.ndarray                    # int32 [classes, 2] the groups of every class
    num_sites: np.ndarray                  # int64 [groups]
    pairs_per_sample: np.ndarray           # int64 [classes]: N_a N_b, or N_a (N_a - 1) / 2 for a class of one group with itself
    counts: np.ndarray                     # int64 [classes, bins]

    @property
    def edges2(self) -> np.ndarray:
        """float64 [bins + 1]: the squared edges e(k) the device compares against."""
        return rdf_edges(self.r_max, self.counts.shape[1])

    @property
    def edges(self) -> np.ndarray:
        """float64 [bins + 1]: the bin edges in nm, sqrt(e(k))."""
        return np.sqrt(self.edges2)

    @property
    def r(self) -> np.ndarray:
        """float64 [bins]: the bin centres in nm."""
        e = self.edges
        return 0.5 * (e[1:] + e[:-1])

    @property
    def shell_volumes(self) -> np.ndarray:
        """float64 [bins]: 4 pi / 3 (e+^3 - e-^3) in nm^3, exact for the edges as they are."""
        e3 = self.edges ** 3
        return 4.0 * np.pi / 3.0 * (e3[1:] - e3[:-1])

    def g(self) -> np.ndarray:
        """float64 [classes, bins]: counts / pairs_per_sample / shell volume / inv_volume_sum -- an ideal gas gives 1; NaN where a class
        has no pair or no sample was counted."""
        pairs = self.pairs_per_sample.astype(np.float64)[:, None]
        norm = pairs * self.shell_volumes[None, :] * self.inv_volume_sum
        return np.where(norm > 0, self.counts / np.where(norm > 0, norm, 1.0), np.nan)

    def coordination(self) -> np.ndarray:
        """float64 [classes, bins]: the running integral up to every bin's outer edge: sites of group b within that distance of a site of
        group a, averaged over the samples and the sites of a (a class of one group with itself counts every pair for both its sites)."""
        na = self.num_sites[self.classes[:, 0]].astype(np.float64)[:, None]
        both = np.where(self.classes[:, 0] == self.classes[:, 1], 2.0, 1.0)[:, None]
        denom = na * float(self.samples)
        return np.where(denom > 0, both * np.cumsum(self.counts, axis=1) / np.where(denom > 0, denom, 1.0), np.nan)


def rdf_from_words(words, layout, counts) -> Rdf:
    """An Rdf from a table's int64 words [classes * bins], its layout (H.RdfLayout) and counts (H.RdfCounts)."""
    nc, ng = int(layout.num_classes), int(layout.num_groups)
    table = np.ascontiguousarray(words, dtype=np.int64).reshape(nc, int(layout.nbins))
    return Rdf(samples=int(counts.samples), dropped=int(counts.dropped), invalid=int(counts.invalid), inv_volume_sum=float(counts.inv_volume_sum),
               interval=int(layout.interval), r_max=float(layout.r_max), dr=float(layout.dr),
               classes=np.array([[layout.classes[c][0], layout.classes[c][1]] for c in range(nc)], dtype=np.int32).reshape(nc, 2),
               num_sites=np.array(layout.num_sites[:ng], dtype=np.int64), pairs_per_sample=np.array(layout.pairs_per_sample[:nc], dtype=np.int64),
               counts=table)


@dataclasses.dataclass
class VanHoveDistinct:
    """The distinct part of the van Hove function per ordered class, lag and bin (Context.vanhove_distinct_read; include/vvhip.h:
    vvhip_vanhove_distinct_* states the sites, the classes, the schedule, the arithmetic and the bins).  `head` and `hist` are the device's
    table as it stands: int64 [rows, 2] -- the visits and the bits of the float64 sum of 1 / V over them -- and int64 [classes, rows, bins];
    row 0 is the sample against itself, row l the lag of l * interval steps."""
    samples: int
    dropped: int                           # samples that were due past max_samples or in a box too small for r_max: nothing was added or stored
    invalid: int                           # pairs whose squared distance was NaN
    origin_floor: int                      # origins with an ordinal below it are dead (the box or the positions were rewritten)
    interval: int
    origin_every: int
    r_max: float
    dr: float
    classes: np.ndarray                    # int32 [classes, 2]: the group at the origin, the group now
    num_sites: np.ndarray                  # int64 [groups]
    pairs_per_sample: np.ndarray           # int64 [classes]: N_a N_b, or N_a (N_a - 1) for a class of one group with itself
    head: np.ndarray                       # int64 [rows, 2]
    hist: np.ndarray                       # int64 [classes, rows, bins]

    @property
    def lag_steps(self) -> np.ndarray:
        """int64 [rows]: row l is the lag of l * interval steps."""
        return np.arange(self.head.shape[0], dtype=np.int64) * self.interval

    @property
    def visits(self) -> np.ndarray:
        """int64 [rows]: the (origin, sample) visits behind every row."""
        return self.head[:, 0]

    @property
    def inv_volume_sum(self) -> np.ndarray:
        """float64 [rows]: 1 / V in nm^-3 summed over the row's visits, in sample order."""
        return np.ascontiguousarray(self.head[:, 1]).view(np.float64)

    @property
    def edges2(self) -> np.ndarray:
        """float64 [bins + 1]: the squared edges e(k) the device compares against."""
        return rdf_edges(self.r_max, self.hist.shape[2])

    @property
    def edges(self) -> np.ndarray:
        """float64 [bins + 1]: the bin edges in nm, sqrt(e(k))."""
        return np.sqrt(self.edges2)

    @property
    def r(self) -> np.ndarray:
        """float64 [bins]: the bin centres in nm."""
        e = self.edges
        return 0.5 * (e[1:] + e[:-1])

    @property
    def shell_volumes(self) -> np.ndarray:
        """float64 [bins]: 4 pi / 3 (e+^3 - e-^3) in nm^3, exact for the edges as they are."""
        e3 = self.edges ** 3
        return 4.0 * np.pi / 3.0 * (e3[1:] - e3[:-1])

    def G_d(self, c: int = 0) -> np.ndarray:
        """float64 [rows, bins]: hist / (P_c * shell volume * inv_volume_sum of the row) -- G_d(r, t) over the mean density of the later
        group, which tends to 1 at large r; NaN where the class has no pair or a row no visit."""
        norm = float(self.pairs_per_sample[c]) * self.shell_volumes[None, :] * self.inv_volume_sum[:, None]
        return np.where(norm > 0, self.hist[c] / np.where(norm > 0, norm, 1.0), np.nan)

    def g(self, c: int = 0) -> np.ndarray:
        """float64 [bins]: row 0 of G_d, the radial distribution function of the class (Rdf.g of the unordered class where ga == gb)."""
        return self.G_d(c)[0]

    def coordination(self, c: int = 0) -> np.ndarray:
        """float64 [rows, bins]: the running integral up to every bin's outer edge: sites of the later group within that distance of where
        a site of the origin group was, averaged over the row's visits and the origin group's sites."""
        denom = float(self.num_sites[self.classes[c, 0]]) * self.visits.astype(np.float64)[:, None]
        return np.where(denom > 0, np.cumsum(self.hist[c], axis=1) / np.where(denom > 0, denom, 1.0), np.nan)


def vanhove_distinct_from_words(words, layout, counts) -> VanHoveDistinct:
    """A VanHoveDistinct from a table's int64 words (head [rows * 2], then hist [classes * rows * bins]), its layout
    (H.VanHoveDistinctLayout) and counts (H.VanHoveDistinctCounts)."""
    words = np.ascontiguousarray(words, dtype=np.int64)
    nc, ng, rows, nb, hw = int(layout.num_classes), int(layout.num_groups), int(layout.num_rows), int(layout.nbins), int(layout.head_words)
    return VanHoveDistinct(samples=int(counts.samples), dropped=int(counts.dropped), invalid=int(counts.invalid),
                           origin_floor=int(counts.origin_floor), interval=int(layout.interval), origin_every=int(layout.origin_every),
                           r_max=float(layout.r_max), dr=float(layout.dr),
                           classes=np.array([[layout.classes[c][0], layout.classes[c][1]] for c in range(nc)], dtype=np.int32).reshape(nc, 2),
                           num_sites=np.array(layout.num_sites[:ng], dtype=np.int64),
                           pairs_per_sample=np.array(layout.pairs_per_sample[:nc], dtype=np.int64),
                           head=words[:hw].reshape(rows, 2).copy(), hist=words[hw:hw + nc * rows * nb].reshape(nc, rows, nb).copy())


@dataclasses.dataclass
class Sdf:
    """Spatial distribution functions per class and voxel (Context.sdf_read; include/vvhip.h: vvhip_sdf_* states the frames, the sites,
    the classes, the arithmetic and the voxels).  `counts` is the device's table as it stands, int64 [classes, n, n, n], indexed by the
    voxel along the frame axes xi1 (o -> a), xi2 (in the plane of o, a, b, on b's side), xi3 = xi1 x xi2."""
    samples: int
    dropped: int                           # samples that were due past max_samples or in a box too small for the cube: nothing was added
    invalid: int                           # pairs of a good frame whose frame coordinates held a NaN
    bad_frames: int                        # (frame, sample) visits whose frame was degenerate: they took part in no pair
    inv_volume_sum: float                  # the counted samples' 1 / V in nm^-3, summed in sample order
    frame_visits: np.ndarray               # int64 [frame groups]: the good frames of the counted samples
    interval: int
    extent: float                          # h in nm: the cube is [-h, h)^3
    classes: np.ndarray                    # int32 [classes, 2]: frame group, site group
    num_frames: np.ndarray                 # int64 [frame groups]
    num_sites: np.ndarray                  # int64 [site groups]
    pairs_per_sample: np.ndarray           # int64 [classes]: N_frames N_sites
    counts: np.ndarray                     # int64 [classes, n, n, n]

    @property
    def nbins(self) -> int:
        return int(self.counts.shape[1])

    @property
    def voxel(self) -> float:
        """The voxel's edge in nm, 2 h / n."""
        return 2.0 * self.extent / self.nbins

    @property
    def edges(self) -> np.ndarray:
        """float64 [n + 1]: the voxel edges along one frame axis in nm, -h .. h."""
        return -self.extent + self.voxel * np.arange(self.nbins + 1, dtype=np.float64)

    @property
    def centres(self) -> np.ndarray:
        """float64 [n]: the voxel centres along one frame axis in nm."""
        e = self.edges
        return 0.5 * (e[1:] + e[:-1])

    def density(self, c: int = 0) -> np.ndarray:
        """float64 [n, n, n] in nm^-3: counts / (frame_visits of the class's frame group * voxel volume) -- the mean number density of
        the class's sites around a frame; NaN where no frame was visited."""
        norm = float(self.frame_visits[self.classes[c, 0]]) * self.voxel ** 3
        return self.counts[c] / norm if norm > 0 else np.full(self.counts[c].shape, np.nan)

    def g(self, c: int = 0) -> np.ndarray:
        """float64 [n, n, n]: density / (N_sites * inv_volume_sum / samples), the density over the mean density of the class's site
        group, which tends to 1 far from the molecule.  The exclusion does not lower N_sites, and the mean density is taken over all
        counted samples while the density counts the good frames only, so with bad frames -- under a barostat -- this is approximate."""
        bulk = float(self.num_sites[self.classes[c, 1]]) * self.inv_volume_sum / self.samples if self.samples > 0 else 0.0
        return self.density(c) / bulk if bulk > 0 else np.full(self.counts[c].shape, np.nan)

    def symmetrized(self, c: int = 0, axes=(2,), quantity: str = "g") -> np.ndarray:
        """float64 [n, n, n]: the mean of `quantity` ("g", "density" or "counts") with its mirror images along the given frame axes (0, 1,
        2 = xi1, xi2, xi3), all 2^len(axes) of them: axes=(2,) for a planar ring, whose two faces are equivalent."""
        out = {"g": self.g, "density": self.density, "counts": lambda k: self.counts[k].astype(np.float64)}[quantity](c)
        for ax in axes:
            out = 0.5 * (out + np.flip(out, axis=int(ax)))
        return out

    def plane(self, c: int = 0, axis: int = 2, lo: float = None, hi: float = None, quantity: str = "g") -> np.ndarray:
        """float64 [n, n]: the mean of `quantity` over the slab of voxels whose centres lie in [lo, hi] nm along frame axis `axis`
        (default: the two central layers, or the central one for odd n) -- a 2-D map over the two remaining axes in their order."""
        out = {"g": self.g, "density": self.density, "counts": lambda k: self.counts[k].astype(np.float64)}[quantity](c)
        x = self.centres
        if lo is None and hi is None:
            lo, hi = -0.75 * self.voxel, 0.75 * self.voxel
        take = (x >= (-np.inf if lo is None else lo)) & (x <= (np.inf if hi is None else hi))
        if not take.any():
            raise ValueError("plane: no voxel centre lies in [lo, hi]")
        return np.take(out, np.nonzero(take)[0], axis=int(axis)).mean(axis=int(axis))


def sdf_from_words(words, layout, counts) -> Sdf:
    """An Sdf from a table's int64 words [classes * n^3], its layout (H.SdfLayout) and counts (H.SdfCounts)."""
    nc, n, nfg, nsg = int(layout.num_classes), int(layout.nbins), int(layout.num_frame_groups), int(layout.num_site_groups)
    return Sdf(samples=int(counts.samples), dropped=int(counts.dropped), invalid=int(counts.invalid), bad_frames=int(counts.bad_frames),
               inv_volume_sum=float(counts.inv_volume_sum), frame_visits=np.array(counts.frame_visits[:nfg], dtype=np.int64),
               interval=int(layout.interval), extent=float(layout.extent),
               classes=np.array([[layout.classes[c][0], layout.classes[c][1]] for c in range(nc)], dtype=np.int32).reshape(nc, 2),
               num_frames=np.array(layout.num_frames[:nfg], dtype=np.int64), num_sites=np.array(layout.num_sites[:nsg], dtype=np.int64),
               pairs_per_sample=np.array(layout.pairs_per_sample[:nc], dtype=np.int64),
               counts=np.ascontiguousarray(words, dtype=np.int64).reshape(nc, n, n, n))


@dataclasses.dataclass
class Contacts:
    """Contact lifetime correlations per class and lag (Context.contacts_read; include/vvhip.h: vvhip_contacts_* states the sites, the
    classes, the contact, the slots and the table).  `words` is the device's table as it stands, int64 [classes, lags, 4]: per lag the
    visits, and the contacts at the origin, at the origin and now, and at every sample from the origin to now, summed over the visits."""
    samples: int
    dropped: int                           # samples that were due past max_samples or in a box too small for the largest cutoff
    invalid: int                           # pairs whose squared distance was NaN
    interval: int
    origin_every: int
    continuous_kept: bool                  # the recorder kept the surviving contacts (word 3)
    classes: np.ndarray                    # int32 [classes, 2] the groups of every class: rows, columns
    rows: np.ndarray                       # int64 [classes] N_a
    cols: np.ndarray                       # int64 [classes] N_b
    r_cut: np.ndarray                      # float64 [classes] nm
    words: np.ndarray                      # int64 [classes, lags, 4]

    @property
    def lag_steps(self) -> np.ndarray:
        """int64 [lags]: the lag of every row in steps, 0 first."""
        return np.arange(self.words.shape[1], dtype=np.int64) * self.interval

    @property
    def origins(self) -> np.ndarray:
        """int64 [lags]: the (origin, sample) pairs every lag has seen (word 0; the same for every class)."""
        return self.words[0, :, 0].copy()

    def _ratio(self, c: int, word: int) -> np.ndarray:
        den = self.words[int(c), :, 1].astype(np.float64)
        return np.where(den > 0, self.words[int(c), :, word] / np.where(den > 0, den, 1.0), np.nan)

    def intermittent(self, c: int) -> np.ndarray:
        """float64 [lags]: C(t) of class c, the fraction of the origins' contacts that are contacts again at t; NaN where no origin had one."""
        return self._ratio(c, 2)

    def continuous(self, c: int) -> np.ndarray:
        """float64 [lags]: S(t) of class c, the fraction of the origins' contacts that held at every sample up to t."""
        if not self.continuous_kept:
            raise ValueError("the recorder was started with continuous=False")
        return self._ratio(c, 3)

    def mean_contacts(self, c: int) -> float:
        """Contacts per row site of class c, averaged over the origins (lag 0); NaN without a sample or a row."""
        den = float(self.words[int(c), 0, 0]) * float(self.rows[int(c)])
        return float(self.words[int(c), 0, 1]) / den if den > 0 else float("nan")

    def _curve(self, c: int, kind: str) -> np.ndarray:
        if kind not in ("intermittent", "continuous"):
            raise ValueError("kind must be 'intermittent' or 'continuous'")
        return self.intermittent(c) if kind == "intermittent" else self.continuous(c)

    def time_to(self, c: int, kind: str = "intermittent", level: float = float(np.exp(-1.0)), dt: float = 1.0) -> float:
        """The first lag time (lag steps x dt) at which the correlation of class c falls below `level`, linearly interpolated between the
        two rows around it; NaN if it never does within the table."""
        y = self._curve(c, kind)
        t = self.lag_steps.astype(np.float64) * float(dt)
        below = np.nonzero(y < level)[0]
        if below.size == 0 or below[0] == 0:
            return float("nan")
        i = int(below[0])
        return float(t[i - 1] + (t[i] - t[i - 1]) * (y[i - 1] - level) / (y[i - 1] - y[i]))

    def lifetime(self, c: int, kind: str = "continuous", dt: float = 1.0) -> float:
        """The trapezoid integral of the correlation of class c over the recorded lags (lag steps x dt): a lower bound of the lifetime
        where the correlation has not decayed within the table."""
        y = self._curve(c, kind)
        t = self.lag_steps.astype(np.float64) * float(dt)
        return float(np.sum(0.5 * (y[1:] + y[:-1]) * (t[1:] - t[:-1])))


def contacts_from_words(words, layout, counts) -> Contacts:
    """A Contacts from a table's int64 words [classes * lags * 4], its layout (H.ContactsLayout) and counts (H.ContactsCounts)."""
    nc = int(layout.num_classes)
    table = np.ascontiguousarray(words, dtype=np.int64).reshape(nc, int(layout.num_lags), 4)
    return Contacts(samples=int(counts.samples), dropped=int(counts.dropped), invalid=int(counts.invalid), interval=int(layout.interval),
                    origin_every=int(layout.origin_every), continuous_kept=bool(layout.continuous),
                    classes=np.array([[layout.classes[c][0], layout.classes[c][1]] for c in range(nc)], dtype=np.int32).reshape(nc, 2),
                    rows=np.array(layout.rows[:nc], dtype=np.int64), cols=np.array(layout.cols[:nc], dtype=np.int64),
                    r_cut=np.array(layout.r_cut[:nc], dtype=np.float64), words=table)


# Conductivity in S/m from e^2 / (nm ps kJ/mol): CODATA 2018 elementary charge (C) and Avogadro constant (1/mol), both exact.
ELEMENTARY_CHARGE = 1.602176634e-19
AVOGADRO = 6.02214076e23
SIEMENS_PER_METRE = ELEMENTARY_CHARGE * ELEMENTARY_CHARGE * AVOGADRO / (1e-9 * 1e-12 * 1e3)


def current_weights(system, molecules: bool = False) -> np.ndarray:
    """float64 [num_atoms]: the weights of a current recorder (include/vvhip.h: vvhip_current_*).  The charges q_i, or with molecules=True
    Q_m m_i / M_m with Q_m and M_m summed in ascending particle index (massless particles: 0), so that sum w_i X_i = sum_m Q_m COM_m."""
    q = np.ascontiguousarray(system.charges, dtype=np.float64)
    if not molecules:
        return q.copy()
    m = np.ascontiguousarray(system.masses, dtype=np.float64)
    mol = np.ascontiguousarray(system.mol_id, dtype=np.int64)
    nmol = int(mol.max()) + 1 if mol.size else 0
    Q = np.bincount(mol, weights=q, minlength=nmol)                  # (sequential float64 sums in ascending particle index)
    M = np.bincount(mol, weights=m, minlength=nmol)
    heavy = (m > 0) & (M[mol] > 0)
    return np.where(heavy, Q[mol] * m / np.where(M[mol] > 0, M[mol], 1.0), 0.0)


@dataclasses.dataclass
class Currents:
    """Collective current correlations per lag (Context.current_read; include/vvhip.h: vvhip_current_* states the sums, the schedule and
    the table).  `words` is the device's table as it stands, int64 [num_lags + 1, 1 + 3 (ND + NC)]: the count, then the bits of the float64
    sums disp[ND][3] and cur[NC][3]; row l is the lag of l * interval steps, row 0 the zero lag."""
    samples: int                           # samples taken, valid or not
    dropped: int                           # samples that were due past max_samples
    out_of_range: int                      # recorded particles found out of range
    invalid_samples: int                   # samples with at least one of them: they add nothing and are no origin
    origin_floor: int                      # origins with an ordinal below it are dead (a barostat move rewrote the positions)
    inv_volume_sum: float                  # the valid samples' 1 / V (nm^-3), summed in sample order
    interval: int
    origin_every: int
    num_groups: int
    frac_bits_position: int
    frac_bits_velocity: int
    words: np.ndarray                      # int64 [num_lags + 1, row_words]

    @property
    def lag_steps(self) -> np.ndarray:
        """int64 [num_lags + 1]: row l is the lag of l * interval steps."""
        return np.arange(self.words.shape[0], dtype=np.int64) * self.interval

    @property
    def count(self) -> np.ndarray:
        """int64 [num_lags + 1]: the time origins behind every row."""
        return self.words[:, 0]

    @property
    def mean_inv_volume(self) -> float:
        """<1 / V> in nm^-3 over the valid samples, NaN without one."""
        valid = self.samples - self.invalid_samples
        return self.inv_volume_sum / valid if valid > 0 else float("nan")

    def _mean(self, first_word: int) -> np.ndarray:
        n = self.count[:, None]
        sums = np.ascontiguousarray(self.words[:, first_word:first_word + 3]).view(np.float64)
        return np.where(n > 0, sums / np.where(n > 0, n, 1), np.nan)

    def displacement(self, g: int, h: int) -> np.ndarray:
        """float64 [num_lags + 1, 3]: <dP_g,a(t) dP_h,a(t)> in (weight nm)^2 for a = x, y, z; symmetric in g, h.  Row 0 is 0."""
        G = self.num_groups
        g, h = (int(g), int(h)) if g <= h else (int(h), int(g))
        if not 0 <= g <= h < G:
            raise ValueError("groups must be in [0, %d)" % G)
        c = g * G - g * (g - 1) // 2 + (h - g)
        return self._mean(1 + 3 * c)

    def correlation(self, g: int, h: int) -> np.ndarray:
        """float64 [num_lags + 1, 3]: <J_g,a(0) J_h,a(t)> in (weight nm/ps)^2 for a = x, y, z; the origin is the first index."""
        G = self.num_groups
        if not (0 <= int(g) < G and 0 <= int(h) < G):
            raise ValueError("groups must be in [0, %d)" % G)
        return self._mean(1 + 3 * (G * (G + 1) // 2 + int(g) * G + int(h)))

    def _per_kt(self, T: float) -> float:
        return SIEMENS_PER_METRE * self.mean_inv_volume / (BOLTZ * float(T))

    def conductivity_einstein_partial(self, T: float, dt: float, fit) -> np.ndarray:
        """float64 [G, G] in S/m: entry (g, h) is the least-squares slope of sum_a <dP_g,a dP_h,a> against the lag time (lag_steps * dt, dt in
        ps) over rows fit = (lo, hi), inclusive, divided by 6 V kB T.  Symmetric; the sum over ALL entries is conductivity_einstein."""
        lo, hi = int(fit[0]), int(fit[1])
        rows = slice(lo, hi + 1)
        t = self.lag_steps[rows].astype(np.float64) * float(dt)
        if t.size < 2:
            raise ValueError("a slope needs at least two lags")
        tc = t - t.mean()
        G = self.num_groups
        out = np.empty((G, G))
        for g in range(G):
            for h in range(g, G):
                y = self.displacement(g, h)[rows].sum(axis=1)
                out[g, h] = out[h, g] = ((y - y.mean()) * tc).sum() / (tc * tc).sum() * self._per_kt(T) / 6.0
        return out

    def conductivity_einstein(self, T: float, dt: float, fit) -> float:
        """The Einstein-Helfand conductivity in S/m: slope / (6 V kB T), the slope of <|dM(t)|^2> summed over all classes, with the weights
        in e, T in K, dt in ps and 1 / V the recorded mean."""
        return float(self.conductivity_einstein_partial(T, dt, fit).sum())

    def conductivity_green_kubo_partial(self, T: float, dt: float, upto: int) -> np.ndarray:
        """float64 [G, G] in S/m: entry (g, h) is the trapezoid of sum_a <J_g,a(0) J_h,a(t)> over rows 0 .. upto against the lag time,
        divided by 3 V kB T.  The sum over all entries is conductivity_green_kubo."""
        upto = int(upto)
        if not 1 <= upto < self.words.shape[0]:
            raise ValueError("upto must be in [1, num_lags]")
        h_t = float(self.interval) * float(dt)
        G = self.num_groups
        out = np.empty((G, G))
        for g in range(G):
            for h in range(G):
                y = self.correlation(g, h)[: upto + 1].sum(axis=1)
                out[g, h] = (0.5 * (y[0] + y[-1]) + y[1:-1].sum()) * h_t * self._per_kt(T) / 3.0
        return out

    def conductivity_green_kubo(self, T: float, dt: float, upto: int) -> float:
        """The Green-Kubo conductivity in S/m: the trapezoid of <J(0) . J(t)> over rows 0 .. upto, summed over all classes, / (3 V kB T)."""
        return float(self.conductivity_green_kubo_partial(T, dt, upto).sum())


def currents_from_words(words, layout, counts) -> Currents:
    """A Currents from a table's int64 words, its layout (H.CurrentLayout) and counts (H.CurrentCounts)."""
    words = np.ascontiguousarray(words, dtype=np.int64).reshape(int(layout.num_lags) + 1, int(layout.row_words))
    return Currents(samples=int(counts.samples), dropped=int(counts.dropped), out_of_range=int(counts.out_of_range),
                    invalid_samples=int(counts.invalid_samples), origin_floor=int(counts.origin_floor),
                    inv_volume_sum=float(counts.inv_volume_sum), interval=int(layout.interval), origin_every=int(layout.origin_every),
                    num_groups=int(layout.num_groups), frac_bits_position=int(layout.frac_bits_position),
                    frac_bits_velocity=int(layout.frac_bits_velocity), words=words)


def modes_in_shells(box, k_max: float, max_per_shell: Optional[int] = None, seed: int = 0) -> np.ndarray:
    """int32 [K, 3]: the integer triples n != 0 of the orthorhombic `box` (nm) with |k| = 2 pi |n / L| <= k_max (1/nm), ONE of every +-pair
    (the first non-zero component is positive), sorted by |n|^2, then by the triple.  max_per_shell thins every |n|^2 shell to at most
    that many triples, drawn without replacement by a generator seeded with (seed, |n|^2), so a shell's choice does not depend on k_max."""
    L = np.asarray(box, dtype=np.float64).reshape(3)
    top = [int(np.floor(float(k_max) * L[a] / (2.0 * np.pi))) for a in range(3)]
    if max(top) > 4095:
        raise ValueError("a mode component beyond 4095: lower k_max")
    axes = [np.arange(-t, t + 1, dtype=np.int64) for t in top]
    n = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    half = (n[:, 0] > 0) | ((n[:, 0] == 0) & (n[:, 1] > 0)) | ((n[:, 0] == 0) & (n[:, 1] == 0) & (n[:, 2] > 0))
    k = 2.0 * np.pi * np.sqrt((((n / L) ** 2)).sum(axis=1))
    n = n[half & (k <= float(k_max))]
    n2 = (n * n).sum(axis=1)
    n = n[np.lexsort((n[:, 2], n[:, 1], n[:, 0], n2))]
    n2 = (n * n).sum(axis=1)
    if max_per_shell is not None:
        keep = []
        for shell in np.unique(n2):
            at = np.nonzero(n2 == shell)[0]
            if at.size > int(max_per_shell):
                at = np.sort(np.random.default_rng([int(seed), int(shell)]).choice(at, int(max_per_shell), replace=False))
            keep.append(at)
        n = n[np.concatenate(keep)] if keep else n
    return np.ascontiguousarray(n, dtype=np.int32)


@dataclasses.dataclass
class DensityModes:
    """Density-mode correlations per lag (Context.modes_read; include/vvhip.h: vvhip_modes_* states the sums, the schedule and the table).
    `words` is the device's table as it stands, int64 [num_lags + 1, 1 + G^2 K]: the count, then the bits of the float64 sums
    cell[g][h][k] of Re rho_g*(0) rho_h(t); row l is the lag of l * interval steps, row 0 the zero lag."""
    samples: int                           # samples taken, valid or not
    dropped: int                           # samples that were due past max_samples
    out_of_range: int                      # recorded particles found out of range
    invalid_samples: int                   # samples with at least one of them: they add nothing and are no origin
    origin_floor: int                      # origins with an ordinal below it are dead (a barostat move rewrote the positions)
    box_sum: np.ndarray                    # float64 [3]: the valid samples' box edges (nm), summed in sample order
    interval: int
    origin_every: int
    num_groups: int
    frac_bits: int
    group_sites: np.ndarray                # int64 [G]: N_g
    modes: Optional[np.ndarray]            # int32 [K, 3] as given to modes_start (None: unknown to this object)
    words: np.ndarray                      # int64 [num_lags + 1, row_words]

    @property
    def num_modes(self) -> int:
        return (self.words.shape[1] - 1) // (self.num_groups * self.num_groups)

    @property
    def lag_steps(self) -> np.ndarray:
        """int64 [num_lags + 1]: row l is the lag of l * interval steps."""
        return np.arange(self.words.shape[0], dtype=np.int64) * self.interval

    @property
    def count(self) -> np.ndarray:
        """int64 [num_lags + 1]: the time origins behind every row."""
        return self.words[:, 0]

    @property
    def mean_box(self) -> np.ndarray:
        """float64 [3]: the mean box edges over the valid samples, NaN without one."""
        valid = self.samples - self.invalid_samples
        return self.box_sum / valid if valid > 0 else np.full(3, np.nan)

    def _cells(self, g: int, h: int) -> np.ndarray:
        G, K = self.num_groups, self.num_modes
        if not (0 <= int(g) < G and 0 <= int(h) < G):
            raise ValueError("groups must be in [0, %d)" % G)
        first = 1 + (int(g) * G + int(h)) * K
        return np.ascontiguousarray(self.words[:, first:first + K]).view(np.float64)

    def F(self, g: int = 0, h: int = 0) -> np.ndarray:
        """float64 [num_lags + 1, K]: <Re rho_g*(0) rho_h(t)> / sqrt(N_g N_h), the origin the first index; NaN where a lag has no origin
        or a group no site."""
        cells = self._cells(g, h)
        n = self.count[:, None].astype(np.float64)
        norm = np.sqrt(float(self.group_sites[int(g)]) * float(self.group_sites[int(h)]))
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where((n > 0) & (norm > 0), cells / n / norm, np.nan)

    def S(self, g: int = 0, h: int = 0) -> np.ndarray:
        """float64 [K]: the static structure factor, row 0 / count / sqrt(N_g N_h)."""
        return self.F(g, h)[0]

    def k_magnitudes(self) -> np.ndarray:
        """float64 [K]: |k| = 2 pi |n / <L>| in 1/nm from the mean box."""
        if self.modes is None:
            raise ValueError("the modes are unknown to this object")
        return 2.0 * np.pi * np.sqrt(((self.modes.astype(np.float64) / self.mean_box) ** 2).sum(axis=1))

    def shells(self) -> np.ndarray:
        """int64 [K]: the shell of every mode, the rank of its |n|^2 among the distinct values."""
        if self.modes is None:
            raise ValueError("the modes are unknown to this object")
        m = self.modes.astype(np.int64)
        return np.unique((m * m).sum(axis=1), return_inverse=True)[1].reshape(-1)

    def shell_average(self, values) -> Tuple[np.ndarray, np.ndarray]:
        """(k [shells], mean [..., shells]): `values` [..., K] (S or F) averaged over the modes of every |n|^2 shell, against the shell's
        mean |k|."""
        sh = self.shells()
        ns = int(sh.max()) + 1 if sh.size else 0
        member = (sh[None, :] == np.arange(ns)[:, None]).astype(np.float64)      # [shells, K]
        per = member.sum(axis=1)
        v = np.asarray(values, dtype=np.float64)
        return member @ self.k_magnitudes() / per, (v[..., None, :] * member).sum(axis=-1) / per

    def relaxation_time(self, g: int, k_shell: int, dt: float = 1.0) -> float:
        """The first lag time (lag steps x dt) at which the shell-averaged F_gg(k, t) / S_gg(k) of shell `k_shell` falls below 1 / e,
        linearly interpolated between the two rows around it; NaN if it never does within the table."""
        y = self.shell_average(self.F(g, g))[1][:, int(k_shell)]
        y = y / y[0]
        t = self.lag_steps.astype(np.float64) * float(dt)
        below = np.nonzero(y < np.exp(-1.0))[0]
        if below.size == 0 or below[0] == 0:
            return float("nan")
        i = int(below[0])
        return float(t[i - 1] + (t[i] - t[i - 1]) * (y[i - 1] - np.exp(-1.0)) / (y[i - 1] - y[i]))


def modes_from_words(words, layout, counts, modes=None) -> DensityModes:
    """A DensityModes from a table's int64 words, its layout (H.ModesLayout), counts (H.ModesCounts) and the modes given at the start."""
    words = np.ascontiguousarray(words, dtype=np.int64).reshape(int(layout.num_lags) + 1, int(layout.row_words))
    G = int(layout.num_groups)
    return DensityModes(samples=int(counts.samples), dropped=int(counts.dropped), out_of_range=int(counts.out_of_range),
                        invalid_samples=int(counts.invalid_samples), origin_floor=int(counts.origin_floor),
                        box_sum=np.array([float(counts.box_sum[a]) for a in range(3)]), interval=int(layout.interval),
                        origin_every=int(layout.origin_every), num_groups=G, frac_bits=int(layout.frac_bits),
                        group_sites=np.array([int(layout.group_sites[g]) for g in range(G)], dtype=np.int64),
                        modes=None if modes is None else np.ascontiguousarray(modes, dtype=np.int32).reshape(-1, 3), words=words)


def _viscosity_of_rows(v_bias, box, cos_acc, inv_mass_total, single):
    """vvhip_calc_viscosity's arithmetic, in its order, on every row (float64, no contraction: the same bits as the C function)."""
    v = v_bias.astype(np.float32).astype(np.float64) if single else v_bias.copy()      # vMaxBuffer is `mixed`
    vol = box[:, 0] * box[:, 1] * box[:, 2]
    k = 2 * 3.1415926 / box[:, 2]
    on = cos_acc != 0
    inv = np.zeros_like(v)
    inv[on] = v[on] * vol[on] * inv_mass_total / cos_acc[on] * k[on] * k[on]
    return np.where(on, v, 0.0), inv


class Context:
    """Device state + force provider around one VVIntegrator.

    force_provider: "tether" (synthetic forces recomputed from the positions before every force
    evaluation, see vvhip_synth_tether_force), "static" (whatever is in the force buffer), or a callable
    ``f(context)`` that fills ``context.force`` on the device.
    """

    def __init__(self, system: SystemSpec, integrator: VVIntegrator, precision: str = "mixed",
                 force_provider="tether", k_tether: float = 1000.0, k_drude: float = 209200.0,
                 random: Optional[np.ndarray] = None, shard: Optional[Tuple[int, int]] = None, device: Optional[int] = None,
                 stream: Optional[int] = None, tune: Optional[dict] = None):
        """tune: {name: value} for vvhip_debug_tune (test hook: launch shape, loaded instead of computed slot words, ...), applied between
        plan creation and binding, on top of the module's DEFAULT_TUNE (which tests patch to reach contexts created elsewhere)."""
        if integrator._context is not None:
            raise H.VVHipError(H.ERR_INVALID, "This Integrator is already bound to a context")   # VVIntegrator.cpp:93-94
        if H.device_count() == 0:
            raise H.VVHipError(H.ERR_NO_DEVICE, "no HIP device visible: the hot path has no CPU fallback")
        if device is not None:
            H.check(H.lib.vvhip_set_device(int(device)), what="hipSetDevice failed")
        self.system, self.integrator, self.precision = system, integrator, precision
        self.force_provider, self.k_tether, self.k_drude = force_provider, float(k_tether), float(k_drude)
        # particles added through the integrator API extend what the system spec lists
        self._particles_ld = list(system.particles_ld) + list(integrator._particlesLD)
        self._image_pairs = list(system.image_pairs) + list(integrator._imagePairs)
        self._electrolyte = list(system.particles_electrolyte) + list(integrator._particlesElectrolyte)
        n = system.num_atoms
        self.shard = (0, n) if shard is None else (int(shard[0]), int(shard[1]))
        self.plan, self.info, self._keep = create_plan(system, integrator, precision, self.shard, self._particles_ld,
                                                       self._image_pairs, self._electrolyte)
        plan = self.plan
        if getattr(system, "virtual_sites", None) and self.info.num_virtual_sites == 0:
            # (in the OpenMM plugin the adapters then keep calling OpenMM's computeVirtualSites; this stand-alone host has no such kernel)
            H.lib.vvhip_plan_destroy(plan)
            self.plan = None
            raise H.VVHipError(H.ERR_UNSUPPORTED,
                               "the System's virtual sites cannot be placed by kernel B (a site on a site, or parents outside the site's wave) "
                               "and this host has no computeVirtualSites of its own")
        for key, value in {**DEFAULT_TUNE, **(tune or {})}.items():
            H.check(H.lib.vvhip_debug_tune(plan, key.encode(), int(value)), plan)

        # ---- device arrays in OpenMM's layouts, shard-local
        R, M = H.REAL[precision], H.MIXED_T[precision]
        b, e = self.shard
        nloc = e - b
        self.nloc = nloc
        velm = np.zeros((nloc, 4), dtype=M)
        velm[:, :3] = system.velocities[b:e]
        m = system.masses[b:e]
        velm[:, 3] = np.where(m != 0, 1.0 / np.where(m != 0, m, 1.0), 0.0)
        posq = np.zeros((nloc, 4), dtype=R)
        posq[:, :3] = system.positions[b:e]
        posq[:, 3] = system.charges[b:e]
        corr = np.zeros((nloc, 4), dtype=R)
        if precision == "mixed":
            corr[:, :3] = system.positions[b:e] - posq[:, :3].astype(np.float64)
        self.padded = padded(n)
        self.velm = H.DeviceArray.from_host(velm)
        self.posq = H.DeviceArray.from_host(posq)
        self.posq_corr = H.DeviceArray.from_host(corr)
        self.site = H.DeviceArray.from_host(posq)
        self.force = H.DeviceArray.from_host(np.zeros(3 * self.padded, dtype=np.int64))
        self.pos_delta = H.DeviceArray.from_host(np.zeros((nloc, 4), dtype=M))
        self._random_injected = random is not None
        if random is None and self.info.num_normal_ld + self.info.num_pairs_ld > 0:
            random = np.random.default_rng(1).standard_normal((1 << 16, 4)).astype(np.float32)   # seed 1
        self.random_host = None if random is None else np.ascontiguousarray(random, dtype=np.float32)
        self.random = None if random is None else H.DeviceArray.from_host(self.random_host)
        self.random_index = 0
        self._own_stream = None
        if stream is None:
            s = C.c_void_p()
            H.check(H.lib.vvhip_stream_create(C.byref(s)), what="hipStreamCreate failed")
            self._own_stream = s.value
            stream = s.value
        self.stream = stream
        buf = H.Buffers(self.velm.ptr, self.posq.ptr, self.posq_corr.ptr if precision == "mixed" else None, self.force.ptr,
                        self.pos_delta.ptr, self.random.ptr if self.random is not None else None,
                        0 if self.random is None else self.random_host.shape[0], stream)
        H.check(H.lib.vvhip_bind(plan, C.byref(buf)), plan)
        box = (C.c_double * 3)(*[float(x) for x in system.box])
        H.check(H.lib.vvhip_set_box(plan, C.byref(box)), plan)
        self._box = np.array(box, dtype=np.float64)
        self.forces_valid = False
        integrator._context = self

    # ---- state access (blocking)
    def synchronize(self):
        H.check(H.lib.vvhip_synchronize(self.plan), self.plan)

    def getVelm(self): self.synchronize(); return self.velm.download()
    def getPosq(self): self.synchronize(); return self.posq.download()
    def getPosqCorrection(self): self.synchronize(); return self.posq_corr.download()
    def getForce(self): self.synchronize(); return self.force.download()

    def getPositions(self):
        p = self.getPosq()[:, :3].astype(np.float64)
        if self.precision == "mixed":
            p = p + self.getPosqCorrection()[:, :3].astype(np.float64)
        return p

    def getVelocities(self): return self.getVelm()[:, :3].astype(np.float64)

    def setVelocities(self, v):
        velm = self.getVelm()
        velm[:, :3] = v
        self.velm.upload(velm)
        self.forces_valid = False                               # VVIntegrator.h:447-449 stateChanged

    def setVelocitiesToTemperature(self, temperature, randomSeed=None, drude_temperature=None, remove_cm=False,
                                   constraints=True) -> H.ThermalizeRecord:
        """Maxwell-Boltzmann velocities at `temperature` [K] for this context's particles, drawn on the device
        (include/vvhip.h: vvhip_set_velocities_to_temperature): OpenMM's Context.setVelocitiesToTemperature(temperature, randomSeed).
        randomSeed=None takes the integrator's getRandomNumberSeed().  drude_temperature=None is OpenMM's meaning (every massive particle
        at `temperature`); a value >= 0 draws each Drude pair's centre of mass at `temperature` and its relative motion at
        drude_temperature.  The plan's in-kernel velocity constraints are applied to the draw unless constraints=False; remove_cm=True
        then removes the centre-of-mass velocity once.  A function of (seed, global particle index, masses, temperatures) alone, so the
        shards of a sharded run draw their own particles.  Blocks; returns the record."""
        seed = self.integrator.getRandomNumberSeed() if randomSeed is None else randomSeed
        flags = (0 if constraints else H.THERMALIZE_NO_CONSTRAINTS) | (H.THERMALIZE_REMOVE_CM if remove_cm else 0)
        out = H.ThermalizeRecord()
        H.check(H.lib.vvhip_set_velocities_to_temperature(self.plan, float(temperature), -1.0 if drude_temperature is None else float(drude_temperature),
                                                          int(seed) & 0xFFFFFFFFFFFFFFFF, flags, C.byref(out)), self.plan)
        self.forces_valid = False                               # VVIntegrator.h:447-449 stateChanged
        return out

    def getKineticEnergy(self) -> float:
        """1/2 sum m v^2 [kJ/mol] (what State.getKineticEnergy() returns through VVIntegrator::computeKineticEnergy)."""
        ke = C.c_double()
        H.check(H.lib.vvhip_compute_kinetic_energy(self.plan, C.byref(ke)), self.plan)
        return ke.value

    def getGroupTemperatures(self):
        """Temperatures of the thermostat groups [atom, COM, Drude] at the last thermostat application: 2KE_g / (dof_g kB) --
        the quantities examples/ommhelper/reporter/drudetemperaturereporter.py:98-133 recomputes on the host in NumPy."""
        st = self.getNHState()
        kb = 8.31446261815324e-3
        return [st.ke2[g] / (self.info.dof[g] * kb) if self.info.dof[g] > 0 else 0.0 for g in range(3)]

    def getDrudeTemperatures(self):
        """(KE_COM, KE_Atom, KE_Drude, T_COM, T_Atom, T_Drude) in kJ/mol and K of the current velocities, over all particles, as
        examples/ommhelper/reporter/drudetemperaturereporter.py defines them (include/vvhip.h: vvhip_drude_temperatures).  T_Drude is 0
        for a System without Drude pairs.  A shard reports its own particles' energies: see distributed.drude_temperatures."""
        ke, t = (C.c_double * 3)(), (C.c_double * 3)()
        H.check(H.lib.vvhip_drude_temperatures(self.plan, C.byref(ke), C.byref(t)), self.plan)
        return tuple(ke) + tuple(t)

    def drude_report_raw(self) -> np.ndarray:
        """The report's raw fixed-point sums (int64[6]) of this plan's particles: what the shards add up (vvhip_drude_report_raw)."""
        raw = (C.c_int64 * 6)()
        H.check(H.lib.vvhip_drude_report_raw(self.plan, C.byref(raw)), self.plan)
        return np.array(raw, dtype=np.int64)

    def drude_report_combine(self, raw) -> tuple:
        """The six numbers of getDrudeTemperatures from raw sums (one shard's, or the sum over all shards)."""
        r = (C.c_int64 * 6)(*[int(x) for x in raw])
        ke, t = (C.c_double * 3)(), (C.c_double * 3)()
        H.check(H.lib.vvhip_drude_report_combine(self.plan, C.byref(r), C.byref(ke), C.byref(t)), self.plan)
        return tuple(ke) + tuple(t)

    # ---- series: samples recorded on the device inside the steps (include/vvhip.h: vvhip_series_*)
    def series_start(self, interval: int, capacity: int = 4096, drude: bool = True, thermostat: bool = True):
        """Record a row after every step whose number is a multiple of `interval` (steps counted since the context was made, through _step,
        run_eager and run_graph alike; run_eager_unfused takes no rows), into a device buffer of `capacity` rows.  No host synchronisation
        until series_read.  Restarting drops what was recorded."""
        mask = (H.SERIES_DRUDE if drude else 0) | (H.SERIES_THERMOSTAT if thermostat else 0)
        H.check(H.lib.vvhip_series_start(self.plan, int(interval), int(capacity), mask), self.plan)

    def series_stop(self):
        H.check(H.lib.vvhip_series_stop(self.plan), self.plan)

    def series_info(self) -> H.SeriesLayout:
        out = H.SeriesLayout()
        H.check(H.lib.vvhip_series_info(self.plan, C.byref(out)), self.plan)
        return out

    def series_read(self, reset: bool = False, combine=None) -> Series:
        """The rows recorded so far (synchronises).  reset=True empties the buffer; the series then continues without gap or repeat.
        `combine`: raw int64 [n, 7] (six sums + overflow flag) -> the same with the shards' words added (distributed.drude_temperature_series)."""
        info = self.series_info()
        rows = (H.SeriesRow * info.capacity)()
        n, first, dropped = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        H.check(H.lib.vvhip_series_read(self.plan, rows, info.capacity, C.byref(n), C.byref(first), C.byref(dropped), int(bool(reset))), self.plan)
        a = np.ctypeslib.as_array(rows)[: n.value]
        out = Series(step=first.value + info.interval * np.arange(n.value, dtype=np.int64), dropped=int(dropped.value))
        if info.mask & H.SERIES_DRUDE:
            words = np.concatenate([a["drude_raw"], a["drude_overflow"][:, None]], axis=1).astype(np.int64)
            if combine is not None:
                words = np.asarray(combine(words), dtype=np.int64)
            out.raw, out.ok = words[:, :6].copy(), words[:, 6] == 0
            out.ke, out.t = np.full((n.value, 3), np.nan), np.full((n.value, 3), np.nan)
            for j in range(n.value):
                if out.ok[j]:
                    r = self.drude_report_combine(out.raw[j])
                    out.ke[j], out.t[j] = r[:3], r[3:]
        if info.mask & H.SERIES_THERMOSTAT:
            nh = a["nh"]
            for f in ("eta", "eta_dot", "eta_dotdot", "ke2", "vscale", "v_bias"):
                setattr(out, f, np.array(nh[f], dtype=np.float64))
            out.box, out.cos_acceleration = np.array(a["box"], dtype=np.float64), np.array(a["cos_acceleration"], dtype=np.float64)
            out.v_max, out.inv_viscosity = _viscosity_of_rows(out.v_bias, out.box, out.cos_acceleration, self.info.inv_mass_total,
                                                              self.precision == "single")
        return out

    # ---- frames: the trajectory recorded on the device inside the steps (include/vvhip.h: vvhip_frames_*)
    def frames_start(self, interval: int, capacity: int = 64, logarithmic: bool = False, subset=None, velocities: bool = False,
                     float64: bool = False, positions: bool = True):
        """Record the positions (and velocities) of this context's particles, or of those of `subset` (global indices, strictly ascending),
        after every step the schedule names -- steps counted as for the series; every `interval`-th one, or with logarithmic=True
        GroReporter(logarithm=True)'s schedule (interval 30: 30, 40, ..., 100, 200, ..., 1000, 2000, ...) -- into a device buffer of
        `capacity` frames.  No host synchronisation until frames_read.  Restarting drops what was recorded."""
        sub = None if subset is None else np.ascontiguousarray(subset, dtype=np.int32).reshape(-1)
        if sub is not None and sub.size == 0:
            raise ValueError("an empty subset records nothing: pass None for every particle")
        mask = (H.FRAMES_POSITIONS if positions else 0) | (H.FRAMES_VELOCITIES if velocities else 0) | (H.FRAMES_FLOAT64 if float64 else 0)
        desc = H.FramesDesc(int(interval), H.FRAMES_LOG10 if logarithmic else H.FRAMES_LINEAR, int(capacity), mask,
                            0 if sub is None else sub.size, None if sub is None else sub.ctypes.data)
        H.check(H.lib.vvhip_frames_start(self.plan, C.byref(desc)), self.plan)

    def frames_stop(self):
        H.check(H.lib.vvhip_frames_stop(self.plan), self.plan)

    def frames_info(self) -> H.FramesLayout:
        out = H.FramesLayout()
        H.check(H.lib.vvhip_frames_info(self.plan, C.byref(out)), self.plan)
        return out

    def frames_read(self, reset: bool = False) -> Frames:
        """The frames recorded so far (synchronises).  reset=True empties the buffer; the recorder then continues without gap or repeat."""
        info = self.frames_info()
        n, dropped = C.c_int32(0), C.c_int64(0)
        H.check(H.lib.vvhip_frames_read(self.plan, None, None, 0, C.byref(n), C.byref(dropped), 0), self.plan)      # (how many there are)
        count, m, fb = n.value, info.num_particles, info.frame_bytes
        raw = np.zeros(max(count, 1) * fb, dtype=np.uint8)
        step = np.zeros(max(count, 1), dtype=np.int64)
        H.check(H.lib.vvhip_frames_read(self.plan, raw.ctypes.data, step.ctypes.data, count, C.byref(n), C.byref(dropped), int(bool(reset))), self.plan)
        assert n.value == count, (n.value, count)       # (nothing runs between the two calls)
        raw = raw[: count * fb].reshape(count, fb)
        dtype = np.float64 if info.component_bytes == 8 else np.float32

        def planes(off):
            if off < 0:
                return None
            a = raw[:, off: off + 3 * info.plane_stride * info.component_bytes].copy().view(dtype).reshape(count, 3, info.plane_stride)
            return np.ascontiguousarray(a[:, :, :m].transpose(0, 2, 1))

        particles = np.zeros(m, dtype=np.int32)
        H.check(H.lib.vvhip_frames_particles(self.plan, particles.ctypes.data if m else None, m), self.plan)
        box = raw[:, 16:40].copy().view(np.float64).reshape(count, 3)
        return Frames(step=step[:count].copy(), box=box, particles=particles, positions=planes(info.off_positions),
                      velocities=planes(info.off_velocities), dropped=int(dropped.value))

    # ---- what the ten accumulating recorders below share: profile, msd, acf, vanhove, vanhove_distinct, rdf, sdf, contacts, current, modes (include/vvhip.h: vvhip_<name>_*)
    def _groups(self, groups):
        """`groups` as the int8 array the descriptions point to (keep it alive across the call), None for None."""
        if groups is None:
            return None
        grp = np.ascontiguousarray(groups, dtype=np.int8).reshape(-1)
        if grp.size != self.system.num_atoms:
            raise ValueError("groups must have one entry per particle of the System")
        return grp

    def _recorder_stop(self, name):
        H.check(getattr(H.lib, f"vvhip_{name}_stop")(self.plan), self.plan)

    def _recorder_info(self, name, layout):
        out = layout()
        H.check(getattr(H.lib, f"vvhip_{name}_info")(self.plan, C.byref(out)), self.plan)
        return out

    def _recorder_read(self, name, layout, counts, from_words, reset, *more):
        info, counts = self._recorder_info(name, layout), counts()
        words = np.zeros(max(int(info.words), 1), dtype=np.int64)
        H.check(getattr(H.lib, f"vvhip_{name}_read")(self.plan, words.ctypes.data, words.size, C.byref(counts), int(bool(reset))), self.plan)
        return from_words(words[: info.words], info, counts, *more)

    # ---- profiles: density and velocity profiles accumulated on the device inside the steps (include/vvhip.h: vvhip_profile_*)
    def profile_start(self, interval: int, nbins: int, axis: int = 2, groups=None, charge: bool = True, mass: bool = False,
                      momentum: bool = False, kinetic: bool = False, max_samples: int = 1 << 20, limits=None):
        """Add, after every step whose number is a multiple of `interval` (steps counted as for the series), every recorded particle to
        its bin of `nbins` along box axis `axis`: its count and, as asked, charge, mass, momentum (three rows) and m |v|^2, as fixed-point
        integers, so that the table is the same bits for any launch shape or shard split.  `groups`: one int per particle of the System
        (-1: not recorded), each group a table of its own; None: everything in group 0.  `limits`: {"charge" | "mass" | "momentum" |
        "kinetic": largest |term|}; a particle beyond one is left out of every row and counted in out_of_range.  At most `max_samples`
        samples are added (the fixed point is sized for them).  No host synchronisation until profile_read."""
        grp = self._groups(groups)
        unknown = set(limits or {}) - set(H.PROFILE_QUANTITIES[1:])
        if unknown:
            raise ValueError(f"limits: unknown quantity {sorted(unknown)}")
        mask = (H.PROFILE_COUNT | (H.PROFILE_CHARGE if charge else 0) | (H.PROFILE_MASS if mass else 0) | (H.PROFILE_MOMENTUM if momentum else 0)
                | (H.PROFILE_KINETIC if kinetic else 0))
        desc = H.ProfileDesc(int(interval), int(axis), int(nbins), mask, 1 if grp is None else max(int(grp.max()) + 1, 1), 0,
                             None if grp is None else grp.ctypes.data, int(max_samples),
                             (C.c_double * 4)(*[float((limits or {}).get(q, 0.0)) for q in H.PROFILE_QUANTITIES[1:]]))
        H.check(H.lib.vvhip_profile_start(self.plan, C.byref(desc)), self.plan)

    def profile_stop(self):
        self._recorder_stop("profile")

    def profile_info(self) -> H.ProfileLayout:
        return self._recorder_info("profile", H.ProfileLayout)

    def profile_read(self, reset: bool = False) -> Profile:
        """The table accumulated so far (synchronises).  reset=True zeroes it; the schedule continues without gap or repeat."""
        return self._recorder_read("profile", H.ProfileLayout, H.ProfileCounts, profile_from_words, reset, self._box)

    # ---- mean-squared displacements accumulated on the device inside the steps (include/vvhip.h: vvhip_msd_*)
    def msd_start(self, interval: int, num_lags: int, origin_every: int = 1, molecules: bool = False, groups=None,
                  max_samples: int = 1 << 20, limit: float = 0.0):
        """After every step whose number is a multiple of `interval` (steps counted as for the series), measure every recorded unit -- a
        particle, or with molecules=True a molecule's centre of mass -- against the stored origins and add, per group and lag of 1 ..
        `num_lags` samples, the pair count and dx^2, dy^2, dz^2 as fixed-point integers, so that the table is the same bits for any launch
        shape or shard split.  Every `origin_every`-th sample is stored as an origin.  `groups`: one int per particle of the System (-1:
        not recorded), each group a table of its own; None: everything in group 0.  `limit` (nm, 0: 64): a displacement component at or
        beyond it leaves the pair out and counts in out_of_range.  At most `max_samples` samples are taken (the fixed point is sized for
        them).  No host synchronisation until msd_read."""
        grp = self._groups(groups)
        desc = H.MsdDesc(int(interval), int(num_lags), int(origin_every), H.MSD_MOLECULES if molecules else H.MSD_PARTICLES,
                         1 if grp is None else max(int(grp.max()) + 1, 1), 0, None if grp is None else grp.ctypes.data, int(max_samples),
                         float(limit))
        H.check(H.lib.vvhip_msd_start(self.plan, C.byref(desc)), self.plan)

    def msd_stop(self):
        self._recorder_stop("msd")

    def msd_info(self) -> H.MsdLayout:
        return self._recorder_info("msd", H.MsdLayout)

    def msd_read(self, reset: bool = False) -> Msd:
        """The table accumulated so far (synchronises).  reset=True zeroes it and restarts the sample ordinal with no live origin; the step
        schedule continues without gap or repeat."""
        return self._recorder_read("msd", H.MsdLayout, H.MsdCounts, msd_from_words, reset)

    # ---- velocity and orientation autocorrelations accumulated on the device inside the steps (include/vvhip.h: vvhip_acf_*)
    def acf_start(self, interval: int, num_lags: int, origin_every: int = 1, mode: str = "velocity", groups=None, pairs=None,
                  max_samples: int = 1 << 20, limit: float = 0.0):
        """After every step whose number is a multiple of `interval` (steps counted as for the series), correlate every recorded unit's
        vector -- mode "velocity": a particle's velocity; "molecules": a molecule's centre-of-mass velocity; "orientation": the unit vector
        from tail to head of every pair of `pairs` ([n, 2] particle indices, head first, both in one molecule) -- with the stored origins
        and add, per group and lag of 0 .. `num_lags` - 1 samples, the pair count and the three products (in orientation mode also the
        squared cosine) as fixed-point integers, so that the table is the same bits for any launch shape or shard split.  Every
        `origin_every`-th sample is an origin.  `groups`: one int per particle of the System -- in orientation mode one per pair -- (-1:
        not recorded), each group a table of its own; None: everything in group 0.  `limit` (velocity modes; nm/ps, 0: 64): a velocity
        component at or beyond it makes the vector bad; a pair with a bad vector at either end is left out and counts in out_of_range.  At
        most `max_samples` samples are taken.  setVelocitiesToTemperature kills the origins stored so far in the velocity modes; host
        uploads of velocities or positions are not detected.  No host synchronisation until acf_read."""
        if mode not in ACF_MODES:
            raise ValueError("mode must be 'velocity', 'molecules' or 'orientation'")
        pr = None
        if mode == "orientation":
            if pairs is None:
                raise ValueError("orientation mode needs pairs")
            pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
            grp = None if groups is None else np.ascontiguousarray(groups, dtype=np.int8).reshape(-1)
            if grp is not None and grp.size != pr.shape[0]:
                raise ValueError("groups must have one entry per pair in orientation mode")
        else:
            if pairs is not None:
                raise ValueError("pairs belong to orientation mode")
            grp = self._groups(groups)
        num_groups = 1 if grp is None or grp.size == 0 else max(int(grp.max()) + 1, 1)
        desc = H.AcfDesc(int(interval), int(num_lags), int(origin_every), ACF_MODES.index(mode), num_groups, 0 if pr is None else int(pr.shape[0]),
                         None if grp is None else grp.ctypes.data, None if pr is None or pr.size == 0 else pr.ctypes.data, int(max_samples), float(limit))
        H.check(H.lib.vvhip_acf_start(self.plan, C.byref(desc)), self.plan)

    def acf_stop(self):
        self._recorder_stop("acf")

    def acf_info(self) -> H.AcfLayout:
        return self._recorder_info("acf", H.AcfLayout)

    def acf_read(self, reset: bool = False) -> Autocorrelations:
        """The table accumulated so far (synchronises).  reset=True zeroes it and restarts the sample ordinal with no live origin; the step
        schedule continues without gap or repeat."""
        return self._recorder_read("acf", H.AcfLayout, H.AcfCounts, acf_from_words, reset)

    # ---- self van Hove functions accumulated on the device inside the steps (include/vvhip.h: vvhip_vanhove_*)
    def vanhove_start(self, interval: int, num_lags: int, edges, origin_every: int = 1, molecules: bool = False, groups=None,
                      max_samples: int = 1 << 20, limit: float = 0.0):
        """After every step whose number is a multiple of `interval` (steps counted as for the series), measure every recorded unit -- a
        particle, or with molecules=True a molecule's centre of mass -- against the stored origins and add, per group and lag of 1 ..
        `num_lags` samples, the pair to the bin of its displacement r between `edges` (nm, ascending, edges[0] >= 0: vanhove_edges gives
        uniform or logarithmic ones) and r^2 and r^4 to the row's moments, all as integers, so that the table is the same bits for any
        launch shape or shard split.  Every `origin_every`-th sample is stored as an origin.  `groups`: one int per particle of the System
        (-1: not recorded), each group a table of its own; None: everything in group 0.  `limit` (nm, 0: 16): a displacement component at
        or beyond it leaves the pair out and counts in out_of_range.  At most `max_samples` samples are taken (the fixed point is sized
        for them).  No host synchronisation until vanhove_read."""
        grp = self._groups(groups)
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        desc = H.VanHoveDesc(int(interval), int(num_lags), int(origin_every), H.VANHOVE_MOLECULES if molecules else H.VANHOVE_PARTICLES,
                             1 if grp is None else max(int(grp.max()) + 1, 1), int(e.size) - 1, None if grp is None else grp.ctypes.data,
                             e.ctypes.data if e.size else None, int(max_samples), float(limit))
        H.check(H.lib.vvhip_vanhove_start(self.plan, C.byref(desc)), self.plan)
        self._vanhove_edges = e.copy()

    def vanhove_stop(self):
        self._recorder_stop("vanhove")

    def vanhove_info(self) -> H.VanHoveLayout:
        return self._recorder_info("vanhove", H.VanHoveLayout)

    def vanhove_read(self, reset: bool = False) -> VanHove:
        """The table accumulated so far (synchronises).  reset=True zeroes it and restarts the sample ordinal with no live origin; the step
        schedule continues without gap or repeat."""
        return self._recorder_read("vanhove", H.VanHoveLayout, H.VanHoveCounts, vanhove_from_words, reset, getattr(self, "_vanhove_edges", None))

    # ---- distinct van Hove functions accumulated on the device inside the steps (include/vvhip.h: vvhip_vanhove_distinct_*)
    def vanhove_distinct_start(self, interval: int, num_lags: int, r_max: float, nbins: int, classes, origin_every: int = 1, groups=None,
                               exclude_same_molecule: bool = False, max_samples: int = 1 << 20):
        """After every step whose number is a multiple of `interval` (steps counted as for the series), histogram, for every class and
        every stored origin that is alive, the minimum-image distances between where the sites of the class's first group were at the
        origin and where the sites of its second group are now, into `nbins` bins of width r_max / nbins (nm), in row l = the lag in
        samples (0 .. `num_lags`; row 0 is the sample against itself), as integers, so that the table is the same bits for any launch
        shape.  Every `origin_every`-th sample is stored as an origin.  `groups`: one int per particle of the System (-1: no site);
        None: everything in group 0.  `classes`: ORDERED pairs of groups (ga at the origin, gb now); ga == gb counts every ordered pair of
        two different sites.  exclude_same_molecule leaves out the pairs inside one molecule.  r_max must not exceed half the shortest
        box edge.  A sharded context raises ERR_UNSUPPORTED.  No host synchronisation until vanhove_distinct_read."""
        grp = self._groups(groups)
        cls = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1, 2)
        num_groups = max(1, 0 if grp is None else int(grp.max()) + 1, int(cls.max()) + 1 if cls.size else 1)      # (a class may name a group without sites)
        desc = H.VanHoveDistinctDesc(int(interval), int(num_lags), int(origin_every), int(nbins), num_groups, int(cls.shape[0]),
                                     int(bool(exclude_same_molecule)), 0, None if grp is None else grp.ctypes.data, cls.ctypes.data,
                                     int(max_samples), float(r_max))
        H.check(H.lib.vvhip_vanhove_distinct_start(self.plan, C.byref(desc)), self.plan)

    def vanhove_distinct_stop(self):
        self._recorder_stop("vanhove_distinct")

    def vanhove_distinct_info(self) -> H.VanHoveDistinctLayout:
        return self._recorder_info("vanhove_distinct", H.VanHoveDistinctLayout)

    def vanhove_distinct_read(self, reset: bool = False) -> VanHoveDistinct:
        """The table accumulated so far (synchronises).  reset=True zeroes it and restarts the sample ordinal with no live origin; the step
        schedule continues without gap or repeat."""
        return self._recorder_read("vanhove_distinct", H.VanHoveDistinctLayout, H.VanHoveDistinctCounts, vanhove_distinct_from_words, reset)

    # ---- radial distribution functions accumulated on the device inside the steps (include/vvhip.h: vvhip_rdf_*)
    def rdf_start(self, interval: int, r_max: float, nbins: int, classes, groups=None, exclude_same_molecule: bool = False,
                  max_samples: int = 1 << 20):
        """After every step whose number is a multiple of `interval` (steps counted as for the series), histogram the minimum-image
        distances of every pair of sites of every class into `nbins` bins of width r_max / nbins (nm), as integers, so that the table is
        the same bits for any launch shape.  `groups`: one int per particle of the System (-1: no site); None: everything in group 0.
        `classes`: pairs of groups (ga, gb); ga == gb counts every unordered pair of the group once.  exclude_same_molecule leaves out the
        pairs inside one molecule.  r_max must not exceed half the shortest box edge.  At most `max_samples` samples are taken.  A sharded
        context raises ERR_UNSUPPORTED.  No host synchronisation until rdf_read."""
        grp = self._groups(groups)
        cls = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1, 2)
        num_groups = max(1, 0 if grp is None else int(grp.max()) + 1, int(cls.max()) + 1 if cls.size else 1)      # (a class may name a group without sites)
        desc = H.RdfDesc(int(interval), int(nbins), num_groups, int(cls.shape[0]),
                         int(bool(exclude_same_molecule)), 0, None if grp is None else grp.ctypes.data, cls.ctypes.data, int(max_samples),
                         float(r_max))
        H.check(H.lib.vvhip_rdf_start(self.plan, C.byref(desc)), self.plan)

    def rdf_sample(self):
        """One sample now, behind what is queued, whatever the schedule says (a configuration the host has just uploaded)."""
        H.check(H.lib.vvhip_rdf_sample(self.plan), self.plan)

    def rdf_stop(self):
        self._recorder_stop("rdf")

    def rdf_info(self) -> H.RdfLayout:
        return self._recorder_info("rdf", H.RdfLayout)

    def rdf_read(self, reset: bool = False) -> Rdf:
        """The histograms accumulated so far (synchronises).  reset=True zeroes counts and table; the step schedule continues without gap
        or repeat."""
        return self._recorder_read("rdf", H.RdfLayout, H.RdfCounts, rdf_from_words, reset)

    # ---- spatial distribution functions accumulated on the device inside the steps (include/vvhip.h: vvhip_sdf_*)
    def sdf_start(self, interval: int, extent: float, nbins: int, frames, classes, frame_groups=None, site_groups=None,
                  exclude_same_molecule: bool = False, max_samples: int = 1 << 20):
        """After every step whose number is a multiple of `interval` (steps counted as for the series), count where the sites sit around
        every frame in the frame's own axes, into `nbins`^3 voxels of the cube [-extent, extent)^3 nm, as integers, so that the table is
        the same bits for any launch shape.  `frames`: triplets (o, a, b) of particles of one molecule -- the origin, xi1 points to a, b
        fixes the xi1-xi2 plane; `frame_groups`: one int per frame (-1: not recorded; None: all in group 0); `site_groups`: one int per
        particle of the System (-1: no site; None: everything in group 0); `classes`: pairs (frame group, site group).
        exclude_same_molecule leaves out the sites of the frame's own molecule.  3 extent^2 must stay below (half the shortest box
        edge)^2.  At most `max_samples` samples are taken.  A sharded context raises ERR_UNSUPPORTED.  No host synchronisation until
        sdf_read."""
        fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1, 3)
        fgrp = None if frame_groups is None else np.ascontiguousarray(frame_groups, dtype=np.int8).reshape(-1)
        if fgrp is not None and fgrp.size != fr.shape[0]:
            raise ValueError("frame_groups must have one entry per frame")
        sgrp = self._groups(site_groups)
        cls = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1, 2)
        count = lambda grp, col: max(1, 0 if grp is None or not grp.size else int(grp.max()) + 1, int(cls[:, col].max()) + 1 if cls.size else 1)      # (a class may name a group without members)
        desc = H.SdfDesc(int(interval), int(nbins), int(fr.shape[0]), count(fgrp, 0), count(sgrp, 1), int(cls.shape[0]),
                         int(bool(exclude_same_molecule)), 0, fr.ctypes.data if fr.size else None, None if fgrp is None else fgrp.ctypes.data,
                         None if sgrp is None else sgrp.ctypes.data, cls.ctypes.data, int(max_samples), float(extent))
        H.check(H.lib.vvhip_sdf_start(self.plan, C.byref(desc)), self.plan)

    def sdf_sample(self):
        """One sample now, behind what is queued, whatever the schedule says (a configuration the host has just uploaded)."""
        H.check(H.lib.vvhip_sdf_sample(self.plan), self.plan)

    def sdf_stop(self):
        self._recorder_stop("sdf")

    def sdf_info(self) -> H.SdfLayout:
        return self._recorder_info("sdf", H.SdfLayout)

    def sdf_read(self, reset: bool = False) -> Sdf:
        """The table accumulated so far (synchronises).  reset=True zeroes counts and table; the step schedule continues without gap or
        repeat."""
        return self._recorder_read("sdf", H.SdfLayout, H.SdfCounts, sdf_from_words, reset)

    # ---- contact lifetime correlations accumulated on the device inside the steps (include/vvhip.h: vvhip_contacts_*)
    def contacts_start(self, interval: int, num_lags: int, classes, r_cut, origin_every: int = 1, groups=None,
                       exclude_same_molecule: bool = False, continuous: bool = True, max_samples: int = 1 << 20):
        """After every step whose number is a multiple of `interval` (steps counted as for the series), build the contact matrix of every
        class -- `classes`: ordered pairs of groups (rows, columns), `r_cut`: one cutoff in nm per class; a pair is a contact where its
        minimum-image distance is strictly below the cutoff -- and correlate it against the stored origins: per lag of 0 .. `num_lags` - 1
        samples the contacts at the origin, those that are contacts again, and (continuous=True) those that never broke, as integers, so
        that the table is the same bits for any launch shape.  Every `origin_every`-th sample is stored as an origin.  `groups`: one int
        per particle of the System (-1: no site); None: everything in group 0.  A class of one group with itself holds every pair twice.
        The cutoffs must not exceed half the shortest box edge.  A sharded context raises ERR_UNSUPPORTED.  No host synchronisation until
        contacts_read."""
        grp = self._groups(groups)
        cls = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1, 2)
        cut = np.ascontiguousarray(r_cut, dtype=np.float64).reshape(-1)
        if cut.size != cls.shape[0]:
            raise ValueError("r_cut must have one entry per class")
        num_groups = max(1, 0 if grp is None else int(grp.max()) + 1, int(cls.max()) + 1 if cls.size else 1)      # (a class may name a group without sites)
        desc = H.ContactsDesc(int(interval), int(num_lags), int(origin_every), num_groups, int(cls.shape[0]), int(bool(exclude_same_molecule)),
                              int(bool(continuous)), 0, None if grp is None else grp.ctypes.data, cls.ctypes.data, cut.ctypes.data,
                              int(max_samples))
        H.check(H.lib.vvhip_contacts_start(self.plan, C.byref(desc)), self.plan)

    def contacts_sample(self):
        """One sample now, behind what is queued, whatever the schedule says (a configuration the host has just uploaded)."""
        H.check(H.lib.vvhip_contacts_sample(self.plan), self.plan)

    def contacts_stop(self):
        self._recorder_stop("contacts")

    def contacts_info(self) -> H.ContactsLayout:
        return self._recorder_info("contacts", H.ContactsLayout)

    def contacts_read(self, reset: bool = False) -> Contacts:
        """The table accumulated so far (synchronises).  reset=True zeroes counts and table, empties every slot and restarts the sample
        ordinal; the step schedule continues without gap or repeat."""
        return self._recorder_read("contacts", H.ContactsLayout, H.ContactsCounts, contacts_from_words, reset)

    # ---- collective current correlations accumulated on the device inside the steps (include/vvhip.h: vvhip_current_*)
    def current_start(self, interval: int, num_lags: int, origin_every: int = 1, weights=None, molecules: bool = False, groups=None,
                      max_samples: int = 1 << 20, limit_position: float = 0.0, limit_velocity: float = 0.0):
        """After every step whose number is a multiple of `interval` (steps counted as for the series), sum w_i X_i and w_i v_i per group
        as fixed-point integers and correlate the sums against the stored origins: per lag of 0 .. `num_lags` samples the products of the
        groups' collective displacements and currents, in float64 in sample order, so that the table is the same bits for any launch
        shape.  `weights`: one float per particle of the System; None: the charges, or with molecules=True Q_m m_i / M_m (the molecules'
        centres of mass carry their net charge).  Every `origin_every`-th sample is stored as an origin.  `groups`: one int per particle
        (-1: not recorded, at most 8 groups); None: everything in group 0.  A position or velocity component at or beyond its limit (nm,
        nm/ps; 0: 64) makes the whole sample invalid.  A sharded context raises ERR_UNSUPPORTED.  No host synchronisation until
        current_read."""
        n = self.system.num_atoms
        if weights is None:
            w = current_weights(self.system, molecules)
        else:
            if molecules:
                raise ValueError("give either weights or molecules=True")
            w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.size != n:
            raise ValueError("weights must have one entry per particle of the System")
        grp = self._groups(groups)
        desc = H.CurrentDesc(int(interval), int(num_lags), int(origin_every), 1 if grp is None else max(int(grp.max()) + 1, 1), w.ctypes.data,
                             None if grp is None else grp.ctypes.data, int(max_samples), float(limit_position), float(limit_velocity))
        H.check(H.lib.vvhip_current_start(self.plan, C.byref(desc)), self.plan)

    def current_stop(self):
        self._recorder_stop("current")

    def current_info(self) -> H.CurrentLayout:
        return self._recorder_info("current", H.CurrentLayout)

    def current_read(self, reset: bool = False) -> Currents:
        """The table accumulated so far (synchronises).  reset=True zeroes it and restarts the sample ordinal with no live origin; the step
        schedule continues without gap or repeat."""
        return self._recorder_read("current", H.CurrentLayout, H.CurrentCounts, currents_from_words, reset)

    # ---- density modes, S(k) and F(k, t), accumulated on the device inside the steps (include/vvhip.h: vvhip_modes_*)
    def modes_start(self, interval: int, modes, num_lags: int = 0, origin_every: int = 1, weights=None, groups=None,
                    max_samples: int = 1 << 20, limit_position: float = 0.0):
        """After every step whose number is a multiple of `interval` (steps counted as for the series), sum w_i exp(i k . X_i) per group
        and mode as fixed-point integers and correlate the sums against the stored origins: per lag of 0 .. `num_lags` samples
        Re rho_g*(0) rho_h(t), in float64 in sample order, so that the table is the same bits for any launch shape.  `modes`: integer
        triples [K, 3] (modes_in_shells), mode k being 2 pi n / L of the box as it stands at the sample.  `weights`: one float per particle
        of the System; None: 1 (number densities); the charges give the charge structure factor.  num_lags = 0: S(k) only, no ring.
        `groups`: one int per particle (-1: not recorded, at most 8 groups); None: everything in group 0.  A position component at or
        beyond the limit (nm; 0: 64) makes the whole sample invalid.  A sharded context raises ERR_UNSUPPORTED.  No host synchronisation
        until modes_read."""
        n = self.system.num_atoms
        w = np.ones(n, dtype=np.float64) if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.size != n:
            raise ValueError("weights must have one entry per particle of the System")
        m = np.ascontiguousarray(modes, dtype=np.int32).reshape(-1, 3)
        if not np.array_equal(m, np.asarray(modes).reshape(-1, 3)):
            raise ValueError("modes must be integer triples")
        grp = self._groups(groups)
        desc = H.ModesDesc(int(interval), int(num_lags), int(origin_every), 1 if grp is None else max(int(grp.max()) + 1, 1), int(m.shape[0]),
                           w.ctypes.data, None if grp is None else grp.ctypes.data, m.ctypes.data, int(max_samples), float(limit_position))
        H.check(H.lib.vvhip_modes_start(self.plan, C.byref(desc)), self.plan)
        self._modes = m.copy()

    def modes_stop(self):
        self._recorder_stop("modes")

    def modes_info(self) -> H.ModesLayout:
        return self._recorder_info("modes", H.ModesLayout)

    def modes_read(self, reset: bool = False) -> DensityModes:
        """The table accumulated so far (synchronises).  reset=True zeroes it and restarts the sample ordinal with no live origin; the step
        schedule continues without gap or repeat."""
        return self._recorder_read("modes", H.ModesLayout, H.ModesCounts, modes_from_words, reset, getattr(self, "_modes", None))

    # ---- removal of the centre-of-mass motion on the device (include/vvhip.h: vvhip_cm_motion_*); nothing is on by default
    def remove_cm_motion_every(self, frequency: int):
        """Subtract the centre-of-mass velocity of all massive particles in front of every step whose 0-based number (steps counted as for
        the series) is a multiple of `frequency`, on the device and inside graph replays: what a CMMotionRemover(frequency) does in
        OpenMM.  Needs a System described with has_cm_motion_remover (the thermostat then counts 3 degrees of freedom less)."""
        H.check(H.lib.vvhip_cm_motion_start(self.plan, int(frequency)), self.plan)

    def remove_cm_motion_stop(self):
        H.check(H.lib.vvhip_cm_motion_stop(self.plan), self.plan)

    def remove_cm_motion(self) -> np.ndarray:
        """One removal now (blocks): returns the velocity V = sum m v / sum m [nm/ps] that was subtracted from every massive particle.
        Independent of the schedule and of has_cm_motion_remover."""
        v = (C.c_double * 3)()
        H.check(H.lib.vvhip_remove_cm_motion(self.plan, C.byref(v)), self.plan)
        return np.array(v, dtype=np.float64)

    def cm_motion_record(self) -> H.CmMotionRecord:
        """frequency, removals done, removals skipped, the last V and the total mass of the scheduled removals (synchronises).  Raises
        (ERR_OVERFLOW) if a removal was skipped because a momentum term was NaN or out of range."""
        out = H.CmMotionRecord()
        H.check(H.lib.vvhip_cm_motion_read(self.plan, C.byref(out)), self.plan)
        return out

    # ---- Monte Carlo barostat: the device half of an attempt (include/vvhip.h: vvhip_barostat_*); the driver is barostat.MonteCarloBarostat
    @property
    def num_molecules(self) -> int:
        """Molecules of the whole System (the N of the barostat's acceptance rule)."""
        return int(self.system.num_molecules)

    def getPeriodicBoxSize(self) -> np.ndarray:
        """The box edges [nm] as the plan holds them."""
        return self._box.copy()

    def scale_box(self, scale):
        """Scale the box edges by scale[0..2] and move every molecule of this context rigidly so that its geometric centre scales with
        them, on the device.  The positions in front of the call are kept on the device until the next scale: restore_box() undoes the
        proposal bit for bit.  Blocks; a position that is not finite or beyond 2^22 nm raises ERR_OVERFLOW and changes nothing."""
        s = (C.c_double * 3)(*[float(x) for x in scale])
        H.check(H.lib.vvhip_barostat_scale(self.plan, C.byref(s)), self.plan)
        self._box = np.array(self.barostat_record().box_after, dtype=np.float64)
        self.forces_valid = False

    def restore_box(self):
        """Undo the last scale_box: positions and box are bit for bit what they were.  Refused (ERR_INVALID) when nothing is pending, or
        when steps were taken, the box was set or a checkpoint was loaded since."""
        H.check(H.lib.vvhip_barostat_restore(self.plan), self.plan)
        self._box = np.array(self.barostat_record().box_before, dtype=np.float64)
        self.forces_valid = False

    def barostat_record(self) -> H.BarostatRecord:
        out = H.BarostatRecord()
        H.check(H.lib.vvhip_barostat_read(self.plan, C.byref(out)), self.plan)
        return out

    # ---- checkpoint: the run's complete state as bytes (include/vvhip.h: vvhip_checkpoint_*)
    def createCheckpoint(self, sections="all") -> bytes:
        """The complete state of the run as a blob in the library's own format (not OpenMM's): particle arrays, forces, extra forces, the
        Langevin normals in use, both thermostat copies, the generator's epoch and seed, the step counter and this context's random index.
        sections="integrator" leaves out posq, correction, velm and force (what an OpenMM adapter stores next to the Context's own
        checkpoint); an int is taken as a mask of H.CKPT_* bits.  A state with a sticky error raised is refused.  Blocks."""
        mask = {"all": H.CKPT_ALL, "integrator": H.CKPT_INTEGRATOR}[sections] if isinstance(sections, str) else int(sections)
        n = C.c_size_t(0)
        H.check(H.lib.vvhip_checkpoint_size(self.plan, mask, C.byref(n)), self.plan)
        buf = C.create_string_buffer(n.value)
        words = (C.c_uint64 * 4)(int(self.random_index), int(bool(self.forces_valid)), 0, 0)
        H.check(H.lib.vvhip_checkpoint_save(self.plan, mask, C.byref(words), buf, n.value), self.plan)
        return buf.raw

    def loadCheckpoint(self, blob):
        """Put a blob of createCheckpoint back: the run continues with the bits of the run that wrote it.  The blob is verified (format,
        every section's digest), compared with this context's structure, uploaded, and the device state verified against its digests.  The
        integrator's parameters are NOT taken from the blob.  A running series, frame, profile, MSD, RDF, current, density-mode, contact, autocorrelation, self or distinct van Hove recorder must be stopped first and started again afterwards, as
        must a removal schedule whose record is to start over; a sharded context refuses."""
        blob = bytes(blob)
        words = (C.c_uint64 * 4)()
        H.check(H.lib.vvhip_checkpoint_load(self.plan, blob, len(blob), C.byref(words)), self.plan)
        self.random_index, self.forces_valid = int(words[0]), bool(words[1])
        hdr = H.CheckpointHeader()
        H.check(H.lib.vvhip_checkpoint_inspect(blob, len(blob), C.byref(hdr)), what="checkpoint header")
        self._box = np.array(hdr.box, dtype=np.float64)                   # (the plan has taken the blob's box)

    def state_digest(self) -> dict:
        """{section name: 64-bit digest} of the state as it stands, computed on the device (vvhip_state_digest): two states are the same
        bits where their digests agree, at 8 bytes copied back per array.  Sections not in use report 0."""
        out = (C.c_uint64 * H.CKPT_SECTIONS)()
        H.check(H.lib.vvhip_state_digest(self.plan, C.byref(out)), self.plan)
        return {name: int(out[k]) for k, name in enumerate(H.CKPT_SECTION_NAMES)}

    def getNHState(self) -> H.NHState:
        s = H.NHState()
        H.check(H.lib.vvhip_get_nh_state(self.plan, C.byref(s)), self.plan)
        return s

    def setNHState(self, s: H.NHState):
        H.check(H.lib.vvhip_set_nh_state(self.plan, C.byref(s)), self.plan)

    # ---- stepping
    def setPeriodicBoxSize(self, lx, ly, lz):
        """A barostat move as the plugin sees it: cu.getPeriodicBoxSize() is read live by the cos kernels (HOST:1057, 1129)."""
        box = (C.c_double * 3)(float(lx), float(ly), float(lz))
        H.check(H.lib.vvhip_set_box(self.plan, C.byref(box)), self.plan)
        self._box = np.array(box, dtype=np.float64)

    def _set_params(self):
        H.check(H.lib.vvhip_set_params(self.plan, C.byref(self.integrator._params())), self.plan)

    def calcForces(self):
        """Plays context->calcForcesAndEnergy (OpenMM's, out of scope for the plugin)."""
        if self.force_provider == "tether":
            H.check(H.lib.vvhip_synth_tether_force(self.plan, self.site.ptr, self.k_tether, self.k_drude), self.plan)
        elif callable(self.force_provider):
            self.force_provider(self)

    def _prepare_random(self) -> int:
        """integration.prepareRandomNumbers(n) of OpenMM, on a fixed buffer (HOST:863)."""
        if self.random is None:
            return 0
        cnt = max(self.info.num_normal_ld, 1) + 2 * max(self.info.num_pairs_ld, 1)
        if self.random_index + cnt <= self.random_host.shape[0]:
            old = self.random_index
            self.random_index += cnt
            return old
        # exhausted: OpenMM's prepareRandomNumbers refills the buffer here; so does this host, with the device generator -- unless the
        # caller injected the normals (parity runs against the oracle, which has no generator and starts over at index 0)
        if not self._random_injected:
            self.fill_random()
        self.random_index = cnt
        return 0

    def _step(self, steps: int):
        L, plan = H.lib, self.plan
        has_ld = self.info.num_normal_ld + self.info.num_pairs_ld > 0
        for _ in range(steps):
            if self.integrator._useMiddleScheme:               # VVIntegrator.cpp:232-270
                self.calcForces()
                ri = self._prepare_random() if has_ld else 0
                H.check(L.vvhip_step_middle(plan, ri), plan)
            else:                                              # VVIntegrator.cpp:272-338
                if not self.forces_valid:
                    self.calcForces()
                    self.forces_valid = True
                H.check(L.vvhip_step_vv_first(plan), plan)
                self.calcForces()
                self.forces_valid = True
                ri = self._prepare_random() if has_ld else 0
                H.check(L.vvhip_step_vv_second(plan, ri), plan)

    def run_graph(self, steps: int, steps_per_graph: int = 50):
        """Replay a captured hipGraph of whole steps (force provider included; both schemes).  With a Langevin subset the
        graph starts with a refill of the random buffer by the device generator, so every replay draws fresh numbers."""
        site = self.site.ptr if self.force_provider == "tether" else None
        H.check(H.lib.vvhip_run_graph(self.plan, int(steps), int(steps_per_graph), site, self.k_tether, self.k_drude), self.plan)
        if not self.integrator._useMiddleScheme and site is not None and steps > 0:
            self.forces_valid = True                                # the last force evaluation was at the final positions

    def graph_prepare(self, steps_per_graph: int = 50):
        """Capture + instantiate + upload the graph for the current thermostat parity without launching it (vvhip_graph_prepare):
        hosts call it after their warm-up so that no capture ever falls into a timed region."""
        site = self.site.ptr if self.force_provider == "tether" else None
        H.check(H.lib.vvhip_graph_prepare(self.plan, int(steps_per_graph), site, self.k_tether, self.k_drude), self.plan)

    def status(self):
        """(mailbox_timed_out, accumulator_overflow): the sticky health flags, read without synchronising."""
        a, b = C.c_int32(0), C.c_int32(0)
        H.check(H.lib.vvhip_status(self.plan, C.byref(a), C.byref(b)), self.plan)
        return bool(a.value), bool(b.value)

    def status_clear(self):
        H.check(H.lib.vvhip_status_clear(self.plan), self.plan)

    def status_words(self):
        """[mailbox wait ran out, accumulator overflow, one-launch rendezvous ran out, constraint cluster hit its iteration cap]: all four
        sticky health words (vvhip_status_words)."""
        w = (C.c_int32 * 4)()
        H.check(H.lib.vvhip_status_words(self.plan, C.byref(w)), self.plan)
        return [int(x) for x in w]

    def fused_status(self):
        """(active, launches): whether vvhip_step_middle runs this plan's step as ONE launch (kernels A and B around an in-kernel
        rendezvous), and how many such launches it has enqueued (vvhip_fused_status)."""
        a, n = C.c_int32(0), C.c_int64(0)
        H.check(H.lib.vvhip_fused_status(self.plan, C.byref(a), C.byref(n), None), self.plan)
        return bool(a.value), int(n.value)

    def recovery_count(self) -> int:
        """How often this plan has repaired a missed rendezvous of the one-launch step (include/vvhip.h: vvhip_recovery_count)."""
        n = C.c_int64(0)
        H.check(H.lib.vvhip_recovery_count(self.plan, C.byref(n)), self.plan)
        return int(n.value)

    def fused_wait_units(self) -> int:
        """Where the self-tuning wait of the one-launch step's rendezvous stands (units of 256 shader clocks; synchronises)."""
        w = C.c_int32(0)
        H.check(H.lib.vvhip_fused_status(self.plan, None, None, C.byref(w)), self.plan)
        return int(w.value)

    def fill_random(self, seed=None):
        """Refill the Langevin random buffer with the device generator (Philox4x32-10 + Box-Muller)."""
        if seed is not None:
            H.check(H.lib.vvhip_set_random_seed(self.plan, int(seed)), self.plan)
        H.check(H.lib.vvhip_fill_random(self.plan), self.plan)

    def run_eager(self, steps: int):
        """The same steps enqueued one by one from C (no per-step Python, no graph; both schemes)."""
        site = self.site.ptr if self.force_provider == "tether" else None
        H.check(H.lib.vvhip_run_eager(self.plan, int(steps), site, self.k_tether, self.k_drude), self.plan)
        if not self.integrator._useMiddleScheme and site is not None and steps > 0:
            self.forces_valid = True

    def run_eager_unfused(self, steps: int):
        """Middle scheme through the per-KernelImpl entry points in VVIntegrator::stepMiddle's order, enqueued from C: the launches
        of the un-fused drop-in path (a host solver between the stages would add its own)."""
        site = self.site.ptr if self.force_provider == "tether" else None
        H.check(H.lib.vvhip_run_eager_unfused(self.plan, int(steps), site, self.k_tether, self.k_drude), self.plan)

    def comm_init(self, unique_id: bytes, nranks: int, rank: int):
        """Give the plan an RCCL communicator (vvhip_comm_init); the id comes from comm_unique_id() on rank 0."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        H.check(H.lib.vvhip_comm_init(self.plan, buf, int(nranks), int(rank)), self.plan)

    def comm_count(self) -> int:
        """Ranks of the plan's RCCL communicator as ncclCommCount reports them (0: none)."""
        n = C.c_int32(0)
        H.check(H.lib.vvhip_comm_count(self.plan, C.byref(n)), self.plan)
        return n.value

    def mailbox_create(self, nranks: int, rank: int) -> bytes:
        """xGMI mailbox exchange (vvhip_mailbox_*): returns this rank's 64-byte IPC handle; gather all ranks' handles in rank
        order and pass them to mailbox_connect()."""
        buf = C.create_string_buffer(64)
        H.check(H.lib.vvhip_mailbox_create(self.plan, int(nranks), int(rank), buf), self.plan)
        return buf.raw

    def mailbox_connect(self, handles: bytes):
        buf = C.create_string_buffer(bytes(handles), len(handles))
        H.check(H.lib.vvhip_mailbox_connect(self.plan, buf), self.plan)

    def mailbox_status(self):
        """(active, timed_out): whether the fused steps use the mailbox, and whether a wait on the peers ever ran out."""
        a, t = C.c_int32(0), C.c_int32(0)
        H.check(H.lib.vvhip_mailbox_status(self.plan, C.byref(a), C.byref(t)), self.plan)
        return bool(a.value), bool(t.value)

    def mailbox_layout(self):
        """(shared_device, arithmetic_layout): whether a peer's box lives on this rank's own device, and whether kernel B takes the
        arithmetic work-item layout next to the exchange."""
        a, t = C.c_int32(0), C.c_int32(0)
        H.check(H.lib.vvhip_mailbox_layout(self.plan, C.byref(a), C.byref(t)), self.plan)
        return bool(a.value), bool(t.value)

    def mailbox_destroy(self):
        H.check(H.lib.vvhip_mailbox_destroy(self.plan), self.plan)

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        H.check(H.lib.vvhip_comm_unique_id(buf), what="ncclGetUniqueId failed (is librccl available?)")
        return buf.raw

    def _viscosity(self):
        v, inv = C.c_double(), C.c_double()
        H.check(H.lib.vvhip_calc_viscosity(self.plan, C.byref(v), C.byref(inv)), self.plan)
        return (v.value, inv.value)

    def generic_launches(self):
        """((count_A, count_B), (stage_set_A, stage_set_B)): launches of this plan that found no compiled specialisation of their stage
        set and ran the generic kernel (vvhip_generic_launches)."""
        n, f = (C.c_int64 * 2)(), (C.c_uint32 * 2)()
        H.check(H.lib.vvhip_generic_launches(self.plan, C.byref(n), C.byref(f)), self.plan)
        return (int(n[0]), int(n[1])), (int(f[0]), int(f[1]))

    @staticmethod
    def rtc_stats():
        """(kernels compiled at run time, launches of kernel A that ran one, of kernel B, seconds spent compiling), process-wide
        (vvhip_rtc_stats)."""
        n, t = (C.c_int64 * 3)(), C.c_double()
        rc = H.lib.vvhip_rtc_stats(C.byref(n), C.byref(t))
        if rc != 0:
            raise RuntimeError("vvhip_rtc_stats failed: %d" % rc)
        return int(n[0]), int(n[1]), int(n[2]), float(t.value)

    @staticmethod
    def rtc_mode(mode=-1):
        """Sets VVHIP_RTC's value for the launches that follow (0 never, 1 stage sets without a compiled kernel, 2 always) and returns
        the previous one; -1 only reads it (vvhip_rtc_mode)."""
        return int(H.lib.vvhip_rtc_mode(int(mode)))

    def timing(self, enable):
        """0 / False off; 1 / True every launch group; 2 kernels A and B only (dispatch timestamps, nothing added to the stream);
        n > 2 as 2 with n events prepared beforehand (vvhip_timing_enable)."""
        H.check(H.lib.vvhip_timing_enable(self.plan, int(enable)), self.plan)

    def timing_read(self):
        a, b, o = C.c_double(), C.c_double(), C.c_double()
        n = (C.c_int32 * 3)()
        H.check(H.lib.vvhip_timing_read(self.plan, C.byref(a), C.byref(b), C.byref(o), C.byref(n)), self.plan)
        return dict(ms_a=a.value, ms_b=b.value, ms_other=o.value, launches=list(n))

    def algorithmic_bytes(self):
        """(bytes_A, bytes_B) per particle of the fused middle step's two kernels (vvhip_algorithmic_bytes)."""
        a, b = C.c_int32(0), C.c_int32(0)
        H.check(H.lib.vvhip_algorithmic_bytes(self.plan, C.byref(a), C.byref(b)), self.plan)
        return a.value, b.value

    def time_kernel(self, kernel: int, reps: int = 200) -> float:
        """Average ms of `reps` back-to-back launches of stage kernel 0 (A) / 1 (B) with the fused step's stage bits.
        Timing only: the physical state is not meaningful afterwards."""
        ms = C.c_double()
        H.check(H.lib.vvhip_time_kernel(self.plan, int(kernel), 0xFFFFFFFF, int(reps), C.byref(ms)), self.plan)
        return ms.value

    def close(self):
        if getattr(self, "plan", None):
            H.lib.vvhip_comm_destroy(self.plan)
            H.lib.vvhip_plan_destroy(self.plan)
            self.plan = None
            self.integrator._context = None
            if self._own_stream:
                H.lib.vvhip_stream_destroy(self._own_stream)
                self._own_stream = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
