"""The synthetic system of tests/test_gpu_barostat.py: about 3 500 particles built so that every way the barostat's kernels can go wrong
is present -- one molecule of 130 particles (three waves; no COM temperature group, which would want it in one), molecules whose
particles alternate in index (so a molecule's lanes are not neighbours and its id is not contiguous), 3 000 one-particle molecules (more
than one block covers), massless particles inside molecules, positions far outside the box on both sides of the origin, and a last wave
with idle lanes."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S = importlib.import_module("openmm-velocityverlet_amd").systems

BOX = np.array([4.0, 4.5, 5.0])
N_SINGLE, N_BIG, N_PAIRED, PAIR_SIZE = 3000, 130, 50, 4      # 50 couples of molecules of 4 particles, interleaved a b a b a b a b


def synthetic(seed=17):
    rng = np.random.default_rng(seed)
    mol = []
    # the interleaved couples go first and take the HIGHEST ids: molecule ids are neither ascending nor contiguous in particle order
    first_paired = N_SINGLE + 1
    for c in range(N_PAIRED):
        a, b = first_paired + 2 * c, first_paired + 2 * c + 1
        mol += [a, b] * PAIR_SIZE
    mol += list(range(1000))                                  # one-particle molecules
    mol += [N_SINGLE] * N_BIG                                 # the big one, in the middle of them
    mol += list(range(1000, N_SINGLE))
    mol = np.array(mol, dtype=np.int32)
    n = mol.size
    nmol = int(mol.max()) + 1
    centre = rng.uniform(-60.0, 60.0, (nmol, 3))              # box edges 4-5 nm: far outside, negative included
    pos = centre[mol] + rng.normal(0.0, 0.2, (n, 3))
    masses = rng.choice([1.008, 12.011, 15.999], n)
    masses[: 2 * PAIR_SIZE * N_PAIRED : 4] = 0.0              # massless particles inside the interleaved molecules
    big = np.flatnonzero(mol == N_SINGLE)
    masses[big[::13]] = 0.0                                   # ... and inside the big one
    vel = rng.normal(0.0, 0.3, (n, 3))
    vel[masses == 0] = 0.0
    charges = rng.uniform(-1.0, 1.0, n)
    return S.SystemSpec(name="barostat_synthetic", masses=masses, charges=charges, positions=pos, velocities=vel, box=BOX.copy(),
                        mol_id=mol, drude_pairs=np.zeros((0, 2), np.int32), constraints=np.zeros((0, 2), np.int32),
                        has_cm_motion_remover=False)


def shard_cut(spec):
    """A cut between molecules that is no multiple of 64: behind the interleaved couples and 333 of the one-particle molecules."""
    cut = 2 * PAIR_SIZE * N_PAIRED + 333
    assert cut % 64 != 0 and not set(spec.mol_id[:cut].tolist()) & set(spec.mol_id[cut:].tolist())
    return cut


# the end-to-end test's harmonic energy 0.5 k |x - x0|^2 [kJ/mol] and pressure: with these 27 of the 50 attempts are accepted on the stand-in
E2E_SPRING, E2E_PRESSURE_BAR = 0.05, 1.0
