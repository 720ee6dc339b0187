"""Systems and settings shared by tests/test_checkpoint.py and tests/test_gpu_checkpoint.py: the four small systems, a context factory,
the three drivers, a hand-made blob for the parser tests, and the bitwise comparison of two states.

One exception to "every bit": NHDevState::rv_delay / rv_calm, the self-tuning wait of the one-launch step's rendezvous, follow how
the blocks happened to arrive in the steps run, not the trajectory -- two runs of the same steps may differ there and nowhere else.  A
checkpoint carries them (a load restores them, and the section's digest is verified against the device at save and load); comparisons
BETWEEN runs mask these 8 bytes per thermostat copy and compare every other byte of the section."""
import ctypes as C
import functools
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_reference as ref      # noqa: E402

PARTICLE_ARRAYS = ("posq", "correction", "velm", "force")


def _pkg():
    return importlib.import_module("openmm-velocityverlet_amd")


@functools.lru_cache(maxsize=None)
def system(name):
    S = _pkg().systems
    if name == "D":
        return S.drude_il(cells=(1, 1, 1), pairs_per_cell=15, seed=34)
    if name == "W":
        return S.rigid_water(S.spce_water(22, seed=22))          # 66 particles: one wave and a bit; SETTLE
    if name == "E":
        return S.edl_slab(num_ion_pairs=20, num_electrode=60, seed=9)      # Langevin subset, images, field
    if name == "H":
        return S.constrain_hydrogens(system("D"))
    raise KeyError(name)


def make(name, prec="mixed", middle=True, cos=0.0, tune=None, shard=None):
    """(integrator, context) of a system with its usual settings; E draws its normals with the device generator (none injected)."""
    I = _pkg().integrator
    spec = system(name)
    water = name == "W"
    it = I.VVIntegrator(300.0 if water else 333.0, 10.0, 1.0, 40.0, 0.002 if water else 0.001)
    it.setMaxDrudeDistance(0.0 if water else 0.02)
    it.setUseMiddleScheme(middle)
    it.setCosAcceleration(cos)
    if name == "E":
        lz = float(spec.box[2])
        it.setMirrorLocation(lz / 2)
        it.setElectricField(2.0 / lz * 2 * 1.602176634e-22)
    return it, I.Context(spec, it, precision=prec, force_provider="tether", tune=tune, shard=shard)


def drive(it, ctx, how, n, spg=4):
    if how == "step":
        it.step(n)
    elif how == "eager":
        ctx.run_eager(n)
    else:
        ctx.run_graph(n, steps_per_graph=spg)


def nh_copy_bytes():
    """sizeof(NHDevState) (csrc/vv_args.hpp): vvhip_nh_state, scales[4], mb_seq, rv_seq, rv_delay, rv_calm."""
    return C.sizeof(_pkg().vvhip.NHState) + 32 + 16


def masked_thermostat(payload: bytes) -> bytes:
    """Both thermostat copies with rv_delay / rv_calm (the last 8 bytes of each copy) zeroed: see the module's text."""
    n = nh_copy_bytes()
    assert len(payload) == 2 * n
    b = bytearray(payload)
    for c in range(2):
        b[(c + 1) * n - 8:(c + 1) * n] = bytes(8)
    return bytes(b)


def state(ctx):
    """Everything two runs are compared on: the four particle arrays as downloaded, and every section's digest from the device --
    the thermostat's taken over the masked bytes of the saved section instead."""
    H = _pkg().vvhip
    d = ctx.state_digest()
    blob = ctx.createCheckpoint()
    _, sections = ref.read_blob(blob)
    for name, (row, payload) in sections.items():
        assert int(row["digest"]) == d[name], name          # the blob's table is the device's digest
    nh = masked_thermostat(sections["thermostat"][1])
    d["thermostat"] = ref.digest(nh)
    out = dict(posq=ctx.getPosq(), velm=ctx.getVelm(), force=ctx.getForce(), correction=ctx.getPosqCorrection() if ctx.precision == "mixed" else None,
               nh=nh, digest=d, random_index=ctx.random_index, forces_valid=ctx.forces_valid, blob=blob, words=ctx.status_words())
    assert H.checkpoint_inspect(blob).num_sections == len(sections)
    return out


def assert_same(a, b, label):
    for k in ("posq", "correction", "velm", "force"):
        if a[k] is not None:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{label}: {k} differs"
    assert a["nh"] == b["nh"], f"{label}: the thermostat copies differ"
    assert a["digest"] == b["digest"], f"{label}: digests differ in {[k for k in a['digest'] if a['digest'][k] != b['digest'][k]]}"
    assert a["words"] == b["words"] == [0, 0, 0, 0], f"{label}: status words {a['words']} {b['words']}"


# ---- a blob made by hand from the documented format (no device): 5 particles in mixed precision, Langevin normals, both thermostat copies
def hand_made_fields():
    return dict(precision=1, num_atoms=5, shard_begin=0, shard_end=5, use_middle_scheme=1, num_nh_chains=3, random_size=6,
                box=(2.5, 2.75, 3.0),
                params=dict(temperature=333.0, frequency=10.0, drude_temperature=1.0, drude_frequency=40.0, step_size=0.001, num_nh_chains=3,
                            loops_per_step=1, max_drude_distance=0.02, friction=5.0, drude_friction=20.0, use_middle_scheme=1,
                            auto_set_com_temp_group=1, auto_set_friction=1, constraint_tolerance=1e-5),
                cursor=dict(parity=1, random_pos=3, fextra_dirty=1, fextra_virtual=0, step_count=23, rng_seed=0x1234567890ABCDEF),
                host_words=(7, 1, 0, 0))


def hand_made_sections():
    rng = np.random.default_rng(20)
    n = 5
    return dict(posq=rng.standard_normal((n, 4)).astype("<f4").tobytes(), correction=rng.standard_normal((n, 4)).astype("<f4").tobytes(),
                velm=rng.standard_normal((n, 4)).astype("<f8").tobytes(), force=rng.integers(-2 ** 40, 2 ** 40, 3 * 32).astype("<i8").tobytes(),
                force_extra=rng.standard_normal((n, 3)).astype("<f4").tobytes(), random=rng.standard_normal((6, 4)).astype("<f4").tobytes(),
                thermostat=rng.standard_normal(2 * nh_copy_bytes() // 8).astype("<f8").tobytes(), epoch=np.array([4], "<u8").tobytes())


def hand_made_blob():
    return ref.write_blob(hand_made_fields(), hand_made_sections())
