"""Child process of tests/test_gpu_cm_motion.py: one removal of the centre-of-mass motion on C3 under the wave layout the environment asks
for (VVHIP_PERIODIC), printed as the layout flag, the bits of V and a digest of the velm bits."""
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("openmm-velocityverlet_amd")
S, I = pkg.systems, pkg.integrator


def main():
    precision = sys.argv[1]
    spec = S.make_config("C3", scale=0.25)
    m = np.asarray(spec.masses)
    v = np.array(spec.velocities, dtype=np.float64)
    v_rms = np.sqrt(np.mean(np.sum(v[m > 0] ** 2, axis=1)))
    v[m > 0] += 0.5 * v_rms * np.array([1.0, -2.0, 3.0]) / np.sqrt(14.0)
    it = I.VVIntegrator(333.0, 10.0, 1.0, 40.0, 0.001)
    it.setMaxDrudeDistance(0.02)
    ctx = I.Context(spec, it, precision=precision, force_provider="tether")
    try:
        ctx.setVelocities(v)
        V = ctx.remove_cm_motion()
        velm = ctx.getVelm()
        print("CMM", ctx.info.periodic_layout, V.view(np.uint64).tolist(), hashlib.sha256(np.ascontiguousarray(velm).tobytes()).hexdigest())
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
