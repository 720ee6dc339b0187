"""Cost of one draw of Maxwell-Boltzmann start velocities: Context.setVelocitiesToTemperature (device; the call blocks) against the host
path it replaces -- systems._maxwell_boltzmann in NumPy plus Context.setVelocities -- on one context, alternating, medians of `repeats`
after two untimed rounds.  Host clock around calls that end in a device synchronise.
usage: python tools/probes/thermalize_cost.py [repeats] [config]"""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

rep = int(sys.argv[1]) if len(sys.argv) > 1 else 9
cfg = sys.argv[2] if len(sys.argv) > 2 else "C3"
pkg = importlib.import_module("openmm-velocityverlet_amd")
I, S = pkg.integrator, pkg.systems
spec = S.make_config(cfg)
it = I.VVIntegrator(333.0, 10, 1.0, 40, 0.001)
it.setMaxDrudeDistance(0.02)
ctx = I.Context(spec, it, precision="mixed", force_provider="tether")
m = np.asarray(spec.masses, dtype=np.float64)
isd = np.zeros(m.size, bool)
isd[np.asarray(spec.drude_pairs)[:, 0]] = True
parent_of = np.arange(m.size) - 1
t = {"device plain": [], "device Drude-aware": [], "host draw (NumPy)": [], "host setVelocities": []}
for r in range(rep + 2):
    ctx.synchronize()
    t0 = time.perf_counter(); ctx.setVelocitiesToTemperature(333.0, 1 + r); t1 = time.perf_counter()
    ctx.setVelocitiesToTemperature(333.0, 1 + r, 1.0); t2 = time.perf_counter()
    v = S._maxwell_boltzmann(np.random.default_rng(1 + r), m, isd, parent_of, 333.0, 1.0); t3 = time.perf_counter()
    ctx.setVelocities(v); ctx.synchronize(); t4 = time.perf_counter()
    if r >= 2:
        for k, d in zip(t, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            t[k].append(1e3 * d)
print(f"{cfg}: {spec.num_atoms} particles, {len(spec.drude_pairs)} Drude pairs, mixed precision, {rep} repeats")
for k, v in t.items():
    print(f"{k:>20}: median {np.median(v):8.3f} ms  (min {min(v):8.3f}, max {max(v):8.3f})")
host = np.median(t["host draw (NumPy)"]) + np.median(t["host setVelocities"])
print(f"{'host path':>20}: {host:8.3f} ms = {host / np.median(t['device Drude-aware']):.0f} x the Drude-aware device call")
ctx.close()
