"""Cost of a checkpoint: Context.createCheckpoint, loadCheckpoint and state_digest against what they replace -- the blocking downloads of
posq, correction, velm and force plus getNHState, and the corresponding uploads -- on one context, alternating, medians of `repeats`
after two untimed rounds.  Host clock around calls that end in a device synchronise.  For the digest alone also bytes / time against
the box's copy rate (a device-to-device copy of the same arrays through torch, bytes read + written over its time; skipped without
torch).
usage: python tools/probes/checkpoint_cost.py [repeats] [config] [scale]"""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

rep = int(sys.argv[1]) if len(sys.argv) > 1 else 9
cfg = sys.argv[2] if len(sys.argv) > 2 else "C3"
scale = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
pkg = importlib.import_module("openmm-velocityverlet_amd")
I, S, H = pkg.integrator, pkg.systems, pkg.vvhip
spec = S.make_config(cfg, scale=scale)
it = I.VVIntegrator(333.0, 10, 1.0, 40, 0.001)
it.setMaxDrudeDistance(0.02)
ctx = I.Context(spec, it, precision="mixed", force_provider="tether")
ctx.run_eager(10)
ctx.synchronize()
t = {"createCheckpoint": [], "loadCheckpoint": [], "state_digest": [], "downloads + getNHState": [], "uploads + setNHState": []}
blob = None
for r in range(rep + 2):
    ctx.synchronize()
    t0 = time.perf_counter(); blob = ctx.createCheckpoint(); t1 = time.perf_counter()
    ctx.loadCheckpoint(blob); t2 = time.perf_counter()
    ctx.state_digest(); t3 = time.perf_counter()
    arrays = (ctx.getPosq(), ctx.getPosqCorrection(), ctx.getVelm(), ctx.getForce()); nh = ctx.getNHState(); t4 = time.perf_counter()
    ctx.posq.upload(arrays[0]); ctx.posq_corr.upload(arrays[1]); ctx.velm.upload(arrays[2]); ctx.force.upload(arrays[3]); ctx.setNHState(nh)
    ctx.synchronize(); t5 = time.perf_counter()
    if r >= 2:
        for k, d in zip(t, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
            t[k].append(1e3 * d)
table = H.checkpoint_sections(blob)
state_bytes = sum(s.bytes for s in table.values())
print(f"{cfg} x {scale:g}: {spec.num_atoms} particles, mixed precision, blob {len(blob)} bytes ({state_bytes / spec.num_atoms:.1f} B per particle), {rep} repeats")
for k, v in t.items():
    print(f"{k:>24}: median {np.median(v):10.3f} ms  (min {min(v):10.3f}, max {max(v):10.3f})")
dg = np.median(t["state_digest"]) * 1e-3
print(f"{'digest, whole call':>24}: {state_bytes / dg / 1e9:10.1f} GB/s read (launches, copy of the words and synchronise included)")
try:
    import torch
    n = state_bytes // 8
    a = torch.empty(n, dtype=torch.int64, device="cuda")
    b = torch.empty_like(a)
    times = []
    for r in range(rep + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record(); torch.cuda.synchronize()
        if r >= 2:
            times.append(e0.elapsed_time(e1) * 1e-3)
    cp = np.median(times)
    print(f"{'device copy, same bytes':>24}: {1e3 * cp:10.3f} ms = {2 * state_bytes / cp / 1e9:.1f} GB/s read + written; the digest call takes {dg / cp:.2f} x the copy's time")
except (ImportError, RuntimeError) as e:
    print(f"no copy rate: torch is not usable here ({type(e).__name__})")
ctx.close()
