"""Cost of a device-side series (Context.series_start) inside graph runs: C3 steps/s of 20 000-step run_graph calls (50-step graphs), the
series off and at intervals 1 000 / 100 / 50, in alternating repeats on ONE context (each setting is warmed up untimed first, so that its
graphs are captured outside the timed region).
usage: python tools/probes/series_cost.py [repeats] [steps] [config]"""
import importlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
pkg = importlib.import_module("openmm-velocityverlet_amd")
I, S = pkg.integrator, pkg.systems
rep = int(sys.argv[1]) if len(sys.argv) > 1 else 5
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
cfg = sys.argv[3] if len(sys.argv) > 3 else "C3"
SETTINGS = [("off", 0), ("1000", 1000), ("100", 100), ("50", 50)]

spec = S.make_config(cfg)
it = I.VVIntegrator(333.0, 10, 1.0, 40, 0.001)
it.setMaxDrudeDistance(0.02)
ctx = I.Context(spec, it, precision="mixed", force_provider="tether")
ctx.run_graph(2000, 50); ctx.synchronize()
rates = {name: [] for name, _ in SETTINGS}
for r in range(rep):
    for name, interval in (SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
        if interval:
            ctx.series_start(interval, capacity=steps // interval + 64)
        else:
            ctx.series_stop()
        ctx.run_graph(2000, 50); ctx.synchronize()                     # capture + warm, untimed
        if interval:
            ctx.series_read(reset=True)
        t0 = time.perf_counter()
        ctx.run_graph(steps, 50); ctx.synchronize()
        rates[name].append(steps / (time.perf_counter() - t0))
        if interval:
            s = ctx.series_read(reset=True)
            assert len(s) == steps // interval and s.dropped == 0 and s.ok.all(), (name, len(s), s.dropped)
ctx.close()
base = np.median(rates["off"])
for name, _ in SETTINGS:
    v = np.array(rates[name])
    print(f"{cfg} series {name:>4}: median {np.median(v):9.1f} steps/s  (min {v.min():9.1f}, max {v.max():9.1f})  "
          f"{100 * (np.median(v) / base - 1):+6.2f} % against off   [{', '.join(f'{x:.0f}' for x in v)}]", flush=True)
