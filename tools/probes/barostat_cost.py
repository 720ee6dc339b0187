"""Cost of the Monte Carlo barostat (barostat.MonteCarloBarostat on Context.scale_box / restore_box) next to graph runs: steps/s of
20 000-step runs as replays of 50-step graphs with the barostat off, and with `iso` attempts every 100 steps whose energy callable
returns 0 (so the figure is the move, the backup, the restore of a rejected attempt and the re-capture of the graphs the new box drops --
not a force evaluation) -- and, with --parent-lib, of another build of the library (the commit before the feature) with nothing on.  One
process per build and repeat, in rotation on one box; inside a process the settings alternate on ONE context, each warmed up untimed first.
usage: python tools/probes/barostat_cost.py [repeats] [steps] [config] [--parent-lib PATH] > profiles/barostat_cost.txt"""
import importlib, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

args = [a for a in sys.argv[1:] if not a.startswith("--")]
parent_lib = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
if parent_lib:
    args.remove(parent_lib)
child = "--child" in sys.argv
rep = int(args[0]) if len(args) > 0 else 5
steps = int(args[1]) if len(args) > 1 else 20000
cfg = args[2] if len(args) > 2 else "C3"
FREQUENCY = 100
SETTINGS = [("off", False), ("iso/100", True)]


def measure(settings, reverse):
    """One context; every setting: 2 000 steps untimed (capture + warm), `steps` steps timed.  Prints RATE lines."""
    pkg = importlib.import_module("openmm-velocityverlet_amd")
    I, S = pkg.integrator, pkg.systems
    spec = S.make_config(cfg)
    it = I.VVIntegrator(300.0 if cfg == "C2" else 333.0, 10, 1.0, 40, 0.002 if cfg == "C2" else 0.001)
    if cfg != "C2":
        it.setMaxDrudeDistance(0.02)
    ctx = I.Context(spec, it, precision="mixed", force_provider="tether")
    ctx.run_graph(2000, 50); ctx.synchronize()
    for name, on in (settings[::-1] if reverse else settings):
        baro = pkg.barostat.MonteCarloBarostat(1.0, 333.0, mode="iso", frequency=FREQUENCY, seed=1) if on else None
        run = (lambda n: baro.run(ctx, n, lambda: 0.0, 50)) if on else (lambda n: ctx.run_graph(n, 50))
        run(2000); ctx.synchronize()
        t0 = time.perf_counter()
        run(steps); ctx.synchronize()
        print(f"RATE {name} {steps / (time.perf_counter() - t0):.3f}", flush=True)
        if on:
            rec = ctx.barostat_record()
            assert rec.scales == (2000 + steps) // FREQUENCY, rec.scales
            print(f"NOTE {name}: {baro.accepted} of {baro.attempts} attempts accepted, {rec.restores} restored", flush=True)
    ctx.close()


if child:
    label = sys.argv[sys.argv.index("--child") + 1]
    measure([("parent", False)] if label == "parent" else SETTINGS, "--reverse" in sys.argv)
    sys.exit(0)

rates = {}
for r in range(rep):
    builds = ([("parent", parent_lib)] if parent_lib else []) + [("this", None)]
    for label, lib in (builds if r % 2 == 0 else builds[::-1]):
        env = dict(os.environ)
        if lib:
            env["VVHIP_LIB"] = os.path.abspath(lib)
        else:
            env.pop("VVHIP_LIB", None)
        cmd = [sys.executable, os.path.abspath(__file__), str(rep), str(steps), cfg, "--child", label] + (["--reverse"] if r % 2 else [])
        out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
        if out.returncode != 0:
            sys.exit(f"{label} child failed ({out.returncode}):\n{out.stdout[-2000:]}{out.stderr[-2000:]}")
        for line in out.stdout.splitlines():
            if line.startswith("RATE "):
                _, name, value = line.split()
                rates.setdefault(name, []).append(float(value))
base = np.median(rates["off"])
for name in (["parent"] if parent_lib else []) + [n for n, _ in SETTINGS]:
    v = np.array(rates[name])
    per = f"  {1e6 * FREQUENCY * (1 / np.median(v) - 1 / base):7.2f} us per attempt" if dict(SETTINGS).get(name) else ""
    print(f"{cfg} barostat {name:>8}: median {np.median(v):9.1f} steps/s  (min {v.min():9.1f}, max {v.max():9.1f})  "
          f"{100 * (np.median(v) / base - 1):+6.2f} % against off{per}   [{', '.join(f'{x:.0f}' for x in v)}]", flush=True)
