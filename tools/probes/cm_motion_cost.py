"""Cost of the device-side removal of the centre-of-mass motion (Context.remove_cm_motion_every) inside graph runs: steps/s of 20 000-step
run_graph calls (50-step graphs) with the feature off, at f = 10 and at f = 100 -- and, with --parent-lib, of another build of the library
(the commit before the feature) next to them.  One process per build and repeat, in rotation on one box; inside a process the settings
alternate on ONE context, each warmed up untimed first so that its graphs are captured outside the timed region.
usage: python tools/probes/cm_motion_cost.py [repeats] [steps] [config] [--parent-lib PATH]"""
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
SETTINGS = [("off", 0), ("f=10", 10), ("f=100", 100)]


def measure(settings, reverse):
    """One context; every setting: switch, 2 000 steps untimed (capture + warm), `steps` steps timed.  Prints RATE lines."""
    pkg = importlib.import_module("openmm-velocityverlet_amd")
    I, S = pkg.integrator, pkg.systems
    spec = S.make_config(cfg)
    it = I.VVIntegrator(300.0 if cfg == "C2" else 333.0, 10, 1.0, 40, 0.002 if cfg == "C2" else 0.001)
    if cfg != "C2":
        it.setMaxDrudeDistance(0.02)
    ctx = I.Context(spec, it, precision="mixed", force_provider="tether")
    ctx.run_graph(2000, 50); ctx.synchronize()
    for name, f in (settings[::-1] if reverse else settings):
        if f:
            ctx.remove_cm_motion_every(f)
        elif hasattr(ctx, "remove_cm_motion_stop") and "vvhip_cm_motion_stop" in pkg.vvhip.EXPORTS:
            ctx.remove_cm_motion_stop()
        ctx.run_graph(2000, 50); ctx.synchronize()
        t0 = time.perf_counter()
        ctx.run_graph(steps, 50); ctx.synchronize()
        print(f"RATE {name} {steps / (time.perf_counter() - t0):.3f}", flush=True)
        if f:
            rec = ctx.cm_motion_record()
            assert rec.skipped == 0 and rec.removals == (2000 + steps) // f, (name, rec.removals, rec.skipped)
    ctx.close()


if child:
    label = sys.argv[sys.argv.index("--child") + 1]
    measure([("parent", 0)] if label == "parent" else SETTINGS, "--reverse" in sys.argv)
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
    f = dict(SETTINGS).get(name, 0)
    per = f"  {1e6 * f * (1 / np.median(v) - 1 / base):6.2f} us per removal" if f else ""
    print(f"{cfg} cm motion {name:>6}: median {np.median(v):9.1f} steps/s  (min {v.min():9.1f}, max {v.max():9.1f})  "
          f"{100 * (np.median(v) / base - 1):+6.2f} % against off{per}   [{', '.join(f'{x:.0f}' for x in v)}]", flush=True)
