"""Cost of the device-side trajectory recorder (Context.frames_start) inside graph runs: steps/s of 20 000-step run_graph calls (50-step
graphs) with the recorder off, float32 positions every 1 000 and every 100 steps, the logarithmic schedule from 10 -- and of the host
alternative at the same frame steps: run_graph in chunks of the interval with Context.getPositions() after each.  With --parent-lib
another build of the library (the commit before the feature) runs with nothing on in the same rotation.  One process per build and repeat,
in rotation on one box; inside a process the settings alternate on ONE context, each warmed up untimed first so that its graphs are
captured outside the timed region.
usage: python tools/probes/frames_cost.py [repeats] [steps] [config] [--parent-lib PATH]"""
import ctypes as C
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
# (name, interval, logarithmic, on the host instead)
SETTINGS = [("off", 0, False, False), ("1000", 1000, False, False), ("100", 100, False, False), ("log10", 10, True, False),
            ("host-1000", 1000, False, True), ("host-100", 100, False, True)]
WARM = 2000


def measure(settings, reverse):
    """One context; every setting: switch, WARM steps untimed (capture + warm), `steps` steps timed.  Prints RATE lines."""
    pkg = importlib.import_module("openmm-velocityverlet_amd")
    I, S, H = pkg.integrator, pkg.systems, pkg.vvhip
    spec = S.make_config(cfg)
    it = I.VVIntegrator(300.0 if cfg == "C2" else 333.0, 10, 1.0, 40, 0.002 if cfg == "C2" else 0.001)
    if cfg != "C2":
        it.setMaxDrudeDistance(0.02)
    ctx = I.Context(spec, it, precision="mixed", force_provider="tether")
    ctx.run_graph(WARM, 50); ctx.synchronize()

    def count(reset):
        """frames recorded and dropped, without downloading them"""
        n, dropped = C.c_int32(0), C.c_int64(0)
        H.check(H.lib.vvhip_frames_read(ctx.plan, None, None, 0, C.byref(n), C.byref(dropped), int(reset)), ctx.plan)
        return n.value, dropped.value

    for name, interval, logarithmic, host in (settings[::-1] if reverse else settings):
        device = interval and not host
        if device:
            ctx.frames_start(interval, capacity=(WARM + steps) // interval + 8 if not logarithmic else 64, logarithmic=logarithmic)
        elif hasattr(ctx, "frames_stop") and "vvhip_frames_stop" in H.EXPORTS:
            ctx.frames_stop()
        first = ctx.series_info().steps
        ctx.run_graph(WARM, 50); ctx.synchronize()
        if device:
            count(True)
        t0 = time.perf_counter()
        if host:
            for _ in range(steps // interval):
                ctx.run_graph(interval, 50)
                ctx.getPositions()
        else:
            ctx.run_graph(steps, 50)
        ctx.synchronize()
        dt = time.perf_counter() - t0
        frames = ""
        if device:
            n, dropped = count(False)
            want = len(H.frames_steps(interval, first + WARM, first + WARM + steps, logarithmic))
            assert n == want and dropped == 0, (name, n, want, dropped)
            frames = f" {n}"
        elif host:
            frames = f" {steps // interval}"
        print(f"RATE {name} {steps / dt:.3f}{frames}", flush=True)
    ctx.close()


if child:
    label = sys.argv[sys.argv.index("--child") + 1]
    measure([("parent", 0, False, False)] if label == "parent" else SETTINGS, "--reverse" in sys.argv)
    sys.exit(0)

rates, frames = {}, {}
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
                f = line.split()
                rates.setdefault(f[1], []).append(float(f[2]))
                if len(f) > 3:
                    frames[f[1]] = int(f[3])
base = np.median(rates["off"])
for name in (["parent"] if parent_lib else []) + [s[0] for s in SETTINGS]:
    v = np.array(rates[name])
    n = frames.get(name, 0)
    per = f"  {n:4d} frames, {1e6 * steps / n * (1 / np.median(v) - 1 / base):8.2f} us per frame" if n else ""
    print(f"{cfg} frames {name:>9}: median {np.median(v):9.1f} steps/s  (min {v.min():9.1f}, max {v.max():9.1f})  "
          f"{100 * (np.median(v) / base - 1):+6.2f} % against off{per}   [{', '.join(f'{x:.0f}' for x in v)}]", flush=True)
