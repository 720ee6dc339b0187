"""Cost of the device-side autocorrelation recorder (Context.acf_start) inside graph runs, per sample, at full-size C3 in mixed precision:
device events around the same run_graph call (20 000 steps as replays of 50-step graphs) with the recorder off and with it sampling every
`interval` steps -- particle velocities with 1, 8 and 32 slots in the ring (num_lags 1, 8, 32, every sample an origin), molecule velocities
with 8, orientations over the Drude pairs with 8 -- and the yardstick beside them on the same context: the MSD recorder at the same shapes
(its kernel moves the same ring bytes).  One context; the settings take turns on it, in reversed order every other repeat, each warmed up
untimed first so that its graphs are captured and the ring is full outside the timed region.  Per setting: the median time, the cost per
sample against `off`, the ring bytes a sample reads and the rate the whole sample's cost amounts to.
With a second library given (the parent commit's build), every repeat also times `off` on it and on this library in a fresh child process
each, the order alternating (the library is chosen when the package is imported: VVHIP_LIB), so that "recorder off" can be put beside the
parent's own run-to-run spread on one box, like with like.
usage: python tools/probes/acf_cost.py [repeats] [steps] [interval] [config] [parent library]      the timing
       python tools/probes/acf_cost.py off [steps] [config]      one timed run with nothing on, one line (what the child processes run)
       python tools/probes/acf_cost.py trace [config]      200 samples per setting and nothing else (for a kernel trace)
       python tools/probes/acf_cost.py scan KEY V ..      the velocity/L32 setting under vvhip_debug_tune(KEY, V) for every V"""
import importlib, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

args = sys.argv[1:]
mode = args[0] if args and args[0] in ("off", "trace", "scan") else "time"
parent_lib, scan_key, scan_values = None, None, [None]
if mode == "off":
    rep, steps, interval, cfg = 1, int(args[1]) if len(args) > 1 else 20000, 10, args[2] if len(args) > 2 else "C3"
elif mode == "trace":
    rep, steps, interval, cfg = 1, 2000, 10, args[1] if len(args) > 1 else "C3"
elif mode == "scan":
    rep, steps, interval, cfg = 5, 20000, 10, "C3"
    scan_key, scan_values = args[1], [int(v) for v in args[2:]]
else:
    rep = int(args[0]) if len(args) > 0 else 5
    steps = int(args[1]) if len(args) > 1 else 20000
    interval = int(args[2]) if len(args) > 2 else 10
    cfg = args[3] if len(args) > 3 else "C3"
    parent_lib = args[4] if len(args) > 4 else None
WARM = 2000
# (name, kind, mode, num_lags)
SETTINGS = [("off", None, None, 0)]
SETTINGS += [(f"acf/velocity/L{l}", "acf", "velocity", l) for l in (1, 8, 32)]
SETTINGS += [("acf/molecules/L8", "acf", "molecules", 8), ("acf/orientation/L8", "acf", "orientation", 8)]
SETTINGS += [(f"msd/particles/L{l}", "msd", False, l) for l in (1, 8, 32)] + [("msd/molecules/L8", "msd", True, 8)]
if mode == "off":
    SETTINGS = SETTINGS[:1]
elif mode == "trace":
    SETTINGS = SETTINGS[1:]
elif mode == "scan":
    SETTINGS = [SETTINGS[0]] + [(f"acf/velocity/L32/{scan_key}={v}", "acf", "velocity", 32) for v in scan_values]

pkg = importlib.import_module("openmm-velocityverlet_amd")
I, S, H = pkg.integrator, pkg.systems, pkg.vvhip
spec = S.make_config(cfg)
n = spec.num_atoms
pairs = np.asarray(spec.drude_pairs, dtype=np.int32).reshape(-1, 2)[:, :2]
it = I.VVIntegrator(333.0, 10, 1.0, 40, 0.001)
it.setMaxDrudeDistance(0.02)
stream = torch.cuda.Stream()
ctx = I.Context(spec, it, precision="mixed", force_provider="tether", stream=stream.cuda_stream)
ctx.run_graph(2000, 50); ctx.synchronize()
has_acf = hasattr(ctx, "acf_stop") and "vvhip_acf_stop" in H.EXPORTS      # (the parent's library has none)
if mode != "off":
    print(f"{cfg}: {n} particles, {len(pairs)} Drude pairs, interval {interval}, {steps} steps per run, library {os.path.relpath(H.LIB_PATH, ROOT)}", flush=True)
times, info, parent_times, child_times = {}, {}, [], []
for r in range(rep):
    for k, (name, kind, what, lags) in enumerate(SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
        ctx.msd_stop()
        if has_acf:
            ctx.acf_stop()
        if mode == "scan" and kind:
            H.check(H.lib.vvhip_debug_tune(ctx.plan, scan_key.encode(), int(name.rsplit("=", 1)[1])), ctx.plan)
        if kind == "msd":
            ctx.msd_start(interval, lags, 1, molecules=what, max_samples=1 << 20)
            info[name] = (ctx.msd_info().num_units, ctx.msd_info().num_origins, 4)
        elif kind == "acf":
            ctx.acf_start(interval, lags, 1, mode=what, pairs=pairs if what == "orientation" else None, max_samples=1 << 20)
            lay = ctx.acf_info()
            info[name] = (lay.num_units, lay.num_origins, lay.row_words)
        ctx.run_graph(WARM, 50); ctx.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(stream)
        ctx.run_graph(steps, 50)
        end.record(stream)
        end.synchronize()
        ctx.synchronize()
        times.setdefault(name, []).append(begin.elapsed_time(end))
        if kind == "acf":
            a = ctx.acf_read()
            assert (a.samples, a.dropped) == ((WARM + steps) // interval, 0), (name, a.samples, a.dropped)
    if parent_lib:      # like with like: both libraries in a fresh child process each, the order alternating
        for lib in ((parent_lib, H.LIB_PATH) if r % 2 == 0 else (H.LIB_PATH, parent_lib)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "off", str(steps), cfg], env=dict(os.environ, VVHIP_LIB=lib),
                                 capture_output=True, text=True, timeout=600, check=True).stdout
            (parent_times if lib == parent_lib else child_times).append(float(out.split()[-1]))
ctx.close()
if mode == "off":
    print(f"off {times['off'][0]:.4f}")
    sys.exit(0)
if mode == "trace":
    sys.exit(0)
base = np.median(times["off"])
samples = steps // interval
for name, kind, what, lags in SETTINGS:
    v = np.array(times[name])
    line = f"{cfg} {name:>28}: median {np.median(v):8.2f} ms for {steps} steps ({1e3 * steps / np.median(v):9.1f} steps/s; min {v.min():8.2f}, max {v.max():8.2f})"
    if kind:
        per = 1e3 * (np.median(v) - base) / samples                  # us per sample
        units, R, W = info[name]
        live = lags - 1 if kind == "acf" else lags                   # slots a steady-state sample reads
        moved = units * 24 * (live + 1)                              # ring reads and the one store
        line += f"  {per:8.2f} us per sample; {units} units, {R} slots, {W} words per row, ring traffic {moved / 1e6:7.2f} MB"
        if per > 0:
            line += f" -> {moved / per / 1e3:7.1f} GB/s over the whole sample"
    print(line + f"   [{', '.join(f'{x:.2f}' for x in v)}]", flush=True)
if parent_times:
    v, w = np.array(parent_times), np.array(child_times)
    print(f"{cfg} {'parent library, off, child':>28}: median {np.median(v):8.2f} ms ({1e3 * steps / np.median(v):9.1f} steps/s; min {v.min():8.2f}, max {v.max():8.2f})   [{', '.join(f'{x:.2f}' for x in v)}]", flush=True)
    print(f"{cfg} {'this library, off, child':>28}: median {np.median(w):8.2f} ms ({1e3 * steps / np.median(w):9.1f} steps/s; min {w.min():8.2f}, max {w.max():8.2f})   [{', '.join(f'{x:.2f}' for x in w)}]; "
          f"its median is {'inside' if v.min() <= np.median(w) <= v.max() else 'OUTSIDE'} the parent's spread", flush=True)
