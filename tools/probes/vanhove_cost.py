"""Cost of the device-side self van Hove recorder (Context.vanhove_start) inside graph runs, per sample, at full-size C3 in mixed
precision: device events around the same run_graph call (20 000 steps as replays of 50-step graphs) with the recorder off and with it
sampling -- the molecules' centres of mass in 128 logarithmic bins, 1 000 lags, every tenth sample an origin (100 ring slots), at interval
10 and at interval 100; the same with every increment a global add ("vanhove_lds" = 0); particle mode for the ions only (every particle of
a molecule with a net charge, cations and anions as two groups) -- and the host alternative beside them: the frame recorder in float64 at
the same steps, and tests/vanhove_reference.py in NumPy over a short stretch of those frames, scaled to one sample's pairs.  One context;
the settings take turns on it, in reversed order every other repeat, each warmed up untimed first so that its graphs are captured and the
ring is full outside the timed region.  Per setting: the median time, the cost per sample against `off`, the increments a sample makes and
the rate the whole sample's cost amounts to.  The condition it checks: the privatised path is no slower than the plain one.
With a second library given (the parent commit's build), every repeat also times `off` on it and on this library in a fresh child process
each, the order alternating (the library is chosen when the package is imported: VVHIP_LIB), so that "recorder off" can be put beside the
parent's own run-to-run spread on one box, like with like.
usage: python tools/probes/vanhove_cost.py [repeats] [steps] [config] [parent library]      the timing
       python tools/probes/vanhove_cost.py off [steps] [config]      one timed run with nothing on, one line (what the child processes run)"""
import importlib, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

args = sys.argv[1:]
mode = "off" if args and args[0] == "off" else "time"
parent_lib = None
if mode == "off":
    rep, steps, cfg = 1, int(args[1]) if len(args) > 1 else 20000, args[2] if len(args) > 2 else "C3"
else:
    rep = int(args[0]) if len(args) > 0 else 5
    steps = int(args[1]) if len(args) > 1 else 20000
    cfg = args[2] if len(args) > 2 else "C3"
    parent_lib = args[3] if len(args) > 3 else None
LAGS, EVERY, BINS = 1000, 10, 128
# (name, kind, molecules, interval, vanhove_lds)
SETTINGS = [("off", None, None, 0, 1),
            ("vanhove/molecules/i10", "vanhove", True, 10, 1), ("vanhove/molecules/i100", "vanhove", True, 100, 1),
            ("vanhove/molecules/i10/plain", "vanhove", True, 10, 0), ("vanhove/molecules/i100/plain", "vanhove", True, 100, 0),
            ("vanhove/ions/i10", "vanhove", False, 10, 1), ("vanhove/ions/i10/plain", "vanhove", False, 10, 0),
            ("frames/float64/i10", "frames", None, 10, 1)]
if mode == "off":
    SETTINGS = SETTINGS[:1]

pkg = importlib.import_module("openmm-velocityverlet_amd")
I, S, H = pkg.integrator, pkg.systems, pkg.vvhip
spec = S.make_config(cfg)
n = spec.num_atoms
mol = np.asarray(spec.mol_id)
Q = np.bincount(mol, weights=np.asarray(spec.charges, dtype=np.float64))
ions = np.where(Q[mol] > 0.5, 0, np.where(Q[mol] < -0.5, 1, -1)).astype(np.int8)
it = I.VVIntegrator(333.0, 10, 1.0, 40, 0.001)
it.setMaxDrudeDistance(0.02)
stream = torch.cuda.Stream()
ctx = I.Context(spec, it, precision="mixed", force_provider="tether", stream=stream.cuda_stream)
ctx.run_graph(2000, 50); ctx.synchronize()
has_recorder = hasattr(ctx, "vanhove_stop") and "vvhip_vanhove_stop" in H.EXPORTS      # (the parent's library has none)
edges = I.vanhove_edges(2.0, BINS, 1e-4) if has_recorder else None
if mode != "off":
    print(f"{cfg}: {n} particles, {LAGS} lags, every {EVERY}th sample an origin, {BINS} logarithmic bins, {steps} steps per run, library {os.path.relpath(H.LIB_PATH, ROOT)}", flush=True)
times, info, parent_times, child_times = {}, {}, [], []
for r in range(rep):
    for name, kind, molecules, interval, lds in (SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
        if has_recorder:
            ctx.vanhove_stop()
        ctx.frames_stop()
        warm = 2000
        if kind == "vanhove":
            H.check(H.lib.vvhip_debug_tune(ctx.plan, b"vanhove_lds", lds), ctx.plan)
            ctx.vanhove_start(interval, LAGS, edges, EVERY, molecules=molecules, groups=None if molecules else ions, max_samples=1 << 20)
            lay = ctx.vanhove_info()
            info[name] = (lay.num_units, lay.num_origins, lay.words)
            warm = LAGS * interval                                   # the ring full: every slot live in the timed region
        elif kind == "frames":
            ctx.frames_start(interval, capacity=8, float64=True)      # (a ring of eight: the cost of writing a frame, not of keeping them)
        ctx.run_graph(warm, 50); ctx.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(stream)
        ctx.run_graph(steps, 50)
        end.record(stream)
        end.synchronize()
        ctx.synchronize()
        times.setdefault(name, []).append(begin.elapsed_time(end))
        if kind == "vanhove":
            v = ctx.vanhove_read()
            assert (v.samples, v.dropped, v.out_of_range) == ((warm + steps) // interval, 0, 0), (name, v.samples, v.dropped, v.out_of_range)
            assert np.array_equal(v.below + v.hist.sum(axis=2) + v.beyond, v.pairs)
    if parent_lib:      # like with like: both libraries in a fresh child process each, the order alternating
        for lib in ((parent_lib, H.LIB_PATH) if r % 2 == 0 else (H.LIB_PATH, parent_lib)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "off", str(steps), cfg], env=dict(os.environ, VVHIP_LIB=lib),
                                 capture_output=True, text=True, timeout=600, check=True).stdout
            (parent_times if lib == parent_lib else child_times).append(float(out.split()[-1]))
if mode == "off":
    ctx.close()
    print(f"off {times['off'][0]:.4f}")
    sys.exit(0)
# the host alternative's second half: the NumPy reference over twelve float64 frames of the molecules' centres, every pair of them one
# (sample, origin) pair as the recorder counts them; a steady-state sample has num_origins of those
import vanhove_reference as VR
ctx.vanhove_stop(); ctx.frames_stop()
ctx.frames_start(10, capacity=12, float64=True)
ctx.run_graph(120, 50)
f = ctx.frames_read()
ctx.close()
masses = np.asarray(spec.masses, dtype=np.float64)
units = VR.molecule_units(masses, mol)
c = np.array([VR.unit_positions(x, masses, mol, None, True, units)[0] for x in f.positions])
t0 = time.perf_counter()
head, hist, out = VR.vanhove_reference(c, np.zeros(c.shape[1], dtype=int), 1, 11, 1, edges, (30, 20, 40), 16.0)
numpy_per_pair = (time.perf_counter() - t0) / len(VR.pairs(12, 1, 11))
base = np.median(times["off"])
medians = {}
for name, kind, molecules, interval, lds in SETTINGS:
    v = np.array(times[name])
    medians[name] = np.median(v)
    line = f"{cfg} {name:>30}: median {np.median(v):8.2f} ms for {steps} steps ({1e3 * steps / np.median(v):9.1f} steps/s; min {v.min():8.2f}, max {v.max():8.2f})"
    if kind == "vanhove":
        per = 1e3 * (np.median(v) - base) / (steps // interval)      # us per sample
        units_, R, words = info[name]
        line += f"  {per:8.2f} us per sample; {units_} units x {R} slots = {units_ * R} increments, ring reads {units_ * 24 * R / 1e6:6.2f} MB, table {words * 8 / 1e6:.2f} MB"
        if per > 0:
            line += f" -> {units_ * R / per / 1e3:7.2f} G increments/s over the whole sample"
    elif kind == "frames":
        per = 1e3 * (np.median(v) - base) / (steps // interval)
        line += f"  {per:8.2f} us per frame of {n * 24 / 1e6:.2f} MB on the device; NumPy over its units: {numpy_per_pair * 1e3:.2f} ms per (sample, origin) pair, {numpy_per_pair * (LAGS // EVERY):.2f} s per sample of {LAGS // EVERY} origins"
    print(line + f"   [{', '.join(f'{x:.2f}' for x in v)}]", flush=True)
for a, b in (("vanhove/molecules/i10", "vanhove/molecules/i10/plain"), ("vanhove/molecules/i100", "vanhove/molecules/i100/plain"), ("vanhove/ions/i10", "vanhove/ions/i10/plain")):
    print(f"{cfg} {a}: the privatised path is {'no slower than' if medians[a] <= medians[b] else 'SLOWER than'} the plain path ({medians[a]:.2f} ms against {medians[b]:.2f} ms)", flush=True)
if parent_times:
    v, w = np.array(parent_times), np.array(child_times)
    print(f"{cfg} {'parent library, off, child':>30}: median {np.median(v):8.2f} ms ({1e3 * steps / np.median(v):9.1f} steps/s; min {v.min():8.2f}, max {v.max():8.2f})   [{', '.join(f'{x:.2f}' for x in v)}]", flush=True)
    print(f"{cfg} {'this library, off, child':>30}: median {np.median(w):8.2f} ms ({1e3 * steps / np.median(w):9.1f} steps/s; min {w.min():8.2f}, max {w.max():8.2f})   [{', '.join(f'{x:.2f}' for x in w)}]; "
          f"its median is {'inside' if v.min() <= np.median(w) <= v.max() else 'OUTSIDE'} the parent's spread", flush=True)
