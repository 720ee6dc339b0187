"""Cost of the device-side current recorder (Context.current_start) inside graph runs, per sample, at full-size C3 in mixed precision:
device events around the same run_graph call with the recorder off and with it sampling every `interval` steps -- the charges as weights,
G = 2 (the particles of cations | anions by their molecule's net charge; neutral molecules are not recorded), num_lags 1000 with
origin_every 1 and 10 -- each with the reduce's agent-scope adds and in its two-level form (vvhip_debug_tune "current_two_level").  The
yardstick runs beside them on the same context: the MSD particle-mode sample with one origin on record (tools/probes/msd_cost.py:
particles-1), which streams bytes of the same order.  One context; the settings take turns on it, in reversed order every other repeat,
each warmed up untimed first so that its graphs are captured and the ring is full outside the timed region.  Per setting: the median
time, the cost per sample against `off`, the bytes the reduce must load -- per recorded particle 4 (index) + 8 (weight) + 1 (group) + 16
(posq) + 16 (correction) + 32 (velm) = 77 B -- and the rate that the whole sample's cost amounts to (the kernels' own times come from a
kernel trace of the `trace` mode).  Then the only alternative a user has without the recorder: tests/current_reference.py (NumPy) on
downloaded float64 frames, timed over `host_samples` samples and scaled.
usage: python tools/probes/current_cost.py [repeats] [steps] [interval] [config]      the timing
       python tools/probes/current_cost.py trace [config]      200 samples per setting and nothing else (for rocprofv3 --kernel-trace --stats)"""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import current_reference as CR

args = sys.argv[1:]
trace = len(args) > 0 and args[0] == "trace"
if trace:
    rep, steps, interval, cfg = 1, 2000, 10, args[1] if len(args) > 1 else "C3"
else:
    rep = int(args[0]) if len(args) > 0 else 5
    steps = int(args[1]) if len(args) > 1 else 20000
    interval = int(args[2]) if len(args) > 2 else 10
    cfg = args[3] if len(args) > 3 else "C3"
WARM = 2000 if trace else 10000      # (1000 samples at the default interval: every slot of the longest ring holds an origin)
NUM_LAGS = 1000
# (name, kind, origin_every, two-level)
SETTINGS = [("off", None, 0, 0), ("msd/particles-1", "msd", 1, 0)]
SETTINGS += [(f"current/E{e}{'/two-level' if two else ''}", "current", e, two) for two in (0, 1) for e in (1, 10)]
if trace:
    SETTINGS = SETTINGS[1:]

pkg = importlib.import_module("openmm-velocityverlet_amd")
I, S, H = pkg.integrator, pkg.systems, pkg.vvhip
spec = S.make_config(cfg)
n = spec.num_atoms
mol = np.asarray(spec.mol_id)
Q = np.bincount(mol, weights=np.asarray(spec.charges, dtype=np.float64))
groups = np.where(Q[mol] > 0.5, 0, np.where(Q[mol] < -0.5, 1, -1)).astype(np.int8)
weights = I.current_weights(spec)
recorded = int(np.count_nonzero(groups >= 0))
it = I.VVIntegrator(333.0, 10, 1.0, 40, 0.001)
it.setMaxDrudeDistance(0.02)
stream = torch.cuda.Stream()
ctx = I.Context(spec, it, precision="mixed", force_provider="tether", stream=stream.cuda_stream)
ctx.run_graph(2000, 50); ctx.synchronize()
print(f"{cfg}: {n} particles, {recorded} recorded ({int(np.count_nonzero(groups == 0))} | {int(np.count_nonzero(groups == 1))}), num_lags {NUM_LAGS}, interval {interval}", flush=True)
times, info = {}, {}
for r in range(rep):
    for name, kind, every, two in (SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
        ctx.msd_stop(); ctx.current_stop()
        H.check(H.lib.vvhip_debug_tune(ctx.plan, b"current_two_level", two), ctx.plan)
        if kind == "msd":
            ctx.msd_start(interval, 1, 1, max_samples=1 << 20)
        elif kind == "current":
            ctx.current_start(interval, NUM_LAGS, every, groups=groups, max_samples=1 << 20)
            lay = ctx.current_info()
            info[name] = (lay.num_origins, lay.row_words, lay.frac_bits_position, lay.frac_bits_velocity)
        ctx.run_graph(WARM, 50); ctx.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(stream)
        ctx.run_graph(steps, 50)
        end.record(stream)
        end.synchronize()
        ctx.synchronize()
        times.setdefault(name, []).append(begin.elapsed_time(end))
        if kind == "current":
            c = ctx.current_read()
            assert (c.samples, c.dropped, c.out_of_range, c.invalid_samples) == ((WARM + steps) // interval, 0, 0, 0), (name, c.samples, c.dropped, c.out_of_range)
            assert np.array_equal(c.count, CR.lag_counts(c.samples, every, NUM_LAGS))
if trace:
    ctx.close()
    sys.exit(0)
ctx.msd_stop(); ctx.current_stop()
host_samples = 64
ctx.frames_start(interval, capacity=host_samples, velocities=True, float64=True)
ctx.current_start(interval, 8, 1, groups=groups, max_samples=1 << 20)
lay = ctx.current_info()
ctx.run_graph(host_samples * interval, 50)
f, c = ctx.frames_read(), ctx.current_read()
ctx.close()
base = np.median(times["off"])
samples = steps // interval
for name, kind, every, two in SETTINGS:
    v = np.array(times[name])
    line = f"{cfg} {name:>24}: median {np.median(v):8.2f} ms for {steps} steps ({1e3 * steps / np.median(v):9.1f} steps/s; min {v.min():8.2f}, max {v.max():8.2f})"
    if kind:
        per = 1e3 * (np.median(v) - base) / samples                  # us per sample
        moved = (2 * 24 + 32) * n if kind == "msd" else 77 * recorded
        line += f"  {per:7.2f} us per sample, {moved / 1e6:6.2f} MB to load -> {moved / per / 1e3:7.1f} GB/s over the whole sample"
        if kind == "current":
            line += f", {info[name][0]} origins x {info[name][1] - 1} cells"
    print(line + f"   [{', '.join(f'{x:.2f}' for x in v)}]", flush=True)
# the host's alternative: NumPy on downloaded frames
t0 = time.perf_counter()
per = [CR.sample_sums(x, v, weights, groups, 2, lay.frac_bits_position, lay.frac_bits_velocity, lay.limit_position, lay.limit_velocity) for x, v in zip(f.positions, f.velocities)]
t_sums = (time.perf_counter() - t0) / host_samples
sums = np.array([s for s, _ in per]); bad = np.array([b for _, b in per])
box = f.box
want = CR.correlate(sums, bad, 2, 8, 1, lay.frac_bits_position, lay.frac_bits_velocity, inv_volume=1.0 / ((box[:, 0] * box[:, 1]) * box[:, 2]))
assert np.array_equal(c.words, want["words"]) and c.samples == host_samples
def correlate_seconds(J):
    t0 = time.perf_counter()
    CR.correlate(np.zeros((J, 2, 6), dtype=np.int64), np.zeros(J, dtype=np.int64), 2, NUM_LAGS, 1, 40, 40)
    return time.perf_counter() - t0
t_corr = (correlate_seconds(NUM_LAGS + 100) - correlate_seconds(NUM_LAGS)) / 100      # (per sample once every slot of the ring holds an origin)
frame_bytes = 48 * n
print(f"{cfg} NumPy reference: {1e3 * t_sums:8.3f} ms per sample for the sums of {recorded} particles from a downloaded float64 frame of {frame_bytes / 1e6:.2f} MB, "
      f"{1e3 * t_corr:8.3f} ms per sample for the {NUM_LAGS} lags (E = 1); the device's table of these {host_samples} samples equals it bit for bit; "
      f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}", flush=True)
