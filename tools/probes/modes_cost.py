"""Cost of the device-side density-mode recorder (Context.modes_start) inside graph runs, per sample, at full-size C3 in mixed precision:
device events around the same run_graph call with the recorder off and with it sampling every `interval` steps.  Workloads:
  a  the ions of the box in two groups (cations | anions by their molecule's net charge), the charges as weights, 256 modes, num_lags 0
  b  the same with 1 000 lags, every sample an origin
  c  all particles in one group, unit weights, 512 modes, num_lags 0
One context; the settings take turns on it, in reversed order every other repeat, each warmed up untimed first so that its graphs are
captured and the ring is full outside the timed region.  Per setting: the median time, the cost per sample against `off`, the (site, mode)
pairs per second that the whole sample's cost amounts to (the kernels' own times come from a kernel trace of the `trace` mode).  Then the
only alternative a user has without the recorder: tests/modes_reference.py (NumPy) on a downloaded float64 frame, timed per sample; the
device's table of those samples must equal it bit for bit.  `scan KEY V1 V2 ..` times workloads a and c under vvhip_debug_tune KEY = each
value (modes_sites_per_thread, modes_k_tile, modes_block_threads).
usage: python tools/probes/modes_cost.py [repeats] [steps] [interval] [config]      the timing
       python tools/probes/modes_cost.py trace [config]      200 samples per setting and nothing else (for rocprofv3 --kernel-trace --stats)
       python tools/probes/modes_cost.py scan KEY V1 [V2 ..]"""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import modes_reference as MR

args = sys.argv[1:]
trace = len(args) > 0 and args[0] == "trace"
scan = len(args) > 1 and args[0] == "scan"
rep, steps, interval, cfg = 5, 20000, 10, "C3"
if trace:
    rep, steps, cfg = 1, 2000, args[1] if len(args) > 1 else "C3"
elif scan:
    rep, steps, scan_key, scan_values = 3, 5000, args[1], [int(v) for v in args[2:]]
else:
    rep = int(args[0]) if len(args) > 0 else rep
    steps = int(args[1]) if len(args) > 1 else steps
    interval = int(args[2]) if len(args) > 2 else interval
    cfg = args[3] if len(args) > 3 else cfg
WARM = 2000 if (trace or scan) else 10000      # (1000 samples at the default interval: every slot of the longest ring holds an origin)

pkg = importlib.import_module("openmm-velocityverlet_amd")
I, S, H = pkg.integrator, pkg.systems, pkg.vvhip
spec = S.make_config(cfg)
n = spec.num_atoms
mol = np.asarray(spec.mol_id)
Q = np.bincount(mol, weights=np.asarray(spec.charges, dtype=np.float64))
ions = np.where(Q[mol] > 0.5, 0, np.where(Q[mol] < -0.5, 1, -1)).astype(np.int8)
charges = np.asarray(spec.charges, dtype=np.float64)
all_modes = I.modes_in_shells(spec.box, 40.0, max_per_shell=6)
assert len(all_modes) >= 512, len(all_modes)
# (name, groups, weights, modes, num_lags, tune)
WORK = {"a": ("a/ions-256-lags0", ions, charges, all_modes[:256], 0), "b": ("b/ions-256-lags1000", ions, charges, all_modes[:256], 1000),
        "c": ("c/all-512-lags0", None, None, all_modes[:512], 0)}
if scan:
    SETTINGS = [("off", None, None)] + [(f"{WORK[k][0]}/{scan_key}={v}", k, {scan_key: v}) for k in "ac" for v in scan_values]
else:
    SETTINGS = [("off", None, None)] + [(WORK[k][0], k, None) for k in "abc"]
if trace:
    SETTINGS = SETTINGS[1:]

it = I.VVIntegrator(333.0, 10, 1.0, 40, 0.001)
it.setMaxDrudeDistance(0.02)
stream = torch.cuda.Stream()
ctx = I.Context(spec, it, precision="mixed", force_provider="tether", stream=stream.cuda_stream)
ctx.run_graph(2000, 50); ctx.synchronize()
print(f"{cfg}: {n} particles, {int(np.count_nonzero(ions >= 0))} ions ({int(np.count_nonzero(ions == 0))} | {int(np.count_nonzero(ions == 1))}), interval {interval}", flush=True)
times, info = {}, {}
for r in range(rep):
    for name, work, tune in (SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
        ctx.modes_stop()
        for key in ("modes_sites_per_thread", "modes_k_tile", "modes_block_threads"):
            H.check(H.lib.vvhip_debug_tune(ctx.plan, key.encode(), int((tune or {}).get(key, 0))), ctx.plan)
        if work:
            _, groups, weights, modes, num_lags = WORK[work]
            ctx.modes_start(interval, modes, num_lags=num_lags, origin_every=1, weights=weights, groups=groups, max_samples=1 << 20)
            lay = ctx.modes_info()
            info[name] = (lay.num_particles, lay.num_modes, lay.num_items, lay.sites_per_thread, lay.k_tile, lay.block_threads, lay.num_origins, lay.row_words)
        ctx.run_graph(WARM, 50); ctx.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(stream)
        ctx.run_graph(steps, 50)
        end.record(stream)
        end.synchronize()
        ctx.synchronize()
        times.setdefault(name, []).append(begin.elapsed_time(end))
        if work:
            d = ctx.modes_read()
            assert (d.samples, d.dropped, d.out_of_range, d.invalid_samples) == ((WARM + steps) // interval, 0, 0, 0), (name, d.samples, d.dropped, d.out_of_range)
            assert d.count[0] == d.samples and (num_lags == 0 or d.count[num_lags] == d.samples - num_lags)
if trace:
    ctx.close()
    sys.exit(0)
base = np.median(times["off"])
samples = steps // interval
for name, work, tune in SETTINGS:
    v = np.array(times[name])
    line = f"{cfg} {name:>40}: median {np.median(v):8.2f} ms for {steps} steps ({1e3 * steps / np.median(v):9.1f} steps/s; min {v.min():8.2f}, max {v.max():8.2f})"
    if work:
        per = 1e3 * (np.median(v) - base) / samples                  # us per sample
        sites, K, items, P, kt, threads, origins, row = info[name]
        line += (f"  {per:7.2f} us per sample, {sites} sites x {K} modes -> {sites * K / per / 1e3:7.2f} G pairs/s over the whole sample; {items} items of "
                 f"{threads} threads x {P} sites x {kt} modes, {origins} origins x {row - 1} cells")
    print(line + f"   [{', '.join(f'{x:.2f}' for x in v)}]", flush=True)
if scan:
    ctx.close()
    sys.exit(0)
# the host's alternative: NumPy on downloaded frames, for workloads a and c
for work in "ac":
    _, groups, weights, modes, num_lags = WORK[work]
    host_samples = 4
    ctx.modes_stop(); ctx.frames_stop()
    ctx.frames_start(interval, capacity=host_samples, float64=True)
    ctx.modes_start(interval, modes, num_lags=0, weights=weights, groups=groups, max_samples=1 << 20)
    lay = ctx.modes_info()
    ctx.run_graph(host_samples * interval, 50)
    f, d = ctx.frames_read(), ctx.modes_read()
    w = np.ones(n) if weights is None else weights
    t0 = time.perf_counter()
    want = MR.modes_reference(f.positions, f.box, w, groups, lay.num_groups, modes, 0, 1, lay.frac_bits, lay.limit_position)
    t_host = (time.perf_counter() - t0) / host_samples
    assert np.array_equal(d.words, want["words"]) and d.samples == host_samples
    print(f"{cfg} NumPy reference, workload {work}: {1e3 * t_host:9.2f} ms per sample for {lay.num_particles} sites x {lay.num_modes} modes from a downloaded float64 "
          f"frame of {24 * n / 1e6:.2f} MB; the device's table of these {host_samples} samples equals it bit for bit; OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}", flush=True)
ctx.close()
