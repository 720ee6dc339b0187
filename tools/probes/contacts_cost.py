"""Cost of the device-side contact recorder (Context.contacts_start) inside graph runs, per sample, at full-size C3 in mixed precision:
device events around the same run_graph call with the recorder off and with it sampling every `interval` steps -- one site per ion (the
first particle of every cation | anion by its molecule's net charge; about 3 000 x 3 000), one class cation - anion with the cutoff at the
first minimum of their g(r) (taken from a short RDF recording on the same context), lags 100 and 1 000 with origin_every 1 and 10, each
with and without the zero-word skip (vvhip_debug_tune "contacts_skip_zero").  The yardsticks run beside them on the same context: the MSD
particle-mode sample with one origin on record and the current sample (tools/probes/msd_cost.py, current_cost.py), whose kernels stream
bytes at 1.15 - 1.19 TB/s.  One context; the settings take turns on it, in reversed order every other repeat, each warmed up untimed
first so that its graphs are captured and the rings are full outside the timed region.  Per setting: the median time, the cost per sample
against `off`, the bytes the correlate kernel must move at the least -- per live slot the origin words, and for the non-zero ones the
sample's and the surviving words, 8 B each -- and the rate that the whole sample's cost amounts to (the kernels' own times come from a
kernel trace of the `trace` mode: the correlate kernel's bytes / its own time is the figure to put beside the MSD and current kernels').
Then the only alternative a user has without the recorder: tests/contacts_reference.py (NumPy) on a downloaded float64 frame.
usage: python tools/probes/contacts_cost.py [repeats] [steps] [interval] [config]      the timing
       python tools/probes/contacts_cost.py trace [config]      200 samples per setting and nothing else (for rocprofv3 --kernel-trace --stats)"""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import contacts_reference as CR

args = sys.argv[1:]
trace = len(args) > 0 and args[0] == "trace"
if trace:
    rep, steps, interval, cfg = 1, 2000, 10, args[1] if len(args) > 1 else "C3"
else:
    rep = int(args[0]) if len(args) > 0 else 5
    steps = int(args[1]) if len(args) > 1 else 10000
    interval = int(args[2]) if len(args) > 2 else 10
    cfg = args[3] if len(args) > 3 else "C3"
WARM = 2000 if trace else 10000      # (1000 samples at the default interval: every slot of the longest ring holds an origin)
# (name, kind, num_lags, origin_every, skip)
SETTINGS = [("off", None, 0, 0, 1), ("msd/particles-1", "msd", 1, 1, 1), ("current/E1", "current", 1000, 1, 1)]
SETTINGS += [(f"contacts/L{l}/E{e}{'' if skip else '/no-skip'}", "contacts", l, e, skip) for skip in (1, 0) for l in (100, 1000) for e in (1, 10)]
if trace:
    SETTINGS = SETTINGS[1:]

pkg = importlib.import_module("openmm-velocityverlet_amd")
I, S, H = pkg.integrator, pkg.systems, pkg.vvhip
spec = S.make_config(cfg)
n = spec.num_atoms
mol = np.asarray(spec.mol_id)
Q = np.bincount(mol, weights=np.asarray(spec.charges, dtype=np.float64))
first = np.zeros(n, dtype=bool)
first[np.unique(mol, return_index=True)[1]] = True
groups = np.where(first & (Q[mol] > 0.5), 0, np.where(first & (Q[mol] < -0.5), 1, -1)).astype(np.int8)
ions = np.where(Q[mol] > 0.5, 0, np.where(Q[mol] < -0.5, 1, -1)).astype(np.int8)
na, nb = int(np.count_nonzero(groups == 0)), int(np.count_nonzero(groups == 1))
it = I.VVIntegrator(333.0, 10, 1.0, 40, 0.001)
it.setMaxDrudeDistance(0.02)
stream = torch.cuda.Stream()
ctx = I.Context(spec, it, precision="mixed", force_provider="tether", stream=stream.cuda_stream)
ctx.run_graph(2000, 50); ctx.synchronize()
# the cutoff: the first minimum of the cation - anion g(r) behind its first maximum, from 20 samples
ctx.rdf_start(10, min(1.2, 0.45 * float(min(spec.box))), 120, [(0, 1)], groups=groups)
ctx.run_graph(200, 50)
rdf = ctx.rdf_read()
ctx.rdf_stop()
g = rdf.g()[0]
peak = int(np.argmax(g))
r_cut = float(rdf.r[peak + int(np.argmin(g[peak:peak + 40]))])
print(f"{cfg}: {n} particles, {na} x {nb} sites, cutoff {r_cut:.3f} nm (g peaks at {rdf.r[peak]:.3f} nm), interval {interval}", flush=True)
times, info = {}, {}
for r in range(rep):
    for name, kind, lags, every, skip in (SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
        ctx.msd_stop(); ctx.current_stop(); ctx.contacts_stop()
        H.check(H.lib.vvhip_debug_tune(ctx.plan, b"contacts_skip_zero", skip), ctx.plan)
        if kind == "msd":
            ctx.msd_start(interval, 1, 1, max_samples=1 << 20)
        elif kind == "current":
            ctx.current_start(interval, lags, every, groups=ions, max_samples=1 << 20)
        elif kind == "contacts":
            ctx.contacts_start(interval, lags, [(0, 1)], [r_cut], origin_every=every, groups=groups, max_samples=1 << 20)
            lay = ctx.contacts_info()
            info[name] = (lay.num_origins, int(lay.sample_words), int(lay.total_bytes), lay.num_mask_items, lay.num_corr_items)
        ctx.run_graph(WARM, 50); ctx.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(stream)
        ctx.run_graph(steps, 50)
        end.record(stream)
        end.synchronize()
        ctx.synchronize()
        times.setdefault(name, []).append(begin.elapsed_time(end))
        if kind == "contacts":
            c = ctx.contacts_read()
            assert (c.samples, c.dropped, c.invalid) == ((WARM + steps) // interval, 0, 0), (name, c.samples, c.dropped, c.invalid)
            info[name] += (c.mean_contacts(0),)
if trace:
    ctx.close()
    sys.exit(0)
ctx.msd_stop(); ctx.current_stop(); ctx.contacts_stop()
host_samples = 4
ctx.frames_start(interval, capacity=host_samples, float64=True)
ctx.contacts_start(interval, 4, [(0, 1)], [r_cut], groups=groups)
ctx.run_graph(host_samples * interval, 50)
f, c = ctx.frames_read(), ctx.contacts_read()
ctx.close()
base = np.median(times["off"])
samples = steps // interval
for name, kind, lags, every, skip in SETTINGS:
    v = np.array(times[name])
    line = f"{cfg} {name:>28}: median {np.median(v):8.2f} ms for {steps} steps ({1e3 * steps / np.median(v):9.1f} steps/s; min {v.min():8.2f}, max {v.max():8.2f})"
    if kind:
        per = 1e3 * (np.median(v) - base) / samples                  # us per sample
        line += f"  {per:8.2f} us per sample"
    if kind == "contacts":
        R, words, total, nm, nc, mean = info[name]
        dense = min(1.0, mean * na / max(1, words))                   # the share of non-zero words, at the most (one contact per word)
        moved = R * words * 8 * (1 + (0 if skip else 2)) + (R * words * 8 * 2 * dense if skip else 0)
        line += f", {R} slots x {words * 8 / 1e6:.2f} MB ({total / 1e6:.0f} MB in all), {mean:.2f} contacts per cation, correlate moves >= {moved / 1e6:8.1f} MB -> {moved / per / 1e3:7.1f} GB/s over the whole sample; {nm} + {nc} x {R} blocks"
    print(line + f"   [{', '.join(f'{x:.2f}' for x in v)}]", flush=True)
# the host's alternative: NumPy on downloaded frames
t0 = time.perf_counter()
want = CR.contacts_reference(f.positions, f.box, groups, [(0, 1)], [r_cut], 4, 1)
t_host = (time.perf_counter() - t0) / host_samples
assert np.array_equal(c.words, want[0]) and c.samples == host_samples
print(f"{cfg} NumPy reference: {1e3 * t_host:8.3f} ms per sample for the {na} x {nb} matrix and four lags from a downloaded float64 frame of {24 * n / 1e6:.2f} MB; "
      f"the device's table of these {host_samples} samples equals it bit for bit; OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}", flush=True)
