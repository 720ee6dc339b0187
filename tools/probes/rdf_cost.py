"""Cost of the device-side RDF recorder (Context.rdf_start) inside graph runs, per sample, at full-size C3: device events around the
same run_graph call with the recorder off and with it sampling every `interval` steps, for two workloads --
  (a) ions:  one atom per molecule (its first), two groups by the molecule's parity, the classes (0,1), (0,0), (1,1), r_max 1.5 nm, 300 bins;
  (b) all:   every particle against every other, r_max = min(L) / 2, 300 bins --
each with one private histogram per block and with one per wave (vvhip_debug_tune "rdf_hist_copies").  One context; the settings take
turns on it, in reversed order every other repeat, each warmed up untimed first so that its graphs are captured outside the timed region.
Per setting: the median time, the cost per sample against `off`, the pairs per second and the share of the pairs that were in range.  Then
the only alternative a user has without the recorder: tests/rdf_reference.py (NumPy) on one downloaded float64 frame, timed on the whole
of (a) and on the first 2 048 sites against all of (b), scaled to its pairs.
usage: python tools/probes/rdf_cost.py [repeats] [config]          the timing
       python tools/probes/rdf_cost.py pmc [config]                two samples per setting through rdf_sample and nothing else (for a counter run)"""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import rdf_reference as RR

args = sys.argv[1:]
pmc = len(args) > 0 and args[0] == "pmc"
rep = 3 if pmc or len(args) < 1 else int(args[0])
cfg = args[1] if len(args) > 1 else "C3"
WARM = 1000

pkg = importlib.import_module("openmm-velocityverlet_amd")
I, S, H = pkg.integrator, pkg.systems, pkg.vvhip
spec = S.make_config(cfg)
n = spec.num_atoms
mol = np.asarray(spec.mol_id)
first = np.nonzero(np.diff(np.concatenate(([-1], mol))) != 0)[0]      # the first particle of every molecule
ions = np.full(n, -1, dtype=np.int8)
ions[first] = mol[first] % 2
half = float(min(spec.box)) / 2
# name -> (groups, classes, r_max, nbins, interval, steps)
WORK = {"ions": (ions, [(0, 1), (0, 0), (1, 1)], 1.5, 300, 10, 5000), "all": (None, [(0, 0)], half, 300, 100, 2000)}
SETTINGS = [("off", None, 1)] + [(f"{w}/{'block' if c == 1 else 'wave'}", w, c) for w in WORK for c in (1, 4)]

it = I.VVIntegrator(333.0, 10, 1.0, 40, 0.001)
it.setMaxDrudeDistance(0.02)
stream = torch.cuda.Stream()
ctx = I.Context(spec, it, precision="mixed", force_provider="tether", stream=stream.cuda_stream)
ctx.run_graph(WARM, 50); ctx.synchronize()


def start(work, copies):
    groups, classes, r_max, nbins, interval, _ = WORK[work]
    H.check(H.lib.vvhip_debug_tune(ctx.plan, b"rdf_hist_copies", copies), ctx.plan)
    ctx.rdf_start(interval, r_max, nbins, classes, groups=groups)


if pmc:
    for name, work, copies in SETTINGS[1:]:
        start(work, copies)
        ctx.rdf_sample(); ctx.rdf_sample()
        r = ctx.rdf_read()
        print(f"{cfg} rdf {name}: {r.samples} samples, {int(r.pairs_per_sample.sum())} pairs per sample, {int(r.counts.sum())} in range, {ctx.rdf_info().num_items} blocks", flush=True)
        ctx.rdf_stop()
    ctx.close()
    sys.exit(0)

times, info = {}, {}
for r in range(rep):
    for name, work, copies in (SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
        ctx.rdf_stop()
        for steps in sorted({w[5] for w in WORK.values()}) if work is None else [WORK[work][5]]:
            if work is not None:
                start(work, copies)
            ctx.run_graph(WARM, 50); ctx.synchronize()
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record(stream)
            ctx.run_graph(steps, 50)
            end.record(stream)
            end.synchronize()
            ctx.synchronize()
            times.setdefault((name, steps), []).append(begin.elapsed_time(end))
            if work is not None:
                m = ctx.rdf_read()
                assert (m.samples, m.dropped, m.invalid) == ((WARM + steps) // WORK[work][4], 0, 0), (name, m.samples, m.dropped, m.invalid)
                info[name] = (int(m.pairs_per_sample.sum()), int(m.counts.sum()) / (float(m.pairs_per_sample.sum()) * m.samples), ctx.rdf_info().num_items)
frame_ctx_positions = ctx.getPositions()
ctx.close()
for name, work, copies in SETTINGS:
    for steps in sorted({w[5] for w in WORK.values()}) if work is None else [WORK[work][5]]:
        v = np.array(times[(name, steps)])
        line = f"{cfg} rdf {name:>11}: median {np.median(v):9.2f} ms for {steps} steps ({1e3 * steps / np.median(v):9.1f} steps/s; min {v.min():9.2f}, max {v.max():9.2f})"
        if work is not None:
            samples = steps // WORK[work][4]
            per = 1e3 * (np.median(v) - np.median(times[("off", steps)])) / samples      # us per sample
            pairs, share, items = info[name]
            line += f"  {per:10.2f} us per sample, {pairs:.4g} pairs in {items} blocks -> {pairs / per / 1e6:8.3f} T pairs/s, {100 * share:5.2f} % in range"
        print(line + f"   [{', '.join(f'{x:.2f}' for x in v)}]", flush=True)
# the host's alternative: NumPy on a downloaded frame
x = frame_ctx_positions
groups, classes, r_max, nbins, _, _ = WORK["ions"]
t0 = time.perf_counter()
table, _ = RR.rdf_reference(x, spec.box, groups, classes, r_max, nbins)
t = time.perf_counter() - t0
pairs = int(RR.pairs_per_sample(groups, classes).sum())
print(f"{cfg} rdf NumPy reference, ions: {t:8.3f} s per sample for {pairs:.4g} pairs ({pairs / t / 1e6:.1f} M pairs/s), OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}", flush=True)
t0 = time.perf_counter()
RR.histogram(x[:2048], x, spec.box, half, 300)
t = time.perf_counter() - t0
pairs_all = n * (n - 1) // 2
print(f"{cfg} rdf NumPy reference, all: {t:8.3f} s for 2048 x {n} pairs ({2048 * n / t / 1e6:.1f} M pairs/s) -> {t * pairs_all / (2048 * n):8.1f} s per sample of {pairs_all:.4g} pairs (scaled)", flush=True)
