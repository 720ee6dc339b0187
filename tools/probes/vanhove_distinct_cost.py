"""Cost of the device-side distinct van Hove recorder (Context.vanhove_distinct_start) inside graph runs, per sample, at full-size C3 in
mixed precision: device events around the same run_graph call with nothing on, with an RDF recorder on the same sites (the unordered
classes (0,1), (0,0), (1,1)), and with the distinct van Hove recorder at 1, 8 and 32 live origins (num_lags = 1, 8, 32, every sample an
origin) in the four ordered classes (0,0), (0,1), (1,0), (1,1) -- the sites are one atom per molecule (its first), cation and anion
centres as two groups by the molecule's parity, as in tools/probes/rdf_cost.py; r_max 1.5 nm, 300 bins, a sample every 10 steps.  The
32-origin setting is also run with one histogram per wave ("vhd_hist_copies" = 4) and with plain global adds ("vhd_lds" = 0).  One
context; the settings take turns on it, in reversed order every other repeat, each warmed up untimed first so that its graphs are
captured and the ring is full outside the timed region.  Per setting: the median time, the cost per sample against `off`, the pairs per
sample and per second, and the ratio to the RDF sample of the same run.  From the shapes a sample does (live origins + 1) times the RDF's
pair work, doubled for the classes of one group with itself; this file is where the real ratio is found.  There is no pass mark.
usage: python tools/probes/vanhove_distinct_cost.py [repeats] [steps] [config]      (the output belongs in profiles/vanhove_distinct_cost.txt)"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

args = sys.argv[1:]
rep = int(args[0]) if len(args) > 0 else 3
steps = int(args[1]) if len(args) > 1 else 2000
cfg = args[2] if len(args) > 2 else "C3"
INTERVAL, R_MAX, NBINS = 10, 1.5, 300
RDF_CLASSES, VHD_CLASSES = [(0, 1), (0, 0), (1, 1)], [(0, 0), (0, 1), (1, 0), (1, 1)]
# (name, kind, live origins, {hook: value})
SETTINGS = [("off", None, 0, {}), ("rdf", "rdf", 0, {})] + [(f"vhd/{r}", "vhd", r, {}) for r in (1, 8, 32)] + \
           [("vhd/32/wave", "vhd", 32, {"vhd_hist_copies": 4}), ("vhd/32/plain", "vhd", 32, {"vhd_lds": 0})]
DEFAULTS = {"vhd_hist_copies": 1, "vhd_lds": 1}

pkg = importlib.import_module("openmm-velocityverlet_amd")
I, S, H = pkg.integrator, pkg.systems, pkg.vvhip
spec = S.make_config(cfg)
n = spec.num_atoms
mol = np.asarray(spec.mol_id)
first = np.nonzero(np.diff(np.concatenate(([-1], mol))) != 0)[0]      # the first particle of every molecule
ions = np.full(n, -1, dtype=np.int8)
ions[first] = mol[first] % 2
it = I.VVIntegrator(333.0, 10, 1.0, 40, 0.001)
it.setMaxDrudeDistance(0.02)
stream = torch.cuda.Stream()
ctx = I.Context(spec, it, precision="mixed", force_provider="tether", stream=stream.cuda_stream)
ctx.run_graph(1000, 50); ctx.synchronize()
print(f"{cfg}: {n} particles, {int(np.count_nonzero(ions == 0))} + {int(np.count_nonzero(ions == 1))} sites, r_max {R_MAX} nm, {NBINS} bins, a sample every "
      f"{INTERVAL} of {steps} steps per run, library {os.path.relpath(H.LIB_PATH, ROOT)}", flush=True)
times, info = {}, {}
for r in range(rep):
    for name, kind, origins, hooks in (SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
        ctx.rdf_stop(); ctx.vanhove_distinct_stop()
        warm = 500
        for key, value in {**DEFAULTS, **hooks}.items():
            H.check(H.lib.vvhip_debug_tune(ctx.plan, key.encode(), value), ctx.plan)
        if kind == "rdf":
            ctx.rdf_start(INTERVAL, R_MAX, NBINS, RDF_CLASSES, groups=ions)
        elif kind == "vhd":
            ctx.vanhove_distinct_start(INTERVAL, origins, R_MAX, NBINS, VHD_CLASSES, groups=ions)
            warm = max(500, (origins + 2) * INTERVAL)                # the ring full: every slot live in the timed region
        ctx.run_graph(warm, 50); ctx.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(stream)
        ctx.run_graph(steps, 50)
        end.record(stream)
        end.synchronize()
        ctx.synchronize()
        times.setdefault(name, []).append(begin.elapsed_time(end))
        if kind == "rdf":
            m = ctx.rdf_read()
            assert (m.samples, m.dropped, m.invalid) == ((warm + steps) // INTERVAL, 0, 0), (name, m.samples, m.dropped, m.invalid)
            info[name] = (int(m.pairs_per_sample.sum()), ctx.rdf_info().num_items)
        elif kind == "vhd":
            v = ctx.vanhove_distinct_read()
            assert (v.samples, v.dropped, v.invalid) == ((warm + steps) // INTERVAL, 0, 0), (name, v.samples, v.dropped, v.invalid)
            assert v.visits[origins] > 0
            lay = ctx.vanhove_distinct_info()
            info[name] = (int(v.pairs_per_sample.sum()) * (origins + 1), lay.num_items * (lay.num_origins + 1))
ctx.close()
base = np.median(times["off"])
rdf_per = 1e3 * (np.median(times["rdf"]) - base) / (steps // INTERVAL)
for name, kind, origins, hooks in SETTINGS:
    v = np.array(times[name])
    line = f"{cfg} {name:>14}: median {np.median(v):8.2f} ms for {steps} steps ({1e3 * steps / np.median(v):9.1f} steps/s; min {v.min():8.2f}, max {v.max():8.2f})"
    if kind:
        per = 1e3 * (np.median(v) - base) / (steps // INTERVAL)      # us per sample
        pairs, blocks = info[name]
        line += f"  {per:9.2f} us per sample, {pairs:.4g} pairs in {blocks} blocks"
        if per > 0:
            line += f" -> {pairs / per / 1e6:6.3f} x 10^12 pairs/s"
        if kind == "vhd" and rdf_per > 0:
            line += f"; {per / rdf_per:6.2f} x the RDF sample ({origins + 1} x the RDF's classes, the two of one group doubled: {pairs / info['rdf'][0]:.2f} x its pairs)"
    print(line + f"   [{', '.join(f'{x:.2f}' for x in v)}]", flush=True)
