"""Cost of the device-side spatial distribution recorder (Context.sdf_start) inside graph runs, per sample, at full-size C3 in mixed
precision: device events around the same run_graph call with nothing on, with the recorder, and with an RDF recorder on the same sites
with r_max = sqrt(3) h, the sphere around the cube.  Frames: one per cation (the molecules of even parity, as in tools/probes/rdf_cost.py)
from its first three particles that have mass and are no Drude particle.  Two classes, each also run alone: the anion centres (the first
atom of every molecule of odd parity) and all atoms.  64 voxels per axis, h = 1 nm, a sample every 10 steps.  The RDF beside it takes
the frames' origins as group 0 against the anion centres, and against every other atom.  One context; the settings take turns on it, in
reversed order every other repeat, each warmed up untimed first so that its graphs are captured outside the timed region.  Per setting:
the median time, the cost per sample against `off`, the pairs per sample and per second, the in-range share of the pairs, and the ratio
to the RDF sample of the same sites in the same run.  There is no pass mark.
usage: python tools/probes/sdf_cost.py [repeats] [steps] [config]      (the output belongs in profiles/sdf_cost.txt)"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

args = sys.argv[1:]
rep = int(args[0]) if len(args) > 0 else 3
steps = int(args[1]) if len(args) > 1 else 2000
cfg = args[2] if len(args) > 2 else "C3"
INTERVAL, EXTENT, NBINS = 10, 1.0, 64
R_MAX = float(np.sqrt(3.0)) * EXTENT

pkg = importlib.import_module("openmm-velocityverlet_amd")
I, S, H = pkg.integrator, pkg.systems, pkg.vvhip
spec = S.make_config(cfg)
n = spec.num_atoms
mol = np.asarray(spec.mol_id)
first = np.nonzero(np.diff(np.concatenate(([-1], mol))) != 0)[0]      # the first particle of every molecule
body = np.asarray(spec.masses) > 0
body[np.asarray(spec.drude_pairs)[:, 0]] = False
frames = []
for at, m in zip(first, mol[first]):
    if m % 2 == 0:
        mem = at + np.nonzero(body[at:at + 64] & (mol[at:at + 64] == m))[0][:3]
        if len(mem) == 3:
            frames.append(mem)
frames = np.array(frames, dtype=np.int32)
anions = first[mol[first] % 2 == 1]
sites = np.full(n, -1, dtype=np.int8)          # sdf: site group 0 the anion centres ...
sites[anions] = 0
everything = np.zeros(n, dtype=np.int8)         # ... or every atom
rdf_ions = np.full(n, -1, dtype=np.int8)       # rdf: group 0 the frames' origins, group 1 the anion centres ...
rdf_ions[frames[:, 0]], rdf_ions[anions] = 0, 1
rdf_all = np.ones(n, dtype=np.int8)             # ... or every other atom
rdf_all[frames[:, 0]] = 0
# (name, kind, groups, the setting's RDF)
SETTINGS = [("off", None, None, None), ("rdf/ions", "rdf", rdf_ions, None), ("rdf/all", "rdf", rdf_all, None),
            ("sdf/ions", "sdf", sites, "rdf/ions"), ("sdf/all", "sdf", everything, "rdf/all")]

it = I.VVIntegrator(333.0, 10, 1.0, 40, 0.001)
it.setMaxDrudeDistance(0.02)
stream = torch.cuda.Stream()
ctx = I.Context(spec, it, precision="mixed", force_provider="tether", stream=stream.cuda_stream)
ctx.run_graph(1000, 50); ctx.synchronize()
print(f"{cfg}: {n} particles, box {np.asarray(spec.box).round(3).tolist()} nm, {len(frames)} frames, {len(anions)} anion centres, h {EXTENT} nm, {NBINS}^3 voxels, "
      f"rdf r_max {R_MAX:.4f} nm, a sample every {INTERVAL} of {steps} steps per run, library {os.path.relpath(H.LIB_PATH, ROOT)}", flush=True)
times, info = {}, {}
for r in range(rep):
    for name, kind, groups, _ in (SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
        ctx.rdf_stop(); ctx.sdf_stop()
        if kind == "rdf":
            ctx.rdf_start(INTERVAL, R_MAX, 300, [(0, 1)], groups=groups)
        elif kind == "sdf":
            ctx.sdf_start(INTERVAL, EXTENT, NBINS, frames, [(0, 0)], site_groups=groups)
        ctx.run_graph(500, 50); ctx.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(stream)
        ctx.run_graph(steps, 50)
        end.record(stream)
        end.synchronize()
        ctx.synchronize()
        times.setdefault(name, []).append(begin.elapsed_time(end))
        taken = (500 + steps) // INTERVAL
        if kind == "rdf":
            m = ctx.rdf_read()
            assert (m.samples, m.dropped, m.invalid) == (taken, 0, 0), (name, m.samples, m.dropped, m.invalid)
            info[name] = (int(m.pairs_per_sample.sum()), ctx.rdf_info().num_items, m.counts.sum() / taken)
        elif kind == "sdf":
            m = ctx.sdf_read()
            assert (m.samples, m.dropped, m.invalid, m.bad_frames) == (taken, 0, 0, 0), (name, m.samples, m.dropped, m.invalid, m.bad_frames)
            info[name] = (int(m.pairs_per_sample.sum()), ctx.sdf_info().num_items, m.counts.sum() / taken)
ctx.close()
base = np.median(times["off"])
per_sample = {name: 1e3 * (np.median(times[name]) - base) / (steps // INTERVAL) for name, kind, _, _ in SETTINGS if kind}      # us
for name, kind, _, beside in SETTINGS:
    v = np.array(times[name])
    line = f"{cfg} {name:>9}: median {np.median(v):8.2f} ms for {steps} steps ({1e3 * steps / np.median(v):9.1f} steps/s; min {v.min():8.2f}, max {v.max():8.2f})"
    if kind:
        per = per_sample[name]
        pairs, blocks, hits = info[name]
        line += f"  {per:9.2f} us per sample, {pairs:.4g} pairs in {blocks} blocks, {100.0 * hits / pairs:5.2f} % in range"
        if per > 0:
            line += f" -> {pairs / per / 1e6:6.3f} x 10^12 pairs/s"
        if beside and per_sample[beside] > 0:
            line += f"; {per / per_sample[beside]:6.2f} x the RDF sample of the same sites ({beside})"
    print(line + f"   [{', '.join(f'{x:.2f}' for x in v)}]", flush=True)
