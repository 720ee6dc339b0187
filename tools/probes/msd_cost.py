"""Cost of the device-side MSD recorder (Context.msd_start) inside graph runs, per sample: device events around run_graph calls of
`steps` steps (50-step graphs) with the recorder off and with it sampling every `interval` steps -- particle mode with 1, 8 and 32 live
origins (num_lags = origins, origin_every = 1), molecule mode with 8 -- each with and without the wave reduction of the four sums
(vvhip_debug_tune "msd_wave_reduce"), and with the accumulating kernel's block size forced ("msd_block_threads").  One context; the
settings alternate on it, in reversed order every other repeat, each warmed up untimed first so that its graphs are captured and the ring
is full outside the timed region.  Per setting: the median time, the cost per
sample against `off`, the bytes a sample must move -- (origins + 1) x 24 B x units for the ring plus the position loads -- and the
bandwidth that cost amounts to.
usage: python tools/probes/msd_cost.py [repeats] [steps] [interval] [config]"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

args = sys.argv[1:]
rep = int(args[0]) if len(args) > 0 else 5
steps = int(args[1]) if len(args) > 1 else 20000
interval = int(args[2]) if len(args) > 2 else 10
cfg = args[3] if len(args) > 3 else "C3"
WARM = 2000
# (name, origins, molecules, wave reduction)
SETTINGS = [("off", 0, False, 1)]
for reduce_ in (1, 0):
    SETTINGS += [(f"particles-{o}{'' if reduce_ else '/per-lane'}", o, False, reduce_) for o in (1, 8, 32)]
    SETTINGS += [(f"molecules-8{'' if reduce_ else '/per-lane'}", 8, True, reduce_)]
# the accumulating kernel's block size, where the default rule does not pick it: (name, origins, molecules, threads)
BLOCKS = [(f"molecules-8/block{t}", 8, True, t) for t in (64, 128, 512)] + [(f"particles-8/block{t}", 8, False, t) for t in (128, 256)]
SETTINGS += [(name, o, mol, 1, t) for name, o, mol, t in BLOCKS]
SETTINGS = [s if len(s) == 5 else s + (0,) for s in SETTINGS]

pkg = importlib.import_module("openmm-velocityverlet_amd")
I, S, H = pkg.integrator, pkg.systems, pkg.vvhip
spec = S.make_config(cfg)
it = I.VVIntegrator(333.0, 10, 1.0, 40, 0.001)
it.setMaxDrudeDistance(0.02)
stream = torch.cuda.Stream()
ctx = I.Context(spec, it, precision="mixed", force_provider="tether", stream=stream.cuda_stream)
ctx.run_graph(WARM, 50); ctx.synchronize()
times, units = {}, {}
for r in range(rep):
    for name, origins, molecules, reduce_, threads in (SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
        ctx.msd_stop()
        H.check(H.lib.vvhip_debug_tune(ctx.plan, b"msd_wave_reduce", reduce_), ctx.plan)
        H.check(H.lib.vvhip_debug_tune(ctx.plan, b"msd_block_threads", threads), ctx.plan)
        if origins:
            ctx.msd_start(interval, origins, 1, molecules=molecules, max_samples=1 << 20)
            units[name] = ctx.msd_info().num_units
        ctx.run_graph(WARM, 50); ctx.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(stream)
        ctx.run_graph(steps, 50)
        end.record(stream)
        end.synchronize()
        ctx.synchronize()
        times.setdefault(name, []).append(begin.elapsed_time(end))
        if origins:
            m = ctx.msd_read()
            assert (m.samples, m.dropped, m.out_of_range) == ((WARM + steps) // interval, 0, 0), (name, m.samples, m.dropped, m.out_of_range)
            assert m.pairs[0, 0] == (m.samples - 1) * units[name]
ctx.close()
base = np.median(times["off"])
samples = steps // interval
for name, origins, molecules, _, _ in SETTINGS:
    v = np.array(times[name])
    line = f"{cfg} msd {name:>22}: median {np.median(v):8.2f} ms for {steps} steps ({1e3 * steps / np.median(v):9.1f} steps/s; min {v.min():8.2f}, max {v.max():8.2f})"
    if origins:
        per = 1e3 * (np.median(v) - base) / samples                  # us per sample
        loads = 32 * spec.num_atoms if not molecules else 32 * int(np.count_nonzero(np.asarray(spec.masses) > 0))      # posq + correction, 16 B each
        moved = (origins + 1) * 24 * units[name] + loads
        line += f"  {per:7.2f} us per sample, {units[name]} units, {moved / 1e6:6.2f} MB to move -> {moved / per / 1e3:7.1f} GB/s"
    print(line + f"   [{', '.join(f'{x:.2f}' for x in v)}]", flush=True)
