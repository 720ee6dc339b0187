"""Cost of the device-side profile recorder (Context.profile_start) inside graph runs: steps/s of 20 000-step run_graph calls (50-step
graphs) with the recorder off; 512 bins x 2 groups x {count, charge} every 100 and every 10 steps; the same with all seven rows -- and of
the host alternative at the same steps: float32 frames recorded on the device, downloaded and binned in NumPy (count and charge).  With
--parent-lib another build of the library (the commit before the feature) runs with nothing on in the same rotation.  With --caps a,b,...
the seven-row recorder at every 10 steps also runs with the accumulating kernel's grid capped at each value (TUNING_LOG.md).  One process
per build and repeat, in rotation on one box; inside a process the settings alternate on ONE context, each warmed up untimed first so that
its graphs are captured outside the timed region.
usage: python tools/probes/profile_cost.py [repeats] [steps] [config] [--parent-lib PATH] [--caps 32,64,...]"""
import importlib, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np


def option(name):
    if name not in sys.argv:
        return None
    value = sys.argv[sys.argv.index(name) + 1]
    return value


parent_lib, caps_arg, label = option("--parent-lib"), option("--caps"), option("--child")
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in (parent_lib, caps_arg, label)]
rep = int(args[0]) if len(args) > 0 else 5
steps = int(args[1]) if len(args) > 1 else 20000
cfg = args[2] if len(args) > 2 else "C3"
caps = [int(c) for c in caps_arg.split(",")] if caps_arg else []
NBINS = 512
# (name, interval, all seven rows, on the host instead, grid cap or 0)
SETTINGS = [("off", 0, False, False, 0), ("2rows-100", 100, False, False, 0), ("2rows-10", 10, False, False, 0),
            ("7rows-100", 100, True, False, 0), ("7rows-10", 10, True, False, 0),
            ("host-100", 100, False, True, 0), ("host-10", 10, False, True, 0)] + [(f"7rows-10/cap{c}", 10, True, False, c) for c in caps]
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
    groups = np.ones(spec.num_atoms, dtype=np.int8)
    if len(spec.drude_pairs):
        groups[np.asarray(spec.drude_pairs)[:, 0]] = 0
    charges = np.asarray(spec.charges, dtype=np.float64)
    group_offset = NBINS * groups.astype(np.int64)
    default_cap = 256

    for name, interval, seven, host, cap in (settings[::-1] if reverse else settings):
        device = interval and not host
        if hasattr(ctx, "profile_stop") and "vvhip_profile_stop" in H.EXPORTS:
            ctx.profile_stop()
            ctx.frames_stop()
            H.check(H.lib.vvhip_debug_tune(ctx.plan, b"profile_grid_cap", cap or default_cap), ctx.plan)
        if device:
            ctx.profile_start(interval, NBINS, groups=groups, charge=True, mass=seven, momentum=seven, kinetic=seven, max_samples=4096)
        elif host:
            ctx.frames_start(interval, capacity=steps // interval + 8)
        ctx.run_graph(WARM, 50); ctx.synchronize()
        if device:
            ctx.profile_read(reset=True)
        elif host:
            ctx.frames_read(reset=True)
        t0 = time.perf_counter()
        ctx.run_graph(steps, 50)
        samples = ""
        if host:                                                    # download every frame, bin count and charge per group
            f = ctx.frames_read()
            table = np.zeros((2, 2, NBINS))
            inv_l = 1.0 / float(spec.box[2])
            for j in range(len(f)):
                t = f.positions[j][:, 2].astype(np.float64) * inv_l
                b = np.minimum(((t - np.floor(t)) * NBINS).astype(np.int64), NBINS - 1) + group_offset
                table[:, 0] += np.bincount(b, minlength=2 * NBINS).reshape(2, NBINS)
                table[:, 1] += np.bincount(b, weights=charges, minlength=2 * NBINS).reshape(2, NBINS)
            assert len(f) == steps // interval and table[:, 0].sum() == len(f) * spec.num_atoms
            samples = f" {len(f)}"
        ctx.synchronize()
        if device:
            p = ctx.profile_read()
            assert (p.samples, p.dropped, p.out_of_range) == (steps // interval, 0, 0), (name, p.samples, p.dropped, p.out_of_range)
            assert p.words[:, 0].sum() == p.samples * spec.num_atoms
            samples = f" {p.samples}"
        dt = time.perf_counter() - t0
        print(f"RATE {name} {steps / dt:.3f}{samples}", flush=True)
    ctx.close()


if label:
    measure([("parent", 0, False, False, 0)] if label == "parent" else SETTINGS, "--reverse" in sys.argv)
    sys.exit(0)

rates, samples = {}, {}
for r in range(rep):
    builds = ([("parent", parent_lib)] if parent_lib else []) + [("this", None)]
    for build, lib in (builds if r % 2 == 0 else builds[::-1]):
        env = dict(os.environ)
        if lib:
            env["VVHIP_LIB"] = os.path.abspath(lib)
        else:
            env.pop("VVHIP_LIB", None)
        cmd = [sys.executable, os.path.abspath(__file__), str(rep), str(steps), cfg, "--child", build] + (["--caps", caps_arg] if caps_arg else []) + (["--reverse"] if r % 2 else [])
        out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
        if out.returncode != 0:
            sys.exit(f"{build} child failed ({out.returncode}):\n{out.stdout[-2000:]}{out.stderr[-2000:]}")
        for line in out.stdout.splitlines():
            if line.startswith("RATE "):
                f = line.split()
                rates.setdefault(f[1], []).append(float(f[2]))
                if len(f) > 3:
                    samples[f[1]] = int(f[3])
base = np.median(rates["off"])
for name in (["parent"] if parent_lib else []) + [s[0] for s in SETTINGS]:
    v = np.array(rates[name])
    n = samples.get(name, 0)
    per = f"  {n:4d} samples, {1e6 * steps / n * (1 / np.median(v) - 1 / base):8.2f} us per sample" if n else ""
    print(f"{cfg} profile {name:>14}: median {np.median(v):9.1f} steps/s  (min {v.min():9.1f}, max {v.max():9.1f})  "
          f"{100 * (np.median(v) / base - 1):+6.2f} % against off{per}   [{', '.join(f'{x:.0f}' for x in v)}]", flush=True)
