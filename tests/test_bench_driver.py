"""bench.py under the driver's own command line (`--gpus 1 --steps 20 --warmup 5`): the short timed region must report the
same steps/s as a long run (round-1 verdict: a capture inside the timed region made the driver's number 3x lower than the
20 000-step figure), and the line must say what was actually launched."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*flags):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_driver_flags_give_the_long_run_figure():
    short = _bench("--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--no-cpu-baseline", "--large-n", "none")
    long_ = _bench("--gpus", "1", "--steps", "20000", "--warmup", "2000", "--full", "--no-cpu-baseline", "--large-n", "none")
    assert short["steps"] == 20 and short["warmup"] == 5 and long_["steps"] == 20000
    # what ran: one replay of a 20-step graph per timed region, captured before it
    assert "1 replay(s) of a 20-step hipGraph" in short["config"]["launch"], short["config"]["launch"]
    assert "200 replay(s) of a 100-step hipGraph" in long_["config"]["launch"], long_["config"]["launch"]
    assert short["config"]["timed_repeats"] >= 5
    # (a timed region carries 22-30 us of its own -- one graph launch + one synchronisation, by the box's host -- whatever K is: of a 200 us region
    # that is 0.83-0.90 of the long-run figure now that a step takes 10 us; the round-1 failure this test guards against was a factor of 3)
    ratio = short["value"] / long_["value"]
    assert 0.75 <= ratio <= 1.15, (short["value"], long_["value"])
    # ms_per_step is the timed region divided by K
    assert abs(short["ms_per_step"] * short["value"] * 1e-3 - 1.0) < 1e-3
    for line in (short, long_):
        r = line["roofline"]
        assert {"bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "avg_launch_us", "avg_launch_us_dispatch_timestamps",
                "avg_launch_us_back_to_back", "launch_timing"} <= set(r)
        # frac = algorithmic bytes of the dominant kernel / its launch duration / peak, by the clock launch_timing names
        k = "A" if r["kernel"] == "vv_kernel_a" else "B"      # (the one-launch step is an instance of kernel B)
        assert abs(r["algorithmic_bytes_per_launch"] / (r["avg_launch_us"][k] * 1e-6) / 1e9 / r["peak"] - r["frac"]) < 2e-3
        assert r["traffic"] is None or (r["traffic_source"] and r["traffic_source"]["file"].startswith("profiles/"))
        assert 0 < line["step"]["frac"] < r["frac"] < 1
        wc = line["config"]["with_constraints"]
        assert wc["roofline"]["kernel"].startswith("vv_kernel_") and 0 < wc["step"]["frac"] < 1
        # round 5: what the step's launches were, and every other BASELINE configuration under the driver's flags
        sl = line["config"]["step_launches"]
        assert sl["integrator_launches_per_step"] == r["launches_per_step"] and sl["integrator_launches_per_step"] in (1, 2)
        assert sl["rtc"]["failed"] == 0 and sl["generic_kernel_launches"] == {"A": 0, "B": 0}
        oc = line["config"]["other_configs"]
        for name in ("C4", "C5", "C2", "C1"):
            assert isinstance(oc[name], dict), oc[name]
            assert oc[name]["steps_per_s_driver_flags"] > 1000 and oc[name]["steps_per_s"] > 1000 and 0 < oc[name]["roofline"]["frac"] < 1
            assert oc[name]["generic_kernel_launches"] == 0
        cl = oc["C3_classic_scheme"]          # the classic scheme of the headline box: one launch per thermostat application
        assert isinstance(cl, dict) and cl["steps_per_s_driver_flags"] > 1000 and cl["integrator_launches_per_step"] == 2 and cl["generic_kernel_launches"] == 0
    # round 6 (the review's item 1): roofline.frac is the ROCPROFV3 fraction -- the live child run's average duration of the kernel when there is
    # one, else the committed summary's -- for the one-launch kernel too; the self-clocked replay of the integrator alone is a named side field
    for line in (short, long_):
        r = line["roofline"]
        k = "A" if r["kernel"] == "vv_kernel_a" else "B"
        assert r["clock"] in ("rocprofv3_child", "rocprofv3_committed_csv", "self_clocked"), r["clock"]
        if r["clock"] == "rocprofv3_child":
            child = r["avg_launch_us_rocprofv3_child"][k]
            assert abs(r["frac"] - r["algorithmic_bytes_per_launch"] / (child * 1e-6) / 8e12) < 2e-4, (r["frac"], child)
            assert r["frac"] == r["frac_rocprofv3_child"] and r["launch_timing"].startswith("avg_launch_us / achieved / frac: rocprofv3 --kernel-trace --stats of a child run")
        elif r["clock"] == "rocprofv3_committed_csv":
            csv_us = r["rocprofv3_cross_check"]["avg_launch_us"][k]
            assert abs(r["frac"] - r["algorithmic_bytes_per_launch"] / (csv_us * 1e-6) / 8e12) < 2e-4
            assert r["rocprofv3_cross_check"]["file"].startswith("profiles/")
        if r["launches_per_step"] == 1:
            # the replay is a modified workload (no provider kernel, zero forces, wall out of reach): comparison only, and says so
            assert 0 < r["frac_integrator_alone_replay"] < 1 and "MODIFIED workload" in r["integrator_alone_replay_caveat"]
            assert r["avg_launch_us_integrator_alone_replay"] == r["avg_launch_us_dispatch_timestamps"]["B"]
    import shutil
    if shutil.which("rocprofv3"):
        r = short["roofline"]
        assert r["clock"] == "rocprofv3_child", (r["clock"], r["launch_timing"])
        if r["launches_per_step"] == 1:
            # (the profiler's per-dispatch handling disturbs the kernel's in-kernel rendezvous: the child may only be SLOWER than the replay, within reason)
            assert 0.9 < r["avg_launch_us"]["B"] / r["avg_launch_us_integrator_alone_replay"] < 1.45
        else:
            assert abs(r["avg_launch_us"]["B"] / r["avg_launch_us_dispatch_timestamps"]["B"] - 1) < 0.15


def test_the_expected_scaling_curve_is_the_one_design_md_states():
    """bench.py at N > 1 prints measured / predicted (config.exchange.predicted); the prediction is DESIGN.md section 6's table."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for series, n, text in (("C3", 8, "103.7 k"), ("C3", 2, "93.6"), ("C4", 8, "85.6 k"), ("C4", 4, "83.3")):
        assert abs(bench.predicted_rate(series, n, "mailbox") / 1e3 - float(text.split()[0])) < 0.06 and text in design
    assert bench.predicted_rate("C3", 1, None) > bench.predicted_rate("C3", 8, "mailbox") > bench.predicted_rate("C3", 2, "mailbox")      # flat, not rising
    assert bench.predicted_rate("C3", 8, "eager") < 40e3 and bench.predicted_rate("C3x80", 8, "mailbox") > 7 * bench.predicted_rate("C3x80", 1, None)
    assert bench.predicted_rate("C2", 8, "mailbox") is None


class _FakeCtx:
    precision = "mixed"

    def algorithmic_bytes(self):
        return (0, 158)


def test_roofline_clock_is_the_profilers():
    """No GPU needed: bench.roofline_block takes frac from the live rocprofv3 child, else from the committed csv, else (and only then) from
    its own clock; the one-launch step's replay figure never is `frac` when a profiler figure exists."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = 111000
    times = {"A": None, "B": 7.0e-3, "A_back_to_back": None, "B_back_to_back": None, "one_launch": True, "how": "replay"}
    live = {"vv_kernel_b<float, double, 68113u, 1056u>": {"calls": 4000, "avg_ns": 8000.0}, "vv_kernel_b<float, double, 1u, 2u>": {"calls": 3, "avg_ns": 1.0},
            "vv_kernel_tether<float, double>": {"calls": 4000, "avg_ns": 5000.0}}
    r = bench.roofline_block(_FakeCtx(), n, times, live=live)
    assert r["clock"] == "rocprofv3_child" and r["avg_launch_us"]["B"] == 8.0
    assert abs(r["frac"] - 158 * n / 8.0e-6 / 8e12) < 1e-4 and r["frac"] == r["frac_rocprofv3_child"]
    assert abs(r["frac_integrator_alone_replay"] - 158 * n / 7.0e-6 / 8e12) < 1e-4 and r["frac_integrator_alone_replay"] > r["frac"]
    # no child: the committed summary of the same workload
    r = bench.roofline_block(_FakeCtx(), n, times, live="rocprofv3 not on PATH", ref_key="C3")
    ref = json.load(open(os.path.join(ROOT, "profiles", "kernel_stats_latest.json")))["C3"]
    us = max((v for k_, v in ref["kernels"].items() if k_.startswith("vv_kernel_b<")), key=lambda v: v["calls"])["avg_ns"] * 1e-3
    assert r["clock"] == "rocprofv3_committed_csv" and abs(r["avg_launch_us"]["B"] - us) < 1e-3
    assert abs(r["frac"] - 158 * n / (us * 1e-6) / 8e12) < 1e-4
    # neither: self-clocked, and the line says so
    r = bench.roofline_block(_FakeCtx(), n, times, live="rocprofv3 not on PATH", ref_key="no such workload")
    assert r["clock"] == "self_clocked" and r["avg_launch_us"]["B"] == 7.0 and "self-clocked" in r["launch_timing"]


@pytest.mark.gpu
def test_cpu_baseline_says_whether_openmm_was_there():
    line = _bench("--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--large-n", "none", "--no-rocprof", "--cpu-seconds", "2")
    cb = line["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0
    assert isinstance(cb["openmm"], dict) or cb["openmm"].startswith(("not installed", "installed, but"))


@pytest.mark.gpu
def test_odd_step_counts_and_tails():
    """K = 21 after W = 5: one replay of a 20-step graph + one host-launched step; the thermostat parity flips between the
    timed regions, so both per-parity executables get used."""
    line = _bench("--gpus", "1", "--steps", "21", "--warmup", "5", "--no-cpu-baseline", "--large-n", "none")
    assert "1 replay(s) of a 20-step hipGraph" in line["config"]["launch"] and "+ 1 host-launched" in line["config"]["launch"]
    assert line["value"] > 1000


def test_plain_command_with_several_gpus_starts_its_own_ranks():
    """`python3 bench.py --gpus 2 ...` WITHOUT a launcher (how the driver's 1-GPU command looks, extended to N): bench.py must start
    torch.distributed.run itself as a child process.  No GPU here: every rank stops at "needs a GPU" -- which proves that two ranks with
    RANK / WORLD_SIZE set were started (under the old code the parent itself exited with a usage error) and that the exit code comes back."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["HIP_VISIBLE_DEVICES"] = ""          # also on a GPU box: this test is about the launcher only
    env["CUDA_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
                        "--backend", "gloo", "--share-device"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode != 0
    assert "launch with torch.distributed.run" not in r.stderr, r.stderr[-2000:]
    assert "starting -m torch.distributed.run --nnodes=1 --nproc-per-node=2" in r.stderr, r.stderr[-2000:]
    assert r.stderr.count("bench.py needs a GPU") >= 1, r.stderr[-3000:]


@pytest.mark.gpu
def test_plain_command_two_ranks_one_gpu():
    """The scaling tier's command as the driver would type it by hand -- no launcher -- with two ranks sharing this box's one GPU:
    rc 0, one JSON line, n_gpus == 2, both ranks in the process group."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-device", "--steps", "20", "--warmup", "5",
                        "--no-cpu-baseline", "--large-n", "none"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 20 and line["value"] > 10
    assert line["config"]["exchange"]["process_group_ranks"] == 2
    one = _bench("--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--large-n", "none", "--no-rocprof")
    assert one["n_gpus"] == 1 and "exchange" not in one["config"]


@pytest.mark.gpu
def test_plain_run_times_k_steps_once_and_dumps_the_last_step(tmp_path):
    """A plain run (no --full): EXACTLY K timed steps in one region, the headline fields and none of the secondary blocks.  --dump-outputs
    writes the state the K steps ended on as float64 .npy files: the same bits in two runs with the same arguments, and what the oracle
    computes for the same W + K steps (1e-5 relative, as smoke())."""
    import importlib
    import numpy as np
    from oracle import oracle as O
    lines, dumps = [], []
    for i in range(2):
        d = tmp_path / f"run{i}"
        lines.append(_bench("--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", str(d)))
        dumps.append({f.stem: np.load(f) for f in sorted(d.glob("*.npy"))})
    for line in lines:
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(line)
        assert line["steps"] == 20 and line["warmup"] == 5 and line["config"]["timed_repeats"] == 1
        assert abs(line["ms_per_step"] * line["value"] * 1e-3 - 1.0) < 1e-3
        assert "roofline" not in line and "cpu_baseline" not in line and "other_configs" not in line["config"]
    a, b = dumps
    assert {"positions", "velocities", "thermostat_eta", "thermostat_eta_dot", "thermostat_ke2"} <= set(a) and set(a) == set(b)
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k]), k
    pkg = importlib.import_module("openmm-velocityverlet_amd")
    spec = pkg.systems.make_config("C3")
    assert a["positions"].shape == a["velocities"].shape == (spec.num_atoms, 3)
    osys = O.OracleSystem(spec, O.Params(temperature=333.0, drude_temperature=1.0, step_size=0.001, max_drude_distance=0.02), "mixed", force_mode=1)
    osys.step(25)
    x_o, v_o = osys.positions(), osys.velm[:, :3].astype(np.float64)
    massive = osys.velm[:, 3] != 0
    assert np.abs(a["positions"] - x_o).max() / np.abs(x_o).max() < 1e-5
    assert np.abs(a["velocities"][massive] - v_o[massive]).max() / np.abs(v_o[massive]).max() < 1e-5


def test_dump_outputs_samples_large_boxes(tmp_path, monkeypatch):
    """No GPU needed: above DUMP_MAX_ROWS particles bench.dump_outputs writes a fixed, seeded sample (the same rows every time, their indices
    beside them), every file float64, the whole dump within 64 MB at the cap."""
    import importlib.util
    import types
    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_mod3", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.DUMP_MAX_ROWS * (3 + 3 + 1) * 8 < 64e6
    nh = types.SimpleNamespace(eta=[[0.1] * 4] * 3, eta_dot=[[0.2] * 5] * 3, eta_dotdot=[[0.3] * 4] * 3, ke2=[1.0, 2.0, 3.0], vscale=[1.0] * 3)
    n = 1000
    pos = np.arange(3 * n, dtype=np.float64).reshape(n, 3)
    vel = -pos
    bench.dump_outputs(str(tmp_path / "all"), pos, vel, nh)
    assert np.array_equal(np.load(tmp_path / "all" / "positions.npy"), pos) and not (tmp_path / "all" / "sample_index.npy").exists()
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 100)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), pos, vel, nh)
    got = {f.name: np.load(f) for f in (tmp_path / "s1").glob("*.npy")}
    assert all(v.dtype == np.float64 for v in got.values())
    idx = got["sample_index.npy"].astype(np.int64)
    assert len(idx) == 100 and len(set(idx)) == 100 and np.array_equal(np.sort(idx), idx)
    assert np.array_equal(got["positions.npy"], pos[idx]) and np.array_equal(got["velocities.npy"], vel[idx])
    assert np.array_equal(np.load(tmp_path / "s2" / "sample_index.npy"), got["sample_index.npy"])
    assert got["thermostat_eta_dot.npy"].shape == (3, 5) and np.array_equal(got["thermostat_ke2.npy"], [1.0, 2.0, 3.0])
