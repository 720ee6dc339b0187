"""Worker for tests/test_gpu_series.py (launched by torch.distributed.run, backend gloo): two ranks share GPU 0, each integrates its
molecule-aligned shard with ShardedStepper and records a series.  The series summed over the ranks (distributed.drude_temperature_series)
must equal the per-call report of the same sharded run at the same steps (distributed.drude_temperatures) bit for bit, every rank must hold
the same thermostat rows, and the result must agree with the single-process series."""
import importlib
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("openmm-velocityverlet_amd")
S, I, D = pkg.systems, pkg.integrator, pkg.distributed

INTERVAL, ROWS = 5, 6


def main():
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    spec = S.make_config("C3", scale=0.25)
    for precision in ("mixed", "single"):
        def make(shard):
            it = I.VVIntegrator(333.0, 10.0, 1.0, 40.0, 0.001)
            it.setMaxDrudeDistance(0.02)
            return it, I.Context(spec, it, precision=precision, force_provider="tether", shard=shard, device=0)
        it, ctx = make(D.shard_bounds(spec, world)[rank])
        ctx.series_start(INTERVAL, capacity=64)
        st = D.ShardedStepper(ctx)
        per_call = []
        for _ in range(ROWS):
            st.step(INTERVAL)
            per_call.append(D.drude_temperatures(ctx))
        got = D.drude_temperature_series(ctx)
        ctx.close()
        assert list(got.step) == [INTERVAL * (j + 1) for j in range(ROWS)] and got.dropped == 0 and got.ok.all(), got.step
        want = np.array(per_call)
        assert np.array_equal(got.ke, want[:, :3]) and np.array_equal(got.t, want[:, 3:]), (rank, precision, got.ke, want)
        mine = np.concatenate([got.ke2, got.vscale, got.eta.reshape(ROWS, -1), got.v_bias[:, None]], axis=1)
        every = [None] * world
        dist.all_gather_object(every, mine)
        assert all(np.array_equal(e, every[0]) for e in every), "the thermostat rows differ between the ranks"
        it1, single = make(None)
        single.series_start(INTERVAL, capacity=64)
        it1.step(INTERVAL * ROWS)
        one = single.series_read()
        single.close()
        assert list(one.step) == list(got.step)
        # (the sharded trajectory itself only agrees with the single-process one to rounding, tests/dist_worker.py: ~1e-11 in mixed
        # precision; in single precision the cold Drude group's few-mK temperature drifts apart faster)
        rtol = 1e-9 if precision == "mixed" else 1e-3
        assert np.allclose(got.ke, one.ke, rtol=rtol, atol=0) and np.allclose(got.t, one.t, rtol=rtol, atol=0), (got.t, one.t)
        assert np.allclose(got.ke2, one.ke2, rtol=rtol, atol=0)
        if rank == 0:
            print(f"{precision}: sharded series == sharded per-call reports, thermostat rows equal on all ranks", flush=True)
    dist.barrier()
    if rank == 0:
        print("SERIES DIST OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
