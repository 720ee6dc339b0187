"""Particle sharding over the GPUs of one node (one process per GPU).

Shards are contiguous particle ranges cut on molecule boundaries, so every Drude pair
and every COM group stays on one GPU.  The only cross-GPU exchange is an element-wise int64 sum of the
<= 3 fixed-point accumulators after each reduction phase (include/vvhip.h: vvhip_step_middle_phase),
issued through torch.distributed (backend "nccl" = RCCL over xGMI on GPUs, "gloo" in CPU tests).
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np


def shard_bounds(system, world_size: int) -> List[Tuple[int, int]]:
    """Cut [0, N) into `world_size` contiguous ranges of nearly equal size whose ends fall between molecules.

    Requires every molecule to occupy a contiguous index range (true for all shipped models); image-charge
    systems are single-GPU in the reference's configs (BASELINE.json C5) and are rejected by the plan."""
    mol = np.asarray(system.mol_id)
    n = mol.shape[0]
    if world_size == 1:
        return [(0, n)]
    change = np.nonzero(np.diff(mol) != 0)[0] + 1            # indices where a new molecule starts
    if len(np.unique(mol)) != len(change) + 1:
        raise ValueError("molecules are not contiguous in particle index: cannot shard by index range")
    starts = np.concatenate([[0], change, [n]])
    cuts = [0]
    for r in range(1, world_size):
        target = r * n / world_size
        k = int(np.argmin(np.abs(starts - target)))
        cuts.append(int(max(starts[k], cuts[-1])))
    cuts.append(n)
    return [(cuts[i], cuts[i + 1]) for i in range(world_size)]


def first_contact_report(local: dict, group=None):
    """What every rank of a multi-GPU run knows about its own set-up, gathered on all ranks and checked for agreement BEFORE the first
    timed region (round-4 review, "first real multi-GPU contact": the in-core RCCL all-reduce at world > 1 and the hipIpc mailbox
    ACROSS devices have never run in the build environment, so the first run that does must at least fail with a readable report).
    `local` = {"device": int, "device_name": str, "peer_access": [bool per rank's device] or None, "rccl_ranks": int, "exchange": chosen
    mechanism, "mailbox_trial": str or None, "world": int, ...}.  Returns (ok, text): ok = every rank chose the same exchange, no two ranks
    sit on one device (unless they say they share it on purpose), every communicator counts the whole world, every device reaches every
    other where the mailbox is used; text = one line per rank + the complaints.  Works on any backend (all_gather_object)."""
    import torch.distributed as dist
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    every = [None] * world
    if world > 1:
        dist.all_gather_object(every, local, group=group)
    else:
        every = [local]
    return check_first_contact(every)


def check_first_contact(every: List[dict]):
    """The agreement rules of first_contact_report on the gathered per-rank records (host-only: unit-tested without a process group)."""
    lines, complaints = [], []
    world = len(every)
    for r, rec in enumerate(every):
        pa = rec.get("peer_access")
        lines.append(f"rank {r}: device {rec.get('device')} ({rec.get('device_name', '?')}), exchange {rec.get('exchange')}, "
                     f"RCCL communicator ranks {rec.get('rccl_ranks')}, peer access {''.join('1' if x else '0' for x in pa) if pa is not None else 'not checked'}, "
                     f"mailbox trial: {rec.get('mailbox_trial')}")
    chosen = {rec.get("exchange") for rec in every}
    if len(chosen) != 1:
        complaints.append(f"the ranks chose different exchange mechanisms: {sorted(map(str, chosen))}")
    if any(rec.get("world") != world for rec in every):
        complaints.append(f"ranks disagree about the world size: {[rec.get('world') for rec in every]} (gathered {world} records)")
    # (a device is (host, local index): on several nodes the local indices repeat)
    devices = [(rec.get("host"), rec.get("device")) for rec in every]
    if len(set(devices)) != world and not all(rec.get("share_device") for rec in every):
        complaints.append(f"two ranks on one device without --share-device: devices {devices}")
    exch = next(iter(chosen)) if len(chosen) == 1 else None
    if exch in ("eager", "graph"):
        bad = [r for r, rec in enumerate(every) if rec.get("rccl_ranks") != world]
        if bad:
            complaints.append(f"RCCL communicator of rank(s) {bad} does not count {world} ranks")
    if exch == "mailbox" and world > 1 and not all(rec.get("share_device") for rec in every):
        if len({rec.get("host") for rec in every}) > 1:
            complaints.append("the mailbox maps the peers' boxes through hipIpc: ranks of ONE host only")
        bad = [r for r, rec in enumerate(every) if rec.get("peer_access") is not None and not all(rec["peer_access"])]
        if bad:
            complaints.append(f"hipDeviceCanAccessPeer denies a pair of devices on rank(s) {bad}: the mailbox stores into the peers' memory")
    text = "\n".join(lines + ["first contact: " + ("all ranks agree" if not complaints else "; ".join(complaints))])
    return not complaints, text


class _DevInt64:
    """Zero-copy view of `count` int64 values at a raw device pointer, via the CUDA array interface."""

    def __init__(self, ptr: int, count: int):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": "<i8", "data": (int(ptr), False), "version": 2}


class ShardedStepper:
    """Drives vvhip_step_middle_phase on this rank's shard and sums the fixed-point accumulators over ranks
    after every reduction phase.  With backend nccl (= RCCL) the all-reduce runs on the GPU over xGMI on the
    plan's stream; with gloo (CPU tests, or several ranks sharing one GPU) the 8..24 bytes are staged through
    the host.  int64 sums are associative, so every rank sees the same bits whatever the rank count."""

    def __init__(self, ctx, group=None):
        import ctypes as C
        import torch.distributed as dist
        from . import vvhip as H
        self.ctx, self.group, self.dist, self.H, self.C = ctx, group, dist, H, C
        self.backend = dist.get_backend(group) if dist.is_initialized() else None
        self.nphase = H.lib.vvhip_step_middle_phases(ctx.plan)
        self._tensors = {}

    def _acc(self, ph):
        """The accumulators alternate between two copies from step to step (thermostat double-buffering), so ask every time."""
        C, H = self.C, self.H
        p, n = C.c_void_p(), C.c_int32()
        H.check(H.lib.vvhip_accumulators(self.ctx.plan, ph, C.byref(p), C.byref(n)), self.ctx.plan)
        return p.value, n.value

    def _all_reduce(self, ph):
        import numpy as np
        import torch
        ptr, n = self._acc(ph)
        if self.backend == "nccl":
            if ptr not in self._tensors:
                self._tensors[ptr] = torch.as_tensor(_DevInt64(ptr, n), device="cuda")
            self.dist.all_reduce(self._tensors[ptr], op=self.dist.ReduceOp.SUM, group=self.group)
        else:
            H = self.H
            host = np.zeros(n, dtype=np.int64)
            H.check(H.lib.vvhip_synchronize(self.ctx.plan), self.ctx.plan)
            H.check(H.lib.vvhip_memcpy_d2h(host.ctypes.data, ptr, host.nbytes), what="d2h")
            t = torch.from_numpy(host)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)
            H.check(H.lib.vvhip_memcpy_h2d(ptr, host.ctypes.data, host.nbytes), what="h2d")

    def step(self, steps: int = 1):
        H, ctx = self.H, self.ctx
        for _ in range(steps):
            ctx.calcForces()
            for ph in range(self.nphase):
                H.check(H.lib.vvhip_step_middle_phase(ctx.plan, ph, 0), ctx.plan)
                if ph < self.nphase - 1 and self.backend is not None:
                    self._all_reduce(ph)


def drude_temperatures(ctx, group=None):
    """The Drude temperature report of a sharded run: every rank's raw fixed-point sums (vvhip_drude_report_raw: its own particles)
    summed over the process group, then turned into (KE_COM, KE_Atom, KE_Drude, T_COM, T_Atom, T_Drude) with the whole system's DOFs.
    int64 sums are associative: every rank gets the single-process result bit for bit.  Collective: every rank of the group calls it."""
    import torch
    import torch.distributed as dist
    raw = torch.from_numpy(ctx.drude_report_raw())
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        if dist.get_backend(group) == "nccl":
            dev = raw.to("cuda")
            dist.all_reduce(dev, op=dist.ReduceOp.SUM, group=group)
            raw = dev.cpu()
        else:
            dist.all_reduce(raw, op=dist.ReduceOp.SUM, group=group)
    return ctx.drude_report_combine(raw.numpy())


def profile_sum(profiles):
    """The profile of a sharded run from its shards' profiles (Context.profile_read of every shard, the same description and the same
    steps behind each): the tables added as int64 words -- integer sums are associative, so the result is the unsharded table bit for
    bit -- and out_of_range added; samples and dropped are the same on every shard."""
    import dataclasses
    from .integrator import profile_views
    first = profiles[0]
    for p in profiles[1:]:
        if (p.words.shape, p.row_of, p.frac_bits, p.axis, p.samples, p.dropped) != (first.words.shape, first.row_of, first.frac_bits, first.axis, first.samples, first.dropped) \
                or not np.array_equal(p.box, first.box):
            raise ValueError("the profiles differ in layout, fixed point, box or number of samples: not shards of one run")
    words = np.sum([p.words for p in profiles], axis=0, dtype=np.int64)
    return dataclasses.replace(first, words=words, out_of_range=sum(p.out_of_range for p in profiles), **profile_views(words, first.row_of, first.frac_bits))


def msd_sum(msds):
    """The MSD table of a sharded run from its shards' tables (Context.msd_read of every shard, the same description and the same steps
    behind each): the words added as int64 -- integer sums are associative, so the result is the unsharded table bit for bit -- and
    out_of_range added; samples, dropped and the origin floor are the same on every shard."""
    import dataclasses
    first = msds[0]
    key = lambda m: (m.words.shape, m.frac_bits, m.interval, m.origin_every, m.molecules, m.samples, m.dropped, m.origin_floor)
    for m in msds[1:]:
        if key(m) != key(first):
            raise ValueError("the MSD tables differ in layout, fixed point, schedule or number of samples: not shards of one run")
    return dataclasses.replace(first, words=np.sum([m.words for m in msds], axis=0, dtype=np.int64), out_of_range=sum(m.out_of_range for m in msds))


def acf_sum(acfs):
    """The autocorrelation table of a sharded run from its shards' tables (Context.acf_read of every shard, the same description and the
    same steps behind each): the words added as int64 -- the result is the unsharded table bit for bit -- and out_of_range added; samples,
    dropped and the origin floor are the same on every shard."""
    import dataclasses
    first = acfs[0]
    key = lambda m: (m.words.shape, m.frac_bits, m.interval, m.origin_every, m.mode, m.samples, m.dropped, m.origin_floor)
    for m in acfs[1:]:
        if key(m) != key(first):
            raise ValueError("the autocorrelation tables differ in layout, fixed point, schedule or number of samples: not shards of one run")
    return dataclasses.replace(first, words=np.sum([m.words for m in acfs], axis=0, dtype=np.int64), out_of_range=sum(m.out_of_range for m in acfs))


def vanhove_sum(tables):
    """The self van Hove table of a sharded run from its shards' tables (Context.vanhove_read of every shard, the same description and the
    same steps behind each): head and hist added as int64 -- the result is the unsharded table bit for bit -- and out_of_range added;
    samples, dropped and the origin floor are the same on every shard."""
    import dataclasses
    first = tables[0]
    key = lambda m: (m.head.shape, m.hist.shape, m.edges.tobytes(), m.frac2_bits, m.r4_hi_bits, m.r4_lo_bits, m.interval, m.origin_every,
                     m.molecules, m.samples, m.dropped, m.origin_floor)
    for m in tables[1:]:
        if key(m) != key(first):
            raise ValueError("the self van Hove tables differ in layout, bins, fixed point, schedule or number of samples: not shards of one run")
    return dataclasses.replace(first, head=np.sum([m.head for m in tables], axis=0, dtype=np.int64),
                               hist=np.sum([m.hist for m in tables], axis=0, dtype=np.int64), out_of_range=sum(m.out_of_range for m in tables))


def drude_temperature_series(ctx, group=None, reset=False):
    """A sharded run's series (Context.series_read): every rank's raw rows -- six fixed-point sums and the overflow flag per row, of its
    own particles -- summed over the process group in one all-reduce, then turned into KE / T with the whole system's DOFs.  Every rank
    gets the single-process series bit for bit; the thermostat part is the same on every rank already (it comes from exchanged sums).
    Collective: every rank of the group calls it, with the same series configuration and the same steps behind it."""
    import torch
    import torch.distributed as dist

    def combine(words):
        t = torch.from_numpy(np.ascontiguousarray(words, dtype=np.int64))
        if dist.is_initialized() and dist.get_world_size(group) > 1:
            if dist.get_backend(group) == "nccl":
                dev = t.to("cuda")
                dist.all_reduce(dev, op=dist.ReduceOp.SUM, group=group)
                t = dev.cpu()
            else:
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        return t.numpy()
    return ctx.series_read(reset=reset, combine=combine)
