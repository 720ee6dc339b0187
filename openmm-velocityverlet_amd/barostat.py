"""Monte Carlo barostat: the host half of an attempt.

What OpenMM's MonteCarloBarostat / MonteCarloAnisotropicBarostat do for a run inside OpenMM (examples/ommhelper/util.py:
apply_mc_barostat offers ``iso``, ``semi-iso``, ``xyz``, ``xy`` and ``z``; examples/run-bulk.py defaults to ``iso``), restated from
OpenMM's documented algorithm -- NOT pinned to OpenMM's random stream.  The decision is a few scalars per attempt; the device half
(every molecule moved rigidly with the box, the proposal undone bit for bit on a rejection) is ``Context.scale_box`` /
``Context.restore_box`` (include/vvhip.h: vvhip_barostat_*).

The driver talks to the context only through ``getPeriodicBoxSize()``, ``scale_box(scale)``, ``restore_box()`` and ``num_molecules``
(``run`` also uses ``run_graph``), so it runs against a NumPy stand-in on the CPU (tests/barostat_reference.py).  This module loads no
library.

One attempt, with V the volume, P the pressure, N the System's molecule count, g an axis group of the mode and scale_g its step [nm^3]:
    g uniformly among the groups, then u, then u2, from numpy.random.Generator(Philox(seed)) -- all three on every attempt, used or not
    dV = scale_g 2 (u - 1/2),  V' = V + dV;  rejected if V' <= 0
    s_a = (V'/V)^(1/|g|) on the group's axes, 1 elsewhere
    E0 = potential_energy();  context.scale_box(s);  E1 = potential_energy()
    w = E1 - E0 + P dV - N kT ln(V'/V)
    accepted iff w <= 0 or u2 < exp(-w / kT);  otherwise context.restore_box()
Adaptation, per group: scale_g starts at 0.01 V; after every 10 attempts of a group, fewer than 25 % accepted divides its scale by 1.1,
more than 75 % multiplies it by 1.1 (capped at 0.3 V), and the group's two counters start over.  adapt=False leaves the scale where
setVolumeScale put it (an adaptive step breaks detailed balance: a few per cent of bias in the mean volume of a very small system).
"""
import math

import numpy as np

BAR_TO_KJ_PER_MOL_NM3 = 0.0602214076          # 1 bar = 1e5 J/m^3 = 1e5 x 6.02214076e23 / 1e3 / 1e27 kJ/(mol nm^3)
GAS_CONSTANT = 8.31446261815324e-3            # kJ/(mol K)

# a mode is a list of axis groups that scale together
MODES = {
    "iso": ((0, 1, 2),),
    "semi-iso": ((0, 1), (2,)),
    "xyz": ((0,), (1,), (2,)),
    "xy": ((0,), (1,)),
    "z": ((2,),),
}


def group_scale(group, volume_ratio):
    """s[0..2] of a move of `group` that takes the volume from V to volume_ratio x V: the 1/|g| power on the group's axes, 1 elsewhere."""
    s = [1.0, 1.0, 1.0]
    f = volume_ratio ** (1.0 / len(group))
    for a in group:
        s[a] = f
    return s


class MonteCarloBarostat:
    def __init__(self, pressure_bar, temperature, mode="iso", frequency=100, seed=0, adapt=True):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}, not {mode!r}")
        if int(frequency) < 1:
            raise ValueError("frequency must be >= 1 step")
        self.pressure_bar, self.temperature = float(pressure_bar), float(temperature)
        self.pressure = self.pressure_bar * BAR_TO_KJ_PER_MOL_NM3          # kJ/(mol nm^3)
        self.kT = GAS_CONSTANT * self.temperature
        self.mode, self.groups = mode, MODES[mode]
        self.frequency, self.seed, self.adapt = int(frequency), int(seed), bool(adapt)
        self._rng = np.random.Generator(np.random.Philox(self.seed))
        n = len(self.groups)
        self.scales = [None] * n                 # nm^3; None: 0.01 V at the first attempt
        self.window_attempts = [0] * n           # since the group's last adaptation
        self.window_accepted = [0] * n
        self.attempts = 0
        self.accepted = 0
        self.last = None                         # (group, dV, w, accepted) of the last attempt

    # ---- the step of the volume moves
    def setVolumeScale(self, scale, group=None):
        """The step [nm^3] of one group, or of every group."""
        for g in (range(len(self.groups)) if group is None else [int(group)]):
            self.scales[g] = float(scale)

    def getVolumeScale(self, group=0):
        return self.scales[group]

    def _adapt(self, g, volume):
        if self.window_attempts[g] < 10:
            return
        if self.adapt:
            if self.window_accepted[g] < 0.25 * self.window_attempts[g]:
                self.scales[g] /= 1.1
            elif self.window_accepted[g] > 0.75 * self.window_attempts[g]:
                self.scales[g] = min(self.scales[g] * 1.1, 0.3 * volume)
        self.window_attempts[g] = 0
        self.window_accepted[g] = 0

    # ---- one attempt
    def attempt(self, context, potential_energy) -> bool:
        """One volume move on `context`; potential_energy() returns kJ/mol for the context's current positions and box.  True: accepted."""
        g = int(self._rng.integers(len(self.groups)))
        u = float(self._rng.random())
        u2 = float(self._rng.random())
        box = np.asarray(context.getPeriodicBoxSize(), dtype=np.float64)
        volume = float(box[0] * box[1] * box[2])
        for k in range(len(self.groups)):
            if self.scales[k] is None:
                self.scales[k] = 0.01 * volume
        d_volume = self.scales[g] * 2.0 * (u - 0.5)
        new_volume = volume + d_volume
        accepted, w = False, math.inf
        if new_volume > 0:
            ratio = new_volume / volume
            e0 = float(potential_energy())
            context.scale_box(group_scale(self.groups[g], ratio))
            e1 = float(potential_energy())
            w = e1 - e0 + self.pressure * d_volume - context.num_molecules * self.kT * math.log(ratio)
            accepted = w <= 0 or u2 < math.exp(-w / self.kT)
            if not accepted:
                context.restore_box()
        self.attempts += 1
        self.window_attempts[g] += 1
        if accepted:
            self.accepted += 1
            self.window_accepted[g] += 1
        self.last = (g, d_volume, w, accepted)
        box = np.asarray(context.getPeriodicBoxSize(), dtype=np.float64)
        self._adapt(g, float(box[0] * box[1] * box[2]))
        return accepted

    def run(self, context, steps, potential_energy, steps_per_graph=50):
        """`steps` steps through context.run_graph in chunks of `frequency`, one attempt after every full chunk.  Returns the attempts'
        outcomes."""
        out, left = [], int(steps)
        while left > 0:
            n = min(self.frequency, left)
            context.run_graph(n, steps_per_graph)
            left -= n
            if n == self.frequency:
                out.append(self.attempt(context, potential_energy))
        return out

    # ---- restart
    def getState(self) -> dict:
        """Everything a restarted run needs to continue the same sequence, JSON-able."""
        def plain(x):
            if isinstance(x, dict):
                return {k: plain(v) for k, v in x.items()}
            if isinstance(x, np.ndarray):
                return [int(v) for v in x]
            return int(x) if isinstance(x, (np.integer, int)) and not isinstance(x, bool) else x
        return {"mode": self.mode, "scales": list(self.scales), "window_attempts": list(self.window_attempts),
                "window_accepted": list(self.window_accepted), "attempts": self.attempts, "accepted": self.accepted,
                "rng": plain(self._rng.bit_generator.state)}

    def setState(self, state: dict):
        if state["mode"] != self.mode:
            raise ValueError(f"the state belongs to mode {state['mode']!r}, this barostat runs {self.mode!r}")
        self.scales = [None if s is None else float(s) for s in state["scales"]]
        self.window_attempts = [int(x) for x in state["window_attempts"]]
        self.window_accepted = [int(x) for x in state["window_accepted"]]
        self.attempts, self.accepted = int(state["attempts"]), int(state["accepted"])
        r = state["rng"]
        self._rng.bit_generator.state = {
            "bit_generator": r["bit_generator"],
            "state": {"counter": np.array(r["state"]["counter"], dtype=np.uint64), "key": np.array(r["state"]["key"], dtype=np.uint64)},
            "buffer": np.array(r["buffer"], dtype=np.uint64), "buffer_pos": int(r["buffer_pos"]),
            "has_uint32": int(r["has_uint32"]), "uinteger": int(r["uinteger"])}
