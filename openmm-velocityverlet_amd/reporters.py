"""Reporters for OpenMM's ``app.Simulation`` on top of the integrator's device-side services.

``DrudeTemperatureReporter`` writes the file that examples/ommhelper/reporter/drudetemperaturereporter.py writes -- the same header,
the same tab-separated columns (step, T_COM, T_Atom, T_Drude, KE_COM, KE_Atom, KE_Drude) -- but takes the numbers from
``simulation.integrator.getDrudeTemperatures()`` (computed on the GPU, 56 bytes copied back) instead of downloading every velocity
and looping over molecules and pairs on the host.  It asks OpenMM for no state at all.
"""
from __future__ import annotations

HEADER = '#"Step"\t"T_COM"\t"T_Atom"\t"T_Drude"\t"KE_COM"\t"KE_Atom"\t"KE_Drude"'


def _plain(x, unit_name):
    """A float from a plain number or an openmm.unit Quantity (the SWIG method returns Quantities in kJ/mol and K)."""
    if hasattr(x, "value_in_unit"):
        from openmm import unit
        return float(x.value_in_unit(getattr(unit, unit_name)))
    return float(x)


class DrudeTemperatureReporter:
    """Reports the temperatures of the molecules' centres of mass, of the atoms inside them and of the Drude pairs' relative
    motion every `reportInterval` steps.

    Parameters
    ----------
    file : str
        The file to write to
    reportInterval : int
        The interval (in time steps) at which to write a line
    append : bool
        Whether to append to an existing file
    """

    def __init__(self, file, reportInterval, append=False):
        self._reportInterval = int(reportInterval)
        self._out = open(file, "a" if append else "w")
        self._hasInitialized = False

    def describeNextReport(self, simulation):
        """(steps until the next report, positions?, velocities?, forces?, energies?): nothing is needed from the State."""
        steps = self._reportInterval - simulation.currentStep % self._reportInterval
        return (steps, False, False, False, False)

    def report(self, simulation, state):
        ke_com, ke_atom, ke_drude, t_com, t_atom, t_drude = simulation.integrator.getDrudeTemperatures()
        if not self._hasInitialized:
            print(HEADER, file=self._out)
            self._hasInitialized = True
        ke = [_plain(x, "kilojoule_per_mole") for x in (ke_com, ke_atom, ke_drude)]
        t = [_plain(x, "kelvin") for x in (t_com, t_atom, t_drude)]
        print(simulation.currentStep, *t, *ke, sep="\t", file=self._out)
        self._out.flush()

    def close(self):
        if self._out is not None and not self._out.closed:
            self._out.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
