"""MI355X-native (HIP/gfx950) backend for the z-gong/openmm-velocityVerlet integrator hot path.

Import with ``importlib.import_module("openmm-velocityverlet_amd")`` (the directory name the build
contract fixes contains a hyphen).  ``systems`` is plain numpy; ``vvhip`` / ``integrator`` load
``lib/libvvhip.so`` (hand-written HIP behind the C ABI of include/vvhip.h) and fail loudly if it has
not been built -- there is no CPU or PyTorch fallback for the hot path.  ``reporters`` holds OpenMM reporters on top of the
integrator's device-side services (DrudeTemperatureReporter); ``barostat`` is the Monte Carlo barostat's host-side driver (plain numpy:
it talks to a context through four methods and loads no library).
"""
import importlib as _importlib

from . import systems  # noqa: F401

_LAZY = ("vvhip", "integrator", "distributed", "reporters", "barostat")


def __getattr__(name):
    if name in _LAZY:
        return _importlib.import_module(f"{__name__}.{name}")
    raise AttributeError(name)
