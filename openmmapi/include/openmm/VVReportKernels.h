// openmm/VVReportKernels.h -- kernels of reports on the integrator's state, NOT part of the reference's interface (its VVKernels.h has no
// such class; FusedVVStepKernel.h is the precedent).  VVIntegrator creates them lazily, on the first call that needs one: they are not in
// initialize() nor in getKernelNames(), so a context that never reports creates exactly the reference's seven kernels.  Kept in a header
// of its own so that the HIP plugin also builds against the REFERENCE's openmmapi headers unchanged.
#ifndef OPENMM_VVREPORTKERNELS_H_
#define OPENMM_VVREPORTKERNELS_H_
#include <string>

#include "openmm/KernelImpl.h"
#include "openmm/Platform.h"
#include "openmm/System.h"

namespace OpenMM {
class ContextImpl;
class VVIntegrator;

// Temperatures of the molecules' centres of mass, of the atoms inside them and of the Drude pairs' relative motion in the current
// velocities, over all particles (examples/ommhelper/reporter/drudetemperaturereporter.py of the reference defines them).
class CalcDrudeTemperaturesKernel : public KernelImpl {
public:
    static std::string Name() { return "CalcDrudeTemperatures"; }
    CalcDrudeTemperaturesKernel(std::string name, const Platform& platform) : KernelImpl(name, platform) {}
    virtual void initialize(const System& system, const VVIntegrator& integrator) = 0;
    // ke = KE_COM, KE_Atom, KE_Drude [kJ/mol]; t = T_COM, T_Atom, T_Drude [K] (0 where a group has no degrees of freedom)
    virtual void calcDrudeTemperatures(ContextImpl& context, const VVIntegrator& integrator, double ke[3], double t[3]) = 0;
};

}  // namespace OpenMM
#endif
