// tests/cpp/report_driver.cpp -- test code.  The Drude temperature report through the C++ layers the way an OpenMM host reaches it:
//   VVIntegrator::getDrudeTemperatures() -> Platform "HIP" -> createKernel("CalcDrudeTemperatures") (lazily, on the first call) ->
//   HipCalcDrudeTemperaturesKernel -> vvhip_drude_temperatures.
//   vv_report_driver OUT nsteps   (GPU) a small Drude system (with a CMMotionRemover and a few HBond constraints), nsteps steps, then the
//                                 report; dumps the system and the velocities to OUT and prints the six numbers as hexadecimal doubles
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "HipVVKernelFactory.h"
#include "HipVVKernels.h"
#include "openmm/CMMotionRemover.h"
#include "openmm/Context.h"
#include "openmm/DrudeForce.h"
#include "openmm/VVIntegrator.h"

using namespace OpenMM;

static unsigned long long lcg_state = 2463534242ull;
static double uniform() { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; return (double) (lcg_state >> 11) / 9007199254740992.0; }
static double gauss() { double s = 0; for (int i = 0; i < 12; i++) s += uniform(); return s - 6.0; }

struct ForceUser { HipContext* cu; HipArray* site; };
static void tether(ContextImpl&, void* user) {
    ForceUser* u = (ForceUser*) user;
    std::shared_ptr<HipVVPlan> plan = HipVVPlan::find(*u->cu);
    plan->check(vvhip_synth_tether_force(plan->get(), u->site->getDevicePointer(), 1000.0, 209200.0));
}
template <class T> static void put(std::ofstream& f, const std::vector<T>& v) { long long n = (long long) v.size(); f.write((const char*) &n, 8); f.write((const char*) v.data(), n * sizeof(T)); }

static int run(const char* out, int nsteps) {
    registerHipVVKernelFactories();
    Platform& hip = Platform::getPlatformByName("HIP");
    const int nmol = 70, per = 8;              // [heavy, drude, heavy, drude, heavy, drude, H, H] per molecule
    const int n = nmol * per;
    System system;
    DrudeForce* drude = new DrudeForce();
    std::vector<double> masses, pos(3 * n), vel(3 * n);
    std::vector<int> molId, pairs, cons;
    std::vector<std::vector<int> > molecules(nmol);
    const double kB = (1.380649e-23 * 6.02214076e23) / 1000.0, box[3] = {3.0, 3.0, 3.0};
    for (int m = 0; m < nmol; m++) {
        double c[3] = {uniform() * box[0], uniform() * box[1], uniform() * box[2]};
        for (int k = 0; k < per; k++) {
            const int i = m * per + k;
            const bool isDrude = k < 6 && (k & 1);
            const double mass = k >= 6 ? 1.008 : (isDrude ? 0.4 : 11.611 + (k == 0 ? 1.996 : 0.0));
            system.addParticle(mass);
            masses.push_back(mass); molId.push_back(m);
            molecules[m].push_back(i);
            if (isDrude) { drude->addParticle(i, i - 1, -1, -1, -1, -2.0, 0.001, 1, 1); pairs.push_back(i); pairs.push_back(i - 1); }
            for (int d = 0; d < 3; d++) {
                pos[3 * i + d] = isDrude ? pos[3 * (i - 1) + d] + 2e-4 * gauss() : c[d] + 0.15 * (2 * uniform() - 1);
                vel[3 * i + d] = gauss() * std::sqrt(kB * (isDrude ? 30.0 : 333.0) / mass);
            }
        }
        if (m % 5 == 0) { system.addConstraint(m * per + 6, m * per + 4, 0.5); cons.push_back(m * per + 6); cons.push_back(m * per + 4); }   // (DOF count only)
    }
    system.addForce(drude);
    system.addForce(new CMMotionRemover());
    VVIntegrator it(333.0, 10.0, 1.0, 40.0, 0.001);
    it.setMaxDrudeDistance(0.02);
    Context ctx(system, it, hip);
    HipContext cu(n, false, true);             // HipPrecision = mixed
    cu.setPeriodicBoxSize(box[0], box[1], box[2]);
    std::vector<double> velm(4 * n);
    std::vector<float> posq(4 * n), corr(4 * n, 0.f);
    for (int i = 0; i < n; i++) {
        for (int d = 0; d < 3; d++) {
            velm[4 * i + d] = vel[3 * i + d];
            posq[4 * i + d] = (float) pos[3 * i + d];
            corr[4 * i + d] = (float) (pos[3 * i + d] - (double) posq[4 * i + d]);
        }
        velm[4 * i + 3] = 1.0 / masses[i];
        posq[4 * i + 3] = 0.0f;
    }
    cu.getVelm().upload(velm.data()); cu.getPosq().upload(posq.data()); cu.getPosqCorrection().upload(corr.data());
    HipArray site; site.initialize(n, 16); site.upload(posq.data());
    HipPlatform::PlatformData pd; pd.contexts.push_back(&cu);
    cu.setPlatformData(&pd);
    ctx.getImpl().setPlatformData(&pd);
    ctx.getImpl().setMolecules(molecules);
    ForceUser fu = {&cu, &site};
    ctx.getImpl().setForceCallback(tether, &fu);
    ctx.initialize();
    it.step(nsteps);
    const std::vector<double> r = it.getDrudeTemperatures();
    const std::vector<double> again = it.getDrudeTemperatures();      // (the kernel is created once; a second call gives the same bits)
    (void) hipDeviceSynchronize();
    cu.getVelm().download(velm.data());
    std::ofstream f(out, std::ios::binary);
    put(f, masses); put(f, molId); put(f, pairs); put(f, cons); put(f, velm);
    std::printf("REPORT");
    for (double x : r) std::printf(" %a", x);
    std::printf("\n%s\n", r == again ? "REPORT OK" : "REPORT CHANGED ON A SECOND CALL");
    return r == again ? 0 : 1;
}

int main(int argc, char** argv) {
    try {
        if (argc >= 3) return run(argv[1], std::atoi(argv[2]));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    std::fprintf(stderr, "usage: vv_report_driver OUT nsteps\n");
    return 64;
}
