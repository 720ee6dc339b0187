/*
 * vvhip.h -- C ABI of libvvhip.so: the MI355X-native (HIP, gfx950) implementation of the per-step
 * hot path of z-gong/openmm-velocityVerlet.
 *
 * Boundary.  In the reference the hot path sits behind seven OpenMM KernelImpl interfaces
 * (openmmapi/include/openmm/VVKernels.h:48-270) that a platform plugin implements in C++
 * (platforms/cuda/include/CudaVVKernels.h, platforms/cuda/src/CudaVVKernels.cpp).  This header is
 * the same surface flattened to C: one entry point per KernelImpl virtual (split where the
 * reference method calls OpenMM's constraint solvers in the middle), raw device pointers instead
 * of CudaArray, plain scalars instead of VVIntegrator getters.  The OpenMM-facing C++ adapters that
 * call it (HipVVKernelFactory, Hip*Kernel) live in platforms/hip/ and are described in
 * INTEGRATION.md.  Citations below are reference file:line under /root/reference; "HOST" is
 * platforms/cuda/src/CudaVVKernels.cpp, "API" is openmmapi/src/VVIntegrator.cpp.
 *
 * Conventions.  Every function returns VVHIP_OK (0) or a negative error code; the text of the last
 * error of a plan is available from vvhip_last_error().  Errors that the reference raises as
 * OpenMMException keep the reference's message text.  Nothing here falls back to a CPU path.
 * All launches go to the hipStream_t given in vvhip_buffers.stream and never synchronise with the
 * host unless the function's comment says so.  A plan is not re-entrant (as the reference: one
 * integrator <-> one context, API:93-94).
 */
#ifndef VVHIP_H
#define VVHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VVHIP_VERSION 1
#define VVHIP_MAX_CHAINS 8
#define VVHIP_NUM_TG 3            /* TG_ATOM, TG_COM, TG_DRUDE (HOST:49) */

enum {
    VVHIP_OK = 0,
    VVHIP_ERR_INVALID = -1,       /* bad argument / API misuse */
    VVHIP_ERR_TOPOLOGY = -2,      /* the reference's OpenMMException cases (API:149,155; HOST:519,537,787,801) */
    VVHIP_ERR_UNSUPPORTED = -3,   /* valid for the reference, not implemented here (message says what) */
    VVHIP_ERR_HIP = -4,           /* a HIP runtime call failed */
    VVHIP_ERR_NO_DEVICE = -5,     /* no usable GPU: the product has no CPU path */
    VVHIP_ERR_EXCHANGE = -6,      /* multi-GPU: a mailbox wait on the peers timed out; the ranks have diverged, the run is void (sticky) */
    VVHIP_ERR_OVERFLOW = -7,      /* a fixed-point accumulator left its range (2KE > 1024 x the thermostat target); sticky */
    VVHIP_ERR_RENDEZVOUS = -8,    /* one-launch step: the blocks did not meet in the in-kernel rendezvous (not resident together); run void; sticky */
    VVHIP_ERR_CONSTRAINT = -9     /* in-kernel constraints: a cluster hit its iteration cap without converging; sticky */
};

/* OpenMM's CudaPrecision / HipPrecision property (examples/run-bulk.py:78) */
enum { VVHIP_SINGLE = 0, VVHIP_MIXED = 1, VVHIP_DOUBLE = 2 };

typedef struct vvhip_plan vvhip_plan;

/* What the reference's initialize() methods read from OpenMM::System, DrudeForce and VVIntegrator
 * (API:92-188, HOST:56-117, 462-667, 761-824, 878-902, 940-969, 998-1035). Host pointers, copied. */
typedef struct {
    int32_t num_atoms;
    int32_t padded_num_atoms;          /* cu.getPaddedNumAtoms(): stride of the planar force buffer */
    const double* masses;              /* System::getParticleMass            [num_atoms]            */
    const int32_t* mol_id;             /* ContextImpl::getMolecules() as particle -> molecule id    */
    int32_t num_molecules;
    int32_t num_drude_pairs;
    const int32_t* drude_pairs;        /* (drude, parent) = DrudeForce p, p1 (HOST:68-73)   [2*n]   */
    int32_t num_constraints;
    const int32_t* constraints;        /* System::getConstraintParameters, DOF accounting   [2*n]   */
    int32_t has_cm_motion_remover;     /* HOST:550-558                                              */
    int32_t num_particles_ld;
    const int32_t* particles_ld;       /* VVIntegrator::addParticleLangevin                         */
    int32_t num_image_pairs;
    const int32_t* image_pairs;        /* (image, parent) = VVIntegrator::addImagePair      [2*n]   */
    int32_t num_electrolyte;
    const int32_t* particles_electrolyte; /* VVIntegrator::addParticleElectrolyte                   */
    /* particle shard owned by this process: atoms [shard_begin, shard_end) of the system described
     * above; must not cut a molecule or a Drude pair.  Device arrays passed to vvhip_bind are indexed
     * from shard_begin.  0,0 = the whole system. */
    int32_t shard_begin, shard_end;
    /* Optional.  System::getConstraintParameters distances [num_constraints] (nm).  When given, the fused steps solve the constraints
     * inside kernels A and B: hydrogen-type clusters (one central particle + up to three peripheral particles of equal mass and
     * distance: what OpenMM's own SHAKE kernel takes, e.g. all X-H bonds), rigid three-site molecules (SETTLE), anything else as
     * general clusters (vvhip_plan_info.num_general_constraints), as long as every connected set of constraints fits one 64-lane wave.
     * NULL: constraints only enter the DOF count and the fused steps refuse to run if there are any (use the split entry points around
     * the host's solver). */
    const double* constraint_distances;
    /* Optional.  System::getVirtualSite for every massless site (OpenMM's TwoParticleAverageSite, ThreeParticleAverageSite,
     * OutOfPlaneSite, LocalCoordinatesSite with three parents -- what examples/ommhelper/oplspsffile.py:982-991 creates for lone pairs).
     * Kernel B then places the sites right after its position update, where the reference calls integration.computeVirtualSites()
     * (HOST:214, 374), and vvhip_plan_info.num_virtual_sites says so; the caller need not launch OpenMM's kernel.  A site is placed from
     * the lane of one of its parents and stored by index (x, y, z; the charge in posq.w stays), so sites cost no work items.
     *   virtual_sites       [5*n]  site particle, kind (VVHIP_VSITE_*), parents 1, 2, 3 (parent 3 = -1 for a two-particle average)
     *   virtual_site_params [12*n] AVERAGE2: w1 w2; AVERAGE3: w1 w2 w3; OUT_OF_PLANE: w12 w13 wCross;
     *                              LOCAL_COORDS: origin weights[3], x weights[3], y weights[3], local position[3] */
    int32_t num_virtual_sites;
    const int32_t* virtual_sites;
    const double* virtual_site_params;
} vvhip_system_desc;

enum { VVHIP_VSITE_AVERAGE2 = 0, VVHIP_VSITE_AVERAGE3 = 1, VVHIP_VSITE_OUT_OF_PLANE = 2, VVHIP_VSITE_LOCAL_COORDS = 3 };

/* VVIntegrator's parameters (openmmapi/include/openmm/VVIntegrator.h:70-431).  The reference reads
 * them through getters at every kernel call; here they are re-read whenever vvhip_set_params is
 * called.  Thermostat masses / DOF are fixed at plan creation, as in the reference (HOST:583-594). */
typedef struct {
    double temperature, frequency, drude_temperature, drude_frequency, step_size;
    int32_t num_nh_chains, loops_per_step;
    double max_drude_distance;
    double friction, drude_friction;
    double mirror_location;
    double electric_field;             /* kJ/(nm e) per particle, as VVIntegrator::setElectricField  */
    double cos_acceleration;
    int32_t use_com_temp_group, use_middle_scheme;
    int32_t auto_set_com_temp_group;   /* 1 = constructor default not overridden (API:67,106-121)    */
    int32_t auto_set_friction;
    double constraint_tolerance;       /* Integrator::getConstraintTolerance (relative, 1e-5 by default); used by the in-kernel SHAKE */
} vvhip_params;

/* Device arrays owned by the caller (OpenMM's HipContext / HipIntegrationUtilities in the plugin). */
typedef struct {
    void* velm;            /* mixed4 [n]: xyz = velocity, w = 1/mass       cu.getVelm()            */
    void* posq;            /* real4  [n]: xyz = position, w = charge       cu.getPosq()            */
    void* posq_correction; /* real4  [n], mixed mode only, else NULL       cu.getPosqCorrection()  */
    void* force;           /* int64  [3*padded]: planar x|y|z, x 2^32      cu.getForce()           */
    void* pos_delta;       /* mixed4 [n], only for the split (constraint) entry points; may be NULL */
    const void* random;    /* float4 [random_size] N(0,1)                  integration.getRandom() */
    uint32_t random_size;
    void* stream;          /* hipStream_t; NULL = the null stream                                  */
} vvhip_buffers;

/* Results of the host-side analysis (readable without a GPU). */
typedef struct {
    int32_t num_particles_nh, num_molecules_nh, num_normal_nh, num_pairs_nh;
    int32_t num_normal_ld, num_pairs_ld, num_images, num_electrolyte;
    int32_t num_temp_groups;                     /* HOST:567-573 */
    int32_t use_com_temp_group;                  /* after the auto rule, API:106-121 */
    double friction;                             /* after the auto rule */
    double dof[VVHIP_NUM_TG], nkbt[VVHIP_NUM_TG];
    double eta_mass[VVHIP_NUM_TG][VVHIP_MAX_CHAINS];
    double inv_mass_total;                       /* HOST:1028-1031 */
    int32_t num_waves, num_slots_used;           /* work-item layout: 64 slots per wave */
    int32_t max_cluster;                         /* largest set of particles that must share a wave */
    int32_t num_shake_clusters;                  /* hydrogen-type constraint clusters solved in-kernel (SHAKE; 0 if none / not possible) */
    int32_t constraints_fused;                   /* 1: no constraints, or all of them are handled in-kernel (hydrogen-type clusters, rigid three-site
                                                    molecules, or general clusters: num_general_constraints) => fused steps are valid */
    int32_t num_settle_clusters;                 /* rigid three-site molecules solved in-kernel (SETTLE) */
    int32_t periodic_layout;                     /* 1: the work-item layout is arithmetic (runs of identical molecules): the fused kernels compute
                                                    particle indices instead of loading them (vv_host.hpp: PeriodicLayout) */
    int32_t num_general_constraints;             /* constraints outside the two rules above (AllBonds, HAngles: chains, rings, triangles) that the
                                                    fused kernels relax by coloured Gauss-Seidel sweeps inside the wave of their molecule; 0 if the
                                                    System has none, or if a component of the constraint graph does not fit one wave */
    int32_t num_virtual_sites;                   /* virtual sites placed by kernel B itself (0: none given, or one of them cannot share a wave with
                                                    its parents -- then the caller runs its own computeVirtualSites after every step, as before) */
    double general_relaxation;                   /* relaxation factor of the general clusters' sweeps (1.2; 1.4 when constraints close triangles); 0 if none */
} vvhip_plan_info;

/* Nose-Hoover chain state + last reduction results (HOST: CudaVVKernels.h:206-215).  The reference
 * keeps these on the host and loses them on restart; here they live on the device and can be saved. */
typedef struct {
    double eta[VVHIP_NUM_TG][VVHIP_MAX_CHAINS];
    double eta_dot[VVHIP_NUM_TG][VVHIP_MAX_CHAINS + 1];
    double eta_dotdot[VVHIP_NUM_TG][VVHIP_MAX_CHAINS];
    double ke2[VVHIP_NUM_TG];                    /* last 2*KE per temperature group */
    double vscale[VVHIP_NUM_TG];                 /* last velocity scale factors     */
    double v_bias;                               /* last periodic velocity bias V (vMaxBuffer[0]) */
} vvhip_nh_state;

/* ---------------------------------------------------------------- life cycle */
/* Host-only: partitions particles (NH / Langevin / image), checks the reference's conflict rules,
 * counts DOF, sizes the thermostat chains and lays particles out in 64-lane waves so that every
 * Drude pair and (with the COM temperature group) every molecule sits inside one wave.
 * Replaces VVIntegrator::initialize's table building (API:123-155) and the initialize() methods of
 * all seven Cuda*Kernel classes.  Does not touch the GPU. */
int vvhip_plan_create(const vvhip_system_desc* system, const vvhip_params* params, int precision,
                      vvhip_plan** plan_out, char* errbuf, size_t errbuf_len);
void vvhip_plan_destroy(vvhip_plan* plan);
const char* vvhip_last_error(const vvhip_plan* plan);
int vvhip_plan_get_info(const vvhip_plan* plan, vvhip_plan_info* info);
/* Copies the wave layout: slots[2*i] = particle index (shard-relative, -1 = idle lane),
 * slots[2*i+1] = packed role word.  `capacity` in slots; returns the number of slots or <0. */
/* Why vvhip_plan_info.constraints_fused is 0 for this plan ("" when it is 1 or the System has no constraints): what of the constraint topology
 * did not fit the in-kernel solvers -- a component with more than the 64 constraints of a wave's list, a particle in more constraints than the 16
 * colours of the sweeps, a constraint across two waves.  The fused steps then refuse (VVHIP_ERR_UNSUPPORTED, with this text) and the split
 * entry points leave the gaps for the host's own solver. */
const char* vvhip_plan_unfused_reason(const vvhip_plan* plan);
int vvhip_plan_get_slots(const vvhip_plan* plan, int32_t* slots, int32_t capacity);

/* Binds device arrays and allocates the plan's own device state (forceExtra, oldDelta, accumulators,
 * chain state, layout tables) on the current device.  First call that needs a GPU. */
int vvhip_bind(vvhip_plan* plan, const vvhip_buffers* buffers);
int vvhip_set_params(vvhip_plan* plan, const vvhip_params* params);
int vvhip_set_box(vvhip_plan* plan, const double box[3]);      /* cu.getPeriodicBoxSize() (HOST:1057,1129) */
/* The plan caches, per work-item, the mass RECIP(velm.w) and the Drude-pair mass fractions (filled on the device from velm.w in
 * front of the first launch that needs them; the reference recomputes them in every kernel, K/drudeNoseHoover.cu:173-180).  A host
 * that rewrites the inverse masses in velm.w (OpenMM does so only in Context::reinitialize, which rebuilds the kernels anyway)
 * calls this; binding a different velm array does it implicitly. */
int vvhip_masses_changed(vvhip_plan* plan);
/* Blocking copies of the thermostat state (checkpoint / tests). */
int vvhip_get_nh_state(vvhip_plan* plan, vvhip_nh_state* out);
int vvhip_set_nh_state(vvhip_plan* plan, const vvhip_nh_state* in);

/* ---------------------------------------------------------------- fused path
 * One whole VVIntegrator step between two force evaluations.  Constraints are solved inside the two kernels when
 * vvhip_plan_info.constraints_fused says so (otherwise the fused steps refuse to run and the split entry points below go around the
 * host's solver); virtual sites are placed by kernel B when described (vvhip_system_desc.virtual_sites), otherwise the caller's own
 * computeVirtualSites follows the step as it follows the reference's.  Forces for the step must already be in `force`.
 *
 * Middle scheme (API:232-270 after calcForcesAndEnergy): 2 launches
 *   pass A: extra forces (Langevin, E-field, cos) + full kick (+ velocity constraints) + molecular COM + per-group
 *           2KE -> fixed-point accumulators; with cos acceleration also the bias moment and the group sums as
 *           moments of the still biased velocities, so that no launch is needed between bias and 2KE
 *   pass B: NH chain (device) + velocity scaling + bias remove/restore + both half drifts (+ position
 *           constraints) + hard wall + image mirror
 * Only molecules larger than one 64-lane wave, chains longer than 4 and systems beyond ~2.6 M particles take more
 * launches (per-molecule COM accumulation, stand-alone chain kernel, the three-launch cos sequence).
 * Classic scheme: vvhip_step_vv_first() = API:295-310, vvhip_step_vv_second() = API:316-336.
 * `random_index` = integration.prepareRandomNumbers(...) for this step (HOST:863), ignored unless
 * Langevin particles exist. */
int vvhip_step_middle(vvhip_plan* plan, uint32_t random_index);
int vvhip_step_vv_first(vvhip_plan* plan);
int vvhip_step_vv_second(vvhip_plan* plan, uint32_t random_index);
/* vvhip_step_middle cut at its global reductions, for hosts that shard particles over GPUs and run a
 * collective in between.  A step has vvhip_step_middle_phases() phases (1 without NH particles, else 2; 3 only
 * where the cos perturbation cannot use its moment form, see above).  After every phase but the last, the host sums
 * the accumulator range reported by vvhip_accumulators(phase) element-wise over ranks (ncclSum on
 * int64; fixed point makes the result independent of rank order) on the plan's stream:
 *     for (ph = 0; ph < P; ph++) { vvhip_step_middle_phase(plan, ph, ri); if (ph < P-1) all_reduce(acc(ph)); }
 * That all-reduce (64 int64 slots per reduced quantity, <= 1.5 KB, latency-bound) is the only cross-GPU
 * exchange per thermostat application. */
int vvhip_step_middle_phases(const vvhip_plan* plan);
/* Algorithmic bytes per particle moved by kernel A / kernel B of this plan's fused middle step (particle arrays + 6 bytes of index per
 * pass, SURVEY section 8d's accounting).  Plans without extra forces and in-kernel constraints keep the kicked velocities in registers in
 * kernel A and repeat the kick in kernel B: 62 + 158 bytes in mixed precision instead of 94 + 134. */
int vvhip_algorithmic_bytes(const vvhip_plan* plan, int32_t* bytes_a, int32_t* bytes_b);
int vvhip_step_middle_phase(vvhip_plan* plan, int phase, uint32_t random_index);
int vvhip_accumulators(vvhip_plan* plan, int phase, void** device_ptr, int32_t* count);

/* Built-in exchange.  Instead of running the collective itself, a host may hand the plan an RCCL communicator:
 * rank 0 calls vvhip_comm_unique_id(), ships the 128 bytes to the other ranks by any means (bench.py uses
 * torch.distributed), every rank calls vvhip_comm_init(); from then on vvhip_step_middle / vvhip_run_graph /
 * vvhip_run_eager issue ncclAllReduce(int64, sum) on the plan's stream between the phases themselves, so a whole
 * sharded step (or a captured graph of steps) needs no host involvement.  librccl is resolved at run time. */
int vvhip_comm_unique_id(void* id128);
int vvhip_comm_init(vvhip_plan* plan, const void* id128, int nranks, int rank);
int vvhip_comm_destroy(vvhip_plan* plan);
/* Ranks of the plan's communicator as RCCL itself reports them (ncclCommCount; 0 without a communicator): what bench.py prints as
 * config.exchange.rccl_ranks, so that a scaling line says how many ranks the collective really spanned. */
int vvhip_comm_count(vvhip_plan* plan, int32_t* ranks);
/* hipDeviceCanAccessPeer(device, peer_device): whether the mailbox's hipIpc mappings of a peer's box can be direct (xGMI / PCIe P2P). */
int vvhip_peer_access(int device, int peer_device, int32_t* can_access);

/* Exchange without a collective launch, for the ranks of ONE node ("mailbox" over xGMI peer mappings).  Every rank calls
 * vvhip_mailbox_create (allocates its uncached box, returns a 64-byte hipIpc handle), the host gathers all handles in rank
 * order (ranks * 64 bytes, any transport) and every rank calls vvhip_mailbox_connect.  From then on the thermostat wave of block 0
 * of kernel B -- which has just folded the rank's accumulators, complete since kernel A ended -- stores the rank's int64 totals into
 * every peer's box (one 8-byte {sequence, payload} word each) and the thermostat wave of every block polls the rank's own box and
 * adds the peers' words: a sharded step stays two launches, replayable from a hipGraph, and all ranks continue with identical
 * bits.  Carries the three kinetic-energy totals, and with the cos perturbation in its moment form also the bias moment and the
 * six group moments (10 totals = 20 words); chain lengths <= 4 (vvhip_mailbox_status: active); everything else keeps using the
 * RCCL communicator if one is set.  A rank that does not hear from its peers within ~5 s raises a sticky flag and carries on
 * with incomplete sums instead of hanging the GPU; the flag surfaces as VVHIP_ERR_EXCHANGE from vvhip_synchronize and from the
 * next vvhip_run_graph / vvhip_run_eager (see vvhip_status), so a host can never take a figure from a diverged run.
 * No reference counterpart (the reference is single-GPU: CudaVVKernelFactory.cpp:68). */
int vvhip_mailbox_create(vvhip_plan* plan, int nranks, int rank, void* handle64);
int vvhip_mailbox_connect(vvhip_plan* plan, const void* handles);
int vvhip_mailbox_status(vvhip_plan* plan, int32_t* active, int32_t* timed_out);
int vvhip_mailbox_destroy(vvhip_plan* plan);
/* After vvhip_mailbox_connect: *shared_device = 1 if a peer's box lives on this rank's own device (several ranks on one GPU: test
 * set-ups) -- kernel B then keeps the explicit work-item layout next to the exchange; *arithmetic_layout = 1 if kernel B of this plan
 * takes the arithmetic layout together with the mailbox exchange. */
int vvhip_mailbox_layout(vvhip_plan* plan, int32_t* shared_device, int32_t* arithmetic_layout);

/* ---------------------------------------------------------------- kernel-interface level
 * One entry per KernelImpl virtual, for use inside OpenMM where constraint solvers run between them. */
/* IntegrateMiddleStepKernel (VVKernels.h:50-86; HOST:119-235) */
int vvhip_reset_extra_force(vvhip_plan* plan);                 /* resetExtraForce                      */
int vvhip_middle_kick(vvhip_plan* plan);                       /* firstIntegrate, before applyVelocityConstraints (HOST:144-148) */
int vvhip_middle_half_drift1(vvhip_plan* plan);                /* firstIntegrate, after  (HOST:154-158) */
int vvhip_middle_half_drift2(vvhip_plan* plan);                /* secondIntegrate, before applyConstraints (HOST:169-173) */
int vvhip_middle_finish(vvhip_plan* plan);                     /* secondIntegrate, after: Pos3 + hard wall (HOST:179-212) */
/* IntegrateVVStepKernel (VVKernels.h:94-130; HOST:296-442) */
int vvhip_vv_half_kick(vvhip_plan* plan, int update_pos_delta);/* HOST:341-348 / 417-424 */
int vvhip_vv_positions(vvhip_plan* plan);                      /* HOST:355-372: positions + hard wall */
/* ModifyDrudeNoseKernel (VVKernels.h:138-157; HOST:670-754): 2 launches (sums | chain + scaling), no host round trip */
int vvhip_scale_velocity(vvhip_plan* plan);
/* ModifyDrudeLangevinKernel (VVKernels.h:165-184; HOST:826-872) */
int vvhip_apply_langevin_force(vvhip_plan* plan, uint32_t random_index);
/* ModifyImageChargeKernel (VVKernels.h:192-211; HOST:904-934) */
int vvhip_update_image_positions(vvhip_plan* plan);
/* ModifyElectricFieldKernel (VVKernels.h:219-238; HOST:971-992) */
int vvhip_apply_electric_force(vvhip_plan* plan);
/* ModifyCosineAccelerateKernel (VVKernels.h:246-269; HOST:1037-1134) */
int vvhip_apply_cosine_force(vvhip_plan* plan);
int vvhip_calc_velocity_bias(vvhip_plan* plan);
int vvhip_remove_velocity_bias(vvhip_plan* plan);
int vvhip_restore_velocity_bias(vvhip_plan* plan);
int vvhip_calc_viscosity(vvhip_plan* plan, double* v_max, double* inv_viscosity);   /* blocks; 8-byte copy */
/* 1/2 sum m v^2 over all massive particles of this shard (blocks; the reference forwards computeKineticEnergy to OpenMM's
 * integration utilities, CudaVVKernels.cpp:233-235 -- a stand-alone host has no such service). kJ/mol. */
int vvhip_compute_kinetic_energy(vvhip_plan* plan, double* kinetic_energy);
/* Drude temperature report: the temperatures of the molecules' centres of mass, of the atoms inside them and of the Drude pairs'
 * relative motion in the current velocities, as examples/ommhelper/reporter/drudetemperaturereporter.py defines them, over ALL
 * particles (NH and Langevin subsets, images and sites alike; massless particles add nothing).  ke = KE_COM, KE_Atom, KE_Drude in
 * kJ/mol, t = T_COM, T_Atom, T_Drude in K; T = 2 KE / (dof R), R = 8.31446261815324e-3 kJ/(mol K), and 0 where dof <= 0 (a System
 * without Drude pairs reports T_Drude = 0).  Runs in the plan's stream behind what is queued, blocks, copies 56 bytes back, and
 * touches no state of the step (accumulators, thermostat, status words, captured graphs).  The sums are fixed point: the same
 * velocities give the same bits whatever the launch shape or the split into shards.  A term outside the fixed-point range (a velocity
 * far beyond physical values, NaN) gives VVHIP_ERR_OVERFLOW for this call only; a plan whose shard cuts a molecule gives
 * VVHIP_ERR_UNSUPPORTED.
 * A SHARD reports its own particles' sums and the WHOLE system's DOFs: add the raw sums of all shards (vvhip_drude_report_raw, int64
 * sums) and turn the total into numbers with vvhip_drude_report_combine -- the single-GPU result, bit for bit. */
int vvhip_drude_temperatures(vvhip_plan* plan, double ke[3], double t[3]);
/* DOFs of the report (COM, Atom, Drude) for the whole system; host only, works on an unbound plan. */
int vvhip_drude_report_dof(const vvhip_plan* plan, double dof[3]);
/* The report's raw sums of 2 KE: (hi, lo) words of sum m|v|^2, of the Drude pairs' term and of the COM term (value = (hi + lo 2^-F) 2^-U,
 * F and U fixed per system: vvhip_drude_report_combine's business); blocks like vvhip_drude_temperatures. */
int vvhip_drude_report_raw(vvhip_plan* plan, int64_t raw[6]);
/* ke / t from raw sums (one shard's, or the element-wise sum over all shards); host only. */
int vvhip_drude_report_combine(const vvhip_plan* plan, const int64_t raw[6], double ke[3], double t[3]);

/* ---------------------------------------------------------------- series: samples recorded on the device
 * A device buffer of rows, configured once per plan.  The plan counts full steps (host side): vvhip_step_middle, vvhip_step_vv_second,
 * the last phase of vvhip_step_middle_phase and the steps of vvhip_run_graph / vvhip_run_eager each advance the count by one; the split
 * per-KernelImpl entry points (vvhip_middle_kick ... vvhip_middle_finish, vvhip_run_eager_unfused) do not, and take no rows.  After every
 * step whose count is a multiple of `interval`, the step entry point itself enqueues one row in the plan's stream: the Drude report's two
 * passes (vvhip_drude_report_raw's kernels, on scratch of the series' own) and one append kernel.  Inside a captured graph the row launches
 * are part of the graph: replays record rows without any host synchronisation.  The row index comes from a device-side cursor; a row past
 * `capacity` is not written but counted as dropped, and the cursor advances either way.  Nothing else of the step changes: a plan without
 * a series launches what it launched before, and a series leaves positions, velocities and thermostat state bit for bit as they were.
 * Row j (0-based, since the start or the last reset) holds the state after step interval * (k0 + j); vvhip_series_read returns that step
 * of row 0.  The graph cache keys on the steps of the graph that take rows: when `interval` divides the graph's length or the length
 * divides `interval`, each parity needs at most two executables and steady-state replays re-capture nothing.  Start, stop and a
 * change of box or parameters drop the captured graphs (the box and cos acceleration of a row are baked into its kernel arguments). */
#define VVHIP_SERIES_DRUDE 1        /* the Drude report's raw words (drude_raw, drude_overflow) */
#define VVHIP_SERIES_THERMOSTAT 2   /* the thermostat state as vvhip_get_nh_state would return it after the step, plus box and cos acceleration */
typedef struct {
    int64_t drude_raw[6];           /* vvhip_drude_report_raw's six words of this shard's particles (0 without VVHIP_SERIES_DRUDE) */
    int64_t drude_overflow;         /* != 0: a term left the fixed-point range (vvhip_drude_report_raw would fail); the row's words are void */
    int64_t reserved;               /* 0 */
    vvhip_nh_state nh;              /* d_nh of the parity current after the step (0 without VVHIP_SERIES_THERMOSTAT) */
    double box[3];                  /* periodic box and cos acceleration the step ran with: with nh.v_bias the inputs of vvhip_calc_viscosity */
    double cos_acceleration;
} vvhip_series_row;
typedef struct {
    int32_t row_bytes;              /* sizeof(vvhip_series_row) */
    int32_t off_drude_raw, off_nh, off_box;     /* byte offsets of the parts inside a row */
    int32_t active, interval, capacity, mask;   /* the series as configured (active = 0: none) */
    int64_t steps;                  /* full steps the plan has counted since vvhip_bind */
    int64_t graph_captures;         /* graph executables captured since vvhip_bind (the cache's misses) */
} vvhip_series_layout;
/* Starts (or restarts, dropping what was recorded) a series on a bound plan: interval >= 1 steps, capacity >= 1 rows, mask of
 * VVHIP_SERIES_*.  VVHIP_SERIES_DRUDE on a plan that cannot report gives VVHIP_ERR_UNSUPPORTED (as vvhip_drude_report_raw).  Synchronises. */
int vvhip_series_start(vvhip_plan* plan, int32_t interval, int32_t capacity, int32_t mask);
/* Synchronises, copies min(rows recorded, capacity, max_rows) rows to rows_out (may be null with max_rows = 0), and returns the rows
 * recorded (n_rows: at most capacity), the step of row 0 and the rows dropped for want of capacity.  reset != 0 empties the buffer: the
 * next row then becomes row 0 and continues the schedule without gap or repeat. */
int vvhip_series_read(vvhip_plan* plan, vvhip_series_row* rows_out, int32_t max_rows, int32_t* n_rows, int64_t* first_step,
                      int64_t* dropped, int32_t reset);
/* Stops the series: no more rows are enqueued; the buffer is released. */
int vvhip_series_stop(vvhip_plan* plan);
/* The row layout, the series' configuration and the step / capture counters; host only, works on an unbound plan. */
int vvhip_series_info(const vvhip_plan* plan, vvhip_series_layout* out);
/* Test hook: 1 if the guard row behind the buffer's last row still holds its fill pattern (nothing was written past capacity). */
int vvhip_debug_series_guard(vvhip_plan* plan, int32_t* intact);
/* ---------------------------------------------------------------- frames: the trajectory recorded on the device
 * What DCDReporter / GroReporter(logarithm=True, subset=...) give a run inside OpenMM (examples/run-bulk.py, run-edl.py): a stand-alone
 * host would have to end its run call, synchronise and download posq and posqCorrection of every particle for each frame.  A frame is a
 * series row that is large: a device buffer of `capacity` frames, a device-side cursor, and after every full step that is due -- counted
 * exactly as for the series, by the same entry points; the split per-KernelImpl entry points and vvhip_run_eager_unfused take none -- the
 * step entry point enqueues one streaming kernel (csrc/vv_dev_frames.inc) and a one-thread kernel that writes the frame's header and
 * advances the cursor.  Inside a captured graph both are part of the graph and the steps that take a frame are part of the graph-cache
 * key.  A frame "after step k" is enqueued behind that step's series row and in front of the removal that precedes step k + 1.  The
 * recorder reads posq, posqCorrection and velm and writes its own buffer and cursor, nothing else; a plan that never starts one launches
 * what it launched before and allocates nothing.
 * Schedule, after full step s (vvhip_frames_schedule is its one statement):
 *     VVHIP_FRAMES_LINEAR   s mod interval = 0
 *     VVHIP_FRAMES_LOG10    GroReporter's logarithmic rule: from step c the next frame is at c + base - (c mod base), base = interval
 *                           while c < interval, else the largest power of ten <= c -- with interval 30: 30, 40, ..., 90, 100, 200, ...,
 *                           900, 1000, 2000, ...  Equivalently s is due iff s = interval, or s > interval and s mod 10^floor(log10(s - 1))
 *                           = 0: a function of s alone, wherever the recorder starts.
 * Frame j (0-based, since the start or the last reset) belongs to the j-th due step after start_step (after the last frame counted
 * before the reset); frames dropped for want of capacity count.
 * Frame layout (vvhip_frames_info): the 64 bytes of vvhip_frame_header, then per quantity three component planes x | y | z of
 * plane_stride elements each (what a DCD frame is on disk), positions first; elements past num_particles stay zero.  Values for recorded
 * particle i, converted once:
 *     mixed precision    float64: (double) posq.xyz + (double) posqCorrection.xyz      float32: that sum rounded once to nearest
 *     single             float64: (double) posq.xyz                                    float32: the bits of posq.xyz
 *     double             float64: posq.xyz                                             float32: (float) posq.xyz
 * and velm.xyz the same way.  Positions are as stored: unwrapped, image particles and virtual sites included.  box is the plan's box when
 * the frame was enqueued (a kernel argument: vvhip_set_box drops the captured graphs).
 * A sharded plan records its own particles: subset intersected with [shard_begin, shard_end), named by vvhip_frames_particles. */
#define VVHIP_FRAMES_POSITIONS  1
#define VVHIP_FRAMES_VELOCITIES 2
#define VVHIP_FRAMES_FLOAT64    4      /* components as double instead of float */
enum { VVHIP_FRAMES_LINEAR = 0, VVHIP_FRAMES_LOG10 = 1 };
typedef struct {
    int32_t interval, schedule, capacity, mask;
    int32_t num_subset;             /* 0 with subset = NULL: every particle of the plan */
    const int32_t* subset;          /* global particle indices, strictly ascending */
} vvhip_frames_desc;
typedef struct {
    int64_t ordinal;                /* the frame's index since the start or the last reset, from the device-side cursor */
    int64_t reserved;               /* 0 */
    double box[3];
    double pad[3];                  /* 0 */
} vvhip_frame_header;               /* 64 bytes, written on the device */
typedef struct {
    int32_t active, interval, schedule, capacity, mask;
    int32_t num_particles;          /* particles this plan records: |subset intersected with [shard_begin, shard_end)| */
    int32_t component_bytes;        /* 4 or 8 */
    int32_t plane_stride;           /* elements per component plane: num_particles rounded up to a multiple of 16 */
    int64_t frame_bytes;            /* 64 + planes * plane_stride * component_bytes */
    int64_t off_positions, off_velocities;      /* byte offsets of the x plane inside a frame, -1 if absent; planes follow as x | y | z */
    int64_t start_step;             /* the plan's step count at vvhip_frames_start */
} vvhip_frames_layout;
/* Starts (or restarts, dropping what was recorded) a recorder; synchronises and drops the captured graphs.  Refused, in this order:
 * interval < 1, capacity < 1, a mask without VVHIP_FRAMES_POSITIONS / VVHIP_FRAMES_VELOCITIES or with unknown bits, an unknown schedule,
 * a subset that is not strictly ascending or leaves [0, num_atoms) (VVHIP_ERR_INVALID naming the argument); an unbound plan; inside a
 * graph capture (VVHIP_ERR_INVALID); an allocation that fails (VVHIP_ERR_HIP with the byte count).  A description that passes the argument
 * checks is kept even where the start is then refused for an unbound plan (active = 0): vvhip_frames_info and vvhip_frames_particles
 * answer for it, so a host can size its buffers before it binds. */
int vvhip_frames_start(vvhip_plan* plan, const vvhip_frames_desc* desc);
/* Synchronises, copies min(frames recorded, capacity, max_frames) frames of frame_bytes each to frames_out and their steps to steps_out
 * (either may be null with max_frames = 0), and returns the frames recorded (n_frames: at most capacity) and the frames dropped for
 * want of capacity.  A header whose ordinal is not its frame's index gives VVHIP_ERR_HIP.  reset != 0 empties the buffer: the next
 * frame becomes frame 0 and continues the schedule without gap or repeat. */
int vvhip_frames_read(vvhip_plan* plan, void* frames_out, int64_t* steps_out, int32_t max_frames, int32_t* n_frames, int64_t* dropped,
                      int32_t reset);
/* Stops the recorder: no more frames are enqueued, the buffers are released, the description is forgotten; synchronises and drops the
 * captured graphs. */
int vvhip_frames_stop(vvhip_plan* plan);
/* The layout of the recorder as described (zeros with active = 0 if none was); host only, works on an unbound plan. */
int vvhip_frames_info(const vvhip_plan* plan, vvhip_frames_layout* out);
/* The global indices of the particles this plan records, in frame order: the first min(num_particles, capacity) of them
 * (vvhip_frames_info gives num_particles); VVHIP_ERR_INVALID if no recorder was described; host only. */
int vvhip_frames_particles(const vvhip_plan* plan, int32_t* global_indices, int32_t capacity);
/* The first n due steps greater than after_step (>= 0) of a schedule; host only, no plan.  VVHIP_ERR_INVALID for interval < 1, an unknown
 * schedule, after_step < 0, n < 0, or steps beyond 2^61 (the logarithmic schedule reaches them within a few hundred frames). */
int vvhip_frames_schedule(int32_t interval, int32_t schedule, int64_t after_step, int32_t n, int64_t* steps_out);
/* Test hook: 1 if the guard frame behind the buffer's last frame still holds its fill pattern (nothing was written past capacity). */
int vvhip_debug_frames_guard(vvhip_plan* plan, int32_t* intact);
/* ---------------------------------------------------------------- profiles: density and velocity profiles accumulated on the device
 * What run-edl.py is run for (number and charge density along z between the electrodes) and what a --cos run of run-bulk.py is run for
 * (the velocity profile v_x of z): sums over particles and samples per bin of one box axis.  A stand-alone host would get them from
 * trajectory frames, 44 B per particle and sample, and bin on the host; a profile is a few KB however many samples it holds.  After every
 * full step whose count is a multiple of `interval` -- counted exactly as for the series and the frames, by the same entry points; a
 * sample "after step k" is enqueued behind that step's frame -- the step entry point enqueues one accumulating kernel
 * (csrc/vv_dev_profile.inc) and a one-thread kernel that advances the sample count.  Inside a captured graph both are part of the graph and
 * the steps that take a sample are part of the graph-cache key.  The recorder reads posq, posqCorrection and velm and writes its own table,
 * nothing else; a plan that never starts one launches what it launched before and allocates nothing.
 * Arithmetic, all float64 without contraction.  For recorded particle i with coordinate c along `axis` -- (double) posq + (double)
 * posqCorrection in mixed precision, else (double) posq; positions are stored unwrapped --
 *     t = c * inv_L,  inv_L = 1.0 / box[axis] (formed on the host from the plan's box when the sample is enqueued: vvhip_set_box drops the
 *     captured graphs),  u = t - floor(t),  b = min((int) (u * (double) nbins), nbins - 1)
 * which is the periodic wrap: c = -1e-20 gives u = 1.0 and lands in the last bin by the clamp.  With v = (double) velm.xyz and m the
 * System's mass of the particle as the plan holds it, the terms per quantity are
 *     COUNT     1
 *     CHARGE    (double) posq.w, as it stands at the sample
 *     MASS      m
 *     MOMENTUM  m * v.x, m * v.y, m * v.z     (three rows)
 *     KINETIC   m * ((v.x * v.x + v.y * v.y) + v.z * v.z)
 * and a term x is added as the integer llrint(x * 2^frac_bits[quantity]), round-half-even (COUNT: the integer 1).  Integer adds commute:
 * the table is the same bits for any launch shape, arrival order or shard split, and the shards' tables add to the unsharded table exactly.
 * A particle any of whose enabled terms is NaN or has |x| >= limit[quantity] is left out of EVERY row for that sample and adds 1 to
 * out_of_range instead.
 * Table: int64 table[num_groups][rows][nbins], the rows being the enabled quantities in the order above (vvhip_profile_layout::row_of).
 * Fraction bits: frac_bits[q] = min(40, 62 - ceil_log2(N + 1) - ceil_log2(max_samples + 1) - log2(limit[q])), so that no word can
 * overflow within max_samples samples; past max_samples a sample adds nothing and counts as dropped.  N and the default limits are those of
 * the description over the WHOLE System (N = num_particles on an unsharded plan): a sharded plan records the particles of its own shard,
 * every shard scales its terms alike, and the shards' tables add as integers to the unsharded table.
 * Unlike a series row or a frame, an accumulating table is not idempotent under the repeat of failed steps: a repaired rendezvous
 * (vvhip_recovery_count) puts the WHOLE allocation, counts and table, back with the step counter before it repeats the steps. */
#define VVHIP_PROFILE_COUNT    1       /* always on */
#define VVHIP_PROFILE_CHARGE   2
#define VVHIP_PROFILE_MASS     4
#define VVHIP_PROFILE_MOMENTUM 8
#define VVHIP_PROFILE_KINETIC  16
enum { VVHIP_PROFILE_Q_COUNT = 0, VVHIP_PROFILE_Q_CHARGE = 1, VVHIP_PROFILE_Q_MASS = 2, VVHIP_PROFILE_Q_MOMENTUM = 3, VVHIP_PROFILE_Q_KINETIC = 4,
       VVHIP_PROFILE_QUANTITIES = 5 };
typedef struct {
    int32_t interval;               /* a sample after every step whose count is a multiple of it */
    int32_t axis;                   /* 0, 1, 2: the box axis the bins divide */
    int32_t nbins;                  /* 1 .. 65536 */
    int32_t mask;                   /* VVHIP_PROFILE_*; COUNT is on whether named or not */
    int32_t num_groups;             /* 1 .. 16 */
    int32_t reserved;               /* 0 */
    const signed char* group;       /* [num_atoms] the group of every particle of the System, -1: not recorded; NULL: everything in group 0 */
    int64_t max_samples;            /* >= 1 */
    double limit[4];                /* charge (e), mass (Da), momentum (Da nm/ps), kinetic (Da nm^2/ps^2): terms at or beyond it are out of
                                       range; rounded up to a power of two.  0 takes the default: charge 16, mass the smallest power of two
                                       above the largest recorded mass, momentum 64 x the mass limit, kinetic 4096 x the mass limit */
} vvhip_profile_desc;
typedef struct {
    int64_t samples;                /* samples in the table since the start or the last reset (at most max_samples) */
    int64_t dropped;                /* samples that were due past max_samples: nothing was added for them */
    int64_t out_of_range;           /* particle-samples left out of every row */
} vvhip_profile_counts;
typedef struct {
    int32_t active, interval, axis, nbins, mask, num_groups;
    int32_t num_particles;          /* particles this plan records: group >= 0 within [shard_begin, shard_end) */
    int32_t rows;                   /* rows per group: 1 .. 7 */
    int64_t max_samples;
    int64_t words;                  /* num_groups * rows * nbins */
    int64_t start_step;             /* the plan's step count at vvhip_profile_start */
    int32_t row_of[VVHIP_PROFILE_QUANTITIES];       /* first row of a quantity inside a group, -1: not recorded */
    int32_t frac_bits[VVHIP_PROFILE_QUANTITIES];    /* value = word * 2^-frac_bits (COUNT: 0) */
    double limit[VVHIP_PROFILE_QUANTITIES];         /* as applied (COUNT: 1) */
} vvhip_profile_layout;
/* Starts (or restarts, dropping what was accumulated) a recorder; synchronises and drops the captured graphs.  Refused, in this order:
 * interval < 1, axis outside 0 .. 2, nbins outside 1 .. 65536, unknown mask bits, num_groups outside 1 .. 16, max_samples < 1, a limit that
 * is negative or not finite, a group entry outside -1 .. num_groups - 1, a quantity whose frac_bits would come out below 8
 * (VVHIP_ERR_INVALID naming the argument or the quantity); an unbound plan; inside a graph capture (VVHIP_ERR_INVALID); an allocation that
 * fails (VVHIP_ERR_HIP).  A description that passes the argument checks is kept even where the start is then refused for an unbound plan
 * (active = 0): vvhip_profile_info answers for it. */
int vvhip_profile_start(vvhip_plan* plan, const vvhip_profile_desc* desc);
/* Synchronises and copies the counts (out may be NULL) and the table's `words` words (words_out may be NULL with capacity_words = 0;
 * a capacity below the table's size is VVHIP_ERR_INVALID).  reset != 0 zeroes counts and table: the schedule continues without gap or
 * repeat. */
int vvhip_profile_read(vvhip_plan* plan, int64_t* words_out, int64_t capacity_words, vvhip_profile_counts* out, int32_t reset);
/* Stops the recorder: no more samples are enqueued, the table is released, the description is forgotten; synchronises and drops the
 * captured graphs. */
int vvhip_profile_stop(vvhip_plan* plan);
/* The recorder as described (zeros, row_of = -1, with active = 0 if none was); host only, works on an unbound plan. */
int vvhip_profile_info(const vvhip_plan* plan, vvhip_profile_layout* out);
/* Test hook: with an unverified recovery snapshot in hand (a vvhip_run_graph / vvhip_run_eager call of at least 64 steps since the last
 * vvhip_synchronize), drains the stream and repairs as after a missed rendezvous -- the snapshot goes back, step counter and riders' words
 * included, the calls since are repeated with two launches per step -- without any rendezvous having failed.  VVHIP_ERR_INVALID without a
 * snapshot. */
int vvhip_debug_recover(vvhip_plan* plan);
/* ---------------------------------------------------------------- mean-squared displacements accumulated on the device
 * What run-bulk.py and run-edl.py add GroReporter('dump.gro', 1000, logarithm=True, ...) for: the mean-squared displacement over many
 * decades of lag time, whose slope gives the ions' diffusion coefficients.  A stand-alone host would get it from trajectory frames, 24 B
 * per particle and sample, and O(samples^2 N) work on the host, the frame ring's capacity bounding the statistics; an accumulating table is
 * a few KB however long the run.  After every full step whose count is a multiple of `interval` -- counted exactly as for the series, the
 * frames and the profiles, by the same entry points (the split per-KernelImpl entry points take none); a sample "after step k" is enqueued
 * behind that step's profile sample -- the step entry point enqueues one accumulating kernel (csrc/vv_dev_msd.inc) and a one-thread kernel
 * that advances the sample ordinal: two launches, no memset, no host work.  Inside a captured graph both are part of the graph and the steps
 * that take a sample are part of the graph-cache key.  The recorder reads posq and posqCorrection and writes its own words, nothing else; a
 * plan that never starts one launches what it launched before and allocates nothing.
 * Units.
 *   VVHIP_MSD_PARTICLES  every recorded particle is a unit.  Its position is X_i in float64, exactly as a float64 frame defines it:
 *                        (double) posq + (double) posqCorrection in mixed precision, (double) posq otherwise; positions are stored unwrapped.
 *   VVHIP_MSD_MOLECULES  a unit is a molecule of vvhip_system_desc.mol_id, restricted to its particles with mass > 0.  Its position is the
 *                        centre of mass in float64 without contraction:  s = 0; for i in ascending particle index: s = s + m_i * X_i;
 *                        c = s / M,  M summed on the host in the same order.  The order of this sum is part of the definition (the
 *                        parallelisation over units is free, the order inside one is not).  The group of a molecule is the group of its
 *                        massive particles; mixed groups inside one molecule are refused; a molecule with group -1, or without mass, is not
 *                        recorded.  A shard that holds some but not all massive particles of a molecule gives VVHIP_ERR_UNSUPPORTED, as the
 *                        barostat and the Drude report do.
 * Schedule.  Sample ordinal j = 0, 1, ... counts the due steps since the start or the last reset.  Every sample whose ordinal is a multiple
 * of origin_every (E) is also stored as an origin, in slot (j / E) mod num_origins of a device ring; num_origins = ceil(num_lags / E) is
 * derived, not chosen.  Row l (0 <= l < num_lags) is the lag of (l + 1) * interval steps.  At sample j every origin k E contributes to row
 * l = j - k E - 1 provided  origin_floor <= k E < j,  j - k E <= num_lags,  and the unit was not out of range.  Accumulation comes first,
 * the store second: when num_origins * E == num_lags the slot that is overwritten was read in the same sample.
 * Terms.  Delta_a = c_a(now) - c_a(origin) in float64, a = x, y, z.  Each of Delta_x^2, Delta_y^2, Delta_z^2 is added as the integer
 * llrint(Delta_a * Delta_a * 2^frac_bits), round-half-even; the pair count as the integer 1.  A unit with any Delta_a that is NaN or has
 * |Delta_a| >= limit is left out of all four words for that pair and adds 1 to out_of_range.  limit is in nm, rounded up to a power of two;
 * 0 takes the default of 64.
 * Table: int64 table[num_groups][num_lags][4], the four words being pairs, sum Delta_x^2, sum Delta_y^2, sum Delta_z^2.
 * frac_bits = min(40, 62 - ceil_log2(U + 1) - ceil_log2(ceil(max_samples / E) + 1) - 2 log2(limit)), so that no word can overflow within
 * max_samples samples; U is the number of recorded units of the WHOLE System in that mode (on an unsharded plan: num_units): a sharded plan
 * records the units of its own shard, every shard scales alike, and the shards' tables add as integers to the unsharded table.  Past
 * max_samples a sample adds nothing, stores no origin and counts as dropped.  Integer adds commute: the table is the same bits for any
 * grid, block size, unit order or shard split.
 * What rewrites positions outside the steps.  vvhip_barostat_scale and vvhip_barostat_restore, with a recorder running, set origin_floor to
 * the current sample ordinal (one one-thread kernel in the stream): older origins are dead, the table is kept.  vvhip_checkpoint_load is
 * refused while a recorder runs.  Host uploads into the bound arrays (vvhip_memcpy_h2d into posq, a re-bind to other arrays) are NOT
 * detected: the next samples measure against origins of the positions that were there before; stop the recorder and start it again.
 * Recovery.  Neither the table nor the ring is idempotent under the repeat of failed steps -- an origin overwritten inside the failed
 * window is needed again by the repeat -- so the rider's recovery words are the WHOLE allocation: counts, floor, table and origin ring,
 * (4 + words) * 8 B + ring_bytes with ring_bytes = num_origins x 3 x stride x 8 B, stride = num_units rounded up to 16. */
#define VVHIP_MSD_PARTICLES 0
#define VVHIP_MSD_MOLECULES 1
typedef struct {
    int32_t interval;               /* a sample after every step whose count is a multiple of it */
    int32_t num_lags;               /* 1 .. 4096: row l is the lag of (l + 1) * interval steps */
    int32_t origin_every;           /* E, 1 .. num_lags: every E-th sample is stored as an origin */
    int32_t mode;                   /* VVHIP_MSD_PARTICLES, VVHIP_MSD_MOLECULES */
    int32_t num_groups;             /* 1 .. 16 */
    int32_t reserved;               /* 0 */
    const signed char* group;       /* [num_atoms] the group of every particle of the System, -1: not recorded; NULL: everything in group 0 */
    int64_t max_samples;            /* >= 1 */
    double limit;                   /* nm: a displacement component at or beyond it is out of range; rounded up to a power of two; 0: 64 */
} vvhip_msd_desc;
typedef struct {
    int64_t samples;                /* samples taken since the start or the last reset (at most max_samples): the next sample's ordinal */
    int64_t dropped;                /* samples that were due past max_samples: nothing was added or stored for them */
    int64_t out_of_range;           /* unit-pairs left out of all four words */
    int64_t origin_floor;           /* origins with an ordinal below it are dead */
} vvhip_msd_counts;
typedef struct {
    int32_t active, interval, num_lags, origin_every, mode, num_groups;
    int32_t num_units;              /* units this plan records (particles: group >= 0 within [shard_begin, shard_end)) */
    int32_t num_origins;            /* ceil(num_lags / origin_every) */
    int32_t frac_bits, reserved;    /* value = word * 2^-frac_bits (pairs: the word itself) */
    int64_t max_samples;
    int64_t words;                  /* num_groups * num_lags * 4 */
    int64_t ring_bytes;             /* num_origins * 3 * stride * 8 */
    int64_t start_step;             /* the plan's step count at vvhip_msd_start */
    double limit;                   /* as applied */
} vvhip_msd_layout;
/* Starts (or restarts, dropping what was accumulated) a recorder; synchronises and drops the captured graphs.  Refused, in this order:
 * interval < 1, num_lags outside 1 .. 4096, origin_every outside 1 .. num_lags, an unknown mode, num_groups outside 1 .. 16, max_samples
 * < 1, a limit that is negative or not finite, a group entry outside -1 .. num_groups - 1 (VVHIP_ERR_INVALID naming the argument); in
 * molecule mode a molecule whose massive particles lie in different groups (VVHIP_ERR_INVALID naming it); frac_bits below 8; num_origins
 * above 1024 (VVHIP_ERR_INVALID); in molecule mode a shard that cuts a molecule (VVHIP_ERR_UNSUPPORTED); an unbound plan; inside a graph
 * capture (VVHIP_ERR_INVALID); an allocation that fails (VVHIP_ERR_HIP, with the byte count).  A description that passes the checks in
 * front of "an unbound plan" is kept even where the start is then refused (active = 0): vvhip_msd_info answers for it, for sizing. */
int vvhip_msd_start(vvhip_plan* plan, const vvhip_msd_desc* desc);
/* Synchronises and copies the counts (out may be NULL) and the table's `words` words (words_out may be NULL with capacity_words = 0; a
 * capacity below the table's size is VVHIP_ERR_INVALID).  reset != 0 zeroes counts, floor and table and restarts the ordinal at 0 with no
 * live origin: the step schedule continues without gap or repeat. */
int vvhip_msd_read(vvhip_plan* plan, int64_t* words_out, int64_t capacity_words, vvhip_msd_counts* out, int32_t reset);
/* Stops the recorder: no more samples are enqueued, table and ring are released, the description is forgotten; synchronises and drops the
 * captured graphs. */
int vvhip_msd_stop(vvhip_plan* plan);
/* The recorder as described (zeros with active = 0 if none was); host only, works on an unbound plan. */
int vvhip_msd_info(const vvhip_plan* plan, vvhip_msd_layout* out);
/* ---------------------------------------------------------------- radial distribution functions accumulated on the device
 * The pair structure g(r) between chosen sites (cation - anion, cation - cation, ion - electrode atom): the first thing plotted from a
 * bulk or slab trajectory, and the one analysis a host cannot afford during a run: a pair histogram is O(N_a N_b) per sample, about 1 s
 * for 3 000 x 3 000 sites in NumPy, against 24 B per particle and sample through the frame ring.  An accumulating histogram is a few KB
 * however long the run.  After every full step whose count is a multiple of `interval` -- counted exactly as for the series, the frames,
 * the profiles and the MSD, by the same entry points (the split per-KernelImpl entry points take none); a sample "after step k" is
 * enqueued behind that step's MSD sample -- the step entry point enqueues three kernels (csrc/vv_dev_rdf.inc): a gather of the sites'
 * float64 positions into a planar scratch, the pair kernel, and a one-thread kernel that counts the sample: no memset, no host work.
 * Inside a captured graph all three are graph nodes and the steps that take a sample are part of the graph-cache key.  The recorder reads
 * posq and posqCorrection and writes its own words and scratch, nothing else; a plan that never starts one launches what it launched
 * before and allocates nothing.
 * Sites.  The particles with group[i] >= 0, each in the one group it names; `group` covers the whole System, NULL puts every particle
 * into group 0; num_groups is 1 .. 16.
 * Classes.  num_classes (1 .. 32) unordered pairs of groups, classes[c] = {ga, gb}, both in [0, num_groups).  A class with ga != gb counts
 * every pair (i in ga, j in gb); a class with ga == gb counts every unordered pair {i, j} of the group once and no particle with itself.
 * With exclude_same_molecule != 0 pairs whose particles have equal vvhip_system_desc.mol_id are left out of every class (counted nowhere).
 * Position.  X_i in float64, exactly as a float64 frame defines it: (double) posq + (double) posqCorrection in mixed precision, (double)
 * posq otherwise; positions are stored unwrapped, in any periodic image.
 * Arithmetic.  All float64, no contraction.  Per axis a = x, y, z, with L the plan's box when the sample is enqueued and inv_L_a =
 * 1.0 / L_a formed once per sample:
 *     d = X_i,a - X_j,a;   n = rint(d * inv_L_a)  (round-half-even);   d = d - L_a * n
 * and then  r2 = (dx * dx + dy * dy) + dz * dz.  Every operation is odd or even in d, so a pair gives the same r2 in either orientation.
 * Bins.  Uniform in r: dr = r_max / nbins in float64 and edges e(k) = ((double) k * dr) * ((double) k * dr), k = 0 .. nbins.  A pair adds
 * the integer 1 to the bin b of its class with  e(b) <= r2 < e(b + 1),  0 <= b < nbins (where edges coincide: the largest such b); a pair
 * with r2 >= e(nbins) adds nothing; a pair whose r2 is NaN adds 1 to `invalid` and to no bin.  The comparisons define the bin, not a
 * square root; the host's views (vvhip_rdf_layout.dr, Python's Rdf.edges) use the same e.  nbins is 1 .. 8192.
 * Table: int64 table[num_classes][nbins].  Integer adds commute: the table is the same bits for any grid, tile shape or order.
 * Range.  r_max must be finite, > 0 and <= min(Lx, Ly, Lz) / 2 of the plan's box at the start (one image per pair).  A sample that is
 * enqueued while the plan's box no longer satisfies this (vvhip_set_box, the barostat's moves) adds nothing and counts as dropped; back in
 * range the samples count again.  The box is a kernel argument: what changes it drops the captured graphs.
 * Counts.  samples; dropped (due past max_samples, or in a box too small for r_max); invalid; and inv_volume_sum, float64: every counted
 * sample adds, in sample order,  s = s + 1.0 / ((Lx * Ly) * Lz)  -- sequential, so reproducible; under a barostat the normalisation of
 * g(r) needs this sum:  g_c(b) = table[c][b] / (P_c * shell(b) * inv_volume_sum),  P_c = pairs_per_sample[c] = N_a N_b, or N_a (N_a - 1)
 * / 2 for ga == gb (exclusion does not lower it), shell(b) = 4 pi / 3 (e(b + 1)^(3/2) - e(b)^(3/2)).
 * Overflow.  Refused at the start where the largest P_c times max_samples reaches 2^62.
 * Sharded plans.  A shard holds its own particles' arrays only, so pairs across shards exist on no device: a plan with a real shard is
 * refused (VVHIP_ERR_UNSUPPORTED) rather than given a partial histogram.
 * Recovery.  An accumulating table is not idempotent under the repeat of failed steps, so the rider's recovery words are the whole
 * allocation, counts and table, (4 + words) * 8 B; the scratch is rewritten by every sample and is not saved.  vvhip_checkpoint_load is
 * refused while a recorder runs, a re-bind drops the captured graphs, as for a profile recorder. */
typedef struct {
    int32_t interval;               /* a sample after every step whose count is a multiple of it */
    int32_t nbins;                  /* 1 .. 8192 */
    int32_t num_groups;             /* 1 .. 16 */
    int32_t num_classes;            /* 1 .. 32 */
    int32_t exclude_same_molecule;  /* != 0: pairs inside one molecule (mol_id) are left out */
    int32_t reserved;               /* 0 */
    const signed char* group;       /* [num_atoms] the group of every particle of the System, -1: no site; NULL: everything in group 0 */
    const int32_t* classes;         /* [num_classes][2] the groups ga, gb of every class */
    int64_t max_samples;            /* >= 1 */
    double r_max;                   /* nm */
} vvhip_rdf_desc;
typedef struct {
    int64_t samples;                /* samples counted since the start or the last reset (at most max_samples) */
    int64_t dropped;                /* samples that were due past max_samples or in a box with min(L) / 2 < r_max: nothing was added */
    int64_t invalid;                /* pairs whose r2 was NaN */
    double inv_volume_sum;          /* the counted samples' 1 / V, summed in sample order */
} vvhip_rdf_counts;
typedef struct {
    int32_t active, interval, nbins, num_groups, num_classes, exclude_same_molecule;
    int32_t tile;                   /* sites per tile of the pair kernel (a site count of tile + 1 is the first with a second tile) */
    int32_t num_items;              /* blocks of the pair kernel per sample */
    int32_t num_sites[16];          /* per group */
    int32_t classes[32][2];
    int64_t pairs_per_sample[32];   /* per class: N_a N_b, or N_a (N_a - 1) / 2 */
    int64_t max_samples;
    int64_t words;                  /* num_classes * nbins */
    int64_t scratch_bytes;          /* the gather's planes: 3 x stride x 8 B, stride = the sites rounded up to 16 */
    int64_t start_step;             /* the plan's step count at vvhip_rdf_start */
    double r_max, dr;               /* dr = r_max / nbins */
} vvhip_rdf_layout;
/* Starts (or restarts, dropping what was accumulated) a recorder; synchronises and drops the captured graphs.  Refused, in this order: a
 * null description, interval < 1, r_max not finite or <= 0, nbins outside 1 .. 8192, num_groups outside 1 .. 16, num_classes outside 1 ..
 * 32, classes NULL, max_samples < 1, a group entry outside -1 .. num_groups - 1, a class entry outside 0 .. num_groups - 1
 * (VVHIP_ERR_INVALID naming the argument); the largest class's pairs per sample times max_samples at or above 2^62; r_max above half the
 * shortest edge of the plan's box (VVHIP_ERR_INVALID); a sharded plan (VVHIP_ERR_UNSUPPORTED); an unbound plan; inside a graph capture
 * (VVHIP_ERR_INVALID); an allocation that fails (VVHIP_ERR_HIP, with the byte count).  A description that passes the checks in front of
 * "an unbound plan" is kept even where the start is then refused (active = 0): vvhip_rdf_info answers for it, for sizing. */
int vvhip_rdf_start(vvhip_plan* plan, const vvhip_rdf_desc* desc);
/* Enqueues one sample now, behind what is queued, whatever the schedule says; it counts as a sample like a scheduled one (a host that
 * analyses a configuration it has uploaded).  VVHIP_ERR_INVALID without a running recorder or inside a graph capture. */
int vvhip_rdf_sample(vvhip_plan* plan);
/* Synchronises and copies the counts (out may be NULL) and the table's `words` words (words_out may be NULL with capacity_words = 0; a
 * capacity below the table's size is VVHIP_ERR_INVALID).  reset != 0 zeroes counts and table: the step schedule continues without gap or
 * repeat. */
int vvhip_rdf_read(vvhip_plan* plan, int64_t* words_out, int64_t capacity_words, vvhip_rdf_counts* out, int32_t reset);
/* Stops the recorder: no more samples are enqueued, table and scratch are released, the description is forgotten; synchronises and drops
 * the captured graphs. */
int vvhip_rdf_stop(vvhip_plan* plan);
/* The recorder as described (zeros with active = 0 if none was); host only, works on an unbound plan. */
int vvhip_rdf_info(const vvhip_plan* plan, vvhip_rdf_layout* out);
/* ---------------------------------------------------------------- collective current correlations accumulated on the device
 * What the ionic conductivity needs: the Einstein-Helfand slope of the collective translational dipole M(t) = sum q_i r_i, or the Green-Kubo
 * integral of the charge current J(t) = sum q_i v_i, both split into cation-cation, anion-anion and cation-anion parts.  The MSD table cannot
 * give it: a product of sums is not a sum of per-particle terms, the cross terms between different ions are missing there.  A stand-alone
 * host gets it from float64 frames, 48 B per particle and sample, O(samples^2 N) work, the frame ring's capacity bounding the statistics; the
 * collective quantity is a handful of 3-vectors per sample, and a collective property has ONE value per time origin, so it needs far more
 * origins than the MSD.  After every full step whose count is a multiple of `interval` -- counted exactly as for the other riders, by the
 * same entry points; a sample "after step k" is enqueued behind that step's RDF sample -- the step entry point enqueues three kernels
 * (csrc/vv_dev_current.inc): the reduce, the correlate and the advance.  No memset, no host work; inside a captured graph they are part of
 * the graph and the steps that take a sample are part of the graph-cache key.  The recorder reads posq, posqCorrection and velm and writes
 * its own words, nothing else; a plan that never starts one launches what it launched before and allocates nothing.
 * Inputs.  weight[num_atoms] (float64, required, read at the start: later changes of posq.w are not followed; the charges q_i, or
 * Q_m m_i / M_m for the molecules' centres of mass: then sum w_i X_i = sum_m Q_m COM_m, the translational dipole without the intramolecular
 * and Drude part).  group[num_atoms]: -1 is not recorded, NULL: everything in group 0; G = num_groups, 1 .. 8.
 * Per-sample sums, as integers.  X_i = (double) posq + (double) posqCorrection in mixed precision, (double) posq otherwise, positions
 * unwrapped, exactly as a float64 frame defines it; v_i = (double) velm.xyz.  For component a
 *     p_ia = llrint((w_i * X_ia) * 2^Fp),   u_ia = llrint((w_i * v_ia) * 2^Fv)      (float64 without contraction, round-half-even)
 *     P_g,a = sum_{i in g} p_ia,            U_g,a = sum_{i in g} u_ia                (int64)
 * W (weight_bound) is the smallest power of two above max |w_i| over the recorded particles of the WHOLE System (1 if all are 0), N their
 * number, and Fp = min(40, 62 - ceil_log2(N + 1) - log2 W - log2 limit_position), Fv likewise with limit_velocity: no sum can overflow.
 * The limits (nm, nm/ps; 0: the default of 64) are rounded up to a power of two.  A recorded particle with any X_ia or v_ia that is NaN
 * or at or beyond its limit is out of range: it adds 1 to out_of_range and makes the sample INVALID.  An invalid sample adds nothing to any
 * row, is not usable as an origin, and adds 1 to invalid_samples; the ordinal still advances.
 * Schedule.  Sample ordinal j = 0, 1, ... counts the due steps since the start or the last reset, valid or not.  Every sample whose ordinal
 * is a multiple of origin_every (E) is also stored as an origin, in slot (j / E) mod num_origins of a device ring of the sums, int64
 * ring[num_origins][G][6] (P_x P_y P_z U_x U_y U_z), with a word per slot that says which sample the slot holds, or -1;
 * num_origins = ceil(num_lags / E) is derived.
 * Table: int64 words[num_lags + 1][row_words], row_words = 1 + 3 (ND + NC): word 0 of a row is an integer count, then disp[ND][3], then
 * cur[NC][3], the bits of doubles.  ND = G (G + 1) / 2 displacement classes c(g, h), g <= h, in the order (0,0) (0,1) .. (0,G-1) (1,1) ..;
 * NC = G^2 current classes (g, h) at index g G + h.  ROW l IS THE LAG OF l * interval STEPS AND ROW 0 IS THE ZERO LAG (unlike the MSD:
 * row 0 holds the t = 0 term of Green-Kubo; its disp words stay 0).  At a valid sample j, all in float64 without contraction:
 *     row 0:   cur[0][g][h][a] += J_g,a(j) * J_h,a(j)   with J = (double) U * 2^-Fv;   count[0] += 1
 *     rows l = 1 .. num_lags, where the origin o = j - l is usable -- o is a multiple of E, origin_floor <= o, and the slot still holds
 *     sample o and it was valid:
 *              disp[l][c(g,h)][a] += dP_g,a * dP_h,a     with dP_g,a = (double) (P_g,a(j) - P_g,a(o)) * 2^-Fp, the subtraction in int64
 *              cur[l][g][h][a]    += J_g,a(o) * J_h,a(j)  (the origin is the first index);   count[l] += 1
 * A cell receives at most one term per sample, so its value is the sequential float64 sum in ascending sample order, and that order is
 * part of the definition: one thread owns a cell for a sample, there are no float atomics, and the bits are the same for any grid, block
 * size or particle order.  Accumulation comes first, the origin store second: when num_origins * E == num_lags the slot that is
 * overwritten at sample j was read in the same sample.  Past max_samples a sample adds nothing, stores no origin and counts as dropped.
 * inv_volume_sum is the sequential float64 sum of 1 / ((Lx * Ly) * Lz), formed on the host, over the valid samples.
 * What rewrites positions outside the steps.  vvhip_barostat_scale and vvhip_barostat_restore, with a recorder running, set origin_floor
 * to the current ordinal: older origins are dead, the table is kept.  vvhip_checkpoint_load is refused while a recorder runs.  Host uploads
 * into the bound arrays are NOT detected, as for the MSD.
 * Recovery.  Neither the table nor the ring is idempotent under the repeat of failed steps, so the rider's recovery words are the WHOLE
 * allocation: head, sums, table, ring and the slots' words. */
typedef struct {
    int32_t interval;               /* a sample after every step whose count is a multiple of it */
    int32_t num_lags;               /* 1 .. 4096: row l is the lag of l * interval steps, row 0 the zero lag */
    int32_t origin_every;           /* E, 1 .. num_lags: every E-th sample is stored as an origin */
    int32_t num_groups;             /* G, 1 .. 8 */
    const double* weight;           /* [num_atoms] required, finite */
    const signed char* group;       /* [num_atoms] the group of every particle of the System, -1: not recorded; NULL: everything in group 0 */
    int64_t max_samples;            /* >= 1 */
    double limit_position;          /* nm: a position component at or beyond it is out of range; rounded up to a power of two; 0: 64 */
    double limit_velocity;          /* nm/ps, likewise */
} vvhip_current_desc;
typedef struct {
    int64_t samples;                /* samples taken since the start or the last reset, valid or not (at most max_samples): the next ordinal */
    int64_t dropped;                /* samples that were due past max_samples: nothing was added or stored for them */
    int64_t out_of_range;           /* recorded particles found out of range, over all samples taken */
    int64_t invalid_samples;        /* samples taken with at least one of them: count[0] = samples - invalid_samples */
    int64_t origin_floor;           /* origins with an ordinal below it are dead */
    double inv_volume_sum;          /* the valid samples' 1 / V, summed in sample order */
} vvhip_current_counts;
typedef struct {
    int32_t active, interval, num_lags, origin_every, num_groups;
    int32_t num_particles;          /* recorded particles (group >= 0) */
    int32_t num_origins;            /* ceil(num_lags / origin_every) */
    int32_t num_disp_classes;       /* ND = G (G + 1) / 2 */
    int32_t num_cur_classes;        /* NC = G^2 */
    int32_t row_words;              /* 1 + 3 (ND + NC) */
    int32_t frac_bits_position;     /* Fp */
    int32_t frac_bits_velocity;     /* Fv */
    int64_t max_samples;
    int64_t words;                  /* (num_lags + 1) * row_words */
    int64_t ring_bytes;             /* num_origins * (G * 6 + 1) * 8: the origins' sums and the slots' words */
    int64_t start_step;             /* the plan's step count at vvhip_current_start */
    double limit_position, limit_velocity;      /* as applied */
    double weight_bound;            /* W */
} vvhip_current_layout;
/* Starts (or restarts, dropping what was accumulated) a recorder; synchronises and drops the captured graphs.  Refused, in this order: a
 * null description, interval < 1, num_lags outside 1 .. 4096, origin_every outside 1 .. num_lags, num_groups outside 1 .. 8, max_samples
 * < 1, a limit_position, then a limit_velocity that is negative or not finite, weight NULL, a group entry outside -1 .. num_groups - 1, a
 * weight that is not finite (VVHIP_ERR_INVALID naming the argument); Fp, then Fv below 8 (VVHIP_ERR_INVALID); a sharded plan
 * (VVHIP_ERR_UNSUPPORTED: the shards' sums would have to be combined before the products are formed); an unbound plan; inside a graph
 * capture (VVHIP_ERR_INVALID); an allocation that fails (VVHIP_ERR_HIP, with the byte count).  A description that passes the checks in
 * front of "an unbound plan" is kept even where the start is then refused (active = 0): vvhip_current_info answers for it, for sizing. */
int vvhip_current_start(vvhip_plan* plan, const vvhip_current_desc* desc);
/* Synchronises and copies the counts (out may be NULL) and the table's `words` words (words_out may be NULL with capacity_words = 0; a
 * capacity below the table's size is VVHIP_ERR_INVALID).  reset != 0 zeroes counts, floor and table and restarts the ordinal at 0 with no
 * live origin: the step schedule continues without gap or repeat. */
int vvhip_current_read(vvhip_plan* plan, int64_t* words_out, int64_t capacity_words, vvhip_current_counts* out, int32_t reset);
/* Stops the recorder: no more samples are enqueued, table and ring are released, the description is forgotten; synchronises and drops the
 * captured graphs. */
int vvhip_current_stop(vvhip_plan* plan);
/* The recorder as described (zeros with active = 0 if none was); host only, works on an unbound plan. */
int vvhip_current_info(const vvhip_plan* plan, vvhip_current_layout* out);
/* ---------------------------------------------------------------- density modes accumulated on the device: S(k) and F(k, t)
 * The scattering side of the observables: the partial and charge structure factors S_gh(k) = <rho_g*(k) rho_h(k)> / sqrt(N_g N_h), whose
 * prepeak is the fingerprint of an ionic liquid, and the coherent intermediate scattering function F_gh(k, t) = <rho_g*(k, 0) rho_h(k, t)> /
 * sqrt(N_g N_h), with rho_g(k) = sum_{i in g} w_i exp(i k . X_i).  Neither follows from the other recorders: the Fourier transform of a g(r)
 * cut at L / 2 is useless below k ~ 4 pi / L, where the prepeak sits, and F(k, t) is a product of collective sums at two times, which is not
 * a sum of per-particle terms.  A stand-alone host gets it from float64 frames, 24 B per particle and sample, then N K sines and cosines.
 * After every full step whose count is a multiple of `interval` -- counted as for the other riders; a sample "after step k" is enqueued
 * behind that step's current sample -- the step entry point enqueues four kernels (csrc/vv_dev_modes.inc): the gather, the mode kernel,
 * the correlate and the advance.  No memset, no host work; inside a captured graph they are part of the graph and the steps that take a
 * sample are part of the graph-cache key.  The recorder reads posq and posqCorrection and writes its own words and scratch, nothing else;
 * a plan that never starts one launches what it launched before and allocates nothing.
 * Inputs.  weight[num_atoms] (float64, required, finite, read at the start: 1 gives number densities, the charges the charge structure
 * factor).  group[num_atoms]: -1 is not recorded, NULL: everything in group 0; G = num_groups, 1 .. 8.  modes[K][3] (int32, K = num_modes,
 * 1 .. 4096, every component in -4095 .. 4095): mode k is the wave vector 2 pi (n_x / L_x, n_y / L_y, n_z / L_z) of the box AS IT STANDS AT
 * THE SAMPLE, commensurate with any orthorhombic box, also after a barostat move.  (0,0,0), duplicates and +-pairs are the caller's business.
 * Position to integer turns.  X_i = (double) posq + (double) posqCorrection in mixed precision, (double) posq otherwise, positions
 * unwrapped, as for the other recorders.  Per axis a, with inv_L_a = 1.0 / box[a] formed on the host at enqueue:
 *     t = X_a * inv_L_a,   u = t - floor(t),   T_a = (uint64) floor(u * 2^32) & 0xFFFFFFFF
 * u = 1.0 (from t = -1e-20) becomes 2^32 and wraps to 0, which is the right phase: no clamp.
 * Phase.  phi = (n_x T_x + n_y T_y + n_z T_z) mod 2^32 in two's-complement 32-bit arithmetic: the multiple of a turn drops out exactly and
 * there is no floating-point argument reduction.
 * Phasor (csrc/vv_layout.h: phasor_turns).  t = (phi + 2^29) mod 2^32, quadrant q = t >> 30, r = (int) (t & (2^30 - 1)) - 2^29,
 * x = (double) r * C with C the double nearest to pi 2^-31 (|x| <= pi / 4), z = x * x,
 *     sn = x + (x * z) * PS(z),   cs = (1.0 - 0.5 * z) + (z * z) * PC(z)
 * with PS = S1 + z (S2 + z (.. S6)) and PC = C1 + z (C2 + z (.. C6)) the six-term fdlibm k_sin / k_cos polynomials, by Horner from the
 * highest coefficient, every * and + rounded on its own, NO fma; (cos, sin) = (cs, sn), (-sn, cs), (-cs, -sn), (sn, -cs) for q = 0 .. 3.
 * Only correctly rounded + - * occur, so NumPy states it bit for bit (tests/modes_reference.py); the absolute error is below 2^-51.
 * Terms and sums.  W (weight_bound) is the smallest power of two above max |w_i| over the recorded particles (1 if all are 0) and
 * F = 30 - log2 W, so that every term fits an int32:
 *     a_ik = (int32) rint((w_i * c_ik) * 2^F),   b_ik = (int32) rint((w_i * s_ik) * 2^F)          (float64, round-half-even)
 *     A_g(k) = sum_{i in g} a_ik,                B_g(k) = sum_{i in g} b_ik                        (int64)
 * Integer adds commute: the sums are the same bits for any grid, block size or particle order.
 * Invalid samples, as for the currents: a recorded particle with a position component that is NaN or at or beyond limit_position (nm;
 * 0: the default of 64; rounded up to a power of two) is out of range: it adds 1 to out_of_range and makes the sample INVALID.  An invalid
 * sample adds nothing to any row, is not usable as an origin, and adds 1 to invalid_samples; the ordinal still advances.
 * Schedule, ring and table, as for vvhip_current_*.  Sample ordinal j = 0, 1, ... counts the due steps since the start or the last reset,
 * valid or not.  num_lags = 0 .. 4096; 0 means the static S(k) only: then there is no ring and num_origins = 0.  Otherwise every sample
 * whose ordinal is a multiple of origin_every (E) is also stored as an origin, in slot (j / E) mod num_origins of a device ring
 * int64 ring[num_origins][G][K][2] (A, B), with a word per slot that says which sample it holds, or -1; num_origins = ceil(num_lags / E).
 * Table: int64 words[num_lags + 1][row_words], row_words = 1 + G^2 K: word 0 of a row is an integer count, then cell[g][h][k], the bits of
 * doubles.  With a = (double) A * 2^-F, b likewise, at a valid sample j, all in float64 without contraction:
 *     row 0:   cell[g][h][k] += a_g(j) * a_h(j) + b_g(j) * b_h(j);   count[0] += 1
 *     rows l = 1 .. num_lags, where the origin o = j - l is usable -- o is a multiple of E, origin_floor <= o, and the slot still holds
 *     sample o and it was valid:
 *              cell[g][h][k] += a_g(o) * a_h(j) + b_g(o) * b_h(j)    (the origin is the first index);   count[l] += 1
 * This is Re rho_g*(o) rho_h(j).  The imaginary part averages to zero in equilibrium and is NOT kept.  A cell receives at most one term
 * per sample, so its value is the sequential float64 sum in ascending sample order, and that order is part of the definition: one thread
 * owns a cell for a sample, there are no float atomics.  Accumulation comes first, the origin store second.  Past max_samples a sample adds
 * nothing, stores no origin and counts as dropped.  box_sum[a] is the sequential float64 sum of L_a over the valid samples: the host needs
 * it for |k| under a barostat.
 * What rewrites positions outside the steps.  vvhip_barostat_scale and vvhip_barostat_restore, with a recorder running, set origin_floor
 * to the current ordinal: older origins are dead, the table is kept; later samples use the new box's wave vectors.  vvhip_checkpoint_load is
 * refused while a recorder runs.  Host uploads into the bound arrays are NOT detected.
 * Recovery.  The rider's recovery words are the WHOLE allocation: head, sums, table, ring and the slots' words.  The turns are scratch,
 * rewritten by every sample, and not saved. */
typedef struct {
    int32_t interval;               /* a sample after every step whose count is a multiple of it */
    int32_t num_lags;               /* 0 .. 4096: row l is the lag of l * interval steps, row 0 the zero lag; 0: S(k) only, no ring */
    int32_t origin_every;           /* E, 1 .. max(1, num_lags): every E-th sample is stored as an origin */
    int32_t num_groups;             /* G, 1 .. 8 */
    int32_t num_modes;              /* K, 1 .. 4096 */
    const double* weight;           /* [num_atoms] required, finite */
    const signed char* group;       /* [num_atoms] the group of every particle of the System, -1: not recorded; NULL: everything in group 0 */
    const int32_t* modes;           /* [num_modes][3] required, every component in -4095 .. 4095 */
    int64_t max_samples;            /* >= 1 */
    double limit_position;          /* nm: a position component at or beyond it is out of range; rounded up to a power of two; 0: 64 */
} vvhip_modes_desc;
typedef struct {
    int64_t samples;                /* samples taken since the start or the last reset, valid or not (at most max_samples): the next ordinal */
    int64_t dropped;                /* samples that were due past max_samples: nothing was added or stored for them */
    int64_t out_of_range;           /* recorded particles found out of range, over all samples taken */
    int64_t invalid_samples;        /* samples taken with at least one of them: count[0] = samples - invalid_samples */
    int64_t origin_floor;           /* origins with an ordinal below it are dead */
    double box_sum[3];              /* the valid samples' L_x, L_y, L_z, summed in sample order */
} vvhip_modes_counts;
typedef struct {
    int32_t active, interval, num_lags, origin_every, num_groups, num_modes;
    int32_t num_particles;          /* recorded particles (group >= 0) */
    int32_t num_origins;            /* ceil(num_lags / origin_every); 0 with num_lags = 0 */
    int32_t row_words;              /* 1 + G^2 K */
    int32_t frac_bits;              /* F */
    int32_t group_sites[8];         /* N_g: the recorded particles of every group */
    int32_t num_items;              /* the mode kernel's work items (blocks) ... */
    int32_t sites_per_thread, k_tile, block_threads;      /* ... and the shape they were built for */
    int64_t max_samples;
    int64_t words;                  /* (num_lags + 1) * row_words */
    int64_t ring_bytes;             /* num_origins * (G * K * 2 + 1) * 8: the origins' sums and the slots' words */
    int64_t scratch_bytes;          /* the turns: 3 planes of uint32, num_particles rounded up to 16 each */
    int64_t start_step;             /* the plan's step count at vvhip_modes_start */
    double limit_position;          /* as applied */
    double weight_bound;            /* W */
} vvhip_modes_layout;
/* Starts (or restarts, dropping what was accumulated) a recorder; synchronises and drops the captured graphs.  Refused, in this order: a
 * null description, interval < 1, num_lags outside 0 .. 4096, origin_every outside 1 .. max(1, num_lags), num_groups outside 1 .. 8,
 * num_modes outside 1 .. 4096, max_samples < 1, a limit_position that is negative or not finite, weight NULL, modes NULL, a mode component
 * outside -4095 .. 4095, a group entry outside -1 .. num_groups - 1, a weight that is not finite (VVHIP_ERR_INVALID naming the argument);
 * F below 8, 31 + ceil_log2(N + 1) above 62 for N recorded particles, a table above 2^26 words (VVHIP_ERR_INVALID); a sharded plan
 * (VVHIP_ERR_UNSUPPORTED: the shards' sums would have to be combined before the products are formed); an unbound plan; inside a graph
 * capture (VVHIP_ERR_INVALID); an allocation that fails (VVHIP_ERR_HIP, with the byte count).  A description that passes the checks in
 * front of "an unbound plan" is kept even where the start is then refused (active = 0): vvhip_modes_info answers for it, for sizing. */
int vvhip_modes_start(vvhip_plan* plan, const vvhip_modes_desc* desc);
/* Synchronises and copies the counts (out may be NULL) and the table's `words` words (words_out may be NULL with capacity_words = 0; a
 * capacity below the table's size is VVHIP_ERR_INVALID).  reset != 0 zeroes counts, floor and table and restarts the ordinal at 0 with no
 * live origin: the step schedule continues without gap or repeat. */
int vvhip_modes_read(vvhip_plan* plan, int64_t* words_out, int64_t capacity_words, vvhip_modes_counts* out, int32_t reset);
/* Stops the recorder: no more samples are enqueued, table, ring and scratch are released, the description is forgotten; synchronises and
 * drops the captured graphs. */
int vvhip_modes_stop(vvhip_plan* plan);
/* The recorder as described (zeros with active = 0 if none was); host only, works on an unbound plan. */
int vvhip_modes_info(const vvhip_plan* plan, vvhip_modes_layout* out);
/* ---------------------------------------------------------------- contact lifetime correlations accumulated on the device
 * How long ion pairs and ion cages live: which anion sits in which cation's first shell, and for how long -- the intermittent and the
 * continuous contact correlation functions that explain the transport coefficients.  The RDF says how many neighbours there are, not which;
 * from frames every sample is an all-pairs pass and a time-correlation function wants hundreds of origins.  On the device a sample is a
 * bit matrix and a lag is a popcount of an AND.  After every full step whose count is a multiple of `interval` -- counted exactly as for
 * the other riders, by the same entry points; a sample "after step k" is enqueued behind that step's density-mode sample -- the step entry
 * point enqueues four kernels (csrc/vv_dev_contacts.inc): a gather of the sites' float64 positions, the mask kernel that builds the sample's
 * bit matrices, the correlate kernel, and a one-wave kernel that counts the sample: no memset, no host work.  Inside a captured graph all
 * four are graph nodes and the steps that take a sample are part of the graph-cache key.  The recorder reads posq and posqCorrection and
 * writes its own words and scratch, nothing else; a plan that never starts one launches what it launched before and allocates nothing.
 * Sites.  As for the RDF: the particles with group[i] >= 0, each in the one group it names; `group` covers the whole System, NULL puts
 * every particle into group 0; num_groups is 1 .. 16.
 * Classes.  num_classes (1 .. 8) ORDERED pairs of groups, classes[c] = {ga, gb}, each with its own cutoff r_cut[c].  The rows of class c are
 * the sites of ga (N_a of them), the columns the sites of gb (N_b), both in ascending particle index.  ga == gb is allowed: the diagonal (a
 * site with itself) is 0, and every unordered pair {i, j} appears twice, as (i, j) and as (j, i) -- every word of the table counts it
 * twice.  With exclude_same_molecule != 0 pairs whose particles have equal vvhip_system_desc.mol_id are 0 in every class.
 * Contact.  r2 is exactly the RDF's: positions in float64, (double) posq + (double) posqCorrection in mixed precision; per axis, with L the
 * plan's box when the sample is enqueued and inv_L_a = 1.0 / L_a,  d = X_i,a - X_j,a;  n = rint(d * inv_L_a);  d = d - L_a * n;  then
 * r2 = (dx * dx + dy * dy) + dz * dz, no contraction.  h_ij = 1 iff r2 < r_cut[c] * r_cut[c] (float64, the compare is strict: a pair AT the
 * cutoff is no contact).  A pair whose r2 is NaN has h = 0 and adds 1 to `invalid` (a cleared pair -- diagonal, same molecule -- adds nothing).
 * Per sample.  j = the 0-based ordinal of the counted samples, E = origin_every, R = num_origins = ceil(num_lags / E) slots, each with
 * origin[s], cont[s] (bit matrices of every class) and ord[s] (-1: empty).  In this order:
 *   1. h(j) is built for every class.
 *   2. If j mod E = 0, slot s = (j / E) mod R takes origin[s] = h(j), cont[s] = h(j), ord[s] = j.
 *   3. Every slot with ord[s] >= 0 and l = j - ord[s] < num_lags (the slot just stored included, at l = 0): cont[s] &= h(j), and for every
 *      class c the four integers  1,  popcount(origin[s]_c),  popcount(origin[s]_c & h(j)_c),  popcount(cont[s]_c)  are added to
 *      table[c][l][0 .. 3].  A slot with l >= num_lags adds nothing (R E > num_lags).
 *   4. samples += 1.
 * Table: int64 table[num_classes][num_lags][4].  Word 2 / word 1 is the intermittent correlation C(t) (the pair is in contact at 0 and at
 * t), word 3 / word 1 the continuous one S(t) (in contact at every sample from 0 to t), word 1 / (word 0 N_a) the mean number of contacts
 * per row site.  continuous = 0 keeps no cont ring: word 3 stays 0.  Integer adds commute: the table is the same bits for any work list.
 * Limits.  num_lags 1 .. 4096, origin_every 1 .. num_lags, R <= 1024.  r_cut[c] finite, > 0 and <= min(Lx, Ly, Lz) / 2 of the plan's box
 * at the start.  Refused where the largest N_a N_b times max_samples reaches 2^62, and where the recorder's whole allocation -- counts,
 * table, slot ordinals, both rings, the sample's matrix and the gather's planes: total_bytes of the layout -- is above
 * VVHIP_CONTACTS_MAX_BYTES = 2^32: the recovery snapshot copies it.  A matrix of class c has ceil(N_b / 64) words for each of N_a rounded
 * up to 64 rows; a ring holds R matrices.
 * Counts.  samples; dropped (due past max_samples, or enqueued while min(L) / 2 is below the largest cutoff: the host decides at enqueue,
 * as for the RDF; nothing is added and j does not move); invalid.
 * Barostat moves (vvhip_barostat_scale / _restore) raise NO origin floor: a contact set is a property of a configuration, not a
 * displacement from one, so the origins stored before a move stay valid.
 * Sharded plans are refused (VVHIP_ERR_UNSUPPORTED): the pairs across shards exist on no device.
 * Recovery.  The rider's recovery words are the whole allocation -- counts, table, ord and both rings (words_bytes of the layout):
 * neither the table nor the surviving contacts are idempotent under the repeat of failed steps, and the repeat needs the origins the
 * failed window overwrote, as for the MSD.  The sample's matrix and the planes are rewritten by every sample and are not saved.
 * vvhip_checkpoint_load is refused while a recorder runs; a re-bind drops the captured graphs. */
#define VVHIP_CONTACTS_MAX_BYTES (1ll << 32)
typedef struct {
    int32_t interval;               /* a sample after every step whose count is a multiple of it */
    int32_t num_lags;               /* 1 .. 4096 */
    int32_t origin_every;           /* 1 .. num_lags */
    int32_t num_groups;             /* 1 .. 16 */
    int32_t num_classes;            /* 1 .. 8 */
    int32_t exclude_same_molecule;  /* != 0: pairs inside one molecule (mol_id) are no contacts */
    int32_t continuous;             /* != 0: keep the surviving contacts (word 3) */
    int32_t reserved;               /* 0 */
    const signed char* group;       /* [num_atoms] the group of every particle of the System, -1: no site; NULL: everything in group 0 */
    const int32_t* classes;         /* [num_classes][2] the groups ga (rows), gb (columns) of every class */
    const double* r_cut;            /* [num_classes] nm */
    int64_t max_samples;            /* >= 1 */
} vvhip_contacts_desc;
typedef struct {
    int64_t samples;                /* samples counted since the start or the last reset (at most max_samples) */
    int64_t dropped;                /* samples that were due past max_samples or in a box with min(L) / 2 below the largest cutoff */
    int64_t invalid;                /* pairs whose r2 was NaN */
} vvhip_contacts_counts;
typedef struct {
    int32_t active, interval, num_lags, origin_every, num_groups, num_classes, exclude_same_molecule, continuous;
    int32_t num_origins;            /* R */
    int32_t rows_per_tile;          /* rows a block of the mask kernel stages (test hook "contacts_rows_per_tile") */
    int32_t words_per_item;         /* column words per work item of the mask kernel (test hook "contacts_words_per_item") */
    int32_t skip_zero_words;        /* the correlate kernel skips zero origin words (test hook "contacts_skip_zero") */
    int32_t num_mask_items, num_corr_items;      /* blocks of the mask kernel per sample; of the correlate kernel per sample and slot */
    int32_t num_sites[16];          /* per group */
    int32_t classes[8][2];
    int32_t rows[8], cols[8];       /* per class: N_a, N_b */
    int64_t class_words[8];         /* per class: ceil(N_b / 64) * (N_a rounded up to 64) */
    int64_t sample_words;           /* their sum: one matrix */
    int64_t max_samples;
    int64_t words;                  /* num_classes * num_lags * 4 */
    int64_t words_bytes;            /* counts, table, ord, rings */
    int64_t scratch_bytes;          /* the sample's matrix and the gather's planes */
    int64_t total_bytes;            /* both: what VVHIP_CONTACTS_MAX_BYTES bounds */
    int64_t start_step;             /* the plan's step count at vvhip_contacts_start */
    double r_cut[8];
} vvhip_contacts_layout;
/* Starts (or restarts, dropping what was accumulated) a recorder; synchronises and drops the captured graphs.  Refused, in this order: a
 * null description, interval < 1, num_lags outside 1 .. 4096, origin_every outside 1 .. num_lags, num_groups outside 1 .. 16, num_classes
 * outside 1 .. 8, classes NULL, r_cut NULL, max_samples < 1, a group entry outside -1 .. num_groups - 1, a class entry outside 0 ..
 * num_groups - 1, a cutoff that is not finite or <= 0 (VVHIP_ERR_INVALID naming the argument); num_origins above 1024; the largest class's
 * N_a N_b times max_samples at or above 2^62; total_bytes above VVHIP_CONTACTS_MAX_BYTES ("contacts: ... VVHIP_CONTACTS_MAX_BYTES"); a
 * cutoff above half the shortest edge of the plan's box (VVHIP_ERR_INVALID); a sharded plan (VVHIP_ERR_UNSUPPORTED); an unbound plan;
 * inside a graph capture (VVHIP_ERR_INVALID); an allocation that fails (VVHIP_ERR_HIP, with the byte count).  A description that passes
 * the checks in front of "an unbound plan" is kept even where the start is then refused (active = 0): vvhip_contacts_info answers for it. */
int vvhip_contacts_start(vvhip_plan* plan, const vvhip_contacts_desc* desc);
/* Enqueues one sample now, behind what is queued, whatever the schedule says; it counts as a sample like a scheduled one (a host that
 * analyses a configuration it has uploaded).  VVHIP_ERR_INVALID without a running recorder or inside a graph capture. */
int vvhip_contacts_sample(vvhip_plan* plan);
/* Synchronises and copies the counts (out may be NULL) and the table's `words` words (words_out may be NULL with capacity_words = 0; a
 * capacity below the table's size is VVHIP_ERR_INVALID).  reset != 0 zeroes counts and table, marks every slot empty and restarts j at 0:
 * the step schedule continues without gap or repeat. */
int vvhip_contacts_read(vvhip_plan* plan, int64_t* words_out, int64_t capacity_words, vvhip_contacts_counts* out, int32_t reset);
/* Stops the recorder: no more samples are enqueued, table, rings and scratch are released, the description is forgotten; synchronises and
 * drops the captured graphs. */
int vvhip_contacts_stop(vvhip_plan* plan);
/* The recorder as described (zeros with active = 0 if none was); host only, works on an unbound plan. */
int vvhip_contacts_info(const vvhip_plan* plan, vvhip_contacts_layout* out);
/* ---------------------------------------------------------------- velocity and orientation autocorrelations accumulated on the device
 * The autocorrelation of a per-unit vector a(t).  Of a velocity it is the Green-Kubo route to the self-diffusion coefficient -- the
 * cross-check of the MSD's slope -- and its cosine transform is the vibrational density of states, which shows where the Drude oscillators
 * sit relative to the thermostat's frequencies; velocity Verlet has the synchronous on-step velocities it wants.  Of a body-fixed unit vector
 * u it is C1(t) = <u(0).u(t)> and C2(t) = <P2(u(0).u(t))>, the rotational relaxation times.  Both want a short sampling interval over many
 * origins: from frames that is 24 - 32 B per particle every few steps and O(samples lags N) work on the host.  After every full step whose
 * count is a multiple of `interval` -- counted exactly as for the other riders, by the same entry points; a sample "after step k" is
 * enqueued behind that step's contact sample, last of the riders -- the step entry point enqueues one accumulating kernel
 * (csrc/vv_dev_acf.inc) and a one-thread kernel that advances the sample ordinal: two launches, no memset, no host work.  Inside a captured
 * graph both are part of the graph and the steps that take a sample are part of the graph-cache key.  The recorder reads velm (the velocity
 * modes) or posq and posqCorrection (orientation mode) and writes its own words, nothing else; a plan that never starts one launches what
 * it launched before and allocates nothing.
 * Units and their vector.
 *   VVHIP_ACF_VELOCITY_PARTICLES  every recorded particle is a unit; a = (double) velm.xyz, the bits a float64 velocity frame records at
 *                        the same step.
 *   VVHIP_ACF_VELOCITY_MOLECULES  a unit is a molecule of vvhip_system_desc.mol_id, restricted to its particles with mass > 0; a is the
 *                        velocity of its centre of mass in float64 without contraction:  s = 0; for i in ascending particle index:
 *                        s = s + m_i * v_i;  a = s / M,  M summed on the host in the same order: the MSD's definition with v for X, and
 *                        the MSD's rules: the group of a molecule is the group of its massive particles, mixed groups inside one molecule
 *                        are refused, a molecule with group -1 or without mass is not recorded, a shard that holds some but not all massive
 *                        particles of a molecule gives VVHIP_ERR_UNSUPPORTED.
 *   VVHIP_ACF_ORIENTATION  a unit is an ordered pair (head, tail) of particle indices of the System, pairs[2 u], pairs[2 u + 1], with
 *                        group[u] its group (one byte per PAIR, -1: not recorded).  Head and tail differ and lie in the same molecule.
 *                        Positions are stored unwrapped and molecules whole, so no minimum image is taken.  d = X_head - X_tail with X as
 *                        the MSD defines it,  n2 = (d_x d_x + d_y d_y) + d_z d_z,  a = u = d * y  with  y ~ n2^(-1/2)  from ONE sequence of
 *                        correctly rounded +, -, * and exact scalings by powers of two -- no sqrt, no rsqrt, no division, no fma -- so that
 *                        device and host give the same bits (csrc/vv_layout.h: acf_inverse_norm; tests/acf_reference.py in NumPy):
 *                        with ex the exponent of n2 and e = ex - (ex & 1), m = n2 2^-e in [1, 4);  y = 1.2929 - 0.2929 m  where m < 2,
 *                        else  y = 0.9142 - 0.10355 m;  four times  y = y * (1.5 - (0.5 * m) * (y * y));  then y = y * 2^(-e / 2).
 *                        | |u|^2 - 1 | <= 2^-49.  On a sharded plan both particles must be in the shard (so for shards on molecule
 *                        boundaries), else VVHIP_ERR_UNSUPPORTED.
 * Bad vectors.  In the velocity modes a vector with a component that is NaN or has |a_c| >= limit (nm/ps, rounded up to a power of two; 0
 * takes the default of 64); in orientation mode one whose n2 is NaN or outside [2^-40, 2^40) nm^2 (limit must be 0 there).  A bad vector is
 * stored in the ring as NaN; a pair with a bad vector at either end is left out of every word and adds 1 to out_of_range.
 * Schedule.  Sample ordinal j = 0, 1, ... counts the due steps since the start or the last reset.  Every sample whose ordinal is a multiple
 * of origin_every (E) is an origin, stored in slot (j / E) mod num_origins of a device ring; num_origins = ceil(num_lags / E) is derived,
 * at most 1024.  ROW l (0 <= l < num_lags) IS THE LAG OF l * interval STEPS: ROW 0 IS THE ZERO LAG (the MSD's row 0 is one interval).  At
 * sample j every origin o = k E with  origin_floor <= o <= j  and  j - o < num_lags  contributes to row j - o; the self term o = j comes
 * from the sample's own vector.  The slot a new origin overwrites held origin j - num_origins E <= j - num_lags, which no row can use.
 * Past max_samples a sample adds nothing, stores nothing and counts as dropped.
 * Terms.  p_c = a_c(o) * a_c(j) in float64, c = x, y, z, signed.  The words of a row: the pair count as the integer 1;
 * llrint(p_x * 2^frac_bits), llrint(p_y * 2^frac_bits), llrint(p_z * 2^frac_bits), round-half-even; in orientation mode a fifth,
 * llrint(cs * cs * 2^frac_bits) with cs = (p_x + p_y) + p_z, for P2.
 * Table: int64 table[num_groups][num_lags][row_words], row_words = 4 in the velocity modes, 5 in orientation mode.
 * frac_bits = min(40, 62 - ceil_log2(U + 1) - ceil_log2(ceil(max_samples / E) + 1) - 2 log2(limit)), log2(limit) = 0 in orientation mode,
 * so that no word can overflow within max_samples samples; U is the number of units the description records over the WHOLE System: a
 * sharded plan records the units of its own shard, every shard scales alike, and the shards' tables add as integers to the unsharded
 * table.  Integer adds commute: the table is the same bits for any grid, block size, unit order or shard split.
 * What rewrites the inputs outside the steps.  vvhip_set_velocities_to_temperature, with a velocity-mode recorder running, sets origin_floor
 * to the current sample ordinal (one one-thread kernel in the stream): older origins are dead, the table is kept; an orientation recorder
 * is left alone.  vvhip_barostat_scale / _restore set NO floor: they leave the velocities alone, and a rigid shift of a molecule keeps its
 * internal vectors up to rounding.  Scheduled removals of the centre-of-mass motion are part of the dynamics.  vvhip_checkpoint_load is
 * refused while a recorder runs.  Host uploads into the bound arrays (vvhip_memcpy_h2d into velm or posq, a re-bind to other arrays) are NOT
 * detected: the next samples correlate against origins of the values that were there before; stop the recorder and start it again.
 * Recovery.  Neither the table nor the ring is idempotent under the repeat of failed steps -- an origin overwritten inside the failed
 * window is needed again by the repeat -- so the rider's recovery words are the WHOLE allocation: counts, floor, table and origin ring,
 * (4 + words) * 8 B + ring_bytes with ring_bytes = num_origins x 3 x stride x 8 B, stride = num_units rounded up to 16.  Nothing caps
 * it: 1024 origins of 111 000 units are 2.7 GB, which every run call that may recover copies once; vvhip_acf_info on an unbound plan
 * gives ring_bytes for a description before anything is allocated -- raise origin_every where the ring is too large. */
#define VVHIP_ACF_VELOCITY_PARTICLES 0
#define VVHIP_ACF_VELOCITY_MOLECULES 1
#define VVHIP_ACF_ORIENTATION 2
typedef struct {
    int32_t interval;               /* a sample after every step whose count is a multiple of it */
    int32_t num_lags;               /* 1 .. 4096: row l is the lag of l * interval steps */
    int32_t origin_every;           /* E, 1 .. num_lags: every E-th sample is an origin */
    int32_t mode;                   /* VVHIP_ACF_VELOCITY_PARTICLES, VVHIP_ACF_VELOCITY_MOLECULES, VVHIP_ACF_ORIENTATION */
    int32_t num_groups;             /* 1 .. 16 */
    int32_t num_pairs;              /* orientation mode: the pairs given, >= 0; else 0 */
    const signed char* group;       /* velocity modes: [num_atoms] the group of every particle of the System; orientation mode: [num_pairs]
                                       the group of every pair; -1: not recorded; NULL: everything in group 0 */
    const int32_t* pairs;           /* orientation mode: [num_pairs][2] head, tail as particle indices of the System; else NULL */
    int64_t max_samples;            /* >= 1 */
    double limit;                   /* velocity modes: nm/ps, a component at or beyond it is bad; rounded up to a power of two; 0: 64.
                                       Orientation mode: 0 */
} vvhip_acf_desc;
typedef struct {
    int64_t samples;                /* samples taken since the start or the last reset (at most max_samples): the next sample's ordinal */
    int64_t dropped;                /* samples that were due past max_samples: nothing was added or stored for them */
    int64_t out_of_range;           /* unit-pairs left out of every word */
    int64_t origin_floor;           /* origins with an ordinal below it are dead */
} vvhip_acf_counts;
typedef struct {
    int32_t active, interval, num_lags, origin_every, mode, num_groups;
    int32_t num_units;              /* units this plan records (those of its shard) */
    int32_t num_origins;            /* ceil(num_lags / origin_every) */
    int32_t frac_bits, row_words;   /* value = word * 2^-frac_bits (pairs: the word itself); 4, or 5 in orientation mode */
    int64_t max_samples;
    int64_t words;                  /* num_groups * num_lags * row_words */
    int64_t ring_bytes;             /* num_origins * 3 * stride * 8 */
    int64_t start_step;             /* the plan's step count at vvhip_acf_start */
    double limit;                   /* as applied (orientation mode: 1) */
} vvhip_acf_layout;
/* Starts (or restarts, dropping what was accumulated) a recorder; synchronises and drops the captured graphs.  Refused, in this order: a
 * null description, interval < 1, num_lags outside 1 .. 4096, origin_every outside 1 .. num_lags, an unknown mode, num_groups outside 1 ..
 * 16, max_samples < 1, a limit that is negative or not finite, or not 0 in orientation mode; in orientation mode num_pairs < 0 or pairs
 * NULL with num_pairs > 0, in the velocity modes pairs or num_pairs given; a group entry outside -1 .. num_groups - 1 (VVHIP_ERR_INVALID
 * naming the argument); in molecule mode a molecule whose massive particles lie in different groups, in orientation mode a pair with an
 * index outside the System, with head = tail or with head and tail in different molecules (VVHIP_ERR_INVALID naming it); frac_bits below
 * 8; num_origins above 1024 (VVHIP_ERR_INVALID); a shard that cuts a molecule (molecule mode) or a recorded pair (orientation mode)
 * (VVHIP_ERR_UNSUPPORTED); an unbound plan; inside a graph capture (VVHIP_ERR_INVALID); an allocation that fails (VVHIP_ERR_HIP, with the
 * byte count).  A description that passes the checks in front of "an unbound plan" is kept even where the start is then refused (active =
 * 0): vvhip_acf_info answers for it, for sizing. */
int vvhip_acf_start(vvhip_plan* plan, const vvhip_acf_desc* desc);
/* Synchronises and copies the counts (out may be NULL) and the table's `words` words (words_out may be NULL with capacity_words = 0; a
 * capacity below the table's size is VVHIP_ERR_INVALID).  reset != 0 zeroes counts, floor and table and restarts the ordinal at 0 with no
 * live origin: the step schedule continues without gap or repeat. */
int vvhip_acf_read(vvhip_plan* plan, int64_t* words_out, int64_t capacity_words, vvhip_acf_counts* out, int32_t reset);
/* Stops the recorder: no more samples are enqueued, table and ring are released, the description is forgotten; synchronises and drops the
 * captured graphs. */
int vvhip_acf_stop(vvhip_plan* plan);
/* The recorder as described (zeros with active = 0 if none was); host only, works on an unbound plan. */
int vvhip_acf_info(const vvhip_plan* plan, vvhip_acf_layout* out);
/* ---------------------------------------------------------------- self van Hove functions accumulated on the device
 * The distribution of single-particle displacements G_s(r, t), of which the MSD keeps the second moment only: from it follow the
 * non-Gaussian parameter alpha_2(t), the self-intermediate scattering function F_s(k, t) and the self-overlap Q_s(t), the standard measures
 * of dynamic heterogeneity and of the cage-to-diffusion crossover that the example scripts' logarithmic GroReporter frames exist to cover.
 * A stand-alone host needs float64 frames for it, 24 B per unit and sample, and a histogram per lag over O(samples x origins x N) pairs; on
 * the device it is an accumulating table of a few MB however long the run.  After every full step whose count is a multiple of `interval`
 * -- counted exactly as for the other riders; a sample "after step k" is enqueued behind that step's autocorrelation sample, the eleventh
 * and last rider -- the step entry point enqueues one accumulating kernel (csrc/vv_dev_vanhove.inc) and a one-thread kernel that advances
 * the sample ordinal: two launches, no memset, no host work.  Inside a captured graph both are part of the graph and the steps that take a
 * sample are part of the graph-cache key.  The recorder reads posq and posqCorrection and writes its own words, nothing else; a plan that
 * never starts one launches what it launched before and allocates nothing.
 * Units.  VVHIP_VANHOVE_PARTICLES and VVHIP_VANHOVE_MOLECULES are the MSD's two modes, word for word: the float64 position, the sequential
 * centre-of-mass sum in ascending particle index with M summed in the same order, the group of a molecule, the refusals.
 * Schedule.  The MSD's, word for word: ordinal j, every E-th sample an origin in slot (j / E) mod num_origins, num_origins = ceil(num_lags /
 * E), row l the lag of (l + 1) * interval steps; at sample j every origin k E contributes to row l = j - k E - 1 provided origin_floor <=
 * k E < j and j - k E <= num_lags.  Accumulation comes first, the store second.
 * Displacement.  Delta_a = c_a(now) - c_a(origin) in float64.  A pair with any Delta_a that is NaN or has |Delta_a| >= limit is out of
 * range: it is left out of every word and adds 1 to out_of_range.  limit is in nm, rounded up to a power of two; 0 takes the default of 16.
 * r2 = (Delta_x * Delta_x + Delta_y * Delta_y) + Delta_z * Delta_z, in this order, without contraction.
 * Bins.  edges[num_bins + 1] in nm, finite, strictly ascending, edges[0] >= 0: uniform or logarithmic or anything else.  The host forms
 * e2[k] = edges[k] * edges[k]; a pair adds the integer 1 to bin b where e2[b] <= r2 < e2[b + 1], decided by comparisons against e2 alone (no
 * square root decides a bin); a pair with r2 < e2[0] adds 1 to `below`, one with r2 >= e2[num_bins] adds 1 to `beyond`; both still enter
 * the moments.
 * Table: int64 head[num_groups][num_lags][6], then int64 hist[num_groups][num_lags][num_bins]; words = head_words + hist_words, at most 2^22
 * (32 MiB).  The six head words: pairs, below, beyond, sum r2 as llrint(r2 * 2^frac2_bits), and sum r2 * r2 in two words: with x = (r2 * r2)
 * * 2^r4_hi_bits,  hi = floor(x),  lo = llrint((x - hi) * 2^r4_lo_bits)  -- every step exact or correctly rounded in float64, so device and
 * host agree bit for bit --, value = (hi + lo * 2^-r4_lo_bits) * 2^-r4_hi_bits.  For every (group, lag): below + sum_b hist + beyond ==
 * pairs.  With cu = ceil_log2(U + 1), U the recorded units of the WHOLE System in that mode, and co = ceil_log2(ceil(max_samples / E) + 1):
 *     frac2_bits  = min(40, 62 - cu - co - 2 log2(limit) - 2)        (r2 < 3 limit^2 < 2^(2 log2(limit) + 2))
 *     r4_hi_bits  = min(40, 62 - cu - co - 4 log2(limit) - 4)        (r2 r2 < 9 limit^4 < 2^(4 log2(limit) + 4))
 *     r4_lo_bits  = min(52, 61 - cu - co)                            (lo <= 2^r4_lo_bits)
 * so that no word can overflow within max_samples samples.  Past max_samples a sample adds nothing, stores no origin and counts as
 * dropped.  Every word is an integer sum: the table is the same bits for any grid, block size, unit order, add path or shard split; a
 * sharded plan records the units of its own shard and the shards' tables add to the unsharded one.
 * What rewrites positions outside the steps, and recovery: as for the MSD.  vvhip_barostat_scale / _restore set origin_floor to the current
 * ordinal; vvhip_checkpoint_load is refused while a recorder runs; the rider's recovery words are the WHOLE allocation, (4 + words) * 8 B +
 * ring_bytes with ring_bytes = num_origins x 3 x stride x 8 B, stride = num_units rounded up to 16. */
#define VVHIP_VANHOVE_PARTICLES 0
#define VVHIP_VANHOVE_MOLECULES 1
#define VVHIP_VANHOVE_MAX_WORDS (1ll << 22)
typedef struct {
    int32_t interval;               /* a sample after every step whose count is a multiple of it */
    int32_t num_lags;               /* 1 .. 4096: row l is the lag of (l + 1) * interval steps */
    int32_t origin_every;           /* E, 1 .. num_lags: every E-th sample is stored as an origin */
    int32_t mode;                   /* VVHIP_VANHOVE_PARTICLES, VVHIP_VANHOVE_MOLECULES */
    int32_t num_groups;             /* 1 .. 16 */
    int32_t num_bins;               /* 1 .. 1024 */
    const signed char* group;       /* [num_atoms] the group of every particle of the System, -1: not recorded; NULL: everything in group 0 */
    const double* edges;            /* [num_bins + 1] nm: finite, strictly ascending, edges[0] >= 0 */
    int64_t max_samples;            /* >= 1 */
    double limit;                   /* nm: a displacement component at or beyond it is out of range; rounded up to a power of two; 0: 16 */
} vvhip_vanhove_desc;
typedef struct {
    int64_t samples;                /* samples taken since the start or the last reset (at most max_samples): the next sample's ordinal */
    int64_t dropped;                /* samples that were due past max_samples: nothing was added or stored for them */
    int64_t out_of_range;           /* unit-pairs left out of every word */
    int64_t origin_floor;           /* origins with an ordinal below it are dead */
} vvhip_vanhove_counts;
typedef struct {
    int32_t active, interval, num_lags, origin_every, mode, num_groups;
    int32_t num_units;              /* units this plan records (those of its shard) */
    int32_t num_origins;            /* ceil(num_lags / origin_every) */
    int32_t num_bins;
    int32_t frac2_bits;             /* sum r2 = word * 2^-frac2_bits */
    int32_t r4_hi_bits, r4_lo_bits; /* sum r2 r2 = (hi + lo * 2^-r4_lo_bits) * 2^-r4_hi_bits */
    int64_t max_samples;
    int64_t words;                  /* head_words + hist_words */
    int64_t head_words;             /* num_groups * num_lags * 6 */
    int64_t hist_words;             /* num_groups * num_lags * num_bins */
    int64_t ring_bytes;             /* num_origins * 3 * stride * 8 */
    int64_t start_step;             /* the plan's step count at vvhip_vanhove_start */
    double limit;                   /* as applied */
} vvhip_vanhove_layout;
/* Starts (or restarts, dropping what was accumulated) a recorder; synchronises and drops the captured graphs.  Refused, in this order: a
 * null description, interval < 1, num_lags outside 1 .. 4096, origin_every outside 1 .. num_lags, an unknown mode, num_groups outside 1 ..
 * 16, max_samples < 1, a limit that is negative or not finite, a group entry outside -1 .. num_groups - 1; num_bins outside 1 .. 1024,
 * edges NULL, an edge that is not finite or negative, edges that do not ascend strictly (VVHIP_ERR_INVALID naming the argument); in
 * molecule mode a molecule whose massive particles lie in different groups (VVHIP_ERR_INVALID naming it); frac2_bits below 8, r4_hi_bits
 * below 0 (VVHIP_ERR_INVALID naming the exponent); more than VVHIP_VANHOVE_MAX_WORDS words (VVHIP_ERR_INVALID with the count); num_origins
 * above 1024 (VVHIP_ERR_INVALID); in molecule mode a shard that cuts a molecule (VVHIP_ERR_UNSUPPORTED); an unbound plan; inside a graph
 * capture (VVHIP_ERR_INVALID); an allocation that fails (VVHIP_ERR_HIP, with the byte count).  A description that passes the checks in
 * front of "an unbound plan" is kept even where the start is then refused (active = 0): vvhip_vanhove_info answers for it, for sizing. */
int vvhip_vanhove_start(vvhip_plan* plan, const vvhip_vanhove_desc* desc);
/* Synchronises and copies the counts (out may be NULL) and the table's `words` words, head then hist (words_out may be NULL with
 * capacity_words = 0; a capacity below the table's size is VVHIP_ERR_INVALID).  reset != 0 zeroes counts, floor and table and restarts the
 * ordinal at 0 with no live origin: the step schedule continues without gap or repeat. */
int vvhip_vanhove_read(vvhip_plan* plan, int64_t* words_out, int64_t capacity_words, vvhip_vanhove_counts* out, int32_t reset);
/* Stops the recorder: no more samples are enqueued, table and ring are released, the description is forgotten; synchronises and drops the
 * captured graphs. */
int vvhip_vanhove_stop(vvhip_plan* plan);
/* The recorder as described (zeros with active = 0 if none was); host only, works on an unbound plan. */
int vvhip_vanhove_info(const vvhip_plan* plan, vvhip_vanhove_layout* out);
/* ---------------------------------------------------------------- distinct van Hove functions accumulated on the device
 * G_d(r, t): the density of OTHER sites at distance r at time t from where a site was at time 0 -- how fast the counter-ion cage around an
 * ion dissolves and what refills the hole the ion leaves; the real-space counterpart of F(k, t) (vvhip_modes_*), and with G_s
 * (vvhip_vanhove_*) the G(r, t) that a scattering experiment measures.  A host cannot produce it during a run: every pair of sites of every
 * sample against every stored origin, (live origins + 1) times the RDF's O(N_a N_b) pair work per sample, on float64 frames of 24 B per
 * site and sample.  After every full step whose count is a multiple of `interval` -- counted exactly as for the other riders; a sample
 * "after step k" is enqueued behind that step's self van Hove sample, the twelfth rider -- the step entry point enqueues three
 * kernels (csrc/vv_dev_vanhove_distinct.inc): a gather of the sites' float64 positions into the planes of "now", the pair kernel over (work
 * items) x (ring slots), and a one-thread kernel that counts the visits and advances the ordinal: no memset, no copy, no host work.  Inside
 * a captured graph all three are graph nodes and the steps that take a sample are part of the graph-cache key.  The recorder reads posq and
 * posqCorrection and writes its own words and planes, nothing else; a plan that never starts one launches what it launched before and
 * allocates nothing.
 * Sites, groups, position.  The RDF's, word for word: the particles with group[i] >= 0, NULL puts every particle into group 0, num_groups
 * is 1 .. 16; X_i in float64 is (double) posq + (double) posqCorrection in mixed precision, (double) posq otherwise, unwrapped; the sites
 * are ordered by group, ascending by particle inside a group.
 * Classes.  num_classes (1 .. 32) ORDERED pairs classes[c] = {ga, gb}: the site at the origin time is in ga, the site at the later time in
 * gb.  ga != gb counts all N_a N_b pairs; ga == gb counts every ordered pair (i, j) with i != j, P_c = N_a (N_a - 1): a site is never paired
 * with its own earlier self (that pairing is G_s).  With exclude_same_molecule != 0 pairs whose particles have equal mol_id are left out of
 * every class, as for the RDF (P_c is not lowered).
 * Schedule.  The MSD's with a zero-lag row in front, as in the autocorrelation recorder: ordinal j, every E-th sample (E = origin_every) is
 * stored as an origin, R = num_origins = ceil(num_lags / E) <= 1024 of them are alive; num_lags + 1 rows, row 0 the sample against itself,
 * row l the lag of l * interval steps.  At sample j the origin k E adds to row l = j - k E provided origin_floor <= k E < j and j - k E <=
 * num_lags; the sample itself always adds to row 0.  Accumulation comes first, the store second: where R E == num_lags the oldest origin
 * still contributes at lag num_lags when the newest is stored (the ring has R + 1 slots, so the two never share one).
 * Arithmetic.  The RDF's with i taken at the origin and j now, all float64, no contraction; per axis, with L the plan's box when the sample
 * is enqueued and inv_L_a = 1.0 / L_a formed once per sample:
 *     d = X_j,a(now) - X_i,a(origin);   n = rint(d * inv_L_a)  (round-half-even);   d = d - L_a * n
 * and then  r2 = (dx * dx + dy * dy) + dz * dz.
 * Bins.  Uniform in r: dr = r_max / nbins and edges e(k) = ((double) k * dr) * ((double) k * dr), k = 0 .. nbins, nbins 1 .. 8192.  A pair
 * adds the integer 1 to the bin b of its class and row with  e(b) <= r2 < e(b + 1)  (comparisons decide, never a square root); a pair with
 * r2 >= e(nbins) adds nothing; a pair whose r2 is NaN adds 1 to `invalid` and to no bin.
 * Table: int64 head[num_lags + 1][2], then int64 hist[num_classes][num_lags + 1][nbins]; words = head_words + hist_words, at most 2^22
 * (32 MiB).  head[l][0]: the (origin, sample) visits to row l; head[l][1]: the bits of a float64 that sums 1.0 / ((Lx * Ly) * Lz) over
 * those visits -- a row receives at most one visit per sample, so the sum is sequential in sample order and reproducible.  Every hist
 * word is an integer sum: the table is the same bits for any work list, tile shape, block size, histogram layout or arrival order.
 *     G_d,c(l, b) = hist[c][l][b] / (P_c * shell(b) * inv_volume_sum[l]),   shell(b) = 4 pi / 3 (e(b + 1)^(3/2) - e(b)^(3/2)),
 * which tends to 1 at large r; row 0 of a class with ga != gb is the RDF's table of that class, with ga == gb twice it.
 * Box and positions changed outside the steps.  r_max must be finite, > 0 and <= min(Lx, Ly, Lz) / 2 of the plan's box at the start.
 * vvhip_set_box (with a box that differs) and vvhip_barostat_scale / _restore set origin_floor to the current ordinal: an origin under
 * another box has no minimum image with the present one; what else rewrites positions outside the steps is handled as for the MSD.  A sample
 * enqueued while min(L) / 2 < r_max adds nothing, stores nothing, does not advance the ordinal, sets origin_floor to the ordinal and counts
 * as dropped, so every row stays a true lag.  Past max_samples a sample adds nothing, stores no origin and counts as dropped.  The box is a
 * kernel argument: what changes it drops the captured graphs.
 * Overflow.  Refused at the start where the largest P_c times max_samples reaches 2^62.
 * Sharded plans are refused (VVHIP_ERR_UNSUPPORTED), as for the RDF.  Recovery.  vvhip_checkpoint_load is refused while a recorder runs;
 * the rider's recovery words are the WHOLE allocation, (4 + words) * 8 B + ring_bytes: counts, table and ring, with ring_bytes =
 * (num_origins + 2) x 3 x stride x 8 B (the R + 1 slots and the spare plane set of a sample that is no origin), stride = the sites
 * rounded up to 16. */
#define VVHIP_VANHOVE_DISTINCT_MAX_WORDS (1ll << 22)
typedef struct {
    int32_t interval;               /* a sample after every step whose count is a multiple of it */
    int32_t num_lags;               /* 1 .. 4096: rows 0 .. num_lags, row l the lag of l * interval steps */
    int32_t origin_every;           /* E, 1 .. num_lags: every E-th sample is stored as an origin */
    int32_t nbins;                  /* 1 .. 8192 */
    int32_t num_groups;             /* 1 .. 16 */
    int32_t num_classes;            /* 1 .. 32 */
    int32_t exclude_same_molecule;  /* != 0: pairs inside one molecule (mol_id) are left out */
    int32_t reserved;               /* 0 */
    const signed char* group;       /* [num_atoms] the group of every particle of the System, -1: no site; NULL: everything in group 0 */
    const int32_t* classes;         /* [num_classes][2] ga (at the origin), gb (now) of every class */
    int64_t max_samples;            /* >= 1 */
    double r_max;                   /* nm */
} vvhip_vanhove_distinct_desc;
typedef struct {
    int64_t samples;                /* samples taken since the start or the last reset (at most max_samples): the next sample's ordinal */
    int64_t dropped;                /* samples that were due past max_samples or in a box with min(L) / 2 < r_max: nothing was added or stored */
    int64_t invalid;                /* pairs whose r2 was NaN */
    int64_t origin_floor;           /* origins with an ordinal below it are dead */
} vvhip_vanhove_distinct_counts;
typedef struct {
    int32_t active, interval, num_lags, origin_every, nbins, num_groups, num_classes, exclude_same_molecule;
    int32_t tile;                   /* sites per tile of the pair kernel */
    int32_t num_items;              /* work items: the pair kernel runs num_items * (num_origins + 1) blocks per sample */
    int32_t num_origins;            /* ceil(num_lags / origin_every) */
    int32_t num_rows;               /* num_lags + 1 */
    int32_t num_sites[16];          /* per group */
    int32_t classes[32][2];
    int64_t pairs_per_sample[32];   /* per class: N_a N_b, or N_a (N_a - 1) */
    int64_t max_samples;
    int64_t words;                  /* head_words + hist_words */
    int64_t head_words;             /* (num_lags + 1) * 2 */
    int64_t hist_words;             /* num_classes * (num_lags + 1) * nbins */
    int64_t ring_bytes;             /* (num_origins + 2) * 3 * stride * 8 */
    int64_t start_step;             /* the plan's step count at vvhip_vanhove_distinct_start */
    double r_max, dr;               /* dr = r_max / nbins */
} vvhip_vanhove_distinct_layout;
/* Starts (or restarts, dropping what was accumulated) a recorder; synchronises and drops the captured graphs.  Refused, in this order: a
 * null description, interval < 1, num_lags outside 1 .. 4096, origin_every outside 1 .. num_lags, r_max not finite or <= 0, nbins outside
 * 1 .. 8192, num_groups outside 1 .. 16, num_classes outside 1 .. 32, classes NULL, max_samples < 1, a group entry outside -1 ..
 * num_groups - 1, a class entry outside 0 .. num_groups - 1 (VVHIP_ERR_INVALID naming the argument); more than
 * VVHIP_VANHOVE_DISTINCT_MAX_WORDS words (VVHIP_ERR_INVALID with the count); num_origins above 1024; the largest class's pairs per sample
 * times max_samples at or above 2^62; r_max above half the shortest edge of the plan's box (VVHIP_ERR_INVALID); a sharded plan
 * (VVHIP_ERR_UNSUPPORTED); an unbound plan; inside a graph capture (VVHIP_ERR_INVALID); an allocation that fails (VVHIP_ERR_HIP, with the
 * byte count).  A description that passes the checks in front of "an unbound plan" is kept even where the start is then refused (active =
 * 0): vvhip_vanhove_distinct_info answers for it, for sizing. */
int vvhip_vanhove_distinct_start(vvhip_plan* plan, const vvhip_vanhove_distinct_desc* desc);
/* Synchronises and copies the counts (out may be NULL) and the table's `words` words, head then hist (words_out may be NULL with
 * capacity_words = 0; a capacity below the table's size is VVHIP_ERR_INVALID).  reset != 0 zeroes counts, floor and table and restarts the
 * ordinal at 0 with no live origin: the step schedule continues without gap or repeat. */
int vvhip_vanhove_distinct_read(vvhip_plan* plan, int64_t* words_out, int64_t capacity_words, vvhip_vanhove_distinct_counts* out, int32_t reset);
/* Stops the recorder: no more samples are enqueued, table and ring are released, the description is forgotten; synchronises and drops the
 * captured graphs. */
int vvhip_vanhove_distinct_stop(vvhip_plan* plan);
/* The recorder as described (zeros with active = 0 if none was); host only, works on an unbound plan. */
int vvhip_vanhove_distinct_info(const vvhip_plan* plan, vvhip_vanhove_distinct_layout* out);
/* ---------------------------------------------------------------- spatial distribution functions accumulated on the device
 * Where the sites sit around a molecule in the molecule's own body frame -- for an imidazolium cation: the anions above the ring, at the
 * C2-H, along the alkyl tail -- the one structure function g(r) cannot give, because g(r) averages exactly these directions.  Per sample
 * it costs what an RDF costs, O(N_frames N_sites), plus a frame per molecule, and its table is three-dimensional, so it wants far more
 * samples than a g(r) before the voxels are smooth: from downloaded frames that is hours on a host.  After every full step whose count is
 * a multiple of `interval` -- counted exactly as for the other riders; a sample "after step k" is enqueued behind that step's distinct van
 * Hove sample, the thirteenth and last rider -- the step entry point enqueues three kernels (csrc/vv_dev_sdf.inc): a gather of the sites'
 * float64 positions and of the frames into planar scratch, the pair kernel, and a one-thread kernel that counts the sample: no memset, no
 * host work.  Inside a captured graph all three are graph nodes and the steps that take a sample are part of the graph-cache key.  The
 * recorder reads posq and posqCorrection and writes its own words and scratch, nothing else; a plan that never starts one launches what it
 * launched before and allocates nothing.
 * Position.  X_i in float64 exactly as for the RDF: (double) posq + (double) posqCorrection in mixed precision, (double) posq otherwise.
 * Frames.  frames[f] = {o, a, b}, num_frames >= 0 triplets of particle indices of the System, pairwise different and in one molecule
 * (vvhip_system_desc.mol_id).  frame_group[f] is one byte per frame, -1: not recorded; NULL puts every frame into group 0;
 * num_frame_groups is 1 .. 16.  Molecules are stored whole and unwrapped (as for the orientation units of vvhip_acf_*), so no minimum image
 * is taken inside a frame.  All float64, no contraction, every product rounded before its sum or difference is taken:
 *     p = X_a - X_o;   q = X_b - X_o
 *     n1 = (p_x p_x + p_y p_y) + p_z p_z;     e1 = p * acf_inverse_norm(n1)
 *     t  = (q_x e1_x + q_y e1_y) + q_z e1_z;  w_c = q_c - t * e1_c
 *     n2 = (w_x w_x + w_y w_y) + w_z w_z;     e2 = w * acf_inverse_norm(n2)
 *     e3_x = e1_y e2_z - e1_z e2_y;   e3_y = e1_z e2_x - e1_x e2_z;   e3_z = e1_x e2_y - e1_y e2_x
 * with acf_inverse_norm the one sequence of +, -, * of the orientation autocorrelation (csrc/vv_layout.h; tests/acf_reference.py:
 * inverse_norm), the same bits on device and host.  e1 points from o to a, e2 lies in the plane of o, a, b on b's side, e3 = e1 x e2 is
 * right-handed.  A frame is bad in a sample when n1 or n2 is NaN or outside [2^-40, 2^40) nm^2 (n2 is not formed where n1 is): it takes
 * part in no pair of that sample and adds 1 to bad_frames; a good frame of a counted sample adds 1 to frame_visits[its group].
 * Sites.  The particles with site_group[i] >= 0 over the whole System; NULL puts every particle into group 0; num_site_groups is 1 .. 16.
 * Classes.  num_classes (1 .. 16) ordered pairs classes[c] = {frame group, site group}; every (good frame, site) pair of the two groups
 * counts, pairs_per_sample[c] = N_frames N_sites.  With exclude_same_molecule != 0 a site whose mol_id is that of the frame's o is counted
 * nowhere (not in `invalid` either); without it the frame's own atoms are sites like any other (o itself lands at xi = 0).
 * Pair.  d = X_s - X_o per axis with the RDF's minimum image, L the plan's box when the sample is enqueued, inv_L_a = 1.0 / L_a formed once
 * per sample:   n = rint(d * inv_L_a)  (round-half-even);   d = d - L_a * n.   Then  xi_k = (d_x e_k,x + d_y e_k,y) + d_z e_k,z,  k = 1, 2, 3.
 * Voxels.  A cube of half-extent `extent` (h, nm) in frame coordinates with nbins (n, 1 .. 128) voxels per axis; inv_w = (double) n /
 * (2.0 * h) formed once; u_k = (xi_k + h) * inv_w.  The pair is in range iff 0 <= u_k < n for all three k, and then adds the integer 1 to
 * table[c][(int) u_1][(int) u_2][(int) u_3]; a pair out of range on any axis adds nothing; a pair of a good frame with a NaN among its u
 * adds 1 to `invalid` and to no voxel.  These comparisons and conversions define the voxel.  The kernel puts a cheaper test in front of
 * them, r2 = (d_x d_x + d_y d_y) + d_z d_z against 3 h^2 (1 + 2^-20) / (1 - delta) with delta bounding how far the frame's e_k as stored
 * are from orthonormal (csrc/vv_dev_sdf.inc proves it conservative: it rejects only pairs the comparisons reject); it is no part of the
 * definition.  (Positions are taken to be below 2^500 nm: beyond, a product overflows and the cheap test and the comparisons may differ.)
 * Table: int64 table[num_classes][n][n][n], xi_1 outermost; words = num_classes n^3, at most VVHIP_SDF_MAX_WORDS = 2^23 (64 MiB).  Integer
 * adds commute: the table is the same bits for any grid, tile shape or arrival order.
 *     density_c(v) = table[c][v] / (frame_visits[frame group] * voxel^3),  voxel = 2 h / n;   g_c(v) = density_c(v) / (N_sites *
 *     inv_volume_sum / samples), which tends to 1 far from the molecule.
 * Range.  h is finite and > 0, and 3 h^2 < (min(Lx, Ly, Lz) / 2)^2 for the plan's box at the start: the cube's corners then lie inside
 * one sphere that holds at most one image of any site, and that image is the per-axis minimum image.  A sample enqueued while the plan's
 * box no longer satisfies this (vvhip_set_box, the barostat's moves) adds nothing -- no visit, no bad frame -- and counts as dropped; back
 * in range the samples count again.  The box is a kernel argument: what changes it drops the captured graphs.
 * Counts.  samples; dropped (due past max_samples, or in a box too small for the cube); invalid; bad_frames; inv_volume_sum, the RDF's
 * sequential float64 sum  s = s + 1.0 / ((Lx * Ly) * Lz)  over the counted samples; frame_visits[16].
 * Overflow.  Refused at the start where the largest class's N_frames N_sites times max_samples reaches 2^62.
 * Sharded plans are refused (VVHIP_ERR_UNSUPPORTED): pairs across shards exist on no device.
 * Recovery.  The rider's recovery words are the whole allocation, counts and table, (21 + words) * 8 B -- up to 64 MiB, and that is what a
 * recovery snapshot copies per run call while the recorder runs; the scratch is rewritten by every sample and is not saved.
 * vvhip_checkpoint_load is refused while a recorder runs, a re-bind drops the captured graphs, as for the RDF. */
#define VVHIP_SDF_MAX_WORDS (1ll << 23)
typedef struct {
    int32_t interval;               /* a sample after every step whose count is a multiple of it */
    int32_t nbins;                  /* n, 1 .. 128 voxels per axis */
    int32_t num_frames;             /* >= 0 */
    int32_t num_frame_groups;       /* 1 .. 16 */
    int32_t num_site_groups;        /* 1 .. 16 */
    int32_t num_classes;            /* 1 .. 16 */
    int32_t exclude_same_molecule;  /* != 0: the sites of the frame's own molecule (mol_id) are left out */
    int32_t reserved;               /* 0 */
    const int32_t* frames;          /* [num_frames][3] the particles o, a, b of every frame */
    const signed char* frame_group; /* [num_frames] the group of every frame, -1: not recorded; NULL: every frame in group 0 */
    const signed char* site_group;  /* [num_atoms] the group of every particle of the System, -1: no site; NULL: everything in group 0 */
    const int32_t* classes;         /* [num_classes][2] frame group, site group of every class */
    int64_t max_samples;            /* >= 1 */
    double extent;                  /* h, nm: the cube is [-h, h)^3 in frame coordinates */
} vvhip_sdf_desc;
typedef struct {
    int64_t samples;                /* samples counted since the start or the last reset (at most max_samples) */
    int64_t dropped;                /* samples that were due past max_samples or in a box too small for the cube: nothing was added */
    int64_t invalid;                /* pairs of a good frame with a NaN among u_1, u_2, u_3 */
    int64_t bad_frames;             /* (frame, counted sample) visits whose n1 or n2 was NaN or outside [2^-40, 2^40) */
    double inv_volume_sum;          /* the counted samples' 1 / V, summed in sample order */
    int64_t frame_visits[16];       /* per frame group: the good frames of the counted samples */
} vvhip_sdf_counts;
typedef struct {
    int32_t active, interval, nbins, num_frame_groups, num_site_groups, num_classes, exclude_same_molecule;
    int32_t tile;                   /* frames per tile of the pair kernel (a frame count of tile + 1 is the first with a second tile) */
    int32_t num_items;              /* blocks of the pair kernel per sample */
    int32_t reserved;               /* 0 */
    int32_t num_frames[16];         /* per frame group */
    int32_t num_sites[16];          /* per site group */
    int32_t classes[16][2];
    int64_t pairs_per_sample[16];   /* per class: N_frames N_sites (the exclusion does not lower it) */
    int64_t max_samples;
    int64_t words;                  /* num_classes * nbins^3 */
    int64_t scratch_bytes;          /* the gather's planes: (3 x stride + 13 x fstride) x 8 B, the sites and the frames rounded up to 16 */
    int64_t start_step;             /* the plan's step count at vvhip_sdf_start */
    double extent, voxel;           /* voxel = 2 extent / nbins, the voxel's edge in nm */
} vvhip_sdf_layout;
/* Starts (or restarts, dropping what was accumulated) a recorder; synchronises and drops the captured graphs.  Refused, in this order: a
 * null description, interval < 1, extent not finite or <= 0, nbins outside 1 .. 128, num_frames < 0, num_frame_groups or num_site_groups
 * outside 1 .. 16, num_classes outside 1 .. 16, classes NULL, frames NULL with num_frames > 0, max_samples < 1, a frame_group entry outside
 * -1 .. num_frame_groups - 1, a site_group entry outside -1 .. num_site_groups - 1, a class entry outside its group count, a frame with an
 * index outside the System, with two equal indices or with particles of different molecules (VVHIP_ERR_INVALID naming the argument or the
 * frame); more than VVHIP_SDF_MAX_WORDS words (VVHIP_ERR_INVALID with the count); the largest class's pairs per sample times max_samples at
 * or above 2^62; 3 extent^2 not below (min(L) / 2)^2 of the plan's box (VVHIP_ERR_INVALID); a sharded plan (VVHIP_ERR_UNSUPPORTED); an
 * unbound plan; inside a graph capture (VVHIP_ERR_INVALID); an allocation that fails (VVHIP_ERR_HIP, with the byte count).  A description
 * that passes the checks in front of "an unbound plan" is kept even where the start is then refused (active = 0): vvhip_sdf_info answers
 * for it, for sizing. */
int vvhip_sdf_start(vvhip_plan* plan, const vvhip_sdf_desc* desc);
/* Enqueues one sample now, behind what is queued, whatever the schedule says; it counts as a sample like a scheduled one.
 * VVHIP_ERR_INVALID without a running recorder or inside a graph capture. */
int vvhip_sdf_sample(vvhip_plan* plan);
/* Synchronises and copies the counts (out may be NULL) and the table's `words` words (words_out may be NULL with capacity_words = 0; a
 * capacity below the table's size is VVHIP_ERR_INVALID).  reset != 0 zeroes counts and table: the step schedule continues without gap or
 * repeat. */
int vvhip_sdf_read(vvhip_plan* plan, int64_t* words_out, int64_t capacity_words, vvhip_sdf_counts* out, int32_t reset);
/* Stops the recorder: no more samples are enqueued, table and scratch are released, the description is forgotten; synchronises and drops
 * the captured graphs. */
int vvhip_sdf_stop(vvhip_plan* plan);
/* The recorder as described (zeros with active = 0 if none was); host only, works on an unbound plan. */
int vvhip_sdf_info(const vvhip_plan* plan, vvhip_sdf_layout* out);
/* ---------------------------------------------------------------- removal of the centre-of-mass motion on the device
 * What OpenMM's CMMotionRemover does inside context->updateContextState() (VVIntegrator.cpp:234, 278): a stand-alone host has no such
 * service, and the thermostat already counts the 3 degrees of freedom as removed (has_cm_motion_remover).  Over ALL particles of the
 * System with mass > 0 -- NH and Langevin subsets, Drude particles and their parents alike --
 *     M = sum m_i,   P = sum m_i v_i,   V = P / M,   v_i <- v_i - V   for every i with m_i > 0
 * with m_i the System's masses as the plan holds them.  Massless particles (images, virtual sites) are neither summed nor touched;
 * positions, velm.w, forces, thermostat state, accumulators, rendezvous words and the four status words are not touched.  This is the
 * documented behaviour of OpenMM's kernel stated in float64, not pinned against OpenMM.
 * Two kernels (sum, subtract) in the plan's stream, nothing in between; the sums are fixed point, so the same velocities give the same
 * V bits whatever the launch shape or wave layout (csrc/vv_args.hpp: CmmArgs states the quantisation).  A term m v outside the
 * fixed-point range (NaN included) makes that removal a no-op and counts it as skipped; no status word is raised.
 * Schedule: with frequency f the removal runs IN FRONT OF every full step whose 0-based index -- the plan's step count before the step,
 * the counter of the series -- is a multiple of f: vvhip_step_middle, vvhip_step_vv_first, phase 0 of vvhip_step_middle_phase and the
 * steps of vvhip_run_graph / vvhip_run_eager enqueue it; the split per-KernelImpl entry points and vvhip_run_eager_unfused do not
 * (inside OpenMM the platform's remover runs and this stays off).  A series row "after step k" is recorded before the removal in
 * front of step k + 1.  Inside a captured graph the removals are part of the graph, and the steps that carry one are part of the
 * graph-cache key: when f divides the graph's length or the length divides f, steady-state replays re-capture nothing.  A repaired
 * rendezvous (vvhip_recovery_count) repeats the removals at the same steps and restores the record's counters with the snapshot.
 * Nothing is on by default: a plan that never calls vvhip_cm_motion_start launches what it launched before. */
typedef struct {
    int32_t frequency;              /* steps between removals; 0: none scheduled */
    int32_t reserved;               /* 0 */
    int64_t removals;               /* scheduled removals done since vvhip_cm_motion_start */
    int64_t skipped;                /* ... skipped because a term left the fixed-point range (nothing was subtracted) */
    double last_v[3];               /* the V of the last scheduled removal, nm/ps (NaN after a skipped one, 0 before the first) */
    double total_mass;              /* M, Da */
} vvhip_cm_motion_record;
/* Schedules a removal in front of every `frequency`-th step (restarts with the new frequency and a cleared record if already on); drops
 * the captured graphs.  Refused, in this order: frequency < 1 (VVHIP_ERR_INVALID); a plan described with has_cm_motion_remover = 0
 * (VVHIP_ERR_INVALID: the thermostat's degrees of freedom would not match); a sharded plan (VVHIP_ERR_UNSUPPORTED: a shard's momentum is
 * partial); an unbound plan; inside a graph capture (VVHIP_ERR_INVALID). */
int vvhip_cm_motion_start(vvhip_plan* plan, int32_t frequency);
/* No further removals; drops the captured graphs.  The record stays readable. */
int vvhip_cm_motion_stop(vvhip_plan* plan);
/* One removal now, in the plan's stream behind what is queued; blocks and returns the V it subtracted (24 bytes back; v_removed may be
 * NULL).  Independent of the schedule, its record, the step counter and has_cm_motion_remover: a plain operation on the velocities, as
 * after setVelocities.  Refused on a sharded plan (VVHIP_ERR_UNSUPPORTED).  A term out of range gives VVHIP_ERR_OVERFLOW for this call
 * only, with the velocities untouched. */
int vvhip_remove_cm_motion(vvhip_plan* plan, double v_removed[3]);
/* Synchronises and copies the schedule's record; VVHIP_ERR_OVERFLOW (record filled) if a scheduled removal was skipped.  The host-only
 * fields (frequency, total_mass) are filled on an unbound plan too. */
int vvhip_cm_motion_read(vvhip_plan* plan, vvhip_cm_motion_record* out);
/* ---------------------------------------------------------------- Maxwell-Boltzmann start velocities on the device
 * What context.setVelocitiesToTemperature(T) gives a run inside OpenMM (examples/run-bulk.py:87): a stand-alone host has no such service.
 * One kernel (csrc/vv_dev_thermalize.inc) writes velm.xyz of this plan's particles; velm.w, positions, forces, thermostat state,
 * accumulators, rendezvous words, the four status words and the series / CM records are not touched.  The result is a pure function of
 * (seed, global particle index, masses, T, T_D) -- not of the wave layout, the launch shape or the shard split, so every rank of a
 * sharded run draws its own particles and the shards' arrays concatenate to the unsharded draw.  For particle g with mass m > 0
 *     (w0 .. w3) = Philox4x32-10(counter {g, 0, 0, 0x5654}, key {seed & 0xffffffff, seed >> 32})
 *     u0 = (w0 + 1) 2^-32, u1 = w1 2^-32, u2 = (w2 + 1) 2^-32, u3 = w3 2^-32,   r0 = sqrt(-2 ln u0), r1 = sqrt(-2 ln u2)
 *     n(g) = (r0 cos 2 pi u1, r0 sin 2 pi u1, r1 cos 2 pi u3)
 * in float64, and with R = 8.31446261815324e-3 kJ/(mol K)
 *     plain mode (drude_temperature < 0; OpenMM's documented behaviour):   v = sqrt(R T / m) n(g)
 *     Drude-aware mode (drude_temperature >= 0), a pair (d, p) with both masses > 0:   M = m_d + m_p, mu = m_d m_p / M,
 *         V = sqrt(R T / M) n(p), w = sqrt(R T_D / mu) n(d), v_d = V + (m_p / M) w, v_p = V - (m_d / M) w;   everybody else as in plain mode
 * Massless particles (images, virtual sites, merged Drudes) get v = 0.  The store rounds to the mode's `mixed` type.  This is OpenMM's
 * behaviour as documented, stated in float64, NOT pinned against OpenMM's bits or its random stream.
 * The call works in the plan's stream behind whatever is queued: (1) the draw; (2) unless VVHIP_THERMALIZE_NO_CONSTRAINTS is set, on a plan
 * that solves its constraints in-kernel (constraints_fused with constraint distances given), one launch of kernel A with exactly the
 * plan's velocity-constraint stages on the bound positions at the current constraint tolerance (the bound arrays must already hold the
 * positions and, in velm.w, the inverse masses: this launch reads them, and the plan's static mass tables are filled from velm.w by
 * the first launch that uses them) -- OpenMM's applyVelocityConstraints
 * after the draw (record.constrained = 1; otherwise 0, and a host with a solver of its own applies it); (3) with
 * VVHIP_THERMALIZE_REMOVE_CM one removal as by the one-off call above (record.cm_removed = 1, v_removed = the V subtracted).  Then it
 * blocks and fills the record.  The step counter, the thermostat state and the Langevin generator (its seed and epoch) are not touched;
 * captured graphs stay valid (velocities are data, not arguments).
 * Refused: temperature < 0 or not finite, drude_temperature NaN or infinite, unknown flag bits (VVHIP_ERR_INVALID); VVHIP_THERMALIZE_REMOVE_CM
 * on a sharded plan (VVHIP_ERR_UNSUPPORTED, before anything is drawn); an unbound plan; inside a graph capture (VVHIP_ERR_INVALID). */
#define VVHIP_THERMALIZE_NO_CONSTRAINTS 1   /* leave the raw draw (tests; hosts with their own solver) */
#define VVHIP_THERMALIZE_REMOVE_CM      2   /* then one removal of the centre-of-mass motion */
typedef struct {
    int64_t drawn;                  /* this plan's particles with mass > 0: every one got a fresh velocity */
    int64_t pairs_split;            /* Drude pairs drawn as centre of mass + relative motion (0 in plain mode) */
    int64_t zeroed;                 /* this plan's massless particles: velocity set to 0 */
    int32_t constrained;            /* 1: the in-kernel velocity constraints ran on the draw */
    int32_t cm_removed;             /* 1: the centre-of-mass velocity was removed */
    double v_removed[3];            /* ... and what was subtracted, nm/ps (0 otherwise) */
} vvhip_thermalize_record;
int vvhip_set_velocities_to_temperature(vvhip_plan* plan, double temperature, double drude_temperature /* < 0: plain */,
                                        uint64_t seed, uint32_t flags, vvhip_thermalize_record* out /* may be NULL */);
/* ---------------------------------------------------------------- Monte Carlo barostat: molecule-wise box scaling on the device
 * The device half of an attempt of OpenMM's MonteCarloBarostat / MonteCarloAnisotropicBarostat (examples/run-bulk.py: --barostat, the
 * default ensemble of the bulk example): a stand-alone host has no such service.  The Monte Carlo decision is a few host scalars per
 * attempt and needs the host's potential energy, which this library does not own (openmm-velocityverlet_amd/barostat.py holds the
 * driver); what is done here: every molecule is moved rigidly so that its centre scales with the box, the proposal can be undone bit
 * for bit, and the plan's box is kept in step.  A plain operation on the bound arrays between run calls -- host-driven, never captured,
 * not scheduled by the step counter: the box is a kernel argument baked into the captured graphs, so graphs run between attempts as
 * they do between two vvhip_set_box calls.  Inside OpenMM the platform's own barostat runs and this stays off.
 * Arithmetic.  Let particle i of this plan have stored position X_i, component-wise in float64: (double) posq + (double) posqCorrection
 * in mixed precision, (double) posq in single, posq in double.  Let mol(i) be its molecule from vvhip_system_desc.mol_id -- ALL particles,
 * massless images and virtual sites included; molecules need not be contiguous in index.  Let n_max be the largest molecule of the whole
 * System (not of the shard) and F = 40 - ceil(log2(n_max)).
 *     Q_i = llrint(X_i 2^F), to nearest even; valid only for finite |X_i| < 2^22 nm, anything else raises a "bad" word
 *     S_m = sum of Q_i over i in m, exact in int64 (|S_m| < 2^62 by construction): integer atomics, any order, the same bits
 *     c_m = ((double) S_m 2^-F) / (double) n_m                the geometric centre
 *     e_a = s_a - 1.0                                         formed once per axis by the host, in double
 *     d_(m,a) = c_(m,a) e_a                                   one multiply (the library is built with contraction off, as everywhere)
 *     X'_i = X_i + d_mol(i)                                   one add
 * Store: mixed precision posq' = (float) X', then corr' = (float) (X' - (double) posq') -- the split of the step's own position store
 * (kernel B's B_POS3 stage; csrc/vv_dev_wave.inc: PosIO) --; single (float) X'; double X'.  posq.w and corr.w keep their bits.  An axis
 * with e_a == 0 keeps the stored bits of that component, posq and correction alike: it is not re-split.  The geometric centre is
 * OpenMM's choice for its barostat as remembered; this is that behaviour stated in float64, NOT pinned against OpenMM.
 * Two kernels (sum, shift) in the plan's stream with only the kernel boundary between them (csrc/vv_dev_barostat.inc); neither touches
 * velocities, velm.w, forces, forceExtra, thermostat copies, accumulators, rendezvous words or status words.  With the bad word up the
 * shift kernel stores nothing at all.  The bits do not depend on the launch shape, the wave layout or the shard split: a sharded plan
 * scales its own molecules (a shard must not cut a molecule: VVHIP_ERR_UNSUPPORTED otherwise), F comes from the whole System, and the
 * shards' arrays concatenate to the unsharded result bit for bit; sending the same scale to every rank is the host's business.
 * Checkpoints carry the box: one taken while a scale is pending records the scaled state, and the backup does not travel -- after a
 * load there is nothing to restore. */
typedef struct {
    int64_t molecules;              /* shard-local molecules moved by a scale */
    int64_t scales, restores;       /* calls done since bind */
    int32_t pending;                /* 1: a scale can still be undone */
    int32_t frac_bits;              /* F */
    double box_before[3], box_after[3];   /* of the last scale */
} vvhip_barostat_record;
/* Enters as vvhip_synchronize does (a pending rendezvous repair is settled first; a sticky status word returns its error).  Copies posq
 * (and the correction) of this plan's particles device-to-device into plan-owned backup buffers (allocated by the first call), runs the
 * two kernels and blocks.  With the bad word raised: VVHIP_ERR_OVERFLOW for this call only, positions and box untouched, nothing pending.
 * Otherwise box[a] *= scale[a] as by vvhip_set_box (the captured graphs go), the recovery snapshot is invalidated as by a checkpoint
 * load, and the scale is pending.  A second scale while one is pending overwrites the backup: the implicit accept.
 * Refused, in this order: a scale component that is not finite or <= 0 (VVHIP_ERR_INVALID, naming it); image pairs with scale[2] != 1
 * (VVHIP_ERR_UNSUPPORTED: the mirror plane would have to move); an unbound plan; inside a graph capture (VVHIP_ERR_INVALID). */
int vvhip_barostat_scale(vvhip_plan* plan, const double scale[3]);
/* Copies the backup back, puts the old box back and clears the pending mark: the state is bit for bit the state before the scale, every
 * vvhip_state_digest word equal.  VVHIP_ERR_INVALID when no scale is pending, or when after the scale the plan's step counter moved or
 * vvhip_set_box, vvhip_bind or vvhip_checkpoint_load was called.  The split per-KernelImpl entry points do not count steps: steps
 * taken through them are NOT detected. */
int vvhip_barostat_restore(vvhip_plan* plan);
/* The record; the host-only fields (molecules, frac_bits) are filled on an unbound plan too. */
int vvhip_barostat_read(vvhip_plan* plan, vvhip_barostat_record* out);

/* ---------------------------------------------------------------- checkpoint: a run's complete state, bit for bit
 * What context.createCheckpoint() / loadCheckpoint() give a run inside OpenMM (examples/run-bulk.py: CheckpointReporter, --cpt): a
 * stand-alone host has no such service.  The state is the list the plan's recovery snapshot keeps (vvhip_recovery_count), made durable:
 * positions, correction, velocities, forces, forceExtra, the Langevin normals in use, BOTH parity copies of the device-resident
 * thermostat state (with the exchange and rendezvous counters and the self-tuning wait), the generator's epoch, and the host's cursor
 * (thermostat parity, random cursor, the two forceExtra flags, the step counter) with the generator's seed.  A run continued from a
 * loaded blob gives the bits of the uninterrupted run on every path (step entry points, vvhip_run_eager, vvhip_run_graph; either
 * scheme).  NOT carried: the rows of a series and the record of the scheduled removals (the host starts both again after a load; the
 * step counter travels, so their schedules continue at the same steps), the parameters (read live from the host's setters, as in the
 * reference; the header holds them as they stood, for inspection), the status words and the plan's tuning.  This is the project's own
 * format, not OpenMM's.
 *
 * Digest.  View a section as 32-bit little-endian words w[j], j = 0 .. n - 1, with global word index g = base + j, g < 2^32; base =
 * shard_begin x (words per particle) for the particle sections (posq, correction, velm, forceExtra), 0 for every other.  In uint64
 * arithmetic mod 2^64
 *     z = ((g << 32) | w[j]) + 0x9E3779B97F4A7C15;   z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;   z ^= z >> 27;  z *= 0x94D049BB133111EB;
 *     z ^= z >> 31;   digest = sum of z over j                                                             (an empty section: 0)
 * The wrapping sum is independent of order, launch shape and wave layout, and for the particle sections additive over shards.
 * vvhip_digest_host computes it on the host (bytes a multiple of 4, base + bytes / 4 <= 2^32: VVHIP_ERR_INVALID otherwise),
 * vvhip_state_digest on the device (csrc/vv_dev_digest.inc) for every section of the plan: 8 bytes copied back per section instead
 * of the arrays.
 *
 * Blob (little-endian, version 1): the 272 bytes of vvhip_checkpoint_header, then `num_sections` vvhip_checkpoint_section entries (40 bytes
 * each, ascending ids), then the payloads, each at a 16-byte aligned offset from the blob's start in the table's order, padding zero;
 * total_bytes = the end of the last payload rounded up to 16.  header_digest = the digest of header bytes [0, 264) at base 0 plus the
 * digest of the table at base 66.  The cursor section's payload is the 32 bytes of the header's vvhip_checkpoint_cursor and is always there. */
enum {
    VVHIP_CKPT_POSQ = 0, VVHIP_CKPT_CORRECTION = 1, VVHIP_CKPT_VELM = 2, VVHIP_CKPT_FORCE = 3, VVHIP_CKPT_FORCE_EXTRA = 4,
    VVHIP_CKPT_RANDOM = 5,        /* the Langevin normals in use (float4 [random_size]; only with Langevin particles) */
    VVHIP_CKPT_THERMOSTAT = 6,    /* both parity copies of the device-resident thermostat state */
    VVHIP_CKPT_EPOCH = 7,         /* refill counter of the device Gaussian generator */
    VVHIP_CKPT_CURSOR = 8,        /* vvhip_checkpoint_cursor */
    VVHIP_CKPT_SECTIONS = 9
};
#define VVHIP_CKPT_MAGIC 0x504B435049485656ull      /* "VVHIPCKP" */
#define VVHIP_CKPT_VERSION 1
#define VVHIP_CKPT_ALL 0x1FFu                       /* mask of (1 << VVHIP_CKPT_*): every section in use */
/* everything but posq, correction, velm and force: what an OpenMM adapter stores next to the Context's own checkpoint */
#define VVHIP_CKPT_INTEGRATOR (VVHIP_CKPT_ALL & ~0xFu)
typedef struct {
    int32_t parity;                 /* which copy of the thermostat state the next application consumes */
    uint32_t random_pos;            /* prepareRandomNumbers cursor of the plan-driven loops */
    int32_t fextra_dirty, fextra_virtual;       /* forceExtra holds / should hold something since the last reset */
    int64_t step_count;             /* full steps counted since vvhip_bind */
    uint64_t rng_seed;              /* vvhip_set_random_seed */
} vvhip_checkpoint_cursor;
typedef struct {
    uint64_t magic;                 /* VVHIP_CKPT_MAGIC */
    uint32_t version;               /* VVHIP_CKPT_VERSION */
    int32_t precision;              /* VVHIP_SINGLE / MIXED / DOUBLE */
    int32_t num_atoms, shard_begin, shard_end, use_middle_scheme;
    int32_t num_nh_chains;
    uint32_t random_size;           /* float4 elements of the bound random buffer */
    double box[3];
    vvhip_params params;            /* as they stood at the save; NOT applied by a load */
    vvhip_checkpoint_cursor cursor;
    uint64_t host_words[4];         /* the host's own words (the stand-alone Context: its random index and "forces valid") */
    uint32_t num_sections, reserved;
    uint64_t total_bytes;
    uint64_t header_digest;
} vvhip_checkpoint_header;
typedef struct {
    uint32_t id, reserved;          /* VVHIP_CKPT_* */
    uint64_t offset, bytes;         /* of the payload, from the blob's start */
    uint64_t digest_base, digest;
} vvhip_checkpoint_section;
int vvhip_digest_host(const void* data, size_t bytes, uint64_t base, uint64_t* out);
/* Settles a pending recovery, synchronises, digests every section on the device (the cursor on the host) and copies the words back;
 * sections not in use (no correction outside mixed precision, no normals without Langevin particles) report 0.  Reads the state and
 * writes scratch of its own: no accumulator, thermostat copy, status word or captured graph is touched.  Refused inside a graph capture. */
int vvhip_state_digest(vvhip_plan* plan, uint64_t out[VVHIP_CKPT_SECTIONS]);
/* Bytes of the blob vvhip_checkpoint_save writes for this mask of sections (the cursor section is always carried). */
int vvhip_checkpoint_size(vvhip_plan* plan, uint32_t sections, size_t* bytes);
/* Enters as vvhip_synchronize does (a missed rendezvous is repaired first); with a sticky status word up it returns that error and
 * writes nothing: a void state is never saved.  Then: device digests, download, host digests of the downloaded bytes (a difference is
 * VVHIP_ERR_HIP), table and header last.  host_words may be NULL (zeros). */
int vvhip_checkpoint_save(vvhip_plan* plan, uint32_t sections, const uint64_t host_words[4], void* blob, size_t bytes);
/* Host only, no plan, safe on arbitrary bytes: bounds, magic, version, the table's sanity and every digest.  Any failure is
 * VVHIP_ERR_INVALID with a text that names the fault and the section (vvhip_checkpoint_error).  out may be NULL. */
int vvhip_checkpoint_inspect(const void* blob, size_t bytes, vvhip_checkpoint_header* out);
/* The text of this thread's last failed vvhip_checkpoint_inspect ("" if none). */
const char* vvhip_checkpoint_error(void);
/* Inspects the blob, compares its structure with the plan (precision, num_atoms, shard, scheme, chain length, random_size with Langevin
 * particles, section sizes: VVHIP_ERR_INVALID saying which), then uploads the sections present into the live arrays, zeroes both
 * accumulator copies and ALL rendezvous words (a plan may go BACK: words of later steps must not meet a restored tag), sets cursor, seed
 * and box, invalidates mass tables, the recovery snapshot and the captured graphs, and verifies vvhip_state_digest against the table
 * (VVHIP_ERR_HIP otherwise).  Refused: inside a graph capture; while a series is running (VVHIP_ERR_INVALID: stop it, load, start it
 * again -- its first row belongs to the old step counter), and likewise while a frame recorder is running; on a sharded plan or one with a communicator / mailbox
 * (VVHIP_ERR_UNSUPPORTED: the peers' exchange counters would have to move together).  A load that fails before its first upload leaves
 * the device state untouched.  The status words and the plan's tuning are left alone: a host that returns to a checkpoint after an
 * error calls vvhip_status_clear itself.  host_words_out may be NULL. */
int vvhip_checkpoint_load(vvhip_plan* plan, const void* blob, size_t bytes, uint64_t host_words_out[4]);

/* Device pointer of the plan-owned forceExtra array (real3[n]); getForceExtra() of the reference
 * (CudaVVKernels.h:86-88). */
int vvhip_force_extra(vvhip_plan* plan, void** device_ptr);

/* ---------------------------------------------------------------- stand-alone host support
 * NOT part of the reference path: lets a host without OpenMM (tests, bench.py) own device memory and
 * produce forces.  vvhip_synth_tether_force writes F = -k_t (x - site) on every massive particle plus a
 * Drude-parent spring -k_d (x_d - x_p), in OpenMM's fixed-point planar layout. */
int vvhip_device_count(int* count);
int vvhip_set_device(int device);
int vvhip_malloc(void** ptr, size_t bytes);
int vvhip_free(void* ptr);
int vvhip_memcpy_h2d(void* dst, const void* src, size_t bytes);
int vvhip_memcpy_d2h(void* dst, const void* src, size_t bytes);
int vvhip_memset(void* dst, int value, size_t bytes);
int vvhip_synchronize(vvhip_plan* plan);         /* hipStreamSynchronize + the sticky health check below */
/* Sticky health flags the kernels raise in pinned host memory (read without synchronising): a mailbox wait on the peers ran out
 * (VVHIP_ERR_EXCHANGE), a fixed-point accumulator left its range (VVHIP_ERR_OVERFLOW).  vvhip_run_graph / vvhip_run_eager refuse
 * to start and vvhip_synchronize returns the error once a flag is up; vvhip_status_clear resets them (after the host has
 * restored a valid state). */
int vvhip_status(vvhip_plan* plan, int32_t* mailbox_timed_out, int32_t* accumulator_overflow);
/* All four words: [0] mailbox wait ran out, [1] accumulator overflow, [2] the one-launch step's in-kernel rendezvous ran out
 * (VVHIP_ERR_RENDEZVOUS), [3] an in-kernel constraint cluster reached its iteration cap unconverged (VVHIP_ERR_CONSTRAINT). */
int vvhip_status_words(vvhip_plan* plan, int32_t words[4]);
int vvhip_status_clear(vvhip_plan* plan);
/* A missed rendezvous of the one-launch step ([2]: its blocks were not resident together within 0.2 s -- another process's kernels on the
 * device) is the one failure the plan-driven loops repair themselves.  vvhip_run_graph / vvhip_run_eager calls of >= 64 steps (test hook
 * "recover_min_steps") start from a device-side snapshot of the physical state (positions, correction, velocities, forces, extra forces,
 * both thermostat copies, the random generator's state), kept with the list of run calls since until a vvhip_synchronize has seen them end
 * well; the vvhip_synchronize that finds [2] raised instead puts the snapshot back, pins the plan to two launches per step (bit for bit
 * the same step; vvhip_fused_status: active = 0), repeats the calls, prints one line on stderr and returns VVHIP_OK -- the trajectory is
 * the one an undisturbed run gives.  Anything else that touches the plan in between (a split entry point, vvhip_set_params, ...) settles
 * the pending calls first.  Not in multi-GPU runs (every rank would have to repeat).  Without a snapshot (short calls, vvhip_step_* driven
 * by the host, "recover" = 0 / VVHIP_RECOVER=0) the failure is VVHIP_ERR_RENDEZVOUS as before, and the plan is pinned to two launches
 * all the same.  *recoveries: how often it has happened to this plan.  Reference contract: one context per device,
 * platforms/cuda/src/CudaVVKernelFactory.cpp:68. */
int vvhip_recovery_count(vvhip_plan* plan, int64_t* recoveries);
/* The middle scheme's step as ONE launch (kernels A and B around an in-kernel rendezvous of co-resident blocks): *active = 1 if
 * vvhip_step_middle takes it for this plan as it stands (a thermostat with <= 4 links, every tile a wave of its own on <= 256
 * co-resident blocks, no RCCL exchange between the halves, a kernel for the plan's pair of stage sets), *launches = fused launches
 * so far (captured ones count once), *wait_units = where the self-tuning wait between a block's publish and its first poll round
 * stands (units of 256 shader clocks; reading it synchronises).  vvhip_debug_tune(plan, "fused", 0) forces the two-launch step
 * (bit-identical results); "fused_poll_delay" >= 0 pins the wait.  Any of the three pointers may be NULL.
 * The classic scheme's two thermostat applications per step (vvhip_step_vv_first / _second) and vvhip_scale_velocity take the same kernel
 * under the same conditions -- sums, rendezvous, chain, scaling (+ half kick and drift / half kick in front) in one launch each, two per
 * classic step instead of four; they count in *launches, *active speaks of the middle scheme only. */
int vvhip_fused_status(vvhip_plan* plan, int32_t* active, int64_t* launches, int32_t* wait_units);
int vvhip_stream_create(void** stream);          /* hipStreamCreateWithFlags(non-blocking) */
int vvhip_stream_destroy(void* stream);
int vvhip_synth_tether_force(vvhip_plan* plan, const void* site /* real4[n] */, double k_tether, double k_drude);
/* Replays hipGraphs of `steps_per_graph` whole steps (optionally with the synthetic force kernel in front of each; both
 * schemes): floor(nsteps / steps_per_graph) replays, the remainder enqueued step by step; returns after enqueueing.  The
 * graph of the current thermostat parity is captured on first use (see vvhip_graph_prepare to do that up front). */
int vvhip_run_graph(vvhip_plan* plan, int nsteps, int steps_per_graph, const void* site, double k_tether, double k_drude);
/* Captures, instantiates and uploads that graph for BOTH thermostat parities WITHOUT launching anything (no-op for a parity
 * whose executable is already there).  The plan keeps one executable per parity, so a host that calls this after its warm-up
 * never pays a capture inside a timed region, whatever mix of replays and odd tails follows; vvhip_run_graph replays floor(nsteps / steps_per_graph) times and enqueues the remainder step by step. */
int vvhip_graph_prepare(vvhip_plan* plan, int steps_per_graph, const void* site, double k_tether, double k_drude);
/* Device Gaussian generator for stand-alone hosts (inside OpenMM the buffer and its refills are OpenMM's): Philox4x32-10 +
 * Box-Muller.  vvhip_fill_random refills the bound random buffer; the vvhip_run_* loops refill it themselves whenever a step's
 * slice (max(normalLD,1) + 2 max(pairsLD,1) float4, HOST:806-807,863) no longer fits, and at the start of every captured graph. */
int vvhip_set_random_seed(vvhip_plan* plan, uint64_t seed);
int vvhip_fill_random(vvhip_plan* plan);
/* The same steps enqueued one by one from C (no graph): fallback when graph capture is not wanted. */
int vvhip_run_eager(vvhip_plan* plan, int nsteps, const void* site, double k_tether, double k_drude);
/* ... and through the per-KernelImpl entry points in VVIntegrator::stepMiddle's order: the launches of the un-fused drop-in path
 * (what a host with its own constraint solver between the stages pays, the solver's launches excluded). */
int vvhip_run_eager_unfused(vvhip_plan* plan, int nsteps, const void* site, double k_tether, double k_drude);
/* HIP-event timing of the dominant kernels on the plan's stream, for bench.py's roofline block. */
/* Average duration of `reps` back-to-back launches of one stage kernel (0 = A, 1 = B) with the given stage bits,
 * bracketed by two HIP events on the plan's stream.  Destroys the physical state (timing only). */
int vvhip_time_kernel(vvhip_plan* plan, int kernel, uint32_t flags, int reps, double* ms_per_launch);
/* Tracing: roctx ranges around every launch group (visible with rocprofv3 --marker-trace); the OpenMM adapter switches it on with
 * VVIntegrator::setDebugEnabled and prints the reference's per-call lines itself (VVIntegrator.h:417-419, CudaVVKernels.cpp:57,120,...).
 * Also VVHIP_ROCTX=1 in the environment.  libroctx64 is resolved at run time. */
int vvhip_set_trace(vvhip_plan* plan, int enable);
/* Every stage set a plan launches runs a kernel compiled for exactly its stage bits.  The reference compiles its kernels per System at
 * run time (CudaVVKernels.cpp:98-101, 639-647); here the stage sets of the BASELINE configurations (+- constraints, classic scheme,
 * sharded, large boxes) are compiled into the library (vv_kernels.hip: SF_*), and a stage set outside that list -- or a thermostat chain
 * of 1, 2 or 4 links instead of the integrator's default 3 -- is compiled by hipRTC from the same source with the same options the first
 * time a plan launches it (csrc/vv_rtc.cpp; ~1 s per kernel, once per process; VVHIP_RTC below).  Only if that is switched off or fails
 * (libhiprtc.so missing; one line on stderr) does the generic kernel with run-time stage bits run, 15-20 % slower:
 * counts[0 / 1] = enqueued launches of kernel A / B of this plan that did (a launch captured into a graph counts once), stage_sets = the
 * last stage bits that did.  tests/test_gpu_specialised.py asserts 0 for every BASELINE configuration +- constraints, classic scheme,
 * sharded, and for stage sets outside the compiled list.  VVHIP_WARN_GENERIC=1 prints them as they happen. */
int vvhip_generic_launches(vvhip_plan* plan, int64_t counts[2], uint32_t stage_sets[2]);
/* Process-wide: counts[0] = kernels compiled at run time so far, counts[1 / 2] = enqueued launches of kernel A / B that ran one;
 * compile_seconds (optional) = time spent in the compiler. */
int vvhip_rtc_stats(int64_t counts[3], double* compile_seconds);
/* Process-wide: stage sets whose run-time compilation FAILED (no compiler library, a compile error); their launches run the generic
 * kernel (15-20 % slower) for the rest of the process.  One line on stderr each; hosts that report performance should look here. */
int vvhip_rtc_failures(int64_t* failed);
/* Sets VVHIP_RTC's value for the launches that follow (process-wide; graphs captured earlier keep their kernels) and returns the previous
 * one; mode < 0 only returns it. */
int vvhip_rtc_mode(int mode);
/* Per-launch timing of eager (not captured) launches, summed per class until vvhip_timing_read.  Kernels A and B: the dispatch's own
 * begin / end timestamps (hipExtLaunchKernel with start / stop events: nothing is added to the stream; what rocprofv3's kernel trace
 * reports).  enable = 1: everything else ("other": force provider, chain launch, collectives) bracketed by recorded events as well;
 * enable = 2: kernels A and B only, so that the stream holds exactly what an untimed run enqueues; enable = n > 2: as 2, with n events
 * created now instead of during the timed launches.  0 switches it off. */
int vvhip_timing_enable(vvhip_plan* plan, int enable);
int vvhip_timing_read(vvhip_plan* plan, double* ms_pass_a, double* ms_pass_b, double* ms_other, int32_t launches[3]);

/* ---------------------------------------------------------------- environment (read once, at vvhip_plan_create)
 * Behaviour switches, all optional.  (The tuning switches of rounds 1-3 -- launch shape, mass tables, velocity round trip, cos moments --
 * are closed experiments, TUNING_LOG.md; what tests still need of them is the per-plan hook vvhip_debug_tune below.)
 *   VVHIP_PERIODIC=1|0        arithmetic work-item layout (vv_host.hpp: PeriodicLayout) always / never; default: from 1.1 M lanes, when the
 *                             system is runs of identical molecules (vvhip_plan_info.periodic_layout tells)
 *   VVHIP_PERIODIC_DEBUG=1    the decomposition into regions and why the layout was (not) enabled, on stderr
 *   VVHIP_FUSED=0             the middle scheme's step (and each thermostat application of the classic scheme) as TWO launches also where the one-launch step (kernels A and B around an in-kernel
 *                             rendezvous of co-resident blocks; vvhip_fused_status) would be taken -- for a GPU that other processes compute
 *                             on at the same time: blocks that are not resident together meet the rendezvous' 0.2 s bound
 *                             (VVHIP_ERR_RENDEZVOUS).  Same results bit for bit
 *   VVHIP_SHAKE_MODE=0        hydrogen-type constraint clusters by Gauss-Seidel sweeps of the central lane (OpenMM's iteration; generic
 *                             kernels) instead of the direct velocity solve / coupled Newton iteration of all lanes of a cluster
 *   VVHIP_ROCTX=1             roctx ranges (see vvhip_set_trace)
 *   VVHIP_RTC=0|1|2           run-time compilation of kernels A / B (vvhip_generic_launches): never / for stage sets without a compiled
 *                             kernel (default) / for every launch (tests: the run-time kernel against the compiled one, bit for bit)
 *   VVHIP_STALL=us[:period]   race detection by timing: every period-th launch of a plan is preceded by a host sleep of `us` microseconds (the GPU
 *                             drains; whatever was only ordered by the depth of the queue lands differently); tests/test_gpu_stalls.py
 *   VVHIP_RTC_VERBOSE=1       one line on stderr per kernel compiled at run time;  VVHIP_RTC_DENY="A:0x441,B:*": these stage sets stay on the
 *                             generic kernel (bisecting)
 *   VVHIP_WARN_GENERIC=1      one line on stderr per stage set that runs on the generic kernel (15-20 % slower)
 * and in the OpenMM adapters (platforms/hip): VVHIP_PLUGIN_DEFER=0 -- run every KernelImpl call as its own launch(es) instead of answering a
 * completed stage-by-stage sequence with the fused step. */

/* ---------------------------------------------------------------- test hooks
 * Used by tests/ to drive single stages against the oracle; not needed by an integrating host.
 * kernel: 0 = A (produce), 1 = B (consume), 2 = chain; flags are the stage bits of csrc/vv_args.hpp. */
int vvhip_debug_launch(vvhip_plan* plan, int kernel, uint32_t flags, uint32_t random_index);
/* One of the plan's tuning choices by name (call between vvhip_plan_create and vvhip_bind; later calls drop the captured graphs):
 * "grid_cap_a" / "grid_cap_b" (most blocks per launch), "block_threads", "split_chain_waves" (the chain becomes its own launch from n waves
 * on), "periodic_kernels" / "periodic_a" (0: load slot words although the layout is arithmetic), "rekick", "no_moments", "mass_tab_a" /
 * "periodic_b", "mass_tab_b", "acc_store", "fused" (0: the middle scheme's step as two launches also where one would do), "fused_poll_delay" (>= 0 pins the wait in front of the rendezvous' first poll round, units of 256 clocks; -1: self-tuning), "fused_late_shift", "gc_omega_permille" (relaxation factor of the general clusters' sweeps x 1000, for rate scans).  Tests
 * use it to run large-system code paths at small sizes. */
int vvhip_debug_tune(vvhip_plan* plan, const char* key, int value);
int vvhip_debug_read_accumulators(vvhip_plan* plan, double out[4], int zero_after);  /* blocks */
int vvhip_debug_set_scales(vvhip_plan* plan, const double scales[4]);                /* vscale[3], bias V; blocks */
int vvhip_debug_timestamps(vvhip_plan* plan, uint32_t flags, int block, long long out[128]);  /* instrumented builds only (tools/probes) */
int vvhip_debug_timestamps_fused(vvhip_plan* plan, int block, long long out[128]);            /* ... one real one-launch step, stamped */
int vvhip_debug_span(vvhip_plan* plan, int kernel, uint32_t flags, int reps, double out[8]);   /* instrumented builds only */
int vvhip_debug_fused_flags(vvhip_plan* plan, int kernel, uint32_t* flags);          /* stage bits of the fused middle step's kernel A (0) / B (1) */
/* The launch shape the plan chose (host-only: before vvhip_bind a whole MI355X of 256 CUs is assumed): shape[0] = threads of the tile waves of a
 * block (the one-launch step and kernel B add the block's thermostat wave), shape[1] / shape[2] = most blocks per launch of kernel A / kernel B,
 * shape[3] = tile waves per block of the one-launch step, 0 where the launch shape rules it out (its other conditions: vvhip_fused_status). */
int vvhip_debug_launch_shape(const vvhip_plan* plan, int32_t shape[4]);
int vvhip_debug_step_spans(vvhip_plan* plan, int nsteps, const void* site, double k_tether, double k_drude, double out[36]);   /* instrumented builds only */
int vvhip_debug_old_delta(vvhip_plan* plan, void** device_ptr);                       /* plan-owned oldDelta (mixed4[n]) */
/* What all plans of this process own at this moment: count = device, uncached and pinned buffers and hipIpc mappings, bytes = of the
 * buffers.  Process-wide counters of the owners themselves (csrc/vv_devmem.hpp), so a test can see that a destroyed plan has returned
 * everything without watching the device's free memory, which moves under other processes' work.  Host only. */
int vvhip_debug_live_buffers(int64_t* count, int64_t* bytes);
/* FNV-1a 64 over the host tables that the last accepted vvhip_<name>_start built, name = "profile", "msd", "rdf", "current", "modes",
 * "contacts", "acf", "vanhove", "vanhove_distinct" or "sdf"; 0 when nothing is described.  Host only, an unbound plan included (it keeps a description that passed the checks).
 * Per vector its size as uint64, then its bytes; flags as one byte; in this order:
 *   profile   grouped, index, group, mass                 msd, acf   grouped, index, first, weight, total, group
 *   rdf       index, mol, items, max_jsites (int32)       current    two_level, index, weight, group
 *   modes     index, weight, modes, items                 contacts   first[0 .. 16], index, mol, mask_items, corr_items, then the fields
 *                                                                    of the word layout (csrc/vv_layout.h: ContactsLayout) one by one
 *   vanhove   grouped, index, first, weight, total, group (as msd), then e2       vanhove_distinct   as rdf
 *   sdf       index, mol, frames, fmol, fgroup, items, max_jsites (int32) */
int vvhip_debug_recorder_digest(const vvhip_plan* plan, const char* name, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* VVHIP_H */
