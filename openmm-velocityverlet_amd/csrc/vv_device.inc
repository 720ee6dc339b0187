// vv_device.inc -- the device code of libvvhip (gfx950, wave64): every __device__ function and __global__ kernel, included inside
// namespace vv by vv_kernels.hip (ahead-of-time build: the compiled list of stage sets and the generic kernels) and by the translation
// unit vv_rtc.cpp hands to hipRTC (one kernel for a stage set outside that list, compiled when a plan first needs it -- what the
// reference does for every System, CudaVVKernels.cpp:98-101, 639-647).  Needs vv_args.hpp; no host code, no host headers.
// The device code in parts (round 6; one translation unit as before -- hipRTC gets the parts flattened into one source, embed_sources.py):
#include "vv_dev_wave.inc"
#include "vv_dev_constraints.inc"
#include "vv_dev_sites.inc"
#include "vv_dev_mailbox.inc"
#include "vv_dev_langevin.inc"
#include "vv_dev_kernel_a.inc"
#include "vv_dev_chain.inc"
#include "vv_dev_kernel_b.inc"
#include "vv_dev_misc.inc"
#include "vv_dev_report.inc"
#include "vv_dev_cmm.inc"
#include "vv_dev_barostat.inc"
#include "vv_dev_thermalize.inc"
#include "vv_dev_digest.inc"
#include "vv_dev_frames.inc"
#include "vv_dev_profile.inc"
#include "vv_dev_msd.inc"
#include "vv_dev_rdf.inc"
#include "vv_dev_current.inc"
#include "vv_dev_modes.inc"
#include "vv_dev_contacts.inc"
#include "vv_dev_acf.inc"
#include "vv_dev_vanhove.inc"
#include "vv_dev_vanhove_distinct.inc"
