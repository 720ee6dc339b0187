"""ctypes binding of lib/libvvhip.so (C ABI: include/vvhip.h).  Pure plumbing: no arithmetic here.

The library is looked up in-tree (``openmm-velocityverlet_amd/lib/libvvhip.so``, built by
``__graft_entry__.build()`` / ``make -C openmm-velocityverlet_amd/csrc``).  If it is missing the
import of this module fails loudly -- there is no Python or CPU fallback for the hot path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# VVHIP_LIB: another build of the same library (A/B runs of two builds on one GPU box, tools/probes); default: the in-tree one
LIB_PATH = os.environ.get("VVHIP_LIB") or os.path.join(HERE, "lib", "libvvhip.so")

MAX_CHAINS = 8
SINGLE, MIXED, DOUBLE = 0, 1, 2
PRECISION = {"single": SINGLE, "mixed": MIXED, "double": DOUBLE}
REAL = {"single": np.float32, "mixed": np.float32, "double": np.float64}
MIXED_T = {"single": np.float32, "mixed": np.float64, "double": np.float64}
OK, ERR_INVALID, ERR_TOPOLOGY, ERR_UNSUPPORTED, ERR_HIP, ERR_NO_DEVICE, ERR_EXCHANGE, ERR_OVERFLOW, ERR_RENDEZVOUS, ERR_CONSTRAINT = 0, -1, -2, -3, -4, -5, -6, -7, -8, -9

# stage bits of csrc/vv_args.hpp (only the test hooks need them)
A_FE_LOAD, A_FE_STORE, A_LD, A_EF, A_COS, A_KICK_FULL, A_KICK_HALF, A_POSDELTA_VV, A_POS1, A_BIAS, A_KE, A_UNBIAS_ACC, A_COMPART, A_CZ_STORE, A_CZ_LOAD = \
    [1 << i for i in range(15)]
B_SCALE, B_UNBIAS, B_BIAS_REMOVE, B_BIAS_RESTORE, B_DRIFT_MIDDLE, B_POS2, B_POS3, B_VV_KICK, B_VV_POS, B_HARDWALL, B_IMAGE, B_CHAIN, B_CZ_LOAD = \
    [1 << i for i in range(13)]
A_MTAB, B_MTAB = 1 << 18, 1 << 16        # static mass tables: added by the library itself (vv_launch.cpp run_a / run_b)
C_CHAIN, C_BIAS = 1, 2


class VVHipError(RuntimeError):
    """Stands in for OpenMMException on the Python side; `.code` is the vvhip error code."""

    def __init__(self, code, message):
        super().__init__(f"[vvhip {code}] {message}")
        self.code = code
        self.message = message


class SystemDesc(C.Structure):
    _fields_ = [("num_atoms", C.c_int32), ("padded_num_atoms", C.c_int32), ("masses", C.c_void_p), ("mol_id", C.c_void_p),
                ("num_molecules", C.c_int32), ("num_drude_pairs", C.c_int32), ("drude_pairs", C.c_void_p),
                ("num_constraints", C.c_int32), ("constraints", C.c_void_p), ("has_cm_motion_remover", C.c_int32),
                ("num_particles_ld", C.c_int32), ("particles_ld", C.c_void_p),
                ("num_image_pairs", C.c_int32), ("image_pairs", C.c_void_p),
                ("num_electrolyte", C.c_int32), ("particles_electrolyte", C.c_void_p),
                ("shard_begin", C.c_int32), ("shard_end", C.c_int32), ("constraint_distances", C.c_void_p),
                ("num_virtual_sites", C.c_int32), ("virtual_sites", C.c_void_p), ("virtual_site_params", C.c_void_p)]


VSITE_AVERAGE2, VSITE_AVERAGE3, VSITE_OUT_OF_PLANE, VSITE_LOCAL_COORDS = 0, 1, 2, 3


class Params(C.Structure):
    _fields_ = [("temperature", C.c_double), ("frequency", C.c_double), ("drude_temperature", C.c_double),
                ("drude_frequency", C.c_double), ("step_size", C.c_double),
                ("num_nh_chains", C.c_int32), ("loops_per_step", C.c_int32),
                ("max_drude_distance", C.c_double), ("friction", C.c_double), ("drude_friction", C.c_double),
                ("mirror_location", C.c_double), ("electric_field", C.c_double), ("cos_acceleration", C.c_double),
                ("use_com_temp_group", C.c_int32), ("use_middle_scheme", C.c_int32),
                ("auto_set_com_temp_group", C.c_int32), ("auto_set_friction", C.c_int32), ("constraint_tolerance", C.c_double)]


class Buffers(C.Structure):
    _fields_ = [("velm", C.c_void_p), ("posq", C.c_void_p), ("posq_correction", C.c_void_p), ("force", C.c_void_p),
                ("pos_delta", C.c_void_p), ("random", C.c_void_p), ("random_size", C.c_uint32), ("stream", C.c_void_p)]


class PlanInfo(C.Structure):
    _fields_ = [("num_particles_nh", C.c_int32), ("num_molecules_nh", C.c_int32), ("num_normal_nh", C.c_int32),
                ("num_pairs_nh", C.c_int32), ("num_normal_ld", C.c_int32), ("num_pairs_ld", C.c_int32),
                ("num_images", C.c_int32), ("num_electrolyte", C.c_int32), ("num_temp_groups", C.c_int32),
                ("use_com_temp_group", C.c_int32), ("friction", C.c_double),
                ("dof", C.c_double * 3), ("nkbt", C.c_double * 3), ("eta_mass", (C.c_double * MAX_CHAINS) * 3),
                ("inv_mass_total", C.c_double), ("num_waves", C.c_int32), ("num_slots_used", C.c_int32),
                ("max_cluster", C.c_int32), ("num_shake_clusters", C.c_int32), ("constraints_fused", C.c_int32),
                ("num_settle_clusters", C.c_int32), ("periodic_layout", C.c_int32), ("num_general_constraints", C.c_int32),
                ("num_virtual_sites", C.c_int32), ("general_relaxation", C.c_double)]


class NHState(C.Structure):
    _fields_ = [("eta", (C.c_double * MAX_CHAINS) * 3), ("eta_dot", (C.c_double * (MAX_CHAINS + 1)) * 3),
                ("eta_dotdot", (C.c_double * MAX_CHAINS) * 3), ("ke2", C.c_double * 3), ("vscale", C.c_double * 3),
                ("v_bias", C.c_double)]


SERIES_DRUDE, SERIES_THERMOSTAT = 1, 2


class SeriesRow(C.Structure):
    """One row of a device-side series (include/vvhip.h: vvhip_series_row)."""
    _fields_ = [("drude_raw", C.c_int64 * 6), ("drude_overflow", C.c_int64), ("reserved", C.c_int64), ("nh", NHState),
                ("box", C.c_double * 3), ("cos_acceleration", C.c_double)]


class SeriesLayout(C.Structure):
    _fields_ = [("row_bytes", C.c_int32), ("off_drude_raw", C.c_int32), ("off_nh", C.c_int32), ("off_box", C.c_int32),
                ("active", C.c_int32), ("interval", C.c_int32), ("capacity", C.c_int32), ("mask", C.c_int32),
                ("steps", C.c_int64), ("graph_captures", C.c_int64)]


FRAMES_POSITIONS, FRAMES_VELOCITIES, FRAMES_FLOAT64 = 1, 2, 4
FRAMES_LINEAR, FRAMES_LOG10 = 0, 1


class FramesDesc(C.Structure):
    """What a frame recorder is to record (include/vvhip.h: vvhip_frames_desc)."""
    _fields_ = [("interval", C.c_int32), ("schedule", C.c_int32), ("capacity", C.c_int32), ("mask", C.c_int32),
                ("num_subset", C.c_int32), ("subset", C.c_void_p)]


class FrameHeader(C.Structure):
    """The 64 bytes in front of every frame, written on the device (include/vvhip.h: vvhip_frame_header)."""
    _fields_ = [("ordinal", C.c_int64), ("reserved", C.c_int64), ("box", C.c_double * 3), ("pad", C.c_double * 3)]


class FramesLayout(C.Structure):
    _fields_ = [("active", C.c_int32), ("interval", C.c_int32), ("schedule", C.c_int32), ("capacity", C.c_int32), ("mask", C.c_int32),
                ("num_particles", C.c_int32), ("component_bytes", C.c_int32), ("plane_stride", C.c_int32),
                ("frame_bytes", C.c_int64), ("off_positions", C.c_int64), ("off_velocities", C.c_int64), ("start_step", C.c_int64)]


PROFILE_COUNT, PROFILE_CHARGE, PROFILE_MASS, PROFILE_MOMENTUM, PROFILE_KINETIC = 1, 2, 4, 8, 16
PROFILE_QUANTITIES = ("count", "charge", "mass", "momentum", "kinetic")      # quantity q has mask bit 1 << q


class ProfileDesc(C.Structure):
    """What a profile recorder is to accumulate (include/vvhip.h: vvhip_profile_desc)."""
    _fields_ = [("interval", C.c_int32), ("axis", C.c_int32), ("nbins", C.c_int32), ("mask", C.c_int32), ("num_groups", C.c_int32),
                ("reserved", C.c_int32), ("group", C.c_void_p), ("max_samples", C.c_int64), ("limit", C.c_double * 4)]


class ProfileCounts(C.Structure):
    _fields_ = [("samples", C.c_int64), ("dropped", C.c_int64), ("out_of_range", C.c_int64)]


class ProfileLayout(C.Structure):
    _fields_ = [("active", C.c_int32), ("interval", C.c_int32), ("axis", C.c_int32), ("nbins", C.c_int32), ("mask", C.c_int32),
                ("num_groups", C.c_int32), ("num_particles", C.c_int32), ("rows", C.c_int32), ("max_samples", C.c_int64),
                ("words", C.c_int64), ("start_step", C.c_int64), ("row_of", C.c_int32 * 5), ("frac_bits", C.c_int32 * 5),
                ("limit", C.c_double * 5)]


MSD_PARTICLES, MSD_MOLECULES = 0, 1


class MsdDesc(C.Structure):
    """What an MSD recorder is to accumulate (include/vvhip.h: vvhip_msd_desc)."""
    _fields_ = [("interval", C.c_int32), ("num_lags", C.c_int32), ("origin_every", C.c_int32), ("mode", C.c_int32), ("num_groups", C.c_int32),
                ("reserved", C.c_int32), ("group", C.c_void_p), ("max_samples", C.c_int64), ("limit", C.c_double)]


class MsdCounts(C.Structure):
    _fields_ = [("samples", C.c_int64), ("dropped", C.c_int64), ("out_of_range", C.c_int64), ("origin_floor", C.c_int64)]


class MsdLayout(C.Structure):
    _fields_ = [("active", C.c_int32), ("interval", C.c_int32), ("num_lags", C.c_int32), ("origin_every", C.c_int32), ("mode", C.c_int32),
                ("num_groups", C.c_int32), ("num_units", C.c_int32), ("num_origins", C.c_int32), ("frac_bits", C.c_int32),
                ("reserved", C.c_int32), ("max_samples", C.c_int64), ("words", C.c_int64), ("ring_bytes", C.c_int64),
                ("start_step", C.c_int64), ("limit", C.c_double)]


class RdfDesc(C.Structure):
    """What an RDF recorder is to accumulate (include/vvhip.h: vvhip_rdf_desc)."""
    _fields_ = [("interval", C.c_int32), ("nbins", C.c_int32), ("num_groups", C.c_int32), ("num_classes", C.c_int32),
                ("exclude_same_molecule", C.c_int32), ("reserved", C.c_int32), ("group", C.c_void_p), ("classes", C.c_void_p),
                ("max_samples", C.c_int64), ("r_max", C.c_double)]


class RdfCounts(C.Structure):
    _fields_ = [("samples", C.c_int64), ("dropped", C.c_int64), ("invalid", C.c_int64), ("inv_volume_sum", C.c_double)]


class RdfLayout(C.Structure):
    _fields_ = [("active", C.c_int32), ("interval", C.c_int32), ("nbins", C.c_int32), ("num_groups", C.c_int32), ("num_classes", C.c_int32),
                ("exclude_same_molecule", C.c_int32), ("tile", C.c_int32), ("num_items", C.c_int32), ("num_sites", C.c_int32 * 16),
                ("classes", (C.c_int32 * 2) * 32), ("pairs_per_sample", C.c_int64 * 32), ("max_samples", C.c_int64), ("words", C.c_int64),
                ("scratch_bytes", C.c_int64), ("start_step", C.c_int64), ("r_max", C.c_double), ("dr", C.c_double)]


class CurrentDesc(C.Structure):
    """What a current recorder is to accumulate (include/vvhip.h: vvhip_current_desc)."""
    _fields_ = [("interval", C.c_int32), ("num_lags", C.c_int32), ("origin_every", C.c_int32), ("num_groups", C.c_int32),
                ("weight", C.c_void_p), ("group", C.c_void_p), ("max_samples", C.c_int64), ("limit_position", C.c_double),
                ("limit_velocity", C.c_double)]


class CurrentCounts(C.Structure):
    _fields_ = [("samples", C.c_int64), ("dropped", C.c_int64), ("out_of_range", C.c_int64), ("invalid_samples", C.c_int64),
                ("origin_floor", C.c_int64), ("inv_volume_sum", C.c_double)]


class CurrentLayout(C.Structure):
    _fields_ = [("active", C.c_int32), ("interval", C.c_int32), ("num_lags", C.c_int32), ("origin_every", C.c_int32), ("num_groups", C.c_int32),
                ("num_particles", C.c_int32), ("num_origins", C.c_int32), ("num_disp_classes", C.c_int32), ("num_cur_classes", C.c_int32),
                ("row_words", C.c_int32), ("frac_bits_position", C.c_int32), ("frac_bits_velocity", C.c_int32), ("max_samples", C.c_int64),
                ("words", C.c_int64), ("ring_bytes", C.c_int64), ("start_step", C.c_int64), ("limit_position", C.c_double),
                ("limit_velocity", C.c_double), ("weight_bound", C.c_double)]


class ModesDesc(C.Structure):
    """What a density-mode recorder is to accumulate (include/vvhip.h: vvhip_modes_desc)."""
    _fields_ = [("interval", C.c_int32), ("num_lags", C.c_int32), ("origin_every", C.c_int32), ("num_groups", C.c_int32),
                ("num_modes", C.c_int32), ("weight", C.c_void_p), ("group", C.c_void_p), ("modes", C.c_void_p),
                ("max_samples", C.c_int64), ("limit_position", C.c_double)]


class ModesCounts(C.Structure):
    _fields_ = [("samples", C.c_int64), ("dropped", C.c_int64), ("out_of_range", C.c_int64), ("invalid_samples", C.c_int64),
                ("origin_floor", C.c_int64), ("box_sum", C.c_double * 3)]


class ModesLayout(C.Structure):
    _fields_ = [("active", C.c_int32), ("interval", C.c_int32), ("num_lags", C.c_int32), ("origin_every", C.c_int32), ("num_groups", C.c_int32),
                ("num_modes", C.c_int32), ("num_particles", C.c_int32), ("num_origins", C.c_int32), ("row_words", C.c_int32),
                ("frac_bits", C.c_int32), ("group_sites", C.c_int32 * 8), ("num_items", C.c_int32), ("sites_per_thread", C.c_int32),
                ("k_tile", C.c_int32), ("block_threads", C.c_int32), ("max_samples", C.c_int64), ("words", C.c_int64),
                ("ring_bytes", C.c_int64), ("scratch_bytes", C.c_int64), ("start_step", C.c_int64), ("limit_position", C.c_double),
                ("weight_bound", C.c_double)]


class ContactsDesc(C.Structure):
    """What a contact recorder is to accumulate (include/vvhip.h: vvhip_contacts_desc)."""
    _fields_ = [("interval", C.c_int32), ("num_lags", C.c_int32), ("origin_every", C.c_int32), ("num_groups", C.c_int32),
                ("num_classes", C.c_int32), ("exclude_same_molecule", C.c_int32), ("continuous", C.c_int32), ("reserved", C.c_int32),
                ("group", C.c_void_p), ("classes", C.c_void_p), ("r_cut", C.c_void_p), ("max_samples", C.c_int64)]


class ContactsCounts(C.Structure):
    _fields_ = [("samples", C.c_int64), ("dropped", C.c_int64), ("invalid", C.c_int64)]


class ContactsLayout(C.Structure):
    _fields_ = [("active", C.c_int32), ("interval", C.c_int32), ("num_lags", C.c_int32), ("origin_every", C.c_int32), ("num_groups", C.c_int32),
                ("num_classes", C.c_int32), ("exclude_same_molecule", C.c_int32), ("continuous", C.c_int32), ("num_origins", C.c_int32),
                ("rows_per_tile", C.c_int32), ("words_per_item", C.c_int32), ("skip_zero_words", C.c_int32), ("num_mask_items", C.c_int32),
                ("num_corr_items", C.c_int32), ("num_sites", C.c_int32 * 16), ("classes", (C.c_int32 * 2) * 8), ("rows", C.c_int32 * 8),
                ("cols", C.c_int32 * 8), ("class_words", C.c_int64 * 8), ("sample_words", C.c_int64), ("max_samples", C.c_int64),
                ("words", C.c_int64), ("words_bytes", C.c_int64), ("scratch_bytes", C.c_int64), ("total_bytes", C.c_int64),
                ("start_step", C.c_int64), ("r_cut", C.c_double * 8)]


CONTACTS_MAX_BYTES = 1 << 32


ACF_VELOCITY_PARTICLES, ACF_VELOCITY_MOLECULES, ACF_ORIENTATION = 0, 1, 2


class AcfDesc(C.Structure):
    """What an autocorrelation recorder is to accumulate (include/vvhip.h: vvhip_acf_desc)."""
    _fields_ = [("interval", C.c_int32), ("num_lags", C.c_int32), ("origin_every", C.c_int32), ("mode", C.c_int32), ("num_groups", C.c_int32),
                ("num_pairs", C.c_int32), ("group", C.c_void_p), ("pairs", C.c_void_p), ("max_samples", C.c_int64), ("limit", C.c_double)]


class AcfCounts(C.Structure):
    _fields_ = [("samples", C.c_int64), ("dropped", C.c_int64), ("out_of_range", C.c_int64), ("origin_floor", C.c_int64)]


class AcfLayout(C.Structure):
    _fields_ = [("active", C.c_int32), ("interval", C.c_int32), ("num_lags", C.c_int32), ("origin_every", C.c_int32), ("mode", C.c_int32),
                ("num_groups", C.c_int32), ("num_units", C.c_int32), ("num_origins", C.c_int32), ("frac_bits", C.c_int32),
                ("row_words", C.c_int32), ("max_samples", C.c_int64), ("words", C.c_int64), ("ring_bytes", C.c_int64),
                ("start_step", C.c_int64), ("limit", C.c_double)]


VANHOVE_PARTICLES, VANHOVE_MOLECULES = 0, 1
VANHOVE_MAX_WORDS = 1 << 22


class VanHoveDesc(C.Structure):
    """What a self van Hove recorder is to accumulate (include/vvhip.h: vvhip_vanhove_desc)."""
    _fields_ = [("interval", C.c_int32), ("num_lags", C.c_int32), ("origin_every", C.c_int32), ("mode", C.c_int32), ("num_groups", C.c_int32),
                ("num_bins", C.c_int32), ("group", C.c_void_p), ("edges", C.c_void_p), ("max_samples", C.c_int64), ("limit", C.c_double)]


class VanHoveCounts(C.Structure):
    _fields_ = [("samples", C.c_int64), ("dropped", C.c_int64), ("out_of_range", C.c_int64), ("origin_floor", C.c_int64)]


class VanHoveLayout(C.Structure):
    _fields_ = [("active", C.c_int32), ("interval", C.c_int32), ("num_lags", C.c_int32), ("origin_every", C.c_int32), ("mode", C.c_int32),
                ("num_groups", C.c_int32), ("num_units", C.c_int32), ("num_origins", C.c_int32), ("num_bins", C.c_int32),
                ("frac2_bits", C.c_int32), ("r4_hi_bits", C.c_int32), ("r4_lo_bits", C.c_int32), ("max_samples", C.c_int64),
                ("words", C.c_int64), ("head_words", C.c_int64), ("hist_words", C.c_int64), ("ring_bytes", C.c_int64),
                ("start_step", C.c_int64), ("limit", C.c_double)]


VANHOVE_DISTINCT_MAX_WORDS = 1 << 22


class VanHoveDistinctDesc(C.Structure):
    """What a distinct van Hove recorder is to accumulate (include/vvhip.h: vvhip_vanhove_distinct_desc)."""
    _fields_ = [("interval", C.c_int32), ("num_lags", C.c_int32), ("origin_every", C.c_int32), ("nbins", C.c_int32),
                ("num_groups", C.c_int32), ("num_classes", C.c_int32), ("exclude_same_molecule", C.c_int32), ("reserved", C.c_int32),
                ("group", C.c_void_p), ("classes", C.c_void_p), ("max_samples", C.c_int64), ("r_max", C.c_double)]


class VanHoveDistinctCounts(C.Structure):
    _fields_ = [("samples", C.c_int64), ("dropped", C.c_int64), ("invalid", C.c_int64), ("origin_floor", C.c_int64)]


class VanHoveDistinctLayout(C.Structure):
    _fields_ = [("active", C.c_int32), ("interval", C.c_int32), ("num_lags", C.c_int32), ("origin_every", C.c_int32), ("nbins", C.c_int32),
                ("num_groups", C.c_int32), ("num_classes", C.c_int32), ("exclude_same_molecule", C.c_int32), ("tile", C.c_int32),
                ("num_items", C.c_int32), ("num_origins", C.c_int32), ("num_rows", C.c_int32), ("num_sites", C.c_int32 * 16),
                ("classes", (C.c_int32 * 2) * 32), ("pairs_per_sample", C.c_int64 * 32), ("max_samples", C.c_int64), ("words", C.c_int64),
                ("head_words", C.c_int64), ("hist_words", C.c_int64), ("ring_bytes", C.c_int64), ("start_step", C.c_int64),
                ("r_max", C.c_double), ("dr", C.c_double)]


SDF_MAX_WORDS = 1 << 23


class SdfDesc(C.Structure):
    """What a spatial distribution recorder is to accumulate (include/vvhip.h: vvhip_sdf_desc)."""
    _fields_ = [("interval", C.c_int32), ("nbins", C.c_int32), ("num_frames", C.c_int32), ("num_frame_groups", C.c_int32),
                ("num_site_groups", C.c_int32), ("num_classes", C.c_int32), ("exclude_same_molecule", C.c_int32), ("reserved", C.c_int32),
                ("frames", C.c_void_p), ("frame_group", C.c_void_p), ("site_group", C.c_void_p), ("classes", C.c_void_p),
                ("max_samples", C.c_int64), ("extent", C.c_double)]


class SdfCounts(C.Structure):
    _fields_ = [("samples", C.c_int64), ("dropped", C.c_int64), ("invalid", C.c_int64), ("bad_frames", C.c_int64),
                ("inv_volume_sum", C.c_double), ("frame_visits", C.c_int64 * 16)]


class SdfLayout(C.Structure):
    _fields_ = [("active", C.c_int32), ("interval", C.c_int32), ("nbins", C.c_int32), ("num_frame_groups", C.c_int32),
                ("num_site_groups", C.c_int32), ("num_classes", C.c_int32), ("exclude_same_molecule", C.c_int32), ("tile", C.c_int32),
                ("num_items", C.c_int32), ("reserved", C.c_int32), ("num_frames", C.c_int32 * 16), ("num_sites", C.c_int32 * 16),
                ("classes", (C.c_int32 * 2) * 16), ("pairs_per_sample", C.c_int64 * 16), ("max_samples", C.c_int64), ("words", C.c_int64),
                ("scratch_bytes", C.c_int64), ("start_step", C.c_int64), ("extent", C.c_double), ("voxel", C.c_double)]


class CmMotionRecord(C.Structure):
    """The record of the scheduled removals of the centre-of-mass motion (include/vvhip.h: vvhip_cm_motion_record)."""
    _fields_ = [("frequency", C.c_int32), ("reserved", C.c_int32), ("removals", C.c_int64), ("skipped", C.c_int64),
                ("last_v", C.c_double * 3), ("total_mass", C.c_double)]


THERMALIZE_NO_CONSTRAINTS, THERMALIZE_REMOVE_CM = 1, 2


class ThermalizeRecord(C.Structure):
    """What one draw of Maxwell-Boltzmann start velocities did (include/vvhip.h: vvhip_thermalize_record)."""
    _fields_ = [("drawn", C.c_int64), ("pairs_split", C.c_int64), ("zeroed", C.c_int64), ("constrained", C.c_int32),
                ("cm_removed", C.c_int32), ("v_removed", C.c_double * 3)]


class BarostatRecord(C.Structure):
    """What the plan knows of its barostat scales (include/vvhip.h: vvhip_barostat_record)."""
    _fields_ = [("molecules", C.c_int64), ("scales", C.c_int64), ("restores", C.c_int64), ("pending", C.c_int32),
                ("frac_bits", C.c_int32), ("box_before", C.c_double * 3), ("box_after", C.c_double * 3)]


CKPT_SECTION_NAMES = ("posq", "correction", "velm", "force", "force_extra", "random", "thermostat", "epoch", "cursor")
CKPT_SECTIONS = len(CKPT_SECTION_NAMES)
CKPT_MAGIC, CKPT_VERSION = 0x504B435049485656, 1
CKPT_ALL = (1 << CKPT_SECTIONS) - 1
CKPT_INTEGRATOR = CKPT_ALL & ~0xF


class CheckpointCursor(C.Structure):
    _fields_ = [("parity", C.c_int32), ("random_pos", C.c_uint32), ("fextra_dirty", C.c_int32), ("fextra_virtual", C.c_int32),
                ("step_count", C.c_int64), ("rng_seed", C.c_uint64)]


class CheckpointHeader(C.Structure):
    """The fixed header of a checkpoint blob (include/vvhip.h: vvhip_checkpoint_header)."""
    _fields_ = [("magic", C.c_uint64), ("version", C.c_uint32), ("precision", C.c_int32), ("num_atoms", C.c_int32),
                ("shard_begin", C.c_int32), ("shard_end", C.c_int32), ("use_middle_scheme", C.c_int32), ("num_nh_chains", C.c_int32),
                ("random_size", C.c_uint32), ("box", C.c_double * 3), ("params", Params), ("cursor", CheckpointCursor),
                ("host_words", C.c_uint64 * 4), ("num_sections", C.c_uint32), ("reserved", C.c_uint32), ("total_bytes", C.c_uint64),
                ("header_digest", C.c_uint64)]


class CheckpointSection(C.Structure):
    _fields_ = [("id", C.c_uint32), ("reserved", C.c_uint32), ("offset", C.c_uint64), ("bytes", C.c_uint64),
                ("digest_base", C.c_uint64), ("digest", C.c_uint64)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the hot path is HIP only; there is no fallback)")
    lib = C.CDLL(LIB_PATH)
    vp, i32, u32, dbl = C.c_void_p, C.c_int32, C.c_uint32, C.c_double
    P = C.POINTER
    sig = {
        "vvhip_plan_create": [P(SystemDesc), P(Params), C.c_int, P(vp), C.c_char_p, C.c_size_t],
        "vvhip_plan_get_info": [vp, P(PlanInfo)],
        "vvhip_plan_get_slots": [vp, vp, i32],
        "vvhip_bind": [vp, P(Buffers)],
        "vvhip_set_params": [vp, P(Params)],
        "vvhip_set_box": [vp, P(dbl * 3)],
        "vvhip_get_nh_state": [vp, P(NHState)],
        "vvhip_set_nh_state": [vp, P(NHState)],
        "vvhip_step_middle": [vp, u32],
        "vvhip_step_vv_first": [vp],
        "vvhip_step_vv_second": [vp, u32],
        "vvhip_step_middle_phases": [vp],
        "vvhip_algorithmic_bytes": [vp, P(i32), P(i32)],
        "vvhip_step_middle_phase": [vp, C.c_int, u32],
        "vvhip_accumulators": [vp, C.c_int, P(vp), P(i32)],
        "vvhip_reset_extra_force": [vp], "vvhip_middle_kick": [vp], "vvhip_middle_half_drift1": [vp],
        "vvhip_middle_half_drift2": [vp], "vvhip_middle_finish": [vp],
        "vvhip_vv_half_kick": [vp, C.c_int], "vvhip_vv_positions": [vp], "vvhip_scale_velocity": [vp],
        "vvhip_apply_langevin_force": [vp, u32], "vvhip_update_image_positions": [vp],
        "vvhip_apply_electric_force": [vp], "vvhip_apply_cosine_force": [vp], "vvhip_calc_velocity_bias": [vp],
        "vvhip_remove_velocity_bias": [vp], "vvhip_restore_velocity_bias": [vp],
        "vvhip_calc_viscosity": [vp, P(dbl), P(dbl)], "vvhip_compute_kinetic_energy": [vp, P(dbl)], "vvhip_force_extra": [vp, P(vp)],
        "vvhip_drude_temperatures": [vp, P(dbl * 3), P(dbl * 3)], "vvhip_drude_report_dof": [vp, P(dbl * 3)],
        "vvhip_drude_report_raw": [vp, P(C.c_int64 * 6)], "vvhip_drude_report_combine": [vp, P(C.c_int64 * 6), P(dbl * 3), P(dbl * 3)],
        "vvhip_series_start": [vp, i32, i32, i32], "vvhip_series_stop": [vp], "vvhip_series_info": [vp, P(SeriesLayout)],
        "vvhip_series_read": [vp, vp, i32, P(i32), P(C.c_int64), P(C.c_int64), i32], "vvhip_debug_series_guard": [vp, P(i32)],
        "vvhip_frames_start": [vp, P(FramesDesc)], "vvhip_frames_stop": [vp], "vvhip_frames_info": [vp, P(FramesLayout)],
        "vvhip_frames_read": [vp, vp, vp, i32, P(i32), P(C.c_int64), i32], "vvhip_frames_particles": [vp, vp, i32],
        "vvhip_frames_schedule": [i32, i32, C.c_int64, i32, vp], "vvhip_debug_frames_guard": [vp, P(i32)],
        "vvhip_profile_start": [vp, P(ProfileDesc)], "vvhip_profile_stop": [vp], "vvhip_profile_info": [vp, P(ProfileLayout)],
        "vvhip_profile_read": [vp, vp, C.c_int64, P(ProfileCounts), i32], "vvhip_debug_recover": [vp],
        "vvhip_msd_start": [vp, P(MsdDesc)], "vvhip_msd_stop": [vp], "vvhip_msd_info": [vp, P(MsdLayout)],
        "vvhip_msd_read": [vp, vp, C.c_int64, P(MsdCounts), i32],
        "vvhip_current_start": [vp, P(CurrentDesc)], "vvhip_current_stop": [vp], "vvhip_current_info": [vp, P(CurrentLayout)],
        "vvhip_current_read": [vp, vp, C.c_int64, P(CurrentCounts), i32],
        "vvhip_modes_start": [vp, P(ModesDesc)], "vvhip_modes_stop": [vp], "vvhip_modes_info": [vp, P(ModesLayout)],
        "vvhip_modes_read": [vp, vp, C.c_int64, P(ModesCounts), i32],
        "vvhip_rdf_start": [vp, P(RdfDesc)], "vvhip_rdf_sample": [vp], "vvhip_rdf_stop": [vp], "vvhip_rdf_info": [vp, P(RdfLayout)],
        "vvhip_rdf_read": [vp, vp, C.c_int64, P(RdfCounts), i32],
        "vvhip_contacts_start": [vp, P(ContactsDesc)], "vvhip_contacts_sample": [vp], "vvhip_contacts_stop": [vp],
        "vvhip_contacts_info": [vp, P(ContactsLayout)], "vvhip_contacts_read": [vp, vp, C.c_int64, P(ContactsCounts), i32],
        "vvhip_acf_start": [vp, P(AcfDesc)], "vvhip_acf_stop": [vp], "vvhip_acf_info": [vp, P(AcfLayout)],
        "vvhip_acf_read": [vp, vp, C.c_int64, P(AcfCounts), i32],
        "vvhip_vanhove_start": [vp, P(VanHoveDesc)], "vvhip_vanhove_stop": [vp], "vvhip_vanhove_info": [vp, P(VanHoveLayout)],
        "vvhip_vanhove_read": [vp, vp, C.c_int64, P(VanHoveCounts), i32],
        "vvhip_vanhove_distinct_start": [vp, P(VanHoveDistinctDesc)], "vvhip_vanhove_distinct_stop": [vp],
        "vvhip_vanhove_distinct_info": [vp, P(VanHoveDistinctLayout)],
        "vvhip_vanhove_distinct_read": [vp, vp, C.c_int64, P(VanHoveDistinctCounts), i32],
        "vvhip_sdf_start": [vp, P(SdfDesc)], "vvhip_sdf_sample": [vp], "vvhip_sdf_stop": [vp], "vvhip_sdf_info": [vp, P(SdfLayout)],
        "vvhip_sdf_read": [vp, vp, C.c_int64, P(SdfCounts), i32],
        "vvhip_cm_motion_start": [vp, i32], "vvhip_cm_motion_stop": [vp], "vvhip_remove_cm_motion": [vp, P(dbl * 3)],
        "vvhip_cm_motion_read": [vp, P(CmMotionRecord)],
        "vvhip_set_velocities_to_temperature": [vp, dbl, dbl, C.c_uint64, u32, P(ThermalizeRecord)],
        "vvhip_barostat_scale": [vp, P(dbl * 3)], "vvhip_barostat_restore": [vp], "vvhip_barostat_read": [vp, P(BarostatRecord)],
        "vvhip_digest_host": [vp, C.c_size_t, C.c_uint64, P(C.c_uint64)], "vvhip_state_digest": [vp, P(C.c_uint64 * CKPT_SECTIONS)],
        "vvhip_checkpoint_size": [vp, u32, P(C.c_size_t)], "vvhip_checkpoint_save": [vp, u32, P(C.c_uint64 * 4), vp, C.c_size_t],
        "vvhip_checkpoint_inspect": [vp, C.c_size_t, P(CheckpointHeader)], "vvhip_checkpoint_load": [vp, vp, C.c_size_t, P(C.c_uint64 * 4)],
        "vvhip_device_count": [P(C.c_int)], "vvhip_set_device": [C.c_int],
        "vvhip_malloc": [P(vp), C.c_size_t], "vvhip_free": [vp],
        "vvhip_memcpy_h2d": [vp, vp, C.c_size_t], "vvhip_memcpy_d2h": [vp, vp, C.c_size_t],
        "vvhip_memset": [vp, C.c_int, C.c_size_t], "vvhip_synchronize": [vp],
        "vvhip_stream_create": [P(vp)], "vvhip_stream_destroy": [vp],
        "vvhip_synth_tether_force": [vp, vp, dbl, dbl],
        "vvhip_run_graph": [vp, C.c_int, C.c_int, vp, dbl, dbl],
        "vvhip_graph_prepare": [vp, C.c_int, vp, dbl, dbl],
        "vvhip_status": [vp, P(i32), P(i32)], "vvhip_status_clear": [vp], "vvhip_recovery_count": [vp, P(C.c_int64)], "vvhip_masses_changed": [vp],
        "vvhip_status_words": [vp, P(i32 * 4)], "vvhip_fused_status": [vp, P(i32), P(C.c_int64), P(i32)],
        "vvhip_run_eager": [vp, C.c_int, vp, dbl, dbl],
        "vvhip_run_eager_unfused": [vp, C.c_int, vp, dbl, dbl],
        "vvhip_set_random_seed": [vp, C.c_uint64], "vvhip_fill_random": [vp],
        "vvhip_comm_count": [vp, P(i32)], "vvhip_peer_access": [C.c_int, C.c_int, P(i32)],
        "vvhip_comm_unique_id": [vp], "vvhip_comm_init": [vp, vp, C.c_int, C.c_int], "vvhip_comm_destroy": [vp],
        "vvhip_mailbox_create": [vp, C.c_int, C.c_int, vp], "vvhip_mailbox_connect": [vp, vp],
        "vvhip_mailbox_status": [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)], "vvhip_mailbox_destroy": [vp],
        "vvhip_mailbox_layout": [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
        "vvhip_time_kernel": [vp, C.c_int, u32, C.c_int, P(dbl)],
        "vvhip_generic_launches": [vp, P(C.c_int64 * 2), P(u32 * 2)],
        "vvhip_rtc_stats": [P(C.c_int64 * 3), P(C.c_double)], "vvhip_rtc_failures": [P(C.c_int64)],
        "vvhip_rtc_mode": [C.c_int],
        "vvhip_timing_enable": [vp, C.c_int], "vvhip_timing_read": [vp, P(dbl), P(dbl), P(dbl), P(i32 * 3)],
        "vvhip_debug_step_spans": [vp, C.c_int, vp, dbl, dbl, P(dbl * 36)], "vvhip_debug_fused_flags": [vp, C.c_int, P(u32)], "vvhip_debug_launch_shape": [vp, P(C.c_int32 * 4)],
        "vvhip_debug_launch": [vp, C.c_int, u32, u32], "vvhip_debug_tune": [vp, C.c_char_p, C.c_int],
        "vvhip_debug_read_accumulators": [vp, P(dbl * 4), C.c_int],
        "vvhip_debug_set_scales": [vp, P(dbl * 4)],
        "vvhip_debug_old_delta": [vp, P(vp)], "vvhip_debug_live_buffers": [P(C.c_int64), P(C.c_int64)],
        "vvhip_debug_recorder_digest": [vp, C.c_char_p, P(C.c_uint64)],
        "vvhip_set_trace": [vp, C.c_int],
        "vvhip_debug_span": [vp, C.c_int, C.c_uint32, C.c_int, P(C.c_double * 8)],
        "vvhip_debug_timestamps": [vp, C.c_uint32, C.c_int, P(C.c_longlong * 128)],
        "vvhip_debug_timestamps_fused": [vp, C.c_int, P(C.c_longlong * 128)],
    }
    for name, args in sig.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            # an OLDER build of the library named by VVHIP_LIB (A/B runs of a previous round's kernels, tools/probes/ab_lib_rates.sh) may lack the newest
            # entry points; the product library must export every one of them (tests/test_host_plan.py checks the header's list)
            if os.environ.get("VVHIP_LIB"):
                continue
            raise
        fn.argtypes = args
        fn.restype = C.c_int
    lib.vvhip_plan_destroy.argtypes = [vp]
    lib.vvhip_plan_destroy.restype = None
    lib.vvhip_last_error.argtypes = [vp]
    lib.vvhip_last_error.restype = C.c_char_p
    lib.vvhip_plan_unfused_reason.argtypes = [vp]
    lib.vvhip_plan_unfused_reason.restype = C.c_char_p
    if hasattr(lib, "vvhip_checkpoint_error") or not os.environ.get("VVHIP_LIB"):      # (an older build named by VVHIP_LIB: see above)
        lib.vvhip_checkpoint_error.argtypes = []
        lib.vvhip_checkpoint_error.restype = C.c_char_p
    return lib


lib = _load()
EXPORTS = sorted(["vvhip_plan_destroy", "vvhip_last_error"] + [n for n in dir(lib) if n.startswith("vvhip_")])


def device_count() -> int:
    n = C.c_int(0)
    lib.vvhip_device_count(C.byref(n))
    return n.value


def check(rc: int, plan=None, what: str = ""):
    if rc != OK:
        msg = lib.vvhip_last_error(plan).decode() if plan else what
        raise VVHipError(rc, msg or what)


def frames_schedule(interval: int, after_step: int, n: int, logarithmic: bool = False) -> np.ndarray:
    """The first n steps after `after_step` at which a frame recorder records (include/vvhip.h: vvhip_frames_schedule, the one statement
    of the linear and the logarithmic schedule)."""
    out = np.zeros(int(n), dtype=np.int64)
    rc = lib.vvhip_frames_schedule(int(interval), FRAMES_LOG10 if logarithmic else FRAMES_LINEAR, int(after_step), int(n), out.ctypes.data)
    if rc != OK:
        raise VVHipError(rc, "vvhip_frames_schedule: interval must be >= 1, after_step >= 0 and the steps below 2^61")
    return out


def frames_steps(interval: int, after_step: int, last_step: int, logarithmic: bool = False) -> np.ndarray:
    """The steps in (after_step, last_step] at which a frame recorder records."""
    out, s = [], int(after_step)
    while s <= last_step:
        chunk = frames_schedule(interval, s, 64, logarithmic)
        out.append(chunk[chunk <= last_step])
        s = int(chunk[-1])
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def digest_host(data, base: int = 0) -> int:
    """The digest of a buffer's 32-bit words at global word index `base` (include/vvhip.h: vvhip_digest_host)."""
    a = np.ascontiguousarray(data).view(np.uint8).reshape(-1) if not isinstance(data, (bytes, bytearray)) else np.frombuffer(data, dtype=np.uint8)
    out = C.c_uint64(0)
    rc = lib.vvhip_digest_host(a.ctypes.data if a.size else None, a.size, int(base), C.byref(out))
    if rc != OK:
        raise VVHipError(rc, "vvhip_digest_host: the bytes are no multiple of 4, or a word index reaches 2^32")
    return out.value


def checkpoint_inspect(blob) -> CheckpointHeader:
    """The header of a checkpoint blob after every check a load makes without a plan: bounds, magic, version, table, all digests
    (vvhip_checkpoint_inspect).  Raises VVHipError(ERR_INVALID) with a text that names the fault."""
    blob = bytes(blob)
    h = CheckpointHeader()
    rc = lib.vvhip_checkpoint_inspect(blob, len(blob), C.byref(h))
    if rc != OK:
        raise VVHipError(rc, lib.vvhip_checkpoint_error().decode())
    return h


def checkpoint_sections(blob) -> dict:
    """{section name: CheckpointSection} of an inspected blob's table."""
    blob = bytes(blob)
    h = checkpoint_inspect(blob)
    table = (CheckpointSection * h.num_sections).from_buffer_copy(blob, C.sizeof(CheckpointHeader))
    return {CKPT_SECTION_NAMES[s.id]: s for s in table}


class DeviceArray:
    """A device allocation with a host-side dtype/shape; upload/download are blocking copies."""

    def __init__(self, shape, dtype, fill=None):
        self.shape = tuple(np.atleast_1d(shape)) if not isinstance(shape, tuple) else shape
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        rc = lib.vvhip_malloc(C.byref(p), max(self.nbytes, 16))
        if rc != OK:
            raise VVHipError(rc, f"hipMalloc of {self.nbytes} bytes failed (is a GPU visible?)")
        self.ptr = p.value
        if fill is not None:
            self.upload(np.full(self.shape, fill, dtype=self.dtype))

    @classmethod
    def from_host(cls, a):
        a = np.ascontiguousarray(a)
        d = cls(a.shape, a.dtype)
        d.upload(a)
        return d

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.nbytes == self.nbytes, (a.shape, self.shape)
        if self.nbytes:
            rc = lib.vvhip_memcpy_h2d(self.ptr, a.ctypes.data, self.nbytes)
            if rc != OK:
                raise VVHipError(rc, "hipMemcpy H2D failed")

    def download(self):
        out = np.empty(self.shape, dtype=self.dtype)
        if self.nbytes:
            rc = lib.vvhip_memcpy_d2h(out.ctypes.data, self.ptr, self.nbytes)
            if rc != OK:
                raise VVHipError(rc, "hipMemcpy D2H failed")
        return out

    def free(self):
        if self.ptr:
            lib.vvhip_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
