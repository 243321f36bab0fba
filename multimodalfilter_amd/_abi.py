"""ctypes binding of ``libmmf_hip.so`` (the C ABI declared in ``include/mmf.h``).

This is the thin layer the product path goes through: tensors stay ``torch.Tensor`` (device
memory + stream plumbing), the arithmetic is the hand-written HIP behind these entry
points.  There is deliberately no fallback: if the library is missing, or a launch fails,
the call raises.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_float, c_int, c_int32, c_size_t, c_uint64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMF_LIB_PATH") or os.path.join(_HERE, "libmmf_hip.so")  # override: experiment builds only

MMF_UNITS = 64
MMF_MAX_RES = 3
MMF_MAX_STATE_DIM = 4
ABI_VERSION = 42
KIND_DYNAMICS, KIND_MEASURE, KIND_JACOBIAN = 0, 1, 2  # particle-network kinds (csrc/particle_net.hip)
PREC_F32, PREC_F16X3, PREC_BF16, PREC_F16X3_DUAL = 0, 1, 2, 3
PRECISIONS = {"f32": PREC_F32, "f16x3": PREC_F16X3}                          # per-particle networks (K2)
IMAGE_PRECISIONS = {"f32": PREC_F32, "f16x3": PREC_F16X3, "bf16": PREC_BF16}  # image encoder (K4)
FLAG_RANGE, FLAG_GAVE_UP, FLAG_NOT_PD = 1, 4, 16  # the device status word (include/mmf.h: MMF_FLAG_*)

_FP = c_void_p  # device pointers travel as integers


class MmfParticleNetDesc(Structure):
    _fields_ = [
        ("d_in", c_int32), ("n_res", c_int32), ("relu_after_join", c_int32), ("n_out", c_int32),
        ("join_in", c_int32), ("join_state_off", c_int32),
        ("w_in", _FP), ("b_in", _FP),
        ("w_enc", _FP * 2), ("b_enc", _FP * 2),
        ("w_join", _FP),
        ("w_res", _FP * (2 * MMF_MAX_RES)), ("b_res", _FP * (2 * MMF_MAX_RES)),
        ("w_head", _FP), ("b_head", _FP),
    ]


TRAJ_MAX_IO, TRAJ_SLOTS = 8, 8
TRAJ_LOAD, TRAJ_LINEAR, TRAJ_STORE, TRAJ_STORE_DIAG = 0, 1, 2, 3
TRAJ_MASK, TRAJ_ADD, TRAJ_ZERO, TRAJ_LOAD_ADD = 4, 5, 6, 7
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SQRT_SQ_PLUS = 0, 1, 2, 3


class MmfTrajInstr(Structure):
    _fields_ = [("op", c_int32), ("dst", c_int32), ("src", c_int32 * 4), ("src_off", c_int32 * 4), ("src_dim", c_int32 * 4),
                ("out_dim", c_int32), ("w_off", c_int32), ("b_off", c_int32), ("res", c_int32),
                ("act", c_int32), ("io", c_int32), ("io_stride", c_int32), ("io_off", c_int32),
                ("fparam", c_float), ("dst_off", c_int32)]


class MmfPfTrainFinalizeArgs(Structure):
    _fields_ = [(n, c_int32) for n in ("T", "N", "SL", "S", "n_res", "d", "n_out", "join_in", "join_state_off", "fused",
                                       "beta_stride", "beta_col")] + \
               [(n, c_void_p) for n in ("pw", "pb", "p_first", "p_head", "p_dout", "p_traj", "grads", "bias_grad", "d_beta", "scratch")]


class MmfTrajPackDesc(Structure):
    _fields_ = [("src", c_uint64), ("kind", c_int32), ("rows", c_int32), ("ld", c_int32), ("col0", c_int32), ("dim", c_int32),
                ("out_pad", c_int32), ("dst_off", c_int32), ("reserved", c_int32)]


TRAJ_PACK_LAYER, TRAJ_PACK_TRANSPOSED, TRAJ_PACK_BIAS = 0, 1, 2


class MmfTrajGradDesc(Structure):
    _fields_ = [("x_col", c_int32), ("x_dim", c_int32), ("dz_col", c_int32), ("out_dim", c_int32),
                ("grad_off", c_int32), ("grad_ld", c_int32), ("bias_off", c_int32), ("reserved", c_int32)]


LOOP_MAX_MEAS = 4


class MmfPfLoopArgs(Structure):
    _fields_ = [("T", c_int32), ("N", c_int32), ("M", c_int32), ("d", c_int32), ("n_meas", c_int32),
                ("resample_mode", c_int32), ("precision", c_int32), ("n_res_dyn", c_int32),
                ("n_res_meas", c_int32), ("logw_stride", c_int32),
                ("dyn_packed", _FP), ("dyn_bias", _FP),
                ("meas_packed", _FP * LOOP_MAX_MEAS), ("meas_bias", _FP * LOOP_MAX_MEAS),
                ("meas_logw", _FP * LOOP_MAX_MEAS),
                ("noise", _FP), ("scale_tril", _FP), ("uniforms", _FP),
                ("states_a", _FP), ("states_b", _FP), ("logw_a", _FP), ("logw_b", _FP),
                ("loglik", _FP), ("estimates", _FP), ("range_flag", _FP),
                ("final_location", POINTER(c_int32)), ("events", POINTER(c_void_p)),
                ("event_stride", c_int32), ("loglik_steps", _FP), ("indices_steps", _FP),
                ("noise_seed", ctypes.c_uint64), ("noise_step0", ctypes.c_uint32), ("noise_traj0", ctypes.c_uint32),
                ("noise_mode", c_int32),
                ("soft_alpha", ctypes.c_float), ("estimate_argmax", c_int32), ("estimate_scratch", _FP),
                ("persistent", c_int32), ("n_sync_words", c_int32), ("sync_words", _FP),
                ("cov_steps", _FP), ("ess_steps", _FP), ("log_evidence_steps", _FP)]


class MmfPfDedupWorkspace(Structure):
    """Run table of ``mmf_pf_forward_loop_dedup`` (include/mmf.h): int32 device arrays."""
    _fields_ = [("rank", _FP), ("run_anc", _FP), ("run_start", _FP), ("n_runs", _FP)]


class MmfPfHistory(Structure):
    """History arrays of ``mmf_pf_forward_loop_history`` (include/mmf.h): float32 device arrays."""
    _fields_ = [("states_steps", _FP), ("logw_in_steps", _FP), ("logw_in0", _FP)]


PHILOX_STREAM_NOISE, PHILOX_STREAM_UNIFORM, PHILOX_STREAM_JITTER = 0, 1, 2  # include/mmf_philox.h: MMF_PHILOX_STREAM_*


class MmfPfRegulariseArgs(Structure):
    """``mmf_pf_regularise`` (include/mmf.h): the kernel jitter of a resampled set."""
    _fields_ = [("N", c_int32), ("M", c_int32), ("d", c_int32), ("shrink", c_int32),
                ("states", _FP), ("cov", _FP), ("ess", _FP), ("mean", _FP), ("resampled", _FP), ("noise", _FP),
                ("noise_seed", ctypes.c_uint64), ("noise_step", ctypes.c_uint32), ("noise_traj0", ctypes.c_uint32),
                ("noise_mode", c_int32), ("scale", c_float), ("floor", c_float * MMF_MAX_STATE_DIM),
                ("bandwidth", _FP), ("factor", _FP)]


class MmfPfLoopRegularise(Structure):
    """What ``mmf_pf_forward_loop_regularised`` adds to ``MmfPfLoopArgs`` (include/mmf.h)."""
    _fields_ = [("scale", c_float), ("floor", c_float * MMF_MAX_STATE_DIM), ("shrink", c_int32), ("noise", _FP),
                ("noise_seed", ctypes.c_uint64), ("noise_step0", ctypes.c_uint32), ("noise_traj0", ctypes.c_uint32),
                ("noise_mode", c_int32), ("cov", _FP), ("ess", _FP), ("resampled", _FP), ("bandwidth_steps", _FP)]


class MmfPfSmoothArgs(Structure):
    _fields_ = [("T", c_int32), ("N", c_int32), ("M", c_int32), ("d", c_int32), ("lag", c_int32),
                ("states_steps", _FP), ("loglik_steps", _FP), ("logw_in_steps", _FP), ("logw_in0", _FP),
                ("indices_steps", _FP), ("mean", _FP), ("cov", _FP), ("unique", _FP)]


class MmfPfSmoothMarginalArgs(Structure):
    _fields_ = [("T", c_int32), ("N", c_int32), ("M", c_int32), ("d", c_int32),
                ("states_steps", _FP), ("pred_steps", _FP), ("loglik_steps", _FP), ("logw_in_steps", _FP),
                ("scale_tril", _FP), ("logd", _FP), ("weights", _FP), ("mean", _FP), ("cov", _FP), ("ess", _FP)]


class MmfPfSmoothSimulateArgs(Structure):
    _fields_ = [("T", c_int32), ("N", c_int32), ("M", c_int32), ("d", c_int32), ("S", c_int32),
                ("states_steps", _FP), ("pred_steps", _FP), ("loglik_steps", _FP), ("logw_in_steps", _FP),
                ("scale_tril", _FP), ("uniforms", _FP), ("indices", _FP), ("trajectories", _FP), ("mean", _FP), ("cov", _FP)]


class MmfPfSmoothPairArgs(Structure):
    _fields_ = [("T", c_int32), ("N", c_int32), ("M", c_int32), ("d", c_int32),
                ("states_steps", _FP), ("pred_steps", _FP), ("loglik_steps", _FP), ("logw_in_steps", _FP),
                ("scale_tril", _FP), ("weights", _FP), ("logd", _FP), ("workspace", _FP),
                ("residual_mean", _FP), ("residual_second_moment", _FP)]


class MmfPfSmoothMapArgs(Structure):
    _fields_ = [("T", c_int32), ("N", c_int32), ("M", c_int32), ("d", c_int32),
                ("states_steps", _FP), ("pred_steps", _FP), ("loglik_steps", _FP), ("logw_in_steps", _FP),
                ("scale_tril", _FP), ("v", _FP), ("step_max", _FP), ("backpointers", _FP), ("indices", _FP),
                ("path", _FP), ("log_posterior", _FP)]


QUANTILES_MAX = 16    # MMF_QUANTILES_MAX
SUMMARY_MAX_M = 16384  # particles per row that mmf_pf_quantiles sorts in LDS and mmf_pf_scores and mmf_pf_density serve
QUANTILES_MAX_M = SCORES_MAX_M = DENSITY_MAX_M = MODES_MAX_M = SUMMARY_MAX_M
PREDICTIVE_MAX_M = SUMMARY_MAX_M  # mixture components per row that mmf_pf_predictive serves
DISTANCE_MAX_M = SUMMARY_MAX_M  # particles of BOTH sets of a row pair together: mmf_pf_distance sorts their union in LDS


class MmfPfQuantilesArgs(Structure):
    _fields_ = [("R", c_int32), ("M", c_int32), ("d", c_int32), ("Q", c_int32), ("probs", ctypes.c_float * QUANTILES_MAX),
                ("states", _FP), ("log_a", _FP), ("log_b", _FP), ("query", _FP), ("quantiles", _FP), ("cdf", _FP)]


class MmfPfScoresArgs(Structure):
    _fields_ = [("R", c_int32), ("M", c_int32), ("d", c_int32), ("scale", ctypes.c_float * MMF_MAX_STATE_DIM),
                ("states", _FP), ("log_a", _FP), ("log_b", _FP), ("truth", _FP), ("crps", _FP), ("energy", _FP), ("spread", _FP),
                ("workspace", _FP), ("workspace_bytes", c_size_t)]


class MmfPfScoresBackwardArgs(Structure):
    _fields_ = [("R", c_int32), ("M", c_int32), ("d", c_int32), ("scale", ctypes.c_float * MMF_MAX_STATE_DIM),
                ("states", _FP), ("log_a", _FP), ("log_b", _FP), ("truth", _FP), ("g_crps", _FP), ("g_energy", _FP),
                ("g_states", _FP), ("g_logw", _FP), ("workspace", _FP), ("workspace_bytes", c_size_t)]


DENSITY_RULES = {"fixed": 0, "silverman": 1, "scott": 2}  # MmfPfDensityArgs.rule


class MmfPfDensityArgs(Structure):
    _fields_ = [("R", c_int32), ("M", c_int32), ("d", c_int32), ("rule", c_int32),
                ("bandwidth", ctypes.c_float * MMF_MAX_STATE_DIM), ("min_bandwidth", ctypes.c_float * MMF_MAX_STATE_DIM),
                ("states", _FP), ("log_a", _FP), ("log_b", _FP), ("truth", _FP), ("log_density", _FP), ("log_score", _FP),
                ("entropy", _FP), ("mode", _FP), ("mode_index", _FP), ("bandwidth_out", _FP),
                ("workspace", _FP), ("workspace_bytes", c_size_t)]


MODES_MAX = 8               # MMF_PF_MODES_MAX
MODES_LDS_MASS_M = 8192     # MMF_PF_MODES_LDS_MASS_M: beyond it the finish of mmf_pf_modes keeps the masses in the workspace


class MmfPfModesArgs(Structure):
    _fields_ = [("R", c_int32), ("M", c_int32), ("d", c_int32), ("max_modes", c_int32), ("link_radius", c_float),
                ("states", _FP), ("log_a", _FP), ("log_b", _FP), ("log_density", _FP), ("bandwidth", _FP),
                ("parent", _FP), ("labels", _FP), ("count", _FP), ("index", _FP), ("modes", _FP), ("mass", _FP), ("mean", _FP),
                ("workspace", _FP), ("workspace_bytes", c_size_t)]


class MmfPfModalitiesArgs(Structure):
    _fields_ = [("R", c_int32), ("M", c_int32), ("d", c_int32), ("K", c_int32), ("logw_stride", c_int32),
                ("states", _FP), ("log_w", _FP), ("loglik", _FP * LOOP_MAX_MEAS), ("modality_logw", _FP),
                ("log_evidence", _FP), ("responsibility", _FP), ("ess", _FP), ("mean", _FP), ("divergence", _FP), ("overlap", _FP)]


class MmfPfDistanceArgs(Structure):
    _fields_ = [("R", c_int32), ("Ma", c_int32), ("Mb", c_int32), ("d", c_int32), ("scale", ctypes.c_float * MMF_MAX_STATE_DIM),
                ("states_a", _FP), ("log_a_a", _FP), ("log_b_a", _FP), ("states_b", _FP), ("log_a_b", _FP), ("log_b_b", _FP),
                ("wasserstein", _FP), ("cramer", _FP), ("ks", _FP), ("energy", _FP), ("terms", _FP),
                ("workspace", _FP), ("workspace_bytes", c_size_t)]


class MmfPfPredictiveArgs(Structure):
    _fields_ = [("R", c_int32), ("M", c_int32), ("d", c_int32),
                ("centres", _FP), ("log_a", _FP), ("log_b", _FP), ("scale_tril", _FP), ("truth", _FP),
                ("mean", _FP), ("covariance", _FP), ("log_score", _FP), ("pit", _FP), ("spread", _FP), ("crps", _FP),
                ("workspace", _FP), ("workspace_bytes", c_size_t)]


RASTER_MAX_M = SUMMARY_MAX_M  # particles per row that mmf_pf_raster serves
RASTER_MAX_CELLS = 128        # cells of a map along each axis at most (at least 2)
RASTER_WAVES = 4              # the waves of mmf_pf_raster's workgroup: each takes a contiguous chunk of ceil(M / 4) particles
RASTER_STAGE = 64             # the particles one of them stages at a time
MEASURE_MAX_PARTICLES = 0x7FFFFFFF // 8  # particles (N * M) of one K2 launch: beyond it mmf_pf_measure* answer MMF_ETOOLARGE


def as_float32(x: float) -> float:
    """``x`` rounded to float32, as a host float of an argument struct is."""
    return c_float(x).value


class MmfPfRasterArgs(Structure):
    _fields_ = [("R", c_int32), ("M", c_int32), ("d", c_int32), ("dims", c_int32 * 2), ("cells", c_int32 * 2),
                ("step", ctypes.c_float * 2),
                ("states", _FP), ("log_a", _FP), ("log_b", _FP), ("center", _FP), ("bandwidth", _FP), ("density", _FP)]


class MmfTrainNet(Structure):
    _fields_ = [("packed", _FP), ("packed_f32", _FP), ("packed_t", _FP), ("head_w", _FP), ("pw", _FP), ("pb", _FP),
                ("p_first", _FP), ("p_head", _FP), ("p_dout", _FP), ("p_traj", _FP), ("packed_dual", _FP)]


class MmfPfTrainArgs(Structure):
    _fields_ = [("T", c_int32), ("N", c_int32), ("M", c_int32), ("d", c_int32), ("n_meas", c_int32),
                ("n_res_dyn", c_int32), ("n_res_meas", c_int32), ("logw_stride", c_int32), ("precision", c_int32),
                ("chunk_traj", c_int32), ("n_splits", c_int32), ("n_slices", c_int32),
                ("dyn", MmfTrainNet), ("meas", MmfTrainNet * LOOP_MAX_MEAS),
                ("dyn_bias", _FP), ("meas_bias", _FP * LOOP_MAX_MEAS), ("meas_logw", _FP * LOOP_MAX_MEAS),
                ("noise", _FP), ("scale_tril", _FP), ("g_estimates", _FP),
                ("states", _FP), ("logw", _FP), ("estimates", _FP), ("d_states0", _FP), ("d_logw0", _FP),
                ("stash", _FP), ("mask", _FP), ("dz", _FP), ("raw", _FP), ("d_raw", _FP), ("loglik", _FP), ("ll_steps", _FP),
                ("g_states_a", _FP), ("g_states_b", _FP), ("g_logw_a", _FP), ("g_logw_b", _FP), ("d_tmp", _FP),
                ("range_flag", _FP), ("dz_scale", _FP),
                ("fused", c_int32), ("fused_act", _FP), ("fused_g_act", _FP), ("fused_sets", c_int32)]


SET_NLL_WAVE_M = 256  # mmf_pf_set_nll: a wave owns a row up to here, a workgroup beyond (csrc/pf_set_loss.hip: kWaveM)


class MmfPfSetNllArgs(Structure):
    _fields_ = [("R", c_int32), ("M", c_int32), ("d", c_int32),
                ("states", _FP), ("logw", _FP), ("truth", _FP), ("scale", _FP), ("g_nll", _FP),
                ("nll", _FP), ("g_states", _FP), ("g_logw", _FP), ("g_log_scale", _FP)]


class MmfTrainFusedArgs(Structure):
    _fields_ = [("packed_dual", _FP), ("n_res", c_int32), ("kind", c_int32), ("d", c_int32), ("N", c_int32), ("M", c_int32),
                ("n_slots", c_int32), ("states", _FP), ("traj_bias", _FP), ("d_out", _FP), ("g_next", _FP), ("d_raw", _FP),
                ("act", _FP), ("g_act", _FP), ("d_states", _FP), ("dz_first_h", _FP), ("sc_first", _FP), ("dz_join_h", _FP),
                ("sc_join", _FP), ("h_last_h", _FP), ("pw", _FP), ("pb", _FP), ("d_states_base", _FP)]


class MmfEkfLoopArgs(Structure):
    _fields_ = [("T", c_int32), ("N", c_int32), ("d", c_int32), ("K", c_int32),
                ("fusion", c_int32), ("feedback", c_int32), ("n_res_dyn", c_int32), ("precision", c_int32),
                ("range_flag", _FP),
                ("dyn_packed", _FP * LOOP_MAX_MEAS), ("dyn_bias", _FP * LOOP_MAX_MEAS),
                ("q_tril", _FP), ("z", _FP), ("r_tril", _FP), ("fuse_w", _FP),
                ("mu", _FP), ("Sigma", _FP), ("mu_pred", _FP), ("A", _FP), ("Sigma_f", _FP),
                ("estimates", _FP), ("feedback_gate", _FP),
                ("persistent", c_int32), ("n_sync_words", c_int32), ("sync_words", _FP)]


class MmfEkfInnovArgs(Structure):
    """The innovation record of ``mmf_ekf_forward_loop_innov`` (include/mmf.h): the NIS gate (< 0: none) and three
    ``(T, K, N)`` device arrays, any of them null."""
    _fields_ = [("nis_gate", c_float), ("nis_steps", _FP), ("loglik_steps", _FP), ("accepted_steps", _FP)]


class MmfEkfSmoothArgs(Structure):
    _fields_ = [("T", c_int32), ("N", c_int32), ("d", c_int32), ("lag", c_int32),
                ("mu", _FP), ("Sigma", _FP), ("A", _FP), ("mu_pred", _FP), ("q_tril", _FP),
                ("mu_s", _FP), ("Sigma_s", _FP), ("gain", _FP), ("Sigma_pred", _FP),
                ("resid_mean", _FP), ("resid_m2", _FP)]


class MmfLstmArgs(Structure):
    _fields_ = [("T", c_int32), ("N", c_int32), ("in_dim", c_int32), ("persistent", c_int32),
                ("x", _FP), ("h0", _FP), ("c0", _FP), ("hT", _FP), ("cT", _FP), ("h2", _FP), ("packed", _FP),
                ("range_flag", _FP), ("sync_words", _FP), ("n_sync_words", c_size_t)]


class MmfImageEncoderDesc(Structure):
    _fields_ = [("conv_w", _FP * 5), ("conv_b", _FP * 5), ("fc_w", _FP), ("fc_b", _FP),
                ("res_w", _FP * 2), ("res_b", _FP * 2), ("variant", c_int32)]


SIGNATURES = {
    "mmf_version": (c_int, []),
    "mmf_pf_reweight_resample": (c_int, [_FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP,
                                         c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mmf_pf_reweight_resample_soft": (c_int, [_FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP,
                                              c_int, c_int, c_int, c_int, c_int, ctypes.c_float, c_void_p]),
    "mmf_pf_reweight_resample_belief": (c_int, [_FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP,
                                                c_int, c_int, c_int, c_int, c_int, ctypes.c_float, _FP, _FP, _FP, c_void_p]),
    "mmf_pf_reweight_resample_adaptive": (c_int, [_FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_int, c_int,
                                                  ctypes.c_float, ctypes.c_float, _FP, _FP, _FP, _FP, c_void_p]),
    "mmf_pf_reweight_resample_lds_bytes": (c_size_t, [c_int, c_int]),
    "mmf_pf_set_resample_cluster": (None, [c_int]),
    "mmf_pf_get_resample_cluster": (c_int, []),
    "mmf_particle_net_floats": (c_size_t, [c_int]),
    "mmf_pack_particle_net": (c_int, [POINTER(MmfParticleNetDesc), _FP, c_int, c_void_p]),
    "mmf_pf_dynamics": (c_int, [_FP, c_int, c_int, _FP, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_int, c_void_p]),
    "mmf_pf_measure": (c_int, [_FP, c_int, c_int, _FP, _FP, _FP, c_int, _FP, c_int, _FP, c_int, c_int, c_int, c_void_p]),
    "mmf_pf_measure_multi": (c_int, [POINTER(c_void_p), c_int, c_int, c_int, _FP, POINTER(c_void_p), POINTER(c_void_p), c_int,
                                     POINTER(c_void_p), _FP, c_int, c_int, c_int, c_void_p]),
    "mmf_dynamics_jacobian": (c_int, [_FP, c_int, c_int, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_void_p]),
    "mmf_ekf_step": (c_int, [_FP] * 10 + [c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mmf_ekf_step_gated": (c_int, [_FP] * 10 + [c_int, c_int, c_int, c_int, c_int, _FP, c_void_p]),
    "mmf_ekf_step_innov": (c_int, [_FP] * 10 + [c_int, c_int, c_int, c_int, c_int, _FP, c_float, _FP, _FP, _FP, c_void_p]),
    "mmf_ekf_step_backward": (c_int, [_FP] * 13 + [c_int, c_int, c_int, c_void_p]),
    "mmf_ukf_sigma_points": (c_int, [_FP, _FP, ctypes.c_float, _FP, _FP, c_int, c_int, c_void_p]),
    "mmf_ukf_moments": (c_int, [_FP, ctypes.c_float, ctypes.c_float, ctypes.c_float, _FP, _FP, _FP, c_int, c_int, c_void_p]),
    "mmf_pf_reweight_backward": (c_int, [_FP, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_int, c_void_p]),
    "mmf_pf_init_particles": (c_int, [_FP, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_int, c_void_p]),
    "mmf_pf_forward_loop": (c_int, [POINTER(MmfPfLoopArgs), c_void_p]),
    "mmf_pf_forward_loop_adaptive": (c_int, [POINTER(MmfPfLoopArgs), ctypes.c_float, _FP, c_void_p]),
    "mmf_pf_forward_loop_dedup": (c_int, [POINTER(MmfPfLoopArgs), POINTER(MmfPfDedupWorkspace), c_void_p]),
    "mmf_pf_forward_loop_history": (c_int, [POINTER(MmfPfLoopArgs), POINTER(MmfPfHistory), ctypes.c_float, _FP,
                                            POINTER(MmfPfDedupWorkspace), c_void_p]),
    "mmf_pf_regularise": (c_int, [POINTER(MmfPfRegulariseArgs), c_void_p]),
    "mmf_pf_forward_loop_regularised": (c_int, [POINTER(MmfPfLoopArgs), POINTER(MmfPfHistory), ctypes.c_float, _FP,
                                                POINTER(MmfPfLoopRegularise), c_void_p]),
    "mmf_pf_smooth": (c_int, [POINTER(MmfPfSmoothArgs), c_void_p]),
    "mmf_pf_smooth_lds_bytes": (c_size_t, [c_int]),
    "mmf_pf_smooth_marginal": (c_int, [POINTER(MmfPfSmoothMarginalArgs), c_void_p]),
    "mmf_pf_smooth_simulate": (c_int, [POINTER(MmfPfSmoothSimulateArgs), c_void_p]),
    "mmf_pf_smooth_pair_moments": (c_int, [POINTER(MmfPfSmoothPairArgs), c_void_p]),
    "mmf_pf_smooth_pair_workspace_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "mmf_pf_smooth_map": (c_int, [POINTER(MmfPfSmoothMapArgs), c_void_p]),
    "mmf_pf_quantiles": (c_int, [POINTER(MmfPfQuantilesArgs), c_void_p]),
    "mmf_pf_quantiles_lds_bytes": (c_size_t, [c_int]),
    "mmf_pf_scores": (c_int, [POINTER(MmfPfScoresArgs), c_void_p]),
    "mmf_pf_scores_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "mmf_pf_scores_backward": (c_int, [POINTER(MmfPfScoresBackwardArgs), c_void_p]),
    "mmf_pf_scores_backward_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "mmf_pf_distance": (c_int, [POINTER(MmfPfDistanceArgs), c_void_p]),
    "mmf_pf_distance_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "mmf_pf_distance_lds_bytes": (c_size_t, [c_int, c_int]),
    "mmf_pf_predictive": (c_int, [POINTER(MmfPfPredictiveArgs), c_void_p]),
    "mmf_pf_predictive_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "mmf_pf_raster": (c_int, [POINTER(MmfPfRasterArgs), c_void_p]),
    "mmf_pf_density": (c_int, [POINTER(MmfPfDensityArgs), c_void_p]),
    "mmf_pf_density_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "mmf_pf_modes": (c_int, [POINTER(MmfPfModesArgs), c_void_p]),
    "mmf_pf_modes_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "mmf_pf_modalities": (c_int, [POINTER(MmfPfModalitiesArgs), c_void_p]),
    "mmf_pf_dedup_plan": (c_int, [c_int, c_int, c_int, ctypes.c_float, c_int]),
    "mmf_pf_dedup_workspace_words": (c_size_t, [c_int, c_int]),
    "mmf_pf_resample_runs": (c_int, [_FP] * 11 + [c_int, c_int, c_int, _FP, _FP, _FP, c_void_p]),
    "mmf_pf_dynamics_runs": (c_int, [_FP, c_int, c_int, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP,
                                     c_int, c_int, c_int, c_void_p]),
    "mmf_pf_dynamics_runs_philox": (c_int, [_FP, c_int, c_int, _FP, _FP, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                            _FP, _FP, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_int, c_void_p]),
    "mmf_pf_dedup_deal": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int]),
    "mmf_pf_argmax_estimate": (c_int, [_FP, _FP, _FP, _FP, c_int, c_int, c_int, c_void_p]),
    "mmf_pf_persistent_plan": (c_int, [c_int, c_int, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "mmf_pf_persistent_sync_words": (c_size_t, [c_int, c_int, c_int, c_int]),
    "mmf_pf_dynamics_philox": (c_int, [_FP, c_int, c_int, _FP, _FP, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                       _FP, _FP, _FP, c_int, c_int, c_int, c_void_p]),
    "mmf_philox_normals": (c_int, [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _FP, c_int, c_int, c_int, c_void_p]),
    "mmf_philox_normals_stream": (c_int, [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _FP, c_int, c_int,
                                          c_int, c_void_p]),
    "mmf_philox_uniforms": (c_int, [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _FP, c_int, c_int, c_void_p]),
    "mmf_dynamics_forward_loop": (c_int, [_FP, c_int, c_int, _FP, _FP, _FP, _FP, c_int, c_int, c_int, c_void_p]),
    "mmf_traj_program": (c_int, [_FP, c_int, _FP, POINTER(c_void_p), c_int, c_int, c_int, c_void_p]),
    "mmf_pf_train_finalize": (c_int, [POINTER(MmfPfTrainFinalizeArgs), c_void_p]),
    "mmf_traj_pack": (c_int, [c_void_p, c_int, _FP, c_void_p]),
    "mmf_traj_weight_grads": (c_int, [c_void_p, c_int, _FP, c_int, _FP, c_int, _FP, c_int, _FP, c_int, c_int, c_void_p]),
    "mmf_fc64_train_forward": (c_int, [_FP, _FP, _FP, _FP, _FP, c_int, c_int, c_void_p]),
    "mmf_fc64_train_backward": (c_int, [_FP, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_void_p]),
    "mmf_fuse_virtual_sensors": (c_int, [_FP, _FP, _FP, _FP, _FP, c_int, c_int, c_int, c_int, c_void_p]),
    "mmf_ekf_forward_loop": (c_int, [POINTER(MmfEkfLoopArgs), c_void_p]),
    "mmf_ekf_forward_loop_belief": (c_int, [POINTER(MmfEkfLoopArgs), _FP, c_void_p]),
    "mmf_ekf_forward_loop_innov": (c_int, [POINTER(MmfEkfLoopArgs), POINTER(MmfEkfInnovArgs), _FP, c_void_p]),
    "mmf_ekf_smooth": (c_int, [POINTER(MmfEkfSmoothArgs), c_void_p]),
    "mmf_ekf_persistent_plan": (c_int, [c_int, c_int]),
    "mmf_ekf_persistent_sync_words": (c_size_t, [c_int, c_int, c_int]),
    "mmf_lstm_blob_floats": (c_size_t, [c_int]),
    "mmf_lstm_pack": (c_int, [_FP] * 9 + [c_int, c_void_p]),
    "mmf_lstm_persistent_plan": (c_int, [c_int, c_int]),
    "mmf_lstm_sync_words": (c_size_t, [c_int]),
    "mmf_lstm_forward": (c_int, [POINTER(MmfLstmArgs), c_void_p]),
    "mmf_dynamics_jacobian_multi": (c_int, [POINTER(c_void_p), c_int, c_int, _FP, POINTER(c_void_p), _FP, _FP, _FP,
                                            c_int, c_int, c_int, c_void_p]),
    "mmf_particle_net_train_forward": (c_int, [_FP, c_int, c_int, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_int, c_void_p]),
    "mmf_particle_net_weight_grads": (c_int, [_FP, _FP, _FP, _FP, c_int, c_int, c_int, c_void_p]),
    "mmf_particle_net_small_grads": (c_int, [_FP] * 9 + [c_int] * 5 + [c_void_p]),
    "mmf_particle_net_weight_grads_acc": (c_int, [_FP, _FP, _FP, _FP, c_int, c_int, c_int, c_int, c_void_p]),
    "mmf_pf_train_forward": (c_int, [POINTER(MmfPfTrainArgs), c_void_p]),
    "mmf_pf_train_backward": (c_int, [POINTER(MmfPfTrainArgs), c_void_p]),
    "mmf_pf_train_backward_sets": (c_int, [POINTER(MmfPfTrainArgs), c_void_p, c_void_p, c_void_p]),
    "mmf_pf_set_nll": (c_int, [POINTER(MmfPfSetNllArgs), c_void_p]),
    "mmf_particle_net_train_fused": (c_int, [POINTER(MmfTrainFusedArgs), c_void_p]),
    "mmf_particle_net_train_fused_multi": (c_int, [POINTER(MmfTrainFusedArgs), c_int, c_void_p]),
    "mmf_particle_net_train_backward": (c_int, [_FP, _FP, c_int, c_int, _FP, _FP, _FP, _FP, c_int, c_int, c_void_p]),
    "mmf_image_encoder_floats": (c_size_t, []),
    "mmf_image_encoder_workspace_bytes": (c_size_t, [c_int, c_int]),
    "mmf_pack_image_encoder": (c_int, [POINTER(MmfImageEncoderDesc), _FP, c_void_p]),
    "mmf_image_convs_backward_floats": (c_size_t, []),
    "mmf_pack_image_convs_backward": (c_int, [POINTER(MmfImageEncoderDesc), _FP, c_void_p]),
    "mmf_image_convs_train_forward": (c_int, [_FP] * 8 + [c_int, c_int, c_void_p]),
    "mmf_image_convs_train_backward": (c_int, [_FP] * 10 + [c_int, c_void_p]),
    "mmf_conv_weight_grads": (c_int, [_FP, _FP, _FP, _FP, c_int, c_int, c_int, c_int, _FP, _FP, c_void_p]),
    "mmf_image_convs_train_backward_h": (c_int, [_FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, c_int, c_void_p]),
    "mmf_conv_weight_grads_h": (c_int, [_FP, _FP, _FP, _FP, _FP, _FP, c_int, c_int, c_int, c_int, _FP, _FP, c_void_p]),
    "mmf_image_encoder": (c_int, [POINTER(c_void_p), c_int, _FP, _FP, _FP, _FP, c_int, c_int, c_int, c_void_p]),
}

_lib = None


class MmfError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load the HIP library; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MmfError(
                f"{LIB_PATH} is missing: build it with `python -m multimodalfilter_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback."
            )
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        got = lib.mmf_version()
        if got != ABI_VERSION:
            raise MmfError(f"ABI mismatch: library {got}, binding {ABI_VERSION}")
        _lib = lib
    return _lib


def _check(code: int, what: str):
    if code != 0:
        kind = "argument error" if code < 0 else "hipError_t"
        raise MmfError(f"{what} failed: {kind} {code}")


def ptr(t: torch.Tensor, *, dtype=torch.float32):
    """Device pointer of a contiguous CUDA/HIP tensor (``None`` -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise MmfError("libmmf_hip works on device memory only (got a CPU tensor); no CPU fallback")
    if t.dtype != dtype:
        raise MmfError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise MmfError("tensor must be contiguous")
    return t.data_ptr()


def vp(t: torch.Tensor, dtype=torch.float32):
    """``ptr`` as the ``c_void_p`` a struct field takes (``None`` -> NULL)."""
    return None if t is None else c_void_p(ptr(t, dtype=dtype))


def _on(t: torch.Tensor):
    """Device context of ``t``; CPU tensors are refused here, before any launch."""
    ptr(t, dtype=t.dtype)
    return torch.cuda.device(t.device)


def stream_of(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


# ------------------------------------------------------------------ typed wrappers
def pf_reweight_resample(loglik, logw_in, states_in, u, estimate, states_out, logw_out,
                         indices_out, mode: int, soft_alpha: float = 1.0):
    """K1; ``soft_alpha < 1`` (modes 1 / 2): torchfilter's soft resampling through
    ``mmf_pf_reweight_resample_soft``."""
    N, M, d = states_in.shape
    M_out = logw_out.shape[1]
    assert loglik.shape == (N, M) and logw_in.shape == (N, M) and estimate.shape == (N, d)
    with _on(states_in):
        if soft_alpha < 1.0 and mode != 0:
            _check(load().mmf_pf_reweight_resample_soft(
                ptr(loglik), ptr(logw_in), ptr(states_in), ptr(u), ptr(estimate), ptr(states_out),
                ptr(logw_out), ptr(indices_out, dtype=torch.int32), N, M, M_out, d, mode, float(soft_alpha),
                stream_of(states_in)), "mmf_pf_reweight_resample_soft")
            return
        _check(load().mmf_pf_reweight_resample(
            ptr(loglik), ptr(logw_in), ptr(states_in), ptr(u), ptr(estimate), ptr(states_out),
            ptr(logw_out), ptr(indices_out, dtype=torch.int32), N, M, M_out, d, mode,
            stream_of(states_in)), "mmf_pf_reweight_resample")


def pf_reweight_resample_belief(loglik, logw_in, states_in, u, estimate, states_out, logw_out, indices_out, mode: int,
                                soft_alpha: float = 1.0, *, cov=None, ess=None, log_evidence=None, M_out: int = None):
    """K1 with the step's belief record (``mmf_pf_reweight_resample_belief``): ``cov (N, d, d)``, ``ess (N)``,
    ``log_evidence (N)`` of the pre-resampling weighted set, each or ``None``.  ``logw_in`` / ``logw_out`` may be ``None``
    where the C entry point takes null (plain resampling: uniform weights in / out)."""
    N, M, d = states_in.shape
    if M_out is None:
        M_out = M if mode == 0 else (logw_out.shape[1] if logw_out is not None else states_out.shape[1])
    assert loglik.shape == (N, M) and estimate.shape == (N, d)
    assert cov is None or cov.shape == (N, d, d)
    assert (ess is None or ess.shape == (N,)) and (log_evidence is None or log_evidence.shape == (N,))
    with _on(states_in):
        _check(load().mmf_pf_reweight_resample_belief(
            ptr(loglik), ptr(logw_in), ptr(states_in), ptr(u), ptr(estimate), ptr(states_out),
            ptr(logw_out), ptr(indices_out, dtype=torch.int32), N, M, M_out, d, mode, float(soft_alpha),
            ptr(cov), ptr(ess), ptr(log_evidence), stream_of(states_in)), "mmf_pf_reweight_resample_belief")


def pf_reweight_resample_adaptive(loglik, logw_in, states_in, u, estimate, states_out, logw_out, indices_out, mode: int,
                                  soft_alpha: float = 1.0, *, ess_threshold: float, resampled=None, cov=None, ess=None,
                                  log_evidence=None):
    """K1 with ESS-triggered resampling (``mmf_pf_reweight_resample_adaptive``): trajectory ``n`` resamples iff
    ``not (ess[n] >= float32(ess_threshold * M))`` and otherwise keeps its particles and carries its normalised weights.
    ``resampled``: ``(N,)`` int32 1 / 0 or ``None``; the record as ``pf_reweight_resample_belief``."""
    N, M, d = states_in.shape
    assert loglik.shape == (N, M) and estimate.shape == (N, d) and logw_out.shape == (N, M) and states_out.shape == (N, M, d)
    assert resampled is None or resampled.shape == (N,)
    assert cov is None or cov.shape == (N, d, d)
    assert (ess is None or ess.shape == (N,)) and (log_evidence is None or log_evidence.shape == (N,))
    with _on(states_in):
        _check(load().mmf_pf_reweight_resample_adaptive(
            ptr(loglik), ptr(logw_in), ptr(states_in), ptr(u), ptr(estimate), ptr(states_out), ptr(logw_out),
            ptr(indices_out, dtype=torch.int32), N, M, d, mode, float(soft_alpha), float(ess_threshold),
            ptr(resampled, dtype=torch.int32), ptr(cov), ptr(ess), ptr(log_evidence), stream_of(states_in)),
            "mmf_pf_reweight_resample_adaptive")


def pf_set_resample_cluster(enabled: bool) -> bool:
    """K1 for few trajectories as a cluster of workgroups per trajectory (same bits; off by default: no faster). Returns the previous setting."""
    was = bool(load().mmf_pf_get_resample_cluster())
    load().mmf_pf_set_resample_cluster(int(bool(enabled)))
    return was


def particle_net_floats(n_res: int) -> int:
    return int(load().mmf_particle_net_floats(n_res))


def pack_particle_net(desc: MmfParticleNetDesc, packed: torch.Tensor, precision: int):
    with _on(packed):
        _check(load().mmf_pack_particle_net(ctypes.byref(desc), ptr(packed), precision,
                                            stream_of(packed)), "mmf_pack_particle_net")


def pf_dynamics(packed, n_res, precision, states_in, traj_bias, noise, scale_tril, states_out,
                range_flag, N, M, d):
    with _on(states_in):
        _check(load().mmf_pf_dynamics(ptr(packed), n_res, precision, ptr(states_in), ptr(traj_bias), ptr(noise),
                                      ptr(scale_tril), ptr(states_out),
                                      ptr(range_flag, dtype=torch.int32), N, M, d,
                                      stream_of(states_in)), "mmf_pf_dynamics")


def dynamics_forward_loop(packed, n_res, precision, x0, traj_bias, out, range_flag, T, N, d):
    with _on(x0):
        _check(load().mmf_dynamics_forward_loop(ptr(packed), n_res, precision, ptr(x0), ptr(traj_bias), ptr(out),
                                                ptr(range_flag, dtype=torch.int32), T, N, d, stream_of(x0)),
               "mmf_dynamics_forward_loop")


def pf_dynamics_philox(packed, n_res, precision, states_in, traj_bias, seed, step, traj0, scale_tril, states_out,
                       range_flag, N, M, d):
    with _on(states_in):
        _check(load().mmf_pf_dynamics_philox(ptr(packed), n_res, precision, ptr(states_in), ptr(traj_bias), seed, step,
                                             traj0, ptr(scale_tril), ptr(states_out),
                                             ptr(range_flag, dtype=torch.int32), N, M, d, stream_of(states_in)),
               "mmf_pf_dynamics_philox")


def philox_normals(seed: int, step: int, traj0: int, out: torch.Tensor):
    N, M, d = out.shape
    with _on(out):
        _check(load().mmf_philox_normals(seed, step, traj0, ptr(out), N, M, d, stream_of(out)), "mmf_philox_normals")


def philox_normals_stream(seed: int, stream: int, step: int, traj0: int, out: torch.Tensor):
    """The ``(N, M, d)`` block of counter step ``step`` on Philox stream ``stream`` (``PHILOX_STREAM_*``; 0 is ``philox_normals``)."""
    N, M, d = out.shape
    with _on(out):
        _check(load().mmf_philox_normals_stream(seed, stream, step, traj0, ptr(out), N, M, d, stream_of(out)),
               "mmf_philox_normals_stream")


def regularise_floor(floor, d: int):
    """``floor`` of regularised resampling as ``d`` floats: one float for every dimension or ``d`` of them, each finite and
    ``>= 0``; anything else is a ``ValueError``."""
    import numbers

    vals = [floor] * d if isinstance(floor, numbers.Real) and not isinstance(floor, bool) else list(floor)
    if len(vals) != d:
        raise ValueError(f"regularisation floor must be a float or d = {d} floats, got {len(vals)}")
    vals = [float(v) for v in vals]
    if not all(v >= 0.0 and v != float("inf") for v in vals):
        raise ValueError(f"regularisation floor must be finite and >= 0, got {vals!r}")
    return vals


def pf_regularise(states, cov, ess, *, scale: float, floor=0.0, shrink: bool = False, mean=None, resampled=None, noise=None,
                  counter=None, bandwidth=None, factor=None):
    """``mmf_pf_regularise`` (include/mmf.h): jitter the resampled set ``states (N, M, d)`` in place with ``h L eps`` -- ``h``
    Silverman's factor on ``ess (N)`` times ``scale``, ``L`` the clamped Cholesky factor of ``cov (N, d, d) + diag(floor^2)``;
    ``shrink`` shrinks towards ``mean (N, d)`` first (Liu & West).  ``noise (N, M, d)`` standard normal, or ``counter = (seed,
    step, traj0)``: generated in the kernel on the jitter stream.  ``resampled (N)`` int32: rows with 0 are left as they are.
    Optional outputs ``bandwidth (N)`` and ``factor (N, d, d)`` (``h L``)."""
    N, M, d = states.shape
    assert cov.shape == (N, d, d) and ess.shape == (N,)
    assert (noise is None) != (counter is None), "either a noise tensor or a counter triple"
    assert noise is None or noise.shape == (N, M, d)
    assert mean is None or mean.shape == (N, d)
    assert resampled is None or resampled.shape == (N,)
    assert (bandwidth is None or bandwidth.shape == (N,)) and (factor is None or factor.shape == (N, d, d))
    a = MmfPfRegulariseArgs()
    a.N, a.M, a.d, a.shrink = N, M, d, int(bool(shrink))
    a.states, a.cov, a.ess, a.mean = vp(states), vp(cov), vp(ess), vp(mean)
    a.resampled, a.noise = vp(resampled, torch.int32), vp(noise)
    if counter is not None:
        a.noise_mode = 2
        a.noise_seed, a.noise_step, a.noise_traj0 = (int(v) for v in counter)
    a.scale = float(scale)
    for i, v in enumerate(regularise_floor(floor, d)):
        a.floor[i] = v
    a.bandwidth, a.factor = vp(bandwidth), vp(factor)
    with _on(states):
        _check(load().mmf_pf_regularise(ctypes.byref(a), stream_of(states)), "mmf_pf_regularise")


def philox_uniforms(seed: int, step0: int, traj0: int, out: torch.Tensor):
    T, N = out.shape
    with _on(out):
        _check(load().mmf_philox_uniforms(seed, step0, traj0, ptr(out), T, N, stream_of(out)), "mmf_philox_uniforms")


def pf_measure(packed, n_res, precision, states, traj_bias, modality_logw, logw_stride, loglik, combine,
               range_flag, N, M, d):
    with _on(states):
        _check(load().mmf_pf_measure(ptr(packed), n_res, precision, ptr(states), ptr(traj_bias),
                                     ptr(modality_logw), logw_stride, ptr(loglik), int(combine),
                                     ptr(range_flag, dtype=torch.int32), N, M, d,
                                     stream_of(states)), "mmf_pf_measure")


def dynamics_jacobian(packed, n_res, precision, states_in, traj_bias, states_out, jac, range_flag, N, d):
    with _on(states_in):
        _check(load().mmf_dynamics_jacobian(ptr(packed), n_res, precision, ptr(states_in), ptr(traj_bias),
                                            ptr(states_out), ptr(jac), ptr(range_flag, dtype=torch.int32), N, d,
                                            stream_of(states_in)), "mmf_dynamics_jacobian")


def pf_persistent_plan(N: int, M: int, n_meas: int) -> int:
    """Workgroups the persistent step loop would use for this problem; <= 0: not eligible (include/mmf.h)."""
    return int(load().mmf_pf_persistent_plan(N, M, n_meas, None, None, None))


def pf_persistent_sync_words(N: int, M: int, d: int, n_meas: int) -> int:
    return int(load().mmf_pf_persistent_sync_words(N, M, d, n_meas))


def ekf_persistent_plan(N: int, K: int) -> int:
    """Workgroups the persistent EKF step loop would use for this problem; <= 0: not eligible (include/mmf.h)."""
    return int(load().mmf_ekf_persistent_plan(N, K))


def ekf_persistent_sync_words(N: int, K: int, d: int) -> int:
    return int(load().mmf_ekf_persistent_sync_words(N, K, d))


def pf_argmax_estimate(loglik, logw_in, states, estimate):
    N, M, d = states.shape
    with _on(states):
        _check(load().mmf_pf_argmax_estimate(ptr(loglik), ptr(logw_in), ptr(states), ptr(estimate), N, M, d,
                                             stream_of(states)), "mmf_pf_argmax_estimate")


def ekf_step(A, mu_pred, q_tril, z, r_tril, fuse_w, mu, Sigma, mu_f, Sigma_f, fusion: int,
             feedback: int, feedback_gate=None):
    """``feedback_gate``: int32 device word; the write-back applies only where it is non-zero
    (``mmf_ekf_step_gated``)."""
    K, N, d = mu_pred.shape
    with _on(mu_pred):
        if feedback_gate is not None:
            _check(load().mmf_ekf_step_gated(ptr(A), ptr(mu_pred), ptr(q_tril), ptr(z), ptr(r_tril),
                                             ptr(fuse_w), ptr(mu), ptr(Sigma), ptr(mu_f), ptr(Sigma_f),
                                             N, d, K, fusion, feedback, ptr(feedback_gate, dtype=torch.int32),
                                             stream_of(mu_pred)), "mmf_ekf_step_gated")
            return
        _check(load().mmf_ekf_step(ptr(A), ptr(mu_pred), ptr(q_tril), ptr(z), ptr(r_tril),
                                   ptr(fuse_w), ptr(mu), ptr(Sigma), ptr(mu_f), ptr(Sigma_f),
                                   N, d, K, fusion, feedback, stream_of(mu_pred)), "mmf_ekf_step")


def ekf_step_innov(A, mu_pred, q_tril, z, r_tril, fuse_w, mu, Sigma, mu_f, Sigma_f, fusion: int, feedback: int,
                   feedback_gate=None, *, nis_gate=None, nis=None, loglik=None, accepted=None):
    """``ekf_step`` that also leaves the innovation statistics and applies the NIS gate (``mmf_ekf_step_innov``,
    include/mmf.h): ``nis_gate`` a threshold > 0 or ``None`` (no gating); ``nis`` / ``loglik`` float32 and ``accepted`` int32,
    each ``(K, N)`` or ``None``."""
    K, N, d = mu_pred.shape
    for t in (nis, loglik, accepted):
        assert t is None or t.shape == (K, N)
    with _on(mu_pred):
        _check(load().mmf_ekf_step_innov(ptr(A), ptr(mu_pred), ptr(q_tril), ptr(z), ptr(r_tril), ptr(fuse_w), ptr(mu),
                                         ptr(Sigma), ptr(mu_f), ptr(Sigma_f), N, d, K, fusion, feedback,
                                         ptr(feedback_gate, dtype=torch.int32), -1.0 if nis_gate is None else float(nis_gate),
                                         ptr(nis), ptr(loglik), ptr(accepted, dtype=torch.int32), stream_of(mu_pred)),
               "mmf_ekf_step_innov")


def image_convs_train_forward(packed, images, a1, h, a2, a3, a4, range_flag=None, precision: int = PREC_F32):
    with _on(images):
        _check(load().mmf_image_convs_train_forward(ptr(packed), ptr(images), ptr(a1), ptr(h), ptr(a2), ptr(a3), ptr(a4),
                                                    ptr(range_flag, dtype=torch.int32), precision,
                                                    images.shape[0], stream_of(images)), "mmf_image_convs_train_forward")


def image_convs_train_backward(packed_bwd, a1, h, a2, a3, g_a4, g1, gh, g2, g3):
    with _on(g_a4):
        _check(load().mmf_image_convs_train_backward(ptr(packed_bwd), ptr(a1), ptr(h), ptr(a2), ptr(a3), ptr(g_a4), ptr(g1),
                                                     ptr(gh), ptr(g2), ptr(g3), g_a4.shape[0], stream_of(g_a4)),
               "mmf_image_convs_train_backward")


def image_convs_train_backward_h(packed_bwd, a1, h, a2, a3, g_a4, g1, gh, g2, g3, scratch):
    assert scratch.numel() >= 4 and scratch.dtype == torch.float32
    with _on(g_a4):
        _check(load().mmf_image_convs_train_backward_h(ptr(packed_bwd), ptr(a1), ptr(h), ptr(a2), ptr(a3), ptr(g_a4), ptr(g1),
                                                       ptr(gh), ptr(g2), ptr(g3), ptr(scratch), g_a4.shape[0], stream_of(g_a4)),
               "mmf_image_convs_train_backward_h")


def conv_weight_grads(g, act, partial, partial_b, n_blocks: int, dw=None, db=None):
    """``partial (n_blocks, 9, 32, 32)``, ``partial_b (n_blocks, 32)``: one slot per workgroup; ``dw (co, ci, k, k)`` /
    ``db (co)``: the slots summed into ``nn.Conv2d``'s layout by a second launch."""
    assert partial.numel() >= n_blocks * 9 * 32 * 32 and partial_b.numel() >= n_blocks * 32
    with _on(g):
        _check(load().mmf_conv_weight_grads(ptr(g), ptr(act), ptr(partial), ptr(partial_b), g.shape[0], g.shape[1],
                                            act.shape[1], n_blocks, ptr(dw), ptr(db), stream_of(g)), "mmf_conv_weight_grads")


def conv_weight_grads_h(g, act, g_absmax, partial, partial_b, range_flag, n_blocks: int, dw=None, db=None):
    """``conv_weight_grads`` on the f16 matrix pipe with three products per product; ``g_absmax``: device scalar (largest |g|)."""
    assert partial.numel() >= n_blocks * 9 * 32 * 32 and partial_b.numel() >= n_blocks * 32 and g_absmax.numel() == 1
    with _on(g):
        _check(load().mmf_conv_weight_grads_h(ptr(g), ptr(act), ptr(g_absmax), ptr(partial), ptr(partial_b),
                                              ptr(range_flag, dtype=torch.int32), g.shape[0], g.shape[1], act.shape[1], n_blocks,
                                              ptr(dw), ptr(db), stream_of(g)), "mmf_conv_weight_grads_h")


def image_convs_backward_floats() -> int:
    return int(load().mmf_image_convs_backward_floats())


def pack_image_convs_backward(desc: MmfImageEncoderDesc, packed: torch.Tensor):
    with _on(packed):
        _check(load().mmf_pack_image_convs_backward(ctypes.byref(desc), ptr(packed), stream_of(packed)),
               "mmf_pack_image_convs_backward")


def ekf_step_backward(A, mu_pred, q_tril, z, r_tril, Sigma_in, g_mu, g_Sigma, g_A, g_mu_pred, g_z, g_r_tril, g_Sigma_in):
    K, N, d = mu_pred.shape
    with _on(mu_pred):
        _check(load().mmf_ekf_step_backward(ptr(A), ptr(mu_pred), ptr(q_tril), ptr(z), ptr(r_tril), ptr(Sigma_in),
                                            ptr(g_mu), ptr(g_Sigma), ptr(g_A), ptr(g_mu_pred), ptr(g_z), ptr(g_r_tril),
                                            ptr(g_Sigma_in), N, d, K, stream_of(mu_pred)), "mmf_ekf_step_backward")


def ukf_sigma_points(mu, Sigma, scale: float, points, not_pd):
    N, d = mu.shape
    with _on(mu):
        _check(load().mmf_ukf_sigma_points(ptr(mu), ptr(Sigma), float(scale), ptr(points), ptr(not_pd, dtype=torch.int32),
                                           N, d, stream_of(mu)), "mmf_ukf_sigma_points")


def ukf_moments(points, wm0: float, wc0: float, wi: float, q_tril, mu_pred, Sigma_pred):
    N, d = mu_pred.shape
    with _on(points):
        _check(load().mmf_ukf_moments(ptr(points), float(wm0), float(wc0), float(wi), ptr(q_tril), ptr(mu_pred),
                                      ptr(Sigma_pred), N, d, stream_of(points)), "mmf_ukf_moments")


def particle_net_train_forward(packed, n_res: int, kind: int, states, traj_bias, stash, mask, out, N: int, M: int, d: int):
    with _on(states):
        _check(load().mmf_particle_net_train_forward(ptr(packed), n_res, kind, ptr(states), ptr(traj_bias),
                                                     ptr(stash), ptr(mask, dtype=torch.int32), ptr(out), N, M, d,
                                                     stream_of(states)),
               "mmf_particle_net_train_forward")


def particle_net_train_backward(packed_t, head_w, n_res: int, kind: int, mask, d_out, dz, d_states, R: int, d: int):
    with _on(d_out):
        _check(load().mmf_particle_net_train_backward(ptr(packed_t), ptr(head_w), n_res, kind,
                                                      ptr(mask, dtype=torch.int32), ptr(d_out), ptr(dz), ptr(d_states),
                                                      R, d, stream_of(d_out)),
               "mmf_particle_net_train_backward")


def particle_net_weight_grads(dz, stash, partial_w, partial_b, n_layers: int, R: int, n_splits: int):
    with _on(dz):
        _check(load().mmf_particle_net_weight_grads(ptr(dz), ptr(stash), ptr(partial_w), ptr(partial_b),
                                                    n_layers, R, n_splits, stream_of(dz)),
               "mmf_particle_net_weight_grads")


def particle_net_small_grads(dz_first, dz_join, h_last, states, d_out, p_first, p_head, p_dout, p_traj,
                             N: int, M: int, n_slices: int):
    with _on(dz_first):
        _check(load().mmf_particle_net_small_grads(ptr(dz_first), ptr(dz_join), ptr(h_last), ptr(states), ptr(d_out),
                                                   ptr(p_first), ptr(p_head), ptr(p_dout), ptr(p_traj), N, M,
                                                   states.shape[1], d_out.shape[1], n_slices, stream_of(dz_first)),
               "mmf_particle_net_small_grads")


def pf_train_forward(args: MmfPfTrainArgs, like: torch.Tensor):
    with _on(like):
        _check(load().mmf_pf_train_forward(ctypes.byref(args), stream_of(like)), "mmf_pf_train_forward")


def pf_train_backward(args: MmfPfTrainArgs, like: torch.Tensor):
    with _on(like):
        _check(load().mmf_pf_train_backward(ctypes.byref(args), stream_of(like)), "mmf_pf_train_backward")


def pf_train_backward_sets(args: MmfPfTrainArgs, g_states_steps, g_logw_steps, like: torch.Tensor):
    """``mmf_pf_train_backward`` with the direct loss gradients of every step's weighted set: ``g_states_steps (T, N, M, d)``
    and ``g_logw_steps (T, N, M)``, either ``None`` (both ``None``: ``mmf_pf_train_backward``, launch for launch)."""
    T, N, M, d = args.T, args.N, args.M, args.d
    assert g_states_steps is None or tuple(g_states_steps.shape) == (T, N, M, d)
    assert g_logw_steps is None or tuple(g_logw_steps.shape) == (T, N, M)
    with _on(like):
        _check(load().mmf_pf_train_backward_sets(ctypes.byref(args), ptr(g_states_steps), ptr(g_logw_steps), stream_of(like)),
               "mmf_pf_train_backward_sets")


def pf_set_nll(states, logw, truth, scale, g_nll=None, *, nll=None, g_states=None, g_logw=None, g_log_scale=None):
    """The mixture log score of weighted particle sets against true states and its closed-form gradients (``mmf_pf_set_nll``,
    include/mmf.h): ``states (..., M, d)`` -- ``R`` rows, the product of the leading sizes --, ``logw (..., M)``, ``truth (...,
    d)``, the component scales ``scale (d)`` on the device and ``g_nll (...)`` or ``None`` (1) -> ``nll (...)``, ``g_states``,
    ``g_logw`` like their inputs and ``g_log_scale (..., d)`` per row, each of which may be ``None`` (not all four).  The
    outputs are written in place."""
    lead, (M, d) = tuple(states.shape[:-2]), states.shape[-2:]
    R = 1
    for n in lead:
        R *= n
    assert tuple(logw.shape) == lead + (M,) and tuple(truth.shape) == lead + (d,) and tuple(scale.shape) == (d,)
    assert g_nll is None or tuple(g_nll.shape) == lead
    for out, shape in ((nll, lead), (g_states, lead + (M, d)), (g_logw, lead + (M,)), (g_log_scale, lead + (d,))):
        assert out is None or tuple(out.shape) == shape
    a = MmfPfSetNllArgs()
    a.R, a.M, a.d = R, M, d
    a.states, a.logw, a.truth, a.scale, a.g_nll = vp(states), vp(logw), vp(truth), vp(scale), vp(g_nll)
    a.nll, a.g_states, a.g_logw, a.g_log_scale = vp(nll), vp(g_states), vp(g_logw), vp(g_log_scale)
    with _on(states):
        _check(load().mmf_pf_set_nll(ctypes.byref(a), stream_of(states)), "mmf_pf_set_nll")


def particle_net_train_fused(args: MmfTrainFusedArgs, like: torch.Tensor):
    """One fused network call of the training backward (see include/mmf.h)."""
    with _on(like):
        _check(load().mmf_particle_net_train_fused(ctypes.byref(args), stream_of(like)), "mmf_particle_net_train_fused")


def pf_measure_multi(packed, n_res: int, precision: int, states, traj_bias, modality_logw, logw_stride: int, loglik, range_flag_t):
    """Every modality's own log-likelihood of the same ``(N, M, d)`` particles in one launch; lists of tensors (``modality_logw``
    entries may be ``None``)."""
    n = len(packed)
    arr = lambda ts: (c_void_p * n)(*[ptr(t) for t in ts])
    N, M, d = states.shape
    with _on(states):
        _check(load().mmf_pf_measure_multi(arr(packed), n, n_res, precision, ptr(states), arr(traj_bias), arr(modality_logw), logw_stride,
                                           arr(loglik), ptr(range_flag_t, dtype=torch.int32), N, M, d, stream_of(states)),
               "mmf_pf_measure_multi")


def particle_net_train_fused_multi(args_list, like: torch.Tensor):
    """Several measurement networks' fused calls of one step as one launch (see include/mmf.h)."""
    arr = (MmfTrainFusedArgs * len(args_list))(*args_list)
    with _on(like):
        _check(load().mmf_particle_net_train_fused_multi(arr, len(args_list), stream_of(like)), "mmf_particle_net_train_fused_multi")


def fuse_virtual_sensors(z, tril, w, z_out, tril_out, mode: int):
    K, N, d = z.shape
    with _on(z):
        _check(load().mmf_fuse_virtual_sensors(ptr(z), ptr(tril), ptr(w), ptr(z_out), ptr(tril_out), N, d, K, mode,
                                               stream_of(z)), "mmf_fuse_virtual_sensors")


def ekf_forward_loop(args: MmfEkfLoopArgs, like: torch.Tensor, Sigma_steps: torch.Tensor = None, innov: MmfEkfInnovArgs = None):
    """Enqueue T fused-EKF steps (see include/mmf.h); ``Sigma_steps (T, N, d, d)``: every step's posterior covariance is
    kept there (``mmf_ekf_forward_loop_belief``); ``innov``: the loop of launches with the innovation step, which fills that
    record (``mmf_ekf_forward_loop_innov``; ``Sigma_steps`` may go with it)."""
    with _on(like):
        if innov is not None:
            _check(load().mmf_ekf_forward_loop_innov(ctypes.byref(args), ctypes.byref(innov), ptr(Sigma_steps), stream_of(like)),
                   "mmf_ekf_forward_loop_innov")
        elif Sigma_steps is None:
            _check(load().mmf_ekf_forward_loop(ctypes.byref(args), stream_of(like)), "mmf_ekf_forward_loop")
        else:
            _check(load().mmf_ekf_forward_loop_belief(ctypes.byref(args), ptr(Sigma_steps), stream_of(like)),
                   "mmf_ekf_forward_loop_belief")


LSTM_HIDDEN, LSTM_LAYERS = 512, 2


def ekf_smooth(mu, Sigma, A, mu_pred, q_tril, lag, mu_s, Sigma_s, gain, Sigma_pred=None, resid_mean=None, resid_m2=None):
    """RTS smoothing of a recorded EKF run (``mmf_ekf_smooth``, include/mmf.h): filtered ``mu (T, N, d)`` / ``Sigma (T, N, d,
    d)``, the transitions' Jacobians ``A (T - 1, N, d, d)`` and predictions ``mu_pred (T - 1, N, d)``, ``q_tril (d, d)`` on the
    device, ``lag`` (``None``: the full smoother) -> ``mu_s``, ``Sigma_s``, ``gain (T - 1, N, d, d)`` and, both or neither and
    with ``lag = None`` only, ``resid_mean (T - 1, N, d)`` / ``resid_m2 (T - 1, N, d, d)``.  ``Sigma_pred``: the
    ``(T - 1, N, d, d)`` workspace, allocated when ``None``.  ``T == 0`` or ``N == 0``: nothing to do, no call."""
    T, N, d = mu.shape
    Tm = max(T - 1, 0)
    assert Sigma.shape == (T, N, d, d) and q_tril.shape == (d, d)
    assert mu_s.shape == (T, N, d) and Sigma_s.shape == (T, N, d, d) and gain.shape == (Tm, N, d, d)
    assert A.shape == (Tm, N, d, d) and mu_pred.shape == (Tm, N, d)
    assert resid_mean is None or resid_mean.shape == (Tm, N, d)
    assert resid_m2 is None or resid_m2.shape == (Tm, N, d, d)
    if T == 0 or N == 0:
        return
    if Sigma_pred is None:
        Sigma_pred = torch.empty((Tm, N, d, d), dtype=torch.float32, device=mu.device)
    assert Sigma_pred.shape == (Tm, N, d, d)
    some = lambda t: vp(t) if T >= 2 else None  # (an empty tensor has no address to speak of)
    a = MmfEkfSmoothArgs()
    a.T, a.N, a.d, a.lag = T, N, d, -1 if lag is None else min(int(lag), 0x7fffffff)
    a.mu, a.Sigma, a.A, a.mu_pred, a.q_tril = vp(mu), vp(Sigma), some(A), some(mu_pred), vp(q_tril)
    a.mu_s, a.Sigma_s, a.gain, a.Sigma_pred = vp(mu_s), vp(Sigma_s), some(gain), some(Sigma_pred)
    a.resid_mean, a.resid_m2 = (None if resid_mean is None else some(resid_mean)), (None if resid_m2 is None else some(resid_m2))
    with _on(mu):
        _check(load().mmf_ekf_smooth(ctypes.byref(a), stream_of(mu)), "mmf_ekf_smooth")


def lstm_blob_floats(in_dim: int) -> int:
    return int(load().mmf_lstm_blob_floats(in_dim))


def lstm_pack(tensors, packed: torch.Tensor, in_dim: int):
    """``tensors``: weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, then the same of layer 1 (fp32, contiguous)."""
    with _on(packed):
        _check(load().mmf_lstm_pack(*[ptr(t) for t in tensors], ptr(packed), in_dim, stream_of(packed)), "mmf_lstm_pack")


def lstm_persistent_plan(N: int, T: int) -> int:
    """> 0: workgroups of the persistent form; 0: not eligible (or no device)."""
    return int(load().mmf_lstm_persistent_plan(N, T))


def lstm_sync_words(N: int) -> int:
    return int(load().mmf_lstm_sync_words(N))


def lstm_forward(args: MmfLstmArgs, like: torch.Tensor):
    """The two-layer recurrence over a whole sequence (see include/mmf.h)."""
    with _on(like):
        _check(load().mmf_lstm_forward(ctypes.byref(args), stream_of(like)), "mmf_lstm_forward")


def image_encoder_floats() -> int:
    return int(load().mmf_image_encoder_floats())


def image_encoder_workspace_bytes(n_images: int, n_nets: int) -> int:
    return int(load().mmf_image_encoder_workspace_bytes(n_images, n_nets))


def pack_image_encoder(desc: MmfImageEncoderDesc, packed: torch.Tensor):
    with _on(packed):
        _check(load().mmf_pack_image_encoder(ctypes.byref(desc), ptr(packed), stream_of(packed)),
               "mmf_pack_image_encoder")


ENCODER_DEFAULT, ENCODER_SPANNING_POOL = 0, 1


def image_encoder(blobs, images: torch.Tensor, feat: torch.Tensor, workspace: torch.Tensor,
                  range_flag, precision: int, variant: int = ENCODER_DEFAULT):
    n = len(blobs)
    arr = (c_void_p * n)(*[ptr(b) for b in blobs])
    N = images.shape[0]
    assert tuple(images.shape[1:]) == (32, 32) and tuple(feat.shape) == (n, N, 64)
    with _on(images):
        _check(load().mmf_image_encoder(arr, n, ptr(images), ptr(feat),
                                        ptr(workspace, dtype=torch.uint8),
                                        ptr(range_flag, dtype=torch.int32), precision, variant, N,
                                        stream_of(images)),
               "mmf_image_encoder")


def traj_program(prog: torch.Tensor, n_instr: int, weights: torch.Tensor, io_tensors, R: int,
                 n_slots: int = TRAJ_SLOTS, vec_width: int = 128):
    """``prog``: uint8 device tensor holding ``n_instr`` MmfTrajInstr; ``io_tensors``: up to
    TRAJ_MAX_IO float32 device tensors (``None`` = unused); ``n_slots`` / ``vec_width``: what the
    program uses (sizes the launch's LDS)."""
    arr = (c_void_p * TRAJ_MAX_IO)(*[ptr(t) for t in io_tensors] + [None] * (TRAJ_MAX_IO - len(io_tensors)))
    with _on(weights):
        _check(load().mmf_traj_program(ptr(prog, dtype=torch.uint8), n_instr, ptr(weights), arr, R,
                                       n_slots, vec_width, stream_of(weights)), "mmf_traj_program")


def pf_train_finalize(args: MmfPfTrainFinalizeArgs, like: torch.Tensor):
    with _on(like):
        _check(load().mmf_pf_train_finalize(ctypes.byref(args), stream_of(like)), "mmf_pf_train_finalize")


def traj_pack(desc: torch.Tensor, n_desc: int, blob: torch.Tensor):
    with _on(blob):
        _check(load().mmf_traj_pack(ptr(desc, dtype=torch.uint8), n_desc, ptr(blob), stream_of(blob)), "mmf_traj_pack")


def traj_weight_grads(desc: torch.Tensor, n_desc: int, stash: torch.Tensor, dz: torch.Tensor, grads: torch.Tensor,
                      partials, n_slices: int, R: int):
    """``desc``: uint8 device tensor of ``n_desc`` MmfTrajGradDesc; ``stash`` / ``dz``: ``(R, ld)``; ``grads``: flat."""
    with _on(grads):
        _check(load().mmf_traj_weight_grads(ptr(desc, dtype=torch.uint8), n_desc, ptr(stash), stash.shape[1], ptr(dz),
                                            dz.shape[1], ptr(grads), grads.numel(), ptr(partials), n_slices, R,
                                            stream_of(grads)), "mmf_traj_weight_grads")


def fc64_train_forward(x, w, b, y):
    R, K = x.shape
    partial = torch.empty((max(1, K // 512), R, 64), dtype=torch.float32, device=x.device)
    with _on(x):
        _check(load().mmf_fc64_train_forward(ptr(x), ptr(w), ptr(b), ptr(y), ptr(partial), R, K, stream_of(x)),
               "mmf_fc64_train_forward")


def fc64_train_backward(g, x, w, dx, dw, db):
    R, K = x.shape
    with _on(x):
        _check(load().mmf_fc64_train_backward(ptr(g), ptr(x), ptr(w), ptr(dx), ptr(dw), ptr(db), R, K, stream_of(x)),
               "mmf_fc64_train_backward")


def pf_reweight_backward(logw_out, states, g_estimate, g_logw_out, d_a, d_states):
    N, M, d = states.shape
    with _on(states):
        _check(load().mmf_pf_reweight_backward(ptr(logw_out), ptr(states), ptr(g_estimate), ptr(g_logw_out), ptr(d_a),
                                               ptr(d_states), N, M, d, stream_of(states)), "mmf_pf_reweight_backward")


def pf_init_particles(mean, covariance, eps, states, logw, not_pd):
    N, M, d = eps.shape
    with _on(eps):
        _check(load().mmf_pf_init_particles(ptr(mean), ptr(covariance), ptr(eps), ptr(states), ptr(logw),
                                            ptr(not_pd, dtype=torch.int32), N, M, d, stream_of(eps)),
               "mmf_pf_init_particles")


def pf_dedup_plan(M: int, d: int, resample_mode: int, soft_alpha: float = 0.0, recording: bool = False) -> bool:
    """Whether ``mmf_pf_forward_loop_dedup`` takes the run path at these sizes / modes (include/mmf.h)."""
    return load().mmf_pf_dedup_plan(int(M), int(d), int(resample_mode), float(soft_alpha), int(bool(recording))) == 1


def pf_dedup_workspace_words(N: int, M: int) -> int:
    return int(load().mmf_pf_dedup_workspace_words(int(N), int(M)))


def pf_dedup_deal(n_runs, N: int, M: int, tile: int, grid: int, b: int, out, cap: int) -> int:
    """``mmf_pf_dedup_deal`` (include/mmf.h): workgroup ``b``'s list of real tiles of the run-consuming dynamics launch.
    ``n_runs`` / ``out``: contiguous int32 numpy arrays on the HOST (or ``None``: the call refuses it).  Returns the list's
    length, negative for a refused argument."""
    p = lambda x: None if x is None else x.ctypes.data
    return int(load().mmf_pf_dedup_deal(p(n_runs), int(N), int(M), int(tile), int(grid), int(b), p(out), int(cap)))


def pf_dedup_workspace(words: torch.Tensor, N: int, M: int):
    """Carve ``MmfPfDedupWorkspace`` out of one int32 tensor of ``pf_dedup_workspace_words(N, M)`` elements:
    ``rank (N, M) | run_anc (N, M + 1) | run_start (N, M + 1) | n_runs (N)``."""
    assert words.dtype == torch.int32 and words.is_contiguous() and words.numel() >= N * M + 2 * N * (M + 1) + N
    ws = MmfPfDedupWorkspace()
    base, o1, o2, o3 = words.data_ptr(), N * M, N * M + N * (M + 1), N * M + 2 * N * (M + 1)
    ws.rank, ws.run_anc, ws.run_start, ws.n_runs = base, base + 4 * o1, base + 4 * o2, base + 4 * o3
    return ws


def pf_resample_runs(loglik, logw_in, states, u, estimate, indices_out, rank, run_anc, run_start, n_runs, *,
                     logw_out=None, cov=None, ess=None, log_evidence=None):
    """K1's run variant alone (``mmf_pf_resample_runs``): the run table of plain systematic resampling."""
    N, M, d = states.shape
    i32 = torch.int32
    with _on(states):
        _check(load().mmf_pf_resample_runs(ptr(loglik), ptr(logw_in), ptr(states), ptr(u), ptr(estimate), ptr(logw_out),
                                           ptr(indices_out, dtype=i32), ptr(rank, dtype=i32), ptr(run_anc, dtype=i32),
                                           ptr(run_start, dtype=i32), ptr(n_runs, dtype=i32), N, M, d, ptr(cov), ptr(ess),
                                           ptr(log_evidence), stream_of(states)), "mmf_pf_resample_runs")


def pf_dynamics_runs(packed, n_res, precision, states_prev, traj_bias, noise, scale_tril, rank, run_anc, run_start, n_runs,
                     states_out, range_flag, N, M, d):
    """The run-consuming dynamics launch alone (``mmf_pf_dynamics_runs``): the network once per run of the table."""
    i32 = torch.int32
    with _on(states_prev):
        _check(load().mmf_pf_dynamics_runs(ptr(packed), n_res, precision, ptr(states_prev), ptr(traj_bias), ptr(noise),
                                           ptr(scale_tril), ptr(rank, dtype=i32), ptr(run_anc, dtype=i32),
                                           ptr(run_start, dtype=i32), ptr(n_runs, dtype=i32), ptr(states_out),
                                           ptr(range_flag, dtype=i32), N, M, d, stream_of(states_prev)),
               "mmf_pf_dynamics_runs")


def pf_dynamics_runs_philox(packed, n_res, precision, states_prev, traj_bias, seed, step, traj0, scale_tril, rank, run_anc,
                            run_start, n_runs, states_out, range_flag, N, M, d):
    i32 = torch.int32
    with _on(states_prev):
        _check(load().mmf_pf_dynamics_runs_philox(ptr(packed), n_res, precision, ptr(states_prev), ptr(traj_bias), seed, step,
                                                  traj0, ptr(scale_tril), ptr(rank, dtype=i32), ptr(run_anc, dtype=i32),
                                                  ptr(run_start, dtype=i32), ptr(n_runs, dtype=i32), ptr(states_out),
                                                  ptr(range_flag, dtype=i32), N, M, d, stream_of(states_prev)),
               "mmf_pf_dynamics_runs_philox")


def pf_forward_loop(args: MmfPfLoopArgs, like: torch.Tensor, events=None, event_stride: int = 1, *,
                    ess_threshold: float = None, resampled_steps=None, dedup: MmfPfDedupWorkspace = None,
                    history: MmfPfHistory = None, regularise: MmfPfLoopRegularise = None) -> int:
    """Enqueue T filter steps; returns the final-location bits (see include/mmf.h).
    ``events``: optional flat list of created ``torch.cuda.Event`` (timing) recorded in C
    around the launches of every ``event_stride``-th step.
    ``ess_threshold``: ESS-triggered resampling (``mmf_pf_forward_loop_adaptive``), ``resampled_steps`` its ``(T, N)`` int32
    decisions or ``None``.  ``dedup``: the run-table workspace (``mmf_pf_forward_loop_dedup``: the dynamics network once per
    distinct resampled ancestor; plain resampling only) or ``None``.  ``history``: the arrays a smoother needs
    (``mmf_pf_forward_loop_history``: the loop of launches with the same threshold / workspace) or ``None``.
    ``regularise``: regularised resampling (``mmf_pf_forward_loop_regularised``: the loop of launches with one jitter launch
    after every K1, the threshold and the history as given, no run table) or ``None``."""
    loc = c_int32(0)
    args.final_location = ctypes.pointer(loc)
    if events is not None:
        arr = (c_void_p * len(events))(*[e.cuda_event for e in events])
        args.events = arr
        args.event_stride = event_stride
    with _on(like):
        if regularise is not None:
            _check(load().mmf_pf_forward_loop_regularised(
                ctypes.byref(args), None if history is None else ctypes.byref(history),
                0.0 if ess_threshold is None else float(ess_threshold), ptr(resampled_steps, dtype=torch.int32),
                ctypes.byref(regularise), stream_of(like)), "mmf_pf_forward_loop_regularised")
        elif history is not None:
            _check(load().mmf_pf_forward_loop_history(
                ctypes.byref(args), ctypes.byref(history), 0.0 if ess_threshold is None else float(ess_threshold),
                ptr(resampled_steps, dtype=torch.int32), None if dedup is None else ctypes.byref(dedup), stream_of(like)),
                "mmf_pf_forward_loop_history")
        elif ess_threshold is not None:
            _check(load().mmf_pf_forward_loop_adaptive(ctypes.byref(args), float(ess_threshold),
                                                       ptr(resampled_steps, dtype=torch.int32), stream_of(like)),
                   "mmf_pf_forward_loop_adaptive")
        elif dedup is not None:
            _check(load().mmf_pf_forward_loop_dedup(ctypes.byref(args), ctypes.byref(dedup), stream_of(like)),
                   "mmf_pf_forward_loop_dedup")
        else:
            _check(load().mmf_pf_forward_loop(ctypes.byref(args), stream_of(like)), "mmf_pf_forward_loop")
    return int(loc.value)


def pf_smooth_lds_bytes(M: int) -> int:
    return int(load().mmf_pf_smooth_lds_bytes(int(M)))


def pf_smooth(states_steps, loglik_steps, logw_in_steps, logw_in0, indices_steps, lag: int, mean, cov=None, unique=None):
    """Ancestry smoothing of a filter run's history (``mmf_pf_smooth``, include/mmf.h): ``states_steps (T, N, M, d)``,
    ``loglik_steps (T, N, M)``, ``logw_in_steps (T, N, M)`` / ``logw_in0 (N, M)`` / ``indices_steps (T, N, M)`` int32 each or
    ``None`` -> ``mean (T, N, d)``, ``cov (T, N, d, d)`` and ``unique (T, N)`` int32, each of the last two or ``None``."""
    T, N, M, d = states_steps.shape
    assert loglik_steps.shape == (T, N, M) and mean.shape == (T, N, d)
    assert logw_in_steps is None or logw_in_steps.shape == (T, N, M)
    assert logw_in0 is None or logw_in0.shape == (N, M)
    assert indices_steps is None or indices_steps.shape == (T, N, M)
    assert cov is None or cov.shape == (T, N, d, d)
    assert unique is None or unique.shape == (T, N)
    a = MmfPfSmoothArgs()
    a.T, a.N, a.M, a.d, a.lag = T, N, M, d, int(lag)
    a.states_steps, a.loglik_steps, a.logw_in_steps, a.logw_in0 = vp(states_steps), vp(loglik_steps), vp(logw_in_steps), vp(logw_in0)
    a.indices_steps, a.mean, a.cov, a.unique = vp(indices_steps, torch.int32), vp(mean), vp(cov), vp(unique, torch.int32)
    with _on(states_steps):
        _check(load().mmf_pf_smooth(ctypes.byref(a), stream_of(states_steps)), "mmf_pf_smooth")


def _smooth_history(a, states_steps, pred_steps, loglik_steps, logw_in_steps, scale_tril):
    """The history the marginal, pair-moment and simulation smoothers share, checked and put into their struct ``a``: the
    sizes and the five inputs; ``pred_steps`` is required from ``T = 2`` on and passed as null below (no transition)."""
    T, N, M, d = states_steps.shape
    assert loglik_steps.shape == (T, N, M) and scale_tril.shape == (d, d)
    assert logw_in_steps is None or logw_in_steps.shape == (T, N, M)
    assert T < 2 or (pred_steps is not None and pred_steps.shape == (T - 1, N, M, d))
    a.T, a.N, a.M, a.d = T, N, M, d
    a.states_steps, a.pred_steps = vp(states_steps), vp(pred_steps if T >= 2 else None)
    a.loglik_steps, a.logw_in_steps, a.scale_tril = vp(loglik_steps), vp(logw_in_steps), vp(scale_tril)


def pf_smooth_marginal(states_steps, pred_steps, loglik_steps, logw_in_steps, scale_tril, weights, mean, cov=None, ess=None,
                       logd=None):
    """Marginal (forward-filter backward-smoothing) particle smoothing of a filter run's history
    (``mmf_pf_smooth_marginal``, include/mmf.h): ``states_steps (T, N, M, d)``, ``pred_steps (T - 1, N, M, d)`` the dynamics
    means ``f(X_t, u_{t+1})`` (``None`` allowed for ``T < 2``), ``loglik_steps (T, N, M)``, ``logw_in_steps (T, N, M)`` or
    ``None`` (uniform), ``scale_tril (d, d)`` on the device -> ``weights (T, N, M)``, ``mean (T, N, d)``, ``cov (T, N, d, d)``
    and ``ess (T, N)``, each of the last two or ``None``.  ``logd``: the ``(T - 1, N, M)`` workspace, allocated when ``None``."""
    T, N, M, d = states_steps.shape
    assert weights.shape == (T, N, M) and mean.shape == (T, N, d)
    assert cov is None or cov.shape == (T, N, d, d)
    assert ess is None or ess.shape == (T, N)
    if T >= 2:
        if logd is None:
            logd = torch.empty((T - 1, N, M), dtype=torch.float32, device=states_steps.device)
        assert logd.shape == (T - 1, N, M)
    else:
        logd = None
    a = MmfPfSmoothMarginalArgs()
    _smooth_history(a, states_steps, pred_steps, loglik_steps, logw_in_steps, scale_tril)
    a.logd, a.weights, a.mean, a.cov, a.ess = vp(logd), vp(weights), vp(mean), vp(cov), vp(ess)
    with _on(states_steps):
        _check(load().mmf_pf_smooth_marginal(ctypes.byref(a), stream_of(states_steps)), "mmf_pf_smooth_marginal")


def pf_smooth_pair_workspace_floats(T: int, N: int, M: int, d: int) -> int:
    return int(load().mmf_pf_smooth_pair_workspace_floats(int(T), int(N), int(M), int(d)))


def pf_smooth_pair_moments(states_steps, pred_steps, loglik_steps, logw_in_steps, scale_tril, weights, logd, residual_mean,
                           residual_second_moment, workspace=None):
    """Two-slice smoothing moments of a filter run's history (``mmf_pf_smooth_pair_moments``, include/mmf.h) after a
    ``pf_smooth_marginal`` call on the same history and ``scale_tril``: the inputs of that call, its ``weights (T, N, M)`` and
    its ``logd (T - 1, N, M)`` -> ``residual_mean (T - 1, N, d)`` and ``residual_second_moment (T - 1, N, d, d)`` (raw) of
    ``X_{t+1}[j] - F_t[i]`` over the particle pairs.  ``workspace``: ``pf_smooth_pair_workspace_floats(T, N, M, d)`` floats,
    allocated when ``None``.  ``T < 2``: there is no transition, nothing is written."""
    T, N, M, d = states_steps.shape
    Tm = max(T - 1, 0)
    assert weights.shape == (T, N, M)
    assert residual_mean.shape == (Tm, N, d) and residual_second_moment.shape == (Tm, N, d, d)
    if T >= 2:
        assert logd is not None and logd.shape == (T - 1, N, M)
        need = pf_smooth_pair_workspace_floats(T, N, M, d)
        if workspace is None:
            workspace = torch.empty((max(need, 1),), dtype=torch.float32, device=states_steps.device)
        assert workspace.numel() >= need
    else:
        logd = workspace = None
    a = MmfPfSmoothPairArgs()
    _smooth_history(a, states_steps, pred_steps, loglik_steps, logw_in_steps, scale_tril)
    a.weights, a.logd, a.workspace = vp(weights), vp(logd), vp(workspace)
    a.residual_mean, a.residual_second_moment = vp(residual_mean), vp(residual_second_moment)
    with _on(states_steps):
        _check(load().mmf_pf_smooth_pair_moments(ctypes.byref(a), stream_of(states_steps)), "mmf_pf_smooth_pair_moments")


def pf_smooth_simulate(states_steps, pred_steps, loglik_steps, logw_in_steps, scale_tril, uniforms, indices, trajectories, mean,
                       cov=None):
    """Backward-simulation particle smoothing of a filter run's history (``mmf_pf_smooth_simulate``, include/mmf.h):
    ``states_steps (T, N, M, d)``, ``pred_steps (T - 1, N, M, d)`` the dynamics means ``f(X_t, u_{t+1})`` (``None`` allowed for
    ``T < 2``), ``loglik_steps (T, N, M)``, ``logw_in_steps (T, N, M)`` or ``None`` (uniform), ``scale_tril (d, d)`` on the
    device, ``uniforms (T, N, S)`` in ``[0, 1)`` -> ``indices (T, N, S)`` int32, ``trajectories (T, N, S, d)``,
    ``mean (T, N, d)`` and ``cov (T, N, d, d)`` or ``None``."""
    T, N, M, d = states_steps.shape
    assert uniforms.dim() == 3 and uniforms.shape[:2] == (T, N)
    S = uniforms.shape[2]
    assert mean.shape == (T, N, d)
    assert indices.shape == (T, N, S) and trajectories.shape == (T, N, S, d)
    assert cov is None or cov.shape == (T, N, d, d)
    a = MmfPfSmoothSimulateArgs()
    _smooth_history(a, states_steps, pred_steps, loglik_steps, logw_in_steps, scale_tril)
    a.S, a.uniforms, a.indices = S, vp(uniforms), vp(indices, torch.int32)
    a.trajectories, a.mean, a.cov = vp(trajectories), vp(mean), vp(cov)
    with _on(states_steps):
        _check(load().mmf_pf_smooth_simulate(ctypes.byref(a), stream_of(states_steps)), "mmf_pf_smooth_simulate")


def pf_smooth_map(states_steps, pred_steps, loglik_steps, logw_in_steps, scale_tril, indices, path, log_posterior, v=None,
                  step_max=None, backpointers=None):
    """MAP path smoothing of a filter run's history (``mmf_pf_smooth_map``, include/mmf.h): ``states_steps (T, N, M, d)``,
    ``pred_steps (T - 1, N, M, d)`` the dynamics means ``f(X_t, u_{t+1})`` (``None`` allowed for ``T < 2``),
    ``loglik_steps (T, N, M)``, ``logw_in_steps (T, N, M)`` or ``None`` (step 0 alone is read: the prior over the step-0 set),
    ``scale_tril (d, d)`` on the device -> ``indices (T, N)`` int32, ``path (T, N, d)``, ``log_posterior (N)``.  ``v (T, N, M)``,
    ``step_max (T, N)`` and ``backpointers (T, N, M)`` int32 -- the recursion's values, their per-step maxima and its
    decisions -- are allocated when ``None``."""
    T, N, M, d = states_steps.shape
    dev = states_steps.device
    assert indices.shape == (T, N) and path.shape == (T, N, d) and log_posterior.shape == (N,)
    if v is None:
        v = torch.empty((T, N, M), dtype=torch.float32, device=dev)
    if step_max is None:
        step_max = torch.empty((T, N), dtype=torch.float32, device=dev)
    if backpointers is None:
        backpointers = torch.empty((T, N, M), dtype=torch.int32, device=dev)
    assert v.shape == (T, N, M) and step_max.shape == (T, N) and backpointers.shape == (T, N, M)
    a = MmfPfSmoothMapArgs()
    _smooth_history(a, states_steps, pred_steps, loglik_steps, logw_in_steps, scale_tril)
    a.v, a.step_max, a.backpointers = vp(v), vp(step_max), vp(backpointers, torch.int32)
    a.indices, a.path, a.log_posterior = vp(indices, torch.int32), vp(path), vp(log_posterior)
    with _on(states_steps):
        _check(load().mmf_pf_smooth_map(ctypes.byref(a), stream_of(states_steps)), "mmf_pf_smooth_map")


def _summary_rows(states, log_a, log_b):
    """``lead, R, M, d`` of ``states (lead..., M, d)``, ``R`` the product of ``lead``; ``log_a``, ``log_b``: ``(lead..., M)`` or ``None``."""
    lead, (M, d) = tuple(states.shape[:-2]), states.shape[-2:]
    R = 1
    for n in lead:
        R *= int(n)
    assert log_a is None or tuple(log_a.shape) == lead + (M,)
    assert log_b is None or tuple(log_b.shape) == lead + (M,)
    return lead, R, M, d


def _summary_workspace(a, need: int, like):
    """``need`` bytes of float64 workspace on ``like``'s device into ``a``; the caller keeps the tensor until the launch is made."""
    work = torch.empty((need // 8,), dtype=torch.float64, device=like.device) if need else None
    a.workspace, a.workspace_bytes = vp(work, torch.float64), need
    return work


def pf_quantiles_lds_bytes(M: int) -> int:
    return int(load().mmf_pf_quantiles_lds_bytes(int(M)))


def pf_quantiles(states, log_a, log_b, probs, quantiles, query=None, cdf=None):
    """Weighted quantiles and the weighted CDF of particle sets on the integer fixed-point weights of K1
    (``mmf_pf_quantiles``, include/mmf.h): ``states (..., M, d)`` -- ``R`` rows, the product of the leading sizes -- with
    log-weights ``log_a + log_b``, each ``(..., M)`` or ``None`` (0; both ``None``: uniform), and ``probs``, up to 16 host
    floats in ``[0, 1]`` -> ``quantiles (..., Q, d)`` (``None`` allowed for an empty ``probs``; not written then).  ``query
    (..., d)`` with ``cdf (..., d)``, both or neither: the weighted share of the particles at or below the query, per
    dimension."""
    probs = [float(p) for p in probs]
    Q = len(probs)
    if Q > QUANTILES_MAX:
        raise MmfError(f"mmf_pf_quantiles takes at most {QUANTILES_MAX} probabilities, got {Q}")
    lead, R, M, d = _summary_rows(states, log_a, log_b)
    assert quantiles is None or tuple(quantiles.shape) == lead + (Q, d)
    assert (query is None) == (cdf is None)
    assert query is None or (tuple(query.shape) == lead + (d,) and tuple(cdf.shape) == lead + (d,))
    a = MmfPfQuantilesArgs()
    a.R, a.M, a.d, a.Q = R, M, d, Q
    for i, p in enumerate(probs):
        a.probs[i] = p
    a.states, a.log_a, a.log_b, a.query = vp(states), vp(log_a), vp(log_b), vp(query)
    a.quantiles, a.cdf = vp(quantiles), vp(cdf)
    with _on(states):
        _check(load().mmf_pf_quantiles(ctypes.byref(a), stream_of(states)), "mmf_pf_quantiles")


def pf_scores_workspace_bytes(R: int, M: int, d: int) -> int:
    return int(load().mmf_pf_scores_workspace_bytes(int(R), int(M), int(d)))


def pf_scores(states, log_a, log_b, truth, crps, energy, spread, scale=None):
    """CRPS per state dimension and the energy score of weighted particle sets against a true state, with their sharpness
    terms (``mmf_pf_scores``, include/mmf.h): ``states (..., M, d)`` -- ``R`` rows, the product of the leading sizes -- with
    log-weights ``log_a + log_b``, each ``(..., M)`` or ``None`` (0; both ``None``: uniform), and ``truth (..., d)`` ->
    ``crps (..., d)``, ``energy (...)``, ``spread (..., d + 1)``, each of which may be ``None`` (not all three); ``truth`` may
    be ``None`` with ``spread`` alone.  ``scale``: ``None`` (ones) or ``d`` positive finite host floats dividing the
    coordinates inside the Euclidean norm of ``energy`` and ``spread[..., d]``.  The workspace of the partial sums is allocated
    here, on the tensors' device."""
    lead, R, M, d = _summary_rows(states, log_a, log_b)
    scale = [1.0] * d if scale is None else [float(s) for s in scale]
    if len(scale) != d or d > MMF_MAX_STATE_DIM:
        raise MmfError(f"mmf_pf_scores takes one scale per state dimension (d = {d} <= {MMF_MAX_STATE_DIM}), got {len(scale)}")
    assert truth is None or tuple(truth.shape) == lead + (d,)
    assert crps is None or tuple(crps.shape) == lead + (d,)
    assert energy is None or tuple(energy.shape) == lead
    assert spread is None or tuple(spread.shape) == lead + (d + 1,)
    a = MmfPfScoresArgs()
    a.R, a.M, a.d = R, M, d
    for i, s in enumerate(scale):
        a.scale[i] = s
    a.states, a.log_a, a.log_b, a.truth = vp(states), vp(log_a), vp(log_b), vp(truth)
    a.crps, a.energy, a.spread = vp(crps), vp(energy), vp(spread)
    with _on(states):
        work = _summary_workspace(a, pf_scores_workspace_bytes(R, M, d), states)
        _check(load().mmf_pf_scores(ctypes.byref(a), stream_of(states)), "mmf_pf_scores")


def pf_scores_backward_workspace_bytes(R: int, M: int, d: int) -> int:
    return int(load().mmf_pf_scores_backward_workspace_bytes(int(R), int(M), int(d)))


def pf_scores_backward(states, log_a, log_b, truth, g_crps, g_energy, *, g_states=None, g_logw=None, scale=None):
    """The gradients of ``pf_scores``' CRPS and energy score (``mmf_pf_scores_backward``, include/mmf.h): ``states (..., M,
    d)``, log-weights ``log_a + log_b``, each ``(..., M)`` or ``None`` (0), ``truth (..., d)`` and the upstream gradients
    ``g_crps (..., d)`` and ``g_energy (...)``, either of which may be ``None`` (that score's terms are left out; not both) ->
    ``g_states`` like ``states`` and ``g_logw (..., M)``, the gradient with respect to ``log_a`` and to ``log_b`` alike,
    either of which may be ``None`` (not both); written in place.  ``scale``: ``pf_scores``'.  The workspace is allocated
    here, on the tensors' device."""
    lead, R, M, d = _summary_rows(states, log_a, log_b)
    scale = [1.0] * d if scale is None else [float(s) for s in scale]
    if len(scale) != d or d > MMF_MAX_STATE_DIM:
        raise MmfError(f"mmf_pf_scores_backward takes one scale per state dimension (d = {d} <= {MMF_MAX_STATE_DIM}), got {len(scale)}")
    assert truth is not None and tuple(truth.shape) == lead + (d,)
    assert g_crps is None or tuple(g_crps.shape) == lead + (d,)
    assert g_energy is None or tuple(g_energy.shape) == lead
    assert g_states is None or tuple(g_states.shape) == lead + (M, d)
    assert g_logw is None or tuple(g_logw.shape) == lead + (M,)
    a = MmfPfScoresBackwardArgs()
    a.R, a.M, a.d = R, M, d
    for i, s in enumerate(scale):
        a.scale[i] = s
    a.states, a.log_a, a.log_b, a.truth = vp(states), vp(log_a), vp(log_b), vp(truth)
    a.g_crps, a.g_energy, a.g_states, a.g_logw = vp(g_crps), vp(g_energy), vp(g_states), vp(g_logw)
    with _on(states):
        work = _summary_workspace(a, pf_scores_backward_workspace_bytes(R, M, d), states)
        _check(load().mmf_pf_scores_backward(ctypes.byref(a), stream_of(states)), "mmf_pf_scores_backward")


def pf_predictive_workspace_bytes(R: int, M: int, d: int) -> int:
    return int(load().mmf_pf_predictive_workspace_bytes(int(R), int(M), int(d)))


def pf_predictive(centres, log_a, log_b, scale_tril, truth=None, *, mean=None, covariance=None, log_score=None, pit=None,
                  spread=None, crps=None):
    """Closed-form scores of predictive Gaussian mixtures with one shared covariance (``mmf_pf_predictive``, include/mmf.h):
    ``centres (..., M, d)`` -- ``R`` rows, the product of the leading sizes -- with log-weights ``log_a + log_b``, each
    ``(..., M)`` or ``None`` (0; both ``None``: uniform), the process noise's ``scale_tril (d, d)`` and ``truth (..., d)`` or
    ``None`` -> ``mean (..., d)``, ``covariance (..., d, d)``, ``log_score (...)``, ``pit (..., d)``, ``spread (..., d)``,
    ``crps (..., d)``, each of which may be ``None`` (not all six); ``log_score``, ``pit`` and ``crps`` need the truth.  The
    outputs are written in place, so a contiguous slice of a larger tensor serves.  The workspace of the partial sums is
    allocated here, on the tensors' device, when ``spread`` or ``crps`` is asked for."""
    lead, R, M, d = _summary_rows(centres, log_a, log_b)
    assert tuple(scale_tril.shape) == (d, d)
    assert truth is None or tuple(truth.shape) == lead + (d,)
    for out, tail in ((mean, (d,)), (covariance, (d, d)), (log_score, ()), (pit, (d,)), (spread, (d,)), (crps, (d,))):
        assert out is None or tuple(out.shape) == lead + tail
    a = MmfPfPredictiveArgs()
    a.R, a.M, a.d = R, M, d
    a.centres, a.log_a, a.log_b, a.scale_tril, a.truth = vp(centres), vp(log_a), vp(log_b), vp(scale_tril), vp(truth)
    a.mean, a.covariance, a.log_score, a.pit = vp(mean), vp(covariance), vp(log_score), vp(pit)
    a.spread, a.crps = vp(spread), vp(crps)
    with _on(centres):
        pairs = spread is not None or crps is not None
        work = _summary_workspace(a, pf_predictive_workspace_bytes(R, M, d) if pairs else 0, centres)
        _check(load().mmf_pf_predictive(ctypes.byref(a), stream_of(centres)), "mmf_pf_predictive")


def pf_density_workspace_bytes(R: int, M: int, d: int) -> int:
    return int(load().mmf_pf_density_workspace_bytes(int(R), int(M), int(d)))


def pf_density(states, log_a, log_b, truth, *, rule="silverman", bandwidth=None, min_bandwidth=None, log_density=None,
               log_score=None, entropy=None, mode=None, mode_index=None, bandwidth_out=None):
    """Gaussian product-kernel density of weighted particle sets (``mmf_pf_density``, include/mmf.h): ``states (..., M, d)``
    -- ``R`` rows, the product of the leading sizes -- with log-weights ``log_a + log_b``, each ``(..., M)`` or ``None`` (0;
    both ``None``: uniform), and ``truth (..., d)`` or ``None`` -> ``log_density (..., M)``, ``log_score (...)`` (needs the
    truth), ``entropy (...)``, ``mode (..., d)``, ``mode_index (...)`` int32, ``bandwidth_out (..., d)``, each of which may be
    ``None`` (not all six).  ``rule``: ``"silverman"`` or ``"scott"`` with ``min_bandwidth``, ``d`` positive finite host
    floats, the floor of the bandwidths; ``"fixed"`` with ``bandwidth``, ``d`` positive finite host floats.  The workspace of
    the partial results is allocated here, on the tensors' device."""
    lead, R, M, d = _summary_rows(states, log_a, log_b)
    if rule not in DENSITY_RULES:
        raise MmfError(f"mmf_pf_density: rule must be one of {sorted(DENSITY_RULES)}, got {rule!r}")
    given = bandwidth if rule == "fixed" else min_bandwidth
    given = [] if given is None else [float(h) for h in given]
    if len(given) != d or d > MMF_MAX_STATE_DIM:
        raise MmfError(f"mmf_pf_density takes one {'bandwidth' if rule == 'fixed' else 'min_bandwidth'} per state dimension "
                       f"(d = {d} <= {MMF_MAX_STATE_DIM}), got {len(given)}")
    assert truth is None or tuple(truth.shape) == lead + (d,)
    assert log_density is None or tuple(log_density.shape) == lead + (M,)
    assert log_score is None or tuple(log_score.shape) == lead
    assert entropy is None or tuple(entropy.shape) == lead
    assert mode is None or tuple(mode.shape) == lead + (d,)
    assert mode_index is None or tuple(mode_index.shape) == lead
    assert bandwidth_out is None or tuple(bandwidth_out.shape) == lead + (d,)
    a = MmfPfDensityArgs()
    a.R, a.M, a.d, a.rule = R, M, d, DENSITY_RULES[rule]
    for i, h in enumerate(given):
        (a.bandwidth if rule == "fixed" else a.min_bandwidth)[i] = h
    a.states, a.log_a, a.log_b, a.truth = vp(states), vp(log_a), vp(log_b), vp(truth)
    a.log_density, a.log_score, a.entropy = vp(log_density), vp(log_score), vp(entropy)
    a.mode, a.mode_index, a.bandwidth_out = vp(mode), vp(mode_index, torch.int32), vp(bandwidth_out)
    with _on(states):
        work = _summary_workspace(a, pf_density_workspace_bytes(R, M, d), states)
        _check(load().mmf_pf_density(ctypes.byref(a), stream_of(states)), "mmf_pf_density")


def pf_raster(states, log_a, log_b, center, bandwidth, density, *, dims, step):
    """Belief maps, the 2-D marginal of the product-kernel density of weighted particle sets on a grid (``mmf_pf_raster``,
    include/mmf.h): ``states (..., M, d)`` -- ``R`` rows, the product of the leading sizes -- with log-weights ``log_a +
    log_b``, each ``(..., M)`` or ``None`` (0; both ``None``: uniform), ``center (..., 2)`` and ``bandwidth (..., 2)`` along
    ``dims = (dx, dy)``, two distinct state dimensions, and ``step``, two positive finite host floats -> ``density (..., Gy,
    Gx)``, whose shape gives the cells (2 .. 128 each).  Written in place, so a contiguous slice of a larger tensor serves."""
    lead, R, M, d = _summary_rows(states, log_a, log_b)
    dims, step = [int(k) for k in dims], [float(s) for s in step]
    if len(dims) != 2 or len(step) != 2:
        raise MmfError(f"mmf_pf_raster takes two state dimensions and two steps, got dims = {dims!r}, step = {step!r}")
    assert tuple(center.shape) == lead + (2,) and tuple(bandwidth.shape) == lead + (2,)
    assert density.dim() == len(lead) + 2 and tuple(density.shape[:-2]) == lead
    a = MmfPfRasterArgs()
    a.R, a.M, a.d = R, M, d
    for k in range(2):
        a.dims[k], a.step[k] = dims[k], step[k]
    a.cells[0], a.cells[1] = int(density.shape[-1]), int(density.shape[-2])
    a.states, a.log_a, a.log_b = vp(states), vp(log_a), vp(log_b)
    a.center, a.bandwidth, a.density = vp(center), vp(bandwidth), vp(density)
    with _on(states):
        _check(load().mmf_pf_raster(ctypes.byref(a), stream_of(states)), "mmf_pf_raster")


def pf_modes_workspace_bytes(R: int, M: int, d: int) -> int:
    return int(load().mmf_pf_modes_workspace_bytes(int(R), int(M), int(d)))


def pf_modes(states, log_a, log_b, log_density, bandwidth, *, link_radius=3.0, max_modes=4, parent=None, labels=None, count=None,
             index=None, modes=None, mass=None, mean=None):
    """Quick-shift modes of weighted particle sets (``mmf_pf_modes``, include/mmf.h): ``states (..., M, d)`` -- ``R`` rows, the
    product of the leading sizes -- with log-weights ``log_a + log_b``, each ``(..., M)`` or ``None`` (0; both ``None``:
    uniform), ``log_density (..., M)`` and ``bandwidth (..., d)`` as ``mmf_pf_density`` writes them, ``link_radius`` (finite,
    positive, in bandwidths) and ``max_modes = K`` (1 .. 8) -> ``parent``, ``labels (..., M)`` int32, ``count (...)`` int32,
    ``index (..., K)`` int32, ``modes (..., K, d)``, ``mass (..., K)``, ``mean (..., K, d)``, each of which may be ``None`` (not
    all seven).  The workspace is allocated here, on the tensors' device."""
    lead, R, M, d = _summary_rows(states, log_a, log_b)
    K = int(max_modes)
    if not 1 <= K <= MODES_MAX:
        raise MmfError(f"mmf_pf_modes reports 1 .. {MODES_MAX} modes, got max_modes = {max_modes!r}")
    assert tuple(log_density.shape) == lead + (M,) and tuple(bandwidth.shape) == lead + (d,)
    assert parent is None or tuple(parent.shape) == lead + (M,)
    assert labels is None or tuple(labels.shape) == lead + (M,)
    assert count is None or tuple(count.shape) == lead
    assert index is None or tuple(index.shape) == lead + (K,)
    assert modes is None or tuple(modes.shape) == lead + (K, d)
    assert mass is None or tuple(mass.shape) == lead + (K,)
    assert mean is None or tuple(mean.shape) == lead + (K, d)
    a = MmfPfModesArgs()
    a.R, a.M, a.d, a.max_modes, a.link_radius = R, M, d, K, float(link_radius)
    a.states, a.log_a, a.log_b = vp(states), vp(log_a), vp(log_b)
    a.log_density, a.bandwidth = vp(log_density), vp(bandwidth)
    a.parent, a.labels, a.count = vp(parent, torch.int32), vp(labels, torch.int32), vp(count, torch.int32)
    a.index, a.modes, a.mass, a.mean = vp(index, torch.int32), vp(modes), vp(mass), vp(mean)
    with _on(states):
        work = _summary_workspace(a, pf_modes_workspace_bytes(R, M, d), states)
        _check(load().mmf_pf_modes(ctypes.byref(a), stream_of(states)), "mmf_pf_modes")


def pf_modalities(states, log_w, logliks, modality_logw, *, log_evidence=None, responsibility=None, ess=None, mean=None,
                  divergence=None, overlap=None):
    """Per-modality attribution of the crossmodal fusion (``mmf_pf_modalities``, include/mmf.h): ``states (..., M, d)`` -- ``R``
    rows, the product of the leading sizes -- with the incoming log-weights ``log_w (..., M)`` or ``None`` (uniform), ``logliks``,
    the ``K`` (1 .. 4) unimodal log-likelihoods ``(..., M)`` of the enabled modalities, and ``modality_logw (..., K)`` or
    ``None`` (0) -> ``log_evidence (..., K + 1)``, ``responsibility (..., K)``, ``ess (..., K + 1)``, ``mean (..., K + 1, d)``,
    ``divergence (..., K)``, ``overlap (..., K, K)``, each of which may be ``None`` (not all six); the entries ``K`` are the
    fused posterior's."""
    lead, R, M, d = _summary_rows(states, log_w, None)
    logliks = list(logliks)
    K = len(logliks)
    if not 1 <= K <= LOOP_MAX_MEAS:
        raise MmfError(f"mmf_pf_modalities takes 1 .. {LOOP_MAX_MEAS} modalities, got {K}")
    for l in logliks:
        assert tuple(l.shape) == lead + (M,)
    assert modality_logw is None or tuple(modality_logw.shape) == lead + (K,)
    assert log_evidence is None or tuple(log_evidence.shape) == lead + (K + 1,)
    assert responsibility is None or tuple(responsibility.shape) == lead + (K,)
    assert ess is None or tuple(ess.shape) == lead + (K + 1,)
    assert mean is None or tuple(mean.shape) == lead + (K + 1, d)
    assert divergence is None or tuple(divergence.shape) == lead + (K,)
    assert overlap is None or tuple(overlap.shape) == lead + (K, K)
    a = MmfPfModalitiesArgs()
    a.R, a.M, a.d, a.K, a.logw_stride = R, M, d, K, K
    a.states, a.log_w, a.modality_logw = vp(states), vp(log_w), vp(modality_logw)
    for k, l in enumerate(logliks):
        a.loglik[k] = ptr(l)
    a.log_evidence, a.responsibility, a.ess = vp(log_evidence), vp(responsibility), vp(ess)
    a.mean, a.divergence, a.overlap = vp(mean), vp(divergence), vp(overlap)
    with _on(states):
        _check(load().mmf_pf_modalities(ctypes.byref(a), stream_of(states)), "mmf_pf_modalities")


def pf_distance_workspace_bytes(R: int, Ma: int, Mb: int, d: int) -> int:
    return int(load().mmf_pf_distance_workspace_bytes(int(R), int(Ma), int(Mb), int(d)))


def pf_distance_lds_bytes(Ma: int, Mb: int) -> int:
    return int(load().mmf_pf_distance_lds_bytes(int(Ma), int(Mb)))


def pf_distance(states_a, log_a_a, log_b_a, states_b, log_a_b, log_b_b, *, wasserstein=None, cramer=None, ks=None, energy=None,
                terms=None, scale=None):
    """Two-sample distances between weighted particle sets (``mmf_pf_distance``, include/mmf.h): ``states_a (..., Ma, d)``
    against ``states_b (..., Mb, d)`` with the same leading sizes -- ``R`` row pairs, their product -- each under its own
    log-weights ``log_a + log_b``, ``(..., M)`` or ``None`` (0; both ``None``: uniform) -> per dimension ``wasserstein``,
    ``cramer``, ``ks (..., d)`` on K1's integer fixed-point weights, and in the Euclidean norm under ``scale`` ``energy (...)``
    and ``terms (..., 3)``, ``E|X - Y|, E|X - X'|, E|Y - Y'|``; each of the five may be ``None`` (not all).  ``scale``:
    ``None`` (ones) or ``d`` positive finite host floats.  The workspace of the partial sums is allocated here, on the
    tensors' device."""
    lead, R, Ma, d = _summary_rows(states_a, log_a_a, log_b_a)
    lead_b, _, Mb, d_b = _summary_rows(states_b, log_a_b, log_b_b)
    assert lead_b == lead and d_b == d and states_b.device == states_a.device
    scale = [1.0] * d if scale is None else [float(s) for s in scale]
    if len(scale) != d or d > MMF_MAX_STATE_DIM:
        raise MmfError(f"mmf_pf_distance takes one scale per state dimension (d = {d} <= {MMF_MAX_STATE_DIM}), got {len(scale)}")
    for out in (wasserstein, cramer, ks):
        assert out is None or tuple(out.shape) == lead + (d,)
    assert energy is None or tuple(energy.shape) == lead
    assert terms is None or tuple(terms.shape) == lead + (3,)
    a = MmfPfDistanceArgs()
    a.R, a.Ma, a.Mb, a.d = R, Ma, Mb, d
    for i, s in enumerate(scale):
        a.scale[i] = s
    a.states_a, a.log_a_a, a.log_b_a = vp(states_a), vp(log_a_a), vp(log_b_a)
    a.states_b, a.log_a_b, a.log_b_b = vp(states_b), vp(log_a_b), vp(log_b_b)
    a.wasserstein, a.cramer, a.ks, a.energy, a.terms = vp(wasserstein), vp(cramer), vp(ks), vp(energy), vp(terms)
    with _on(states_a):
        need = pf_distance_workspace_bytes(R, Ma, Mb, d) if energy is not None or terms is not None else 0
        work = _summary_workspace(a, need, states_a)
        _check(load().mmf_pf_distance(ctypes.byref(a), stream_of(states_a)), "mmf_pf_distance")
