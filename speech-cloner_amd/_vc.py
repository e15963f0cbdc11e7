"""ctypes binding of libvc_hip.so (C ABI declared in include/vc_hip.h).

This is the only place Python touches the native library.  There is NO CPU fallback: if the
library is missing or an entry point fails, an exception is raised (``VCError``).
"""
import contextlib
import ctypes as C
import os
import threading

# Caller requirement (documented in INTEGRATION.md, not enforced here -- this module never writes os.environ):
# independent work (window chunks in decoder.predict(n_streams=...), consecutive batches) is pipelined over HIP streams,
# and the HIP runtime folds streams onto GPU_MAX_HW_QUEUES hardware queues (default 4); two streams sharing a queue
# serialise.  A caller that keeps more than ~3 batches in flight exports GPU_MAX_HW_QUEUES=16 BEFORE the process makes
# its first GPU call (bench.py does); results do not depend on it.

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('VC_LIB_PATH', os.path.join(_HERE, 'libvc_hip.so'))   # override: kernel A/B experiments

VC_OK = 0
VC_ABI_VERSION = 7      # include/vc_hip.h: VC_ABI_VERSION -- lib() refuses a library that reports another one


class VCError(RuntimeError):
    pass


class FrontendCfg(C.Structure):
    """struct vc_frontend_cfg (include/vc_hip.h)."""
    _fields_ = [('sample_rate', C.c_int32), ('hop_length', C.c_int32), ('win_length', C.c_int32),
                ('n_fft', C.c_int32), ('n_mels', C.c_int32), ('n_mfcc', C.c_int32),
                ('pre_emphasis', C.c_float), ('mean_abs_amp_norm', C.c_float),
                ('mfcc_norm_factor', C.c_float), ('M_dB_norm_factor', C.c_float),
                ('P_dB_norm_factor', C.c_float),
                ('mfcc_normaleze_first_mfcc', C.c_int32), ('calc_mfcc_derivate', C.c_int32),
                ('clip_output', C.c_int32)]


class DenoiseCfg(C.Structure):
    """struct vc_denoise_cfg (include/vc_hip.h, "Noise suppression")."""
    _fields_ = [('rule', C.c_int32), ('n_init', C.c_int32), ('a_spp', C.c_float), ('a_noise', C.c_float), ('a_dd', C.c_float),
                ('xi_h1', C.c_float), ('xi_min', C.c_float), ('gain_min', C.c_float), ('gamma_max', C.c_float)]


class WpeCfg(C.Structure):
    """struct vc_wpe_cfg (include/vc_hip.h, "Dereverberation")."""
    _fields_ = [('taps', C.c_int32), ('delay', C.c_int32), ('iterations', C.c_int32), ('context', C.c_int32),
                ('floor_rel', C.c_float), ('load_rel', C.c_float)]


VC_F32, VC_BF16 = 0, 1
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3
GEMM_PLAIN, GEMM_HIGHWAY = 0, 1
GEMM_MAX_GROUPS = 32
GRU_FORM_NONE, GRU_FORM_RESIDENT, GRU_FORM_MFMA = 0, 1, 2       # include/vc_hip.h: VC_GRU_FORM_*


class GemmGroup(C.Structure):
    """struct vc_gemm_group (include/vc_hip.h)."""
    _fields_ = [('d_Bt', C.c_void_p), ('K', C.c_int32), ('taps', C.c_int32), ('pad_l', C.c_int32),
                ('c_off', C.c_int32)]


class GemmDesc(C.Structure):
    """struct vc_gemm_desc (include/vc_hip.h)."""
    _fields_ = [('dtype', C.c_int32), ('mode', C.c_int32), ('d_X', C.c_void_p),
                ('M', C.c_int32), ('T', C.c_int32), ('Cin', C.c_int32), ('ldx', C.c_int32),
                ('N', C.c_int32), ('n_groups', C.c_int32),
                ('groups', GemmGroup * GEMM_MAX_GROUPS),
                ('d_pro_scale', C.c_void_p), ('d_pro_shift', C.c_void_p),
                ('pro_relu', C.c_int32), ('pro_pool', C.c_int32),
                ('d_epi_scale', C.c_void_p), ('d_epi_shift', C.c_void_p), ('act', C.c_int32),
                ('d_R', C.c_void_p), ('ldr', C.c_int32), ('d_C', C.c_void_p), ('ldc', C.c_int32),
                ('out_f32', C.c_int32), ('drop_keep', C.c_float), ('drop_seed', C.c_ulonglong),
                ('sum_groups', C.c_int32), ('epi_pool', C.c_int32),
                ('d_workspace', C.c_void_p), ('workspace_bytes', C.c_size_t)]


CBHG_FRONT_MAX_HIGHWAY = 4


class CbhgFrontDesc(C.Structure):
    """struct vc_cbhg_front_desc (include/vc_hip.h)."""
    _fields_ = [('d_x', C.c_void_p), ('x_f32', C.c_int32), ('ldx', C.c_int32), ('n_windows', C.c_int32), ('T', C.c_int32),
                ('n_features', C.c_int32), ('prenet_units', C.c_int32), ('width', C.c_int32), ('n_banks', C.c_int32),
                ('bank_filters', C.c_int32), ('n_highway', C.c_int32), ('gru_units', C.c_int32),
                ('d_pk_dense1', C.c_void_p), ('d_pk_dense2', C.c_void_p), ('d_pk_bank', C.c_void_p),
                ('d_pk_proj1', C.c_void_p), ('d_pk_proj2', C.c_void_p), ('d_pk_gru', C.c_void_p),
                ('d_pk_highway', C.c_void_p * CBHG_FRONT_MAX_HIGHWAY),
                ('d_coef', C.c_void_p),
                ('d_xproj', C.c_void_p), ('ldp', C.c_int32)]


class LayoutItem(C.Structure):
    """struct vc_layout_item (include/vc_hip.h)."""
    _fields_ = [('src', C.c_void_p), ('dst', C.c_void_p), ('k', C.c_int32), ('cin', C.c_int32), ('cout', C.c_int32),
                ('mode', C.c_int32)]


class W16Item(C.Structure):
    """struct vc_w16_item (include/vc_hip.h)."""
    _fields_ = [('src', C.c_void_p), ('dst', C.c_void_p), ('scale_dst', C.c_void_p), ('k', C.c_int32), ('cin', C.c_int32),
                ('cout', C.c_int32), ('mode', C.c_int32), ('row_len', C.c_int32), ('tap_stride', C.c_int32),
                ('plane_stride', C.c_int32), ('base', C.c_int32), ('group', C.c_int32), ('scale_n', C.c_int32)]


class Gemm16Pair(C.Structure):
    """struct vc_gemm16_pair (include/vc_hip.h)."""
    _fields_ = [('d_Bt0', C.c_void_p), ('d_Bt1', C.c_void_p), ('taps0', C.c_int32), ('extra', C.c_int32),
                ('pad_l', C.c_int32), ('c_off0', C.c_int32), ('c_off1', C.c_int32), ('row0', C.c_int32),
                ('nrows0', C.c_int32), ('nrows1', C.c_int32), ('s_off0', C.c_int32), ('s_off1', C.c_int32)]


class Gemm16Desc(C.Structure):
    """struct vc_gemm16_desc (include/vc_hip.h)."""
    _fields_ = [('d_X16', C.c_void_p), ('d_row_scale', C.c_void_p), ('M', C.c_int32), ('T', C.c_int32), ('C', C.c_int32),
                ('ldx', C.c_int32), ('n_pairs', C.c_int32), ('ragged', C.c_int32), ('pairs', Gemm16Pair * 16),
                ('d_col_scale', C.c_void_p), ('d_col_shift', C.c_void_p), ('d_C', C.c_void_p), ('ldc', C.c_int32),
                ('accumulate', C.c_int32), ('act', C.c_int32), ('atomic_splits', C.c_int32), ('d_workspace', C.c_void_p),
                ('workspace_bytes', C.c_size_t)]


MX8_MAX_GROUPS = 32
MX8_OUT_MX, MX8_OUT_BF16, MX8_OUT_F32 = 0, 1, 2


class Mx8Group(C.Structure):
    """struct vc_mx8_group (include/vc_hip.h)."""
    _fields_ = [('d_W', C.c_void_p), ('d_Ws', C.c_void_p), ('taps', C.c_int32), ('pad_l', C.c_int32),
                ('c_off', C.c_int32), ('reserved', C.c_int32)]


class Mx8ConvDesc(C.Structure):
    """struct vc_mx8_conv_desc (include/vc_hip.h)."""
    _fields_ = [('d_X', C.c_void_p), ('d_Xs', C.c_void_p), ('M', C.c_int32), ('T', C.c_int32), ('Cin', C.c_int32),
                ('n_groups', C.c_int32), ('groups', Mx8Group * MX8_MAX_GROUPS), ('d_epi_scale', C.c_void_p),
                ('d_epi_shift', C.c_void_p), ('act', C.c_int32), ('pool', C.c_int32), ('out_mode', C.c_int32),
                ('n_out', C.c_int32), ('d_C', C.c_void_p), ('d_Cs', C.c_void_p), ('d_workspace', C.c_void_p),
                ('workspace_bytes', C.c_size_t)]


class WgradGroup(C.Structure):
    """struct vc_wgrad_group (include/vc_hip.h)."""
    _fields_ = [('d_dYT', C.c_void_p), ('d_dW', C.c_void_p), ('N', C.c_int32), ('taps', C.c_int32),
                ('shift0', C.c_int32), ('ldw', C.c_int32)]


class WgradDesc(C.Structure):
    """struct vc_wgrad_desc (include/vc_hip.h)."""
    _fields_ = [('d_XT', C.c_void_p), ('ldxt', C.c_int32), ('ldyt', C.c_int32), ('Cin', C.c_int32),
                ('M', C.c_int32), ('T', C.c_int32), ('margin', C.c_int32), ('n_groups', C.c_int32),
                ('splits_allowed', C.c_int32), ('groups', WgradGroup * GEMM_MAX_GROUPS)]


_lib = None
_lock = threading.Lock()

_P = C.c_void_p
_SIGS = {
    'vc_version': (C.c_int, []),
    'vc_last_error': (C.c_char_p, []),
    'vc_target_arch': (C.c_char_p, []),
    'vc_set_option': (C.c_int, [C.c_char_p, C.c_int]),
    'vc_get_option': (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    'vc_frontend_host_tables': (C.c_int, [C.POINTER(FrontendCfg), _P, _P]),
    'vc_frontend_plan_create': (C.c_int, [C.POINTER(FrontendCfg), _P, C.POINTER(_P)]),
    'vc_frontend_plan_destroy': (None, [_P]),
    'vc_frontend_num_frames': (C.c_int32, [_P, C.c_int32]),
    'vc_frontend_mfcc_width': (C.c_int32, [_P]),
    'vc_frontend_power_width': (C.c_int32, [_P]),
    'vc_frontend_get_mel': (C.c_int, [_P, _P]),
    'vc_frontend_get_dct': (C.c_int, [_P, _P]),
    'vc_frontend_workspace_bytes': (C.c_size_t, [_P, C.c_int32, C.c_int32]),
    'vc_frontend_f32': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P,
                                  C.c_size_t, _P]),
    'vc_frontend_stages_f32': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P,
                                         C.c_size_t, _P, C.c_int32]),
    'vc_conv_gemm_workspace_bytes': (C.c_size_t, [C.POINTER(GemmDesc)]),
    'vc_conv_gemm': (C.c_int, [C.POINTER(GemmDesc), _P]),
    'vc_softmax_argmax': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P]),
    'vc_softmax_argmax_dual': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P]),
    'vc_gru_workspace_bytes': (C.c_size_t, [C.c_int32, C.c_int32]),
    'vc_gru_bidir': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P,
                               C.c_size_t, _P]),
    'vc_gru_form': (C.c_int32, [C.c_int32] * 4),
    'vc_gru_packed_bytes': (C.c_size_t, [C.c_int32] * 3),
    'vc_gru_pack': (C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, C.c_size_t, _P]),
    'vc_gru_bidir_packed': (C.c_int, [C.c_int32, _P, _P, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    'vc_lstm_bidir': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    'vc_convert': (C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_size_t, _P]),
    'vc_conv_wgrad': (C.c_int, [C.POINTER(WgradDesc), _P]),
    'vc_transpose_pad': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32,
                                   C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    'vc_stats_workspace_floats': (C.c_size_t, [C.c_int32, C.c_int32]),
    'vc_bn_train_stats': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_float, C.c_float,
                                    _P, _P, _P, _P, _P, _P]),
    'vc_affine_act': (C.c_int, [_P, _P, _P, C.c_int32, _P, _P, C.c_size_t, C.c_int32, _P]),
    'vc_bn_backward': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P,
                                 C.c_int32, _P, _P, _P, _P, _P]),
    'vc_lstm_train_forward': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    'vc_lstm_backward': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'vc_bn_post_routing': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    'vc_relu_dropout_backward': (C.c_int, [_P, _P, C.c_float, _P, C.c_size_t, _P]),
    'vc_highway_backward': (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    'vc_col_sum': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P]),
    'vc_fill': (C.c_int, [_P, C.c_float, C.c_size_t, _P]),
    'vc_weight_layouts': (C.c_int, [_P, C.c_int32, _P]),
    'vc_split16': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    'vc_weights16': (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P]),
    'vc_transpose_split16': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, _P, _P, _P]),
    'vc_gemm16_workspace_bytes': (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    'vc_gemm16': (C.c_int, [C.POINTER(Gemm16Desc), _P]),
    'vc_mx8_quantize': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    'vc_mx8_conv_workspace_bytes': (C.c_size_t, [C.POINTER(Mx8ConvDesc)]),
    'vc_mx8_conv': (C.c_int, [C.POINTER(Mx8ConvDesc), _P]),
    'vc_axpby': (C.c_int, [_P, C.c_int32, C.c_float, _P, C.c_int32, C.c_float, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    'vc_mse_loss': (C.c_int, [_P, _P, C.c_size_t, C.c_float, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    'vc_softmax_ce': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    'vc_adam_step': (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_float, C.c_float, C.c_float, C.c_float,
                               C.c_float, _P]),
    'vc_gru_train_forward': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    'vc_gru_backward': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'vc_conv_gemm_epi_pool_supported': (C.c_int, [C.POINTER(GemmDesc)]),
    'vc_highway_pack': (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P]),
    'vc_highway_chain': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P), C.POINTER(_P), _P, C.c_int32,
                                   _P, _P, C.c_int32, _P, C.c_int32, _P]),
    'vc_mfma_pack': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'vc_prenet_chain_supported': (C.c_int, [C.c_int32] * 3),
    'vc_prenet_chain': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, _P]),
    'vc_cbhg_front_coef_floats': (C.c_int32, []),
    'vc_cbhg_front_supported': (C.c_int, [C.c_int32] * 8),
    'vc_cbhg_front': (C.c_int, [C.POINTER(CbhgFrontDesc), _P]),
    'vc_gather_rows': (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, _P, _P]),
    'vc_vocoder_plan_create': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(_P)]),
    'vc_vocoder_plan_destroy': (None, [_P]),
    'vc_vocoder_num_samples': (C.c_int32, [_P, C.c_int32]),
    'vc_vocoder_workspace_bytes': (C.c_size_t, [_P, C.c_int32, C.c_int32, C.c_int32]),
    'vc_power_to_amp': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P]),
    'vc_griffin_lim_f32': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P,
                                     C.c_size_t, _P]),
    'vc_vocoder_workspace_bytes_momentum': (C.c_size_t, [_P, C.c_int32, C.c_int32, C.c_int32]),
    'vc_griffin_lim_momentum_f32': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, _P, C.c_int32,
                                              _P, _P, C.c_size_t, _P]),
    'vc_inv_preemphasis_normalize': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _P]),
    'vc_cut_windows': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'vc_compound_stitch': (C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P,
                                     C.c_float, _P]),
    'vc_phase_init': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _P, _P]),
    'vc_phase_spsi_workspace_bytes': (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    'vc_phase_spsi': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_size_t, _P]),
    'vc_resample_plan_create': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(_P)]),
    'vc_resample_plan_destroy': (None, [_P]),
    'vc_resample_f32': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P]),
    'vc_mel_cepstra': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P]),
    'vc_dtw_workspace_size': (C.c_size_t, [C.c_int32] * 4),
    'vc_dtw_f32': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, _P, _P, _P,
                             _P, C.c_size_t, _P]),
    'vc_dtw_backtrack': (C.c_int, [_P, C.c_size_t, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'vc_frame_mcd_f32': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, _P, _P]),
    # speech activity (csrc/vc_activity.hip); the pitch rows stay the table's last two (tests/test_f0_cpu.py)
    'vc_frame_energy_tile': (C.c_int, [C.c_int32, C.c_int32]),
    'vc_frame_energy_f32': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    'vc_activity_mask': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, _P, _P]),
    'vc_mask_compact': (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    'vc_compact_rows_f32': (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    'vc_path_map': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P]),
    'vc_speech_gain_f32': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_float, _P, _P]),
    'vc_scale_rows_f32': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    # content preservation (csrc/vc_content.hip)
    'vc_ppg_metrics_f32': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P]),
    'vc_phn_segments_tile': (C.c_int, []),
    'vc_phn_segments': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    'vc_edit_distance_rows': (C.c_int, []),
    'vc_edit_distance_workspace_bytes': (C.c_size_t, [C.c_int32] * 3),
    'vc_edit_distance_i32': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_size_t, _P]),
    # speaker similarity (csrc/vc_gmm.hip)
    'vc_gmm_tile_frames': (C.c_int, []),
    'vc_gmm_partitions': (C.c_int, [C.c_int32]),
    'vc_gmm_table_floats': (C.c_size_t, [C.c_int32] * 3),
    'vc_gmm_workspace_bytes': (C.c_size_t, [C.c_int32] * 3),
    'vc_spk_features_f32': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'vc_gmm_prepare_f32': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'vc_gmm_loglik_f32': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    'vc_gmm_score_f32': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    'vc_gmm_accumulate_f32': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    'vc_gmm_update_f32': (C.c_int, [C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_float, C.c_float, _P, _P,
                                    _P, _P]),
    # pitch tracking (csrc/vc_f0.hip, csrc/vc_f0_track.hip); the two older pitch rows still close the table
    'vc_f0_candidates_f32': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_float, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, _P]),
    'vc_f0_viterbi_tile': (C.c_int32, []),
    'vc_f0_viterbi_workspace_size': (C.c_size_t, [C.c_int32] * 3),
    'vc_f0_viterbi_f32': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, _P, _P, _P, _P,
                                    _P, C.c_size_t, _P]),
    # forced alignment (csrc/vc_align.hip); the two older pitch rows still close the table
    'vc_align_workspace_bytes': (C.c_size_t, [C.c_int32] * 3),
    'vc_align_f32': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, C.c_size_t,
                               _P]),
    # full-sum alignment (csrc/vc_fullsum.hip)
    'vc_fullsum_workspace_bytes': (C.c_size_t, [C.c_int32] * 3),
    'vc_fullsum_f32': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    # phone-loop decoding (csrc/vc_decode.hip)
    'vc_decode_workspace_bytes': (C.c_size_t, [C.c_int32] * 3),
    'vc_decode_f32': (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P,
                                C.c_size_t, _P]),
    # duration conversion (csrc/vc_warp.hip)
    'vc_duration_map_workspace_bytes': (C.c_size_t, [C.c_int32] * 2),
    'vc_duration_map': (C.c_int, [_P] * 6 + [C.c_int32, C.c_int32, _P] + [C.c_int32] * 5 + [_P] * 6 + [C.c_size_t, _P]),
    'vc_time_warp': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_float, _P]),
    # pitch conversion (csrc/vc_pitch.hip)
    'vc_psola_max_marks': (C.c_int32, [C.c_int32]),
    'vc_psola_plan': (C.c_int, [_P, _P, _P] + [C.c_int32] * 4 + [_P] * 7),
    'vc_psola_ola_f32': (C.c_int, [_P] * 7 + [C.c_int32, C.c_int32, C.c_float, _P, _P]),
    # waveform time scaling (csrc/vc_wsola.hip)
    'vc_wsola_max_grains': (C.c_int32, [C.c_int32] * 3),
    'vc_wsola_plan': (C.c_int, [_P, C.c_int32, _P, _P, _P] + [C.c_int32] * 6 + [C.c_float] + [_P] * 5),
    'vc_wsola_ola_f32': (C.c_int, [_P, C.c_int32] + [_P] * 5 + [C.c_int32] * 5 + [_P, _P]),
    # differential-spectrum conversion (csrc/vc_vocoder.hip)
    'vc_spectral_diff_gain_f32': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float,
                                            _P, C.c_int32, _P, _P]),
    'vc_stft_filter_workspace_bytes': (C.c_size_t, [_P, C.c_int32, C.c_int32]),
    'vc_stft_filter_f32': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_size_t, _P]),
    # postfilters (csrc/vc_postfilter.hip)
    'vc_traj_stats_f32': (C.c_int, [_P, _P] + [C.c_int32] * 3 + [_P, _P]),
    'vc_gv_filter_f32': (C.c_int, [_P] * 4 + [C.c_int32] * 3 + [C.c_float] * 2 + [_P, _P]),
    'vc_ms_stats_f32': (C.c_int, [_P] * 3 + [C.c_int32] * 3 + [_P, _P]),
    'vc_ms_filter_f32': (C.c_int, [_P] * 4 + [C.c_int32] * 3 + [C.c_float] * 2 + [_P, _P]),
    # harmonic-plus-noise vocoder (csrc/vc_hnm.hip)
    'vc_hnm_max_harmonics': (C.c_int32, []),
    'vc_hnm_tile_intervals': (C.c_int32, []),
    'vc_env_cepstral_f32': (C.c_int, [_P, _P, _P] + [C.c_int32] * 5 + [C.c_float, _P, _P, _P]),
    'vc_hnm_plan': (C.c_int, [_P, _P] + [C.c_int32] * 4 + [C.c_float] * 2 + [_P] * 6),
    'vc_noise_init_f32': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int64, _P, _P]),
    'vc_hnm_noise_gain_f32': (C.c_int, [_P, _P, _P] + [C.c_int32] * 4 + [C.c_float, _P, _P]),
    'vc_hnm_synth_f32': (C.c_int, [_P] * 8 + [C.c_int32] * 4 + [C.c_int64, C.c_float, _P, _P]),
    # noise suppression (csrc/vc_vocoder.hip, csrc/vc_denoise.hip)
    'vc_stft_power_f32': (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    'vc_noise_gain_f32': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    # intelligibility (csrc/vc_stoi.hip)
    'vc_stoi_energy_f32': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P]),
    'vc_stoi_keep_f32': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, _P, _P, _P]),
    'vc_stoi_bands_f32': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P]),
    'vc_stoi_score_f32': (C.c_int, [_P, _P] + [C.c_int32] * 5 + [_P, C.c_int32, _P, _P, _P]),
    'vc_si_sdr_f32': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    # spectral mapping (csrc/vc_mapping.hip)
    'vc_jd_tile': (C.c_int, []),
    'vc_jd_table_floats': (C.c_size_t, [C.c_int32] * 2),
    'vc_jd_workspace_size': (C.c_size_t, [C.c_int32] * 2),
    'vc_mlpg_workspace_size': (C.c_size_t, [C.c_int32] * 3),
    'vc_jd_prepare_f32': (C.c_int, [_P] * 6 + [C.c_int32, C.c_int32, _P, _P]),
    'vc_jd_accumulate_f32': (C.c_int, [_P] * 6 + [C.c_int32] * 5 + [_P, C.c_int32, _P, _P, _P, _P, C.c_size_t, _P]),
    'vc_jd_update_f32': (C.c_int, [_P, _P, C.c_int32, C.c_int32] + [_P] * 7 + [C.c_float, C.c_float] + [_P] * 7),
    'vc_jd_map_f32': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    'vc_mlpg_f32': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_size_t, _P]),
    'vc_cep_gain_f32': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, C.c_int32] + [C.c_float] * 4
                        + [_P, _P]),
    # dereverberation (csrc/vc_vocoder.hip, csrc/vc_dereverb.hip)
    'vc_stft_complex_f32': (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    'vc_istft_complex_f32': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_size_t, _P]),
    'vc_wpe_max_frames': (C.c_int32, [C.c_int32]),
    'vc_wpe_f32': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    # exemplar conversion (csrc/vc_knn.hip)
    'vc_knn_key_width': (C.c_int32, [C.c_int32]),
    'vc_ppg_key_i8': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    'vc_knn_splits': (C.c_int32, [C.c_int32] * 3),
    'vc_knn_workspace_bytes': (C.c_size_t, [C.c_int32] * 4),
    'vc_knn_i8': (C.c_int, [_P] * 5 + [C.c_int32, C.c_int32, _P, _P] + [C.c_int32] * 4 + [_P, C.c_size_t, _P, _P, _P]),
    'vc_knn_mean_f32': (C.c_int, [_P, _P] + [C.c_int32] * 3 + [_P, C.c_int32, C.c_int32, _P, _P, _P]),
    'vc_f0_yin_f32': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                C.c_float, _P, _P, C.c_int32, _P]),
    'vc_f0_metrics_f32': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P]),
}


def lib():
    """Load (once) and return the ctypes handle of libvc_hip.so; raises VCError if absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise VCError('native library %s not found -- run `python -c "import __graft_entry__ as g; '
                          'g.build()"` (or make -C speech-cloner_amd/csrc); there is no CPU fallback'
                          % LIB_PATH)
        # torch ships its own libamdhip64; it must be the HIP runtime of the process.  Loading this
        # library first would pull in the system copy and leave two runtimes ("no ROCm-capable
        # device" from the second one), so torch is imported before the dlopen.
        import torch  # noqa: F401
        h = C.CDLL(LIB_PATH)
        h.vc_version.restype, h.vc_version.argtypes = C.c_int, []
        got = h.vc_version()
        if got != VC_ABI_VERSION:
            # a stale build (or a VC_LIB_PATH override built from older sources) would take shifted pointer / size
            # arguments: refuse it here instead of faulting on the device
            raise VCError('native library %s reports ABI version %d, this binding is written for %d -- rebuild it '
                          '(make -C speech-cloner_amd/csrc)' % (LIB_PATH, got, VC_ABI_VERSION))
        for name, (res, args) in _SIGS.items():
            try:
                fn = getattr(h, name)
            except AttributeError:
                # exports added without a version bump (vc_resample_*, then vc_mel_cepstra / vc_dtw_* / vc_frame_mcd_f32, then
                # vc_f0_*, then the speech-activity launches, then the content launches, then vc_spk_* / vc_gmm_*, then the pitch-tracking launches, then vc_align_*, then vc_fullsum_*, then vc_decode_*, then vc_duration_map / vc_time_warp, then vc_psola_*, then vc_spectral_diff_gain_f32 / vc_stft_filter_*, then vc_wsola_*, then the postfilter launches, then the vc_hnm_* launches, then vc_stft_power_f32 / vc_noise_gain_f32, then the vc_stoi_* launches and vc_si_sdr_f32, then the spectral-mapping launches (vc_jd_*, vc_mlpg_f32, vc_cep_gain_f32), then the exemplar launches (vc_ppg_key_i8, vc_knn_*), then the
                # packed-weights recurrence calls vc_gru_form / vc_gru_pack / vc_gru_bidir_packed): a build older than this binding
                # lacks them
                raise VCError('native library %s does not export %s -- it was built from older sources, rebuild it '
                              '(make -C speech-cloner_amd/csrc)' % (LIB_PATH, name)) from None
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def set_option(name, value):
    """vc_set_option (include/vc_hip.h): pick between equivalent HIP kernels; -1 restores the default."""
    check(lib().vc_set_option(name.encode(), int(value)))


def get_option(name):
    v = C.c_int(0)
    check(lib().vc_get_option(name.encode(), C.byref(v)))
    return v.value


@contextlib.contextmanager
def options(**kw):
    """with _vc.options(gru_mfma=1): ...  -- sets, then restores, library options."""
    old = {k: get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            set_option(k, v)


# Three kernels fill an otherwise idle chip at the price of extra workgroup time: the k = 3 projection's K split over two
# workgroups per row tile (-43 % for that launch alone, +0.8 % per step when ten batches are in flight), the
# front-end's one-launch form, whose blocks WAIT for their utterance (-14 % alone, +5.5 % per pipelined step: a waiting
# block keeps its CU from the register-filling MFMA launches of the other streams), and the register-resident
# recurrence, which takes one CU per sequence and direction for all 400 steps where the MFMA form packs sixteen sequences
# on one (the MFMA form is worth +7.7 % frames/s with ten batches of 64 windows in flight).  The library's defaults
# serve a caller with one batch at a time (the reference's test.py); a caller that keeps several batches in flight on
# several streams runs its loop under this context (bench.py's throughput loop does).
THROUGHPUT_OPTIONS = {'proj256_split': 0, 'fe_fused': 0}
# ... and the kernel form such a caller pins where the default would choose by the makespan of one call
# (tests/test_abi.py holds THROUGHPUT_OPTIONS to the two switched-off kernels above, so the forced form has its own table).
THROUGHPUT_FORMS = {'gru_mfma': 1}


def throughput_mode():
    """with _vc.throughput_mode(): ...  -- the option set for callers that keep several batches in flight."""
    return options(**THROUGHPUT_OPTIONS, **THROUGHPUT_FORMS)


def check(rc):
    if rc != VC_OK:
        msg = lib().vc_last_error()
        raise VCError('libvc_hip error %d: %s' % (rc, msg.decode('utf-8', 'replace') if msg else '?'))


def ptr(t):
    """Device/host pointer of a torch tensor or numpy array (None -> NULL)."""
    if t is None:
        return None
    if hasattr(t, 'data_ptr'):
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(t.ctypes.data)


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
