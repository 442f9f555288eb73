"""ctypes binding of libvtd_hip.so (the C ABI in include/vtd.h).

Loading is strict: there is no CPU or eager-PyTorch fallback anywhere in this package.  ``require()``
raises when the library is missing (run ``python __graft_entry__.py`` / ``build_native.py``) or when
no HIP device is visible, so a mis-provisioned GPU box fails loudly instead of silently passing.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# VTD_LIB_VARIANT=<tag>: an instrumented build (build_native.py, tools/conv_experiment.sh) living beside the product library
_VARIANT = os.environ.get("VTD_LIB_VARIANT", "")
LIB_PATH = os.path.join(_HERE, "_lib", f"libvtd_hip_{_VARIANT}.so" if _VARIANT else "libvtd_hip.so")

_lib = None


class NativeError(RuntimeError):
    pass


class TrocrConfig(C.Structure):
    """vtd_trocr_config of include/vtd.h"""
    _fields_ = [("image_size", C.c_int32), ("patch_size", C.c_int32), ("enc_hidden", C.c_int32), ("enc_layers", C.c_int32),
                ("enc_heads", C.c_int32), ("enc_ffn", C.c_int32), ("enc_qkv_bias", C.c_int32), ("enc_ln_eps", C.c_float),
                ("dec_hidden", C.c_int32), ("dec_layers", C.c_int32), ("dec_heads", C.c_int32), ("dec_ffn", C.c_int32),
                ("vocab_size", C.c_int32), ("max_positions", C.c_int32), ("dec_ln_eps", C.c_float),
                ("decoder_start_token_id", C.c_int32), ("eos_token_id", C.c_int32), ("pad_token_id", C.c_int32), ("max_length", C.c_int32)]


class Detection(C.Structure):
    _fields_ = [("bbox", C.c_int32 * 4), ("polygon", C.c_int32 * 8), ("confidence", C.c_float), ("area", C.c_float),
                ("first_x", C.c_int32), ("first_y", C.c_int32)]


class DbHeadBranch(C.Structure):
    """vtd_dbhead_branch of include/vtd.h: device pointers to one DB-head branch's fp32 tensors, PyTorch layouts"""
    _fields_ = [(k, C.c_void_p) for k in ("conv_w", "conv_b", "bn1_w", "bn1_b", "bn1_mean", "bn1_var", "ct1_w", "ct1_b", "bn2_w", "bn2_b",
                                          "bn2_mean", "bn2_var", "ct2_w", "ct2_b")]


class DbHeadParams(C.Structure):
    _fields_ = [("branch", DbHeadBranch * 2)]


class FpnParams(C.Structure):
    """vtd_fpn_params of include/vtd.h: device pointers to the FPN's ten live fp32 tensors (inner_blocks.0..3, layer_blocks.3)"""
    _fields_ = [("inner_w", C.c_void_p * 4), ("inner_b", C.c_void_p * 4), ("layer_w", C.c_void_p), ("layer_b", C.c_void_p)]


BLOCK_FIELDS = ("conv1_w", "bn1_w", "bn1_b", "bn1_mean", "bn1_var", "conv2_w", "bn2_w", "bn2_b", "bn2_mean", "bn2_var",
                "ds_w", "ds_bn_w", "ds_bn_b", "ds_bn_mean", "ds_bn_var")


class BasicBlockParams(C.Structure):
    """vtd_basicblock_params of include/vtd.h: device pointers to one BasicBlock's fp32 tensors, PyTorch layouts"""
    _fields_ = [(k, C.c_void_p) for k in BLOCK_FIELDS]


BOTTLENECK_FIELDS = BLOCK_FIELDS[:10] + ("conv3_w", "bn3_w", "bn3_b", "bn3_mean", "bn3_var") + BLOCK_FIELDS[10:]


class BottleneckParams(C.Structure):
    """vtd_bottleneck_params of include/vtd.h: device pointers to one Bottleneck's fp32 tensors, PyTorch layouts"""
    _fields_ = [(k, C.c_void_p) for k in BOTTLENECK_FIELDS]


class StemParams(C.Structure):
    """vtd_stem_params of include/vtd.h: device pointers to the stem's fp32 tensors (conv weight, BatchNorm gamma, beta, running mean, var)"""
    _fields_ = [(k, C.c_void_p) for k in ("w", "gamma", "beta", "mean", "var")]


FpnTaps = C.c_void_p * 4   # padded taps C2, C3, C4, C5

ADAMW_SLICE = 64     # VTD_ADAMW_SLICE of include/vtd.h
ADAMW_CHUNK = 4096   # VTD_ADAMW_CHUNK


class AdamwTensor(C.Structure):
    """vtd_adamw_tensor of include/vtd.h (48 bytes): device pointers to one parameter's p, g, exp_avg, exp_avg_sq and its per-step scalars"""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64), ("step_size", C.c_float),
                ("bc2_sqrt", C.c_float)]


class AdamwHyper(C.Structure):
    """vtd_adamw_hyper of include/vtd.h"""
    _fields_ = [(k, C.c_float) for k in ("decay", "one_minus_beta1", "beta2", "one_minus_beta2", "eps")]


# name -> (restype, argtypes); kept in one table so tests can check it against include/vtd.h
SIGNATURES = {
    "vtd_version": (C.c_char_p, []),
    "vtd_strerror": (C.c_char_p, [C.c_int]),
    "vtd_device_count": (C.c_int, []),
    "vtd_detector_create": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "vtd_detector_destroy": (None, [C.c_void_p]),
    "vtd_detector_set_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "vtd_detector_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "vtd_detector_finalize": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vtd_detector_preprocess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vtd_detector_set_input_nchw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vtd_detector_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_detector_read_tap": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "vtd_detector_macs_per_frame": (C.c_int64, [C.c_void_p]),
    "vtd_detector_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "vtd_detector_num_ops": (C.c_int, [C.c_void_p]),
    "vtd_detector_get_profile": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                           C.POINTER(C.c_double), C.c_void_p]),
    "vtd_detector_set_tuning": (C.c_int, [C.c_void_p, C.c_char_p]),
    "vtd_detector_get_tuning": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_int64]),
    "vtd_detector_tuning_measured": (C.c_int, [C.c_void_p]),
    "vtd_postproc_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "vtd_postproc_destroy": (None, [C.c_void_p]),
    "vtd_copy_to_pinned_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "vtd_postproc_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "vtd_recognizer_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "vtd_recognizer_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "vtd_recognizer_destroy": (None, [C.c_void_p]),
    "vtd_recognizer_set_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "vtd_recognizer_finalize": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vtd_recognizer_crop_resize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "vtd_recognizer_set_input_nchw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vtd_recognizer_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "vtd_recognizer_read_tap": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "vtd_recognizer_macs_per_crop": (C.c_int64, [C.c_void_p]),
    "vtd_recognizer_set_tuning": (C.c_int, [C.c_void_p, C.c_char_p]),
    "vtd_recognizer_get_tuning": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_int64]),
    "vtd_recognizer_tuning_measured": (C.c_int, [C.c_void_p]),
    "vtd_trocr_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "vtd_trocr_destroy": (None, [C.c_void_p]),
    "vtd_trocr_set_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "vtd_trocr_finalize": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vtd_trocr_encode_crops": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "vtd_trocr_encode_pixels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vtd_trocr_generate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_trocr_num_slots": (C.c_int, [C.c_void_p]),
    "vtd_trocr_encode_crops_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "vtd_trocr_encode_pixels_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "vtd_trocr_stage_crops_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vtd_trocr_encode_staged_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vtd_trocr_generate_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_trocr_last_steps": (C.c_int, [C.c_void_p]),
    "vtd_dbloss_workspace_bytes": (C.c_int64, []),
    "vtd_dbloss_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "vtd_dbloss_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "vtd_detector_forward_features": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "vtd_dbhead_pack_features": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vtd_dbhead_train_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "vtd_dbhead_train_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(DbHeadParams), C.c_int, C.c_float, C.c_float,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_dbhead_train_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(DbHeadParams), C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DbHeadParams), C.c_void_p, C.c_void_p]),
    "vtd_dbhead_train_backward_input": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(DbHeadParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_dbhead_unpack_input_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vtd_detector_forward_trunk": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_fpn_train_pack_tap": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vtd_fpn_train_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "vtd_fpn_train_forward": (C.c_int, [C.POINTER(FpnTaps), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(FpnParams), C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "vtd_fpn_train_unpack_p2": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vtd_fpn_train_pack_grad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vtd_fpn_train_backward": (C.c_int, [C.POINTER(FpnTaps), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(FpnParams), C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.POINTER(FpnParams), C.c_void_p, C.c_void_p]),
    "vtd_basicblock_train_workspace_bytes": (C.c_int64, [C.c_int] * 7),
    "vtd_basicblock_train_forward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BasicBlockParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_basicblock_train_backward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BasicBlockParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.POINTER(BasicBlockParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_resblock_train_workspace_bytes": (C.c_int64, [C.c_int] * 7),
    "vtd_resblock_train_forward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BasicBlockParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_resblock_train_backward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BasicBlockParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.POINTER(BasicBlockParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_resblock_train_combine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "vtd_bottleneck_train_workspace_bytes": (C.c_int64, [C.c_int] * 7),
    "vtd_bottleneck_train_forward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BottleneckParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_bottleneck_train_backward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BottleneckParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.POINTER(BottleneckParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_bottleneck256_train_workspace_bytes": (C.c_int64, [C.c_int] * 7),
    "vtd_bottleneck256_train_forward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BottleneckParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_bottleneck256_train_backward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BottleneckParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.POINTER(BottleneckParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_bottleneck128_train_workspace_bytes": (C.c_int64, [C.c_int] * 7),
    "vtd_bottleneck128_train_forward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BottleneckParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_bottleneck128_train_backward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BottleneckParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.POINTER(BottleneckParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_bottleneck64_train_workspace_bytes": (C.c_int64, [C.c_int] * 7),
    "vtd_bottleneck64_train_forward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BottleneckParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_bottleneck64_train_backward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BottleneckParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.POINTER(BottleneckParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_block64_train_workspace_bytes": (C.c_int64, [C.c_int] * 7),
    "vtd_block64_train_forward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BasicBlockParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_block64_train_backward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BasicBlockParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.POINTER(BasicBlockParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_resblock_bn_train_workspace_bytes": (C.c_int64, [C.c_int] * 7),
    "vtd_resblock_bn_train_forward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BasicBlockParams), C.c_int, C.c_float, C.c_float, C.c_void_p,
                                                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_resblock_bn_train_backward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BasicBlockParams), C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                                                                C.c_void_p, C.c_void_p, C.POINTER(BasicBlockParams), C.c_void_p, C.c_void_p,
                                                                                C.c_void_p, C.c_void_p]),
    "vtd_block_bn_train_workspace_bytes": (C.c_int64, [C.c_int] * 7),
    "vtd_block_bn_train_forward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BasicBlockParams), C.c_int, C.c_float, C.c_float, C.c_void_p,
                                                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_block_bn_train_backward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BasicBlockParams), C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                                                             C.c_void_p, C.c_void_p, C.POINTER(BasicBlockParams), C.c_void_p, C.c_void_p,
                                                                             C.c_void_p, C.c_void_p]),
    "vtd_trunk_bn_train_workspace_bytes": (C.c_int64, [C.c_int] * 7),
    "vtd_trunk_bn_train_forward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BasicBlockParams), C.c_int, C.c_float, C.c_float, C.c_void_p,
                                                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_trunk_bn_train_backward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BasicBlockParams), C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                                                             C.c_void_p, C.c_void_p, C.POINTER(BasicBlockParams), C.c_void_p, C.c_void_p,
                                                                             C.c_void_p, C.c_void_p]),
    "vtd_bottleneck_bn_train_workspace_bytes": (C.c_int64, [C.c_int] * 7),
    "vtd_bottleneck_bn_train_forward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BottleneckParams), C.c_int, C.c_float, C.c_float, C.c_void_p,
                                                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_bottleneck_bn_train_backward": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(BottleneckParams), C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                                                                  C.c_void_p, C.c_void_p, C.POINTER(BottleneckParams), C.c_void_p, C.c_void_p,
                                                                                  C.c_void_p, C.c_void_p]),
    "vtd_stem_train_pack_input": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vtd_stem_train_workspace_bytes": (C.c_int64, [C.c_int] * 4),
    "vtd_stem_train_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(StemParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "vtd_stem_train_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(StemParams), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.POINTER(StemParams), C.c_void_p, C.c_void_p]),
    "vtd_stem_bn_train_workspace_bytes": (C.c_int64, [C.c_int] * 4),
    "vtd_stem_bn_train_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(StemParams), C.c_int, C.c_float, C.c_float, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vtd_stem_bn_train_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(StemParams), C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(StemParams), C.c_void_p, C.c_void_p]),
    "vtd_detector_forward_pool": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "vtd_detector_forward_c2": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "vtd_fpn_train_input_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "vtd_fpn_train_backward_input": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(FpnParams), C.c_void_p, C.c_int, C.POINTER(FpnTaps),
                                               C.c_void_p, C.c_void_p]),
    "vtd_fpn_train_unpack_tap_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vtd_binary_counts_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    "vtd_adamw_step": (C.c_int, [C.POINTER(AdamwTensor), C.c_int, C.POINTER(AdamwHyper), C.c_void_p]),
    "vtd_trocr_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "vtd_trocr_get_option": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    "vtd_trocr_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "vtd_trocr_get_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]),
    "vtd_trocr_get_gemm_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_void_p]),
    "vtd_trocr_read_tap": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "vtd_trocr_encoder_tokens": (C.c_int, [C.c_void_p]),
    "vtd_trocr_logits_stride": (C.c_int, [C.c_void_p]),
    "vtd_trocr_macs_per_crop": (C.c_int64, [C.c_void_p]),
    "vtd_trocr_set_tuning": (C.c_int, [C.c_void_p, C.c_char_p]),
    "vtd_trocr_get_tuning": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_int64]),
    "vtd_trocr_tuning_measured": (C.c_int, [C.c_void_p]),
    "vtd_ctc_greedy_decode": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
}


def load():
    """dlopen the library and bind every declared symbol (no device needed)."""
    global _lib
    if _lib is None:
        # torch first: it ships its own libamdhip64; loaded after ours the process ends up with two HIP runtimes and the
        # second one to initialise sees no device (observed with build() + smoke() in one process)
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise NativeError(f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950)")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def require():
    """The library plus a visible GPU, or an exception.  Product code paths call this, never load()."""
    lib = load()
    n = lib.vtd_device_count()
    if n <= 0:
        raise NativeError("libvtd_hip.so loaded but no HIP device is visible; this package has no CPU fallback")
    return lib


def check(code, what=""):
    if code != 0:
        msg = load().vtd_strerror(code)
        raise NativeError(f"{what or 'vtd call'} failed: {msg.decode() if msg else code} ({code})")
