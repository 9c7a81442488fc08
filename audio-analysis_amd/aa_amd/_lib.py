"""ctypes binding of libaa.so (include/aa.h).

torch is imported first on purpose: the library's DT_NEEDED libamdhip64.so.7
then resolves to the HIP runtime torch already loaded, so device pointers from
torch tensors and the library's launches live in one runtime.  There is no
fallback: if the shared object is missing or does not load, every compute call
raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import torch  # noqa: F401  (must precede loading libaa.so, see above)

# AA_LIB: an alternative build of the same library (tools/ab_build.py variants)
LIB_PATH = Path(os.environ.get("AA_LIB") or Path(__file__).resolve().parent / "libaa.so")
ABI_VERSION = 5

AA_PREC_F32 = 0
AA_PREC_BF16 = 1
AA_PREC_FP8 = 2
AA_PREC_BF16X3 = 3

AA_OP = {
    "conv2d": 1,
    "batchnorm": 2,
    "leakyrelu": 3,
    "maxpool2d": 4,
    "globalmaxpool2d": 5,
    "sigmoid": 6,
    "magtransform": 7,
    "relu": 8,
    "dense": 9,
}

# aa_status (include/aa.h)
AA_OK = 0
AA_ERR_INVALID = 1
AA_ERR_HIP = 2
AA_ERR_UNSUPPORTED = 3
AA_ERR_WORKSPACE = 4

AA_WIN_OK = 0
AA_WIN_NONFINITE = 1

AA_SN_NONFINITE = 1
AA_SN_RUN_OVERFLOW = 2


class AAError(RuntimeError):
    pass


class Window(C.Structure):
    _fields_ = [("src", C.c_int64), ("n_valid", C.c_int32), ("pad_left", C.c_int32)]


class FeConfig(C.Structure):
    _fields_ = [
        ("win_len", C.c_int32), ("n_fft", C.c_int32), ("hop", C.c_int32), ("n_mels", C.c_int32),
        ("normalize", C.c_int32), ("db_scale", C.c_int32), ("power", C.c_float),
        ("amin", C.c_float), ("top_db", C.c_float), ("mean_sub", C.c_int32),
        ("channels", C.c_int32), ("out_f16", C.c_int32),
    ]


# aa_fe_kernel (include/aa.h): the stft launch a front-end plan chose
AA_FE_K = {"fe_stft_mel_small": 0, "fe_stft_mel_4096": 1, "fe_stft_mel": 2, "fe_stft_mel_mixed": 3}


class FeInfo(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("T", C.c_int32), ("kmin", C.c_int32), ("kmax", C.c_int32),
                ("nnz", C.c_int32), ("nparts", C.c_int32), ("lds_bytes", C.c_int64), ("grid", C.c_int32)]


class Layer(C.Structure):
    _fields_ = [
        ("op", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32), ("filters", C.c_int32),
        ("alpha", C.c_float), ("eps", C.c_float), ("off", C.c_int64 * 4),
    ]


class Node(C.Structure):
    _fields_ = [
        ("op", C.c_int32), ("in0", C.c_int32), ("in1", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32),
        ("sh", C.c_int32), ("sw", C.c_int32), ("pt", C.c_int32), ("pb", C.c_int32), ("pl", C.c_int32),
        ("pr", C.c_int32), ("filters", C.c_int32), ("act", C.c_int32), ("alpha", C.c_float),
        ("off", C.c_int64 * 2),
    ]


AA_G = {"conv": 1, "dwconv": 2, "maxpool": 3, "avgpool": 4, "gmaxpool": 5, "gavgpool": 6, "add": 7, "mul": 8,
        "affine": 9, "dense": 10, "pow": 11}
AA_GACT = {None: 0, "linear": 0, "relu": 1, "leaky": 2, "sigmoid": 3, "swish": 4}

# aa_gkernel (include/aa.h): the launch a graph node was planned for
AA_GK = {"x3p": 1, "x3t_256x16": 2, "x3t_128x32": 3, "x3t_64x128": 4, "x3t_split_kc2": 5, "x3t_split_kc1": 6,
         "x3t_64x64_kc2": 7, "x3t_64x64_pd2": 8, "x3t_64x64": 9, "matvec": 10, "matvec_t": 11, "f32_s": 12,
         "f32_lds_3x3x3": 13, "f32_lds_3x3x1": 14, "f32_lds": 15, "f32": 16, "dwpool4_s1": 17, "dwpool4_s2": 18,
         "dwpool4_k3": 19, "dwpool4": 20, "dwpool": 21, "dw4": 22, "dw1": 23, "pool2d": 24, "gpool4": 25,
         "gpool": 26, "binary": 27, "affine": 28, "pow": 29, "dense": 30}


class NodePlan(C.Structure):
    _fields_ = [
        ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("kernel", C.c_int32), ("bn", C.c_int32),
        ("cout_pad", C.c_int32), ("cin_pad", C.c_int32), ("split", C.c_int32), ("cslice", C.c_int32),
        ("skip", C.c_int32), ("nolaunch", C.c_int32), ("scale_src", C.c_int32), ("res_src", C.c_int32),
        ("pool_into", C.c_int32), ("in0", C.c_int32), ("in1", C.c_int32), ("act", C.c_int32),
        ("alpha", C.c_float), ("last_use", C.c_int32), ("off", C.c_int64),
    ]


class GraphLayout(C.Structure):
    _fields_ = [("per_win", C.c_int64), ("part_off", C.c_int64), ("n_outputs", C.c_int32),
                ("sigmoid_out", C.c_int32)]


class SnConfig(C.Structure):
    _fields_ = [("sr", C.c_int32), ("n_fft", C.c_int32), ("hop_length", C.c_int32),
                ("signal_width", C.c_double), ("freq_range", C.c_double)]


class SnComponent(C.Structure):
    _fields_ = [("left", C.c_int32), ("top", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("area", C.c_int32), ("order", C.c_int32)]


class RsSegment(C.Structure):
    """aa_rs_segment: one recording of an aa_resample_batch launch."""
    _fields_ = [("src_off", C.c_int64), ("n_in", C.c_int64), ("dst_off", C.c_int64), ("n_out", C.c_int64),
                ("kind", C.c_int32), ("channels", C.c_int32)]


AA_RS_S16 = 0
AA_RS_F32 = 1


class FlacInfo(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("channels", C.c_int32), ("bits_per_sample", C.c_int32),
                ("total_frames", C.c_int64)]


class FlacFrame(C.Structure):
    _fields_ = [("offset", C.c_int64), ("out_at", C.c_int64), ("nbytes", C.c_int32), ("block", C.c_int32),
                ("keep", C.c_int32), ("channels", C.c_int32), ("bits", C.c_int32), ("stream", C.c_int32)]


# aa_flac_status (include/aa.h)
AA_FLAC_OK = 0
AA_FLAC_CRC = 1
AA_FLAC_MALFORMED = 2
AA_FLAC_FALLBACK = 3
AA_FLAC_WG = 64


class VorbisInfo(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("channels", C.c_int32), ("blocksize_0", C.c_int32),
                ("blocksize_1", C.c_int32), ("total_frames", C.c_int64)]


class VorbisPacket(C.Structure):
    _fields_ = [("offset", C.c_int64), ("pos", C.c_int64), ("blk_at", C.c_int64), ("nbytes", C.c_int32),
                ("n", C.c_int32), ("blockflag", C.c_int32), ("prev", C.c_int32), ("next", C.c_int32),
                ("lstart", C.c_int32), ("rend", C.c_int32), ("stream", C.c_int32)]


class VorbisStream(C.Structure):
    _fields_ = [("setup_at", C.c_int64), ("out_at", C.c_int64), ("frames", C.c_int64), ("s0", C.c_int64),
                ("first_packet", C.c_int64), ("n_packets", C.c_int64), ("channels", C.c_int32),
                ("sample_rate", C.c_int32), ("blocksize_0", C.c_int32), ("blocksize_1", C.c_int32),
                ("ws_need", C.c_int32 * 2)]


class VorbisPlan(C.Structure):
    _fields_ = [("stride", C.c_int64), ("blk_floats", C.c_int64), ("max_out", C.c_int64),
                ("max_channels", C.c_int32), ("reserved", C.c_int32)]


# aa_vorbis_status (include/aa.h)
AA_VORBIS_OK = 0
AA_VORBIS_FALLBACK = 1
AA_VORBIS_WG = 64


class Mp3Info(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("channels", C.c_int32), ("total_frames", C.c_int64),
                ("n_frames", C.c_int32), ("delay", C.c_int32), ("padding", C.c_int32), ("reserved", C.c_int32)]


class Mp3Frame(C.Structure):
    _fields_ = [("main_at", C.c_int64), ("main_lo", C.c_int64), ("main_end", C.c_int64), ("stream", C.c_int32),
                ("number", C.c_int32), ("ms", C.c_int32), ("nodata", C.c_int32), ("scfsi", C.c_int32 * 2),
                ("part2_3_length", C.c_int32 * 4), ("big_values", C.c_int32 * 4), ("global_gain", C.c_int32 * 4),
                ("scalefac_compress", C.c_int32 * 4), ("window_switching", C.c_int32 * 4),
                ("block_type", C.c_int32 * 4), ("mixed", C.c_int32 * 4), ("table_select", C.c_int32 * 12),
                ("subblock_gain", C.c_int32 * 12), ("region0_count", C.c_int32 * 4), ("region1_count", C.c_int32 * 4),
                ("preflag", C.c_int32 * 4), ("scalefac_scale", C.c_int32 * 4), ("count1table_select", C.c_int32 * 4)]


class Mp3Stream(C.Structure):
    _fields_ = [("out_at", C.c_int64), ("frames", C.c_int64), ("skip", C.c_int64), ("first_frame", C.c_int64),
                ("n_frames", C.c_int64), ("channels", C.c_int32), ("sample_rate", C.c_int32),
                ("sr_index", C.c_int32), ("reserved", C.c_int32)]


# aa_mp3_status (include/aa.h)
AA_MP3_OK = 0
AA_MP3_NODATA = 1
AA_MP3_MALFORMED = 2
AA_MP3_WG = 64


# the band-pass filter's geometry (include/aa.h AA_SOS_*)
AA_SOS_MAX_SECTIONS = 2
AA_SOS_CHUNK = 32
AA_SOS_BLOCK = 8192
AA_SOS_LEVELS = 16
AA_SOS_MAX_N = 1 << 28


# the old cacophony index's geometry (include/aa.h AA_CI_*)
AA_CI_N = 2048
AA_CI_HOP = 1024
AA_CI_BANDS = 10
AA_CI_MAX_REC = 64


class SosJob(C.Structure):
    _fields_ = [("src", C.c_int64), ("n", C.c_int64), ("dst", C.c_int64), ("n_sections", C.c_int32),
                ("n_levels", C.c_int32), ("sos", C.c_double * 12), ("p", C.c_double * 16),
                ("pw", C.c_double * 256)]


_lib = None

_SIGS = {
    "aa_abi_version": (C.c_int, []),
    "aa_last_error": (C.c_char_p, []),
    "aa_fe_create": (C.c_int, [C.POINTER(FeConfig), C.c_void_p, C.POINTER(C.c_void_p)]),
    "aa_fe_destroy": (C.c_int, [C.c_void_p]),
    "aa_fe_n_frames": (C.c_int, [C.c_void_p]),
    "aa_fe_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32]),
    "aa_fe_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "aa_fe_n_stages": (C.c_int, [C.c_void_p]),
    "aa_fe_stage_info": (C.c_int, [C.c_void_p, C.c_int32, C.c_char_p, C.c_int32,
                                   C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "aa_fe_set_timing": (C.c_int, [C.c_void_p, C.c_uint32]),
    "aa_fe_stage_time": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double),
                                   C.POINTER(C.c_int64)]),
    "aa_fe_plan": (C.c_int, [C.POINTER(FeConfig), C.c_void_p, C.POINTER(C.c_void_p)]),
    "aa_fe_plan_info": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(FeInfo)]),
    "aa_fe_plan_image": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "aa_fe_plan_passes": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]),
    "aa_model_create": (C.c_int, [C.POINTER(Layer), C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                  C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "aa_model_destroy": (C.c_int, [C.c_void_p]),
    "aa_model_n_outputs": (C.c_int, [C.c_void_p]),
    "aa_model_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32]),
    "aa_model_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "aa_model_n_stages": (C.c_int, [C.c_void_p]),
    "aa_model_stage_info": (C.c_int, [C.c_void_p, C.c_int32, C.c_char_p, C.c_int32,
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "aa_model_set_timing": (C.c_int, [C.c_void_p, C.c_uint32]),
    "aa_model_set_input_f16": (C.c_int, [C.c_void_p, C.c_int32]),
    "aa_model_stage_time": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double),
                                      C.POINTER(C.c_int64)]),
    "aa_model_stage_shape": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32)]),
    "aa_model_forward_prefix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_void_p]),
    "aa_model_plan": (C.c_int, [C.POINTER(Layer), C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "aa_model_stage_image": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                       C.POINTER(C.c_size_t)]),
    "aa_model_first_lane_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "aa_graph_create": (C.c_int, [C.POINTER(Node), C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "aa_graph_destroy": (C.c_int, [C.c_void_p]),
    "aa_graph_n_outputs": (C.c_int, [C.c_void_p]),
    "aa_graph_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32]),
    "aa_graph_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_size_t, C.c_void_p]),
    "aa_graph_n_stages": (C.c_int, [C.c_void_p]),
    "aa_graph_set_timing": (C.c_int, [C.c_void_p, C.c_uint32]),
    "aa_graph_time_stage": (C.c_int, [C.c_void_p, C.c_int32]),
    "aa_graph_stage_time": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "aa_graph_stage_info": (C.c_int, [C.c_void_p, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double)]),
    "aa_graph_plan": (C.c_int, [C.POINTER(Node), C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "aa_graph_node_plan": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(NodePlan)]),
    "aa_graph_plan_layout": (C.c_int, [C.c_void_p, C.POINTER(GraphLayout)]),
    "aa_graph_node_image": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_size_t)]),
    "aa_track_mean": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "aa_span_nonzero": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                  C.c_void_p]),
    "aa_sosfilt_plan": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.POINTER(SosJob)]),
    "aa_sosfilt_workspace_bytes": (C.c_size_t, [C.POINTER(SosJob), C.c_int32]),
    "aa_sosfilt_run": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_size_t,
                                 C.c_void_p]),
    "aa_pcm_s16_to_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "aa_resample_poly": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "aa_resample_batch": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64,
                                    C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                    C.c_void_p]),
    "aa_sn_create": (C.c_int, [C.POINTER(SnConfig), C.POINTER(C.c_void_p)]),
    "aa_sn_destroy": (C.c_int, [C.c_void_p]),
    "aa_sn_geometry": (C.c_int, [C.POINTER(SnConfig), C.POINTER(C.c_int32)]),
    "aa_sn_n_frames": (C.c_int64, [C.c_void_p, C.c_int64]),
    "aa_sn_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int64]),
    "aa_sn_batch_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int32]),
    "aa_sn_run_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32,
                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32,
                                  C.c_void_p]),
    "aa_sn_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p,
                            C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aa_sn_spectrogram": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "aa_sn_n_stages": (C.c_int, [C.c_void_p]),
    "aa_sn_stage_info": (C.c_int, [C.c_void_p, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_double),
                                   C.POINTER(C.c_double)]),
    "aa_sn_set_timing": (C.c_int, [C.c_void_p, C.c_uint32]),
    "aa_sn_stage_time": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "aa_sn_components_from_mask": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "aa_ci_n_frames": (C.c_int64, [C.c_int64]),
    "aa_ci_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "aa_ci_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "aa_ci_destroy": (C.c_int, [C.c_void_p]),
    "aa_ci_workspace_bytes": (C.c_size_t, [C.POINTER(C.c_int64), C.c_int32]),
    "aa_ci_run": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32,
                            C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aa_flac_info": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(FlacInfo)]),
    "aa_flac_decode": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "aa_flac_index": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(FlacInfo), C.c_void_p, C.c_int64,
                                C.POINTER(C.c_int64)]),
    "aa_flac_device_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int64]),
    "aa_flac_decode_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "aa_flac_decode_frames_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "aa_vorbis_info": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(VorbisInfo)]),
    "aa_vorbis_decode": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "aa_vorbis_index": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(VorbisStream), C.c_void_p, C.c_int64,
                                  C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                  C.POINTER(C.c_int64)]),
    "aa_vorbis_device_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                      C.POINTER(VorbisPlan)]),
    "aa_vorbis_decode_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_int64, C.POINTER(VorbisPlan), C.c_void_p, C.c_void_p,
                                          C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "aa_vorbis_decode_packets_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                C.c_void_p, C.c_int64, C.POINTER(VorbisPlan), C.c_void_p,
                                                C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                                                C.c_void_p]),
    "aa_mp3_info": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(Mp3Info)]),
    "aa_mp3_decode": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "aa_mp3_index": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(Mp3Stream), C.c_void_p, C.c_int64,
                               C.POINTER(C.c_int64), C.c_void_p, C.c_int64]),
    "aa_mp3_tables": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "aa_mp3_table": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "aa_mp3_synth_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "aa_mp3_device_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "aa_mp3_decode_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "aa_mp3_decode_frames_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                            C.c_size_t]),
    "aa_read_file": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "aa_tracks_from_signals": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int32, C.c_void_p,
                                         C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
}

EXPORTED = tuple(_SIGS)


def lib():
    """Load libaa.so once; raises if it is absent (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise AAError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc gfx950)")
        h = C.CDLL(str(LIB_PATH))
        for name, (res, args) in _SIGS.items():
            try:
                f = getattr(h, name)
            except AttributeError:
                if os.environ.get("AA_LIB_AB"):
                    continue  # an older A/B build (tools/ab_head.py) lacks newer entry points
                raise AAError(f"{LIB_PATH} lacks {name}: a stale libaa.so (rebuild with __graft_entry__.build())")
            f.restype = res
            f.argtypes = args
        v = h.aa_abi_version()
        if v != ABI_VERSION:
            raise AAError(f"libaa.so ABI {v} != {ABI_VERSION}")
        _lib = h
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().aa_last_error().decode(errors="replace")
        raise AAError(f"{what or 'libaa'} failed ({rc}): {msg}")


def stream_ptr(stream=None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def dptr(t) -> int:
    if t is None:
        return 0
    if not t.is_cuda:
        raise AAError("libaa needs device tensors")
    if not t.is_contiguous():
        raise AAError("libaa needs contiguous tensors")
    return int(t.data_ptr())


class StageTiming:
    """Per-launch HIP-event timing of a plan/model handle (aa_fe_stage_* /
    aa_model_stage_*); subclasses set ``_timing_prefix`` and ``_h``."""
    _timing_prefix = ""

    def _fn(self, what):
        return getattr(lib(), f"{self._timing_prefix}_{what}")

    def n_stages(self) -> int:
        return self._fn("n_stages")(self._h)

    def stage_info(self, i: int):
        """(name, algorithmic flops per window, algorithmic bytes per window)"""
        name = C.create_string_buffer(96)
        fl, by = C.c_double(), C.c_double()
        check(self._fn("stage_info")(self._h, i, name, 96, C.byref(fl), C.byref(by)),
              f"{self._timing_prefix}_stage_info")
        return name.value.decode(), fl.value, by.value

    def set_timing(self, on=True, stages=None) -> None:
        """Time every stage (``on``) or only the stage indices in ``stages``
        (graphs: one stage, or every one)."""
        if self._timing_prefix == "aa_graph" and on and stages is not None:
            st = list(stages)
            if len(st) != 1:
                raise ValueError("graph models time one node or every node (stages=None), "
                                 f"not a subset of {len(st)}")
            check(lib().aa_graph_time_stage(self._h, int(st[0])), "aa_graph_time_stage")
            return
        mask = 0
        if on:
            mask = 0xFFFFFFFF if stages is None else sum(1 << int(i) for i in stages)
        check(self._fn("set_timing")(self._h, mask), f"{self._timing_prefix}_set_timing")

    def stage_time(self, i: int):
        """(total ms, launches) recorded for stage i since the last call"""
        ms, cnt = C.c_double(), C.c_int64()
        check(self._fn("stage_time")(self._h, i, C.byref(ms), C.byref(cnt)),
              f"{self._timing_prefix}_stage_time")
        return ms.value, cnt.value
