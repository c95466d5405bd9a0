"""ctypes binding of libac3mi.so — signatures follow include/ac3mi.h one to one."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AC3MI_LIB") or os.path.join(_HERE, "libac3mi.so")   # override: A/B builds only
HEADER_DIR = os.path.join(os.path.dirname(_HERE), "include")

c_void_p, c_int, c_float, c_size_t, c_char_p = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
                                                ctypes.c_size_t, ctypes.c_char_p)


class AC3MIError(RuntimeError):
    pass


class XformDescC(ctypes.Structure):
    _fields_ = [("acmod", c_int), ("lfeon", c_int), ("output", c_int), ("bias", c_float)]


class DecodeDescC(ctypes.Structure):
    _fields_ = [("flags", c_int), ("level", c_float), ("bias", c_float), ("dynrng", c_int),
                ("acmod", c_int), ("lfeon", c_int), ("frame_bytes", c_int)]


class DecodeTapsC(ctypes.Structure):
    _fields_ = [("d_coef", c_void_p), ("d_blksw", c_void_p), ("d_exp", c_void_p), ("d_bap", c_void_p),
                ("d_dynrng_out", c_void_p), ("d_dynrng_in", c_void_p)]


class EncodeDescC(ctypes.Structure):
    _fields_ = [("sample_rate", c_int), ("bit_rate", c_int), ("channels", c_int)]


class EncodeTapsC(ctypes.Structure):
    _fields_ = [("d_mdct", c_void_p), ("d_exponent", c_void_p), ("d_exp_samples", c_void_p),
                ("d_encoded_exp", c_void_p), ("d_bap", c_void_p), ("d_exp_strategy", c_void_p),
                ("d_snroffst", c_void_p)]


class BsiInfoC(ctypes.Structure):
    """ac3mi_bsi_info"""
    _fields_ = ([(k, ctypes.c_uint8) for k in ("verdict", "fscod", "frmsizecod", "bsid", "bsmod", "acmod", "lfeon", "cmixlev",
                                               "surmixlev", "dsurmod", "dialnorm", "dialnorm2", "compr", "compr2", "langcod",
                                               "langcod2", "audprodi", "audprodi2", "copyrightb", "origbs", "addbsil", "reserved")] +
                [(k, ctypes.c_uint16) for k in ("present", "timecod1", "timecod2", "block0_bit", "reserved2")] +
                [("word", ctypes.c_uint32)])


def bsi_info_dtype():
    """ac3mi_bsi_info as a numpy structured dtype (36 bytes; a uint8 tensor [..., 36] views as it)"""
    import numpy as np
    t = {ctypes.c_uint8: "u1", ctypes.c_uint16: "<u2", ctypes.c_uint32: "<u4"}
    dt = np.dtype([(k, t[c]) for k, c in BsiInfoC._fields_])
    assert dt.itemsize == ctypes.sizeof(BsiInfoC) == 36
    return dt


class FrameRefC(ctypes.Structure):
    """ac3mi_frame_ref"""
    _fields_ = [("offset", ctypes.c_uint32), ("bytes", ctypes.c_uint16), ("sizecod", ctypes.c_uint8), ("reserved", ctypes.c_uint8)]


class ScanInfoC(ctypes.Structure):
    """ac3mi_scan_info"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("n_frames", "consumed", "skipped", "rejected", "flags", "reserved")]


class LoudnessDescC(ctypes.Structure):
    """ac3mi_loudness_desc"""
    _fields_ = [("sample_rate", ctypes.c_int), ("channels", ctypes.c_int), ("role", ctypes.c_uint8 * 6)]


class ResampleDescC(ctypes.Structure):
    """ac3mi_resample_desc"""
    _fields_ = [("in_rate", ctypes.c_int), ("out_rate", ctypes.c_int), ("channels", ctypes.c_int)]


class LoudnessResultC(ctypes.Structure):
    """ac3mi_loudness_result"""
    _fields_ = [("mean_energy", ctypes.c_double), ("max_block_energy", ctypes.c_double), ("lkfs", ctypes.c_float),
                ("blocks", ctypes.c_uint32), ("blocks_abs", ctypes.c_uint32), ("blocks_rel", ctypes.c_uint32),
                ("dialnorm", ctypes.c_uint8), ("flags", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 6)]


def loudness_result_dtype():
    """ac3mi_loudness_result as a numpy structured dtype (40 bytes; a uint8 tensor [..., 40] views as it)"""
    import numpy as np
    dt = np.dtype([("mean_energy", "<f8"), ("max_block_energy", "<f8"), ("lkfs", "<f4"), ("blocks", "<u4"), ("blocks_abs", "<u4"),
                   ("blocks_rel", "<u4"), ("dialnorm", "u1"), ("flags", "u1"), ("reserved", "u1", (6,))])
    assert dt.itemsize == ctypes.sizeof(LoudnessResultC) == 40
    return dt


class LoudnessRangeResultC(ctypes.Structure):
    """ac3mi_loudness_range_result"""
    _fields_ = [("max_short_energy", ctypes.c_double), ("lra", ctypes.c_float), ("low_lkfs", ctypes.c_float), ("high_lkfs", ctypes.c_float),
                ("max_short_lkfs", ctypes.c_float), ("blocks", ctypes.c_uint32), ("blocks_abs", ctypes.c_uint32),
                ("blocks_rel", ctypes.c_uint32), ("lra_tenths", ctypes.c_uint16), ("low_bin", ctypes.c_uint16),
                ("high_bin", ctypes.c_uint16), ("flags", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 5)]


def loudness_range_result_dtype():
    """ac3mi_loudness_range_result as a numpy structured dtype (48 bytes; a uint8 tensor [..., 48] views as it)"""
    import numpy as np
    dt = np.dtype([("max_short_energy", "<f8"), ("lra", "<f4"), ("low_lkfs", "<f4"), ("high_lkfs", "<f4"), ("max_short_lkfs", "<f4"),
                   ("blocks", "<u4"), ("blocks_abs", "<u4"), ("blocks_rel", "<u4"), ("lra_tenths", "<u2"), ("low_bin", "<u2"),
                   ("high_bin", "<u2"), ("flags", "u1"), ("reserved", "u1", (5,))])
    assert dt.itemsize == ctypes.sizeof(LoudnessRangeResultC) == 48
    return dt


class TruePeakResultC(ctypes.Structure):
    """ac3mi_truepeak_result"""
    _fields_ = [("true_peak_index", ctypes.c_uint64), ("samples", ctypes.c_uint64), ("true_peak", ctypes.c_uint32),
                ("sample_peak", ctypes.c_uint32), ("full_scale", ctypes.c_uint32), ("slot_true_peak", ctypes.c_uint32 * 6),
                ("slot_sample_peak", ctypes.c_uint32 * 6), ("dbtp", ctypes.c_float), ("dbfs", ctypes.c_float),
                ("true_peak_slot", ctypes.c_uint8), ("sample_peak_slot", ctypes.c_uint8), ("flags", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8 * 9)]


def truepeak_result_dtype():
    """ac3mi_truepeak_result as a numpy structured dtype (96 bytes; a uint8 tensor [..., 96] views as it)"""
    import numpy as np
    dt = np.dtype([("true_peak_index", "<u8"), ("samples", "<u8"), ("true_peak", "<u4"), ("sample_peak", "<u4"), ("full_scale", "<u4"),
                   ("slot_true_peak", "<u4", (6,)), ("slot_sample_peak", "<u4", (6,)), ("dbtp", "<f4"), ("dbfs", "<f4"),
                   ("true_peak_slot", "u1"), ("sample_peak_slot", "u1"), ("flags", "u1"), ("reserved", "u1", (9,))])
    assert dt.itemsize == ctypes.sizeof(TruePeakResultC) == 96
    return dt


class LimitResultC(ctypes.Structure):
    """ac3mi_limit_result"""
    _fields_ = [("samples", ctypes.c_uint64), ("reduced", ctypes.c_uint64), ("max_detect", ctypes.c_uint32),
                ("min_gain_q24", ctypes.c_uint32), ("in_dbtp", ctypes.c_float), ("reduction_db", ctypes.c_float),
                ("flags", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 7)]


def limit_result_dtype():
    """ac3mi_limit_result as a numpy structured dtype (40 bytes; a uint8 tensor [..., 40] views as it)"""
    import numpy as np
    dt = np.dtype([("samples", "<u8"), ("reduced", "<u8"), ("max_detect", "<u4"), ("min_gain_q24", "<u4"), ("in_dbtp", "<f4"),
                   ("reduction_db", "<f4"), ("flags", "u1"), ("reserved", "u1", (7,))])
    assert dt.itemsize == ctypes.sizeof(LimitResultC) == 40
    return dt


def _struct_dtype(cls, size):
    import numpy as np
    t = {ctypes.c_uint8: "u1", ctypes.c_uint16: "<u2", ctypes.c_uint32: "<u4"}
    dt = np.dtype([(k, t[c]) for k, c in cls._fields_])
    assert dt.itemsize == ctypes.sizeof(cls) == size
    return dt


def frame_ref_dtype():
    """ac3mi_frame_ref as a numpy structured dtype (8 bytes; a uint8 tensor [..., 8] views as it)"""
    return _struct_dtype(FrameRefC, 8)


def scan_info_dtype():
    """ac3mi_scan_info as a numpy structured dtype (24 bytes; a uint8 tensor [..., 24] views as it)"""
    return _struct_dtype(ScanInfoC, 24)


_lib = None


def declared_symbols():
    """Every function name declared in include/*.h (the drop-in boundary)."""
    names = []
    for fn in sorted(os.listdir(HEADER_DIR)):
        if not fn.endswith(".h"):
            continue
        text = open(os.path.join(HEADER_DIR, fn)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"typedef[^;{]*\(\s*\*[^;]*;", "", text)        # function-pointer typedefs
        for m in re.finditer(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{}]*\)\s*;", text):
            if m.group(1) not in ("defined", "sizeof", "void", "int"):
                names.append(m.group(1))
        for m in re.finditer(r"extern\s+\w+\s+(\w+)\s*\[", text):      # exported tables (MapTab)
            names.append(m.group(1))
    return sorted(set(names))


def load_library():
    """Load libac3mi.so; raises loudly when the HIP library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AC3MIError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(there is no CPU fallback)" % LIB_PATH)
    # torch wheels carry their own libamdhip64; if libac3mi.so pulled in /opt/rocm's copy
    # first, torch would later see "No HIP GPUs".  Load torch's runtime first so the
    # process holds exactly one HIP runtime (plumbing concern only: C hosts have no torch).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    lib.ac3mi_create.restype = c_void_p
    lib.ac3mi_create.argtypes = [c_int]
    lib.ac3mi_destroy.argtypes = [c_void_p]
    lib.ac3mi_destroy.restype = None
    lib.ac3mi_last_error.restype = c_char_p
    lib.ac3mi_last_error.argtypes = [c_void_p]
    lib.ac3mi_device_count.restype = c_int
    lib.ac3mi_dev_alloc.restype = c_void_p
    lib.ac3mi_dev_alloc.argtypes = [c_void_p, c_size_t]
    lib.ac3mi_dev_free.argtypes = [c_void_p, c_void_p]
    lib.ac3mi_dev_free.restype = None
    lib.ac3mi_memcpy_h2d.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t]
    lib.ac3mi_memcpy_d2h.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t]
    lib.ac3mi_memset.argtypes = [c_void_p, c_void_p, c_int, c_size_t]
    lib.ac3mi_set_encode_mode.argtypes = [c_void_p, c_int]
    lib.ac3mi_set_encode_block_switch.argtypes = [c_void_p, c_int]
    lib.ac3mi_set_encode_rematrix.argtypes = [c_void_p, c_int]
    lib.ac3mi_set_encode_coupling.argtypes = [c_void_p, c_int, c_int]
    lib.ac3mi_set_encode_bandwidth.argtypes = [c_void_p, c_int, c_int]
    lib.ac3mi_set_encode_metadata.argtypes = [c_void_p, c_void_p]
    lib.ac3mi_encode_metadata_word.argtypes = [c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    lib.ac3mi_set_encode_metadata_frames.argtypes = [c_void_p, c_void_p]
    lib.ac3mi_set_encode_metadata_source.argtypes = [c_void_p, c_int]
    lib.ac3mi_bsi_read.argtypes = [c_void_p, c_int, ctypes.POINTER(BsiInfoC)]
    lib.ac3mi_bsi_read_batch.argtypes = [c_void_p, c_void_p, c_int, c_int, c_size_t, c_void_p]
    lib.ac3mi_frame_scan.argtypes = [c_void_p, c_size_t, c_int, c_int, ctypes.POINTER(FrameRefC), ctypes.POINTER(ScanInfoC)]
    lib.ac3mi_frame_scan_batch.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.ac3mi_frame_gather_batch.argtypes = [c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                             c_void_p, c_int, c_int]
    lib.ac3mi_loudness_state_bytes.restype = c_size_t
    lib.ac3mi_loudness_state_bytes.argtypes = []
    lib.ac3mi_loudness_roles.argtypes = [c_int, c_void_p]
    lib.ac3mi_loudness_tables.argtypes = [c_int, c_void_p, c_void_p, c_void_p]
    lib.ac3mi_loudness_batch.argtypes = [c_void_p, ctypes.POINTER(LoudnessDescC), c_void_p, c_int, c_int, c_void_p]
    lib.ac3mi_loudness_read_batch.argtypes = [c_void_p, c_void_p, c_int, c_void_p]
    lib.ac3mi_loudness_read.argtypes = [c_void_p, ctypes.POINTER(LoudnessResultC)]
    lib.ac3mi_loudness_words_batch.argtypes = [c_void_p, c_void_p, c_int, c_int, ctypes.c_uint32, c_void_p]
    lib.ac3mi_loudness_range_state_bytes.restype = c_size_t
    lib.ac3mi_loudness_range_state_bytes.argtypes = []
    lib.ac3mi_loudness_range_batch.argtypes = [c_void_p, ctypes.POINTER(LoudnessDescC), c_void_p, c_int, c_int, c_void_p, c_void_p]
    lib.ac3mi_loudness_range_read_batch.argtypes = [c_void_p, c_void_p, c_int, c_void_p]
    lib.ac3mi_loudness_range_read.argtypes = [c_void_p, ctypes.POINTER(LoudnessRangeResultC)]
    lib.ac3mi_truepeak_state_bytes.restype = c_size_t
    lib.ac3mi_truepeak_state_bytes.argtypes = []
    lib.ac3mi_truepeak_tables.argtypes = [c_void_p]
    lib.ac3mi_truepeak_ceiling.restype = ctypes.c_uint32
    lib.ac3mi_truepeak_ceiling.argtypes = [ctypes.c_double]
    lib.ac3mi_truepeak_batch.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p]
    lib.ac3mi_truepeak_read_batch.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_uint32, c_void_p]
    lib.ac3mi_truepeak_read.argtypes = [c_void_p, ctypes.c_uint32, ctypes.POINTER(TruePeakResultC)]
    lib.ac3mi_truepeak_host.argtypes = [c_int, c_void_p, c_void_p, c_int, c_void_p]
    lib.ac3mi_limit_state_bytes.restype = c_size_t
    lib.ac3mi_limit_state_bytes.argtypes = []
    lib.ac3mi_limit_release_step.restype = ctypes.c_uint32
    lib.ac3mi_limit_release_step.argtypes = [c_int, ctypes.c_double]
    lib.ac3mi_limit_batch.argtypes = [c_void_p, c_int, c_void_p, ctypes.c_uint32, ctypes.c_uint32, c_void_p, c_void_p, c_int, c_int, c_void_p]
    lib.ac3mi_limit_read_batch.argtypes = [c_void_p, c_void_p, c_int, c_void_p]
    lib.ac3mi_limit_read.argtypes = [c_void_p, ctypes.POINTER(LimitResultC)]
    lib.ac3mi_limit_host.argtypes = [c_int, c_void_p, ctypes.c_uint32, ctypes.c_uint32, c_void_p, c_void_p, c_int, c_void_p]
    lib.ac3mi_resample_ratio.argtypes = [c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    lib.ac3mi_resample_tables.argtypes = [c_int, c_int, c_void_p]
    lib.ac3mi_resample_state_bytes.restype = c_size_t
    lib.ac3mi_resample_state_bytes.argtypes = []
    lib.ac3mi_resample_plan.argtypes = [c_int, c_int, ctypes.c_uint64, ctypes.c_uint64, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    lib.ac3mi_resample_batch.argtypes = [c_void_p, ctypes.POINTER(ResampleDescC), c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]
    lib.ac3mi_resample_host.argtypes = [ctypes.POINTER(ResampleDescC), c_void_p, c_int, c_void_p, c_int, c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    lib.ac3mi_set_encode_drc.argtypes = [c_void_p, c_int, c_void_p]
    lib.ac3mi_set_encode_dynrng_frames.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.ac3mi_set_encode_drc_source.argtypes = [c_void_p, c_int]
    lib.ac3mi_set_encode_exp_strategy.argtypes = [c_void_p, c_int]
    lib.ac3mi_set_encode_layout.argtypes = [c_void_p, c_int, c_int, c_int]
    lib.ac3mi_memcpy_d2d.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t]
    lib.ac3mi_sync.argtypes = [c_void_p]
    lib.ac3mi_timer_start.argtypes = [c_void_p]
    lib.ac3mi_timer_stop.argtypes = [c_void_p, ctypes.POINTER(c_float)]
    lib.ac3mi_xform_planes.argtypes = [ctypes.POINTER(XformDescC), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    lib.ac3mi_imdct_batch.argtypes = [c_void_p, ctypes.POINTER(XformDescC), c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_int, c_int]
    lib.ac3mi_syncinfo.argtypes = [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    lib.ac3mi_decode_planes.argtypes = [ctypes.POINTER(DecodeDescC), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    lib.ac3mi_decode_batch.argtypes = [c_void_p, ctypes.POINTER(DecodeDescC), c_void_p, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(DecodeTapsC)]
    lib.ac3mi_decode_s16_batch.argtypes = [c_void_p, ctypes.POINTER(DecodeDescC), c_void_p, c_int, c_int, c_int,
                                           c_void_p, c_void_p, c_void_p, c_void_p]
    lib.ac3mi_encode_frame_bytes.argtypes = [ctypes.POINTER(EncodeDescC)]
    lib.ac3mi_encode_tables.argtypes = [c_void_p] * 5
    lib.ac3mi_encode_batch.argtypes = [c_void_p, ctypes.POINTER(EncodeDescC), c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_int, c_int, c_int, ctypes.POINTER(EncodeTapsC)]
    lib.ac3mi_set_decode_mode.argtypes = [c_void_p, ctypes.c_int]
    if hasattr(lib, "ac3mi_set_fixed_shape"):       # (absent from a build of before it: AC3MI_LIB A/B runs)
        lib.ac3mi_set_fixed_shape.argtypes = [c_void_p, ctypes.c_int]
    if hasattr(lib, "ac3mi_fill_workspaces"):       # (likewise)
        lib.ac3mi_fill_workspaces.argtypes = [c_void_p, ctypes.c_int]
    if hasattr(lib, "ac3mi_debug_search_curve"):    # (likewise)
        lib.ac3mi_debug_search_curve.argtypes = [c_void_p, c_void_p]
    if hasattr(lib, "ac3mi_debug_launch_log"):      # (likewise)
        lib.ac3mi_debug_launch_log.argtypes = [c_void_p, c_void_p, ctypes.c_int]
    lib.ac3mi_set_decode_crc.argtypes = [c_void_p, ctypes.c_int]
    lib.ac3mi_crc_check_batch.argtypes = [c_void_p, c_void_p, c_int, c_int, c_size_t, c_void_p]
    lib.ac3mi_set_mix_state.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.ac3mi_probe_valu_rate.argtypes = [c_void_p, ctypes.POINTER(ctypes.c_double)]
    lib.ac3mi_probe_salu_rate.argtypes = [c_void_p, ctypes.POINTER(ctypes.c_double)]
    lib.ac3mi_probe_mixed_rate.argtypes = [c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    lib.ac3mi_probe_copy_rate.argtypes = [c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double)]
    lib.ac3mi_set_tile_frames.argtypes = [c_void_p, ctypes.c_longlong]
    lib.ac3mi_transcode_batch.argtypes = [c_void_p, ctypes.POINTER(DecodeDescC), ctypes.POINTER(EncodeDescC), c_void_p, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          ctypes.c_int, c_void_p]
    _lib = lib
    return lib
