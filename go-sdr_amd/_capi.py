"""ctypes declarations for libhzsdr_hip.so (include/hzsdr.h).

The product path is the HIP library: if it is missing this module raises at
import time -- there is no CPU fallback.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# HZSDR_LIB: another build of the same library (A/B measurements of two kernels in one GPU call)
LIB_PATH = os.environ.get("HZSDR_LIB") or os.path.join(_HERE, "libhzsdr_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libhzsdr_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
        "or `make -C go-sdr_amd/csrc` (needs hipcc); there is no CPU fallback")



def _one_hip_runtime():
    """One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64
    (same SONAME as /opt/rocm's).  If this library is loaded first it binds the
    system copy, a later `import torch` maps the bundled copy as well, and the
    second runtime to initialise finds no GPU ("No HIP GPUs are available").
    So when torch is installed but not imported yet, map ITS runtime first: the
    dynamic loader then satisfies our DT_NEEDED libamdhip64.so.7 with it, and
    torch's own import later reuses the same mapping.  Without torch (the cgo /
    C++ case) nothing happens and the system ROCm runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        with open("/proc/self/maps") as f:
            if any("libamdhip64" in line for line in f):
                return
    except OSError:
        pass
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(p):
        C.CDLL(p, mode=C.RTLD_GLOBAL)


_one_hip_runtime()
lib = C.CDLL(LIB_PATH)

FMT_C64, FMT_U8, FMT_I16, FMT_I8 = 1, 2, 3, 4
MEM_HOST, MEM_DEVICE = 0, 1
FFT_BACKWARD, FFT_FORWARD = 0, 1
FIR_PATH_NONE, FIR_PATH_TRANSFORM, FIR_PATH_MATRIX = 0, 1, 2
FIR_KERNEL_NONE, FIR_KERNEL_TRANSFORM, FIR_KERNEL_MATRIX_CHUNKS, FIR_KERNEL_MATRIX_PASSES = 0, 1, 2, 3
FIR_IMPL_AUTO, FIR_IMPL_TRANSFORMS, FIR_IMPL_MATRIX_CHUNKS = 0, 1, 2  # hzsdr_chain_fir_options
CONV_CONVOLVE, CONV_CROSS_CORRELATE = 0, 1

(OK, ERR_FORMAT_MISMATCH, ERR_FORMAT_UNKNOWN, ERR_DST_TOO_SMALL, ERR_CONVERSION_NOT_IMPLEMENTED,
 ERR_LENGTH_MISMATCH, ERR_INVALID_ARGUMENT, ERR_NO_DEVICE, ERR_HIP, ERR_OUT_OF_MEMORY) = range(10)


class NcoSegment(C.Structure):
    _fields_ = [("first", C.c_uint64), ("count", C.c_uint64), ("t0", C.c_double),
                ("step", C.c_double)]


vp, sz, i32, u32, i64, u64, f32, f64 = (C.c_void_p, C.c_size_t, C.c_int, C.c_uint, C.c_int64,
                                        C.c_uint64, C.c_float, C.c_double)
psz = C.POINTER(C.c_size_t)
pvp = C.POINTER(C.c_void_p)

# name -> (restype, argtypes); every symbol include/hzsdr.h declares
SIGNATURES = {
    "hzsdr_backend": (C.c_char_p, []),
    "hzsdr_version": (C.c_char_p, []),
    "hzsdr_strerror": (C.c_char_p, [i32]),
    "hzsdr_format_size": (i32, [i32]),
    "hzsdr_device_count": (i32, [C.POINTER(i32)]),
    "hzsdr_open": (i32, [i32, i32, pvp]),
    "hzsdr_close": (i32, [vp]),
    "hzsdr_last_error": (C.c_char_p, [vp]),
    "hzsdr_memspace": (i32, [vp]),
    "hzsdr_set_stream": (i32, [vp, vp]),
    "hzsdr_use_own_stream": (i32, [vp]),
    "hzsdr_get_stream": (vp, [vp]),
    "hzsdr_synchronize": (i32, [vp]),
    "hzsdr_call_count": (i32, [vp, C.POINTER(C.c_ulonglong)]),
    "hzsdr_malloc_device": (i32, [vp, sz, pvp]),
    "hzsdr_free_device": (i32, [vp, vp]),
    "hzsdr_malloc_pinned": (i32, [vp, sz, pvp]),
    "hzsdr_free_pinned": (i32, [vp, vp]),
    "hzsdr_memcpy_h2d": (i32, [vp, vp, vp, sz]),
    "hzsdr_memcpy_d2h": (i32, [vp, vp, vp, sz]),
    "hzsdr_convert": (i32, [vp, i32, vp, sz, i32, vp, sz, psz]),
    "hzsdr_i16_shift_lsb_to_msb": (i32, [vp, vp, sz, i32]),
    "hzsdr_lut_create": (i32, [vp, i32, i32, vp, sz, pvp]),
    "hzsdr_lut_lookup": (i32, [vp, i32, vp, sz, i32, vp, sz, psz]),
    "hzsdr_lut_free": (i32, [vp]),
    "hzsdr_lut_identity": (i32, [vp]),
    "hzsdr_scale": (i32, [vp, vp, sz, f32]),
    "hzsdr_rotate": (i32, [vp, vp, sz, f32, f32]),
    "hzsdr_add": (i32, [vp, vp, sz, vp, sz, vp, sz]),
    "hzsdr_sum": (i32, [vp, i32, vp, pvp, i32, sz]),
    "hzsdr_rotlut_create": (i32, [vp, i32, f32, f32, pvp]),
    "hzsdr_rotlut_set_multiplier": (i32, [vp, f32, f32]),
    "hzsdr_rotlut_apply": (i32, [vp, vp, sz]),
    "hzsdr_rotlut_free": (i32, [vp]),
    "hzsdr_nco_create": (i32, [vp, u64, pvp]),
    "hzsdr_nco_shift": (i32, [vp, f64, vp, sz]),
    "hzsdr_nco_get_time": (i32, [vp, C.POINTER(f64)]),
    "hzsdr_nco_set_time": (i32, [vp, f64]),
    "hzsdr_nco_set_ulp1": (i32, [vp, i32]),
    "hzsdr_nco_free": (i32, [vp]),
    "hzsdr_nco_segments": (i32, [u64, f64, u64, C.POINTER(NcoSegment), sz, psz, C.POINTER(f64)]),
    "hzsdr_decimate": (i32, [vp, i32, vp, sz, i32, vp, sz, u32, i64, psz]),
    "hzsdr_downsample": (i32, [vp, i32, vp, sz, i32, vp, sz, u32, i64, psz]),
    "hzsdr_fft_plan": (i32, [vp, vp, sz, vp, sz, i32, pvp]),
    "hzsdr_fft_plan_batch": (i32, [vp, vp, vp, sz, sz, i32, pvp]),
    "hzsdr_fft_transform": (i32, [vp]),
    "hzsdr_fft_free": (i32, [vp]),
    "hzsdr_convolve_create": (i32, [vp, vp, sz, vp, sz, vp, sz, i32, pvp]),
    "hzsdr_convolve_freq_create": (i32, [vp, vp, sz, vp, sz, vp, sz, pvp]),
    "hzsdr_conv_exec": (i32, [vp]),
    "hzsdr_conv_set_filter": (i32, [vp, vp, sz]),
    "hzsdr_conv_free": (i32, [vp]),
    "hzsdr_convolution_blocks": (i32, [vp, vp, sz, vp, sz, vp, sz, psz]),
    "hzsdr_beamform_angles_2d": (i32, [f64, f64, C.POINTER(f64), C.POINTER(f64), i32,
                                       C.POINTER(f32)]),
    "hzsdr_beamform_angles": (i32, [f64, f64, C.POINTER(f64), i32, C.POINTER(f32)]),
    "hzsdr_beamform": (i32, [vp, vp, i32, pvp, C.POINTER(f32), i32, sz]),
    "hzsdr_beamform_partial": (i32, [vp, vp, i32, pvp, C.POINTER(f32), i32, sz, i32]),
    "hzsdr_peak_lag": (i32, [vp, vp, sz, C.POINTER(i64)]),
    "hzsdr_mean_phase": (i32, [vp, vp, vp, sz, C.POINTER(f64)]),
    "hzsdr_fftshift_scale": (i32, [vp, vp, sz, f32]),
    "hzsdr_graft": (i32, [vp, vp, sz, pvp, i32, sz]),
    "hzsdr_byteswap": (i32, [vp, i32, vp, sz]),
    "hzsdr_convert_foreign": (i32, [vp, i32, vp, sz, i32, i32, vp, sz, i32, psz]),
    "hzsdr_chain_create": (i32, [vp, i32, u64, pvp]),
    "hzsdr_chain_shift": (i32, [vp, f64]),
    "hzsdr_chain_gain": (i32, [vp, f32]),
    "hzsdr_chain_rotate": (i32, [vp, f32, f32]),
    "hzsdr_chain_decimate": (i32, [vp, u32]),
    "hzsdr_chain_downsample": (i32, [vp, u32]),
    "hzsdr_chain_convolution": (i32, [vp, vp, sz, u32]),
    "hzsdr_chain_fir_decimate": (i32, [vp, C.POINTER(f32), sz, u32]),
    "hzsdr_chain_mix_in_order": (i32, [vp, i32]),
    "hzsdr_chain_shift_ulp1": (i32, [vp, i32]),
    "hzsdr_chain_fir_options": (i32, [vp, i32, u32, i32]),
    "hzsdr_chain_pipeline": (i32, [vp, i32]),
    "hzsdr_chain_plan": (i32, [vp, sz, psz, psz]),
    "hzsdr_chain_run": (i32, [vp, vp, sz, vp, sz, psz, psz]),
    "hzsdr_chain_run_after": (i32, [vp, vp, sz, vp, sz, psz, psz, vp]),
    "hzsdr_chain_run_batch": (i32, [vp, vp, vp, sz, sz, sz, psz, psz]),
    "hzsdr_chain_run_batch_after": (i32, [vp, vp, vp, sz, sz, sz, psz, psz, vp]),
    "hzsdr_mgpu_open": (i32, [C.POINTER(C.c_int), i32, pvp]),
    "hzsdr_mgpu_close": (i32, [vp]),
    "hzsdr_mgpu_shards": (i32, [vp]),
    "hzsdr_mgpu_ctx": (i32, [vp, i32, pvp]),
    "hzsdr_mgpu_shard_channels": (i32, [i32, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hzsdr_mgpu_beamform": (i32, [vp, vp, i32, i32, C.POINTER(C.c_void_p), C.POINTER(C.c_float), i32, sz, i32]),
    "hzsdr_mgpu_synchronize": (i32, [vp]),
    "hzsdr_mgpu_last_error": (C.c_char_p, [vp]),
    "hzsdr_mgpu_peer_pairs": (i32, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hzsdr_chain_reset": (i32, [vp]),
    "hzsdr_chain_set_time": (i32, [vp, f64]),
    "hzsdr_chain_time": (i32, [vp, C.POINTER(f64)]),
    "hzsdr_chain_last_fir_path": (i32, [vp, C.POINTER(i32)]),
    "hzsdr_chain_last_fir_kernel": (i32, [vp, C.POINTER(i32)]),
    "hzsdr_chain_free": (i32, [vp]),
    "hzsdr_ring_create": (i32, [vp, sz, i32, pvp]),
    "hzsdr_ring_iq_buffer": (i32, [vp, pvp, psz, psz]),
    "hzsdr_ring_acquire": (i32, [vp, C.POINTER(i32), pvp]),
    "hzsdr_ring_submit": (i32, [vp, i32, sz]),
    "hzsdr_ring_submit_many": (i32, [vp, i32, i32, sz]),
    "hzsdr_ring_release": (i32, [vp, i32]),
    "hzsdr_ring_pop": (i32, [vp, pvp, psz]),
    "hzsdr_ring_in_flight": (i32, [vp]),
    "hzsdr_ring_free": (i32, [vp]),
}

# name -> (restype, argtypes); every symbol include/hzsdr_spectrum.h declares
SPECTRUM_SIGNATURES = {
    "hzsdr_spectrum_create": (i32, [vp, i32, sz, sz, sz, C.POINTER(f32), f32, i32, i32, pvp]),
    "hzsdr_spectrum_push": (i32, [vp, vp, sz, vp, sz, psz]),
    "hzsdr_spectrum_rows_for": (i32, [vp, sz, psz]),
    "hzsdr_spectrum_pending": (i32, [vp, psz, psz]),
    "hzsdr_spectrum_options": (i32, [vp, i32]),
    "hzsdr_spectrum_last_form": (i32, [vp, C.POINTER(i32)]),
    "hzsdr_spectrum_reset": (i32, [vp]),
    "hzsdr_spectrum_free": (i32, [vp]),
}
ORDER_ZERO_FIRST, ORDER_NEGATIVE_FIRST = 0, 1  # fft.ZeroFirst = false, fft.NegativeFirst = true (fft/result.go:34-47)
SPECTRUM_POWER, SPECTRUM_DB = 0, 1
SPECTRUM_FORM_AUTO, SPECTRUM_FORM_ROW_WALK, SPECTRUM_FORM_FRAME_PARALLEL = 0, 1, 2

# name -> (restype, argtypes); every symbol include/hzsdr_channelizer.h declares
CHANNELIZER_SIGNATURES = {
    "hzsdr_channelizer_create": (i32, [vp, i32, sz, C.POINTER(f32), sz, sz, i32, i32, pvp]),
    "hzsdr_channelizer_push": (i32, [vp, vp, sz, vp, sz, sz, psz]),
    "hzsdr_channelizer_frames_for": (i32, [vp, sz, psz]),
    "hzsdr_channelizer_pending": (i32, [vp, psz, C.POINTER(u64)]),
    "hzsdr_channelizer_reset": (i32, [vp]),
    "hzsdr_channelizer_free": (i32, [vp]),
}
CHANNELIZER_FRAME_MAJOR, CHANNELIZER_CHANNEL_MAJOR = 0, 1

# name -> (restype, argtypes); every symbol include/hzsdr_synthesizer.h declares
SYNTHESIZER_SIGNATURES = {
    "hzsdr_synthesizer_create": (i32, [vp, i32, sz, C.POINTER(f32), sz, sz, i32, i32, pvp]),
    "hzsdr_synthesizer_push": (i32, [vp, vp, sz, sz, vp, sz, psz]),
    "hzsdr_synthesizer_flush": (i32, [vp, vp, sz, psz]),
    "hzsdr_synthesizer_pending": (i32, [vp, psz, C.POINTER(u64)]),
    "hzsdr_synthesizer_group_frames": (i32, [vp, psz]),
    "hzsdr_synthesizer_reset": (i32, [vp]),
    "hzsdr_synthesizer_free": (i32, [vp]),
}

# name -> (restype, argtypes); every symbol include/hzsdr_resampler.h declares
RESAMPLER_SIGNATURES = {
    "hzsdr_resampler_create": (i32, [vp, i32, sz, sz, C.POINTER(f32), sz, sz, pvp]),
    "hzsdr_resampler_push": (i32, [vp, vp, sz, sz, vp, sz, sz, psz]),
    "hzsdr_resampler_flush": (i32, [vp, vp, sz, sz, psz]),
    "hzsdr_resampler_outputs_for": (i32, [vp, sz, psz]),
    "hzsdr_resampler_pending": (i32, [vp, C.POINTER(u64), C.POINTER(u64), psz]),
    "hzsdr_resampler_plan": (i32, [vp, psz, C.POINTER(i32)]),
    "hzsdr_resampler_reset": (i32, [vp]),
    "hzsdr_resampler_free": (i32, [vp]),
}
RESAMPLER_FORM_DIRECT, RESAMPLER_FORM_TAPS_GLOBAL, RESAMPLER_FORM_TAPS_UNIFORM, RESAMPLER_FORM_WINDOW_PADDED = 1, 2, 4, 8

# name -> (restype, argtypes); every symbol include/hzsdr_demod.h declares
DEMOD_SIGNATURES = {
    "hzsdr_demod_create": (i32, [vp, i32, i32, sz, C.POINTER(f32), sz, sz, pvp]),
    "hzsdr_demod_push": (i32, [vp, vp, sz, sz, vp, sz, sz, psz]),
    "hzsdr_demod_flush": (i32, [vp, vp, sz, sz, psz]),
    "hzsdr_demod_outputs_for": (i32, [vp, sz, psz]),
    "hzsdr_demod_pending": (i32, [vp, C.POINTER(u64), C.POINTER(u64), psz]),
    "hzsdr_demod_plan": (i32, [vp, psz, C.POINTER(i32)]),
    "hzsdr_demod_reset": (i32, [vp]),
    "hzsdr_demod_free": (i32, [vp]),
}
DEMOD_FM, DEMOD_PHASE, DEMOD_ENVELOPE, DEMOD_POWER = 1, 2, 3, 4
DEMOD_FORM_HALF_TILE, DEMOD_FORM_TRANSPOSED = 1, 2

# name -> (restype, argtypes); every symbol include/hzsdr_tuner.h declares
TUNER_SIGNATURES = {
    "hzsdr_tuner_create": (i32, [vp, i32, C.POINTER(C.c_uint32), sz, sz, C.POINTER(f32), sz, pvp]),
    "hzsdr_tuner_push": (i32, [vp, vp, sz, vp, sz, sz, psz]),
    "hzsdr_tuner_flush": (i32, [vp, vp, sz, sz, psz]),
    "hzsdr_tuner_outputs_for": (i32, [vp, sz, psz]),
    "hzsdr_tuner_pending": (i32, [vp, C.POINTER(u64), C.POINTER(u64), psz]),
    "hzsdr_tuner_plan": (i32, [vp, psz, psz, C.POINTER(i32)]),
    "hzsdr_tuner_set_words": (i32, [vp, sz, sz, C.POINTER(C.c_uint32)]),
    "hzsdr_tuner_readout": (i32, [vp, i32, sz, vp, sz]),
    "hzsdr_tuner_reset": (i32, [vp]),
    "hzsdr_tuner_free": (i32, [vp]),
}
TUNER_FORM_CHUNKED, TUNER_FORM_TRANSPOSED = 1, 2
TUNER_READ_TAPS, TUNER_READ_T2, TUNER_READ_T1, TUNER_READ_T0 = 1, 2, 3, 4

# name -> (restype, argtypes); every symbol include/hzsdr_chanbank.h declares
CHANBANK_SIGNATURES = {
    "hzsdr_chanbank_create": (i32, [vp, i32, sz, C.POINTER(f32), sz, sz, i32, i32, pvp]),
    "hzsdr_chanbank_push": (i32, [vp, vp, sz, vp, sz, sz, psz]),
    "hzsdr_chanbank_frames_for": (i32, [vp, sz, psz]),
    "hzsdr_chanbank_pending": (i32, [vp, psz, C.POINTER(u64)]),
    "hzsdr_chanbank_plan": (i32, [vp, psz, psz, C.POINTER(i32)]),
    "hzsdr_chanbank_readout": (i32, [vp, i32, sz, vp, sz]),
    "hzsdr_chanbank_reset": (i32, [vp]),
    "hzsdr_chanbank_free": (i32, [vp]),
}
CHANBANK_FORM_A_LDS = 1
CHANBANK_READ_DFT, CHANBANK_READ_TAPS = 1, 2

# name -> (restype, argtypes); every symbol include/hzsdr_covar.h declares
COVAR_SIGNATURES = {
    "hzsdr_covar_create": (i32, [vp, i32, sz, sz, pvp]),
    "hzsdr_covar_push": (i32, [vp, vp, sz, sz, vp, sz, sz, psz]),
    "hzsdr_covar_push_channels": (i32, [vp, pvp, sz, vp, sz, sz, psz]),
    "hzsdr_covar_flush": (i32, [vp, vp, sz, psz]),
    "hzsdr_covar_blocks_for": (i32, [vp, sz, psz]),
    "hzsdr_covar_pending": (i32, [vp, C.POINTER(u64), C.POINTER(u64), psz]),
    "hzsdr_covar_plan": (i32, [vp, psz, psz, C.POINTER(i32)]),
    "hzsdr_covar_reset": (i32, [vp]),
    "hzsdr_covar_free": (i32, [vp]),
    "hzsdr_scan_create": (i32, [vp, sz, vp, sz, pvp]),
    "hzsdr_scan_run": (i32, [vp, vp, sz, sz, vp, sz, sz]),
    "hzsdr_scan_free": (i32, [vp]),
}
COVAR_FORM_ONE_TILE, COVAR_FORM_THREE_TILES = 1, 2

# name -> (restype, argtypes); every symbol include/hzsdr_iir.h declares
IIR_SIGNATURES = {
    "hzsdr_iir_create": (i32, [vp, i32, C.POINTER(f32), sz, i32, sz, pvp]),
    "hzsdr_iir_push": (i32, [vp, vp, sz, sz, vp, sz, sz, psz]),
    "hzsdr_iir_set_sections": (i32, [vp, C.POINTER(f32), sz]),
    "hzsdr_iir_get_state": (i32, [vp, C.POINTER(f32), sz]),
    "hzsdr_iir_set_state": (i32, [vp, C.POINTER(f32), sz, u64]),
    "hzsdr_iir_position": (i32, [vp, C.POINTER(u64)]),
    "hzsdr_iir_plan": (i32, [vp, psz, psz, C.POINTER(i32)]),
    "hzsdr_iir_reset": (i32, [vp]),
    "hzsdr_iir_free": (i32, [vp]),
}
IIR_REAL_F32 = 32
IIR_MAX_SECTIONS, IIR_MAX_ROWS = 8, 8192
IIR_FORM_PER_ROW, IIR_FORM_COMPLEX = 1, 2

# name -> (restype, argtypes); every symbol include/hzsdr_symsync.h declares
SYMSYNC_SIGNATURES = {
    "hzsdr_symsync_create": (i32, [vp, i32, C.POINTER(f32), i32, sz, pvp]),
    "hzsdr_symsync_push": (i32, [vp, vp, sz, sz, vp, sz, sz, vp, psz]),
    "hzsdr_symsync_max_symbols": (i32, [vp, sz, psz]),
    "hzsdr_symsync_set_params": (i32, [vp, C.POINTER(f32)]),
    "hzsdr_symsync_get_state": (i32, [vp, C.POINTER(f32), sz]),
    "hzsdr_symsync_set_state": (i32, [vp, C.POINTER(f32), sz, u64]),
    "hzsdr_symsync_position": (i32, [vp, C.POINTER(u64)]),
    "hzsdr_symsync_plan": (i32, [vp, psz, psz, C.POINTER(i32)]),
    "hzsdr_symsync_reset": (i32, [vp]),
    "hzsdr_symsync_free": (i32, [vp]),
}
SYMSYNC_REAL_F32 = 32  # (IIR_REAL_F32: one value names the real float32 rows all along the chain)
SYMSYNC_MAX_ROWS = 8192
SYMSYNC_FORM_PER_ROW, SYMSYNC_FORM_COMPLEX = 1, 2

# name -> (restype, argtypes); every symbol include/hzsdr_carrier.h declares
CARRIER_SIGNATURES = {
    "hzsdr_carrier_create": (i32, [vp, i32, C.POINTER(f32), i32, sz, pvp]),
    "hzsdr_carrier_push": (i32, [vp, vp, sz, sz, vp, sz, vp, sz]),
    "hzsdr_carrier_set_params": (i32, [vp, C.POINTER(f32)]),
    "hzsdr_carrier_get_state": (i32, [vp, C.POINTER(C.c_uint32), sz]),
    "hzsdr_carrier_set_state": (i32, [vp, C.POINTER(C.c_uint32), sz, u64]),
    "hzsdr_carrier_position": (i32, [vp, C.POINTER(u64)]),
    "hzsdr_carrier_plan": (i32, [vp, psz, psz, C.POINTER(i32)]),
    "hzsdr_carrier_reset": (i32, [vp]),
    "hzsdr_carrier_free": (i32, [vp]),
}
CARRIER_TONE, CARRIER_BPSK, CARRIER_QPSK = 0, 1, 2
CARRIER_MAX_ROWS = 8192
CARRIER_FORM_PER_ROW, CARRIER_FORM_MODE = 1, 2

# name -> (restype, argtypes); every symbol include/hzsdr_agc.h declares
AGC_SIGNATURES = {
    "hzsdr_agc_create": (i32, [vp, i32, C.POINTER(f32), i32, sz, pvp]),
    "hzsdr_agc_push": (i32, [vp, vp, sz, sz, vp, sz, vp, sz]),
    "hzsdr_agc_set_params": (i32, [vp, C.POINTER(f32)]),
    "hzsdr_agc_get_state": (i32, [vp, C.POINTER(f32), sz]),
    "hzsdr_agc_set_state": (i32, [vp, C.POINTER(f32), sz, u64]),
    "hzsdr_agc_position": (i32, [vp, C.POINTER(u64)]),
    "hzsdr_agc_plan": (i32, [vp, psz, psz, C.POINTER(i32)]),
    "hzsdr_agc_reset": (i32, [vp]),
    "hzsdr_agc_free": (i32, [vp]),
}
AGC_REAL_F32 = 32  # (IIR_REAL_F32: one value names the real float32 rows all along the chain)
AGC_MAX_ROWS = 8192
AGC_FORM_PER_ROW, AGC_FORM_COMPLEX = 1, 2

# name -> (restype, argtypes); every symbol include/hzsdr_equalizer.h declares
EQUALIZER_SIGNATURES = {
    "hzsdr_equalizer_create": (i32, [vp, i32, i32, sz, sz, C.POINTER(f32), i32, sz, pvp]),
    "hzsdr_equalizer_push": (i32, [vp, vp, sz, sz, vp, vp, sz, vp, sz]),
    "hzsdr_equalizer_set_params": (i32, [vp, C.POINTER(f32)]),
    "hzsdr_equalizer_get_state": (i32, [vp, C.POINTER(f32), sz]),
    "hzsdr_equalizer_set_state": (i32, [vp, C.POINTER(f32), sz]),
    "hzsdr_equalizer_plan": (i32, [vp, psz, psz, C.POINTER(i32)]),
    "hzsdr_equalizer_reset": (i32, [vp]),
    "hzsdr_equalizer_free": (i32, [vp]),
}
EQUALIZER_REAL_F32 = 32  # (IIR_REAL_F32: one value names the real float32 rows all along the chain)
EQUALIZER_MAX_ROWS, EQUALIZER_MAX_TAPS = 8192, 64
EQUALIZER_CMA, EQUALIZER_DD_BPSK, EQUALIZER_DD_QPSK = 0, 1, 2
EQUALIZER_FORM_PER_ROW, EQUALIZER_FORM_COMPLEX = 1, 2

# name -> (restype, argtypes); every symbol include/hzsdr_framesync.h declares
FRAMESYNC_SIGNATURES = {
    "hzsdr_framesync_create": (i32, [vp, i32, C.c_uint, C.c_uint, u64, C.c_uint, C.c_uint, C.POINTER(u64), C.POINTER(C.c_uint), C.c_uint, i32, u64, sz, pvp]),
    "hzsdr_framesync_push": (i32, [vp, vp, sz, sz, vp, vp, sz, sz, vp, vp, vp, psz]),
    "hzsdr_framesync_get_state": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), sz]),
    "hzsdr_framesync_set_state": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), sz]),
    "hzsdr_framesync_positions": (i32, [vp, C.POINTER(u64), sz]),
    "hzsdr_framesync_plan": (i32, [vp, psz, psz, psz, C.POINTER(i32)]),
    "hzsdr_framesync_reset": (i32, [vp]),
    "hzsdr_framesync_free": (i32, [vp]),
}
FRAMESYNC_MAX_ROWS, FRAMESYNC_MAX_WORD, FRAMESYNC_MAX_PAYLOAD, FRAMESYNC_MAX_HYPOTHESES = 8192, 64, 8192, 4
FRAMESYNC_FORM_COMPLEX, FRAMESYNC_FORM_DIBIT, FRAMESYNC_FORM_DIFF = 1, 2, 4

# name -> (restype, argtypes); every symbol include/hzsdr_hdlc.h declares
HDLC_SIGNATURES = {
    "hzsdr_hdlc_create": (i32, [vp, i32, i32, C.c_uint, C.c_uint, C.c_uint, i32, i32, sz, pvp]),
    "hzsdr_hdlc_push": (i32, [vp, vp, sz, sz, vp, vp, sz, sz, vp, vp, vp, psz]),
    "hzsdr_hdlc_get_state": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), sz]),
    "hzsdr_hdlc_set_state": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), sz]),
    "hzsdr_hdlc_positions": (i32, [vp, C.POINTER(u64), sz]),
    "hzsdr_hdlc_plan": (i32, [vp, psz, psz, psz, C.POINTER(i32)]),
    "hzsdr_hdlc_reset": (i32, [vp]),
    "hzsdr_hdlc_free": (i32, [vp]),
}
HDLC_MAX_ROWS, HDLC_MAX_BYTES = 8192, 1024
HDLC_EVENT_ABORT, HDLC_EVENT_FLAG = 0, 1
HDLC_FORM_COMPLEX, HDLC_FORM_DIFF, HDLC_FORM_FCS16, HDLC_FORM_FCS32, HDLC_FORM_MSB_FIRST, HDLC_FORM_KEEP_BAD = 1, 4, 8, 16, 32, 64

# name -> (restype, argtypes); every symbol include/hzsdr_viterbi.h declares
VITERBI_SIGNATURES = {
    "hzsdr_viterbi_create": (i32, [vp, i32, C.c_uint, C.c_uint, C.POINTER(C.c_uint), C.c_uint, u64, C.c_uint, i32, sz, f32, C.c_uint, C.c_uint32, C.c_uint32,
                                   C.c_uint32, sz, pvp]),
    "hzsdr_viterbi_decode": (i32, [vp, vp, sz, vp, sz, vp, sz, vp]),
    "hzsdr_viterbi_sizes": (i32, [vp, psz, psz, psz, psz]),
    "hzsdr_viterbi_plan": (i32, [vp, psz, psz, psz, C.POINTER(i32)]),
    "hzsdr_viterbi_free": (i32, [vp]),
}
VITERBI_MAX_ROWS, VITERBI_MIN_K, VITERBI_MAX_K, VITERBI_MAX_RATE, VITERBI_MAX_PATTERN, VITERBI_MAX_BITS, VITERBI_MAX_FRAMES = 8192, 3, 9, 4, 64, 8192, 1 << 22
VITERBI_BITS, VITERBI_SOFT_F32 = 1, 32
VITERBI_TAIL, VITERBI_TRUNCATED = 0, 1
VITERBI_FORM_LDS, VITERBI_FORM_SCRATCH = 1, 2

# name -> (restype, argtypes); every symbol include/hzsdr_ldpc.h declares
LDPC_SIGNATURES = {
    "hzsdr_ldpc_create": (i32, [vp, i32, sz, sz, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), sz, sz, sz, sz, f32, C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                sz, pvp]),
    "hzsdr_ldpc_decode": (i32, [vp, vp, sz, vp, sz, vp, sz, vp]),
    "hzsdr_ldpc_sizes": (i32, [vp, psz, psz, psz, psz, psz, psz]),
    "hzsdr_ldpc_plan": (i32, [vp, psz, psz, psz, C.POINTER(i32)]),
    "hzsdr_ldpc_free": (i32, [vp]),
}
LDPC_MAX_ROWS, LDPC_MAX_CHECKS, LDPC_MAX_VARIABLES, LDPC_MAX_EDGES, LDPC_MAX_DEGREE, LDPC_MAX_BITS, LDPC_MAX_ITERS, LDPC_MAX_FRAMES = \
    8192, 16384, 16384, 65536, 64, 8192, 255, 1 << 22
LDPC_BITS, LDPC_SOFT_F32 = 1, 32
LDPC_FORM_TABLES_LDS, LDPC_FORM_TABLES_CACHE = 1, 2

# name -> (restype, argtypes); every symbol include/hzsdr_demap.h declares
DEMAP_SIGNATURES = {
    "hzsdr_demap_create": (i32, [vp, i32, C.c_uint, C.POINTER(f32), sz, C.POINTER(C.c_uint32), sz, C.POINTER(C.c_uint8), C.POINTER(f32), sz, sz, pvp]),
    "hzsdr_demap_run": (i32, [vp, vp, sz, vp, sz, vp, sz]),
    "hzsdr_demap_sizes": (i32, [vp, psz, psz, psz, psz]),
    "hzsdr_demap_plan": (i32, [vp, psz, psz, psz, C.POINTER(i32)]),
    "hzsdr_demap_free": (i32, [vp]),
}
DEMAP_MAX_ROWS, DEMAP_MAX_BITS, DEMAP_MAX_SYMBOLS, DEMAP_MAX_LLRS, DEMAP_MAX_OUT, DEMAP_MAX_FRAMES = 8192, 8, 8192, 16384, 8192, 1 << 22
DEMAP_ERASED = 0xFFFFFFFF
DEMAP_C64, DEMAP_REAL_F32, DEMAP_LLR_F32 = 1, 32, 33
DEMAP_FORM_GROUPED, DEMAP_FORM_PERM, DEMAP_FORM_TREE = 1, 2, 4

# name -> (restype, argtypes); every symbol include/hzsdr_rs.h declares
RS_SIGNATURES = {
    "hzsdr_rs_create": (i32, [vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, vp, vp, vp, sz, sz, pvp]),
    "hzsdr_rs_decode": (i32, [vp, vp, sz, sz, vp, sz, vp, sz, sz, vp]),
    "hzsdr_rs_sizes": (i32, [vp, psz, psz, psz, psz]),
    "hzsdr_rs_plan": (i32, [vp, psz, psz, psz, psz]),
    "hzsdr_rs_free": (i32, [vp]),
}
RS_MAX_ROWS, RS_MIN_ROOTS, RS_MAX_ROOTS, RS_MAX_N, RS_MAX_INTERLEAVE, RS_MAX_SCRAMBLE, RS_MAX_FRAMES = 8192, 2, 64, 255, 8, 2040, 1 << 22

# name -> (restype, argtypes); every symbol include/hzsdr_softframe.h declares
SOFTFRAME_SIGNATURES = {
    "hzsdr_softframe_create": (i32, [vp, i32, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_uint), sz, pvp]),
    "hzsdr_softframe_push": (i32, [vp, vp, sz, sz, vp, vp, vp, vp, sz, vp, sz, vp]),
    "hzsdr_softframe_get_state": (i32, [vp, C.POINTER(u64), C.POINTER(f32), sz]),
    "hzsdr_softframe_set_state": (i32, [vp, C.POINTER(u64), C.POINTER(f32), sz]),
    "hzsdr_softframe_positions": (i32, [vp, C.POINTER(u64), sz]),
    "hzsdr_softframe_plan": (i32, [vp, psz, psz, C.POINTER(i32)]),
    "hzsdr_softframe_reset": (i32, [vp]),
    "hzsdr_softframe_free": (i32, [vp]),
}
SOFTFRAME_MAX_ROWS, SOFTFRAME_MAX_PAYLOAD, SOFTFRAME_MAX_HYPOTHESES, SOFTFRAME_MAX_SLOTS = 8192, 8192, 4, 1 << 22
SOFTFRAME_SERVED, SOFTFRAME_OUTSIDE, SOFTFRAME_NO_HYPOTHESIS = 0, 1, 2
SOFTFRAME_FORM_COMPLEX, SOFTFRAME_FORM_DIBIT = 1, 2

for _name, (_res, _args) in (*SIGNATURES.items(), *SPECTRUM_SIGNATURES.items(), *CHANNELIZER_SIGNATURES.items(),
                             *SYNTHESIZER_SIGNATURES.items(), *RESAMPLER_SIGNATURES.items(), *DEMOD_SIGNATURES.items(), *TUNER_SIGNATURES.items(),
                             *CHANBANK_SIGNATURES.items(), *COVAR_SIGNATURES.items(), *IIR_SIGNATURES.items(), *SYMSYNC_SIGNATURES.items(),
                             *CARRIER_SIGNATURES.items(), *AGC_SIGNATURES.items(), *FRAMESYNC_SIGNATURES.items(), *VITERBI_SIGNATURES.items(),
                             *RS_SIGNATURES.items(), *SOFTFRAME_SIGNATURES.items(), *EQUALIZER_SIGNATURES.items(), *HDLC_SIGNATURES.items(),
                             *LDPC_SIGNATURES.items(), *DEMAP_SIGNATURES.items()):
    _fn = getattr(lib, _name)  # AttributeError here = header and library disagree
    _fn.restype = _res
    _fn.argtypes = _args
