"""ctypes loader for libt41rx.so, the C ABI declared in include/t41rx.h.

The library is the product: HIP kernels + C++ host side.  There is no Python or CPU
implementation of the path behind it; if the shared object is missing, loading fails loudly.

Both binding tables live here, SYMBOLS (include/t41rx.h, receive) and TX_SYMBOLS (include/t41tx.h, transmit), and
load() binds both: no entry point is ever called with ctypes' default conversions.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# override: a kernel build of tools/build_variant.sh.  A diagnostic build refuses t41rx_create() unless the environment
# says T41RX_ALLOW_EXPERIMENT=1 (rx_experiments.hpp, rx_host.cpp); the tools that use one set it themselves.
LIB_PATH = os.environ.get("T41RX_LIB", os.path.join(_HERE, "libt41rx.so"))

T41RX_OK = 0
ERR_ARG, ERR_UNSUPPORTED, ERR_HIP, ERR_NOMEM, ERR_STATE = -1, -2, -3, -4, -5
DEMOD_USB, DEMOD_LSB, DEMOD_AM, DEMOD_NFM = 0, 1, 2, 3
DEMOD_SAM = 8  # synchronous AM (SDT.h:67), fft_length 512
SSB_MODE, CW_MODE, DATA_MODE = 0, 1, 2
# the bits of a channel's mask in the stage map (T41RX_STAGE_*, t41rx_set_stage_map)
STAGE_EQ, STAGE_NR, STAGE_NB, STAGE_CW_DETECT, STAGE_CW_DECODE = 1, 2, 4, 8, 16
STAGE_ALL = 31
SETS_STAGES = 1  # T41RX_SETS_STAGES: parameter sets loaded next to the chain-splitting stages (t41rx_set_param_sets_ex)


class Params(C.Structure):
    """struct t41rx_params (include/t41rx.h)."""
    _fields_ = [
        ("fft_length", C.c_int32),
        ("mode", C.c_int32),
        ("FLoCut", C.c_int32),
        ("FHiCut", C.c_int32),
        ("rfGainAllBands", C.c_int32),
        ("RFgain", C.c_int32),
        ("IQAmpCorrectionFactor", C.c_float),
        ("IQPhaseCorrectionFactor", C.c_float),
        ("AGCMode", C.c_int32),
        ("audioVolume", C.c_int32),
        ("nfmFilterBW", C.c_int32),
        ("xmtMode", C.c_int32),
        ("CWFreqShift", C.c_int32),
        ("am_lpf_f0", C.c_int32),
        ("AGC_thresh", C.c_int32),
        ("nfm_demod", C.c_int32),
        ("nrOptionSelect", C.c_int32),
        ("ANR_notchOn", C.c_int32),
        ("NR_PSI", C.c_float),
        ("NR_alpha", C.c_float),
        ("NR_beta", C.c_float),
    ]


class PanadapterOut(C.Structure):
    """struct t41rx_panadapter_out (include/t41rx.h): device pointers of the panadapter's row buffers, each may be NULL."""
    _fields_ = [
        ("pixel", C.c_void_p),
        ("y_new", C.c_void_p),
        ("y_old", C.c_void_p),
        ("waterfall", C.c_void_p),
        ("spec", C.c_void_p),
        ("audio_spect", C.c_void_p),
        ("smeter", C.c_void_p),
    ]


class TxParams(C.Structure):
    """struct t41tx_params (include/t41tx.h)"""
    _fields_ = [("mode", C.c_int32), ("IQXAmpCorrectionFactor", C.c_float), ("IQXPhaseCorrectionFactor", C.c_float)]


# every symbol include/t41rx.h declares: (restype, argtypes)
_vp, _fp = C.c_void_p, C.POINTER(C.c_float)
SYMBOLS = {
    "t41rx_abi_version": (C.c_int, []),
    "t41rx_strerror": (C.c_char_p, [C.c_int]),
    "t41rx_last_error": (C.c_char_p, []),
    "t41rx_supported_fft_length": (C.c_int, [C.c_int]),
    "t41rx_default_params": (None, [C.POINTER(Params)]),
    "t41rx_coeff_blob_bytes": (C.c_size_t, [C.c_int]),
    "t41rx_design_coeffs": (C.c_int, [C.POINTER(Params), _vp, C.c_size_t]),
    "t41rx_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.POINTER(Params)]),
    "t41rx_destroy": (C.c_int, [_vp]),
    "t41rx_set_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "t41rx_get_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "t41rx_get_coeffs": (C.c_int, [_vp, _vp, C.c_size_t]),
    "t41rx_set_coeffs": (C.c_int, [_vp, _vp, C.c_size_t]),
    "t41rx_set_nco_freq": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int]),
    "t41rx_reset": (C.c_int, [_vp]),
    "t41rx_n_channels": (C.c_int, [_vp]),
    "t41rx_frame_len": (C.c_int, [_vp]),
    "t41rx_set_buffer_layout": (C.c_int, [_vp, C.c_int]),
    "t41rx_get_buffer_layout": (C.c_int, [_vp]),
    "t41rx_set_audio_rate": (C.c_int, [_vp, C.c_int]),
    "t41rx_get_audio_rate": (C.c_int, [_vp]),
    "t41rx_audio_frame_len": (C.c_int, [_vp]),
    "t41rx_set_input_map": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int, C.c_int]),
    "t41rx_get_input_map": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int]),
    "t41rx_set_output_map": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int, C.c_int]),
    "t41rx_get_output_map": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]),
    "t41rx_audio_rows": (C.c_int, [_vp]),
    "t41rx_set_stage_map": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.c_int]),
    "t41rx_get_stage_map": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.c_int]),
    "t41rx_set_param_sets": (C.c_int, [_vp, C.POINTER(Params), C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "t41rx_get_param_sets": (C.c_int, [_vp, C.POINTER(Params), C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "t41rx_param_sets_compatible": (C.c_int, [C.POINTER(Params), C.POINTER(Params)]),
    "t41rx_set_param_sets_ex": (C.c_int, [_vp, C.POINTER(Params), C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int32]),
    "t41rx_get_param_sets_flags": (C.c_int, [_vp]),
    "t41rx_param_sets_compatible_ex": (C.c_int, [C.POINTER(Params), C.POINTER(Params), C.c_int32]),
    "t41rx_process_device": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp]),
    "t41rx_process_host": (C.c_int, [_vp, _fp, _fp, _fp, C.c_int]),
    "t41rx_set_audio_spectrum": (C.c_int, [_vp, _vp, _vp, C.c_int]),
    "t41rx_process_device_q15": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp]),
    "t41rx_process_host_q15": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int]),
    "t41rx_state_bytes": (C.c_size_t, [_vp]),
    "t41rx_get_state": (C.c_int, [_vp, _vp, C.c_size_t]),
    "t41rx_set_state": (C.c_int, [_vp, _vp, C.c_size_t]),
    "t41rx_set_debug_taps": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int]),
    "t41rx_set_display_spectrum": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int]),
    "t41rx_set_noise_blanker": (C.c_int, [_vp, C.c_int]),
    "t41rx_get_noise_blanker": (C.c_int, [_vp]),
    "t41rx_set_receive_eq_bands": (C.c_int, [_vp, _vp]),
    "t41rx_set_receive_eq": (C.c_int, [_vp, C.c_int, _vp]),
    "t41rx_get_receive_eq": (C.c_int, [_vp, _vp]),
    "t41rx_set_receive_eq_map": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int]),
    "t41rx_get_receive_eq_map": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int]),
    "t41rx_set_cw_tables": (C.c_int, [_vp, _vp, _vp]),
    "t41rx_set_cw_filter": (C.c_int, [_vp, C.c_int]),
    "t41rx_get_cw_filter": (C.c_int, [_vp]),
    "t41rx_set_cw_filter_map": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int]),
    "t41rx_get_cw_filter_map": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int]),
    "t41rx_set_nr_map": (C.c_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]),
    "t41rx_get_nr_map": (C.c_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]),
    "t41rx_set_cw_detector": (C.c_int, [_vp, C.c_int, _vp, C.c_int]),
    "t41rx_get_cw_detector": (C.c_int, [_vp]),
    "t41rx_set_cw_decode_tree": (C.c_int, [_vp, _vp, C.c_int]),
    "t41rx_set_cw_decoder": (C.c_int, [_vp, C.c_int, _vp, C.c_int]),
    "t41rx_get_cw_decoder": (C.c_int, [_vp]),
    "t41rx_set_cw_clock": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32]),
    "t41rx_reset_cw_histograms": (C.c_int, [_vp, _vp, C.c_int]),
    "t41rx_set_calibration": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "t41rx_set_cal_corrections": (C.c_int, [_vp, _vp, _vp]),
    "t41rx_calibrate_device": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp]),
    "t41rx_calibrate_device_q15": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp]),
    "t41rx_calibrate_host": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int]),
    "t41rx_calibrate_host_q15": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int]),
    "t41rx_set_ft8_tables": (C.c_int, [_vp, _vp, _vp]),
    "t41rx_set_ft8": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int]),
    "t41rx_get_ft8": (C.c_int, [_vp]),
    "t41rx_set_ft8_map": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int, C.c_int]),
    "t41rx_get_ft8_map": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]),
    "t41rx_ft8_rows": (C.c_int, [_vp]),
    "t41rx_set_ft8_clock": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32]),
    "t41rx_ft8_sync": (C.c_int, [_vp, _vp, C.c_int]),
    "t41rx_ft8_state_bytes": (C.c_size_t, [_vp]),
    "t41rx_ft8_get_state": (C.c_int, [_vp, _vp, C.c_size_t]),
    "t41rx_ft8_set_state": (C.c_int, [_vp, _vp, C.c_size_t]),
    "t41rx_ft8_audio_device_q15": (C.c_int, [_vp, _vp, C.c_int]),
    "t41rx_ft8_audio_device": (C.c_int, [_vp, _vp, C.c_int]),
    "t41rx_ft8_audio_host_q15": (C.c_int, [_vp, _vp, C.c_int]),
    "t41rx_ft8_audio_host": (C.c_int, [_vp, _vp, C.c_int]),
    "t41rx_ft8_audio_begin": (C.c_int, [_vp, _vp, C.c_int]),
    "t41rx_ft8_audio_end": (C.c_int, [_vp, _vp, C.c_int]),
    "t41rx_set_ft8_decode_tables": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "t41rx_set_ft8_decode": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
    "t41rx_get_ft8_decode": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "t41rx_set_ft8_decode_debug": (C.c_int, [_vp, _vp, _vp]),
    "t41rx_ft8_decode_device": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_int, _vp, _vp]),
    "t41rx_ft8_decode_host": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_int, _vp]),
    "t41rx_set_panadapter_tables": (C.c_int, [_vp, C.POINTER(C.c_uint16), C.c_int]),
    "t41rx_set_panadapter": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PanadapterOut), C.c_int]),
    "t41rx_set_panadapter_levels": (C.c_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int]),
    "t41rx_get_panadapter": (C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "t41rx_set_panadapter_counter": (C.c_int, [_vp, C.c_int64]),
    "t41rx_set_panadapter_map": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int, C.c_int]),
    "t41rx_get_panadapter_map": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]),
    "t41rx_panadapter_rows": (C.c_int, [_vp]),
    "t41rx_set_beacon": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int32), _vp, _vp, C.c_int]),
    "t41rx_set_beacon_clock": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32]),
    "t41rx_get_beacon": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "t41rx_beacon_state_bytes": (C.c_size_t, [_vp]),
    "t41rx_beacon_get_state": (C.c_int, [_vp, _vp, C.c_size_t]),
    "t41rx_beacon_set_state": (C.c_int, [_vp, _vp, C.c_size_t]),
}

# every symbol include/t41tx.h declares
TX_SYMBOLS = {
    "t41tx_default_params": (None, [C.POINTER(TxParams)]),
    "t41tx_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.POINTER(TxParams)]),
    "t41tx_destroy": (C.c_int, [_vp]),
    "t41tx_set_params": (C.c_int, [_vp, C.POINTER(TxParams)]),
    "t41tx_reset": (C.c_int, [_vp]),
    "t41tx_n_channels": (C.c_int, [_vp]),
    "t41tx_process_device_q15": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, _vp]),
    "t41tx_process_host_q15": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int]),
    "t41tx_set_transmit_eq_bands": (C.c_int, [_vp, _vp]),
    "t41tx_set_transmit_eq": (C.c_int, [_vp, C.c_int, _vp]),
    "t41tx_get_transmit_eq": (C.c_int, [_vp, _vp]),
    "t41tx_state_bytes": (C.c_size_t, [_vp]),
    "t41tx_get_state": (C.c_int, [_vp, _vp, C.c_size_t]),
    "t41tx_set_state": (C.c_int, [_vp, _vp, C.c_size_t]),
    "t41tx_set_cw_tone": (C.c_int, [_vp, _vp, _vp]),
    "t41tx_process_cw_device_q15": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp]),
    "t41tx_process_cw_host_q15": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int]),
    "t41tx_set_cal_tone": (C.c_int, [_vp, _vp, _vp, C.c_float]),
    "t41tx_set_cal_corrections": (C.c_int, [_vp, _vp, _vp]),
    "t41tx_process_cal_device_q15": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp]),
    "t41tx_process_cal_host_q15": (C.c_int, [_vp, _vp, _vp, C.c_int]),
}

_lib = None


class T41RxError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        super().__init__("t41rx status %d%s" % (status, (": " + detail) if detail else ""))


def load():
    """Load libt41rx.so and bind every declared symbol (raises if the build is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s not found: build it with `make -C t41_sdr_amd/csrc` (or __graft_entry__.build()). "
            "There is no CPU fallback for the RX path." % LIB_PATH)
    # PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).
    # Import it first so this library binds to the SAME runtime instance that owns torch's
    # device memory and streams; two runtimes in one process do not see each other's state.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in {**SYMBOLS, **TX_SYMBOLS}.items():
        fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status):
    if status != T41RX_OK:
        lib = load()
        detail = lib.t41rx_last_error().decode("utf-8", "replace")
        if not detail:
            detail = lib.t41rx_strerror(status).decode()
        raise T41RxError(status, detail)
