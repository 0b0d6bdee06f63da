"""The Python layer's own argument checks, without a GPU: every refusal rx.py / tx.py make before they call the library,
with its exception type and exact text, and for every setter one valid argument set, which a null context makes the C
side refuse with T41RX_ERR_ARG -- so the Python checks let it through and the call arrived with the table's arity.
The objects are made with __new__ (no context is created), as test_python_mirrors_keep_their_params_when_refused does."""
import ctypes as C

import numpy as np
import pytest

N = 3  # n_channels of both objects
PAN = "pixel, y_new, y_old, waterfall, spec, audio_spect, smeter"


@pytest.fixture
def T(built):
    import t41_sdr_amd
    return t41_sdr_amd


@pytest.fixture
def rx(T):
    from t41_sdr_amd import _lib
    r = T.RxChain.__new__(T.RxChain)
    r._lib, r._ctx, r.params = _lib.load(), C.c_void_p(), T.default_params()
    r.n_channels, r.device, r.frame_len, r.layout, r._n_streams = N, 0, 2048, "channel", 0
    return r


@pytest.fixture
def tx(T):
    from t41_sdr_amd import tx as txm
    t = T.TxChain.__new__(T.TxChain)
    t._lib, t._ctx, t.params = txm._load(), C.c_void_p(), T.default_tx_params()
    t.n_channels, t.device = N, 0
    return t


def refused(exc, message, call, *a, **kw):
    with pytest.raises(exc) as e:
        call(*a, **kw)
    assert type(e.value) is exc and str(e.value) == message, (str(e.value), message)


def reaches_the_library(T, call, *a, **kw):
    """a valid argument set: the null context is all that is wrong with the call"""
    from t41_sdr_amd import _lib
    with pytest.raises(T.T41RxError) as e:
        call(*a, **kw)
    assert e.value.status == _lib.ERR_ARG, str(e.value)


def z(*shape, dtype=np.float32):
    return np.zeros(shape, dtype)


# ------------------------------------------------------------------------------------------ parameters
def test_unknown_parameter_fields(T, rx, tx):
    refused(AttributeError, "t41rx_params has no field 'nope'", T.default_params, nope=1)
    refused(AttributeError, "t41rx_params has no field 'nope'", T.default_params, mode=1, nope=1)
    refused(AttributeError, "t41tx_params has no field 'nope'", T.default_tx_params, nope=1)
    before = bytes(rx.params), bytes(tx.params)
    refused(AttributeError, "t41rx_params has no field 'nope'", rx.CalcFilters, FLoCut=300, nope=1)
    refused(AttributeError, "t41rx_params has no field 'nope'", rx.SetupMode, nope=1)
    refused(AttributeError, "t41tx_params has no field 'nope'", tx.set_params, mode=1, nope=1)
    reaches_the_library(T, rx.CalcFilters, FLoCut=300)
    reaches_the_library(T, tx.set_params, mode=1)
    assert (bytes(rx.params), bytes(tx.params)) == before
    assert T.default_params(FLoCut=300).FLoCut == 300 and T.default_tx_params(mode=1).mode == 1


def test_objects_with_only_lib_ctx_and_params_change_their_parameters(T):
    from t41_sdr_amd import tx as txm
    r, t = T.RxChain.__new__(T.RxChain), T.TxChain.__new__(T.TxChain)
    r._lib, r._ctx, r.params = txm._load(), C.c_void_p(), T.default_params()
    t._lib, t._ctx, t.params = txm._load(), C.c_void_p(), T.default_tx_params()
    reaches_the_library(T, r.CalcFilters, audioVolume=10)
    reaches_the_library(T, t.set_params, IQXAmpCorrectionFactor=0.5)
    refused(AttributeError, "t41rx_params has no field 'nope'", r.CalcFilters, nope=1)
    refused(AttributeError, "t41tx_params has no field 'nope'", t.set_params, nope=1)
    for obj in (r, t):  # and they are collected without a complaint
        obj.close()
        obj.close()


# ------------------------------------------------------------------------------------------ RX tables
def test_rx_table_setters(T, rx):
    refused(ValueError, "receive-EQ band table must be [14][4][5] or [14][20], got (14, 19)", rx.set_receive_eq_bands, z(14, 19))
    refused(ValueError, "receive-EQ band table must be [14][4][5] or [14][20], got (20, 14)", rx.set_receive_eq_bands, z(20, 14))
    refused(ValueError, "receive-EQ band table must be [14][4][5] or [14][20], got (1,)", rx.set_receive_eq_bands, 1.0)
    reaches_the_library(T, rx.set_receive_eq_bands, z(14, 4, 5))
    reaches_the_library(T, rx.set_receive_eq_bands, z(14, 20, dtype=np.float64))
    refused(ValueError, "receive-EQ levels must be 14 ints, got (13,)", rx.set_receive_eq, 1, [100] * 13)
    refused(ValueError, "receive-EQ levels must be 14 ints, got (2, 7)", rx.set_receive_eq, 1, z(2, 7))
    reaches_the_library(T, rx.set_receive_eq, 1, [100] * 14)
    reaches_the_library(T, rx.set_receive_eq, 0)

    refused(ValueError, "CW filter tables must be [5][6][5] or [5][30], got (5, 29)", rx.set_cw_tables, z(5, 29))
    refused(ValueError, "CW filter tables must be [5][6][5] or [5][30], got (6, 25)", rx.set_cw_tables, z(6, 25))
    refused(ValueError, "CW decode FIR must be 64 taps, got (63,)", rx.set_cw_tables, None, z(63))
    refused(ValueError, "CW filter tables must be [5][6][5] or [5][30], got (150,)", rx.set_cw_tables, z(150), z(63))  # the first wins
    reaches_the_library(T, rx.set_cw_tables, z(5, 6, 5), z(64))
    reaches_the_library(T, rx.set_cw_tables, z(5, 30))
    reaches_the_library(T, rx.set_cw_tables, None, z(64))
    reaches_the_library(T, rx.set_cw_tables)

    both = "window and mag_db must both be given or both be None"
    refused(ValueError, both, rx.set_ft8_tables, z(2048))
    refused(ValueError, both, rx.set_ft8_tables, None, z(16385))
    refused(ValueError, both, rx.set_ft8_tables, z(7), None)  # before any shape
    refused(ValueError, "FT8 tables must be 2048 and 16385 floats, got (2047,) and (16385,)", rx.set_ft8_tables, z(2047), z(16385))
    refused(ValueError, "FT8 tables must be 2048 and 16385 floats, got (2048,) and (1, 16385)", rx.set_ft8_tables, z(2048), z(1, 16385))
    reaches_the_library(T, rx.set_ft8_tables, z(2048), z(16385))
    reaches_the_library(T, rx.set_ft8_tables)

    reaches_the_library(T, rx.set_cw_decode_tree, bytes(129))
    reaches_the_library(T, rx.set_cw_decode_tree, "A" * 129)
    reaches_the_library(T, rx.set_cw_decode_tree, z(129, dtype=np.uint8))


def test_cal_corrections_of_both_chains(T, rx, tx):
    for c in (rx, tx):
        both = "amp and phase must both be given or both be None"
        refused(ValueError, both, c.set_cal_corrections, [1.0] * N)
        refused(ValueError, both, c.set_cal_corrections, None, [0.0] * N)
        refused(ValueError, both, c.set_cal_corrections, z(7), None)  # before any shape
        refused(ValueError, "corrections must be 3 floats each, got (3,) and (2,)", c.set_cal_corrections, z(3), z(2))
        refused(ValueError, "corrections must be 3 floats each, got (1, 3) and (3,)", c.set_cal_corrections, z(1, 3), z(3))
        reaches_the_library(T, c.set_cal_corrections, [1.0] * N, z(N, dtype=np.float64))
        reaches_the_library(T, c.set_cal_corrections)


def test_input_map_arguments(T, rx):
    head = "stream_of_channel must be a 1-d array of int32 stream numbers, got "
    refused(ValueError, head + "(3, 1) int64", rx.set_input_map, z(3, 1, dtype=np.int64))
    refused(ValueError, head + "(3,) float64", rx.set_input_map, [0.0, 1.0, 0.0])
    refused(ValueError, head + "(3,) int64", rx.set_input_map, [0, 2**31, 0])
    refused(ValueError, head + "(3,) int64", rx.set_input_map, [0, -2**31 - 1, 0])
    rx._n_streams = 2
    reaches_the_library(T, rx.set_input_map, [0, 1, 0])
    reaches_the_library(T, rx.set_input_map, np.array([0, 1, 0], np.uint8), 4)
    refused(ValueError, head + "(0,) float64", rx.set_input_map, [])
    reaches_the_library(T, rx.set_input_map, z(0, dtype=np.int32))
    reaches_the_library(T, rx.set_input_map, None)
    assert rx._n_streams == 2 and rx.n_streams == 2  # a refused map leaves the count
    rx._n_streams = 0
    assert rx.n_streams == N


def test_panadapter_arguments(T, rx):
    head = "gradient must be a 1-d array of uint16 colour words, got "
    refused(ValueError, head + "(117,) float64", rx.set_panadapter_tables, z(117, dtype=np.float64))
    refused(ValueError, head + "(2,) int64", rx.set_panadapter_tables, [0, 0x10000])
    refused(ValueError, head + "(2,) int64", rx.set_panadapter_tables, [-1, 5])
    refused(ValueError, head + "(1, 117) uint16", rx.set_panadapter_tables, z(1, 117, dtype=np.uint16))
    reaches_the_library(T, rx.set_panadapter_tables, np.arange(117))
    refused(ValueError, head + "(0,) float64", rx.set_panadapter_tables, [])
    reaches_the_library(T, rx.set_panadapter_tables, z(0, dtype=np.int64))

    nf = "noise_floor must be n_channels = 3 int32 values, got "
    refused(ValueError, nf + "(2,) int64", rx.set_panadapter_levels, [1, 2])
    refused(ValueError, nf + "(3,) float64", rx.set_panadapter_levels, [1.0, 2.0, 3.0])
    refused(ValueError, nf + "(3,) int64", rx.set_panadapter_levels, [0, 2**31, 0])
    refused(ValueError, "gain_correction must be n_channels = 3 floats, got (2,)", rx.set_panadapter_levels, None, [1.0, 2.0])
    refused(ValueError, nf + "(2,) int64", rx.set_panadapter_levels, [1, 2], [1.0, 2.0])  # the first wins
    reaches_the_library(T, rx.set_panadapter_levels, [1, 2, 3], [0.5, 0.5, 0.5], 10)
    reaches_the_library(T, rx.set_panadapter_levels, None, [1, 2, 3])
    reaches_the_library(T, rx.set_panadapter_levels)

    refused(ValueError, "max_rows must be >= 1", rx.set_panadapter, max_rows=0)
    refused(ValueError, "unknown panadapter output 'nope' (one of %s)" % PAN, rx.set_panadapter, outputs=["nope"])
    refused(ValueError, "unknown panadapter output 'nope' (one of %s)" % PAN, rx.set_panadapter, outputs={"nope": None})
    rx._pan = keep = {"pixel": object()}
    reaches_the_library(T, rx.set_panadapter, False)
    assert rx._pan is keep  # a refused switch-off leaves the buffers
    reaches_the_library(T, rx.set_panadapter_counter, 5)
    reaches_the_library(T, rx.panadapter_status)
    assert [r[0] for r in T.RxChain.PANADAPTER_ROWS] == PAN.split(", ")


def test_ft8_decode_arguments(T, rx):
    import torch
    good = dict(costas=z(7, dtype=np.int64), gray=np.arange(8), nm=z(83, 7, dtype=np.uint8), mn=z(174, 3, dtype=np.int32), nrw=[7] * 83)
    refused(ValueError, "costas must have shape (7,), got (6,)", rx.set_ft8_decode_tables, **dict(good, costas=z(6, dtype=np.int64)))
    refused(ValueError, "nm must have shape (83, 7), got (7, 83)", rx.set_ft8_decode_tables, **dict(good, nm=z(7, 83, dtype=np.uint8)))
    refused(ValueError, "mn must have shape (174, 3), got (174,)", rx.set_ft8_decode_tables, **dict(good, mn=z(174, dtype=np.uint8)))
    refused(ValueError, "gray does not fit uint8", rx.set_ft8_decode_tables, **dict(good, gray=np.arange(8) + 249))
    refused(ValueError, "nrw does not fit uint8", rx.set_ft8_decode_tables, **dict(good, nrw=[-1] * 83))
    refused(ValueError, "gray must have shape (8,), got (9,)", rx.set_ft8_decode_tables,
            **dict(good, gray=np.arange(9), nrw=[-1] * 83))  # in the order of the arguments
    reaches_the_library(T, rx.set_ft8_decode_tables, **good)
    reaches_the_library(T, rx.set_ft8_decode)
    reaches_the_library(T, rx.set_ft8_decode, 5, 30, 20)
    with pytest.raises(T.T41RxError):
        rx.ft8_decode_params

    refused(ValueError, "select must have n_channels = 3 entries, got (2,)", rx.ft8_decode, [0, 1])
    refused(ValueError, "select does not fit int8", rx.ft8_decode, [0, 1, 128])
    wf = "waterfall must be a uint8 CUDA tensor [n_channels, bytes per channel] with unit inner stride"
    refused(ValueError, wf, rx.ft8_decode, None, torch.zeros(N, 92 * 1472, dtype=torch.uint8))
    refused(ValueError, wf, rx.ft8_decode, [0, 0, 0], z(N, 92 * 1472, dtype=np.uint8))


# ------------------------------------------------------------------------------------------ channel masks
def test_channel_masks(T, rx):
    for call in (rx.reset_cw_histograms, rx.ft8_sync, rx.ft8_audio_begin, rx.ft8_audio_end):
        refused(ValueError, "channels must have n_channels = 3 entries, got (2,)", call, [1, 0])
        refused(ValueError, "channels must have n_channels = 3 entries, got (1, 3)", call, [[1, 0, 1]])
        refused(ValueError, "channels must have n_channels = 3 entries, got (1,)", call, 1)
        reaches_the_library(T, call, [1, 0, 5])
        reaches_the_library(T, call, np.array([0.0, 0.5, 0.0]))
        reaches_the_library(T, call)


# ------------------------------------------------------------------------------------------ switches and getters
def test_rx_switches_getters_and_blobs(T, rx):
    for call, args in ((rx.set_noise_blanker, (1,)), (rx.set_cw_filter, (2,)), (rx.set_cw_clock, ()), (rx.set_cw_clock, (5, 64, 3)),
                       (rx.set_ft8_clock, ()), (rx.set_ft8_clock, (5, 64, 3)), (rx.set_calibration, ()),
                       (rx.set_calibration, (True, 1, 2, 3) + T.RxChain.CAL_BINS["tx", T.DEMOD_USB] + (8,)), (rx.SetNCOFreq, (1000,)),
                       (rx.SetNCOFreq, ([1000, 2000, 3000],)), (rx.reset, ()), (rx.get_params, ()), (rx.coeffs, ()), (rx.get_state, ()),
                       (rx.ft8_state, ()), (rx.set_coeffs, (z(64, dtype=np.uint8),)), (rx.set_state, (z(64, dtype=np.uint8),)),
                       (rx.set_ft8_state, (bytearray(64),)), (rx.state_records, ())):
        reaches_the_library(T, call, *args)
    for name in ("input_map", "noise_blanker", "receive_eq", "cw_filter", "cw_detector", "cw_decoder", "ft8"):
        with pytest.raises(T.T41RxError) as e:
            getattr(rx, name)
        assert e.value.status == -1, name
    assert rx.layout == "channel"
    reaches_the_library(T, rx.set_buffer_layout, "time")
    assert rx.layout == "channel"
    with pytest.raises(KeyError):
        rx.set_buffer_layout("frames")
    assert T.RxChain.CAL_BINS == {("rx", T.DEMOD_LSB): (310, 460), ("rx", T.DEMOD_USB): (65, 192),
                                  ("tx", T.DEMOD_LSB): (240, 305), ("tx", T.DEMOD_USB): (209, 273)}


def test_result_tensor_stages(T, rx):
    readers = ((rx.cw_results, "the CW detector is off", "_cw"), (rx.cw_text, "the CW decoder is off", "_cw_text"),
               (rx.ft8_status, "FT8 receive is off", "_ft8"))
    for reader, message, attr in readers:  # the keep-alive attribute was never set
        assert not hasattr(rx, attr)
        refused(ValueError, message, reader, 1)
    refused(ValueError, "FT8 receive is off", rx.ft8_power)
    for switch, (reader, message, attr) in zip((rx.set_cw_detector, rx.set_cw_decoder, rx.set_ft8), readers):
        refused(ValueError, "max_frames must be >= 1", switch, 1, 0)
        refused(ValueError, "max_frames must be >= 1", switch, True, max_frames=-3)
        setattr(rx, attr, "kept")
        reaches_the_library(T, switch, 0)
        assert getattr(rx, attr) == "kept"  # a refused switch-off leaves the tensor
        setattr(rx, attr, None)
        refused(ValueError, message, reader, 1)
    refused(ValueError, "FT8 receive is off", rx.ft8_power)


def test_result_views_are_the_first_frames(T, rx):
    """the views of the first n_frames, on CPU tensors standing in for the stages' CUDA ones"""
    import torch
    rx._cw = torch.arange(N * 5 * 4, dtype=torch.float32).view(N, 5, 4)
    rx._cw_text = torch.arange(N * 5 * 2, dtype=torch.int32).view(N, 5, 2)
    rx._ft8 = (torch.zeros(N, 2, 8, dtype=torch.uint8), torch.arange(N * 5 * 4, dtype=torch.int32).view(N, 5, 4))
    for view, src, w in ((rx.cw_results(2), rx._cw, 4), (rx.cw_text(2), rx._cw_text, 2), (rx.ft8_status(2), rx._ft8[1], 4)):
        assert tuple(view.shape) == (N, 2, w) and view.data_ptr() == src.data_ptr()
        assert torch.equal(view.reshape(-1), src.reshape(-1)[:N * 2 * w])
    assert rx.ft8_power() is rx._ft8[0]
    assert rx.cw_results(5).data_ptr() == rx._cw.data_ptr() and torch.equal(rx.cw_results(5), rx._cw)


# ------------------------------------------------------------------------------------------ the process calls
def test_check_shape(T, rx):
    L = 2048
    tail = " (n_channels=3, n_streams=3), got "
    assert rx._check_shape((3, L), (3, L)) == 1 and rx._check_shape((3, 5 * L), (3, 5 * L)) == 5
    for si, sq in (((2, L), (2, L)), ((3, L), (3, 2 * L)), ((3, L + 1), (3, L + 1)), ((3, 0), (3, 0)), ((3 * L,), (3 * L,)), ((1, 3, L), (1, 3, L))):
        refused(ValueError, "I/Q must be [3, k*frame_len=2048]" + tail + "%r / %r" % (si, sq), rx._check_shape, si, sq)
    rx._n_streams = 2
    assert rx._check_shape((2, L), (2, L)) == 1 and rx._out_shape(4) == (3, 4 * L)
    refused(ValueError, "I/Q must be [2, k*frame_len=2048] (n_channels=3, n_streams=2), got (3, 2048) / (3, 2048)", rx._check_shape, (3, L), (3, L))
    rx.layout = "time"
    assert rx._check_shape((4, 2, L), (4, 2, L)) == 4 and rx._out_shape(4) == (4, 3, L)
    refused(ValueError, "time-major I/Q must be [n_frames, 2, frame_len=2048] (n_channels=3, n_streams=2), got (4, 3, 2048) / (4, 3, 2048)",
            rx._check_shape, (4, 3, L), (4, 3, L))
    rx._n_streams = 0
    for si, sq in (((3, L), (3, L)), ((0, 3, L), (0, 3, L)), ((1, 3, L), (2, 3, L)), ((1, 3, L - 1), (1, 3, L - 1))):
        refused(ValueError, "time-major I/Q must be [n_frames, 3, frame_len=2048]" + tail + "%r / %r" % (si, sq), rx._check_shape, si, sq)


def test_check_out(T, rx):
    import torch
    L = 2048
    like = z(3, L)
    msg = "out must be a writeable C-contiguous float32 array of shape (3, 2048) (n_channels=3, n_streams=3)"
    ro = z(3, L)
    ro.flags.writeable = False
    for out in (z(2, L), z(3, L, dtype=np.float64), z(L, 3).T, ro, [0.0], torch.zeros(3, L)):
        refused(ValueError, msg, rx._check_out_numpy, out, like, 1)
    good = z(3, L)
    assert rx._check_out_numpy(good, like, 1) is good
    refused(ValueError, "out must be a writeable C-contiguous int16 array of shape (3, 4096) (n_channels=3, n_streams=3)",
            rx._check_out_numpy, good, z(3, L, dtype=np.int16), 2)
    rx._n_streams = 2
    refused(ValueError, "out must be a writeable C-contiguous float32 array of shape (3, 2048) (n_channels=3, n_streams=2)",
            rx.ProcessIQData, z(2, L), z(2, L), out=z(2, L))  # out= of the input's shape instead of the output's
    refused(ValueError, "out must be a writeable C-contiguous int16 array of shape (3, 2048) (n_channels=3, n_streams=2)",
            rx.ProcessIQData_q15, z(2, L, dtype=np.int16), z(2, L, dtype=np.int16), out=z(3, L))
    t = torch.zeros(2, L)
    refused(ValueError, "out must be a contiguous torch.float32 CUDA tensor of shape (3, 2048) on cpu (n_channels=3, n_streams=2)",
            rx._check_out_torch, torch.zeros(3, L), t, 1)
    rx.layout = "time"
    refused(ValueError, "out must be a writeable C-contiguous float32 array of shape (2, 3, 2048) (n_channels=3, n_streams=2)",
            rx.ProcessIQData, z(2, 2, L), z(2, 2, L), out=z(2, 2, L))


def test_process_calls(T, rx):
    import torch
    L = 2048
    # numpy: converted to the entry's type, checked, and handed to the host entries
    reaches_the_library(T, rx.ProcessIQData, z(3, L), z(3, L))
    reaches_the_library(T, rx.ProcessIQData, z(3, 2 * L, dtype=np.float64), z(3, 2 * L, dtype=np.int16), out=z(3, 2 * L))
    reaches_the_library(T, rx.ProcessIQData_q15, z(3, L, dtype=np.int16), z(3, L, dtype=np.int16))
    reaches_the_library(T, rx.ProcessIQData_q15, z(3, L, dtype=np.int32), z(3, L, dtype=np.int64), out=z(3, L, dtype=np.int16))
    refused(ValueError, "I/Q must be [3, k*frame_len=2048] (n_channels=3, n_streams=3), got (2, 2048) / (2, 2048)",
            rx.ProcessIQData, z(2, L), z(2, L))
    refused(ValueError, "I/Q must be [3, k*frame_len=2048] (n_channels=3, n_streams=3), got (3, 2048) / (3, 4096)",
            rx.ProcessIQData_q15, z(3, L, dtype=np.int16), z(3, 2 * L, dtype=np.int16))
    # CPU tensors are no CUDA tensors
    f, h = torch.zeros(3, L), torch.zeros(3, L, dtype=torch.int16)
    refused(ValueError, "I/Q must be contiguous float32 CUDA tensors", rx.ProcessIQData, f, f)
    refused(ValueError, "Q_in_L/Q_in_R must be contiguous int16 CUDA tensors", rx.ProcessIQData_q15, h, h)
    for i, q in ((f, f), (h, h)):
        refused(ValueError, "I/Q must be contiguous float32 or int16 CUDA tensors on device 0", rx.ProcessIQData2_rx, i, q)
    for name in ("post_nco", "dec", "demod"):
        refused(ValueError, "%s must be a contiguous float32 CUDA tensor on device 0" % name, rx.set_debug_taps, **{name: f})
    refused(ValueError, "spect must be a contiguous float32 CUDA tensor on device 0", rx.set_audio_spectrum, f, f)
    refused(ValueError, "maxima must be a contiguous float32 CUDA tensor on device 0", rx.set_audio_spectrum, None, f)
    refused(ValueError, "spec_old must be a contiguous float32 CUDA tensor on device 0", rx.set_display_spectrum, None, f)
    for call in (rx.set_debug_taps, rx.set_audio_spectrum, rx.set_display_spectrum):
        reaches_the_library(T, call)
    assert not hasattr(rx, "_taps") and not hasattr(rx, "_spect") and not hasattr(rx, "_disp")


def test_ft8_audio(T, rx):
    import torch
    refused(ValueError, "pcm must be int16 or float32, got float64", rx.ft8_audio, z(3, 128, dtype=np.float64))
    refused(ValueError, "pcm must be int16 or float32, got int32", rx.ft8_audio, z(3, 100, dtype=np.int32))
    for shape in ((3, 100), (2, 128), (3, 0), (3 * 128,), (3, 192)):
        refused(ValueError, "pcm must be [n_channels = 3, 128 * k], got %r" % (shape,), rx.ft8_audio, z(*shape, dtype=np.int16))
    refused(ValueError, "FT8 receive is off", rx.ft8_audio, z(3, 128, dtype=np.int16))
    refused(ValueError, "FT8 receive is off", rx.ft8_audio, z(3, 256))
    refused(ValueError, "pcm must be [n_channels = 3, 128 * k], got (3, 100)", rx.ft8_audio, z(3, 100))  # the shape before the switch
    tensor = "pcm must be a contiguous int16 or float32 CUDA tensor or numpy array"
    refused(ValueError, tensor, rx.ft8_audio, torch.zeros(3, 128, dtype=torch.int16))
    refused(ValueError, tensor, rx.ft8_audio, torch.zeros(3, 100))
    refused(ValueError, tensor, rx.ft8_audio, [[0] * 128] * 3)
    rx._ft8 = (None, None)
    reaches_the_library(T, rx.ft8_audio, z(3, 128, dtype=np.int16))
    reaches_the_library(T, rx.ft8_audio, z(3, 256))


def test_calibration_receive_call(T, rx):
    L = 2048
    refused(ValueError, "I/Q must be [3, k*2048], got (2, 2048) / (2, 2048)", rx.ProcessIQData2_rx, z(2, L), z(2, L))
    refused(ValueError, "I/Q must be [3, k*2048], got (3, 2048) / (3, 4096)", rx.ProcessIQData2_rx, z(3, L), z(3, 2 * L))
    refused(ValueError, "I/Q must be [1, k*2048], got (3, 2048) / (3, 2048)", rx.ProcessIQData2_rx, z(3, L), z(3, L), shared_input=True)
    refused(ValueError, "I/Q must be [1, k*2048], got (100,) / (100,)", rx.ProcessIQData2_rx, z(100), z(100), shared_input=True)
    refused(ValueError, "I/Q must be [3, k*2048], got (2048,) / (2048,)", rx.ProcessIQData2_rx, z(L), z(L))
    refused(ValueError, "update must hold n_frames=2 flags, got (3,)", rx.ProcessIQData2_rx, z(3, 2 * L), z(3, 2 * L), update=[1, 0, 1])
    refused(ValueError, "pixel must be a contiguous int16 buffer of shape (3, 1, 512) next to I/Q",
            rx.ProcessIQData2_rx, z(3, L), z(3, L), pixel=z(3, 1, 511, dtype=np.int16))
    refused(ValueError, "pixel must be a contiguous int16 buffer of shape (3, 1, 512) next to I/Q",
            rx.ProcessIQData2_rx, z(3, L), z(3, L), pixel=z(3, 1, 512), spec=z(3, 1, 511))  # the first wins
    refused(ValueError, "spec must be a contiguous float32 buffer of shape (3, 2, 512) next to I/Q",
            rx.ProcessIQData2_rx, z(3, 2 * L), z(3, 2 * L), pixel=True, spec=z(3, 2, 512, dtype=np.float64))
    refused(ValueError, "spec must be a contiguous float32 buffer of shape (3, 1, 512) next to I/Q",
            rx.ProcessIQData2_rx, z(3, L), z(3, L), update=[1, 0, 1], spec=z(3, 512))  # the side buffers before the flags
    reaches_the_library(T, rx.ProcessIQData2_rx, z(3, L), z(3, L))
    reaches_the_library(T, rx.ProcessIQData2_rx, z(2 * L, dtype=np.int16), z(2 * L, dtype=np.int16), update=[1, 0], shared_input=True,
                        pixel=True, spec=z(3, 2, 512))
    reaches_the_library(T, rx.ProcessIQData2_rx, z(3, L, dtype=np.float64), z(3, L, dtype=np.int16), pixel=z(3, 1, 512, dtype=np.int16))
    assert not hasattr(rx, "_cal_keep")


# ------------------------------------------------------------------------------------------ the transmit side
def test_tx_table_setters(T, tx):
    refused(ValueError, "transmit-EQ band table must be [14][4][5] or [14][20], got (14, 19)", tx.set_transmit_eq_bands, z(14, 19))
    refused(ValueError, "transmit-EQ band table must be [14][4][5] or [14][20], got (20, 14)", tx.set_transmit_eq_bands, z(20, 14))
    reaches_the_library(T, tx.set_transmit_eq_bands, z(14, 4, 5))
    refused(ValueError, "transmit-EQ levels must be 14 ints, got (15,)", tx.set_transmit_eq, 1, [100] * 15)
    reaches_the_library(T, tx.set_transmit_eq, 1, [100] * 14)
    reaches_the_library(T, tx.set_transmit_eq, 0)
    reaches_the_library(T, tx.get_transmit_eq)
    refused(ValueError, "CW tone tables must be 256 floats each, got (255,) and (256,)", tx.set_cw_tone, z(255), z(256))
    refused(ValueError, "CW tone tables must be 256 floats each, got (256,) and (2, 128)", tx.set_cw_tone, z(256), z(2, 128))
    reaches_the_library(T, tx.set_cw_tone, *T.sine_tone(8))
    refused(ValueError, "calibration tone tables must be 256 floats each, got (255,) and (256,)", tx.set_cal_tone, z(255), z(256), 0.5)
    refused(ValueError, "calibration tone tables must be 256 floats each, got (256,) and (257,)", tx.set_cal_tone, z(256), z(257), 0.5)
    reaches_the_library(T, tx.set_cal_tone, *T.cal_tone(), level=0.5)
    for call, args in ((tx.reset, ()), (tx.get_state, ()), (tx.set_state, (z(64, dtype=np.uint8),))):
        reaches_the_library(T, call, *args)


def test_tx_process_calls(T, tx):
    import torch
    F = T.TxChain.FRAME
    assert (F, T.TxChain.KEY_PER_FRAME) == (2048, 16)
    assert tx._frames((3, F)) == 1 and tx._frames((3, 4 * F)) == 4
    for shape in ((2, F), (3, 0), (3, F + 1), (3 * F,), (1, 3, F)):
        refused(ValueError, "samples must be [n_channels=3, k*2048], got %r" % (shape,), tx._frames, shape)
    refused(ValueError, "samples must be [n_channels=3, k*2048], got (2, 2048)", tx.ExciterIQData, z(2, F, dtype=np.int16))
    reaches_the_library(T, tx.ExciterIQData, z(3, F, dtype=np.int16))
    reaches_the_library(T, tx.ExciterIQData, z(3, F, dtype=np.float64))  # converted
    refused(ValueError, "Q_in_L_Ex must be a contiguous int16 CUDA tensor on device 0", tx.ExciterIQData, torch.zeros(3, F, dtype=torch.int16))

    refused(ValueError, "key must be [n_channels=3, n_frames*16=32], got (3, 16)", tx.CW_ExciterIQData, 2, z(3, 16, dtype=np.uint8))
    refused(ValueError, "key must be [n_channels=3, n_frames*16=16], got (16,)", tx.CW_ExciterIQData, 1, z(16, dtype=np.float64))
    refused(ValueError, "key must be a numpy array or a contiguous uint8 CUDA tensor on device 0",
            tx.CW_ExciterIQData, 1, torch.zeros(3, 16, dtype=torch.uint8))
    refused(ValueError, "key must be a numpy array or a contiguous uint8 CUDA tensor on device 0", tx.CW_ExciterIQData, 1, [[1] * 16] * 3)
    reaches_the_library(T, tx.CW_ExciterIQData, 2, z(3, 32, dtype=np.uint8))
    reaches_the_library(T, tx.CW_ExciterIQData, 1)
    reaches_the_library(T, tx.CW_ExciterIQData, 0)
    reaches_the_library(T, tx.ProcessIQData2_tx, 1)
    reaches_the_library(T, tx.ProcessIQData2_tx, -1)
