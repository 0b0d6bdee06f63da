"""Host-side mirror of the reference's receive-path interface, over the C ABI.

The reference (tmr4/T41_SDR) drives the path through globals and three functions:
  InitializeDataArrays()  T41_SDR.ino:473   -> RxChain(...)
  SetupMode()/CalcFilters()  Filter.cpp:235-249,341-385  -> RxChain.CalcFilters(**changes)
  ProcessIQData()  Process.cpp:70           -> RxChain.ProcessIQData(float_buffer_L, float_buffer_R)
Names and argument meanings follow the firmware (bands[].FLoCut, NCOFreq, audioVolume ...).
PyTorch is used only as the owner of device memory / streams; all arithmetic happens in
libt41rx.so (HIP).  No CPU fallback exists.
"""
import ctypes as C

import numpy as np

from . import _lib, panadapter
from ._lib import DEMOD_AM, DEMOD_LSB, DEMOD_NFM, DEMOD_SAM, DEMOD_USB, Params, T41RxError, check  # noqa: F401


def default_params(**overrides):
    """gwv.cpp:14-96 / bands[] defaults (20 m row) with AGCMode = 0."""
    lib = _lib.load()
    p = Params()
    lib.t41rx_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError("t41rx_params has no field %r" % k)
        setattr(p, k, v)
    return p


def design_coeffs(params):
    """CalcFilters() on the host: returns the coefficient blob (bytes-like numpy uint8)."""
    lib = _lib.load()
    n = lib.t41rx_coeff_blob_bytes(params.fft_length)
    if n == 0:
        raise T41RxError(_lib.ERR_ARG, "unsupported fft_length %d" % params.fft_length)
    blob = np.zeros(n, dtype=np.uint8)
    check(lib.t41rx_design_coeffs(C.byref(params), blob.ctypes.data_as(C.c_void_p), n))
    return blob


def ft8_tables():
    """(window[2048], mag_db[16385]) for RxChain.set_ft8_tables(), in the firmware's types: ft_blackman_i(i, 2048) in f32
    (ft8.cpp:168-178) and (float)(10.0 * log((float)(10 * m) + 0.1)) with the sum and the logarithm in double
    (ft8.cpp:238-240).  numpy's cos / log stand in for the firmware's libm."""
    f = np.float32
    alpha = f(0.16)
    a0, a1, a2 = (f(1) - alpha) / f(2), f(0.5), alpha / f(2)
    x1 = np.cos(f(2) * f(np.pi) * np.arange(2048, dtype=np.float32) / f(2047), dtype=np.float32)
    x2 = f(2) * x1 * x1 - f(1)
    window = (a0 - a1 * x1 + a2 * x2).astype(np.float32)
    m = np.arange(16385, dtype=np.int64)
    mag_db = (10.0 * np.log((10 * m).astype(np.float32).astype(np.float64) + 0.1)).astype(np.float32)
    return window, mag_db


BLOB_HEADER_WORDS = 32  # magic, abi, fft_length, mode, sizeof(params), 3 reserved | t41rx_params padded to 24 words
STATE_HEADER_BYTES = 32  # checkpoint header: magic, abi, fft_length, n_channels, floats per channel, sections, spectrumZoom, reserved


def blob_params(blob):
    """the t41rx_params a coefficient blob was designed for (what set_coeffs() installs)"""
    p = Params()
    raw = np.ascontiguousarray(blob, dtype=np.uint8)[4 * 8:4 * 8 + C.sizeof(Params)].tobytes()
    C.memmove(C.byref(p), raw, C.sizeof(Params))
    return p


def blob_fields(blob, fft_length):
    """Split a coefficient blob into the reference's arrays (numpy views)."""
    f = np.frombuffer(blob, dtype=np.float32)
    o = BLOB_HEADER_WORDS
    out = {}
    for name, n in (("dec1", 28), ("dec2", 46), ("int1", 48), ("int2", 32), ("biquad_lowpass1", 5),
                    ("scalars", 16), ("agc", 16), ("mask", 2 * fft_length)):
        out[name] = f[o:o + n]
        o += n
    return out


class RxChain:
    """n_channels independent T41 receive channels resident on one MI355X."""

    def __init__(self, n_channels, params=None, device=0, NCOFreq=None):
        self._lib = _lib.load()
        self.params = params if params is not None else default_params()
        self._ctx = C.c_void_p()
        check(self._lib.t41rx_create(C.byref(self._ctx), int(device), int(n_channels), C.byref(self.params)))
        self.n_channels = int(n_channels)
        self.device = int(device)
        self.frame_len = self._lib.t41rx_frame_len(self._ctx)
        self.layout = "channel"
        self._n_streams = 0  # the input map's row count (set_input_map), 0 = no map
        if NCOFreq is not None:
            self.SetNCOFreq(NCOFreq)

    # -- configuration ---------------------------------------------------------------------
    def CalcFilters(self, **changes):
        """Filter/mode/gain change between two ProcessIQData() calls; state is kept.  A refused change leaves
        self.params as it was (t41rx_set_params validates before it changes anything)."""
        p = Params.from_buffer_copy(self.params)
        for k, v in changes.items():
            if not hasattr(p, k):
                raise AttributeError("t41rx_params has no field %r" % k)
            setattr(p, k, v)
        check(self._lib.t41rx_set_params(self._ctx, C.byref(p)))
        self.params = p

    SetupMode = CalcFilters

    def SetNCOFreq(self, NCOFreq):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(NCOFreq, dtype=np.int32), (self.n_channels,)))
        check(self._lib.t41rx_set_nco_freq(self._ctx, a.ctypes.data_as(C.POINTER(C.c_int32)), self.n_channels))

    def get_params(self):
        """the parameters the context runs with (after set_coeffs(): the ones the blob was designed for)"""
        p = Params()
        check(self._lib.t41rx_get_params(self._ctx, C.byref(p)))
        return p

    def coeffs(self):
        n = self._lib.t41rx_coeff_blob_bytes(self.params.fft_length)
        blob = np.zeros(n, dtype=np.uint8)
        check(self._lib.t41rx_get_coeffs(self._ctx, blob.ctypes.data_as(C.c_void_p), n))
        return blob

    def set_coeffs(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        check(self._lib.t41rx_set_coeffs(self._ctx, blob.ctypes.data_as(C.c_void_p), blob.size))
        # the context now runs the parameters the blob was designed for: a later CalcFilters(one
        # field) must start from THEM, not from what this object was created with
        self.params = self.get_params()

    def reset(self):
        check(self._lib.t41rx_reset(self._ctx))

    def set_buffer_layout(self, layout):
        """"channel" (default): I / Q / audio are [n_channels, n_frames*frame_len]; "time": [n_frames, n_channels,
        frame_len] -- the [n_channels, frame_len] buffers of consecutive single-frame calls stacked as they arrive
        (t41rx_set_buffer_layout; FFT_LENGTH 512)."""
        code = {"channel": 0, "time": 1}[layout]
        check(self._lib.t41rx_set_buffer_layout(self._ctx, code))
        self.layout = layout

    def set_input_map(self, stream_of_channel, n_streams=None):
        """Receiver groups (t41rx_set_input_map): channel c reads row stream_of_channel[c] of I / Q, which then hold
        n_streams rows -- [n_streams, n_frames*frame_len], time-major [n_frames, n_streams, frame_len] -- while the audio
        and every side output stay [n_channels, ...].  n_streams defaults to max + 1.  None switches the map off.
        Configuration, like the buffer layout: in no checkpoint, kept across reset() / set_state() / CalcFilters()."""
        if stream_of_channel is None:
            check(self._lib.t41rx_set_input_map(self._ctx, None, 0, 0))
            self._n_streams = 0
            return
        m = np.asarray(stream_of_channel)
        if m.ndim != 1 or not np.issubdtype(m.dtype, np.integer) or (m.size and (m.min() < -2**31 or m.max() >= 2**31)):
            raise ValueError("stream_of_channel must be a 1-d array of int32 stream numbers, got %r %s" % (m.shape, m.dtype))
        m = np.ascontiguousarray(m, dtype=np.int32)
        if n_streams is None:
            n_streams = int(m.max()) + 1 if m.size else 0
        check(self._lib.t41rx_set_input_map(self._ctx, m.ctypes.data_as(C.POINTER(C.c_int32)), int(m.size), int(n_streams)))

        self._n_streams = int(n_streams)

    @property
    def n_streams(self):
        """rows of I / Q a process call reads: the input map's n_streams, or n_channels with the map off"""
        return self._n_streams if self._n_streams > 0 else self.n_channels

    @property
    def input_map(self):
        """the input map as an int32 array [n_channels] (a copy), or None with the map off"""
        m = np.zeros(self.n_channels, np.int32)
        v = self._lib.t41rx_get_input_map(self._ctx, m.ctypes.data_as(C.POINTER(C.c_int32)), self.n_channels)
        if v < 0:
            check(v)
        return m if v > 0 else None

    def set_noise_blanker(self, on):
        """NB_on (Process.cpp:873-876): the receive noise blanker on the demodulated audio, behind the noise reduction and
        the notch (t41rx_set_noise_blanker; 0 / 1, fft_length 512).  Kept across CalcFilters() / set_coeffs()."""
        check(self._lib.t41rx_set_noise_blanker(self._ctx, int(on)))

    @property
    def noise_blanker(self):
        v = self._lib.t41rx_get_noise_blanker(self._ctx)
        if v < 0:
            check(v)
        return v

    def set_receive_eq_bands(self, coeffs):
        """The receive equalizer's band table (t41rx_set_receive_eq_bands): the firmware's EQ_Band1Coeffs ..
        EQ_Band14Coeffs as [14][4][5] or [14][20], {b0, b1, b2, a1, a2} per section with the a's negated.  Kept across
        CalcFilters() / set_coeffs(); the filter memories are not reset."""
        c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.float32))
        if c.size != 14 * 4 * 5 or c.shape[0] != 14:
            raise ValueError("receive-EQ band table must be [14][4][5] or [14][20], got %r" % (c.shape,))
        check(self._lib.t41rx_set_receive_eq_bands(self._ctx, c.ctypes.data_as(C.c_void_p)))

    def set_receive_eq(self, on, levels=None):
        """receiveEQFlag and EEPROMData.equalizerRec (Process.cpp:828-832, Filter.cpp:117-165): the receive equalizer on
        the demodulated audio, in front of the noise reduction, the notch and the noise blanker (t41rx_set_receive_eq;
        0 / 1, fft_length 512, a band table loaded first).  levels: 14 ints, or None to keep the current ones (100 each
        until set).  Kept across CalcFilters() / set_coeffs()."""
        if levels is None:
            check(self._lib.t41rx_set_receive_eq(self._ctx, int(on), None))
            return
        lv = np.ascontiguousarray(np.asarray(levels, dtype=np.int32))
        if lv.shape != (14,):
            raise ValueError("receive-EQ levels must be 14 ints, got %r" % (lv.shape,))
        check(self._lib.t41rx_set_receive_eq(self._ctx, int(on), lv.ctypes.data_as(C.c_void_p)))

    @property
    def receive_eq(self):
        """(on, levels): the receive equalizer's switch and its 14 levels"""
        lv = np.zeros(14, np.int32)
        v = self._lib.t41rx_get_receive_eq(self._ctx, lv.ctypes.data_as(C.c_void_p))
        if v < 0:
            check(v)
        return v, lv

    def set_cw_tables(self, audio_filters=None, decode_fir=None):
        """The CW receive tables (t41rx_set_cw_tables): audio_filters = the firmware's CW_AudioFilterCoeffs1..5 as
        [5][6][5] or [5][30], {b0, b1, b2, a1, a2} per section with the a's negated; decode_fir = CW_Filter_Coeffs2, 64
        taps.  None keeps what is loaded.  Kept across CalcFilters() / set_coeffs(); no memory is reset."""
        f = d = None
        if audio_filters is not None:
            f = np.ascontiguousarray(np.asarray(audio_filters, dtype=np.float32))
            if f.size != 5 * 6 * 5 or f.shape[0] != 5:
                raise ValueError("CW filter tables must be [5][6][5] or [5][30], got %r" % (f.shape,))
        if decode_fir is not None:
            d = np.ascontiguousarray(np.asarray(decode_fir, dtype=np.float32))
            if d.shape != (64,):
                raise ValueError("CW decode FIR must be 64 taps, got %r" % (d.shape,))
        check(self._lib.t41rx_set_cw_tables(self._ctx, None if f is None else f.ctypes.data_as(C.c_void_p),
                                            None if d is None else d.ctypes.data_as(C.c_void_p)))

    def set_cw_filter(self, CWFilterIndex):
        """CWFilterIndex (Process.cpp:882-912): 0 .. 4 = the 0.8 / 1.0 / 1.3 / 1.8 / 2.0 kHz narrow audio filter behind the
        noise blanker, 5 = off (the default).  Runs only while xmtMode == CW_MODE; fft_length 512; the filter tables
        loaded first.  Kept across CalcFilters() / set_coeffs()."""
        check(self._lib.t41rx_set_cw_filter(self._ctx, int(CWFilterIndex)))

    @property
    def cw_filter(self):
        v = self._lib.t41rx_get_cw_filter(self._ctx)
        if v < 0:
            check(v)
        return v

    def set_cw_detector(self, on, max_frames=1):
        """decoderFlag (DoCWReceiveProcessing(), CWProcessing.cpp:322-373).  on = 1 allocates and returns the result
        tensor, float32 CUDA [n_channels, max_frames, 4]; a process call of n <= max_frames frames fills its first
        n_channels * n * 4 floats as [n_channels][n][corrResultL, goertzelMagnitude, aveCorrResult, combinedCoeff]
        (cw_results(n) is that view).  on = 0 switches the detector off and returns None.  The `combinedCoeff > 50`
        decision and the Morse decoder behind it are set_cw_decoder()'s.  Runs only while xmtMode == CW_MODE; fft_length 512; the
        decode FIR loaded first.  Kept across CalcFilters() / set_coeffs()."""
        if not on:
            check(self._lib.t41rx_set_cw_detector(self._ctx, 0, None, 0))
            self._cw = None
            return None
        import torch
        if int(max_frames) < 1:
            raise ValueError("max_frames must be >= 1")
        t = torch.zeros(self.n_channels, int(max_frames), 4, dtype=torch.float32, device="cuda:%d" % self.device)
        check(self._lib.t41rx_set_cw_detector(self._ctx, int(on), C.c_void_p(t.data_ptr()), int(max_frames)))
        self._cw = t  # keep alive
        return t

    @property
    def cw_detector(self):
        v = self._lib.t41rx_get_cw_detector(self._ctx)
        if v < 0:
            check(v)
        return v

    def cw_results(self, n_frames):
        """the detector's results of the last process call of n_frames frames: a view [n_channels, n_frames, 4]"""
        t = getattr(self, "_cw", None)
        if t is None:
            raise ValueError("the CW detector is off")
        return t.view(-1)[:self.n_channels * int(n_frames) * 4].view(self.n_channels, int(n_frames), 4)

    def set_cw_decode_tree(self, tree):
        """The Morse decoder's bigMorseCodeTree (CWProcessing.cpp:540; t41rx_set_cw_decode_tree): 129 bytes, as bytes,
        str or uint8 array.  The library has no table of its own.  Kept across CalcFilters() / set_coeffs()."""
        if isinstance(tree, str):
            tree = tree.encode("ascii")
        t = np.ascontiguousarray(np.frombuffer(tree, np.uint8) if isinstance(tree, (bytes, bytearray)) else np.asarray(tree, dtype=np.uint8))
        check(self._lib.t41rx_set_cw_decode_tree(self._ctx, t.ctypes.data_as(C.c_void_p), int(t.size)))

    def set_cw_decoder(self, on, max_frames=1):
        """The Morse decoder behind the detector (DoCWDecoding(), CWProcessing.cpp:365-371, :519-815;
        t41rx_set_cw_decoder).  on = 1 allocates and returns the text tensor, int32 CUDA [n_channels, max_frames, 2]; a
        process call of n <= max_frames frames fills its first n_channels * n * 2 words as [n_channels][n][character
        code or 0, ditLength behind the frame] (cw_text(n) is that view).  on = 0 switches it off and returns None.  Runs
        exactly when the detector runs (xmtMode == CW_MODE, set_cw_detector(1)); fft_length 512; the tree loaded first.
        Kept across CalcFilters() / set_coeffs()."""
        if not on:
            check(self._lib.t41rx_set_cw_decoder(self._ctx, 0, None, 0))
            self._cw_text = None
            return None
        import torch
        if int(max_frames) < 1:
            raise ValueError("max_frames must be >= 1")
        t = torch.zeros(self.n_channels, int(max_frames), 2, dtype=torch.int32, device="cuda:%d" % self.device)
        check(self._lib.t41rx_set_cw_decoder(self._ctx, int(on), C.c_void_p(t.data_ptr()), int(max_frames)))
        self._cw_text = t  # keep alive
        return t

    @property
    def cw_decoder(self):
        v = self._lib.t41rx_get_cw_decoder(self._ctx)
        if v < 0:
            check(v)
        return v

    def cw_text(self, n_frames):
        """the decoder's words of the last process call of n_frames frames: a view [n_channels, n_frames, 2]"""
        t = getattr(self, "_cw_text", None)
        if t is None:
            raise ValueError("the CW decoder is off")
        return t.view(-1)[:self.n_channels * int(n_frames) * 2].view(self.n_channels, int(n_frames), 2)

    def set_cw_clock(self, t0_ms=0, num=32, den=3):
        """The decoder's clock (t41rx_set_cw_clock): millis(n) = t0_ms + floor(n * num / den) for the channel's n-th
        decoder frame; the default is one frame of 2048 samples at 192 kS/s.  From the next call; n is not touched."""
        check(self._lib.t41rx_set_cw_clock(self._ctx, int(t0_ms), int(num), int(den)))

    def reset_cw_histograms(self, channels=None):
        """ResetHistograms() (CWProcessing.cpp:501-517), what the firmware runs at every retune, on the channels whose
        entry is non-zero (None: all): both histograms' words 0 .. 749 and the scalars it names, nothing else."""
        if channels is None:
            check(self._lib.t41rx_reset_cw_histograms(self._ctx, None, 0))
            return
        m = np.ascontiguousarray(np.asarray(channels).astype(bool).astype(np.uint8))
        if m.shape != (self.n_channels,):
            raise ValueError("channels must have n_channels = %d entries, got %r" % (self.n_channels, m.shape))
        check(self._lib.t41rx_reset_cw_histograms(self._ctx, m.ctypes.data_as(C.c_void_p), self.n_channels))

    # -- FT8 receive up to the waterfall ------------------------------------------------------
    def set_ft8_tables(self, window=None, mag_db=None):
        """The FT8 tables (t41rx_set_ft8_tables): window = ft_blackman_i(i, 2048), 2048 floats; mag_db[m] = 10.0 *
        log((float)(10 * m) + 0.1), 16385 floats.  None, None computes both with ft8_tables().  The library has no table of
        its own.  Kept across CalcFilters() / set_coeffs()."""
        if window is None and mag_db is None:
            window, mag_db = ft8_tables()
        if window is None or mag_db is None:
            raise ValueError("window and mag_db must both be given or both be None")
        w = np.ascontiguousarray(np.asarray(window, dtype=np.float32))
        m = np.ascontiguousarray(np.asarray(mag_db, dtype=np.float32))
        if w.shape != (2048,) or m.shape != (16385,):
            raise ValueError("FT8 tables must be 2048 and 16385 floats, got %r and %r" % (w.shape, m.shape))
        check(self._lib.t41rx_set_ft8_tables(self._ctx, w.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p)))

    def set_ft8(self, on, max_frames=1):
        """FT8 receive on a USB context (Process.cpp:627-686, ft8.cpp:153-268; t41rx_set_ft8): the audio collector, the
        two q15 FFTs per 15 frames and the waterfall rows, with the firmware's slot timing.  on = 1 allocates and returns
        (power, status): uint8 CUDA [n_channels, 2, 92 * 1472], the two halves of export_fft_power, and int32 CUDA
        [n_channels, max_frames, 4]; a process call of n <= max_frames <= 1380 frames fills the status' first n_channels *
        n * 4 words as [n_channels][n][FT_8_counter, ft8_flag, 0 or 1 + the half completed in this frame, dataLoop]
        (ft8_status(n) is that view).  on = 0 switches it off and returns None.  Nothing is collected before ft8_sync().
        fft_length 512, mode USB; the tables loaded first.  Kept across CalcFilters() / set_coeffs()."""
        if not on:
            check(self._lib.t41rx_set_ft8(self._ctx, 0, None, None, 0))
            self._ft8 = None
            return None
        import torch
        if int(max_frames) < 1:
            raise ValueError("max_frames must be >= 1")
        dev = "cuda:%d" % self.device
        power = torch.zeros(self.n_channels, 2, 92 * 1472, dtype=torch.uint8, device=dev)
        status = torch.zeros(self.n_channels, int(max_frames), 4, dtype=torch.int32, device=dev)
        check(self._lib.t41rx_set_ft8(self._ctx, int(on), C.c_void_p(power.data_ptr()), C.c_void_p(status.data_ptr()), int(max_frames)))
        self._ft8 = (power, status)  # keep alive
        return power, status

    @property
    def ft8(self):
        v = self._lib.t41rx_get_ft8(self._ctx)
        if v < 0:
            check(v)
        return v

    def ft8_status(self, n_frames):
        """the FT8 status words of the last process call of n_frames frames: a view [n_channels, n_frames, 4]"""
        t = getattr(self, "_ft8", None)
        if t is None:
            raise ValueError("FT8 receive is off")
        return t[1].view(-1)[:self.n_channels * int(n_frames) * 4].view(self.n_channels, int(n_frames), 4)

    def ft8_power(self):
        """export_fft_power, uint8 CUDA [n_channels, 2, 92 * 1472]: the half a status word reported complete holds the
        finished slot, [92 blocks][time_sub 0 / 512][freq_sub 0 / 1][368]"""
        t = getattr(self, "_ft8", None)
        if t is None:
            raise ValueError("FT8 receive is off")
        return t[0]

    def set_ft8_clock(self, t0_ms=0, num=32, den=3):
        """The slot timing's clock (t41rx_set_ft8_clock): millis(n) = t0_ms + floor(n * num / den) for the channel's n-th
        FT8 frame; the default is one frame of 2048 samples at 192 kS/s.  From the next call; n is not touched."""
        check(self._lib.t41rx_set_ft8_clock(self._ctx, int(t0_ms), int(num), int(den)))

    def ft8_sync(self, channels=None):
        """auto_sync_FT8()'s success branch (ft8.cpp:133-136) on the channels whose entry is non-zero (None: all):
        start_time = millis(n), ft8_flag = 1, FT_8_counter = 0, syncFlag = true.  The caller's clock decides when."""
        if channels is None:
            check(self._lib.t41rx_ft8_sync(self._ctx, None, 0))
            return
        m = np.ascontiguousarray(np.asarray(channels).astype(bool).astype(np.uint8))
        if m.shape != (self.n_channels,):
            raise ValueError("channels must have n_channels = %d entries, got %r" % (self.n_channels, m.shape))
        check(self._lib.t41rx_ft8_sync(self._ctx, m.ctypes.data_as(C.c_void_p), self.n_channels))

    def ft8_state(self):
        """the FT8 memory's record (t41rx_ft8_get_state): 8 int32 of header, then [n_channels][3088] int32 (uint8 array)"""
        n = self._lib.t41rx_ft8_state_bytes(self._ctx)
        buf = np.zeros(n, dtype=np.uint8)
        check(self._lib.t41rx_ft8_get_state(self._ctx, buf.ctypes.data_as(C.c_void_p), n))
        return buf

    def set_ft8_state(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        check(self._lib.t41rx_ft8_set_state(self._ctx, buf.ctypes.data_as(C.c_void_p), buf.size))

    # -- FT8 from 12 kS/s audio (DEMOD_FT8_WAV) ----------------------------------------------
    def ft8_audio(self, pcm):
        """The collector of DEMOD_FT8_WAV (Process.cpp:278-335; t41rx_ft8_audio_*) on 12 kS/s audio, without the receive
        chain: pcm [n_channels, 128 * k], int16 (a WAV file's samples, taken as they are) or float32 (through
        arm_float_to_q15), a CUDA tensor (default stream, no synchronisation) or a numpy array.  Always channel-major:
        the input map and the buffer layout do not apply.  Needs set_ft8(1, max_frames >= k); writes the same power halves
        and returns the call's status words, the view ft8_status(k)."""
        n = self.n_channels
        if isinstance(pcm, np.ndarray):
            if pcm.dtype not in (np.int16, np.float32):
                raise ValueError("pcm must be int16 or float32, got %s" % pcm.dtype)
            a = np.ascontiguousarray(pcm)
            k = self._ft8_audio_frames(a.shape)
            fn = self._lib.t41rx_ft8_audio_host_q15 if a.dtype == np.int16 else self._lib.t41rx_ft8_audio_host
            check(fn(self._ctx, a.ctypes.data_as(C.c_void_p), k))
            return self.ft8_status(k)
        import torch
        if not (isinstance(pcm, torch.Tensor) and pcm.is_cuda and pcm.dtype in (torch.int16, torch.float32) and pcm.is_contiguous()):
            raise ValueError("pcm must be a contiguous int16 or float32 CUDA tensor or numpy array")
        if pcm.device.index != self.device:
            raise ValueError("pcm lives on another device than this RxChain")
        k = self._ft8_audio_frames(tuple(pcm.shape))
        fn = self._lib.t41rx_ft8_audio_device_q15 if pcm.dtype == torch.int16 else self._lib.t41rx_ft8_audio_device
        check(fn(self._ctx, C.c_void_p(pcm.data_ptr()), k))
        return self.ft8_status(k)

    def _ft8_audio_frames(self, shape):
        if len(shape) != 2 or shape[0] != self.n_channels or shape[1] < 128 or shape[1] % 128:
            raise ValueError("pcm must be [n_channels = %d, 128 * k], got %r" % (self.n_channels, tuple(shape)))
        if getattr(self, "_ft8", None) is None:
            raise ValueError("FT8 receive is off")
        return shape[1] // 128

    def _ft8_audio_mark(self, fn, channels):
        if channels is None:
            check(fn(self._ctx, None, 0))
            return
        m = np.ascontiguousarray(np.asarray(channels).astype(bool).astype(np.uint8))
        if m.shape != (self.n_channels,):
            raise ValueError("channels must have n_channels = %d entries, got %r" % (self.n_channels, m.shape))
        check(fn(self._ctx, m.ctypes.data_as(C.c_void_p), self.n_channels))

    def ft8_audio_begin(self, channels=None):
        """setupFT8Wav() (ft8.cpp:1372) on the channels whose entry is non-zero (None: all): FT_8_counter = 0, nothing else"""
        self._ft8_audio_mark(self._lib.t41rx_ft8_audio_begin, channels)

    def ft8_audio_end(self, channels=None):
        """the WAV mode's exit (Process.cpp:339-342) on the channels whose entry is non-zero (None: all): syncFlag = 0,
        FT_8_counter = 0, ft8_flag = 0, nothing else"""
        self._ft8_audio_mark(self._lib.t41rx_ft8_audio_end, channels)

    def set_ft8_decode_tables(self, costas, gray, nm, mn, nrw):
        """The FT8 decode's tables (t41rx_set_ft8_decode_tables): kCostas_map[7], kGray_map[8], kNm[83][7], kMn[174][3] and
        kNrw[83] of ft8_constants.cpp as uint8.  The library has no table of its own, and refuses tables that would take
        the kernels' indexing outside their arrays."""
        arrs = []
        for a, shape, what in ((costas, (7,), "costas"), (gray, (8,), "gray"), (nm, (83, 7), "nm"), (mn, (174, 3), "mn"), (nrw, (83,), "nrw")):
            a = np.asarray(a)
            if a.shape != shape:
                raise ValueError("%s must have shape %r, got %r" % (what, shape, a.shape))
            if a.min() < 0 or a.max() > 255:
                raise ValueError("%s does not fit uint8" % what)
            arrs.append(np.ascontiguousarray(a, dtype=np.uint8))
        check(self._lib.t41rx_set_ft8_decode_tables(self._ctx, *[a.ctypes.data_as(C.c_void_p) for a in arrs]))

    def set_ft8_decode(self, max_candidates=20, min_score=40, ldpc_iterations=10):
        """kMax_candidates (1..20), kMin_score and kLDPC_iterations (1..50) of the decode (t41rx_set_ft8_decode); the
        defaults are the firmware's (ft8.cpp:64-72)."""
        check(self._lib.t41rx_set_ft8_decode(self._ctx, int(max_candidates), int(min_score), int(ldpc_iterations)))

    @property
    def ft8_decode_params(self):
        """(max_candidates, min_score, ldpc_iterations)"""
        v = [C.c_int(), C.c_int(), C.c_int()]
        check(self._lib.t41rx_get_ft8_decode(self._ctx, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def ft8_decode(self, select=None, waterfall=None, debug=False):
        """find_sync() and, per candidate, extract_likelihood(), bp_decode(), pack_bits() and the CRC check on finished slots
        (t41rx_ft8_decode_device, on the current torch stream; synchronises to hand the records back).  Channel c reads
        slot select[c] (-1 = skip, 0, 1; None = all 0) of its row of `waterfall`, a uint8 CUDA tensor [n_channels, bytes
        per channel] whose rows hold one or two slots of 92 * 1472 bytes; waterfall None reads the context's own
        export_fft_power (set_ft8), where select names the half a status word reported complete.  Returns a numpy array
        [n_channels] of dtype t41_sdr_amd.ft8.RESULT (ft8.messages() turns it into text); with debug also the stage taps
        log174 [n_channels, 20, 174] f32 and plain [n_channels, 20, 174] uint8."""
        import torch
        from . import ft8 as F
        n = self.n_channels
        dev = "cuda:%d" % self.device
        sel = None
        if select is not None:
            sel = np.asarray(select)
            if sel.shape != (n,):
                raise ValueError("select must have n_channels = %d entries, got %r" % (n, sel.shape))
            if ((sel < -128) | (sel > 127)).any():
                raise ValueError("select does not fit int8")
            sel = np.ascontiguousarray(sel, dtype=np.int8)
        ptr, stride = None, 0
        if waterfall is not None:
            if not (isinstance(waterfall, torch.Tensor) and waterfall.is_cuda and waterfall.dtype == torch.uint8 and waterfall.dim() == 2
                    and waterfall.shape[0] == n and waterfall.stride(1) == 1):
                raise ValueError("waterfall must be a uint8 CUDA tensor [n_channels, bytes per channel] with unit inner stride")
            need = F.SLOT_BYTES * (2 if sel is not None and (sel == 1).any() else 1)
            if waterfall.shape[1] < need:
                raise ValueError("waterfall rows hold %d bytes, the call reads %d" % (waterfall.shape[1], need))
            ptr, stride = C.c_void_p(waterfall.data_ptr()), int(waterfall.stride(0)) if n > 1 else int(waterfall.shape[1])
        res = torch.zeros(n, F.RESULT.itemsize, dtype=torch.uint8, device=dev)
        taps = None
        if debug:
            taps = (torch.zeros(n, F.MAX_CANDIDATES, 174, dtype=torch.float32, device=dev),
                    torch.zeros(n, F.MAX_CANDIDATES, 174, dtype=torch.uint8, device=dev))
            check(self._lib.t41rx_set_ft8_decode_debug(self._ctx, C.c_void_p(taps[0].data_ptr()), C.c_void_p(taps[1].data_ptr())))
        try:
            stream = torch.cuda.current_stream(res.device).cuda_stream
            check(self._lib.t41rx_ft8_decode_device(self._ctx, ptr, stride, None if sel is None else sel.ctypes.data_as(C.c_void_p), n,
                                                    C.c_void_p(res.data_ptr()), C.c_void_p(stream)))
            out = res.cpu().numpy().view(F.RESULT).reshape(n)
            if debug:
                return out, taps[0].cpu().numpy(), taps[1].cpu().numpy()
            return out
        finally:
            if debug:
                torch.cuda.synchronize(res.device)
                check(self._lib.t41rx_set_ft8_decode_debug(self._ctx, None, None))

    def get_state(self):
        n = self._lib.t41rx_state_bytes(self._ctx)
        buf = np.zeros(n, dtype=np.uint8)
        check(self._lib.t41rx_get_state(self._ctx, buf.ctypes.data_as(C.c_void_p), n))
        return buf

    def set_state(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        check(self._lib.t41rx_set_state(self._ctx, buf.ctypes.data_as(C.c_void_p), buf.size))

    def state_records(self, buf=None):
        """the per-channel records of a checkpoint (default: a fresh one) as float32 [n_channels, floats]"""
        buf = self.get_state() if buf is None else np.ascontiguousarray(buf, dtype=np.uint8)
        per = int(buf[:STATE_HEADER_BYTES].view(np.int32)[4])  # floats per channel of the path's section (the side stages' follow it)
        return buf[STATE_HEADER_BYTES:STATE_HEADER_BYTES + 4 * per * self.n_channels].view(np.float32).reshape(self.n_channels, per)

    # -- the hot path ----------------------------------------------------------------------
    def ProcessIQData(self, float_buffer_L, float_buffer_R, out=None):
        """One ProcessIQData() per channel (or several consecutive ones).

        torch CUDA tensors [n_channels, n_frames*frame_len] (float32, contiguous) run on the
        current torch stream without synchronising and return a tensor; numpy arrays go
        through the host-pointer entry point and return a numpy array.
        """
        if isinstance(float_buffer_L, np.ndarray):
            I = np.ascontiguousarray(float_buffer_L, dtype=np.float32)
            Q = np.ascontiguousarray(float_buffer_R, dtype=np.float32)
            nfr = self._check_shape(I.shape, Q.shape)
            audio = np.empty(self._out_shape(nfr), I.dtype) if out is None else self._check_out_numpy(out, I, nfr)
            fp = C.POINTER(C.c_float)
            check(self._lib.t41rx_process_host(self._ctx, I.ctypes.data_as(fp), Q.ctypes.data_as(fp),
                                               audio.ctypes.data_as(fp), nfr))
            return audio
        import torch
        I, Q = float_buffer_L, float_buffer_R
        if not (I.is_cuda and Q.is_cuda and I.dtype == torch.float32 and Q.dtype == torch.float32
                and I.is_contiguous() and Q.is_contiguous()):
            raise ValueError("I/Q must be contiguous float32 CUDA tensors")
        if I.device.index != self.device or Q.device.index != self.device:
            raise ValueError("I/Q live on another device than this RxChain")
        nfr = self._check_shape(tuple(I.shape), tuple(Q.shape))
        audio = self._new_out_torch(I, nfr) if out is None else self._check_out_torch(out, I, nfr)
        stream = torch.cuda.current_stream(I.device).cuda_stream
        check(self._lib.t41rx_process_device(self._ctx, I.data_ptr(), Q.data_ptr(), audio.data_ptr(), nfr,
                                             C.c_void_p(stream)))
        return audio

    def ProcessIQData_q15(self, Q_in_L, Q_in_R, out=None):
        """The same on the firmware's wire format (Process.cpp:102-111, 936-937): int16 (q15) blocks
        of the L and R record queues in -- I is taken from the R queue, Q from the L queue, as the
        firmware does -- and the q15 samples handed to Q_out_L.play() out.
        torch CUDA int16 tensors or numpy int16 arrays, [n_channels, n_frames*frame_len]."""
        if isinstance(Q_in_L, np.ndarray):
            a = np.ascontiguousarray(Q_in_L, dtype=np.int16)
            b = np.ascontiguousarray(Q_in_R, dtype=np.int16)
            nfr = self._check_shape(a.shape, b.shape)
            audio = np.empty(self._out_shape(nfr), a.dtype) if out is None else self._check_out_numpy(out, a, nfr)
            check(self._lib.t41rx_process_host_q15(self._ctx, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                                   audio.ctypes.data_as(C.c_void_p), nfr))
            return audio
        import torch
        a, b = Q_in_L, Q_in_R
        if not (a.is_cuda and b.is_cuda and a.dtype == torch.int16 and b.dtype == torch.int16
                and a.is_contiguous() and b.is_contiguous()):
            raise ValueError("Q_in_L/Q_in_R must be contiguous int16 CUDA tensors")
        if a.device.index != self.device or b.device.index != self.device:
            raise ValueError("the queues live on another device than this RxChain")
        nfr = self._check_shape(tuple(a.shape), tuple(b.shape))
        audio = self._new_out_torch(a, nfr) if out is None else self._check_out_torch(out, a, nfr)
        stream = torch.cuda.current_stream(a.device).cuda_stream
        check(self._lib.t41rx_process_device_q15(self._ctx, a.data_ptr(), b.data_ptr(), audio.data_ptr(), nfr,
                                                 C.c_void_p(stream)))
        return audio

    def _side_tensor(self, t, per_frame, what):
        """validate a side-output tensor; returns (pointer, frames it has room for)"""
        if t is None:
            return None, None
        import torch
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device.index == self.device):
            raise ValueError("%s must be a contiguous float32 CUDA tensor on device %d" % (what, self.device))
        frames = t.numel() // (self.n_channels * per_frame)
        if frames < 1:
            raise ValueError("%s holds less than one frame (%d floats per channel and frame)" % (what, per_frame))
        return C.c_void_p(t.data_ptr()), frames

    def set_debug_taps(self, post_nco=None, dec=None, demod=None):
        """stage taps (torch CUDA float32 tensors or None): post_nco [n_channels, n_frames*2*frame_len],
        dec [n_channels, n_frames*fft_length], demod [n_channels, n_frames*fft_length/2].  Calls with
        more frames than the smallest of them holds are refused."""
        N = self.params.fft_length
        got = [self._side_tensor(post_nco, 2 * self.frame_len, "post_nco"), self._side_tensor(dec, N, "dec"),
               self._side_tensor(demod, N // 2, "demod")]
        frames = [f for _, f in got if f is not None]
        check(self._lib.t41rx_set_debug_taps(self._ctx, got[0][0], got[1][0], got[2][0], min(frames) if frames else 0))
        self._taps = (post_nco, dec, demod)  # keep alive

    def set_audio_spectrum(self, spect=None, maxima=None):
        """the display by-product of the path (Process.cpp:550-570): torch CUDA float32 tensors
        [n_channels, n_frames, 1024] and [n_channels, n_frames, 3], or None/None to switch it off"""
        ps, fs = self._side_tensor(spect, 1024, "spect")
        pm, fm = self._side_tensor(maxima, 3, "maxima")
        frames = [f for f in (fs, fm) if f is not None]
        check(self._lib.t41rx_set_audio_spectrum(self._ctx, ps, pm, min(frames) if frames else 0))
        self._spect = (spect, maxima)  # keep alive

    def set_display_spectrum(self, spec=None, spec_old=None, spectrumZoom=1):
        """the display FFT (CalcZoom1Magn / ZoomFFTExe, FFT.cpp:67-251): torch CUDA float32 tensors
        [n_channels, n_frames, 512] for FFT_spec and FFT_spec_old, or None/None to switch it off"""
        ps, fs = self._side_tensor(spec, 512, "spec")
        po, fo = self._side_tensor(spec_old, 512, "spec_old")
        frames = [f for f in (fs, fo) if f is not None]
        check(self._lib.t41rx_set_display_spectrum(self._ctx, ps, po, int(spectrumZoom), min(frames) if frames else 0))
        self._disp = (spec, spec_old)  # keep alive

    # -- the panadapter stage ------------------------------------------------------------------
    PANADAPTER_ROWS = (("pixel", "int16", 512), ("y_new", "int16", 512), ("y_old", "int16", 512), ("waterfall", "uint16", 512),
                       ("spec", "float32", 512), ("audio_spect", "float32", 1024), ("smeter", "float32", 4))

    def set_panadapter_tables(self, gradient):
        """The waterfall's colour words gradient[] (Display.cpp:148-161; t41rx_set_panadapter_tables): 117 uint16.  The
        library has no table of its own."""
        g = np.asarray(gradient)
        if g.ndim != 1 or not np.issubdtype(g.dtype, np.integer) or (g.size and (g.min() < 0 or g.max() > 0xFFFF)):
            raise ValueError("gradient must be a 1-d array of uint16 colour words, got %r %s" % (g.shape, g.dtype))
        g = np.ascontiguousarray(g, dtype=np.uint16)
        check(self._lib.t41rx_set_panadapter_tables(self._ctx, g.ctypes.data_as(C.POINTER(C.c_uint16)), int(g.size)))

    def set_panadapter(self, on=True, spectrumZoom=0, currentScale=1, pixel_offset=0, spectrumNoiseFloor=panadapter.SPECTRUM_NOISE_FLOOR,
                       update_period=panadapter.UPDATE_PERIOD, update_phase=0, max_rows=1, outputs=None):
        """ShowSpectrum()'s pixels and waterfall row and DrawSmeterBar()'s dBm as a stage of the path
        (t41rx_set_panadapter), at the firmware's cadence: frame n of the stage's count is an update frame when n %
        update_period == update_phase (panadapter.rows_of_call()).  outputs: None allocates every row buffer, a list of
        names of PANADAPTER_ROWS allocates those, a dict name -> CUDA tensor [n_channels, max_rows, width] uses the
        caller's; what is left out is not written.  Returns the dict of row buffers: a call with k update frames writes
        rows 0 .. k-1 of every channel (panadapter_status()).  on = False switches the stage off and returns None.
        Starts the stage's memory and its frame counter from power-on.  fft_length 512; the colour table loaded first."""
        if not on:
            check(self._lib.t41rx_set_panadapter(self._ctx, 0, 0, 0, 0, 0, 1, 0, None, 0))
            self._pan = None
            return None
        import torch
        if int(max_rows) < 1:
            raise ValueError("max_rows must be >= 1")
        kinds = {name: (getattr(torch, dt), width) for name, dt, width in self.PANADAPTER_ROWS}
        if outputs is None:
            outputs = list(kinds)
        bufs = {}
        for name in outputs:
            if name not in kinds:
                raise ValueError("unknown panadapter output %r (one of %s)" % (name, ", ".join(kinds)))
            dt, width = kinds[name]
            shape = (self.n_channels, int(max_rows), width)
            t = outputs[name] if isinstance(outputs, dict) else None
            if t is None:  # (uint16: allocated as int16 and viewed, the type torch fills on every build)
                t = torch.zeros(shape, dtype=torch.int16 if dt == torch.uint16 else dt, device="cuda:%d" % self.device).view(dt)
            elif not (t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape and t.device.index == self.device):
                raise ValueError("%s must be a contiguous %s CUDA tensor of shape %r on device %d" % (name, dt, shape, self.device))
            bufs[name] = t
        out = _lib.PanadapterOut(**{name: C.c_void_p(t.data_ptr()) for name, t in bufs.items()})
        self._pan = None
        check(self._lib.t41rx_set_panadapter(self._ctx, 1, int(spectrumZoom), int(currentScale), int(pixel_offset), int(spectrumNoiseFloor),
                                             int(update_period), int(update_phase), C.byref(out), int(max_rows)))
        self._pan = bufs  # keep alive
        return bufs

    def set_panadapter_levels(self, noise_floor=None, gain_correction=None, attenuator=0):
        """currentNoiseFloor[currentBand] (ints) and bands[currentBand].gainCorrection (floats) per channel, None = zeros,
        and `attenuator` (t41rx_set_panadapter_levels).  From the next process call."""
        nf = gc = None
        if noise_floor is not None:
            nf = np.asarray(noise_floor)
            if nf.shape != (self.n_channels,) or not np.issubdtype(nf.dtype, np.integer) or (nf.min() < -2**31 or nf.max() >= 2**31):
                raise ValueError("noise_floor must be n_channels = %d int32 values, got %r %s" % (self.n_channels, nf.shape, nf.dtype))
            nf = np.ascontiguousarray(nf, dtype=np.int32)
        if gain_correction is not None:
            gc = np.ascontiguousarray(np.asarray(gain_correction, dtype=np.float32))
            if gc.shape != (self.n_channels,):
                raise ValueError("gain_correction must be n_channels = %d floats, got %r" % (self.n_channels, gc.shape))
        check(self._lib.t41rx_set_panadapter_levels(self._ctx, None if nf is None else nf.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    None if gc is None else gc.ctypes.data_as(C.POINTER(C.c_float)), int(attenuator)))

    def panadapter_status(self):
        """(on, frame_counter, rows_written, first_row_frame): the stage's switch, its frame count behind the last process
        call, the rows that call wrote and the frame count of its row 0 (-1: none)"""
        n, k, f = C.c_int64(), C.c_int32(), C.c_int64()
        v = self._lib.t41rx_get_panadapter(self._ctx, C.byref(n), C.byref(k), C.byref(f))
        if v < 0:
            check(v)
        return bool(v), n.value, k.value, f.value

    def set_panadapter_counter(self, n):
        """the stage's frame counter (t41rx_set_panadapter_counter), n >= 0"""
        check(self._lib.t41rx_set_panadapter_counter(self._ctx, int(n)))

    # -- IQ calibration ----------------------------------------------------------------------
    CAL_BINS ={("rx", DEMOD_LSB): (310, 460), ("rx", DEMOD_USB): (65, 192),   # cal_bins[], Process2.cpp:429-444
                ("tx", DEMOD_LSB): (240, 305), ("tx", DEMOD_USB): (209, 273)}

    def set_calibration(self, on=True, spectrumZoom=0, currentScale=1, pixel_offset=0, bin0=310, bin1=460, capture_bins=10):
        """ProcessIQData2() / PlotCalSpectrum() (t41rx_set_calibration): the display FFT's zoom, displayScale[currentScale],
        bands[].pixel_offset and the two windows [bin - capture_bins, bin + capture_bins).  Starts the calibration memory
        from power-on.  fft_length 512, channel-major."""
        check(self._lib.t41rx_set_calibration(self._ctx, int(bool(on)), int(spectrumZoom), int(currentScale), int(pixel_offset),
                                              int(bin0), int(bin1), int(capture_bins)))

    def set_cal_corrections(self, amp=None, phase=None):
        """one (IQAmpCorrectionFactor, IQPhaseCorrectionFactor) candidate per channel for the calibration calls
        (t41rx_set_cal_corrections): two arrays of n_channels floats, or None, None for the params' factors"""
        if amp is None and phase is None:
            check(self._lib.t41rx_set_cal_corrections(self._ctx, None, None))
            return
        if amp is None or phase is None:
            raise ValueError("amp and phase must both be given or both be None")
        a = np.ascontiguousarray(np.asarray(amp, dtype=np.float32))
        p = np.ascontiguousarray(np.asarray(phase, dtype=np.float32))
        if a.shape != (self.n_channels,) or p.shape != (self.n_channels,):
            raise ValueError("corrections must be %d floats each, got %r and %r" % (self.n_channels, a.shape, p.shape))
        check(self._lib.t41rx_set_cal_corrections(self._ctx, a.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p)))

    def ProcessIQData2_rx(self, I, Q, update=None, shared_input=False, pixel=False, spec=False):
        """The receive half of ProcessIQData2() with PlotCalSpectrum()'s measurement, n_frames frames per channel.
        I / Q: float32 (float_buffer_L / _R) or int16 (the queues Q_in_L / Q_in_R: I is taken from the R queue),
        [n_channels, n_frames * 2048], or with shared_input one recording [n_frames * 2048] (or [1, ...]) for all channels.
        update: n_frames bytes, updateDisplayFlag per frame, None = every frame.  pixel / spec: True for a fresh zeroed
        buffer, or a buffer [n_channels, n_frames, 512] (int16 / float32) whose rows of frames without the flag are left
        alone.  numpy arrays use the host entries, torch CUDA tensors the device entries on the current stream.
        Returns (result [n_channels, n_frames, 3] = refAmplitude, adjAmplitude, adjdB, pixel or None, spec or None)."""
        host = isinstance(I, np.ndarray)
        if host:
            q15 = I.dtype == np.int16
            I = np.ascontiguousarray(I, dtype=np.int16 if q15 else np.float32)
            Q = np.ascontiguousarray(Q, dtype=I.dtype)
        else:
            import torch
            q15 = I.dtype == torch.int16
            if not (I.is_cuda and Q.is_cuda and I.dtype == Q.dtype and I.dtype in (torch.int16, torch.float32)
                    and I.is_contiguous() and Q.is_contiguous() and I.device.index == self.device and Q.device.index == self.device):
                raise ValueError("I/Q must be contiguous float32 or int16 CUDA tensors on device %d" % self.device)
        si, sq = tuple(I.shape), tuple(Q.shape)
        rows = 1 if shared_input else self.n_channels
        if len(si) == 1 and shared_input:
            si = (1,) + si
        if tuple(Q.shape) != tuple(I.shape) or len(si) != 2 or si[0] != rows or si[1] == 0 or si[1] % 2048:
            raise ValueError("I/Q must be [%d, k*2048], got %r / %r" % (rows, tuple(I.shape), sq))
        nfr = si[1] // 2048
        shape = (self.n_channels, nfr)

        def side(buf, dtype_np, what):
            if buf is False or buf is None:
                return None
            if buf is True:
                if host:
                    return np.zeros(shape + (512,), dtype_np)
                return torch.zeros(shape + (512,), dtype=torch.int16 if dtype_np == np.int16 else torch.float32, device=I.device)
            ok = tuple(buf.shape) == shape + (512,) and (
                (isinstance(buf, np.ndarray) and buf.dtype == dtype_np and buf.flags["C_CONTIGUOUS"] and buf.flags["WRITEABLE"]) if host
                else (buf.is_cuda and buf.is_contiguous() and buf.device == I.device
                      and buf.dtype == (torch.int16 if dtype_np == np.int16 else torch.float32)))
            if not ok:
                raise ValueError("%s must be a contiguous %s buffer of shape %r next to I/Q" % (what, np.dtype(dtype_np).name, shape + (512,)))
            return buf

        pixel, spec = side(pixel, np.int16, "pixel"), side(spec, np.float32, "spec")
        if host:
            u = None
            if update is not None:
                u = np.ascontiguousarray(np.asarray(update) != 0, dtype=np.uint8)
                if u.shape != (nfr,):
                    raise ValueError("update must hold n_frames=%d flags, got %r" % (nfr, u.shape))
            res = np.zeros(shape + (3,), np.float32)
            p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
            fn = self._lib.t41rx_calibrate_host_q15 if q15 else self._lib.t41rx_calibrate_host
            check(fn(self._ctx, p(I), p(Q), int(bool(shared_input)), p(u), p(res), p(pixel), p(spec), nfr))
            return res, pixel, spec
        u = None
        if update is not None:
            u = update if isinstance(update, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(update) != 0, dtype=np.uint8)).to(I.device)
            if not (u.is_cuda and u.dtype == torch.uint8 and u.is_contiguous() and tuple(u.shape) == (nfr,)):
                raise ValueError("update must hold n_frames=%d uint8 flags" % nfr)
        res = torch.zeros(shape + (3,), dtype=torch.float32, device=I.device)
        p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        stream = torch.cuda.current_stream(I.device).cuda_stream
        fn = self._lib.t41rx_calibrate_device_q15 if q15 else self._lib.t41rx_calibrate_device
        check(fn(self._ctx, p(I), p(Q), int(bool(shared_input)), p(u), p(res), p(pixel), p(spec), nfr, C.c_void_p(stream)))
        self._cal_keep = (I, Q, u)  # alive until the next call: the launch is asynchronous
        return res, pixel, spec

    def _out_shape(self, nfr):
        """the audio's shape for a call of nfr frames: n_channels rows, whatever the input map makes of the input's"""
        if self.layout == "time":
            return (nfr, self.n_channels, self.frame_len)
        return (self.n_channels, nfr * self.frame_len)

    def _new_out_torch(self, like, nfr):
        import torch
        return torch.empty(self._out_shape(nfr), dtype=like.dtype, device=like.device)

    def _rows_text(self):
        return "(n_channels=%d, n_streams=%d)" % (self.n_channels, self.n_streams)

    def _check_out_torch(self, out, like, nfr):
        shape = self._out_shape(nfr)
        if not (out.is_cuda and out.dtype == like.dtype and out.is_contiguous() and tuple(out.shape) == shape
                and out.device == like.device):
            raise ValueError("out must be a contiguous %s CUDA tensor of shape %r on %s %s"
                             % (like.dtype, shape, like.device, self._rows_text()))
        return out

    def _check_out_numpy(self, out, like, nfr):
        shape = self._out_shape(nfr)
        if not (isinstance(out, np.ndarray) and out.dtype == like.dtype and out.shape == shape
                and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]):
            raise ValueError("out must be a writeable C-contiguous %s array of shape %r %s" % (like.dtype, shape, self._rows_text()))
        return out

    def _check_shape(self, si, sq):
        """n_frames of a call on I / Q of these shapes: one row per channel, or with an input map one per stream"""
        rows = self.n_streams
        if self.layout == "time":
            if si != sq or len(si) != 3 or si[0] == 0 or si[1] != rows or si[2] != self.frame_len:
                raise ValueError("time-major I/Q must be [n_frames, %d, frame_len=%d] %s, got %r / %r"
                                 % (rows, self.frame_len, self._rows_text(), si, sq))
            return si[0]
        if si != sq or len(si) != 2 or si[0] != rows or si[1] == 0 or si[1] % self.frame_len:
            raise ValueError("I/Q must be [%d, k*frame_len=%d] %s, got %r / %r"
                             % (rows, self.frame_len, self._rows_text(), si, sq))
        return si[1] // self.frame_len

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self._lib.t41rx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
