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

from . import _args, _lib, panadapter
from ._args import F32P, I32P, U16P, U32P, channel_mask, cuda, cuda_tensor, get_blob, int_table, kept, ptr, run, set_blob, table, table_pair, value, with_fields
from ._lib import DEMOD_AM, DEMOD_LSB, DEMOD_NFM, DEMOD_SAM, DEMOD_USB, SETS_STAGES, Params, T41RxError, check  # noqa: F401


def default_params(**overrides):
    """gwv.cpp:14-96 / bands[] defaults (20 m row) with AGCMode = 0."""
    lib = _lib.load()
    p = Params()
    lib.t41rx_default_params(C.byref(p))
    return with_fields(p, "t41rx_params", overrides)


def design_coeffs(params):
    """CalcFilters() on the host: returns the coefficient blob (bytes-like numpy uint8)."""
    lib = _lib.load()
    n = lib.t41rx_coeff_blob_bytes(params.fft_length)
    if n == 0:
        raise T41RxError(_lib.ERR_ARG, "unsupported fft_length %d" % params.fft_length)
    return get_blob(lib.t41rx_design_coeffs, C.byref(params), n)


def param_sets_compatible(a, b, stages=False):
    """The rule of RxChain.set_param_sets() on two t41rx_params, on the host (t41rx_param_sets_compatible): (True, "")
    when they may share a chain, else (False, the clause they break).  An invalid struct raises T41RxError.
    stages=True: the rule of sets loaded next to the chain-splitting stages (t41rx_param_sets_compatible_ex with
    T41RX_SETS_STAGES), which lets nrOptionSelect and ANR_notchOn differ."""
    lib = _lib.load()
    if stages:
        rc = lib.t41rx_param_sets_compatible_ex(C.byref(a), C.byref(b), SETS_STAGES)
    else:
        rc = lib.t41rx_param_sets_compatible(C.byref(a), C.byref(b))
    if rc == _lib.ERR_UNSUPPORTED:
        return False, lib.t41rx_last_error().decode()
    check(rc)
    return True, ""


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
        self._audio_rate = 192000  # set_audio_rate
        self._n_streams = 0  # the input map's row count (set_input_map), 0 = no map
        self._audio_rows = None  # the output map's row count (set_output_map), None = no map
        self._ft8_rows = None  # the FT8 map's row count (set_ft8_map), None = no map
        if NCOFreq is not None:
            self.SetNCOFreq(NCOFreq)

    # -- configuration ---------------------------------------------------------------------
    def CalcFilters(self, **changes):
        """Filter/mode/gain change between two ProcessIQData() calls; state is kept.  A refused change leaves
        self.params as it was (t41rx_set_params validates before it changes anything)."""
        p = with_fields(Params.from_buffer_copy(self.params), "t41rx_params", changes)
        check(self._lib.t41rx_set_params(self._ctx, C.byref(p)))
        self.params = p

    SetupMode = CalcFilters

    def SetNCOFreq(self, NCOFreq):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(NCOFreq, dtype=np.int32), (self.n_channels,)))
        check(self._lib.t41rx_set_nco_freq(self._ctx, ptr(a, I32P), self.n_channels))

    def get_params(self):
        """the parameters the context runs with (after set_coeffs(): the ones the blob was designed for)"""
        p = Params()
        check(self._lib.t41rx_get_params(self._ctx, C.byref(p)))
        return p

    def coeffs(self):
        return get_blob(self._lib.t41rx_get_coeffs, self._ctx, self._lib.t41rx_coeff_blob_bytes(self.params.fft_length))

    def set_coeffs(self, blob):
        set_blob(self._lib.t41rx_set_coeffs, self._ctx, blob)
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

    _AUDIO_RATES = {192000: 0, 24000: 1}  # T41RX_AUDIO_RATE_192K, T41RX_AUDIO_RATE_24K

    def set_audio_rate(self, rate):
        """192000 (default): the process calls return frame_len samples per channel and frame, the firmware's DAC rate;
        24000: the audio as it leaves the demodulator and the stages behind it, times VolumeToAmplification(audioVolume),
        256 samples per channel and frame, no interpolators (t41rx_set_audio_rate; FFT_LENGTH 512).  Configuration, like
        the buffer layout; a refused change leaves the rate as it was."""
        if isinstance(rate, bool) or rate not in self._AUDIO_RATES:
            raise ValueError("audio rate must be 24000 or 192000, got %r" % (rate,))
        check(self._lib.t41rx_set_audio_rate(self._ctx, self._AUDIO_RATES[rate]))
        self._audio_rate = int(rate)

    @property
    def audio_rate(self):
        """samples per second of the audio the process calls return: 192000 or 24000"""
        return getattr(self, "_audio_rate", 192000)

    @property
    def audio_frame_len(self):
        """samples per channel and frame the process calls return: frame_len, or 256 at 24 kS/s"""
        return 256 if self.audio_rate == 24000 else self.frame_len

    def set_input_map(self, stream_of_channel, n_streams=None):
        """Receiver groups (t41rx_set_input_map): channel c reads row stream_of_channel[c] of I / Q, which then hold
        n_streams rows -- [n_streams, n_frames*frame_len], time-major [n_frames, n_streams, frame_len] -- while the audio
        and every side output stay [n_channels, ...].  n_streams defaults to max + 1.  None switches the map off.
        Configuration, like the buffer layout: in no checkpoint, kept across reset() / set_state() / CalcFilters()."""
        if stream_of_channel is None:
            check(self._lib.t41rx_set_input_map(self._ctx, None, 0, 0))
            self._n_streams = 0
            return
        m = int_table(stream_of_channel, np.int32, None, "stream_of_channel must be a 1-d array of int32 stream numbers, got %r %s")
        if n_streams is None:
            n_streams = int(m.max()) + 1 if m.size else 0
        check(self._lib.t41rx_set_input_map(self._ctx, ptr(m, I32P), int(m.size), int(n_streams)))
        self._n_streams = int(n_streams)

    @property
    def n_streams(self):
        """rows of I / Q a process call reads: the input map's n_streams, or n_channels with the map off"""
        return self._n_streams if self._n_streams > 0 else self.n_channels

    @property
    def input_map(self):
        """the input map as an int32 array [n_channels] (a copy), or None with the map off"""
        m = np.zeros(self.n_channels, np.int32)
        return m if value(self._lib.t41rx_get_input_map(self._ctx, ptr(m, I32P), self.n_channels)) > 0 else None

    def set_output_map(self, row_of_channel, n_rows=None):
        """Receiver groups (t41rx_set_output_map): channel c writes its audio to row row_of_channel[c] of the audio, or with
        -1 writes none; the audio then holds n_rows rows -- [n_rows, n_frames*audio_frame_len], time-major [n_frames,
        n_rows, audio_frame_len] -- while I / Q and every side output keep their shapes.  No row may be named twice;
        n_rows defaults to max + 1 (0 with every channel muted: the process calls then return an empty (0, ...) result).
        A muted channel computes everything but its interpolators and its audio stores.  None switches the map off.
        Configuration, like the input map: in no checkpoint, kept across reset() / set_state() / CalcFilters(); FFT_LENGTH 512."""
        if row_of_channel is None:
            check(self._lib.t41rx_set_output_map(self._ctx, None, 0, 0))
            self._audio_rows = None
            return
        m = int_table(row_of_channel, np.int32, None, "row_of_channel must be a 1-d array of int32 row numbers (-1: no audio), got %r %s")
        if n_rows is None:
            n_rows = max(int(m.max()) + 1, 0) if m.size else 0
        check(self._lib.t41rx_set_output_map(self._ctx, ptr(m, I32P), int(m.size), int(n_rows)))
        self._audio_rows = int(n_rows)

    @property
    def audio_rows(self):
        """rows of audio a process call writes: the output map's n_rows, or n_channels with the map off"""
        # kept here like the input map's row count and the audio rate, and read the same way: the shape checks make no call
        # into the library and work on an object that never set a map.  (A map set through the raw handle is not seen.)
        rows = getattr(self, "_audio_rows", None)
        return self.n_channels if rows is None else rows

    @property
    def output_map(self):
        """the output map as an int32 array [n_channels] (a copy, -1: muted), or None with the map off"""
        m = np.zeros(self.n_channels, np.int32)
        return m if value(self._lib.t41rx_get_output_map(self._ctx, ptr(m, I32P), self.n_channels, None)) > 0 else None

    def set_stage_map(self, stages):
        """Receiver groups (t41rx_set_stage_map): stages[c] is channel c's mask of STAGE_EQ, STAGE_NR (noise reduction and
        notch), STAGE_NB, STAGE_CW_DETECT and STAGE_CW_DECODE.  A stage runs on a channel when the chain's switch for it
        is on and the channel's bit is set; a channel whose bit is clear is processed as with the stage switched off, and
        the stage's memory for it stays as it was.  STAGE_CW_DECODE needs STAGE_CW_DETECT.  None removes the map: every
        stage on every channel.  Configuration, like the output map: in no checkpoint, kept across reset() / set_state()
        / CalcFilters(); FFT_LENGTH 512."""
        if stages is None:
            check(self._lib.t41rx_set_stage_map(self._ctx, None, 0))
            return
        m = int_table(stages, np.uint32, None, "stages must be a 1-d array of n_channels STAGE_* masks, got %r %s")
        check(self._lib.t41rx_set_stage_map(self._ctx, ptr(m, U32P), int(m.size)))

    @property
    def stage_map(self):
        """the stage map as a uint32 array [n_channels] of STAGE_* masks (a copy), or None with no map set"""
        m = np.zeros(self.n_channels, np.uint32)
        return m if value(self._lib.t41rx_get_stage_map(self._ctx, ptr(m, U32P), self.n_channels)) > 0 else None

    def set_param_sets(self, sets, set_of_channel=None, stages=False):
        """Receiver groups (t41rx_set_param_sets): the context's own parameters are set 0, sets[i] becomes set i + 1, and
        channel c is processed exactly as a chain created with set set_of_channel[c] would process it.  sets: a sequence
        of t41rx_params, or of dicts of changes against set 0 (dict(mode=DEMOD_LSB, FLoCut=-3000, FHiCut=-200)).  Which
        sets may share a chain is one rule, param_sets_compatible().  None removes the sets.  Configuration, like the
        input map: in no checkpoint, kept across reset() / set_state(); CalcFilters() changes set 0.
        stages=True loads them next to the chain-splitting stages (t41rx_set_param_sets_ex with T41RX_SETS_STAGES): the
        equalizer, noise reduction / notch, the blanker and the CW stages then run with sets loaded, every channel with
        its own set's values; without it sets and those stages refuse each other."""
        if stages not in (False, True, 0, 1):
            raise ValueError("stages must be False or True, got %r" % (stages,))
        if sets is None:
            if set_of_channel is not None:
                raise ValueError("set_of_channel goes with sets: pass both, or None to remove the sets")
            check(self._lib.t41rx_set_param_sets(self._ctx, None, 0, None, 0))
            return
        if set_of_channel is None:
            raise ValueError("set_of_channel must be given with sets: n_channels=%d set numbers in [0, %d]" % (self.n_channels, len(sets)))
        arr = (Params * max(len(sets), 1))()
        for i, s in enumerate(sets):
            if isinstance(s, Params):
                arr[i] = s
            elif isinstance(s, dict):
                arr[i] = with_fields(Params.from_buffer_copy(self.params), "t41rx_params", s)
            else:
                raise ValueError("sets[%d] must be a t41rx_params or a dict of changes against set 0, got %s" % (i, type(s).__name__))
        m = int_table(set_of_channel, np.int32, None, "set_of_channel must be a 1-d array of int32 set numbers, got %r %s")
        if stages:
            check(self._lib.t41rx_set_param_sets_ex(self._ctx, arr, len(sets), ptr(m, I32P), int(m.size), SETS_STAGES))
        else:
            check(self._lib.t41rx_set_param_sets(self._ctx, arr, len(sets), ptr(m, I32P), int(m.size)))

    @property
    def param_sets_stages(self):
        """True when the loaded parameter sets were loaded with stages=True (t41rx_get_param_sets_flags); False with plain
        sets or none"""
        return bool(value(self._lib.t41rx_get_param_sets_flags(self._ctx)) & SETS_STAGES)

    @property
    def param_sets(self):
        """the extra parameter sets 1..K as a list of t41rx_params (copies); empty without sets"""
        k = value(self._lib.t41rx_get_param_sets(self._ctx, None, 0, None, 0))
        arr = (Params * max(k, 1))()
        value(self._lib.t41rx_get_param_sets(self._ctx, arr, k, None, 0))
        return [Params.from_buffer_copy(arr[i]) for i in range(k)]

    @property
    def set_of_channel(self):
        """the channels' set numbers as an int32 array [n_channels] (a copy), or None without sets"""
        m = np.zeros(self.n_channels, np.int32)
        return m if value(self._lib.t41rx_get_param_sets(self._ctx, None, 0, ptr(m, I32P), self.n_channels)) > 0 else None

    def set_noise_blanker(self, on):
        """NB_on (Process.cpp:873-876): the receive noise blanker on the demodulated audio, behind the noise reduction and
        the notch (t41rx_set_noise_blanker; 0 / 1, fft_length 512).  Kept across CalcFilters() / set_coeffs()."""
        check(self._lib.t41rx_set_noise_blanker(self._ctx, int(on)))

    @property
    def noise_blanker(self):
        return value(self._lib.t41rx_get_noise_blanker(self._ctx))

    def set_receive_eq_bands(self, coeffs):
        """The receive equalizer's band table (t41rx_set_receive_eq_bands): the firmware's EQ_Band1Coeffs ..
        EQ_Band14Coeffs as [14][4][5] or [14][20], {b0, b1, b2, a1, a2} per section with the a's negated.  Kept across
        CalcFilters() / set_coeffs(); the filter memories are not reset."""
        c = table(coeffs, np.float32, (14, 20), "receive-EQ band table must be [14][4][5] or [14][20], got %r", rows=True)
        check(self._lib.t41rx_set_receive_eq_bands(self._ctx, ptr(c)))

    def set_receive_eq(self, on, levels=None):
        """receiveEQFlag and EEPROMData.equalizerRec (Process.cpp:828-832, Filter.cpp:117-165): the receive equalizer on
        the demodulated audio, in front of the noise reduction, the notch and the noise blanker (t41rx_set_receive_eq;
        0 / 1, fft_length 512, a band table loaded first).  levels: 14 ints, or None to keep the current ones (100 each
        until set).  Kept across CalcFilters() / set_coeffs()."""
        lv = None if levels is None else table(levels, np.int32, (14,), "receive-EQ levels must be 14 ints, got %r")
        check(self._lib.t41rx_set_receive_eq(self._ctx, int(on), ptr(lv)))

    @property
    def receive_eq(self):
        """(on, levels): the receive equalizer's switch and its 14 levels"""
        lv = np.zeros(14, np.int32)
        return value(self._lib.t41rx_get_receive_eq(self._ctx, ptr(lv))), lv

    def set_receive_eq_map(self, levels):
        """Receiver groups (t41rx_set_receive_eq_map): levels[c] is channel c's EEPROMData.equalizerRec, [n_channels][14]
        ints.  Where the equalizer runs on channel c -- the switch of set_receive_eq() on, and STAGE_EQ in the stage map
        or no stage map -- the channel is processed exactly as a chain with set_receive_eq(1, levels[c]) would process
        it.  The switch, the band table, the stage map and the chain's own levels stay what they are.  None removes the
        map.  Configuration, like the stage map: in no checkpoint, kept across reset() / set_state() / CalcFilters();
        FFT_LENGTH 512."""
        if levels is None:
            check(self._lib.t41rx_set_receive_eq_map(self._ctx, None, 0))
            return
        a = np.asarray(levels)
        if a.ndim != 2 or a.shape[1] != 14 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("levels must be an [n_channels][14] array of ints, got %r %s" % (a.shape, a.dtype))
        m = int_table(a.reshape(-1), np.int32, None, "levels must fit int32, got %r %s")
        check(self._lib.t41rx_set_receive_eq_map(self._ctx, ptr(m, I32P), int(a.shape[0])))

    @property
    def receive_eq_map(self):
        """the equalizer level map as an int32 array [n_channels][14] (a copy), or None with no map set"""
        m = np.zeros((self.n_channels, 14), np.int32)
        return m if value(self._lib.t41rx_get_receive_eq_map(self._ctx, ptr(m, I32P), self.n_channels)) > 0 else None

    def set_cw_tables(self, audio_filters=None, decode_fir=None):
        """The CW receive tables (t41rx_set_cw_tables): audio_filters = the firmware's CW_AudioFilterCoeffs1..5 as
        [5][6][5] or [5][30], {b0, b1, b2, a1, a2} per section with the a's negated; decode_fir = CW_Filter_Coeffs2, 64
        taps.  None keeps what is loaded.  Kept across CalcFilters() / set_coeffs(); no memory is reset."""
        f = d = None
        if audio_filters is not None:
            f = table(audio_filters, np.float32, (5, 30), "CW filter tables must be [5][6][5] or [5][30], got %r", rows=True)
        if decode_fir is not None:
            d = table(decode_fir, np.float32, (64,), "CW decode FIR must be 64 taps, got %r")
        check(self._lib.t41rx_set_cw_tables(self._ctx, ptr(f), ptr(d)))

    def set_cw_filter(self, CWFilterIndex):
        """CWFilterIndex (Process.cpp:882-912): 0 .. 4 = the 0.8 / 1.0 / 1.3 / 1.8 / 2.0 kHz narrow audio filter behind the
        noise blanker, 5 = off (the default).  Runs only while xmtMode == CW_MODE; fft_length 512; the filter tables
        loaded first.  Kept across CalcFilters() / set_coeffs()."""
        check(self._lib.t41rx_set_cw_filter(self._ctx, int(CWFilterIndex)))

    @property
    def cw_filter(self):
        return value(self._lib.t41rx_get_cw_filter(self._ctx))

    def set_cw_filter_map(self, filter_of_channel):
        """Receiver groups (t41rx_set_cw_filter_map): filter_of_channel[c] is channel c's CWFilterIndex, 0 .. 4 or 5 = off.
        While the map is loaded channel c is processed exactly as the same channel of a chain with
        set_cw_filter(filter_of_channel[c]) would be: its audio, the five filter memories (only the selected one
        advances), the interpolator memories.  The chain's own index is kept, not consulted, and still what cw_filter
        returns.  None removes the map.  An index below 5 needs the filter tables and cannot stand next to parameter
        sets.  Configuration, like the stage map: in no checkpoint, kept across reset() / set_state() / CalcFilters();
        FFT_LENGTH 512."""
        if filter_of_channel is None:
            check(self._lib.t41rx_set_cw_filter_map(self._ctx, None, 0))
            return
        m = int_table(filter_of_channel, np.int32, None, "filter_of_channel must be a 1-d array of n_channels CWFilterIndex values (0 .. 5), got %r %s")
        check(self._lib.t41rx_set_cw_filter_map(self._ctx, ptr(m, I32P), int(m.size)))

    @property
    def cw_filter_map(self):
        """the CW filter map as an int32 array [n_channels] (a copy), or None with no map set"""
        m = np.zeros(self.n_channels, np.int32)
        return m if value(self._lib.t41rx_get_cw_filter_map(self._ctx, ptr(m, I32P), self.n_channels)) > 0 else None

    def set_nr_map(self, nr_of_channel, notch_of_channel=None):
        """Receiver groups (t41rx_set_nr_map): nr_of_channel[c] is channel c's nrOptionSelect (0 off, 1 Kim, 2 spectral,
        3 LMS) and notch_of_channel[c] its ANR_notchOn (0 / 1).  While the map is loaded channel c is processed exactly
        as the same channel of a chain with CalcFilters(nrOptionSelect=nr_of_channel[c], ANR_notchOn=notch_of_channel[c])
        would be: its audio, Xanr()'s record, the Kim / spectral record -- the stale statics of a kind that changes
        between two calls included.  A function runs where the channel's entry asks for it and STAGE_NR is in the stage
        map or no stage map is set; a channel with 0 / 0 is not touched.  The chain's own two values are kept, not
        consulted, and still what params returns; NR_alpha, NR_beta, NR_PSI and the pass band stay the chain's.
        set_nr_map(None) removes the map.  A non-zero entry cannot stand next to parameter sets; an entry 2 needs a pass
        band the spectral function accepts.  Configuration, like the stage map: in no checkpoint, kept across reset() /
        set_state() / CalcFilters(); FFT_LENGTH 512."""
        if nr_of_channel is None:
            if notch_of_channel is not None:
                raise ValueError("notch_of_channel goes with nr_of_channel: pass both, or None to remove the map")
            check(self._lib.t41rx_set_nr_map(self._ctx, None, None, 0))
            return
        if notch_of_channel is None:
            raise ValueError("notch_of_channel must be given with nr_of_channel: n_channels=%d values 0 / 1" % self.n_channels)
        k = int_table(nr_of_channel, np.int32, None, "nr_of_channel must be a 1-d array of n_channels nrOptionSelect values (0 .. 3), got %r %s")
        t = int_table(notch_of_channel, np.int32, (int(k.size),), "notch_of_channel must be a 1-d array of ANR_notchOn values (0 / 1) as long as nr_of_channel, got %r %s")
        check(self._lib.t41rx_set_nr_map(self._ctx, ptr(k, I32P), ptr(t, I32P), int(k.size)))

    @property
    def nr_map(self):
        """the noise-reduction map as two int32 arrays [n_channels] (copies), (nr_of_channel, notch_of_channel), or None
        with no map set"""
        k, t = np.zeros(self.n_channels, np.int32), np.zeros(self.n_channels, np.int32)
        return (k, t) if value(self._lib.t41rx_get_nr_map(self._ctx, ptr(k, I32P), ptr(t, I32P), self.n_channels)) > 0 else None

    def set_cw_detector(self, on, max_frames=1):
        """decoderFlag (DoCWReceiveProcessing(), CWProcessing.cpp:322-373).  on = 1 allocates and returns the result
        tensor, float32 CUDA [n_channels, max_frames, 4]; a process call of n <= max_frames frames fills its first
        n_channels * n * 4 floats as [n_channels][n][corrResultL, goertzelMagnitude, aveCorrResult, combinedCoeff]
        (cw_results(n) is that view).  on = 0 switches the detector off and returns None.  The `combinedCoeff > 50`
        decision and the Morse decoder behind it are set_cw_decoder()'s.  Runs only while xmtMode == CW_MODE; fft_length 512; the
        decode FIR loaded first.  Kept across CalcFilters() / set_coeffs()."""
        return self._result_stage("_cw", self._lib.t41rx_set_cw_detector, on, max_frames, ("float32", None, 4))

    @property
    def cw_detector(self):
        return value(self._lib.t41rx_get_cw_detector(self._ctx))

    def cw_results(self, n_frames):
        """the detector's results of the last process call of n_frames frames: a view [n_channels, n_frames, 4]"""
        return self._first_frames(kept(self, "_cw", "the CW detector is off"), n_frames, 4)

    def set_cw_decode_tree(self, tree):
        """The Morse decoder's bigMorseCodeTree (CWProcessing.cpp:540; t41rx_set_cw_decode_tree): 129 bytes, as bytes,
        str or uint8 array.  The library has no table of its own.  Kept across CalcFilters() / set_coeffs()."""
        if isinstance(tree, str):
            tree = tree.encode("ascii")
        t = np.ascontiguousarray(np.frombuffer(tree, np.uint8) if isinstance(tree, (bytes, bytearray)) else np.asarray(tree, dtype=np.uint8))
        check(self._lib.t41rx_set_cw_decode_tree(self._ctx, ptr(t), int(t.size)))

    def set_cw_decoder(self, on, max_frames=1):
        """The Morse decoder behind the detector (DoCWDecoding(), CWProcessing.cpp:365-371, :519-815;
        t41rx_set_cw_decoder).  on = 1 allocates and returns the text tensor, int32 CUDA [n_channels, max_frames, 2]; a
        process call of n <= max_frames frames fills its first n_channels * n * 2 words as [n_channels][n][character
        code or 0, ditLength behind the frame] (cw_text(n) is that view).  on = 0 switches it off and returns None.  Runs
        exactly when the detector runs (xmtMode == CW_MODE, set_cw_detector(1)); fft_length 512; the tree loaded first.
        Kept across CalcFilters() / set_coeffs()."""
        return self._result_stage("_cw_text", self._lib.t41rx_set_cw_decoder, on, max_frames, ("int32", None, 2))

    @property
    def cw_decoder(self):
        return value(self._lib.t41rx_get_cw_decoder(self._ctx))

    def cw_text(self, n_frames):
        """the decoder's words of the last process call of n_frames frames: a view [n_channels, n_frames, 2]"""
        return self._first_frames(kept(self, "_cw_text", "the CW decoder is off"), n_frames, 2)

    def set_cw_clock(self, t0_ms=0, num=32, den=3):
        """The decoder's clock (t41rx_set_cw_clock): millis(n) = t0_ms + floor(n * num / den) for the channel's n-th
        decoder frame; the default is one frame of 2048 samples at 192 kS/s.  From the next call; n is not touched."""
        check(self._lib.t41rx_set_cw_clock(self._ctx, int(t0_ms), int(num), int(den)))

    def reset_cw_histograms(self, channels=None):
        """ResetHistograms() (CWProcessing.cpp:501-517), what the firmware runs at every retune, on the channels whose
        entry is non-zero (None: all): both histograms' words 0 .. 749 and the scalars it names, nothing else."""
        check(self._lib.t41rx_reset_cw_histograms(self._ctx, *channel_mask(channels, self.n_channels)))

    # -- FT8 receive up to the waterfall ------------------------------------------------------
    def set_ft8_tables(self, window=None, mag_db=None):
        """The FT8 tables (t41rx_set_ft8_tables): window = ft_blackman_i(i, 2048), 2048 floats; mag_db[m] = 10.0 *
        log((float)(10 * m) + 0.1), 16385 floats.  None, None computes both with ft8_tables().  The library has no table of
        its own.  Kept across CalcFilters() / set_coeffs()."""
        if window is None and mag_db is None:
            window, mag_db = ft8_tables()
        if window is None or mag_db is None:
            raise ValueError("window and mag_db must both be given or both be None")
        w, m = table_pair(window, mag_db, (2048,), (16385,), "FT8 tables must be 2048 and 16385 floats, got %r and %r")
        check(self._lib.t41rx_set_ft8_tables(self._ctx, ptr(w), ptr(m)))

    def set_ft8(self, on, max_frames=1):
        """FT8 receive on a USB context (Process.cpp:627-686, ft8.cpp:153-268; t41rx_set_ft8): the audio collector, the
        two q15 FFTs per 15 frames and the waterfall rows, with the firmware's slot timing.  on = 1 allocates and returns
        (power, status): uint8 CUDA [n_channels, 2, 92 * 1472], the two halves of export_fft_power, and int32 CUDA
        [n_channels, max_frames, 4]; a process call of n <= max_frames <= 1380 frames fills the status' first n_channels *
        n * 4 words as [n_channels][n][FT_8_counter, ft8_flag, 0 or 1 + the half completed in this frame, dataLoop]
        (ft8_status(n) is that view).  on = 0 switches it off and returns None.  Nothing is collected before ft8_sync().
        fft_length 512, mode USB; the tables loaded first.  Kept across CalcFilters() / set_coeffs().
        With an FT8 map (set_ft8_map) both tensors hold ft8_rows rows in place of n_channels."""
        return self._result_stage("_ft8", self._lib.t41rx_set_ft8, on, max_frames, ("uint8", 2, 92 * 1472), ("int32", None, 4), rows=self.ft8_rows)

    def set_ft8_map(self, row_of_channel, n_rows=None):
        """Receiver groups (t41rx_set_ft8_map): FT8 receive runs on channel c only when row_of_channel[c] >= 0, and then
        writes row row_of_channel[c] of the power and status tensors, which hold n_rows rows -- [n_rows, 2, 92 * 1472] and
        [n_rows, max_frames, 4]; a channel with -1 is processed as with FT8 off and its FT8 memory stays as it was.  No row
        may be named twice; n_rows defaults to max + 1 (at least 1).  ft8_audio() then takes [n_rows, 128 * k], and
        ft8_decode() without a waterfall takes and returns rows.  None removes the map.  While FT8 receive is on the rows
        cannot change: set_ft8(0), set_ft8_map(...), set_ft8(1, ...); at equal n_rows the map may change between any two
        calls.  Configuration, like the stage map: in no checkpoint, kept across reset() / set_state() / CalcFilters();
        FFT_LENGTH 512."""
        if row_of_channel is None:
            check(self._lib.t41rx_set_ft8_map(self._ctx, None, 0, 0))
            self._ft8_rows = None
            return
        m = int_table(row_of_channel, np.int32, None, "row_of_channel must be a 1-d array of int32 row numbers (-1: no FT8 receive), got %r %s")
        if n_rows is None:
            n_rows = max(int(m.max()) + 1, 1) if m.size else 1
        check(self._lib.t41rx_set_ft8_map(self._ctx, ptr(m, I32P), int(m.size), int(n_rows)))
        self._ft8_rows = int(n_rows)

    @property
    def ft8_map(self):
        """the FT8 map as an int32 array [n_channels] (a copy, -1: not listed), or None with no map set"""
        m = np.zeros(self.n_channels, np.int32)
        return m if value(self._lib.t41rx_get_ft8_map(self._ctx, ptr(m, I32P), self.n_channels, None)) > 0 else None

    @property
    def ft8_rows(self):
        """rows of the FT8 power and status tensors and of ft8_audio()'s pcm: the FT8 map's n_rows, or n_channels with no map"""
        rows = getattr(self, "_ft8_rows", None)  # (kept here and read as audio_rows is: the shape checks make no call into the library)
        return self.n_channels if rows is None else rows

    @property
    def ft8(self):
        return value(self._lib.t41rx_get_ft8(self._ctx))

    def ft8_status(self, n_frames):
        """the FT8 status words of the last process call of n_frames frames: a view [ft8_rows, n_frames, 4]"""
        return self._first_frames(kept(self, "_ft8", "FT8 receive is off")[1], n_frames, 4, rows=self.ft8_rows)

    def ft8_power(self):
        """export_fft_power, uint8 CUDA [ft8_rows, 2, 92 * 1472]: the half a status word reported complete holds the
        finished slot, [92 blocks][time_sub 0 / 512][freq_sub 0 / 1][368]"""
        return kept(self, "_ft8", "FT8 receive is off")[0]

    def set_ft8_clock(self, t0_ms=0, num=32, den=3):
        """The slot timing's clock (t41rx_set_ft8_clock): millis(n) = t0_ms + floor(n * num / den) for the channel's n-th
        FT8 frame; the default is one frame of 2048 samples at 192 kS/s.  From the next call; n is not touched."""
        check(self._lib.t41rx_set_ft8_clock(self._ctx, int(t0_ms), int(num), int(den)))

    def ft8_sync(self, channels=None):
        """auto_sync_FT8()'s success branch (ft8.cpp:133-136) on the channels whose entry is non-zero (None: all):
        start_time = millis(n), ft8_flag = 1, FT_8_counter = 0, syncFlag = true.  The caller's clock decides when."""
        check(self._lib.t41rx_ft8_sync(self._ctx, *channel_mask(channels, self.n_channels)))

    def ft8_state(self):
        """the FT8 memory's record (t41rx_ft8_get_state): 8 int32 of header, then [n_channels][3088] int32 (uint8 array)"""
        return get_blob(self._lib.t41rx_ft8_get_state, self._ctx, self._lib.t41rx_ft8_state_bytes(self._ctx))

    def set_ft8_state(self, buf):
        set_blob(self._lib.t41rx_ft8_set_state, self._ctx, buf)

    # -- FT8 from 12 kS/s audio (DEMOD_FT8_WAV) ----------------------------------------------
    def ft8_audio(self, pcm):
        """The collector of DEMOD_FT8_WAV (Process.cpp:278-335; t41rx_ft8_audio_*) on 12 kS/s audio, without the receive
        chain: pcm [ft8_rows, 128 * k] (n_channels rows without an FT8 map), int16 (a WAV file's samples, taken as they are) or float32 (through
        arm_float_to_q15), a CUDA tensor (default stream, no synchronisation) or a numpy array.  Always channel-major:
        the input map and the buffer layout do not apply.  Needs set_ft8(1, max_frames >= k); writes the same power halves
        and returns the call's status words, the view ft8_status(k)."""
        host = isinstance(pcm, np.ndarray)
        if host:
            if pcm.dtype not in (np.int16, np.float32):
                raise ValueError("pcm must be int16 or float32, got %s" % pcm.dtype)
            pcm = np.ascontiguousarray(pcm)
            q15 = pcm.dtype == np.int16
        else:
            import torch
            if not (isinstance(pcm, torch.Tensor) and cuda_tensor(pcm, (torch.int16, torch.float32))):
                raise ValueError("pcm must be a contiguous int16 or float32 CUDA tensor or numpy array")
            if pcm.device.index != self.device:
                raise ValueError("pcm lives on another device than this RxChain")
            q15 = pcm.dtype == torch.int16
        k = self._ft8_audio_frames(tuple(pcm.shape))
        lib = self._lib
        fn = ((lib.t41rx_ft8_audio_host_q15 if q15 else lib.t41rx_ft8_audio_host) if host
              else (lib.t41rx_ft8_audio_device_q15 if q15 else lib.t41rx_ft8_audio_device))
        check(fn(self._ctx, ptr(pcm), k))  # (the device entries run on the default stream)
        return self.ft8_status(k)

    def _ft8_audio_frames(self, shape):
        rows = self.ft8_rows
        if len(shape) != 2 or shape[0] != rows or shape[1] < 128 or shape[1] % 128:
            raise ValueError("pcm must be [%s = %d, 128 * k], got %r" % ("n_channels" if rows == self.n_channels else "ft8_rows", rows, tuple(shape)))
        kept(self, "_ft8", "FT8 receive is off")
        return shape[1] // 128

    def ft8_audio_begin(self, channels=None):
        """setupFT8Wav() (ft8.cpp:1372) on the channels whose entry is non-zero (None: all): FT_8_counter = 0, nothing else"""
        check(self._lib.t41rx_ft8_audio_begin(self._ctx, *channel_mask(channels, self.n_channels)))

    def ft8_audio_end(self, channels=None):
        """the WAV mode's exit (Process.cpp:339-342) on the channels whose entry is non-zero (None: all): syncFlag = 0,
        FT_8_counter = 0, ft8_flag = 0, nothing else"""
        check(self._lib.t41rx_ft8_audio_end(self._ctx, *channel_mask(channels, self.n_channels)))

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
        check(self._lib.t41rx_set_ft8_decode_tables(self._ctx, *[ptr(a) for a in arrs]))

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
        log174 [n_channels, 20, 174] f32 and plain [n_channels, 20, 174] uint8.  With an FT8 map (set_ft8_map) and
        waterfall None the decode is by row: select, the records and the taps are [ft8_rows, ...]."""
        import torch
        from . import ft8 as F
        n = self.ft8_rows if waterfall is None else self.n_channels
        dev = cuda(self.device)
        sel = None
        if select is not None:
            sel = np.asarray(select)
            if sel.shape != (n,):
                raise ValueError("select must have %s = %d entries, got %r" % ("n_channels" if n == self.n_channels else "ft8_rows", n, sel.shape))
            if ((sel < -128) | (sel > 127)).any():
                raise ValueError("select does not fit int8")
            sel = np.ascontiguousarray(sel, dtype=np.int8)
        wf, stride = None, 0
        if waterfall is not None:
            if not (isinstance(waterfall, torch.Tensor) and waterfall.is_cuda and waterfall.dtype == torch.uint8 and waterfall.dim() == 2
                    and waterfall.shape[0] == n and waterfall.stride(1) == 1):
                raise ValueError("waterfall must be a uint8 CUDA tensor [n_channels, bytes per channel] with unit inner stride")
            need = F.SLOT_BYTES * (2 if sel is not None and (sel == 1).any() else 1)
            if waterfall.shape[1] < need:
                raise ValueError("waterfall rows hold %d bytes, the call reads %d" % (waterfall.shape[1], need))
            wf, stride = waterfall, int(waterfall.stride(0)) if n > 1 else int(waterfall.shape[1])
        res = torch.zeros(n, F.RESULT.itemsize, dtype=torch.uint8, device=dev)
        taps = None
        if debug:
            taps = (torch.zeros(n, F.MAX_CANDIDATES, 174, dtype=torch.float32, device=dev),
                    torch.zeros(n, F.MAX_CANDIDATES, 174, dtype=torch.uint8, device=dev))
            check(self._lib.t41rx_set_ft8_decode_debug(self._ctx, ptr(taps[0]), ptr(taps[1])))
        try:
            check(self._lib.t41rx_ft8_decode_device(self._ctx, ptr(wf), stride, ptr(sel), n, ptr(res), _args.stream_of(self.device)))
            out = res.cpu().numpy().view(F.RESULT).reshape(n)
            if debug:
                return out, taps[0].cpu().numpy(), taps[1].cpu().numpy()
            return out
        finally:
            if debug:
                torch.cuda.synchronize(res.device)
                check(self._lib.t41rx_set_ft8_decode_debug(self._ctx, None, None))

    def get_state(self):
        return get_blob(self._lib.t41rx_get_state, self._ctx, self._lib.t41rx_state_bytes(self._ctx))

    def set_state(self, buf):
        set_blob(self._lib.t41rx_set_state, self._ctx, buf)

    def state_records(self, buf=None):
        """the per-channel records of a checkpoint (default: a fresh one) as float32 [n_channels, floats]"""
        buf = self.get_state() if buf is None else np.ascontiguousarray(buf, dtype=np.uint8)
        per = int(buf[:STATE_HEADER_BYTES].view(np.int32)[4])  # floats per channel of the path's section (the side stages' follow it)
        return buf[STATE_HEADER_BYTES:STATE_HEADER_BYTES + 4 * per * self.n_channels].view(np.float32).reshape(self.n_channels, per)

    def _result_stage(self, attr, entry, on, max_frames, *tensors, rows=None):
        """The switch of a stage that owns its result tensors, each (dtype, dimensions behind n_channels -- or behind `rows`,
        for a stage whose results have a row map --) with None for max_frames.  Off: tells the library and drops them.  On: allocates them zeroed, hands them to entry(ctx, on,
        pointers ..., max_frames) and keeps them alive in self.<attr>; a refused call leaves self.<attr> as it was."""
        if not on:
            check(entry(self._ctx, 0, *[None] * len(tensors), 0))
            setattr(self, attr, None)
            return None
        import torch
        if int(max_frames) < 1:
            raise ValueError("max_frames must be >= 1")
        ts = tuple(torch.zeros((self.n_channels if rows is None else int(rows),) + tuple(int(max_frames) if d is None else d for d in dims),
                               dtype=getattr(torch, dtype), device=cuda(self.device)) for dtype, *dims in tensors)
        check(entry(self._ctx, int(on), *[ptr(t) for t in ts], int(max_frames)))
        keep = ts[0] if len(ts) == 1 else ts
        setattr(self, attr, keep)  # keep alive
        return keep

    def _first_frames(self, t, n_frames, width, rows=None):
        """the part of a result tensor [n_channels, max_frames, width] a call of n_frames frames filled, as [n_channels, n_frames, width]
        (rows: the leading dimension of a stage whose results have a row map)"""
        rows = self.n_channels if rows is None else int(rows)
        return t.view(-1)[:rows * int(n_frames) * width].view(rows, int(n_frames), width)

    # -- the hot path ----------------------------------------------------------------------
    def ProcessIQData(self, float_buffer_L, float_buffer_R, out=None):
        """One ProcessIQData() per channel (or several consecutive ones).

        torch CUDA tensors [n_channels, n_frames*frame_len] (float32, contiguous) run on the
        current torch stream without synchronising and return a tensor; numpy arrays go
        through the host-pointer entry point and return a numpy array.  The result (and `out`) holds
        audio_frame_len samples per channel and frame: frame_len, or 256 after set_audio_rate(24000).
        """
        return self._process(float_buffer_L, float_buffer_R, out, "float32", F32P, self._lib.t41rx_process_host, self._lib.t41rx_process_device,
                             "I/Q must be contiguous float32 CUDA tensors", "I/Q live on another device than this RxChain")

    def ProcessIQData_q15(self, Q_in_L, Q_in_R, out=None):
        """The same on the firmware's wire format (Process.cpp:102-111, 936-937): int16 (q15) blocks
        of the L and R record queues in -- I is taken from the R queue, Q from the L queue, as the
        firmware does -- and the q15 samples handed to Q_out_L.play() out.
        torch CUDA int16 tensors or numpy int16 arrays, [n_channels, n_frames*frame_len]."""
        return self._process(Q_in_L, Q_in_R, out, "int16", C.c_void_p, self._lib.t41rx_process_host_q15, self._lib.t41rx_process_device_q15,
                             "Q_in_L/Q_in_R must be contiguous int16 CUDA tensors", "the queues live on another device than this RxChain")

    def _process(self, a, b, out, dtype, ptype, host_entry, device_entry, not_cuda, elsewhere):
        """ProcessIQData() and ProcessIQData_q15(): numpy arrays are converted to dtype and go to the host entry, tensors
        must be of dtype already and go to the device entry with the current stream; the messages are the caller's"""
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a, dtype=dtype)
            b = np.ascontiguousarray(b, dtype=dtype)
            nfr = self._check_shape(a.shape, b.shape)
            audio = np.empty(self._out_shape(nfr), a.dtype) if out is None else self._check_out_numpy(out, a, nfr)
            check(host_entry(self._ctx, ptr(a, ptype), ptr(b, ptype), ptr(audio, ptype), nfr))
            return audio
        import torch
        want = getattr(torch, dtype)
        if not (cuda_tensor(a, want) and cuda_tensor(b, want)):
            raise ValueError(not_cuda)
        if a.device.index != self.device or b.device.index != self.device:
            raise ValueError(elsewhere)
        nfr = self._check_shape(tuple(a.shape), tuple(b.shape))
        audio = torch.empty(self._out_shape(nfr), dtype=want, device=a.device) if out is None else self._check_out_torch(out, a, nfr)
        check(device_entry(self._ctx, a.data_ptr(), b.data_ptr(), audio.data_ptr(), nfr, _args.stream_of(self.device)))
        return audio

    def _side_tensors(self, *sides):
        """validate side-output tensors, each (tensor or None, floats per channel and frame, name); returns their pointers
        and the frames the smallest of them has room for (0 if none is given)"""
        ptrs, frames = [], []
        for t, per_frame, what in sides:
            if t is not None:
                import torch
                if not cuda_tensor(t, torch.float32, self.device):
                    raise ValueError("%s must be a contiguous float32 CUDA tensor on device %d" % (what, self.device))
                frames.append(t.numel() // (self.n_channels * per_frame))
                if frames[-1] < 1:
                    raise ValueError("%s holds less than one frame (%d floats per channel and frame)" % (what, per_frame))
            ptrs.append(ptr(t))
        return ptrs, min(frames) if frames else 0

    def set_debug_taps(self, post_nco=None, dec=None, demod=None):
        """stage taps (torch CUDA float32 tensors or None): post_nco [n_channels, n_frames*2*frame_len],
        dec [n_channels, n_frames*fft_length], demod [n_channels, n_frames*fft_length/2].  Calls with
        more frames than the smallest of them holds are refused."""
        N = self.params.fft_length
        ptrs, frames = self._side_tensors((post_nco, 2 * self.frame_len, "post_nco"), (dec, N, "dec"), (demod, N // 2, "demod"))
        check(self._lib.t41rx_set_debug_taps(self._ctx, *ptrs, frames))
        self._taps = (post_nco, dec, demod)  # keep alive

    def set_audio_spectrum(self, spect=None, maxima=None):
        """the display by-product of the path (Process.cpp:550-570): torch CUDA float32 tensors
        [n_channels, n_frames, 1024] and [n_channels, n_frames, 3], or None/None to switch it off"""
        ptrs, frames = self._side_tensors((spect, 1024, "spect"), (maxima, 3, "maxima"))
        check(self._lib.t41rx_set_audio_spectrum(self._ctx, *ptrs, frames))
        self._spect = (spect, maxima)  # keep alive

    def set_display_spectrum(self, spec=None, spec_old=None, spectrumZoom=1):
        """the display FFT (CalcZoom1Magn / ZoomFFTExe, FFT.cpp:67-251): torch CUDA float32 tensors
        [n_channels, n_frames, 512] for FFT_spec and FFT_spec_old, or None/None to switch it off"""
        ptrs, frames = self._side_tensors((spec, 512, "spec"), (spec_old, 512, "spec_old"))
        check(self._lib.t41rx_set_display_spectrum(self._ctx, *ptrs, int(spectrumZoom), frames))
        self._disp = (spec, spec_old)  # keep alive

    # -- the panadapter stage ------------------------------------------------------------------
    PANADAPTER_ROWS = (("pixel", "int16", 512), ("y_new", "int16", 512), ("y_old", "int16", 512), ("waterfall", "uint16", 512),
                       ("spec", "float32", 512), ("audio_spect", "float32", 1024), ("smeter", "float32", 4))

    def set_panadapter_tables(self, gradient):
        """The waterfall's colour words gradient[] (Display.cpp:148-161; t41rx_set_panadapter_tables): 117 uint16.  The
        library has no table of its own."""
        g = int_table(gradient, np.uint16, None, "gradient must be a 1-d array of uint16 colour words, got %r %s")
        check(self._lib.t41rx_set_panadapter_tables(self._ctx, ptr(g, U16P), int(g.size)))

    def set_panadapter(self, on=True, spectrumZoom=0, currentScale=1, pixel_offset=0, spectrumNoiseFloor=panadapter.SPECTRUM_NOISE_FLOOR,
                       update_period=panadapter.UPDATE_PERIOD, update_phase=0, max_rows=1, outputs=None):
        """ShowSpectrum()'s pixels and waterfall row and DrawSmeterBar()'s dBm as a stage of the path
        (t41rx_set_panadapter), at the firmware's cadence: frame n of the stage's count is an update frame when n %
        update_period == update_phase (panadapter.rows_of_call()).  outputs: None allocates every row buffer, a list of
        names of PANADAPTER_ROWS allocates those, a dict name -> CUDA tensor [n_channels, max_rows, width] uses the
        caller's; what is left out is not written.  Returns the dict of row buffers: a call with k update frames writes
        rows 0 .. k-1 of every channel (panadapter_status()).  on = False switches the stage off and returns None.
        Starts the stage's memory and its frame counter from power-on.  fft_length 512; the colour table loaded first.
        With a panadapter map (set_panadapter_map) every buffer holds panadapter_rows rows in place of n_channels."""
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
            shape = (self.panadapter_rows, int(max_rows), width)
            t = outputs[name] if isinstance(outputs, dict) else None
            if t is None:  # (uint16: allocated as int16 and viewed, the type torch fills on every build)
                t = torch.zeros(shape, dtype=torch.int16 if dt == torch.uint16 else dt, device=cuda(self.device)).view(dt)
            elif not (cuda_tensor(t, dt, self.device) and tuple(t.shape) == shape):
                raise ValueError("%s must be a contiguous %s CUDA tensor of shape %r on device %d" % (name, dt, shape, self.device))
            bufs[name] = t
        out = _lib.PanadapterOut(**{name: ptr(t) for name, t in bufs.items()})
        self._pan = None
        check(self._lib.t41rx_set_panadapter(self._ctx, 1, int(spectrumZoom), int(currentScale), int(pixel_offset), int(spectrumNoiseFloor),
                                             int(update_period), int(update_phase), C.byref(out), int(max_rows)))
        self._pan = bufs  # keep alive
        return bufs

    def set_panadapter_map(self, row_of_channel, n_rows=None):
        """Receiver groups (t41rx_set_panadapter_map): the panadapter stage runs on channel c only when row_of_channel[c]
        >= 0, and then writes row row_of_channel[c] of the seven row buffers, which hold n_rows rows -- [n_rows, max_rows,
        width]; a channel with -1 is processed as with the panadapter off: no tap, audioMaxSquaredAve and its panadapter
        memory stay as they were.  The beacon monitor behind it runs on the listed channels only (its snr, events and
        record stay by channel).  Each listed channel's dbm takes RFgain / rfGainAllBands from its own parameter set.  No
        row may be named twice; n_rows defaults to max + 1 (at least 1).  None removes the map.  While the panadapter is
        on the rows cannot change: set_beacon(False), set_panadapter(False), set_panadapter_map(...), set_panadapter(...),
        set_beacon(...); at equal n_rows the map may change between any two calls.  Configuration, like the stage map: in
        no checkpoint, kept across reset() / set_state() / CalcFilters(); FFT_LENGTH 512."""
        if row_of_channel is None:
            check(self._lib.t41rx_set_panadapter_map(self._ctx, None, 0, 0))
            return
        m = int_table(row_of_channel, np.int32, None, "row_of_channel must be a 1-d array of int32 row numbers (-1: no panadapter), got %r %s")
        if n_rows is None:
            n_rows = max(int(m.max()) + 1, 1) if m.size else 1
        check(self._lib.t41rx_set_panadapter_map(self._ctx, ptr(m, I32P), int(m.size), int(n_rows)))

    @property
    def panadapter_map(self):
        """the panadapter map as an int32 array [n_channels] (a copy, -1: not listed), or None with no map set"""
        m = np.zeros(self.n_channels, np.int32)
        return m if value(self._lib.t41rx_get_panadapter_map(self._ctx, ptr(m, I32P), self.n_channels, None)) > 0 else None

    @property
    def panadapter_rows(self):
        """rows of the panadapter's row buffers: the panadapter map's n_rows, or n_channels with no map"""
        return value(self._lib.t41rx_panadapter_rows(self._ctx))  # (asked, not kept: a host call without a sync)

    def set_panadapter_levels(self, noise_floor=None, gain_correction=None, attenuator=0):
        """currentNoiseFloor[currentBand] (ints) and bands[currentBand].gainCorrection (floats) per channel, None = zeros,
        and `attenuator` (t41rx_set_panadapter_levels).  From the next process call."""
        nf = gc = None
        if noise_floor is not None:
            nf = int_table(noise_floor, np.int32, (self.n_channels,), "noise_floor must be n_channels = %d int32 values, got %%r %%s" % self.n_channels)
        if gain_correction is not None:
            gc = table(gain_correction, np.float32, (self.n_channels,), "gain_correction must be n_channels = %d floats, got %%r" % self.n_channels)
        check(self._lib.t41rx_set_panadapter_levels(self._ctx, ptr(nf, I32P), ptr(gc, F32P), int(attenuator)))

    def panadapter_status(self):
        """(on, frame_counter, rows_written, first_row_frame): the stage's switch, its frame count behind the last process
        call, the rows that call wrote and the frame count of its row 0 (-1: none)"""
        n, k, f = C.c_int64(), C.c_int32(), C.c_int64()
        v = value(self._lib.t41rx_get_panadapter(self._ctx, C.byref(n), C.byref(k), C.byref(f)))
        return bool(v), n.value, k.value, f.value

    def set_panadapter_counter(self, n):
        """the stage's frame counter (t41rx_set_panadapter_counter), n >= 0"""
        check(self._lib.t41rx_set_panadapter_counter(self._ctx, int(n)))

    # -- the beacon monitor behind the panadapter ------------------------------------------------
    def set_beacon(self, on=True, mode=0, band=None, max_rows=None):
        """BeaconLoop()'s per-beacon SNR table as a stage behind the panadapter (Beacon.cpp:455-569; t41rx_set_beacon):
        one BeaconLoop() call per panadapter row on the row's dbm.  band: n_channels ints 0 .. 4, the one band each
        channel monitors.  mode 0 is the firmware's cycle, 1 records every beacon change.  on allocates and returns (snr,
        events): float32 CUDA [n_channels, 18], the channel's column of beaconSNR, kept across calls, and int32 CUDA
        [n_channels, max_rows, 4], per row of the last call {beacon recorded or -1, snrCount, count, band}.  max_rows:
        None = the panadapter's.  on = False switches it off and returns None.  Needs set_panadapter() with the smeter
        rows; set_beacon_clock() first: the switch reads the clock."""
        if not on:
            check(self._lib.t41rx_set_beacon(self._ctx, 0, 0, None, None, None, 0))
            self._beacon = None
            return None
        b = int_table(band if band is not None else [], np.int32, (self.n_channels,),
                      "band must be n_channels = %d int32 values, got %%r %%s" % self.n_channels)
        if b.min() < 0 or b.max() > 4:
            raise ValueError("band must be 0 .. 4 (20, 17, 15, 12, 10 m), got %r" % (b.tolist(),))
        if int(mode) not in (0, 1):
            raise ValueError("mode must be 0 (the firmware's cycle) or 1 (continuous), got %r" % (mode,))
        if max_rows is None:
            pan = getattr(self, "_pan", None)
            max_rows = next(iter(pan.values())).shape[1] if pan else 1
        if int(max_rows) < 1:
            raise ValueError("max_rows must be >= 1")
        return self._result_stage("_beacon", lambda ctx, on_, snr, ev, rows: self._lib.t41rx_set_beacon(ctx, on_, int(mode), ptr(b, I32P), snr, ev, rows),
                                  on, max_rows, ("float32", 18), ("int32", None, 4))

    def set_beacon_clock(self, t0_ms=0, num=32, den=3):
        """The schedule's clock (t41rx_set_beacon_clock): slot(n) = ((t0_ms + floor(n * num / den)) // 1000 % 180) // 10 at
        the panadapter's frame number n of a row; t0_ms in [0, 180000).  The default is one frame of 2048 samples at
        192 kS/s.  n is the row's update frame, the first of the firmware's sweep: fold the sweep's length into t0_ms for
        the time of its end."""
        check(self._lib.t41rx_set_beacon_clock(self._ctx, int(t0_ms), int(num), int(den)))

    def _get_beacon(self):
        snr, st = np.zeros((self.n_channels, 18), np.float32), np.zeros((self.n_channels, 8), np.int32)
        if not value(self._lib.t41rx_get_beacon(self._ctx, ptr(snr, F32P), ptr(st, I32P))):
            raise ValueError("the beacon monitor is off")
        return snr, st

    def beacon_snr(self):
        """the SNR table, float32 [n_channels, 18] (t41rx_get_beacon; synchronises): row c is beaconSNR[.][band of c]"""
        return self._get_beacon()[0]

    def beacon_status(self):
        """BeaconLoop()'s statics, int32 [n_channels, 8] (t41rx_get_beacon; synchronises): beacon.STATUS_WORDS, min and
        max as their floats' bits"""
        return self._get_beacon()[1]

    def beacon_state(self):
        """the stage's record (t41rx_beacon_get_state): 8 int32 of header, then per channel 8 status words and snr[18]"""
        return get_blob(self._lib.t41rx_beacon_get_state, self._ctx, self._lib.t41rx_beacon_state_bytes(self._ctx))

    def set_beacon_state(self, buf):
        set_blob(self._lib.t41rx_beacon_set_state, self._ctx, buf)

    # -- IQ calibration ----------------------------------------------------------------------
    CAL_BINS = {("rx", DEMOD_LSB): (310, 460), ("rx", DEMOD_USB): (65, 192),   # cal_bins[], Process2.cpp:429-444
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
        _args.set_cal_corrections(self, self._lib.t41rx_set_cal_corrections, amp, phase)

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
            if not (cuda_tensor(I, (torch.int16, torch.float32), self.device) and cuda_tensor(Q, I.dtype, self.device)):
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
            tdtype = None if host else getattr(torch, np.dtype(dtype_np).name)
            if buf is True:
                return np.zeros(shape + (512,), dtype_np) if host else torch.zeros(shape + (512,), dtype=tdtype, device=I.device)
            ok = tuple(buf.shape) == shape + (512,) and (
                (isinstance(buf, np.ndarray) and buf.dtype == dtype_np and buf.flags["C_CONTIGUOUS"] and buf.flags["WRITEABLE"]) if host
                else cuda_tensor(buf, tdtype, self.device))
            if not ok:
                raise ValueError("%s must be a contiguous %s buffer of shape %r next to I/Q" % (what, np.dtype(dtype_np).name, shape + (512,)))
            return buf

        pixel, spec = side(pixel, np.int16, "pixel"), side(spec, np.float32, "spec")
        u = None
        if update is not None and host:
            u = np.ascontiguousarray(np.asarray(update) != 0, dtype=np.uint8)
            if u.shape != (nfr,):
                raise ValueError("update must hold n_frames=%d flags, got %r" % (nfr, u.shape))
        elif update is not None:
            u = update if isinstance(update, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(update) != 0, dtype=np.uint8)).to(I.device)
            if not (cuda_tensor(u, torch.uint8) and tuple(u.shape) == (nfr,)):
                raise ValueError("update must hold n_frames=%d uint8 flags" % nfr)
        res = np.zeros(shape + (3,), np.float32) if host else torch.zeros(shape + (3,), dtype=torch.float32, device=I.device)
        lib = self._lib
        run(host, lib.t41rx_calibrate_host_q15 if q15 else lib.t41rx_calibrate_host,
            lib.t41rx_calibrate_device_q15 if q15 else lib.t41rx_calibrate_device, self.device,
            self._ctx, ptr(I), ptr(Q), int(bool(shared_input)), ptr(u), ptr(res), ptr(pixel), ptr(spec), nfr)
        if not host:
            self._cal_keep = (I, Q, u)  # alive until the next call: the launch is asynchronous
        return res, pixel, spec

    def _out_shape(self, nfr):
        """the audio's shape for a call of nfr frames: audio_rows rows (n_channels, or the output map's n_rows), whatever
        the input map makes of the input's"""
        rows = self.audio_rows
        if self.layout == "time":
            return (nfr, rows, self.audio_frame_len)
        return (rows, nfr * self.audio_frame_len)

    def _rows_text(self):
        rows = getattr(self, "_audio_rows", None)  # (named with an output map set only)
        return "(n_channels=%d, n_streams=%d%s)" % (self.n_channels, self.n_streams, "" if rows is None else ", audio_rows=%d" % rows)

    def _check_out_torch(self, out, like, nfr):
        shape = self._out_shape(nfr)
        if not (cuda_tensor(out, like.dtype) and tuple(out.shape) == shape and out.device == like.device):
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
        _args.close(self, "t41rx_destroy")

    __del__ = _args.finalize
