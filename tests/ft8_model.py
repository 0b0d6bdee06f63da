"""FT8 receive up to the finished waterfall, restated from the firmware in numpy integer and f32 arithmetic.

What it restates, per channel and per frame of 256 floats of float_buffer_L behind the demodulator and the AGC
(the position of the library's demod tap, in front of the equaliser):

  collector   Process.cpp:629-663, while syncFlag: arm_float_to_q15 (truncating, saturating), the 68-iteration loop
              as written and in its order (roll two words, write one at `+ leftover`), ++dataLoop, the three
              `leftover` cells at dataLoop 4 / 8 / 12, the last cell and DSP_Flag = 1 at 15.  The quirks are kept:
              words 1020..1023 and 2044..2047 are never rolled; with leftover >= 1 iteration i rolls the sample that
              iteration i - leftover of the same frame has just written; the `leftover` cell written behind frames
              3 / 7 / 11 is rolled by the next frame.  collect_closed_form() is the same frame without the sequential
              dependence (what the kernel does); test_ft8_model.py holds the two against each other.
  block       Process.cpp:668-672, ft8.cpp:223-268, when DSP_Flag == 1 and ft8_flag == 1: for time_sub 0 and 512 the
              Blackman-windowed 2048-point q15 real FFT, arm_shift_q15 by 5, arm_cmplx_mag_squared_q15, mag_db[] looked
              up by that value, and for freq_sub 0 / 1 the 368 averaged, clipped bytes at 1472 * FT_8_counter + ...
              Only FFT bins 0..736 are ever read, and no more are computed.  FT_8_counter++, at 92 ft8_flag = 0 and the
              frame reports "slot complete"; DSP_Flag = 0.  A DSP_Flag left standing while ft8_flag was 0 makes block 0
              of the next slot fire on the first frame after the restart, off the 15-frame phase: kept.
  slot timing update_synchronization() (ft8.cpp:154-166) at the end of every frame with ft8_flag == 0 and syncFlag, in
              uint32 arithmetic on the clock millis(n) = t0 + floor(n * num / den) (default 32 / 3), n = the channel's
              count of FT8 frames since power-on or reset.  auto_sync_FT8() polls the RTC and stays with the caller:
              sync() performs its success branch (start_time = millis(n), ft8_flag = 1, FT_8_counter = 0, syncFlag =
              true) and touches nothing else.

The power bytes go to one of two halves [2][92 * 1472] per channel so that a finished slot stays readable; the state
word `half` names the one being written and flips when block 92 is written.  (ft8_decode() runs inside the frame that
completes a slot and clears ft8_decode_flag there, so the collector never pauses.)

arm_rfft_q15 (2048 points, forward, bit reversal on) is CMSIS-DSP's, restated as its Cortex-M7 (ARM_MATH_DSP) build
computes it: arm_cfft_q15 on the 1024 complex points (re = even, im = odd sample) -- arm_radix4_butterfly_q15 with the
first stage on inputs shifted right by 2 (two halving adds with 0) and one halving add, three middle stages with two
halvings, the last stage with one (1 / 1024 in all); saturating adds (__QADD16 / __QSUB16 / __QASX / __QSAX), halving
adds that floor (__SHADD16 / __SHSUB16 / __SHASX / __SHSAX), twiddle products `__SMUAD(C, x) >> 16` and the upper half
of `__SMUSDX(C, x)`; outputs b and c of a butterfly stored swapped, so the bit reversal behind the stages is the plain
binary one -- then arm_split_rfft_q15 with the A / B tables at modifier 4: `(__SMLAD(...)) >> 16`, which halves once
more (bin k holds X[k] / 2048 in q15 units), and bin 0 as `(re + im) >> 1`.

What the firmware leaves open (the library is linked precompiled and its source and tables are not at hand), and what
this model and the kernel decide:
  * table rounding: twiddleCoef_1024_q15[k] = (cos, sin)(2 pi k / 1024) and realCoefAQ15 / realCoefBQ15 at angle
    2 pi k / 2048, A = (0.5 (1 - sin), -0.5 cos), B = (0.5 (1 + sin), 0.5 cos), each as round-half-away(x * 32768)
    computed in double and saturated to -32768..32767 (CMSIS documents `round(x * pow(2, 15))`);
  * the rounding of a halving add: floor (arithmetic shift), as the instructions do;
  * the `>> 16` of the products: arithmetic shifts of signed 32-bit sums that wrap (no saturation);
  * the one wrapped sum of __SMUAD in arm_cmplx_mag_squared_q15 at re = im = -32768: the sum is taken in 64 bits,
    so (re*re + im*im) >> 17 lies in 0..16384 and mag_db has 16385 entries (the 32-bit wrap would give -16384, an
    index in front of the table);
  * `(q15_t)(float)`: the f32 product is truncated toward zero, saturated to int32 and its low 16 bits kept (the
    firmware's window never exceeds 1.0, so nothing wraps there); `(int)db` likewise truncates, saturates, NaN -> 0;
  * newlib's cosf / log in ft8_tables(): numpy's are used; the tables are the caller's in any case.
"""
import numpy as np

GULP = 1024              # input_gulp_size
FFT_SIZE = 2048
BUF_WORDS = 3 * GULP     # ft8_dsp_buffer
ROW = 368                # ft8_buffer
BLOCK_BYTES = 4 * ROW    # offset_step
SLOT_BLOCKS = 92         # ft8_msg_samples
HALF_BYTES = SLOT_BLOCKS * BLOCK_BYTES
BINS = 2 * ROW + 1       # FFT bins 0..736 are read
MAG_ENTRIES = 16385
SCALARS = 16
WORDS = SCALARS + BUF_WORDS
MAGIC = 0x46313454       # "T41F"
ABI = 5
# the scalars of a channel's record, in order (words 9..15 zero)
S_N, S_SYNC, S_FT8FLAG, S_DSPFLAG, S_COUNTER, S_DATALOOP, S_LEFTOVER, S_START, S_HALF = range(9)
KCOSTAS = (3, 1, 4, 0, 6, 5, 2)  # kCostas_map (tests/golden/ft8/costas.npz holds the same)


def ft8_tables():
    """(window[2048], mag_db[16385]) in the firmware's types: ft_blackman_i(i, 2048) in f32 (ft8.cpp:168-178) and
    (float)(10.0 * log((float)(10 * m) + 0.1)) with the sum and the logarithm in double (ft8.cpp:238-240)"""
    f = np.float32
    alpha = f(0.16)
    a0, a1, a2 = (f(1) - alpha) / f(2), f(0.5), alpha / f(2)
    i = np.arange(FFT_SIZE, dtype=np.float32)
    x1 = np.cos(f(2) * f(np.pi) * i / f(FFT_SIZE - 1), dtype=np.float32)
    x2 = f(2) * x1 * x1 - f(1)
    window = (a0 - a1 * x1 + a2 * x2).astype(np.float32)
    m = np.arange(MAG_ENTRIES, dtype=np.int64)
    mag_db = (10.0 * np.log((10 * m).astype(np.float32).astype(np.float64) + 0.1)).astype(np.float32)
    return window, mag_db


# ---- q15 helpers (int64 arrays: every wrap and saturation is written out) ---------------------------------------------
def _sat16(x):
    return np.clip(x, -32768, 32767)


def _wrap16(x):
    return ((x + 32768) & 0xFFFF) - 32768


def _wrap32(x):
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _round_q15(x):
    r = np.where(x >= 0, np.floor(x * 32768.0 + 0.5), np.ceil(x * 32768.0 - 0.5))
    return _sat16(r.astype(np.int64))


def float_to_q15(x):
    """arm_float_to_q15 without ARM_MATH_ROUNDING: (q15_t)__SSAT((q31_t)(x * 32768.0f), 16), toward zero"""
    p = np.asarray(x, np.float32) * np.float32(32768.0)
    return _sat16(np.trunc(np.clip(np.nan_to_num(p, nan=0.0), -2147483648.0, 2147483520.0)).astype(np.int64))


def _tables():
    k = np.arange(768, dtype=np.float64)
    tw = (_round_q15(np.cos(2 * np.pi * k / 1024)), _round_q15(np.sin(2 * np.pi * k / 1024)))
    a = 2 * np.pi * np.arange(BINS, dtype=np.float64) / 2048
    A = (_round_q15(0.5 * (1.0 - np.sin(a))), _round_q15(-0.5 * np.cos(a)))
    B = (_round_q15(0.5 * (1.0 + np.sin(a))), _round_q15(0.5 * np.cos(a)))
    rev = np.array([int(format(i, "010b")[::-1], 2) for i in range(1024)])
    return tw, A, B, rev


_TW, _A, _B, _REV = _tables()


def _twiddle(k, xr, xi):
    """out = (x * conj(W^k)): re = __SMUAD(C, x) >> 16, im = upper half of __SMUSDX(C, x)"""
    c, s = _TW[0][k], _TW[1][k]
    return _wrap32(c * xr + s * xi) >> 16, _wrap32(c * xi - s * xr) >> 16


def cfft1024_q15(re, im):
    """arm_cfft_q15 (1024 points, forward, bit reversal): int arrays [..., 1024] in, the same out, scaled by 1 / 1024"""
    re = np.array(re, dtype=np.int64)
    im = np.array(im, dtype=np.int64)
    # ---- first stage: inputs >> 2, output 0 halved once, the others through `>> 16` of the twiddle product
    j = np.arange(256)
    ar, ai, br, bi = re[..., j] >> 2, im[..., j] >> 2, re[..., j + 256] >> 2, im[..., j + 256] >> 2
    cr, ci, dr, di = re[..., j + 512] >> 2, im[..., j + 512] >> 2, re[..., j + 768] >> 2, im[..., j + 768] >> 2
    Rr, Ri, Sr, Si = _sat16(ar + cr), _sat16(ai + ci), _sat16(ar - cr), _sat16(ai - ci)
    Tr, Ti = _sat16(br + dr), _sat16(bi + di)
    re[..., j], im[..., j] = (Rr + Tr) >> 1, (Ri + Ti) >> 1
    re[..., j + 256], im[..., j + 256] = _twiddle(2 * j, _sat16(Rr - Tr), _sat16(Ri - Ti))
    Ur, Ui = _sat16(br - dr), _sat16(bi - di)
    re[..., j + 512], im[..., j + 512] = _twiddle(j, _sat16(Sr + Ui), _sat16(Si - Ur))       # __QSAX
    re[..., j + 768], im[..., j + 768] = _twiddle(3 * j, _sat16(Sr - Ui), _sat16(Si + Ur))   # __QASX
    # ---- middle stages: n2 = 64, 16, 4; twiddle step 4, 16, 64
    n2, mod = 256, 1
    for _ in range(3):
        n1, n2, mod = n2, n2 >> 2, mod << 2
        jj = np.arange(n2)
        i0 = (np.arange(0, 1024, n1)[:, None] + jj[None, :]).ravel()
        ic = np.broadcast_to(jj * mod, (1024 // n1, n2)).ravel()
        i1, i2, i3 = i0 + n2, i0 + 2 * n2, i0 + 3 * n2
        ar, ai, br, bi = re[..., i0], im[..., i0], re[..., i1], im[..., i1]
        cr, ci, dr, di = re[..., i2], im[..., i2], re[..., i3], im[..., i3]
        Rr, Ri, Sr, Si = _sat16(ar + cr), _sat16(ai + ci), _sat16(ar - cr), _sat16(ai - ci)
        Tr, Ti = _sat16(br + dr), _sat16(bi + di)
        re[..., i0], im[..., i0] = ((Rr + Tr) >> 1) >> 1, ((Ri + Ti) >> 1) >> 1
        re[..., i1], im[..., i1] = _twiddle(2 * ic, (Rr - Tr) >> 1, (Ri - Ti) >> 1)            # __SHSUB16
        Ur, Ui = _sat16(br - dr), _sat16(bi - di)
        re[..., i2], im[..., i2] = _twiddle(ic, (Sr + Ui) >> 1, (Si - Ur) >> 1)                # __SHSAX
        re[..., i3], im[..., i3] = _twiddle(3 * ic, (Sr - Ui) >> 1, (Si + Ur) >> 1)            # __SHASX
    # ---- last stage: four neighbours, no twiddles, one halving
    g = 4 * np.arange(256)
    ar, ai, br, bi = re[..., g], im[..., g], re[..., g + 1], im[..., g + 1]
    cr, ci, dr, di = re[..., g + 2], im[..., g + 2], re[..., g + 3], im[..., g + 3]
    Rr, Ri, Tr, Ti = _sat16(ar + cr), _sat16(ai + ci), _sat16(br + dr), _sat16(bi + di)
    Sr, Si, Ur, Ui = _sat16(ar - cr), _sat16(ai - ci), _sat16(br - dr), _sat16(bi - di)
    re[..., g], im[..., g] = (Rr + Tr) >> 1, (Ri + Ti) >> 1
    re[..., g + 1], im[..., g + 1] = (Rr - Tr) >> 1, (Ri - Ti) >> 1
    re[..., g + 2], im[..., g + 2] = (Sr + Ui) >> 1, (Si - Ur) >> 1
    re[..., g + 3], im[..., g + 3] = (Sr - Ui) >> 1, (Si + Ur) >> 1
    return re[..., _REV], im[..., _REV]


def rfft2048_q15(x):
    """arm_rfft_q15 (2048 points, forward): q15 samples [..., 2048] -> (re, im) of bins 0..736, X[k] / 2048"""
    x = np.asarray(x, dtype=np.int64)
    zr, zi = cfft1024_q15(x[..., 0::2], x[..., 1::2])
    k = np.arange(1, BINS)
    ar, ai, br, bi = _A[0][k], _A[1][k], _B[0][k], _B[1][k]
    pr, pi, qr, qi = zr[..., k], zi[..., k], zr[..., 1024 - k], zi[..., 1024 - k]
    outR = _wrap32(_wrap32(pr * ar - pi * ai) + qr * br + qi * bi) >> 16   # __SMUSD, __SMLAD
    outI = _wrap32(_wrap32(qr * bi - qi * br) + pr * ai + pi * ar) >> 16   # __SMUSDX, __SMLADX
    re = np.concatenate([((zr[..., :1] + zi[..., :1]) >> 1), _wrap16(outR)], axis=-1)
    im = np.concatenate([np.zeros_like(zr[..., :1]), _wrap16(outI)], axis=-1)
    return re, im


def mag_index(x):
    """window-multiplied q15 samples [..., 2048] -> arm_cmplx_mag_squared_q15 of the bins shifted left by 5, 0..16384"""
    re, im = rfft2048_q15(x)
    re, im = _sat16(re * 32), _sat16(im * 32)   # arm_shift_q15(., 5, .)
    return (re * re + im * im) >> 17


def window_q15(buf, window):
    """(q15_t)((float)buf[i] * window[i])"""
    p = np.asarray(buf).astype(np.float32) * np.asarray(window, np.float32)
    t = np.trunc(np.clip(np.nan_to_num(p, nan=0.0), -2147483648.0, 2147483520.0)).astype(np.int64)
    return _wrap16(t)


def power_rows(buf, window, mag_db):
    """extract_power() on one channel's 3072-word buffer: the 1472 bytes of a block"""
    out = np.zeros(BLOCK_BYTES, np.uint8)
    j = np.arange(ROW)
    for ts in range(2):
        m = mag_index(window_q15(buf[512 * ts:512 * ts + FFT_SIZE], window))
        for fs in range(2):
            db = (mag_db[m[2 * j + fs]] + mag_db[m[2 * j + fs + 1]]) / np.float32(2)
            s = np.trunc(np.clip(np.nan_to_num(db.astype(np.float32), nan=0.0), -2147483648.0, 2147483520.0))
            out[736 * ts + ROW * fs + j] = np.clip(s, 0, 255).astype(np.uint8)
    return out


def collect_literal(buf, q, dataLoop, leftover):
    """the 68-iteration loop of Process.cpp:635-644 as written, on one channel's buffer (in place)"""
    for i in range(68):
        k = i + dataLoop * 68
        buf[k] = buf[k + 1024]
        buf[1024 + k] = buf[2048 + k]
        if 2048 + k + leftover < BUF_WORDS:  # (only a hand-made record with leftover ahead of dataLoop // 4 gets past the end)
            buf[2048 + k + leftover] = q[(i * 15) // 4]


def collect_closed_form(buf, q, dataLoop, leftover):
    """the same frame without the sequential dependence: every read is of the buffer as the frame found it, except
    that from iteration `leftover` on the middle third takes what iteration i - leftover has just written"""
    old = buf.copy()
    i = np.arange(68)
    k = i + dataLoop * 68
    src = q[(i * 15) // 4]
    buf[k] = old[k + 1024]
    mid = old[2048 + k]
    if leftover >= 1:
        mid[leftover:] = src[:68 - leftover]
    buf[1024 + k] = mid
    ok = 2048 + k + leftover < BUF_WORDS
    buf[(2048 + k + leftover)[ok]] = src[ok]


class FT8Model:
    """n_channels independent FT8 receivers: scal [n][16] int32-valued words, buf [n][3072], power [n][2][92 * 1472]"""

    def __init__(self, n_channels, window=None, mag_db=None, t0=0, num=32, den=3):
        w, m = ft8_tables()
        self.window = np.asarray(w if window is None else window, np.float32)
        self.mag_db = np.asarray(m if mag_db is None else mag_db, np.float32)
        self.nch = int(n_channels)
        self.t0, self.num, self.den = int(t0), int(num), int(den)
        self.scal = np.zeros((self.nch, SCALARS), np.int64)
        self.buf = np.zeros((self.nch, BUF_WORDS), np.int64)
        self.power = np.zeros((self.nch, 2, HALF_BYTES), np.uint8)
        self.collect = collect_literal

    def millis(self, n):
        return (self.t0 + (int(n) & 0xFFFFFFFF) * self.num // self.den) & 0xFFFFFFFF

    def sync(self, channels=None):
        """auto_sync_FT8()'s success branch on the channels whose entry is non-zero (None: all)"""
        for c in range(self.nch):
            if channels is not None and not channels[c]:
                continue
            s = self.scal[c]
            s[S_START] = self.millis(s[S_N])
            s[S_FT8FLAG], s[S_COUNTER], s[S_SYNC] = 1, 0, 1

    def frame(self, c, x):
        """one frame of channel c on 256 floats; returns the frame's four status words"""
        s, buf = self.scal[c], self.buf[c]
        done = 0
        if s[S_SYNC]:
            q = float_to_q15(x)
            self.collect(buf, q, int(s[S_DATALOOP]), int(s[S_LEFTOVER]))
            s[S_DATALOOP] += 1
            if s[S_DATALOOP] == 15:
                buf[3071] = q[255]
                s[S_DATALOOP] = s[S_LEFTOVER] = 0
                s[S_DSPFLAG] = 1
            elif s[S_DATALOOP] in (4, 8, 12):
                if 2048 + s[S_DATALOOP] * 68 + s[S_LEFTOVER] < BUF_WORDS:
                    buf[2048 + s[S_DATALOOP] * 68 + s[S_LEFTOVER]] = q[255]
                s[S_LEFTOVER] += 1
        if s[S_DSPFLAG] == 1 and s[S_FT8FLAG] == 1:
            o = BLOCK_BYTES * int(s[S_COUNTER])
            self.power[c, int(s[S_HALF]), o:o + BLOCK_BYTES] = power_rows(buf, self.window, self.mag_db)
            s[S_COUNTER] += 1
            if s[S_COUNTER] == SLOT_BLOCKS:
                s[S_FT8FLAG] = 0
                done = 1 + int(s[S_HALF])
                s[S_HALF] ^= 1
            s[S_DSPFLAG] = 0
        if s[S_FT8FLAG] == 0 and s[S_SYNC]:
            ft8_time = (self.millis(s[S_N]) - int(s[S_START])) & 0xFFFFFFFF
            if ft8_time % 15000 <= 200:
                s[S_FT8FLAG], s[S_COUNTER] = 1, 0
        s[S_N] = (int(s[S_N]) + 1) & 0xFFFFFFFF
        return int(s[S_COUNTER]), int(s[S_FT8FLAG]), done, int(s[S_DATALOOP])

    def process(self, audio):
        """audio [n_channels, n_frames * 256] f32 -> status [n_channels, n_frames, 4] int32"""
        audio = np.asarray(audio, np.float32).reshape(self.nch, -1, 256)
        st = np.zeros((self.nch, audio.shape[1], 4), np.int32)
        for c in range(self.nch):
            for f in range(audio.shape[1]):
                st[c, f] = self.frame(c, audio[c, f])
        return st

    def words(self):
        """[n_channels][3088] int32: the record's body (n and start_time as their 32 bits)"""
        w = np.concatenate([self.scal, self.buf], axis=1)
        return (w & 0xFFFFFFFF).astype(np.uint32).view(np.int32)

    def record(self):
        """the library's FT8 state record: header of 8 int32 (magic "T41F", ABI, n_channels, words per channel, zeros)"""
        hdr = np.array([MAGIC, ABI, self.nch, WORDS, 0, 0, 0, 0], np.int32)
        return np.concatenate([hdr, self.words().ravel()]).view(np.uint8)

    def load_record(self, rec):
        w = np.ascontiguousarray(rec, np.uint8).view(np.int32)
        assert w[0] == MAGIC and w[2] == self.nch and w[3] == WORDS
        body = w[8:].reshape(self.nch, WORDS).astype(np.int64)
        self.scal = body[:, :SCALARS].copy()
        for k in (S_N, S_START):
            self.scal[:, k] &= 0xFFFFFFFF
        self.buf = body[:, SCALARS:].copy()
