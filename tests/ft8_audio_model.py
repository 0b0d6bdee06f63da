"""FT8 from 12 kS/s audio: the collector of DEMOD_FT8_WAV (Process.cpp:278-335, ft8.cpp:259-268, :1359-1374,
Utility.cpp:868-888), restated on top of ft8_model -- its float_to_q15, power_rows, record layout and tables.

What it restates, per channel and per frame of 128 samples at 12 kS/s:

  collector   Process.cpp:301-313: q = arm_float_to_q15(x) (truncating, saturating; for int16 input readWave's
              `raw / 32768.0f` followed by that conversion is the identity, so int16 samples are taken as they are), then
              for i in 0..67 with k = i + 68 * dataLoop
                  buf[k] = buf[k + 1024]; buf[1024 + k] = buf[2048 + k]; buf[2048 + k] = q[(int)((float)i * 120.0 / 64.0)]
              The index is (i * 15) >> 3 and never exceeds 125.  There is no `leftover`, no "last cell", no syncFlag gate
              and no DSP_Flag.  68 x 15 = 1020: cells 1020..1023, 2044..2047 and 3068..3071 keep what the record held.
  block       Process.cpp:315-327: ++dataLoop == 15 sets dataLoop = 0 and runs process_FT8_FFT() unconditionally (ft8_flag
              is not asked): extract_power(1472 * FT_8_counter) into the half being written, FT_8_counter++, at 92
              ft8_flag = 0, the slot is complete -- the frame reports 1 + that half, `half` flips as in the live stage --
              and FT_8_counter = 0 (:325).  update_synchronization() is never called.
  n           the frame count behind millis() advances by one per frame: a 128-sample frame lasts the same 32 / 3 ms as a
              live one.  syncFlag, DSP_Flag, leftover and start_time are not touched.
  begin       setupFT8Wav() (ft8.cpp:1372): FT_8_counter = 0.
  end         the mode's exit (Process.cpp:339-342): syncFlag = 0, FT_8_counter = 0, ft8_flag = 0.
              Neither resets dataLoop, as in the firmware.

The status words of a frame keep the live stage's meaning: FT_8_counter behind the frame, ft8_flag, 0 or 1 + the completed
half, dataLoop.

What the firmware leaves open, and what this model and the kernel decide: the live stage leaves FT_8_counter at 92 next to
ft8_flag 0 between a slot's last block and its restart.  The firmware never enters the WAV mode without setupFT8Wav(); a
caller who does (no begin()) would have extract_power() write behind export_fft_power and the counter run away.  Here such
a block writes nothing and leaves the counter at 92 until begin() or end().

audio() has two forms.  "literal" is the loop as written, frame after frame.  "gulp" is what the kernel does: up to a whole
gulp of 15 frames collected in one pass -- cell c = 68 * d + i for the frames d0 <= d < d1, each cell rolled once, every
cell independent of every other -- then the block when d1 == 15, and the status words in closed form.
test_ft8_audio_model.py holds the two against each other.

Out of scope: the x2 linear interpolation to 24 kS/s for listening (Process.cpp:293-297; it reads 128 stale floats beyond
what readWave() filled), the pacing by Q_in_L.clear() / Q_in_R.clear(), and the SD card.
"""
import numpy as np

import ft8_model as M

FRAME = 128                                 # FFT_length / 2 / 2 samples per ProcessIQData()
CELLS = 68                                  # cells per frame
SLOT_FRAMES = 15 * M.SLOT_BLOCKS            # 1380
HOLES = tuple(b + k for b in (0, 1024, 2048) for k in range(1020, 1024))
# (int)(((float)i) * 120.0 / 64.0): the product and the quotient in double, truncated
INDEX = np.array([int(float(np.float32(i)) * 120.0 / 64.0) for i in range(CELLS)])


def to_q15(x):
    """a frame's samples as q15: int16 as they are, floats through arm_float_to_q15"""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.int64)
    return M.float_to_q15(x)


class FT8AudioModel(M.FT8Model):
    """FT8Model with the WAV collector: audio() next to process(), begin() and end() next to sync(), one record"""

    def begin(self, channels=None):
        for c in range(self.nch):
            if channels is None or channels[c]:
                self.scal[c, M.S_COUNTER] = 0

    def end(self, channels=None):
        for c in range(self.nch):
            if channels is None or channels[c]:
                self.scal[c, M.S_SYNC] = self.scal[c, M.S_COUNTER] = self.scal[c, M.S_FT8FLAG] = 0

    def _block(self, c):
        """process_FT8_FFT() and Process.cpp:318-326; returns the frame's third status word"""
        s = self.scal[c]
        if s[M.S_COUNTER] >= M.SLOT_BLOCKS:   # (no begin(): see the module's text)
            return 0
        o = M.BLOCK_BYTES * int(s[M.S_COUNTER])
        self.power[c, int(s[M.S_HALF]), o:o + M.BLOCK_BYTES] = M.power_rows(self.buf[c], self.window, self.mag_db)
        s[M.S_COUNTER] += 1
        if s[M.S_COUNTER] < M.SLOT_BLOCKS:
            return 0
        done = 1 + int(s[M.S_HALF])
        s[M.S_FT8FLAG] = 0
        s[M.S_HALF] ^= 1
        s[M.S_COUNTER] = 0
        return done

    def audio_frame(self, c, x):
        """one frame of channel c on 128 samples, the loop as written; returns the frame's four status words"""
        s, buf = self.scal[c], self.buf[c]
        q = to_q15(x)
        dataLoop = int(s[M.S_DATALOOP])
        for i in range(CELLS):
            buf[i + dataLoop * 68] = buf[i + 1024 + dataLoop * 68]
            buf[1024 + i + dataLoop * 68] = buf[i + 2048 + dataLoop * 68]
            buf[2048 + i + dataLoop * 68] = q[int(float(np.float32(i)) * 120.0 / 64.0)]
        done = 0
        dataLoop += 1
        if dataLoop == 15:
            dataLoop = 0
            done = self._block(c)
        s[M.S_DATALOOP] = dataLoop
        s[M.S_N] = (int(s[M.S_N]) + 1) & 0xFFFFFFFF
        return int(s[M.S_COUNTER]), int(s[M.S_FT8FLAG]), done, dataLoop

    def _audio_gulps(self, c, x):
        """a call of channel c on [n_frames][128] samples, a gulp at a time; returns its status words [n_frames][4]"""
        s, buf = self.scal[c], self.buf[c]
        nfr = x.shape[0]
        assert nfr <= SLOT_FRAMES
        q = to_q15(x).reshape(-1)
        dl0, c0, flag0, half0 = (int(s[k]) for k in (M.S_DATALOOP, M.S_COUNTER, M.S_FT8FLAG, M.S_HALF))
        f, d0 = 0, dl0
        while f < nfr:
            d1 = min(15, d0 + nfr - f)
            cell = np.arange(CELLS * d0, CELLS * d1)
            d, i = cell // CELLS, cell % CELLS
            src = q[(f + d - d0) * FRAME + ((i * 15) >> 3)]
            buf[cell] = buf[cell + 1024]
            buf[cell + 1024] = buf[cell + 2048]
            buf[cell + 2048] = src
            f += d1 - d0
            d0 = d1
            if d1 == 15:
                d0 = 0
                self._block(c)
        s[M.S_DATALOOP] = d0
        s[M.S_N] = (int(s[M.S_N]) + nfr) & 0xFFFFFFFF
        # the status words in closed form: nb blocks have run behind frame f
        st = np.zeros((nfr, 4), np.int32)
        fr = np.arange(nfr)
        nb = (dl0 + fr + 1) // 15
        st[:, 3] = (dl0 + fr + 1) % 15
        if c0 >= M.SLOT_BLOCKS:
            st[:, 0], st[:, 1] = c0, flag0
        else:
            over = c0 + nb >= M.SLOT_BLOCKS   # at most one completion in 1380 frames
            st[:, 0] = np.where(over, c0 + nb - M.SLOT_BLOCKS, c0 + nb)
            st[:, 1] = np.where(over, 0, flag0)
            st[dl0 + fr + 1 == 15 * (M.SLOT_BLOCKS - c0), 2] = 1 + half0
        return st

    def audio(self, pcm, form="literal"):
        """pcm [n_channels, n_frames * 128] int16 or f32 -> status [n_channels, n_frames, 4] int32"""
        pcm = np.asarray(pcm)
        pcm = pcm.reshape(self.nch, -1, FRAME)
        st = np.zeros((self.nch, pcm.shape[1], 4), np.int32)
        for c in range(self.nch):
            if form == "gulp":
                st[c] = self._audio_gulps(c, pcm[c])
            else:
                for f in range(pcm.shape[1]):
                    st[c, f] = self.audio_frame(c, pcm[c, f])
        return st


def transmission(tones, j0, amp, start, n_samples=SLOT_FRAMES * FRAME, sigma=0.0, seed=None):
    """79 symbols as 12 kS/s audio: continuous-phase 8-FSK, 6.25 Hz spacing, tone 0 at j0 x 6.25 Hz, 1920 samples per symbol
    from sample `start`, silence around it, Gaussian noise of `sigma` from default_rng(seed) on the whole slot; f32"""
    f = np.repeat(6.25 * (j0 + np.asarray(tones)), 1920)
    ph = 2 * np.pi * np.cumsum(f) / 12000.0
    x = np.zeros(n_samples, np.float64)
    n = min(len(ph), n_samples - start)
    x[start:start + n] = amp * np.sin(ph[:n])
    if sigma:
        x += np.random.default_rng(seed).normal(0.0, sigma, n_samples)
    return x.astype(np.float32)


def pcm16(x):
    """f32 audio as the int16 samples of a WAV file (arm_float_to_q15's own rounding)"""
    return M.float_to_q15(x).astype(np.int16)
