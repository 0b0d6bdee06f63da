"""The beacon monitor, restated as scalar Python from the firmware's text (Beacon.cpp): the schedule (GetBeaconNow(),
:204-208), BeaconLoop()'s synced branch call by call (:466-569) with its unsynced branch as the switch-on (:610-614),
GetSNRColor() (:282-295) and the 96-byte record of DisplayBeaconsSNR() (:359-424).  float32 where the firmware computes
in float.  A channel monitors one band: monitorFreq[b] == (b == own band).

The status words are the library's (include/t41rx.h): min and max as float bits, snrCount, count, changeBandFlag,
currentBeacon, band, own band."""
import math

import numpy as np

F32 = np.float32
BEACONS, BANDS, NOISE_COUNT = 18, 5, 23  # NOISE_HI - NOISE_LO - 2 = 28 - 3 - 2


def slot(n, t0_ms=0, num=32, den=3):
    """GetBeacon20mNow() on the stage's clock at frame n: ((t0_ms + floor(n * num / den)) / 1000 % 180) / 10, integers"""
    return ((int(t0_ms) + int(n) * int(num) // int(den)) // 1000 % 180) // 10


def beacon_now(s, band):
    """GetBeaconNow(band) in slot s"""
    index = s - band
    return index + (18 if index < 0 else 0)


class Monitor:
    """one channel's BeaconLoop() statics, `band`, and its column of beaconSNR"""

    def __init__(self, own_band, n_on=0, clock=(0, 32, 3), mode=0):
        self.clock, self.mode, self.own = tuple(int(v) for v in clock), int(mode), int(own_band)
        # the unsynced branch: currentBeacon = GetBeacon20mNow(), count = 0, changeBandFlag = true, band = the last monitored
        self.min, self.max = F32(0.0), F32(-1000.0)
        self.snrCount = 0
        self.count = 0
        self.changeBandFlag = True
        self.currentBeacon = slot(n_on, *self.clock)
        self.band = self.own
        self.snr = np.zeros(BEACONS, F32)  # BeaconInit()

    def call(self, dbm, n):
        """one BeaconLoop() with the sweep's dbm at frame n; returns the event record {beacon recorded or -1, snrCount as
        compared, count behind the call, band behind the call}"""
        dbm = F32(dbm)
        recorded, seen = -1, self.snrCount
        if self.count == 0 and self.changeBandFlag:
            self.band += 1
            if self.band > 4:
                self.band = 0
            if self.band == self.own:  # monitorFreq[band]
                self.changeBandFlag = False
        elif self.count > 0:
            self.snrCount += 1
            seen = self.snrCount
            if dbm < self.min:
                self.min = dbm
            if dbm > self.max:
                self.max = dbm
            beacon = beacon_now(slot(n, *self.clock), self.band)
            if beacon != self.currentBeacon:
                if self.snrCount != NOISE_COUNT:
                    with np.errstate(invalid="ignore", over="ignore"):
                        value = F32(self.max - self.min)
                    self.snr[beacon] = value if value > 0 else F32(0.0)
                else:
                    self.snr[beacon] = F32(0.0)
                recorded = beacon
                self.snrCount = 0
                self.currentBeacon = beacon
                self.min, self.max = F32(0.0), F32(-1000.0)
                self.count += 1
                if self.mode == 1:
                    self.count = 1
                if self.count > 18:
                    self.count = 0
                    self.changeBandFlag = True
        else:  # count == 0 and not changeBandFlag
            beacon = beacon_now(slot(n, *self.clock), self.band)
            if beacon != self.currentBeacon:
                self.count += 1
        return [recorded, seen, self.count, self.band]

    def run(self, dbms, frames):
        """calls in order; returns the event records int32 [k, 4]"""
        return np.array([self.call(d, n) for d, n in zip(dbms, frames)], np.int32).reshape(-1, 4)

    def status(self):
        bits = np.array([self.min, self.max], F32).view(np.int32)
        return np.array([bits[0], bits[1], self.snrCount, self.count, int(self.changeBandFlag), self.currentBeacon, self.band, self.own], np.int32)


# ---- the end-to-end scenario of the tests: one stream of weak noise, a 1 kHz tone (USB, inside 500 .. 1500 Hz) keyed on
# for frames 2 .. 7 of the 20 frames of two slots.  The clock runs 500 ms per frame and 19 frames late, so that the call
# that sees a slot change is the last frame of the slot on the air: the window BeaconLoop() books under the beacon that
# begins on ITS clock is then exactly that beacon's slot on the air.
E2E_FRAMES, E2E_PER_SLOT, E2E_SLOTS = 360, 20, (4, 11)
E2E_CLOCK = (180000 - 19 * 500, 500, 1)
E2E_SIGMA, E2E_AMP = 0.01, 0.02
E2E_PARAMS = dict(FLoCut=500, FHiCut=1500)


def e2e_stream(L=2048):
    """I, Q float32 [1, E2E_FRAMES * L] for NCOFreq 0, mode USB"""
    rng = np.random.default_rng(0xBEAC)
    n = np.arange(E2E_FRAMES * L, dtype=np.float64)
    key = np.zeros(E2E_FRAMES * L)
    for s in E2E_SLOTS:
        key[(E2E_PER_SLOT * s + 2) * L:(E2E_PER_SLOT * s + 8) * L] = 1.0
    x = E2E_AMP * key * np.exp(2j * np.pi * (48000.0 - 1000.0) / 192000.0 * n)  # +Fs/4 and the I flip: audio at +1 kHz
    x += E2E_SIGMA * (rng.standard_normal(E2E_FRAMES * L) + 1j * rng.standard_normal(E2E_FRAMES * L)) / np.sqrt(2)
    return x.real.astype(np.float32)[None], x.imag.astype(np.float32)[None]


def e2e_conditions(tables):
    """the three conditions' first two on five tables [5][18], one per band: returns per band (smaller of the two chosen
    entries, largest other entry) after asserting the two largest are the chosen beacons shifted by the band and every
    other entry lies below half of the smaller"""
    out = []
    for k in range(BANDS):
        t = np.asarray(tables[k], F32)
        want = sorted((s - k) % 18 for s in E2E_SLOTS)
        assert sorted(np.argsort(t, kind="stable")[-2:].tolist()) == want, (k, t)
        small, others = min(t[b] for b in want), max(t[b] for b in range(BEACONS) if b not in want)
        assert others < 0.5 * small, (k, small, others)
        out.append((float(small), float(others)))
    return out


def to_int(snr):
    """float -> int of GetSNRColor()'s argument: truncation; saturating where C leaves it undefined, NaN -> 0"""
    snr = float(snr)
    if math.isnan(snr):
        return 0
    return max(-2**31, min(2**31 - 1, int(snr))) if math.isfinite(snr) else (2**31 - 1 if snr > 0 else -2**31)


def snr_levels(table):
    """beaconData[i * 5 + j + 5] of DisplayBeaconsSNR(): one `index` for the whole walk, moved only where snr > 0"""
    out = np.zeros((BEACONS, BANDS), np.uint8)
    index = 0
    for i in range(BEACONS):
        for j in range(BANDS):
            snr = to_int(table[i][j])
            if snr > 0:
                index = snr // 6
            out[i, j] = index if index < 10 else 9
    return out


def monitor_record(table, band, beacon, volume):
    rec = bytearray(96)
    rec[0], rec[1], rec[2], rec[3], rec[4] = ord("B"), ord("M"), band & 255, beacon & 255, volume & 255
    rec[5:95] = snr_levels(table).tobytes()
    rec[95] = ord(";")
    return bytes(rec)
