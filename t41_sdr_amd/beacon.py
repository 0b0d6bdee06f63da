"""The beacon monitor's host-side helpers (t41rx_set_beacon; RxChain.set_beacon): the NCDXF schedule as the firmware
evaluates it, and what DisplayBeaconsSNR() makes of the SNR table (Beacon.cpp:204-208, 282-295, 359-424) -- the colour
indices and the 96-byte record handed to T41BeaconSendData().  The library carries no beacon names, maps or bearings:
beacons are 0 .. 17 in the schedule's order, bands 0 .. 4 are 20, 17, 15, 12 and 10 m."""
import math

import numpy as np

BEACONS = 18
BANDS = 5
SLOT_SECONDS = 10
CYCLE_SECONDS = 180
RECORD_BYTES = 96
STATUS_WORDS = ("min", "max", "snrCount", "count", "changeBandFlag", "currentBeacon", "band", "own_band")


def beacon_now(seconds, band):
    """GetBeaconNow(band) at `seconds` of the clock (any integer number of seconds; the firmware's is the time of day):
    the beacon transmitting on that band, (seconds % 180) // 10 - band, plus 18 if negative."""
    seconds, band = int(seconds), int(band)
    if seconds < 0 or not 0 <= band < BANDS:
        raise ValueError("need seconds >= 0 and 0 <= band < 5")
    index = (seconds % CYCLE_SECONDS) // SLOT_SECONDS - band
    return index + (BEACONS if index < 0 else 0)


def _to_int(snr):
    """the float -> int conversion of GetSNRColor()'s argument.  Truncation toward zero where C defines it; the firmware
    leaves a non-finite or out-of-range value undefined, here it saturates at the int32 limits and NaN gives 0."""
    snr = float(snr)
    if math.isnan(snr):
        return 0
    if snr >= 2147483647.0:
        return 2147483647
    if snr <= -2147483648.0:
        return -2147483648
    return int(snr)


def snr_levels(table):
    """GetSNRColor()'s index for every cell of beaconSNR as DisplayBeaconsSNR() stores it in its record: table is
    [18][5] (beacon, band); returns uint8 [18][5], 0 .. 9 (S0 .. S9 colours), snr // 6 capped at 9.
    The firmware's quirk is kept: `index` is ONE variable for the whole walk (beacons outer, bands inner, starting at 0)
    and GetSNRColor() leaves it alone when snr <= 0, so such a cell repeats the index of the cell before it.  Every band is
    taken as monitored (monitorFreq[j]): one channel per band."""
    t = np.asarray(table, dtype=np.float32)
    if t.shape != (BEACONS, BANDS):
        raise ValueError("table must be [18][5] (beacon, band), got %r" % (t.shape,))
    out = np.zeros((BEACONS, BANDS), np.uint8)
    index = 0
    for i in range(BEACONS):
        for j in range(BANDS):
            snr = _to_int(t[i, j])
            if snr > 0:
                index = snr // 6
            out[i, j] = index if index < 10 else 9
    return out


def monitor_record(tables_of_5_channels, band, beacon, volume):
    """The 96-byte record DisplayBeaconsSNR() sends (Beacon.cpp:387-424): 'B', 'M', band, beacon, audioVolume as bytes,
    the 90 levels of snr_levels() at [5 + beacon * 5 + band], ';'.  tables_of_5_channels: for each band 0 .. 4 the 18
    floats of the channel that monitors it (RxChain.beacon_snr()[c])."""
    cols = list(tables_of_5_channels)
    if len(cols) != BANDS:
        raise ValueError("need one table per band (5), got %d" % len(cols))
    table = np.zeros((BEACONS, BANDS), np.float32)
    for j, col in enumerate(cols):
        c = np.asarray(col, dtype=np.float32)
        if c.shape != (BEACONS,):
            raise ValueError("the table of band %d must be 18 floats, got %r" % (j, c.shape))
        table[:, j] = c
    rec = bytearray(RECORD_BYTES)
    rec[0:2] = b"BM"
    rec[2], rec[3], rec[4] = int(band) & 0xFF, int(beacon) & 0xFF, int(volume) & 0xFF
    rec[5:95] = snr_levels(table).tobytes()
    rec[95] = ord(";")
    return bytes(rec)
