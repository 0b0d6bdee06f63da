"""FT8 decode, the host half: the records of t41rx_ft8_decode_*() as numpy types, unpack77_fields() (ft8.cpp:618-667 with
its helpers, :958-1332) and the slot's message list as the loop of ft8_decode() builds newlyDecoded (:788-804, :839-842).

The device does find_sync(), extract_likelihood(), bp_decode(), pack_bits() and the CRC (ft8_decode_kernel.hip); what is
left is string work on at most 20 payloads of 77 bits per channel.  The restatement keeps the firmware's prints as they
come out of its buffers:
  a hashed call is printed by int_to_dd(result + 1, n, 7, true) and result[8] = '>': the '>' lands on the seventh digit,
    so the print is '<+' and the first six digits of the zero-padded hash and '>'; the 12-bit hash of a type 4 message
    likewise shows three of its four digits;
  "CQ nnn" is printed with full_sign: "CQ +nnn";
  int_to_dd() prints a digit past 9 as the character behind '9' (a report field above +99);
  igrid4 == 32400 (MAXGRID4 itself) is read as the grid "AA00".
The decoded[] log with its RTC stamps, Target_Distance() and the locator check, and everything drawn stay with the caller.
"""
import numpy as np

MAX_CANDIDATES = 20
SLOT_BYTES = 135424  # 92 * 1472
K_MAX_DECODED_MESSAGES, K_MAX_MESSAGE_LENGTH = 10, 35

# t41rx_ft8_candidate / t41rx_ft8_result (include/t41rx.h)
CANDIDATE = np.dtype([("score", "<i2"), ("time_offset", "<i2"), ("freq_offset", "<i2"), ("time_sub", "u1"), ("freq_sub", "u1"),
                      ("n_errors", "<i2"), ("iterations", "u1"), ("flags", "u1"), ("a91", "u1", (12,)), ("reserved", "u1", (8,))])
RESULT = np.dtype([("num_candidates", "<i4"), ("num_valid", "<i4"), ("select", "<i4"), ("reserved", "<i4"),
                   ("cand", CANDIDATE, (MAX_CANDIDATES,))])
assert CANDIDATE.itemsize == 32 and RESULT.itemsize == 656

MAX22, NTOKENS, MAXGRID4 = 4194304, 2063592, 32400


def charn(c, table_idx):
    """integer index -> character by one of six tables (ft8.cpp:1303-1332)"""
    if table_idx != 2 and table_idx != 3:
        if c == 0:
            return " "
        c -= 1
    if table_idx != 4:
        if c < 10:
            return chr(ord("0") + c)
        c -= 10
    if table_idx != 3:
        if c < 26:
            return chr(ord("A") + c)
        c -= 26
    if table_idx == 0:
        if c < 5:
            return "+-./?"[c]
    elif table_idx == 5:
        if c == 0:
            return "/"
    return "_"


def int_to_dd(value, width, full_sign):
    s = ""
    if value < 0:
        s, value = "-", -value
    elif full_sign:
        s = "+"
    divisor = 10 ** (width - 1)
    while divisor >= 1:
        digit = value // divisor
        s += chr(ord("0") + digit)
        value -= digit * divisor
        divisor //= 10
    return s


def trim(s):
    return s.strip(" ")


def unpack28(n28, ip, i3):
    """-> (rc, text)"""
    if n28 < NTOKENS:
        if n28 <= 2:
            return 0, ("DE", "QRZ", "CQ")[n28]
        if n28 <= 1002:
            return 0, "CQ " + int_to_dd(n28 - 3, 3, True)
        if n28 <= 532443:
            n, aaaa = n28 - 1003, [""] * 4
            for i in (3, 2, 1, 0):
                aaaa[i] = charn(n % 27, 4)
                if i:
                    n //= 27
            return 0, "CQ " + "".join(aaaa).lstrip(" ")
        return -1, ""
    n28 -= NTOKENS
    if n28 < MAX22:
        buf = list("<" + int_to_dd(n28, 7, True))  # '<', '+', seven digits
        buf[8] = ">"                               # result[8] = '>': on the seventh digit
        return 0, "".join(buf[:9])
    n = n28 - MAX22
    c = [""] * 6
    c[5] = charn(n % 27, 4)
    n //= 27
    c[4] = charn(n % 27, 4)
    n //= 27
    c[3] = charn(n % 27, 4)
    n //= 27
    c[2] = charn(n % 10, 3)
    n //= 10
    c[1] = charn(n % 36, 2)
    n //= 36
    c[0] = charn(n % 37, 1)
    result = trim("".join(c))
    if len(result) == 0:
        return -1, ""
    if ip:
        if i3 == 1:
            result += "/R"
        elif i3 == 2:
            result += "/P"
    return 0, result


def unpack_type1(a77, i3):
    n28a = (a77[0] << 21) | (a77[1] << 13) | (a77[2] << 5) | (a77[3] >> 3)
    n28b = ((a77[3] & 0x07) << 26) | (a77[4] << 18) | (a77[5] << 10) | (a77[6] << 2) | (a77[7] >> 6)
    ir = (a77[7] & 0x20) >> 5
    igrid4 = ((a77[7] & 0x1F) << 10) | (a77[8] << 2) | (a77[9] >> 6)
    rc, field1 = unpack28(n28a >> 1, n28a & 1, i3)
    if rc < 0:
        return -1, "", "", ""
    rc, field2 = unpack28(n28b >> 1, n28b & 1, i3)
    if rc < 0:
        return -2, field1, "", ""
    if igrid4 <= MAXGRID4:
        n = igrid4
        d3 = chr(ord("0") + n % 10)
        n //= 10
        d2 = chr(ord("0") + n % 10)
        n //= 10
        d1 = chr(ord("A") + n % 18)
        n //= 18
        d0 = chr(ord("A") + n % 18)
        field3 = ("R " if ir > 0 else "") + d0 + d1 + d2 + d3
    else:
        irpt = igrid4 - MAXGRID4
        if irpt == 1:
            field3 = ""
        elif irpt == 2:
            field3 = "RRR"
        elif irpt == 3:
            field3 = "RR73"
        elif irpt == 4:
            field3 = "73"
        else:
            field3 = ("R" if ir > 0 else "") + int_to_dd(irpt - 35, 2, True)
    return 0, field1, field2, field3


def _shift_right_1(a71):
    b71, carry = [], 0
    for i in range(9):
        b71.append(carry | (a71[i] >> 1))
        carry = 0x80 if (a71[i] & 1) else 0
    return b71


def unpack_text(a71):
    b71 = _shift_right_1(a71)
    c14 = [""] * 13
    for idx in range(12, -1, -1):
        rem = 0
        for i in range(9):  # divide the long integer in b71 by 42
            rem = (rem << 8) | b71[i]
            b71[i] = rem // 42
            rem = rem % 42
        c14[idx] = charn(rem, 0)
    return 0, trim("".join(c14))


def unpack_telemetry(a71):
    return 0, "".join("%02X" % b for b in _shift_right_1(a71))


def unpack_nonstandard(a77):
    n12 = (a77[0] << 4) | (a77[1] >> 4)
    n58 = (a77[1] & 0x0F) << 54
    for i, sh in zip(range(2, 8), (46, 38, 30, 22, 14, 6)):
        n58 |= a77[i] << sh
    n58 |= a77[8] >> 2
    iflip = (a77[8] >> 1) & 1
    nrpt = ((a77[8] & 1) << 1) | (a77[9] >> 7)
    icq = (a77[9] >> 6) & 1
    c11 = [""] * 11
    for i in range(10, -1, -1):
        c11[i] = charn(n58 % 38, 5)
        if i:
            n58 //= 38
    c11 = "".join(c11)
    buf = list("<" + int_to_dd(n12, 4, True))  # '<', '+', four digits
    buf[5] = ">"                               # call_3[5] = '>': on the fourth digit
    call_3 = "".join(buf[:6])
    call_1, call_2 = (c11, call_3) if iflip else (call_3, c11)
    if icq == 0:
        field1 = trim(call_1)
        field3 = {1: "RRR", 2: "RR73", 3: "73"}.get(nrpt, "")
    else:
        field1, field3 = "CQ", ""
    return 0, field1, trim(call_2), field3


def unpack77_fields(a91):
    """(rc, field1, field2, field3) of the 77 payload bits at the front of a91 (12 bytes, MSB first); rc < 0: a message type
    the firmware does not print (0.1 - 0.4, i3 = 3, 5 and the unspecified tokens)"""
    a77 = [int(b) for b in np.asarray(a91, np.uint8).ravel()[:10]]
    n3 = ((a77[8] << 2) & 0x04) | ((a77[9] >> 6) & 0x03)
    i3 = (a77[9] >> 3) & 0x07
    if i3 == 0 and n3 == 0:
        rc, f1 = unpack_text(a77)
        return rc, f1, "", ""
    if i3 == 0 and n3 == 5:
        rc, f1 = unpack_telemetry(a77)
        return rc, f1, "", ""
    if i3 == 1 or i3 == 2:
        return unpack_type1(a77, i3)
    if i3 == 4:
        return unpack_nonstandard(a77)
    return -1, "", "", ""


SLOT_SAMPLES = 1380 * 128  # a slot of DEMOD_FT8_WAV: 92 blocks of 15 frames of 128 samples at 12 kS/s


def read_wav(path):
    """the samples of a WAV file as an int16 array, with stdlib `wave` alone and load_wav()'s acceptance rules
    (Utility.cpp:830): PCM, one channel, 16 bits; anything else raises ValueError.  Like the firmware it does not ask for
    the sample rate: the collector takes the samples as 12 kS/s."""
    import wave
    try:
        with wave.open(path, "rb") as f:  # (wave itself reads nothing but PCM)
            if f.getcomptype() != "NONE" or f.getnchannels() != 1 or f.getsampwidth() != 2:
                raise ValueError("%s: not a PCM, mono, 16-bit WAV file (channels %d, bytes per sample %d)"
                                 % (path, f.getnchannels(), f.getsampwidth()))
            raw = f.readframes(f.getnframes())
    except wave.Error as e:
        raise ValueError("%s: %s" % (path, e))
    return np.frombuffer(raw, "<i2").astype(np.int16)


def _golden_decode_tables():
    import os
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ft8")
    try:
        ldpc, costas = np.load(os.path.join(d, "ldpc.npz")), np.load(os.path.join(d, "costas.npz"))
    except OSError:
        raise ValueError("decode_recordings: no tables given and none under %s (the library has no table of its own)" % d)
    return costas["kCostas_map"], ldpc["kGray_map"], ldpc["kNm"], ldpc["kMn"], ldpc["kNrw"]


def decode_recordings(recordings, device=0, tables=None):
    """A decode farm on 12 kS/s recordings: a list of int16 arrays of at least 176 640 samples (a 15 s slot; what follows
    is not read) -> per recording the list of its de-duplicated message texts.  One chain with a channel per recording, one
    call of 1380 frames through the collector of DEMOD_FT8_WAV (RxChain.ft8_audio), ft8_decode() on the finished half and
    messages(); the receive chain does not run.  tables = (kCostas_map, kGray_map, kNm, kMn, kNrw) of ft8_constants.cpp; None
    reads the fixtures of a source tree (tests/golden/ft8)."""
    from .rx import RxChain, default_params
    recs = [np.asarray(r) for r in recordings]
    if not recs:
        return []
    for k, r in enumerate(recs):
        if r.dtype != np.int16 or r.ndim != 1 or r.size < SLOT_SAMPLES:
            raise ValueError("recording %d must be a 1-d int16 array of at least %d samples, got %s %r" % (k, SLOT_SAMPLES, r.dtype, r.shape))
    pcm = np.ascontiguousarray(np.stack([r[:SLOT_SAMPLES] for r in recs]))
    rx = RxChain(len(recs), default_params(mode=0), device=device)
    rx.set_ft8_tables()
    rx.set_ft8_decode_tables(*(_golden_decode_tables() if tables is None else tables))
    rx.set_ft8(1, SLOT_SAMPLES // 128)
    rx.ft8_audio_begin()
    done = rx.ft8_audio(pcm)[:, -1, 2].cpu().numpy()
    if (done < 1).any():
        raise RuntimeError("decode_recordings: a slot did not complete in its 1380 frames")
    return [[m["text"] for m in found] for found in messages(rx.ft8_decode(select=done - 1))]


def _cdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def messages(result):
    """per channel the slot's list as ft8_decode() builds newlyDecoded: the candidates in record order with flags == 3 and
    rc >= 0, printed as "%.13s %.13s %.6s", duplicates dropped, at most 10, length below 35.  Every entry is a dict with
    text, field1..3, freq_hz = (int)((freq_offset + freq_sub / 2) * 6.25), score, snr = (min(score, 160) - 160) / 6 as C
    divides, and the candidate's offsets."""
    res = np.atleast_1d(np.asarray(result))
    if res.dtype != RESULT:
        res = res.view(RESULT)
    out = []
    for r in res:
        found = []
        for idx in range(int(r["num_candidates"])):
            c = r["cand"][idx]
            if int(c["flags"]) != 3:
                continue
            rc, f1, f2, f3 = unpack77_fields(c["a91"])
            if rc < 0:
                continue
            text = "%s %s %s" % (f1[:13], f2[:13], f3[:6])
            if any(m["text"] == text for m in found):
                continue
            if len(found) < K_MAX_DECODED_MESSAGES and len(text) < K_MAX_MESSAGE_LENGTH:
                score = int(c["score"])
                freq = np.float32(np.float32(int(c["freq_offset"])) + np.float32(int(c["freq_sub"])) / np.float32(2.0)) * np.float32(6.25)
                found.append(dict(text=text, field1=f1, field2=f2, field3=f3, freq_hz=int(freq), score=score,
                                  snr=_cdiv(min(score, 160) - 160, 6), time_offset=int(c["time_offset"]),
                                  freq_offset=int(c["freq_offset"]), time_sub=int(c["time_sub"]), freq_sub=int(c["freq_sub"])))
        out.append(found)
    return out
