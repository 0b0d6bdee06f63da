"""Test-side FT8 helpers: a message packer written from the protocol's field layout (the 77-bit message types of the FT4 /
FT8 protocol description; NOT derived from the unpacker under test), the encoder (77 bits + CRC-14 -> kGenerator -> 174
bits -> Gray map -> 79 tones with Costas arrays at 0 / 36 / 72) and paint(), which writes a transmission into a waterfall.
"""
import numpy as np

import ft8_decode_model as D

NTOKENS, MAX22, MAXGRID4 = 2063592, 4194304, 32400
A0 = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ+-./?"   # free text
A1 = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"        # first character of a call
A2 = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"         # second
A3 = "0123456789"                                    # third: the call area digit
A4 = " ABCDEFGHIJKLMNOPQRSTUVWXYZ"                   # suffix
A5 = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ/"       # nonstandard calls


# ---- packer ------------------------------------------------------------------------------------------------------------
def pack28(call):
    """a call, a token (DE, QRZ, CQ, "CQ 123", "CQ TEST") or a 22-bit hash given as "<n>" -> n28"""
    if call == "DE":
        return 0
    if call == "QRZ":
        return 1
    if call == "CQ":
        return 2
    if call.startswith("CQ "):
        rest = call[3:]
        if rest.isdigit():
            assert len(rest) == 3
            return 3 + int(rest)
        assert 1 <= len(rest) <= 4 and rest.isalpha()
        n = 0
        for ch in rest.rjust(4):
            n = n * 27 + A4.index(ch)
        return 1003 + n
    if call.startswith("<"):
        h = int(call[1:-1])
        assert 0 <= h < MAX22
        return NTOKENS + h
    c = call
    if len(c) >= 3 and c[2].isdigit():
        c6 = c
    else:
        assert c[1].isdigit(), call
        c6 = " " + c
    c6 = c6.ljust(6)
    assert len(c6) == 6, call
    n = A1.index(c6[0])
    n = n * 36 + A2.index(c6[1])
    n = n * 10 + A3.index(c6[2])
    for ch in c6[3:]:
        n = n * 27 + A4.index(ch)
    return NTOKENS + MAX22 + n


def pack_grid_or_report(extra):
    """-> (ir, igrid4) for a grid, "R " + grid, a report "+05" / "-12" / "R-07", RRR, RR73, 73 or the empty string"""
    if extra == "":
        return 0, MAXGRID4 + 1
    if extra in ("RRR", "RR73", "73"):
        return 0, MAXGRID4 + {"RRR": 2, "RR73": 3, "73": 4}[extra]
    ir = 0
    if extra.startswith("R ") or (extra[0] == "R" and extra[1] in "+-"):
        ir, extra = 1, extra[1:].strip()
    if extra[0] in "+-":
        return ir, MAXGRID4 + 35 + int(extra)
    g = extra
    assert len(g) == 4
    return ir, ((ord(g[0]) - 65) * 18 + (ord(g[1]) - 65)) * 100 + int(g[2:])


def _bits_to_a77(value):
    """a 77-bit integer -> 10 bytes, MSB first, the last three bits zero"""
    assert 0 <= value < (1 << 77)
    return np.frombuffer((value << 3).to_bytes(10, "big"), np.uint8).copy()


def pack_standard(call_to, call_de, extra, i3=1):
    """type 1 (i3 = 1, suffix /R) or 2 (i3 = 2, suffix /P): n28a ipa n28b ipb ir igrid4 i3 = 28 1 28 1 1 15 3 bits"""
    def split(c):
        for suf in ("/R", "/P"):
            if c.endswith(suf):
                assert (suf == "/R") == (i3 == 1)
                return c[:-2], 1
        return c, 0
    a, ipa = split(call_to)
    b, ipb = split(call_de)
    ir, igrid4 = pack_grid_or_report(extra)
    v = pack28(a)
    v = (v << 1) | ipa
    v = (v << 28) | pack28(b)
    v = (v << 1) | ipb
    v = (v << 1) | ir
    v = (v << 15) | igrid4
    v = (v << 3) | i3
    return _bits_to_a77(v)


def pack_free_text(text):
    """type 0.0: 13 characters to base 42, 71 bits; n3 = 0, i3 = 0"""
    assert len(text) <= 13
    n = 0
    for ch in text.rjust(13):
        n = n * 42 + A0.index(ch)
    assert n < (1 << 71)
    return _bits_to_a77(n << 6)


def pack_telemetry(hex18):
    """type 0.5: 71 bits of telemetry as 18 hex digits; n3 = 5, i3 = 0"""
    n = int(hex18, 16)
    assert len(hex18) == 18 and n < (1 << 71)
    return _bits_to_a77((n << 6) | (5 << 3))


def pack_type4(hash12, call, hashed_first, nrpt=0, icq=0):
    """type 4: n12 n58 iflip nrpt icq i3 = 12 58 1 2 1 3 bits; iflip = 1 when the hashed call is the second one"""
    assert 0 <= hash12 < 4096 and len(call) <= 11
    n58 = 0
    for ch in call.rjust(11):
        n58 = n58 * 38 + A5.index(ch)
    v = hash12
    v = (v << 58) | n58
    v = (v << 1) | (0 if hashed_first else 1)
    v = (v << 2) | nrpt
    v = (v << 1) | icq
    v = (v << 3) | 4
    return _bits_to_a77(v)


def pack_raw(i3, n3=0, body=0):
    """any other type: 71 (i3 = 0) or 74 body bits, then n3 / i3"""
    return _bits_to_a77((body << 6) | (n3 << 3) | i3) if i3 == 0 else _bits_to_a77((body << 3) | i3)


# ---- encoder -----------------------------------------------------------------------------------------------------------
def crc14(bits):
    """CRC-14 (polynomial 0x6757 with its leading 1) by long division of a bit sequence, written independently of crc()"""
    poly = [int(b) for b in "110011101010111"]
    r = list(bits) + [0] * 14
    for i in range(len(bits)):
        if r[i]:
            for j, p in enumerate(poly):
                r[i + j] ^= p
    return r[-14:]


def add_crc(a77):
    """10 payload bytes -> 91 bits: the 77 message bits and the CRC-14 of the message zero-extended to 82 bits"""
    bits = list(np.unpackbits(np.asarray(a77, np.uint8))[:77])
    return np.array(bits + crc14(bits + [0] * 5), np.uint8)


def encode174(bits91, t=None):
    t = t or D.tables()
    gen = np.unpackbits(t.generator, axis=1)[:, :D.K]  # [83][91]
    parity = (gen.astype(np.int64) @ np.asarray(bits91, np.int64)) % 2
    return np.concatenate([bits91, parity.astype(np.uint8)])


def tones_of(codeword, t=None):
    t = t or D.tables()
    sym = codeword.reshape(D.ND, 3)
    data = t.gray[(sym[:, 0] << 2) | (sym[:, 1] << 1) | sym[:, 2]]
    tones = np.zeros(D.NN, np.int64)
    for s0 in (0, 36, 72):
        tones[s0:s0 + 7] = t.costas
    tones[7:36] = data[:29]
    tones[43:72] = data[29:]
    return tones


def encode(a77):
    """10 payload bytes -> (79 tones, 174 codeword bits)"""
    cw = encode174(add_crc(a77))
    return tones_of(cw), cw


def a91_of(a77):
    return np.packbits(np.concatenate([add_crc(a77), np.zeros(5, np.uint8)]))


# ---- waterfall ---------------------------------------------------------------------------------------------------------
def blank(floor=0):
    return np.full((D.NUM_BLOCKS, 4, D.NUM_BINS), floor, np.uint8)


def paint(wf, tones, time_offset, freq_offset, alt, level, floor):
    """writes a transmission into a [92][4][368] uint8 waterfall: symbol s sits in block time_offset + s (symbols outside
    the slot are lost), its eight bins at freq_offset read `floor`, the tone's bin `level`"""
    for s, tone in enumerate(tones):
        r = time_offset + s
        if 0 <= r < D.NUM_BLOCKS:
            wf[r, alt, freq_offset:freq_offset + 8] = floor
            wf[r, alt, freq_offset + int(tone)] = level
    return wf


def noisy_transmission(seed, tones, amp=50, level=70, floor=40, where=(3, 200, 1)):
    """a weak transmission (tone bins `level` over `floor`) under uniform byte noise 0 .. amp - 1 on the whole slot"""
    wf = paint(blank(0), tones, where[0], where[1], where[2], level, floor)
    rng = np.random.default_rng(seed)
    return np.clip(wf.astype(np.int64) + rng.integers(0, amp, wf.shape), 0, 255).astype(np.uint8)


def audio(tones, amp=0.14, j0=160):
    """the transmission as audio @24 kS/s: 8-FSK, 6.25 Hz spacing, tone 0 at j0 x 6.25 Hz, 0.16 s = 3840 samples = 15 frames
    per symbol, continuous phase, from a gulp boundary (test_ft8_model._transmission's form)"""
    f = np.repeat(6.25 * (j0 + np.asarray(tones)), 3840)
    ph = 2 * np.pi * np.cumsum(f) / 24000.0
    return (amp * np.sin(ph)).astype(np.float32)
