"""FT8 decode of a finished slot: the restatement (tests/ft8_decode_model.py), the package's unpacker and message list
(t41_sdr_amd/ft8.py) and the test-side codec (tests/ft8_codec.py) on their own, no device.  The kernels are held to the
model byte for byte in test_ft8_decode.py.
"""
import numpy as np
import pytest

import ft8_codec as Cd
import ft8_decode_model as D
import ft8_model as M

BP_SLOW_SEED, BP_SLOW_ITER = 1, 4     # Cd.noisy_transmission(seed, ..): found with the model, fixed here
BP_FAIL_SEED, BP_FAIL_ERRORS = 23, 2
WHERE = (3, 200, 1)                   # time_offset, freq_offset, alt of those two


def _msg():
    return Cd.pack_standard("W9XYZ", "K1ABC", "-12")


def _cands(res):
    return [tuple(int(c[k]) for k in ("score", "time_offset", "freq_offset", "time_sub", "freq_sub")) for c in res["cand"][:int(res["num_candidates"])]]


# ---- find_sync ---------------------------------------------------------------------------------------------------------
def test_score_literal_against_vectorised_and_c_division():
    t = D.tables()
    rng = np.random.default_rng(2)
    nb = 64
    p = rng.integers(0, 256, (D.NUM_BLOCKS, 4, nb)).astype(np.uint8)
    sc = D.scores(p, t.costas, num_bins=nb)
    assert sc.shape == (4, 27, nb - 8 - D.MIN_BIN) and sc.min() < 0 < sc.max()
    for alt in range(4):
        for ti, to in enumerate(D.T_OFFSETS):
            for fi in range(sc.shape[2]):
                assert sc[alt, ti, fi] == D.score_literal(p, alt, int(to), D.MIN_BIN + fi, t.costas, num_bins=nb)
    # a constructed negative score: time_offset 0 (21 symbols), one off-Costas bin at 41 in the first symbol, all else zero:
    # the sum is -41, and -41 / 21 is -1 in C (toward zero), not -2
    q = np.zeros((D.NUM_BLOCKS, 4, nb), np.uint8)
    off = [j for j in range(8) if j != int(t.costas[0])][0]
    q[0, 0, D.MIN_BIN + off] = 41
    assert D.score_literal(q, 0, 0, D.MIN_BIN, t.costas, num_bins=nb) == -1
    assert D.scores(q, t.costas, num_bins=nb)[0, 7, 0] == -1 and -41 // 21 == -2 and D.cdiv(-41, 21) == -1


def test_heap_replay_is_not_the_top_20():
    """both cases replayed by hand from ft8.cpp:278-317, 393-414.
    Capacity 3, five entries of score 50 and then one of 51: the first three fill the heap [a0 a1 a2] (heapify_up stops on
    >=), the next two are dropped (eviction is strict), 51 evicts heap[0] = a0: heap[0] = heap[2] = a2, heapify_down finds
    no smaller child, 51 goes in behind.  The survivors among the equal minima are a2 and a1 -- the FIRST one was evicted,
    which no "top 3 by score" with a fixed tie rule gives together with the array order [a2 a1 51]."""
    entries = [(50, i) for i in range(5)] + [(51, 5)]
    heap = D.heap_replay(entries, 3, 40)
    assert heap == [(50, 2), (50, 1), (51, 5)]
    top = sorted(entries, key=lambda e: -e[0])[:3]  # stable: the earliest of equal scores
    assert top == [(51, 5), (50, 0), (50, 1)] and sorted(heap) != sorted(top)
    top_last = sorted(reversed(entries), key=lambda e: -e[0])[:3]  # the latest of equal scores
    assert top_last == [(51, 5), (50, 4), (50, 3)] and sorted(heap) != sorted(top_last)
    # capacity 4: 50 50 50 60 | 61 62 evict two of the 50s, a 50 is dropped, 70 evicts the last 50, 50 and 55 are dropped
    # (55 < heap[0] = 60).  The array ends as [60 62 61 70]: heap order, neither sorted nor arrival order
    entries = [(50, i) for i in range(3)] + [(60 + i, 10 + i) for i in range(3)] + [(50, 99), (70, 100), (50, 101), (55, 102)]
    heap = D.heap_replay(entries, 4, 40)
    assert heap == [(60, 10), (62, 12), (61, 11), (70, 100)]
    assert heap != sorted(heap) and heap != sorted(heap, reverse=True)
    assert D.heap_replay([(39, 0), (40, 1)], 3, 40) == [(40, 1)]  # score < min_score skips


# ---- round trips -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [(-7, 48, 0), (19, 359, 3), (0, 100, 2), (3, 200, 1)])
def test_painted_message_round_trips(where):
    from t41_sdr_amd import ft8 as F
    a77 = _msg()
    tones, cw = Cd.encode(a77)
    assert D.ldpc_check(cw) == 0 and D.crc_matches(Cd.a91_of(a77))  # the encoder against the decoder's tables
    wf = Cd.paint(Cd.blank(0), tones, where[0], where[1], where[2], 120, 40)
    res, log174, plain = D.decode(wf)
    want = (where[0], where[1], where[2] // 2, where[2] % 2)
    hit = [i for i, c in enumerate(_cands(res)) if c[1:] == want]
    assert len(hit) == 1
    c = res["cand"][hit[0]]
    assert c["n_errors"] == 0 and c["iterations"] == 0 and c["flags"] == 3 and c["score"] == 560
    assert np.array_equal(c["a91"], Cd.a91_of(a77)) and np.array_equal(plain[hit[0]], cw)
    msgs = F.messages(res)[0]
    assert [m["text"] for m in msgs] == ["W9XYZ K1ABC -12"]
    assert msgs[0]["freq_hz"] == int((where[1] + (where[2] % 2) / 2) * 6.25) and msgs[0]["snr"] == 0 and msgs[0]["score"] == 560


def test_flipped_payload_bit_fails_crc_or_parity():
    a77 = _msg()
    _, cw = Cd.encode(a77)
    for bit in (0, 40, 76):
        bad = cw.copy()
        bad[bit] ^= 1
        assert D.ldpc_check(bad) > 0  # a single flipped bit always breaks its three checks
        a91 = D.pack_bits(bad, D.K)
        assert not D.crc_matches(a91)
    # flipping the payload BEFORE the parity is computed keeps the parity and fails the CRC
    bits = Cd.add_crc(a77)
    bits[5] ^= 1
    cw2 = Cd.encode174(bits)
    assert D.ldpc_check(cw2) == 0 and not D.crc_matches(D.pack_bits(cw2, D.K))


# ---- bp_decode ---------------------------------------------------------------------------------------------------------
def test_bp_cases_stay_non_trivial():
    t = D.tables()
    tones, cw = Cd.encode(_msg())
    cand = (0, WHERE[0], WHERE[1], WHERE[2] // 2, WHERE[2] % 2)
    slow = D.extract_likelihood(Cd.noisy_transmission(BP_SLOW_SEED, tones), cand, t.gray)
    plain, n_errors, it = D.bp_decode(slow)
    assert (n_errors, it) == (0, BP_SLOW_ITER) and it >= 2 and np.array_equal(plain, cw)
    assert D.ldpc_check((slow > 0).astype(np.uint8)) > 0  # the hard decision of the input is no codeword
    lit = D.bp_decode_literal(slow)
    assert np.array_equal(lit[0], plain) and lit[1:] == (n_errors, it)  # the loops as written against the vectorised form
    fail = D.extract_likelihood(Cd.noisy_transmission(BP_FAIL_SEED, tones), cand, t.gray)
    plain, n_errors, it = D.bp_decode(fail)
    assert (n_errors, it) == (BP_FAIL_ERRORS, D.LDPC_ITERATIONS) and n_errors > 0
    lit = D.bp_decode_literal(fail)
    assert np.array_equal(lit[0], plain) and lit[1:] == (n_errors, it)
    assert D.bp_decode(slow, 1)[1:] == (D.ldpc_check((slow > 0).astype(np.uint8)), 1)


def test_zero_variance_gives_nan_and_the_all_zero_codeword():
    """the firmware's quirk: a flat symbol field has log174 = 0, variance 0, norm_factor inf, 0 * inf = NaN; zn > 0 is
    false everywhere, plain is all zero, and the all-zero codeword passes ldpc_check() and the CRC"""
    log174 = D.normalise(np.zeros(D.N, np.float32))
    assert np.isnan(log174).all()
    plain, n_errors, it = D.bp_decode(log174)
    assert not plain.any() and (n_errors, it) == (0, 0)
    assert D.crc_matches(D.pack_bits(plain, D.K))
    # a silent slot searched with min_score 0: the first three entries of the loop (score 0) fill the heap and nothing evicts
    # them; each "decodes" to the all-zero payload
    res, log_all, plain_all = D.decode(Cd.blank(0), min_score=0, max_candidates=3)
    assert _cands(res) == [(0, -7, 48, 0, 0), (0, -7, 49, 0, 0), (0, -7, 50, 0, 0)]
    assert (res["cand"]["flags"][:3] == 3).all() and res["num_valid"] == 3 and not res["cand"]["a91"].any()
    assert np.isnan(log_all[:3]).all() and not plain_all.any()
    # a negative variance (rounding) is NaN too
    with np.errstate(all="ignore"):
        assert np.isnan(np.sqrt(np.float32(16.0) / np.float32(-1e-3)))


# ---- unpack ------------------------------------------------------------------------------------------------------------
UNPACK = [
    (lambda: Cd.pack_standard("CQ", "K1ABC", "FN42"), "CQ K1ABC FN42"),
    (lambda: Cd.pack_standard("CQ 123", "K1ABC", "FN42"), "CQ +123 K1ABC FN42"),   # int_to_dd(.., full_sign)
    (lambda: Cd.pack_standard("CQ TEST", "K1ABC", "FN42"), "CQ TEST K1ABC FN42"),
    (lambda: Cd.pack_standard("CQ DX", "G4ABC", "IO91"), "CQ DX G4ABC IO91"),
    (lambda: Cd.pack_standard("DE", "K1ABC", "FN42"), "DE K1ABC FN42"),
    (lambda: Cd.pack_standard("QRZ", "K1ABC", ""), "QRZ K1ABC "),
    (lambda: Cd.pack_standard("W9XYZ", "K1ABC/R", "R FN42"), "W9XYZ K1ABC/R R FN42"),
    (lambda: Cd.pack_standard("G4ABC/P", "PA9XYZ", "JO22", i3=2), "G4ABC/P PA9XYZ JO22"),
    (lambda: Cd.pack_standard("W9XYZ", "K1ABC", "-12"), "W9XYZ K1ABC -12"),
    (lambda: Cd.pack_standard("W9XYZ", "K1ABC", "+05"), "W9XYZ K1ABC +05"),
    (lambda: Cd.pack_standard("W9XYZ", "K1ABC", "R-07"), "W9XYZ K1ABC R-07"),
    (lambda: Cd.pack_standard("W9XYZ", "K1ABC", "RRR"), "W9XYZ K1ABC RRR"),
    (lambda: Cd.pack_standard("W9XYZ", "K1ABC", "RR73"), "W9XYZ K1ABC RR73"),
    (lambda: Cd.pack_standard("W9XYZ", "K1ABC", "73"), "W9XYZ K1ABC 73"),
    (lambda: Cd.pack_standard("W9XYZ", "K1ABC", ""), "W9XYZ K1ABC "),
    (lambda: Cd.pack_standard("<1234567>", "K1ABC", "FN42"), "<+123456> K1ABC FN42"),  # '>' lands on the seventh digit
    (lambda: Cd.pack_standard("<42>", "K1ABC", "FN42"), "<+000004> K1ABC FN42"),
    (lambda: Cd.pack_free_text("HELLO WORLD"), "HELLO WORLD  "),
    (lambda: Cd.pack_free_text("TNX BOB 73 GL"), "TNX BOB 73 GL  "),
    (lambda: Cd.pack_free_text("+-./?"), "+-./?  "),
    (lambda: Cd.pack_telemetry("0123456789ABCDEF01"), "0123456789ABC  "),             # %.13s of 18 digits
    (lambda: Cd.pack_type4(1234, "PJ4/K1ABC", True, nrpt=2), "<+123> PJ4/K1ABC RR73"),  # '>' lands on the fourth digit
    (lambda: Cd.pack_type4(7, "PJ4/K1ABC", False, nrpt=1), "PJ4/K1ABC <+000> RRR"),
    (lambda: Cd.pack_type4(7, "YW18FIFA", True, nrpt=3), "<+000> YW18FIFA 73"),
    (lambda: Cd.pack_type4(7, "YW18FIFA", True, icq=1), "CQ YW18FIFA "),
]


@pytest.mark.parametrize("k", range(len(UNPACK)))
def test_unpack_round_trips(k):
    from t41_sdr_amd import ft8 as F
    make, text = UNPACK[k]
    a77 = make()
    rc, f1, f2, f3 = F.unpack77_fields(Cd.a91_of(a77))
    assert rc == 0 and "%s %s %s" % (f1[:13], f2[:13], f3[:6]) == text
    if k == 20:
        assert f1 == "0123456789ABCDEF01"


def test_unpack_refuses_the_other_types():
    from t41_sdr_amd import ft8 as F
    for i3, n3 in ((3, 0), (5, 0), (0, 1), (0, 2), (0, 3), (0, 4), (0, 6), (6, 0), (7, 0)):
        assert F.unpack77_fields(Cd.pack_raw(i3, n3, body=12345))[0] == -1, (i3, n3)
    # a token the protocol leaves unspecified (532444 .. NTOKENS - 1) in either call
    v = ((600000 << 1) << 29 | (Cd.pack28("K1ABC") << 1)) << 16 | (Cd.MAXGRID4 + 1)
    assert F.unpack77_fields(Cd._bits_to_a77((v << 3) | 1))[0] == -1
    v = ((Cd.pack28("K1ABC") << 1) << 29 | (600000 << 1)) << 16 | (Cd.MAXGRID4 + 1)
    assert F.unpack77_fields(Cd._bits_to_a77((v << 3) | 1))[0] == -2
    assert F.charn(41, 0) == "?" and F.charn(42, 0) == "_" and F.int_to_dd(-5, 2, True) == "-05" and F.trim("  A B  ") == "A B"
    assert F.int_to_dd(332, 2, True) == "+Q2"  # a digit past 9 is the character behind '9'


def _result_of(payloads, flags=None, scores=None):
    from t41_sdr_amd import ft8 as F
    r = np.zeros(1, F.RESULT)
    r["num_candidates"] = len(payloads)
    for i, a77 in enumerate(payloads):
        c = r["cand"][0, i]
        c["a91"] = Cd.a91_of(a77)
        c["flags"] = 3 if flags is None else flags[i]
        c["score"] = 100 + i if scores is None else scores[i]
        c["freq_offset"], c["freq_sub"] = 100 + i, i % 2
    return r


def test_messages_dedup_caps_and_fields():
    from t41_sdr_amd import ft8 as F
    assert F.CANDIDATE == D.CAND and F.RESULT == D.RESULT
    a, b = Cd.pack_standard("CQ", "K1ABC", "FN42"), Cd.pack_standard("W9XYZ", "K1ABC", "-12")
    r = _result_of([a, b, a, Cd.pack_raw(3), b, b], flags=[3, 3, 3, 3, 1, 2], scores=[100, 166, 100, 100, 100, 100])
    m = F.messages(r)[0]
    assert [x["text"] for x in m] == ["CQ K1ABC FN42", "W9XYZ K1ABC -12"]  # the duplicate, the refused type, flags != 3 dropped
    assert m[0]["snr"] == -10 and m[0]["freq_hz"] == 625 and m[1]["snr"] == 0 and m[1]["freq_hz"] == int(101.5 * 6.25)
    assert F._cdiv(99 - 160, 6) == -10 and (99 - 160) // 6 == -11  # C truncation
    many = [Cd.pack_standard("CQ", "K1ABC", "FN%02d" % i) for i in range(14)]
    m = F.messages(_result_of(many))[0]
    assert len(m) == 10 and m[-1]["text"] == "CQ K1ABC FN09"  # kMax_decoded_messages
    # length below 35: 13 + 1 + 13 + 1 + 6 = 34 is the longest there is, so the cap never cuts; a record array of several
    # channels gives one list each
    r2 = np.concatenate([_result_of([a]), _result_of([])])
    assert [len(x) for x in F.messages(r2)] == [1, 0]


# ---- end to end on the models ------------------------------------------------------------------------------------------
def test_audio_through_the_waterfall_model_decodes():
    """an encoded message as audio (0.14 of the q15 range, symbol s in gulp s, tone 0 at row 160) through FT8Model; the
    decode model reads its waterfall.  The strongest candidate is the one test_ft8_model.py predicts: time_offset 0, row
    160, time_sub 1 (the window centred on the middle third), freq_sub 0; it decodes at iteration 0.  The log-scaled rows
    are broad, so neighbouring candidates decode the same message too: messages() keeps one."""
    from t41_sdr_amd import ft8 as F
    tones, cw = Cd.encode(_msg())
    w, m = M.ft8_tables()
    mod = M.FT8Model(1, w, m)
    mod.collect = M.collect_closed_form
    mod.sync()
    mod.process(Cd.audio(tones)[None, :])
    res, _, plain = D.decode(mod.power[0, 0])
    cands = _cands(res)
    print(cands, res["cand"]["flags"])
    best = int(np.argmax([c[0] for c in cands]))
    assert cands[best][1:] == (0, 160, 1, 0) and res["cand"][best]["flags"] == 3 and res["cand"][best]["iterations"] == 0
    assert np.array_equal(plain[best], cw)
    msgs = F.messages(res)[0]
    assert [x["text"] for x in msgs] == ["W9XYZ K1ABC -12"] and res["num_valid"] >= 1


# ---- ABI and bindings --------------------------------------------------------------------------------------------------
NEW = ("t41rx_set_ft8_decode_tables", "t41rx_set_ft8_decode", "t41rx_get_ft8_decode", "t41rx_set_ft8_decode_debug",
       "t41rx_ft8_decode_device", "t41rx_ft8_decode_host")


def test_entry_points_declared_exported_and_bound(built):
    import ctypes as C
    import os
    import re
    import t41_sdr_amd as T
    import t41_sdr_amd._lib as lib
    from rx_harness import assert_entry_points
    root = D.ROOT
    hdr = assert_entry_points(NEW, ("set_ft8_decode_tables", "set_ft8_decode", "ft8_decode_params", "ft8_decode"), abi_version=5,
                              pattern=r"T41RX_API\s+int\s+%s\s*\(")
    assert callable(T.ft8.unpack77_fields) and callable(T.ft8.messages)
    assert lib.load().t41rx_abi_version() == 5
    assert not open(os.path.join(root, "include", "t41tx.h")).read().count("ft8")
    assert "#define T41RX_FT8_MAX_CANDIDATES 20" in hdr and "#define T41RX_FT8_SLOT_BYTES 135424" in hdr and 92 * 1472 == 135424

    class Cand(C.Structure):  # the header's structs, field for field
        _fields_ = [("score", C.c_int16), ("time_offset", C.c_int16), ("freq_offset", C.c_int16), ("time_sub", C.c_uint8),
                    ("freq_sub", C.c_uint8), ("n_errors", C.c_int16), ("iterations", C.c_uint8), ("flags", C.c_uint8),
                    ("a91", C.c_uint8 * 12), ("reserved", C.c_uint8 * 8)]

    class Result(C.Structure):
        _fields_ = [("num_candidates", C.c_int32), ("num_valid", C.c_int32), ("select", C.c_int32), ("reserved", C.c_int32),
                    ("cand", Cand * 20)]
    assert C.sizeof(Cand) == 32 == T.ft8.CANDIDATE.itemsize and C.sizeof(Result) == 656 == T.ft8.RESULT.itemsize
    for f, _ in Cand._fields_:
        assert getattr(Cand, f).offset == T.ft8.CANDIDATE.fields[f][1], f
    for f, _ in Result._fields_:
        assert getattr(Result, f).offset == T.ft8.RESULT.fields[f][1], f
    body = re.search(r"typedef struct \{([^}]*)\} t41rx_ft8_candidate;", hdr).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?[,;]", body) == [f for f, _ in Cand._fields_]
