"""FT8 decode of a finished slot, restated in numpy: find_sync(), extract_likelihood(), bp_decode(), pack_bits(), crc() and
the loop of ft8_decode() up to the CRC check (ft8.cpp:270-616, 669-703, 727-790), operation for operation, quirks included.
ft8_decode_kernel.hip is held to this model byte for byte (tests/test_ft8_decode.py).

The waterfall is export_fft_power of one slot: [92 blocks][4 alts = 2 * time_sub + freq_sub][368 bins] uint8.

find_sync        integer arithmetic.  Loop order alt 0..3, time_offset -7..19, freq_offset 48..359; the score is the sum of
                 8 * p8[sync_map[k]] - (p8[0] + .. + p8[7]) over the Costas symbols that fall inside blocks 0..91, divided by
                 their number as C divides (toward zero; scores can be negative); `score < min_score` skips.  The min-heap is
                 replayed as written: eviction only on score > heap[0].score (strictly), heap[0] = heap[last] and
                 heapify_down, then insertion and heapify_up (which stops on >=).  The result is the heap ARRAY in array
                 order, the order ft8_decode() walks: which of several equal-minimum candidates survives and where every
                 candidate ends up hangs on the replay -- it is not "the top 20".
extract_likelihood  time_offset may be negative; the data symbols still lie inside the slot.  log174 are max4 differences of
                 uint8 values, exact integers in f32; sum and sum2 are integers below 2^24 (174 * 255^2 = 11 314 350), exact
                 in any summation order.  variance = (sum2 - sum * sum * inv_n) * inv_n and norm_factor = sqrtf(16.0f /
                 variance) in f32, one rounding per operation.  FIRMWARE QUIRK: variance 0 gives inf and 0 * inf = NaN in
                 log174, a negative variance gives NaN; NaN is carried as IEEE does: zn > 0 is false, plain is all zero, the
                 all-zero codeword passes ldpc_check() and the CRC (crc of zeros is 0), so such a candidate "decodes".
bp_decode        f32, every expression in source order, one rounding per operation, IEEE division: zn = codeword + tov0 +
                 tov1 + tov2; fast_tanh(-toc / 2) with its +-4.97 clamps; Tmn the product over the check's entries in index
                 order k, skipping bit i; 2 * fast_atanh(-Tmn).  plain is the hard decision of the last iteration begun, not
                 of the best one; *ok = min_errors.  The model also records iter at exit: the index of the iteration whose
                 check found 0 errors, else max_iters.
pack_bits, crc   MSB first; CRC-14 (polynomial 0x2757, initalize_constants()) over 82 bits of the masked copy.

What this leaves unpinned: the firmware's compiler may fuse a * b + c on the Cortex-M7; the restatement fixes one rounding
per operation, as every f32 restatement here does ("FT8 decode").
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NN, ND, N, K, M = 79, 58, 174, 91, 83
NUM_BLOCKS, NUM_BINS, MIN_BIN = 92, 368, 48
SLOT_BYTES = NUM_BLOCKS * 4 * NUM_BINS
MAX_CANDIDATES, MIN_SCORE, LDPC_ITERATIONS = 20, 40, 10
CRC_POLYNOMIAL, CRC_WIDTH = 0x2757, 14
T_OFFSETS = np.arange(-7, NUM_BLOCKS - NN + 7)  # -7 .. 19
f32 = np.float32

CAND = np.dtype([("score", "<i2"), ("time_offset", "<i2"), ("freq_offset", "<i2"), ("time_sub", "u1"), ("freq_sub", "u1"),
                 ("n_errors", "<i2"), ("iterations", "u1"), ("flags", "u1"), ("a91", "u1", (12,)), ("reserved", "u1", (8,))])
RESULT = np.dtype([("num_candidates", "<i4"), ("num_valid", "<i4"), ("select", "<i4"), ("reserved", "<i4"),
                   ("cand", CAND, (MAX_CANDIDATES,))])
assert CAND.itemsize == 32 and RESULT.itemsize == 656


class Tables:
    """kCostas_map, kGray_map, kNm, kMn, kNrw (and the tests' kGenerator) from tests/golden/ft8/"""

    def __init__(self):
        d = np.load(os.path.join(ROOT, "tests", "golden", "ft8", "ldpc.npz"))
        self.costas = np.load(os.path.join(ROOT, "tests", "golden", "ft8", "costas.npz"))["kCostas_map"].astype(np.uint8)
        self.gray, self.nm, self.mn, self.nrw, self.generator = (d[k] for k in ("kGray_map", "kNm", "kMn", "kNrw", "kGenerator"))


_tables = None


def tables():
    global _tables
    if _tables is None:
        _tables = Tables()
    return _tables


# ---- find_sync ---------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    """C's int division: toward zero"""
    q = abs(int(a)) // abs(int(b))
    return q if (a >= 0) == (b > 0) else -q


def score_literal(power, alt, time_offset, freq_offset, sync_map, num_blocks=NUM_BLOCKS, num_bins=NUM_BINS):
    """the score loop of find_sync() as written (ft8.cpp:347-390), on the flat waterfall"""
    p = np.asarray(power, np.uint8).ravel()
    score, num_symbols = 0, 0
    for m in (0, 36, 72):
        for k in range(7):
            if time_offset + k + m < 0:
                continue
            if time_offset + k + m >= num_blocks:
                break
            offset = ((time_offset + k + m) * 4 + alt) * num_bins + freq_offset
            p8 = p[offset:offset + 8].astype(np.int64)
            score += 8 * int(p8[int(sync_map[k])]) - int(p8.sum())
            num_symbols += 1
    return cdiv(score, num_symbols)


def scores(power, sync_map, num_blocks=NUM_BLOCKS, num_bins=NUM_BINS, min_bin=MIN_BIN):
    """every score of find_sync() at once: [4 alts][time_offset -7 .. num_blocks - 73][freq_offset min_bin .. num_bins - 9]"""
    p = np.asarray(power, np.uint8).reshape(num_blocks, 4, num_bins).astype(np.int64)
    t_off = np.arange(-7, num_blocks - NN + 7)
    nf = num_bins - 8 - min_bin
    fo = min_bin + np.arange(nf)
    csum = np.concatenate([np.zeros((num_blocks, 4, 1), np.int64), np.cumsum(p, axis=2)], axis=2)
    s8 = csum[:, :, fo + 8] - csum[:, :, fo]  # [block][alt][f]
    total = np.zeros((4, t_off.size, nf), np.int64)
    count = np.zeros(t_off.size, np.int64)
    for m in (0, 36, 72):
        for k in range(7):
            sym = t_off + k + m
            ok = (sym >= 0) & (sym < num_blocks)
            s = np.clip(sym, 0, num_blocks - 1)
            term = 8 * p[s][:, :, fo + int(sync_map[k])] - s8[s]  # [t][alt][f]
            total += np.where(ok[None, :, None], term.transpose(1, 0, 2), 0)
            count += ok
    q = np.abs(total) // count[None, :, None]
    return np.where(total < 0, -q, q)


def heapify_down(heap, heap_size):
    current = 0
    while True:
        largest, left = current, 2 * current + 1
        right = left + 1
        if left < heap_size and heap[left][0] < heap[largest][0]:
            largest = left
        if right < heap_size and heap[right][0] < heap[largest][0]:
            largest = right
        if largest == current:
            break
        heap[largest], heap[current] = heap[current], heap[largest]
        current = largest


def heapify_up(heap, heap_size):
    current = heap_size - 1
    while current > 0:
        parent = (current - 1) // 2
        if heap[current][0] >= heap[parent][0]:
            break
        heap[parent], heap[current] = heap[current], heap[parent]
        current = parent


def heap_replay(entries, num_candidates, min_score, stats=None):
    """find_sync()'s heap (ft8.cpp:393-414) over entries (score, ...) in loop order; returns the heap array"""
    heap = []
    for e in entries:
        if e[0] < min_score:
            continue
        if stats is not None and len(heap) == num_candidates:
            stats["full"] = True
            if e[0] == heap[0][0]:
                stats["tie_at_minimum"] = stats.get("tie_at_minimum", 0) + 1
        if len(heap) == num_candidates and e[0] > heap[0][0]:
            heap[0] = heap[-1]
            heap.pop()
            heapify_down(heap, len(heap))
        if len(heap) < num_candidates:
            heap.append(tuple(e))
            heapify_up(heap, len(heap))
    return heap


def find_sync(power, sync_map, num_candidates=MAX_CANDIDATES, min_score=MIN_SCORE, stats=None):
    """-> the heap array as a list of (score, time_offset, freq_offset, time_sub, freq_sub)"""
    sc = scores(power, sync_map)
    alt, ti, fi = np.nonzero(sc >= min_score)  # C order = the firmware's loop order
    entries = [(int(sc[a, t, f]), int(t) - 7, int(f) + MIN_BIN, int(a) // 2, int(a) % 2) for a, t, f in zip(alt, ti, fi)]
    if stats is not None:
        stats["qualifying"] = len(entries)
    return heap_replay(entries, num_candidates, min_score, stats)


# ---- extract_likelihood ------------------------------------------------------------------------------------------------
def max4(a, b, c, d):
    return np.maximum(np.maximum(a, b), np.maximum(c, d))


def extract_likelihood(power, cand, code_map):
    """-> log174 [174] f32"""
    p = np.asarray(power, np.uint8).reshape(NUM_BLOCKS, 4, NUM_BINS)
    _, time_offset, freq_offset, time_sub, freq_sub = cand
    k = np.arange(ND)
    sym = np.where(k < ND // 2, k + 7, k + 14) + time_offset
    assert sym.min() >= 0 and sym.max() < NUM_BLOCKS
    s2 = p[sym, 2 * time_sub + freq_sub][:, freq_offset + np.asarray(code_map, np.int64)].astype(f32)  # [58][8]
    log174 = np.empty((ND, 3), f32)
    log174[:, 0] = max4(s2[:, 4], s2[:, 5], s2[:, 6], s2[:, 7]) - max4(s2[:, 0], s2[:, 1], s2[:, 2], s2[:, 3])
    log174[:, 1] = max4(s2[:, 2], s2[:, 3], s2[:, 6], s2[:, 7]) - max4(s2[:, 0], s2[:, 1], s2[:, 4], s2[:, 5])
    log174[:, 2] = max4(s2[:, 1], s2[:, 3], s2[:, 5], s2[:, 7]) - max4(s2[:, 0], s2[:, 2], s2[:, 4], s2[:, 6])
    return normalise(log174.ravel())


def normalise(log174):
    """the variance and norm_factor of extract_likelihood() (ft8.cpp:447-461) on integer-valued log174"""
    log174 = np.asarray(log174, f32)
    li = log174.astype(np.int64)
    assert np.array_equal(li.astype(f32), log174)
    s, s2 = f32(int(li.sum())), f32(int((li * li).sum()))  # integers below 2^24: the f32 running sums are exact
    assert abs(int(li.sum())) < 2 ** 24 and int((li * li).sum()) < 2 ** 24
    with np.errstate(all="ignore"):
        inv_n = f32(1.0) / f32(N)
        variance = f32(f32(s2 - f32(f32(s * s) * inv_n)) * inv_n)
        norm_factor = np.sqrt(f32(f32(16.0) / variance))
        return (log174 * f32(norm_factor)).astype(f32)


# ---- bp_decode ---------------------------------------------------------------------------------------------------------
def ldpc_check(codeword, t=None):
    t = t or tables()
    errors = 0
    for j in range(M):
        x = 0
        for i in range(int(t.nrw[j])):
            x ^= int(codeword[int(t.nm[j, i]) - 1])
        errors += x != 0
    return errors


def fast_tanh(x):
    with np.errstate(all="ignore"):
        x = np.asarray(x, f32)
        x2 = x * x
        a = x * (f32(945.0) + x2 * (f32(105.0) + x2))
        b = f32(945.0) + x2 * (f32(420.0) + x2 * f32(15.0))
        return np.where(x < f32(-4.97), f32(-1.0), np.where(x > f32(4.97), f32(1.0), a / b)).astype(f32)


def fast_atanh(x):
    with np.errstate(all="ignore"):
        x = np.asarray(x, f32)
        x2 = x * x
        a = x * (f32(945.0) + x2 * (f32(-735.0) + x2 * f32(64.0)))
        b = f32(945.0) + x2 * (f32(-1050.0) + x2 * f32(225.0))
        return (a / b).astype(f32)


def bp_decode(codeword, max_iters=LDPC_ITERATIONS, t=None):
    """-> (plain [174] uint8, min_errors, iter at exit)"""
    t = t or tables()
    cw = np.asarray(codeword, f32)
    nm, mn, nrw = t.nm.astype(np.int64), t.mn.astype(np.int64), t.nrw.astype(np.int64)
    used = np.arange(7)[None, :] < nrw[:, None]            # [83][7]
    bit = np.where(used, nm - 1, 0)                        # bit of entry (i, j)
    chk = mn - 1                                           # [174][3]
    # kk with kMn[ibj][kk] - 1 == i, per entry (exactly one: the tables' contract)
    kk = np.array([[int(np.nonzero(chk[bit[i, j]] == i)[0][0]) if used[i, j] else 0 for j in range(7)] for i in range(M)])
    tov = np.zeros((N, 3), f32)
    plain = np.zeros(N, np.uint8)
    min_errors, it = M, 0
    with np.errstate(all="ignore"):
        while it < max_iters:
            zn = ((cw + tov[:, 0]) + tov[:, 1]) + tov[:, 2]
            plain = (zn > 0).astype(np.uint8)
            errors = ldpc_check(plain, t)
            if errors < min_errors:
                min_errors = errors
                if errors == 0:
                    break
            toc = fast_tanh(-(zn[bit] - tov[bit, kk]) / f32(2))   # [83][7]; unused entries are never read
            for j in range(3):
                tmn = np.ones(N, f32)
                for k in range(7):
                    take = (k < nrw[chk[:, j]]) & (nm[chk[:, j], k] - 1 != np.arange(N))
                    tmn = np.where(take, tmn * toc[chk[:, j], k], tmn).astype(f32)
                tov[:, j] = f32(2) * fast_atanh(-tmn)
            it += 1
    return plain, min_errors, it


def bp_decode_literal(codeword, max_iters=LDPC_ITERATIONS, t=None):
    """bp_decode() loop for loop (ft8.cpp:518-594), scalar f32: what the vectorised form above is held to"""
    t = t or tables()
    cw = np.asarray(codeword, f32)
    tov = np.zeros((N, 3), f32)
    toc = np.zeros((M, 7), f32)
    plain = np.zeros(N, np.uint8)
    min_errors, it = M, 0
    with np.errstate(all="ignore"):
        while it < max_iters:
            zn = np.zeros(N, f32)
            for i in range(N):
                zn[i] = f32(f32(f32(cw[i] + tov[i, 0]) + tov[i, 1]) + tov[i, 2])
                plain[i] = 1 if zn[i] > 0 else 0
            errors = ldpc_check(plain, t)
            if errors < min_errors:
                min_errors = errors
                if errors == 0:
                    break
            for i in range(M):
                for j in range(int(t.nrw[i])):
                    ibj = int(t.nm[i, j]) - 1
                    toc[i, j] = zn[ibj]
                    for k3 in range(3):
                        if int(t.mn[ibj, k3]) - 1 == i:
                            toc[i, j] = f32(toc[i, j] - tov[ibj, k3])
            for i in range(M):
                for j in range(int(t.nrw[i])):
                    toc[i, j] = fast_tanh(f32(-toc[i, j] / f32(2)))
            for i in range(N):
                for j in range(3):
                    ichk = int(t.mn[i, j]) - 1
                    tmn = f32(1.0)
                    for k in range(int(t.nrw[ichk])):
                        if int(t.nm[ichk, k]) - 1 != i:
                            tmn = f32(tmn * toc[ichk, k])
                    tov[i, j] = f32(f32(2) * fast_atanh(f32(-tmn)))
            it += 1
    return plain, min_errors, it


# ---- pack_bits, crc ----------------------------------------------------------------------------------------------------
def pack_bits(plain, num_bits):
    packed = np.zeros((num_bits + 7) // 8, np.uint8)
    for i in range(num_bits):
        if plain[i]:
            packed[i // 8] |= 0x80 >> (i % 8)
    return packed


def crc(message, num_bits):
    remainder, idx_byte = 0, 0
    for idx_bit in range(num_bits):
        if idx_bit % 8 == 0:
            remainder ^= int(message[idx_byte]) << (CRC_WIDTH - 8)
            idx_byte += 1
        if remainder & (1 << (CRC_WIDTH - 1)):
            remainder = ((remainder << 1) ^ CRC_POLYNOMIAL) & 0xFFFF
        else:
            remainder = (remainder << 1) & 0xFFFF
    return remainder & ((1 << CRC_WIDTH) - 1)


def crc_matches(a91):
    a = np.array(a91, np.uint8)
    chksum = ((int(a[9]) & 0x07) << 11) | (int(a[10]) << 3) | (int(a[11]) >> 5)
    a[9] &= 0xF8
    a[10] = 0
    a[11] = 0
    return chksum == crc(a, 96 - 14)


# ---- the loop of ft8_decode() up to the CRC check ----------------------------------------------------------------------
def decode(power, select=0, max_candidates=MAX_CANDIDATES, min_score=MIN_SCORE, ldpc_iterations=LDPC_ITERATIONS, t=None,
           stats=None):
    """one channel's slot -> (result record (RESULT scalar array of shape ()), log174 [20][174] f32, plain [20][174] uint8);
    the rows of unused candidates are zero"""
    t = t or tables()
    res = np.zeros((), RESULT)
    log_all, plain_all = np.zeros((MAX_CANDIDATES, N), f32), np.zeros((MAX_CANDIDATES, N), np.uint8)
    res["select"] = select
    if select < 0:
        return res, log_all, plain_all
    heap = find_sync(power, t.costas, max_candidates, min_score, stats)
    res["num_candidates"] = len(heap)
    valid = 0
    for idx, cand in enumerate(heap):
        c = res["cand"][idx]
        c["score"], c["time_offset"], c["freq_offset"], c["time_sub"], c["freq_sub"] = cand
        log174 = extract_likelihood(power, cand, t.gray)
        plain, n_errors, it = bp_decode(log174, ldpc_iterations, t)
        log_all[idx], plain_all[idx] = log174, plain
        c["n_errors"], c["iterations"] = n_errors, it
        flags = 0
        if n_errors == 0:
            a91 = pack_bits(plain, K)
            c["a91"] = a91
            flags = 1 | (2 if crc_matches(a91) else 0)
        c["flags"] = flags
        valid += flags == 3
    res["num_valid"] = valid
    return res, log_all, plain_all


def decode_all(waterfalls, select=None, **kw):
    """[n][SLOT_BYTES] (or a list) -> (RESULT [n], log174 [n][20][174], plain [n][20][174])"""
    n = len(waterfalls)
    out = [decode(waterfalls[c], 0 if select is None else int(select[c]), **kw) for c in range(n)]
    return np.array([o[0] for o in out], RESULT), np.array([o[1] for o in out]), np.array([o[2] for o in out])
