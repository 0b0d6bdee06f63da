"""What the transmit tests share: the microphone recipe, one device call of the exciter, and the bit-for-bit comparison
of an (I, Q) pair of q15 outputs."""
import numpy as np

from rx_harness import to_q15

F = 2048


def mic(nch, nfr, seed=1, level=0.5):
    """speech-band multi-tone + noise at 192 kS/s as q15 (what the codec would deliver)"""
    rng = np.random.default_rng(seed)
    n = np.arange(nfr * F)
    x = np.zeros((nch, nfr * F))
    for c in range(nch):
        for _ in range(4):
            x[c] += rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * rng.uniform(300, 2800) / 192000.0 * n + rng.uniform(0, 6.28))
        x[c] += 0.01 * rng.standard_normal(n.size)
    x *= level / np.abs(x).max()
    return to_q15(x)


def cat(parts):
    return tuple(np.concatenate([p[i] for p in parts], axis=1) for i in (0, 1))


def assert_same(got, ref, what=""):
    for g, r, side in ((got[0], ref[0], "I"), (got[1], ref[1], "Q")):
        if not np.array_equal(g, r):
            d = g.astype(np.int32) - r.astype(np.int32)
            bad = np.argwhere(d)
            raise AssertionError("%s %s: %d of %d samples differ (max |d| %d), first at [channel, sample] %s"
                                 % (what, side, len(bad), d.size, np.abs(d).max(), bad[0].tolist()))


def dev(q):
    import torch
    return torch.from_numpy(np.ascontiguousarray(q)).cuda()


def run(tx, q):
    """one device call on the current stream; numpy (I, Q)"""
    import torch
    oL, oR = tx.ExciterIQData(dev(q))
    torch.cuda.synchronize()
    return oL.cpu().numpy(), oR.cpu().numpy()
