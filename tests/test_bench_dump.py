"""bench.py --dump-outputs on CPU tensors: the last timed launch's audio, a fixed sample of channels, at most 64 MB, the
same channels in every run whatever the buffer layout."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (importing it touches no GPU)


class _Launch:
    """what dump_outputs reads of a bench.Workload, over one CPU output buffer"""

    def __init__(self, n, frames, frame_len, layout, q15=False):
        import torch
        self.torch, self.dev, self.n, self.frames, self.frame_len, self.layout = torch, "cpu", n, frames, frame_len, layout
        self.audio = (torch.arange(n, dtype=torch.float64)[:, None] * 4096
                      + torch.arange(frames * frame_len, dtype=torch.float64)[None, :] % 4096).float()  # channel c: c * 4096 + t % 4096
        x = self.audio if layout == "channel" else self.audio.view(n, frames, frame_len).transpose(0, 1).contiguous()
        self.outs = [x.to(torch.int16) if q15 else x]

    def channels_of(self, x, idx_t):
        return bench.Workload.channels_of(self, x, idx_t)


def test_dump_budget_is_under_64_MB():
    assert 0 < bench.DUMP_BYTES <= 64e6


@pytest.mark.parametrize("n,frames,frame_len,layout,q15,rows,cols", [
    (512, 16, 256, "channel", False, 3, 4096),    # bounded by bytes: whole launches of 3 channels
    (512, 16, 256, "time", False, 3, 4096),       # the same from a time-major buffer
    (512, 1, 256, "channel", False, 5, 256),      # bounded by the channel count
    (64, 4, 16384, "channel", False, 1, 12288),   # one channel's launch is over the budget: its last samples
    (4, 1, 2048, "channel", True, 4, 2048),       # q15 samples; fewer channels than the sample
])
def test_dump_is_a_fixed_bounded_sample_of_the_last_launch(tmp_path, monkeypatch, n, frames, frame_len, layout, q15, rows, cols):
    monkeypatch.setattr(bench, "DUMP_BYTES", 48 << 10)
    monkeypatch.setattr(bench, "DUMP_CHANNELS", 5)
    w = _Launch(n, frames, frame_len, layout, q15)
    bench.dump_outputs(w, 0, str(tmp_path / "a"))
    bench.dump_outputs(w, 0, str(tmp_path / "b"))
    a = np.load(tmp_path / "a" / "audio.npy")
    assert a.dtype == np.float32 and a.shape == (rows, cols)
    assert np.array_equal(a, np.load(tmp_path / "b" / "audio.npy"))
    ch = a[:, 0].astype(np.int64) // 4096  # the channel index, from the values
    assert (np.diff(ch) > 0).all()
    want = w.audio.numpy()[ch][:, frames * frame_len - cols:]
    assert np.array_equal(a, want.astype(np.int16).astype(np.float32) if q15 else want)


def test_bench_options():
    """--full and --dump-outputs are options of the benchmark; a plain run is the default"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout
