#!/usr/bin/env python3
"""Which kernels the process call launches, over a fixed list of small calls: the parity tests cannot see a wrong choice of
kernel form (every form computes the same values), so a change of the launch rules is checked by comparing the kernel
names two libraries launch for the same calls, in start order.

Every case is a fresh 3-channel chain and two calls on it, of 3 and of 5 frames (either side of the pipelined forms'
threshold of 4), each followed by a synchronisation.  The list covers every mode x AGC x sample format; input map x
parameter sets x audio rate; each stage tap and side output alone, FT8, the panadapter (its update frame falls into the
second call only); each chain-splitting stage alone, the CW filter at both rates; and FFT_LENGTH 1024 and 4096, the
latter with and without T41RX_SEG_RUN in the environment of t41rx_create().  Only the Python API of the package is used.

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/launch_census.py      (once per library)
  python tools/launch_census.py --list                       the case list, no device needed
  python tools/launch_census.py --compare DIR_A DIR_B         the two traces' kernel-name columns in start order
"""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NCH = 3
FRAMES = (3, 5)
MODES = {"usb": 0, "lsb": 1, "am": 2, "nfm": 3, "sam": 8}


def case_list():
    """[(name, dict)]: params = t41rx_params overrides; q15, map, sets, a24, seg_run = the call's switches; stage = the one
    tap, side output or stage the case switches on"""
    cases = []

    def add(name, **kw):
        cases.append((name, kw))

    for mode in MODES:
        for agc in (0, 1):
            for q15 in (0, 1):
                cuts = dict(FLoCut=-3000, FHiCut=-200) if mode == "lsb" else {}
                add("512/%s/agc%d/%s" % (mode, agc, "q15" if q15 else "f32"), params=dict(mode=MODES[mode], AGCMode=agc, **cuts), q15=q15)
    add("512/nfm_atan", params=dict(mode=MODES["nfm"], nfm_demod=1))
    add("512/usb/general_gains", params=dict(RFgain=3, IQAmpCorrectionFactor=1.01))
    for agc in (0, 1):
        for q15 in (0, 1):
            for m, s, r in [(m, s, r) for m in (0, 1) for s in (0, 1) for r in (0, 1)][1:]:
                add("512/usb/agc%d/%s/map%d_sets%d_%s" % (agc, "q15" if q15 else "f32", m, s, "24k" if r else "192k"),
                    params=dict(AGCMode=agc), q15=q15, map=m, sets=s, a24=r)
    for mode in ("am", "nfm", "sam"):
        for m in (0, 1):
            add("512/%s/map%d_24k" % (mode, m), params=dict(mode=MODES[mode]), map=m, a24=1)
    for r in (0, 1):
        rate = "24k" if r else "192k"
        for stage in ("tap_nco", "tap_dec", "tap_demod", "spect", "disp", "ft8", "pan", "eq", "nr", "notch", "nb", "cw_filter", "cw_det", "cw_dec"):
            add("512/usb/%s/%s" % (stage, rate), stage=stage, a24=r)
        add("512/usb/agc1/tap_demod/%s" % rate, params=dict(AGCMode=1), stage="tap_demod", a24=r)
        add("512/usb/ft8+nb/%s" % rate, stage="ft8+nb", a24=r)
        add("512/usb/ft8+tap_demod/%s" % rate, stage="ft8+tap_demod", a24=r)
        add("512/usb/sets/spect/%s" % rate, stage="spect", sets=1, a24=r)
        add("512/usb/map/nb/q15/%s" % rate, stage="nb", map=1, q15=1, a24=r)
    for n in (1024, 4096):
        for mode in ("usb", "am", "nfm"):
            for agc in (0, 1):
                for q15 in (0, 1):
                    add("%d/%s/agc%d/%s" % (n, mode, agc, "q15" if q15 else "f32"), params=dict(fft_length=n, mode=MODES[mode], AGCMode=agc), q15=q15)
        add("%d/usb/map" % n, params=dict(fft_length=n), map=1)
        add("%d/usb/general_gains" % n, params=dict(fft_length=n, RFgain=3, IQAmpCorrectionFactor=1.01))
    for q15 in (0, 1):
        add("4096/usb/seg_run/%s" % ("q15" if q15 else "f32"), params=dict(fft_length=4096), q15=q15, seg_run=2)
    add("4096/usb/seg_run/map", params=dict(fft_length=4096), map=1, seg_run=2)
    return cases


def run_case(T, name, c, keep):
    import numpy as np
    import torch
    stage = c.get("stage", "")
    params = dict(c.get("params", {}))
    if stage.startswith("cw_"):
        params["xmtMode"] = 1  # T41RX_CW_MODE
    if stage == "nr":
        params["nrOptionSelect"] = 1
    if stage == "notch":
        params["ANR_notchOn"] = 1
    if c.get("seg_run"):
        os.environ["T41RX_SEG_RUN"] = str(c["seg_run"])
    try:
        rx = T.RxChain(NCH, T.default_params(**params), NCOFreq=[-3000, 0, 12000])
    finally:
        os.environ.pop("T41RX_SEG_RUN", None)
    nmax = max(FRAMES)
    golden = os.path.join(ROOT, "tests", "golden")
    rows = NCH
    if c.get("map"):
        rx.set_input_map([0, 0, 1], 2)
        rows = 2
    if c.get("sets"):
        rx.set_param_sets([dict(FLoCut=300, FHiCut=2400)], [0, 1, 0])
    if c.get("a24"):
        rx.set_audio_rate(24000)
    N = rx.params.fft_length

    def zeros(*shape):
        t = torch.zeros(NCH, *shape, device="cuda")
        keep.append(t)
        return t

    for part in stage.split("+"):
        if part == "tap_nco":
            rx.set_debug_taps(post_nco=zeros(nmax * 2 * rx.frame_len))
        elif part == "tap_dec":
            rx.set_debug_taps(dec=zeros(nmax * N))
        elif part == "tap_demod":
            rx.set_debug_taps(demod=zeros(nmax * N // 2))
        elif part == "spect":
            rx.set_audio_spectrum(zeros(nmax, 1024), zeros(nmax, 3))
        elif part == "disp":
            rx.set_display_spectrum(zeros(nmax, 512), zeros(nmax, 512), 1)
        elif part == "ft8":
            rx.set_ft8_tables()
            rx.set_ft8(1, nmax)
        elif part == "pan":
            # frames 0 .. 2 are the first call, 3 .. 7 the second: one update frame, in the second
            rx.set_panadapter_tables(np.load(os.path.join(golden, "display", "gradient.npz"))["gradient"])
            rx.set_panadapter(True, update_period=8, update_phase=5, max_rows=1)
        elif part == "eq":
            rx.set_receive_eq_bands(np.load(os.path.join(golden, "eq", "rx_eq_bands.npz"))["coeffs_f32"])
            rx.set_receive_eq(1)
        elif part == "nb":
            rx.set_noise_blanker(1)
        elif part in ("cw_filter", "cw_det", "cw_dec"):
            z = np.load(os.path.join(golden, "cw", "cw_tables.npz"))
            rx.set_cw_tables(z["filters_f32"], z["fir_f32"])
            if part == "cw_filter":
                rx.set_cw_filter(2)
            else:
                rx.set_cw_detector(1, nmax)
            if part == "cw_dec":
                rx.set_cw_decode_tree(np.load(os.path.join(golden, "cw", "morse_tree.npz"))["tree"])
                rx.set_cw_decoder(1, nmax)
    rng = np.random.default_rng(7)
    for nfr in FRAMES:
        i = (0.1 * rng.standard_normal((rows, nfr * rx.frame_len))).astype(np.float32)
        q = (0.1 * rng.standard_normal((rows, nfr * rx.frame_len))).astype(np.float32)
        if c.get("q15"):
            # the q15 entry takes (Q, I): the firmware's I comes from the R queue
            a, b = (torch.from_numpy(np.round(v * 32768).astype(np.int16)).cuda() for v in (q, i))
            rx.ProcessIQData_q15(a, b)
        else:
            rx.ProcessIQData(torch.from_numpy(i).cuda(), torch.from_numpy(q).cuda())
        torch.cuda.synchronize()
    rx.close()


def kernel_names(trace_dir):
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if len(files) != 1:
        raise SystemExit("%s: expected one *kernel_trace.csv, found %d" % (trace_dir, len(files)))
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [r["Kernel_Name"] for r in rows]


def compare(dir_a, dir_b):
    a, b = kernel_names(dir_a), kernel_names(dir_b)
    cases = case_list()
    ours = lambda names: sum(1 for n in names if "t41" in n)  # noqa: E731  (the rest are torch's own: uploads' fills)
    print("%d cases x %d calls; A: %d kernel launches (%d of the library's, %d distinct names), B: %d (%d, %d)"
          % (len(cases), len(FRAMES), len(a), ours(a), len(set(a)), len(b), ours(b), len(set(b))))
    if a == b:
        print("the two kernel-name columns in start order are identical")
        return 0
    # hipMemcpy / hipMemset of pageable memory run as blit kernels of the runtime's own (__amd_rocclr_*): a library that
    # uploads a table at another moment moves those and no kernel of the path
    blit = lambda names: [n for n in names if not n.startswith("__amd_rocclr_")]  # noqa: E731
    print("the full columns differ (the runtime's blit kernels: %d in A, %d in B)" % (len(a) - len(blit(a)), len(b) - len(blit(b))))
    a, b = blit(a), blit(b)
    if a == b:
        print("without the runtime's blit kernels the two columns (%d launches) in start order are identical" % len(a))
        return 0
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    print("the columns differ from launch %d on:\n  A: %s\n  B: %s" % (k, a[k:k + 3], b[k:k + 3]))
    return 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    cases = case_list()
    if a.list:
        for name, c in cases:
            print(name, c)
        print("%d cases x %d calls" % (len(cases), len(FRAMES)))
        return
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("launch_census needs a HIP device")
    keep = []
    for name, c in cases:
        run_case(T, name, c, keep)
        del keep[:]
    print("launch census: %d cases x %d calls done" % (len(cases), len(FRAMES)))


if __name__ == "__main__":
    main()
