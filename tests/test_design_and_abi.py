"""Host logic of the product library without a GPU: every C-ABI symbol of include/t41rx.h is
exported, the host-side coefficient designer matches the oracle's, argument checking and error
codes behave, and creating a context without a HIP device fails loudly (no CPU fallback)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T(built):
    import t41_sdr_amd
    t41_sdr_amd.load()
    return t41_sdr_amd


def test_every_declared_symbol_is_exported(T):
    hdr = open(os.path.join(ROOT, "include", "t41rx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(t41rx_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 20
    lib = C.CDLL(T.LIB_PATH)
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, "declared in include/t41rx.h but not exported: %s" % missing
    from t41_sdr_amd import _lib
    assert declared == set(_lib.SYMBOLS), "python binding and header disagree"
    assert lib.t41rx_abi_version() == 5


def _declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(t41[rt]x_[a-z0-9_]+)\s*\(", hdr))


def test_nothing_but_the_declared_symbols_is_exported(T):
    """the converse: libt41rx.so is built with -fvisibility=hidden and an export list
    (t41_sdr_amd/csrc/exports.map); its dynamic symbol table is the two headers' entry points and nothing else --
    no t41:: C++ symbol, no kernel stub, no host helper, no diagnostic hook"""
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", T.LIB_PATH], text=True)
    exported = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    declared = _declared("t41rx.h") | _declared("t41tx.h")
    assert exported == declared, "exported but not declared: %s; declared but not exported: %s" % (
        sorted(exported - declared), sorted(declared - exported))
    # and the export list itself names exactly those (plus the diagnostic builds' t41rx_debug_* pattern)
    m = open(os.path.join(ROOT, "t41_sdr_amd", "csrc", "exports.map")).read()
    m = re.sub(r"#.*", "", m)
    listed = set(re.findall(r"\b(t41[rt]x_[a-z0-9_]+);", m))
    assert listed == declared
    # every declaration carries the export attribute (a declaration without it would be hidden by -fvisibility=hidden)
    for header in ("t41rx.h", "t41tx.h"):
        hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for name in _declared(header):
            assert re.search(r"T41RX_API[^;]*\b%s\s*\(" % name, hdr), "%s lacks T41RX_API in %s" % (name, header)


def test_params_struct_layout_matches_header(T):
    hdr = open(os.path.join(ROOT, "include", "t41rx.h")).read()
    body = re.search(r"typedef struct t41rx_params \{(.*?)\} t41rx_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|float)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in T.Params._fields_]
    assert C.sizeof(T.Params) == 4 * len(fields)


@pytest.mark.parametrize("kw", [
    dict(mode=0, FLoCut=200, FHiCut=3000),
    dict(mode=1, FLoCut=-3000, FHiCut=-200),
    dict(mode=2, FLoCut=-3000, FHiCut=3000),
    dict(mode=3, FLoCut=200, FHiCut=3000, nfmFilterBW=12000),
    dict(mode=0, FLoCut=400, FHiCut=600, rfGainAllBands=6, RFgain=3, audioVolume=55),
    dict(mode=0, FLoCut=100, FHiCut=11000),  # > 10 kHz: resampler design caps at 10 kHz (Filter.cpp:408)
    dict(mode=0, FLoCut=400, FHiCut=600, fft_length=4096),
    dict(mode=0, FLoCut=200, FHiCut=3000, fft_length=1024),
    dict(mode=0, FLoCut=200, FHiCut=3000, AGCMode=1),
    dict(mode=2, FLoCut=-3000, FHiCut=3000, AGCMode=2, AGC_thresh=30),
    dict(mode=3, FLoCut=200, FHiCut=3000, AGCMode=3),
    dict(mode=1, FLoCut=-3000, FHiCut=-200, AGCMode=4, AGC_thresh=10),
])
def test_designer_matches_oracle(T, kw):
    p = T.default_params(**kw)
    N = p.fft_length
    got = T.blob_fields(T.design_coeffs(p), N)
    ref = O.coeff_arrays(O.design(O.default_params(**kw)), N)
    for k in ("dec1", "dec2", "int1", "int2", "biquad_lowpass1", "agc"):
        assert np.array_equal(got[k], ref[k]), k  # same f32 arithmetic -> bit-exact
    # the mask goes through a different f32 FFT decomposition: rounding-level agreement
    assert np.abs(got["mask"] - ref["mask"]).max() < 4e-7 * np.abs(ref["mask"]).max()


def test_scalars_follow_process_cpp(T):
    p = T.default_params(mode=1, FLoCut=-2800, FHiCut=-300, rfGainAllBands=4, RFgain=7, audioVolume=40,
                         IQAmpCorrectionFactor=1.05, IQPhaseCorrectionFactor=0.02, xmtMode=1, CWFreqShift=600)
    s = T.blob_fields(T.design_coeffs(p), 512)["scalars"]
    assert s[0] == np.float32(10.0 ** float(np.float32(4) / np.float32(20)))       # Process.cpp:117
    assert s[1] == 7.0 and s[2] == np.float32(-1.05) and s[3] == np.float32(0.02)  # :133, :166
    fk = float(np.float32(2800.0 * 0.001))  # float * double -> double -> float; LSB uses -FLoCut, :485
    assert s[4] == np.float32(7.0874 * fk ** -1.232)
    assert s[5] == 20.0                                                             # DSP_Fn.cpp:453
    x = np.float32(0.4)
    assert s[6] == np.float32(8.0) * (np.float32(5) * x * x * x * x * x)            # :929, :964
    assert s[7] == 1.0 and s[8] == 600.0                                            # LSB + CW: +CWFreqShift


def test_design_rejects_bad_arguments(T):
    from t41_sdr_amd import _lib
    lib = T.load()
    p = T.default_params()
    n = lib.t41rx_coeff_blob_bytes(512)
    assert n == 4 * (32 + 28 + 46 + 48 + 32 + 5 + 16 + 16 + 1024)  # 32-word header: 8 + t41rx_params padded to 24; 16 scalar slots
    assert lib.t41rx_coeff_blob_bytes(500) == 0
    buf = (C.c_uint8 * n)()
    assert lib.t41rx_design_coeffs(C.byref(p), buf, n - 1) == _lib.ERR_ARG
    assert lib.t41rx_design_coeffs(None, buf, n) == _lib.ERR_ARG
    for bad in (dict(fft_length=300), dict(mode=9), dict(FLoCut=3000, FHiCut=200), dict(audioVolume=101),
                dict(mode=1, FLoCut=200, FHiCut=3000), dict(FHiCut=20000), dict(AGCMode=5), dict(AGCMode=-1)):
        with pytest.raises(T.T41RxError) as e:
            T.design_coeffs(T.default_params(**bad))
        assert e.value.status == _lib.ERR_ARG
    assert b"argument" in lib.t41rx_strerror(_lib.ERR_ARG)


def test_no_cpu_fallback_without_a_device(T):
    """On a box without a HIP device creating a context must fail with ERR_HIP, never silently
    run somewhere else."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from t41_sdr_amd import _lib
    with pytest.raises(T.T41RxError) as e:
        T.RxChain(4)
    assert e.value.status == _lib.ERR_HIP


def test_product_never_touches_the_oracle():
    """the shipped package must not import, link or open anything under oracle/"""
    pkg = os.path.join(ROOT, "t41_sdr_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".h")) or f == "Makefile":
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle_lib" not in txt and "t41_oracle" not in txt and "libt41oracle" not in txt, f
    import subprocess
    so = os.path.join(pkg, "libt41rx.so")
    if os.path.exists(so):
        assert "t41oracle" not in subprocess.run(["ldd", so], capture_output=True, text=True).stdout


def test_diagnostic_builds_are_fenced(T, tmp_path):
    """the diagnostic switches (T41RX_STAMP, _CLK, _PIPE_STAT: stamps / counters next to the product's
    values) sit behind ONE guard (t41_sdr_amd/csrc/rx_experiments.hpp): without -DT41RX_EXPERIMENT=1 they do not compile,
    and a library built with them refuses t41rx_create() unless the environment opts in.  Checked here with the dispatch
    translation unit (no kernels: seconds) linked against the product's objects, and the other way round: every kernel
    object answers for itself (T41RX_BUILD_FLAGS), so a diagnostic display_kernel.o (the cheapest unit that includes
    rx_device.hpp) among the product's objects, the product's rx_dispatch.o included, is fenced the same way."""
    import subprocess
    csrc = os.path.join(ROOT, "t41_sdr_amd", "csrc")
    base = ["hipcc", "-O1", "-std=c++17", "-fPIC", "-fvisibility=hidden", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include")]
    for unit in ("rx_dispatch.hip", "cal_kernel.hip"):
        for flag in ("-DT41RX_STAMP", "-DT41RX_CLK", "-DT41RX_PIPE_STAT"):
            r = subprocess.run(base + [flag, "-fsyntax-only", unit], cwd=csrc, capture_output=True, text=True)
            assert r.returncode != 0 and "T41RX_EXPERIMENT=1" in r.stderr, (unit, flag, r.stderr[-400:])
    # the product's objects, as the Makefile lists them (the one list)
    listed = [subprocess.check_output(["make", "-s", target], cwd=csrc, text=True).split() for target in ("print-rxk-objs", "print-host-objs")]
    assert "rx_dispatch.o" in listed[0] and "display_kernel.o" in listed[0] and "rx_host.o" in listed[1]
    # one unit built with a switch, every other object the product's
    for unit in ("rx_dispatch", "display_kernel"):
        obj = str(tmp_path / (unit + "_exp.o"))
        subprocess.check_call(base + ["-DT41RX_EXPERIMENT=1", "-DT41RX_CLK", "-c", unit + ".hip", "-o", obj], cwd=csrc)
        objs = [os.path.join(csrc, o) for o in listed[0] + listed[1] if o != unit + ".o"]
        lib_path = str(tmp_path / ("libt41rx_%s_exp.so" % unit))
        subprocess.check_call(["hipcc", "-shared", "-fPIC", "--offload-arch=gfx950", obj] + objs + ["-o", lib_path])
        code = ("import ctypes as C, sys; lib = C.CDLL(%r); lib.t41rx_last_error.restype = C.c_char_p; ctx = C.c_void_p(); "
                "p = (C.c_int32 * 32)(); lib.t41rx_default_params(p); rc = lib.t41rx_create(C.byref(ctx), 0, 4, p); "
                "print(rc, lib.t41rx_last_error().decode())" % lib_path)
        env = {k: v for k, v in os.environ.items() if k != "T41RX_ALLOW_EXPERIMENT"}
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (unit, r.stderr[-500:])
        rc, msg = r.stdout.strip().split(" ", 1)
        assert int(rc) == -2 and "diagnostics" in msg and "T41RX_ALLOW_EXPERIMENT" in msg, (unit, rc, msg)   # T41RX_ERR_UNSUPPORTED
        env["T41RX_ALLOW_EXPERIMENT"] = "1"
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert "EXPERIMENT BUILD" in r.stderr and "diagnostics on" in r.stderr, unit
        assert "kernel diagnostics" not in r.stdout, unit   # past the fence (and, without a GPU, on to T41RX_ERR_HIP)
    # the product library is not one
    assert T.load().t41rx_abi_version() == 5


def _rxk_objs(csrc):
    import subprocess
    return subprocess.check_output(["make", "-s", "print-rxk-objs"], cwd=csrc, text=True).split()


def test_every_kernel_object_reports_its_build_flags(built):
    """The fence asks every object of the Makefile's RXK_OBJS (the one list of what an experiment build recompiles): each
    defines its own t41::build_flags_<object>() (rx_experiments.hpp: T41RX_BUILD_FLAGS), and rx_dispatch.o, whose
    kernel_build_flags() is their OR, references each of them.  An object that joins the list without one fails here."""
    import subprocess
    csrc = os.path.join(ROOT, "t41_sdr_amd", "csrc")
    names = [o[:-2] for o in _rxk_objs(csrc)]
    assert len(names) >= 9 and "rx_dispatch" in names and "cal_kernel" in names
    symbols = lambda o: subprocess.check_output(["nm", "-C", os.path.join(csrc, o + ".o")], text=True).splitlines()  # noqa: E731
    dispatch = symbols("rx_dispatch")
    assert any(re.search(r"\bT t41::kernel_build_flags\(\)$", s) for s in dispatch)
    for name in names:
        if name == "rx_dispatch":
            continue
        fn = re.escape("t41::build_flags_%s()" % name)
        assert any(re.search(r"\bT %s$" % fn, s) for s in symbols(name)), "%s.o does not define %s" % (name, fn)
        assert any(re.search(r"\bU %s$" % fn, s) for s in dispatch), "rx_dispatch.o does not ask %s" % fn


def _to_rebuild(csrc, *make_args):
    """the objects `make -n` would compile"""
    import subprocess
    out = subprocess.check_output(["make", "-n"] + list(make_args), cwd=csrc, text=True)
    return sorted(m.group(1) for m in re.finditer(r"^\S.* -c \S+ -o (\S+\.o)$", out, re.M))


def test_objects_depend_on_their_flags_and_their_own_headers(built, tmp_path):
    """The Makefile on the tree just built: with the same flags nothing is to do; with other KFLAGS exactly RXK_OBJS are
    rebuilt (objects depend on their class's compile line); and header dependencies are the compiler's own, so a change
    to a stage's header (here cw_kernels.hpp, in a copy of csrc) rebuilds that stage's kernel and the receive host, and
    none of the fused rx512 kernels."""
    import shutil
    import subprocess
    csrc = os.path.join(ROOT, "t41_sdr_amd", "csrc")
    rxk = sorted(_rxk_objs(csrc))
    assert subprocess.run(["make", "-q"], cwd=csrc).returncode == 0 and _to_rebuild(csrc) == []
    assert _to_rebuild(csrc, "KFLAGS=-DT41RX_EXPERIMENT=1") == rxk
    # a copy at the same depth (the rules name ../../include and ../libt41rx.so), with the times of the original
    for d in ("include", "examples"):
        shutil.copytree(os.path.join(ROOT, d), str(tmp_path / d), copy_function=shutil.copy2)
    copy = str(tmp_path / "t41_sdr_amd" / "csrc")
    shutil.copytree(csrc, copy, copy_function=shutil.copy2)
    shutil.copy2(os.path.join(ROOT, "t41_sdr_amd", "libt41rx.so"), str(tmp_path / "t41_sdr_amd"))
    assert _to_rebuild(copy) == []
    os.utime(os.path.join(copy, "cw_kernels.hpp"))
    again = _to_rebuild(copy)
    host = subprocess.check_output(["make", "-s", "print-host-objs"], cwd=csrc, text=True).split()
    assert "cw_kernel.o" in again and {o for o in host if o.startswith("rx_")} <= set(again), again
    assert not [o for o in again if o.startswith("rx512_")] and not set(again) & set(rxk), again


def test_the_environment_is_read_in_one_place():
    """getenv occurs in rx_host.cpp only, and names the fence's opt-in, the tests' hook and the two variables of the
    diagnostic builds (which t41rx_create() reads on a diagnostic library only): no kernel file, no dispatch and no stage
    host consults the environment."""
    csrc = os.path.join(ROOT, "t41_sdr_amd", "csrc")
    found = {}
    for name in sorted(os.listdir(csrc)):
        if os.path.splitext(name)[1] in (".hpp", ".hip", ".cpp", ".h", ".inc"):
            names = re.findall(r"getenv\s*\(\s*\"?(\w*)", open(os.path.join(csrc, name)).read())
            if names:
                found[name] = sorted(names)
    assert found == {"rx_host.cpp": ["T41RX_ALLOW_EXPERIMENT", "T41RX_PIPE_STAT", "T41RX_SEG_RUN", "T41RX_STAMP_TAPS"]}, found


def test_kernel_sources_carry_no_build_switches():
    """The kernel sources build one form: the only T41RX_* macros a preprocessor conditional may test are the diagnostic
    builds' (rx_experiments.hpp).  The A/B switches of rounds 1-5 were folded into the product form; their measurements
    are in DESIGN.md and profiles/."""
    allowed = {"T41RX_EXPERIMENT", "T41RX_STAMP", "T41RX_PIPE_STAT", "T41RX_CLK", "T41RX_DIAGNOSTICS"}
    csrc = os.path.join(ROOT, "t41_sdr_amd", "csrc")
    found = []
    for name in sorted(os.listdir(csrc)):
        if os.path.splitext(name)[1] not in (".hpp", ".hip", ".cpp", ".h"):
            continue
        with open(os.path.join(csrc, name)) as f:
            for no, line in enumerate(f, 1):
                if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                    for macro in re.findall(r"\bT41RX_\w+", line.split("//")[0]):
                        if macro not in allowed:
                            found.append("%s:%d: %s" % (name, no, line.strip()))
    assert not found, found


def test_no_source_includes_a_kernel_file():
    """Every .hip file is a translation unit of its own with a Makefile rule of its own: no .cpp, .hpp or .hip file under
    t41_sdr_amd/csrc #includes one (a host file that did would be compiled as device code, and a setter would rebuild
    the kernels).  Kernel text shared between kernels is an .inc file; those may be included."""
    csrc = os.path.join(ROOT, "t41_sdr_amd", "csrc")
    found, seen = [], 0
    for name in sorted(os.listdir(csrc)):
        if os.path.splitext(name)[1] not in (".hpp", ".hip", ".cpp"):
            continue
        seen += 1
        with open(os.path.join(csrc, name)) as f:
            for no, line in enumerate(f, 1):
                if re.match(r"\s*#\s*include\s*[\"<][^\">]*\.hip[\">]", line):
                    found.append("%s:%d: %s" % (name, no, line.strip()))
    assert seen and not found, found
    # and the Makefile builds each of them into an object of that name, which the library links
    listed = set(re.findall(r"\b(\w+)\.o\b", open(os.path.join(csrc, "Makefile")).read()))
    hips = {os.path.splitext(n)[0] for n in os.listdir(csrc) if n.endswith(".hip")}
    assert hips and hips <= listed, sorted(hips - listed)


def _prototypes(header):
    """{name: (return type, [parameter types])} of every T41RX_API declaration of a header, names and comments dropped"""
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    out = {}
    for ret, name, params in re.findall(r"\bT41RX_API\s+([\w \*]+?)\s*\b(t41[rt]x_\w+)\s*\(([^;{]*)\)\s*;", hdr):
        params = [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]
        if params in (["void"], [""]):
            params = []
        out[name] = (re.sub(r"\s+", " ", ret).strip(), [re.match(r"(.*?)\w+$", p).group(1).strip() for p in params])
    return out


@pytest.mark.parametrize("header,table", [("t41rx.h", "SYMBOLS"), ("t41tx.h", "TX_SYMBOLS")])
def test_binding_tables_match_the_headers(T, header, table):
    """Every entry point of both headers is in its ctypes table (_lib.SYMBOLS receive, _lib.TX_SYMBOLS transmit) and
    nothing else is, with the header's return type, its number of parameters, every scalar parameter's exact type and a
    pointer type for every pointer; load() binds both tables to the one handle.  A wrong arity would not fail a call:
    it would corrupt it."""
    from t41_sdr_amd import _lib, tx
    protos, mirror = _prototypes(header), getattr(_lib, table)
    assert len(protos) >= 20 and set(protos) == _declared(header)  # the parser saw every declaration
    assert set(mirror) == set(protos), sorted(set(mirror) ^ set(protos))
    results = {"int": C.c_int, "size_t": C.c_size_t, "const char *": C.c_char_p, "void": None}
    scalars = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float}
    lib = T.load()
    for name, (ret, params) in protos.items():
        res, args = mirror[name]
        assert res is results[ret], (name, ret, res)
        assert len(args) == len(params), (name, params, args)
        for want, got in zip(params, args):
            if "*" in want:
                assert got is C.c_void_p or issubclass(got, C._Pointer), (name, want, got)
            else:
                assert got is scalars[want], (name, want, got)
        fn = getattr(lib, name)  # bound by load(), whichever chain is used first
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert tx._load() is lib and tx.TX_SYMBOLS is _lib.TX_SYMBOLS and tx.TxParams is _lib.TxParams is T.TxParams
    assert not set(_lib.SYMBOLS) & set(_lib.TX_SYMBOLS)
