"""The panadapter map's entry points (t41rx_set_panadapter_map / t41rx_get_panadapter_map / t41rx_panadapter_rows) without
a GPU: the three prototypes are in the header, in exports.map and in _lib.SYMBOLS with matching types; RxChain has the
three members; the header no longer says that the panadapter and the beacon monitor are per context; the README and
DESIGN.md carry the new sections.  What the map makes a call compute is test_panadapter_map.py and test_beacon_map.py."""
import ctypes as C
import os
import re

from rx_harness import ROOT, assert_entry_points

NEW = ("t41rx_set_panadapter_map", "t41rx_get_panadapter_map", "t41rx_panadapter_rows")
CTYPES = {"t41rx_ctx *": C.c_void_p, "const t41rx_ctx *": C.c_void_p, "const int32_t *": C.POINTER(C.c_int32), "int32_t *": C.POINTER(C.c_int32),
          "int": C.c_int, "int *": C.POINTER(C.c_int)}


def test_entry_points_declared_exported_and_bound(built):
    import t41_sdr_amd._lib as lib
    hdr = assert_entry_points(NEW, ("set_panadapter_map", "panadapter_map", "panadapter_rows"), abi_version=5, pattern=r"T41RX_API\s+int\s+%s\s*\(")
    assert lib.load().t41rx_abi_version() == 5
    # the prototypes' types are the bound ones, argument by argument
    for name in NEW:
        args = re.search(r"T41RX_API\s+int\s+%s\s*\(([^)]*)\)" % name, hdr).group(1)
        # an argument's type: its text without the name, blanks squeezed, one blank in front of the star
        kinds = [re.sub(r"\s*\*\s*", " *", " ".join(re.sub(r"\w+\s*$", "", a).split())) for a in args.split(",")]
        restype, argtypes = lib.SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == len(kinds), (name, kinds)
        for k, bound in zip(kinds, argtypes):
            assert CTYPES[k] is bound or CTYPES[k] == bound, (name, k, bound)
    # the same return conventions as the FT8 map's three calls
    for new, old in zip(NEW, ("t41rx_set_ft8_map", "t41rx_get_ft8_map", "t41rx_ft8_rows")):
        assert lib.SYMBOLS[new][0] is lib.SYMBOLS[old][0] and [str(a) for a in lib.SYMBOLS[new][1]] == [str(a) for a in lib.SYMBOLS[old][1]]
    # the FT8 map's rules, to the letter, in the new block
    doc = hdr[hdr.index("receiver groups: the panadapter map"):hdr.index("T41RX_API int t41rx_set_panadapter_map")]
    for words in ("n == n_channels entries, each -1 or a row in [0, n_rows)", "removes the map", "Everything is checked on the host before anything changes",
                  "n_rows outside 1..n_channels", "an entry outside [-1, n_rows)", "a row named twice", "t41rx_panadapter_rows()",
                  "beacon off,", "in no checkpoint", "T41RX_ERR_UNSUPPORTED at a long fft_length", "Synchronises the device, then uploads",
                  "RFgain and rfGainAllBands from its own effective"):
        assert words in " ".join(doc.replace(" * ", " ").split()), words


def test_the_header_no_longer_says_per_context():
    hdr = " ".join(open(os.path.join(ROOT, "include", "t41rx.h")).read().replace(" * ", " ").split())
    assert "Still per context: the panadapter" not in hdr
    assert "the panadapter, the beacon monitor, the side outputs and the stage taps stay context-wide" not in hdr
    assert "The panadapter, the beacon monitor and the side outputs stay context-wide" not in hdr
    assert hdr.count("t41rx_set_panadapter_map") >= 6  # the block, the prototype and the three corrected sentences


def test_the_documents_carry_the_new_sections():
    readme = open(os.path.join(ROOT, "README.md")).read()
    status = readme[readme.index("## Status"):]
    first = status[status.index("\n* "):]
    assert first.startswith("\n* Receiver groups with a panadapter map"), first[:80]  # the entry at the top of the list
    for words in ("t41rx_set_panadapter_map", "RxChain.set_panadapter_map", "panadapter_list_kernel", "beacon_list_kernel", "rx_panmap.hpp",
                  "profiles/pan_map_isa_fingerprint.txt", "profiles/pan_map_kernel_resources.txt", "tools/pan_map_probe.py"):
        assert words in first[:first.index("\n* ", 3)], words
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "\n### Panadapter map (`t41rx_set_panadapter_map`" in design
    section = design[design.index("\n### Panadapter map ("):design.index("\n## 5. Multi-GPU")]
    for words in ("**The rule.**", "**The list.**", "**Kernels.**", "**dBm per channel.**", "tap_map", "panadapter_kernel.inc", "beacon_kernel.inc"):
        assert words in section, words
    six = design[design.index("\n## 6. Out of scope"):design.index("\n## 7. ")]
    assert '"Panadapter map"' in six
    assert "rx_panmap.hpp" in design[design.index("## 3b."):design.index("## 4. Kernels")]
