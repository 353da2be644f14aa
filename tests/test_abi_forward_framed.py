"""CPU-side checks of zmqg_forward_framed_multi's boundary (no GPU calls): the
header declares the call with its four parameters and the framing struct,
zmqg_forward_framing is 48 bytes in C with every member at the binding's
offset, the ZMQG_FRAMING_* / ZMQG_FWD_* values are the binding's, the built
library exports the call, the Python binding has it, the four "Not offered"
paragraphs point to it, and the ABI version is still 5."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zmqg_curve.h")
LIB = os.path.join(ROOT, "libzmq_amd", "libzmqg_curve.so")
NAME = "zmqg_forward_framed_multi"

# zmqg_forward_framing's members in order with their offsets (LP64)
FIELDS = [("size", 0), ("reserved", 4), ("recv", 8), ("send", 12), ("mode", 16), ("reserved2", 20), ("plan", 24),
          ("ws_results", 32), ("mask", 40)]
CONSTANTS = dict(ZMQG_FRAMING_ZMTP="FRAMING_ZMTP", ZMQG_FRAMING_WS="FRAMING_WS",
                 ZMQG_FRAMING_WS_MASKED="FRAMING_WS_MASKED", ZMQG_FWD_STATIC="FWD_STATIC", ZMQG_FWD_SUB="FWD_SUB",
                 ZMQG_FWD_ROUTER="FWD_ROUTER", ZMQG_FWD_LB="FWD_LB")


def _text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_call_and_its_struct():
    text = _text()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert m, "not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["zmqg_ctx *ctx", "const zmqg_forward_zmtp *args", "const zmqg_forward_framing *framing",
                    "void *stream"]
    assert re.search(r"typedef\s+struct\s+zmqg_forward_framing\s*\{[^}]*\}\s*zmqg_forward_framing\s*;", text)


def _compiles(src):
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_framing_layout_in_c_matches_the_binding():
    from libzmq_amd import curve
    py = [(n, getattr(curve.ForwardFraming, n).offset) for n, _ in curve.ForwardFraming._fields_]
    assert py == FIELDS and ctypes.sizeof(curve.ForwardFraming) == 48
    src = '#include <stddef.h>\n#include "zmqg_curve.h"\n'
    src += "typedef char total[sizeof(zmqg_forward_framing) == 48 ? 1 : -1];\n"
    for n, off in py:
        src += "typedef char off_%s[offsetof(zmqg_forward_framing, %s) == %d ? 1 : -1];\n" % (n, n, off)
    _compiles(src + "int main(void){return 0;}\n")


def test_constants_match_the_binding():
    from libzmq_amd import curve
    src = '#include "zmqg_curve.h"\n'
    for c_name, py_name in CONSTANTS.items():
        src += "typedef char is_%s[%s == %du ? 1 : -1];\n" % (c_name, c_name, getattr(curve, py_name))
    _compiles(src + "int main(void){return 0;}\n")
    assert [getattr(curve, CONSTANTS[k]) for k in CONSTANTS] == [0, 1, 2, 0, 1, 2, 3]


def test_library_exports_the_call():
    assert os.path.exists(LIB), "build first: make -C libzmq_amd/csrc"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    assert NAME in set(l.split()[-1] for l in out.splitlines() if l.strip())


def test_binding_has_the_call():
    from libzmq_amd import curve
    assert callable(curve.CurveContext.forward_framed_multi)
    assert len(curve._lib.zmqg_forward_framed_multi.argtypes) == 4


def test_the_four_forward_calls_point_to_it():
    """Each forward call's contract names the framed call where it spoke of
    WebSocket framing, and the table of replaced reference calls lists it."""
    raw = open(HEADER).read()
    blocks = re.findall(r"/\*.*?\*/", raw, flags=re.S)
    for call in ("zmqg_forward_zmtp_multi", "zmqg_forward_zmtp_sub_multi", "zmqg_forward_zmtp_router_multi",
                 "zmqg_forward_zmtp_lb_multi"):
        own = [b for b in blocks if b.startswith("/* %s:" % call)]
        assert len(own) == 1, call
        flat = " ".join(own[0].replace("*", " ").split())
        assert re.search(r"WebSocket framing[^.;]*zmqg_forward_framed_multi", flat), call
    top = " ".join(blocks[0].replace("*", " ").split())
    assert re.search(r"src/proxy\.cpp:90-138, src/ws_decoder\.cpp:39-249, src/ws_encoder\.cpp:26-126 "
                     r"zmqg_forward_framed_multi", top)


def test_abi_version_unchanged():
    """The call is an addition: the ABI version stays 5."""
    from libzmq_amd import curve
    assert curve._lib.zmqg_abi_version() == 5
    assert re.search(r"#define ZMQG_CURVE_ABI_VERSION 5\b", open(HEADER).read())
