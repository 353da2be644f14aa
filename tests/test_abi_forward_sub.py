"""CPU-side checks of zmqg_forward_zmtp_sub_multi's boundary (no GPU calls): the
header declares the call and zmqg_forward_subs, the struct's size and member
offsets in C are the binding's, the built library exports the call, the Python
binding has it and builds the table, and the ABI version is still 5."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zmqg_curve.h")
LIB = os.path.join(ROOT, "libzmq_amd", "libzmqg_curve.so")
NAME = "zmqg_forward_zmtp_sub_multi"

FIELDS = ["size", "flags", "n_subs", "sub_idx", "sub_off", "sub_len", "sub_bytes", "sub_bytes_len", "match_out"]


def _text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_call_and_its_struct():
    text = _text()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert m, "not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["zmqg_ctx *ctx", "const zmqg_forward_zmtp *args", "const zmqg_forward_subs *subs", "void *stream"]
    assert re.search(r"typedef\s+struct\s+zmqg_forward_subs\s*\{[^}]*\}\s*zmqg_forward_subs\s*;", text)
    assert re.search(r"#define\s+ZMQG_SUBS_INVERT\s+1u\b", text)
    # the table of replaced reference calls names it
    assert re.search(r"xpub_t::xsend.*?%s" % NAME, open(HEADER).read(), flags=re.S)


def _compiles(src):
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_forward_subs_layout_in_c_matches_the_binding():
    from libzmq_amd import curve
    py = [(n, getattr(curve.ForwardSubs, n).offset) for n, _ in curve.ForwardSubs._fields_]
    assert [n for n, _ in py] == FIELDS
    assert ctypes.sizeof(curve.ForwardSubs) == 64 and [o for _, o in py] == [0, 4, 8, 16, 24, 32, 40, 48, 56]
    src = '#include <stddef.h>\n#include "zmqg_curve.h"\n'
    src += "typedef char total[sizeof(zmqg_forward_subs) == %d ? 1 : -1];\n" % ctypes.sizeof(curve.ForwardSubs)
    for n, off in py:
        src += "typedef char off_%s[offsetof(zmqg_forward_subs, %s) == %d ? 1 : -1];\n" % (n, n, off)
    src += "typedef char invert[ZMQG_SUBS_INVERT == %d ? 1 : -1];\n" % curve.SUBS_INVERT
    _compiles(src + "int main(void){return 0;}\n")


def test_library_exports_the_call():
    assert os.path.exists(LIB), "build first: make -C libzmq_amd/csrc"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    assert NAME in set(l.split()[-1] for l in out.splitlines() if l.strip())


def test_binding_has_the_call_and_builds_the_table():
    from libzmq_amd import curve
    for attr in ("forward_zmtp_sub_multi", "forward_subs_table", "forward_zmtp_multi"):
        assert callable(getattr(curve.CurveContext, attr))
    assert len(curve._lib.zmqg_forward_zmtp_sub_multi.argtypes) == 4
    idx, off, ln, raw = curve.CurveContext.forward_subs_table([[b"a", b""], [], [b"xyz"]])
    assert idx.tolist() == [0, 2, 2, 3] and off.tolist() == [0, 1, 1] and ln.tolist() == [1, 0, 3]
    assert raw.tobytes() == b"axyz"
    assert (idx.dtype, off.dtype, ln.dtype, raw.dtype) == ("uint32", "uint64", "uint32", "uint8")
    idx, off, ln, raw = curve.CurveContext.forward_subs_table([[], []])
    assert idx.tolist() == [0, 0, 0] and len(off) == len(ln) == len(raw) == 0
    assert (idx.dtype, off.dtype, ln.dtype, raw.dtype) == ("uint32", "uint64", "uint32", "uint8")


def test_abi_version_unchanged():
    """The call is an addition: the ABI version stays 5."""
    from libzmq_amd import curve
    assert curve._lib.zmqg_abi_version() == 5
    assert re.search(r"#define ZMQG_CURVE_ABI_VERSION 5\b", open(HEADER).read())
