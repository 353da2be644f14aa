"""CPU-side checks of zmqg_forward_zmtp_router_multi's boundary (no GPU calls):
the header declares the call and zmqg_forward_router, the struct's size (80)
and member offsets in C are the binding's, the flags and the four
ZMQG_ROUTE_* values agree, the built library exports the call, the Python
binding has it and builds the table and the pair bases, the ABI version is
still 5 and zmqg_forward_zmtp keeps its size."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zmqg_curve.h")
LIB = os.path.join(ROOT, "libzmq_amd", "libzmqg_curve.so")
NAME = "zmqg_forward_zmtp_router_multi"

FIELDS = ["size", "flags", "src_id_off", "src_id_len", "n_ids", "id_off", "id_len", "id_dst", "id_bytes",
          "id_bytes_len", "dest_out"]


def _text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_call_and_its_struct():
    text = _text()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert m, "not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["zmqg_ctx *ctx", "const zmqg_forward_zmtp *args", "const zmqg_forward_router *router",
                    "void *stream"]
    assert re.search(r"typedef\s+struct\s+zmqg_forward_router\s*\{[^}]*\}\s*zmqg_forward_router\s*;", text)
    # the table of replaced reference calls names it, and the two sibling calls point to it
    raw = open(HEADER).read()
    assert re.search(r"router_t::xrecv / xsend, lookup_out_pipe.*?%s" % NAME, raw, flags=re.S)
    assert len(re.findall(NAME, raw)) >= 5


def _compiles(src):
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_forward_router_layout_in_c_matches_the_binding():
    from libzmq_amd import curve
    py = [(n, getattr(curve.ForwardRouter, n).offset) for n, _ in curve.ForwardRouter._fields_]
    assert [n for n, _ in py] == FIELDS
    assert ctypes.sizeof(curve.ForwardRouter) == 80 and [o for _, o in py] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64, 72]
    src = '#include <stddef.h>\n#include "zmqg_curve.h"\n'
    src += "typedef char total[sizeof(zmqg_forward_router) == 80 ? 1 : -1];\n"
    for n, off in py:
        src += "typedef char off_%s[offsetof(zmqg_forward_router, %s) == %d ? 1 : -1];\n" % (n, n, off)
    for c_name, value in (("ZMQG_ROUTER_PREPEND", 1), ("ZMQG_ROUTER_ROUTE", 2), ("ZMQG_ROUTE_NONE", 0xffffffff),
                          ("ZMQG_ROUTE_ADDRESS", 0xfffffffe), ("ZMQG_ROUTE_UNKNOWN", 0xfffffffd),
                          ("ZMQG_ROUTE_MALFORMED", 0xfffffffc)):
        src += "typedef char v_%s[%s == %uu ? 1 : -1];\n" % (c_name, c_name, value)
    # the parent call's struct is unchanged
    src += "typedef char parent[sizeof(zmqg_forward_zmtp) == 232 ? 1 : -1];\n"
    _compiles(src + "int main(void){return 0;}\n")
    assert ctypes.sizeof(curve.ForwardZmtp) == 232
    assert (curve.ROUTER_PREPEND, curve.ROUTER_ROUTE) == (1, 2)
    assert (curve.ROUTE_NONE, curve.ROUTE_ADDRESS, curve.ROUTE_UNKNOWN, curve.ROUTE_MALFORMED) == (
        0xffffffff, 0xfffffffe, 0xfffffffd, 0xfffffffc)


def test_library_exports_the_call():
    assert os.path.exists(LIB), "build first: make -C libzmq_amd/csrc"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    assert NAME in set(l.split()[-1] for l in out.splitlines() if l.strip())


def test_binding_has_the_call_the_table_and_the_pair_bases():
    from libzmq_amd import curve
    K = curve.CurveContext
    for attr in ("forward_zmtp_router_multi", "forward_router_table", "forward_router_pair_base"):
        assert callable(getattr(K, attr))
    assert len(curve._lib.zmqg_forward_zmtp_router_multi.argtypes) == 4
    # sorted as blob_t orders: a prefix first, bytes unsigned, the empty id in front
    off, ln, dst, raw = K.forward_router_table([(b"b", 0), (b"ab", 1), (b"a", 2), (b"\x80", 3), (b"", 4), (b"a\x00", 5)])
    ids = [raw.tobytes()[int(o):int(o) + int(n)] for o, n in zip(off, ln)]
    assert ids == [b"", b"a", b"a\x00", b"ab", b"b", b"\x80"] and dst.tolist() == [4, 2, 5, 1, 0, 3]
    assert (off.dtype, ln.dtype, dst.dtype, raw.dtype) == ("uint64", "uint32", "uint32", "uint8")
    off, ln, dst, raw = K.forward_router_table([])
    assert len(off) == len(ln) == len(dst) == len(raw) == 0
    assert (off.dtype, ln.dtype, dst.dtype, raw.dtype) == ("uint64", "uint32", "uint32", "uint8")
    # the pair space: m = 2 with PREPEND alone, d' = 1 with ROUTE
    ri, ci = [0, 2, 2, 5], [0, 1, 1, 3]
    assert K.forward_router_pair_base(0, ri, ci, 4) == K.forward_pair_base(ri, ci, 4) == [0, 10, 10, 28]
    assert K.forward_router_pair_base(curve.ROUTER_PREPEND, ri, ci, 4) == [0, 20, 20, 56]
    assert K.forward_router_pair_base(curve.ROUTER_ROUTE, None, ci, 4) == [0, 5, 9, 15]
    assert K.forward_router_pair_base(curve.ROUTER_ROUTE | curve.ROUTER_PREPEND, ri, None, 4) == [0, 4, 8, 12]


def test_abi_version_unchanged():
    """The call is an addition: the ABI version stays 5."""
    from libzmq_amd import curve
    assert curve._lib.zmqg_abi_version() == 5
    assert re.search(r"#define ZMQG_CURVE_ABI_VERSION 5\b", open(HEADER).read())
