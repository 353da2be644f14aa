"""CPU-side checks of zmqg_forward_zmtp_lb_multi's boundary (no GPU calls): the
header declares the call and zmqg_forward_lb, the struct's size (80) and member
offsets in C are the binding's, the flag and the three ZMQG_LB_* values agree,
the built library exports the call, the Python binding has it and builds the
pair bases, the ABI version is still 5 and zmqg_forward_zmtp keeps its size."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zmqg_curve.h")
LIB = os.path.join(ROOT, "libzmq_amd", "libzmqg_curve.so")
NAME = "zmqg_forward_zmtp_lb_multi"

FIELDS = ["size", "flags", "src_id_off", "src_id_len", "n_groups", "stream_group", "grp_idx", "n_lb", "lb_dst",
          "lb_cur", "dest_out"]


def _text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_call_and_its_struct():
    text = _text()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert m, "not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["zmqg_ctx *ctx", "const zmqg_forward_zmtp *args", "const zmqg_forward_lb *lb", "void *stream"]
    assert re.search(r"typedef\s+struct\s+zmqg_forward_lb\s*\{[^}]*\}\s*zmqg_forward_lb\s*;", text)
    # the table of replaced reference calls names it with lb_t's lines, and the three sibling calls point to it
    raw = open(HEADER).read()
    assert re.search(r"lb_t::sendpipe.*?src/lb\.cpp:56-131.*?src/dealer\.cpp:110-113.*?src/push\.cpp:45-48.*?%s"
                     % NAME, raw, flags=re.S)
    assert len(re.findall(NAME, raw)) >= 6
    # the contract states the launch count and the order
    assert re.search(r"zmqg_forward_zmtp_multi's and two more", raw) and re.search(r"stream-major order", raw)


def _compiles(src):
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_forward_lb_layout_in_c_matches_the_binding():
    from libzmq_amd import curve
    py = [(n, getattr(curve.ForwardLb, n).offset) for n, _ in curve.ForwardLb._fields_]
    assert [n for n, _ in py] == FIELDS
    assert ctypes.sizeof(curve.ForwardLb) == 80 and [o for _, o in py] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64, 72]
    src = '#include <stddef.h>\n#include "zmqg_curve.h"\n'
    src += "typedef char total[sizeof(zmqg_forward_lb) == 80 ? 1 : -1];\n"
    for n, off in py:
        src += "typedef char off_%s[offsetof(zmqg_forward_lb, %s) == %d ? 1 : -1];\n" % (n, n, off)
    for c_name, value in (("ZMQG_LB_PREPEND", 1), ("ZMQG_LB_NO_GROUP", 0xffffffff), ("ZMQG_LB_NONE", 0xffffffff),
                          ("ZMQG_LB_NO_PEER", 0xfffffffd)):
        src += "typedef char v_%s[%s == %uu ? 1 : -1];\n" % (c_name, c_name, value)
    # the parent call's struct is unchanged
    src += "typedef char parent[sizeof(zmqg_forward_zmtp) == 232 ? 1 : -1];\n"
    _compiles(src + "int main(void){return 0;}\n")
    assert ctypes.sizeof(curve.ForwardZmtp) == 232
    assert (curve.LB_PREPEND, curve.LB_NO_GROUP, curve.LB_NONE, curve.LB_NO_PEER) == (
        1, 0xffffffff, 0xffffffff, 0xfffffffd)


def test_library_exports_the_call():
    assert os.path.exists(LIB), "build first: make -C libzmq_amd/csrc"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    assert NAME in set(l.split()[-1] for l in out.splitlines() if l.strip())


def test_binding_has_the_call_and_the_pair_bases():
    from libzmq_amd import curve
    K = curve.CurveContext
    for attr in ("forward_zmtp_lb_multi", "forward_lb_pair_base"):
        assert callable(getattr(K, attr))
    assert len(curve._lib.zmqg_forward_zmtp_lb_multi.argtypes) == 4
    # the pair space: one route slot a stream, m = 2 with PREPEND
    ci = [0, 1, 1, 3]
    assert K.forward_lb_pair_base(0, ci, 4, 3) == [0, 5, 9, 15]
    assert K.forward_lb_pair_base(0, ci, 4, 3) == K.forward_router_pair_base(curve.ROUTER_ROUTE, None, ci, 4)
    assert K.forward_lb_pair_base(curve.LB_PREPEND, ci, 4, 3) == [0, 10, 18, 30]
    assert K.forward_lb_pair_base(curve.LB_PREPEND, None, 4, 3) == [0, 8, 16, 24]
    assert K.forward_lb_pair_base(0, None, 0, 2) == [0, 0, 0]


def test_abi_version_unchanged():
    """The call is an addition: the ABI version stays 5."""
    from libzmq_amd import curve
    assert curve._lib.zmqg_abi_version() == 5
    assert re.search(r"#define ZMQG_CURVE_ABI_VERSION 5\b", open(HEADER).read())
