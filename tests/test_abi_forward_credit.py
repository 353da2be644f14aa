"""CPU-side checks of zmqg_forward_credit_multi's boundary (no GPU calls): the
header compiles as C and as C++ and declares the call with its five parameters,
zmqg_forward_credit is 32 bytes with every member at the binding's offset,
ZMQG_ERR_HWM and the ZMQG_CREDIT_* values are the header's and the binding's,
the library exports the call, the three "Not offered" paragraphs that spoke of
high-water marks and the table at the top name it, its own block says why the
load balancer is refused, the ABI version is still 5, and the -EINVAL cases of
the credit struct return before the ctx or the device is touched."""
import ctypes
import errno
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zmqg_curve.h")
LIB = os.path.join(ROOT, "libzmq_amd", "libzmqg_curve.so")
NAME = "zmqg_forward_credit_multi"

# zmqg_forward_credit's members in order with their offsets (LP64)
FIELDS = [("size", 0), ("flags", 4), ("dst_credit", 8), ("dst_taken", 16), ("dst_dropped", 24)]


def _text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _compiles(src, cxx=False):
    cmd = ["g++", "-std=c++11", "-x", "c++"] if cxx else ["gcc", "-std=c99", "-x", "c"]
    r = subprocess.run(cmd[:2] + ["-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")] + cmd[2:] +
                       ["-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_header_declares_the_call_and_its_struct():
    text = _text()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert m, "not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["zmqg_ctx *ctx", "const zmqg_forward_zmtp *args", "const zmqg_forward_framing *framing",
                    "const zmqg_forward_credit *credit", "void *stream"]
    assert re.search(r"typedef\s+struct\s+zmqg_forward_credit\s*\{[^}]*\}\s*zmqg_forward_credit\s*;", text)


def test_layout_and_constants_in_c_and_cxx_match_the_binding():
    from libzmq_amd import curve
    py = [(n, getattr(curve.ForwardCredit, n).offset) for n, _ in curve.ForwardCredit._fields_]
    assert py == FIELDS and ctypes.sizeof(curve.ForwardCredit) == 32
    assert (curve.ERR_HWM, curve.CREDIT_UNLIMITED, curve.CREDIT_CONSUME) == (0x7a000003, 0xffffffff, 1)
    src = '#include <stddef.h>\n#include "zmqg_curve.h"\n'
    src += "typedef char total[sizeof(zmqg_forward_credit) == 32 ? 1 : -1];\n"
    for n, off in py:
        src += "typedef char off_%s[offsetof(zmqg_forward_credit, %s) == %d ? 1 : -1];\n" % (n, n, off)
    src += "typedef char hwm[ZMQG_ERR_HWM == 0x7a000003 ? 1 : -1];\n"
    src += "typedef char unl[ZMQG_CREDIT_UNLIMITED == 0xffffffffu ? 1 : -1];\n"
    src += "typedef char con[ZMQG_CREDIT_CONSUME == 1u ? 1 : -1];\n"
    src += "typedef char abi[ZMQG_CURVE_ABI_VERSION == 5 ? 1 : -1];\n"
    src += "int (*const call)(zmqg_ctx *, const zmqg_forward_zmtp *, const zmqg_forward_framing *,\n"
    src += "                  const zmqg_forward_credit *, void *) = zmqg_forward_credit_multi;\n"
    src += "int main(void){return sizeof call == 0;}\n"
    _compiles(src)
    _compiles(src, cxx=True)


def test_library_exports_the_call_and_the_binding_has_it():
    from libzmq_amd import curve
    assert os.path.exists(LIB), "build first: make -C libzmq_amd/csrc"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    assert NAME in set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert callable(curve.CurveContext.forward_credit_multi)
    assert len(curve._lib.zmqg_forward_credit_multi.argtypes) == 5


def test_the_header_points_to_it():
    raw = open(HEADER).read()
    blocks = re.findall(r"/\*.*?\*/", raw, flags=re.S)
    flat = lambda b: " ".join(b.replace("*", " ").split())
    for call in ("zmqg_forward_zmtp_sub_multi", "zmqg_forward_zmtp_router_multi", "zmqg_forward_zmtp_lb_multi"):
        own = [b for b in blocks if b.startswith("/* %s:" % call)]
        assert len(own) == 1, call
        tail = flat(own[0]).split("Not offered:")[-1]
        assert re.search(r"high-water marks[^;]*zmqg_forward_credit_multi", tail), call
    top = flat(blocks[0])
    assert re.search(r"src/pipe\.cpp:535-541, :207-234, src/dist\.cpp:196-210, src/router\.cpp:185-200 " + NAME, top)
    own = [b for b in blocks if b.startswith("/* %s:" % NAME)]
    assert len(own) == 1
    text = flat(own[0])
    for cite in ("src/pipe.cpp:535-541", "src/pipe.cpp:207-234", "src/dist.cpp:196-210", "src/router.cpp:185-200",
                 "src/lb.cpp:103-107", "src/xpub.cpp:314"):
        assert cite in text, cite
    off = text.split("Not offered:")[-1]
    for word in ("ZMQG_FWD_LB", "ZMQ_XPUB_NODROP", "ZMQ_ROUTER_MANDATORY", "low-water mark", "bytes"):
        assert word in off, word


def test_abi_version_unchanged():
    from libzmq_amd import curve
    assert curve._lib.zmqg_abi_version() == 5
    assert re.search(r"#define ZMQG_CURVE_ABI_VERSION 5\b", open(HEADER).read())


def test_einval_before_the_ctx_is_touched():
    """A defect of the credit struct, the load balancer's mode, a missing
    credit array with destinations, a null argument: -EINVAL without a read of
    the ctx (a block of zeros stands for it: no device is opened here)."""
    from libzmq_amd import curve as C
    fake = ctypes.create_string_buffer(4096)
    words = (ctypes.c_uint32 * 4)()
    ptr = ctypes.addressof(words)
    E = -errno.EINVAL

    def call(ctx=ctypes.addressof(fake), null_args=False, null_framing=False, null_credit=False, mode=C.FWD_STATIC,
             n_dst=2, fr=None, a_size=None, **cr):
        a = C.ForwardZmtp(ctypes.sizeof(C.ForwardZmtp) if a_size is None else a_size, 0)
        a.n_streams, a.n_dst = 1, n_dst
        f = C.ForwardFraming(ctypes.sizeof(C.ForwardFraming), 0, C.FRAMING_ZMTP, C.FRAMING_ZMTP, mode, 0, None, None,
                             None)
        for k, v in (fr or {}).items():
            setattr(f, k, v)
        c = C.ForwardCredit(ctypes.sizeof(C.ForwardCredit), 0, ptr, ptr, ptr)
        for k, v in cr.items():
            setattr(c, k, v)
        return C._lib.zmqg_forward_credit_multi(ctx, None if null_args else ctypes.byref(a),
                                                None if null_framing else ctypes.byref(f),
                                                None if null_credit else ctypes.byref(c), None)

    assert call(ctx=None) == E and call(null_args=True) == E and call(null_framing=True) == E
    assert call(null_credit=True) == E
    assert call(size=0) == E and call(size=24) == E and call(size=40) == E
    assert call(flags=2) == E and call(flags=3) == E and call(flags=0x80000000) == E
    lb = C.ForwardLb(ctypes.sizeof(C.ForwardLb), 0)
    assert call(mode=C.FWD_LB, fr=dict(plan=ctypes.addressof(lb))) == E and call(mode=C.FWD_LB) == E
    assert call(dst_credit=None) == E and call(dst_taken=None) == E and call(dst_dropped=None) == E
    assert call(fr=dict(size=40)) == E and call(a_size=8) == E
    assert bytes(fake) == bytes(4096) and list(words) == [0] * 4
