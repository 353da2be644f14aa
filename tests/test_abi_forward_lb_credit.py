"""CPU-side checks of zmqg_forward_lb_credit_multi's boundary (no GPU calls):
the header compiles as C and as C++ and declares the call with its five
parameters, the library exports it and the binding has it, its own block cites
lb_t's loop, the deactivation and check_hwm, states the loop and the cursor's
meaning, the two "Not offered" paragraphs that refused the load balancer under
credits point to it and keep their words, the table at the top names it, the
ABI version is still 5, zmqg_forward_credit_multi still refuses ZMQG_FWD_LB,
and the -EINVAL cases of the credit struct and the mode return before the ctx
or the device is touched."""
import ctypes
import errno
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zmqg_curve.h")
LIB = os.path.join(ROOT, "libzmq_amd", "libzmqg_curve.so")
NAME = "zmqg_forward_lb_credit_multi"


def _text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _compiles(src, cxx=False):
    cmd = ["g++", "-std=c++11", "-x", "c++"] if cxx else ["gcc", "-std=c99", "-x", "c"]
    r = subprocess.run(cmd[:2] + ["-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")] + cmd[2:] +
                       ["-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_header_declares_the_call():
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, _text())
    assert m, "not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["zmqg_ctx *ctx", "const zmqg_forward_zmtp *args", "const zmqg_forward_framing *framing",
                    "const zmqg_forward_credit *credit", "void *stream"]


def test_compiles_in_c_and_cxx_with_the_credit_calls_struct():
    src = '#include <stddef.h>\n#include "zmqg_curve.h"\n'
    src += "typedef char total[sizeof(zmqg_forward_credit) == 32 ? 1 : -1];\n"
    src += "typedef char abi[ZMQG_CURVE_ABI_VERSION == 5 ? 1 : -1];\n"
    src += "typedef char hwm[ZMQG_ERR_HWM == 0x7a000003 ? 1 : -1];\n"
    src += "typedef char lb[ZMQG_FWD_LB == 3u ? 1 : -1];\n"
    src += "int (*const call)(zmqg_ctx *, const zmqg_forward_zmtp *, const zmqg_forward_framing *,\n"
    src += "                  const zmqg_forward_credit *, void *) = %s;\n" % NAME
    src += "int main(void){return sizeof call == 0;}\n"
    _compiles(src)
    _compiles(src, cxx=True)


def test_library_exports_the_call_and_the_binding_has_it():
    from libzmq_amd import curve
    assert os.path.exists(LIB), "build first: make -C libzmq_amd/csrc"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    assert NAME in set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert callable(curve.CurveContext.forward_lb_credit_multi)
    assert len(curve._lib.zmqg_forward_lb_credit_multi.argtypes) == 5


def test_the_header_states_the_contract_and_points_to_it():
    raw = open(HEADER).read()
    blocks = re.findall(r"/\*.*?\*/", raw, flags=re.S)
    flat = lambda b: " ".join(b.replace("*", " ").split())
    own = [b for b in blocks if b.startswith("/* %s:" % NAME)]
    assert len(own) == 1
    text = flat(own[0])
    for cite in ("src/lb.cpp:56-131", ":103-107", "src/pipe.cpp:535-541", "src/pipe.cpp:222-234", "src/lb.cpp:78-101"):
        assert cite in text, cite
    for word in ("swap entries cur and A", "original ring position", "ZMQG_ERR_HWM", "ZMQG_LB_NO_PEER", "Identity.",
                 "saturates at 0", "approximate across calls", "Launches:", "epochs", "unspecified"):
        assert word in text, word
    off = text.split("Not offered:")[-1]
    for word in ("permuted ring", "has_out", "ZMQ_XPUB_NODROP", "ZMQ_ROUTER_MANDATORY", "low-water mark", "bytes",
                 "compacting"):
        assert word in off, word
    # the two paragraphs that sent the reader away now say where to
    for call in ("zmqg_forward_zmtp_lb_multi", "zmqg_forward_credit_multi"):
        tail = flat([b for b in blocks if b.startswith("/* %s:" % call)][0]).split("Not offered:")[-1]
        assert NAME in tail, call
        assert "src/lb.cpp:103-107" in tail, call
    top = flat(blocks[0])
    assert re.search(r"src/lb\.cpp:56-131 \(:103-107\), src/pipe\.cpp:207-220, :535-541 " + NAME, top)


def test_abi_version_unchanged():
    from libzmq_amd import curve
    assert curve._lib.zmqg_abi_version() == 5


def _caller(C, fn, fake, ptr):
    def call(ctx=None, null_args=False, null_framing=False, null_credit=False, mode=C.FWD_LB, n_dst=2, fr=None,
             a_size=None, plan=True, **cr):
        ctx = ctypes.addressof(fake) if ctx is None else ctx
        a = C.ForwardZmtp(ctypes.sizeof(C.ForwardZmtp) if a_size is None else a_size, 0)
        a.n_streams, a.n_dst = 1, n_dst
        lb = C.ForwardLb(ctypes.sizeof(C.ForwardLb), 0)
        f = C.ForwardFraming(ctypes.sizeof(C.ForwardFraming), 0, C.FRAMING_ZMTP, C.FRAMING_ZMTP, mode, 0,
                             ctypes.addressof(lb) if plan else None, None, None)
        for k, v in (fr or {}).items():
            setattr(f, k, v)
        c = C.ForwardCredit(ctypes.sizeof(C.ForwardCredit), 0, ptr, ptr, ptr)
        for k, v in cr.items():
            setattr(c, k, v)
        return fn(ctx, None if null_args else ctypes.byref(a), None if null_framing else ctypes.byref(f),
                  None if null_credit else ctypes.byref(c), None)
    return call


def test_einval_before_the_ctx_is_touched():
    """A defect of the credit struct, a mode other than the load balancer's, a
    missing credit array with destinations, a null argument, and the framed LB
    call's own launch-free cases: -EINVAL without a read of the ctx (a block of
    zeros stands for it: no device is opened here)."""
    from libzmq_amd import curve as C
    fake = ctypes.create_string_buffer(4096)
    words = (ctypes.c_uint32 * 4)()
    ptr = ctypes.addressof(words)
    E = -errno.EINVAL
    call = _caller(C, C._lib.zmqg_forward_lb_credit_multi, fake, ptr)
    assert call(ctx=0) == E and call(null_args=True) == E and call(null_framing=True) == E
    assert call(null_credit=True) == E
    assert call(size=0) == E and call(size=24) == E and call(size=40) == E
    assert call(flags=2) == E and call(flags=3) == E and call(flags=0x80000000) == E
    for mode in (C.FWD_STATIC, C.FWD_SUB, C.FWD_ROUTER, 4):
        assert call(mode=mode) == E and call(mode=mode, plan=False) == E
    assert call(dst_credit=None) == E and call(dst_taken=None) == E and call(dst_dropped=None) == E
    assert call(fr=dict(size=40)) == E and call(a_size=8) == E
    # the framed call's and the load balancer's own: no plan, a reserved word, a framing out of range; a stream
    # without stream_group (the zeroed zmqg_forward_lb has none)
    assert call(plan=False) == E and call(fr=dict(reserved=1)) == E and call(fr=dict(recv=3)) == E
    assert call() == E
    assert bytes(fake) == bytes(4096) and list(words) == [0] * 4


def test_the_credit_call_still_refuses_the_load_balancer():
    from libzmq_amd import curve as C
    fake = ctypes.create_string_buffer(4096)
    words = (ctypes.c_uint32 * 4)()
    call = _caller(C, C._lib.zmqg_forward_credit_multi, fake, ctypes.addressof(words))
    assert call(mode=C.FWD_LB) == -errno.EINVAL and call(mode=C.FWD_LB, plan=False) == -errno.EINVAL
    assert bytes(fake) == bytes(4096)
