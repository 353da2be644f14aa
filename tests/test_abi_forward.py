"""CPU-side checks of zmqg_forward_zmtp_multi's boundary (no GPU calls): the
header declares the call and its two structs, zmqg_forward_result is 32 bytes
in C with the documented offsets, the built library exports the call, the
Python binding has it with structures of the C sizes, and the ABI version is
still 5."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zmqg_curve.h")
LIB = os.path.join(ROOT, "libzmq_amd", "libzmqg_curve.so")
NAME = "zmqg_forward_zmtp_multi"

# zmqg_forward_zmtp's members in order (LP64: every member but the first two is 8 bytes)
FIELDS = ["size", "reserved", "n_streams", "stream_sid", "stream_off", "stream_len", "in", "max_msg_size",
          "max_frames", "frame_in_off", "frame_len", "plain_off", "plain", "flags_out", "status_out", "results",
          "carry_idx", "carry_off", "carry_len", "carry_flags", "n_dst", "dst_sid", "route_idx", "route_dst", "out",
          "out_bytes", "pair_off", "pair_status", "dst_results", "fwd"]


def _text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_call_and_its_structs():
    text = _text()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert m, "not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["zmqg_ctx *ctx", "const zmqg_forward_zmtp *args", "void *stream"]
    for struct in ("zmqg_forward_result", "zmqg_forward_zmtp"):
        assert re.search(r"typedef\s+struct\s+%s\s*\{[^}]*\}\s*%s\s*;" % (struct, struct), text), struct


def _compiles(src):
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_forward_result_is_32_bytes_in_c():
    _compiles('#include <stddef.h>\n#include "zmqg_curve.h"\n'
              'typedef char size_is_32[sizeof(zmqg_forward_result) == 32 ? 1 : -1];\n'
              'typedef char off_seq[offsetof(zmqg_forward_result, seq) == 0 ? 1 : -1];\n'
              'typedef char off_held_first[offsetof(zmqg_forward_result, held_first) == 8 ? 1 : -1];\n'
              'typedef char off_forwarded[offsetof(zmqg_forward_result, forwarded) == 16 ? 1 : -1];\n'
              'typedef char off_failed[offsetof(zmqg_forward_result, failed) == 24 ? 1 : -1];\n'
              'typedef char off_pad[offsetof(zmqg_forward_result, pad) == 28 ? 1 : -1];\n'
              'int main(void){return 0;}\n')


def test_forward_zmtp_layout_in_c_matches_the_binding():
    """Every member at the offset the Python structure gives it (the binding's
    `inp` is the header's `in`), and the same total size."""
    from libzmq_amd import curve
    py = [("in" if n == "inp" else n, getattr(curve.ForwardZmtp, n).offset) for n, _ in curve.ForwardZmtp._fields_]
    assert [n for n, _ in py] == FIELDS
    src = '#include <stddef.h>\n#include "zmqg_curve.h"\n'
    src += "typedef char total[sizeof(zmqg_forward_zmtp) == %d ? 1 : -1];\n" % ctypes.sizeof(curve.ForwardZmtp)
    for n, off in py:
        src += "typedef char off_%s[offsetof(zmqg_forward_zmtp, %s) == %d ? 1 : -1];\n" % (n, n, off)
    _compiles(src + "int main(void){return 0;}\n")
    assert ctypes.sizeof(curve.ForwardResult) == 32
    assert [(n, getattr(curve.ForwardResult, n).offset) for n, _ in curve.ForwardResult._fields_] == [
        ("seq", 0), ("held_first", 8), ("forwarded", 16), ("failed", 24), ("pad", 28)]


def test_library_exports_the_call():
    assert os.path.exists(LIB), "build first: make -C libzmq_amd/csrc"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    assert NAME in set(l.split()[-1] for l in out.splitlines() if l.strip())


def test_binding_has_the_call():
    from libzmq_amd import curve
    for attr in ("forward_zmtp_multi", "forward_results", "forward_pair_base"):
        assert callable(getattr(curve.CurveContext, attr))
    assert len(curve._lib.zmqg_forward_zmtp_multi.argtypes) == 3
    # base(s) = the sum of (c(t) + max_frames) * d(t): routes 2, 1, 0, 2 and carries 1, 0, 3, 0 at max_frames 6
    assert curve.CurveContext.forward_pair_base([0, 2, 3, 3, 5], [0, 1, 1, 4, 4], 6) == [0, 14, 20, 20, 32]
    assert curve.CurveContext.forward_pair_base([0, 2, 3, 3, 5], None, 6) == [0, 12, 18, 18, 30]


def test_abi_version_unchanged():
    """The call is an addition: the ABI version stays 5."""
    from libzmq_amd import curve
    assert curve._lib.zmqg_abi_version() == 5
    assert re.search(r"#define ZMQG_CURVE_ABI_VERSION 5\b", open(HEADER).read())
