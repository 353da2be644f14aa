"""CPU-side checks of zmqg_encode_zmtp_multi's boundary (no GPU calls): the
header declares it, its result struct is 32 bytes in C, the built library
exports it, the Python binding has it."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zmqg_curve.h")
LIB = os.path.join(ROOT, "libzmq_amd", "libzmqg_curve.so")
NAME = "zmqg_encode_zmtp_multi"


def test_header_declares_encode_zmtp_multi():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert m, "not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 16
    assert args[0] == "zmqg_ctx *ctx" and args[1] == "uint64_t n_streams" and args[-1] == "void *stream"
    assert args[-2] == "zmqg_zmtp_send_result *results"


def test_send_result_is_32_bytes_in_c():
    src = ('#include <stddef.h>\n#include "zmqg_curve.h"\n'
           'typedef char size_is_32[sizeof(zmqg_zmtp_send_result) == 32 ? 1 : -1];\n'
           'typedef char same_as_recv[sizeof(zmqg_zmtp_send_result) == sizeof(zmqg_zmtp_result) ? 1 : -1];\n'
           'typedef char off_frames[offsetof(zmqg_zmtp_send_result, frames) == 0 ? 1 : -1];\n'
           'typedef char off_out_off[offsetof(zmqg_zmtp_send_result, out_off) == 8 ? 1 : -1];\n'
           'typedef char off_out_bytes[offsetof(zmqg_zmtp_send_result, out_bytes) == 16 ? 1 : -1];\n'
           'typedef char off_error[offsetof(zmqg_zmtp_send_result, error) == 24 ? 1 : -1];\n'
           'int main(void){return 0;}\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_library_exports_encode_zmtp_multi():
    assert os.path.exists(LIB), "build first: make -C libzmq_amd/csrc"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    assert NAME in set(l.split()[-1] for l in out.splitlines() if l.strip())


def test_binding_has_encode_zmtp_multi():
    from libzmq_amd import curve
    assert callable(getattr(curve.CurveContext, "encode_zmtp_multi"))
    assert callable(getattr(curve.CurveContext, "zmtp_send_results"))
    assert len(curve._lib.zmqg_encode_zmtp_multi.argtypes) == 16


def test_abi_version_unchanged():
    """The call is an addition: the ABI version stays 5."""
    from libzmq_amd import curve
    assert curve._lib.zmqg_abi_version() == 5
