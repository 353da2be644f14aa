"""CPU-side checks of the WebSocket calls' boundary (no GPU calls): the header
declares zmqg_decode_ws_multi and zmqg_encode_ws_multi, zmqg_ws_result is 48
bytes in C, the built library exports both, the Python binding has them, and
the ABI version is still 5."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zmqg_curve.h")
LIB = os.path.join(ROOT, "libzmq_amd", "libzmqg_curve.so")
NAMES = ["zmqg_decode_ws_multi", "zmqg_encode_ws_multi"]


def _args(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, "not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_decode_ws_multi():
    args = _args("zmqg_decode_ws_multi")
    assert len(args) == 17
    assert args[0] == "zmqg_ctx *ctx" and args[1] == "uint64_t n_streams" and args[-1] == "void *stream"
    assert args[6] == "int must_mask" and args[7] == "int64_t max_msg_size" and args[-2] == "zmqg_ws_result *results"


def test_header_declares_encode_ws_multi():
    args = _args("zmqg_encode_ws_multi")
    assert len(args) == 17
    assert args[0] == "zmqg_ctx *ctx" and args[1] == "uint64_t n_streams" and args[-1] == "void *stream"
    assert args[10] == "const uint32_t *mask" and args[11] == "uint8_t *out"
    assert args[-2] == "zmqg_zmtp_send_result *results"
    # the ZMTP call's arguments with `mask` put in front of `out`
    assert [a for a in args if a != "const uint32_t *mask"] == _args("zmqg_encode_zmtp_multi")


def test_ws_result_is_48_bytes_in_c():
    src = ('#include <stddef.h>\n#include "zmqg_curve.h"\n'
           'typedef char size_is_48[sizeof(zmqg_ws_result) == 48 ? 1 : -1];\n'
           'typedef char off_frames[offsetof(zmqg_ws_result, frames) == 0 ? 1 : -1];\n'
           'typedef char off_consumed[offsetof(zmqg_ws_result, consumed) == 8 ? 1 : -1];\n'
           'typedef char off_out_bytes[offsetof(zmqg_ws_result, out_bytes) == 16 ? 1 : -1];\n'
           'typedef char off_error[offsetof(zmqg_ws_result, error) == 24 ? 1 : -1];\n'
           'typedef char off_ctl_opcode[offsetof(zmqg_ws_result, ctl_opcode) == 28 ? 1 : -1];\n'
           'typedef char off_ctl_off[offsetof(zmqg_ws_result, ctl_off) == 32 ? 1 : -1];\n'
           'typedef char off_ctl_len[offsetof(zmqg_ws_result, ctl_len) == 40 ? 1 : -1];\n'
           'typedef char recv_is_32[sizeof(zmqg_zmtp_result) == 32 ? 1 : -1];\n'
           'typedef char send_is_32[sizeof(zmqg_zmtp_send_result) == 32 ? 1 : -1];\n'
           'int main(void){return 0;}\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


@pytest.mark.parametrize("name", NAMES)
def test_library_exports(name):
    assert os.path.exists(LIB), "build first: make -C libzmq_amd/csrc"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    assert name in set(l.split()[-1] for l in out.splitlines() if l.strip())


def test_binding_has_the_ws_calls():
    from libzmq_amd import curve
    for attr in ("decode_ws_multi", "ws_results", "encode_ws_multi", "zmtp_send_results"):
        assert callable(getattr(curve.CurveContext, attr))
    assert len(curve._lib.zmqg_decode_ws_multi.argtypes) == 17
    assert len(curve._lib.zmqg_encode_ws_multi.argtypes) == 17
    assert curve.WS_MULTI_TILE == 16384


def test_abi_version_unchanged():
    """The calls are additions: the ABI version stays 5."""
    from libzmq_amd import curve
    assert curve._lib.zmqg_abi_version() == 5
