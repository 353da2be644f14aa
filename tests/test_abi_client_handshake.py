"""CPU-side checks of the client handshake calls' boundary (no GPU calls): the
header declares zmqg_curve_client_hello_batch / _welcome_batch / _ready_batch
with their argument lists, the new status code is zmq.h's, the header is still
C99, the built library exports the three names, the Python binding has them,
and the ABI version is unchanged."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zmqg_curve.h")
LIB = os.path.join(ROOT, "libzmq_amd", "libzmqg_curve.so")

ARGS = {
    "zmqg_curve_client_hello_batch": [
        "zmqg_ctx *ctx", "uint64_t n", "const uint8_t *server_pk", "const uint8_t *cn_secret",
        "const uint64_t *nonce", "uint8_t *state", "uint8_t *hello_out", "int32_t *status_out", "void *stream"],
    "zmqg_curve_client_welcome_batch": [
        "zmqg_ctx *ctx", "uint64_t n", "const uint8_t *state", "const uint8_t *client_pk",
        "const uint8_t *client_sk", "const uint64_t *cmd_off", "const uint32_t *cmd_len", "const uint8_t *cmd",
        "const uint8_t *vouch_nonce", "const uint64_t *nonce", "const uint64_t *meta_off",
        "const uint32_t *meta_len", "const uint8_t *meta", "const uint64_t *out_off", "uint8_t *out",
        "uint8_t *precom_out", "int32_t *status_out", "void *stream"],
    "zmqg_curve_client_ready_batch": [
        "zmqg_ctx *ctx", "uint64_t n", "const uint8_t *precom", "const uint64_t *cmd_off", "const uint32_t *cmd_len",
        "const uint8_t *cmd", "uint64_t *peer_nonce_out", "const uint64_t *meta_off", "uint8_t *meta_out",
        "uint32_t *meta_len_out", "int32_t *status_out", "void *stream"],
}


@pytest.mark.parametrize("name", sorted(ARGS))
def test_header_declares_the_call(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, "not declared"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ARGS[name]


def test_new_code_matches_zmq_h():
    """include/zmq.h:433 of the reference."""
    text = open(HEADER).read()
    codes = dict(re.findall(r"#define (ZMQG_[A-Z_]+)\s+(0x[0-9a-f]+|\d+)", text))
    assert int(codes["ZMQG_ERR_MALFORMED_READY"], 16) == 0x10000016
    assert (codes["ZMQG_HS_HELLO_BYTES"], codes["ZMQG_HS_CLIENT_STATE_BYTES"]) == ("200", "128")


def test_header_compiles_as_c99_with_the_calls():
    src = ('#include "zmqg_curve.h"\n'
           'int main(void){\n'
           ' int (*h)(zmqg_ctx *, uint64_t, const uint8_t *, const uint8_t *, const uint64_t *, uint8_t *, uint8_t *,\n'
           '          int32_t *, void *) = zmqg_curve_client_hello_batch;\n'
           ' int (*w)(zmqg_ctx *, uint64_t, const uint8_t *, const uint8_t *, const uint8_t *, const uint64_t *,\n'
           '          const uint32_t *, const uint8_t *, const uint8_t *, const uint64_t *, const uint64_t *,\n'
           '          const uint32_t *, const uint8_t *, const uint64_t *, uint8_t *, uint8_t *, int32_t *, void *)\n'
           '     = zmqg_curve_client_welcome_batch;\n'
           ' int (*r)(zmqg_ctx *, uint64_t, const uint8_t *, const uint64_t *, const uint32_t *, const uint8_t *,\n'
           '          uint64_t *, const uint64_t *, uint8_t *, uint32_t *, int32_t *, void *)\n'
           '     = zmqg_curve_client_ready_batch;\n'
           ' return (h && w && r && ZMQG_CURVE_ABI_VERSION == 5 && ZMQG_ERR_MALFORMED_READY == 0x10000016\n'
           '         && ZMQG_HS_HELLO_BYTES == 200 && ZMQG_HS_CLIENT_STATE_BYTES == 128) ? 0 : 1;}\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_library_exports_the_calls():
    assert os.path.exists(LIB), "build first: make -C libzmq_amd/csrc"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert not [n for n in ARGS if n not in exported]


def test_binding_has_the_calls():
    from libzmq_amd import curve
    for method, name in (("client_hello_batch", "zmqg_curve_client_hello_batch"),
                         ("client_welcome_batch", "zmqg_curve_client_welcome_batch"),
                         ("client_ready_batch", "zmqg_curve_client_ready_batch")):
        assert callable(getattr(curve.CurveContext, method))
        assert len(getattr(curve._lib, name).argtypes) == len(ARGS[name])
    assert curve.ERR_MALFORMED_READY == 0x10000016
    assert (curve.HS_HELLO_BYTES, curve.HS_CLIENT_STATE_BYTES) == (200, 128)


def test_abi_version_unchanged():
    """The calls are additions: the ABI version stays 5."""
    from libzmq_amd import curve
    assert curve._lib.zmqg_abi_version() == 5
