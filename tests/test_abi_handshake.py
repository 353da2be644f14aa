"""CPU-side checks of the handshake calls' boundary (no GPU calls): the header
declares zmqg_curve_server_hello_batch / _initiate_batch / _ready_batch with
their argument lists, the new status codes are zmq.h's, the header is still
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
    "zmqg_curve_server_hello_batch": [
        "zmqg_ctx *ctx", "uint64_t n", "const uint8_t server_sk[32]", "const uint64_t *cmd_off",
        "const uint32_t *cmd_len", "const uint8_t *cmd", "const uint8_t *random", "uint8_t *state",
        "uint8_t *welcome_out", "int32_t *status_out", "void *stream"],
    "zmqg_curve_server_initiate_batch": [
        "zmqg_ctx *ctx", "uint64_t n", "const uint8_t *state", "const uint64_t *cmd_off", "const uint32_t *cmd_len",
        "const uint8_t *cmd", "uint8_t *client_key_out", "uint8_t *precom_out", "uint64_t *peer_nonce_out",
        "const uint64_t *meta_off", "uint8_t *meta_out", "uint32_t *meta_len_out", "int32_t *status_out",
        "void *stream"],
    "zmqg_curve_server_ready_batch": [
        "zmqg_ctx *ctx", "uint64_t n", "const uint8_t *precom", "const uint64_t *nonce", "const uint64_t *meta_off",
        "const uint32_t *meta_len", "const uint8_t *meta", "const uint64_t *out_off", "uint8_t *out", "void *stream"],
}


@pytest.mark.parametrize("name", sorted(ARGS))
def test_header_declares_the_call(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, "not declared"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ARGS[name]


def test_new_codes_match_zmq_h():
    """include/zmq.h:427-431 of the reference."""
    text = open(HEADER).read()
    codes = dict(re.findall(r"#define (ZMQG_[A-Z_]+)\s+(0x[0-9a-f]+|\d+)", text))
    assert int(codes["ZMQG_ERR_KEY_EXCHANGE"], 16) == 0x10000003
    assert int(codes["ZMQG_ERR_MALFORMED_HELLO"], 16) == 0x10000013
    assert int(codes["ZMQG_ERR_MALFORMED_INITIATE"], 16) == 0x10000014
    assert (codes["ZMQG_HS_STATE_BYTES"], codes["ZMQG_HS_RANDOM_BYTES"], codes["ZMQG_HS_WELCOME_BYTES"]) == (
        "128", "96", "168")


def test_header_compiles_as_c99_with_the_calls():
    src = ('#include "zmqg_curve.h"\n'
           'int main(void){\n'
           ' int (*h)(zmqg_ctx *, uint64_t, const uint8_t *, const uint64_t *, const uint32_t *, const uint8_t *,\n'
           '          const uint8_t *, uint8_t *, uint8_t *, int32_t *, void *) = zmqg_curve_server_hello_batch;\n'
           ' int (*i)(zmqg_ctx *, uint64_t, const uint8_t *, const uint64_t *, const uint32_t *, const uint8_t *,\n'
           '          uint8_t *, uint8_t *, uint64_t *, const uint64_t *, uint8_t *, uint32_t *, int32_t *, void *)\n'
           '     = zmqg_curve_server_initiate_batch;\n'
           ' int (*r)(zmqg_ctx *, uint64_t, const uint8_t *, const uint64_t *, const uint64_t *, const uint32_t *,\n'
           '          const uint8_t *, const uint64_t *, uint8_t *, void *) = zmqg_curve_server_ready_batch;\n'
           ' return (h && i && r && ZMQG_CURVE_ABI_VERSION == 5 && ZMQG_ERR_KEY_EXCHANGE == 0x10000003) ? 0 : 1;}\n')
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
    for method, name in (("server_hello_batch", "zmqg_curve_server_hello_batch"),
                         ("server_initiate_batch", "zmqg_curve_server_initiate_batch"),
                         ("server_ready_batch", "zmqg_curve_server_ready_batch")):
        assert callable(getattr(curve.CurveContext, method))
        assert len(getattr(curve._lib, name).argtypes) == len(ARGS[name])
    assert (curve.ERR_KEY_EXCHANGE, curve.ERR_MALFORMED_HELLO, curve.ERR_MALFORMED_INITIATE) == (
        0x10000003, 0x10000013, 0x10000014)


def test_abi_version_unchanged():
    """The calls are additions: the ABI version stays 5."""
    from libzmq_amd import curve
    assert curve._lib.zmqg_abi_version() == 5
