"""CPU-side checks of zmqg_decode_zmtp_multi's boundary (no GPU calls): the
header declares it, the built library exports it, the Python binding has it."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zmqg_curve.h")
LIB = os.path.join(ROOT, "libzmq_amd", "libzmqg_curve.so")
NAME = "zmqg_decode_zmtp_multi"


def test_header_declares_decode_zmtp_multi():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert m, "not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 16
    assert args[0] == "zmqg_ctx *ctx" and args[1] == "uint64_t n_streams" and args[-1] == "void *stream"
    assert args[-2] == "zmqg_zmtp_result *results"


def test_library_exports_decode_zmtp_multi():
    assert os.path.exists(LIB), "build first: make -C libzmq_amd/csrc"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    assert NAME in set(l.split()[-1] for l in out.splitlines() if l.strip())


def test_binding_has_decode_zmtp_multi():
    from libzmq_amd import curve
    assert callable(getattr(curve.CurveContext, "decode_zmtp_multi"))
    assert callable(getattr(curve.CurveContext, "zmtp_results"))
    assert len(curve._lib.zmqg_decode_zmtp_multi.argtypes) == 16


def test_binding_tile_constant_matches_kernel():
    """tests/test_zmtp_multi.py places frame headers around curve.ZMTP_MULTI_TILE."""
    from libzmq_amd import curve
    src = open(os.path.join(ROOT, "libzmq_amd", "csrc", "curve_zmtp_multi.hpp")).read()
    assert int(re.search(r"constexpr uint32_t kZmtpMultiTile = (\d+);", src).group(1)) == curve.ZMTP_MULTI_TILE
