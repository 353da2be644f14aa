"""CPU-side checks of zmqg_decode_zmtp's boundary (no GPU calls): the binding's
scan tile is the kernel's, and the header states the two contracts the steered
tests (tests/test_zmtp_scan_model.py, tests/test_gpu_zmtp_scan_edges.py) hold
the code to."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zmqg_curve.h")


def test_binding_scan_tile_matches_kernel():
    """tests/zmtp_scan_steer.py and tests/zmtp_scan_model.py take the tile from curve.ZMTP_SCAN_TILE."""
    from libzmq_amd import curve
    src = open(os.path.join(ROOT, "libzmq_amd", "csrc", "curve_zmtp.hpp")).read()
    threads = int(re.search(r"constexpr uint32_t kZmtpThreads = (\d+);", src).group(1))
    m = re.search(r"constexpr uint32_t kZmtpWgBytes = (\d+)u \* kZmtpThreads;", src)
    assert threads == 256 and int(m.group(1)) * threads == curve.ZMTP_SCAN_TILE == 16384


def test_header_states_early_stop_and_alignment():
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    assert "may return fewer frames than are complete" in text
    assert "until a call returns 0 frames" in text
    assert "any byte alignment of `in` is valid" in text
