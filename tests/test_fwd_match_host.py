"""The prefix compare of zmqg_forward_zmtp_sub_multi's match kernel
(fwd_prefix_match and fwd_sub_range, libzmq_amd/csrc/curve_fwd_match.hpp),
compiled for the host with AddressSanitizer and UBSan as a stand-alone program
and run: the prefix edge table (empty, equal, one byte longer, one byte
shorter, last byte differing, first byte differing) for topics of 0 to 300
bytes and staging windows of 0 to 256, topic and sub_bytes in heap blocks of
exactly their size, and a subscription that claims one byte past
sub_bytes_len, which must neither match nor be read."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fwd_prefix_match_host(tmp_path):
    exe = str(tmp_path / "test_fwd_match")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++11", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "test_fwd_match.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fwd_match ok" in r.stdout
