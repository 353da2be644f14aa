"""The admit arithmetic of zmqg_forward_credit_multi's kernels
(fwd_credit_admits, fwd_credit_taken, fwd_credit_dropped and fwd_credit_left,
libzmq_amd/csrc/curve_fwd_credit.hpp), compiled for the host with
AddressSanitizer and UBSan as a stand-alone program and run: credits of 0, 1,
D - 1, D, D + 1 and unlimited, counts and credits near 2^32 - 1, the consume
write-back never wrapping and never producing the unlimited value, and a sweep
against pipe_t's own counters (src/pipe.cpp:207-234, :535-541); the credit,
taken and dropped arrays lie in heap blocks of exactly their size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fwd_credit_admit_host(tmp_path):
    exe = str(tmp_path / "test_fwd_credit")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++11", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "test_fwd_credit.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fwd_credit ok" in r.stdout
