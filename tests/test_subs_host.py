"""The two pure helpers of zmqg_subs_update_multi's kernels (subs_classify and
subs_slot_equal, libzmq_amd/csrc/curve_subs.hpp), compiled for the host with
AddressSanitizer and UBSan as a stand-alone program and run: every
classification edge (payloads of 0, 1, 6, 7, 9 and 10 bytes, a name length byte
past the end, "\\x09SUBSCRIBX", a first byte of 0 / 1 / 2 with and without
COMMAND) and the slot compare for lengths 0 to 41, payloads and slots in heap
blocks of exactly their size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_subs_helpers_host(tmp_path):
    exe = str(tmp_path / "test_subs")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++11", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "test_subs.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "subs ok" in r.stdout
