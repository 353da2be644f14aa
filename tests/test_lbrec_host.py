"""The look-back record's pack / valid / value helpers
(libzmq_amd/csrc/curve_lbrec.hpp), compiled for the host with
AddressSanitizer and UBSan as a stand-alone program and run: epochs 1,
2^31 - 1, 2^31 and 2^32 - 1, values 0, 2^32 - 1, 2^32 and 2^64 - 1, a zero
record invalid, records of other calls invalid."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lbrec_pack_unpack_host(tmp_path):
    exe = str(tmp_path / "test_lbrec")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++11", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "host", "test_lbrec.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lbrec ok" in r.stdout
