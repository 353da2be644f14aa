"""The id lookup of zmqg_forward_zmtp_router_multi's route kernel (fwd_id_view,
fwd_id_less, fwd_id_equal and fwd_route_lookup,
libzmq_amd/csrc/curve_fwd_route.hpp), compiled for the host with
AddressSanitizer and UBSan as a stand-alone program and run: void entries
(offset past the end, length past the end, off + len overflowing 64 bits), the
ordering edge cases (a prefix of the other, equal bytes with different length,
the empty id, a difference in the last byte only or the first only) under
staging windows of 0 to 256 bytes, n_ids 0 and 1, and a random sweep against
std::map<std::string, uint32_t>::find on sorted tables of up to 1000 ids; the
address and id_bytes lie in heap blocks of exactly their size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fwd_route_lookup_host(tmp_path):
    exe = str(tmp_path / "test_fwd_route")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++11", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "test_fwd_route.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fwd_route ok" in r.stdout
