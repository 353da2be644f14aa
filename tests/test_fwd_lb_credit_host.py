"""The per-entry arithmetic of zmqg_forward_lb_credit_multi's group kernel
(fwd_lbc_dist, fwd_lbc_full_at, fwd_lbc_visits, fwd_lbc_left,
fwd_lbc_deactivate and fwd_lbc_orig, libzmq_amd/csrc/curve_fwd_lb_credit.hpp),
compiled for the host with AddressSanitizer and UBSan as a stand-alone program
and run: a sequential driver that walks a ring in epochs, as the kernel does,
against lb_t's loop taken message by message (src/lb.cpp:56-131, :103-107) --
rings of 1, 2, 3, 64, 65 and 257 entries, credits of 0, 1, 2, unlimited and
2^32 - 2, every cursor, every message count from 0 to the sum of the credits
+ 3 -- and the 64-bit arithmetic alone at a ring of 2^31 - 1 entries; the ring,
the credits and the working arrays lie in heap blocks of exactly their size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fwd_lb_credit_epochs_host(tmp_path):
    exe = str(tmp_path / "test_fwd_lb_credit")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++11", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "test_fwd_lb_credit.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fwd_lb_credit ok" in r.stdout
