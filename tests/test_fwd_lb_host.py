"""The choice arithmetic of zmqg_forward_zmtp_lb_multi's kernels (fwd_lb_range,
fwd_lb_cur0, fwd_lb_at and fwd_lb_pick, libzmq_amd/csrc/curve_fwd_lb.hpp),
compiled for the host with AddressSanitizer and UBSan as a stand-alone program
and run: clamped and falling grp_idx, A = 0 and A = 1, cursors of 0, A - 1, A and
2^32 - 1, message counts up to 2^31 - 1 added to a cursor near 2^31 (a 32-bit
wrap would show), and a sweep of several calls on one table against the
sequential lb_t loop (src/lb.cpp:56-131 with every write succeeding); grp_idx,
lb_dst and lb_cur lie in heap blocks of exactly their size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fwd_lb_choice_host(tmp_path):
    exe = str(tmp_path / "test_fwd_lb")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++11", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "test_fwd_lb.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fwd_lb ok" in r.stdout
