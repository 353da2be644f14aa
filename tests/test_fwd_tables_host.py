"""The forward calls' table of host arrays (fwd_table_dims and fwd_table_fill,
libzmq_amd/csrc/curve_fwd_common.hpp), compiled for the host with
AddressSanitizer and UBSan as a stand-alone program and run: the pair bases
against the models' pair_base formulas restated there, the element bases over
the routed streams only, the load balancer's group lists (every grouped stream
once, rising within its group), for one stream, a stream without routes in the
middle, the id slots of PREPEND, one route slot a stream, no group, an empty
group and a stream without one, and 65 streams; the rejections (falling or
non-zero-based index arrays, a route at n_dst, a stream's pairs and the sum of
all pairs just past check_n's limit, and that limit itself accepted).  The
inputs and the word buffer lie in heap blocks of exactly their size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fwd_tables_host(tmp_path):
    exe = str(tmp_path / "test_fwd_tables")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++11", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "test_fwd_tables.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fwd_tables ok" in r.stdout
