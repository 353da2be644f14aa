"""The context's device-memory owner and growable array
(libzmq_amd/csrc/curve_devbuf.hpp: DevArena, DevBuf, grown_cap), compiled for
the host with AddressSanitizer (leak checking on) and UBSan as a stand-alone
program and run on a counting malloc allocator that fails the k-th allocation
on request.

The context's own group functions (ensure_workspace and the ZMTP groups,
curve_ctx.hpp) launch kernels and query hipCUB, so a HIP-free program cannot
reach them: the program's group is built from the same two types and the same
policy function, in the same shape -- one capacity that reads 0 while its
members are reserved, members of several element types and multipliers, a
fixed-size member, members reserved only under a condition (the sort
fallback's), one doubled from a floor and one sized exactly by the call.

Grow to 8, to 1025, back to 8; then, for every allocation k of the call that
grows 1024 -> 2048, that allocation fails: the call fails, the capacity reads 0
(for the two members reserved after the capacity group, as ws.temp and ws.rt
are, the group stands and the member itself reads {null, 0}), every member is
{null, 0} or an array of the arena's that covers its count -- the count of the
capacity it was last reserved for, the new one for those before the failure --
the arena holds exactly the non-null members, the retry succeeds at 2048 with
every member sized for it, the peak of live bytes stays within that of the same
sequence without a failure, and "free everything" leaves nothing."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_arena_host(tmp_path):
    exe = str(tmp_path / "test_devbuf")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++11", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "host", "test_devbuf.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "devbuf ok" in r.stdout
