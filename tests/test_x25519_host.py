"""The device X25519 arithmetic (libzmq_amd/csrc/curve_x25519.hpp) on the host,
under AddressSanitizer and UBSan: tests/host/test_x25519_host.cpp includes the
unmodified header with the HIP qualifiers defined away and calls k_scalarmult
and k_beforenm one "thread" at a time, a block of indices >= n included, on
outputs of exactly n items.  A GPU cannot report a wrapped int32_t or a store
one item past the end; this build does (signed-overflow checks stay on).

Vectors: the whole edge fixture (tests/golden/x25519_edge_vectors.json), the
existing x25519_vectors.json, and 2,000 seeded random pairs with the oracle's
outputs.  The run must be clean and every vector must match.

-std=c++20 because fe_carry shifts negative carries left (`h[0] -= c << 26`):
defined since C++20 (and what the device compiler does); under -std=c++17
UBSan reports "left shift of negative value" at the first line of fe_carry.

Sensitivity: mutants of a copy of the header (an exact-text replacement whose
target must occur once) are compiled and run the same way and must fail; each
also runs on the 200 random pairs of test_x25519.py's GPU test alone.  The
mutant of fe10_tobytes' quotient (q = h[9] >> 63) survives those 200 and is
killed by the steered out_* classes only."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_x25519_host.cpp")
HEADER = os.path.join(ROOT, "libzmq_amd", "csrc", "curve_x25519.hpp")
FLAGS = ["-O1", "-g", "-std=c++20", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-Wno-unknown-pragmas"]
E = json.load(open(os.path.join(ROOT, "tests", "golden", "x25519_edge_vectors.json")))["vectors"]
V = json.load(open(os.path.join(ROOT, "tests", "golden", "x25519_vectors.json")))

MUTANTS = {
    # (a) the canonical reduction's quotient from the top limb's sign alone
    "tobytes_q": ("""    int64_t q = (19 * h[9] + (1ll << 24)) >> 25;
#pragma unroll
    for (int i = 0; i < 10; ++i)
        q = (h[i] + q) >> ((i & 1) ? 25 : 26);
""", "    int64_t q = h[9] >> 63;\n"),
    # (b) the clamp without bit 254
    "clamp_bit254": ("    k[3] |= 1ull << 62;\n", ""),
    # (c) fe_carry without its last line (limb 0 left up to 19 carries wide)
    "carry_last": ("""    c = (h[9] + (1ll << 24)) >> 25; h[0] += c * 19; h[9] -= c << 25;
    c = (h[0] + (1ll << 25)) >> 26; h[1] += c; h[0] -= c << 26;
""", "    c = (h[9] + (1ll << 24)) >> 25; h[0] += c * 19; h[9] -= c << 25;\n"),
}


def line(scalar, point, rc, out, k=None):
    """k: None = k_scalarmult only, else (brc, key hex or None)."""
    s = f"{scalar} {point} {out} {rc}"
    return s if k is None else s + " " + (k[1] if k[0] == 0 else "-")


def edge_lines():
    return [line(v["scalar"], v["point"], v["rc"], v["out"], (v["brc"], v["k"])) for v in E]


def oracle_lines(pairs):
    out = []
    for sc, pt in pairs:
        rc, q = O.x25519(sc, pt)
        brc, k = O.box_beforenm(pt, sc)
        out.append(line(sc.hex(), pt.hex(), rc, q.hex(), (brc, k.hex() if k else None)))
    return out


def gpu_test_random_pairs():
    """The 200 random pairs of test_x25519.py::test_device_scalarmult_and_beforenm."""
    rng = np.random.default_rng(7)
    return [(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
            for _ in range(200)]


def build(tmp, header=None):
    exe = os.path.join(str(tmp), "test_x25519_host")
    cmd = ["g++"] + FLAGS + ["-o", exe, SRC]
    if header:
        cmd.insert(1, '-DX25519_HPP="%s"' % header)
    subprocess.check_call(cmd)
    return exe


def run(exe, tmp, name, lines):
    path = os.path.join(str(tmp), name)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return subprocess.run([exe, path], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("x25519_host"))


def test_device_x25519_on_the_host_is_clean(tmp_path, exe):
    lines = edge_lines()
    lines += [line(v["scalar"], v["point"], v["rc"], v["out"]) for v in V["scalarmult"]]
    lines += [line(v["sk"], v["pk"], v["rc"], "00" * 32 if v["rc"] else O.x25519(bytes.fromhex(v["sk"]),
                                                                                   bytes.fromhex(v["pk"]))[1].hex(),
                   (v["rc"], v["k"])) for v in V["beforenm"]]
    lines += [line(v["scalar"], "09" + "00" * 31, v["rc"], v["out"]) for v in V["base"]]
    rng = np.random.default_rng(0x25519)
    lines += oracle_lines([(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(),
                            rng.integers(0, 256, 32, dtype=np.uint8).tobytes()) for _ in range(2000)])
    assert len(lines) % 64 != 0  # the last block is a partial one, and one whole block lies past n
    r = run(exe, tmp_path, "all.txt", lines)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"x25519 host ok {len(lines)}" in r.stdout and "runtime error" not in r.stderr


def test_thread_past_n_writes_nothing(tmp_path, exe):
    """n = 1, 63, 64, 65: the launch covers n / 64 + 1 whole blocks, the arrays n items."""
    lines = edge_lines()
    for n in (1, 63, 64, 65):
        r = run(exe, tmp_path, f"n{n}.txt", lines[:n])
        assert r.returncode == 0 and f"x25519 host ok {n}" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_is_killed(tmp_path, name):
    old, new = MUTANTS[name]
    text = open(HEADER).read()
    assert text.count(old) == 1, name
    header = str(tmp_path / "curve_x25519.hpp")
    with open(header, "w") as f:
        f.write(text.replace(old, new))
    mutant = build(tmp_path, header)
    r = run(mutant, tmp_path, "edge.txt", edge_lines())
    assert r.returncode != 0, name + " survived the edge set"
    failed = sorted({int(x.split()[2].rstrip(":")) for x in r.stdout.splitlines() if x.startswith("scalarmult line")})
    killers = sorted({E[i - 1]["cls"] for i in failed})
    rr = run(mutant, tmp_path, "random200.txt", oracle_lines(gpu_test_random_pairs()))
    print(f"mutant {name}: edge set rc {r.returncode}, killed by {killers or r.stderr.strip().splitlines()[:1]}; "
          f"the GPU test's 200 random pairs: {'survives' if rr.returncode == 0 else 'killed'}")
    if name == "tobytes_q":
        assert rr.returncode == 0, rr.stdout + rr.stderr  # random outputs do not reach the reduction's edges
        assert any(k.startswith("out_") for k in killers) and all(k.startswith("out_") for k in killers)
