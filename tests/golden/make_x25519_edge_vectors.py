#!/usr/bin/env python3
"""Generates tests/golden/x25519_edge_vectors.json (run in the build container,
not on the GPU box): libsodium 1.0.18's answers -- the library of
make_x25519_vectors.py, loaded with ctypes from the image's conda environment --
for every vector of tests/x25519_steer.py's edge_vectors(): outputs steered next
to 0, p and the limb boundaries of the device arithmetic, non-canonical and
saturated inputs, powers of two, and the scalar corners.  Per vector: cls,
scalar, point, rc / out of crypto_scalarmult_curve25519, brc / k of
crypto_box_beforenm(k, point, scalar), and for the scalar class base =
crypto_scalarmult_curve25519_base(scalar).  One vector per line, to stay below
the largest fixture committed."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import x25519_steer as S  # noqa: E402

L = ctypes.CDLL("/opt/conda/lib/libsodium.so.23")
assert L.sodium_init() >= 0
L.sodium_version_string.restype = ctypes.c_char_p


def scalarmult(n, p):
    q = ctypes.create_string_buffer(32)
    rc = L.crypto_scalarmult_curve25519(q, bytes(n), bytes(p))
    return rc, q.raw


def scalarmult_base(n):
    q = ctypes.create_string_buffer(32)
    rc = L.crypto_scalarmult_curve25519_base(q, bytes(n))
    return rc, q.raw


def beforenm(pk, sk):
    k = ctypes.create_string_buffer(b"\xaa" * 32, 32)
    rc = L.crypto_box_beforenm(k, bytes(pk), bytes(sk))
    return rc, k.raw


vectors, window = S.edge_vectors()
rows = []
for cls, sc, pt in vectors:
    rc, q = scalarmult(sc, pt)
    brc, k = beforenm(pt, sc)
    row = {"cls": cls, "scalar": sc.hex(), "point": pt.hex(), "rc": rc, "out": q.hex(), "brc": brc,
           "k": k.hex() if brc == 0 else None}
    if cls == "scalar":
        rc, q = scalarmult_base(sc)
        assert rc == 0
        row["base"] = q.hex()
    rows.append(row)
head = {"source": "libsodium " + L.sodium_version_string().decode() + " (ctypes, build container); inputs: "
                  "tests/x25519_steer.py edge_vectors()",
        "libsodium": L.sodium_version_string().decode(), "window": window}
out = os.path.join(HERE, "x25519_edge_vectors.json")
with open(out, "w") as f:
    f.write(json.dumps(head)[:-1] + ', "vectors": [\n')
    f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
    f.write("\n]}\n")
json.load(open(out))
size, limit = os.path.getsize(out), os.path.getsize(os.path.join(HERE, "curve_golden.json"))
assert size <= limit, (size, limit)
print("wrote", out, len(rows), "vectors,", size, "bytes")
