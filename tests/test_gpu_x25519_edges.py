"""zmqg_scalarmult_batch and zmqg_box_beforenm_batch at the field-arithmetic
edges (tests/x25519_steer.py): the whole of tests/golden/x25519_edge_vectors.json
-- outputs steered next to 0, p, every limb boundary of the ten-limb form and
2^254, inputs in [p, 2^255) and with saturated limbs, powers of two, the scalar
corners, small-order points with bit 255 set -- shuffled and interleaved with 64
random pairs so failing, steered and ordinary items share waves.  The expected
values are libsodium 1.0.18's (the fixture; the oracle for the random pairs).

Geometry: n = 1, 63, 64, 65, 129 with one sentinel item past n in the outputs
and the status, and the byte arrays passed at byte offset 1 of their allocations
(the kernels address bytes; status stays 4-byte aligned); n = 0 writes nothing."""
import functools
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

E = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "x25519_edge_vectors.json")))
H = bytes.fromhex
OUT_FILL, K_FILL, ST_FILL = 0xA5, 0x5A, 7


@functools.lru_cache(maxsize=None)
def mixed_set():
    """[(cls, scalar, point, rc, out, brc, k or None)]: the edge set and 64 random pairs, shuffled."""
    items = [(v["cls"], H(v["scalar"]), H(v["point"]), v["rc"], H(v["out"]), v["brc"], H(v["k"]) if v["k"] else None)
             for v in E["vectors"]]
    rng = np.random.default_rng(0xED6E)
    for _ in range(64):
        sc, pt = (rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(2))
        rc, out = O.x25519(sc, pt)
        brc, k = O.box_beforenm(pt, sc)
        items.append(("random", sc, pt, rc, out, brc, k))
    return tuple(items[i] for i in rng.permutation(len(items)))


def geometry_set(n):
    """n items of the mixed set: a steered near-p output first, a failing item last (the tail lane)."""
    m = mixed_set()
    items = list(m[:n])
    if n > 1:
        items[0] = next(x for x in m if x[0] == "out_nearp")
    items[-1] = next(x for x in m if x[3] != 0)
    return items


def _bytes_at(torch, data, offset):
    """A device byte tensor holding `data` at byte `offset` of its allocation."""
    buf = torch.zeros(offset + len(data), dtype=torch.uint8, device="cuda")
    buf[offset:] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to("cuda")
    return buf[offset:]


def _call(torch, ctx, which, items, offset=0):
    """Runs one kernel over `items` with one sentinel item past n in the output
    and the status (and `offset` bytes before the output), checks the sentinels
    and returns (status[n], output bytes)."""
    n = len(items)
    fill = OUT_FILL if which != "beforenm" else K_FILL
    out = torch.full((offset + 32 * (n + 1),), fill, dtype=torch.uint8, device="cuda")
    st = torch.full((n + 1,), ST_FILL, dtype=torch.int32, device="cuda")
    sc = _bytes_at(torch, b"".join(x[1] for x in items), offset)
    pt = _bytes_at(torch, b"".join(x[2] for x in items), offset)
    o = out[offset:offset + 32 * n]
    if which == "scalarmult":
        ctx.scalarmult_batch(sc, pt, o, st[:n])
    elif which == "base":
        ctx.scalarmult_batch(sc, None, o, st[:n])
    else:
        ctx.box_beforenm_batch(pt, sc, o, st[:n])
    torch.cuda.synchronize()
    ob, s = out.cpu().numpy().tobytes(), st.cpu().numpy()
    assert ob[:offset] == bytes([fill]) * offset and ob[offset + 32 * n:] == bytes([fill]) * 32, "output sentinel"
    assert s[n] == ST_FILL, "status sentinel"
    return s[:n], ob[offset:offset + 32 * n]


def _check(which, items, s, o):
    for i, (cls, _, _, rc, out, brc, k) in enumerate(items):
        if which == "scalarmult":
            assert s[i] == rc and o[32 * i:32 * i + 32] == out, (i, cls)
        else:
            assert s[i] == brc, (i, cls)
            assert o[32 * i:32 * i + 32] == (k if brc == 0 else bytes([K_FILL]) * 32), (i, cls)


def test_scalarmult_edge_set(torch_cuda, C):
    items = mixed_set()
    s, o = _call(torch_cuda, C.CurveContext(0, 1), "scalarmult", items)
    _check("scalarmult", items, s, o)
    assert int((s != 0).sum()) == sum(v["rc"] != 0 for v in E["vectors"]) == 7


def test_beforenm_edge_set(torch_cuda, C):
    items = mixed_set()
    s, o = _call(torch_cuda, C.CurveContext(0, 1), "beforenm", items)
    _check("beforenm", items, s, o)
    # the small-order points with bit 255 set and nothing else (u = 2^0 is not in in_bits)
    fails = sum(v["brc"] != 0 for v in E["vectors"])
    assert fails == sum(v["cls"] == "in_small_order_hi" for v in E["vectors"]) == 7
    assert int((s != 0).sum()) == fails and int((s == -1).sum()) == fails


def test_base_point_scalar_class(torch_cuda, C):
    vs = [v for v in E["vectors"] if v["cls"] == "scalar"]
    items = [("scalar", H(v["scalar"]), bytes(32)) for v in vs]
    s, o = _call(torch_cuda, C.CurveContext(0, 1), "base", items)
    assert (s == 0).all()
    assert [o[32 * i:32 * i + 32].hex() for i in range(len(vs))] == [v["base"] for v in vs]


@pytest.mark.parametrize("which", ["scalarmult", "beforenm"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_geometry(torch_cuda, C, which, n):
    ctx = C.CurveContext(0, 1)
    items = geometry_set(n)
    s0, o0 = _call(torch_cuda, ctx, which, items)
    _check(which, items, s0, o0)
    s1, o1 = _call(torch_cuda, ctx, which, items, offset=1)
    assert (s1 == s0).all() and o1 == o0
    assert s0[n - 1] == -1


def test_n_zero_writes_nothing(torch_cuda, C):
    torch = torch_cuda
    ctx = C.CurveContext(0, 1)
    out = torch.full((64,), OUT_FILL, dtype=torch.uint8, device="cuda")
    st = torch.full((2,), ST_FILL, dtype=torch.int32, device="cuda")
    inp = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ctx.scalarmult_batch(inp[:0], inp[:0], out[:0], st[:0])
    ctx.scalarmult_batch(inp[:0], None, out[:0], st[:0])
    ctx.box_beforenm_batch(inp[:0], inp[:0], out[:0], st[:0])
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == OUT_FILL).all() and (st.cpu().numpy() == ST_FILL).all()
