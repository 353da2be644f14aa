"""X25519 at its field-arithmetic edges, on the CPU: the steered and extreme
vectors of tests/x25519_steer.py (outputs next to 0, p, the limb boundaries of
the device's ten-limb form and 2^254; inputs in [p, 2^255), saturated limbs,
powers of two, the scalar corners) with libsodium 1.0.18's answers in
tests/golden/x25519_edge_vectors.json.  Three opinions must agree on every
vector: Python integers (x25519_steer.x25519_int), libsodium (the fixture) and
the oracle (oracle/keys_oracle.c, radix 2^51, whose fe51_tobytes and
non-canonical inputs nothing else pins).  The fixture's inputs are the
builder's, so it cannot drift from the classes, and what each class claims is
asserted from the fixture's outputs."""
import collections
import json
import os

from oracle import oracle as O
from tests import x25519_steer as S

HERE = os.path.dirname(os.path.abspath(__file__))
F = json.load(open(os.path.join(HERE, "golden", "x25519_edge_vectors.json")))
V = F["vectors"]
H = bytes.fromhex
CLASSES = S.STEERED + ("in_noncanon", "in_small_order_hi", "in_limbs", "in_bits", "scalar")


def of(cls):
    return [v for v in V if v["cls"] == cls]


def test_fixture_is_the_builders_set():
    vec, window = S.edge_vectors()
    assert [(v["cls"], v["scalar"], v["point"]) for v in V] == [(c, s.hex(), p.hex()) for c, s, p in vec]
    assert F["window"] == window and F["libsodium"] == "1.0.18"
    count = collections.Counter(v["cls"] for v in V)
    print(dict(count))
    assert set(count) == set(CLASSES)
    assert os.path.getsize(os.path.join(HERE, "golden", "x25519_edge_vectors.json")) <= \
        os.path.getsize(os.path.join(HERE, "golden", "curve_golden.json"))


def test_integers_libsodium_and_oracle_agree():
    for i, v in enumerate(V):
        sc, pt = H(v["scalar"]), H(v["point"])
        assert S.x25519_int(sc, pt) == (v["rc"], H(v["out"])), (i, v["cls"])
        assert O.x25519(sc, pt) == (v["rc"], H(v["out"])), (i, v["cls"])
        assert v["brc"] == v["rc"] and (v["k"] is None) == (v["brc"] != 0)
        rc, k = O.box_beforenm(pt, sc)
        assert rc == v["brc"] and (k.hex() if k else None) == v["k"], (i, v["cls"])
        if v["brc"] == 0:  # crypto_box_beforenm = HSalsa20(shared point, 0^16)
            assert O.hsalsa20(bytes(16), H(v["out"])).hex() == v["k"]
        if v["cls"] == "scalar":
            nine = S.enc(9)
            assert S.x25519_int(sc, nine) == (0, H(v["base"])) and O.x25519(sc, nine) == (0, H(v["base"]))


def test_steered_outputs_lie_in_their_windows():
    for cls in S.STEERED:
        assert of(cls)
        for v in of(cls):
            assert v["rc"] == 0 and S.in_window(cls, S.le(H(v["out"])), F["window"]), v
    assert {S.le(H(v["out"])) for v in of("out_small")} == {x for x in range(2, 19) if S.reachable(x)}
    assert {S.P - S.le(H(v["out"])) for v in of("out_nearp")} == {d for d in range(2, 20) if S.reachable(S.P - d)}
    for b in S.EDGE_BITS:  # every limb offset and half-limb point, on both sides
        assert any(abs(S.le(H(v["out"])) - (1 << b)) <= F["window"] for v in of("out_limb+")), b
        assert any(abs(S.P - S.le(H(v["out"])) - (1 << b)) <= F["window"] for v in of("out_limb-")), b
    # each target under a random scalar, 32 x 00 and 32 x ff
    for cls in S.STEERED:
        by_out = collections.defaultdict(set)
        for v in of(cls):
            by_out[v["out"]].add(v["scalar"])
        for scalars in by_out.values():
            assert len(scalars) == 3 and {"00" * 32, "ff" * 32} < scalars


def test_input_class_properties():
    for v in of("in_noncanon"):  # p + k computes what k does
        u = S.le(H(v["point"])) & S.M255
        assert S.P + 2 <= u <= S.P + 18
        assert (v["rc"], H(v["out"])) == S.x25519_int(H(v["scalar"]), S.enc(u - S.P)) == \
            O.x25519(H(v["scalar"]), S.enc(u - S.P))
        assert v["rc"] == 0
    assert sorted(S.le(H(v["point"])) for v in of("in_noncanon")) == \
        sorted(S.P + k | hi for k in range(2, 19) for hi in (0, 1 << 255))
    assert [H(v["point"]) for v in of("in_small_order_hi")] == \
        [S.enc(S.le(s) | 1 << 255) for s in S.small_order_points()]
    for v in of("in_small_order_hi"):
        assert v["rc"] == -1 and v["out"] == "00" * 32 and v["brc"] == -1 and v["k"] is None
    assert sum(v["rc"] != 0 for v in V) == 7
    pts = {v["point"] for v in of("in_limbs")}
    assert {S.enc(S.M255).hex(), "ff" * 32} <= pts
    for i in range(10):
        assert {S.enc(S.limb_ones(i)).hex(), S.enc(S.M255 ^ S.limb_ones(i)).hex()} <= pts
    js = {S.le(H(v["point"])).bit_length() - 1 for v in of("in_bits")}
    assert all(S.le(H(v["point"])) == 1 << (S.le(H(v["point"])).bit_length() - 1) for v in of("in_bits"))
    for i in range(10):  # thinned, but every limb keeps its first and last bit
        assert {S.LIMB_BIT[i], S.LIMB_BIT[i] + S.LIMB_WIDTH[i] - 1} - {0} <= js


def test_bit_255_never_changes_a_result():
    for i, v in enumerate(V):
        sc, pt = H(v["scalar"]), H(v["point"])
        flipped = S.enc(S.le(pt) ^ 1 << 255)
        assert O.x25519(sc, flipped) == (v["rc"], H(v["out"])), (i, v["cls"])
        assert S.x25519_int(sc, flipped) == (v["rc"], H(v["out"])), (i, v["cls"])
    pairs = collections.defaultdict(set)  # and libsodium says so where the fixture holds both
    for v in of("in_noncanon"):
        pairs[S.le(H(v["point"])) & S.M255].add((v["scalar"], v["rc"], v["out"], v["k"]))
    assert len(pairs) == 17 and all(len(x) == 1 for x in pairs.values())
    assert sum(S.le(H(v["point"])) >> 255 for v in of("in_noncanon")) == 17


def test_a_scalar_and_its_clamped_form_agree():
    sc = of("scalar")
    assert len(sc) == 24
    by_scalar = collections.defaultdict(list)
    for v in sc:
        by_scalar[v["scalar"]].append(v)
    assert len(by_scalar) == 8 and all(len(x) == 3 for x in by_scalar.values())
    clamped_pairs = 0
    for s, vs in by_scalar.items():
        c = S.clamped_bytes(H(s)).hex()
        if c != s and c in by_scalar:
            clamped_pairs += 1
            assert [(v["point"], v["rc"], v["out"], v["k"], v["base"]) for v in vs] == \
                [(v["point"], v["rc"], v["out"], v["k"], v["base"]) for v in by_scalar[c]]
        for v in vs:  # whether its clamped form is in the set or not: the other two opinions
            assert O.x25519(H(c), H(v["point"])) == (v["rc"], H(v["out"]))
            assert S.x25519_int(H(c), H(v["point"])) == (v["rc"], H(v["out"]))
    assert clamped_pairs >= 1
    assert {v["point"] for v in sc} >= {S.enc(9).hex(), S.enc(S.M255).hex()}
