"""Steering X25519 to its field-arithmetic edges (test infrastructure, not a conftest).

The device X25519 (libzmq_amd/csrc/curve_x25519.hpp) works in GF(p), p = 2^255 -
19, in ten signed limbs of 26 / 25 bits.  Where such code goes wrong -- the
canonical reduction of fe10_tobytes, values next to 0, p and a limb boundary,
inputs in [p, 2^255) -- a random key pair lands with probability ~2^-25 or less.
The output can be chosen, though: for a clamped scalar k and a target x that is
the u-coordinate of a point of prime order l on the curve (or l' on the twist),

    P = (k^-1 mod order) * x        gives        X25519(k, P) = x,

P computed by an unclamped Montgomery ladder in Python integers.  Not every x is
reachable: x must lie in the prime-order subgroup of the curve or of its twist
(about one value in four); reachable() decides by multiplying by l and by l'.

x25519_int is the high-precision reference (RFC 7748 section 5 in Python
integers, the inverse by pow, libsodium's return code: an all-zero result is
-1).  edge_vectors() is the seeded builder of the labelled set
tests/golden/x25519_edge_vectors.json holds libsodium's answers for."""
import functools
import json
import os
import random

P = (1 << 255) - 19
A24 = 121665
L = (1 << 252) + 27742317777372353535851937790883648493  # curve order = 8 l
LT = (2 * P + 2 - 8 * L) // 4  # twist order = 4 l'
assert 8 * L + 4 * LT == 2 * P + 2
M255 = (1 << 255) - 1
WINDOW = 16  # |d| of the steered 2^b + d; edge_vectors() widens it when a pair would be empty
PER_EDGE = 3
SEED = 0x25519ED6E

# the device limbs: limb i at bit ceil(25.5 i), 26 bits wide when i is even, else 25
LIMB_BIT = [(51 * i + 1) // 2 for i in range(10)]
LIMB_WIDTH = [25 if i & 1 else 26 for i in range(10)]
EDGE_BITS = sorted(LIMB_BIT[1:] + [b - 1 for b in LIMB_BIT[1:]])  # limb offsets and the half-limb points
STEERED = ("out_small", "out_nearp", "out_limb+", "out_limb-", "out_mid")

_HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def small_order_points():
    """The 7 points of tests/golden/x25519_vectors.json libsodium rejects."""
    v = json.load(open(os.path.join(_HERE, "golden", "x25519_vectors.json")))
    pts = [bytes.fromhex(x["point"]) for x in v["scalarmult"] if x["rc"] != 0]
    assert len(pts) == 7
    return tuple(pts)


def le(b):
    return int.from_bytes(bytes(b), "little")


def enc(x):
    return int(x).to_bytes(32, "little")


def clamp(scalar):
    """RFC 7748 decodeScalar25519, as an integer."""
    return (le(scalar) & ~7 & ~(1 << 255)) | (1 << 254)


def clamped_bytes(scalar):
    return enc(clamp(scalar))


def ladder(k, u, bits=None):
    """(X, Z) of k * (u : 1) on the Montgomery curve (the RFC 7748 ladder, any
    integer k >= 0, no clamping); u is taken mod p."""
    x1 = u % P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in reversed(range(bits or max(k.bit_length(), 1))):
        kt = (k >> t) & 1
        if swap ^ kt:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b = (x2 + z2) % P, (x2 - z2) % P
        aa, bb = a * a % P, b * b % P
        e = (aa - bb) % P
        da, cb = (x3 - z3) * a % P, (x3 + z3) * b % P
        x3 = (da + cb) ** 2 % P
        z3 = x1 * (da - cb) ** 2 % P
        x2 = aa * bb % P
        z2 = e * (aa + A24 * e) % P
    if swap:
        x2, x3, z2, z3 = x3, x2, z3, z2
    return x2, z2


def x25519_int(scalar, point):
    """crypto_scalarmult_curve25519 in Python integers: (rc, 32 bytes)."""
    x, z = ladder(clamp(scalar), le(point) & M255, 255)
    out = x * pow(z, P - 2, P) % P
    return (0 if out else -1), enc(out)


@functools.lru_cache(maxsize=None)
def reachable(x):
    """"curve" / "twist" when x is the u-coordinate of a point of prime order
    l on the curve / l' on the twist (so some point maps to it under every
    clamped scalar), else None."""
    if not 1 < x < P - 1:
        return None
    if ladder(L, x)[1] == 0:
        return "curve"
    if ladder(LT, x)[1] == 0:
        return "twist"
    return None


def steer(scalar, x):
    """The 32-byte point P with X25519(scalar, P) = x; x must be reachable."""
    order = {"curve": L, "twist": LT}[reachable(x)]
    X, Z = ladder(pow(clamp(scalar) % order, -1, order), x)
    assert Z != 0
    return enc(X * pow(Z, P - 2, P) % P)


def limb_ones(i):
    return ((1 << LIMB_WIDTH[i]) - 1) << LIMB_BIT[i]


def in_window(cls, x, window=WINDOW):
    """Whether the output x lies where the steered class `cls` claims."""
    if cls == "out_small":
        return 2 <= x < 19
    if cls == "out_nearp":
        return 2 <= P - x < 20
    if cls == "out_limb+":
        return any(abs(x - (1 << b)) <= window for b in EDGE_BITS)
    if cls == "out_limb-":
        return any(abs(P - x - (1 << b)) <= window for b in EDGE_BITS)
    if cls == "out_mid":
        return abs(x - (1 << 254)) <= window
    raise ValueError(cls)


def _nearest(base, sign, count, window):
    """Up to `count` reachable sign * (base + d) mod p, smallest |d| first."""
    out = []
    for a in range(window + 1):
        for d in ((0,) if a == 0 else (a, -a)):
            x = (base + d) % P if sign > 0 else (P - (base + d)) % P
            if reachable(x) and len(out) < count:
                out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def edge_vectors():
    """(vectors, window): the labelled set [(cls, scalar, point)], the same on
    every call and every machine, and the |d| window the limb classes needed."""
    rng = random.Random(SEED)
    rb = lambda: bytes(rng.randrange(256) for _ in range(32))  # noqa: E731
    vec = []
    window = WINDOW
    targets = [("out_small", x) for x in range(2, 19) if reachable(x)]
    targets += [("out_nearp", P - d) for d in range(2, 20) if reachable(P - d)]
    assert any(c == "out_small" for c, _ in targets) and any(c == "out_nearp" for c, _ in targets)
    for b in EDGE_BITS:
        for cls, sign in (("out_limb+", 1), ("out_limb-", -1)):
            w = WINDOW
            while not (xs := _nearest(1 << b, sign, PER_EDGE, w)):
                w *= 2  # never skip a (b, sign) pair
            window = max(window, w)
            targets += [(cls, x) for x in xs]
    mid = _nearest(1 << 254, 1, 6, WINDOW)
    assert mid
    targets += [("out_mid", x) for x in mid]
    so = {le(s) % P for s in small_order_points()}
    for cls, x in targets:
        for sc in (rb(), bytes(32), b"\xff" * 32):
            pt = steer(sc, x)
            assert le(pt) % P not in so
            vec.append((cls, sc, pt))
    for b in EDGE_BITS:  # every (b, sign) pair has a vector
        assert any(c == "out_limb+" and abs(x - (1 << b)) <= window for c, x in targets), b
        assert any(c == "out_limb-" and abs(P - x - (1 << b)) <= window for c, x in targets), b

    for k in range(2, 19):
        sc = rb()  # one scalar for both, so the fixture shows libsodium ignoring bit 255
        for hi in (0, 1 << 255):
            vec.append(("in_noncanon", sc, enc(P + k | hi)))
    for s in small_order_points():
        vec.append(("in_small_order_hi", rb(), enc(le(s) | 1 << 255)))
    even = sum(limb_ones(i) for i in range(0, 10, 2))
    limbs = [M255, (1 << 256) - 1]
    for i in range(10):
        limbs += [limb_ones(i), M255 ^ limb_ones(i)]
    limbs += [even, M255 ^ even]
    vec += [("in_limbs", rb(), enc(u)) for u in limbs]
    # u = 2^j: every limb's first two, middle and last two bits (all of j = 1 .. 254
    # would put the fixture past the largest one committed)
    js = sorted({j for i in range(10) for lo, hi in [(LIMB_BIT[i], LIMB_BIT[i] + LIMB_WIDTH[i] - 1)]
                 for j in (lo, lo + 1, (lo + hi) // 2, hi - 1, hi)} - {0})
    vec += [("in_bits", rb(), enc(1 << j)) for j in js]
    r = rb()
    scalars = [bytes(32), b"\xff" * 32, b"\x07" + bytes(31), bytes(31) + b"\x80", bytes(31) + b"\x40",
               b"\xff" * 31 + b"\x3f", r, clamped_bytes(r)]
    assert r != clamped_bytes(r)
    ru = rb()
    for sc in scalars:
        for u in (enc(9), ru, enc(M255)):
            vec.append(("scalar", sc, u))
    return tuple(vec), window
