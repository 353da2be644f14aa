"""An integer model of the radix-2^32 Poly1305 block of
libzmq_amd/csrc/curve_device.hpp (poly32_add, poly32_mul_add, poly32_block,
poly32_window_full), limb by limb in the order of the source, with every
intermediate held to the bound written beside it there:

* the four 64-bit sums of word products d0..d3, and d3 >> 32 <= 2^30;
* g = a4 r0 + (d3 >> 32) < 2^31 + 2^30 + 1 (a 32-bit word on the device);
* d0 after the early fold of 5 (g >> 2), e0, t1, t2, t3 (64-bit, no wrap);
* the carry out of word 3, (t3 >> 32) - (d3 >> 32) <= 2 (<= 1 without a next
  block), and the fifth word on return: <= 6 with the next block added, <= 4
  without;
* a4 <= 8 wherever a block starts.

Run over the extreme keys of tests/poly_steer.py (largest and smallest words
and limbs of r) and the clamp's own corners, the accumulators 0, p - 1,
2^130 - 1 and the largest partially reduced input (h0..h3 all ones, h4 = 6),
and all-0xff / all-zero blocks; the result must equal big-integer Poly1305
(poly_steer.poly1305_int) -- block by block as (h + m) r mod p, and for whole
messages walked in windows as the frame kernels walk them."""
import itertools

import numpy as np
import pytest

from tests import poly_steer as S

M32 = (1 << 32) - 1
P = S.P


class Bound(AssertionError):
    pass


def _lt(x, bound, what):
    if not 0 <= x < bound:
        raise Bound(f"{what} = {x:#x} is not below {bound:#x}")
    return x


def mad64(a, b, c, what):
    """v_mad_u64_u32: 32-bit a, b, 64-bit c; the sum must not wrap."""
    _lt(a, 1 << 32, what + " a")
    _lt(b, 1 << 32, what + " b")
    return _lt(a * b + c, 1 << 64, what)


def key32_words(key32):
    """PolyKey32 of curve_device.hpp poly32_key."""
    k = [int.from_bytes(key32[4 * i:4 * i + 4], "little") for i in range(4)]
    r = [k[0] & 0x0fffffff, k[1] & 0x0ffffffc, k[2] & 0x0ffffffc, k[3] & 0x0ffffffc]
    s = [0] + [x + (x >> 2) for x in r[1:]]
    for x in r:
        _lt(x, 1 << 28, "r word")
    for x in s[1:]:
        _lt(x, 5 << 26, "s word")
    return r, s


def r_int(r):
    return r[0] | (r[1] << 32) | (r[2] << 64) | (r[3] << 96)


def value(h):
    return sum(x << (32 * i) for i, x in enumerate(h))


def poly32_add(h, m, hib):
    _lt(h[4], 7, "h4 on entry")
    a, c = [], 0
    for i in range(4):
        t = h[i] + m[i] + c
        a.append(t & M32)
        c = t >> 32
    a.append(_lt(h[4] + hib + c, 9, "a4"))
    assert value(a) == value(h) + value(m) + (hib << 128)
    return a


def poly32_mul_add(a, r, s, nxt=None, nhib=0):
    """a r (+ the next block) as the device computes it; nxt: four words or None."""
    for i in range(4):
        _lt(a[i], 1 << 32, "a word")
    _lt(a[4], 9, "a4")
    r0, r1, r2, r3 = r
    _, s1, s2, s3 = s
    d0 = mad64(a[3], s1, mad64(a[2], s2, mad64(a[1], s3, a[0] * r0, "d0"), "d0"), "d0")
    d1 = mad64(a[4], s1, mad64(a[3], s2, mad64(a[2], s3, mad64(a[1], r0, a[0] * r1, "d1"), "d1"), "d1"), "d1")
    d2 = mad64(a[4], s2, mad64(a[3], s3, mad64(a[2], r0, mad64(a[1], r1, a[0] * r2, "d2"), "d2"), "d2"), "d2")
    d3 = mad64(a[4], s3, mad64(a[3], r0, mad64(a[2], r1, mad64(a[1], r2, a[0] * r3, "d3"), "d3"), "d3"), "d3")
    _lt(d0, 19 << 58, "d0")
    _lt(d1, (18 << 58) + (5 << 29), "d1")
    _lt(d2, (17 << 58) + (5 << 29), "d2")
    _lt(d3, (16 << 58) + (5 << 29), "d3")
    d3h = _lt(d3 >> 32, (1 << 30) + 1, "d3 >> 32")
    g = _lt(a[4] * r0 + d3h, (1 << 31) + (1 << 30) + 1, "g")
    d0 = _lt(mad64(g >> 2, 5, d0, "d0 fold"), (19 << 58) + (1 << 32), "d0 after the fold")
    w = ((g & 3) - d3h) & M32
    n = nxt if nxt is not None else [0, 0, 0, 0]
    if nxt is not None:
        d0 = mad64(n[0], 1, d0, "e0")
    _lt(d0, (19 << 58) + (1 << 33), "e0")
    t1 = mad64(d0 >> 32, 1, d1, "t1")
    if nxt is not None:
        t1 = mad64(n[1], 1, t1, "t1")
    _lt(t1, 1 << 63, "t1")
    t2 = mad64(t1 >> 32, 1, d2, "t2")
    if nxt is not None:
        t2 = mad64(n[2], 1, t2, "t2")
    _lt(t2, 1 << 63, "t2")
    t3 = mad64(t2 >> 32, 1, d3, "t3")
    if nxt is not None:
        t3 = mad64(n[3], 1, t3, "t3")
    _lt((t3 >> 32) - d3h, 3 if nxt is not None else 2, "carry out of word 3")
    o4 = ((t3 >> 32) + w + (nhib if nxt is not None else 0)) & M32
    _lt(o4, 7 if nxt is not None else 5, "h4 on return")
    o = [d0 & M32, t1 & M32, t2 & M32, t3 & M32, o4]
    want = value(a) * r_int(r) + (value(n) + (nhib << 128) if nxt is not None else 0)
    assert value(o) % P == want % P
    return o


def poly32_block(h, m, hib, r, s):
    return poly32_mul_add(poly32_add(h, m, hib), r, s)


def poly32_window_full(h, r, s, c, from2=False):
    if from2:
        a = poly32_add(h, c[8:12], 1)
    else:
        a = poly32_add(h, c[0:4], 1)
        a = poly32_mul_add(a, r, s, c[4:8], 1)
        a = poly32_mul_add(a, r, s, c[8:12], 1)
    a = poly32_mul_add(a, r, s, c[12:16], 1)
    return poly32_mul_add(a, r, s)


def poly32_finish(h, key32):
    _lt(h[4], 5, "h4 at the finish")
    v = value(h)
    assert v < 2 * P
    v = v - P if v >= P else v
    return ((v + int.from_bytes(key32[16:32], "little")) & S.M128).to_bytes(16, "little")


def words(b):
    return [int.from_bytes(b[4 * i:4 * i + 4], "little") for i in range(len(b) // 4)]


def corner_keys():
    """The clamp's corners: every word of r at its largest or smallest value
    (0 and the largest multiple of 4 below 2^28), all 16 combinations."""
    out = []
    for pick in itertools.product((0, 1), repeat=4):
        w = [(0x0fffffff if i == 0 else 0x0ffffffc) if p else 0 for i, p in enumerate(pick)]
        out.append(b"".join(x.to_bytes(4, "little") for x in w) + bytes(range(16)))
    return out


@pytest.fixture(scope="module")
def keys():
    ks = [S.message_stream(n, 32) for n in S.extreme_nonces()]
    return ks + corner_keys()


def split(v):
    return [(v >> (32 * i)) & M32 for i in range(4)] + [v >> 128]


ACCS = [("0", split(0)), ("p-1", split(P - 1)), ("2^130-1", split((1 << 130) - 1)),
        ("largest", [M32, M32, M32, M32, 6])]
BLOCKS = [("ff", [M32] * 4), ("00", [0] * 4)]


def test_block_bounds_and_value(keys):
    n = 0
    for key32 in keys:
        r, s = key32_words(key32)
        for (an, h), (bn, m), hib in itertools.product(ACCS, BLOCKS, (0, 1)):
            o = poly32_block(h, m, hib, r, s)
            assert value(o) % P == (value(h) + value(m) + (hib << 128)) * r_int(r) % P, (an, bn, hib)
            assert o[4] <= 4
            # the same block as the first of a run, the next block added on the way
            for (nn, nx), nhib in itertools.product(BLOCKS, (0, 1)):
                o2 = poly32_mul_add(poly32_add(h, m, hib), r, s, nx, nhib)
                assert o2[4] <= 6, (an, bn, nn)
                # and the block after it, from the largest fifth word a run can hand on
                poly32_mul_add(o2, r, s, nx, nhib)
                poly32_mul_add(o2, r, s)
            n += 1
    assert n >= 16 * len(ACCS) * len(BLOCKS) * 2


def test_window_runs(keys):
    """Four-block and two-block windows from every accumulator, against (h + m) r block by block."""
    for key32 in keys:
        r, s = key32_words(key32)
        R = r_int(r)
        for (_, h), (_, m) in itertools.product(ACCS, BLOCKS):
            c = m * 4
            for from2 in (False, True):
                o = poly32_window_full(h, r, s, c, from2)
                v = value(h)
                for _ in range(2 if from2 else 4):
                    v = (v + value(m) + (1 << 128)) * R % P
                assert value(o) % P == v
                assert o[4] <= 4
                # the form poly32_window takes for the same blocks: one poly32_block each
                g = h
                for j in range(2 if from2 else 0, 4):
                    g = poly32_block(g, c[4 * j:4 * j + 4], 1, r, s)
                assert value(g) % P == v


def mac_in_windows(ct, key32):
    """The frame kernels' walk: window 0 holds ciphertext bytes 0..31 in block
    slots 2 and 3, window w > 0 bytes 64 w - 32 ..; whole windows through
    poly32_window_full, the rest block by block with the 0x01 pad."""
    r, s = key32_words(key32)
    h = [0, 0, 0, 0, 0]
    pos, first = 0, True
    while pos < len(ct):
        room = 32 if first else 64
        piece = ct[pos:pos + room]
        if len(piece) == room:
            c = words((bytes(32) if first else b"") + piece)
            h = poly32_window_full(h, r, s, c, from2=first)
        else:
            for i in range(0, len(piece), 16):
                b = piece[i:i + 16]
                if len(b) == 16:
                    h = poly32_block(h, words(b), 1, r, s)
                else:
                    h = poly32_block(h, words(b + b"\x01" + bytes(15 - len(b))), 0, r, s)
        pos += room
        first = False
    return poly32_finish(h, key32), value(h) % P


@pytest.mark.parametrize("length", [1, 16, 31, 32, 33, 96, 97, 160, 1057 - 32, 224])
def test_messages_against_big_integers(keys, length):
    rng = np.random.default_rng(20261020 + length)
    for key32 in keys:
        for ct in (bytes([0xff]) * length, bytes(length), rng.integers(0, 256, length, dtype=np.uint8).tobytes()):
            tag, h = mac_in_windows(ct, key32)
            want_tag, want_h = S.poly1305_int(ct, key32)
            assert h == want_h
            assert tag == want_tag


def test_steered_accumulators(keys):
    """Messages solved so that the accumulator before the freeze sits on the
    targets of poly_steer (0, p - 1, 2^128, -s, ...): the finish's conditional
    subtraction and the carries of h + s, through the model's windows."""
    rng = np.random.default_rng(20261021)
    done = 0
    for key32 in keys[:6]:
        if S.key_rs(key32)[0] == 0:
            continue
        for name, T in S.targets(key32):
            for length in (32, 96, 161):
                try:
                    ct, _ = S.steer(key32, length, (length // 16) // 2, T, rng)
                except S.SteerError:
                    continue
                tag, h = mac_in_windows(ct, key32)
                assert h == T % P, name
                assert tag == S.poly1305_int(ct, key32)[0], name
                done += 1
    assert done >= 40
