"""Poly1305 steered to its reduction edges, on the CPU (tests/poly_steer.py).

* The big-integer reference against the oracle and the golden vectors; steered
  MESSAGE frames decode in the oracle, their near-miss tags (tag +-1, +-5) fail.
* Limb-exact Python models of the two device forms of
  libzmq_amd/csrc/curve_device.hpp, each asserting at every step the bounds its
  comments state:
    - radix 2^32, sequential: poly32_key / poly32_block / poly32_finish
      (k_frames_seq, k_frames_lds);
    - radix 2^26 with powers of r: poly_r_from_key / block_limbs / acc_mul /
      fe_mul_s / fe_from_wide / poly_finish as k_frames<G = 1, 2, 4> composes
      them (curve_frames.hpp: lane q takes windows q, q + G, ..., the lanes'
      shares are summed in 32 bits).
  Both equal poly1305_int on the steered set, the extreme-key set and 2,000
  random cases.
* Coverage, measured in the models: the steered set takes both arms of the
  final select of each form, each arm from more than one target.  Printed, not
  required (they depend on the integer the form holds for a residue, which
  steering mod p does not control): whether the f-add of poly32_block ripples
  out of h3, the largest h4 it returns, the largest limb 1 poly_finish sees.
* Mutants: no final subtraction (each form), the carry out of f0 + s[0] dropped,
  limb 1 masked before poly_finish's first carry -- each rejected by the steered
  or extreme-key set, while the first passes all 2,000 random cases: the gap
  random payloads leave."""
import functools
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import poly_steer as S

M26, M32 = (1 << 26) - 1, (1 << 32) - 1
LENGTHS = S.FRAME_LENGTHS


def words(b16):
    return [int.from_bytes(b16[4 * i:4 * i + 4], "little") for i in range(4)]


def stream_blocks(ct):
    """(m0..m3, full) per 16-byte block, a partial one with its 0x01 pad byte."""
    for i in range(0, len(ct), 16):
        b = ct[i:i + 16]
        full = len(b) == 16
        yield words(b if full else b + b"\x01" + bytes(15 - len(b))), full


# ------------------------------------------------------------------ radix 2^32
def poly32_model(ct, key32, stats=None, mutant=None):
    st = stats if stats is not None else {}
    k = words(key32[:16])
    r0, r1, r2, r3 = k[0] & 0x0fffffff, k[1] & 0x0ffffffc, k[2] & 0x0ffffffc, k[3] & 0x0ffffffc
    s1, s2, s3 = r1 + (r1 >> 2), r2 + (r2 >> 2), r3 + (r3 >> 2)
    assert max(s1, s2, s3) <= M32
    h = [0, 0, 0, 0, 0]
    for m, full in stream_blocks(ct):
        a, c = [], 0
        for i in range(4):
            t = h[i] + m[i] + c
            a.append(t & M32)
            c = t >> 32
        a4 = h[4] + (1 if full else 0) + c
        assert a4 <= 6
        a0, a1, a2, a3 = a
        d0 = a0 * r0 + a1 * s3 + a2 * s2 + a3 * s1
        d1 = a0 * r1 + a1 * r0 + a2 * s3 + a3 * s2 + a4 * s1
        d2 = a0 * r2 + a1 * r1 + a2 * r0 + a3 * s3 + a4 * s2
        d3 = a0 * r3 + a1 * r2 + a2 * r1 + a3 * r0 + a4 * s3
        assert max(d0, d1, d2, d3) < 1 << 64  # sums of word products fit 64 bits
        h0 = d0 & M32
        t = (d1 & M32) + (d0 >> 32)
        h1, c = t & M32, t >> 32
        c1 = (d1 >> 32) + c
        assert c1 <= M32
        t = (d2 & M32) + c1
        h2, c = t & M32, t >> 32
        c2 = (d2 >> 32) + c
        assert c2 <= M32
        t = (d3 & M32) + c2
        h3, c = t & M32, t >> 32
        h4 = a4 * r0 + (d3 >> 32) + c
        assert h4 <= M32
        f = (h4 >> 2) + (h4 & ~3 & M32)
        assert f <= M32
        t = h0 + f
        o, c = [t & M32], t >> 32
        for x in (h1, h2, h3):
            t = x + c
            o.append(t & M32)
            c = t >> 32
        if c:
            st["ripple"] = st.get("ripple", 0) + 1  # the f-add rippled out of h3
        o.append((h4 & 3) + c)
        assert o[4] <= 4  # "h4 <= 4 on return"
        st["max_h4"] = max(st.get("max_h4", 0), o[4])
        h = o
    # poly32_finish
    g, c = [], 5
    for i in range(4):
        t = h[i] + c
        g.append(t & M32)
        c = t >> 32
    g4 = h[4] + c
    sub = bool(g4 >> 2)
    st["arm"] = "sub" if sub else "keep"
    if mutant == "nosub":
        sub = False
    f = g if sub else h[:4]
    sw = words(key32[16:32])
    tag, c = [], 0
    for i in range(4):
        t = f[i] + sw[i] + c
        tag.append(t & M32)
        c = t >> 32
        if mutant == "drop_c0" and i == 0:
            c = 0
    return b"".join(x.to_bytes(4, "little") for x in tag)


# ------------------------------------------------------------------ radix 2^26
def alignbit(hi, lo, sh):
    return (((hi << 32) | lo) >> sh) & M32


def r_from_key(k):
    return [k[0] & 0x3ffffff, alignbit(k[1], k[0], 26) & 0x3ffff03, alignbit(k[2], k[1], 20) & 0x3ffc0ff,
            alignbit(k[3], k[2], 14) & 0x3f03fff, (k[3] >> 8) & 0x00fffff]


def block_limbs(m, full):
    return [m[0] & M26, alignbit(m[1], m[0], 26) & M26, alignbit(m[2], m[1], 20) & M26,
            alignbit(m[3], m[2], 14) & M26, (m[3] >> 8) | ((1 << 24) if full else 0)]


def _products(h, p):
    assert all(x < (1 << 26) + (1 << 8) for x in p)  # "r limbs < 2^26 + 2^8"
    s = [0] + [p[i] * 5 for i in range(1, 5)]
    assert max(s) <= M32
    return [h[0] * p[0] + h[1] * s[4] + h[2] * s[3] + h[3] * s[2] + h[4] * s[1],
            h[0] * p[1] + h[1] * p[0] + h[2] * s[4] + h[3] * s[3] + h[4] * s[2],
            h[0] * p[2] + h[1] * p[1] + h[2] * p[0] + h[3] * s[4] + h[4] * s[3],
            h[0] * p[3] + h[1] * p[2] + h[2] * p[1] + h[3] * p[0] + h[4] * s[4],
            h[0] * p[4] + h[1] * p[3] + h[2] * p[2] + h[3] * p[1] + h[4] * p[0]]


def fe_mul_s(h, p, st):
    assert all(x < 1 << 27 for x in h)  # "h limbs < 2^27"
    d = _products(h, p)
    o, c = [0] * 5, 0
    for i in range(5):
        d[i] += c
        assert d[i] < 1 << 64
        c = d[i] >> 26
        assert c <= M32
        o[i] = d[i] & M26
    assert c * 5 <= M32
    o[0] += c * 5
    assert o[0] <= M32
    c = o[0] >> 26
    o[0] &= M26
    o[1] += c
    st["mul_l1_excess"] = max(st.get("mul_l1_excess", 0), o[1] - M26)
    return o


def acc_mul(a, m, p):
    assert all(x < 1 << 27 for x in m)
    d = _products(m, p)
    a = [a[i] + d[i] for i in range(5)]
    assert max(a) < 1 << 64
    return a


def fe_from_wide(w):
    a = list(w)
    for i in range(4):
        a[i + 1] += a[i] >> 26
        a[i] &= M26
    assert max(a) < 1 << 64
    a[0] += (a[4] >> 26) * 5
    a[4] &= M26
    a[1] += a[0] >> 26
    a[0] &= M26
    assert max(a) <= M32
    return a


def poly_finish(h, key32, st, mutant=None):
    h0, h1, h2, h3, h4 = h
    st["finish_l1"] = max(st.get("finish_l1", 0), h1)
    if mutant == "mask_l1":
        h1 &= M26
    c = h1 >> 26; h1 &= M26; h2 += c
    c = h2 >> 26; h2 &= M26; h3 += c
    c = h3 >> 26; h3 &= M26; h4 += c
    c = h4 >> 26; h4 &= M26; h0 += c * 5
    assert h0 <= M32
    c = h0 >> 26; h0 &= M26; h1 += c
    g0 = h0 + 5
    c = g0 >> 26; g0 &= M26
    g1 = h1 + c
    c = g1 >> 26; g1 &= M26
    g2 = h2 + c
    c = g2 >> 26; g2 &= M26
    g3 = h3 + c
    c = g3 >> 26; g3 &= M26
    g4 = (h4 + c - (1 << 26)) & M32
    sub = not (g4 >> 31)
    st["arm"] = "sub" if sub else "keep"
    if mutant == "nosub":
        sub = False
    if sub:
        h0, h1, h2, h3, h4 = g0, g1, g2, g3, g4
    assert h1 <= M26, "h1 << 26 would lose a bit"
    assert max(h0, h2, h3, h4) <= M26
    sw = words(key32[16:32])
    f0 = ((h0 | (h1 << 26)) & M32) + sw[0]
    f1 = (((h1 >> 6) | (h2 << 20)) & M32) + sw[1] + (0 if mutant == "drop_c0" else f0 >> 32)
    f2 = (((h2 >> 12) | (h3 << 14)) & M32) + sw[2] + (f1 >> 32)
    f3 = (((h3 >> 18) | (h4 << 8)) & M32) + sw[3] + (f2 >> 32)
    return b"".join((x & M32).to_bytes(4, "little") for x in (f0, f1, f2, f3))


def frames26_model(ct, key32, stats=None, mutant=None, G=1):
    """The tag as k_frames<G> computes it: the stream is the 32 key bytes and
    the ciphertext in 64-byte windows (window 0's first two blocks are the key
    area), L the last window with kb blocks."""
    st = stats if stats is not None else {}
    r = r_from_key(words(key32[:16]))
    assert sum(x << (26 * i) for i, x in enumerate(r)) == S.key_rs(key32)[0]
    P1 = r
    P2 = fe_mul_s(list(r), r, st)
    P3 = fe_mul_s(list(P2), r, st)
    P4 = fe_mul_s(list(P2), P2, st)
    PG, k = P4, 1
    while k < G:
        PG = fe_mul_s(list(PG), PG, st)
        k <<= 1
    pw = {1: P1, 2: P2, 3: P3, 4: P4}
    size = 32 + len(ct)
    nw = (size + 63) >> 6
    L = nw - 1
    kb = (size - 64 * L + 15) >> 4
    sb = bytes(32) + bytes(ct)
    blk = list(stream_blocks(sb))  # block 4w + j of the stream
    tot = [0] * 5
    for q in range(G):
        H, lastH = None, 0
        for w in range(q, nw, G):
            if w < L:
                a = [0] * 5
                if H is not None:
                    a = acc_mul(a, fe_from_wide(H), PG)
                if w > 0:
                    a = acc_mul(a, block_limbs(*blk[4 * w]), P4)
                    a = acc_mul(a, block_limbs(*blk[4 * w + 1]), P3)
                a = acc_mul(a, block_limbs(*blk[4 * w + 2]), P2)
                a = acc_mul(a, block_limbs(*blk[4 * w + 3]), P1)
                H, lastH = a, w
            else:
                a = [0] * 5
                for j in range(4):
                    if j < kb and not (w == 0 and j < 2):
                        a = acc_mul(a, block_limbs(*blk[4 * w + j]), pw[kb - j])
                u = fe_from_wide(a)
                tot = [tot[i] + u[i] for i in range(5)]
        if H is not None:
            e = fe_mul_s(fe_from_wide(H), pw[kb], st)
            for _ in range(L - 1 - lastH):
                e = fe_mul_s(e, P4, st)
            tot = [tot[i] + e[i] for i in range(5)]
        assert max(tot) <= M32  # the 32-bit lane sums cannot wrap
    return poly_finish(fe_from_wide(tot), key32, st, mutant)


# ------------------------------------------------------------------ the sets
@functools.lru_cache(maxsize=None)
def steered_set():
    cases = S.standard_cases(LENGTHS)
    assert len(cases) == len(LENGTHS) * len(S.targets(bytes(32))) - 1
    frames, used = S.steered_frames(cases, np.random.default_rng(20261019))
    print(f"steered set: {len(frames)} frames on {used} nonces, mean tries "
          f"{sum(f.tries for f in frames) / len(frames):.1f}, worst {max(f.tries for f in frames)}")
    return frames


@functools.lru_cache(maxsize=None)
def extreme_set():
    rng = np.random.default_rng(20261024)
    return ([f for ln in (16, 64, 65, 1025) for f in S.extreme_frames(ln)]
            + [f for ln in (65, 1025) for b in (0xff, 0x00) for f in S.extreme_steered(ln, rng, b)])


@functools.lru_cache(maxsize=None)
def random_set():
    rng = np.random.default_rng(5)
    out = []
    for _ in range(2000):
        n = int(rng.choice([1, 15, 16, 17, 33, 64, 100, 255, 300]))
        out.append((rng.integers(0, 256, n, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes()))
    return out


FORMS = [("poly32", poly32_model), ("fe26 G=1", functools.partial(frames26_model, G=1)),
         ("fe26 G=2", functools.partial(frames26_model, G=2)), ("fe26 G=4", functools.partial(frames26_model, G=4))]


# ------------------------------------------------------------------ the helper against the references
def test_poly1305_int_equals_oracle_and_golden():
    golden = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "curve_golden.json")))
    vecs = golden["primitives"]["poly1305"]
    assert len(vecs) >= 20
    for v in vecs:
        k, m = bytes.fromhex(v["k"]), bytes.fromhex(v["m"])
        assert S.poly1305_int(m, k)[0].hex() == v["tag"]
    for m, k in random_set()[:300]:
        assert S.poly1305_int(m, k)[0] == O.poly1305(m, k)
    for f in steered_set() + extreme_set():
        assert f.tag == O.poly1305(f.ct, f.key32)


def test_steer_rejects_what_it_cannot_do():
    rng = np.random.default_rng(1)
    k = S.message_stream(3, 32)
    with pytest.raises(ValueError):
        S.steer(k, 15, 0, 0, rng)  # no full block
    with pytest.raises(ValueError):
        S.steer(k, 40, 2, 0, rng)  # block 2 is partial
    # one block and T = 0: the solution is p - 2^128 under every key, no block
    assert not S.reachable(16, 0) and (0 - (1 << 128)) % S.P > S.M128
    with pytest.raises(S.SteerError):
        S.steer(k, 16, 0, 0, rng)
    ct, _ = S.steer(k, 100, 3, S.P - 1, rng, base=0xff)
    assert S.poly1305_int(ct, k)[1] == S.P - 1
    assert sum(ct[i:i + 16] != b"\xff" * 16 for i in range(0, 96, 16)) <= 2 and ct[96:] == b"\xff" * 4


def _decode(wires, peer0=2):
    n = len(wires)
    wl = np.array([len(w) for w in wires], np.uint32)
    off = np.concatenate([[0], np.cumsum(wl)[:-1]]).astype(np.uint64)
    buf = np.frombuffer(b"".join(wires) + bytes(64), np.uint8)
    peer = np.array([peer0], np.uint64)
    out, fl, st = O.decode_batch(O.make_sessions([S.TEST_KEY], dec_prefix=S.PREFIX), peer, np.zeros(n, np.uint32), off,
                                 wl, buf, off, len(buf))
    return out, fl, st, off, int(peer[0])


def test_steered_frames_decode_and_encode_in_the_oracle():
    fr = steered_set()
    out, fl, st, off, peer = _decode([f.wire for f in fr])
    assert (st == 0).all() and peer == fr[-1].nonce
    for i, f in enumerate(fr):
        assert bytes(out[int(off[i]):int(off[i]) + len(f.payload)]) == f.payload
        assert fl[i] == f.flags_byte & 3 and f.flags_byte < 4
    # the encode direction: crypto_box_easy_afternm of flags byte || payload
    for f in fr[::7]:
        box = O.box_easy_afternm(bytes([f.flags_byte]) + f.payload, S.PREFIX + f.nonce.to_bytes(8, "big"), S.TEST_KEY)
        assert box == f.tag + f.ct


def test_near_miss_tags_fail_in_the_oracle():
    fr = steered_set()
    # (the four near misses of a frame share its nonce, and a failed MAC has
    # advanced the peer nonce already: one batch per kind)
    for k in range(4):
        _, _, st, _, peer = _decode([f.near_misses()[k] for f in fr])
        assert (st == S.ERR_CRYPTOGRAPHIC).all(), k
        assert peer == fr[-1].nonce


# ------------------------------------------------------------------ the models
@pytest.mark.parametrize("name,model", FORMS)
def test_models_equal_the_reference(name, model):
    st = {}
    for f in steered_set() + extreme_set():
        assert model(f.ct, f.key32, st) == f.tag, (name, f.name, len(f.ct), f.nonce)
    for m, k in random_set():
        assert model(m, k, st) == S.poly1305_int(m, k)[0]
    print(f"{name}: bounds held on {len(steered_set())} steered, {len(extreme_set())} extreme-key and 2000 random "
          f"cases; {st}")


@pytest.mark.parametrize("name,model", FORMS)
def test_steered_set_takes_both_arms_of_the_final_select(name, model):
    arms = {"sub": set(), "keep": set()}
    agg = {}
    for f in steered_set():
        st = {}
        assert model(f.ct, f.key32, st) == f.tag
        arms[st["arm"]].add(f.name)
        for k in ("ripple", "max_h4", "finish_l1", "mul_l1_excess"):
            if k in st:
                agg[k] = max(agg.get(k, 0), st[k])
    rnd = {"sub": 0, "keep": 0}
    for m, k in random_set():
        st = {}
        model(m, k, st)
        rnd[st["arm"]] += 1
    print(f"{name}: final select, steered set: subtract-p arm from targets {sorted(arms['sub'])}, keep arm from "
          f"{sorted(arms['keep'])}; random cases: {rnd}")
    if name == "poly32":
        print(f"{name}: f-add rippled out of h3: {'yes' if agg.get('ripple') else 'never'}; "
              f"largest h4 returned: {agg.get('max_h4')}")
    else:
        print(f"{name}: largest limb 1 entering poly_finish: 2^26 + {agg['finish_l1'] - (1 << 26)}; "
              f"largest fe_mul_s limb-1 excess: {agg.get('mul_l1_excess')}")
    assert len(arms["sub"]) > 1 and len(arms["keep"]) > 1


def _rejected(model, frames, mutant):
    return sum(model(f.ct, f.key32, None, mutant) != f.tag for f in frames)


@pytest.mark.parametrize("name,model,mutant", [("poly32", poly32_model, "nosub"), ("poly32", poly32_model, "drop_c0")]
                         + [(n, m, mu) for n, m in FORMS[1:] for mu in ("nosub", "drop_c0", "mask_l1")])
def test_mutants_are_rejected(name, model, mutant):
    a, b = _rejected(model, steered_set(), mutant), _rejected(model, extreme_set(), mutant)
    rnd = sum(model(m, k, None, mutant) != S.poly1305_int(m, k)[0] for m, k in random_set())
    print(f"{name} mutant {mutant}: rejected on {a} of {len(steered_set())} steered, {b} of {len(extreme_set())} "
          f"extreme-key, {rnd} of 2000 random cases")
    assert a + b > 0
    if mutant == "nosub":
        assert rnd == 0  # the gap: random payloads never reach the final subtraction
