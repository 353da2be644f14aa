"""Steering Poly1305 to its reduction edges (test infrastructure, not a conftest).

The device MACs (libzmq_amd/csrc/curve_device.hpp and the kernels built on it)
never see a chosen Poly1305 key: (r, s) is the first 32 bytes of the XSalsa20
stream and the message is ciphertext, so on random payloads the accumulator is
uniform mod p = 2^130 - 5 and the final conditional subtraction, the values next
to 0 and p and the carries of `h + s` are reached with probability ~2^-100.
Decode accepts any ciphertext, though, and the accumulator is affine in every
16-byte block, so with (r, s) fixed by the session key and nonce one full block
can be solved to put the accumulator, before the final freeze, on any target T:

    x = (T - A) * r^-k mod p       A: the accumulator with x = 0,
                                   k: blocks from the free one to the end

which is a valid block when x < 2^128 (about one try in four; otherwise another
block is re-randomised).  Encode reaches the same state from plaintext =
steered ciphertext XOR keystream.

A ciphertext shorter than 16 bytes has no full block and cannot be steered.
What steering mod p does not control is the integer (T, T + p, ...) a device
form holds for that residue, so representation-dependent events (a carry that
ripples out of h3 in poly32_block, say) are measured, not forced.

poly1305_int is the high-precision reference (RFC 8439 in Python integers);
the oracle is used for HSalsa20 / Salsa20 only."""
import functools

import numpy as np

from oracle import oracle as O

P = (1 << 130) - 5
M128 = (1 << 128) - 1
CLAMP = 0x0ffffffc0ffffffc0ffffffc0fffffff
MAX_TRIES = 200
ERR_CRYPTOGRAPHIC = 0x11000001

# the session key every steered MESSAGE frame of the suite is made under
TEST_KEY = bytes((37 * i + 11) & 0xff for i in range(32))
PREFIX = O.CLIENT_PREFIX  # the sender's nonce prefix (the decoder's dec_prefix)


class SteerError(RuntimeError):
    pass


def key_rs(key32):
    return int.from_bytes(key32[:16], "little") & CLAMP, int.from_bytes(key32[16:32], "little")


def blocks_of(m):
    """The message's blocks as integers, pad bit / pad byte included."""
    m = bytes(m)
    return [int.from_bytes(m[i:i + 16], "little") | (1 << (8 * len(m[i:i + 16]))) for i in range(0, len(m), 16)]


def poly1305_int(m, key32):
    """(tag, h): RFC 8439 Poly1305 of m under key32; h is the accumulator mod p
    before the pad s is added."""
    r, s = key_rs(key32)
    h = 0
    for b in blocks_of(m):
        h = (h + b) * r % P
    return ((h + s) & M128).to_bytes(16, "little"), h


def targets(key32):
    """[(name, T)]: the accumulator values worth reaching under this (r, s)."""
    _, s = key_rs(key32)
    ns = (-s) & M128
    return [("0", 0), ("1", 1), ("4", 4), ("p-1", P - 1), ("p-5", P - 5),  # next to zero and p
            ("2^128-1", M128), ("2^128", 1 << 128), ("2^129", 1 << 129),  # word and limb edges
            ("2^26-1", (1 << 26) - 1),  # limb 0 saturated, the others zero
            ("-s", ns), ("-s-1", (ns - 1) & M128), ("-s+2^129", ns + (1 << 129)),  # carry out of h + s
            # T + p = 2^130 + (2^26 - 1) 2^26 + (2^26 - 5 + e): the 2^130 fold carries limb 0 into a
            # saturated limb 1 (curve_device.hpp fe_from_wide leaves limb 1 = 2^26 for poly_finish)
            ("2^52", 1 << 52), ("2^52+4", (1 << 52) + 4)]


def reachable(length, T):
    """False for the one case no key allows: a single full block x gives the
    accumulator (x + 2^128) r with 2^128 <= x + 2^128 < 2^129 < p, which is
    never 0 mod p (r is invertible).  Every other (length >= 16, T) is reached
    under some nonce."""
    return not (length == 16 and T % P == 0)


def steer(key32, length, free_block, T, rng, base=None, first=None):
    """(ciphertext, tries): `length` bytes whose Poly1305 accumulator under
    key32 is T mod p before the freeze.  free_block: index of the full block
    that is solved.  base: a byte value kept in every block except the solved
    one and the one that is re-randomised between tries (None: random bytes).
    first: allowed values of ciphertext byte 0 (the encode direction needs
    ct[0] ^ ks[32] in 0..3): pinned when another block is solved, a condition
    on the solution when block 0 is.  Raises SteerError after MAX_TRIES tries,
    or at once when nothing is left to re-randomise (a single block)."""
    r, _ = key_rs(key32)
    nfull, nb = length // 16, (length + 15) // 16
    if nfull < 1:
        raise ValueError("a ciphertext under 16 bytes has no full block to solve")
    if not 0 <= free_block < nfull:
        raise ValueError("free_block must name a full block")
    if r == 0:
        raise SteerError("r = 0: the tag does not depend on the message")
    first = None if first is None else sorted(first)
    ct = bytearray(rng.integers(0, 256, length, dtype=np.uint8).tobytes() if base is None else bytes([base]) * length)
    if first is not None and free_block != 0:
        ct[0] = first[int(rng.integers(0, len(first)))]
    ct[16 * free_block:16 * free_block + 16] = bytes(16)
    pw = [1] * (nb + 1)
    for j in range(1, nb + 1):
        pw[j] = pw[j - 1] * r % P
    bl = blocks_of(ct)
    A = sum(b * pw[nb - i] for i, b in enumerate(bl)) % P
    inv = pow(pw[nb - free_block], P - 2, P)
    rr = None if nb == 1 else free_block + 1 if free_block + 1 < nb else free_block - 1
    for tries in range(1, MAX_TRIES + 1):
        x = (T - A) * inv % P
        if x <= M128 and (first is None or free_block != 0 or (x & 0xff) in first):
            ct[16 * free_block:16 * free_block + 16] = x.to_bytes(16, "little")
            return bytes(ct), tries
        if rr is None:
            break
        lo, hi = 16 * rr, min(16 * rr + 16, length)
        keep0 = rr == 0 and first is not None
        new = bytearray(rng.integers(0, 256, hi - lo, dtype=np.uint8).tobytes())
        if keep0:
            new[0] = ct[0]
        ct[lo:hi] = new
        nv = int.from_bytes(new, "little") | (1 << (8 * (hi - lo)))
        A = (A + (nv - bl[rr]) * pw[nb - rr]) % P
        bl[rr] = nv
    raise SteerError(f"no block below 2^128 for length {length}, free block {free_block}")


# ------------------------------------------------------------------ streams and frames
def stream(precom, prefix16, nonce8, n):
    """n bytes of the XSalsa20 stream of crypto_box_afternm: subkey =
    HSalsa20(nonce[:16], key), then Salsa20 under nonce[16:24].  Bytes 0..31
    are the Poly1305 key, byte 32 + i masks message byte i."""
    return O.salsa20_stream(n, bytes(nonce8), O.hsalsa20(bytes(prefix16), bytes(precom)))


def message_stream(nonce, n, precom=TEST_KEY, prefix=PREFIX):
    return stream(precom, prefix, int(nonce).to_bytes(8, "big"), n)


def xor(a, b):
    return (np.frombuffer(bytes(a), np.uint8) ^ np.frombuffer(bytes(b), np.uint8)[:len(a)]).tobytes()


def wire_frame(nonce, tag, ct):
    """The MESSAGE command: "\\x07MESSAGE" || BE64(nonce) || tag || ct."""
    return b"\x07MESSAGE" + int(nonce).to_bytes(8, "big") + bytes(tag) + bytes(ct)


def near_miss_tags(tag):
    """tag + 1, - 1, + 5, - 5 mod 2^128 (tag - 5 is what a missing final
    subtraction of p yields)."""
    t = int.from_bytes(tag, "little")
    return [((t + d) & M128).to_bytes(16, "little") for d in (1, -1, 5, -5)]


class Frame:
    """One steered MESSAGE frame and everything the checks need."""

    def __init__(self, nonce, ks, ct, name, T, free_block, tries):
        self.nonce, self.ks, self.ct, self.name, self.T = nonce, ks, ct, name, T
        self.free_block, self.tries = free_block, tries
        self.key32 = ks[:32]
        self.tag, self.h = poly1305_int(ct, self.key32)
        assert self.h == T % P
        self.wire = wire_frame(nonce, self.tag, ct)
        pt = xor(ct, ks[32:])
        self.flags_byte, self.payload = pt[0], pt[1:]  # what encodes to this frame

    def near_misses(self):
        return [wire_frame(self.nonce, t, self.ct) for t in near_miss_tags(self.tag)]


# ciphertext lengths of the shared frame-kernel set (payload = length - 1): around
# the block and 64-byte window edges, and the two largest the frame kernels take
# (4,576 = 72 whole windows of stream with the key, the kernels' limit)
FRAME_LENGTHS = [16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 97, 128, 129, 1025, 4574, 4576]


def standard_cases(lengths, free=("first", "middle", "last")):
    """(length, target index, free block) for every length x target, the free
    block in rotation; the one unreachable pair (16 bytes, T = 0: reachable())
    is left out here, by name, and nowhere else."""
    names = targets(bytes(32))
    return [(ln, ti, free[(i + ti) % len(free)]) for i, ln in enumerate(lengths) for ti in range(len(names))
            if not (ln == 16 and names[ti][0] == "0")]


def steered_frames(cases, rng, nonce0=3, precom=TEST_KEY, encodable=True, base=None):
    """One Frame per case (ct_length, target_index, free) with free in
    "first" / "middle" / "last", under increasing nonces from nonce0.  A case
    that cannot be realised under a nonce (SteerError: a single block, or a
    solved block 0 that must also give a flags byte in 0..3) moves to the next
    nonce; no case is dropped.  Returns (frames, nonces_used)."""
    frames, nonce = [], nonce0
    for length, ti, free in cases:
        nfull = length // 16
        fb = {"first": 0, "middle": nfull // 2, "last": nfull - 1}[free]
        for _ in range(100000):
            ks = message_stream(nonce, 32 + length, precom)
            name, T = targets(ks[:32])[ti]
            if not reachable(length, T):
                raise ValueError(f"case {(length, name)} is unreachable under every key")
            try:
                ct, tries = steer(ks[:32], length, fb, T, rng, base=base,
                                  first=[ks[32] ^ f for f in range(4)] if encodable else None)
            except SteerError:
                nonce += 1
                continue
            frames.append(Frame(nonce, ks, ct, name, T, fb, tries))
            nonce += 1
            break
        else:
            raise SteerError(f"case {(length, ti, free)} was never realised")
    assert len(frames) == len(cases)
    return frames, nonce - nonce0


def box_item(rng, length, ti, free_block=None):
    """(key, nonce24, message, box): a crypto_box_easy_afternm item whose
    ciphertext is steered to target ti; box = tag || ciphertext."""
    while True:
        key = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        nonce = rng.integers(0, 256, 24, dtype=np.uint8).tobytes()
        ks = stream(key, nonce[:16], nonce[16:], 32 + length)
        fb = (length // 16 - 1) if free_block is None else free_block
        try:
            ct, _ = steer(ks[:32], length, fb, targets(ks[:32])[ti][1], rng)
        except SteerError:
            continue  # a single block: another key and nonce
        tag, _ = poly1305_int(ct, ks[:32])
        return key, nonce, xor(ct, ks[32:]), tag + ct


# ------------------------------------------------------------------ extreme keys
def r_words(key32):
    r, _ = key_rs(key32)
    return [(r >> (32 * i)) & 0xffffffff for i in range(4)]


def r_limbs(key32):
    r, _ = key_rs(key32)
    return [(r >> (26 * i)) & 0x3ffffff for i in range(5)]


@functools.lru_cache(maxsize=None)
def extreme_nonces(precom=TEST_KEY, count=1 << 14, nonce0=3):
    """The nonces in nonce0 .. nonce0 + count whose Poly1305 key has the largest
    or the smallest clamped 32-bit word r0..r3 or 26-bit limb of r: at most 18,
    sorted.  They reach the largest products the limb forms can see."""
    feats = []
    for n in range(nonce0, nonce0 + count):
        k = message_stream(n, 32, precom)
        feats.append(r_words(k) + r_limbs(k))
    f = np.array(feats, dtype=np.uint64)
    return tuple(sorted({int(nonce0 + i) for i in np.concatenate([f.argmax(axis=0), f.argmin(axis=0)])}))


def extreme_steered(length, rng, base=0xff, precom=TEST_KEY):
    """One frame per extreme key (increasing nonces): `base` in every block but
    the solved one and its re-randomised neighbour, steered to the targets in
    rotation, the free block first / middle / last in rotation.  Decode only:
    the flags byte is whatever it comes to.  length >= 17."""
    out = []
    for i, n in enumerate(extreme_nonces(precom)):
        ks = message_stream(n, 32 + length, precom)
        tg = targets(ks[:32])
        name, T = tg[(5 * i) % len(tg)]
        nfull = length // 16
        fb = (0, nfull // 2, nfull - 1)[i % 3]
        ct, tries = steer(ks[:32], length, fb, T, rng, base=base)
        out.append(Frame(n, ks, ct, name, T, fb, tries))
    return out


def extreme_frames(length, precom=TEST_KEY, bases=(0xff, 0x00)):
    """Unsteered frames of `length` ciphertext bytes, all-0xff and all-zero,
    under the extreme keys (increasing nonces)."""
    out = []
    for n in extreme_nonces(precom):
        for b in bases:
            ks = message_stream(n, 32 + length, precom)
            ct = bytes([b]) * length
            _, h = poly1305_int(ct, ks[:32])
            out.append(Frame(n, ks, ct, "base %02x" % b, h, -1, 0))
    return out
