"""Streams that steer zmqg_decode_zmtp's candidate scan, links and walk to their
edges (libzmq_amd/csrc/curve_zmtp.hpp), shared by tests/test_zmtp_scan_model.py
(CPU: the model of tests/zmtp_scan_model.py against the oracle, and the
coverage facts) and tests/test_gpu_zmtp_scan_edges.py (the device against the
oracle).  TEST INFRASTRUCTURE ONLY.

Frames are real CURVE MESSAGE frames (oracle.encode_batch, zmtp_oracle.frame)
of one connection per stream, nonces 3, 4, ...; a filler first frame sized to
fit puts the steered offset where it must be.  Exceptions, noted where they
are made: minimal frames (00 08 07 MESSAGE: a MESSAGE command too short to
decode), bytes planted inside a ciphertext, hand-made headers.

A case is a dict: cls, name, stream, max_msg, max_frames, precom, want (the
outcome the oracle alone must give: frames, consumed, error) and, for the
early-stop streams, kth (the frame a planted LARGE header covers)."""
import functools
import struct
import zlib

import numpy as np

from oracle import oracle as O
from oracle import zmtp_oracle as Z
from tests.zmtp_scan_model import tile

PEER0 = 2
MIN = b"\x00\x08" + Z.MESSAGE  # a complete minimal frame
PING = Z.frame(b"\x04PING\x00\x00\x00")


class Conn:
    """One connection's sender: frames with rising nonces."""

    def __init__(self, name):
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.precom = self.rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        self.nonce = 3

    def bodies(self, lens):
        n = len(lens)
        if n == 0:
            return []
        lens = np.asarray(lens, np.uint32)
        in_off = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]]).astype(np.uint64)
        inp = np.frombuffer(self.rng.bytes(max(int(lens.sum()), 1)), np.uint8)
        wl = lens.astype(np.uint64) + 33
        out_off = np.concatenate([[0], np.cumsum(wl)[:-1]]).astype(np.uint64)
        wire = O.encode_batch(O.make_sessions([self.precom]), np.zeros(n, np.uint32),
                              np.arange(self.nonce, self.nonce + n, dtype=np.uint64), np.zeros(n, np.uint8), in_off,
                              lens, inp, out_off, int(wl.sum()))
        self.nonce += n
        return [bytearray(wire[int(o):int(o) + int(w)].tobytes()) for o, w in zip(out_off, wl)]

    def frames(self, lens):
        return [Z.frame(b) for b in self.bodies(lens)]

    def fill(self, total):
        """Frames of exactly `total` bytes together (>= 35)."""
        if 35 <= total <= 257:
            return self.frames([total - 35])
        if total >= 265:
            return self.frames([total - 42])
        return self.frames([0]) + self.fill(total - 35)


def large(body):
    return bytes([Z.LARGE]) + struct.pack(">Q", len(body)) + bytes(body)


def case(cls, name, conn, stream, want, max_msg=-1, max_frames=64, kth=None, **kw):
    d = dict(cls=cls, name=name, stream=bytes(stream), max_msg=max_msg, max_frames=max_frames, precom=conn.precom,
             want=want, kth=kth)
    d.update(kw)
    return d


def whole(frames):
    """The oracle returns every frame and consumes the stream."""
    return dict(frames=len(frames), consumed=sum(len(f) for f in frames), error=0)


GENERIC_EDGE = 16 * 37


def edges():
    """A chunk edge in mid-round, the round edges, a list edge (another workgroup), the next."""
    return (GENERIC_EDGE, 4096, 8192, 12288, tile(), 2 * tile())


@functools.lru_cache(maxsize=None)
def class_a():
    """The second frame's signature at B + d, short and LARGE header."""
    out = []
    for B in edges():
        for d in range(-16, 17):
            for kind in ("short", "large"):
                c = Conn("a-%d-%d-%s" % (B, d, kind))
                q = B + d
                fr = c.fill(q - (2 if kind == "short" else 9))
                k = len(fr)
                fr += c.frames([40 if kind == "short" else 300, 5, 64, 100])
                out.append(case("a", "%s@%d%+d" % (kind, B, d), c, b"".join(fr), whole(fr), B=B, d=d, kind=kind, q=q,
                                second=k))
    return out


@functools.lru_cache(maxsize=None)
def class_b():
    """Stream start (signatures at q = 2 and q = 9) and every end."""
    out = []
    for kind, first in (("q2", 40), ("q9", 300)):
        c = Conn("b-" + kind)
        fr = c.frames([first, 64, 5, 100, 64])
        out.append(case("b", kind, c, b"".join(fr), whole(fr), q=2 if kind == "q2" else 9))
    for r in range(16):
        c = Conn("b-end-%d" % r)
        pre = c.fill(16 * 20 + (r - 10 - 99 - 342) % 16) + c.frames([64, 300])  # (99 + 342: the two frames' bytes)
        P = b"".join(pre)
        assert (len(P) + 10) % 16 == r
        short, lg = c.frames([40, 400])
        done = dict(frames=len(pre), consumed=len(P), error=0)
        out.append(case("b", "end%d" % r, c, P + MIN, dict(frames=len(pre) + 1, consumed=len(P) + 10, error=0), r=r))
        for k in range(1, 8):  # 1..7 bytes of the signature
            out.append(case("b", "end%d-sig%d" % (r, k), c, P + MIN[:2 + k], done, r=r))
        out.append(case("b", "end%d-body" % r, c, P + short[:2 + 8 + 3], done, r=r))  # a whole signature, a short body
        out.append(case("b", "end%d-hdr1" % r, c, P + short[:1], done, r=r))
        for k in range(2, 9):  # 2..8 bytes of a LARGE header
            out.append(case("b", "end%d-large%d" % (r, k), c, P + lg[:k], done, r=r))
    return out


SHADOW_SIZES = ((0x01, 0x10), (0x01, 0x00), (0x02, 0x10), (0x03, 0x08), (0x05, 0x20))
EARLY_LENS = [64, 100, 40, 150, 64, 5]  # (frames 1, 3 and 5 have short headers)


def early_stream(c, k, flag, last):
    """EARLY_LENS frames, the 7 bytes in front of frame k overwritten with
    flag 00 00 00 00 00 last (the ciphertext's tail: not an oracle frame any
    more, it fails its MAC): a LARGE header whose size ends in frame k's own
    flags and size bytes."""
    bodies = c.bodies(EARLY_LENS)
    bodies[k - 1][-7:] = bytes([flag, 0, 0, 0, 0, 0, last])
    return [Z.frame(b) for b in bodies]


@functools.lru_cache(maxsize=None)
def class_c():
    """Shadows of true LARGE headers; the early stop and its negative."""
    out = []
    for b7, b8 in SHADOW_SIZES:
        c = Conn("c-%02x%02x" % (b7, b8))
        fr = c.frames([64, b7 * 256 + b8 - 33, 100, b7 * 256 + b8 - 33, 5])
        assert fr[1][7:9] == bytes([b7, b8])
        out.append(case("c", "shadow-%02x%02x" % (b7, b8), c, b"".join(fr), whole(fr),
                        shadows=2 if not b7 & Z.LARGE and b8 >= 8 else 0))
    for k in (1, 3, 5):
        for flag in (0x02, 0x03, 0x06):
            c = Conn("c-early-%d-%d" % (k, flag))
            fr = early_stream(c, k, flag, 0)
            out.append(case("c", "early-k%d-f%02x" % (k, flag), c, b"".join(fr), whole(fr), kth=k))
            c = Conn("c-late-%d-%d" % (k, flag))
            fr = early_stream(c, k, flag, 1)  # the planted size is 65536 + frame k's: too large
            out.append(case("c", "noearly-k%d-f%02x" % (k, flag), c, b"".join(fr), whole(fr), shadows=0))
    return out


@functools.lru_cache(maxsize=None)
def class_d():
    """Candidate and signature density."""
    out = []
    c = Conn("d-min")
    fr = c.fill(tile() - 1000) + [MIN] * 2000 + c.frames([64])  # (minimal frames: too short to decode)
    out.append(case("d", "min2000", c, b"".join(fr), whole(fr), max_frames=2100, dense=True))
    c = Conn("d-sig8")
    b = c.bodies([64, 2000, 64, 100])
    b[1][33:33 + 8 * 200] = Z.MESSAGE * 200  # (planted: signatures 8 apart, none with a header)
    fr = [Z.frame(x) for x in b]
    out.append(case("d", "sig8", c, b"".join(fr), whole(fr), sig8=True))
    c = Conn("d-flood")
    b = c.bodies([64, 9000, 64, 100])
    pat = b"\x00\x10" + Z.MESSAGE + bytes(6)  # (planted: the "flood" pattern of tests/test_zmtp.py)
    b[1][33:33 + 16 * 540] = pat * 540
    fr = [Z.frame(x) for x in b]
    out.append(case("d", "flood", c, b"".join(fr), whole(fr), flood=True))
    return out


PLANT = b"\x00\x20" + Z.MESSAGE  # (planted: a short header and the signature inside a ciphertext)


@functools.lru_cache(maxsize=None)
def class_e():
    """Links and walk."""
    out = []
    c = Conn("e-own")
    b = c.bodies([64, 100, 300, 64, 40])
    b[2][40:50] = PLANT
    fr = [Z.frame(x) for x in b]
    out.append(case("e", "own-list", c, b"".join(fr), whole(fr), src="nb"))
    c = Conn("e-later")
    b = c.bodies([1000] * 40)
    b[30][500:510] = PLANT
    fr = [Z.frame(x) for x in b]
    out.append(case("e", "later-list", c, b"".join(fr), whole(fr), src="first_w"))
    c = Conn("e-exact")
    b = c.bodies([64, 200, 64, 64])
    b[1][100:102] = bytes([0, len(b[1]) - 102])  # (planted: a frame that ends where the next true one starts)
    b[1][102:110] = Z.MESSAGE
    fr = [Z.frame(x) for x in b]
    out.append(case("e", "linked-off-chain", c, b"".join(fr), whole(fr), off_chain=True))
    c = Conn("e-gap")
    fr = c.frames([64, 66 * tile(), 64, 64])
    out.append(case("e", "gap65", c, b"".join(fr), whole(fr), gap=True))
    c = Conn("e-cut")
    b = c.bodies([64, 100, 300, 64, 40, 64])
    b[2][40:50] = PLANT
    fr = [Z.frame(x) for x in b]
    fr.insert(5, PING)  # runs [0..2] and [3..4], then the PING, then a frame never reached
    s = b"".join(fr)
    end = lambda k: sum(len(f) for f in fr[:k])
    # inside a linked run; at a run's last frame; right before the PING (not returned); with the PING
    for mf, what in ((2, "in-run"), (3, "run-end"), (5, "before-extra"), (6, "with-extra")):
        out.append(case("e", "cut-" + what, c, s, dict(frames=mf, consumed=end(mf), error=0), max_frames=mf,
                        cut=what))
    return out


@functools.lru_cache(maxsize=None)
def long_case(nlists):
    """(f) A planted header in the last list of an nlists-list stream made of
    a few large frames: the smallest stream of that many lists."""
    n = (nlists - 1) * tile() + 1
    c = Conn("f-%d" % nlists)
    nbig = max(2, (nlists + 2047) // 2048)  # frames of at most 32 MiB
    tail = [64, 300, 64, 40]
    rest = n - sum(l + 33 + (9 if l + 33 > 255 else 2) for l in tail)
    bigs = [rest // nbig - 42] * nbig
    bigs[0] += rest - sum(x + 42 for x in bigs)
    b = c.bodies(bigs + tail)
    b[nbig + 1][40:50] = PLANT
    fr = [Z.frame(x) for x in b]
    s = b"".join(fr)
    assert len(s) == n
    return case("f", "lists%d" % nlists, c, s, whole(fr), nlists=nlists)


@functools.lru_cache(maxsize=None)
def class_g():
    """Size fields and max_msg_size."""
    out = []
    lens = [64, 100, 300, 40]
    for v in (0xFFFFFFFF, 0x100000000, 0x8000000000000000):
        for pos in ("first", "mid", "last"):
            c = Conn("g-%x-%s" % (v, pos))
            fr = c.frames(lens)
            # (hand-made: a LARGE header with that size, the signature, and valid frames in its claimed body)
            H = bytes([Z.LARGE]) + struct.pack(">Q", v) + Z.MESSAGE + bytes(range(24))
            k = dict(first=0, mid=2, last=4)[pos]
            s = b"".join(fr[:k]) + H + b"".join(fr[k:])
            out.append(case("g", "size%x-%s" % (v, pos), c, s,
                            dict(frames=k, consumed=sum(len(f) for f in fr[:k]), error=0 if v <= 0xFFFFFFFF else
                                 Z.EMSGSIZE)))
    sizes = [l + 33 for l in lens]
    for mm, k in ((max(sizes), 4), (max(sizes) - 1, 2), (0, 0), (7, 0)):
        c = Conn("g-max%d" % mm)
        fr = c.frames(lens)
        out.append(case("g", "max_msg%d" % mm, c, b"".join(fr),
                        dict(frames=k, consumed=sum(len(f) for f in fr[:k]), error=0 if k == 4 else Z.EMSGSIZE),
                        max_msg=mm))
    c = Conn("g-large3")
    fr = c.frames(lens)
    odd = bytes([Z.LARGE]) + struct.pack(">Q", 3) + b"\xaa\xbb\xcc"  # (hand-made: non-canonical LARGE, size 3)
    s = b"".join(fr[:2]) + odd + b"".join(fr[2:])
    out.append(case("g", "large3", c, s, dict(frames=3, consumed=len(fr[0]) + len(fr[1]) + 12, error=0)))
    c = Conn("g-0000")
    fr = c.frames(lens)
    s = b"".join(fr) + b"\x00\x00"  # (hand-made: an empty frame ends the stream)
    out.append(case("g", "tail0000", c, s, dict(frames=5, consumed=len(s), error=0)))
    return out


CLASSES = dict(a=class_a, b=class_b, c=class_c, d=class_d, e=class_e, g=class_g)
LONG_LISTS = (1025, 8193)  # zmtp_suffix_min's per = 2 (registers) and per = 9 (the loop)


def expected(cs, max_frames=None, stream=None, peer=PEER0):
    """What the device must return for the case: zmtp_oracle.parse and
    oracle.decode_batch over the parsed frames, as
    tests/test_zmtp.py::test_decode_zmtp_matches_oracle takes them."""
    stream = cs["stream"] if stream is None else stream
    ref = Z.parse(stream, cs["max_msg"], cs["max_frames"] if max_frames is None else max_frames)
    fr = ref["frames"]
    nf = len(fr)
    f_off = np.array([f[1] for f in fr], np.uint64)
    f_len = np.array([f[2] for f in fr], np.uint32)
    plen = np.maximum(f_len.astype(np.int64) - 33, 0)
    dec = O.make_sessions([cs["precom"]], dec_prefix=O.CLIENT_PREFIX)
    inp = np.frombuffer(stream, np.uint8)
    pn = np.array([peer], np.uint64)
    # each payload at its body's offset (include/zmqg_curve.h)
    out, fl, st = O.decode_batch(dec, pn, np.zeros(nf, np.uint32), f_off, f_len, inp, f_off, len(stream))
    fl = np.array([int(fl[i]) | (Z.msg_flags(fr[i][0]) if st[i] == 0 else 0) for i in range(nf)], np.uint8)
    return dict(frames=nf, consumed=ref["consumed"], error=ref["error"], out_bytes=int(plen.sum()), f_off=f_off,
                f_len=f_len, plen=plen, flags=fl, status=st.astype(np.int64) & 0xFFFFFFFF, out=out, peer=int(pn[0]))
