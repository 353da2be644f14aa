"""Steered batches for the per-session tables behind every multi-session call
(k_replay_* with k_fixup, k_nonce_*, and the sort fallback above 8,192
sessions; libzmq_amd/csrc/zmqg_curve.hip) -- test infrastructure, not a test.

A decode batch is real MESSAGE frames from the oracle.  Every steered pair has
a session of its own:
  kill pair    frame a at i with nonce N, frame b at j > i with a nonce <= N:
               b must get INVALID_SEQUENCE (catches a prefix that is missing);
  keep triple  frames at i < j < k with nonces N, N + 1, N + 7: all pass
               (catches a later maximum leaking backwards).
The positions between are background sessions with rising nonces and about one
replay in ten.  `want` holds the status each frame was built for; the expected
values of the GPU test are the oracle's alone (Batch.expected, EncodeCase.expected)
and tests/test_session_tables_model.py asserts that they equal `want`.
"""
import functools

import numpy as np

from oracle import oracle as O

OK, UNEXPECTED, SEQ, MALFORMED_UNSPEC, MALFORMED_MSG, CRYPTO = (0, 0x10000001, 0x10000002, 0x10000011, 0x10000012,
                                                                0x11000001)
ERR_SESSION, ERR_BOUND = 0x7A000001, 0x7A000002  # include/zmqg_curve.h
SENTINEL = 0x33
BIG = 4700  # payload bytes of a frame above the frame kernel's 4,608 wire bytes: the body finisher reads excl
T256 = 256
RISE, REPLAY, FIXED = 0, 1, 2
U64 = 2 ** 64


def oracle_sessions(keys, dec_prefix=O.CLIENT_PREFIX, enc_prefix=O.CLIENT_PREFIX):
    """keys: (S, 32) uint8.  The oracle's session array, vectorised."""
    s = np.zeros(len(keys), O.SESSION_DTYPE)
    s["precom"] = keys
    s["enc_prefix"] = np.frombuffer(enc_prefix, np.uint8)
    s["dec_prefix"] = np.frombuffer(dec_prefix, np.uint8)
    return s


def session_keys(S, seed=0):
    return np.random.default_rng(9000 + 31 * S + seed).integers(0, 256, (S, 32), dtype=np.uint8)


def regions_mask(size, start, length):
    """bool[size]: the union of [start, start + length) (vectorised)."""
    d = np.zeros(size + 1, np.int64)
    np.add.at(d, np.asarray(start, np.int64), 1)
    np.add.at(d, np.asarray(start, np.int64) + np.asarray(length, np.int64), -1)
    return np.cumsum(d)[:size] > 0


class Batch:
    """One decode call: n frames over a ctx of S sessions."""

    def __init__(self, name, S, n, seed=0, bg=8, first=(), real=None, max_len=0):
        self.name, self.S, self.n, self.max_len = name, S, n, max_len
        self.rng = np.random.default_rng(1000003 * S + 7 * n + seed)
        bg = min(bg, S - 1)
        self.bg = [s for s in range(S - 1, -1, -1) if s not in first][:bg][::-1]
        self.pool = list(first) + [s for s in range(S) if s not in self.bg and s not in first]
        self.sid = np.full(n, -1, np.int64)
        self.op = np.zeros(n, np.uint8)
        self.nonce = np.zeros(n, np.uint64)
        self.size = {}      # payload sizes that are not random
        self.tamper = {}    # i -> "tag" | "sig" | "short" | "over"
        self.bad = {}       # i -> an unknown sid (>= S)
        self.want = {}      # i -> the status the frame was built for
        self.marks = []     # (kind, indices, note)
        self.peer0 = np.full(S, 2, np.uint64)
        self.real = None if real is None else set(int(i) for i in real)
        self._built = self._exp = None

    # ---- placing frames
    def session(self, peer0=2):
        s = self.pool.pop(0)
        self.peer0[s] = peer0
        return s

    def put(self, i, s, nonce, want, size=None, tamper=None):
        assert 0 <= i < self.n and self.sid[i] == -1, (self.name, i)
        self.sid[i], self.op[i], self.nonce[i], self.want[i] = s, FIXED, np.uint64(nonce % U64), want
        if size is not None:
            self.size[i] = size
        if tamper:
            self.tamper[i] = tamper
        if self.real is not None:
            self.real.add(i)

    def auto(self, i, s, op):
        """A frame of a shared session: rising, or a replay of the session's running maximum."""
        assert self.sid[i] == -1, (self.name, i)
        self.sid[i], self.op[i] = s, op
        if self.real is not None:
            self.real.add(i)

    def unknown(self, i, value):
        assert value >= self.S
        self.put(i, 0, 5, ERR_SESSION)
        self.bad[i] = value

    def fits(self, *idx):
        return all(0 <= i < self.n for i in idx)

    def kill(self, i, j, N=1000, s=None, eq=True, note=""):
        if not self.fits(i, j):
            return False
        s = self.session() if s is None else s
        self.put(i, s, N, OK)
        self.put(j, s, N if eq else N - 1, SEQ)
        self.marks.append(("kill", (i, j), note))
        return True

    def keep(self, i, j, k, N=1000, note=""):
        if not self.fits(i, j, k):
            return False
        s = self.session()
        for x, v in ((i, N), (j, N + 1), (k, N + 7)):
            self.put(x, s, v, OK)
        self.marks.append(("keep", (i, j, k), note))
        return True

    # ---- the frames
    def build(self):
        if self._built:
            return self._built
        n, rng, S = self.n, self.rng, self.S
        real = np.arange(n) if self.real is None else np.array(sorted(self.real), np.int64)
        free = real[self.sid[real] == -1]
        self.sid[free] = rng.choice(self.bg, len(free))
        self.op[free] = np.where(rng.random(len(free)) < 0.1, REPLAY, RISE)
        cur = {}
        want = np.full(n, MALFORMED_UNSPEC, np.int64)  # (a frame that is not real is empty)
        step = rng.integers(1, 4, len(real))
        for r, i in enumerate(real.tolist()):
            op = self.op[i]
            if op == FIXED:
                want[i] = self.want[i]
                continue
            s = int(self.sid[i])
            c = cur.get(s, int(self.peer0[s]))
            if op == RISE:
                c += int(step[r])
                self.nonce[i], want[i], cur[s] = c, OK, c
            else:
                self.nonce[i], want[i] = max(c - int(step[r]) + 1, 0), SEQ
        size = np.zeros(n, np.int64)
        size[real] = rng.integers(0, 41, len(real))
        for i, z in self.size.items():
            size[i] = z
        flags = np.zeros(n, np.uint8)
        flags[real] = rng.choice([0, 1, 3], len(real))
        assert all(O.wire_size(f, 0, 9) == 42 for f in (0, 1, 3))
        wl = np.zeros(n, np.int64)
        wl[real] = size[real] + 33
        gap = np.zeros(n, np.int64)
        gap[real] = rng.integers(0, 4, len(real))
        woff = np.zeros(n, np.int64)
        woff[real] = 40 + np.cumsum(wl[real] + gap[real]) - wl[real]
        total = int(woff[real[-1]] + wl[real[-1]]) + 64 if len(real) else 64
        in_off = np.zeros(n, np.int64)
        in_off[real] = np.cumsum(size[real]) - size[real]
        pay = rng.integers(0, 256, int(size.sum()) + 1, dtype=np.uint8)
        self.keys = session_keys(S)
        wire = O.encode_batch(oracle_sessions(self.keys), self.sid[real], self.nonce[real], flags[real], in_off[real],
                              size[real], pay, woff[real], total)
        for i, kind in self.tamper.items():
            a = int(woff[i])
            if kind == "tag":
                wire[a + int(wl[i]) - 1] ^= 0x10
            elif kind == "sig":
                wire[a + 1] ^= 0xFF
            elif kind == "short":
                wl[i] = 20
            else:
                assert kind == "over" and wl[i] > self.max_len > 0
        if self.max_len:
            assert all(wl[i] <= self.max_len or self.tamper.get(i) == "over" for i in real.tolist())
        # every frame's payload region in `out`, three sentinel bytes apart
        plen = np.maximum(wl - 33, 0)
        pout = np.cumsum(plen + 3) - plen
        sid_dev = self.sid.copy()
        sid_dev[sid_dev < 0] = rng.choice(self.bg, int((sid_dev < 0).sum()))  # (the empty frames)
        for i, v in self.bad.items():
            sid_dev[i] = v
        skip = np.zeros(n, bool)  # frames the call does not process: not in the oracle's batch
        skip[np.array(list(self.bad) + [i for i, k in self.tamper.items() if k == "over"], np.int64)] = True
        self._built = dict(n=n, real=real, want=want, wire=wire, woff=woff.astype(np.uint64), wl=wl.astype(np.uint32),
                           pout=pout.astype(np.uint64), plen=plen, out_size=int(pout[-1] + plen[-1]) + 8 if n else 8,
                           sid_dev=sid_dev.astype(np.uint32), skip=skip, size=size, flags=flags)
        return self._built

    def expected(self):
        """The oracle's sequential decode of the frames the call processes."""
        if self._exp:
            return self._exp
        b = self.build()
        keep = ~b["skip"]
        peer = self.peer0.copy()
        sid = b["sid_dev"][keep]
        out, fl, st = O.decode_batch(oracle_sessions(self.keys), peer, sid, b["woff"][keep], b["wl"][keep], b["wire"],
                                     b["pout"][keep], b["out_size"])
        status = np.zeros(self.n, np.int64)
        flags = np.zeros(self.n, np.uint8)
        status[keep], flags[keep] = st.astype(np.int64) & 0xFFFFFFFF, fl
        for i, v in self.bad.items():
            status[i] = ERR_SESSION
        for i, k in self.tamper.items():
            if k == "over":
                status[i] = ERR_BOUND
        # regions the call writes: every frame of 33 bytes or more but the ones above max_len
        # (an unknown session's region is zero-filled like a header failure's, include/zmqg_curve.h)
        writes = (b["wl"] >= 33) & (status != ERR_BOUND)
        mask = regions_mask(b["out_size"], b["pout"][writes], b["plen"][writes])
        bad = np.array(sorted(self.bad), np.int64)
        if len(bad):  # (the oracle never saw them: its buffer is zero there)
            assert not out[regions_mask(b["out_size"], b["pout"][bad], b["plen"][bad])].any()
        exp_out = np.where(mask, out, np.uint8(SENTINEL))
        hv = np.isin(st.astype(np.int64) & 0xFFFFFFFF, [OK, CRYPTO, SEQ])
        smax = np.zeros(self.S, np.uint64)
        wire_nonce = self.nonce[keep]
        np.maximum.at(smax, sid[hv].astype(np.int64), wire_nonce[hv])
        self._exp = dict(status=status, flags=flags, out=exp_out, peer=peer, smax=smax, hv_sid=sid[hv],
                         hv_nonce=wire_nonce[hv], hv_index=np.flatnonzero(keep)[hv])
        return self._exp

    def tables_input(self):
        """(sid, v) as the frame kernel hands them to the tables, from the
        oracle's statuses: v = the nonce of a header-valid frame, else 0."""
        e = self.expected()
        v = np.zeros(self.n, np.uint64)
        v[e["hv_index"]] = e["hv_nonce"]
        return self.build()["sid_dev"], v


# ------------------------------------------------------------------ class `tile`
TILE_S, TILE_FULL = 256, 129 * T256 + 1


@functools.lru_cache(maxsize=None)
def tile_batch(n):
    """S = 256 (T = 256): pairs at the tile edge, the two row-block edges and
    the last tile; a pair over a row block with nothing of it; cut to n."""
    T = T256
    b = Batch("tile%d" % n, TILE_S, n, bg=8)
    for k in (1, 64, 65, 128, 129):
        b.kill(k * T - 1, k * T, N=1000 + k, eq=k % 2 == 0, note="edge%d" % k)
        b.keep(k * T - 2, k * T + 1, k * T + 2, note="edge%d" % k)
    b.kill(5, 128 * T + 7, note="tile0-tile128")      # nothing of the session in row block 1
    b.keep(9, 64 * T + 9, 128 * T + 9, note="blocks0-1-2")
    b.kill(63 * T + 10, 64 * T + 20, note="tile63-tile64")
    b.kill(3, 40, note="tile0")
    if n == 1:
        b.put(0, b.session(), 3, OK)
    return b


def class_tile():
    """The full batch, one row block (r1 == tiles), a last block of one row, n = T, T + 1 and 1."""
    return [tile_batch(n) for n in (TILE_FULL, 64 * T256, 65 * T256, T256, T256 + 1, 1)]


# ------------------------------------------------------------------ class `step`
def _first(S):
    return (8192,) if S > 8192 else ()


@functools.lru_cache(maxsize=None)
def class_step(S=64):
    """Pairs and whole sessions inside the 64-frame step of k_replay_frames /
    k_nonce_frames (steps start at multiples of 64)."""
    out = []
    for n in (5 * 256 + 63, 5 * 256 + 1):
        b = Batch("step_pairs%d_S%d" % (n, S), S, n, seed=1, bg=8, first=_first(S))
        b.kill(127, 128, note="lanes63|0")
        b.kill(192, 193, note="lanes0,1")
        b.kill(320, 383, eq=False, note="lanes0,63")
        b.kill(384 + 62, 384 + 63, note="lanes62,63")
        b.keep(448, 449, 511, note="lanes0,1,63")
        b.keep(512 + 61, 512 + 62, 512 + 63, note="lanes61,62,63")
        b.keep(639, 640, 641, note="lanes63|0,1")
        for lo, bad in ((3, S), (20, S + 1), (40, 0xFFFFFFFF)):  # an unknown session between the two lanes
            b.kill(704 + lo, 704 + lo + 6, note="unknown-between")
            b.unknown(704 + lo + 3, bad)
        s = b.session()  # a forged header of the same session between the two lanes
        b.put(768 + 4, s, 700, OK)
        b.put(768 + 8, s, 2 ** 40, UNEXPECTED, tamper="sig")
        b.put(768 + 12, s, 700, SEQ)
        b.marks.append(("kill", (768 + 4, 768 + 12), "forged-between"))
        if n % 64 == 63:
            b.kill(1280 + 10, 1280 + 62, note="last-step-of-63")
        else:
            b.kill(1279, 1280, note="last-step-of-1")
        out.append(b)
    n = 5 * 256 + 63
    b = Batch("step_full_S%d" % S, S, n, seed=2, bg=8, first=_first(S))
    lanes = np.arange(64)
    runs = dict(rising=(2, 100 + 3 * lanes, [OK] * 64),
                replay_mid=(4, np.where(lanes == 30, 100 + 29, 100 + lanes), [SEQ if l == 30 else OK for l in lanes]),
                falling=(6, 500 - lanes, [OK] + [SEQ] * 63), equal=(8, np.full(64, 77), [OK] + [SEQ] * 63))
    for name, (g, nonce, want) in runs.items():
        s = b.session()
        for l in range(64):
            b.put(64 * g + l, s, int(nonce[l]), want[l])
        b.marks.append(("full", tuple(range(64 * g, 64 * g + 64)), name))
    s0, s1 = b.session(), b.session()  # two sessions interleaved over a step, a replay in each
    for l in range(64):
        k = l // 2
        v, w = (200 + k, OK) if k != 9 + (l % 2) * 11 else (200 + k - 1, SEQ)
        b.put(64 * 10 + l, (s0, s1)[l % 2], v, w)
    b.marks.append(("interleaved", tuple(range(640, 704)), "2x32"))
    out.append(b)
    # 32 sessions with two lanes each, shared with the background
    b = Batch("step_32x2_S%d" % S, S, n, seed=3, bg=40)
    for g in (3, 11):
        order = b.rng.permutation(32)
        for l in range(64):
            k = int(order[l % 32])
            b.auto(64 * g + l, b.bg[k], RISE if l < 32 or (k + g) % 2 else REPLAY)
        b.marks.append(("pairs32", tuple(range(64 * g, 64 * g + 64)), "32x2"))
    out.append(b)
    # 62 sessions with one lane each and one session with two
    b = Batch("step_62dup_S%d" % S, S, n, seed=4, bg=1)
    sess = [b.session() for _ in range(63)]
    for g, eq in ((3, True), (12, False)):
        order = [int(x) for x in b.rng.permutation(62)]
        it = iter(order)
        for l in range(64):
            if l in (17, 45):
                b.put(64 * g + l, sess[62], (300 if l == 17 or eq else 301) + 10 * g, OK if l == 17 or not eq else SEQ)
            else:
                b.put(64 * g + l, sess[next(it)], 50 + g, OK)
        b.marks.append(("dup", (64 * g + 17, 64 * g + 45), "kill" if eq else "keep"))
    out.append(b)
    return out


# ------------------------------------------------------------------ class `value`
@functools.lru_cache(maxsize=None)
def class_value():
    S, n = 128, 700
    b = Batch("value", S, n, seed=5, bg=8)
    edges = [(2 ** 32 - 1, 2 ** 32), (2 ** 63 - 1, 2 ** 63), (2 ** 64 - 2, 2 ** 64 - 1)]
    for k, (lo, hi) in enumerate(edges):
        for base, far in ((64 + 8 * k, 3), (250 + k, 6), (509 + k, 3)):  # in a step; across 255|256, 511|512
            s = b.session()
            b.put(base, s, lo, OK)
            b.put(base + far, s, hi, OK)
            b.marks.append(("keep", (base, base + far), "%x" % hi))
        for base, far in ((128 + 8 * k, 3), (244 + k, 20), (500 + k, 30)):
            s = b.session()
            b.put(base, s, hi, OK)
            b.put(base + far, s, lo, SEQ)  # (passes if compared in 32 bits, or signed)
            b.marks.append(("kill", (base, base + far), "%x" % hi))
    s = b.session(peer0=0)  # a header-valid frame with nonce 0
    b.put(300, s, 0, SEQ)
    b.put(310, s, 1, OK)
    s = b.session(peer0=10 ** 6)  # the peer nonce above every nonce of the batch
    for i, v in ((320, 10), (330, 20), (340, 15)):
        b.put(i, s, v, SEQ)
    b.high = s
    s = b.session(peer0=500)
    b.put(350, s, 500, SEQ)
    b.put(351, s, 501, OK)
    s = b.session(peer0=499)
    b.put(352, s, 500, OK)
    s = b.session(peer0=2 ** 64 - 2)
    b.put(360, s, 2 ** 64 - 1, OK)
    b.put(365, s, 2 ** 64 - 1, SEQ)
    b.idle = [b.session(peer0=77 + k) for k in range(5)]  # no frame in the batch
    return [b]


# ------------------------------------------------------------------ class `status`
@functools.lru_cache(maxsize=None)
def class_status(S=256):
    """Kill pairs (and the big frame's keep triple) whose members have other
    statuses, each across a tile edge (T = 256) and inside one step."""
    T = T256
    b = Batch("status_S%d" % S, S, 7 * T + 17, seed=6, bg=8, first=_first(S))
    variants = ("tag_a", "sig_a", "short_a", "both_b", "big_kill", "big_keep")
    for k, var in enumerate(variants):
        for where, (i, j, m) in (("tile", ((k + 1) * T - 2, (k + 1) * T + 1, (k + 1) * T + 3)),
                                 ("step", ((k + 1) * T + 64 + 7, (k + 1) * T + 64 + 23, (k + 1) * T + 64 + 40))):
            s, N = b.session(), 900 + k
            if var == "tag_a":  # a MAC failure still advances the peer nonce
                b.put(i, s, N, CRYPTO, tamper="tag")
                b.put(j, s, N, SEQ)
            elif var == "sig_a":  # a forged header does not
                b.put(i, s, N + 5, UNEXPECTED, tamper="sig")
                b.put(j, s, N, OK)
            elif var == "short_a":  # nor does a frame shorter than 33 bytes
                b.put(i, s, N + 5, MALFORMED_MSG, tamper="short")
                b.put(j, s, N, OK)
            elif var == "both_b":  # a replay that is tampered too: the nonce is checked first
                b.put(i, s, N, OK)
                b.put(j, s, N, SEQ, tamper="tag", size=20)
            elif var == "big_kill":
                b.put(i, s, N, OK)
                b.put(j, s, N, SEQ, size=BIG)
            else:
                b.put(i, s, N, OK)
                b.put(j, s, N + 1, OK, size=BIG)
                b.put(m, s, N + 7, OK)
            b.marks.append((var, (i, j), where))
    c = Batch("status_bound_S%d" % S, S, 2 * T + 17, seed=7, bg=8, first=_first(S), max_len=300)
    for where, (i, j) in (("tile", (T - 2, T + 1)), ("step", (T + 64 + 7, T + 64 + 23))):
        s = c.session()  # above max_len with a huge nonce in its header: not processed
        c.put(i, s, 2 ** 60, ERR_BOUND, size=400, tamper="over")
        c.put(j, s, 5, OK)
        c.marks.append(("over_a", (i, j), where))
    return [b, c]


# ------------------------------------------------------------------ class `geometry`
GEO_BIG_N = 4096 * 256 + 1


@functools.lru_cache(maxsize=None)
def geometry_257():
    b = Batch("geo_S257", 257, 3 * 512 + 5, seed=8, bg=8)
    b.kill(511, 512, note="T512")
    b.keep(255, 256, 300, note="inside-T512")
    b.kill(1023, 1024, eq=False, note="T512")
    b.keep(1022, 1025, 1536, note="T512")
    return b


@functools.lru_cache(maxsize=None)
def geometry_8192():
    T = 8192
    b = Batch("geo_S8192", 8192, 2 * T + 1, seed=9, bg=8, first=(0, 255, 256, 8191))
    b.kill(T - 1, T, note="T8192")            # session 0
    b.keep(T - 2, T + 1, T + 2, note="T8192")  # session 255
    b.kill(2 * T - 1, 2 * T, note="T8192")    # session 256
    b.kill(5, 2 * T - 3, note="tile0-tile1")  # session 8191
    return b


@functools.lru_cache(maxsize=None)
def geometry_big():
    """S = 8 over 4096 * 256 + 1 frames: more than kReplayMaxTiles tiles of 256,
    so T = 512.  About 4,000 real frames; the others are empty."""
    n = GEO_BIG_N
    rng = np.random.default_rng(10)
    b = Batch("geo_S8_T512", 8, n, seed=10, bg=3, real=rng.choice(n, 4000, replace=False))
    b.kill(511, 512, note="T512")
    b.keep(510, 513, 514, note="T512")
    b.kill(n - 2, n - 1, note="last")
    b.kill(100, n - 5, note="far")
    b.keep(255, 256, 257, note="inside-T512")
    return b


# ------------------------------------------------------------------ class `sort`
SORT_S = 8193


@functools.lru_cache(maxsize=None)
def class_sort_unknown():
    """The sort fallback: a kill pair with a frame of an unknown session
    between its members whose low bits are the pair's session id."""
    out = []
    for s, bad in ((0, 16384), (0, 8193 + 8192), (0, 2 ** 31), (0, 0xFFFFFFFF), (1, 16385)):
        b = Batch("sort_s%d_bad%x" % (s, bad), SORT_S, 300, seed=bad % 1000, bg=8, first=(8192, 0, 1))
        assert b.session() == 8192
        b.put(10, 8192, 9, OK)
        b.pool = b.pool[2:]
        b.kill(100, 140, N=50, s=s, note="unknown-between")
        b.unknown(120, bad)
        b.kill(200, 203, N=60, eq=False, s=1 - s, note="step")
        b.unknown(201, bad)
        out.append(b)
    return out


def class_sort():
    return class_step(SORT_S) + class_status(SORT_S) + class_sort_unknown()


# ------------------------------------------------------------------ class `nonce`
class EncodeCase:
    """One ZMQG_OPT_NONCE_AUTO encode: sid pattern, payloads of 0 to 16 bytes."""

    def __init__(self, name, S, sid, send0=None, max_len=0, over=(), seed=0, size_hi=17):
        self.name, self.S, self.n, self.max_len = name, S, len(sid), max_len
        self.sid = np.asarray(sid, np.uint32)
        rng = np.random.default_rng(77 + seed + self.n)
        self.size = rng.integers(0, size_hi, self.n).astype(np.uint32)
        self.over = np.zeros(self.n, bool)
        for i in over:
            self.size[i], self.over[i] = max_len + 10, True
        assert not max_len or ((self.size > max_len) == self.over).all()
        self.flags = rng.choice([0, 1], self.n).astype(np.uint8)
        self.in_off = (np.cumsum(self.size.astype(np.int64)) - self.size).astype(np.uint64)
        self.pay = rng.integers(0, 256, int(self.size.sum()) + 1, dtype=np.uint8)
        wl = self.size.astype(np.int64) + 33
        self.wl = wl
        self.woff = (np.cumsum(wl + 2) - wl).astype(np.uint64)
        self.total = int(self.woff[-1]) + int(wl[-1]) + 16
        self.send0 = np.ones(S, np.uint64) if send0 is None else np.asarray(send0, np.uint64)
        self.keys = session_keys(S)

    def expected(self, send=None):
        """One counter per session, taken in batch order by every frame of a
        known session (one above max_len included: it leaves a gap); the wire
        is the oracle's encode with those nonces."""
        send = self.send0 if send is None else send
        known = self.sid < self.S
        idx = np.flatnonzero(known)
        order = idx[np.argsort(self.sid[idx], kind="stable")]
        ss = self.sid[order].astype(np.int64)
        start = np.flatnonzero(np.r_[True, ss[1:] != ss[:-1]]) if len(ss) else np.zeros(0, np.int64)
        rank = np.arange(len(ss)) - np.repeat(start, np.diff(np.r_[start, len(ss)]))
        nonce = np.zeros(self.n, np.uint64)
        nonce[order] = send[ss] + rank.astype(np.uint64)  # (mod 2^64)
        after = send.copy()
        after[ss[start]] += np.diff(np.r_[start, len(ss)]).astype(np.uint64)
        proc = known & ~self.over
        p = np.flatnonzero(proc)
        wire = O.encode_batch(oracle_sessions(self.keys), self.sid[p], nonce[p], self.flags[p], self.in_off[p],
                              self.size[p], self.pay, self.woff[p], self.total)
        mask = regions_mask(self.total, self.woff[p], self.wl[p])
        status = np.where(~known, ERR_SESSION, np.where(self.over, ERR_BOUND, 0)).astype(np.int64)
        return dict(wire=np.where(mask, wire, np.uint8(SENTINEL)), status=status, send=after, nonce=nonce, known=known)


def _send0(b):
    s = np.ones(b.S, np.uint64)
    s[b.bg[0]] = 2 ** 32 - 2
    if len(b.bg) > 1:
        s[b.bg[1]] = 2 ** 63 - 2
    return s


def _from_batch(b, **kw):
    return EncodeCase("nonce_" + b.name, b.S, b.build()["sid_dev"], _send0(b), **kw)


@functools.lru_cache(maxsize=None)
def nonce_tile():
    return _from_batch(tile_batch(TILE_FULL))


@functools.lru_cache(maxsize=None)
def nonce_step():
    cases = [_from_batch(b) for b in class_step(64)]
    # a frame above max_len inside a run of its session: it takes its nonce
    sid = np.random.default_rng(5).integers(0, 64, 300)
    sid[100:111] = 7
    cases.append(EncodeCase("nonce_over_S64", 64, sid, max_len=64, over=(105,), size_hi=17))
    cases.append(EncodeCase("nonce_over_S1", 1, np.zeros(200, np.int64), np.array([2 ** 32 - 50], np.uint64),
                            max_len=64, over=(60,)))
    return cases


@functools.lru_cache(maxsize=None)
def nonce_geometry(which):
    if which == "big":  # every frame real here: empty payloads
        b = geometry_big()
        return EncodeCase("nonce_geo_S8_T512", 8, b.build()["sid_dev"], _send0(b), size_hi=1)
    return _from_batch(geometry_257() if which == 257 else geometry_8192())


# zmqg_encode_zmtp_multi with nonce == NULL: max_sessions = 8192 and T = 256 < S
SEND_MULTI_S = 8192
SEND_MULTI_STREAM_SID = [0, 255, 256, 8191, 4000, 255]  # streams 1 and 5 share session 255


@functools.lru_cache(maxsize=None)
def send_multi_case():
    """About 600 frames over six sessions' streams: three tiles of 256, pairs of
    one session across 255 | 256 and 511 | 512."""
    rng = np.random.default_rng(600)
    n = 2 * 256 + 90
    fs = rng.integers(0, 6, n).astype(np.uint32)
    fs[[255, 256]] = 1        # session 255, one stream
    fs[[254, 257]] = (5, 1)   # session 255 through two streams
    fs[[511, 512]] = 5        # the stream that does not fit
    fs[[510, 513]] = 3
    lens = rng.integers(0, 17, n).astype(np.uint32)
    flags = rng.choice([0, 1], n).astype(np.uint8)
    payloads = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in lens]
    send = {0: 2 ** 32 - 2, 255: 2 ** 63 - 2, 256: 1, 8191: 2 ** 32 - 40, 4000: 5}
    return dict(n=n, frame_stream=fs, lens=lens, flags=flags, payloads=payloads, nonce=None, send=send)
