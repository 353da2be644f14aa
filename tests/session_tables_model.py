"""Plain model of the per-session tables behind every multi-session call
(libzmq_amd/csrc/zmqg_curve.hip: k_replay_tiles / _colblk / _colscan /
_frames, k_nonce_tiles / _colblk / _colscan / _frames) -- test infrastructure,
not a test.  Geometry: where a frame index lands (tile, row block, 64-frame
step, lane).  Emulation: the four kernels of each table restated step by step
over (sid, v) alone, with no cryptography, so that tests/test_session_tables_model.py
can show that the steered batches of tests/session_tables_steer.py reach the
seams -- each named mutation of this emulation (MUTATIONS) must make a steered
case disagree with the oracle.  The GPU test takes no expected value from here.
"""
import functools

import numpy as np

STEP = 64  # one wave walks a tile 64 frames at a time
M64 = 2 ** 64 - 1

MUTATIONS = ("blkprefix_short", "colscan_inclusive", "tile_end_short", "tile_end_long", "dup_ignored", "dup_all_lanes",
             "lane0_self", "update_before_read", "cmp32", "cmp_signed", "popcount_all", "update_by_one")


# ------------------------------------------------------------------ geometry
@functools.lru_cache(maxsize=None)
def K():
    """The kernels' constants as the binding mirrors them (imported late: the
    library loads after torch has loaded the HIP runtime, as in every GPU test)."""
    from libzmq_amd import curve
    assert curve.REPLAY_TILE_MIN % STEP == 0
    return dict(TILE_MIN=curve.REPLAY_TILE_MIN, RB=curve.REPLAY_ROW_BLOCK, MAX_TILES=curve.REPLAY_MAX_TILES,
                MAX_SESSIONS=curve.REPLAY_MAX_SESSIONS, ZSEND_MAX_TILES=curve.ZSEND_MAX_TILES)


def tile_frames(n, S):
    """replay_tile_frames: frames per tile for n frames and S sessions."""
    T = K()["TILE_MIN"]
    while T < S:
        T *= 2
    while (n + T - 1) // T > K()["MAX_TILES"]:
        T *= 2
    return T


def zsend_tile_frames(n, keys):
    """zsend_tile_frames: the send side's tile (zmqg_encode_zmtp_multi hands it to the nonce tables)."""
    T = K()["TILE_MIN"]
    while True:
        tiles = (n + T - 1) // T
        if tiles <= K()["ZSEND_MAX_TILES"] and tiles * keys <= (4 << 20):
            return T
        T *= 2


def locate(i, n, S, T=None):
    """(tile, row block, step within the tile, lane) of frame i."""
    T = T or tile_frames(n, S)
    assert 0 <= i < n and T % STEP == 0
    t = i // T
    return t, t // K()["RB"], (i - t * T) // STEP, i % STEP


def _gt(mut):
    if mut == "cmp32":
        return lambda a, b: (a & 0xFFFFFFFF) > (b & 0xFFFFFFFF)
    if mut == "cmp_signed":
        sg = lambda x: x - 2 ** 64 if x >> 63 else x
        return lambda a, b: sg(a) > sg(b)
    return lambda a, b: a > b


def _tile_ends(n, T, tiles, mut):
    """[b, e) of each tile as the *_tiles kernel sees it."""
    out = []
    for t in range(tiles):
        b, e = t * T, min(t * T + T, n)
        if mut == "tile_end_short":
            e -= 1
        elif mut == "tile_end_long":
            e = min(e + 1, n)
        out.append((b, e))
    return out


def _columns(tiles, col, start, join, mut):
    """k_*_colblk + k_*_colscan for one session: col[t] (the tile's own
    value) -> (the exclusive prefix per tile, the total)."""
    RB = K()["RB"]
    rbs = (tiles + RB - 1) // RB
    blk = []
    for rb in range(rbs):
        m = None
        for r in range(rb * RB, min(rb * RB + RB, tiles)):
            m = col[r] if m is None else join(m, col[r])
        blk.append(m)
    pre, total = [None] * tiles, start
    for rb in range(rbs):
        m = start
        for k in range(rb - 1 if mut == "blkprefix_short" and rb else rb):
            m = join(m, blk[k])
        for r in range(rb * RB, min(rb * RB + RB, tiles)):
            x = col[r]
            pre[r] = join(m, x) if mut == "colscan_inclusive" else m
            m = join(m, x)
        if min(rb * RB + RB, tiles) == tiles:
            total = m
    return pre, total


# ------------------------------------------------------------------ replay tables
def replay(sid, v, S, peer, mut=None, T=None):
    """sid, v: per frame, the session and the header-valid nonce (0: none).
    peer: the S peer nonces before the batch.  Returns dict(excl, passes, peer,
    smax): excl[i] the tables' exclusive max (only meaningful where v[i] != 0),
    passes[i] the replay verdict v > max(excl, peer before), the peer nonces
    and session maxima afterwards."""
    n = len(sid)
    T = T or tile_frames(n, S)
    tiles = (n + T - 1) // T
    gt = _gt(mut)
    mx = lambda a, b: b if gt(b, a) else a
    nz = np.flatnonzero((np.asarray(v) != 0) & (np.asarray(sid) < S)).tolist()
    sof = dict(zip(nz, np.asarray(sid)[nz].tolist())).__getitem__
    vof = dict(zip(nz, np.asarray(v)[nz].tolist())).__getitem__
    # k_replay_tiles
    own = {}
    ends = _tile_ends(n, T, tiles, mut)
    for i in nz:
        for t in {i // T, (i - 1) // T if i else 0}:  # (tile_end_long reaches one frame into the next tile)
            if ends[t][0] <= i < ends[t][1]:
                k = (t, sof(i))
                own[k] = mx(own.get(k, 0), vof(i))
    # k_replay_colblk, k_replay_colscan
    sessions = sorted({k[1] for k in own})
    pre, smax = {}, [0] * S
    peer_after = [int(x) for x in peer]
    for s in sessions:
        p, total = _columns(tiles, [own.get((t, s), 0) for t in range(tiles)], 0, mx, mut)
        for t in range(tiles):
            pre[(t, s)] = p[t]
        smax[s] = total
        if gt(total, peer_after[s]):
            peer_after[s] = total
    # k_replay_frames: the steps that hold a nonce (the others change nothing)
    excl = [0] * n
    steps = {}
    for i in nz:
        steps.setdefault(i // STEP, []).append(i)
    cur_tile, table = -1, {}
    for st in sorted(steps):
        t = st * STEP // T
        if t != cur_tile:
            cur_tile, table = t, {}
        lanes = steps[st]
        get = lambda s: table.get(s, pre.get((t, s), 0))
        if mut == "update_before_read":
            for i in lanes:
                table[sof(i)] = mx(get(sof(i)), vof(i))
        for i in lanes:
            s, x = sof(i), get(sof(i))
            group = [j for j in lanes if sof(j) == s]
            if len(group) > 1 and mut != "dup_ignored":
                if mut == "dup_all_lanes":
                    earlier = group
                else:
                    earlier = [j for j in group if j < i]
                    if mut == "lane0_self" and i % STEP == 0:
                        earlier = [i]
                for j in earlier:
                    x = mx(x, vof(j))
            excl[i] = x
        if mut != "update_before_read":
            for i in lanes:
                table[sof(i)] = mx(get(sof(i)), vof(i))
    passes = {}
    for i in nz:
        prev = mx(excl[i], int(peer[sof(i)]))
        passes[i] = gt(vof(i), prev)
    return dict(excl=excl, passes=passes, peer=peer_after, smax=smax)


# ------------------------------------------------------------------ send nonces
def nonces(sid, S, send, mut=None, T=None):
    """sid per frame, send: the S counters before the call.  Returns
    dict(nonce, send): nonce[i] of each frame with sid < S (None otherwise) and
    the counters afterwards, all mod 2^64."""
    n = len(sid)
    T = T or tile_frames(n, S)
    tiles = (n + T - 1) // T
    sid = np.asarray(sid)
    inn = np.flatnonzero(sid < S).tolist()
    sof = sid.tolist().__getitem__
    add = lambda a, b: (a + b) & M64
    own = {}
    ends = _tile_ends(n, T, tiles, mut)
    for i in inn:
        t = i // T
        if i < ends[t][1]:
            own[(t, sof(i))] = own.get((t, sof(i)), 0) + 1
        if t and i < ends[t - 1][1]:  # (tile_end_long reaches one frame into the next tile)
            own[(t - 1, sof(i))] = own.get((t - 1, sof(i)), 0) + 1
    pre, after = {}, [int(x) for x in send]
    for s in sorted({k[1] for k in own}):
        p, total = _columns(tiles, [own.get((t, s), 0) for t in range(tiles)], int(send[s]), add, mut)
        for t in range(tiles):
            pre[(t, s)] = p[t]
        after[s] = total
    out = [None] * n
    steps = {}
    for i in inn:
        steps.setdefault(i // STEP, []).append(i)
    cur_tile, table = -1, {}
    for st in sorted(steps):
        t = st * STEP // T
        if t != cur_tile:
            cur_tile, table = t, {}
        groups = {}  # one session per round, its lanes in lane (= batch) order
        for j in steps[st]:
            groups.setdefault(sof(j), []).append(j)
        for s, group in groups.items():
            base = table.get(s, pre.get((t, s), int(send[s])))
            for below, j in enumerate(group):
                out[j] = add(base, len(group) if mut == "popcount_all" else below)
            table[s] = add(base, 1 if mut == "update_by_one" else len(group))
    return dict(nonce=out, send=after)
