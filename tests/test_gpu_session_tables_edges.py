"""The per-session tables behind every multi-session call -- the replay prefix
(k_replay_* with k_fixup, the sort fallback above 8,192 sessions) and the send
nonces (k_nonce_*) -- over the steered batches of tests/session_tables_steer.py:
kill pairs and keep triples at the 64-frame step, the tile, the 64-tile row
block, the tile-count cap and the session-count limit, nonce values at 2^32,
2^63 and 2^64 - 1, frames of every status between a pair, every frame-kernel
variant.  That the batches reach those seams is asserted on the CPU
(tests/test_session_tables_model.py); here every expected value comes from the
oracle (oracle.decode_batch, oracle.encode_batch), never from the model:
statuses, flags, the whole output buffer (payloads, zero fills, sentinels),
every session's peer nonce and session_max_out, bit-exact; for the encodes the
whole wire buffer, status_out and the counters."""
import numpy as np
import pytest

from tests import session_tables_steer as S
from tests.session_tables_model import locate, tile_frames

pytestmark = pytest.mark.gpu


def _t(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to("cuda")


class Dev:
    """One ctx of S sessions; all of them are installed again before each
    batch (one zmqg_session_set_batch), with the batch's peer nonces / counters."""

    def __init__(self, torch, C, S_):
        self.torch, self.C, self.S = torch, C, S_
        self.ctx = C.CurveContext(0, S_)
        self.keys = S.session_keys(S_)
        self.d_keys = _t(torch, self.keys)

    def install(self, keys, peer=None, send=None):
        assert (keys == self.keys).all()
        self.ctx.session_set_batch(np.arange(self.S, dtype=np.uint32), self.d_keys, self.C.CLIENT_PREFIX,
                                   self.C.CLIENT_PREFIX, peer_nonce=peer, send_nonce=send)

    def peers(self, which=None):
        which = range(self.S) if which is None else which
        return np.array([self.ctx.get_peer_nonce(int(s)) for s in which], np.uint64)

    def counters(self, which):
        return np.array([self.ctx.get_nonce(int(s)) for s in which], np.uint64)

    def decode(self, b):
        torch = self.torch
        bb, e = b.build(), b.expected()
        self.install(b.keys, peer=b.peer0)
        n = b.n
        out = torch.full((bb["out_size"],), S.SENTINEL, dtype=torch.uint8, device="cuda")
        fl = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        smax = torch.full((self.S,), -1, dtype=torch.int64, device="cuda")
        self.ctx.decode_batch(_t(torch, bb["sid_dev"]), _t(torch, bb["woff"]), _t(torch, bb["wl"]),
                              _t(torch, bb["wire"]), _t(torch, bb["pout"]), out, fl, st, max_len=b.max_len,
                              session_max_out=smax)
        torch.cuda.synchronize()
        got_st = st.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        bad = np.flatnonzero(got_st != e["status"])
        assert bad.size == 0, (b.name, "status", bad[:8].tolist(), [hex(x) for x in got_st[bad[:8]]],
                               [hex(x) for x in e["status"][bad[:8]]])
        assert np.array_equal(fl.cpu().numpy(), e["flags"]), (b.name, "flags")
        got = out.cpu().numpy()
        bad = np.flatnonzero(got != e["out"])
        assert bad.size == 0, (b.name, "out", bad[:8].tolist())
        # every session that has a frame, the steered ones' neighbours and a sample of the idle ones
        which = np.unique(np.r_[bb["sid_dev"][bb["sid_dev"] < self.S], np.arange(0, self.S, max(self.S // 64, 1)),
                                self.S - 1]).astype(np.int64)
        which = np.arange(self.S) if self.S <= 1024 else which
        peers = self.peers(which)
        assert np.array_equal(peers, e["peer"][which]), (b.name, "peer", which[peers != e["peer"][which]][:8].tolist(),
                                                         peers[peers != e["peer"][which]][:8].tolist())
        got_smax = smax.cpu().numpy().view(np.uint64)
        assert np.array_equal(got_smax, e["smax"]), (b.name, "smax", np.flatnonzero(got_smax != e["smax"])[:8].tolist())

    def encode(self, cases):
        """The calls queued back to back on the current stream, with no
        synchronisation between them; each starts from the counters the one
        before it left."""
        torch = self.torch
        self.install(cases[0].keys, send=cases[0].send0)
        send, runs = cases[0].send0, []
        for c in cases:
            e = c.expected(send)
            send = e["send"]
            out = torch.full((c.total,), S.SENTINEL, dtype=torch.uint8, device="cuda")
            st = torch.full((c.n,), -1, dtype=torch.int32, device="cuda")
            args = (_t(torch, c.sid), None, _t(torch, c.flags), _t(torch, c.in_off), _t(torch, c.size),
                    _t(torch, c.pay), _t(torch, c.woff), out)
            runs.append((c, e, out, st, args))
        for c, e, out, st, args in runs:
            self.ctx.encode_batch(*args, max_len=c.max_len, status_out=st, nonce_auto=True)
        torch.cuda.synchronize()
        for k, (c, e, out, st, args) in enumerate(runs):
            got_st = st.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
            assert np.array_equal(got_st, e["status"]), (c.name, k, "status")
            bad = np.flatnonzero(out.cpu().numpy() != e["wire"])
            assert bad.size == 0, (c.name, k, "wire", bad[:8].tolist())
        which = np.unique(np.r_[c.sid[c.sid < self.S], 0, self.S - 1]).astype(np.int64)
        which = np.arange(self.S) if self.S <= 1024 else which
        assert np.array_equal(self.counters(which), send[which]), (c.name, "counters")

    def close(self):
        self.ctx.close()


def run_decode(torch, C, cases):
    devs = {}
    for b in cases:
        if b.S not in devs:
            devs[b.S] = Dev(torch, C, b.S)
        devs[b.S].decode(b)
    for d in devs.values():
        d.close()


# ------------------------------------------------------------------ decode
def test_tile_edges(torch_cuda, C):
    """Tile edges, the row-block edges, a row block with nothing of the session,
    a last tile of one frame; the batch cut to one row block, to a last block
    of one row, to T, T + 1 and 1."""
    cases = S.class_tile()
    full = cases[0]
    assert tile_frames(full.n, full.S) == 256 and locate(full.n - 1, full.n, full.S)[:2] == (129, 2)
    run_decode(torch_cuda, C, cases)


VARIANTS = ["", "0", "1", "2", "4", "8"]


def _variant(monkeypatch, G):
    if G:
        monkeypatch.setenv("ZMQG_FRAMES_G", G)


@pytest.mark.parametrize("G", VARIANTS)
def test_tile_row_block_edge_every_frame_kernel(torch_cuda, C, monkeypatch, G):
    """The 65-tile cut under every frame-kernel variant: each writes the tables' inputs itself."""
    _variant(monkeypatch, G)
    run_decode(torch_cuda, C, [S.tile_batch(65 * 256)])


@pytest.mark.parametrize("G", VARIANTS)
def test_step(torch_cuda, C, monkeypatch, G):
    """Pairs at the lanes of one 64-frame step and across two, a session that
    fills a step (rising, one replay, falling, all equal), 2 x 32, 32 x 2,
    62 + a duplicate pair, an unknown session or a forged header between a
    pair's lanes, last steps of 63 lanes and of 1."""
    _variant(monkeypatch, G)
    cases = S.class_step()
    assert locate(128, cases[0].n, 64)[2:] == (2, 0) and [c.n % 64 for c in cases[:2]] == [63, 1]
    run_decode(torch_cuda, C, cases)


@pytest.mark.parametrize("G", VARIANTS)
def test_status(torch_cuda, C, monkeypatch, G):
    """The earlier frame tampered (advances the peer nonce), forged, short or
    above max_len (does not); the later one a tampered replay, or a big frame
    (the body finisher reads excl) -- across a tile edge and inside one step."""
    _variant(monkeypatch, G)
    run_decode(torch_cuda, C, S.class_status())


def test_values(torch_cuda, C):
    """Nonces at 2^32, 2^63 and 2^64 - 1 in both orders, a header-valid nonce 0,
    peer nonces above, at and one below the first nonce, idle sessions."""
    run_decode(torch_cuda, C, S.class_value())


def test_geometry_T512_by_sessions(torch_cuda, C):
    run_decode(torch_cuda, C, [S.geometry_257()])


def test_geometry_8192_sessions(torch_cuda, C):
    """The largest table-path ctx: T = 8192, the kernels' largest dynamic LDS
    (96 KiB in k_replay_frames, 64 KiB in k_replay_tiles)."""
    b = S.geometry_8192()
    assert tile_frames(b.n, b.S) == 8192 and locate(8192, b.n, b.S)[0] == 1
    run_decode(torch_cuda, C, [b])


def test_geometry_T512_by_tile_cap(torch_cuda, C):
    """4096 * 256 + 1 frames (about 4,000 real, the others empty): T doubles to 512."""
    b = S.geometry_big()
    assert tile_frames(b.n, b.S) == 512 and tile_frames(b.n - 1, b.S) == 256
    run_decode(torch_cuda, C, [b])


def test_sort_fallback_step_and_status(torch_cuda, C):
    """8,193 sessions (session 8192 in use): the sort fallback on the step and status batches."""
    run_decode(torch_cuda, C, S.class_step(S.SORT_S) + S.class_status(S.SORT_S))


def test_sort_fallback_unknown_session_between_a_pair(torch_cuda, C):
    """A frame whose sid is not a session's, but whose low bits are, between
    the two frames of a kill pair: it neither joins nor splits the session's
    run (sid 16384, 8193 + 8192, 2^31, 2^32 - 1 against session 0; 16385
    against session 1).  The expected values are the oracle's on the batch
    without those frames."""
    run_decode(torch_cuda, C, S.class_sort_unknown())


# ------------------------------------------------------------------ encode
def run_encode(torch, C, cases, twice=False):
    for c in cases:
        d = Dev(torch, C, c.S)
        d.encode([c, c] if twice else [c])
        d.close()


def test_nonce_tile_edges(torch_cuda, C):
    run_encode(torch_cuda, C, [S.nonce_tile()])


def test_nonce_step(torch_cuda, C):
    """The step layouts as session patterns (unknown sessions inside a step take
    no nonce), counters that start at 2^32 - 2, 2^63 - 2 and 1, and a frame
    above max_len inside a run of its session, with several sessions and with
    one: it takes its nonce and leaves a gap."""
    run_encode(torch_cuda, C, S.nonce_step())


def test_nonce_two_calls_back_to_back(torch_cuda, C):
    """The second call's snapshot of the counters sees the first call's advance."""
    run_encode(torch_cuda, C, [S.nonce_step()[0], S.nonce_geometry(257)], twice=True)


@pytest.mark.parametrize("which", [257, 8192, "big"])
def test_nonce_geometry(torch_cuda, C, which):
    run_encode(torch_cuda, C, [S.nonce_geometry(which)])


def test_nonce_send_multi_tile_below_session_count(torch_cuda, C):
    """zmqg_encode_zmtp_multi with nonce == NULL on a ctx of 8,192 sessions:
    its nonce tables run with T = 256 < S over three tiles; one stream does not
    fit out_bytes, and its frames that do not fit take no nonce."""
    from tests import zmtp_send_model as ZM
    from tests.test_zmtp_send_multi import PAD, _compare, _run, _total
    torch = torch_cuda
    cs = S.send_multi_case()
    d = Dev(torch, C, S.SEND_MULTI_S)
    send0 = np.ones(d.S, np.uint64)
    for s, v in cs["send"].items():
        send0[s] = v
    d.install(d.keys, send=send0)
    precoms, down = [k.tobytes() for k in d.keys], [False] * d.S
    args = (precoms, down, S.SEND_MULTI_STREAM_SID, cs["frame_stream"], None, cs["flags"], cs["lens"], cs["payloads"])
    full = ZM.model(*args, 2 ** 62, 0, send=[int(x) for x in send0], encode=False)
    total, r5 = _total(full), full["results"][5]
    cap = r5["out_off"] + r5["out_bytes"] // 2
    ref = ZM.model(*args, cap, total + PAD, send=[int(x) for x in send0], enc_prefix=C.CLIENT_PREFIX,
                   dec_prefix=C.CLIENT_PREFIX)
    assert 0 < ref["results"][5]["frames"] < full["results"][5]["frames"]
    assert all(ref["fit"][i] for i in (254, 255, 256, 257)) and not all(ref["fit"])
    got = _run(torch, C, precoms, down, S.SEND_MULTI_STREAM_SID, cs, cap, total + PAD, send=True, ctx=d.ctx)
    _compare(got, ref, cap)
    assert got["send"] == ref["send"]
    d.close()
