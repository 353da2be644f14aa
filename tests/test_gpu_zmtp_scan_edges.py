"""zmqg_decode_zmtp / _async over the steered streams of
tests/zmtp_scan_steer.py: signatures and headers at every distance from every
chunk, round and list edge of k_zmtp_scan, the stream's start and every end,
shadows and the early stop, candidate density, links and the walk's paths,
streams of 1,025 and 8,193 lists, size fields and max_msg_size.  That the
streams reach those edges is asserted on the CPU (tests/test_zmtp_scan_model.py,
from the model's coverage facts); here every expected value comes from the
oracle (zmtp_oracle.parse, oracle.decode_batch), never from the model: the
call's result, offsets, lengths, flags, statuses, payload bytes and the
session's peer nonce, bit-exact."""
import functools

import numpy as np
import pytest

from tests import zmtp_scan_steer as S

pytestmark = pytest.mark.gpu


class Dev:
    """One context and one set of device buffers for a class of streams.
    The session is set again before each stream (its key, peer nonce 2)."""

    def __init__(self, torch, C, cap, nbytes):
        self.torch, self.C = torch, C
        dev = torch.device("cuda", 0)
        self.ctx = C.CurveContext(0, 1)
        self.arena = torch.zeros(nbytes + 32, dtype=torch.uint8, device=dev)  # (16-byte aligned, as torch allocates)
        assert self.arena.data_ptr() % 16 == 0
        self.out = torch.empty(nbytes + 32, dtype=torch.uint8, device=dev)
        self.foff = torch.empty(cap, dtype=torch.int64, device=dev)
        self.flen = torch.empty(cap, dtype=torch.int32, device=dev)
        self.poff = torch.empty(cap, dtype=torch.int64, device=dev)
        self.fl = torch.empty(cap, dtype=torch.uint8, device=dev)
        self.st = torch.empty(cap, dtype=torch.int32, device=dev)
        self.res = torch.zeros(4, dtype=torch.int64, device=dev)

    def run(self, cs, stream=None, off=0, use_async=False, reset=True, max_frames=None):
        """One call over `stream` placed at byte `off` of the allocation."""
        torch, C = self.torch, self.C
        s = cs["stream"] if stream is None else stream
        n, mf = len(s), cs["max_frames"] if max_frames is None else max_frames
        if reset:
            self.ctx.session_set(0, cs["precom"], C.SERVER_PREFIX, C.CLIENT_PREFIX, False, S.PEER0)
        d_in = self.arena[off:off + n]
        if n:
            d_in.copy_(torch.from_numpy(np.frombuffer(s, np.uint8).copy()))
        for t in (self.foff, self.flen, self.poff, self.st):
            t.fill_(-1)
        self.fl.fill_(0xEE)
        self.out.fill_(0x77)
        args = (0, d_in, n, cs["max_msg"], mf, self.foff, self.flen, self.poff, self.out, self.fl, self.st)
        if use_async:  # the result read once the stream is done
            self.res.fill_(-1)
            self.ctx.decode_zmtp_async(*args, self.res)
            torch.cuda.synchronize()
            r = self.ctx.zmtp_result(self.res)
        else:
            r = self.ctx.decode_zmtp(*args)
        nf = min(int(r["frames"]), mf)
        return dict(result=r, n=n, f_off=self.foff[:nf].cpu().numpy().view(np.uint64),
                    f_len=self.flen[:nf].cpu().numpy().view(np.uint32),
                    out_off=self.poff[:nf].cpu().numpy().view(np.uint64), flags=self.fl[:nf].cpu().numpy(),
                    status=self.st[:nf].cpu().numpy().astype(np.int64) & 0xFFFFFFFF,
                    pad_len=self.flen[nf:mf].cpu().numpy(), out=self.out[:n].cpu().numpy(),
                    peer=self.ctx.get_peer_nonce(0))

    def close(self):
        self.ctx.close()


def compare(got, exp, name):
    r = got["result"]
    assert r == dict(frames=exp["frames"], consumed=exp["consumed"], out_bytes=exp["out_bytes"], error=exp["error"]), \
        (name, r, {k: exp[k] for k in ("frames", "consumed", "out_bytes", "error")})
    assert (got["f_off"] == exp["f_off"]).all() and (got["f_len"] == exp["f_len"]).all(), name
    assert (got["out_off"] == exp["f_off"]).all(), name  # each payload at its body's offset
    assert (got["status"] == exp["status"]).all(), (name, got["status"].tolist(), exp["status"].tolist())
    assert (got["flags"] == exp["flags"]).all(), name
    if got["n"]:  # entries from result.frames on: empty frames (nothing is written for an empty buffer)
        assert (got["pad_len"] == 0).all(), name
    for a, ln in zip(exp["f_off"], exp["plen"]):
        a, ln = int(a), int(ln)
        assert (got["out"][a:a + ln] == exp["out"][a:a + ln]).all(), (name, a)
    assert got["peer"] == exp["peer"], name


def run_class(torch, C, cases, **kw):
    dev = Dev(torch, C, max(c["max_frames"] for c in cases), max(len(c["stream"]) for c in cases))
    ran = 0
    for cs in cases:
        assert cs["kth"] is None
        compare(dev.run(cs, **kw), S.expected(cs), cs["name"])
        ran += 1
    dev.close()
    assert ran == len(cases)


def test_signature_positions(torch_cuda, C):
    run_class(torch_cuda, C, S.class_a())


def test_signature_positions_async(torch_cuda, C):
    run_class(torch_cuda, C, S.class_a(), use_async=True)


@pytest.mark.parametrize("off", [1, 4, 8, 15])
def test_signature_positions_misaligned(torch_cuda, C, off):
    """`in` at byte offsets 1, 4, 8 and 15 of an allocation: any alignment is
    valid (include/zmqg_curve.h)."""
    cases = [c for c in S.class_a() if c["B"] == S.GENERIC_EDGE]
    assert len(cases) == 66
    run_class(torch_cuda, C, cases, off=off)


def test_stream_start_and_end(torch_cuda, C):
    run_class(torch_cuda, C, S.class_b())


def test_shadows(torch_cuda, C):
    cases = [c for c in S.class_c() if c["kth"] is None]
    assert len(cases) == 14
    run_class(torch_cuda, C, cases)


def test_early_stop_and_resume(torch_cuda, C):
    """A planted LARGE header covers frame k's start: the call returns the
    oracle's first k + 1 frames with error 0, and the calls repeated from
    `consumed` (in + consumed: any alignment) until one returns no frame give
    the rest: together the oracle's frames, statuses and peer nonce."""
    cases = [c for c in S.class_c() if c["kth"] is not None]
    assert len(cases) == 9
    dev = Dev(torch_cuda, C, 64, max(len(c["stream"]) for c in cases))
    for cs in cases:
        s, k, full = cs["stream"], cs["kth"], S.expected(cs)
        assert full["frames"] == len(S.EARLY_LENS) and full["consumed"] == len(s)
        first = S.expected(cs, max_frames=k + 1)
        got = dev.run(cs)
        compare(got, first, cs["name"])
        assert got["result"]["error"] == 0 and got["result"]["frames"] == k + 1 < cs["max_frames"]
        pos, peer, f_off, status = first["consumed"], first["peer"], list(first["f_off"]), list(first["status"])
        calls = 1
        while True:
            exp = S.expected(cs, stream=s[pos:], peer=peer)
            got = dev.run(cs, stream=s[pos:], off=pos, reset=False)
            compare(got, exp, cs["name"] + "+%d" % pos)
            calls += 1
            if got["result"]["frames"] == 0:
                break
            f_off += [int(x) + pos for x in got["f_off"]]
            status += list(got["status"])
            pos, peer = pos + got["result"]["consumed"], got["peer"]
        assert pos == len(s) and calls == (2 if k + 1 == full["frames"] else 3)
        assert f_off == [int(x) for x in full["f_off"]] and [int(x) for x in status] == [int(x) for x in full["status"]]
        assert peer == full["peer"]
    dev.close()


def test_early_stop_streams_multi(torch_cuda, C):
    """zmqg_decode_zmtp_multi's sequential parser has no early stop (the one
    exception to "the semantics of n_streams zmqg_decode_zmtp calls",
    include/zmqg_curve.h): the same streams, every frame in one call."""
    from tests.test_zmtp_multi import _compare, _oracle, _run
    cases = [c for c in S.class_c() if c["kth"] is not None]
    arena, offs = bytearray(), []
    for cs in cases:
        arena += bytes(-len(arena) % 16)
        offs.append(len(arena))
        arena += cs["stream"]
    arena = np.frombuffer(bytes(arena), np.uint8).copy()
    lens, sids, precoms = [len(c["stream"]) for c in cases], list(range(len(cases))), [c["precom"] for c in cases]
    ref = _oracle(C, arena, offs, lens, sids, precoms, -1, 8)
    assert all(r["frames"] == len(S.EARLY_LENS) and r["consumed"] == n for r, n in zip(ref["results"], lens))
    _compare(_run(torch_cuda, C, arena, offs, lens, sids, precoms, -1, 8), ref, arena, 8)


def test_density(torch_cuda, C):
    run_class(torch_cuda, C, S.class_d())


def test_links_and_walk(torch_cuda, C):
    run_class(torch_cuda, C, S.class_e())


def test_sizes(torch_cuda, C):
    run_class(torch_cuda, C, S.class_g())


@functools.lru_cache(maxsize=None)
def long_expected(nlists):
    return S.expected(S.long_case(nlists))


def run_long(torch, C, nlists):
    cs = S.long_case(nlists)
    dev = Dev(torch, C, cs["max_frames"], len(cs["stream"]))
    compare(dev.run(cs), long_expected(nlists), cs["name"])
    dev.close()


def test_stream_of_1025_lists(torch_cuda, C):
    """zmtp_suffix_min with two entries a thread (registers)."""
    run_long(torch_cuda, C, 1025)


@pytest.mark.parametrize("cub", [False, True])
def test_stream_of_8193_lists(torch_cuda, C, monkeypatch, cub):
    """zmtp_suffix_min with nine entries a thread (the loop).  Above 8,192
    lists the counts are scanned by hipCUB with or without ZMQG_ZMTP_CUB."""
    if cub:
        monkeypatch.setenv("ZMQG_ZMTP_CUB", "1")
    run_long(torch_cuda, C, 8193)
