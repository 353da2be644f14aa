"""Pure-Python model of zmqg_forward_zmtp_multi's contract (include/zmqg_curve.h)
-- test infrastructure, not a test.  The receive side is the reference's
decoder loop per stream (oracle.zmtp_oracle.parse) and one oracle CURVE decode
over all slots in slot order (oracle.oracle.decode_batch), as for
zmqg_decode_zmtp_multi; the rule of what is forwarded and the pair layout are
stated element by element; the send side is tests/zmtp_send_model.py's model
over the pairs."""
import numpy as np

from oracle import oracle as O
from oracle import zmtp_oracle as Z
from tests import zmtp_send_model as M

MORE, COMMAND = 1, 2  # ZMQG_MSG_*
ERR_SESSION = M.ERR_SESSION
NO_STREAM = 0xFFFFFFFF  # a pair that is not live names no stream


def source_frames(precom, parts, nonce0=3, enc_prefix=O.CLIENT_PREFIX, dec_prefix=O.SERVER_PREFIX):
    """The ZMTP frames one client connection sends: parts = [(msg_t flags,
    payload bytes)], sealed with nonces nonce0, nonce0 + 1, ...; one bytes
    object per frame, for the caller to join, cut, tamper with or repeat."""
    from tests.helpers import pack, wire_layout
    n = len(parts)
    if n == 0:
        return []
    flags = np.array([f for f, _ in parts], np.uint8)
    lens = np.array([len(p) for _, p in parts], np.uint32)
    inp, in_off = pack([p for _, p in parts])
    sid = np.zeros(n, np.uint32)
    out_off, wl, total = wire_layout(flags, lens, [False], sid)
    wire = O.encode_batch(O.make_sessions([precom], enc_prefix, dec_prefix), sid,
                          np.arange(nonce0, nonce0 + n, dtype=np.uint64), flags, in_off, lens, inp, out_off, total)
    return [Z.frame(wire[int(o):int(o) + int(w)].tobytes()) for o, w in zip(out_off, wl)]


def arena_of(streams, gap=3):
    """The streams packed into one buffer at odd offsets that are no multiple
    of 16, junk in the gaps.  Returns (arena, offsets)."""
    buf, offs = bytearray(), []
    for s, st in enumerate(streams):
        buf += (b"\x00\x10\x07MESSAGE" + bytes(range(6)))[:gap + 2 * (s % 5)]
        while len(buf) % 2 == 0 or len(buf) % 16 == 0:
            buf += b"\x00"
        offs.append(len(buf))
        buf += st
    buf += b"\x00" * 8
    return np.frombuffer(bytes(buf), np.uint8).copy(), offs


def rule(elements):
    """elements: Q(s) as (msg_t flags, failed) in order, carry first (a carried
    part never fails).  Returns dict(seq, held_first, forwarded, failed, live):
    F = the first failed element, E = the last element below F that is no
    command and has MORE clear; the non-command elements below E + 1 are
    live."""
    seq = len(elements)
    F = next((i for i, (_, bad) in enumerate(elements) if bad), seq)
    E = max((i for i in range(F) if not elements[i][0] & COMMAND and not elements[i][0] & MORE), default=-1)
    live = [i <= E and not elements[i][0] & COMMAND for i in range(seq)]
    return dict(seq=seq, held_first=E + 1, forwarded=sum(live), failed=int(F < seq), live=live)


def pair_base(carry_counts, route_counts, max_frames):
    """base(s), n_streams + 1 entries (the last is N): stream s owns
    (c(s) + max_frames) * d(s) pairs, p = base(s) + q * d(s) + k."""
    base = [0]
    for c, d in zip(carry_counts, route_counts):
        base.append(base[-1] + (c + max_frames) * d)
    return base


def receive(arena, offs, lens, sids, precoms, peer, max_msg, max_frames, dec_prefix=O.CLIENT_PREFIX):
    """zmqg_decode_zmtp_multi's outputs: dict(results, f_off, f_len, status,
    flags, out, peer); `out` spans the arena, a returned frame's payload at its
    body's offset (a failed frame's region zero-filled), zeros elsewhere."""
    S, ns = len(offs), len(precoms)
    slots = S * max_frames
    f_off, f_len = np.zeros(slots, np.uint64), np.zeros(slots, np.uint32)
    zfl, sid = np.zeros(slots, np.uint8), np.zeros(slots, np.uint32)  # (padding: an empty frame on session 0)
    results = []
    for s in range(S):
        r = Z.parse(arena[offs[s]:offs[s] + lens[s]].tobytes(), max_msg, max_frames) if max_frames else dict(
            frames=[], consumed=0, error=0)
        for j, (f, body, size) in enumerate(r["frames"]):
            k = s * max_frames + j
            f_off[k], f_len[k], zfl[k], sid[k] = offs[s] + body, size, f, sids[s]
        results.append(dict(frames=len(r["frames"]), consumed=r["consumed"], error=r["error"],
                            out_bytes=sum(max(f[2] - 33, 0) for f in r["frames"])))
    known = sid < ns
    dec = np.concatenate([O.make_sessions([p], dec_prefix=dec_prefix) for p in precoms])
    peer = np.array(peer, np.uint64)
    status, flags = np.full(slots, ERR_SESSION, np.int64), np.zeros(slots, np.uint8)
    out = np.zeros(len(arena), np.uint8)
    if known.any():
        out, fl, st = O.decode_batch(dec, peer, sid[known], f_off[known], f_len[known], arena, f_off[known],
                                     len(arena))
        status[known] = st.astype(np.int64) & 0xffffffff
        flags[known] = [int(a) | Z.msg_flags(int(z)) if s_ == 0 else 0 for a, z, s_ in zip(fl, zfl[known], st)]
    return dict(results=results, f_off=f_off, f_len=f_len, status=status, flags=flags, out=out,
                peer=[int(x) for x in peer])


def model(precoms, downgrade, arena, offs, lens, sids, peer, max_msg, max_frames, carry, plain, dst_sid, routes,
          send, out_bytes, out_size, enc_prefix=O.SERVER_PREFIX, dec_prefix=O.CLIENT_PREFIX, encode=True):
    """The whole call on a broker's ctx (it decodes what clients sealed and
    seals as a server).  carry[s]: the stream's carried parts as (offset into
    plain, length, flags); plain: the bytes `plain` holds before the call (the
    carried payloads are read there; None: the arena, plain == in); routes[s]:
    the stream's destinations; peer / send: every session's counters before
    the call.  Returns dict(recv, fwd, base, N, pairs, enc): recv as receive()
    returns it, fwd one rule() per stream, pairs[p] = (stream, element, route,
    live) and enc zmtp_send_model.model's result over the pairs."""
    S = len(offs)
    recv = receive(arena, offs, lens, sids, precoms, peer, max_msg, max_frames, dec_prefix)
    src = arena if plain is None else plain
    fwd, elems = [], []
    for s in range(S):
        q = [(int(fl), False, int(off), int(ln)) for off, ln, fl in carry[s]]
        for j in range(recv["results"][s]["frames"]):
            k = s * max_frames + j
            q.append((int(recv["flags"][k]), recv["status"][k] != 0, int(recv["f_off"][k]),
                      int(recv["f_len"][k]) - 33))
        fwd.append(rule([(e[0], e[1]) for e in q]))
        elems.append(q)
    base = pair_base([len(c) for c in carry], [len(r) for r in routes], max_frames)
    N = base[-1]
    frame_stream, flags, lens_p, payloads, pairs = [], [], [], [], []
    for s in range(S):
        for q in range(len(carry[s]) + max_frames):
            live = q < fwd[s]["seq"] and fwd[s]["live"][q]
            for k, dst in enumerate(routes[s]):
                pairs.append((s, q, k, live))
                if live:
                    fl, _, off, ln = elems[s][q]
                    # a returned frame's payload is what the receive side decoded; a carried part's is in plain
                    data = (src if q < len(carry[s]) else recv["out"])[off:off + ln].tobytes()
                    frame_stream.append(dst), flags.append(fl & MORE), lens_p.append(ln), payloads.append(data)
                else:
                    frame_stream.append(NO_STREAM), flags.append(0), lens_p.append(0), payloads.append(b"")
    assert len(pairs) == N
    enc = M.model(precoms, downgrade, dst_sid, frame_stream, None, flags, lens_p, payloads, out_bytes, out_size,
                  send=send, enc_prefix=enc_prefix, dec_prefix=dec_prefix, encode=encode)
    return dict(recv=recv, fwd=fwd, base=base, N=N, pairs=pairs, enc=enc, frame_stream=frame_stream, flags=flags,
                lens=lens_p, payloads=payloads)
