"""Pure-Python model of zmqg_forward_framed_multi's contract
(include/zmqg_curve.h) -- test infrastructure, not a test.  It composes what is
already there:

  receive side  ZMTP: forward_model.receive.  WebSocket: ws_model.parse per
                stream and one oracle CURVE decode over all slots in slot order
                (ws_receive below), the analogue of forward_model.receive.
  plan          the mode's own model (forward_model, forward_sub_model,
                forward_router_model, forward_lb_model) run on the ZMTP twin of
                the input: the MESSAGE bodies the WebSocket parse returned, in
                ZMTP frames whose flags byte carries the WebSocket flags byte's
                MORE / COMMAND bits.  The plan depends on the decoded slots
                alone, and the twin's slots are checked against the receive
                side's, slot for slot.
  send side     ZMTP: zmtp_send_model.model.  WebSocket: ws_send_model.model
                over the plan's frame_stream / flags / lens / payloads, the
                mask indexed by pair.
"""
import struct

import numpy as np

from oracle import oracle as O
from oracle import zmtp_oracle as Z
from tests import forward_lb_model as FL
from tests import forward_model as F
from tests import forward_router_model as FR
from tests import forward_sub_model as FS
from tests import ws_model as W
from tests import ws_send_model as WS
from tests import zmtp_send_model as M

ZMTP, WS_PLAIN, WS_MASKED = 0, 1, 2          # ZMQG_FRAMING_*
STATIC, SUB, ROUTER, LB = 0, 1, 2, 3         # ZMQG_FWD_*
MORE, COMMAND = F.MORE, F.COMMAND


def bodies(precom, parts, nonce0=3):
    """The MESSAGE commands one client connection sends for parts = [(msg_t
    flags, payload)]: forward_model.source_frames without the ZMTP header."""
    return [f[9:] if f[0] & Z.LARGE else f[2:] for f in F.source_frames(precom, parts, nonce0)]


def zmtp_frame(body, msg_flags=0):
    """A ZMTP frame around `body` whose flags byte carries msg_t MORE / COMMAND."""
    body = bytes(body)
    zf = (Z.MORE if msg_flags & MORE else 0) | (Z.COMMAND if msg_flags & COMMAND else 0)
    if len(body) > 255:
        return bytes([zf | Z.LARGE]) + struct.pack(">Q", len(body)) + body
    return bytes([zf, len(body)]) + body


def ws_receive(arena, offs, lens, sids, precoms, peer, must_mask, max_msg, max_frames, dec_prefix=O.CLIENT_PREFIX):
    """zmqg_decode_ws_multi's outputs: dict(results, f_off, f_len, status,
    flags, out, peer) as forward_model.receive returns them, results with the
    control frame's fields, plus plain (the arena with every returned body and
    control payload unmasked: what the CURVE decode reads), body / ctl (masks
    of the bytes of the returned bodies / of the control payloads) and wsflags
    (msg_t flags from each slot's WebSocket flags byte)."""
    S, ns = len(offs), len(precoms)
    slots = S * max_frames
    f_off, f_len = np.zeros(slots, np.uint64), np.zeros(slots, np.uint32)
    mfl, sid = np.zeros(slots, np.uint8), np.zeros(slots, np.uint32)  # (padding: an empty frame on session 0)
    results, plain = [], arena.copy()
    body, ctl = np.zeros(len(arena), bool), np.zeros(len(arena), bool)

    def put(a, b):
        plain[a:a + len(b)] = np.frombuffer(b, np.uint8)

    for s in range(S):
        r = W.parse(arena[offs[s]:offs[s] + lens[s]].tobytes(), must_mask, max_msg, max_frames) if max_frames else dict(
            frames=[], consumed=0, error=0, ctl=None)
        for j, (fl, boff, size, key) in enumerate(r["frames"]):
            k, a = s * max_frames + j, offs[s] + boff
            f_off[k], f_len[k], mfl[k], sid[k] = a, size, W.msg_flags(fl), sids[s]
            body[a:a + size] = True
            if must_mask:
                put(a, W.unmask(arena[a:a + size].tobytes(), key, 1))
        res = dict(frames=len(r["frames"]), consumed=r["consumed"],
                   out_bytes=sum(max(f[2] - 33, 0) for f in r["frames"]), error=r["error"], ctl_opcode=0, ctl_off=0,
                   ctl_len=0)
        if r["ctl"]:
            op, coff, size, key = r["ctl"]
            a = offs[s] + coff
            res.update(ctl_opcode=op, ctl_off=a, ctl_len=size)
            ctl[a:a + size] = True
            if must_mask:
                put(a, W.unmask(arena[a:a + size].tobytes(), key, 0))
        results.append(res)
    known = sid < ns
    dec = np.concatenate([O.make_sessions([p], dec_prefix=dec_prefix) for p in precoms])
    peer = np.array(peer, np.uint64)
    status, flags = np.full(slots, F.ERR_SESSION, np.int64), np.zeros(slots, np.uint8)
    out = np.zeros(len(arena), np.uint8)
    if known.any():
        out, fl, st = O.decode_batch(dec, peer, sid[known], f_off[known], f_len[known], plain, f_off[known],
                                     len(arena))
        status[known] = st.astype(np.int64) & 0xffffffff
        flags[known] = [int(a) | int(m) if s_ == 0 else 0 for a, m, s_ in zip(fl, mfl[known], st)]
    return dict(results=results, f_off=f_off, f_len=f_len, status=status, flags=flags, out=out,
                peer=[int(x) for x in peer], plain=plain, body=body, ctl=ctl, wsflags=mfl)


def zmtp_twin(recv, max_frames):
    """The ZMTP twin of a WebSocket receive side: per stream, the returned
    frames' MESSAGE bodies (unmasked) in ZMTP frames.  Returns (arena, offs,
    lens) for forward_model.receive."""
    streams = []
    for s, r in enumerate(recv["results"]):
        fr = []
        for k in range(s * max_frames, s * max_frames + r["frames"]):
            a, n = int(recv["f_off"][k]), int(recv["f_len"][k])
            fr.append(zmtp_frame(recv["plain"][a:a + n].tobytes(), int(recv["wsflags"][k])))
        streams.append(b"".join(fr))
    arena, offs = F.arena_of(streams)
    return arena, offs, [len(x) for x in streams]


def plan(mode, precoms, downgrade, arena, offs, lens, sids, peer, max_msg, max_frames, carry, plain, dst_sid, send,
         routes=None, **kw):
    """The mode's own model without its encode (everything fits, nothing is
    written): fwd, base, N, pairs, frame_stream, flags, lens, payloads and the
    mode's extras, with enc the ZMTP layout."""
    common = (precoms, downgrade, arena, offs, lens, sids, peer, max_msg, max_frames, carry, plain, dst_sid)
    big = dict(out_bytes=2 ** 62, out_size=0, encode=False)
    if mode == STATIC:
        return F.model(*common, routes, send, **big)
    if mode == SUB:
        return FS.model(*common, routes, send, kw["subs"], invert=kw.get("invert", False), **big)
    if mode == ROUTER:
        return FR.model(*common, routes, send, kw["flags"], kw.get("src_ids"), kw.get("table"), **big)
    assert mode == LB
    return FL.model(*common, send, kw["flags"], kw.get("src_ids"), kw["stream_group"], kw["table"], **big)


def model(mode, recv_fr, send_fr, precoms, downgrade, arena, offs, lens, sids, peer, max_msg, max_frames, carry, plain,
          dst_sid, send, out_bytes, out_size, routes=None, mask=None, encode=True, **kw):
    """The whole call.  The arguments are forward_model.model's (lb: no
    routes), the framings, the mode with its own model's arguments as keywords
    (subs, invert / flags, src_ids, table / flags, src_ids, stream_group,
    table) and, for a masked send side, mask: one 32-bit key value per pair.
    out_bytes None: everything fits and out_size is taken behind the total.
    Returns dict(recv, twin, fwd, base, N, pairs, frame_stream, flags, lens,
    payloads, enc, total, cap, ...the mode's extras)."""
    src = arena if plain is None else plain
    if recv_fr == ZMTP:
        recv, twin, twin_max = None, (arena, offs, lens), max_msg
    else:  # (the WebSocket parse has applied max_msg; the twin holds what it returned)
        recv = ws_receive(arena, offs, lens, sids, precoms, peer, recv_fr == WS_MASKED, max_msg, max_frames)
        twin, twin_max = zmtp_twin(recv, max_frames), -1
    # (carried parts and routing ids are read at their own offsets in `plain`, whatever the twin's layout is)
    m = plan(mode, precoms, downgrade, *twin, sids, peer, twin_max, max_frames, carry, src, dst_sid, send,
             routes=routes, **kw)
    t = m["recv"]
    recv = recv or t
    assert [r["frames"] for r in t["results"]] == [r["frames"] for r in recv["results"]]
    assert (t["status"] == recv["status"]).all() and (t["flags"] == recv["flags"]).all() and t["peer"] == recv["peer"]
    N = m["N"]
    if send_fr == ZMTP:
        enc_of = lambda cap, size, enc: M.model(precoms, downgrade, dst_sid, m["frame_stream"], None, m["flags"],
                                                m["lens"], m["payloads"], cap, size, send=send,
                                                enc_prefix=O.SERVER_PREFIX, dec_prefix=O.CLIENT_PREFIX, encode=enc)
    else:
        keys = None
        if send_fr == WS_MASKED:
            assert mask is not None and len(mask) == N
            keys = [int(x) for x in mask]
        enc_of = lambda cap, size, enc: WS.model(precoms, downgrade, dst_sid, m["frame_stream"], None, m["flags"],
                                                 m["lens"], m["payloads"], keys, cap, size, send=send,
                                                 enc_prefix=O.SERVER_PREFIX, dec_prefix=O.CLIENT_PREFIX, encode=enc)
    total = enc_of(2 ** 62, 0, False)["frame_off"][-1] if len(dst_sid) else 0
    cap = total if out_bytes is None else out_bytes
    size = out_size if out_bytes is not None else total + out_size
    if len(dst_sid):
        enc = enc_of(cap, size, encode)
    else:  # no destinations: the send side is pair_off[0] = 0 alone
        enc = dict(out=np.full(size, M.SENTINEL, np.uint8), frame_off=[0], status=[], results=[],
                   send=[int(x) for x in send])
    out = dict(m)
    out.update(recv=recv, twin=twin, enc=enc, total=total, cap=cap, size=size)
    return out
