"""Pure-Python model of zmqg_encode_ws_multi's contract (include/zmqg_curve.h)
-- test infrastructure, not a test: tests/zmtp_send_model.py's layout, fit,
status, nonce and result rules, stated frame by frame in batch order, with the
WebSocket frame size F and tests/ws_model.frame around each MESSAGE command
(from the CPU oracle, oracle.oracle.encode_batch)."""
import errno

import numpy as np

from oracle import oracle as O
from tests import ws_model as W
from tests.zmtp_send_model import ERR_BOUND, ERR_SESSION, SENTINEL, UINT64_MAX, make_batch, oracle_sessions  # noqa: F401


def frame_bytes(flags, downgrade_sub, length, masked):
    """F: 2 bytes, the extended size of W + 1, the key, the flags byte, the MESSAGE command."""
    w = O.wire_size(int(flags), int(bool(downgrade_sub)), int(length))
    return W.header_bytes(w, masked) + w


def model(precoms, downgrade, stream_sid, frame_stream, nonce, flags, lens, payloads, mask, out_bytes, out_size,
          send=None, enc_prefix=O.CLIENT_PREFIX, dec_prefix=O.SERVER_PREFIX, encode=True):
    """As tests/zmtp_send_model.model; mask: None, or one 32-bit key value per
    frame.  Returns dict(out, frame_off, status, results, send, nonce, fit, F,
    hdr): hdr[i] = the bytes in front of frame i's MESSAGE command."""
    n_sessions, n_streams, n = len(precoms), len(stream_sid), len(frame_stream)
    assert n_streams > 0 or n == 0
    masked = mask is not None
    stream_ok = [int(s) < n_sessions for s in stream_sid]
    valid = [int(fs) < n_streams and stream_ok[int(fs)] for fs in frame_stream]
    sid = [int(stream_sid[int(fs)]) if v else None for fs, v in zip(frame_stream, valid)]
    F = [frame_bytes(flags[i], downgrade[sid[i]], lens[i], masked) if valid[i] else 0 for i in range(n)]
    B = [0] * n_streams
    for i in range(n):
        if valid[i]:
            B[int(frame_stream[i])] += F[i]
    base, total = [], 0
    for s in range(n_streams):
        base.append(total)
        total += B[s]
    pos_next = [0] * n_streams
    frame_off = [UINT64_MAX] * n + [sum(B)]
    for i in range(n):
        if valid[i]:
            s = int(frame_stream[i])
            frame_off[i] = base[s] + pos_next[s]
            pos_next[s] += F[i]
    fit = [valid[i] and frame_off[i] + F[i] <= out_bytes for i in range(n)]
    status = [0 if fit[i] else ERR_BOUND if valid[i] else ERR_SESSION for i in range(n)]
    counters = [int(x) for x in send] if send is not None else [0] * n_sessions
    used = [None] * n
    for i in range(n):
        if fit[i]:
            if nonce is not None:
                used[i] = int(nonce[i])
            else:
                used[i] = counters[sid[i]]
                counters[sid[i]] = (counters[sid[i]] + 1) % 2 ** 64
    results = [dict(frames=0, out_off=base[s], out_bytes=0, error=0 if stream_ok[s] else errno.EINVAL)
               for s in range(n_streams)]
    for i in range(n):
        if valid[i]:
            r = results[int(frame_stream[i])]
            if fit[i]:
                r["frames"] += 1
                r["out_bytes"] += F[i]
            else:
                r["error"] = errno.ENOBUFS
    out = np.full(out_size, SENTINEL, np.uint8)
    hdr = [None] * n
    for i in range(n):
        if valid[i]:
            w = O.wire_size(int(flags[i]), int(bool(downgrade[sid[i]])), int(lens[i]))
            hdr[i] = F[i] - w
    idx = [i for i in range(n) if fit[i]] if out_size else []
    if idx:
        if encode:
            from tests.helpers import pack
            inp, in_off = pack([payloads[i] for i in idx])
            wire = O.encode_batch(oracle_sessions(precoms, downgrade, enc_prefix, dec_prefix),
                                  [sid[i] for i in idx], [used[i] for i in idx], [int(flags[i]) for i in idx], in_off,
                                  [int(lens[i]) for i in idx], inp, [frame_off[i] + hdr[i] for i in idx],
                                  max(frame_off[i] + F[i] for i in idx))
        for i in idx:
            a, key = frame_off[i], int(mask[i]) if masked else None
            if encode:
                f = W.frame(wire[a + hdr[i]:a + F[i]].tobytes(), key)
                assert len(f) == F[i]
                out[a:a + F[i]] = np.frombuffer(f, np.uint8)
            else:
                out[a:a + hdr[i]] = np.frombuffer(W.frame(bytes(F[i] - hdr[i]), key)[:hdr[i]], np.uint8)
    return dict(out=out, frame_off=frame_off, status=status, results=results, send=counters, nonce=used, fit=fit,
                F=F, hdr=hdr)
