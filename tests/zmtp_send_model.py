"""Pure-Python model of zmqg_encode_zmtp_multi's contract (include/zmqg_curve.h)
-- test infrastructure, not a test: the layout, fit, status, nonce and result
rules stated frame by frame in batch order, the MESSAGE commands from the CPU
oracle (oracle.oracle.encode_batch) and the ZMTP headers from
oracle.zmtp_oracle.frame."""
import errno

import numpy as np

from oracle import oracle as O
from oracle import zmtp_oracle as Z

ERR_SESSION, ERR_BOUND = 0x7A000001, 0x7A000002  # include/zmqg_curve.h
UINT64_MAX = 2 ** 64 - 1
SENTINEL = 0xEE


def oracle_sessions(precoms, downgrade, enc_prefix=O.CLIENT_PREFIX, dec_prefix=O.SERVER_PREFIX):
    return np.concatenate([O.make_sessions([p], enc_prefix, dec_prefix, bool(d)) for p, d in zip(precoms, downgrade)])


def frame_bytes(flags, downgrade_sub, length):
    """F: the MESSAGE command plus its ZMTP header (2 bytes, 9 above 255)."""
    w = O.wire_size(int(flags), int(bool(downgrade_sub)), int(length))
    return w + (9 if w > 255 else 2)


def make_batch(rng, n, n_streams, sizes, flag_choices=(0, 1, 2, 3, 12, 16), frame_stream=None):
    """n frames in arrival order over n_streams streams (random unless given),
    with explicit nonces that include 2^32 - 1, 2^32 and 2^64 - 1."""
    fs = rng.integers(0, n_streams, n).astype(np.uint32) if frame_stream is None else np.asarray(frame_stream,
                                                                                                 np.uint32)
    lens = rng.choice(sizes, n).astype(np.uint32)
    flags = rng.choice(flag_choices, n).astype(np.uint8)
    payloads = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in lens]
    nonce = (np.uint64(2 ** 32 - 3) + np.arange(n, dtype=np.uint64))
    if n:
        nonce[-1] = np.uint64(2 ** 64 - 1)
    return dict(n=n, frame_stream=fs, lens=lens, flags=flags, payloads=payloads, nonce=nonce)


def model(precoms, downgrade, stream_sid, frame_stream, nonce, flags, lens, payloads, out_bytes, out_size,
          send=None, enc_prefix=O.CLIENT_PREFIX, dec_prefix=O.SERVER_PREFIX, encode=True):
    """precoms / downgrade: the ctx's sessions.  nonce: one per frame, or None
    for the device counters, which start at `send` (one per session).
    Returns dict(out, frame_off, status, results, send, nonce, fit): `out` is
    out_size bytes, SENTINEL wherever the call writes nothing; frame_off has
    n + 1 entries; `send` the counters afterwards; `nonce` the nonce each
    fitting frame was sealed with.  encode=False leaves the MESSAGE bodies out
    (headers and layout only); out_size = 0 gives the layout alone, to size
    `out` with."""
    n_sessions, n_streams, n = len(precoms), len(stream_sid), len(frame_stream)
    assert n_streams > 0 or n == 0
    stream_ok = [int(s) < n_sessions for s in stream_sid]
    valid = [int(fs) < n_streams and stream_ok[int(fs)] for fs in frame_stream]
    sid = [int(stream_sid[int(fs)]) if v else None for fs, v in zip(frame_stream, valid)]
    F = [frame_bytes(flags[i], downgrade[sid[i]], lens[i]) if valid[i] else 0 for i in range(n)]
    # B(s), base(s): regions packed in stream order
    B = [0] * n_streams
    for i in range(n):
        if valid[i]:
            B[int(frame_stream[i])] += F[i]
    base, total = [], 0
    for s in range(n_streams):
        base.append(total)
        total += B[s]
    # pos(i): the stream's valid frames before i
    pos_next = [0] * n_streams
    frame_off = [UINT64_MAX] * n + [sum(B)]
    for i in range(n):
        if valid[i]:
            s = int(frame_stream[i])
            frame_off[i] = base[s] + pos_next[s]
            pos_next[s] += F[i]
    fit = [valid[i] and frame_off[i] + F[i] <= out_bytes for i in range(n)]
    status = [0 if fit[i] else ERR_BOUND if valid[i] else ERR_SESSION for i in range(n)]
    # nonces: the caller's, or get_and_inc_nonce per fitting frame in batch order
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
    idx = [i for i in range(n) if fit[i]] if out_size else []
    if idx:
        hdr = {i: 9 if F[i] > 257 else 2 for i in idx}
        if encode:
            from tests.helpers import pack
            inp, in_off = pack([payloads[i] for i in idx])
            wire = O.encode_batch(oracle_sessions(precoms, downgrade, enc_prefix, dec_prefix),
                                  [sid[i] for i in idx], [used[i] for i in idx], [int(flags[i]) for i in idx], in_off,
                                  [int(lens[i]) for i in idx], inp, [frame_off[i] + hdr[i] for i in idx],
                                  max(frame_off[i] + F[i] for i in idx))
        for i in idx:
            a, w = frame_off[i], F[i] - hdr[i]
            if encode:
                out[a:a + F[i]] = np.frombuffer(Z.frame(wire[a + hdr[i]:a + F[i]].tobytes()), np.uint8)
            else:
                out[a:a + hdr[i]] = np.frombuffer(Z.frame(bytes(w))[:hdr[i]], np.uint8)
    return dict(out=out, frame_off=frame_off, status=status, results=results, send=counters, nonce=used, fit=fit,
                F=F)
