"""WebSocket framing restatement for CURVE MESSAGE commands -- test
infrastructure, not a test: the checker for zmqg_decode_ws_multi /
zmqg_encode_ws_multi, pinned to the reference's own ws_decoder_t / ws_encoder_t
by tests/golden/ws_vectors.json (tests/test_ws_model.py).

  frame(body, mask, flags, opcode)
      ws_encoder_t on one message (src/ws_encoder.cpp:26-126): 0x80 | opcode,
      the MASK bit and the size (7 bits, 126 + 2 bytes, 127 + 8 bytes, big
      endian), the key BE32(mask), then -- binary frames only -- the flags byte
      (ws_protocol_t: more 1, command 2), then the body; flags byte and body
      XORed with the key from key byte 0 on.  form=126 / 127 forces a
      non-minimal size form, which the decoder accepts.
  parse(buf, must_mask, max_msg_size, max_frames)
      ws_decoder_t's state machine (src/ws_decoder.cpp:39-249) from offset 0,
      over the bytes that are present: a check is made once its deciding bytes
      are there, and the first one whose bytes are missing leaves the frame for
      the next call.  It stops after a control frame (returned apart: the
      engine answers it, src/ws_engine.cpp:891-894) and, as the engine does,
      after the first binary frame that is not a MESSAGE command.
  unmask(data, key, start)
      data[i] ^ key[(start + i) % 4] (RFC 6455 section 5.3).
"""
import struct

OP_BINARY, OP_CLOSE, OP_PING, OP_PONG = 2, 8, 9, 10  # src/ws_protocol.hpp:14-21
MORE, COMMAND = 1, 2                                  # src/ws_protocol.hpp:23-27
EPROTO, EMSGSIZE = 71, 90
MESSAGE = b"\x07MESSAGE"


def key_bytes(mask):
    """The four key bytes of a 32-bit mask value (put_uint32: big endian)."""
    return mask if isinstance(mask, (bytes, bytearray)) else struct.pack(">I", int(mask))


def unmask(data, key, start=0):
    key = key_bytes(key)
    return bytes(b ^ key[(start + i) & 3] for i, b in enumerate(bytes(data)))


def header(size, masked, opcode=OP_BINARY, form=None):
    """Byte 0, byte 1 and the extended size of a frame whose payload is `size` bytes."""
    m = 0x80 if masked else 0
    if form is None:
        form = 125 if size <= 125 else 126 if size <= 0xFFFF else 127
    if form == 125:
        assert size <= 125
        return bytes([0x80 | opcode, m | size])
    if form == 126:
        assert size <= 0xFFFF
        return bytes([0x80 | opcode, m | 126]) + struct.pack(">H", size)
    return bytes([0x80 | opcode, m | 127]) + struct.pack(">Q", size)


def frame(body, mask=None, flags=0, opcode=OP_BINARY, form=None):
    body = bytes(body)
    payload = (bytes([flags]) if opcode == OP_BINARY else b"") + body
    h = header(len(payload), mask is not None, opcode, form)
    if mask is None:
        return h + payload
    return h + key_bytes(mask) + unmask(payload, mask)


def header_bytes(size, masked, form=None):
    """Bytes in front of a binary frame's body: header, key and flags byte."""
    return len(header(size + 1, masked, OP_BINARY, form)) + (4 if masked else 0) + 1


def parse(buf, must_mask, max_msg_size=-1, max_frames=None):
    """dict(frames=[(ws_flags, body_off, body_len, key)], consumed, error,
    ctl=None | (opcode, off, len, key), fail_at); key is b"" without
    must_mask; fail_at: with an error, the offset behind the byte that decided
    it (where the reference's decoder stops reading).  The bodies stay as they
    are in buf (masked)."""
    buf = bytes(buf)
    n = len(buf)
    pos, frames, error, ctl, fail_at = 0, [], 0, None, None
    while max_frames is None or len(frames) < max_frames:
        if pos + 1 > n:
            break
        b0 = buf[pos]
        op = b0 & 0x0F
        if not b0 & 0x80 or op not in (OP_BINARY, OP_CLOSE, OP_PING, OP_PONG):
            error, fail_at = EPROTO, pos + 1
            break
        if pos + 2 > n:
            break
        b1 = buf[pos + 1]
        if bool(b1 & 0x80) != bool(must_mask):
            error, fail_at = EPROTO, pos + 2
            break
        size, q = b1 & 0x7F, pos + 2
        if size == 126:
            if q + 2 > n:
                break
            size, q = struct.unpack(">H", buf[q:q + 2])[0], q + 2
        elif size == 127:
            if q + 8 > n:
                break
            size, q = struct.unpack(">Q", buf[q:q + 8])[0], q + 8
        key = b""
        if must_mask:
            if q + 4 > n:
                break
            key, q = buf[q:q + 4], q + 4
        flags = 0
        if op == OP_BINARY:
            if size == 0:
                error, fail_at = EPROTO, q
                break
            if q + 1 > n:
                break
            flags = buf[q] ^ (key[0] if must_mask else 0)
            q += 1
            size -= 1
        # max_msg_size: src/ws_decoder.cpp:166-173; the 2^32 - 1 bound is this
        # library's restriction (32-bit frame lengths), as in oracle/zmtp_oracle.py
        if (max_msg_size >= 0 and size > max_msg_size) or size > 0xFFFFFFFF:
            error, fail_at = EMSGSIZE, q
            break
        if q + size > n:
            break  # incomplete: wait for more bytes
        pos = q + size
        if op != OP_BINARY:
            ctl = (op, q, size, key)
            break
        frames.append((flags, q, size, key))
        body = unmask(buf[q:q + min(size, 8)], key, 1) if must_mask else buf[q:q + 8]
        if size < 8 or body != MESSAGE:
            break  # the mechanism rejects it; the connection ends here
    return dict(frames=frames, consumed=pos, error=error, ctl=ctl, fail_at=fail_at)


def msg_flags(ws_flags):
    """msg_t flags the decoder gives a binary frame (src/ws_decoder.cpp:155-158)."""
    return (1 if ws_flags & MORE else 0) | (2 if ws_flags & COMMAND else 0)
