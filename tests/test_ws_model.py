"""tests/ws_model.py against tests/golden/ws_vectors.json, which is recorded
from the reference's own ws_decoder_t and ws_encoder_t
(tests/golden/make_ws_vectors.py, tests/host/ws_ref_vectors.cpp): every
decoder record fed whole and bytewise, every encoder record, RFC 6455's
masking example, and frame -> parse round trips.  No GPU."""
import hashlib
import json
import os

import pytest

from tests import ws_model as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ws_vectors.json")
with open(GOLDEN) as _f:
    DOC = json.load(_f)

# msg_t flags of the decoder's messages (src/msg.hpp:55-63)
MSG_FLAGS = {W.OP_CLOSE: 2 | 20, W.OP_PING: 2 | 4, W.OP_PONG: 2 | 8}


def _pattern(n):
    return bytes((7 * j + 3) & 0xFF for j in range(n))


def _same(blob, data):
    if blob["len"] != len(data):
        return False
    if "data" in blob:
        return blob["data"] == data.hex()
    return blob["sha256"] == hashlib.sha256(data).hexdigest() and blob["head"] == data[:32].hex()


def _decode_all(buf, must_mask, max_msg_size):
    """The model applied as the reference's decoder runs: on through control
    frames and non-MESSAGE frames, to the end of the bytes or the first error.
    Returns (messages as (msg_t flags, unmasked bytes), error, fail_at)."""
    msgs, pos = [], 0
    while True:
        r = W.parse(buf[pos:], must_mask, max_msg_size)
        for fl, off, size, key in r["frames"]:
            body = buf[pos + off:pos + off + size]
            msgs.append((W.msg_flags(fl), W.unmask(body, key, 1) if must_mask else body))
        if r["ctl"]:
            op, off, size, key = r["ctl"]
            body = buf[pos + off:pos + off + size]
            msgs.append((MSG_FLAGS[op], W.unmask(body, key, 0) if must_mask else body))
        if r["error"]:
            return msgs, r["error"], pos + r["fail_at"]
        if r["consumed"] == 0:
            return msgs, 0, None
        pos += r["consumed"]


def test_fixture_covers_the_issue_cases():
    names = {(d["name"], d["must_mask"]) for d in DOC["decode"]}
    for mm in (0, 1):
        for op in range(16):
            assert ("opcode_%d" % op, mm) in names
        for size in (0, 1, 2, 125, 126, 127, 65535, 65536):
            assert ("binary_size_%d" % size, mm) in names and ("ping_size_%d" % size, mm) in names
        for name in ("fin_clear", "wrong_mask_bit", "binary_size_5_form_126", "binary_size_5_form_127",
                     "binary_11_maxmsgsize_9", "binary_11_maxmsgsize_10", "binary_11_maxmsgsize_11",
                     "close_10_maxmsgsize_9", "close_10_maxmsgsize_10", "close_10_maxmsgsize_11",
                     "cut_op2_form127_at_0", "cut_op2_form127_at_%d" % (15 if mm else 11)):
            assert (name, mm) in names
    sizes = {(e["must_mask"], e["body_pattern_len"] + 1) for e in DOC["encode"]}
    assert {(m, s) for m in (0, 1) for s in (125, 126, 65535, 65536)} <= sizes


@pytest.mark.parametrize("rec", DOC["decode"], ids=lambda d: "%s-mask%d" % (d["name"], d["must_mask"]))
def test_model_reproduces_decoder_record(rec):
    buf = bytes.fromhex(rec["prefix"]) + _pattern(rec["pattern_len"])
    msgs, error, fail_at = _decode_all(buf, rec["must_mask"], rec["maxmsgsize"])
    for how in ("whole", "bytewise"):  # the decoder's answer does not depend on how the bytes arrive
        ref = rec[how]
        assert len(ref["msgs"]) == len(msgs), how
        for want, (fl, data) in zip(ref["msgs"], msgs):
            assert want["flags"] == fl and _same(want, data), how
        assert (ref["rc"] == -1) == (error != 0), how
        if error:
            # the reference sets errno for EMSGSIZE only; EPROTO is this library's choice
            assert ref["errno"] == (W.EMSGSIZE if error == W.EMSGSIZE else 0), how
            assert ref["fed"] == fail_at, how
        else:
            assert ref["fed"] == len(buf), how


@pytest.mark.parametrize("rec", DOC["encode"],
                         ids=lambda e: "mask%d-%d-flags%d" % (e["must_mask"], e["body_pattern_len"], e["flags"]))
def test_model_reproduces_encoder_record(rec):
    body = _pattern(rec["body_pattern_len"])
    # (msg_t more / command and the flags byte's more / command have the same values, 1 and 2)
    out = W.frame(body, rec["random"] if rec["must_mask"] else None, rec["flags"] & 3)
    assert _same(rec["out"], out)
    assert len(out) == W.header_bytes(len(body), bool(rec["must_mask"])) + len(body)
    # and back through the model's decoder
    r = W.parse(out, rec["must_mask"])
    assert r["error"] == 0 and r["consumed"] == len(out) and len(r["frames"]) == 1
    fl, off, size, key = r["frames"][0]
    assert fl == rec["flags"] & 3 and size == len(body)
    assert (W.unmask(out[off:], key, 1) if rec["must_mask"] else out[off:]) == body


def test_rfc6455_masking_example():
    """RFC 6455 section 5.7: "Hello" under the key 37 fa 21 3d."""
    key = bytes.fromhex("37fa213d")
    assert W.unmask(b"Hello", key) == bytes.fromhex("7f9f4d5158")
    assert W.unmask(bytes.fromhex("7f9f4d5158"), 0x37FA213D) == b"Hello"
    assert W.frame(b"Hello", key, opcode=W.OP_PING) == bytes.fromhex("8985" "37fa213d" "7f9f4d5158")
    # a binary frame's body starts at key byte 1: the flags byte took key byte 0
    f = W.frame(b"Hello", key, flags=W.MORE)
    assert f[:7] == bytes.fromhex("8286" "37fa213d" "36") and W.unmask(f[7:], key, 1) == b"Hello"


@pytest.mark.parametrize("mask", [None, 0x37FA213D, 0, 0xFFFFFFFF])
def test_frame_parse_round_trip(mask):
    bodies = [W.MESSAGE + _pattern(n) for n in (0, 1, 40, 116, 117, 118, 65526, 65527, 65528)]
    forms = [None, 126, 127, None, None, 127, None, 127, None]
    buf, want = b"", []
    for i, (b, form) in enumerate(zip(bodies, forms)):
        f = W.frame(b, None if mask is None else (mask + i) & 0xFFFFFFFF, flags=i & 3, form=form)
        want.append((i & 3, len(buf) + len(f) - len(b), len(b)))
        buf += f
    ping = W.frame(b"ping!", None if mask is None else mask, opcode=W.OP_PING)
    tail = W.frame(W.MESSAGE, None if mask is None else mask)
    r = W.parse(buf + ping + tail, mask is not None)
    assert [f[:3] for f in r["frames"]] == want and r["error"] == 0
    assert r["consumed"] == len(buf) + len(ping)  # the control frame ends the parse and is consumed
    op, off, size, key = r["ctl"]
    assert (op, size) == (W.OP_PING, 5) and off == len(buf) + len(ping) - 5
    for (fl, off, size, key), b in zip(r["frames"], bodies):
        got = buf[off:off + size]
        assert (W.unmask(got, key, 1) if mask is not None else got) == b
    # max_frames stops the parse before the next frame, whatever it is
    r = W.parse(buf + ping, mask is not None, max_frames=len(bodies))
    assert len(r["frames"]) == len(bodies) and r["ctl"] is None and r["consumed"] == len(buf)
    # a frame that is not a MESSAGE command is the last one returned
    r = W.parse(W.frame(b"\x04PING123", mask) + buf, mask is not None)
    assert len(r["frames"]) == 1 and r["consumed"] == W.header_bytes(8, mask is not None) + 8
    # every proper prefix of a frame is incomplete, except that a clear FIN bit shows at once
    f = W.frame(bodies[2], mask)
    for cut in range(len(f)):
        assert W.parse(f[:cut], mask is not None) == dict(frames=[], consumed=0, error=0, ctl=None, fail_at=None)
    assert W.parse(b"\x02", mask is not None)["error"] == W.EPROTO
    assert W.parse(b"\x82", mask is not None)["error"] == 0
