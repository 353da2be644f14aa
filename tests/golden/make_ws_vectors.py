#!/usr/bin/env python3
"""Records tests/golden/ws_vectors.json from the reference's own ws_decoder_t
and ws_encoder_t: compiles tests/host/ws_ref_vectors.cpp with the reference's
src/msg.cpp, metadata.cpp, err.cpp, ws_decoder.cpp, decoder_allocators.cpp and
ws_encoder.cpp where they lie (REF, default /root/reference; the test-only
tests/host/ref_platform/platform.hpp in place of the generated one) into a
temporary directory, feeds it the cases below and writes what it answers.
Nothing of the reference enters the repository: the JSON holds the byte
strings this file makes up and the decoder's / encoder's results.

Long byte strings are kept short: an input is `prefix` (hex) followed by
`pattern_len` bytes of the pattern (byte j = (7 j + 3) mod 256); a result
longer than 64 bytes is its length, its SHA-256 and its first 32 bytes.

    python tests/golden/make_ws_vectors.py
"""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF", "/root/reference")
KEY = 0x37FA213D  # RFC 6455 section 5.7's example key
REF_SOURCES = ["msg", "metadata", "err", "ws_decoder", "decoder_allocators", "ws_encoder"]


def pattern(n):
    return bytes((7 * j + 3) & 0xFF for j in range(n))


def blob(b):
    b = bytes(b)
    if len(b) <= 64:
        return dict(len=len(b), data=b.hex())
    return dict(len=len(b), sha256=hashlib.sha256(b).hexdigest(), head=b[:32].hex())


def build(tmp):
    exe = os.path.join(tmp, "ws_ref_vectors")
    inc = ["-I" + os.path.join(ROOT, "tests/host/ref_platform"), "-I" + os.path.join(REF, "src"),
           "-I" + os.path.join(REF, "include")]
    srcs = [os.path.join(REF, "src", f + ".cpp") for f in REF_SOURCES]
    subprocess.check_call(["g++", "-O1", "-std=c++11"] + inc + ["-o", exe,
                                                                os.path.join(ROOT, "tests/host/ws_ref_vectors.cpp")]
                          + srcs + ["-lpthread"])
    return exe


def hdr(op, size, masked, form=None, fin=0x80):
    """Byte 0, byte 1, the extended size and the key."""
    m = 0x80 if masked else 0
    if form is None:
        form = 125 if size <= 125 else 126 if size <= 0xFFFF else 127
    if form == 125:
        h = bytes([fin | op, m | size])
    elif form == 126:
        h = bytes([fin | op, m | 126]) + struct.pack(">H", size)
    else:
        h = bytes([fin | op, m | 127]) + struct.pack(">Q", size)
    return h + (struct.pack(">I", KEY) if masked else b"")


def decode_cases():
    """(name, must_mask, maxmsgsize, prefix, pattern_len)"""
    cases = []
    for mm in (0, 1):
        add = lambda name, prefix, plen=0, maxmsg=-1: cases.append((name, mm, maxmsg, bytes(prefix), plen))
        for op in range(16):
            add("opcode_%d" % op, hdr(op, 3, mm), 3)
        add("fin_clear", hdr(2, 3, mm, fin=0), 3)
        add("fin_clear_lone", b"\x02")
        add("lone_0x82", b"\x82")
        add("wrong_mask_bit", hdr(2, 3, not mm), 3)
        add("wrong_mask_bit_ping", hdr(9, 0, not mm))
        for size in (0, 1, 2, 125, 126, 127, 65535, 65536):
            add("binary_size_%d" % size, hdr(2, size, mm), size)
            add("ping_size_%d" % size, hdr(9, size, mm), size)
        for size, form in ((5, 126), (5, 127), (200, 127), (0, 126), (0, 127)):
            add("binary_size_%d_form_%d" % (size, form), hdr(2, size, mm, form), size)
            add("pong_size_%d_form_%d" % (size, form), hdr(10, size, mm, form), size)
        add("binary_size_0_no_key", hdr(2, 0, mm)[:2])
        for d in (-1, 0, 1):  # a binary frame's message size is its payload without the flags byte
            add("binary_11_maxmsgsize_%d" % (10 + d), hdr(2, 11, mm), 11, 10 + d)
            add("close_10_maxmsgsize_%d" % (10 + d), hdr(8, 10, mm), 10, 10 + d)
        add("binary_maxmsgsize_no_flags_byte", hdr(2, 11, mm), 0, 5)
        add("binary_top_bit_size_maxmsgsize", hdr(2, 2 ** 63 + 5, mm), 8, 1000)
        add("ping_maxmsgsize_0", hdr(9, 1, mm), 1, 0)
        for op, size, form in ((2, 21, 125), (2, 21, 126), (2, 21, 127), (9, 20, 125), (8, 20, 127)):
            full = hdr(op, size, mm, form) + pattern(size)
            for cut in range(len(full) - size + 2):
                add("cut_op%d_form%d_at_%d" % (op, form, cut), full[:cut])
            add("cut_op%d_form%d_body" % (op, form), full[:-1])
        for fl in (0, 1, 2, 3, 0xFC, 0xFF):  # the flags byte on the wire (masked: XORed with key byte 0)
            add("flags_byte_%02x" % fl, hdr(2, 4, mm) + bytes([fl]) + b"abc")
        seq = hdr(2, 4, mm) + pattern(4) + hdr(9, 2, mm) + b"hi" + hdr(2, 9, mm) + pattern(9) + hdr(10, 0, mm) \
            + hdr(8, 2, mm) + b"\x03\xe8" + hdr(2, 2, mm) + b"zz"
        add("sequence", seq)
        add("sequence_then_bad_opcode", seq + b"\x81\x00")
    return cases


def encode_cases():
    """(must_mask, random, msg_t flags, body bytes): W + 1 = 125, 126, 65,535, 65,536"""
    cases = []
    for mm in (0, 1):
        for size in (125, 126, 65535, 65536):
            cases.append((mm, KEY, 0, size - 1))
        cases += [(mm, 0x01020304, 0, 5), (mm, 0xFFFFFFFF, 1, 5), (mm, 0, 2, 5), (mm, KEY, 3, 0)]
    return cases


def main():
    if not os.path.isfile(os.path.join(REF, "src", "ws_decoder.cpp")):
        sys.exit("make_ws_vectors: no reference sources at " + REF)
    dcases, ecases = decode_cases(), encode_cases()
    lines = []
    for _, mm, maxmsg, prefix, plen in dcases:
        data = (prefix + pattern(plen)).hex() or "-"
        for step in (0, 1):
            lines.append("D %d %d %d %s" % (mm, maxmsg, step, data))
    for mm, rnd, fl, n in ecases:
        lines.append("E %d %d %d %s" % (mm, rnd, fl, pattern(n).hex() or "-"))
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, check=True,
                             universal_newlines=True).stdout.splitlines()
    assert len(out) == len(lines), (len(out), len(lines))

    def answer(line):
        t = line.split()
        rc, fed, err, n = int(t[0]), int(t[1]), int(t[2]), int(t[3])
        assert len(t) == 4 + 2 * n
        msgs = [dict(flags=int(t[4 + 2 * i]), **blob(bytes.fromhex(t[5 + 2 * i].replace("-", "")))) for i in range(n)]
        return dict(rc=rc, fed=fed, errno=err, msgs=msgs)

    dec = []
    for i, (name, mm, maxmsg, prefix, plen) in enumerate(dcases):
        dec.append(dict(name=name, must_mask=mm, maxmsgsize=maxmsg, prefix=prefix.hex(), pattern_len=plen,
                        whole=answer(out[2 * i]), bytewise=answer(out[2 * i + 1])))
    enc = []
    for (mm, rnd, fl, n), line in zip(ecases, out[2 * len(dcases):]):
        enc.append(dict(must_mask=mm, random=rnd, flags=fl, body_pattern_len=n,
                        out=blob(bytes.fromhex(line.replace("-", "")))))
    doc = dict(source="the reference's ws_decoder_t / ws_encoder_t driven by tests/host/ws_ref_vectors.cpp",
               pattern="byte j of a pattern run is (7 j + 3) mod 256", key=KEY, decode=dec, encode=enc)
    path = os.path.join(HERE, "ws_vectors.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("make_ws_vectors: %d decode and %d encode records -> %s (%d bytes)" % (len(dec), len(enc), path,
                                                                                  os.path.getsize(path)))


if __name__ == "__main__":
    main()
