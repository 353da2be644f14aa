"""Pure-Python model of the CURVE handshake -- test infrastructure, not a test.

The server functions state the contract of zmqg_curve_server_hello_batch /
_initiate_batch / _ready_batch (include/zmqg_curve.h) item by item: the
reference's curve_server_t::process_hello, produce_welcome, process_initiate
and produce_ready (src/curve_server.cpp:117-458), the checks in the reference's
order.  The client functions produce and open the commands a curve_client_t
would (src/curve_client_tools.hpp:36-180, src/curve_client.cpp:180-230), with
overrides for the hostile cases a real client cannot make.  Boxes and ladders
come from the CPU oracle (oracle.oracle)."""
import json
import os

from oracle import oracle as O

ERR_UNEXPECTED_COMMAND = 0x10000001  # include/zmq.h:424-437
ERR_KEY_EXCHANGE = 0x10000003
ERR_MALFORMED_UNSPECIFIED = 0x10000011
ERR_MALFORMED_HELLO = 0x10000013
ERR_MALFORMED_INITIATE = 0x10000014
ERR_CRYPTOGRAPHIC = 0x11000001
STATE_BYTES, RANDOM_BYTES, WELCOME_BYTES = 128, 96, 168
BASE_POINT = b"\x09" + bytes(31)


def be64(v):
    return int(v).to_bytes(8, "big")  # src/wire.hpp put_uint64


def public(sk):
    """crypto_scalarmult_base."""
    rc, pk = O.x25519(sk, BASE_POINT)
    assert rc == 0
    return pk


def _box(m, nonce, pk, sk):
    """crypto_box_easy: None where crypto_box_beforenm fails."""
    rc, k = O.box_beforenm(pk, sk)
    return None if rc != 0 else O.box_easy_afternm(m, nonce, k)


def _box_open(c, nonce, pk, sk):
    """crypto_box_open_easy: the plaintext, or None."""
    rc, k = O.box_beforenm(pk, sk)
    if rc != 0:
        return None
    rc, m = O.box_open_easy_afternm(c, nonce, k)
    return m if rc == 0 else None


def _basic_structure_ok(cmd):
    """check_basic_command_structure (src/mechanism_base.cpp:14-25)."""
    return not (len(cmd) <= 1 or len(cmd) <= cmd[0])


# ------------------------------------------------------------------ client
def client_hello(server_pk, cn_sk, nonce, cn_pk=None):
    """produce_hello (src/curve_client_tools.hpp:36-71).  cn_pk: a chosen C'
    written into the command instead of the public key of cn_sk."""
    box = _box(bytes(64), b"CurveZMQHELLO---" + be64(nonce), server_pk, cn_sk)
    return b"\x05HELLO\x01\x00" + bytes(72) + (public(cn_sk) if cn_pk is None else cn_pk) + be64(nonce) + box


def client_open_welcome(welcome, server_pk, cn_sk):
    """process_welcome (src/curve_client_tools.hpp:73-110): (S', cookie) with
    cookie = cookie nonce(16) || cookie box(80), or None."""
    if len(welcome) != 168 or welcome[:8] != b"\x07WELCOME":
        return None
    m = _box_open(welcome[24:], b"WELCOME-" + welcome[8:24], server_pk, cn_sk)
    return None if m is None else (m[:32], m[32:128])


def client_initiate(client_pk, client_sk, server_pk, cn_sk, sn_pk, cookie, nonce, meta, vouch_nonce=bytes(16),
                    vouch_plain=None, chosen_c=None, vouch_box=None):
    """produce_initiate (src/curve_client_tools.hpp:112-195).  Overrides:
    vouch_plain, a foreign vouch plaintext (64 bytes) instead of C' || S;
    vouch_box, a ready-made vouch box (80 bytes); `cookie`, any 96 bytes (a
    foreign cookie box); chosen_c, the C written into the box instead of
    client_pk."""
    cn_pk = public(cn_sk)
    if vouch_box is None:
        plain = cn_pk + server_pk if vouch_plain is None else vouch_plain
        vouch_box = _box(plain, b"VOUCH---" + vouch_nonce, sn_pk, client_sk)
    c = client_pk if chosen_c is None else chosen_c
    box = _box(c + vouch_nonce + vouch_box + meta, b"CurveZMQINITIATE" + be64(nonce), sn_pk, cn_sk)
    return b"\x08INITIATE" + cookie + be64(nonce) + box


def client_open_ready(ready, precom):
    """process_ready (src/curve_client.cpp:180-230): the metadata, or None."""
    if len(ready) < 30 or ready[:6] != b"\x05READY":
        return None
    rc, m = O.box_open_easy_afternm(ready[14:], b"CurveZMQREADY---" + ready[6:14], precom)
    return m if rc == 0 else None


# ------------------------------------------------------------------ server
def server_hello(server_sk, cmd, random96):
    """(status, welcome, state): 168 and 128 bytes, zeros on failure."""
    fail = lambda code: (code, bytes(WELCOME_BYTES), bytes(STATE_BYTES))
    assert len(random96) == RANDOM_BYTES
    if not _basic_structure_ok(cmd):
        return fail(ERR_MALFORMED_UNSPECIFIED)
    if len(cmd) < 6 or cmd[:6] != b"\x05HELLO":
        return fail(ERR_UNEXPECTED_COMMAND)
    if len(cmd) != 200:
        return fail(ERR_MALFORMED_HELLO)
    if cmd[6] != 1 or cmd[7] != 0:
        return fail(ERR_MALFORMED_HELLO)
    cn_client = cmd[80:112]
    if _box_open(cmd[120:200], b"CurveZMQHELLO---" + cmd[112:120], cn_client, server_sk) is None:
        return fail(ERR_CRYPTOGRAPHIC)
    cn_secret, cookie_key = random96[0:32], random96[32:64]
    cookie_nonce, welcome_nonce = random96[64:80], random96[80:96]
    cookie_box = O.box_easy_afternm(cn_client + cn_secret, b"COOKIE--" + cookie_nonce, cookie_key)
    box = _box(public(cn_secret) + cookie_nonce + cookie_box, b"WELCOME-" + welcome_nonce, cn_client, server_sk)
    rc, precom = O.box_beforenm(cn_client, cn_secret)
    assert rc == 0  # C' passed the ladder with server_sk, so it is not of small order
    return 0, b"\x07WELCOME" + welcome_nonce + box, cn_client + cn_secret + cookie_key + precom


def server_initiate(state, cmd):
    """(status, C, precom, peer_nonce, meta); on failure (code, 32 zeros,
    32 zeros, 0, None): no metadata byte is written."""
    fail = lambda code: (code, bytes(32), bytes(32), 0, None)
    assert len(state) == STATE_BYTES
    cn_client, cn_secret, cookie_key, precom = state[0:32], state[32:64], state[64:96], state[96:128]
    if not _basic_structure_ok(cmd):
        return fail(ERR_MALFORMED_UNSPECIFIED)
    if len(cmd) < 9 or cmd[:9] != b"\x08INITIATE":
        return fail(ERR_UNEXPECTED_COMMAND)
    if len(cmd) < 257:
        return fail(ERR_MALFORMED_INITIATE)
    rc, cookie_plain = O.box_open_easy_afternm(cmd[25:105], b"COOKIE--" + cmd[9:25], cookie_key)
    if rc != 0:
        return fail(ERR_CRYPTOGRAPHIC)
    if cookie_plain != cn_client + cn_secret:
        return fail(ERR_CRYPTOGRAPHIC)
    rc, plain = O.box_open_easy_afternm(cmd[113:], b"CurveZMQINITIATE" + cmd[105:113], precom)
    if rc != 0:
        return fail(ERR_CRYPTOGRAPHIC)
    client_key = plain[0:32]
    vouch = _box_open(plain[48:128], b"VOUCH---" + plain[32:48], client_key, cn_secret)
    if vouch is None:
        return fail(ERR_CRYPTOGRAPHIC)
    if vouch[0:32] != cn_client:
        return fail(ERR_KEY_EXCHANGE)
    return 0, client_key, precom, int.from_bytes(cmd[105:113], "big"), plain[128:]


def server_ready(precom, nonce, meta):
    """produce_ready: "\\x05READY" || BE64(nonce) || box(meta)."""
    return b"\x05READY" + be64(nonce) + O.box_easy_afternm(meta, b"CurveZMQREADY---" + be64(nonce), precom)


# ------------------------------------------------------------------ whole handshakes
def random_handshake(rng, server_sk, meta_len=None, hello_nonce=1):
    """One valid handshake with random keys: a dict of everything the client
    and the server hold and exchange (the server side from the model)."""
    rb = lambda n: rng.integers(0, 256, n, dtype="uint8").tobytes()
    server_pk = public(server_sk)
    client_sk, cn_sk = rb(32), rb(32)
    client_pk = public(client_sk)
    random96 = rb(RANDOM_BYTES)
    hello = client_hello(server_pk, cn_sk, hello_nonce)
    st, welcome, state = server_hello(server_sk, hello, random96)
    assert st == 0
    sn_pk, cookie = client_open_welcome(welcome, server_pk, cn_sk)
    meta = rb(int(rng.integers(0, 120)) if meta_len is None else meta_len)
    initiate = client_initiate(client_pk, client_sk, server_pk, cn_sk, sn_pk, cookie, hello_nonce + 1, meta, rb(16))
    st, c, precom, peer, got_meta = server_initiate(state, initiate)
    assert st == 0 and c == client_pk and got_meta == meta and peer == hello_nonce + 1
    return dict(server_pk=server_pk, client_pk=client_pk, client_sk=client_sk, cn_sk=cn_sk, sn_pk=sn_pk,
                cookie=cookie, random=random96, hello=hello, welcome=welcome, state=state, initiate=initiate,
                precom=precom, peer_nonce=peer, meta=meta)


def _flip(b, pos, bit=0):
    b = bytearray(b)
    b[pos] ^= 1 << bit
    return bytes(b)


def hello_cases(hs, initiate_cmd=None):
    """(name, command, status the rules give) for one handshake `hs`
    (random_handshake): every HELLO reject rule, inputs that break two rules
    at once (the earlier rule wins), and inputs the reference accepts."""
    h = hs["hello"]
    other = client_hello(public(bytes(range(32))), hs["cn_sk"], 1)  # sealed for another server
    return [
        ("valid", h, 0),
        ("padding bytes are not inspected", h[:8] + bytes(range(1, 73)) + h[80:], 0),
        ("empty", b"", ERR_MALFORMED_UNSPECIFIED),
        ("one byte", b"\x05", ERR_MALFORMED_UNSPECIFIED),
        ("name length == size, wrong name too", b"\xc8" + h[1:], ERR_MALFORMED_UNSPECIFIED),
        ("name length == size 5", b"\x05HELL", ERR_MALFORMED_UNSPECIFIED),
        ("shorter than the name", b"\x03HELL", ERR_UNEXPECTED_COMMAND),
        ("wrong name", b"\x05HELLP" + h[6:], ERR_UNEXPECTED_COMMAND),
        ("wrong name and wrong size", b"\x05JELLO" + h[6:150], ERR_UNEXPECTED_COMMAND),
        ("an INITIATE", hs["initiate"] if initiate_cmd is None else initiate_cmd, ERR_UNEXPECTED_COMMAND),
        ("199 bytes", h[:199], ERR_MALFORMED_HELLO),
        ("201 bytes", h + b"\x00", ERR_MALFORMED_HELLO),
        ("wrong size and wrong version", h[:6] + b"\x02\x00" + h[8:190], ERR_MALFORMED_HELLO),
        ("version 1.1", h[:7] + b"\x01" + h[8:], ERR_MALFORMED_HELLO),
        ("version 2.0", h[:6] + b"\x02" + h[7:], ERR_MALFORMED_HELLO),
        ("wrong version and broken box", _flip(h[:6] + b"\x00" + h[7:], 150), ERR_MALFORMED_HELLO),
        ("box tag bit", _flip(h, 120 + 5, 3), ERR_CRYPTOGRAPHIC),
        ("box ciphertext bit", _flip(h, 136 + 40, 6), ERR_CRYPTOGRAPHIC),
        ("last box bit", _flip(h, 199, 7), ERR_CRYPTOGRAPHIC),
        ("short nonce bit", _flip(h, 119), ERR_CRYPTOGRAPHIC),
        ("C' bit", _flip(h, 80 + 13, 2), ERR_CRYPTOGRAPHIC),
        ("sealed for another server", other, ERR_CRYPTOGRAPHIC),
        ("C' = 0", h[:80] + bytes(32) + h[112:], ERR_CRYPTOGRAPHIC),
        ("C' = 1", h[:80] + b"\x01" + bytes(31) + h[112:], ERR_CRYPTOGRAPHIC),
    ]


def initiate_cases(hs, server_sk):
    """(name, command, status the rules give) against hs["state"]: every
    INITIATE reject rule, two rules at once, and what the reference accepts."""
    server_pk = public(server_sk)
    ini = hs["initiate"]
    assert len(ini) >= 257 + 8, "the base handshake needs some metadata"
    cn_pk = public(hs["cn_sk"])
    state = hs["state"]
    cookie_key = state[64:96]
    cnonce = hs["cookie"][:16]
    vn = bytes(range(100, 116))

    def build(**kw):
        args = dict(cookie=hs["cookie"], nonce=hs["peer_nonce"], meta=hs["meta"], vouch_nonce=vn)
        args.update(kw)
        return client_initiate(hs["client_pk"], hs["client_sk"], server_pk, hs["cn_sk"], hs["sn_pk"], **args)

    foreign_cookie = cnonce + O.box_easy_afternm(cn_pk + bytes(range(32)), b"COOKIE--" + cnonce, cookie_key)
    good_vouch = _box(cn_pk + server_pk, b"VOUCH---" + vn, hs["sn_pk"], hs["client_sk"])
    stranger_sk = bytes(range(7, 39))
    empty = build(meta=b"")
    assert len(empty) == 257
    return [
        ("valid", ini, 0),
        ("257 bytes: no metadata", empty, 0),
        ("the vouch's second half is not inspected", build(vouch_plain=cn_pk + bytes(32)), 0),
        ("empty", b"", ERR_MALFORMED_UNSPECIFIED),
        ("one byte", b"\x08", ERR_MALFORMED_UNSPECIFIED),
        ("name length beyond the size, wrong name too", b"\xff" + ini[1:255], ERR_MALFORMED_UNSPECIFIED),
        ("shorter than the name", b"\x03INITI", ERR_UNEXPECTED_COMMAND),
        ("wrong name", b"\x08INITIATF" + ini[9:], ERR_UNEXPECTED_COMMAND),
        ("wrong name and too short", b"\x08INITIATF" + ini[9:100], ERR_UNEXPECTED_COMMAND),
        ("a HELLO", hs["hello"], ERR_UNEXPECTED_COMMAND),
        ("256 bytes", empty[:256], ERR_MALFORMED_INITIATE),
        ("9 bytes", b"\x08INITIATE", ERR_MALFORMED_INITIATE),
        ("256 bytes and a broken cookie", _flip(empty[:256], 50), ERR_MALFORMED_INITIATE),
        ("cookie nonce bit", _flip(ini, 9 + 3, 1), ERR_CRYPTOGRAPHIC),
        ("cookie tag bit", _flip(ini, 25 + 15, 7), ERR_CRYPTOGRAPHIC),
        ("cookie ciphertext bit", _flip(ini, 41 + 63, 4), ERR_CRYPTOGRAPHIC),
        ("a valid cookie box with foreign content", build(cookie=foreign_cookie), ERR_CRYPTOGRAPHIC),
        ("short nonce bit", _flip(ini, 105 + 7), ERR_CRYPTOGRAPHIC),
        ("box tag bit", _flip(ini, 113 + 8, 5), ERR_CRYPTOGRAPHIC),
        ("ciphertext bit in C", _flip(ini, 129 + 1, 2), ERR_CRYPTOGRAPHIC),
        ("ciphertext bit in the vouch", _flip(ini, 129 + 60, 6), ERR_CRYPTOGRAPHIC),
        ("ciphertext bit in the metadata", _flip(ini, 129 + 128 + 3, 1), ERR_CRYPTOGRAPHIC),
        ("last ciphertext bit", _flip(ini, len(ini) - 1, 7), ERR_CRYPTOGRAPHIC),
        ("vouch box bit (inside a valid box)", build(vouch_box=_flip(good_vouch, 30, 3)), ERR_CRYPTOGRAPHIC),
        ("vouch tag bit (inside a valid box)", build(vouch_box=_flip(good_vouch, 2, 0)), ERR_CRYPTOGRAPHIC),
        ("a vouch sealed by another key than C", build(chosen_c=public(stranger_sk)), ERR_CRYPTOGRAPHIC),
        ("C = 0", build(chosen_c=bytes(32)), ERR_CRYPTOGRAPHIC),
        ("a valid vouch for a foreign C'", build(vouch_plain=public(stranger_sk) + server_pk), ERR_KEY_EXCHANGE),
        ("a foreign C' and a broken metadata byte",
         _flip(build(vouch_plain=public(stranger_sk) + server_pk), 129 + 128 + 1), ERR_CRYPTOGRAPHIC),
        ("a foreign cookie and a foreign C'",
         build(cookie=foreign_cookie, vouch_plain=public(stranger_sk) + server_pk), ERR_CRYPTOGRAPHIC),
    ]


def golden_transcripts():
    """The six libsodium 1.0.18 handshake transcripts at the head of
    tests/golden/box_vectors.json (six boxes each: hello, cookie, welcome,
    vouch, initiate, ready; tests/golden/make_box_vectors.py) as the commands
    and values of one connection each."""
    here = os.path.dirname(os.path.abspath(__file__))
    vec = json.load(open(os.path.join(here, "golden", "box_vectors.json")))["items"]
    H = bytes.fromhex
    out = []
    for j in range(6):
        it = vec[6 * j:6 * j + 6]
        assert [v["kind"] for v in it] == ["hello", "cookie", "welcome", "vouch", "initiate", "ready"]
        hello, cookie, welcome, vouch, initiate, ready = it
        cn_pk, sn_sk = H(cookie["m"])[:32], H(cookie["m"])[32:]
        t = dict(server_sk=H(welcome["sk"]), server_pk=H(hello["pk"]), cn_sk=H(hello["sk"]), cn_pk=cn_pk,
                 random=sn_sk + H(cookie["key"]) + H(cookie["nonce"])[8:] + H(welcome["nonce"])[8:],
                 hello=b"\x05HELLO\x01\x00" + bytes(72) + cn_pk + H(hello["nonce"])[16:] + H(hello["c"]),
                 welcome=b"\x07WELCOME" + H(welcome["nonce"])[8:] + H(welcome["c"]),
                 state=cn_pk + sn_sk + H(cookie["key"]) + H(ready["key"]),
                 initiate=b"\x08INITIATE" + H(cookie["nonce"])[8:] + H(cookie["c"]) + H(initiate["nonce"])[16:]
                 + H(initiate["c"]),
                 client_pk=H(initiate["m"])[:32], precom=H(ready["key"]), meta=H(initiate["m"])[128:],
                 peer_nonce=int.from_bytes(H(initiate["nonce"])[16:], "big"),
                 ready_nonce=int.from_bytes(H(ready["nonce"])[16:], "big"),
                 ready=b"\x05READY" + H(ready["nonce"])[16:] + H(ready["c"]), ready_meta=H(ready["m"]))
        assert H(welcome["pk"]) == cn_pk and len(t["hello"]) == 200 and len(t["welcome"]) == 168
        out.append(t)
    return out
