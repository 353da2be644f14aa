"""Pure-Python model of the client's CURVE handshake steps -- test
infrastructure, not a test.

The three functions state the contract of zmqg_curve_client_hello_batch /
_welcome_batch / _ready_batch (include/zmqg_curve.h) item by item: the
reference's crypto_box_keypair + produce_hello, process_welcome +
produce_initiate (src/curve_client_tools.hpp:29-234) and process_ready up to
parse_metadata (src/curve_client.cpp:179-214), with what the reference draws
with randombytes passed in.  Boxes and ladders come from the CPU oracle
(oracle.oracle); the server's side and the shared helpers from
tests/curve_handshake_model.py."""
from oracle import oracle as O
from tests import curve_handshake_model as M

ERR_UNEXPECTED_COMMAND = M.ERR_UNEXPECTED_COMMAND
ERR_CRYPTOGRAPHIC = M.ERR_CRYPTOGRAPHIC
ERR_MALFORMED_READY = 0x10000016  # include/zmq.h:433
HELLO_BYTES, STATE_BYTES = 200, 128
be64 = M.be64


def client_hello(server_pk, cn_secret, nonce):
    """(status, hello, state): 200 and 128 bytes, zeros where
    crypto_box(.., S, c') fails (a small-order S)."""
    rc, k1 = O.box_beforenm(server_pk, cn_secret)
    if rc != 0:
        return ERR_CRYPTOGRAPHIC, bytes(HELLO_BYTES), bytes(STATE_BYTES)
    cn_pk = M.public(cn_secret)
    box = O.box_easy_afternm(bytes(64), b"CurveZMQHELLO---" + be64(nonce), k1)
    hello = b"\x05HELLO\x01\x00" + bytes(72) + cn_pk + be64(nonce) + box
    return 0, hello, cn_pk + cn_secret + k1 + server_pk


def client_welcome(state, client_pk, client_sk, cmd, vouch_nonce, nonce, meta):
    """(status, initiate, precom); on failure (code, None, 32 zeros): no
    byte of the INITIATE is written."""
    fail = lambda code: (code, None, bytes(32))
    assert len(state) == STATE_BYTES and len(vouch_nonce) == 16
    cn_pk, cn_secret, k1, server_pk = state[0:32], state[32:64], state[64:96], state[96:128]
    if len(cmd) < 8 or cmd[:8] != b"\x07WELCOME":
        return fail(ERR_UNEXPECTED_COMMAND)
    if len(cmd) != 168:
        return fail(ERR_CRYPTOGRAPHIC)
    rc, plain = O.box_open_easy_afternm(cmd[24:], b"WELCOME-" + cmd[8:24], k1)
    if rc != 0:
        return fail(ERR_CRYPTOGRAPHIC)
    sn_pk, cookie = plain[:32], plain[32:128]
    rc, precom = O.box_beforenm(sn_pk, cn_secret)
    if rc != 0:
        return fail(ERR_CRYPTOGRAPHIC)  # the reference asserts (src/curve_client_tools.hpp:105-106)
    rc, kv = O.box_beforenm(sn_pk, client_sk)
    assert rc == 0  # the same point passed the ladder with c'
    vouch_box = O.box_easy_afternm(cn_pk + server_pk, b"VOUCH---" + vouch_nonce, kv)
    box = O.box_easy_afternm(client_pk + vouch_nonce + vouch_box + meta, b"CurveZMQINITIATE" + be64(nonce), precom)
    return 0, b"\x08INITIATE" + cookie + be64(nonce) + box, precom


def client_ready(precom, cmd):
    """(status, peer_nonce, meta); on failure (code, 0, None)."""
    fail = lambda code: (code, 0, None)
    if len(cmd) < 6 or cmd[:6] != b"\x05READY":
        return fail(ERR_UNEXPECTED_COMMAND)
    if len(cmd) < 30:
        return fail(ERR_MALFORMED_READY)
    rc, meta = O.box_open_easy_afternm(cmd[14:], b"CurveZMQREADY---" + cmd[6:14], precom)
    if rc != 0:
        return fail(ERR_CRYPTOGRAPHIC)
    return 0, int.from_bytes(cmd[6:14], "big"), meta


def client_state(hs, nonce=1):
    """The state record the HELLO call leaves for handshake `hs`
    (curve_handshake_model.random_handshake)."""
    st, _, state = client_hello(hs["server_pk"], hs["cn_sk"], nonce)
    assert st == 0
    return state


def welcome_with(hs, sn_pk, welcome_nonce=bytes(range(16))):
    """A WELCOME whose box is valid for hs's client and holds a chosen S'."""
    rc, k1 = O.box_beforenm(hs["server_pk"], hs["cn_sk"])
    assert rc == 0
    return b"\x07WELCOME" + welcome_nonce + O.box_easy_afternm(sn_pk + hs["cookie"], b"WELCOME-" + welcome_nonce, k1)


def welcome_cases(hs):
    """(name, command, status the rules give) against client_state(hs): every
    WELCOME reject rule, inputs that break two rules at once (the earlier rule
    wins), and what the reference accepts."""
    w = hs["welcome"]
    flip = M._flip
    ready = M.server_ready(hs["precom"], 1, hs["meta"])
    # the same server answering another client's HELLO (its key is the one
    # that client shares with S), and another server answering ours
    rc, k = O.box_beforenm(hs["server_pk"], bytes(range(40, 72)))
    assert rc == 0
    for_other = w[:24] + O.box_easy_afternm(hs["sn_pk"] + hs["cookie"], b"WELCOME-" + w[8:24], k)
    other_sk = bytes(range(3, 35))
    st, by_other, _ = M.server_hello(other_sk, M.client_hello(M.public(other_sk), hs["cn_sk"], 1), hs["random"])
    assert st == 0 and len(by_other) == 168
    return [
        ("valid", w, 0),
        ("a valid box with another S'", welcome_with(hs, M.public(bytes(range(9, 41)))), 0),
        ("empty", b"", ERR_UNEXPECTED_COMMAND),
        ("one byte", b"\x07", ERR_UNEXPECTED_COMMAND),
        ("short of the name", b"\x07WELCOM", ERR_UNEXPECTED_COMMAND),
        ("wrong name", b"\x07WELCOMF" + w[8:], ERR_UNEXPECTED_COMMAND),
        ("wrong name length byte", b"\x08WELCOME" + w[8:], ERR_UNEXPECTED_COMMAND),
        ("wrong name and wrong size", b"\x07XELCOME" + w[8:100], ERR_UNEXPECTED_COMMAND),
        ("a READY", ready, ERR_UNEXPECTED_COMMAND),
        ("an ERROR", b"\x05ERROR\x05nope!", ERR_UNEXPECTED_COMMAND),
        ("the name alone", w[:8], ERR_CRYPTOGRAPHIC),
        ("167 bytes", w[:167], ERR_CRYPTOGRAPHIC),
        ("169 bytes", w + b"\x00", ERR_CRYPTOGRAPHIC),
        ("box tag bit", flip(w, 24 + 5, 3), ERR_CRYPTOGRAPHIC),
        ("box ciphertext bit", flip(w, 40 + 70, 6), ERR_CRYPTOGRAPHIC),
        ("nonce bit", flip(w, 8 + 3, 1), ERR_CRYPTOGRAPHIC),
        ("last byte", flip(w, 167, 7), ERR_CRYPTOGRAPHIC),
        ("sealed for another C'", for_other, ERR_CRYPTOGRAPHIC),
        ("sealed by another server", by_other, ERR_CRYPTOGRAPHIC),
        ("S' = 0 inside a valid box", welcome_with(hs, bytes(32)), ERR_CRYPTOGRAPHIC),
        ("S' = 1 inside a valid box", welcome_with(hs, b"\x01" + bytes(31)), ERR_CRYPTOGRAPHIC),
    ]


def ready_cases(hs):
    """(name, command, status the rules give) against hs["precom"]."""
    assert len(hs["meta"]) >= 8, "the base handshake needs some metadata"
    r = M.server_ready(hs["precom"], 1, hs["meta"])
    flip = M._flip
    empty = M.server_ready(hs["precom"], 2 ** 64 - 1, b"")
    assert len(empty) == 30
    return [
        ("valid", r, 0),
        ("30 bytes: no metadata", empty, 0),
        ("empty", b"", ERR_UNEXPECTED_COMMAND),
        ("short of the name", b"\x05READ", ERR_UNEXPECTED_COMMAND),
        ("wrong name", b"\x05READZ" + r[6:], ERR_UNEXPECTED_COMMAND),
        ("wrong name and too short", b"\x05REEDY" + r[6:20], ERR_UNEXPECTED_COMMAND),
        ("a WELCOME", hs["welcome"], ERR_UNEXPECTED_COMMAND),
        ("an ERROR", b"\x05ERROR\x05nope!", ERR_UNEXPECTED_COMMAND),
        ("the name alone", r[:6], ERR_MALFORMED_READY),
        ("29 bytes", empty[:29], ERR_MALFORMED_READY),
        ("box tag bit", flip(r, 14 + 2, 5), ERR_CRYPTOGRAPHIC),
        ("box ciphertext bit", flip(r, 30 + 3, 2), ERR_CRYPTOGRAPHIC),
        ("nonce bit", flip(r, 6 + 7), ERR_CRYPTOGRAPHIC),
        ("last byte", flip(r, len(r) - 1, 7), ERR_CRYPTOGRAPHIC),
        ("30 bytes with a broken tag", flip(empty, 29, 4), ERR_CRYPTOGRAPHIC),
        ("a READY under another precom", M.server_ready(bytes(range(50, 82)), 1, hs["meta"]), ERR_CRYPTOGRAPHIC),
    ]
