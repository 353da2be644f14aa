"""The handshake model (tests/curve_handshake_model.py) pinned to libsodium
1.0.18 through tests/golden/box_vectors.json: the fixture's first 36 items are
six complete handshake transcripts of six boxes each (hello, cookie, welcome,
vouch, initiate, ready; tests/golden/make_box_vectors.py), and the model's
server must reproduce each WELCOME, state, INITIATE verdict and READY from the
transcript's inputs byte for byte.  Then each reject rule of
zmqg_curve_server_hello_batch / _initiate_batch (include/zmqg_curve.h;
reference src/curve_server.cpp:117-383) once against the model."""
import json
import os

import numpy as np
import pytest

from tests import curve_handshake_model as M

VEC = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "box_vectors.json")))["items"]
H = bytes.fromhex


TRANSCRIPTS = M.golden_transcripts()


def test_fixture_is_six_transcripts():
    """What the transcripts rest on: one key opens HELLO and seals WELCOME, one
    key (crypto_box_beforenm(C', s')) seals INITIATE and READY."""
    for j in range(6):
        hello, cookie, welcome, vouch, initiate, ready = VEC[6 * j:6 * j + 6]
        assert hello["key"] == welcome["key"]
        assert initiate["key"] == ready["key"]
        assert M.O.box_beforenm(H(cookie["m"])[:32], H(cookie["m"])[32:]) == (0, H(ready["key"]))
        assert H(welcome["m"]) == M.public(H(cookie["m"])[32:]) + H(cookie["nonce"])[8:] + H(cookie["c"])
        assert 163 <= len(H(initiate["m"])) <= 198 and 35 <= len(H(ready["m"])) <= 70
        assert H(initiate["m"])[32:128] == H(vouch["nonce"])[8:] + H(vouch["c"])


@pytest.mark.parametrize("j", range(6))
def test_server_reproduces_transcript(j):
    t = TRANSCRIPTS[j]
    st, welcome, state = M.server_hello(t["server_sk"], t["hello"], t["random"])
    assert st == 0
    assert welcome == t["welcome"]
    assert state == t["state"]
    st, c, precom, peer, meta = M.server_initiate(state, t["initiate"])
    assert (st, c, precom, peer, meta) == (0, t["client_pk"], t["precom"], t["peer_nonce"], t["meta"])
    assert M.server_ready(precom, t["ready_nonce"], t["ready_meta"]) == t["ready"]


@pytest.mark.parametrize("j", range(6))
def test_client_side_of_transcript(j):
    """The client functions make the fixture's HELLO and open what the server sent."""
    t = TRANSCRIPTS[j]
    assert M.client_hello(t["server_pk"], t["cn_sk"], int.from_bytes(t["hello"][112:120], "big")) == t["hello"]
    sn_pk, cookie = M.client_open_welcome(t["welcome"], t["server_pk"], t["cn_sk"])
    assert sn_pk == M.public(t["random"][:32]) and cookie == t["initiate"][9:105]
    assert M.client_open_ready(t["ready"], t["precom"]) == t["ready_meta"]
    assert M.client_open_ready(t["ready"][:-1] + bytes([t["ready"][-1] ^ 1]), t["precom"]) is None


SERVER_SK = bytes(range(1, 33))
HS = M.random_handshake(np.random.default_rng(2024), SERVER_SK, meta_len=40)


@pytest.mark.parametrize("name,cmd,want", M.hello_cases(HS), ids=[c[0] for c in M.hello_cases(HS)])
def test_hello_rule(name, cmd, want):
    st, welcome, state = M.server_hello(SERVER_SK, cmd, HS["random"])
    assert st == want
    if want != 0:
        assert welcome == bytes(168) and state == bytes(128)
    else:
        assert M.client_open_welcome(welcome, HS["server_pk"], HS["cn_sk"]) is not None


@pytest.mark.parametrize("name,cmd,want", M.initiate_cases(HS, SERVER_SK),
                         ids=[c[0] for c in M.initiate_cases(HS, SERVER_SK)])
def test_initiate_rule(name, cmd, want):
    st, c, precom, peer, meta = M.server_initiate(HS["state"], cmd)
    assert st == want
    if want != 0:
        assert (c, precom, peer, meta) == (bytes(32), bytes(32), 0, None)
    else:
        assert (c, precom, peer) == (HS["client_pk"], HS["precom"], HS["peer_nonce"])
        assert meta == cmd_meta(cmd)


def cmd_meta(cmd):
    rc, plain = M.O.box_open_easy_afternm(cmd[113:], b"CurveZMQINITIATE" + cmd[105:113], HS["precom"])
    assert rc == 0
    return plain[128:]


def test_every_status_code_is_reached():
    got = {c[2] for c in M.hello_cases(HS)} | {c[2] for c in M.initiate_cases(HS, SERVER_SK)}
    assert got == {0, M.ERR_MALFORMED_UNSPECIFIED, M.ERR_UNEXPECTED_COMMAND, M.ERR_MALFORMED_HELLO,
                   M.ERR_MALFORMED_INITIATE, M.ERR_CRYPTOGRAPHIC, M.ERR_KEY_EXCHANGE}
