"""The client model (tests/curve_client_model.py) pinned to libsodium: for
each of the six libsodium 1.0.18 handshake transcripts of
tests/golden/box_vectors.json the model must reproduce the fixture's HELLO,
k1, INITIATE and precom byte for byte from the client's secrets (the `hello`
item's sk = c', the `vouch` item's sk = c and the vouch nonce), and open the
fixture's READY.  Then every case of welcome_cases / ready_cases once against
the model.  No GPU."""
import functools
import json
import os

import numpy as np
import pytest

from tests import curve_client_model as CM
from tests import curve_handshake_model as M

SERVER_SK = bytes(range(1, 33))


@functools.lru_cache(maxsize=None)
def transcripts():
    """golden_transcripts() plus the client-side secrets of each."""
    here = os.path.dirname(os.path.abspath(__file__))
    vec = json.load(open(os.path.join(here, "golden", "box_vectors.json")))["items"]
    T = M.golden_transcripts()
    for j, t in enumerate(T):
        hello, vouch = vec[6 * j], vec[6 * j + 3]
        assert hello["kind"] == "hello" and vouch["kind"] == "vouch"
        t["k1"] = bytes.fromhex(hello["key"])
        t["client_sk"] = bytes.fromhex(vouch["sk"])
        t["vouch_nonce"] = bytes.fromhex(vouch["nonce"])[8:]
        t["hello_nonce"] = int.from_bytes(t["hello"][112:120], "big")
    return T


@functools.lru_cache(maxsize=None)
def base_hs():
    return M.random_handshake(np.random.default_rng(2024), SERVER_SK, meta_len=40)


@pytest.mark.parametrize("j", range(6))
def test_model_reproduces_the_libsodium_transcript(j):
    t = transcripts()[j]
    st, hello, state = CM.client_hello(t["server_pk"], t["cn_sk"], t["hello_nonce"])
    assert st == 0
    assert hello == t["hello"]
    assert state[0:32] == t["cn_pk"] and state[32:64] == t["cn_sk"] and state[96:128] == t["server_pk"]
    assert state[64:96] == t["k1"]
    st, initiate, precom = CM.client_welcome(state, t["client_pk"], t["client_sk"], t["welcome"], t["vouch_nonce"],
                                             t["peer_nonce"], t["meta"])
    assert st == 0
    assert initiate == t["initiate"]
    assert precom == t["precom"]
    assert CM.client_ready(precom, t["ready"]) == (0, t["ready_nonce"], t["ready_meta"])


def test_small_order_server_key_is_rejected_at_hello():
    for pk in (bytes(32), b"\x01" + bytes(31)):
        assert CM.client_hello(pk, bytes(range(32)), 1) == (CM.ERR_CRYPTOGRAPHIC, bytes(200), bytes(128))


def test_welcome_cases_against_the_model():
    hs = base_hs()
    state = CM.client_state(hs)
    cases = CM.welcome_cases(hs)
    for name, cmd, code in cases:
        st, initiate, precom = CM.client_welcome(state, hs["client_pk"], hs["client_sk"], cmd, bytes(16), 2,
                                                 hs["meta"])
        assert st == code, (name, hex(st), hex(code))
        if code != 0:
            assert initiate is None and precom == bytes(32), name
        else:
            assert len(initiate) == 257 + len(hs["meta"]) and precom != bytes(32), name
    # the valid WELCOME gives the INITIATE the server model accepts, and the server's precom
    st, initiate, precom = CM.client_welcome(state, hs["client_pk"], hs["client_sk"], hs["welcome"], bytes(16), 2,
                                             hs["meta"])
    assert M.server_initiate(hs["state"], initiate) == (0, hs["client_pk"], hs["precom"], 2, hs["meta"])
    assert precom == hs["precom"]
    assert {c[2] for c in cases} == {0, CM.ERR_UNEXPECTED_COMMAND, CM.ERR_CRYPTOGRAPHIC}
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)


def test_ready_cases_against_the_model():
    hs = base_hs()
    cases = CM.ready_cases(hs)
    for name, cmd, code in cases:
        st, peer, meta = CM.client_ready(hs["precom"], cmd)
        assert st == code, (name, hex(st), hex(code))
        if code != 0:
            assert peer == 0 and meta is None, name
    assert CM.client_ready(hs["precom"], cases[0][1]) == (0, 1, hs["meta"])
    assert CM.client_ready(hs["precom"], cases[1][1]) == (0, 2 ** 64 - 1, b"")
    assert {c[2] for c in cases} == {0, CM.ERR_UNEXPECTED_COMMAND, CM.ERR_MALFORMED_READY, CM.ERR_CRYPTOGRAPHIC}
