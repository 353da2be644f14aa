"""The CPU model of zmqg_decode_zmtp's parser (tests/zmtp_scan_model.py) over
the steered streams of tests/zmtp_scan_steer.py, against the oracle
(oracle/zmtp_oracle.py), with no GPU.  Per stream: the oracle alone gives the
outcome the case was built for (asserted first), then the model's result and
frames equal the oracle's -- for an early-stop stream (a planted LARGE header
covers frame k's start) the oracle's first k + 1 frames, and the calls
repeated from `consumed` the whole parse.  Per class: the coverage facts the
class is meant to reach, taken from the model, so that
tests/test_gpu_zmtp_scan_edges.py, which runs the same streams on the device,
is known to reach those edges."""
import pytest

from oracle import zmtp_oracle as Z
from tests import zmtp_scan_model as M
from tests import zmtp_scan_steer as S


def check(cs, ran, mis=0):
    """One stream: the oracle's outcome, then the model against the oracle.
    Returns the model's facts."""
    s = cs["stream"]
    full = Z.parse(s, cs["max_msg"], cs["max_frames"])
    assert dict(frames=len(full["frames"]), consumed=full["consumed"], error=full["error"]) == cs["want"], cs["name"]
    ref = full if cs["kth"] is None else Z.parse(s, cs["max_msg"], cs["kth"] + 1)
    got = M.decode(s, cs["max_msg"], cs["max_frames"], mis)
    assert got["frames"] == ref["frames"], cs["name"]
    assert (got["consumed"], got["error"]) == (ref["consumed"], ref["error"]), cs["name"]
    assert got["out_bytes"] == sum(max(f[2] - 33, 0) for f in ref["frames"])
    ran.append(cs["name"])
    return got["facts"]


def resumed(cs):
    """Calls repeated from `consumed` until one returns no frame."""
    s, pos, frames, calls = cs["stream"], 0, [], 0
    while True:
        r = M.decode(s[pos:], cs["max_msg"], cs["max_frames"], pos % 16)
        calls += 1
        assert r["error"] == 0
        if not r["frames"]:
            return frames, pos, calls
        frames += [(f, o + pos, l) for f, o, l in r["frames"]]
        pos += r["consumed"]


def check_a():
    cases, ran = S.class_a(), []
    assert len(cases) == len(S.edges()) * 33 * 2
    phases = dict(short=set(), large=set())
    hdr_before, tail_after = set(), set()
    for cs in cases:
        f = check(cs, ran)
        c = [x for x in f["cands"] if x["q"] == cs["q"]]
        assert len(c) == 1 and c[0]["kind"] == cs["kind"] and c[0]["p"] == cs["q"] - (9 if cs["kind"] == "large" else 2)
        c = c[0]
        phases[cs["kind"]].add(c["q"] % 16)
        for unit, name in ((1, "chunk"), (M.LANES, "round"), (M.tile() // M.CHUNK, "list")):
            if c["hdr_chunk"] // unit < c["chunk"] // unit:
                hdr_before.add((cs["kind"], name))
            if c["tail_chunk"] // unit > c["chunk"] // unit:
                tail_after.add(name)
        assert f["runs"] == 1 and f["unlinked"] == 1  # a clean stream
        if cs["B"] == S.GENERIC_EDGE:  # `in` at byte offsets 1, 4, 8, 15 of an allocation
            for mis in (1, 4, 8, 15):
                check(cs, [], mis)
    assert phases["short"] == phases["large"] == set(range(16))
    assert hdr_before == {(k, u) for k in ("short", "large") for u in ("chunk", "round", "list")}
    assert tail_after == {"chunk", "round", "list"}
    assert len(ran) == len(cases)
    return len(cases)


def check_b():
    cases, ran = S.class_b(), []
    assert len(cases) == 2 + 16 * (1 + 7 + 1 + 1 + 7)
    ends, paths = set(), set()
    for cs in cases:
        f = check(cs, ran)
        paths |= {x["path"] for x in f["cands"]}
        if "q" in cs:  # the first chunk is loaded byte by byte
            c = [x for x in f["cands"] if x["q"] == cs["q"]]
            assert len(c) == 1 and c[0]["chunk"] == 0 and c[0]["path"] == "bytewise"
        elif cs["name"] == "end%d" % cs["r"]:
            n = len(cs["stream"])
            last = f["cands"][-1]
            assert n % 16 == cs["r"] and last["q"] + 8 == n and last["path"] == "bytewise"
            assert any(x["path"] == "fast" for x in f["cands"])
            ends.add(n % 16)
        else:  # a cut last frame: no candidate for it
            assert f["cands"][-1]["q"] + 8 < cs["want"]["consumed"]
    assert ends == set(range(16)) and paths == {"fast", "bytewise"}
    assert len(ran) == len(cases)
    return len(cases)


def check_c():
    cases, ran = S.class_c(), []
    assert len(cases) == 5 + 9 + 9
    dropped = 0
    for cs in cases:
        f = check(cs, ran)
        dropped += f["shadows_dropped"]
        if cs["kth"] is None:
            assert f["shadows_dropped"] == cs["shadows"] and f["true_starts_dropped"] == 0
            continue
        k = cs["kth"]
        assert f["true_starts_dropped"] == 1 and f["shadows_dropped"] >= 1
        full = Z.parse(cs["stream"], cs["max_msg"], cs["max_frames"])
        frames, pos, calls = resumed(cs)
        assert frames == full["frames"] and pos == full["consumed"] == len(cs["stream"])
        # (the last frame covered: the first call already returns everything)
        assert calls == (2 if k + 1 == len(full["frames"]) else 3)
    assert dropped >= 1
    assert len(ran) == len(cases)
    return len(cases)


def check_d():
    cases, ran = S.class_d(), []
    assert len(cases) == 3
    for cs in cases:
        f = check(cs, ran)
        if cs.get("dense"):
            assert f["two_in_chunk"] and f["m"] >= 2002
            assert f["max_list_count"] >= M.tile() // 10 and f["max_passes"] == (f["max_list_count"] + 63) // 64 >= 26
            assert f["runs"] == 1
        if cs.get("sig8"):
            assert f["two_sigs_in_chunk"]
        if cs.get("flood"):
            lanes = {}
            for x in f["cands"]:
                lanes.setdefault((x["list"], x["round"]), set()).add(x["lane"])
            assert any(len(v) == M.LANES for v in lanes.values())
            assert f["unlinked"] >= 540 and f["jumps"] >= 1
    assert len(ran) == len(cases)
    return len(cases)


def check_e():
    cases, ran = S.class_e(), []
    assert len(cases) == 4 + 4
    for cs in cases:
        f = check(cs, ran)
        if cs.get("src") == "nb":  # the next unlinked candidate in the walker's own list
            assert f["next_src"][0] == "nb" and f["nwg"] == 1 and f["runs"] == 2 and f["jumps"] == 1
        if cs.get("src") == "first_w":  # ... in a later list
            assert f["next_src"][0] == "first_w" and f["first_w_not_last"] and f["runs"] == 2 and f["jumps"] == 1
        if cs.get("off_chain"):
            assert f["linked_off_chain"] == 1 and f["runs"] == 2
        if cs.get("gap"):
            assert f["max_lists_skipped"] >= 64 and f["runs"] == 1 and f["unlinked"] == 1
        if "cut" in cs:
            assert f["full"] == (cs["cut"] != "with-extra")
            assert f["runs"] == (1 if cs["cut"] in ("in-run", "run-end") else 2)
    assert len(ran) == len(cases)
    return len(cases)


def check_f(nlists):
    ran = []
    cs = S.long_case(nlists)
    f = check(cs, ran)
    assert f["nwg"] == nlists and f["per"] == (nlists + 1023) // 1024
    assert f["suffix_shape"] == ("regs" if f["per"] <= 8 else "loop")
    assert f["next_src"][0] == "first_w" and f["first_w_not_last"] and f["runs"] == 2 and f["jumps"] == 1
    assert f["max_lists_skipped"] >= 64
    assert f["inline_sum"] == (nlists <= 8192)
    assert len(ran) == 1
    return 1


def check_g():
    cases, ran = S.class_g(), []
    assert len(cases) == 9 + 4 + 2
    errors = set()
    for cs in cases:
        check(cs, ran)
        errors.add(cs["want"]["error"])
    assert errors == {0, Z.EMSGSIZE}
    assert len(ran) == len(cases)
    return len(cases)


def test_signature_positions():
    check_a()


def test_stream_start_and_end():
    check_b()


def test_shadows_and_early_stop():
    check_c()


def test_density():
    check_d()


def test_links_and_walk():
    check_e()


@pytest.mark.parametrize("nlists", S.LONG_LISTS)
def test_stream_length(nlists):
    check_f(nlists)


def test_sizes():
    check_g()


@pytest.mark.parametrize("switch,checker", [("SHADOW_RULE", check_c), ("SUFFIX_MIN", check_e),
                                            ("AFTER_ALL_LISTS", check_e)])
def test_a_broken_model_is_caught(monkeypatch, switch, checker):
    """The model without its shadow rule, with a suffix minimum that returns
    "none", or with `after` searched over 64 lists only fails its class."""
    monkeypatch.setattr(M, switch, False)
    with pytest.raises(AssertionError):
        checker()
