"""CPU-side checks of zmqg_subs_update_multi's boundary (no GPU calls): the header
declares the call, zmqg_subs_update and zmqg_subs_result, the structs' sizes and
member offsets in C are the binding's, the constants agree, the built library
exports the call, the Python binding has it, the ABI version is still 5 and
zmqg_forward_subs still has its size."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zmqg_curve.h")
LIB = os.path.join(ROOT, "libzmq_amd", "libzmqg_curve.so")
NAME = "zmqg_subs_update_multi"

FIELDS = ["size", "flags", "n_dst", "cap", "slot_bytes", "cnt", "slot_len", "bytes", "sub_idx", "sub_off", "sub_len",
          "n_streams", "max_frames", "results", "frame_len", "plain_off", "flags_out", "status_out", "plain",
          "stream_dst", "n_clear", "clear_dst", "clear_cnt", "clear_len", "clear_note", "sub_status", "topic_off",
          "topic_len", "note_flags", "note_stream", "results_out"]
STATUS = ["NONE", "ADDED", "DUPLICATE", "REMOVED", "NOT_FOUND", "FULL", "TOO_LONG"]


def _text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_call_and_its_structs():
    text = _text()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert m, "not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["zmqg_ctx *ctx", "const zmqg_subs_update *args", "void *stream"]
    for st in ("zmqg_subs_update", "zmqg_subs_result"):
        assert re.search(r"typedef\s+struct\s+%s\s*\{[^}]*\}\s*%s\s*;" % (st, st), text)
    # the table of replaced reference calls names it, and the forward call's "Not offered" points to it
    raw = open(HEADER).read()
    assert re.search(r"xpub_t::xread_activated / mtrie add, rm / xpipe_terminated.*?%s" % NAME, raw, flags=re.S)
    block = raw[raw.index("/* zmqg_forward_zmtp_sub_multi:"):raw.index("#define ZMQG_SUBS_INVERT")]
    assert NAME in block[block.index("Not offered"):]


def _compiles(src):
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_layout_and_constants_in_c_match_the_binding():
    from libzmq_amd import curve
    py = [(n, getattr(curve.SubsUpdate, n).offset) for n, _ in curve.SubsUpdate._fields_]
    assert [n for n, _ in py] == FIELDS
    # two 4-byte members, then 8-byte members only
    assert [o for _, o in py] == [0, 4] + list(range(8, 8 * (len(FIELDS) - 1), 8))
    assert ctypes.sizeof(curve.SubsUpdate) == 8 * (len(FIELDS) - 1) == 240
    assert ctypes.sizeof(curve.SubsResult) == 32
    assert [n for n, _ in curve.SubsResult._fields_] == ["seen", "changed", "notes", "rejected"]
    src = '#include <stddef.h>\n#include "zmqg_curve.h"\n'
    src += "typedef char total[sizeof(zmqg_subs_update) == %d ? 1 : -1];\n" % ctypes.sizeof(curve.SubsUpdate)
    src += "typedef char res[sizeof(zmqg_subs_result) == 32 ? 1 : -1];\n"
    for n, off in py:
        src += "typedef char off_%s[offsetof(zmqg_subs_update, %s) == %d ? 1 : -1];\n" % (n, n, off)
    for i, n in enumerate(["seen", "changed", "notes", "rejected"]):
        src += "typedef char roff_%s[offsetof(zmqg_subs_result, %s) == %d ? 1 : -1];\n" % (n, n, 8 * i)
    for i, n in enumerate(STATUS):
        assert getattr(curve, "SUB_" + n) == i
        src += "typedef char st_%s[ZMQG_SUB_%s == %d ? 1 : -1];\n" % (n, n, i)
    assert (curve.SUBS_VERBOSE, curve.SUBS_VERBOSER, curve.SUBS_MAX_DST) == (2, 4, 8192)
    src += "typedef char fl[ZMQG_SUBS_VERBOSE == 2 && ZMQG_SUBS_VERBOSER == 4 && ZMQG_SUBS_INVERT == 1 ? 1 : -1];\n"
    src += "typedef char mx[ZMQG_SUBS_MAX_DST == 8192 ? 1 : -1];\n"
    src += "typedef char msg[ZMQG_MSG_SUBSCRIBE == %d && ZMQG_MSG_CANCEL == %d ? 1 : -1];\n" % (curve.SUBSCRIBE,
                                                                                             curve.CANCEL)
    # zmqg_forward_subs is untouched
    src += "typedef char fs[sizeof(zmqg_forward_subs) == 64 ? 1 : -1];\n"
    assert ctypes.sizeof(curve.ForwardSubs) == 64
    _compiles(src + "int main(void){return 0;}\n")


def test_library_exports_the_call():
    assert os.path.exists(LIB), "build first: make -C libzmq_amd/csrc"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    assert NAME in set(l.split()[-1] for l in out.splitlines() if l.strip())


def test_binding_has_the_call_and_reads_a_store():
    import numpy as np
    from libzmq_amd import curve
    for attr in ("subs_update_multi", "subs_store", "subs_store_view", "subs_results"):
        assert callable(getattr(curve.CurveContext, attr))
    assert len(curve._lib.zmqg_subs_update_multi.argtypes) == 3
    # a store of 2 destinations x 2 slots x 8 bytes as numpy arrays: the counts and lengths are clamped
    raw = np.zeros(32, np.uint8)
    raw[0:3], raw[8:10], raw[16:24] = list(b"abc"), list(b"de"), list(b"01234567")
    store = dict(n_dst=2, cap=2, slot_bytes=8, cnt=np.array([2, 9], np.uint32),
                 slot_len=np.array([3, 2, 0xffffffff, 0], np.uint32), bytes=raw,
                 sub_idx=np.array([0, 1, 3], np.uint32), sub_off=np.array([8, 16, 24, 0], np.uint64),
                 sub_len=np.array([2, 8, 0, 0], np.uint32))
    assert curve.CurveContext.subs_store_view(store) == [[b"abc", b"de"], [b"01234567", b""]]
    assert curve.CurveContext.subs_store_view(store, view=True) == [[b"de"], [b"01234567", b""]]


def test_abi_version_unchanged():
    """The call is an addition: the ABI version stays 5."""
    from libzmq_amd import curve
    assert curve._lib.zmqg_abi_version() == 5
    assert re.search(r"#define ZMQG_CURVE_ABI_VERSION 5\b", open(HEADER).read())
