"""Host-side mirror of libzmq's CURVE message codec over the MI355X C ABI.

Python view of include/zmqg_curve.h (libzmq_amd/libzmqg_curve.so).  Two
layers:

* ``CurveContext`` -- the batch API: one call encodes or decodes many frames
  held in device memory (torch tensors on the ctx's device) or host memory.
* ``CurveEncoding`` -- the single-message interface of the reference's
  ``curve_encoding_t`` (src/curve_mechanism_base.hpp:26-59): ``encode(msg)``,
  ``decode(msg) -> (rc, error_event_code)``, ``get_writable_precom_buffer``,
  ``set_peer_nonce``, ``get_and_inc_nonce``, with the reference's return /
  errno / error-event conventions (src/curve_mechanism_base.cpp:80-284).

There is no CPU fallback: if the HIP library is missing, importing this module
raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``.
"""
import ctypes
import errno
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZMQG_CURVE_LIB") or os.path.join(HERE, "libzmqg_curve.so")  # override: experiments

# include/zmq.h:424-437 (= ZMQG_ERR_* of include/zmqg_curve.h)
ERR_UNEXPECTED_COMMAND = 0x10000001
ERR_INVALID_SEQUENCE = 0x10000002
ERR_MALFORMED_UNSPECIFIED = 0x10000011
ERR_MALFORMED_MESSAGE = 0x10000012
ERR_CRYPTOGRAPHIC = 0x11000001
# the handshake's (include/zmq.h:427-431)
ERR_KEY_EXCHANGE = 0x10000003
ERR_MALFORMED_HELLO = 0x10000013
ERR_MALFORMED_INITIATE = 0x10000014
HS_STATE_BYTES, HS_RANDOM_BYTES, HS_WELCOME_BYTES = 128, 96, 168  # ZMQG_HS_*
# the client's (include/zmq.h:433)
ERR_MALFORMED_READY = 0x10000016
HS_HELLO_BYTES, HS_CLIENT_STATE_BYTES = 200, 128
# library codes (zmqg_curve.h): unknown session; frame above the caller's max_len
ERR_SESSION = 0x7A000001
ERR_BOUND = 0x7A000002
ERR_HWM = 0x7A000003
# the largest max_len for which a call skips the large-frame kernels
MAX_LEN_FRAME_KERNEL_DECODE = 4608
MAX_LEN_FRAME_KERNEL_ENCODE = 4565

# src/msg.hpp:55-62
MORE, COMMAND, SUBSCRIBE, CANCEL = 1, 2, 12, 16
CLIENT_PREFIX = b"CurveZMQMESSAGEC"  # src/curve_client.cpp:22-23
SERVER_PREFIX = b"CurveZMQMESSAGES"

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: the MI355X CURVE path has no CPU fallback. "
        "Build it with `make -C libzmq_amd/csrc` (hipcc --offload-arch=gfx950).")

_P = ctypes.c_void_p
_U64 = ctypes.c_uint64
_U32 = ctypes.c_uint32
_lib = ctypes.CDLL(LIB_PATH)
_lib.zmqg_abi_version.restype = ctypes.c_int
_lib.zmqg_ctx_create.argtypes = [ctypes.c_int, _U32, ctypes.POINTER(_P)]
_lib.zmqg_ctx_destroy.argtypes = [_P]
_lib.zmqg_session_set.argtypes = [_P, _U32, _P, _P, _P, ctypes.c_int, _U64]
_lib.zmqg_session_set_batch.argtypes = [_P, _U64, _P, _P, _P, _P, _P, _P, _P]
_lib.zmqg_session_set_batch_ex.argtypes = [_P, _U64, _P, _P, _P, _P, _P, _P, _P, _P]
_lib.zmqg_session_set_peer_nonce.argtypes = [_P, _U32, _U64]
_lib.zmqg_session_get_peer_nonce.argtypes = [_P, _U32, ctypes.POINTER(_U64)]
_lib.zmqg_session_set_nonce.argtypes = [_P, _U32, _U64]
_lib.zmqg_session_get_nonce.argtypes = [_P, _U32, ctypes.POINTER(_U64)]
_lib.zmqg_wire_size.argtypes = [ctypes.c_uint8, ctypes.c_int, _U64]
_lib.zmqg_wire_size.restype = _U64
_lib.zmqg_encode_batch.argtypes = [_P, _U64] + [_P] * 9
_lib.zmqg_decode_batch.argtypes = [_P, _U64] + [_P] * 9
OPT_NONCE_AUTO = 1  # zmqg_batch_opts.flags: encode nonces from the sessions' send counters
OPT_VERIFY_FIRST = 2  # zmqg_batch_opts.flags: decode writes out only after each frame's verdict
OPT_REPLAY_HOST = 4  # zmqg_batch_opts.flags: the caller applied the header / replay rules (verdict_in)
OPT_STREAM_OUT = 8  # zmqg_batch_opts.flags: decode output not cache-resident (whole-segment stores; a hint)


class BatchOpts(ctypes.Structure):  # zmqg_batch_opts
    _fields_ = [("size", _U32), ("flags", _U32), ("max_len", _U64), ("status_out", _P),
                ("session_max_out", _P), ("out_bytes", _U64), ("verdict_in", _P)]


_lib.zmqg_encode_batch_ex.argtypes = [_P, _U64] + [_P] * 8 + [ctypes.POINTER(BatchOpts), _P]
_lib.zmqg_decode_batch_ex.argtypes = [_P, _U64] + [_P] * 8 + [ctypes.POINTER(BatchOpts), _P]
_lib.zmqg_session_max_batch.argtypes = [_P, _U64] + [_P] * 6
_lib.zmqg_encode_host.argtypes = [_P, _U64, _P, _P, _P, _P, _P, _P, _U64, _P, _P, _U64]
_lib.zmqg_decode_host.argtypes = [_P, _U64, _P, _P, _P, _P, _U64, _P, _P, _U64, _P, _P]
_lib.zmqg_encode_msg.argtypes = [_P, _U32, _U64, ctypes.c_uint8, _P, _U32, _P]
_lib.zmqg_decode_msg.argtypes = [_P, _U32, _P, _U32, _P, _P, _P]
class ZmtpResult(ctypes.Structure):  # zmqg_zmtp_result
    _fields_ = [("frames", _U64), ("consumed", _U64), ("out_bytes", _U64), ("error", ctypes.c_int32),
                ("pad", ctypes.c_int32)]


_lib.zmqg_encode_zmtp.argtypes = [_P, _U64] + [_P] * 9
_lib.zmqg_decode_zmtp.argtypes = [_P, _U32, _P, _U64, ctypes.c_int64, _U64] + [_P] * 6 + [ctypes.POINTER(ZmtpResult),
                                                                                       _P]
_lib.zmqg_decode_zmtp_async.argtypes = [_P, _U32, _P, _U64, ctypes.c_int64, _U64] + [_P] * 8
_lib.zmqg_decode_zmtp_multi.argtypes = [_P, _U64] + [_P] * 4 + [ctypes.c_int64, _U64] + [_P] * 8
_lib.zmqg_encode_zmtp_multi.argtypes = [_P, _U64, _P, _U64] + [_P] * 7 + [_U64] + [_P] * 4
ZMTP_MULTI_TILE = 16384  # kZmtpMultiTile: bytes of a stream zmqg_decode_zmtp_multi's kernel holds in LDS at a time
ZMTP_SCAN_TILE = 16384  # kZmtpWgBytes: bytes of a stream one workgroup of zmqg_decode_zmtp's candidate scan lists
REPLAY_TILE_MIN = 256  # replay_tile_frames' first T: the fewest frames of a tile of the tables k_replay_*, k_nonce_*
REPLAY_ROW_BLOCK = 64  # kReplayRB: table rows (tiles) per block of the tables' column passes
REPLAY_MAX_TILES = 4096  # kReplayMaxTiles: above this many tiles the tile doubles
REPLAY_MAX_SESSIONS = 8192  # kReplayMaxSessions: the tables' limit; more sessions take the sort fallback (decode only)
ZSEND_MAX_TILES = 4096  # kZsendMaxTiles: the same bound for zmqg_encode_zmtp_multi's tables (zsend_tile_frames)


class ForwardResult(ctypes.Structure):  # zmqg_forward_result
    _fields_ = [("seq", _U64), ("held_first", _U64), ("forwarded", _U64), ("failed", ctypes.c_int32),
                ("pad", ctypes.c_int32)]


class ForwardZmtp(ctypes.Structure):  # zmqg_forward_zmtp
    _fields_ = [("size", _U32), ("reserved", _U32),
                ("n_streams", _U64), ("stream_sid", _P), ("stream_off", _P), ("stream_len", _P), ("inp", _P),
                ("max_msg_size", ctypes.c_int64), ("max_frames", _U64), ("frame_in_off", _P), ("frame_len", _P),
                ("plain_off", _P), ("plain", _P), ("flags_out", _P), ("status_out", _P), ("results", _P),
                ("carry_idx", _P), ("carry_off", _P), ("carry_len", _P), ("carry_flags", _P),
                ("n_dst", _U64), ("dst_sid", _P), ("route_idx", _P), ("route_dst", _P),
                ("out", _P), ("out_bytes", _U64), ("pair_off", _P), ("pair_status", _P), ("dst_results", _P),
                ("fwd", _P)]


SUBS_INVERT = 1  # ZMQG_SUBS_INVERT


class ForwardSubs(ctypes.Structure):  # zmqg_forward_subs
    _fields_ = [("size", _U32), ("flags", _U32), ("n_subs", _U64), ("sub_idx", _P), ("sub_off", _P),
                ("sub_len", _P), ("sub_bytes", _P), ("sub_bytes_len", _U64), ("match_out", _P)]


# ZMQG_SUB_*: what became of a slot of zmqg_subs_update_multi
SUB_NONE, SUB_ADDED, SUB_DUPLICATE, SUB_REMOVED, SUB_NOT_FOUND, SUB_FULL, SUB_TOO_LONG = range(7)
SUBS_VERBOSE, SUBS_VERBOSER = 2, 4  # ZMQG_SUBS_VERBOSE / _VERBOSER
SUBS_MAX_DST = 8192  # ZMQG_SUBS_MAX_DST
SUBS_NO_NOTE = 0xffffffff  # note_stream of a slot that does not notify


class SubsResult(ctypes.Structure):  # zmqg_subs_result
    _fields_ = [("seen", _U64), ("changed", _U64), ("notes", _U64), ("rejected", _U64)]


class SubsUpdate(ctypes.Structure):  # zmqg_subs_update
    _fields_ = [("size", _U32), ("flags", _U32), ("n_dst", _U64), ("cap", _U64), ("slot_bytes", _U64),
                ("cnt", _P), ("slot_len", _P), ("bytes", _P), ("sub_idx", _P), ("sub_off", _P), ("sub_len", _P),
                ("n_streams", _U64), ("max_frames", _U64), ("results", _P), ("frame_len", _P), ("plain_off", _P),
                ("flags_out", _P), ("status_out", _P), ("plain", _P), ("stream_dst", _P),
                ("n_clear", _U64), ("clear_dst", _P), ("clear_cnt", _P), ("clear_len", _P), ("clear_note", _P),
                ("sub_status", _P), ("topic_off", _P), ("topic_len", _P), ("note_flags", _P), ("note_stream", _P),
                ("results_out", _P)]


_lib.zmqg_subs_update_multi.argtypes = [_P, ctypes.POINTER(SubsUpdate), _P]

ROUTER_PREPEND, ROUTER_ROUTE = 1, 2  # ZMQG_ROUTER_*
ROUTE_NONE, ROUTE_ADDRESS, ROUTE_UNKNOWN, ROUTE_MALFORMED = 0xffffffff, 0xfffffffe, 0xfffffffd, 0xfffffffc  # ZMQG_ROUTE_*


class ForwardRouter(ctypes.Structure):  # zmqg_forward_router
    _fields_ = [("size", _U32), ("flags", _U32), ("src_id_off", _P), ("src_id_len", _P), ("n_ids", _U64),
                ("id_off", _P), ("id_len", _P), ("id_dst", _P), ("id_bytes", _P), ("id_bytes_len", _U64),
                ("dest_out", _P)]


LB_PREPEND = 1  # ZMQG_LB_PREPEND
LB_NO_GROUP, LB_NONE, LB_NO_PEER = 0xffffffff, 0xffffffff, 0xfffffffd  # ZMQG_LB_*


class ForwardLb(ctypes.Structure):  # zmqg_forward_lb
    _fields_ = [("size", _U32), ("flags", _U32), ("src_id_off", _P), ("src_id_len", _P), ("n_groups", _U64),
                ("stream_group", _P), ("grp_idx", _P), ("n_lb", _U64), ("lb_dst", _P), ("lb_cur", _P),
                ("dest_out", _P)]


FRAMING_ZMTP, FRAMING_WS, FRAMING_WS_MASKED = 0, 1, 2  # ZMQG_FRAMING_*
FWD_STATIC, FWD_SUB, FWD_ROUTER, FWD_LB = 0, 1, 2, 3  # ZMQG_FWD_*


class ForwardFraming(ctypes.Structure):  # zmqg_forward_framing
    _fields_ = [("size", _U32), ("reserved", _U32), ("recv", _U32), ("send", _U32), ("mode", _U32),
                ("reserved2", _U32), ("plan", _P), ("ws_results", _P), ("mask", _P)]


CREDIT_UNLIMITED, CREDIT_CONSUME = 0xffffffff, 1  # ZMQG_CREDIT_*


class ForwardCredit(ctypes.Structure):  # zmqg_forward_credit
    _fields_ = [("size", _U32), ("flags", _U32), ("dst_credit", _P), ("dst_taken", _P), ("dst_dropped", _P)]


_lib.zmqg_forward_credit_multi.argtypes = [_P, ctypes.POINTER(ForwardZmtp), ctypes.POINTER(ForwardFraming),
                                           ctypes.POINTER(ForwardCredit), _P]
_lib.zmqg_forward_lb_credit_multi.argtypes = [_P, ctypes.POINTER(ForwardZmtp), ctypes.POINTER(ForwardFraming),
                                              ctypes.POINTER(ForwardCredit), _P]
_lib.zmqg_forward_framed_multi.argtypes = [_P, ctypes.POINTER(ForwardZmtp), ctypes.POINTER(ForwardFraming), _P]
_lib.zmqg_forward_zmtp_lb_multi.argtypes = [_P, ctypes.POINTER(ForwardZmtp), ctypes.POINTER(ForwardLb), _P]
_lib.zmqg_forward_zmtp_multi.argtypes = [_P, ctypes.POINTER(ForwardZmtp), _P]
_lib.zmqg_forward_zmtp_router_multi.argtypes = [_P, ctypes.POINTER(ForwardZmtp), ctypes.POINTER(ForwardRouter), _P]
_lib.zmqg_forward_zmtp_sub_multi.argtypes = [_P, ctypes.POINTER(ForwardZmtp), ctypes.POINTER(ForwardSubs), _P]
_lib.zmqg_decode_ws_multi.argtypes = [_P, _U64] + [_P] * 4 + [ctypes.c_int, ctypes.c_int64, _U64] + [_P] * 8
_lib.zmqg_encode_ws_multi.argtypes = [_P, _U64, _P, _U64] + [_P] * 8 + [_U64] + [_P] * 4
WS_MULTI_TILE = 16384  # kWsTile: the same for zmqg_decode_ws_multi's kernel
_lib.zmqg_scalarmult_batch.argtypes = [_P, _U64] + [_P] * 5
_lib.zmqg_box_beforenm_batch.argtypes = [_P, _U64] + [_P] * 5
_lib.zmqg_box_afternm_batch.argtypes = [_P, _U64] + [_P] * 8
_lib.zmqg_box_open_afternm_batch.argtypes = [_P, _U64] + [_P] * 9
_lib.zmqg_curve_server_hello_batch.argtypes = [_P, _U64] + [_P] * 9
_lib.zmqg_curve_server_initiate_batch.argtypes = [_P, _U64] + [_P] * 12
_lib.zmqg_curve_server_ready_batch.argtypes = [_P, _U64] + [_P] * 8
_lib.zmqg_curve_client_hello_batch.argtypes = [_P, _U64] + [_P] * 7
_lib.zmqg_curve_client_welcome_batch.argtypes = [_P, _U64] + [_P] * 16
_lib.zmqg_curve_client_ready_batch.argtypes = [_P, _U64] + [_P] * 10
_lib.zmqg_z85_encode_batch.argtypes = [_P, _U64] + [_P] * 7
_lib.zmqg_z85_decode_batch.argtypes = [_P, _U64] + [_P] * 7
_lib.zmqg_host_alloc.argtypes = [_P, _U64, ctypes.POINTER(_P)]
_lib.zmqg_host_free.argtypes = [_P, _P]
_lib.zmqg_ctx_stream.argtypes = [_P, ctypes.POINTER(_P)]
_lib.zmqg_fence_record.argtypes = [_P, _P, ctypes.POINTER(_U64)]
_lib.zmqg_fence_query.argtypes = [_P, _U64]
_lib.zmqg_fence_wait.argtypes = [_P, _U64]
_lib.zmqg_ctx_set_profiling.argtypes = [_P, ctypes.c_int]
_lib.zmqg_ctx_get_profile.argtypes = [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_U64)]
_lib.zmqg_last_error.argtypes = [_P]
_lib.zmqg_last_error.restype = ctypes.c_char_p
_lib.zmqg_fence_record_notify.argtypes = [_P, _P, ctypes.c_int, ctypes.POINTER(_U64)]
_lib.zmqg_notify_quiesce.argtypes = [_P]
_lib.zmqg_build_id.restype = ctypes.c_char_p
assert _lib.zmqg_abi_version() == 5


def build_id():
    """(source id, commit) the loaded library was built from (zmqg_build_id)."""
    sid, _, commit = _lib.zmqg_build_id().decode().partition(" ")
    return sid, commit


def lib():
    return _lib


def wire_size(msg_flags, downgrade_sub, payload_len):
    """Encoded frame size (src/curve_mechanism_base.cpp:113-128, 169)."""
    return int(_lib.zmqg_wire_size(msg_flags & 0xFF, int(bool(downgrade_sub)), payload_len))


class ZmqgError(RuntimeError):
    pass


def _ptr(x):
    """Device/host address of a torch tensor or numpy array."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return ctypes.c_void_p(x.ctypes.data)
    return ctypes.c_void_p(x.data_ptr())


def _stream_handle(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    if isinstance(stream, int):
        return ctypes.c_void_p(stream)
    return ctypes.c_void_p(stream.cuda_stream)


class CurveContext:
    """A zmqg_ctx: a session table on one GPU plus batch encode/decode."""

    def __init__(self, device=0, max_sessions=1):
        self._ctx = _P()
        self.device = device
        self.max_sessions = max_sessions
        self.downgrade = [False] * max_sessions
        rc = _lib.zmqg_ctx_create(device, max_sessions, ctypes.byref(self._ctx))
        if rc != 0:
            raise ZmqgError(f"zmqg_ctx_create failed: {rc}")

    def close(self):
        if self._ctx:
            _lib.zmqg_ctx_destroy(self._ctx)
            self._ctx = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise ZmqgError(f"{what} failed: {rc} ({_lib.zmqg_last_error(self._ctx).decode()})")

    def session_set(self, sid, precom, enc_prefix, dec_prefix, downgrade_sub=False, peer_nonce=1):
        precom, enc_prefix, dec_prefix = bytes(precom), bytes(enc_prefix), bytes(dec_prefix)
        if len(precom) != 32 or len(enc_prefix) != 16 or len(dec_prefix) != 16:
            raise ValueError("precom must be 32 bytes and prefixes 16 bytes")
        self.downgrade[sid] = bool(downgrade_sub)
        self._check(_lib.zmqg_session_set(self._ctx, sid, precom, enc_prefix, dec_prefix, int(bool(downgrade_sub)),
                                          peer_nonce), "zmqg_session_set")

    def session_set_batch(self, sid, precom, enc_prefix, dec_prefix, downgrade=None, peer_nonce=None, stream=None,
                          send_nonce=None):
        """zmqg_session_set_batch(_ex): sid / downgrade / peer_nonce /
        send_nonce are host sequences (numpy-convertible), precom a device
        tensor of n x 32 bytes (e.g. box_beforenm_batch's k_out); asynchronous
        on `stream`."""
        sid = np.ascontiguousarray(sid, dtype=np.uint32)
        n = len(sid)
        enc_prefix, dec_prefix = bytes(enc_prefix), bytes(dec_prefix)
        if len(enc_prefix) != 16 or len(dec_prefix) != 16:
            raise ValueError("prefixes must be 16 bytes")
        dg = None if downgrade is None else np.ascontiguousarray(downgrade, dtype=np.uint8)
        pn = None if peer_nonce is None else np.ascontiguousarray(peer_nonce, dtype=np.uint64)
        sn = None if send_nonce is None else np.ascontiguousarray(send_nonce, dtype=np.uint64)
        if (dg is not None and len(dg) != n) or (pn is not None and len(pn) != n) or (sn is not None and len(sn) != n):
            raise ValueError("downgrade / peer_nonce / send_nonce must have one entry per session")
        self._check(_lib.zmqg_session_set_batch_ex(self._ctx, n, sid.ctypes.data, _ptr(precom), enc_prefix,
                                                   dec_prefix, None if dg is None else dg.ctypes.data,
                                                   None if pn is None else pn.ctypes.data,
                                                   None if sn is None else sn.ctypes.data, _stream_handle(stream)),
                    "zmqg_session_set_batch_ex")
        for i, s in enumerate(sid.tolist()):
            self.downgrade[s] = bool(dg[i]) if dg is not None else False

    def set_peer_nonce(self, sid, nonce):
        self._check(_lib.zmqg_session_set_peer_nonce(self._ctx, sid, nonce), "zmqg_session_set_peer_nonce")

    def get_peer_nonce(self, sid):
        v = _U64(0)
        self._check(_lib.zmqg_session_get_peer_nonce(self._ctx, sid, ctypes.byref(v)), "zmqg_session_get_peer_nonce")
        return v.value

    def set_nonce(self, sid, nonce):
        """The session's send counter (_cn_nonce) used by nonce_auto encodes."""
        self._check(_lib.zmqg_session_set_nonce(self._ctx, sid, nonce), "zmqg_session_set_nonce")

    def get_nonce(self, sid):
        v = _U64(0)
        self._check(_lib.zmqg_session_get_nonce(self._ctx, sid, ctypes.byref(v)), "zmqg_session_get_nonce")
        return v.value

    # ---- profiling hooks (HIP events around the body kernels) ----
    # zmqg_curve.h ZMQG_PROF_*: MAIN = the frame kernel (dominant kernel),
    # CALL = the whole batch call, BODY = the chunked body kernel (big frames)
    PROF_ENCODE_MAIN, PROF_DECODE_MAIN, PROF_ENCODE_CALL, PROF_DECODE_CALL = 0, 1, 2, 3
    PROF_ENCODE_BODY, PROF_DECODE_BODY = 4, 5

    def set_profiling(self, enable):
        self._check(_lib.zmqg_ctx_set_profiling(self._ctx, int(bool(enable))), "zmqg_ctx_set_profiling")

    def get_profile(self, kind):
        """(total_ms, launches) for `kind` since the last call; resets."""
        ms = ctypes.c_double(0)
        cnt = _U64(0)
        self._check(_lib.zmqg_ctx_get_profile(self._ctx, kind, ctypes.byref(ms), ctypes.byref(cnt)),
                    "zmqg_ctx_get_profile")
        return ms.value, cnt.value

    # ---- device-resident batches (torch tensors on self.device) ----
    # max_len / status_out / session_max_out: zmqg_batch_opts (the _ex calls)
    # nonce_auto: encode takes nonces from the sessions' send counters (nonce may be None)
    @staticmethod
    def _opts(max_len, status_out, session_max_out, nonce_auto=False, verify_first=False, out_bytes=0,
              verdict_in=None, stream_out=False):
        if (not max_len and status_out is None and session_max_out is None and not nonce_auto and not verify_first
                and verdict_in is None and not stream_out):
            return None
        fl = ((OPT_NONCE_AUTO if nonce_auto else 0) | (OPT_VERIFY_FIRST if verify_first else 0)
              | (OPT_REPLAY_HOST if verdict_in is not None else 0) | (OPT_STREAM_OUT if stream_out else 0))
        o = BatchOpts(ctypes.sizeof(BatchOpts), fl, int(max_len or 0), _ptr(status_out), _ptr(session_max_out),
                      int(out_bytes), _ptr(verdict_in))
        return ctypes.byref(o), o

    def encode_batch(self, sid, nonce, flags, in_off, length, inp, out_off, out, stream=None, max_len=0,
                     status_out=None, nonce_auto=False, stream_out=False):
        """stream_out: ZMQG_OPT_STREAM_OUT, the cache hint for outputs the
        device's caches do not hold."""
        n = int(sid.numel())
        o = self._opts(max_len, status_out, None, nonce_auto, stream_out=stream_out)
        self._check(_lib.zmqg_encode_batch_ex(self._ctx, n, _ptr(sid), _ptr(nonce), _ptr(flags), _ptr(in_off),
                                              _ptr(length), _ptr(inp), _ptr(out_off), _ptr(out),
                                              o[0] if o else None, _stream_handle(stream)), "zmqg_encode_batch")

    def decode_batch(self, sid, in_off, wire_len, inp, out_off, out, flags_out, status_out, stream=None, max_len=0,
                     session_max_out=None, verify_first=False, out_bytes=None, verdict_in=None, stream_out=False):
        """session_max_out: int64 tensor of max_sessions entries (device),
        receives each session's largest header-valid nonce of the batch.
        verify_first: ZMQG_OPT_VERIFY_FIRST (out receives only verified
        payloads and zeros; out's extent is taken from the tensor unless
        out_bytes is given).  verdict_in: int32 tensor (device) of the host's
        header / replay verdicts, ZMQG_OPT_REPLAY_HOST (with verify_first).
        stream_out: ZMQG_OPT_STREAM_OUT, the cache hint for outputs the device's
        caches do not hold."""
        n = int(sid.numel())
        if out_bytes is None:
            out_bytes = out.numel() * out.element_size() if verify_first else 0
        o = self._opts(max_len, None, session_max_out, verify_first=verify_first, out_bytes=out_bytes,
                       verdict_in=verdict_in, stream_out=stream_out)
        self._check(_lib.zmqg_decode_batch_ex(self._ctx, n, _ptr(sid), _ptr(in_off), _ptr(wire_len), _ptr(inp),
                                              _ptr(out_off), _ptr(out), _ptr(flags_out), _ptr(status_out),
                                              o[0] if o else None, _stream_handle(stream)), "zmqg_decode_batch")

    def session_max_batch(self, sid, in_off, wire_len, inp, session_max_out, stream=None):
        """Header pass: session_max_out (int64, max_sessions entries) = each
        session's largest header-valid nonce among the frames (sharded decode)."""
        n = int(sid.numel())
        self._check(_lib.zmqg_session_max_batch(self._ctx, n, _ptr(sid), _ptr(in_off), _ptr(wire_len), _ptr(inp),
                                                _ptr(session_max_out), _stream_handle(stream)),
                    "zmqg_session_max_batch")

    # ---- ZMTP framing on the device (device tensors) ----
    def encode_zmtp(self, sid, nonce, flags, in_off, length, inp, out, frame_off, stream=None):
        """Encode and frame n messages back to back in `out`; frame_off (n + 1
        int64) receives the frame offsets and the total."""
        n = int(sid.numel())
        self._check(_lib.zmqg_encode_zmtp(self._ctx, n, _ptr(sid), _ptr(nonce), _ptr(flags), _ptr(in_off),
                                          _ptr(length), _ptr(inp), _ptr(out), _ptr(frame_off),
                                          _stream_handle(stream)), "zmqg_encode_zmtp")

    def decode_zmtp(self, sid, inp, in_bytes, max_msg_size, max_frames, frame_in_off, frame_len, out_off, out,
                    flags_out, status_out, stream=None):
        """Parse and decode a received stream of one connection; returns
        dict(frames, consumed, out_bytes, error)."""
        r = ZmtpResult()
        self._check(_lib.zmqg_decode_zmtp(self._ctx, sid, _ptr(inp), in_bytes, max_msg_size, max_frames,
                                          _ptr(frame_in_off), _ptr(frame_len), _ptr(out_off), _ptr(out),
                                          _ptr(flags_out), _ptr(status_out), ctypes.byref(r),
                                          _stream_handle(stream)), "zmqg_decode_zmtp")
        return dict(frames=r.frames, consumed=r.consumed, out_bytes=r.out_bytes, error=r.error)

    def decode_zmtp_async(self, sid, inp, in_bytes, max_msg_size, max_frames, frame_in_off, frame_len, out_off, out,
                          flags_out, status_out, result, stream=None):
        """The same without synchronising: `result` is a device int64 tensor of
        4 entries (zmqg_zmtp_result: frames, consumed, out_bytes, error | pad)
        filled when the stream gets there; read it with zmtp_result()."""
        self._check(_lib.zmqg_decode_zmtp_async(self._ctx, sid, _ptr(inp), in_bytes, max_msg_size, max_frames,
                                                _ptr(frame_in_off), _ptr(frame_len), _ptr(out_off), _ptr(out),
                                                _ptr(flags_out), _ptr(status_out), _ptr(result),
                                                _stream_handle(stream)), "zmqg_decode_zmtp_async")

    @staticmethod
    def zmtp_result(result):
        r = result.cpu().numpy().view(np.uint64)
        return dict(frames=int(r[0]), consumed=int(r[1]), out_bytes=int(r[2]),
                    error=int(np.int32(r[3] & np.uint64(0xffffffff))))

    def decode_zmtp_multi(self, stream_sid, stream_off, stream_len, inp, max_msg_size, max_frames, frame_in_off,
                          frame_len, out_off, out, flags_out, status_out, results, stream=None):
        """Parse and decode the receive buffers of many connections in one
        asynchronous call: stream s is inp[stream_off[s] .. +stream_len[s]) on
        session stream_sid[s] (int32 / int64 / int32 tensors of n_streams
        entries).  The per-frame tensors hold n_streams * max_frames entries,
        stream s owning slots [s * max_frames, (s + 1) * max_frames); `results`
        is a device int64 tensor of n_streams x 4 (one zmqg_zmtp_result per
        stream), read with zmtp_results() once the stream is done."""
        n = int(stream_sid.numel())
        self._check(_lib.zmqg_decode_zmtp_multi(self._ctx, n, _ptr(stream_sid), _ptr(stream_off), _ptr(stream_len),
                                                _ptr(inp), max_msg_size, max_frames, _ptr(frame_in_off),
                                                _ptr(frame_len), _ptr(out_off), _ptr(out), _ptr(flags_out),
                                                _ptr(status_out), _ptr(results), _stream_handle(stream)),
                    "zmqg_decode_zmtp_multi")

    @staticmethod
    def zmtp_results(results):
        """decode_zmtp_multi's `results` (synchronised) as a list of dicts, one per stream."""
        r = results.cpu().numpy().view(np.uint64).reshape(-1, 4)
        return [dict(frames=int(x[0]), consumed=int(x[1]), out_bytes=int(x[2]),
                     error=int(np.int32(x[3] & np.uint64(0xffffffff)))) for x in r]

    def encode_zmtp_multi(self, stream_sid, frame_stream, nonce, flags, in_off, length, inp, out, frame_off,
                          status_out, results, stream=None, out_bytes=None):
        """Encode and frame n messages that arrive interleaved over many
        connections, in one asynchronous call: frame i belongs to stream
        frame_stream[i] (int32, n entries), which sends on session
        stream_sid[frame_stream[i]] (int32, n_streams entries); every stream's
        frames land in a contiguous region of `out`, the regions packed in
        stream order.  nonce None: the sessions' device send counters.
        out_bytes: the capacity of `out` (default: the tensor's extent); a
        frame that would end beyond it is not written (ERR_BOUND).  frame_off
        (n + 1 int64) receives the frame offsets and the total, status_out
        (int32, n entries, or None) each frame's status, and `results`, a
        device int64 tensor of n_streams x 4 (one zmqg_zmtp_send_result per
        stream), is read with zmtp_send_results() once the stream is done."""
        n_streams, n = int(stream_sid.numel()), int(frame_stream.numel())
        if out_bytes is None:
            out_bytes = out.numel() * out.element_size()
        self._check(_lib.zmqg_encode_zmtp_multi(self._ctx, n_streams, _ptr(stream_sid), n, _ptr(frame_stream),
                                                _ptr(nonce), _ptr(flags), _ptr(in_off), _ptr(length), _ptr(inp),
                                                _ptr(out), int(out_bytes), _ptr(frame_off), _ptr(status_out),
                                                _ptr(results), _stream_handle(stream)), "zmqg_encode_zmtp_multi")

    @staticmethod
    def zmtp_send_results(results):
        """encode_zmtp_multi's `results` (synchronised) as a list of dicts, one per stream."""
        r = results.cpu().numpy().view(np.uint64).reshape(-1, 4)
        return [dict(frames=int(x[0]), out_off=int(x[1]), out_bytes=int(x[2]),
                     error=int(np.int32(x[3] & np.uint64(0xffffffff)))) for x in r]

    @staticmethod
    def forward_pair_base(route_idx, carry_idx, max_frames):
        """base(s) of forward_zmtp_multi's pairs, n_streams + 1 entries: the
        last one is N, the pair count (pair_off holds N + 1 entries)."""
        r = np.asarray(route_idx, np.int64)
        c = np.zeros_like(r) if carry_idx is None else np.asarray(carry_idx, np.int64)
        return [0] + [int(x) for x in np.cumsum((np.diff(c) + int(max_frames)) * np.diff(r))]

    def forward_zmtp_multi(self, stream_sid, stream_off, stream_len, inp, max_msg_size, max_frames, frame_in_off,
                           frame_len, plain_off, plain, flags_out, status_out, results, dst_sid, route_idx, route_dst,
                           out, pair_off, pair_status, dst_results, fwd, carry_idx=None, carry_off=None,
                           carry_len=None, carry_flags=None, stream=None, out_bytes=None):
        """A broker's round in one asynchronous call (zmqg_forward_zmtp_multi):
        decode_zmtp_multi on the first thirteen arguments (plain_off / plain
        are its out_off / out), then every whole message of source stream s
        re-encoded for each of its destinations route_dst[route_idx[s] ..
        route_idx[s + 1]], destination t sending on session dst_sid[t] (int32
        device tensor) with the device send counters, as encode_zmtp_multi
        over the pairs: pair_off (int64, N + 1), pair_status (int32, N, or
        None) and dst_results (int64, n_dst x 4: zmtp_send_results()) are its
        frame_off / status_out / results, N = forward_pair_base(...)[-1].
        route_idx, route_dst and carry_idx are host sequences, copied before
        the call returns.  carry_idx / carry_off / carry_len / carry_flags:
        the parts held back by earlier calls, per stream (int64 / int32 /
        uint8 device tensors of carry_idx[-1] entries, offsets into plain).
        fwd is a device int64 tensor of n_streams x 4 (one zmqg_forward_result
        per stream), read with forward_results() once the stream is done."""
        a, keep = self._forward_args(stream_sid, stream_off, stream_len, inp, max_msg_size, max_frames, frame_in_off,
                                     frame_len, plain_off, plain, flags_out, status_out, results, dst_sid, route_idx,
                                     route_dst, out, pair_off, pair_status, dst_results, fwd, carry_idx, carry_off,
                                     carry_len, carry_flags, out_bytes)
        self._check(_lib.zmqg_forward_zmtp_multi(self._ctx, ctypes.byref(a), _stream_handle(stream)),
                    "zmqg_forward_zmtp_multi")
        del keep

    @staticmethod
    def _forward_args(stream_sid, stream_off, stream_len, inp, max_msg_size, max_frames, frame_in_off, frame_len,
                      plain_off, plain, flags_out, status_out, results, dst_sid, route_idx, route_dst, out, pair_off,
                      pair_status, dst_results, fwd, carry_idx, carry_off, carry_len, carry_flags, out_bytes):
        """The zmqg_forward_zmtp of a forward call, and the host arrays it points into."""
        n = 0 if stream_sid is None else int(stream_sid.numel())
        ci = None if carry_idx is None else np.ascontiguousarray(carry_idx, dtype=np.uint32)
        if route_idx is None:  # (forward_zmtp_router_multi with ROUTER_ROUTE: no routes are read)
            ri, rd = None, np.zeros(0, np.uint32)
        else:
            ri = np.ascontiguousarray(route_idx, dtype=np.uint32)
            rd = np.ascontiguousarray(route_dst, dtype=np.uint32)
        if (ri is not None and (len(ri) != n + 1 or len(rd) != int(ri[-1]))) or (ci is not None and len(ci) != n + 1):
            raise ValueError("route_idx / carry_idx hold n_streams + 1 entries, route_dst route_idx[-1]")
        if out_bytes is None:
            out_bytes = 0 if out is None else out.numel() * out.element_size()
        a = ForwardZmtp(ctypes.sizeof(ForwardZmtp), 0, n, _ptr(stream_sid), _ptr(stream_off), _ptr(stream_len),
                        _ptr(inp), max_msg_size, max_frames, _ptr(frame_in_off), _ptr(frame_len), _ptr(plain_off),
                        _ptr(plain), _ptr(flags_out), _ptr(status_out), _ptr(results),
                        None if ci is None else ci.ctypes.data, _ptr(carry_off), _ptr(carry_len), _ptr(carry_flags),
                        0 if dst_sid is None else int(dst_sid.numel()), _ptr(dst_sid),
                        None if ri is None else ri.ctypes.data,
                        rd.ctypes.data if len(rd) else None, _ptr(out), int(out_bytes), _ptr(pair_off),
                        _ptr(pair_status), _ptr(dst_results), _ptr(fwd))
        return a, (ri, rd, ci)

    def forward_zmtp_sub_multi(self, stream_sid, stream_off, stream_len, inp, max_msg_size, max_frames, frame_in_off,
                               frame_len, plain_off, plain, flags_out, status_out, results, dst_sid, route_idx,
                               route_dst, out, pair_off, pair_status, dst_results, fwd, sub_idx, sub_off, sub_len,
                               sub_bytes, n_subs=None, sub_bytes_len=None, invert=False, match_out=None,
                               carry_idx=None, carry_off=None, carry_len=None, carry_flags=None, stream=None,
                               out_bytes=None):
        """forward_zmtp_multi for an XPUB side (zmqg_forward_zmtp_sub_multi): a
        forwarded message goes only to the routes whose destination holds a
        subscription that is a prefix of the message's first part.  The table
        is device tensors, CSR by destination (forward_subs_table() builds the
        arrays): sub_idx int32 of n_dst + 1, sub_off int64 and sub_len int32
        of n_subs (default: sub_off's length), sub_bytes uint8 of
        sub_bytes_len (default: its length).  invert: ZMQG_SUBS_INVERT.
        match_out: a device uint8 tensor of N entries, 1 for a live pair, or
        None.  The table is read on the stream and not copied."""
        a, keep = self._forward_args(stream_sid, stream_off, stream_len, inp, max_msg_size, max_frames, frame_in_off,
                                     frame_len, plain_off, plain, flags_out, status_out, results, dst_sid, route_idx,
                                     route_dst, out, pair_off, pair_status, dst_results, fwd, carry_idx, carry_off,
                                     carry_len, carry_flags, out_bytes)
        sb = self._subs_plan(sub_idx, sub_off, sub_len, sub_bytes, n_subs, sub_bytes_len, invert, match_out)
        self._check(_lib.zmqg_forward_zmtp_sub_multi(self._ctx, ctypes.byref(a), ctypes.byref(sb),
                                                     _stream_handle(stream)), "zmqg_forward_zmtp_sub_multi")
        del keep

    @staticmethod
    def _subs_plan(sub_idx=None, sub_off=None, sub_len=None, sub_bytes=None, n_subs=None, sub_bytes_len=None,
                   invert=False, match_out=None):
        """The zmqg_forward_subs of forward_zmtp_sub_multi's table arguments."""
        if n_subs is None:
            n_subs = 0 if sub_off is None else int(sub_off.numel())
        if sub_bytes_len is None:
            sub_bytes_len = 0 if sub_bytes is None else int(sub_bytes.numel())
        return ForwardSubs(ctypes.sizeof(ForwardSubs), SUBS_INVERT if invert else 0, int(n_subs), _ptr(sub_idx),
                           _ptr(sub_off), _ptr(sub_len), _ptr(sub_bytes), int(sub_bytes_len), _ptr(match_out))

    @staticmethod
    def forward_subs_table(prefixes_per_dst):
        """The subscription table of forward_zmtp_sub_multi for a list (by
        destination) of lists of bytes: (sub_idx uint32 of n_dst + 1, sub_off
        uint64, sub_len uint32, sub_bytes uint8) as numpy arrays, the
        prefixes packed back to back in order."""
        flat = [bytes(p) for d in prefixes_per_dst for p in d]
        idx = np.cumsum([0] + [len(d) for d in prefixes_per_dst]).astype(np.uint32)
        lens = np.array([len(p) for p in flat], np.uint32)
        off = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
        return idx, off, lens, np.frombuffer(b"".join(flat), np.uint8).copy()

    @staticmethod
    def subs_store(n_dst, cap, slot_bytes, device=None):
        """An empty subscription store for subs_update_multi and its view, as a
        dict of zeroed device tensors: cnt int32 [n_dst], slot_len int32
        [n_dst * cap], bytes uint8 [n_dst * cap * slot_bytes] (the store);
        sub_idx int32 [n_dst + 1], sub_off int64 and sub_len int32 [n_dst *
        cap] (the view, forward_zmtp_sub_multi's table with sub_bytes =
        bytes); plus n_dst, cap, slot_bytes."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        n = int(n_dst) * int(cap)
        z = lambda count, dt: torch.zeros((max(int(count), 1),), dtype=dt, device=dev)
        return dict(n_dst=int(n_dst), cap=int(cap), slot_bytes=int(slot_bytes), cnt=z(n_dst, torch.int32),
                    slot_len=z(n, torch.int32), bytes=z(n * int(slot_bytes), torch.uint8),
                    sub_idx=z(int(n_dst) + 1, torch.int32), sub_off=z(n, torch.int64), sub_len=z(n, torch.int32))

    @staticmethod
    def subs_store_view(store, view=False):
        """The prefixes a store holds (synchronised), a list of bytes per
        destination, read as the device reads it: counts clamped to cap,
        lengths to slot_bytes.  view=True: the same through the published
        view (sub_idx / sub_off / sub_len over bytes), as the forward call
        reads it."""
        host = lambda x: x if isinstance(x, np.ndarray) else x.cpu().numpy()
        D, cap, sb = store["n_dst"], store["cap"], store["slot_bytes"]
        raw = host(store["bytes"]).tobytes()
        if view:
            idx, off, ln = (host(store[k]).view(t) for k, t in (("sub_idx", np.uint32), ("sub_off", np.uint64),
                                                                ("sub_len", np.uint32)))
            return [[raw[int(off[j]):int(off[j]) + int(ln[j])] for j in range(int(idx[t]), int(idx[t + 1]))]
                    for t in range(D)]
        cnt, sl = host(store["cnt"]).view(np.uint32), host(store["slot_len"]).view(np.uint32)
        return [[raw[(t * cap + i) * sb:(t * cap + i) * sb + min(int(sl[t * cap + i]), sb)]
                 for i in range(min(int(cnt[t]), cap))] for t in range(D)]

    @staticmethod
    def _subs_args(store, stream_dst, max_frames, results, frame_len, plain_off, flags_out, status_out, plain,
                   sub_status, topic_off, topic_len, note_flags, note_stream, results_out, clear_dst, clear_cnt,
                   clear_len, clear_note, flags):
        """The zmqg_subs_update of a subs_update_multi call, and the host arrays it points into."""
        sd = np.ascontiguousarray([] if stream_dst is None else stream_dst, dtype=np.uint32)
        cd = np.ascontiguousarray([] if clear_dst is None else clear_dst, dtype=np.uint32)
        a = SubsUpdate(ctypes.sizeof(SubsUpdate), int(flags), store["n_dst"], store["cap"], store["slot_bytes"],
                       _ptr(store["cnt"]), _ptr(store["slot_len"]), _ptr(store["bytes"]), _ptr(store["sub_idx"]),
                       _ptr(store["sub_off"]), _ptr(store["sub_len"]), len(sd), int(max_frames), _ptr(results),
                       _ptr(frame_len), _ptr(plain_off), _ptr(flags_out), _ptr(status_out), _ptr(plain),
                       sd.ctypes.data if len(sd) else None, len(cd), cd.ctypes.data if len(cd) else None,
                       _ptr(clear_cnt), _ptr(clear_len), _ptr(clear_note), _ptr(sub_status), _ptr(topic_off),
                       _ptr(topic_len), _ptr(note_flags), _ptr(note_stream), _ptr(results_out))
        return a, (sd, cd)

    def subs_update_multi(self, store, stream_dst=None, max_frames=0, results=None, frame_len=None, plain_off=None,
                          flags_out=None, status_out=None, plain=None, sub_status=None, topic_off=None,
                          topic_len=None, note_flags=None, note_stream=None, results_out=None, clear_dst=None,
                          clear_cnt=None, clear_len=None, clear_note=None, flags=0, stream=None):
        """An XPUB's subscription direction in one asynchronous call
        (zmqg_subs_update_multi): the SUBSCRIBE / CANCEL elements that a
        decode_zmtp_multi call queued earlier on the stream has left in
        results / frame_len / plain_off / flags_out / status_out / plain
        (max_frames slots a stream) are applied to `store` (subs_store()),
        stream s editing destination stream_dst[s]; the destinations in
        clear_dst are emptied; the view is republished.  stream_dst and
        clear_dst are host sequences, copied before the call returns.
        Per slot (n_streams * max_frames entries): sub_status int32 (SUB_*),
        topic_off int64, topic_len int32, note_flags uint8 (SUBSCRIBE /
        CANCEL), note_stream int32 (0: notify upstream, else SUBS_NO_NOTE) --
        the last four are encode_zmtp_multi's in_off, length, flags and
        frame_stream with inp = plain and one stream.  results_out: a device
        int64 tensor of n_streams x 4, read with subs_results().  clear_cnt
        int32 [n_clear], clear_len int32 and clear_note uint8 [n_dst * cap].
        flags: SUBS_VERBOSE, SUBS_VERBOSER."""
        a, keep = self._subs_args(store, stream_dst, max_frames, results, frame_len, plain_off, flags_out, status_out,
                                  plain, sub_status, topic_off, topic_len, note_flags, note_stream, results_out,
                                  clear_dst, clear_cnt, clear_len, clear_note, flags)
        self._check(_lib.zmqg_subs_update_multi(self._ctx, ctypes.byref(a), _stream_handle(stream)),
                    "zmqg_subs_update_multi")
        del keep

    @staticmethod
    def subs_results(results_out):
        """subs_update_multi's `results_out` (synchronised) as a list of dicts, one per stream."""
        r = results_out.cpu().numpy().view(np.uint64).reshape(-1, 4)
        return [dict(seen=int(x[0]), changed=int(x[1]), notes=int(x[2]), rejected=int(x[3])) for x in r]

    @staticmethod
    def forward_router_pair_base(flags, route_idx, carry_idx, max_frames):
        """base(s) of forward_zmtp_router_multi's pairs, n_streams + 1 entries,
        the last one N: stream s owns m * (c(s) + max_frames) * d'(s) pairs, m
        = 2 with ROUTER_PREPEND alone (an id slot in front of every element),
        d' = 1 with ROUTER_ROUTE (route_idx is not read then; n_streams is
        taken from carry_idx, or route_idx when carry_idx is None)."""
        route = bool(flags & ROUTER_ROUTE)
        m = 2 if flags & ROUTER_PREPEND and not route else 1
        n = len(carry_idx if carry_idx is not None else route_idx) - 1
        d = np.ones(n, np.int64) if route else np.diff(np.asarray(route_idx, np.int64))
        c = np.zeros(n, np.int64) if carry_idx is None else np.diff(np.asarray(carry_idx, np.int64))
        return [0] + [int(x) for x in np.cumsum(m * (c + int(max_frames)) * d)]

    @staticmethod
    def forward_router_table(ids_with_dst):
        """The id table of forward_zmtp_router_multi for (id bytes,
        destination) pairs: sorted as blob_t orders (bytes compare that way in
        Python), (id_off uint64, id_len uint32, id_dst uint32, id_bytes uint8)
        as numpy arrays, the ids packed back to back in order."""
        rows = sorted((bytes(i), int(d)) for i, d in ids_with_dst)
        lens = np.array([len(i) for i, _ in rows], np.uint32)
        off = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
        return (off, lens, np.array([d for _, d in rows], np.uint32),
                np.frombuffer(b"".join(i for i, _ in rows), np.uint8).copy())

    def forward_zmtp_router_multi(self, stream_sid, stream_off, stream_len, inp, max_msg_size, max_frames,
                                  frame_in_off, frame_len, plain_off, plain, flags_out, status_out, results, dst_sid,
                                  route_idx, route_dst, out, pair_off, pair_status, dst_results, fwd, flags,
                                  src_id_off=None, src_id_len=None, id_off=None, id_len=None, id_dst=None,
                                  id_bytes=None, n_ids=None, id_bytes_len=None, dest_out=None, carry_idx=None,
                                  carry_off=None, carry_len=None, carry_flags=None, stream=None, out_bytes=None):
        """forward_zmtp_multi for a proxy with a ROUTER side
        (zmqg_forward_zmtp_router_multi).  flags: ROUTER_PREPEND (every
        message gets its source's routing id in front: src_id_off int64 and
        src_id_len int32 device tensors of n_streams, offsets into plain),
        ROUTER_ROUTE (the first part of every message is an address, looked up
        in the id table and consumed: id_off int64, id_len int32, id_dst int32
        of n_ids (default: id_off's length), id_bytes uint8 of id_bytes_len
        (default: its length), device tensors that forward_router_table()
        builds; route_idx / route_dst may be None), both, or 0 (the parent
        call).  dest_out: a device int32 tensor of N entries
        (forward_router_pair_base(...)[-1]) that receives each pair's
        destination or ROUTE_NONE / _ADDRESS / _UNKNOWN / _MALFORMED, or None.
        The table is read on the stream and not copied."""
        a, keep = self._forward_args(stream_sid, stream_off, stream_len, inp, max_msg_size, max_frames, frame_in_off,
                                     frame_len, plain_off, plain, flags_out, status_out, results, dst_sid, route_idx,
                                     route_dst, out, pair_off, pair_status, dst_results, fwd, carry_idx, carry_off,
                                     carry_len, carry_flags, out_bytes)
        rt = self._router_plan(flags, src_id_off, src_id_len, id_off, id_len, id_dst, id_bytes, n_ids, id_bytes_len,
                               dest_out)
        self._check(_lib.zmqg_forward_zmtp_router_multi(self._ctx, ctypes.byref(a), ctypes.byref(rt),
                                                        _stream_handle(stream)), "zmqg_forward_zmtp_router_multi")
        del keep

    @staticmethod
    def _router_plan(flags, src_id_off=None, src_id_len=None, id_off=None, id_len=None, id_dst=None, id_bytes=None,
                     n_ids=None, id_bytes_len=None, dest_out=None):
        """The zmqg_forward_router of forward_zmtp_router_multi's arguments."""
        if n_ids is None:
            n_ids = 0 if id_off is None else int(id_off.numel())
        if id_bytes_len is None:
            id_bytes_len = 0 if id_bytes is None else int(id_bytes.numel())
        return ForwardRouter(ctypes.sizeof(ForwardRouter), int(flags), _ptr(src_id_off), _ptr(src_id_len), int(n_ids),
                             _ptr(id_off), _ptr(id_len), _ptr(id_dst), _ptr(id_bytes), int(id_bytes_len),
                             _ptr(dest_out))

    @staticmethod
    def forward_lb_pair_base(flags, carry_idx, max_frames, n_streams):
        """base(s) of forward_zmtp_lb_multi's pairs, n_streams + 1 entries, the
        last one N: stream s owns m * (c(s) + max_frames) pairs, m = 2 with
        LB_PREPEND (an id slot in front of every element), else 1."""
        m = 2 if flags & LB_PREPEND else 1
        n = int(n_streams)
        c = np.zeros(n, np.int64) if carry_idx is None else np.diff(np.asarray(carry_idx, np.int64))
        return [0] + [int(x) for x in np.cumsum(m * (c + int(max_frames)))]

    def forward_zmtp_lb_multi(self, stream_sid, stream_off, stream_len, inp, max_msg_size, max_frames, frame_in_off,
                              frame_len, plain_off, plain, flags_out, status_out, results, dst_sid, out, pair_off,
                              pair_status, dst_results, fwd, flags, stream_group, grp_idx, lb_dst, lb_cur,
                              n_groups=None, n_lb=None, src_id_off=None, src_id_len=None, dest_out=None,
                              carry_idx=None, carry_off=None, carry_len=None, carry_flags=None, stream=None,
                              out_bytes=None):
        """forward_zmtp_multi for a proxy whose send side is a DEALER or a PUSH
        socket (zmqg_forward_zmtp_lb_multi): every whole message goes to the
        next active destination of its stream's group in turn, as lb_t does.
        There are no routes.  stream_group: a host sequence of n_streams group
        indices or LB_NO_GROUP, copied before the call returns.  grp_idx (int32,
        n_groups + 1), lb_dst (int32, n_lb) and lb_cur (int32, n_groups) are
        device tensors that live across calls: group g's active destinations
        are lb_dst[grp_idx[g] .. grp_idx[g + 1]), lb_cur[g] its cursor, read
        and written by the call (n_groups defaults to lb_cur's length, n_lb to
        lb_dst's).  flags: 0 or LB_PREPEND (every message gets its source's
        routing id in front: src_id_off int64 and src_id_len int32 device
        tensors of n_streams, offsets into plain).  dest_out: a device int32
        tensor of N entries (forward_lb_pair_base(...)[-1]) that receives each
        pair's destination, LB_NO_PEER or LB_NONE, or None."""
        a, keep = self._forward_args(stream_sid, stream_off, stream_len, inp, max_msg_size, max_frames, frame_in_off,
                                     frame_len, plain_off, plain, flags_out, status_out, results, dst_sid, None,
                                     None, out, pair_off, pair_status, dst_results, fwd, carry_idx, carry_off,
                                     carry_len, carry_flags, out_bytes)
        lb, sg = self._lb_plan(int(a.n_streams), flags, stream_group, grp_idx, lb_dst, lb_cur, n_groups, n_lb,
                               src_id_off, src_id_len, dest_out)
        self._check(_lib.zmqg_forward_zmtp_lb_multi(self._ctx, ctypes.byref(a), ctypes.byref(lb),
                                                    _stream_handle(stream)), "zmqg_forward_zmtp_lb_multi")
        del keep, sg

    @staticmethod
    def _lb_plan(n_streams, flags, stream_group=None, grp_idx=None, lb_dst=None, lb_cur=None, n_groups=None,
                 n_lb=None, src_id_off=None, src_id_len=None, dest_out=None):
        """The zmqg_forward_lb of forward_zmtp_lb_multi's arguments, and the host array it points into."""
        sg = None if stream_group is None else np.ascontiguousarray(stream_group, dtype=np.uint32)
        if sg is not None and len(sg) != n_streams:
            raise ValueError("stream_group holds n_streams entries")
        if n_groups is None:
            n_groups = 0 if lb_cur is None else int(lb_cur.numel())
        if n_lb is None:
            n_lb = 0 if lb_dst is None else int(lb_dst.numel())
        lb = ForwardLb(ctypes.sizeof(ForwardLb), int(flags), _ptr(src_id_off), _ptr(src_id_len), int(n_groups),
                       sg.ctypes.data if sg is not None and len(sg) else None, _ptr(grp_idx), int(n_lb),
                       _ptr(lb_dst), _ptr(lb_cur), _ptr(dest_out))
        return lb, sg

    def forward_framed_multi(self, recv, send, mode, stream_sid, stream_off, stream_len, inp, max_msg_size, max_frames,
                             frame_in_off, frame_len, plain_off, plain, flags_out, status_out, results, dst_sid,
                             route_idx, route_dst, out, pair_off, pair_status, dst_results, fwd, ws_results=None,
                             mask=None, carry_idx=None, carry_off=None, carry_len=None, carry_flags=None, stream=None,
                             out_bytes=None, **plan):
        """A forward call with a framing chosen per side
        (zmqg_forward_framed_multi).  recv / send: FRAMING_ZMTP, FRAMING_WS
        (unmasked) or FRAMING_WS_MASKED, the framing of the receive buffers
        and of the send runs.  mode: FWD_STATIC (forward_zmtp_multi's rule),
        FWD_SUB, FWD_ROUTER or FWD_LB, with that call's own table arguments as
        keywords (sub_idx ..., flags / id_off ..., flags / stream_group ...;
        FWD_LB reads no routes: route_idx and route_dst may be None).  With a
        WebSocket receive side the per-stream results go to ws_results, a
        device int64 tensor of n_streams x 6 read with ws_results(), and
        `results` may be None.  With FRAMING_WS_MASKED on the send side, mask
        is an int32 device tensor of N entries, pair p's 32-bit key value (N
        from the mode's *_pair_base).  Everything else is the mode's call."""
        a, fr, keep = self._framed_args(recv, send, mode, stream_sid, stream_off, stream_len, inp, max_msg_size,
                                        max_frames, frame_in_off, frame_len, plain_off, plain, flags_out, status_out,
                                        results, dst_sid, route_idx, route_dst, out, pair_off, pair_status,
                                        dst_results, fwd, ws_results, mask, carry_idx, carry_off, carry_len,
                                        carry_flags, out_bytes, plan)
        self._check(_lib.zmqg_forward_framed_multi(self._ctx, ctypes.byref(a), ctypes.byref(fr),
                                                   _stream_handle(stream)), "zmqg_forward_framed_multi")
        del keep

    def _framed_args(self, recv, send, mode, stream_sid, stream_off, stream_len, inp, max_msg_size, max_frames,
                     frame_in_off, frame_len, plain_off, plain, flags_out, status_out, results, dst_sid, route_idx,
                     route_dst, out, pair_off, pair_status, dst_results, fwd, ws_results, mask, carry_idx, carry_off,
                     carry_len, carry_flags, out_bytes, plan):
        """The zmqg_forward_zmtp and zmqg_forward_framing of a framed call, and what they point into."""
        a, keep = self._forward_args(stream_sid, stream_off, stream_len, inp, max_msg_size, max_frames, frame_in_off,
                                     frame_len, plain_off, plain, flags_out, status_out, results, dst_sid, route_idx,
                                     route_dst, out, pair_off, pair_status, dst_results, fwd, carry_idx, carry_off,
                                     carry_len, carry_flags, out_bytes)
        if mode == FWD_STATIC:
            if plan:
                raise ValueError("FWD_STATIC takes no table arguments")
            p = None
        elif mode == FWD_SUB:
            p = self._subs_plan(**plan)
        elif mode == FWD_ROUTER:
            p = self._router_plan(**plan)
        elif mode == FWD_LB:
            p, sg = self._lb_plan(int(a.n_streams), **plan)
            keep += (sg,)
        else:
            raise ValueError("mode is one of FWD_STATIC, FWD_SUB, FWD_ROUTER, FWD_LB")
        fr = ForwardFraming(ctypes.sizeof(ForwardFraming), 0, int(recv), int(send), int(mode), 0,
                            None if p is None else ctypes.addressof(p), _ptr(ws_results), _ptr(mask))
        return a, fr, keep + (p,)

    def forward_credit_multi(self, recv, send, mode, dst_credit, dst_taken, dst_dropped, stream_sid, stream_off,
                             stream_len, inp, max_msg_size, max_frames, frame_in_off, frame_len, plain_off, plain,
                             flags_out, status_out, results, dst_sid, route_idx, route_dst, out, pair_off, pair_status,
                             dst_results, fwd, consume=False, ws_results=None, mask=None, carry_idx=None,
                             carry_off=None, carry_len=None, carry_flags=None, stream=None, out_bytes=None, **plan):
        """forward_framed_multi with a high-water mark per destination
        (zmqg_forward_credit_multi): destination t takes at most dst_credit[t]
        more whole messages in this call (CREDIT_UNLIMITED: all), in pair
        order; the pairs of a refused message are not sent and report ERR_HWM
        in pair_status, for that destination alone.  dst_credit, dst_taken and
        dst_dropped are int32 device tensors of n_dst entries; taken / dropped
        receive the admitted / refused messages per destination, and with
        consume=True dst_credit is left holding what remains.  dst_credit
        lives on the device across calls; the host adds to it on the stream
        when a peer has read.  mode: FWD_STATIC, FWD_SUB or FWD_ROUTER.
        Everything else is forward_framed_multi's."""
        a, fr, keep = self._framed_args(recv, send, mode, stream_sid, stream_off, stream_len, inp, max_msg_size,
                                        max_frames, frame_in_off, frame_len, plain_off, plain, flags_out, status_out,
                                        results, dst_sid, route_idx, route_dst, out, pair_off, pair_status,
                                        dst_results, fwd, ws_results, mask, carry_idx, carry_off, carry_len,
                                        carry_flags, out_bytes, plan)
        cr = ForwardCredit(ctypes.sizeof(ForwardCredit), CREDIT_CONSUME if consume else 0, _ptr(dst_credit),
                           _ptr(dst_taken), _ptr(dst_dropped))
        self._check(_lib.zmqg_forward_credit_multi(self._ctx, ctypes.byref(a), ctypes.byref(fr), ctypes.byref(cr),
                                                   _stream_handle(stream)), "zmqg_forward_credit_multi")
        del keep

    def forward_lb_credit_multi(self, recv, send, dst_credit, dst_taken, dst_dropped, stream_sid, stream_off,
                                stream_len, inp, max_msg_size, max_frames, frame_in_off, frame_len, plain_off, plain,
                                flags_out, status_out, results, dst_sid, out, pair_off, pair_status, dst_results, fwd,
                                consume=False, ws_results=None, mask=None, carry_idx=None, carry_off=None,
                                carry_len=None, carry_flags=None, stream=None, out_bytes=None, **plan):
        """forward_framed_multi with FWD_LB under a high-water mark per
        destination (zmqg_forward_lb_credit_multi): a destination whose
        credit has run out is taken out of its group's ring for the rest of the
        call and the message goes to the next one, as lb_t does for a full
        pipe; a message that finds the whole ring full is not sent, reports
        ERR_HWM in pair_status and LB_NO_PEER in dest_out, and stays whole in
        `plain` for a later call's carry.  dst_credit, dst_taken and
        dst_dropped are forward_credit_multi's; the table arguments (flags,
        stream_group, grp_idx, lb_dst, lb_cur, ...) are forward_zmtp_lb_multi's
        as keywords.  lb_cur[g] is left at the original ring position the
        cursor points at."""
        a, fr, keep = self._framed_args(recv, send, FWD_LB, stream_sid, stream_off, stream_len, inp, max_msg_size,
                                        max_frames, frame_in_off, frame_len, plain_off, plain, flags_out, status_out,
                                        results, dst_sid, None, None, out, pair_off, pair_status, dst_results, fwd,
                                        ws_results, mask, carry_idx, carry_off, carry_len, carry_flags, out_bytes, plan)
        cr = ForwardCredit(ctypes.sizeof(ForwardCredit), CREDIT_CONSUME if consume else 0, _ptr(dst_credit),
                           _ptr(dst_taken), _ptr(dst_dropped))
        self._check(_lib.zmqg_forward_lb_credit_multi(self._ctx, ctypes.byref(a), ctypes.byref(fr), ctypes.byref(cr),
                                                      _stream_handle(stream)), "zmqg_forward_lb_credit_multi")
        del keep

    @staticmethod
    def forward_results(fwd):
        """forward_zmtp_multi's `fwd` (synchronised) as a list of dicts, one per source stream."""
        r = fwd.cpu().numpy().view(np.uint64).reshape(-1, 4)
        return [dict(seq=int(x[0]), held_first=int(x[1]), forwarded=int(x[2]),
                     failed=int(np.int32(x[3] & np.uint64(0xffffffff)))) for x in r]

    def decode_ws_multi(self, stream_sid, stream_off, stream_len, inp, must_mask, max_msg_size, max_frames,
                        frame_in_off, frame_len, out_off, out, flags_out, status_out, results, stream=None):
        """decode_zmtp_multi for WebSocket framing (ws_decoder_t): the
        arguments are the same, plus must_mask (True on a server's receive
        side: every frame carries a masking key, and its body is unmasked --
        in place when out is inp -- before it is decoded).  `results` is a
        device int64 tensor of n_streams x 6 (one zmqg_ws_result per stream),
        read with ws_results() once the stream is done."""
        n = int(stream_sid.numel())
        self._check(_lib.zmqg_decode_ws_multi(self._ctx, n, _ptr(stream_sid), _ptr(stream_off), _ptr(stream_len),
                                              _ptr(inp), int(bool(must_mask)), max_msg_size, max_frames,
                                              _ptr(frame_in_off), _ptr(frame_len), _ptr(out_off), _ptr(out),
                                              _ptr(flags_out), _ptr(status_out), _ptr(results),
                                              _stream_handle(stream)), "zmqg_decode_ws_multi")

    @staticmethod
    def ws_results(results):
        """decode_ws_multi's `results` (synchronised) as a list of dicts, one per stream."""
        r = results.cpu().numpy().view(np.uint64).reshape(-1, 6)
        return [dict(frames=int(x[0]), consumed=int(x[1]), out_bytes=int(x[2]),
                     error=int(np.int32(x[3] & np.uint64(0xffffffff))), ctl_opcode=int(np.int32(x[3] >> np.uint64(32))),
                     ctl_off=int(x[4]), ctl_len=int(x[5])) for x in r]

    def encode_ws_multi(self, stream_sid, frame_stream, nonce, flags, in_off, length, inp, mask, out, frame_off,
                        status_out, results, stream=None, out_bytes=None):
        """encode_zmtp_multi with WebSocket framing (ws_encoder_t's binary
        frame around each MESSAGE command).  mask None: unmasked frames, a
        server's send side; else an int32 tensor of n entries, the 32-bit
        value whose big-endian bytes are frame i's masking key (what the
        reference takes from generate_random).  `results` is read with
        zmtp_send_results()."""
        n_streams, n = int(stream_sid.numel()), int(frame_stream.numel())
        if out_bytes is None:
            out_bytes = out.numel() * out.element_size()
        self._check(_lib.zmqg_encode_ws_multi(self._ctx, n_streams, _ptr(stream_sid), n, _ptr(frame_stream),
                                              _ptr(nonce), _ptr(flags), _ptr(in_off), _ptr(length), _ptr(inp),
                                              _ptr(mask), _ptr(out), int(out_bytes), _ptr(frame_off),
                                              _ptr(status_out), _ptr(results), _stream_handle(stream)),
                    "zmqg_encode_ws_multi")

    # ---- handshake key derivation (device tensors of n x 32 bytes) ----
    def scalarmult_batch(self, scalar, point, out, status_out, stream=None):
        """crypto_scalarmult_curve25519 per item; point None = the base point."""
        n = int(status_out.numel())
        self._check(_lib.zmqg_scalarmult_batch(self._ctx, n, _ptr(scalar), _ptr(point), _ptr(out), _ptr(status_out),
                                               _stream_handle(stream)), "zmqg_scalarmult_batch")

    def box_beforenm_batch(self, pk, sk, k_out, status_out, stream=None):
        """crypto_box_beforenm(k, pk, sk) per item."""
        n = int(status_out.numel())
        self._check(_lib.zmqg_box_beforenm_batch(self._ctx, n, _ptr(pk), _ptr(sk), _ptr(k_out), _ptr(status_out),
                                                 _stream_handle(stream)), "zmqg_box_beforenm_batch")

    # ---- handshake boxes: crypto_box_easy_afternm / _open_ per item ----
    def box_afternm_batch(self, key, nonce, in_off, length, inp, out_off, out, stream=None):
        """Seal: out[out_off[i]] = tag || ciphertext of in[in_off[i] .. +length[i]]
        under key[i] (32 B) and nonce[i] (24 B)."""
        n = int(in_off.numel())
        self._check(_lib.zmqg_box_afternm_batch(self._ctx, n, _ptr(key), _ptr(nonce), _ptr(in_off), _ptr(length),
                                                _ptr(inp), _ptr(out_off), _ptr(out), _stream_handle(stream)),
                    "zmqg_box_afternm_batch")

    def box_open_afternm_batch(self, key, nonce, in_off, length, inp, out_off, out, status_out, stream=None):
        """Open: length[i] = 16 + plaintext bytes; status 0 or -1."""
        n = int(in_off.numel())
        self._check(_lib.zmqg_box_open_afternm_batch(self._ctx, n, _ptr(key), _ptr(nonce), _ptr(in_off),
                                                     _ptr(length), _ptr(inp), _ptr(out_off), _ptr(out),
                                                     _ptr(status_out), _stream_handle(stream)),
                    "zmqg_box_open_afternm_batch")

    # ---- the server's handshake steps (curve_server_t), device tensors ----
    def server_hello_batch(self, server_sk, cmd_off, cmd_len, cmd, random, state, welcome_out, status_out,
                           stream=None):
        """process_hello + produce_welcome per item: HELLO command i is
        cmd[cmd_off[i] .. +cmd_len[i]); server_sk the 32-byte long-term secret
        (device), random n x 96 bytes (s' | cookie key | cookie nonce | WELCOME
        nonce).  Fills status_out (0 or ERR_*), welcome_out (n x 168) and state
        (n x 128: C' | s' | cookie key | precom)."""
        n = int(status_out.numel())
        self._check(_lib.zmqg_curve_server_hello_batch(self._ctx, n, _ptr(server_sk), _ptr(cmd_off), _ptr(cmd_len),
                                                       _ptr(cmd), _ptr(random), _ptr(state), _ptr(welcome_out),
                                                       _ptr(status_out), _stream_handle(stream)),
                    "zmqg_curve_server_hello_batch")

    def server_initiate_batch(self, state, cmd_off, cmd_len, cmd, client_key_out, precom_out, peer_nonce_out,
                              meta_off, meta_out, meta_len_out, status_out, stream=None):
        """process_initiate up to the ZAP decision per item: `state` as
        server_hello_batch wrote it.  Fills status_out, client_key_out and
        precom_out (n x 32), peer_nonce_out (int64, n), meta_len_out (int32, n)
        and each accepted item's metadata at meta_out[meta_off[i] ..]."""
        n = int(status_out.numel())
        self._check(_lib.zmqg_curve_server_initiate_batch(self._ctx, n, _ptr(state), _ptr(cmd_off), _ptr(cmd_len),
                                                          _ptr(cmd), _ptr(client_key_out), _ptr(precom_out),
                                                          _ptr(peer_nonce_out), _ptr(meta_off), _ptr(meta_out),
                                                          _ptr(meta_len_out), _ptr(status_out),
                                                          _stream_handle(stream)),
                    "zmqg_curve_server_initiate_batch")

    def server_ready_batch(self, precom, nonce, meta_off, meta_len, meta, out_off, out, stream=None):
        """produce_ready per item: 30 + meta_len[i] bytes at out[out_off[i]],
        "\\x05READY" || BE64(nonce[i]) || box of the metadata under precom[i]."""
        n = int(nonce.numel())
        self._check(_lib.zmqg_curve_server_ready_batch(self._ctx, n, _ptr(precom), _ptr(nonce), _ptr(meta_off),
                                                       _ptr(meta_len), _ptr(meta), _ptr(out_off), _ptr(out),
                                                       _stream_handle(stream)), "zmqg_curve_server_ready_batch")

    # ---- the client's handshake steps (curve_client_t), device tensors ----
    def client_hello_batch(self, server_pk, cn_secret, nonce, state, hello_out, status_out, stream=None):
        """crypto_box_keypair + produce_hello per item: server_pk and cn_secret
        n x 32 bytes (S and the random bytes of c'), nonce int64 n.  Fills
        status_out (0 or ERR_CRYPTOGRAPHIC), hello_out (n x 200) and state
        (n x 128: C' | c' | k1 | S)."""
        n = int(status_out.numel())
        self._check(_lib.zmqg_curve_client_hello_batch(self._ctx, n, _ptr(server_pk), _ptr(cn_secret), _ptr(nonce),
                                                       _ptr(state), _ptr(hello_out), _ptr(status_out),
                                                       _stream_handle(stream)), "zmqg_curve_client_hello_batch")

    def client_welcome_batch(self, state, client_pk, client_sk, cmd_off, cmd_len, cmd, vouch_nonce, nonce, meta_off,
                             meta_len, meta, out_off, out, precom_out, status_out, stream=None):
        """process_welcome + produce_initiate per item: `state` as
        client_hello_batch wrote it, WELCOME command i is cmd[cmd_off[i] ..
        +cmd_len[i]), client_pk / client_sk n x 32, vouch_nonce n x 16, nonce
        int64 n, the metadata meta[meta_off[i] .. +meta_len[i]).  Fills
        status_out, precom_out (n x 32) and each accepted item's INITIATE
        (257 + meta_len[i] bytes) at out[out_off[i] ..]."""
        n = int(status_out.numel())
        self._check(_lib.zmqg_curve_client_welcome_batch(self._ctx, n, _ptr(state), _ptr(client_pk), _ptr(client_sk),
                                                         _ptr(cmd_off), _ptr(cmd_len), _ptr(cmd), _ptr(vouch_nonce),
                                                         _ptr(nonce), _ptr(meta_off), _ptr(meta_len), _ptr(meta),
                                                         _ptr(out_off), _ptr(out), _ptr(precom_out),
                                                         _ptr(status_out), _stream_handle(stream)),
                    "zmqg_curve_client_welcome_batch")

    def client_ready_batch(self, precom, cmd_off, cmd_len, cmd, peer_nonce_out, meta_off, meta_out, meta_len_out,
                           status_out, stream=None):
        """process_ready up to parse_metadata per item: READY command i is
        cmd[cmd_off[i] .. +cmd_len[i]), precom n x 32.  Fills status_out,
        peer_nonce_out (int64, n), meta_len_out (int32, n) and each accepted
        item's metadata at meta_out[meta_off[i] ..]."""
        n = int(status_out.numel())
        self._check(_lib.zmqg_curve_client_ready_batch(self._ctx, n, _ptr(precom), _ptr(cmd_off), _ptr(cmd_len),
                                                       _ptr(cmd), _ptr(peer_nonce_out), _ptr(meta_off),
                                                       _ptr(meta_out), _ptr(meta_len_out), _ptr(status_out),
                                                       _stream_handle(stream)), "zmqg_curve_client_ready_batch")

    # ---- batched Z85 (zmq_z85_encode / zmq_z85_decode), device tensors ----
    def z85_encode_batch(self, in_off, length, inp, out_off, out, status_out, stream=None):
        n = int(in_off.numel())
        self._check(_lib.zmqg_z85_encode_batch(self._ctx, n, _ptr(in_off), _ptr(length), _ptr(inp), _ptr(out_off),
                                               _ptr(out), _ptr(status_out), _stream_handle(stream)),
                    "zmqg_z85_encode_batch")

    def z85_decode_batch(self, in_off, length, inp, out_off, out, status_out, stream=None):
        n = int(in_off.numel())
        self._check(_lib.zmqg_z85_decode_batch(self._ctx, n, _ptr(in_off), _ptr(length), _ptr(inp), _ptr(out_off),
                                               _ptr(out), _ptr(status_out), _stream_handle(stream)),
                    "zmqg_z85_decode_batch")

    # ---- host-memory batches (numpy), staged through pinned buffers ----
    def encode_host(self, sid, nonce, flags, in_off, length, inp, out_off, out_size):
        sid = np.ascontiguousarray(sid, np.uint32)
        nonce = np.ascontiguousarray(nonce, np.uint64)
        flags = np.ascontiguousarray(flags, np.uint8)
        in_off = np.ascontiguousarray(in_off, np.uint64)
        length = np.ascontiguousarray(length, np.uint32)
        inp = np.ascontiguousarray(inp, np.uint8)
        out_off = np.ascontiguousarray(out_off, np.uint64)
        out = np.zeros(max(out_size, 1), np.uint8)
        self._check(_lib.zmqg_encode_host(self._ctx, len(sid), _ptr(sid), _ptr(nonce), _ptr(flags), _ptr(in_off),
                                          _ptr(length), _ptr(inp), inp.nbytes, _ptr(out_off), _ptr(out), out.nbytes),
                    "zmqg_encode_host")
        return out[:out_size]

    def decode_host(self, sid, in_off, wire_len, inp, out_off, out_size):
        sid = np.ascontiguousarray(sid, np.uint32)
        in_off = np.ascontiguousarray(in_off, np.uint64)
        wire_len = np.ascontiguousarray(wire_len, np.uint32)
        inp = np.ascontiguousarray(inp, np.uint8)
        out_off = np.ascontiguousarray(out_off, np.uint64)
        n = len(sid)
        out = np.zeros(max(out_size, 1), np.uint8)
        fl = np.zeros(max(n, 1), np.uint8)
        st = np.zeros(max(n, 1), np.int32)
        self._check(_lib.zmqg_decode_host(self._ctx, n, _ptr(sid), _ptr(in_off), _ptr(wire_len), _ptr(inp),
                                          inp.nbytes, _ptr(out_off), _ptr(out), out.nbytes, _ptr(fl), _ptr(st)),
                    "zmqg_decode_host")
        return out[:out_size], fl[:n], st[:n]


    # ---- one message, host bytes (zmqg_encode_msg / zmqg_decode_msg) ----
    def encode_msg(self, sid, nonce, flags, payload):
        """The MESSAGE command for one message (bytes) on session sid."""
        p = np.frombuffer(bytes(payload), np.uint8)
        out = np.zeros(wire_size(flags, 1 if self.downgrade[sid] else 0, len(p)), np.uint8)
        self._check(_lib.zmqg_encode_msg(self._ctx, sid, nonce, flags, _ptr(p) if len(p) else None, len(p),
                                         _ptr(out)), "zmqg_encode_msg")
        return out.tobytes()

    def decode_msg(self, sid, wire):
        """(payload bytes or None, flags, status) of one received frame."""
        w = np.frombuffer(bytes(wire), np.uint8)
        out = np.zeros(max(len(w) - 33, 1), np.uint8)
        fl = np.zeros(1, np.uint8)
        st = np.zeros(1, np.int32)
        self._check(_lib.zmqg_decode_msg(self._ctx, sid, _ptr(w) if len(w) else None, len(w), _ptr(out), _ptr(fl),
                                         _ptr(st)), "zmqg_decode_msg")
        if st[0] != 0:
            return None, 0, int(st[0])
        return out[:len(w) - 33].tobytes(), int(fl[0]), 0


class Msg:
    """Minimal stand-in for zmq::msg_t on this path: bytes + flags byte
    (src/msg.hpp:55-62).  ``set_flags`` ORs, as msg_t::set_flags does."""

    def __init__(self, data=b"", flags=0):
        self.data = bytes(data)
        self.flags = flags

    def size(self):
        return len(self.data)

    def set_flags(self, f):
        self.flags |= f


class CurveEncoding:
    """curve_encoding_t (src/curve_mechanism_base.hpp:26-59) backed by the GPU.

    Each instance owns one session of a shared CurveContext (or its own)."""

    def __init__(self, encode_nonce_prefix, decode_nonce_prefix, downgrade_sub, ctx=None, sid=0):
        self._enc_prefix = bytes(encode_nonce_prefix)
        self._dec_prefix = bytes(decode_nonce_prefix)
        self._downgrade_sub = bool(downgrade_sub)
        self._ctx = ctx if ctx is not None else CurveContext(0, 1)
        self._sid = sid
        self._cn_nonce = 1  # src/curve_mechanism_base.cpp:59-60
        self._precom = bytearray(32)
        self._installed = None

    def get_writable_precom_buffer(self):
        self._installed = None
        return self._precom

    def _install(self, peer_nonce=None):
        key = bytes(self._precom)
        if self._installed != key:
            cur = 1 if peer_nonce is None else peer_nonce
            self._ctx.session_set(self._sid, key, self._enc_prefix, self._dec_prefix, self._downgrade_sub, cur)
            self._installed = key

    def get_and_inc_nonce(self):
        n = self._cn_nonce
        self._cn_nonce += 1
        return n

    def set_peer_nonce(self, nonce):
        self._install()
        self._ctx.set_peer_nonce(self._sid, nonce)

    def get_peer_nonce(self):
        self._install()
        return self._ctx.get_peer_nonce(self._sid)

    def encode(self, msg):
        """Replaces msg's content with the MESSAGE frame; returns 0."""
        self._install()
        nonce = self.get_and_inc_nonce()
        payload = np.frombuffer(msg.data, np.uint8) if msg.size() else np.zeros(1, np.uint8)
        ws = wire_size(msg.flags, self._downgrade_sub, msg.size())
        out = self._ctx.encode_host([self._sid], [nonce], [msg.flags], [0], [msg.size()], payload, [0], ws)
        msg.data = out.tobytes()
        msg.flags = 0  # the encoder output is a fresh msg_t (src/curve_mechanism_base.cpp:167-177)
        return 0

    def decode(self, msg):
        """Returns (rc, error_event_code): (0, None) and msg holds the payload
        with the decoded flags ORed in, or (-1, code) with errno EPROTO."""
        self._install()
        wire = np.frombuffer(msg.data, np.uint8) if msg.size() else np.zeros(1, np.uint8)
        plen = max(msg.size() - 33, 0)
        out, fl, st = self._ctx.decode_host([self._sid], [0], [msg.size()], wire, [0], plen)
        if st[0] != 0:
            return -1, int(st[0])
        msg.data = out[:plen].tobytes()
        msg.set_flags(int(fl[0]))
        return 0, None


EPROTO = errno.EPROTO
