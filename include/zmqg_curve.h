/*
 * zmqg_curve.h -- C ABI of the MI355X CurveZMQ MESSAGE AEAD path.
 *
 * This is the drop-in boundary for libzmq's CURVE message codec:
 *
 *   reference call                                   replaced by
 *   -----------------------------------------------  ---------------------------
 *   curve_encoding_t::encode
 *     src/curve_mechanism_base.cpp:111-205           zmqg_encode_batch
 *     (crypto_box_easy_afternm :172-174)
 *   curve_mechanism_base_t::decode
 *     src/curve_mechanism_base.cpp:38-52             zmqg_decode_batch
 *     check_basic_command_structure
 *       src/mechanism_base.cpp:14-25
 *     curve_encoding_t::decode / check_validity
 *       src/curve_mechanism_base.cpp:80-109, 207-284
 *     (crypto_box_open_easy_afternm :226-228)
 *   curve_encoding_t state (_cn_precom, prefixes,
 *     _downgrade_sub, _cn_peer_nonce)
 *     src/curve_mechanism_base.hpp:44-58             zmqg_session_set,
 *                                                    zmqg_session_*_peer_nonce
 *   curve_encoding_t::get_writable_precom_buffer
 *     src/curve_mechanism_base.hpp:36                zmqg_session_set (precom)
 *   curve_encoding_t::set_peer_nonce
 *     src/curve_mechanism_base.hpp:42                zmqg_session_set_peer_nonce
 *   curve_encoding_t::get_and_inc_nonce (_cn_nonce)
 *     src/curve_mechanism_base.hpp:41                ZMQG_OPT_NONCE_AUTO,
 *                                                    zmqg_session_*_nonce
 *   curve_server_t::process_hello, produce_welcome
 *     src/curve_server.cpp:117-254                   zmqg_curve_server_hello_batch
 *   curve_server_t::process_initiate (to ZAP)
 *     src/curve_server.cpp:256-383                   zmqg_curve_server_initiate_batch
 *   curve_server_t::produce_ready
 *     src/curve_server.cpp:419-458                   zmqg_curve_server_ready_batch
 *   crypto_box_keypair, produce_hello
 *     src/curve_client_tools.hpp:230-234, :29-65     zmqg_curve_client_hello_batch
 *   process_welcome, produce_initiate
 *     src/curve_client_tools.hpp:67-199              zmqg_curve_client_welcome_batch
 *   curve_client_t::process_ready (to parse_metadata)
 *     src/curve_client.cpp:179-214                   zmqg_curve_client_ready_batch
 *   ws_decoder_t + curve_mechanism_base_t::decode
 *     src/ws_decoder.cpp:39-249,
 *     src/ws_engine.cpp:887-915                      zmqg_decode_ws_multi
 *   curve_encoding_t::encode + ws_encoder_t
 *     src/ws_encoder.cpp:26-126                      zmqg_encode_ws_multi
 *   zmq_proxy's forward over CURVE connections
 *     src/proxy.cpp:90-138, src/fq.cpp:52-94,
 *     src/dist.cpp:127-189, src/pipe.cpp:222-247     zmqg_forward_zmtp_multi
 *   xpub_t::xsend / mtrie match / dist_t::match
 *     src/xpub.cpp:290-326,
 *     src/generic_mtrie_impl.hpp:523-561,
 *     src/dist.cpp:49-62                             zmqg_forward_zmtp_sub_multi
 *   xpub_t::xread_activated / mtrie add, rm / xpipe_terminated
 *     src/xpub.cpp:72-170, :253-277,
 *     src/generic_mtrie_impl.hpp:41-126, 376-521     zmqg_subs_update_multi
 *   router_t::xrecv / xsend, lookup_out_pipe
 *     src/router.cpp:263-332, :161-261,
 *     src/socket_base.cpp:2187-2200                  zmqg_forward_zmtp_router_multi
 *   lb_t::sendpipe (dealer_t::sendpipe, push_t::xsend)
 *     src/lb.cpp:56-131, src/dealer.cpp:110-113,
 *     src/push.cpp:45-48                             zmqg_forward_zmtp_lb_multi
 *   ws_engine_t on either side of zmq_proxy's forward
 *     src/proxy.cpp:90-138,
 *     src/ws_decoder.cpp:39-249,
 *     src/ws_encoder.cpp:26-126                      zmqg_forward_framed_multi
 *   pipe_t::check_hwm / check_write / write, dist_t::write, router_t::xsend
 *     src/pipe.cpp:535-541, :207-234,
 *     src/dist.cpp:196-210, src/router.cpp:185-200   zmqg_forward_credit_multi
 *   lb_t::sendpipe with pipes that refuse a write
 *     src/lb.cpp:56-131 (:103-107),
 *     src/pipe.cpp:207-220, :535-541                 zmqg_forward_lb_credit_multi
 *
 * One call processes a batch of independent MESSAGE frames.  Each frame
 * belongs to a session (one CURVE connection = one curve_encoding_t).  The
 * caller assigns encode nonces, or lets the device take them from each
 * session's send counter (ZMQG_OPT_NONCE_AUTO; the reference's
 * get_and_inc_nonce, src/curve_mechanism_base.hpp:41).  Decode applies the reference's replay
 * rule exactly as if curve_encoding_t::decode had been called on the batch's
 * frames one by one in batch order, and updates each session's peer nonce.
 *
 * Conventions
 *   - Return 0 on success, a negative errno value on failure (-EINVAL bad
 *     argument, -ENOMEM, -EIO a HIP runtime error).  Per-frame protocol
 *     errors are not call failures: they are reported in status_out with the
 *     reference's codes (ZMQ_PROTOCOL_ERROR_ZMTP_*, include/zmq.h:424-437).
 *   - Batch pointers (descriptors, in, out, flags_out, status_out) must be
 *     device memory of the ctx's device, or host memory the device can
 *     access (hipHostMalloc).  Batch calls are asynchronous on `stream`
 *     (a hipStream_t; NULL = the null stream); results are valid once the
 *     stream has been synchronised.
 *   - A ctx is externally synchronised, like the reference's mechanism (one
 *     I/O thread per connection): issue one ctx's batches on one stream.
 *   - No exceptions cross this boundary.
 */
#ifndef ZMQG_CURVE_H_INCLUDED
#define ZMQG_CURVE_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZMQG_CURVE_ABI_VERSION 5

/* Per-frame status codes, identical to include/zmq.h:424-437. */
#define ZMQG_STATUS_OK 0
#define ZMQG_ERR_UNEXPECTED_COMMAND 0x10000001  /* ZMQ_PROTOCOL_ERROR_ZMTP_UNEXPECTED_COMMAND */
#define ZMQG_ERR_INVALID_SEQUENCE 0x10000002    /* ZMQ_PROTOCOL_ERROR_ZMTP_INVALID_SEQUENCE */
#define ZMQG_ERR_MALFORMED_UNSPECIFIED 0x10000011 /* ..._MALFORMED_COMMAND_UNSPECIFIED */
#define ZMQG_ERR_MALFORMED_MESSAGE 0x10000012   /* ..._MALFORMED_COMMAND_MESSAGE */
#define ZMQG_ERR_CRYPTOGRAPHIC 0x11000001       /* ZMQ_PROTOCOL_ERROR_ZMTP_CRYPTOGRAPHIC */
/* Library codes (not protocol errors; the reference has no equivalent):
 * ZMQG_ERR_SESSION  sid[i] >= the ctx's max_sessions (the frame is not
 *                   processed; decode: payload region zero-filled as for a
 *                   header failure)
 * ZMQG_ERR_BOUND    the frame is longer than zmqg_batch_opts.max_len (the
 *                   caller's promise was broken; the frame is not processed
 *                   and its output region is left as it was)
 * ZMQG_ERR_HWM      zmqg_forward_credit_multi: the pair was live and its
 *                   destination's credit refused its message;
 *                   zmqg_forward_lb_credit_multi: the pair's message found
 *                   every entry of its group's ring full */
#define ZMQG_ERR_SESSION 0x7a000001
#define ZMQG_ERR_BOUND 0x7a000002
#define ZMQG_ERR_HWM 0x7a000003

/* msg_t flag bits used on this path (src/msg.hpp:55-62). */
#define ZMQG_MSG_MORE 1
#define ZMQG_MSG_COMMAND 2
#define ZMQG_MSG_SUBSCRIBE 12
#define ZMQG_MSG_CANCEL 16

typedef struct zmqg_ctx zmqg_ctx;

/* ABI version of the loaded library (== ZMQG_CURVE_ABI_VERSION). */
int zmqg_abi_version(void);

/* Create a context on HIP device `device` with a session table of
 * `max_sessions` entries (sids 0 .. max_sessions-1). */
int zmqg_ctx_create(int device, uint32_t max_sessions, zmqg_ctx **ctx_out);
int zmqg_ctx_destroy(zmqg_ctx *ctx);

/* Install session `sid`: the connection's precomputed key (_cn_precom, the
 * output of crypto_box_beforenm, src/curve_client_tools.hpp:105 /
 * src/curve_server.cpp:382-383), the 16-byte encode/decode nonce prefixes
 * ("CurveZMQMESSAGEC"/"CurveZMQMESSAGES" swapped per side,
 * src/curve_client.cpp:22-23, src/curve_server.cpp:24-25), the downgrade_sub
 * flag (src/zmtp_engine.cpp:339-351) and the initial peer nonce (the
 * reference starts at 1 and the handshake advances it).  The two XSalsa20
 * subkeys HSalsa20(precom, prefix) are derived on the device.  Synchronous. */
int zmqg_session_set(zmqg_ctx *ctx, uint32_t sid, const uint8_t precom[32], const uint8_t enc_prefix[16],
                     const uint8_t dec_prefix[16], int downgrade_sub, uint64_t peer_nonce);

/* Install n sessions in one launch, asynchronously on `stream`: the mass
 * handshake's counterpart of zmqg_session_set (each server connection's
 * precom comes from crypto_box_beforenm at src/curve_server.cpp:382-383, each
 * client's at src/curve_client_tools.hpp:105; zmqg_box_beforenm_batch
 * derives them on the device and its k_out is passed here as is).
 *   sid          host array: n distinct session ids below max_sessions
 *                (-EINVAL otherwise)
 *   precom       device-accessible, 4-byte aligned: session i's 32-byte
 *                precomputed key at precom[32*i]
 *   enc_prefix, dec_prefix   the 16-byte nonce prefixes, common to the batch
 *                (one side's connections all use the same pair)
 *   downgrade    host array of n downgrade_sub flags, or NULL (all 0)
 *   peer_nonce   host array of n initial peer nonces, or NULL (all 1)
 * The send nonce of each session starts at 1, as with zmqg_session_set.
 * The host arrays are copied before the call returns; the install runs on
 * `stream` (batch calls issued after it on that stream see the sessions),
 * and the ctx's accessors order after it.  A second install waits for the
 * first to have read its descriptors. */
int zmqg_session_set_batch(zmqg_ctx *ctx, uint64_t n, const uint32_t *sid, const uint8_t *precom,
                           const uint8_t enc_prefix[16], const uint8_t dec_prefix[16], const uint8_t *downgrade,
                           const uint64_t *peer_nonce, void *stream);
/* The same with each session's send nonce: send_nonce is a host array of n
 * initial send nonces, or NULL (all 1).  A connection installed after its
 * handshake continues from the handshake's nonces -- the client's MESSAGE
 * nonces start at 3 after HELLO (1) and INITIATE (2), src/curve_client.cpp
 * and curve_client_tools.hpp; the server's at 2 after READY (1) -- so a
 * mass install needs no zmqg_session_set_nonce call per session. */
int zmqg_session_set_batch_ex(zmqg_ctx *ctx, uint64_t n, const uint32_t *sid, const uint8_t *precom,
                              const uint8_t enc_prefix[16], const uint8_t dec_prefix[16], const uint8_t *downgrade,
                              const uint64_t *peer_nonce, const uint64_t *send_nonce, void *stream);

/* curve_encoding_t::set_peer_nonce / read back _cn_peer_nonce.  Synchronous:
 * they are ordered after the work previously issued on the stream of the
 * ctx's last batch call (no device-wide synchronisation). */
int zmqg_session_set_peer_nonce(zmqg_ctx *ctx, uint32_t sid, uint64_t peer_nonce);
int zmqg_session_get_peer_nonce(zmqg_ctx *ctx, uint32_t sid, uint64_t *peer_nonce_out);

/* The session's send nonce (_cn_nonce, src/curve_mechanism_base.hpp:41-50):
 * the next nonce zmqg_encode_batch_ex assigns under ZMQG_OPT_NONCE_AUTO.
 * zmqg_session_set starts it at 1, as the reference's constructor does
 * (src/curve_mechanism_base.cpp:59); set it after the handshake has used its
 * nonces.  Synchronous, ordered like the peer-nonce accessors. */
int zmqg_session_set_nonce(zmqg_ctx *ctx, uint32_t sid, uint64_t nonce);
int zmqg_session_get_nonce(zmqg_ctx *ctx, uint32_t sid, uint64_t *nonce_out);

/* Bytes of the encoded frame for a payload of `payload_len` bytes and msg_t
 * flags `msg_flags`: "\x07MESSAGE"(8) + nonce(8) + tag(16) + mlen, where
 * mlen = 1 + [1 | 7 | 10 for SUBSCRIBE/CANCEL] + payload_len
 * (src/curve_mechanism_base.cpp:113-128, 169). */
uint64_t zmqg_wire_size(uint8_t msg_flags, int downgrade_sub, uint64_t payload_len);

/* Encode n frames (curve_encoding_t::encode).  Frame i: session sid[i],
 * nonce nonce[i], msg_t flags flags[i], payload in[in_off[i] .. +len[i]).
 * Writes zmqg_wire_size(flags[i], session.downgrade_sub, len[i]) bytes at
 * out[out_off[i]]: "\x07MESSAGE" || BE64(nonce) || tag || ciphertext.
 * Output frames must not overlap each other or the input.  sid[i] must be
 * below max_sessions: a frame with another sid is not encoded (its output
 * region is left as it was; zmqg_encode_batch_ex reports it). */
int zmqg_encode_batch(zmqg_ctx *ctx, uint64_t n, const uint32_t *sid, const uint64_t *nonce, const uint8_t *flags,
                      const uint64_t *in_off, const uint32_t *len, const uint8_t *in, const uint64_t *out_off,
                      uint8_t *out, void *stream);

/* Decode n frames (curve_mechanism_base_t::decode).  Frame i: session sid[i],
 * wire bytes in[in_off[i] .. +wire_len[i]).  On success status_out[i] = 0,
 * flags_out[i] = plaintext flags & (MORE|COMMAND) (the caller ORs them into
 * the msg_t, as msg_t::set_flags does, src/msg.cpp:433-436) and the payload,
 * wire_len[i] - 33 bytes, is written at out[out_off[i]].  On failure
 * status_out[i] is the reference's error code, flags_out[i] = 0 and, when
 * wire_len[i] >= 33, the payload region is zero-filled: plaintext of a frame
 * that failed is never left in `out`.  Each session's peer nonce advances as
 * the reference's check_validity does (src/curve_mechanism_base.cpp:98-106,
 * including on a later MAC failure).
 *
 * In-place decode: `out` may be `in`, with every frame in one of two
 * layouts: out_off[i] = in_off[i] + 33, each payload byte over its own
 * ciphertext byte (the reference's crypto_box_open_easy_afternm decrypts
 * into message + 16, src/curve_mechanism_base.cpp:222-228, which puts the
 * flags byte at wire offset 16 and the payload at 17 -- a different layout,
 * not offered here), or out_off[i] = in_off[i], the payload at the frame's
 * start as after the reference's memmove (:253-260).  Otherwise `out` must not overlap `in`.  On
 * failure the payload region is zero-filled as above; in the second layout a
 * frame of more than 4.5 KiB that fails has its whole wire region zeroed.
 *
 * Unauthenticated plaintext: the kernels decrypt and authenticate in one
 * pass, so until the call has completed on its stream, `out` may hold
 * plaintext of frames that then fail (it is zeroed before completion).  The
 * reference's libsodium verifies first and writes nothing for a forged frame
 * (SURVEY.md a12).  Results at completion are identical; a caller whose
 * `out` is visible to another party while the call runs (e.g. mapped host
 * memory read by a second thread) sets ZMQG_OPT_VERIFY_FIRST
 * (zmqg_decode_batch_ex), under which `out` only ever receives verified
 * payloads and zeros. */
int zmqg_decode_batch(zmqg_ctx *ctx, uint64_t n, const uint32_t *sid, const uint64_t *in_off,
                      const uint32_t *wire_len, const uint8_t *in, const uint64_t *out_off, uint8_t *out,
                      uint8_t *flags_out, int32_t *status_out, void *stream);

/* Options of the _ex batch calls (every field optional: a zeroed struct, or
 * opts = NULL, gives the plain calls' behaviour).
 *   size             sizeof(zmqg_batch_opts) (ABI check)
 *   flags            ZMQG_OPT_NONCE_AUTO (encode): ignore `nonce` (it may be
 *                    NULL) and take each frame's nonce from its session's
 *                    send counter on the device, in batch order, as
 *                    curve_encoding_t::get_and_inc_nonce does per message
 *                    (src/curve_mechanism_base.hpp:41, called at
 *                    src/curve_mechanism_base.cpp:116); the counters advance
 *                    by each session's frame count.  Several sessions: at
 *                    most 8192 (-EINVAL above).
 *   max_len          0, or a bound on every len[i] (encode) / wire_len[i]
 *                    (decode).  A bound under which every frame fits the frame
 *                    kernel (stream <= 4.5 KiB: decode wire_len <= 4608, encode
 *                    len <= 4565) lets the call skip the large-frame kernels
 *                    (two fewer launches).  A frame above the bound fails with
 *                    ZMQG_ERR_BOUND.  Under ZMQG_OPT_NONCE_AUTO such a frame
 *                    of a known session still takes its nonce (the session's
 *                    counter counts every frame of the batch that names it,
 *                    with one session and with several), so the nonces on
 *                    the wire have a gap there.
 *   status_out       encode only: n entries (device-accessible), 0 or
 *                    ZMQG_ERR_SESSION / ZMQG_ERR_BOUND per frame.
 *   session_max_out  decode only: max_sessions entries (device-accessible):
 *                    per session, the largest header-valid nonce among this
 *                    batch's frames (0 where it has none) -- the value a rank
 *                    contributes to shard.peer_prefix when a session's frames
 *                    span GPUs.
 *   flags            ZMQG_OPT_VERIFY_FIRST (decode): no byte of `out` is
 *                    written before the frame's tag and replay verdict, as
 *                    libsodium's open verifies before it decrypts
 *                    (src/curve_mechanism_base.cpp:226-228).  The frames are
 *                    decoded into a device staging area of the ctx laid out
 *                    like `out`, then one kernel copies each verified payload
 *                    to out[out_off[i]] and zero-fills the payload region of
 *                    each failed one (a frame above max_len, or shorter than
 *                    33 bytes, is left as it was).  Needs out_bytes.  For
 *                    `out` another party can read while the call runs (mapped
 *                    host memory: curve_batcher_t's receive slots).  Costs one
 *                    extra read and write of the payload bytes.
 *   out_bytes        extent of `out`: every out_off[i] + wire_len[i] - 33 is
 *                    at most this (required by ZMQG_OPT_VERIFY_FIRST, which
 *                    checks it on the device: a frame whose payload region
 *                    would end past out_bytes fails with ZMQG_ERR_BOUND and
 *                    nothing of it is written; 0 is valid for a batch whose
 *                    frames carry no payload bytes).
 *   flags            ZMQG_OPT_REPLAY_HOST (decode, with VERIFY_FIRST and
 *                    verdict_in): the caller has already applied the header
 *                    rules and the replay rule to the frames in batch order,
 *                    as check_basic_command_structure and check_validity do
 *                    (src/mechanism_base.cpp:14-25,
 *                    src/curve_mechanism_base.cpp:80-106: the nonce must
 *                    exceed the connection's peer nonce, which advances
 *                    before the MAC), keeping the connections' peer nonces
 *                    itself -- a host that sees every frame in order does
 *                    this with one compare per frame.  The device then only
 *                    authenticates and opens: it neither reads nor writes its
 *                    sessions' peer nonces (zmqg_session_set_peer_nonce
 *                    before a later call that does), and the call is two
 *                    kernel launches instead of seven for several sessions.
 *   verdict_in       with ZMQG_OPT_REPLAY_HOST: n entries (device-accessible),
 *                    per frame 0 (open it) or the ZMQG_ERR_* code the host's
 *                    rules gave it, which is then the frame's status (its
 *                    payload region zero-filled, flags 0).
 *   flags            ZMQG_OPT_STREAM_OUT (decode, and encode in
 *                    zmqg_encode_batch_ex): a cache hint, results unchanged.
 *                    The outputs go to memory the device's caches do not
 *                    hold (batches rotating over more buffers than the 256
 *                    MiB Infinity Cache keeps, as a receive ring does): each
 *                    64-byte output piece is staged through LDS and leaves a
 *                    step later with 15 other frames' in one store
 *                    instruction, instead of each lane's own 16-byte pieces.
 *                    Config 2 from HBM: decode 60 against 75 us, encode 66
 *                    against 71 us; with the output lines already cached it
 *                    costs the decode ~5 us.
 *                    Applies to the one-lane-per-frame kernel; on decode
 *                    when every payload starts 64-byte aligned.
 * A caller built against the struct without out_bytes (or verdict_in)
 * passes the smaller size and gets the old behaviour. */
#define ZMQG_OPT_NONCE_AUTO 1u
#define ZMQG_OPT_VERIFY_FIRST 2u
#define ZMQG_OPT_REPLAY_HOST 4u
#define ZMQG_OPT_STREAM_OUT 8u
typedef struct zmqg_batch_opts {
    uint32_t size;
    uint32_t flags;
    uint64_t max_len;
    int32_t *status_out;
    uint64_t *session_max_out;
    uint64_t out_bytes;
    const int32_t *verdict_in;
} zmqg_batch_opts;
int zmqg_encode_batch_ex(zmqg_ctx *ctx, uint64_t n, const uint32_t *sid, const uint64_t *nonce, const uint8_t *flags,
                         const uint64_t *in_off, const uint32_t *len, const uint8_t *in, const uint64_t *out_off,
                         uint8_t *out, const zmqg_batch_opts *opts, void *stream);
int zmqg_decode_batch_ex(zmqg_ctx *ctx, uint64_t n, const uint32_t *sid, const uint64_t *in_off,
                         const uint32_t *wire_len, const uint8_t *in, const uint64_t *out_off, uint8_t *out,
                         uint8_t *flags_out, int32_t *status_out, const zmqg_batch_opts *opts, void *stream);

/* Header pass of a sharded decode: writes
 * session_max_out[s] (max_sessions entries, device-accessible) = the largest
 * header-valid nonce among the n wire frames of session s (0 where none).
 * When one session's frames are split over ranks (GPUs), rank r decodes its
 * slice after setting each session's peer nonce to max(peer before the batch,
 * the session maxima of ranks < r) -- the exclusive max-scan over ranks of
 * these vectors (libzmq_amd/shard.py peer_prefix) -- and the slices' results
 * equal one decode of the whole batch.  Reads 16 bytes per frame.
 * Asynchronous on `stream`. */
int zmqg_session_max_batch(zmqg_ctx *ctx, uint64_t n, const uint32_t *sid, const uint64_t *in_off,
                           const uint32_t *wire_len, const uint8_t *in, uint64_t *session_max_out, void *stream);

/* Host-memory convenience forms of the two batch calls: every pointer is
 * ordinary (pageable) host memory.  They stage through the ctx's pinned
 * buffers with hipMemcpyAsync H2D, run the batch and copy back D2H, and
 * return after the stream has synchronised.  This is the path an I/O thread
 * calling with socket buffers takes. */
int zmqg_encode_host(zmqg_ctx *ctx, uint64_t n, const uint32_t *sid, const uint64_t *nonce, const uint8_t *flags,
                     const uint64_t *in_off, const uint32_t *len, const uint8_t *in, uint64_t in_bytes,
                     const uint64_t *out_off, uint8_t *out, uint64_t out_bytes);
int zmqg_decode_host(zmqg_ctx *ctx, uint64_t n, const uint32_t *sid, const uint64_t *in_off,
                     const uint32_t *wire_len, const uint8_t *in, uint64_t in_bytes, const uint64_t *out_off,
                     uint8_t *out, uint64_t out_bytes, uint8_t *flags_out, int32_t *status_out);

/* One message on one session, host memory in and out: the call the
 * reference engine makes per message (curve_encoding_t::encode / decode,
 * src/curve_mechanism_base.cpp:111-205, :207-284, from
 * src/stream_engine_base.cpp:331-348 / :281-291) without descriptor arrays.
 * The bytes are copied once into the ctx's page-locked, device-mapped
 * message buffer, the frame kernel works on it in place over PCIe (no
 * hipMemcpy), and the result is copied once out of it after the stream
 * has synchronised.
 *
 * zmqg_encode_msg: `out` receives zmqg_wire_size(flags, downgrade of sid,
 * len) bytes, the MESSAGE command for `nonce`.
 * zmqg_decode_msg: `out` receives wire_len - 33 payload bytes (`out` may be
 * `in`: the payload then starts at in[0]; a frame shorter than 33 bytes
 * fails its header checks and needs no room), *flags_out the
 * plaintext MORE / COMMAND bits and *status_out 0 or the
 * ZMQ_PROTOCOL_ERROR_ZMTP_* code; on a failure `out` is left untouched and
 * the session's peer nonce advances as the reference's does.
 * Both return 0 or -errno (-EINVAL for bad arguments). */
int zmqg_encode_msg(zmqg_ctx *ctx, uint32_t sid, uint64_t nonce, uint8_t flags, const uint8_t *in, uint32_t len,
                    uint8_t *out);
int zmqg_decode_msg(zmqg_ctx *ctx, uint32_t sid, const uint8_t *in, uint32_t wire_len, uint8_t *out,
                    uint8_t *flags_out, int32_t *status_out);

/* Asynchronous host path.  The reference's
 * engine encodes and decodes one message at a time on the I/O thread
 * (src/stream_engine_base.cpp:281-291 in_event, :331-348 out_event); an
 * engine that batches across its connections instead needs host memory the
 * kernels can work on in place and a way to learn, without blocking, that a
 * submitted batch is finished.
 *
 * zmqg_host_alloc returns page-locked host memory mapped into the device's
 * address space: batch calls take pointers into it directly (descriptors,
 * `in`, `out`, flags_out, status_out) and the kernels read and write it over
 * PCIe with no staging copy.  Free it with zmqg_host_free (after the batches
 * using it have finished).
 *
 * zmqg_ctx_stream gives the ctx's own non-blocking stream for callers without
 * one.  zmqg_fence_record marks the point after everything issued so far on
 * `stream` and returns a fence id (ids increase per ctx); zmqg_fence_query
 * returns 1 once the stream has passed it, 0 while it has not (never
 * blocks), and zmqg_fence_wait blocks until it has.  A fence is released by
 * the first query or wait that finds it reached; later queries of a released
 * or unknown id below the last issued one return 1. */
int zmqg_host_alloc(zmqg_ctx *ctx, uint64_t bytes, void **ptr_out);
int zmqg_host_free(zmqg_ctx *ctx, void *ptr);
int zmqg_ctx_stream(zmqg_ctx *ctx, void **stream_out);
int zmqg_fence_record(zmqg_ctx *ctx, void *stream, uint64_t *fence_out);
int zmqg_fence_query(zmqg_ctx *ctx, uint64_t fence);
int zmqg_fence_wait(zmqg_ctx *ctx, uint64_t fence);

/* Completion wake-up for a sleeping I/O thread.  The reference's I/O thread
 * sleeps in epoll_wait (src/epoll.cpp:157-158) and is woken only by a file
 * descriptor it watches -- its mailbox's eventfd (src/io_thread.cpp:54,
 * src/signaler.cpp) or a socket; an engine with nothing to write has reset
 * POLLOUT (src/stream_engine_base.cpp:350-353) and resumes only through
 * restart_output / restart_input (:383-390, :400-442).
 *
 * zmqg_fence_record_notify is zmqg_fence_record plus a wake-up: once the
 * stream has passed the fence, an 8-byte 1 is written to `fd` (eventfd
 * counter semantics; a pipe's write end works too) from a HIP runtime thread,
 * and from then on zmqg_fence_query of that fence returns 1.  The poller
 * watches `fd` for POLLIN, reads it, and polls its fences.  `fd` must stay
 * open until zmqg_notify_quiesce has returned 0: that call waits until every
 * notification enqueued on the ctx so far has been delivered (the streams
 * must be able to reach them), at most ~10 s: -ETIMEDOUT then (a stuck
 * stream), and `fd` must stay open.  zmqg_ctx_destroy waits for them too and,
 * on such a timeout, returns -ETIMEDOUT with the ctx's host state left
 * allocated for the late host functions.  If the fence is recorded but its
 * notification cannot be queued, the call fails with *fence_out set (the
 * fence can still be waited for); a failure before the fence leaves it 0.
 * (Replaces no reference symbol: the reference codec is synchronous.) */
int zmqg_fence_record_notify(zmqg_ctx *ctx, void *stream, int fd, uint64_t *fence_out);
int zmqg_notify_quiesce(zmqg_ctx *ctx);

/* ZMTP framing on the device.
 *
 * zmqg_encode_zmtp: zmqg_encode_batch plus the engine's ZMTP encoder
 * (src/v3_1_encoder.cpp:23-60) in one call: the n encoded MESSAGE commands
 * are laid out back to back in `out` as ZMTP frames -- flags (0, or LARGE
 * when the body exceeds 255 bytes; the boxed msg_t carries no MORE/COMMAND,
 * src/curve_mechanism_base.cpp:166-177), size (1 byte, or 8 bytes big
 * endian), body -- ready to be written to the socket.  frame_off[0..n]
 * (device-accessible, n + 1 entries) receives each frame's offset and the
 * total in frame_off[n]; offsets are computed on the device.  Asynchronous.
 *
 * zmqg_decode_zmtp: the engine's ZMTP decoder (src/v2_decoder.cpp:35-140)
 * and curve_mechanism_base_t::decode over a received byte stream of one
 * connection (session sid), on the device.  Frames are found from offset 0;
 * up to max_frames of them are decoded: frame i's body is
 * in[frame_in_off[i] .. +frame_len[i]), its payload (frame_len[i] - 33
 * bytes) is written at out[out_off[i]] with out_off[i] = frame_in_off[i] --
 * the body's own offset, so `out` may be `in` (decoded in place, each
 * payload left at its body's start as after the reference's memmove,
 * src/curve_mechanism_base.cpp:253-260: a received buffer becomes the
 * messages' data without a copy, as v2_decoder's zero-copy msg_t slices do,
 * src/v2_decoder.cpp:88-113) -- and flags_out / status_out are as for zmqg_decode_batch,
 * with the ZMTP frame's MORE / COMMAND bits ORed into flags_out of a
 * decoded frame (msg_t::set_flags ORs, src/msg.cpp:433-436).  result:
 * frames returned, bytes of `in` they cover (an incomplete last frame is
 * left for the next call), payload bytes written (their sum), and error = EMSGSIZE when
 * a frame's size exceeds max_msg_size (>= 0; -1 = no limit), where the
 * reference decoder fails (src/v2_decoder.cpp:74-84): the frames before it
 * are returned.  A size above 2^32 - 1 also ends the parse with EMSGSIZE:
 * that is a restriction of this library (frame lengths are 32-bit), not
 * reference behaviour -- on LP64 the reference's size_t check
 * (src/v2_decoder.cpp:78) never fires and it would accept such a frame.  A complete frame that is not a MESSAGE command
 * is returned as the last frame, with the status the mechanism gives it;
 * the reference's engine stops at the first failing frame, and so should
 * the caller.  Arrays hold max_frames entries (entries from result.frames
 * on hold empty frames: length 0, a malformed status); `out` at least
 * in_bytes.  Returns after the stream has synchronised: the result is the
 * call's only read back (the frame count stays on the device; the decode
 * runs over max_frames).  in_bytes < 2^31; any byte alignment of `in` is valid
 * (the scan cuts the stream in 16-byte-aligned address space and reads no byte
 * outside [in, in + in_bytes)).
 * Early stop: a call may return fewer frames than are complete in the buffer,
 * with error == 0, frames < max_frames, consumed < in_bytes and every status
 * as the mechanism gives it (0 for valid frames).  It happens when the seven
 * bytes in front of a short MESSAGE frame (the end of the previous frame's
 * body, which the peer chooses) read as a LARGE header whose size field, completed by the frame's own flags
 * and size bytes, passes max_msg_size and fits the buffer (for instance a
 * flags byte with the LARGE bit and six zero bytes: the size is then the
 * frame's own): the parse then ends with that frame as the call's last.  The
 * returned frames are always a prefix of the reference decoder's, so the
 * caller repeats the call from `consumed` (in + consumed, in_bytes - consumed)
 * until a call returns 0 frames; only then are the bytes left an incomplete
 * frame that waits for the socket.
 *
 * zmqg_decode_zmtp_async: the same, without synchronising: `result` must be
 * device-accessible (device memory, or pinned host memory from
 * zmqg_host_alloc) and holds the result once the stream reaches this point
 * (zmqg_fence_record / _query).
 *
 * zmqg_decode_zmtp_multi: the same decoder (src/v2_decoder.cpp:35-140,
 * maxmsgsize :74-84) over the receive buffers of many connections in one
 * asynchronous call -- an I/O thread's shape: n_streams buffers of at most
 * in_batch_size bytes each (src/options.cpp:221) -- with the semantics of
 * n_streams zmqg_decode_zmtp calls in stream order, with one exception: this
 * call's sequential parser has no early stop (see zmqg_decode_zmtp), it
 * returns every complete frame of a stream up to max_frames.  Stream s is
 * in[stream_off[s] .. +stream_len[s]), received on session stream_sid[s];
 * streams do not overlap, any byte alignment of stream_off is valid,
 * stream_len[s] < 2^31, and no byte outside a stream is read (nothing
 * between two streams is parsed).  The three stream arrays, the per-frame
 * arrays and results (n_streams entries) are device-accessible; the host
 * reads nothing back.  Every per-frame array holds n_streams * max_frames
 * entries (<= 2^31 - 1, else -EINVAL); stream s owns slots [s * max_frames,
 * (s + 1) * max_frames): slot s * max_frames + j, j < results[s].frames,
 * describes the stream's j-th frame as zmqg_decode_zmtp would -- frame_in_off
 * = out_off = the body's absolute offset in `in` (`out` may be `in`; otherwise
 * `out` spans the same offsets), frame_len the body size, flags_out the
 * plaintext bits with the frame's MORE / COMMAND bits ORed in, status_out as
 * for zmqg_decode_batch -- and the stream's remaining slots hold empty frames
 * (offset 0, length 0, a malformed status, flags 0).  results[s]: frames,
 * consumed (relative to stream_off[s]; an incomplete last frame is left for
 * the next call), out_bytes (the stream's payload bytes), error (0, or
 * EMSGSIZE where a size exceeds max_msg_size or 2^32 - 1: that stream ends
 * there, the frames before it are returned).  A complete frame that is not a
 * MESSAGE command is returned as its stream's last frame; a stream with more
 * than max_frames frames returns the first max_frames.  No stream's outcome
 * depends on another stream's bytes.  Replay and peer nonces are as if
 * curve_encoding_t::decode ran on all returned frames in slot order (stream
 * 0's frames, then stream 1's, ...): two streams may name one session, the
 * later one then sees the earlier one's nonces; stream_sid[s] >= max_sessions
 * gives that stream's frames ZMQG_ERR_SESSION.  With n_streams == 0 nothing is
 * done; with max_frames == 0 results is zero-filled on the stream.  The call
 * is one launch more than zmqg_decode_batch_ex (one workgroup per stream
 * parses it in LDS); ZMQG_OPT_VERIFY_FIRST / _REPLAY_HOST / _STREAM_OUT are
 * not offered on this call. */
typedef struct zmqg_zmtp_result {
    uint64_t frames;
    uint64_t consumed;
    uint64_t out_bytes;
    int32_t error;
    int32_t pad;
} zmqg_zmtp_result;
int zmqg_encode_zmtp(zmqg_ctx *ctx, uint64_t n, const uint32_t *sid, const uint64_t *nonce, const uint8_t *flags,
                     const uint64_t *in_off, const uint32_t *len, const uint8_t *in, uint8_t *out,
                     uint64_t *frame_off, void *stream);
int zmqg_decode_zmtp(zmqg_ctx *ctx, uint32_t sid, const uint8_t *in, uint64_t in_bytes, int64_t max_msg_size,
                     uint64_t max_frames, uint64_t *frame_in_off, uint32_t *frame_len, uint64_t *out_off,
                     uint8_t *out, uint8_t *flags_out, int32_t *status_out, zmqg_zmtp_result *result,
                     void *stream);
int zmqg_decode_zmtp_async(zmqg_ctx *ctx, uint32_t sid, const uint8_t *in, uint64_t in_bytes, int64_t max_msg_size,
                           uint64_t max_frames, uint64_t *frame_in_off, uint32_t *frame_len, uint64_t *out_off,
                           uint8_t *out, uint8_t *flags_out, int32_t *status_out, zmqg_zmtp_result *result,
                           void *stream);
int zmqg_decode_zmtp_multi(zmqg_ctx *ctx, uint64_t n_streams, const uint32_t *stream_sid,
                           const uint64_t *stream_off, const uint32_t *stream_len, const uint8_t *in,
                           int64_t max_msg_size, uint64_t max_frames, uint64_t *frame_in_off, uint32_t *frame_len,
                           uint64_t *out_off, uint8_t *out, uint8_t *flags_out, int32_t *status_out,
                           zmqg_zmtp_result *results, void *stream);

/* zmqg_encode_zmtp_multi: the send side of an I/O thread in one asynchronous
 * call.  The n outgoing messages come in arrival (batch) order, interleaved
 * over n_streams connections (A1 B1 A2 C1 B2 ...); every connection gets its
 * own contiguous run of ZMTP frames in `out`, ready for send() -- what
 * stream_engine_base_t::out_event builds per connection in _outpos
 * (src/stream_engine_base.cpp:314-380: the pull loop :331, the ZMTP encoder
 * :343, src/v2_encoder.cpp:23-60; out_batch_size, src/options.cpp:222).  The
 * batch is not sorted and the host reads nothing back; all arrays are
 * device-accessible.  Frame i belongs to stream frame_stream[i], which sends
 * on session stream_sid[frame_stream[i]].
 *
 * Validity.  A stream is valid when stream_sid[s] < max_sessions; a frame is
 * valid when frame_stream[i] < n_streams and its stream is valid.
 * Sizes.  For a valid frame W = zmqg_wire_size(flags[i], the session's
 * downgrade_sub, len[i]) and F(i) = W + (W > 255 ? 9 : 2), as in
 * zmqg_encode_zmtp.
 * Layout.  B(s) = the sum of F over the valid frames of stream s (0 for an
 * invalid stream); base(s) = the sum of B(t), t < s: the regions are packed
 * back to back in stream order; pos(i) = the sum of F(j) over the valid frames
 * j < i of the same stream.  frame_off[i] = base(stream) + pos(i) for a valid
 * frame, UINT64_MAX for an invalid one, and frame_off[n] = the sum of all B
 * (n + 1 entries).
 * Fit.  A valid frame fits when frame_off[i] + F(i) <= out_bytes (checked on
 * the device, as ZMQG_OPT_VERIFY_FIRST's out_bytes is: `out` is typically a
 * pinned slot of fixed size).  Offsets rise within a stream, so the fitting
 * frames of a stream are a prefix of it.
 *   - a valid frame that fits: its ZMTP header and MESSAGE command are written
 *     at out[frame_off[i] .. +F(i)), the bytes zmqg_encode_zmtp would write for
 *     that frame; status_out[i] = 0.
 *   - a valid frame that does not fit: nothing of it is written, status_out[i]
 *     = ZMQG_ERR_BOUND, frame_off[i] keeps its computed value, and it consumes
 *     no nonce.
 *   - an invalid frame: nothing is written, status_out[i] = ZMQG_ERR_SESSION.
 * Nonces.  nonce != NULL: frame i uses nonce[i] (the caller resubmits a frame
 * that did not fit with the same nonce).  nonce == NULL: the nonces come from
 * the sessions' device send counters, as under ZMQG_OPT_NONCE_AUTO, taken in
 * batch order over the fitting frames of each session; each counter advances
 * by its number of fitting frames.  Two streams may name one session: a later
 * frame in batch order then takes the later nonce, whichever stream it is in.
 * max_sessions > 8192 with nonce == NULL gives -EINVAL.
 * results[s] (n_streams entries): frames = the stream's fitting frames,
 * out_off = base(s), out_bytes = the sum of their F -- out[out_off ..
 * +out_bytes) goes to the socket, and on the peer these two are exactly
 * zmqg_decode_zmtp_multi's stream_off / stream_len -- and error = EINVAL for
 * an invalid stream (frames 0, bytes 0), ENOBUFS when a valid frame of the
 * stream did not fit, else 0.
 * No byte of `out` is written outside the ranges of fitting frames, and
 * nothing at or past out_bytes.  `out` must not overlap `in`.  status_out may
 * be NULL.  Frames of any size (those above 4.5 KiB go through the large-frame
 * kernels as in zmqg_encode_batch).  ZMQG_OPT_STREAM_OUT and max_len are not
 * offered on this call.
 * Returns -EINVAL for a null ctx, n_streams > 8192, n_streams == 0 with n > 0,
 * a null results or stream_sid with n_streams > 0, a null frame_off, a null
 * required array with n > 0, n > 2^31 - 1; -ENOMEM / -EIO as elsewhere.  With
 * n == 0, frame_off[0] = 0 and every results[s] is filled (frames 0, bytes 0,
 * out_off 0, error 0 or EINVAL) on the stream.  Five launches before the
 * encode's own (nine with device nonces), whatever n and n_streams are. */
typedef struct zmqg_zmtp_send_result {
    uint64_t frames;     /* frames of this stream that were encoded */
    uint64_t out_off;    /* start of the stream's region in `out` */
    uint64_t out_bytes;  /* bytes of the encoded frames: out[out_off .. +out_bytes) goes to the socket */
    int32_t error;       /* 0, ENOBUFS, EINVAL */
    int32_t pad;
} zmqg_zmtp_send_result;
int zmqg_encode_zmtp_multi(zmqg_ctx *ctx, uint64_t n_streams, const uint32_t *stream_sid, uint64_t n,
                           const uint32_t *frame_stream, const uint64_t *nonce, const uint8_t *flags,
                           const uint64_t *in_off, const uint32_t *len, const uint8_t *in, uint8_t *out,
                           uint64_t out_bytes, uint64_t *frame_off, int32_t *status_out,
                           zmqg_zmtp_send_result *results, void *stream);

/* zmqg_forward_zmtp_multi: a broker's I/O thread in one asynchronous call --
 * from the receive buffers of many connections to the send buffers of many
 * connections, what zmq_proxy does message by message (src/proxy.cpp:90-138,
 * fed by fq_t::recvpipe, src/fq.cpp:52-94, sending through lb_t or
 * dist_t::distribute, src/dist.cpp:127-189): decrypt a frame from connection A,
 * encrypt the same bytes for B, or for B, C and D.  It is
 * zmqg_decode_zmtp_multi, a plan made on the device, and
 * zmqg_encode_zmtp_multi, queued back to back: between the two the host neither
 * synchronises, nor reads statuses back, nor uploads descriptors.
 *
 * Receive side.  n_streams, stream_sid, stream_off, stream_len, in,
 * max_msg_size, max_frames, frame_in_off, frame_len, plain_off (that call's
 * out_off), plain (its out), flags_out, status_out and results are
 * zmqg_decode_zmtp_multi's arguments, and everything that call states holds:
 * every output is what that call writes -- slots, results, statuses, flags,
 * the payloads at plain[plain_off[..]], the peer nonces, plain == in, two
 * streams on one session, stream_sid[s] >= max_sessions.
 *
 * Sequence.  For source stream s, Q(s) is its carried parts, entries
 * carry_idx[s] .. carry_idx[s + 1] of carry_off / carry_len / carry_flags
 * (payloads plain[carry_off[i] .. +carry_len[i]) with their msg_t flags,
 * decoded by an earlier call and held back), followed by its returned frames,
 * slots j < results[s].frames.  c(s) is its number of carried parts, d(s) =
 * route_idx[s + 1] - route_idx[s] its number of routes, the destinations
 * route_dst[route_idx[s] ..]; destination t sends on session dst_sid[t], and a
 * stream that names a destination twice sends it two copies.  An element is a
 * command when its flags carry ZMQG_MSG_COMMAND.  Commands are never forwarded
 * and neither end nor break a message: the engine handles them itself
 * (src/stream_engine_base.cpp:635-637) and the session keeps them out of the
 * pipe; a carried entry with COMMAND set is skipped the same way.
 *
 * What is forwarded.  F(s) is the index in Q(s) of the first returned frame
 * with a non-zero status, or |Q(s)|; E(s) the largest index below F(s) of an
 * element that is no command and has ZMQG_MSG_MORE clear, or -1.  Exactly the
 * non-command elements below E(s) + 1 are forwarded, each to every route of
 * the stream: whole messages only, as parts become visible to the reader only
 * when their message is complete (pipe_t::write, src/pipe.cpp:222-234: the
 * ypipe is written with incomplete = more).  Messages completed before a
 * failing frame are still delivered (stream_engine_base_t::error flushes the
 * session, src/stream_engine_base.cpp:667-699); the incomplete tail of a failed
 * connection is dropped (pipe_t::rollback, src/pipe.cpp:236-247).
 * fwd[s] (n_streams entries): seq = |Q(s)|, held_first = E(s) + 1 (== seq:
 * nothing is held), forwarded = the elements forwarded, failed = 1 when a
 * returned frame of the stream has a non-zero status -- the host then drops
 * what is held instead of carrying it.  Held data parts (at or behind
 * held_first) stay decoded in `plain`: the host passes them as the stream's
 * carry in a later call and keeps that region of `plain` alive until then (a
 * returned frame becomes the carried part {plain_off, frame_len - 33,
 * flags_out}).  Held commands are the host's to process now.
 *
 * Pairs.  Element q of stream s (q < c(s) + max_frames, carry first) and its
 * k-th route form pair p = base(s) + q * d(s) + k, base(s) = the sum over t < s
 * of (c(t) + max_frames) * d(t); N = base(n_streams), which the host computes
 * from carry_idx and route_idx.  pair_off has N + 1 entries, pair_status N (or
 * is NULL).  A pair is live when its element is forwarded.
 *
 * Send side.  Exactly zmqg_encode_zmtp_multi over the N pairs in pair order
 * with n_dst streams, stream_sid = dst_sid and nonce == NULL (the sessions'
 * device send counters).  A live pair is the frame {frame_stream = its
 * destination, flags = the element's MORE bit alone, in = plain, in_off = the
 * element's offset in plain, len = its payload length: frame_len - 33 of a
 * returned frame, carry_len of a carried part}; a pair that is not live names
 * no stream.  All of that call's rules hold, with out, out_bytes, pair_off,
 * pair_status and dst_results as its out, out_bytes, frame_off, status_out and
 * results: layout, fit and the prefix property, ZMQG_ERR_BOUND with no nonce
 * taken, ENOBUFS / EINVAL in dst_results, two destinations on one session
 * taking nonces in pair order, nothing written at or past out_bytes.  A pair
 * that is not live, or whose destination's session is invalid, gets pair_status
 * ZMQG_ERR_SESSION and pair_off UINT64_MAX and takes no nonce.  Each
 * destination's run out[dst_results[t].out_off .. +out_bytes) so holds the
 * forwarded messages in (stream, element) order: the parts of one message are
 * contiguous and never interleaved with another source's, within a call and,
 * through the carry, across calls.  A pair that did not fit (ZMQG_ERR_BOUND)
 * is the host's to resend, with zmqg_encode_zmtp_multi from `plain`.
 *
 * Arrays marked HOST below are read on the host and copied (to pinned staging
 * of the ctx, as zmqg_session_set_batch copies its arrays) before the call
 * returns; a later call waits until the device has fetched them.  All others
 * are device-accessible, and the host reads nothing back.  `out` must not
 * overlap `in` or `plain`.
 * Returns -EINVAL for a null ctx or args, size != sizeof(zmqg_forward_zmtp) or
 * reserved != 0, the -EINVAL cases of the two underlying calls (n_streams,
 * max_frames or their product above 2^31 - 1, a null results, with max_frames
 * > 0 a null receive-side array, n_dst > 8192, max_sessions > 8192, with n_dst
 * > 0 a null dst_sid or dst_results, a null pair_off, with N > 0 a null plain
 * or out), a null fwd, a null route_idx, route_idx[0] != 0 or a falling
 * route_idx, a route_dst entry >= n_dst (or a null route_dst with routes), a
 * carry_idx that does not start at 0 or falls, null carry arrays with carried
 * parts, N > 2^31 - 1; nothing is queued then.  With n_streams == 0 nothing is
 * done.  With N == 0 the receive side and fwd are still done, pair_off[0] = 0
 * and dst_results are filled as zmqg_encode_zmtp_multi fills them for n == 0.
 * max_frames == 0 with carried parts is valid: results is zero-filled and the
 * carries alone are flushed.
 * Launches: zmqg_decode_zmtp_multi's (one more than zmqg_decode_batch_ex's),
 * one copy of the HOST arrays, two for the plan (one wave per source stream;
 * one lane per pair), then zmqg_encode_zmtp_multi's with device nonces (nine
 * before the encode's own), whatever the sizes are.  WebSocket framing on
 * either side is zmqg_forward_framed_multi; routing by XPUB topics is
 * zmqg_forward_zmtp_sub_multi, routing by ROUTER identities
 * zmqg_forward_zmtp_router_multi, DEALER's and PUSH's round-robin choice per
 * message (lb_t) zmqg_forward_zmtp_lb_multi: route_dst is per stream and per
 * call, and cannot give it. */
typedef struct zmqg_forward_result {   /* per source stream, 32 bytes */
    uint64_t seq;         /* elements of the stream's sequence Q(s) */
    uint64_t held_first;  /* index in Q(s) of the first element not forwarded (== seq: none held) */
    uint64_t forwarded;   /* elements forwarded (each to every destination of the stream) */
    int32_t failed;       /* 1: a returned frame of the stream has a non-zero status */
    int32_t pad;
} zmqg_forward_result;
typedef struct zmqg_forward_zmtp {
    uint32_t size, reserved;                       /* sizeof(zmqg_forward_zmtp), 0 */
    /* receive side: zmqg_decode_zmtp_multi's arguments and outputs */
    uint64_t n_streams;
    const uint32_t *stream_sid;
    const uint64_t *stream_off;
    const uint32_t *stream_len;
    const uint8_t *in;
    int64_t max_msg_size;
    uint64_t max_frames;
    uint64_t *frame_in_off;
    uint32_t *frame_len;
    uint64_t *plain_off;
    uint8_t *plain;                                /* may be `in` */
    uint8_t *flags_out;
    int32_t *status_out;
    zmqg_zmtp_result *results;
    /* parts carried over from earlier calls (optional) */
    const uint32_t *carry_idx;                     /* HOST, n_streams + 1, rising from 0; NULL = none */
    const uint64_t *carry_off;                     /* carry_idx[n_streams] entries each: offsets into plain, */
    const uint32_t *carry_len;                     /* payload lengths, */
    const uint8_t *carry_flags;                    /* msg_t flags */
    /* routes */
    uint64_t n_dst;
    const uint32_t *dst_sid;                       /* n_dst: the session each destination sends on */
    const uint32_t *route_idx;                     /* HOST, n_streams + 1, rising from 0 */
    const uint32_t *route_dst;                     /* HOST, route_idx[n_streams] entries, each < n_dst */
    /* send side: zmqg_encode_zmtp_multi's outputs over the pairs */
    uint8_t *out;
    uint64_t out_bytes;
    uint64_t *pair_off;                            /* N + 1 */
    int32_t *pair_status;                          /* N, or NULL */
    zmqg_zmtp_send_result *dst_results;            /* n_dst */
    zmqg_forward_result *fwd;                      /* n_streams */
} zmqg_forward_zmtp;
int zmqg_forward_zmtp_multi(zmqg_ctx *ctx, const zmqg_forward_zmtp *args, void *stream);

/* zmqg_forward_zmtp_sub_multi: zmqg_forward_zmtp_multi for an XSUB/XPUB proxy --
 * every forwarded message goes only to the routes whose destination is
 * subscribed to it, what xpub_t::xsend decides for the first part of each
 * message (src/xpub.cpp:290-326: generic_mtrie_t::match, src/
 * generic_mtrie_impl.hpp:523-561, marking pipes through dist_t::match, src/
 * dist.cpp:49-62, then dist_t::send_to_matching).  The subscriptions are a flat
 * table on the device, by destination; the decision is made there between the
 * decode and the encode, from the plaintext the decode has left in `plain`.
 *
 * Base behaviour.  Everything zmqg_forward_zmtp_multi states holds -- the
 * receive side, Q(s), F, E, fwd[s], the carry, the pair numbering and N, the
 * send side as zmqg_encode_zmtp_multi over the pairs, fit and ENOBUFS, nonces
 * in pair order, the -EINVAL cases -- with one change: which pairs are live.
 * fwd[s] is unchanged: `forwarded` counts what the rule lets through, whatever
 * matches.
 *
 * Messages.  The data elements of stream s are the non-command elements of Q(s)
 * below held_first, in order.  The first one is a head, and so is every data
 * element whose predecessor among them has ZMQG_MSG_MORE clear; commands in
 * between change nothing.  The topic of a message is its head's whole payload:
 * plain[carry_off .. +carry_len) of a carried head, plain[plain_off[slot] ..
 * +frame_len[slot] - 33) of a returned frame.  A head carried from an earlier
 * call is matched in the call that forwards its message, against that call's
 * table (the verdict is taken when the first part is sent, and _more_send keeps
 * it for the later parts, src/xpub.cpp:295); later parts are never looked at.
 *
 * Match.  Destination t's subscriptions are the prefixes j in [sub_idx[t],
 * sub_idx[t + 1]), prefix j = sub_bytes[sub_off[j] .. +sub_len[j]).  t matches
 * a topic when some such j has sub_len[j] <= the topic's length and its bytes
 * equal to the topic's first sub_len[j] bytes (generic_mtrie_t::match walks the
 * topic down the trie and reports the pipes of every node it passes).  The
 * empty prefix matches every topic, the empty one included.  With
 * ZMQG_SUBS_INVERT the verdict is negated (options.invert_matching,
 * src/xpub.cpp:308-310, dist_t::reverse_match, src/dist.cpp:64-78): a
 * destination without subscriptions then matches everything.  Two matching
 * subscriptions of one destination give one copy (dist_t::match marks a pipe
 * once, src/dist.cpp:51-53); a stream that routes one destination twice still
 * gives it two.
 *
 * Live pairs.  Pair (element q, route k) of stream s is live when q is forwarded
 * and destination route_dst[route_idx[s] + k] matches the topic of q's message.
 * A pair that is not live is treated exactly as in zmqg_forward_zmtp_multi: it
 * names no stream, gets pair_status ZMQG_ERR_SESSION and pair_off UINT64_MAX,
 * takes no nonce and occupies no byte of `out`.  match_out[p] (N entries, or
 * NULL) is 1 for a live pair, else 0: it tells "filtered" from "invalid
 * session".
 *
 * The table.  All five arrays and match_out are device-accessible, none is a
 * HOST array: the table lives on the device across calls, the caller updates it
 * in stream order when a subscription changes (the SUBSCRIBE / CANCEL commands
 * reach the host as held commands), and the call copies nothing of it.  The
 * host cannot validate it, so the device bounds every read: sub_idx entries
 * above n_subs are clamped to it, a falling pair of sub_idx entries is an empty
 * range, a subscription with sub_off + sub_len > sub_bytes_len never matches
 * and no byte of it is read; no byte outside sub_bytes[0 .. sub_bytes_len) or
 * outside the topic is read.
 *
 * Returns -EINVAL for a null subs, subs->size != sizeof(zmqg_forward_subs),
 * flag bits other than ZMQG_SUBS_INVERT, n_subs > 2^31 - 1, with n_dst > 0 a
 * null sub_idx, with n_subs > 0 a null sub_off or sub_len, a null sub_bytes
 * with sub_bytes_len > 0, and every case of zmqg_forward_zmtp_multi; nothing is
 * queued then.
 * Launches: zmqg_forward_zmtp_multi's and two more, whatever the sizes are (one
 * wave per source stream for the heads; one wave per element for the match,
 * the waves of heads walking their routes with a subscription a lane).  With
 * N == 0 the two are not queued.
 * Not offered: ROUTER identities (zmqg_forward_zmtp_router_multi, which does not
 * combine with this table); load balancing (zmqg_forward_zmtp_lb_multi, which
 * does not either); maintaining the table on the device from
 * SUBSCRIBE / CANCEL commands (they stay held commands for the host;
 * zmqg_subs_update_multi, a call of its own, keeps such a table);
 * ZMQ_XPUB_MANUAL, ZMQ_XPUB_NODROP, the welcome message; high-water marks here
 * (a subscriber's HWM is zmqg_forward_credit_multi with ZMQG_FWD_SUB);
 * the XSUB upstream direction; WebSocket framing here (it is
 * zmqg_forward_framed_multi with ZMQG_FWD_SUB). */
#define ZMQG_SUBS_INVERT 1u            /* options.invert_matching: dist_t::reverse_match, src/dist.cpp:64-78 */
typedef struct zmqg_forward_subs {
    uint32_t size, flags;              /* sizeof(zmqg_forward_subs); 0 or ZMQG_SUBS_INVERT */
    uint64_t n_subs;                   /* entries of sub_off / sub_len (<= 2^31 - 1) */
    const uint32_t *sub_idx;           /* args->n_dst + 1: destination t owns subscriptions sub_idx[t] .. sub_idx[t+1] */
    const uint64_t *sub_off;           /* prefix j = sub_bytes[sub_off[j] .. +sub_len[j]) */
    const uint32_t *sub_len;
    const uint8_t *sub_bytes;
    uint64_t sub_bytes_len;            /* extent of sub_bytes */
    uint8_t *match_out;                /* N entries, or NULL */
} zmqg_forward_subs;
int zmqg_forward_zmtp_sub_multi(zmqg_ctx *ctx, const zmqg_forward_zmtp *args,
                                const zmqg_forward_subs *subs, void *stream);

/* zmqg_subs_update_multi: the subscription direction of an XSUB/XPUB proxy --
 * the SUBSCRIBE / CANCEL traffic that zmqg_decode_zmtp_multi (or a forward
 * call's receive side) has decoded from the subscribers' connections, applied
 * to a subscription store that lives on the device, published as the table
 * zmqg_forward_zmtp_sub_multi reads, and judged for what must be passed
 * upstream: xpub_t::xread_activated (src/xpub.cpp:72-170) with
 * generic_mtrie_t::add / rm (src/generic_mtrie_impl.hpp:41-126, 376-521), and
 * xpub_t::xpipe_terminated (src/xpub.cpp:253-277) for peers that have gone.
 * The call is asynchronous on `stream`; the host neither synchronises nor reads
 * the store back.  Every array is device-accessible unless marked HOST; the two
 * HOST arrays are copied before the call returns.
 *
 * The store.  Caller-owned device memory, all zero = empty, written by this
 * call only: cnt[n_dst], slot_len[n_dst * cap], bytes[n_dst * cap * slot_bytes]
 * (8-byte aligned).  Destination t's live prefixes are its slots t * cap + i,
 * i < cnt[t]: prefix = bytes[(t * cap + i) * slot_bytes .. +slot_len[t * cap +
 * i]).  Their order within a destination is unspecified (a removal moves the
 * destination's last slot into the hole); nothing observable depends on it.
 * The device never trusts the store: cnt[t] is read as min(cnt[t], cap),
 * slot_len as min(slot_len, slot_bytes), and no byte outside the three arrays is
 * read or written.  A store that only this call has written holds no prefix
 * twice in one destination; for any other, "the destinations holding a topic"
 * below counts slots, and a cancel removes the first slot that holds the topic.
 * cnt[t] is written (clamped) for the destinations named in stream_dst and
 * clear_dst, the others' entries are left as they are.
 *
 * The view.  sub_idx[n_dst + 1], sub_off[n_dst * cap], sub_len[n_dst * cap] are
 * outputs: zmqg_forward_subs's arrays.  After the call sub_idx is the exclusive
 * sum of the new counts, entry sub_idx[t] + i names slot t * cap + i -- sub_off
 * (t * cap + i) * slot_bytes, sub_len the slot's length -- and entries at or
 * past sub_idx[n_dst] are left as they were.  The forward call takes sub_bytes =
 * bytes, sub_bytes_len = n_dst * cap * slot_bytes, n_subs = n_dst * cap.
 *
 * The input.  n_streams, max_frames, results, frame_len, plain_off, flags_out,
 * status_out, plain are the outputs of a zmqg_decode_zmtp_multi call queued
 * earlier on the same stream, with its slot numbering s * max_frames + j.
 * stream_dst (HOST, n_streams entries): stream s edits destination
 * stream_dst[s].  The elements of stream s are its slots j < min(results[s].
 * frames, max_frames) in order, up to but not including the first one with a
 * non-zero status (the connection fails there: nothing from that frame on is
 * examined).
 *
 * Classification.  An element's payload p is the frame_len - 33 bytes at
 * plain[plain_off]; what the engine and XPUB make of it
 * (zmtp_engine_t::process_command_message, src/zmtp_engine.cpp:533-563, whose
 * result is ignored at src/stream_engine_base.cpp:635-637;
 * session_base_t::push_msg, src/session_base.cpp:158-172; msg_t::command_body,
 * src/msg.cpp:526-559; src/xpub.cpp:88-100):
 *   ZMQG_MSG_COMMAND set:  len >= 10 and p starts with "\x09SUBSCRIBE": a
 *     subscribe, topic p[10..); len >= 7 and p starts with "\x06CANCEL": a
 *     cancel, topic p[7..); anything else (PING, PONG, other commands, len 0, a
 *     name length byte above len - 1) is no subscription element: the session
 *     drops it or the host handles it, it is never an error.
 *   ZMQG_MSG_COMMAND clear:  len >= 1 and p[0] 1 / 0: a subscribe / cancel,
 *     topic p[1..) (what a downgrade_sub peer sends); anything else is an XPUB
 *     user message, the host's to deal with, and no subscription element.
 *   ZMQG_MSG_MORE is ignored (ZMQ_ONLY_FIRST_SUBSCRIBE off).
 *
 * Apply.  Each stream's subscription elements are applied to its destination
 * in order; sub_status says what became of each:
 *   ZMQG_SUB_NONE       no subscription element
 *   ZMQG_SUB_ADDED      subscribe, stored
 *   ZMQG_SUB_DUPLICATE  subscribe, the destination already holds exactly these bytes
 *   ZMQG_SUB_REMOVED    cancel, removed
 *   ZMQG_SUB_NOT_FOUND  cancel, the destination does not hold it (also a topic
 *                       longer than slot_bytes)
 *   ZMQG_SUB_FULL       subscribe, cnt == cap
 *   ZMQG_SUB_TOO_LONG   subscribe, topic longer than slot_bytes
 * FULL and TOO_LONG change nothing: they are the host's signal to deal with
 * that subscriber.  The empty topic is an ordinary prefix.
 *
 * Clear.  clear_dst (HOST, n_clear entries) names destinations whose peer has
 * gone.  Every prefix such a destination t holds is removed and cnt[t] becomes
 * 0; for each former slot i < cnt_before: clear_len[t * cap + i] = its length,
 * clear_note[t * cap + i] = its upstream verdict (0 / 1), and the prefix bytes
 * and slot_len stay in the store until a later call reuses the slot.
 * clear_cnt[k] = cnt_before of clear_dst[k].  Every other entry of clear_len
 * and clear_note is left as it was.
 *
 * Upstream.  The order of events is the one of a replay: the clears in
 * clear_dst order (a destination's slots in slot order), then the elements in
 * (stream, slot) order.  With H = the destinations holding the topic just
 * before an event in that order:
 *   an ADDED notifies when H == 0 (mtrie add's first_added);
 *   a REMOVED or cleared prefix notifies when H == 1 (last_value_removed);
 *   a NOT_FOUND cancel notifies -- the reference's rule is rm_result !=
 *     values_remain (src/xpub.cpp:118-122), which lets not_found through, and
 *     that is kept;
 *   DUPLICATE, FULL, TOO_LONG and NONE do not notify.
 * ZMQG_SUBS_VERBOSE: every ADDED and DUPLICATE notifies (ZMQ_XPUB_VERBOSE).
 * ZMQG_SUBS_VERBOSER: that, and every cancel and every cleared prefix
 * (ZMQ_XPUB_VERBOSER).
 *
 * Per-slot outputs, n_streams * max_frames entries each, all written:
 * sub_status; topic_off, an absolute offset into `plain`, and topic_len;
 * note_flags, ZMQG_MSG_SUBSCRIBE or ZMQG_MSG_CANCEL for any subscription
 * element; note_stream, 0 when the slot notifies, else UINT32_MAX.  A NONE slot
 * gets 0 / 0 / 0 / 0 / UINT32_MAX.  topic_off, topic_len, note_flags and
 * note_stream are zmqg_encode_zmtp_multi's in_off, len, flags and frame_stream
 * with in = plain and one stream, the upstream session: one more queued call
 * sends the notifications upstream, no read-back.  results_out[s]: seen (the
 * stream's subscription elements), changed (ADDED + REMOVED), notes, rejected
 * (FULL + TOO_LONG).
 *
 * Returns -EINVAL for a null ctx or args, args->size != sizeof(zmqg_subs_update),
 * flag bits other than the two above, n_dst > 8192, cap == 0, slot_bytes no
 * multiple of 8 or outside 8 .. 65536, n_dst * cap > 2^31 - 1, n_streams,
 * max_frames or n_streams * max_frames > 2^31 - 1, a null sub_idx; with n_dst >
 * 0 a null cnt, slot_len, bytes, sub_off or sub_len or a misaligned bytes; with
 * n_streams > 0 a null stream_dst, results or results_out; with n_streams *
 * max_frames > 0 a null input or per-slot array; with n_clear > 0 a null
 * clear_dst, clear_cnt, clear_len or clear_note; entries of stream_dst or
 * clear_dst that are not distinct or not below n_dst, or a destination named
 * in both.  Nothing is queued then.  With n_streams == 0 and n_clear == 0 only
 * the view is republished; max_frames == 0 is valid.
 * Launches: five kernels and one copy whatever the sizes are (classify; the
 * holders of every topic at call start; apply; the verdicts; the view); a
 * kernel with nothing to do is not queued.  The verdicts compare every event
 * with the events before it: the call is off the per-message path.
 * Not offered: ZMQ_XPUB_MANUAL, ZMQ_ONLY_FIRST_SUBSCRIBE, the welcome message,
 * fan-out of the notifications to several upstreams (one encode call per
 * upstream), growing a store in place. */
#define ZMQG_SUB_NONE 0
#define ZMQG_SUB_ADDED 1
#define ZMQG_SUB_DUPLICATE 2
#define ZMQG_SUB_REMOVED 3
#define ZMQG_SUB_NOT_FOUND 4
#define ZMQG_SUB_FULL 5
#define ZMQG_SUB_TOO_LONG 6
#define ZMQG_SUBS_VERBOSE 2u           /* ZMQ_XPUB_VERBOSE: _verbose_subs, src/xpub.cpp:189-191 */
#define ZMQG_SUBS_VERBOSER 4u          /* ZMQ_XPUB_VERBOSER: and _verbose_unsubs, src/xpub.cpp:192-194 */
#define ZMQG_SUBS_MAX_DST 8192u
typedef struct zmqg_subs_result {
    uint64_t seen;                     /* subscription elements of the stream */
    uint64_t changed;                  /* ADDED + REMOVED */
    uint64_t notes;                    /* slots that notify */
    uint64_t rejected;                 /* FULL + TOO_LONG */
} zmqg_subs_result;
typedef struct zmqg_subs_update {
    uint32_t size, flags;              /* sizeof(zmqg_subs_update); ZMQG_SUBS_VERBOSE / _VERBOSER */
    uint64_t n_dst, cap, slot_bytes;   /* the store */
    uint32_t *cnt;
    uint32_t *slot_len;
    uint8_t *bytes;
    uint32_t *sub_idx;                 /* the view */
    uint64_t *sub_off;
    uint32_t *sub_len;
    uint64_t n_streams, max_frames;    /* the input: a zmqg_decode_zmtp_multi call's */
    const zmqg_zmtp_result *results;
    const uint32_t *frame_len;
    const uint64_t *plain_off;
    const uint8_t *flags_out;
    const int32_t *status_out;
    const uint8_t *plain;
    const uint32_t *stream_dst;        /* HOST, n_streams */
    uint64_t n_clear;                  /* destinations whose peer has gone */
    const uint32_t *clear_dst;         /* HOST, n_clear */
    uint32_t *clear_cnt;               /* n_clear */
    uint32_t *clear_len;               /* n_dst * cap */
    uint8_t *clear_note;               /* n_dst * cap */
    int32_t *sub_status;               /* per slot, n_streams * max_frames each */
    uint64_t *topic_off;
    uint32_t *topic_len;
    uint8_t *note_flags;
    uint32_t *note_stream;
    zmqg_subs_result *results_out;     /* n_streams */
} zmqg_subs_update;
int zmqg_subs_update_multi(zmqg_ctx *ctx, const zmqg_subs_update *args, void *stream);

/* zmqg_forward_zmtp_router_multi: zmqg_forward_zmtp_multi for a proxy with a
 * ROUTER side -- a request/reply broker, a worker pool.  What a ROUTER does to
 * messages is decided per message from the plaintext the decode has left in
 * `plain`:
 *   ZMQG_ROUTER_PREPEND  the receive side is a ROUTER (router_t::xrecv,
 *     src/router.cpp:263-332): every message gets the sending peer's routing id
 *     in front, as an extra first part with MORE set.
 *   ZMQG_ROUTER_ROUTE    the send side is a ROUTER (router_t::xsend,
 *     src/router.cpp:161-261): the first part of every message is an address; an
 *     address without MORE is a malformed message and is silently ignored
 *     (:168-171, :207-211); otherwise it is looked up among the peers' routing
 *     ids (lookup_out_pipe, src/socket_base.cpp:2187-2200: an exact match on the
 *     blob_t), it is never sent itself, and the remaining parts go to that peer,
 *     or are dropped when there is none (:221, :251-254, ZMQ_ROUTER_MANDATORY
 *     off).
 * flags == 0 is valid and is exactly zmqg_forward_zmtp_multi (no other field of
 * `router` is read, dest_out is not written).  `args` is that call's struct.
 *
 * Base behaviour.  Everything zmqg_forward_zmtp_multi states holds -- the
 * receive side, Q(s), F, E, fwd[s] (unchanged: `forwarded` counts what the rule
 * lets through), the carry, the send side as zmqg_encode_zmtp_multi over the
 * pairs, fit and ENOBUFS, nonces in pair order, the -EINVAL cases -- with two
 * changes: the pair space, and which pairs are live.  Data elements, heads and
 * messages are defined as in zmqg_forward_zmtp_sub_multi; every message below
 * held_first is complete.
 *
 * Outgoing message.  A message's data parts; with PREPEND the part {flags MORE,
 * payload id(s)} in front of them, id(s) = plain[src_id_off[s] ..
 * +src_id_len[s]): the source ids live in `plain`, where the encode reads every
 * other payload, in a region the host owns (with plain == in the gaps between
 * streams will do: nothing outside a stream is parsed).  src_id_off / src_id_len
 * are trusted as carry_off / carry_len are.
 * Without ROUTE every part of the outgoing message goes to every route of its
 * stream.  With ROUTE route_idx and route_dst are not read and may be NULL, and
 * every stream has one route slot: the address is the first part of the outgoing
 * message -- the head's payload, or id(s) with PREPEND also set (a ROUTER to
 * ROUTER proxy).  An address part with MORE clear (possible only without
 * PREPEND) makes the message malformed: it is dropped.  Otherwise the
 * destination t is the lookup of the address bytes; the remaining parts go to
 * t, or are dropped when the lookup finds nothing; the address part is never
 * sent.  A head carried from an earlier call is looked up in the call that
 * forwards its message, in that call's table.
 *
 * Lookup.  Defined for any table, since the host cannot validate one on the
 * device.  Entry j, id_bytes[id_off[j] .. +id_len[j]), is void when id_off[j] >
 * id_bytes_len or id_len[j] > id_bytes_len - id_off[j]: none of its bytes is
 * read, it orders as the empty id and never equals an address.  less(a, b) is
 * blob_t::operator< (src/blob.hpp:92): memcmp over the shorter length gives < 0,
 * or gives 0 and a is shorter.  Start with lo = 0, hi = n_ids; while lo < hi,
 * mid = lo + (hi - lo) / 2, and less(entry[mid], address) ? lo = mid + 1 : hi =
 * mid.  The address is found when lo < n_ids, entry[lo] is not void and has the
 * address's length and bytes, and id_dst[lo] < n_dst.  On a table sorted by less
 * with distinct ids that is std::map::find's answer; two ids may name one
 * destination.  No byte outside id_bytes[0 .. id_bytes_len) and no byte outside
 * the address is read.  The table lives on the device across calls (none of its
 * arrays is a HOST array, the call copies nothing of it); the caller updates it
 * in stream order when a peer connects or leaves.
 *
 * Pair space.  m = 2 with PREPEND set and ROUTE clear, else 1; d'(s) = 1 with
 * ROUTE, else d(s).  Stream s, slot and route k form pair p = base(s) + slot *
 * d'(s) + k, base(s) = the sum over t < s of m * (c(t) + max_frames) * d'(t).
 * With m = 1 slot q is element q; with m = 2 slot 2q + 1 is element q and slot
 * 2q the id part in front of it.  N = base(n_streams) <= 2^31 - 1; pair_off has
 * N + 1 entries, pair_status and dest_out N.
 *
 * Live pairs.  An id slot is live when its element is a forwarded head: the
 * frame {MORE, in_off = src_id_off[s], len = src_id_len[s]} to route k, with a
 * nonce like any frame.  Without ROUTE an element slot is live when its element
 * is forwarded.  With ROUTE it is live when the element is forwarded, is not the
 * address part, its message is not malformed and the lookup of its message's
 * address was found; its destination is the one found.  A pair that is not live
 * is zmqg_forward_zmtp_multi's: no stream, pair_status ZMQG_ERR_SESSION,
 * pair_off UINT64_MAX, no nonce, no byte of `out`.
 * dest_out[p] (device-accessible, N entries, or NULL): a live pair's destination
 * index (also when that destination's session is invalid and the encode reports
 * ZMQG_ERR_SESSION); ZMQG_ROUTE_ADDRESS for a forwarded head consumed as an
 * address, ZMQG_ROUTE_MALFORMED for the head of a one-part message,
 * ZMQG_ROUTE_UNKNOWN for a forwarded non-address part whose lookup failed (what
 * a host that wants ZMQ_ROUTER_MANDATORY-style reporting reads),
 * ZMQG_ROUTE_NONE for everything else.  With ROUTE and PREPEND together there
 * is no slot for the address and no ADDRESS entry.
 *
 * Returns -EINVAL for a null router, size != sizeof(zmqg_forward_router), flag
 * bits other than the two; with PREPEND and n_streams > 0 a null src_id_off or
 * src_id_len; with ROUTE n_ids > 2^31 - 1, with n_ids > 0 a null id_off, id_len
 * or id_dst, a null id_bytes with id_bytes_len > 0; and every case of
 * zmqg_forward_zmtp_multi, the route_idx / route_dst cases skipped under ROUTE
 * and N computed as above (under ROUTE also N > 0 with n_dst == 0, the send
 * side's own case of frames without streams, which routes cannot reach);
 * nothing is queued then.
 * Launches: with PREPEND alone zmqg_forward_zmtp_multi's and one more (the
 * heads, one wave per source stream); with ROUTE two more (the heads; one wave
 * per element for the lookup, the waves of heads searching the table with the
 * lanes over the bytes of each compare).  With N == 0 the extra ones are not
 * queued.
 * Not offered: ZMQ_ROUTER_MANDATORY and its errors, ZMQ_ROUTER_HANDOVER,
 * ZMQ_ROUTER_RAW; maintaining the id table on the device; DEALER's round-robin
 * choice (lb_t), which is zmqg_forward_zmtp_lb_multi (with its own PREPEND for
 * a ROUTER frontend); high-water marks here (a full peer's drop is
 * zmqg_forward_credit_multi with ZMQG_FWD_ROUTER); WebSocket framing here (it is
 * zmqg_forward_framed_multi with ZMQG_FWD_ROUTER); combining with the
 * subscription table. */
#define ZMQG_ROUTER_PREPEND 1u   /* receive side is a ROUTER: router_t::xrecv */
#define ZMQG_ROUTER_ROUTE   2u   /* send side is a ROUTER: router_t::xsend */
#define ZMQG_ROUTE_NONE      0xffffffffu  /* slot not forwarded (held, command, past seq, unused id slot) */
#define ZMQG_ROUTE_ADDRESS   0xfffffffeu  /* the address part: consumed, never sent */
#define ZMQG_ROUTE_UNKNOWN   0xfffffffdu  /* part of a message whose address names no destination: dropped */
#define ZMQG_ROUTE_MALFORMED 0xfffffffcu  /* a one-part message on a ROUTE call: dropped */
typedef struct zmqg_forward_router {
    uint32_t size, flags;        /* sizeof(zmqg_forward_router); PREPEND | ROUTE (0 = zmqg_forward_zmtp_multi) */
    const uint64_t *src_id_off;  /* PREPEND: n_streams; stream s's id = plain[src_id_off[s] .. +src_id_len[s]) */
    const uint32_t *src_id_len;  /* PREPEND: n_streams (any length, 0 included) */
    uint64_t n_ids;              /* ROUTE: entries of the id table (<= 2^31 - 1) */
    const uint64_t *id_off;      /* id j = id_bytes[id_off[j] .. +id_len[j]) */
    const uint32_t *id_len;
    const uint32_t *id_dst;      /* the destination (index into dst_sid) id j names */
    const uint8_t *id_bytes;
    uint64_t id_bytes_len;       /* extent of id_bytes */
    uint32_t *dest_out;          /* N entries, or NULL */
} zmqg_forward_router;
int zmqg_forward_zmtp_router_multi(zmqg_ctx *ctx, const zmqg_forward_zmtp *args,
                                   const zmqg_forward_router *router, void *stream);

/* zmqg_forward_zmtp_lb_multi: zmqg_forward_zmtp_multi for a proxy whose send
 * side is a DEALER or a PUSH socket -- the backend of a request/reply broker, a
 * streamer.  Such a socket sends through lb_t (dealer_t::sendpipe,
 * src/dealer.cpp:110-113, push_t::xsend, src/push.cpp:45-48): every whole
 * message goes to the next active pipe in turn (lb_t::sendpipe,
 * src/lb.cpp:56-131).  The turn is taken per message, which route_dst -- per
 * source stream and per call -- cannot express: the host does not know how many
 * messages a receive buffer holds until the decode has run.  Here the choice is
 * made on the device between the decode and the encode, and the cursor stays
 * there between calls.  With ZMQG_LB_PREPEND the receive side is a ROUTER, as
 * under ZMQG_ROUTER_PREPEND: a ROUTER/DEALER broker is this call one way and
 * zmqg_forward_zmtp_router_multi with ROUTE the other.  `args` is
 * zmqg_forward_zmtp_multi's struct.
 *
 * Base behaviour.  Everything zmqg_forward_zmtp_multi states holds -- the
 * receive side, Q(s), F, E, fwd[s] (unchanged: `forwarded` counts what the rule
 * lets through), the carry, the send side as zmqg_encode_zmtp_multi over the
 * pairs, fit and ENOBUFS, nonces in pair order -- with two changes: the pair
 * space, and which pairs are live.  Data elements, heads and messages are
 * defined as in zmqg_forward_zmtp_sub_multi; every message below held_first is
 * complete, and there is one message per forwarded head.
 *
 * Pair space.  route_idx and route_dst are not read and may be NULL; every
 * stream has one route slot, as under ZMQG_ROUTER_ROUTE.  m = 2 with PREPEND,
 * else 1.  Stream s owns m * (c(s) + max_frames) pairs, base(s) is the running
 * sum, p = base(s) + slot.  With m = 1 slot q is element q; with m = 2 slot
 * 2q + 1 is element q and slot 2q the id part in front of it, {flags MORE,
 * payload plain[src_id_off[s] .. +src_id_len[s])} (zmqg_forward_zmtp_router_
 * multi's layout with d' = 1, and its rules for the ids).  N = base(n_streams)
 * <= 2^31 - 1; pair_off has N + 1 entries, pair_status and dest_out N.
 *
 * The table.  A group is one load balancer: one DEALER or PUSH socket the
 * thread serves.  stream_group[s] (a HOST array) names the group that
 * distributes stream s's messages, or ZMQG_LB_NO_GROUP.  Group g's active
 * destinations are lb_dst[grp_idx[g] .. grp_idx[g + 1]), indices into dst_sid:
 * lb_t's _pipes[0 .. _active), in its order.  lb_cur[g] is lb_t's _current.
 * grp_idx, lb_dst and lb_cur live on the device across calls; they are not HOST
 * arrays and the call copies nothing of them.  The host rewrites the table in
 * stream order when a worker connects, leaves or stops being writable.  The
 * device trusts none of it: grp_idx entries above n_lb are clamped to n_lb, a
 * falling pair of grp_idx entries is an empty range; A(g) is the size of group
 * g's range, cur0(g) = lb_cur[g] mod A(g), or 0 when A(g) = 0; no element
 * outside grp_idx[0 .. n_groups], lb_dst[0 .. n_lb) and lb_cur[0 .. n_groups)
 * is read or written.
 *
 * Choice.  The messages of group g are the forwarded messages of the streams
 * with stream_group[s] == g, by rising stream and, within a stream, by rising
 * element: the order in which zmqg_forward_zmtp_multi lays messages into a
 * destination's run.  The i-th message of the group (from 0) goes to entry
 * lb_dst[grp_idx[g] + (cur0 + i) mod A] (grp_idx[g] clamped), all its parts and
 * with PREPEND its id part.  After the call lb_cur[g] = (cur0 + M(g)) mod A, M(g)
 * the group's messages in this call, or 0 when A = 0.  lb_cur is written for
 * every group, clamped, whether or not the group had streams.  That is
 * lb_t::sendpipe with every write succeeding: _pipes[_current] takes the
 * message, and ++_current wraps at _active after its last part
 * (src/lb.cpp:118-124); _more and _dropping never carry over between calls,
 * because only whole messages are forwarded.  Order: the reference's fq_t hands
 * lb_t the sources' messages interleaved by arrival (fq_t::recvpipe,
 * src/fq.cpp:52-94); stream-major order is one such arrival order, fixed here
 * so that the call is deterministic.
 *
 * Live pairs.  An element slot is live when its element is forwarded, its
 * stream has a group, A(g) > 0 and the chosen entry's value t is below n_dst;
 * its destination is t.  An id slot is live when its element is a forwarded
 * head, under the same conditions.  A message whose entry names no destination
 * (t >= n_dst) still takes its turn: the cursor moves past it.  A pair that is
 * not live is zmqg_forward_zmtp_multi's: no stream, pair_status
 * ZMQG_ERR_SESSION, pair_off UINT64_MAX, no nonce, no byte of `out`.
 * dest_out[p] (device-accessible, N entries, or NULL): t for a live pair (also
 * when t's session is invalid and the encode reports ZMQG_ERR_SESSION);
 * ZMQG_LB_NO_PEER for every slot of a forwarded element, or of the id in front
 * of a forwarded head, that is not live -- the host re-offers those messages as
 * carries in a later call: they are whole and still in `plain`; ZMQG_LB_NONE
 * for everything else.
 *
 * Returns -EINVAL for a null lb, size != sizeof(zmqg_forward_lb), flag bits
 * other than ZMQG_LB_PREPEND; with PREPEND and n_streams > 0 a null src_id_off
 * or src_id_len; n_groups or n_lb above 2^31 - 1; with n_groups > 0 a null
 * grp_idx or lb_cur; a null lb_dst with n_lb > 0; with n_streams > 0 a null
 * stream_group or an entry that is neither below n_groups nor
 * ZMQG_LB_NO_GROUP; N > 0 with n_dst == 0; and every case of
 * zmqg_forward_zmtp_multi, the route_idx / route_dst cases skipped and N
 * computed as above; nothing is queued then.  With n_streams == 0 nothing is
 * done and lb_cur is left alone.
 * Launches: zmqg_forward_zmtp_multi's and two more, whatever the sizes are
 * (one wave per source stream for the heads and, in the same pass, the
 * messages' ranks; one wave per group for the streams' ring positions and the
 * cursors); the pairs launch is this call's own.  With N == 0 the heads and the
 * pairs are not queued, and the groups' launch, which then only clamps lb_cur,
 * is queued when n_groups > 0.
 * Not offered: high-water marks and lb_t's deactivation of a full pipe
 * (src/lb.cpp:103-107): the host keeps a pipe that is not writable out of
 * lb_dst (zmqg_forward_credit_multi, which drops for a full destination in the
 * other modes, refuses this one: lb_t skips a full pipe, it does not drop;
 * zmqg_forward_lb_credit_multi is this call with that skip made on the
 * device); the exact turn after a membership change (the host edits the range
 * without reading the cursor, the device clamps it); WebSocket framing here
 * (it is zmqg_forward_framed_multi with ZMQG_FWD_LB); combining with the
 * subscription or the id table. */
#define ZMQG_LB_PREPEND  1u           /* receive side is a ROUTER: as ZMQG_ROUTER_PREPEND */
#define ZMQG_LB_NO_GROUP 0xffffffffu  /* stream_group[s]: this stream's messages are not distributed */
#define ZMQG_LB_NONE     0xffffffffu  /* dest_out: slot not forwarded (held, command, past seq, unused id slot) */
#define ZMQG_LB_NO_PEER  0xfffffffdu  /* dest_out: part of a forwarded message that found no destination */
typedef struct zmqg_forward_lb {      /* 80 bytes */
    uint32_t size, flags;             /* sizeof(zmqg_forward_lb); 0 or ZMQG_LB_PREPEND */
    const uint64_t *src_id_off;       /* PREPEND: n_streams, as zmqg_forward_router's */
    const uint32_t *src_id_len;
    uint64_t n_groups;                /* load balancers (one per DEALER / PUSH socket the thread serves) */
    const uint32_t *stream_group;     /* HOST, n_streams: < n_groups, or ZMQG_LB_NO_GROUP */
    const uint32_t *grp_idx;          /* device, n_groups + 1: group g's active destinations are lb_dst[grp_idx[g] .. grp_idx[g+1]) */
    uint64_t n_lb;                    /* entries of lb_dst (<= 2^31 - 1) */
    const uint32_t *lb_dst;           /* device: indices into dst_sid, lb_t's _pipes[0 .. _active) per group */
    uint32_t *lb_cur;                 /* device, n_groups: lb_t's _current, read and written by the call */
    uint32_t *dest_out;               /* device, N entries, or NULL */
} zmqg_forward_lb;
int zmqg_forward_zmtp_lb_multi(zmqg_ctx *ctx, const zmqg_forward_zmtp *args,
                               const zmqg_forward_lb *lb, void *stream);

/* WebSocket framing (ZWS 2.0 over RFC 6455): the reference's second caller of
 * the mechanism, ws_engine_t::decode_and_push (src/ws_engine.cpp:887-915),
 * whose frames come from ws_decoder_t / ws_encoder_t (src/ws_engine.cpp:
 * 221-250) in place of the ZMTP ones.
 *
 * zmqg_decode_ws_multi: zmqg_decode_zmtp_multi with ws_decoder_t's framing
 * (src/ws_decoder.cpp:39-249).  Everything zmqg_decode_zmtp_multi states about
 * streams, slots and their order of replay, two streams on one session,
 * stream_sid[s] >= max_sessions, empty slots, n_streams == 0, max_frames == 0,
 * the -EINVAL cases, asynchrony, alignment, isolation of the streams and
 * `out` == `in` holds here.  The framing, from offset 0 of each stream, in the
 * decoder's own order over the bytes that are present -- a check whose
 * deciding bytes are all in the stream is made; the first one whose bytes are
 * not leaves the frame for the next call, consumed staying at the frame's
 * first byte (a lone last byte 0x02 is an error, a lone 0x82 is incomplete):
 *   1. byte 0: FIN (0x80) set and the opcode (low 4 bits) 2 binary, 8 close,
 *      9 ping or 10 pong, else error = EPROTO (:41-63); RSV bits are ignored.
 *   2. byte 1: the MASK bit equals must_mask (the decoder's !_client: a
 *      server's receive side is masked), else EPROTO (:72-75); the low 7 bits
 *      are the size, or 126: two bytes big endian follow, or 127: eight bytes
 *      (:77-128); non-minimal forms are accepted as the reference accepts them.
 *   3. with must_mask, the 4-byte masking key (:131-144).
 *   4. a binary frame: size 0 gives EPROTO (:83-84, :104-105, :122-123,
 *      :136-137); then one flags byte (XORed with key byte 0), bit 1 = msg_t
 *      MORE, bit 2 = COMMAND (:146-163, src/ws_protocol.hpp:23-27); the size
 *      drops by one.
 *   5. with max_msg_size >= 0 a size above it gives EMSGSIZE (:166-173; for a
 *      binary frame the size after step 4); so does a size above 2^32 - 1 (this
 *      library's restriction, as on the ZMTP calls).
 *   6. `size` body bytes; with must_mask body byte i of a binary frame is
 *      XORed with key[(i + 1) % 4], of a control frame with key[i % 4]
 *      (:234-243).
 * EPROTO is this library's choice (the reference's decoder returns -1 there
 * and sets no errno).  An error ends the stream's parse: the frames before it
 * are returned and consumed ends at the failing frame's first byte.
 * A binary frame takes the next slot of its stream: frame_in_off = out_off =
 * the absolute offset of its body (the byte behind the flags byte), frame_len
 * the body size; the unmasked body is decoded as curve_mechanism_base_t::decode
 * would (src/ws_engine.cpp:895), flags_out / status_out as for
 * zmqg_decode_batch with the frame's MORE / COMMAND bits ORed into flags_out,
 * the payload at the body's start.  A binary frame that is not a MESSAGE
 * command (shorter than 8 bytes, or not starting with "\x07MESSAGE" once
 * unmasked) is returned as its stream's last frame with the mechanism's
 * status.  A close, ping or pong frame takes no slot and is not given to the
 * mechanism (src/ws_engine.cpp:891-894): it ends the stream's parse, consumed
 * includes it, and results[s].ctl_opcode / ctl_off / ctl_len describe its
 * payload, which is written unmasked at out[ctl_off ..), ctl_off being its
 * absolute offset in `in`; the host answers it and submits the rest of the
 * buffer with its next call.  A stream that has max_frames frames stops before
 * the next frame, whatever that is.
 * With `out` != `in`, `in` is never written, and in `out` only the bytes of
 * returned frames' bodies and of a control payload are (within a body, the
 * bytes behind the payload are unspecified).  With `out` == `in` masked bodies
 * are unmasked and then decoded in place; header, key and flags bytes are
 * never rewritten.  As for zmqg_decode_batch, a payload region holds
 * unauthenticated plaintext until the stream reaches the end of the call.
 * Two launches more than zmqg_decode_batch_ex with must_mask (the parse, then
 * the unmask over every returned body), one without (two when a control
 * payload has to be copied to an `out` that is not `in`).
 * ZMQG_OPT_VERIFY_FIRST / _REPLAY_HOST / _STREAM_OUT are not offered. */
typedef struct zmqg_ws_result {
    uint64_t frames;     /* binary frames returned in the stream's slots */
    uint64_t consumed;   /* bytes of the stream parsed (a control frame that ended the parse included) */
    uint64_t out_bytes;  /* payload bytes of the returned frames */
    int32_t error;       /* 0, EPROTO, EMSGSIZE */
    int32_t ctl_opcode;  /* 0, or 8 / 9 / 10: a close / ping / pong frame ended the parse */
    uint64_t ctl_off;    /* its payload, unmasked: out[ctl_off .. +ctl_len), absolute offset */
    uint64_t ctl_len;
} zmqg_ws_result;        /* 48 bytes */
int zmqg_decode_ws_multi(zmqg_ctx *ctx, uint64_t n_streams, const uint32_t *stream_sid, const uint64_t *stream_off,
                         const uint32_t *stream_len, const uint8_t *in, int must_mask, int64_t max_msg_size,
                         uint64_t max_frames, uint64_t *frame_in_off, uint32_t *frame_len, uint64_t *out_off,
                         uint8_t *out, uint8_t *flags_out, int32_t *status_out, zmqg_ws_result *results,
                         void *stream);

/* zmqg_encode_ws_multi: zmqg_encode_zmtp_multi with ws_encoder_t's frame
 * (src/ws_encoder.cpp:26-126) around each MESSAGE command, a msg_t without
 * MORE / COMMAND / subscribe / cancel (src/curve_mechanism_base.cpp:166-177).
 * zmqg_encode_zmtp_multi's contract holds -- validity, layout, fit, nonces,
 * results, the untouched bytes, the -EINVAL cases -- with the frame format and
 * F replaced.  `mask` is NULL for the server side (_must_mask false), else n
 * device-accessible entries: frame i's key bytes k are BE32(mask[i]), as
 * put_uint32 (..., random) writes them (:64-69); the device has no random
 * source, the caller supplies what generate_random would return.  With W =
 * zmqg_wire_size(...) and size = W + 1 the frame is: 0x82; the MASK bit (0x80
 * with mask != NULL) ORed with the size (size <= 125), or with 126 and two
 * bytes big endian (size <= 0xFFFF), or with 127 and eight bytes; the four key
 * bytes when masked; the flags byte 0 ^ k[0]; the W bytes of the MESSAGE
 * command, byte j XORed with k[(j + 1) % 4] when masked.  F(i) = 2 + (0 | 2 |
 * 8) + (masked ? 4 : 0) + size.  results[s].out_off / out_bytes are the
 * peer's zmqg_decode_ws_multi stream_off / stream_len.  Five launches before
 * the encode's own (nine with device nonces), and with mask != NULL one behind
 * it: the XOR over the bodies of the fitting frames; a frame that does not fit
 * or is invalid stays untouched. */
int zmqg_encode_ws_multi(zmqg_ctx *ctx, uint64_t n_streams, const uint32_t *stream_sid, uint64_t n,
                         const uint32_t *frame_stream, const uint64_t *nonce, const uint8_t *flags,
                         const uint64_t *in_off, const uint32_t *len, const uint8_t *in, const uint32_t *mask,
                         uint8_t *out, uint64_t out_bytes, uint64_t *frame_off, int32_t *status_out,
                         zmqg_zmtp_send_result *results, void *stream);

/* zmqg_forward_framed_multi: the four forward calls with a framing chosen for
 * each side -- a proxy whose one side is ws_engine_t (src/ws_engine.cpp) and
 * whose other side is the ZMTP engine, or WebSocket on both: zmq_proxy's
 * forward (src/proxy.cpp:90-138) between ws_decoder_t (src/ws_decoder.cpp:
 * 39-249) and ws_encoder_t (src/ws_encoder.cpp:26-126).  The framing is
 * orthogonal to the routing rule: statuses, MORE / COMMAND bits, frame counts
 * and the payloads in `plain` come out of either decoder in the same slot
 * layout, and the plan reads nothing else.
 *
 * Relation to the existing calls.  `args` is zmqg_forward_zmtp_multi's struct.
 * framing->mode names the rule and framing->plan its struct:
 *   ZMQG_FWD_STATIC  zmqg_forward_zmtp_multi, plan == NULL
 *   ZMQG_FWD_SUB     zmqg_forward_zmtp_sub_multi, plan a zmqg_forward_subs
 *   ZMQG_FWD_ROUTER  zmqg_forward_zmtp_router_multi, plan a zmqg_forward_router
 *                    (flags == 0 is the static rule, as there)
 *   ZMQG_FWD_LB      zmqg_forward_zmtp_lb_multi, plan a zmqg_forward_lb
 * The contract is the one stated for the mode's own call, with two
 * substitutions and nothing else changed: zmqg_decode_ws_multi replaces
 * zmqg_decode_zmtp_multi on the receive side when recv is not ZMTP, and
 * zmqg_encode_ws_multi replaces zmqg_encode_zmtp_multi on the send side when
 * send is not ZMTP.  The sequence Q(s) with F, E and fwd[s], the carry, the
 * pair space and N of the mode, live pairs, match_out and dest_out, lb_cur, the
 * nonces in pair order, fit, ENOBUFS and the prefix property are the mode's.
 * With recv == send == ZMQG_FRAMING_ZMTP the call is the mode's own call, byte
 * for byte and nonce for nonce.
 *
 * Receive side, recv = ZMQG_FRAMING_WS or _WS_MASKED.  Every output is what
 * zmqg_decode_ws_multi writes with must_mask = (recv == ZMQG_FRAMING_WS_MASKED):
 * slots, statuses and flags with the frame's MORE / COMMAND bits from the
 * WebSocket flags byte, the payloads at the body's offset in plain, plain == in
 * with masked bodies unmasked and decoded in place, the peer nonces, EPROTO and
 * EMSGSIZE, a stream that ends at a control frame.  The results go to
 * framing->ws_results (n_streams entries); args->results is neither read nor
 * written and may be NULL.  A close / ping / pong frame ends its stream's parse
 * exactly as in zmqg_decode_ws_multi: the frames returned before it are in Q(s)
 * and are forwarded by the usual rule; the host answers it from ctl_opcode /
 * ctl_off / ctl_len and submits the rest of the buffer from `consumed` in its
 * next call; a message that is open reaches across the control frame through
 * the carry, like any other held part.  max_frames == 0 zero-fills ws_results.
 *
 * Send side, send = ZMQG_FRAMING_WS or _WS_MASKED.  Exactly
 * zmqg_encode_ws_multi over the N pairs; a pair's liveness, flags, offset and
 * length come from the plan as in the mode's call.  mask is NULL for
 * ZMQG_FRAMING_WS and framing->mask for _WS_MASKED: N device-accessible
 * entries indexed by pair index p, of which only those of live, fitting pairs
 * are read.  The host knows N before the call (from carry_idx, route_idx and
 * the mode) and fills N words from its random source, as for
 * zmqg_encode_ws_multi.  dst_results[t].out_off / out_bytes are the peer's
 * zmqg_decode_ws_multi stream_off / stream_len.
 *
 * Members a chosen framing does not use (ws_results, mask, args->results) are
 * neither read nor written.
 * Returns -EINVAL, with nothing queued, for a null framing, size !=
 * sizeof(zmqg_forward_framing), a non-zero reserved or reserved2, recv, send or
 * mode out of range, a non-NULL plan with ZMQG_FWD_STATIC and a NULL plan
 * otherwise, the plan struct's own size / flag cases as its call makes them,
 * recv != ZMTP with n_streams > 0 and a null ws_results, recv == ZMTP with a
 * null args->results, send == ZMQG_FRAMING_WS_MASKED with N > 0 and a null
 * mask, and every case of the mode's own call.
 * Launches: the sum of the parts.  The mode's own, and: a masked receive side
 * takes zmqg_decode_ws_multi's two launches more than a batch decode where
 * zmqg_decode_zmtp_multi takes one; an unmasked receive side one, and two
 * when a control payload has to be copied to a plain that is not in; a masked
 * send side the one XOR launch behind the encode.
 * Out of scope: a framing per stream or per destination within one call (an
 * XPUB bound to tcp:// and ws:// at once makes two calls); answering pings on
 * the device; ZMQG_OPT_* on this call. */
#define ZMQG_FRAMING_ZMTP      0u
#define ZMQG_FRAMING_WS        1u   /* WebSocket, unmasked: a server's send side, a client's receive side */
#define ZMQG_FRAMING_WS_MASKED 2u   /* WebSocket, masked: a server's receive side (must_mask), a client's send side */
#define ZMQG_FWD_STATIC 0u          /* zmqg_forward_zmtp_multi's rule; plan == NULL */
#define ZMQG_FWD_SUB    1u          /* plan: const zmqg_forward_subs * */
#define ZMQG_FWD_ROUTER 2u          /* plan: const zmqg_forward_router * */
#define ZMQG_FWD_LB     3u          /* plan: const zmqg_forward_lb * */
typedef struct zmqg_forward_framing {   /* 48 bytes */
    uint32_t size, reserved;        /* sizeof(zmqg_forward_framing), 0 */
    uint32_t recv, send;            /* ZMQG_FRAMING_* of the receive buffers / of the send runs */
    uint32_t mode, reserved2;       /* ZMQG_FWD_*, 0 */
    const void *plan;               /* the mode's struct */
    zmqg_ws_result *ws_results;     /* recv != ZMTP: n_streams entries, device-accessible */
    const uint32_t *mask;           /* send == WS_MASKED: N entries, device-accessible */
} zmqg_forward_framing;
int zmqg_forward_framed_multi(zmqg_ctx *ctx, const zmqg_forward_zmtp *args,
                              const zmqg_forward_framing *framing, void *stream);

/* zmqg_forward_credit_multi: zmqg_forward_framed_multi with a high-water mark
 * per destination -- what a PUB / XPUB socket does for a subscriber whose pipe
 * is full (it drops for that one and keeps serving the others) and a ROUTER
 * without ZMQ_ROUTER_MANDATORY for a full peer (it drops the message).
 *
 * The reference counts in whole messages, per pipe:
 *   pipe_t::check_hwm (src/pipe.cpp:535-541): full when _hwm > 0 and
 *     _msgs_written - _peers_msgs_read >= _hwm;
 *   pipe_t::check_write / write (src/pipe.cpp:207-234): _msgs_written rises on
 *     a part without MORE only, so a multipart message is refused at its first
 *     part or not at all;
 *   dist_t::write (src/dist.cpp:196-210, from send_to_matching, :127-142): a
 *     pipe that refuses a write leaves _matching, _active and _eligible; it
 *     gets none of the message's further parts and no later message until it
 *     is re-activated, and the other pipes still get the message;
 *   router_t::xsend (src/router.cpp:185-200): when the addressed pipe's
 *     check_write fails, _current_out is dropped and the rest of the message
 *     discarded.
 * The peer's read count does not change within a call, so over the messages of
 * one call this is: at most dst_credit[t] more whole messages for destination
 * t, everything after that dropped for t alone.  The credit is hwm -
 * (_msgs_written - _peers_msgs_read), 0 for a pipe that is not writable, and
 * ZMQG_CREDIT_UNLIMITED for hwm == 0.
 *
 * `args` and `framing` are zmqg_forward_framed_multi's and mean what they mean
 * there; the modes are ZMQG_FWD_STATIC, _SUB and _ROUTER, with either framing
 * on either side.  Everything that call states holds: the receive side, Q(s),
 * F, E, fwd[s], the carry, the mode's pair space and N, match_out / dest_out
 * (they keep describing the routing decision), fit, ENOBUFS, the prefix
 * property, the nonces in pair order.  One thing changes: which pairs are live.
 *
 * Deliveries.  A delivery is (source stream s, forwarded message, route slot
 * k) with at least one pair that is live under the mode's own rule; all its
 * live pairs have one destination t.  Its position is p0 = base(s) + slot0 *
 * d'(s) + k, slot0 the first slot of the outgoing message: the id slot in an
 * m = 2 pair space, else the head element's slot -- whether or not pair p0 is
 * itself live (under ZMQG_ROUTER_ROUTE alone it is the consumed address).
 *
 * Admission.  The deliveries of destination t are ordered by p0; the i-th
 * (from 0) is admitted iff i < dst_credit[t] as it stood when the call was
 * queued, and ZMQG_CREDIT_UNLIMITED admits all.  A stream that names t twice
 * makes two deliveries and takes two credits.  The count does not look at
 * dst_sid[t]: a destination with an invalid session still takes credits, and
 * its pairs report ZMQG_ERR_SESSION as before.
 *
 * Outputs.  Every pair of an admitted delivery is the mode's live pair,
 * unchanged.  Every live pair of a refused delivery becomes not live: it names
 * no stream, takes no nonce and writes no byte of `out`, its pair_off is
 * UINT64_MAX and its pair_status (when given) ZMQG_ERR_HWM, which tells an HWM
 * drop from the other pairs that are not live (ZMQG_ERR_SESSION).  A masked
 * send side does not read its mask entry.  The other destinations of the same
 * message are not affected.  For every t < n_dst, with D(t) the deliveries of
 * t in this call: dst_taken[t] = min(D(t), dst_credit[t]) (D(t) when
 * unlimited) and dst_dropped[t] = D(t) - dst_taken[t].  taken counts
 * admissions: a pair that then does not fit is ZMQG_ERR_BOUND and the host's
 * to send again, as before.  With ZMQG_CREDIT_CONSUME, dst_credit[t] :=
 * dst_credit[t] - dst_taken[t] (unlimited stays), written behind every read of
 * the old value; without the flag dst_credit is not written.  dst_credit lives
 * on the device across calls, like lb_cur: the host adds to it, in stream
 * order, when a peer's read count comes in.
 *
 * Identity.  With every credit ZMQG_CREDIT_UNLIMITED every output of the
 * framed call is what zmqg_forward_framed_multi produces on the same input,
 * byte for byte and nonce for nonce, and dst_dropped is all zero.
 *
 * Returns -EINVAL, with nothing queued, for a null credit, size !=
 * sizeof(zmqg_forward_credit), unknown flag bits, mode ZMQG_FWD_LB, n_dst > 0
 * with a null dst_credit, dst_taken or dst_dropped, and every case of
 * zmqg_forward_framed_multi.  With n_streams == 0 nothing is done; with N == 0
 * and n_dst > 0 dst_taken and dst_dropped are zero-filled on the stream and
 * dst_credit is not written.
 * Launches: zmqg_forward_framed_multi's, and seven whatever N and n_dst are --
 * the starts with their counts per tile of pairs, two column passes, the
 * ranks, the verdict on every pair and the totals in front of the send side,
 * ZMQG_ERR_HWM behind it (not queued without pair_status) -- and under
 * ZMQG_FWD_STATIC the heads, which that mode's plan does not need itself.
 * Not offered: ZMQG_FWD_LB -- lb_t skips a full pipe and swaps it out of the
 * ring (src/lb.cpp:103-107), so the message goes to the next pipe instead of
 * being dropped, and every later choice moves with it: a reordering that
 * depends on the data, where this call only clears pairs (the host keeps a
 * full pipe out of lb_dst, or calls zmqg_forward_lb_credit_multi, which makes
 * that choice on the device); ZMQ_XPUB_NODROP (src/xpub.cpp:314: one full pipe
 * refuses the message for all, a dependency across destinations);
 * ZMQ_ROUTER_MANDATORY's EAGAIN; the low-water mark and re-activation, which
 * are the host's (it refills dst_credit); limits counted in bytes. */
#define ZMQG_CREDIT_UNLIMITED 0xffffffffu
#define ZMQG_CREDIT_CONSUME 1u           /* write dst_credit[t] - dst_taken[t] back (UNLIMITED stays) */
typedef struct zmqg_forward_credit {     /* 32 bytes */
    uint32_t size, flags;                /* sizeof(zmqg_forward_credit); 0 or ZMQG_CREDIT_CONSUME */
    uint32_t *dst_credit;                /* device, n_dst: whole messages t may still take */
    uint32_t *dst_taken;                 /* device, n_dst, out: deliveries admitted */
    uint32_t *dst_dropped;               /* device, n_dst, out: deliveries refused */
} zmqg_forward_credit;
int zmqg_forward_credit_multi(zmqg_ctx *ctx, const zmqg_forward_zmtp *args,
                              const zmqg_forward_framing *framing,
                              const zmqg_forward_credit *credit, void *stream);

/* zmqg_forward_lb_credit_multi: zmqg_forward_framed_multi with ZMQG_FWD_LB
 * under per-destination high-water marks -- what a PUSH or a DEALER socket does
 * for a worker whose pipe is full.  lb_t does not drop (lb_t::sendpipe,
 * src/lb.cpp:56-131): when _pipes[_current] refuses the write
 * (pipe_t::check_write / check_hwm, src/pipe.cpp:207-220, src/pipe.cpp:535-541)
 * it takes the pipe out of the active range -- _active--, then the pipe at
 * _current and the one at _active change places, or _current = 0 when there is
 * nothing to swap (src/lb.cpp:103-107) -- and offers the message to the next
 * one.  PUSH/PULL pipelines and ROUTER/DEALER worker pools rely on that to keep
 * a slow worker from being overrun.  The host cannot prepare the ring for it:
 * how many messages a receive buffer holds is known after the decode only.
 *
 * `args` and `framing` are zmqg_forward_framed_multi's; framing->mode must be
 * ZMQG_FWD_LB and framing->plan a zmqg_forward_lb.  `credit` is
 * zmqg_forward_credit_multi's struct, unchanged.  Either framing on either side
 * and ZMQG_LB_PREPEND work as in the framed call.  Everything that call states
 * for ZMQG_FWD_LB holds: the receive side, Q(s), F, E, fwd[s], the carry, the
 * pair space with m = 1 or 2, N, the group table and its clamps, the order of a
 * group's messages (streams rising, elements rising), fit, ENOBUFS, the prefix
 * property, the nonces in pair order.  Two things change: the choice, and the
 * cursor after the call.
 *
 * State of group g when the call is queued.  The working ring R[0 .. A) is a
 * copy of lb_dst[lo .. lo + A0), lo and A0 the group's clamped range; the call
 * never writes lb_dst.  cur = cur0(g).  Ring position j has a working credit
 * w[j] = dst_credit[R[j]] as it stood when the call was queued.
 * ZMQG_CREDIT_UNLIMITED never runs out.  An entry that names no destination
 * (R[j] >= n_dst) never runs out either: it keeps taking its turn, as in
 * zmqg_forward_zmtp_lb_multi.
 *
 * Choice.  Per message, in the group's order:
 *     while A > 0:
 *         if w[cur] is unlimited or > 0:
 *             the message goes to R[cur]; a finite w[cur] drops by one
 *             if ++cur >= A: cur = 0
 *             break
 *         A -= 1                                   (src/lb.cpp:103-107)
 *         if cur < A: swap entries cur and A (R and w together)
 *         else:       cur = 0
 *     if no entry took it (A == 0): the message is refused
 * Admission is per whole message, at its head: _msgs_written rises on a part
 * without MORE only (pipe_t::write, src/pipe.cpp:222-234), so the later parts
 * of an admitted message always pass.  Only whole messages are forwarded, so
 * lb_t's _more / _dropping branch (src/lb.cpp:78-101), which discards the rest
 * of a message whose pipe went away between its parts, cannot arise.
 *
 * Outputs.  An admitted message has the LB call's live pairs, unchanged:
 * dest_out = t, the entry's value, and when t names no destination
 * ZMQG_LB_NO_PEER with pair_status ZMQG_ERR_SESSION as there.  A refused
 * message -- every entry of the ring was deactivated in this call -- has no live
 * pair: every slot of its elements, and the id slot in front of its head, names
 * no stream, takes no nonce, writes no byte of `out`, reads no mask entry; its
 * pair_off is UINT64_MAX, its dest_out ZMQG_LB_NO_PEER and its pair_status
 * (when given) ZMQG_ERR_HWM.  The message is whole in `plain`, and the host
 * re-offers it as a carry once a peer has read.  A stream without a group, and
 * a range that was empty from the start, report ZMQG_ERR_SESSION as in the LB
 * call.
 * lb_cur[g] after the call is the original ring position (the index into the
 * group's range of lb_dst) of the entry the working cursor points at after the
 * last message, or 0 when A ended at 0.  With no deactivation that is (cur0 +
 * M(g)) mod A, the LB call's value.  The permuted ring does not outlive the
 * call: a later call starts from lb_dst as the host keeps it, and finds an
 * entry whose credit is still 0 full again.  The exact turn after a
 * deactivation is therefore lb_t's within a call and approximate across calls,
 * like the turn after a membership change in zmqg_forward_zmtp_lb_multi.
 * Counts.  X(t) is the number of messages sent to t < n_dst in this call.
 * dst_taken[t] = min(X(t), dst_credit[t]) (X(t) when unlimited), dst_dropped[t]
 * = X(t) - dst_taken[t]; with ZMQG_CREDIT_CONSUME dst_credit[t] := dst_credit[t]
 * - dst_taken[t] (unlimited stays), written in a launch behind every read of
 * the old value; without the flag dst_credit is not written.  taken counts
 * admissions: a pair that then does not fit is ZMQG_ERR_BOUND and the host's to
 * send again.  When every destination is named by at most one ring entry over
 * all groups -- all that lb_t can have -- X(t) <= dst_credit[t] and dst_dropped
 * is all zero: refused messages are not counted against any destination.  A
 * destination named by several entries is counted per entry, each with the
 * whole credit; it may then be sent more than its credit: dst_dropped shows
 * the excess, and the write-back saturates at 0.  That is defined and
 * memory-safe.
 *
 * Identity.  With every credit ZMQG_CREDIT_UNLIMITED every output equals
 * zmqg_forward_framed_multi's with ZMQG_FWD_LB on the same input, byte for byte
 * and nonce for nonce, lb_cur included.
 *
 * Returns -EINVAL, with nothing queued, for a null credit, size !=
 * sizeof(zmqg_forward_credit), unknown flag bits, a mode other than
 * ZMQG_FWD_LB, n_dst > 0 with a null dst_credit, dst_taken or dst_dropped, and
 * every case of zmqg_forward_framed_multi with ZMQG_FWD_LB.  With n_streams ==
 * 0 nothing is done.  With N == 0 and n_dst > 0 dst_taken and dst_dropped are
 * zero-filled on the stream, dst_credit is not written and lb_cur is clamped as
 * in the LB call.  A grp_idx that does not rise can make two groups' ranges
 * overlap: all accesses stay in bounds, and the outcome of the overlapping
 * groups is unspecified.
 * Launches: the framed LB call's -- with the groups' launch one workgroup per
 * group, walking the group in epochs between deactivations (at most A0 + 1 of
 * them), and the pairs' launch reading its result -- and three more whatever the
 * sizes are: a memset of the counts X in front, the totals, and ZMQG_ERR_HWM
 * behind the send side (not queued without pair_status).
 * Not offered: persisting the permuted ring or an _active count across calls;
 * lb_t::has_out's eager deactivation; ZMQ_XPUB_NODROP, ZMQ_ROUTER_MANDATORY;
 * the low-water mark and re-activation, which are the host's (it refills
 * dst_credit); limits counted in bytes; compacting the pairs that are not live
 * before the encode. */
int zmqg_forward_lb_credit_multi(zmqg_ctx *ctx, const zmqg_forward_zmtp *args,
                                 const zmqg_forward_framing *framing,
                                 const zmqg_forward_credit *credit, void *stream);

/* Handshake key derivation in batches, one
 * 32-byte item per thread, items packed back to back:
 *   zmqg_scalarmult_batch: crypto_scalarmult_curve25519(out, scalar, point)
 *     (libsodium 1.0.18; RFC 7748 X25519): status -1 where the result is all
 *     zero (a small-order point), else 0.  point == NULL: the base point, as
 *     crypto_scalarmult_base for zmq_curve_public (src/zmq_utils.cpp:222-245);
 *     status always 0.
 *   zmqg_box_beforenm_batch: crypto_box_beforenm(k, pk, sk) =
 *     HSalsa20(X25519(sk, pk), 0^16), the connection's precomputed key
 *     (src/curve_client_tools.hpp:105, src/curve_server.cpp:382-383; the
 *     reference asserts success): status -1 and k not written where the
 *     scalar multiplication fails.
 * Asynchronous on `stream`; pointers as for the batch calls. */
int zmqg_scalarmult_batch(zmqg_ctx *ctx, uint64_t n, const uint8_t *scalar, const uint8_t *point, uint8_t *out,
                          int32_t *status_out, void *stream);
int zmqg_box_beforenm_batch(zmqg_ctx *ctx, uint64_t n, const uint8_t *pk, const uint8_t *sk, uint8_t *k_out,
                            int32_t *status_out, void *stream);

/* Handshake boxes in batches: every CURVE
 * command body is one crypto_box / crypto_secretbox with its own key and
 * 24-byte nonce -- HELLO (src/curve_client_tools.hpp:45), WELCOME
 * (src/curve_server.cpp:232, opened at src/curve_client_tools.hpp:92), the
 * cookie (src/curve_server.cpp:208, :334), INITIATE's vouch and box
 * (src/curve_client_tools.hpp:140, :177; src/curve_server.cpp:291, :359) and
 * READY (src/curve_server.cpp:441, src/curve_client.cpp:206).  With
 * crypto_box(pk, sk) = crypto_box_afternm(crypto_box_beforenm(pk, sk)) and
 * crypto_secretbox(k) = crypto_box_afternm(k) (libsodium 1.0.18), these two
 * calls plus zmqg_box_beforenm_batch seal and open all of them.  Item i:
 * key[32i .. +32], nonce[24i .. +24], input in[in_off[i] .. +len[i]], output
 * at out[out_off[i]] (the "easy" layouts: no NaCl zero padding).
 *   zmqg_box_afternm_batch: crypto_box_easy_afternm -- writes
 *     tag(16) || ciphertext(len[i]).
 *   zmqg_box_open_afternm_batch: crypto_box_open_easy_afternm -- reads
 *     tag || ciphertext (len[i] bytes), writes len[i] - 16 plaintext bytes,
 *     status_out[i] = 0; -1 where len[i] < 16 or the tag does not verify
 *     (checked before any plaintext is written; the region is then
 *     zero-filled).
 * One thread per box; inputs and outputs must not overlap.  Asynchronous on
 * `stream`; pointers as for the batch calls. */
int zmqg_box_afternm_batch(zmqg_ctx *ctx, uint64_t n, const uint8_t *key, const uint8_t *nonce,
                           const uint64_t *in_off, const uint32_t *len, const uint8_t *in, const uint64_t *out_off,
                           uint8_t *out, void *stream);
int zmqg_box_open_afternm_batch(zmqg_ctx *ctx, uint64_t n, const uint8_t *key, const uint8_t *nonce,
                                const uint64_t *in_off, const uint32_t *len, const uint8_t *in,
                                const uint64_t *out_off, uint8_t *out, int32_t *status_out, void *stream);

/* The server side of the CURVE handshake in batches (SURVEY.md section 8f
 * row 3): curve_server_t's HELLO -> WELCOME and INITIATE -> READY steps
 * (src/curve_server.cpp:117-458) for many connections per call, with the
 * reference's contract: the same commands in, the same commands out, the same
 * ZMQ_PROTOCOL_ERROR_* code for each rejected command, decided in the same
 * order.  The outputs feed zmqg_session_set_batch_ex as they are.
 *
 * The client side is the block after this one (zmqg_curve_client_*_batch).
 *
 * Out of scope: the state machine (which command to send or expect when);
 * ZAP and parse_metadata -- the INITIATE call returns the client's long-term
 * key and the metadata bytes and the host does the rest, as the reference
 * does between INITIATE and READY (src/curve_server.cpp:385-416); ERROR
 * commands.
 *
 * Conventions of the three calls: asynchronous on `stream`; every pointer is
 * device-accessible; command bytes may start at any byte alignment, the packed
 * fixed-size arrays (state, random, welcome_out, client_key_out, precom_out)
 * are 4-byte aligned; n == 0 returns 0 and does nothing; a null pointer with
 * n > 0, or n > 2^31 - 1, returns -EINVAL; the host reads nothing back.  A
 * rejected command is not a call failure: its code is in status_out.
 *
 * zmqg_curve_server_hello_batch: process_hello + produce_welcome
 * (src/curve_server.cpp:117-254).  Item i is the command body
 * cmd[cmd_off[i] .. +cmd_len[i]).  server_sk is the socket's long-term secret
 * (_secret_key), common to the batch.  random[96 i ..] supplies what the
 * reference draws with randombytes (the device has no RNG, and the call is
 * deterministic): bytes 0..32 s' (the short-term secret, _cn_secret), 32..64
 * the cookie key (:204), 64..80 the cookie nonce (:194), 80..96 the WELCOME
 * nonce (:221).  Checks, in this order, the first that fails giving the status:
 *   1. len <= 1 or len <= cmd[0]                 ZMQG_ERR_MALFORMED_UNSPECIFIED
 *      (check_basic_command_structure, src/mechanism_base.cpp:14-25)
 *   2. len < 6 or not "\x05HELLO" (:126)         ZMQG_ERR_UNEXPECTED_COMMAND
 *   3. len != 200 (:133)                         ZMQG_ERR_MALFORMED_HELLO
 *   4. cmd[6] != 1 or cmd[7] != 0 (:144)         ZMQG_ERR_MALFORMED_HELLO
 *   5. the box cmd[120..200) does not open under k1 = crypto_box_beforenm(C' =
 *      cmd[80..112), server_sk) and nonce "CurveZMQHELLO---" || cmd[112..120)
 *      (:169)                                    ZMQG_ERR_CRYPTOGRAPHIC
 *      A C' whose X25519 result is all zero (small order) counts as not
 *      opening, as libsodium's crypto_box_open does.  The 64 plaintext bytes
 *      are not inspected; the reference does not inspect them either.
 * On success status_out[i] = 0; welcome_out[168 i ..] holds the WELCOME command
 * "\x07WELCOME" || WELCOME nonce || box, the box (:232) under k1 and nonce
 * "WELCOME-" || WELCOME nonce over S' || cookie nonce || cookie box with S' =
 * X25519(s', 9) and the cookie box (:208) crypto_secretbox of C' || s' under
 * the cookie key and nonce "COOKIE--" || cookie nonce; and state[128 i ..]
 * holds C'(32) | s'(32) | cookie key(32) | precom(32) with precom =
 * crypto_box_beforenm(C', s'), the connection's _cn_precom.  It is derived
 * here, where its ladder runs beside the other two, not at INITIATE where the
 * reference derives it (:382-383); the value is the same.  `state` holds
 * secrets: the caller owns it and clears it.  On failure the item's WELCOME
 * slot and state record are zero-filled. */
#define ZMQG_ERR_KEY_EXCHANGE 0x10000003       /* ZMQ_PROTOCOL_ERROR_ZMTP_KEY_EXCHANGE */
#define ZMQG_ERR_MALFORMED_HELLO 0x10000013    /* ..._MALFORMED_COMMAND_HELLO */
#define ZMQG_ERR_MALFORMED_INITIATE 0x10000014 /* ..._MALFORMED_COMMAND_INITIATE */
#define ZMQG_HS_STATE_BYTES 128
#define ZMQG_HS_RANDOM_BYTES 96
#define ZMQG_HS_WELCOME_BYTES 168
int zmqg_curve_server_hello_batch(zmqg_ctx *ctx, uint64_t n, const uint8_t server_sk[32], const uint64_t *cmd_off,
                                  const uint32_t *cmd_len, const uint8_t *cmd, const uint8_t *random, uint8_t *state,
                                  uint8_t *welcome_out, int32_t *status_out, void *stream);

/* zmqg_curve_server_initiate_batch: process_initiate up to the ZAP decision
 * (src/curve_server.cpp:256-383).  state[128 i ..] is what the HELLO call
 * wrote for this connection (a gathered array when the batch order differs).
 * Checks, in this order:
 *   1. basic structure, as above                 ZMQG_ERR_MALFORMED_UNSPECIFIED
 *   2. len < 9 or not "\x08INITIATE" (:265)      ZMQG_ERR_UNEXPECTED_COMMAND
 *   3. len < 257 (:272)                          ZMQG_ERR_MALFORMED_INITIATE
 *   4. the cookie box cmd[25..105) does not open under state's cookie key and
 *      nonce "COOKIE--" || cmd[9..25) (:291)     ZMQG_ERR_CRYPTOGRAPHIC
 *   5. its 64 plaintext bytes differ from state's C' || s' (:302)
 *                                                ZMQG_ERR_CRYPTOGRAPHIC
 *   6. the box cmd[113..len) does not open under state's precom and nonce
 *      "CurveZMQINITIATE" || cmd[105..113) (:334) ZMQG_ERR_CRYPTOGRAPHIC
 *   7. its plaintext is C(32) || vouch nonce(16) || vouch box(80) || metadata;
 *      the vouch box does not open under crypto_box_beforenm(C, s') and nonce
 *      "VOUCH---" || vouch nonce (:359; a small-order C counts as not
 *      opening)                                  ZMQG_ERR_CRYPTOGRAPHIC
 *   8. the vouch's first 32 plaintext bytes differ from C' (:370)
 *                                                ZMQG_ERR_KEY_EXCHANGE
 * On success status_out[i] = 0, client_key_out[32 i ..] = C (what
 * send_zap_request receives), precom_out[32 i ..] = precom (packed, so the
 * array goes to zmqg_session_set_batch_ex as is), peer_nonce_out[i] =
 * BE64(cmd[105..113)), the value the reference passes to set_peer_nonce (:330)
 * and that call's peer_nonce entry, meta_len_out[i] = len - 257 and the
 * metadata bytes (parse_metadata's input, :415) at meta_out[meta_off[i] ..].
 * On failure the key and precom slots are zero, peer_nonce_out[i] and
 * meta_len_out[i] are 0 and no byte of meta_out is written.  The INITIATE tag
 * is verified over the ciphertext before anything is decrypted, and the
 * metadata is decrypted to meta_out only after check 8 has passed. */
int zmqg_curve_server_initiate_batch(zmqg_ctx *ctx, uint64_t n, const uint8_t *state, const uint64_t *cmd_off,
                                     const uint32_t *cmd_len, const uint8_t *cmd, uint8_t *client_key_out,
                                     uint8_t *precom_out, uint64_t *peer_nonce_out, const uint64_t *meta_off,
                                     uint8_t *meta_out, uint32_t *meta_len_out, int32_t *status_out, void *stream);

/* zmqg_curve_server_ready_batch: produce_ready (src/curve_server.cpp:419-458).
 * Writes 30 + meta_len[i] bytes at out[out_off[i]] (any alignment): "\x05READY"
 * || BE64(nonce[i]) || box of meta[meta_off[i] .. +meta_len[i]) under
 * precom[32 i ..] and nonce "CurveZMQREADY---" || BE64(nonce[i]) (:435-441).
 * nonce[i] is what get_and_inc_nonce returns there: 1 for a fresh connection,
 * whose session is then installed with send nonce 2 (zmqg_session_set_batch_ex
 * above).  Outputs must not overlap each other or `meta`. */
int zmqg_curve_server_ready_batch(zmqg_ctx *ctx, uint64_t n, const uint8_t *precom, const uint64_t *nonce,
                                  const uint64_t *meta_off, const uint32_t *meta_len, const uint8_t *meta,
                                  const uint64_t *out_off, uint8_t *out, void *stream);

/* The client side of the CURVE handshake in batches: curve_client_t's HELLO,
 * WELCOME -> INITIATE and READY steps (src/curve_client.cpp:112-214,
 * src/curve_client_tools.hpp:29-199) for many connections per call -- a
 * process that dials many CURVE peers.  The commands are the reference's byte
 * for byte, and a rejected command gets the code the reference reports.  The
 * outputs feed zmqg_session_set_batch_ex as they are; the client's session is
 * installed with send nonce 3 (see that call's comment) and READY's peer nonce.
 *
 * Out of scope: the state machine, ZAP (a server matter), parse_metadata --
 * the READY call returns the metadata bytes -- and ERROR commands.  The caller
 * dispatches by command name, as process_handshake_command does
 * (src/curve_client.cpp:65-78): a READY or ERROR command passed to the WELCOME
 * call is "unexpected" there.
 *
 * Conventions as for the three server calls: asynchronous on `stream`; every
 * pointer is device-accessible; command bytes (cmd, meta, out, meta_out) may
 * start at any byte alignment, the packed fixed-size arrays (server_pk,
 * cn_secret, state, hello_out, client_pk, client_sk, vouch_nonce, precom,
 * precom_out) are 4-byte aligned; n == 0 returns 0 and does nothing; a null
 * pointer with n > 0, or n > 2^31 - 1, returns -EINVAL; the host reads nothing
 * back.  A rejected command is not a call failure: its code is in status_out.
 * The device has no RNG: what the reference draws with randombytes comes in as
 * an argument, and each call is deterministic.
 *
 * zmqg_curve_client_hello_batch: crypto_box_keypair
 * (src/curve_client_tools.hpp:230-234) + produce_hello (:29-65,
 * src/curve_client.cpp:112-131).  server_pk[32 i ..] is connection i's server
 * long-term key S (per item: a dialling process talks to many servers),
 * cn_secret[32 i ..] the 32 random bytes of the short-term secret c' (used as
 * given; X25519 clamps them), nonce[i] what get_and_inc_nonce returns, 1 on a
 * fresh connection.  Per item C' = X25519(c', 9), k1 = crypto_box_beforenm(S,
 * c') and the box of 64 zero bytes under k1 and nonce "CurveZMQHELLO---" ||
 * BE64(nonce).  On success status_out[i] = 0, hello_out[200 i ..] =
 * "\x05HELLO" 01 00 | 72 zero bytes | C' | BE64(nonce) | box(80) and
 * state[128 i ..] = C'(32) | c'(32) | k1(32) | S(32).  Where X25519(c', S) is
 * all zero (a small-order S) crypto_box fails and the reference reports
 * ZMQ_PROTOCOL_ERROR_ZMTP_CRYPTOGRAPHIC (src/curve_client.cpp:118-120):
 * status_out[i] = ZMQG_ERR_CRYPTOGRAPHIC and the item's HELLO slot and state
 * record are zero-filled.  `state` holds secrets: the caller owns it and
 * clears it. */
#define ZMQG_ERR_MALFORMED_READY 0x10000016 /* ..._MALFORMED_COMMAND_READY */
#define ZMQG_HS_HELLO_BYTES 200
#define ZMQG_HS_CLIENT_STATE_BYTES 128
int zmqg_curve_client_hello_batch(zmqg_ctx *ctx, uint64_t n, const uint8_t *server_pk, const uint8_t *cn_secret,
                                  const uint64_t *nonce, uint8_t *state, uint8_t *hello_out, int32_t *status_out,
                                  void *stream);

/* zmqg_curve_client_welcome_batch: process_welcome + produce_initiate
 * (src/curve_client_tools.hpp:67-199, src/curve_client.cpp:133-177), which the
 * reference runs back to back.  state[128 i ..] is what the HELLO call wrote;
 * client_pk / client_sk[32 i ..] the long-term pair C, c; item i's command is
 * cmd[cmd_off[i] .. +cmd_len[i]); vouch_nonce[16 i ..] the 16 random bytes of
 * :137; nonce[i] INITIATE's nonce, 2 on a fresh connection; the client's
 * metadata (as add_basic_properties produces it; any length, 0 included) is
 * meta[meta_off[i] .. +meta_len[i]).  Checks, in this order, the first that
 * fails giving the status:
 *   1. len < 8 or not "\x07WELCOME"               ZMQG_ERR_UNEXPECTED_COMMAND
 *      (is_handshake_command, :286-290; nothing is read from an empty
 *      command; the client does not call check_basic_command_structure)
 *   2. len != 168 (:75)                           ZMQG_ERR_CRYPTOGRAPHIC
 *      (the reference reports CRYPTOGRAPHIC for every process_welcome
 *      failure, src/curve_client.cpp:139-141, not MALFORMED_WELCOME)
 *   3. the box cmd[24..168) does not open under state's k1 and nonce
 *      "WELCOME-" || cmd[8..24) (:92)             ZMQG_ERR_CRYPTOGRAPHIC
 *   4. its plaintext is S'(32) || cookie(96); X25519(c', S') is all zero (a
 *      small-order S' inside a valid box)         ZMQG_ERR_CRYPTOGRAPHIC
 *      Deviation: the reference zmq_asserts there (:105-106) and aborts the
 *      process; a batch call reports the connection instead.
 * On success status_out[i] = 0, precom_out[32 i ..] = crypto_box_beforenm(S',
 * c') (packed, so the array goes to zmqg_session_set_batch_ex and to the READY
 * call as is) and 257 + meta_len[i] bytes are written at out[out_off[i]]:
 * "\x08INITIATE" | cookie(96) | BE64(nonce) | box, the box (:177) under precom
 * and nonce "CurveZMQINITIATE" || BE64(nonce) over C | vouch_nonce | vouch
 * box(80) | metadata, the vouch box (:140) that of C' || S under
 * crypto_box_beforenm(S', c) and nonce "VOUCH---" || vouch_nonce.  On failure
 * the precom slot is zero and no byte of `out` is written (every verdict is
 * known before the first seal).  Outputs must not overlap each other, `cmd`
 * or `meta`; 257 + meta_len[i] must fit 32 bits. */
int zmqg_curve_client_welcome_batch(zmqg_ctx *ctx, uint64_t n, const uint8_t *state, const uint8_t *client_pk,
                                    const uint8_t *client_sk, const uint64_t *cmd_off, const uint32_t *cmd_len,
                                    const uint8_t *cmd, const uint8_t *vouch_nonce, const uint64_t *nonce,
                                    const uint64_t *meta_off, const uint32_t *meta_len, const uint8_t *meta,
                                    const uint64_t *out_off, uint8_t *out, uint8_t *precom_out, int32_t *status_out,
                                    void *stream);

/* zmqg_curve_client_ready_batch: process_ready up to parse_metadata
 * (src/curve_client.cpp:179-214).  Checks, in this order:
 *   1. len < 6 or not "\x05READY"                 ZMQG_ERR_UNEXPECTED_COMMAND
 *   2. len < 30                                   ZMQG_ERR_MALFORMED_READY
 *   3. the box cmd[14..len) does not open under precom[32 i ..] and nonce
 *      "CurveZMQREADY---" || cmd[6..14)           ZMQG_ERR_CRYPTOGRAPHIC
 *      (the tag is verified over the whole ciphertext before any byte is
 *      decrypted)
 * On success status_out[i] = 0, peer_nonce_out[i] = BE64(cmd[6..14)), the value
 * :204 passes to set_peer_nonce and zmqg_session_set_batch_ex's peer_nonce
 * entry, meta_len_out[i] = len - 30 and the metadata bytes (parse_metadata's
 * input) are at meta_out[meta_off[i] ..].  On failure both are 0 and no byte
 * of meta_out is written. */
int zmqg_curve_client_ready_batch(zmqg_ctx *ctx, uint64_t n, const uint8_t *precom, const uint64_t *cmd_off,
                                  const uint32_t *cmd_len, const uint8_t *cmd, uint64_t *peer_nonce_out,
                                  const uint64_t *meta_off, uint8_t *meta_out, uint32_t *meta_len_out,
                                  int32_t *status_out, void *stream);

/* Batched Z85 key codec: zmq_z85_encode /
 * zmq_z85_decode (src/zmq_utils.cpp:100-180, include/zmq.h:537-540) over n
 * independent items, one per thread.  Item i: input bytes
 * in[in_off[i] .. +len[i]), output at out[out_off[i]]; status_out[i] = 0 or
 * EINVAL where the reference returns NULL with errno EINVAL.
 *   encode: len % 4 == 0, writes len * 5 / 4 characters and a NUL.
 *   decode: len = strlen of the string (>= 5, multiple of 5), writes
 *     len * 4 / 5 bytes; an invalid character or a group above 0xffffffff
 *     fails the item after the groups before it were written, as the
 *     reference's loop does.
 * Pointers as for the batch calls (device or device-accessible host memory);
 * asynchronous on `stream`. */
int zmqg_z85_encode_batch(zmqg_ctx *ctx, uint64_t n, const uint64_t *in_off, const uint32_t *len, const uint8_t *in,
                          const uint64_t *out_off, char *out, int32_t *status_out, void *stream);
int zmqg_z85_decode_batch(zmqg_ctx *ctx, uint64_t n, const uint64_t *in_off, const uint32_t *len, const char *in,
                          const uint64_t *out_off, uint8_t *out, int32_t *status_out, void *stream);

/* Profiling hooks (off by default).  When enabled, the ctx records a HIP
 * event pair on the batch's stream around each of its kernels of one kind:
 *   ZMQG_PROF_ENCODE_MAIN / ZMQG_PROF_DECODE_MAIN  the frame kernel alone
 *     (every frame up to 4.5 KiB of stream: the dominant kernel),
 *   ZMQG_PROF_ENCODE_CALL / ZMQG_PROF_DECODE_CALL  the whole batch call,
 *   ZMQG_PROF_ENCODE_BODY / ZMQG_PROF_DECODE_BODY  the chunked body kernel
 *     (larger frames) alone.
 * zmqg_ctx_get_profile synchronises the device, returns the summed elapsed
 * milliseconds and launch count for `kind` since the last reset, and resets. */
#define ZMQG_PROF_ENCODE_MAIN 0
#define ZMQG_PROF_DECODE_MAIN 1
#define ZMQG_PROF_ENCODE_CALL 2
#define ZMQG_PROF_DECODE_CALL 3
#define ZMQG_PROF_ENCODE_BODY 4
#define ZMQG_PROF_DECODE_BODY 5
int zmqg_ctx_set_profiling(zmqg_ctx *ctx, int enable);
int zmqg_ctx_get_profile(zmqg_ctx *ctx, int kind, double *ms_total, uint64_t *launches);

/* Text for the last HIP error seen by this ctx (static storage). */
const char *zmqg_last_error(zmqg_ctx *ctx);

/* Build identity, "<source id> <commit>": the first 16 hex digits of the
 * SHA-256 of the library's sources (the .hip and .hpp files of libzmq_amd/csrc and this
 * header, in name order) and the git commit the tree was at when it was
 * built.  Measurement files under profiles/ carry the source id of the
 * library they measured; bench.py folds them into its line only when it
 * equals the loaded library's. */
const char *zmqg_build_id(void);

#ifdef __cplusplus
}
#endif

#endif
