// The context (zmqg_ctx): its device buffers, error reporting and stream
// ordering.  Part of zmqg_curve.hip, included there after the types it names.
// Every stream-ordered allocation is a DevBuf reserved from ctx->mem, which
// zmqg_ctx_destroy frees whole ("Who owns device memory"): a new
// buffer is declared once here and reserved once in its group.
#pragma once
#include "curve_devbuf.hpp"

// the arena's allocator: the only stream-ordered allocation calls of the library
struct HipMem {
    typedef hipStream_t stream_t;
    typedef hipError_t error_t;
    static hipError_t alloc_async(void **p, size_t bytes, hipStream_t st) { return hipMallocAsync(p, bytes, st); }
    static hipError_t free_async(void *p, hipStream_t st) { return hipFreeAsync(p, st); }
    static void free_now(void *p) { (void) hipFree(p); }
};

namespace {

typedef unsigned long long u64ll;

struct Workspace {
    uint64_t cap = 0; // frames (0 while the group grows: a failed growth is taken up again by the next call)
    DevBuf<FrameHot> hot;
    DevBuf<FramePow> pw;
    DevBuf<FrameFin> fin;
    DevBuf<uint32_t> powtab;     // [cap][kMaxPow][5], entries k >= kPowInline
    DevBuf<u64ll> acc;           // [cap][5]
    DevBuf<uint32_t> cnt;        // [cap]
    DevBuf<uint32_t> chunk_end;  // [cap]
    DevBuf<u64ll> v;             // [cap] accepted nonce or 0
    DevBuf<u64ll> excl;          // [cap]
    DevBuf<uint32_t> list_frame; // [cap] big-frame list: frame index at each position
    DevBuf<PostOp> post;         // [cap] decode: k_post's zero fills and in-place moves
    DevBuf<u64ll> psnap;         // [cap] session peer nonce before the batch, per frame
    DevBuf<ZState> zs;           // call state carried from call to call (on the device)
    DevBuf<u64ll> lb_flag;       // [cap] look-back state per workgroup ticket
    DevBuf<u64ll> lb_agg;        // [cap]
    DevBuf<u64ll> lb_inc;        // [cap]
    DevBuf<u64ll> lb_rec;        // [2 kFramesBS] k_frames_seq's one-round look-back records
    DevBuf<uint64_t> nonce;      // [cap] ZMQG_OPT_NONCE_AUTO over several sessions: each frame's nonce
    // replay_multi's sort fallback (max_sessions > kReplayMaxSessions), reserved only there
    DevBuf<u64ll> v_s;       // [cap] sorted
    DevBuf<u64ll> excl_s;    // [cap]
    DevBuf<uint32_t> iota;   // [cap]
    DevBuf<uint32_t> perm;   // [cap]
    DevBuf<uint32_t> keys_s; // [cap]
    DevBuf<uint8_t> last;    // [cap] last frame of its session in the batch
    DevBuf<uint8_t, 0> temp; // its hipCUB temporaries
    // sized by the call, not by cap
    DevBuf<u64ll, 0> rt;      // replay tables: [tiles][S] then [row blocks][S] (also the nonce tables)
    DevBuf<uint8_t, 0> stage; // ZMQG_OPT_VERIFY_FIRST: decoded payloads before the verdict copy
    bool use_last = false;    // the last replay ran the sort fallback (k_fixup writes the peer nonces)
};

// the synchronous zmqg_decode_zmtp's result, written by the decode into mapped host memory
struct ZmtpResHost {
    zmqg_zmtp_result r;
};

// device buffers of the ZMTP framing calls (the capacities: 0 while their group grows)
struct ZmtpWs {
    uint64_t n_cap = 0;         // send side: frames
    DevBuf<uint64_t> F;         // [n_cap + 1] frame bytes
    DevBuf<uint64_t> wire_off;  // [n_cap] body offsets
    uint64_t g_cap = 0;         // receive side: 16 KiB workgroups of the stream
    DevBuf<uint64_t> cand_wg;   // [g_cap * kZmtpWgCap] each workgroup's candidates, in order
    DevBuf<uint64_t> count_wg;  // [g_cap + 1]
    DevBuf<uint64_t> off_wg;    // [g_cap + 1] exclusive sum of count_wg
    DevBuf<uint64_t> first_w;   // [g_cap + 1] first unlinked candidate in workgroup lists >= w
    DevBuf<uint16_t> count16;   // [g_cap + 8] count_wg as 16-bit fields (k_zmtp_compact sums them)
    uint64_t c_cap = 0;         // receive side: candidates
    DevBuf<uint64_t> cand;      // [c_cap] sorted candidates
    DevBuf<uint64_t> nb;        // [c_cap] next unlinked candidate in the 256-candidate segment
    DevBuf<uint32_t> wid;       // [c_cap] each candidate's workgroup list
    DevBuf<uint64_t> cdesc;     // [c_cap] their frames: body offset | body length << 32
    DevBuf<uint8_t> cflag;      // [c_cap] their flags bytes
    uint64_t f_cap = 0;         // receive side: frames (max_frames)
    DevBuf<uint64_t> run;       // [2 (f_cap + 1)]
    DevBuf<uint64_t> runpre;    // [f_cap + 1]
    DevBuf<uint32_t> sid_fill;  // [f_cap]
    DevBuf<uint8_t> fflags;     // [f_cap]
    DevBuf<ZmtpWalk> walk;
    ZmtpResHost *res = nullptr;     // the synchronous call's result, mapped host memory
    ZmtpResHost *res_dev = nullptr; // (its device address)
    DevBuf<uint8_t, 0> temp;    // hipCUB temporaries
    uint64_t s_cap = 0;         // zmqg_encode_zmtp_multi: frames
    DevBuf<uint32_t> s_sid;     // [s_cap] the session each frame is encoded on (or none)
    DevBuf<uint64_t> s_woff;    // [s_cap] body offsets
    DevBuf<u64ll> s_tab;        // [tiles][streams], [row blocks][streams], bases and totals [2][streams]
    uint64_t p_cap = 0;         // zmqg_forward_zmtp_multi: pairs (the encode's inputs; not s_sid / s_woff, its own)
    DevBuf<uint32_t> p_stream;  // [p_cap] the destination each pair goes to (or none)
    DevBuf<uint8_t> p_flags;    // [p_cap] its MORE bit
    DevBuf<uint64_t> p_off;     // [p_cap] its payload's offset in `plain`
    DevBuf<uint32_t> p_len;     // [p_cap] and length
    DevBuf<uint32_t> p_tab;     // the call's host arrays as one table (curve_fwd_common.hpp)
    uint64_t m_cap = 0;         // zmqg_forward_zmtp_sub_multi: pairs
    DevBuf<uint8_t> p_match;    // [m_cap] at a head's pairs: its route's destination is subscribed to the topic
    uint64_t e_cap = 0;         // and elements of the routed streams
    DevBuf<uint32_t> e_head;    // [e_cap] the index in Q(s) of each forwarded element's head
    uint64_t v_cap = 0;         // zmqg_forward_zmtp_router_multi with ROUTE: elements
    DevBuf<uint32_t> e_verdict; // [v_cap] at a head: the destination its address names, or UNKNOWN / MALFORMED
    uint64_t l_cap = 0;         // zmqg_forward_zmtp_lb_multi: elements
    DevBuf<uint32_t> e_rank;    // [l_cap] at a forwarded data element: the rank of its message within the stream
    uint64_t ls_cap = 0;        // and source streams
    DevBuf<uint32_t> s_msgs;    // [ls_cap] the stream's forwarded messages
    DevBuf<uint32_t> s_first;   // [ls_cap] the ring position of its first message
    uint64_t k_cap = 0;         // zmqg_forward_credit_multi: pairs
    DevBuf<uint32_t> p_key;     // [k_cap] at a delivery's first pair: its destination (else none)
    DevBuf<uint32_t> p_rank;    // [k_cap] and its rank among that destination's deliveries
    DevBuf<uint8_t> p_hwm;      // [k_cap] the pair was live and its delivery was refused
    DevBuf<uint32_t> k_tab;     // [tiles][destinations], [row blocks][destinations], totals [destinations]
    uint64_t lc_cap = 0;        // zmqg_forward_lb_credit_multi: elements
    DevBuf<uint32_t> e_pick;    // [lc_cap] at ebase[s] + i: where stream s's i-th message goes, or refused
    uint64_t lr_cap = 0;        // and ring entries (n_lb), at each group's absolute positions
    DevBuf<uint32_t> r_orig;    // [lr_cap] the working ring: each entry's original position in its group
    DevBuf<uint32_t> r_w;       // [lr_cap] and its working credit
    DevBuf<uint32_t> x_tot;     // [destinations] the messages sent to each
    uint64_t u_cap = 0;         // zmqg_subs_update_multi: events (cleared slots, then the decode call's slots)
    DevBuf<uint32_t> u_h0;      // [u_cap] the slots holding the event's topic at call start
    DevBuf<int8_t> u_delta;     // [u_cap] what the event did to its destination's hold on the topic: +1 / -1 / 0
    DevBuf<uint32_t> u_tab;     // the call's host arrays: stream_dst, clear_dst
};
} // namespace

struct zmqg_ctx {
    int device = 0;
    int cus = 256; // compute units of the device (one persistent body workgroup each)
    uint32_t max_sessions = 0;
    int sort_bits = 0; // ceil(log2(max_sessions)); > 0: several sessions (the replay tables or the sort fallback)
    DevSession *sessions = nullptr;
    unsigned long long *peer = nullptr; // [max_sessions]
    unsigned long long *send = nullptr; // [max_sessions] send nonces (_cn_nonce) for ZMQG_OPT_NONCE_AUTO
    DevArena<HipMem> mem;               // owns every buffer below, ws's and zw's
    DevBuf<u64ll, 0> zero_peer;         // [max_sessions] zeros: ZMQG_OPT_REPLAY_HOST's peer snapshot
    Workspace ws;
    ZmtpWs zw;
    // host staging for the *_host entry points
    uint8_t *pin = nullptr;
    size_t pin_bytes = 0;
    uint8_t *mpin = nullptr, *mpin_dev = nullptr; // the per-message buffer (zmqg_*_msg), device-mapped
    size_t mpin_bytes = 0;
    // pinned, device-mapped staging for a call's host arrays (the descriptors
    // of zmqg_session_set_batch's install, zmqg_forward_zmtp_multi's tables),
    // free again once `sinst_done` is reached
    uint8_t *sinst = nullptr, *sinst_dev = nullptr;
    size_t sinst_bytes = 0;
    hipEvent_t sinst_done = nullptr;
    hipEvent_t order_ev = nullptr; // zmqg_*_msg: own_stream waits for the last batch stream's work
    uint8_t *dbuf = nullptr;
    size_t dbuf_bytes = 0;
    hipStream_t own_stream = nullptr;
    // the stream of the last batch call (the session accessors and the
    // per-message calls order after it); has_last tells "none yet" from the
    // null stream, which is a stream like any other here
    hipStream_t last_stream = nullptr;
    bool has_last = false;
    std::vector<uint8_t> h_downgrade; // host copy of each session's downgrade_sub
    // profiling: event pairs per kind, recycled through a pool
    bool profiling = false;
    int frames_cap[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // decode frame-kernel workgroups resident at once, G = 1,
                                                     // 2, 4, seq, lds, split 2, 4, 8, seq under STREAM_OUT
    int force_g = -1;                 // ZMQG_FRAMES_G: frame-kernel variant override (experiments)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof[6];
    std::vector<hipEvent_t> event_pool;
    // completion fences of the asynchronous host path: (id, event) pending,
    // events recycled through fence_pool
    std::vector<std::pair<uint64_t, hipEvent_t>> fences;
    std::vector<hipEvent_t> fence_pool;
    // zmqg_fence_record_notify: ids whose host function has run (a fence
    // found there is reached whatever its event says), and the host
    // functions enqueued and not yet finished
    std::mutex notify_mu;
    std::vector<uint64_t> notified;
    std::atomic<int> notify_pending{0};
    uint64_t fence_ctr = 0;
    std::mutex fence_mu;
    char last_error[256] = {0};
    std::mutex mu;
};

#define ZCHECK(ctx, expr)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            snprintf((ctx)->last_error, sizeof((ctx)->last_error), "%s:%d %s: %s", __FILE__,   \
                     __LINE__, #expr, hipGetErrorString(e_));                                  \
            return -EIO;                                                               \
        }                                                                                      \
    } while (0)

// Room for `count` elements in one of the ctx's buffers, on `st`.  A group of
// buffers behind one capacity sets it to 0, reserves every member, then sets
// it: a failure part-way leaves 0, the next call reserves again (the members
// that grew are no-ops then), and no call ever runs on a half-grown group.
#define ZRESERVE(ctx, buf, count, st) ZCHECK(ctx, (buf).reserve((ctx)->mem, (count), (st)))

// The same for a group whose members all have `cap` elements; `names` is the
// group as last_error reports it.
template <class... Bufs>
static int reserve_group(zmqg_ctx *ctx, hipStream_t st, const char *names, uint64_t &cap, uint64_t floor,
                         uint64_t need, Bufs &...bufs)
{
    if (need <= cap)
        return 0;
    const uint64_t grown = grown_cap(cap, floor, need);
    cap = 0;
    hipError_t e = hipSuccess;
    (void) (((e = bufs.reserve(ctx->mem, grown, st)) == hipSuccess) && ...); // (in order, up to the first failure)
    if (e != hipSuccess) {
        snprintf(ctx->last_error, sizeof ctx->last_error, "reserve_group(%s): %s", names, hipGetErrorString(e));
        return -EIO;
    }
    cap = grown;
    return 0;
}

// a grid of one wave per item, `threads` a workgroup
static inline unsigned wave_grid(uint64_t n, uint32_t threads)
{
    const uint64_t per = threads / 64u;
    return (unsigned) ((n + per - 1) / per);
}

// The decode's options for a receive side with this maxmsgsize, in *o, or null:
// a maxmsgsize within the frame kernel's range bounds every frame, so the
// large-frame launches are skipped.
static inline const zmqg_batch_opts *decode_len_bound(int64_t max_msg_size, zmqg_batch_opts *o)
{
    if (max_msg_size < 0 || (uint64_t) max_msg_size > kMaxFrameStream)
        return nullptr;
    *o = zmqg_batch_opts{};
    o->size = sizeof *o;
    o->max_len = max_msg_size > 0 ? (uint64_t) max_msg_size : 1u;
    return o;
}

// The ctx's work is ordered by stream: a batch call runs on the caller's
// stream (which then becomes the ctx's last stream); every call that uses
// the ctx's workspace or sessions on another stream than the last one --
// the batch calls, the session installs and accessors, the per-message
// calls -- first makes it wait for everything queued on the last one (an
// event recorded there, order_after_last; nothing when the stream is the
// same).  The null stream is a stream like any other: with own_stream
// non-blocking it is not ordered implicitly.
static void set_last(zmqg_ctx *ctx, hipStream_t st)
{
    ctx->last_stream = st;
    ctx->has_last = true;
}

static int order_after_last(zmqg_ctx *ctx, hipStream_t st)
{
    if (ctx->has_last && ctx->last_stream != st) {
        if (!ctx->order_ev)
            ZCHECK(ctx, hipEventCreateWithFlags(&ctx->order_ev, hipEventDisableTiming));
        ZCHECK(ctx, hipEventRecord(ctx->order_ev, ctx->last_stream));
        ZCHECK(ctx, hipStreamWaitEvent(st, ctx->order_ev, 0));
    }
    set_last(ctx, st);
    return 0;
}

namespace {

__global__ void k_zstate_init(ZState *zs);

// Workspace for n frames, grown in stream order on the batch's stream: the
// old buffers are freed and the new ones allocated and initialised on `st`,
// after the work already queued there (no device-wide synchronisation).
int ensure_workspace(zmqg_ctx *ctx, uint64_t n, hipStream_t st)
{
    Workspace &w = ctx->ws;
    const bool sorts = ctx->max_sessions > kReplayMaxSessions; // the sort fallback of replay_multi
    if (n > w.cap) {
        const uint64_t cap = grown_cap(w.cap, 1024, n);
        w.cap = 0;
        ZRESERVE(ctx, w.hot, cap, st);
        ZRESERVE(ctx, w.pw, cap, st);
        ZRESERVE(ctx, w.fin, cap, st);
        ZRESERVE(ctx, w.powtab, cap * kMaxPow * 5, st);
        ZRESERVE(ctx, w.acc, cap * 5, st);
        ZRESERVE(ctx, w.cnt, cap, st);
        ZRESERVE(ctx, w.chunk_end, cap, st);
        ZRESERVE(ctx, w.v, cap, st);
        ZRESERVE(ctx, w.excl, cap, st);
        ZRESERVE(ctx, w.list_frame, cap, st);
        ZRESERVE(ctx, w.post, cap, st);
        ZRESERVE(ctx, w.psnap, cap, st);
        ZRESERVE(ctx, w.lb_flag, cap, st);
        ZRESERVE(ctx, w.lb_agg, cap, st);
        ZRESERVE(ctx, w.lb_inc, cap, st);
        ZRESERVE(ctx, w.lb_rec, 2 * kFramesBS, st);
        ZRESERVE(ctx, w.nonce, cap, st);
        if (sorts) {
            ZRESERVE(ctx, w.v_s, cap, st);
            ZRESERVE(ctx, w.excl_s, cap, st);
            ZRESERVE(ctx, w.iota, cap, st);
            ZRESERVE(ctx, w.perm, cap, st);
            ZRESERVE(ctx, w.keys_s, cap, st);
            ZRESERVE(ctx, w.last, cap, st);
        }
        ZCHECK(ctx, hipMemsetAsync(w.lb_flag, 0, cap * sizeof(unsigned long long), st));
        ZCHECK(ctx, hipMemsetAsync(w.lb_rec, 0, 2 * kFramesBS * sizeof(unsigned long long), st)); // (no record valid)
        if (!w.zs) {
            ZRESERVE(ctx, w.zs, 1, st);
            hipLaunchKernelGGL(k_zstate_init, dim3(1), dim3(64), 0, st, w.zs);
            ZCHECK(ctx, hipGetLastError());
        }
        w.cap = cap;
    }
    if (sorts) { // hipCUB temporaries for n frames
        size_t need = 0, b = 0;
        ZCHECK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, need, (const uint32_t *) nullptr, w.keys_s.p,
                                                        (const uint32_t *) nullptr, w.perm.p, (int) n, 0,
                                                        kSortKeyBits));
        ZCHECK(ctx, hipcub::DeviceScan::ExclusiveScanByKey(nullptr, b, w.keys_s.p, w.v_s.p, w.excl_s.p, hipcub::Max(),
                                                            0ull, (int) n));
        need = b > need ? b : need;
        ZRESERVE(ctx, w.temp, grown_cap(w.temp.count, 4096, need), st);
    }
    return 0;
}

// ZMQG_OPT_REPLAY_HOST: a zeroed peer-nonce table for the frame kernels
int ensure_zero_peer(zmqg_ctx *ctx, hipStream_t st)
{
    if (ctx->zero_peer)
        return 0;
    ZRESERVE(ctx, ctx->zero_peer, ctx->max_sessions, st);
    ZCHECK(ctx, hipMemsetAsync(ctx->zero_peer, 0, sizeof(unsigned long long) * ctx->max_sessions, st));
    return 0;
}

// the receive side's per-frame buffers for n frames (under ctx->mu)
int zmtp_frame_cap(zmqg_ctx *ctx, uint64_t n, hipStream_t st)
{
    ZmtpWs &z = ctx->zw;
    if (n <= z.f_cap)
        return 0;
    const uint64_t cap = grown_cap(z.f_cap, 1024, n);
    z.f_cap = 0;
    ZRESERVE(ctx, z.run, 2 * (cap + 1), st);
    ZRESERVE(ctx, z.runpre, cap + 1, st);
    ZRESERVE(ctx, z.sid_fill, cap, st);
    ZRESERVE(ctx, z.fflags, cap, st);
    z.f_cap = cap;
    return 0;
}

} // namespace
