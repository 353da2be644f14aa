// curve_fwd_route.hpp -- zmqg_forward_zmtp_router_multi's part of the plan: what a
// ROUTER does to the messages it proxies.  On its receive side every message
// gets the sending peer's routing id in front (router_t::xrecv,
// src/router.cpp:263-332); on its send side the first part of every message is
// an address, looked up among the peers' routing ids (router_t::xsend,
// src/router.cpp:161-261, lookup_out_pipe, src/socket_base.cpp:2187-2200: a
// std::map<blob_t, out_pipe_t>::find), never sent, and the rest goes to the
// peer it names or nowhere.
//
// The ids are a flat table on the device, sorted as blob_t orders
// (src/blob.hpp:92): the lookup is a lower bound and one compare for equality.
//
//   k_fwd_heads         (curve_fwd_match.hpp) the head of every forwarded element
//   k_fwd_route         one wave per element; the waves of heads stay: the
//                       address's first kFwdTopicWin bytes staged in LDS, the
//                       search wave-uniform (at most 31 steps), each compare
//                       with the lanes over the bytes and a ballot for the
//                       first difference; one verdict word per head
//   k_fwd_pairs_router  one lane per pair of the router pair space: its
//                       element or id slot, the head's verdict, the encode's
//                       frame and dest_out
//
// The entry view (with its void test), fwd_id_less, fwd_id_equal and
// fwd_route_lookup also compile for the host (tests/host/test_fwd_route.cpp);
// only the search for the first differing byte has a wave-cooperative form.
#pragma once
#include "curve_fwd_common.hpp"

namespace zmqg {

constexpr uint32_t kFwdRouteNone = ZMQG_ROUTE_NONE, kFwdRouteAddress = ZMQG_ROUTE_ADDRESS;
constexpr uint32_t kFwdRouteUnknown = ZMQG_ROUTE_UNKNOWN, kFwdRouteMalformed = ZMQG_ROUTE_MALFORMED;

// An address: win holds its first min(len, win_len) bytes (a staged copy);
// bytes at or past win_len are read from p itself.
struct FwdAddr {
    const uint8_t *win;
    uint32_t win_len;
    const uint8_t *p;
    uint32_t len;
    ZMQG_FWD_FN uint8_t at(uint64_t i) const { return i < win_len ? win[i] : p[i]; }
};

// Entry j of a table the host cannot validate.  An entry that does not lie
// within id_bytes[0 .. id_bytes_len) is void: none of its bytes is read, it
// orders as the empty id and equals no address.
struct FwdId {
    const uint8_t *p;
    uint32_t len;
    bool is_void;
};

ZMQG_FWD_FN FwdId fwd_id_view(uint64_t j, const uint64_t *id_off, const uint32_t *id_len, const uint8_t *id_bytes,
                               uint64_t id_bytes_len)
{
    const uint64_t off = id_off[j];
    const uint32_t len = id_len[j];
    FwdId e;
    e.is_void = off > id_bytes_len || len > id_bytes_len - off;
    e.p = e.is_void || !id_bytes ? nullptr : id_bytes + off;
    e.len = e.is_void ? 0u : len;
    return e;
}

// The index of the first byte among the first n at which id and the address
// differ, or n: one byte after the other.
struct FwdSerialDiff {
    ZMQG_FWD_FN uint64_t operator()(const uint8_t *id, const FwdAddr &a, uint64_t n) const
    {
        uint64_t i = 0;
        while (i < n && id[i] == a.at(i))
            ++i;
        return i;
    }
};

// blob_t::operator< (src/blob.hpp:92): memcmp over the shorter length gives
// < 0, or gives 0 and the entry is shorter.
template <class Diff> ZMQG_FWD_FN bool fwd_id_less(const FwdId &e, const FwdAddr &a, const Diff &diff)
{
    const uint64_t n = e.len < a.len ? e.len : a.len;
    const uint64_t d = diff(e.p, a, n);
    return d < n ? e.p[d] < a.at(d) : e.len < a.len;
}

template <class Diff> ZMQG_FWD_FN bool fwd_id_equal(const FwdId &e, const FwdAddr &a, const Diff &diff)
{
    return !e.is_void && e.len == a.len && diff(e.p, a, a.len) == a.len;
}

// The destination the address names, or kFwdRouteUnknown: the lower bound of
// the address under fwd_id_less, found when that entry is the address and names
// a destination below n_dst.  Defined for any table; on one sorted by
// fwd_id_less with distinct ids it is std::map::find.
template <class Diff>
ZMQG_FWD_FN uint32_t fwd_route_lookup(const FwdAddr &a, uint64_t n_ids, const uint64_t *id_off,
                                       const uint32_t *id_len, const uint32_t *id_dst, const uint8_t *id_bytes,
                                       uint64_t id_bytes_len, uint64_t n_dst, const Diff &diff)
{
    uint64_t lo = 0, hi = n_ids;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (fwd_id_less(fwd_id_view(mid, id_off, id_len, id_bytes, id_bytes_len), a, diff))
            lo = mid + 1u;
        else
            hi = mid;
    }
    if (lo >= n_ids || !fwd_id_equal(fwd_id_view(lo, id_off, id_len, id_bytes, id_bytes_len), a, diff))
        return kFwdRouteUnknown;
    const uint32_t t = id_dst[lo];
    return t < n_dst ? t : kFwdRouteUnknown;
}

#if defined(__HIPCC__)

constexpr uint32_t kFwdRouteThreads = 256; // k_fwd_route: 4 waves, an element each
constexpr uint32_t kFwdRouterPrepend = ZMQG_ROUTER_PREPEND, kFwdRouterRoute = ZMQG_ROUTER_ROUTE;

// FwdSerialDiff with the wave's lanes over the bytes, 64 a step (every lane
// calls it with the same arguments and gets the same answer)
struct FwdWaveDiff {
    uint32_t lane;
    __device__ __forceinline__ uint64_t operator()(const uint8_t *id, const FwdAddr &a, uint64_t n) const
    {
        for (uint64_t i0 = 0; i0 < n; i0 += 64u) {
            const uint64_t i = i0 + lane;
            const bool ne = i < n && id[i] != a.at(i);
            const uint64_t m = __builtin_amdgcn_ballot_w64(ne);
            if (m)
                return i0 + (uint64_t) __builtin_ctzll(m);
        }
        return n;
    }
};

// One wave per element e of the element space (ebase as in k_fwd_heads).
// verdict[e], written for forwarded heads only: the destination the message's
// address names, kFwdRouteUnknown, or kFwdRouteMalformed for a head that is its
// whole message.  The address is the head's payload, or with prepend the
// stream's own id (MORE set by definition: never malformed).
__global__ __launch_bounds__(kFwdRouteThreads) void k_fwd_route(
    uint32_t n_elems, FwdSrc src, FwdTab tab, const uint8_t *__restrict__ plain,
    const uint32_t *__restrict__ head, uint32_t prepend, const uint64_t *__restrict__ src_id_off,
    const uint32_t *__restrict__ src_id_len, uint64_t n_ids, const uint64_t *__restrict__ id_off,
    const uint32_t *__restrict__ id_len, const uint32_t *__restrict__ id_dst, const uint8_t *__restrict__ id_bytes,
    uint64_t id_bytes_len, uint64_t n_dst, uint32_t *__restrict__ verdict)
{
    __shared__ uint8_t s_win[kFwdRouteThreads / 64u][kFwdTopicWin];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t e = blockIdx.x * (kFwdRouteThreads / 64u) + w;
    if (e >= n_elems)
        return; // (the whole wave; no barrier below)
    const uint32_t s = fwd_stream_of(tab.ebase, src.n_streams, e), q = e - tab.ebase[s];
    if (q >= src.fwd[s].held_first || head[e] != q)
        return; // not forwarded, or no head
    const FwdElem el = prepend ? fwd_id_part(src_id_off, src_id_len, s) : fwd_elem(src, s, q);
    if (!(el.flags & ZMQG_MSG_MORE)) { // an address that is the whole message: src/router.cpp:168-171, :207-211
        if (lane == 0)
            verdict[e] = kFwdRouteMalformed;
        return;
    }
    uint8_t *win = s_win[w];
    FwdAddr a;
    a.win = win;
    a.win_len = el.len < kFwdTopicWin ? el.len : kFwdTopicWin;
    a.p = plain + el.off;
    a.len = el.len;
    for (uint32_t i = lane; i < a.win_len; i += 64u)
        win[i] = a.p[i];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // (the window is the wave's own: no barrier)
    const uint32_t t = fwd_route_lookup(a, n_ids, id_off, id_len, id_dst, id_bytes, id_bytes_len, n_dst,
                                        FwdWaveDiff{lane});
    if (lane == 0)
        verdict[e] = t;
}

// One lane per pair; prepend alone has id slots, route one route slot a stream
// (curve_fwd_common.hpp).  Destination rule: without route the pair's route, an id part only in front of
// a head; with route the verdict of the message's head, the address part itself
// consumed unless the id part stands for it (prepend).
__global__ __launch_bounds__(256) void k_fwd_pairs_router(
    uint32_t n, FwdSrc src, FwdTab tab, uint32_t rflags, const uint32_t *__restrict__ head,
    const uint32_t *__restrict__ verdict, const uint64_t *__restrict__ src_id_off,
    const uint32_t *__restrict__ src_id_len, FwdPairsOut out, uint32_t *__restrict__ dest_out)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n)
        return;
    const uint32_t s = fwd_stream_of(tab.base, src.n_streams, p);
    const bool route = rflags & kFwdRouterRoute, prepend = rflags & kFwdRouterPrepend;
    // (d > 0: the stream has pairs)
    const uint32_t r0 = route ? 0u : tab.ridx[s], d = route ? 1u : tab.ridx[s + 1] - r0;
    const uint32_t r = p - tab.base[s], slot = r / d, k = r - slot * d;
    const FwdSlot sl = fwd_slot(slot, prepend && !route);
    const FwdElem el = fwd_elem(src, s, sl.q);
    const bool forwarded = sl.q < src.fwd[s].held_first && !(el.flags & ZMQG_MSG_COMMAND);
    // (head[] is written for forwarded elements, verdict[] for their heads only)
    const uint32_t h = forwarded ? head[tab.ebase[s] + sl.q] : kFwdNoHead;
    uint32_t dest = kFwdRouteNone;
    if (forwarded && !route) {
        if (!sl.id_slot || h == sl.q)
            dest = tab.rdst[r0 + k];
    } else if (forwarded) {
        const uint32_t v = verdict[tab.ebase[s] + h];
        if (!prepend && h == sl.q) // the address part: consumed
            dest = v == kFwdRouteMalformed ? kFwdRouteMalformed : kFwdRouteAddress;
        else
            dest = v;
    }
    fwd_store_pair(out, p, dest < kFwdRouteMalformed, dest,
                   sl.id_slot ? fwd_id_part(src_id_off, src_id_len, s) : el);
    if (dest_out)
        dest_out[p] = dest;
}

#endif // __HIPCC__

} // namespace zmqg
