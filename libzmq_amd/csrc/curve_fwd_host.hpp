// curve_fwd_host.hpp -- the host path of the forward calls: forward_begin,
// the entry's own fwd_plan_*, forward_finish ("Forwarding").  Part of
// zmqg_curve.hip, included there after the receive and send sides it queues.
#pragma once
#include "curve_fwd_common.hpp"
#include "curve_fwd_credit.hpp"
#include "curve_fwd_lb_credit.hpp"

static_assert(kFwdNoStream == kZsendNoSession, "curve_fwd_common.hpp restates the send side's value");

// The framing of the two sides (ZMQG_FRAMING_*): what decodes the receive
// buffers, what encodes the send runs.  The plan between them reads slots and
// fwd[s] only, which either decoder fills alike.  The four zmqg_forward_zmtp_*
// entries pass kFwdFramingZmtp; zmqg_forward_framed_multi the caller's choice.
struct FwdFraming {
    uint32_t recv, send;
    zmqg_ws_result *ws_results; // recv != ZMTP: takes the place of args->results
    const uint32_t *mask;       // send == WS_MASKED: one key per pair
    bool ws_recv() const { return recv != ZMQG_FRAMING_ZMTP; }
};
static const FwdFraming kFwdFramingZmtp = {ZMQG_FRAMING_ZMTP, ZMQG_FRAMING_ZMTP, nullptr, nullptr};

struct FwdCall {
    std::unique_lock<std::mutex> lk; // ctx->mu, from forward_begin to the end of the call
    const zmqg_forward_zmtp *a;
    hipStream_t st;
    FwdFraming fr;
    FwdTableDims t; // t.N pairs, t.EN elements of the routed streams
    FwdTab tab;
    FwdSrc src;
    FwdPairsOut out;
    const zmqg_forward_credit *credit = nullptr; // zmqg_forward_credit_multi: the pass in front of the send side
    bool credit_in_plan = false; // zmqg_forward_lb_credit_multi: the plan has applied the credits itself, no pass
    bool empty() const { return a->n_streams == 0; } // nothing to queue
};

static int forward_begin(zmqg_ctx *ctx, const FwdTableIn &in, const FwdFraming &fr, void *stream, FwdCall &c)
{
    const zmqg_forward_zmtp *args = in.a;
    if (!ctx || !args || args->size != sizeof *args || args->reserved != 0)
        return -EINVAL;
    const zmqg_forward_zmtp &a = *args;
    const uint64_t S = a.n_streams, MF = a.max_frames;
    // the two underlying calls' own cases (the results array is the receive framing's)
    if ((fr.ws_recv() ? S > 0 && !fr.ws_results : !a.results) || check_n(S) || check_n(MF) || check_n(S * MF))
        return -EINVAL;
    if (a.n_dst > kZsendMaxStreams || ctx->max_sessions > kReplayMaxSessions)
        return -EINVAL;
    hipStream_t st = (hipStream_t) stream;
    ZCHECK(ctx, hipSetDevice(ctx->device));
    c.a = args;
    c.st = st;
    c.fr = fr;
    if (S == 0)
        return 0;
    if (MF > 0 && (!a.stream_sid || !a.stream_off || !a.stream_len || !a.in || !a.frame_in_off || !a.frame_len ||
                   !a.plain_off || !a.plain || !a.flags_out || !a.status_out))
        return -EINVAL;
    if (!a.pair_off || !a.fwd || (a.n_dst > 0 && (!a.dst_sid || !a.dst_results)))
        return -EINVAL;
    FwdTableDims &t = c.t;
    int rc;
    if ((rc = fwd_table_dims(in, t)))
        return rc;
    const uint64_t N = t.N;
    if (a.carry_idx && a.carry_idx[S] > 0 && (!a.carry_off || !a.carry_len || !a.carry_flags))
        return -EINVAL;
    if (N > 0 && (!a.plain || !a.out || (fr.send == ZMQG_FRAMING_WS_MASKED && !fr.mask)))
        return -EINVAL;
    // (the send side's own case: frames and no streams; routes cannot name none)
    if (in.one_route && N > 0 && a.n_dst == 0)
        return -EINVAL;
    c.lk = std::unique_lock<std::mutex>(ctx->mu);
    ZmtpWs &z = ctx->zw;
    if ((rc = order_after_last(ctx, st)))
        return rc;
    // the host arrays, copied before the call returns: the pinned staging, then
    // one copy to the device
    if ((rc = sinst_room(ctx, 4 * (size_t) t.words)))
        return rc;
    fwd_table_fill(in, t, (uint32_t *) ctx->sinst);
    ZRESERVE(ctx, z.p_tab, grown_cap(z.p_tab.count, 1024, t.words), st);
    ZCHECK(ctx, hipMemcpyAsync(z.p_tab, ctx->sinst, 4 * (size_t) t.words, hipMemcpyHostToDevice, st));
    ZCHECK(ctx, hipEventRecord(ctx->sinst_done, st));
    if ((rc = reserve_group(ctx, st, "p_stream..p_len", z.p_cap, 1024, N, z.p_stream, z.p_flags, z.p_off, z.p_len)))
        return rc;
    c.tab = fwd_tab(z.p_tab, S, t);
    c.src = FwdSrc{(uint32_t) S, MF,          c.tab.cidx,  a.carry_off,  a.carry_len, a.carry_flags,
                   a.plain_off,  a.frame_len, a.flags_out, a.status_out, a.fwd};
    c.out = FwdPairsOut{z.p_stream, z.p_flags, z.p_off, z.p_len};
    return 0;
}

// The receive side in its framing, then what each stream forwards
static int forward_receive(zmqg_ctx *ctx, const FwdCall &c)
{
    const zmqg_forward_zmtp &a = *c.a;
    const uint64_t S = a.n_streams, MF = a.max_frames;
    const dim3 grid(wave_grid(S, kFwdThreads)), block(kFwdThreads);
    int rc;
    if (c.fr.ws_recv()) {
        zmqg_ws_result *res = c.fr.ws_results;
        if (MF == 0)
            ZCHECK(ctx, hipMemsetAsync(res, 0, S * sizeof *res, c.st));
        else if ((rc = decode_ws_multi_locked(ctx, S, a.stream_sid, a.stream_off, a.stream_len, a.in,
                                              c.fr.recv == ZMQG_FRAMING_WS_MASKED, a.max_msg_size, MF, a.frame_in_off,
                                              a.frame_len, a.plain_off, a.plain, a.flags_out, a.status_out, res,
                                              c.st)))
            return rc;
        hipLaunchKernelGGL(k_fwd_scan<zmqg_ws_result>, grid, block, 0, c.st, c.src, (const zmqg_ws_result *) res,
                           a.fwd);
    } else {
        if (MF == 0)
            ZCHECK(ctx, hipMemsetAsync(a.results, 0, S * sizeof *a.results, c.st));
        else if ((rc = decode_zmtp_multi_locked(ctx, S, a.stream_sid, a.stream_off, a.stream_len, a.in,
                                                a.max_msg_size, MF, a.frame_in_off, a.frame_len, a.plain_off, a.plain,
                                                a.flags_out, a.status_out, a.results, c.st)))
            return rc;
        hipLaunchKernelGGL(k_fwd_scan<zmqg_zmtp_result>, grid, block, 0, c.st, c.src,
                           (const zmqg_zmtp_result *) a.results, a.fwd);
    }
    ZCHECK(ctx, hipGetLastError());
    return 0;
}

// The send side in its framing: the pairs are its frames, the destinations its
// streams, a masked pair's key mask[p]
extern "C++" template <ZsendFraming FR>
static int forward_send(zmqg_ctx *ctx, const FwdCall &c, const uint32_t *mask)
{
    const zmqg_forward_zmtp &a = *c.a;
    return encode_multi_locked<FR>(ctx, a.n_dst, a.dst_sid, c.t.N, c.out.p_stream, nullptr, c.out.p_flags, c.out.p_off,
                                   c.out.p_len, a.plain, mask, a.out, a.out_bytes, a.pair_off, a.pair_status,
                                   a.dst_results, c.st);
}

// The pair space of the plan, as zmqg_forward_credit_multi's pass reads it
// (FwdCreditSpace, curve_fwd_credit.hpp, without the arrays)
struct FwdCreditMode {
    bool twice, one_route, addr;
};

// zmqg_forward_credit_multi between the plan and the send side: the starts and
// their counts per tile, the column passes, the ranks, the verdict on every
// pair, the totals (curve_fwd_credit.hpp).  Without pairs the totals are zeros.
static int fwd_credit_pass(zmqg_ctx *ctx, const FwdCall &c, const FwdCreditMode &cm)
{
    const zmqg_forward_credit &cr = *c.credit;
    ZmtpWs &z = ctx->zw;
    const uint32_t N = (uint32_t) c.t.N, D = (uint32_t) c.a->n_dst;
    if (D == 0)
        return 0;
    if (N == 0) {
        ZCHECK(ctx, hipMemsetAsync(cr.dst_taken, 0, 4 * (size_t) D, c.st));
        ZCHECK(ctx, hipMemsetAsync(cr.dst_dropped, 0, 4 * (size_t) D, c.st));
        return 0;
    }
    const uint32_t T = zsend_tile_frames(N, D); // (kFwdCreditTile until the table outgrows its bounds)
    const uint32_t tiles = (N + T - 1) / T, rbs = (tiles + kFwdCreditRB - 1) / kFwdCreditRB;
    int rc;
    if ((rc = reserve_group(ctx, c.st, "p_key..p_hwm", z.k_cap, 1024, N, z.p_key, z.p_rank, z.p_hwm)))
        return rc;
    const size_t need = ((size_t) tiles + rbs + 1) * D; // counts, block sums, totals
    ZRESERVE(ctx, z.k_tab, grown_cap(z.k_tab.count, 4096, need), c.st);
    uint32_t *cnt = z.k_tab, *blk = cnt + (size_t) tiles * D, *tot = blk + (size_t) rbs * D;
    const FwdCreditSpace sp = {cm.twice, cm.one_route, cm.addr, z.e_head.p, z.e_verdict.p};
    const dim3 cg((D + 255) / 256, rbs), pg((N + 255) / 256);
    hipLaunchKernelGGL(k_fwd_credit_tiles, dim3(tiles), dim3(256), D * sizeof(uint32_t), c.st, N, T, D, c.src, c.tab,
                       sp, (const uint32_t *) c.out.p_stream, z.p_key.p, cnt, tot);
    ZCHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fwd_credit_colblk, cg, dim3(256), 0, c.st, tiles, D, (const uint32_t *) cnt, blk, tot);
    ZCHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fwd_credit_colscan, cg, dim3(256), 0, c.st, tiles, D, cnt, (const uint32_t *) blk);
    ZCHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fwd_credit_ranks, dim3(tiles), dim3(kFwdCreditThreads), D * sizeof(uint32_t), c.st, N, T, D,
                       (const uint32_t *) z.p_key.p, (const uint32_t *) cnt, z.p_rank.p);
    ZCHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fwd_credit_apply, pg, dim3(256), 0, c.st, N, D, c.src, c.tab, sp,
                       (const uint32_t *) z.p_key.p, (const uint32_t *) z.p_rank.p,
                       (const uint32_t *) cr.dst_credit, c.out, z.p_hwm.p);
    ZCHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fwd_credit_totals, dim3((D + 255) / 256), dim3(256), 0, c.st, D, (const uint32_t *) tot,
                       cr.dst_credit, cr.dst_taken, cr.dst_dropped, cr.flags & ZMQG_CREDIT_CONSUME);
    ZCHECK(ctx, hipGetLastError());
    return 0;
}

// The send side; in front of it zmqg_forward_credit_multi's pass, and behind it
// ZMQG_ERR_HWM for the pairs the pass cleared (or, for
// zmqg_forward_lb_credit_multi, the pairs the plan left without a destination)
static int forward_finish(zmqg_ctx *ctx, const FwdCall &c, const FwdCreditMode &cm = FwdCreditMode())
{
    const zmqg_forward_zmtp &a = *c.a;
    int rc;
    if (c.credit && !c.credit_in_plan && (rc = fwd_credit_pass(ctx, c, cm)))
        return rc;
    if (a.n_dst == 0) {
        ZCHECK(ctx, hipMemsetAsync(a.pair_off, 0, sizeof(uint64_t), c.st));
        return 0;
    }
    if (c.fr.send == ZMQG_FRAMING_WS_MASKED)
        rc = forward_send<kZsendWsMasked>(ctx, c, c.fr.mask);
    else if (c.fr.send == ZMQG_FRAMING_WS)
        rc = forward_send<kZsendWs>(ctx, c, nullptr);
    else
        rc = forward_send<kZsendZmtp>(ctx, c, nullptr);
    if (rc || !c.credit || !a.pair_status || c.t.N == 0)
        return rc;
    hipLaunchKernelGGL(k_fwd_credit_status, dim3((unsigned) ((c.t.N + 255) / 256)), dim3(256), 0, c.st,
                       (uint32_t) c.t.N, (const uint8_t *) ctx->zw.p_hwm.p, a.pair_status);
    ZCHECK(ctx, hipGetLastError());
    return 0;
}

// zmqg_forward_zmtp_multi: the pairs (one lane per pair); in front of them, for
// zmqg_forward_credit_multi alone, the heads (the table then has its ebase row)
static int fwd_plan_static(zmqg_ctx *ctx, const FwdCall &c)
{
    ZmtpWs &z = ctx->zw;
    const uint64_t S = c.src.n_streams, N = c.t.N;
    int rc;
    if (c.credit && (rc = reserve_group(ctx, c.st, "e_head", z.e_cap, 1024, c.t.EN, z.e_head)))
        return rc;
    if ((rc = forward_receive(ctx, c)) || N == 0)
        return rc;
    if (c.credit) {
        hipLaunchKernelGGL(k_fwd_heads<false>, dim3(wave_grid(S, kFwdThreads)), dim3(kFwdThreads), 0, c.st, c.src,
                           c.tab, z.e_head.p, nullptr, nullptr);
        ZCHECK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_fwd_pairs<false>, dim3((unsigned) ((N + 255) / 256)), dim3(256), 0, c.st, (uint32_t) N, c.src,
                       c.tab, c.out, nullptr, nullptr, nullptr);
    ZCHECK(ctx, hipGetLastError());
    return 0;
}

// zmqg_forward_zmtp_sub_multi: the heads (one wave per source stream), each
// head's topic against its routes' subscriptions (one wave per element; N > 0:
// EN > 0), the pairs
static int fwd_plan_sub(zmqg_ctx *ctx, const FwdCall &c, const zmqg_forward_subs &subs)
{
    ZmtpWs &z = ctx->zw;
    const uint64_t S = c.src.n_streams, N = c.t.N, EN = c.t.EN;
    int rc;
    if ((rc = reserve_group(ctx, c.st, "p_match", z.m_cap, 1024, N, z.p_match)) ||
        (rc = reserve_group(ctx, c.st, "e_head", z.e_cap, 1024, EN, z.e_head)))
        return rc;
    if ((rc = forward_receive(ctx, c)) || N == 0)
        return rc;
    hipLaunchKernelGGL(k_fwd_heads<false>, dim3(wave_grid(S, kFwdThreads)), dim3(kFwdThreads), 0, c.st, c.src, c.tab,
                       z.e_head.p, nullptr, nullptr);
    ZCHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fwd_match, dim3(wave_grid(EN, kFwdMatchThreads)), dim3(kFwdMatchThreads), 0, c.st,
                       (uint32_t) EN, c.src, c.tab, c.a->plain, z.e_head.p, (uint32_t) subs.n_subs, subs.sub_idx,
                       subs.sub_off, subs.sub_len, subs.sub_bytes, subs.sub_bytes_len, subs.flags & ZMQG_SUBS_INVERT,
                       z.p_match.p);
    ZCHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fwd_pairs<true>, dim3((unsigned) ((N + 255) / 256)), dim3(256), 0, c.st, (uint32_t) N, c.src,
                       c.tab, c.out, z.e_head.p, z.p_match.p, subs.match_out);
    ZCHECK(ctx, hipGetLastError());
    return 0;
}

// zmqg_forward_zmtp_router_multi with a flag set: the heads; with ROUTE the
// lookup of every head's address (one wave per element; N > 0: EN > 0); the
// router pair space
static int fwd_plan_router(zmqg_ctx *ctx, const FwdCall &c, const zmqg_forward_router &rt)
{
    ZmtpWs &z = ctx->zw;
    const bool route = rt.flags & ZMQG_ROUTER_ROUTE;
    const uint64_t S = c.src.n_streams, N = c.t.N, EN = c.t.EN;
    int rc;
    if ((rc = reserve_group(ctx, c.st, "e_head", z.e_cap, 1024, EN, z.e_head)) ||
        (route && (rc = reserve_group(ctx, c.st, "e_verdict", z.v_cap, 1024, EN, z.e_verdict))))
        return rc;
    if ((rc = forward_receive(ctx, c)) || N == 0)
        return rc;
    hipLaunchKernelGGL(k_fwd_heads<false>, dim3(wave_grid(S, kFwdThreads)), dim3(kFwdThreads), 0, c.st, c.src, c.tab,
                       z.e_head.p, nullptr, nullptr);
    ZCHECK(ctx, hipGetLastError());
    if (route) {
        hipLaunchKernelGGL(k_fwd_route, dim3(wave_grid(EN, kFwdRouteThreads)), dim3(kFwdRouteThreads), 0, c.st,
                           (uint32_t) EN, c.src, c.tab, c.a->plain, z.e_head.p, rt.flags & ZMQG_ROUTER_PREPEND,
                           rt.src_id_off, rt.src_id_len, rt.n_ids, rt.id_off, rt.id_len, rt.id_dst, rt.id_bytes,
                           rt.id_bytes_len, c.a->n_dst, z.e_verdict.p);
        ZCHECK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_fwd_pairs_router, dim3((unsigned) ((N + 255) / 256)), dim3(256), 0, c.st, (uint32_t) N, c.src,
                       c.tab, rt.flags, z.e_head.p, z.e_verdict.p, rt.src_id_off, rt.src_id_len, c.out, rt.dest_out);
    ZCHECK(ctx, hipGetLastError());
    return 0;
}

// zmqg_forward_zmtp_lb_multi: the heads with the rank of every message within
// its stream, every stream's ring position and every group's new cursor, the
// pairs (one wave per source stream; one wave per group; one lane per pair).
// Without pairs the groups alone, which then only clamp the cursors.
static int fwd_plan_lb(zmqg_ctx *ctx, const FwdCall &c, const zmqg_forward_lb &lb)
{
    ZmtpWs &z = ctx->zw;
    const uint64_t S = c.src.n_streams, G = lb.n_groups, N = c.t.N, EN = c.t.EN;
    const uint32_t *sgrp = c.tab.rdst, *gidx = sgrp + S, *gstr = gidx + (G + 1);
    int rc;
    if ((rc = reserve_group(ctx, c.st, "e_rank", z.l_cap, 1024, EN, z.e_rank)) ||
        (rc = reserve_group(ctx, c.st, "s_msgs, s_first", z.ls_cap, 1024, S, z.s_msgs, z.s_first)) ||
        (rc = reserve_group(ctx, c.st, "e_head", z.e_cap, 1024, EN, z.e_head)))
        return rc;
    if ((rc = forward_receive(ctx, c)))
        return rc;
    if (N > 0) {
        hipLaunchKernelGGL(k_fwd_heads<true>, dim3(wave_grid(S, kFwdThreads)), dim3(kFwdThreads), 0, c.st, c.src,
                           c.tab, z.e_head.p, z.e_rank.p, z.s_msgs.p);
        ZCHECK(ctx, hipGetLastError());
    }
    if (G > 0) {
        hipLaunchKernelGGL(k_fwd_lb_groups, dim3(wave_grid(G, kFwdThreads)), dim3(kFwdThreads), 0, c.st, (uint32_t) G,
                           gidx, gstr, N > 0 ? z.s_msgs.p : nullptr, lb.grp_idx, (uint32_t) lb.n_lb, lb.lb_cur,
                           z.s_first.p);
        ZCHECK(ctx, hipGetLastError());
    }
    if (N > 0) {
        hipLaunchKernelGGL(k_fwd_pairs_lb, dim3((unsigned) ((N + 255) / 256)), dim3(256), 0, c.st, (uint32_t) N, c.src,
                           c.tab, lb.flags & ZMQG_LB_PREPEND, sgrp, z.e_head.p, z.e_rank.p, z.s_first.p, lb.grp_idx,
                           (uint32_t) lb.n_lb, lb.lb_dst, c.a->n_dst, lb.src_id_off, lb.src_id_len, c.out,
                           lb.dest_out);
        ZCHECK(ctx, hipGetLastError());
    }
    return 0;
}

// zmqg_forward_lb_credit_multi: fwd_plan_lb with the choice made under the
// credits (curve_fwd_lb_credit.hpp): the heads, one workgroup per group for the
// epochs, the pairs, the totals.  X(t) is zeroed on the stream in front of them.
// Without pairs the totals are zeros and k_fwd_lb_groups clamps the cursors.
static int fwd_plan_lb_credit(zmqg_ctx *ctx, const FwdCall &c, const zmqg_forward_lb &lb)
{
    ZmtpWs &z = ctx->zw;
    const zmqg_forward_credit &cr = *c.credit;
    const uint64_t S = c.src.n_streams, G = lb.n_groups, N = c.t.N, EN = c.t.EN;
    const uint32_t D = (uint32_t) c.a->n_dst;
    const uint32_t *sgrp = c.tab.rdst, *gidx = sgrp + S, *gstr = gidx + (G + 1);
    int rc;
    if ((rc = reserve_group(ctx, c.st, "e_rank", z.l_cap, 1024, EN, z.e_rank)) ||
        (rc = reserve_group(ctx, c.st, "s_msgs, s_first", z.ls_cap, 1024, S, z.s_msgs, z.s_first)) ||
        (rc = reserve_group(ctx, c.st, "e_head", z.e_cap, 1024, EN, z.e_head)) ||
        (rc = reserve_group(ctx, c.st, "e_pick", z.lc_cap, 1024, EN, z.e_pick)) ||
        (rc = reserve_group(ctx, c.st, "r_orig, r_w", z.lr_cap, 1024, lb.n_lb, z.r_orig, z.r_w)) ||
        (rc = reserve_group(ctx, c.st, "p_key..p_hwm", z.k_cap, 1024, N, z.p_key, z.p_rank, z.p_hwm)))
        return rc;
    ZRESERVE(ctx, z.x_tot, grown_cap(z.x_tot.count, 1024, D), c.st);
    if ((rc = forward_receive(ctx, c)))
        return rc;
    if (N == 0) {
        if (G > 0) {
            hipLaunchKernelGGL(k_fwd_lb_groups, dim3(wave_grid(G, kFwdThreads)), dim3(kFwdThreads), 0, c.st,
                               (uint32_t) G, gidx, gstr, nullptr, lb.grp_idx, (uint32_t) lb.n_lb, lb.lb_cur,
                               z.s_first.p);
            ZCHECK(ctx, hipGetLastError());
        }
        if (D > 0) {
            ZCHECK(ctx, hipMemsetAsync(cr.dst_taken, 0, 4 * (size_t) D, c.st));
            ZCHECK(ctx, hipMemsetAsync(cr.dst_dropped, 0, 4 * (size_t) D, c.st));
        }
        return 0;
    }
    // (N > 0: forward_begin has seen to n_dst > 0)
    ZCHECK(ctx, hipMemsetAsync(z.x_tot.p, 0, 4 * (size_t) D, c.st));
    hipLaunchKernelGGL(k_fwd_heads<true>, dim3(wave_grid(S, kFwdThreads)), dim3(kFwdThreads), 0, c.st, c.src, c.tab,
                       z.e_head.p, z.e_rank.p, z.s_msgs.p);
    ZCHECK(ctx, hipGetLastError());
    if (G > 0) {
        hipLaunchKernelGGL(k_fwd_lb_credit_groups, dim3((unsigned) G), dim3(kFwdThreads), 0, c.st, gidx, gstr,
                           (const uint32_t *) z.s_msgs.p, (const uint32_t *) c.tab.ebase, lb.grp_idx,
                           (uint32_t) lb.n_lb, lb.lb_dst, D, (const uint32_t *) cr.dst_credit, lb.lb_cur, z.s_first.p,
                           z.r_orig.p, z.r_w.p, z.e_pick.p, z.x_tot.p);
        ZCHECK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_fwd_pairs_lb_credit, dim3((unsigned) ((N + 255) / 256)), dim3(256), 0, c.st, (uint32_t) N,
                       c.src, c.tab, lb.flags & ZMQG_LB_PREPEND, sgrp, z.e_head.p, z.e_rank.p,
                       (const uint32_t *) z.e_pick.p, lb.grp_idx, (uint32_t) lb.n_lb, lb.src_id_off, lb.src_id_len,
                       c.out, lb.dest_out, z.p_hwm.p);
    ZCHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fwd_credit_totals, dim3((D + 255) / 256), dim3(256), 0, c.st, D,
                       (const uint32_t *) z.x_tot.p, cr.dst_credit, cr.dst_taken, cr.dst_dropped,
                       cr.flags & ZMQG_CREDIT_CONSUME);
    ZCHECK(ctx, hipGetLastError());
    return 0;
}
