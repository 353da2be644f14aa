#!/usr/bin/env python3
"""Batched handshake key derivation rate on one MI355X: crypto_box_beforenm
(X25519 + HSalsa20) and crypto_scalarmult_base for N random keys, keys/s;
handshake boxes (zmqg_box_afternm_batch / _open_) of HELLO (64 B) and
INITIATE-like (256 B) plaintexts, boxes/s;
the server's HELLO and INITIATE steps as one call each
(zmqg_curve_server_hello_batch / _initiate_batch) beside the same steps
composed from the calls above, handshakes/s, at N and at 1024 connections (an
accept burst), and the client's HELLO and WELCOME -> INITIATE steps
(zmqg_curve_client_hello_batch / _welcome_batch) in the same way;
and the CPU reference for scale (libsodium via the oracle's dlopen is not
exposed, so the oracle's portable C X25519 on one core)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libzmq_amd import curve as C  # noqa: E402


def _median_ms(fns, rounds=5, window=0.25):
    """Median call time in ms of each fn: all warmed up, then `rounds` rounds
    that alternate between them, each timing enough calls to fill `window` s."""
    per = []
    for fn in fns:
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        per.append(max(1, int(window / max(time.perf_counter() - t0, 1e-6))))
    got = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(per[k]):
                fn()
            torch.cuda.synchronize()
            got[k].append((time.perf_counter() - t0) / per[k] * 1e3)
    return [float(np.median(g)) for g in got]


def handshake_lines(ctx, n):
    """Server HELLO and INITIATE for n connections, handshakes/s: the one-call
    forms (zmqg_curve_server_hello_batch / _initiate_batch) and, beside each,
    the same step composed from the library's other batch calls with their
    inputs already gathered (only the launches count) -- HELLO: two beforenm,
    one scalarmult_base, one open, two seals; INITIATE: three opens and one
    beforenm.  Then the client's HELLO and WELCOME -> INITIATE
    (zmqg_curve_client_hello_batch / _welcome_batch) the same way -- HELLO:
    one scalarmult_base, one beforenm, one seal; WELCOME: one open, two
    beforenm, two seals.  The commands are valid handshakes from the model
    (256 distinct ones, repeated)."""
    from tests import curve_handshake_model as M
    rng = np.random.default_rng(5)
    server_sk = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    base = [M.random_handshake(rng, server_sk, meta_len=40) for _ in range(min(n, 256))]
    hs = [base[i % len(base)] for i in range(n)]

    def dev(b):
        a = np.frombuffer(b, np.uint8) if isinstance(b, (bytes, bytearray)) else np.ascontiguousarray(b)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        elif a.dtype == np.uint32:
            a = a.view(np.int32)
        return torch.from_numpy(a.copy()).cuda()

    u8 = lambda size: torch.zeros(size, dtype=torch.uint8, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    idx = np.arange(n, dtype=np.uint64)
    # ---- HELLO
    sk = dev(server_sk)
    cmd = dev(b"".join(h["hello"] for h in hs))
    off, ln = dev(idx * 200), dev(np.full(n, 200, np.uint32))
    rnd = dev(b"".join(h["random"] for h in hs))
    state, wel = u8(128 * n), u8(168 * n)
    fused_hello = lambda: ctx.server_hello_batch(sk, off, ln, cmd, rnd, state, wel, st)
    cpk = dev(b"".join(h["hello"][80:112] for h in hs))
    ssk = dev(server_sk * n)
    sps = dev(b"".join(h["random"][:32] for h in hs))
    k1, spk, pre = u8(32 * n), u8(32 * n), u8(32 * n)
    hbox = dev(b"".join(h["hello"][120:200] for h in hs))
    hnonce = dev(b"".join(b"CurveZMQHELLO---" + h["hello"][112:120] for h in hs))
    cnonce = dev(b"".join(b"COOKIE--" + h["random"][64:80] for h in hs))
    wnonce = dev(b"".join(b"WELCOME-" + h["random"][80:96] for h in hs))
    ckey = dev(b"".join(h["random"][32:64] for h in hs))
    cplain = dev(b"".join(h["state"][:64] for h in hs))
    wplain = dev(rng.integers(0, 256, 128 * n, dtype=np.uint8))
    hplain, cbox, wbox = u8(64 * n), u8(80 * n), u8(144 * n)
    o64, o80, o128, o144 = dev(idx * 64), dev(idx * 80), dev(idx * 128), dev(idx * 144)
    l64, l80, l128 = (dev(np.full(n, v, np.uint32)) for v in (64, 80, 128))

    def composed_hello():
        ctx.box_beforenm_batch(cpk, ssk, k1, st)
        ctx.scalarmult_batch(sps, None, spk, st)
        ctx.box_beforenm_batch(cpk, sps, pre, st)
        ctx.box_open_afternm_batch(k1, hnonce, o80, l80, hbox, o64, hplain, st)
        ctx.box_afternm_batch(ckey, cnonce, o64, l64, cplain, o80, cbox)
        ctx.box_afternm_batch(k1, wnonce, o128, l128, wplain, o144, wbox)

    fused_hello()
    composed_hello()
    torch.cuda.synchronize()
    assert bool((st == 0).all())
    assert wel.cpu().numpy().tobytes() == b"".join(h["welcome"] for h in hs)
    # ---- INITIATE
    istate = dev(b"".join(h["state"] for h in hs))
    ilen = len(hs[0]["initiate"])
    icmd = dev(b"".join(h["initiate"] for h in hs))
    ioff, iln = dev(idx * ilen), dev(np.full(n, ilen, np.uint32))
    ck, ipre, meta = u8(32 * n), u8(32 * n), u8(40 * n)
    peer = torch.zeros(n, dtype=torch.int64, device="cuda")
    mlen = torch.zeros(n, dtype=torch.int32, device="cuda")
    moff = dev(idx * 40)
    fused_initiate = lambda: ctx.server_initiate_batch(istate, ioff, iln, icmd, ck, ipre, peer, moff, meta, mlen, st)
    blen = ilen - 113
    cookie = dev(b"".join(h["initiate"][25:105] for h in hs))
    cn2 = dev(b"".join(b"COOKIE--" + h["initiate"][9:25] for h in hs))
    ibox = dev(b"".join(h["initiate"][113:] for h in hs))
    inonce = dev(b"".join(b"CurveZMQINITIATE" + h["initiate"][105:113] for h in hs))
    pkey = dev(b"".join(h["precom"] for h in hs))
    plains = [O_open(h) for h in hs[:len(base)]]
    plains = [plains[i % len(base)] for i in range(n)]
    cc = dev(b"".join(p[:32] for p in plains))
    vbox = dev(b"".join(p[48:128] for p in plains))
    vnonce = dev(b"".join(b"VOUCH---" + p[32:48] for p in plains))
    kv, cpl, ipl, vpl = u8(32 * n), u8(64 * n), u8((blen - 16) * n), u8(64 * n)
    ob, lb, op = dev(idx * blen), dev(np.full(n, blen, np.uint32)), dev(idx * (blen - 16))

    def composed_initiate():
        ctx.box_open_afternm_batch(ckey, cn2, o80, l80, cookie, o64, cpl, st)
        ctx.box_open_afternm_batch(pkey, inonce, ob, lb, ibox, op, ipl, st)
        ctx.box_beforenm_batch(cc, sps, kv, st)
        ctx.box_open_afternm_batch(kv, vnonce, o80, l80, vbox, o64, vpl, st)

    fused_initiate()
    torch.cuda.synchronize()
    assert bool((st == 0).all()) and ipre.cpu().numpy().tobytes() == b"".join(h["precom"] for h in hs)
    composed_initiate()
    torch.cuda.synchronize()
    assert bool((st == 0).all())
    # ---- client HELLO: composed = scalarmult_base, beforenm, one seal
    from tests import curve_client_model as CM
    srv = dev(b"".join(h["server_pk"] for h in hs))
    cns = dev(b"".join(h["cn_sk"] for h in hs))
    one = dev(np.ones(n, np.uint64))
    cstate, chello = u8(128 * n), u8(200 * n)
    fused_chello = lambda: ctx.client_hello_batch(srv, cns, one, cstate, chello, st)
    cpub, k1c, zeros64, hbox_out = u8(32 * n), u8(32 * n), u8(64 * n), u8(80 * n)

    def composed_chello():
        ctx.scalarmult_batch(cns, None, cpub, st)
        ctx.box_beforenm_batch(srv, cns, k1c, st)
        ctx.box_afternm_batch(k1c, hnonce, o64, l64, zeros64, o80, hbox_out)

    fused_chello()
    composed_chello()
    torch.cuda.synchronize()
    assert bool((st == 0).all())
    assert chello.cpu().numpy().tobytes() == b"".join(h["hello"] for h in hs)
    assert hbox_out.cpu().numpy().tobytes() == b"".join(h["hello"][120:] for h in hs)
    # ---- client WELCOME -> INITIATE: composed = one open, two beforenm, two seals
    cstates = [CM.client_state(h) for h in base]
    wstate = dev(b"".join(cstates[i % len(base)] for i in range(n)))
    lpk, lsk = dev(b"".join(h["client_pk"] for h in hs)), dev(b"".join(h["client_sk"] for h in hs))
    wcmd, woff, wln = dev(b"".join(h["welcome"] for h in hs)), dev(idx * 168), dev(np.full(n, 168, np.uint32))
    vn = dev(b"".join(p[32:48] for p in plains))
    two = dev(np.full(n, 2, np.uint64))
    cmeta, ml40 = dev(b"".join(h["meta"] for h in hs)), dev(np.full(n, 40, np.uint32))
    iout, cpre = u8(ilen * n), u8(32 * n)
    fused_cwelcome = lambda: ctx.client_welcome_batch(wstate, lpk, lsk, woff, wln, wcmd, vn, two, moff, ml40, cmeta,
                                                      ioff, iout, cpre, st)
    k1s = dev(b"".join(cstates[i % len(base)][64:96] for i in range(n)))
    wbox_in = dev(b"".join(h["welcome"][24:] for h in hs))
    wnonce_c = dev(b"".join(b"WELCOME-" + h["welcome"][8:24] for h in hs))
    snpk = dev(b"".join(h["sn_pk"] for h in hs))
    vplain = dev(b"".join(s[0:32] + s[96:128] for s in (cstates[i % len(base)] for i in range(n))))
    iplain = dev(b"".join(plains))
    l144 = dev(np.full(n, 144, np.uint32))
    lp = dev(np.full(n, blen - 16, np.uint32))
    wpl, pre_c, kv_c, vbox_o, ibox_o = u8(128 * n), u8(32 * n), u8(32 * n), u8(80 * n), u8(blen * n)

    def composed_cwelcome():
        ctx.box_open_afternm_batch(k1s, wnonce_c, o144, l144, wbox_in, o128, wpl, st)
        ctx.box_beforenm_batch(snpk, cns, pre_c, st)
        ctx.box_beforenm_batch(snpk, lsk, kv_c, st)
        ctx.box_afternm_batch(kv_c, vnonce, o64, l64, vplain, o80, vbox_o)
        ctx.box_afternm_batch(pre_c, inonce, op, lp, iplain, ob, ibox_o)

    fused_cwelcome()
    torch.cuda.synchronize()
    assert bool((st == 0).all()) and iout.cpu().numpy().tobytes() == b"".join(h["initiate"] for h in hs)
    assert cpre.cpu().numpy().tobytes() == b"".join(h["precom"] for h in hs)
    composed_cwelcome()
    torch.cuda.synchronize()
    assert bool((st == 0).all()) and ibox_o.cpu().numpy().tobytes() == b"".join(h["initiate"][113:] for h in hs)
    for name, fused, composed in (("server HELLO", fused_hello, composed_hello),
                                  ("server INITIATE", fused_initiate, composed_initiate),
                                  ("client HELLO", fused_chello, composed_chello),
                                  ("client WELCOME", fused_cwelcome, composed_cwelcome)):
        f, c = _median_ms([fused, composed])
        print(f"{name:16s} {n} conns  one call {f:8.3f} ms {n / f / 1e3:8.3f} M handshakes/s   "
              f"composed {c:8.3f} ms {n / c / 1e3:8.3f} M/s   ratio {c / f:5.2f}")


def O_open(h):
    """The INITIATE box's plaintext of a model handshake (C | vouch | metadata)."""
    from oracle import oracle as O
    rc, plain = O.box_open_easy_afternm(h["initiate"][113:], b"CurveZMQINITIATE" + h["initiate"][105:113], h["precom"])
    assert rc == 0
    return plain


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    rng = np.random.default_rng(1)
    pk = torch.from_numpy(rng.integers(0, 256, 32 * n, dtype=np.uint8)).cuda()
    sk = torch.from_numpy(rng.integers(0, 256, 32 * n, dtype=np.uint8)).cuda()
    k = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx = C.CurveContext(0, 1)
    for name, fn in (("beforenm", lambda: ctx.box_beforenm_batch(pk, sk, k, st)),
                     ("scalarmult_base", lambda: ctx.scalarmult_batch(sk, None, k, st))):
        fn()
        torch.cuda.synchronize()
        reps = 3
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        print(f"{name:16s} {n} keys  {dt * 1e3:8.2f} ms  {n / dt / 1e6:6.3f} M keys/s")
    key = torch.from_numpy(rng.integers(0, 256, 32 * n, dtype=np.uint8)).cuda()
    nonce = torch.from_numpy(rng.integers(0, 256, 24 * n, dtype=np.uint8)).cuda()
    for L in (64, 256):
        i = torch.arange(n, device="cuda", dtype=torch.int64)
        m = torch.from_numpy(rng.integers(0, 256, L * n, dtype=np.uint8)).cuda()
        box = torch.zeros((L + 16) * n, dtype=torch.uint8, device="cuda")
        back = torch.zeros(L * n, dtype=torch.uint8, device="cuda")
        ln = torch.full((n,), L, dtype=torch.int32, device="cuda")
        lb = torch.full((n,), L + 16, dtype=torch.int32, device="cuda")
        for name, fn in (("box seal %d B" % L,
                          lambda: ctx.box_afternm_batch(key, nonce, i * L, ln, m, i * (L + 16), box)),
                         ("box open %d B" % L,
                          lambda: ctx.box_open_afternm_batch(key, nonce, i * (L + 16), lb, box, i * L, back, st))):
            fn()
            torch.cuda.synchronize()
            reps = 5
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / reps
            print(f"{name:16s} {n} boxes {dt * 1e3:8.3f} ms  {n / dt / 1e6:6.2f} M boxes/s")
        assert bool((st == 0).all()) and torch.equal(back, m)
    for hn in sorted({n, 1024}):
        handshake_lines(ctx, hn)
    from oracle import oracle as O
    m = 200
    t0 = time.perf_counter()
    for i in range(m):
        O.box_beforenm(bytes(pk[32 * i:32 * i + 32].cpu().numpy()), bytes(sk[32 * i:32 * i + 32].cpu().numpy()))
    dt = time.perf_counter() - t0
    print(f"oracle beforenm (portable C, 1 core): {m / dt / 1e3:.1f} k keys/s")


if __name__ == "__main__":
    main()
