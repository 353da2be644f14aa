"""CPU restatement of zmqg_decode_zmtp's parser (libzmq_amd/csrc/curve_zmtp.hpp:
k_zmtp_scan, k_zmtp_compact, k_zmtp_next_walk, k_zmtp_frames), with the
kernels' geometry: 16-byte chunks, four rounds of 256 lanes, one list per
16 KiB tile, the tiles cut in 16-byte-aligned address space (`mis` = the
stream's first byte's address modulo 16).  TEST INFRASTRUCTURE ONLY.

decode() returns the call's result and frames plus the coverage facts the
steered tests assert (tests/zmtp_scan_steer.py): which edges of the scan, the
links and the walk a stream reaches is decided here, never by the kernel.
Signatures are found with bytes.find, everything else is per candidate, so a
128 MiB stream of a few frames costs what its candidates cost."""
import functools
import struct

CHUNK = 16
LANES = 256            # kZmtpThreads
NEXT_THREADS = 1024    # kZmtpNextThreads
SUFFIX_REGS = 8        # zmtp_suffix_min's R
INLINE_SUM_LISTS = 8192
NONE = (1 << 64) - 1
LARGE = 2
EMSGSIZE = 90
MESSAGE = b"\x07MESSAGE"

# switches the discrimination checks flip (tests/test_zmtp_scan_model.py)
SHADOW_RULE = True
SUFFIX_MIN = True
AFTER_ALL_LISTS = True


@functools.lru_cache(maxsize=None)
def tile():
    """kZmtpWgBytes, from the binding (tests/test_abi_zmtp_scan.py pins it to
    the kernel's).  Not taken at import: the GPU tests load torch's HIP
    runtime before the library's."""
    from libzmq_amd import curve
    assert curve.ZMTP_SCAN_TILE % (CHUNK * LANES) == 0
    return curve.ZMTP_SCAN_TILE


def size_ok(size, max_msg):
    if max_msg >= 0 and size > max_msg:
        return False
    return size <= 0xFFFFFFFF


def header(b, n, p):
    """zmtp_header: (hdr, size) or None when the header is not complete."""
    if p + 2 > n:
        return None
    if b[p] & LARGE:
        if p + 9 > n:
            return None
        return 9, struct.unpack(">Q", b[p + 1:p + 9])[0]
    return 2, b[p + 1]


def load_path(ci, n, mis):
    """zmtp_scan_load's path for chunk ci (aligned address space): the three
    vector loads when the 16 bytes before the chunk, the chunk and the 8
    bytes after it lie inside the stream, else byte by byte."""
    ub = CHUNK * ci
    return "fast" if ub >= 16 + mis and ub + 24 <= mis + n else "bytewise"


def cand_at(b, n, q, max_msg):
    """zmtp_cand_at for the signature at q: (p, kind, shadow) -- the frame
    start, 'large' / 'short', and whether q - 2 passed as a short header too
    and was dropped for the LARGE one."""
    short = None
    if q >= 2 and not b[q - 2] & LARGE:
        size, p = b[q - 1], q - 2
        if size_ok(size, max_msg) and size >= 8 and size <= n - p - 2:
            short = p
    if q >= 9 and b[q - 9] & LARGE:
        size, p = struct.unpack(">Q", b[q - 8:q])[0], q - 9
        if size_ok(size, max_msg) and size >= 8 and size <= n - p - 9:
            if SHADOW_RULE:
                return p, "large", short is not None
            if short is None:
                return p, "large", False
            return (p, "large", False), (short, "short", False)  # (rule off: both)
    if short is not None:
        return short, "short", False
    return None


def scan(b, n, max_msg, mis):
    """k_zmtp_scan: the per-tile lists and the facts of the scan."""
    TILE = tile()
    WG_CAP = TILE // 8  # kZmtpWgCap
    nwg = (mis + n + TILE - 1) // TILE
    lists = [[] for _ in range(nwg)]
    cands, per_chunk = [], {}
    shadows, dropped_at, sig_chunks = 0, set(), {}
    q = b.find(MESSAGE)
    while q >= 0:
        ci = (q + mis) // CHUNK
        sig_chunks[ci] = sig_chunks.get(ci, 0) + 1
        r = cand_at(b, n, q, max_msg)
        found = [] if r is None else (list(r) if isinstance(r[0], tuple) else [r])
        for p, kind, shadow in found:
            if shadow:
                shadows += 1
                dropped_at.add(q - 2)
            if per_chunk.get(ci, 0) >= 2:  # (f[k][2]: never reached, signatures are >= 8 apart)
                continue
            per_chunk[ci] = per_chunk.get(ci, 0) + 1
            w = ci // (TILE // CHUNK)
            lists[w].append(p)
            cands.append(dict(p=p, q=q, kind=kind, chunk=ci, lane=ci % LANES, round=ci // LANES % (TILE // CHUNK // LANES), list=w,
                              path=load_path(ci, n, mis),
                              hdr_chunk=(p + mis) // CHUNK, tail_chunk=(q + 7 + mis) // CHUNK))
        q = b.find(MESSAGE, q + 1)
    for l in lists:
        assert len(l) <= WG_CAP and l == sorted(set(l))
    return nwg, lists, dict(cands=cands, shadows_dropped=shadows, dropped_at=dropped_at,
                            two_in_chunk=any(v == 2 for v in per_chunk.values()),
                            two_sigs_in_chunk=any(v == 2 for v in sig_chunks.values()),
                            max_list_count=max([len(l) for l in lists] or [0]))


def compact(b, n, nwg, lists):
    """k_zmtp_compact: the candidate array, each candidate's frame, and the
    links: nb per candidate, first_w per list."""
    counts = [len(l) for l in lists]
    off = [0] * (nwg + 1)
    for w in range(nwg):
        off[w + 1] = off[w] + counts[w]  # (count16 sums or the hipCUB scan: the same numbers)
    m = off[nwg]
    cand, wid, cdesc, cflag, nb = [0] * m, [0] * m, [0] * m, [0] * m, [NONE] * m
    unl = [False] * m
    first_w = [NONE] * nwg
    max_skip, max_passes = 0, 0
    for w in range(nwg):
        c, o, lst = counts[w], off[w], lists[w]
        after, ws = NONE, w + 1
        while c > 0 and ws < nwg:  # 64 lists' counts at a time
            nz = [x for x in range(ws, min(ws + 64, nwg)) if counts[x]]
            if nz:
                after = lists[nz[0]][0]
                max_skip = max(max_skip, nz[0] - (w + 1))
                break
            if not AFTER_ALL_LISTS:
                break
            ws += 64
        carry = NONE
        passes = (c + 63) // 64
        max_passes = max(max_passes, passes)
        for j in range(passes - 1, -1, -1):  # 64 entries a pass, the later passes' minimum carried
            u = [NONE] * 64
            for lane in range(64):
                k = j * 64 + lane
                if k < c:
                    p = lst[k]
                    nxt = lst[k + 1] if k + 1 < c else after
                    hdr, size = header(b, n, p)
                    cand[o + k], wid[o + k] = p, w
                    cdesc[o + k] = (p + hdr) | (size << 32)
                    cflag[o + k] = b[p]
                    unl[o + k] = nxt != p + hdr + size
                    u[lane] = o + k if unl[o + k] else NONE
            for lane in range(62, -1, -1):
                u[lane] = min(u[lane], u[lane + 1])
            for lane in range(64):
                u[lane] = min(u[lane], carry)
                if j * 64 + lane < c:
                    nb[o + j * 64 + lane] = u[lane]
            carry = u[0]
        first_w[w] = carry
    return dict(m=m, cand=cand, wid=wid, cdesc=cdesc, cflag=cflag, nb=nb, first_w=first_w, unl=unl,
                max_lists_skipped=max_skip, max_passes=max_passes)


def suffix_min(first_w, count):
    """zmtp_suffix_min<1024>: each thread a contiguous run of `per` entries."""
    T = NEXT_THREADS
    per = (count + T - 1) // T
    shape = "1" if per <= 1 else ("regs" if per <= SUFFIX_REGS else "loop")
    if not SUFFIX_MIN:
        return [NONE] * count, per, shape
    r0 = [min(t * per, count) for t in range(T)]
    r1 = [min(r0[t] + per, count) for t in range(T)]
    x = [min(first_w[r0[t]:r1[t]] or [NONE]) for t in range(T)]
    out = list(first_w)
    later = NONE  # the minimum over the later threads
    for t in range(T - 1, -1, -1):
        c = later
        for s in range(r1[t] - 1, r0[t] - 1, -1):
            c = min(c, first_w[s])
            out[s] = c
        later = min(later, x[t])
    return out, per, shape


def walk(b, n, max_msg, max_frames, C, first_w, nwg):
    """zmtp_walk: the runs on the chain, the frame after it, the result."""
    m, cand, cdesc, nb, wid = C["m"], C["cand"], C["cdesc"], C["nb"], C["wid"]
    frames, runs, q, full = 0, [], 0, False
    jumps, searches, src, fw_not_last = 0, 0, [], False
    if m > 0 and cand[0] == 0 and max_frames > 0:
        cur = 0
        while True:
            last, s = nb[cur], "nb"
            if last == NONE:
                wn = wid[cur] + 1
                last, s = (first_w[wn] if wn < nwg else NONE), "first_w"
                if last not in (NONE, m - 1):
                    fw_not_last = True
            if last == NONE:
                last, s = m - 1, "fallback"
            src.append(s)
            if frames + (last - cur + 1) >= max_frames:
                last = cur + (max_frames - frames) - 1
                full = True
            runs.append((cur, last, frames))
            frames += last - cur + 1
            d = cdesc[last]
            q = (d & 0xFFFFFFFF) + (d >> 32)
            if full:
                break
            lo, hi = last + 1, m
            searches += 1
            while lo < hi:
                mid = (lo + hi) >> 1
                if cand[mid] < q:
                    lo = mid + 1
                else:
                    hi = mid
            if lo < m and cand[lo] == q:
                if lo != last + 1:
                    jumps += 1
                cur = lo
                continue
            break
    res = dict(frames=frames, consumed=q, error=0, extra=None)
    if not full and q < n:
        h = header(b, n, q)
        if h is not None:
            hdr, size = h
            if not size_ok(size, max_msg):
                res["error"] = EMSGSIZE
            elif size <= n - q - hdr:
                res.update(extra=q, frames=frames + 1, consumed=q + hdr + size)
    facts = dict(runs=len(runs), jumps=jumps, searches=searches, next_src=src, first_w_not_last=fw_not_last,
                 full=full, chain_end=q)
    return res, runs, facts


def descriptors(b, n, C, runs, res):
    """k_zmtp_frames: one thread per candidate finds its run; the extra frame."""
    fr = [None] * res["frames"]
    for k in range(C["m"] if runs else 0):
        lo, hi = 0, len(runs)
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if runs[mid][0] <= k:
                lo = mid
            else:
                hi = mid
        if k < runs[lo][0] or k > runs[lo][1]:
            continue  # not on the chain
        d = C["cdesc"][k]
        fr[runs[lo][2] + k - runs[lo][0]] = (C["cflag"][k], d & 0xFFFFFFFF, d >> 32)
    if res["extra"] is not None:
        q = res["extra"]
        hdr, size = header(b, n, q)
        fr[res["frames"] - 1] = (b[q], q + hdr, size)
    assert None not in fr
    return fr


def decode(buf, max_msg=-1, max_frames=1 << 31, mis=0):
    """dict(frames=[(zmtp_flags, body_off, body_len)], consumed, error,
    out_bytes, facts) of one zmqg_decode_zmtp call over `buf`."""
    b = bytes(buf)
    n = len(b)
    if n == 0 or max_frames == 0:
        return dict(frames=[], consumed=0, error=0, out_bytes=0, facts=None)
    nwg, lists, f = scan(b, n, max_msg, mis)
    C = compact(b, n, nwg, lists)
    fw, per, shape = suffix_min(C["first_w"], nwg)
    res, runs, wf = walk(b, n, max_msg, max_frames, C, fw, nwg)
    fr = descriptors(b, n, C, runs, res)
    f.update(wf)
    on = set(k for a, z, _ in runs for k in range(a, z + 1))
    f.update(nwg=nwg, m=C["m"], linked_off_chain=sum(1 for k in range(C["m"]) if not C["unl"][k] and k not in on),
             unlinked=sum(C["unl"]), per=per, suffix_shape=shape, max_lists_skipped=C["max_lists_skipped"],
             max_passes=C["max_passes"], inline_sum=nwg <= INLINE_SUM_LISTS,
             # a true frame start (the chain reached it) that a planted LARGE header covered
             true_starts_dropped=int(not wf["full"] and wf["chain_end"] in f["dropped_at"]),
             paths={p: sum(1 for c in f["cands"] if c["path"] == p) for p in ("fast", "bytewise")})
    return dict(frames=fr, consumed=res["consumed"], error=res["error"],
                out_bytes=sum(max(x[2] - 33, 0) for x in fr), facts=f)
