"""Geometry of the chunked body path (k_body / k_post in
libzmq_amd/csrc/zmqg_curve.hip), in plain Python: which tiles, segments, carries
and move segments a call reaches.  TEST INFRASTRUCTURE ONLY: it classifies and
chooses inputs; expected bytes never come from here (they come from the oracle).

A frame whose boxed plaintext is mlen = wire_size - 32 bytes takes the body
path from mlen = 4,577.  Its body (the plaintext past byte 32) is cut into
chunks of 128 bytes, one lane each; 64 consecutive chunks of the call's
big-frame list are a tile, and wave W of NW walks the tiles
[tiles * W // NW, tiles * (W + 1) // NW).  The list order of a call is the
order in which its frames arrive at an atomic, so only a call whose big frames
all have the same chunk count has a layout that is known beforehand:
chunk_end is c, 2c, ... whatever the order.  classify() is for that case."""
from collections import Counter

CHUNK = 128          # kChunk
TILE = 64            # chunks per tile (one lane each)
BODY_MIN_MLEN = 4577  # kMaxFrameStream - 32 + 1
POW_INLINE = 6       # kPowInline: r^(8 * 2^k) for k >= 6 lives in powtab
POST_SEG, POST_SEGS, POST_ROUND, SEAM = 64 * 1024, 12, 4096, 33

CLASSES = (
    "uniform_carry_out", "uniform_carry_in", "uniform_ends_frame", "uniform_open_at_run_end",
    "uniform_open_at_run_end_powtab", "mixed_2_segments", "mixed_3_segments", "mixed_carry_in",
    "mixed_open_carry_out", "mixed_open_at_run_end", "mixed_open_at_run_end_powtab", "one_chunk_at_lane_0",
    "one_chunk_at_lane_63", "frame_end_on_tile_edge", "frame_end_on_tile_edge_in_run", "partial_last_tile",
    "frames_in_1_wave", "frames_in_2_waves", "frames_in_3_or_more_waves", "frames_in_1_wave_over_tiles",
    "runs_of_0", "runs_of_1", "runs_of_2", "runs_of_3", "open_at_run_end_powtab",
)


def geometry(mlen):
    """(nch, blast, lastb) of body_geometry: body chunks, Poly1305 blocks of the
    last chunk, bytes of the last chunk."""
    if mlen <= 32:
        return 1, 0, 0
    body = mlen - 32
    nch = (body + CHUNK - 1) // CHUNK
    lastb = body - CHUNK * (nch - 1)
    return nch, (lastb + 15) // 16, lastb


def mlen_of(nch, lastb):
    """The boxed plaintext length with nch body chunks, the last of lastb bytes."""
    assert nch >= 1 and 1 <= lastb <= CHUNK
    return 32 + CHUNK * (nch - 1) + lastb


def runs(total_chunks, NW):
    """[tb, te) of every wave."""
    tiles = (total_chunks + TILE - 1) // TILE
    return [(tiles * W // NW, tiles * (W + 1) // NW) for W in range(NW)]


def tile_segments(t, c, total):
    """The frame segments of tile t in a list of frames of c chunks each:
    (frame, first chunk of the frame in the tile, chunks) per segment."""
    g0, g1 = TILE * t, min(TILE * t + TILE, total)
    return [(i, max(g0, i * c) - i * c, min(g1, (i + 1) * c) - max(g0, i * c))
            for i in range(g0 // c, (g1 - 1) // c + 1)]


def classify(c, N, NW):
    """Tile, frame and run classes of a call of N big frames of c chunks each on
    NW waves: a Counter over CLASSES (every class present, 0 when not reached).
    The tile classes follow k_body's finish: a tile is uniform when its 64 lanes
    hold one frame; the carry is what a wave takes from a tile whose last
    segment leaves its frame open into the wave's next tile."""
    assert c >= 36 and N >= 1
    total = c * N
    out = Counter({k: 0 for k in CLASSES})
    wave_of = {}
    for W, (tb, te) in enumerate(runs(total, NW)):
        out["runs_of_%d" % min(te - tb, 3)] += 1
        carry = None  # the frame the previous tile of this run left open
        for t in range(tb, te):
            wave_of[t] = W
            segs = tile_segments(t, c, total)
            lanes = sum(s[2] for s in segs)
            last_tile = t + 1 == te
            cin = carry == segs[0][0]
            li, lc0, ln = segs[-1]
            open_ = lc0 + ln < c          # the last segment does not end its frame
            after = c - 2 - (lc0 + ln - 1)  # frame_after_power's exponent (in chunks) at a run's end
            if lanes == TILE and len(segs) == 1:
                out["uniform_carry_in"] += cin
                if open_ and not last_tile:
                    out["uniform_carry_out"] += 1
                elif open_:
                    out["uniform_open_at_run_end"] += 1
                    out["uniform_open_at_run_end_powtab"] += after >= 1 << POW_INLINE
                else:
                    out["uniform_ends_frame"] += 1
            else:
                assert len(segs) <= 3
                out["mixed_2_segments"] += len(segs) == 2
                out["mixed_3_segments"] += len(segs) == 3
                out["mixed_carry_in"] += cin
                out["partial_last_tile"] += lanes < TILE
                if lanes == TILE and open_ and not last_tile:
                    out["mixed_open_carry_out"] += 1
                elif open_:
                    out["mixed_open_at_run_end"] += 1
                    out["mixed_open_at_run_end_powtab"] += after >= 1 << POW_INLINE
                out["one_chunk_at_lane_0"] += len(segs) > 1 and segs[0][2] == 1
                out["one_chunk_at_lane_63"] += lanes == TILE and len(segs) > 1 and ln == 1
            if lanes == TILE and not open_:
                out["frame_end_on_tile_edge"] += 1
                out["frame_end_on_tile_edge_in_run"] += not last_tile
            carry = li if (open_ and lanes == TILE) else None
    for i in range(N):
        t0, t1 = i * c // TILE, ((i + 1) * c - 1) // TILE
        waves = len({wave_of[t] for t in range(t0, t1 + 1)})
        out["frames_in_%s" % ("1_wave", "2_waves", "3_or_more_waves")[min(waves, 3) - 1]] += 1
        out["frames_in_1_wave_over_tiles"] += waves == 1 and t1 > t0
    # (either kind of tile: frame_after_power reads powtab)
    out["open_at_run_end_powtab"] = out["uniform_open_at_run_end_powtab"] + out["mixed_open_at_run_end_powtab"]
    return out


def reached(counts):
    """The non-empty classes, as text for a test's printed line."""
    return ", ".join(f"{k}={counts[k]}" for k in CLASSES if counts[k])


def post_segments(length):
    """k_post's cut of an in-place move of `length` payload bytes:
    (segment bytes, segments, bytes of the last segment) as in post_seg_len."""
    per = (length + POST_SEGS - 1) // POST_SEGS
    seg = max((per + POST_ROUND - 1) // POST_ROUND * POST_ROUND, POST_SEG)
    nseg = (length + seg - 1) // seg
    return seg, nseg, length - (nseg - 1) * seg


# ---------------------------------------------------------------- the steered calls
# (tests/test_gpu_body_edges.py runs them; tests/test_body_layout_model.py
# checks at several wave counts that they reach what they are there for)
LASTB = (1, 2, 15, 16, 17, 33, 112, 113, 127, 128)
LASTB_36 = (65, 66, 79, 80, 81, 97, 112, 113, 127, 128)  # 36 chunks exist only for mlen 4,577-4,640
ALIGN_FRAMES = 16 * 16 * len(LASTB)  # every (input mod 16, output mod 16, lastb) once

SMALL_C = (36, 37, 63, 64, 65, 100, 128, 192)
SMALL_TILES = 300
LARGE_C = (36, 64, 65, 100, 192)
POW_K = range(6, 15)
SEAM_LENGTHS = (65535, 65536, 65537, 65568, 65569, 65570, 131072, 131073, 196608 + 4095, 196608 + 4096,
                196608 + 4097, 786431, 786432, 786433, 12 * 69632, 12 * 69632 + 1)


def lastb_set(c):
    return LASTB_36 if c == 36 else LASTB


def small_frames(c):
    return SMALL_TILES * TILE // c


def large_frames(c, NW, shrunk=False):
    return ((3 if shrunk else 5) * NW // 2 + 1) * TILE // c + 1


def one_frame_chunks():
    return [(1 << k) + d for k in POW_K for d in (-1, 0, 1)]


def two_tile_chunks(NW):
    """One frame of NW + 1 tiles, so one wave walks two (2^17 + 1 chunks on an MI355X)."""
    return TILE * NW + 1


# what each group of calls must reach between its members
SMALL_MUST = {
    "mixed_3_segments": (36, 37),
    "one_chunk_at_lane_0": (37, 63, 65),
    "one_chunk_at_lane_63": (37, 63, 65),
    "frames_in_3_or_more_waves": (100, 192),
    "open_at_run_end_powtab": (192,),
    "frame_end_on_tile_edge": (64, 128, 192),
}
LARGE_MUST = {
    36: ("mixed_carry_in", "mixed_open_carry_out", "mixed_3_segments", "frames_in_1_wave_over_tiles", "runs_of_2",
         "runs_of_3"),
    64: ("uniform_ends_frame", "frame_end_on_tile_edge_in_run", "runs_of_2", "runs_of_3"),
    65: ("uniform_carry_in", "uniform_carry_out", "mixed_carry_in", "mixed_open_carry_out", "one_chunk_at_lane_0",
         "one_chunk_at_lane_63", "frames_in_1_wave_over_tiles", "runs_of_2", "runs_of_3"),
    100: ("uniform_carry_in", "uniform_carry_out", "mixed_carry_in", "mixed_open_carry_out",
          "frames_in_1_wave_over_tiles", "open_at_run_end_powtab", "runs_of_2", "runs_of_3"),
    192: ("uniform_carry_in", "uniform_carry_out", "frames_in_1_wave_over_tiles", "frame_end_on_tile_edge_in_run",
          "open_at_run_end_powtab", "runs_of_2", "runs_of_3"),
}
LARGE_MUST_SHRUNK = {
    36: ("mixed_carry_in", "mixed_open_carry_out", "mixed_3_segments", "runs_of_1", "runs_of_2"),
    64: ("uniform_ends_frame", "frame_end_on_tile_edge_in_run", "runs_of_1", "runs_of_2"),
    65: ("uniform_carry_in", "uniform_carry_out", "mixed_carry_in", "mixed_open_carry_out", "one_chunk_at_lane_0",
         "one_chunk_at_lane_63", "frames_in_1_wave_over_tiles", "runs_of_1", "runs_of_2"),
    100: ("uniform_carry_in", "uniform_carry_out", "mixed_carry_in", "mixed_open_carry_out",
          "frames_in_1_wave_over_tiles", "runs_of_1", "runs_of_2"),
    192: ("uniform_carry_in", "uniform_carry_out", "frame_end_on_tile_edge_in_run", "runs_of_1", "runs_of_2"),
}
