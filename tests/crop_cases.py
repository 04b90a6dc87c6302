"""Cases for tests/test_compact_crops.py: which windows of a clip are worth decoding, the crafted and the damaged blobs
they are cut from, and the numpy side of the comparisons.  Nothing here touches the GPU.

Geometry ("a window of a compact blob"): sample t of channel c of the decoded clip is the
un-trimmed interleaved position 512 + t * ch + c; hop h is the positions [1024 ch h, 1024 ch (h + 1)); a clip of nf
frames has the hops 0 .. nf, the last one being the bare tail (the second half of frame nf - 1 alone)."""
from __future__ import annotations

import numpy as np

import compact_decode_cases as K

HOP, FRAME = K.HOP, K.FRAME
DELAY = 512
F32 = np.float32
NAN_BITS = 0x7FC00ABC        # a NaN payload nothing computes
ROUND = 4096                 # glc_api.hip kDecodeChunkFrames
PREFIX_ROWS = 4096           # glc_kernels.hip kR2wPrefixRows: rows in front of a window per k_r2w_prefix workgroup


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def hop_of(t, c, ch):
    return (DELAY + t * ch + c) // (HOP * ch)


def first_sample_of_hop(h, ch):
    """The first per-channel sample index whose sample frame lies WHOLLY at or behind the start of hop h."""
    return max(0, -(-(h * HOP * ch - DELAY) // ch))


def boundary_sample(h, ch):
    """The per-channel sample index whose sample frame holds the first position of hop h (h >= 1).  For 1 and 2
    channels the frame starts exactly there; for 3 and 6 the boundary falls inside it (512 is no multiple of ch)."""
    return (h * HOP * ch - DELAY) // ch


def edge_windows(n, ch, nf):
    """(start, length) windows of a clip of n samples per channel (nf frames) at every edge the geometry has."""
    w = {(0, 1), (0, n), (n - 1, 1), (0, n - 1), (1, n - 1)}
    last_hop = hop_of(n - 1, ch - 1, ch)
    # inside one hop
    for h in (0, 1, last_hop):
        a = first_sample_of_hop(h, ch)
        if a + 7 < n and hop_of(a + 6, ch - 1, ch) == h:
            w.add((a + 2, 5))
    # starting / ending on a hop boundary of the un-trimmed stream, and one sample to either side of it; for 3 and 6
    # channels the windows (b, 1) straddle the boundary inside one sample frame
    for h in range(1, last_hop + 1):
        b = boundary_sample(h, ch)
        for s in (b - 1, b, b + 1):
            if 0 <= s < n:
                w.add((s, 1))
                w.add((s, min(n - s, HOP)))            # a hop's worth from here
                if s > 0:
                    w.add((max(0, s - HOP), s - max(0, s - HOP)))   # ... and up to here
    # exactly one hop, for every hop (every pairing of halo frame and own frame: raw / compressed)
    for h in range(0, last_hop + 1):
        a, b = first_sample_of_hop(h, ch), min(n, first_sample_of_hop(h + 1, ch))
        if b > a:
            w.add((a, b - a))
    # the tail: the last samples, alone and with the hop in front
    for k in (1, 2, 3, 300):
        if k <= n:
            w.add((n - k, k))
    return sorted(x for x in w if x[1] > 0 and x[0] + x[1] <= n)


def reaches_tail(n, ch, nf):
    return hop_of(n - 1, ch - 1, ch) == nf


def want_crops(shape, planar, margin, ch, entries):
    """The expected bits of a NaN-pattern tensor of `shape` after the crops `entries` = [(whole clip's interleaved
    samples, start, length)] were decoded into its leading slice."""
    want = np.full(shape, NAN_BITS, np.uint32)
    for i, (ref, start, length) in enumerate(entries):
        piece = bits(ref).reshape(-1, ch)[start:start + length]
        assert piece.shape[0] == length
        if planar:
            want[i, :ch, margin:margin + length] = piece.T
        else:
            want[i, :length, :ch] = piece
    return want


# ------------------------------------------------------------------------------------------ crafted blobs

def crafted():
    """(name, ch, frames) descriptions as compact_decode_cases.pack takes them."""
    rng = np.random.RandomState(29)
    c = []
    c.append(("raw-first-and-last-3ch", 3, [("raw", K.raw_planes(rng, 3))] + [("c", [K.row(rng, 20 + f) for _ in range(3)]) for f in range(4)] +
              [("raw", K.raw_planes(rng, 3))]))
    c.append(("alternating-raw-stereo", 2, [("raw", K.raw_planes(rng, 2)) if f % 2 else ("c", [K.row(rng, 10), K.row(rng, 0)])
                                            for f in range(9)]))
    lens = (0, 1, 63, 64, 65, 1023, 1024)
    c.append(("list-lengths-stereo", 2, [("c", [K.row(rng, lens[(f + 3 * k) % len(lens)]) for k in range(2)]) for f in range(7)]))
    ext = K.Row(np.array([0, 1, 511, 1022, 1023], np.uint16), np.array([-32768, 32767, -32768, 32767, -1], np.int16))
    inf = K.Row(np.array([5, 700], np.uint16), np.array([100, -100], np.int16), 0x7F800000)
    zero_q = K.Row(np.array([9], np.uint16), np.array([0], np.int16), 0x7F800000)      # a stored zero times inf: NaN
    c.append(("extremes-and-inf-stereo", 2, [("c", [ext, inf]), ("c", [zero_q, ext]), ("c", [K.row(rng, 3), K.row(rng, 4)]),
                                             ("c", [inf, zero_q]), ("c", [K.row(rng, 5), ext])]))
    return c


def crafted_windows(nf, ch):
    """A few windows of a crafted stream of nf frames (nf * HOP samples per channel): one whose only frame is the first,
    one whose only frame is the last (inside the bare tail hop), and some across the middle."""
    n = nf * HOP
    only_first = (0, boundary_sample(1, ch))                     # inside hop 0: frame 0 alone
    t = first_sample_of_hop(nf, ch)
    only_last = (t, n - t)                                       # hop nf: frame nf - 1 alone
    mid = [(first_sample_of_hop(2, ch) - 3, 2 * HOP + 5), (HOP, 1), (0, n), (first_sample_of_hop(nf - 1, ch), 17),
           (n // 2 - 100, 313), (n - 1, 1)]
    return [only_first, only_last] + mid


def scan_blob(rows, ch=1, seed=31):
    """A blob of `rows` rows whose frames' lists have 0..4 entries, raw frames at the scan's edges."""
    rng = np.random.RandomState(seed)
    nf = rows // ch
    raw_at = {1, (K.SCAN_BLOCK - 1) // ch, K.SCAN_BLOCK // ch, nf - 2}
    return [("raw", K.raw_planes(rng, ch)) if f in raw_at and 0 < f < nf - 1 else ("c", [K.row(rng, (f * 7 + k) % 5) for k in range(ch)])
            for f in range(nf)]


def table_windows(rows, ch):
    """(first_frame, frames) windows of a blob of `rows` rows whose first row is 0, 1, 1023, 1024, 1025 or the last
    one (as far as a frame starts there) and whose length is 1, 3, 4, 5 rows (rounded to frames), 1024, 1025 and
    2048 rows - the window's own scan block - where they fit."""
    nf = rows // ch
    firsts = sorted({r // ch for r in (0, ch, K.SCAN_BLOCK - ch, K.SCAN_BLOCK - 1, K.SCAN_BLOCK, K.SCAN_BLOCK + 1, rows - 1) if 0 <= r < rows})
    out = []
    for f0 in firsts:
        for length in (1, 3, 4, 5, K.SCAN_BLOCK, K.SCAN_BLOCK + 1, 2 * K.SCAN_BLOCK):
            fr = -(-length // ch)
            if f0 + fr <= nf:
                out.append((f0, fr))
    return sorted(set(out))


# ------------------------------------------------------------------------------------------ damaged blobs

def stereo_stream(nf=8, seed=37):
    rng = np.random.RandomState(seed)
    return [("c", [K.row(rng, 12 + f), K.row(rng, 30 - f)]) for f in range(nf)]


def with_bad_list(frames, row, ch=2):
    """The description with the list of `row` made non-ascending (a repeated bin)."""
    fr = [(k, list(body)) for k, body in frames]
    fr[row // ch][1][row % ch] = K.Row(np.array([3, 40, 40, 900], np.uint16), np.arange(1, 5, dtype=np.int16))
    return fr
