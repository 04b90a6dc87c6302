"""Cases and models for tests/test_store_draw.py (glc_decode_crops_device_store, DESIGN.md section 3, "drawing from the
store").  Nothing here touches the GPU.

The planner's model is written from the design text, not from the kernel: crop i of a call is number k = i % per_round
of its round and owns table rows [k * max_frames * ch, ...), block slots [k * max_frames, ...) and max_hops hop
descriptors.  Its geometry is glc_plan_crop's (the host function, held to brute force by tests/test_crop_plan.py); the
descriptor of a hop is the rule of section 4, D2 by descriptor."""
from __future__ import annotations

import numpy as np

import crop_cases as CC

HOP, FRAME, DELAY = CC.HOP, CC.FRAME, CC.DELAY
NO_BLOB, BAD_CROP, BAD_HEADER = 64, 128, 1
ROUND_BUDGET = 4097                      # frames + 1 of every crop of a round
NULL_DESC = (-1, -1, 0, 0, 0, 0, 0)
U64 = (1 << 64) - 1

DIR_DTYPE = np.dtype([("addr", "<u8"), ("cap", "<u8"), ("first_row", "<u4"), ("rows", "<u4"), ("win0", "<u4"), ("win1", "<u4")])
DESC_DTYPE = np.dtype([("prev", "<i4"), ("cur", "<i4"), ("first", "<u4"), ("cnt", "<u4"), ("dst", "<u8"), ("cstride", "<u8"), ("j0", "<u8")])
assert DIR_DTYPE.itemsize == 32 and DESC_DTYPE.itemsize == 40


def slots(length, ch):
    per_hop = HOP * ch
    hops = (per_hop - ch + DELAY % ch + length * ch - 1) // per_hop + 1
    return hops, hops + 1


def per_round(length, ch):
    return ROUND_BUDGET // (slots(length, ch)[1] + 1)


def frames_of(n):
    return -(-(DELAY + n) // HOP) - 1 if n > 512 else 0


def entry(offset, nbytes, stored=1, n_pairs=0, n_raw_rows=0):
    """One glc_store_entry as the four int64 the tensors hold (offsets above 2^63 as their two's complement)."""
    s = lambda v: v - (1 << 64) if v >= (1 << 63) else v
    return [s(offset & U64), s(nbytes & U64), n_pairs, n_raw_rows | (stored << 32)]


def verdict_of(entries, lengths, arena_bytes, max_length, clip, start, length):
    """0, BAD_CROP or NO_BLOB for one selection; entries / lengths as the int64 the tensors hold."""
    if clip < 0 or clip >= len(entries):
        return BAD_CROP
    n = lengths[clip]
    if n < 0 or n > max_length or n <= 512 or start < 0 or length > n or start > n - length:
        return BAD_CROP
    off, size, _, raw_stored = (v & U64 for v in entries[clip])
    if (raw_stored >> 32) == 0 or off % 64 or off > arena_bytes or size > arena_bytes - off:
        return NO_BLOB
    return 0


def plan_model(g, arena, arena_bytes, entries, lengths, max_length, clips, starts, length, ch, planar, clip_stride, channel_stride):
    """-> (dir rows, descriptor rows [n][max_hops], verdicts) as the planner must write them."""
    max_hops, max_frames = slots(length, ch)
    rounds_of = per_round(length, ch)
    planes = planar and ch > 1
    per_hop = HOP * ch
    dirs, descs, verdicts = [], [], []
    for i, (clip, start) in enumerate(zip(clips, starts)):
        k = i % rounds_of
        slot0, dst = k * max_frames, i * clip_stride
        v = verdict_of(entries, lengths, arena_bytes, max_length, clip, start, length)
        verdicts.append(v)
        span = length * ch
        if v:
            dirs.append((arena, 0, slot0 * ch, 0, 0, 0))
            row = []
            for s in range(max_hops):
                j0 = s * per_hop
                row.append((-1, -1, 0, min(per_hop, span - j0), dst if planes else dst + j0, channel_stride if planes else 0, j0)
                           if j0 < span else NULL_DESC)
            descs.append(row)
            continue
        n = lengths[clip]
        nf = frames_of(n)
        p = g.plan_crop(n * ch, ch, start, length)
        assert p.n_hops <= max_hops and p.n_frames <= max_frames
        dirs.append((arena + (entries[clip][0] & U64), entries[clip][1] & U64, slot0 * ch, nf * ch, p.first_frame * ch, p.n_frames * ch))
        t0 = DELAY + start * ch                           # what the crop keeps of the un-trimmed stream: [t0, t0 + span)
        base = slot0 - p.first_frame
        row = []
        for s in range(max_hops):
            h = p.first_hop + s
            if s >= p.n_hops:
                row.append(NULL_DESC)
                continue
            lo, hi = max(t0, h * per_hop), min(t0 + span, (h + 1) * per_hop)
            assert hi > lo
            j0 = lo - t0
            row.append((base + h - 1 if h >= 1 else -1, base + h if h < nf else -1, lo - h * per_hop, hi - lo,
                        dst if planes else dst + j0, channel_stride if planes else 0, j0))
        descs.append(row)
    return dirs, descs, verdicts


def boundary_starts(n, ch, length):
    """Starts of a crop of `length` in a clip of n samples per channel: the ends, and every start that puts the crop's
    first or last sample frame on either side of a hop boundary of the un-trimmed stream."""
    if length > n:
        return []
    pts = {0, n - length}
    last_hop = CC.hop_of(n - 1, ch - 1, ch)
    for h in range(1, last_hop + 1):
        b = CC.boundary_sample(h, ch)
        for s in (b - 1, b, b + 1):
            pts.add(s)                   # the crop starts there
            pts.add(s - length)          # ... or ends there
            pts.add(s - length + 1)
    return sorted(p for p in pts if 0 <= p <= n - length)


def edge_draws(n, ch, nf):
    """(start, length) crops of a clip: crop_cases.edge_windows, a crop with no halo frame (it starts inside hop 0), one
    that reaches the bare tail hop when the clip has samples there, and single samples."""
    w = set(CC.edge_windows(n, ch, nf))
    w.add((0, min(n, 7)))                                         # hop 0: frame 0 alone, no halo frame
    if CC.reaches_tail(n, ch, nf):
        t = CC.first_sample_of_hop(nf, ch)
        w.add((t, n - t))                                         # the bare tail hop alone
        w.add((max(0, t - 5), n - max(0, t - 5)))                 # ... and with the hop in front
    for s in (0, n // 2, n - 1):
        w.add((s, 1))
    return sorted(w)
