"""Cases and models for tests/test_store_ragged.py and tests/test_store_ragged_plan.py
(glc_decode_ragged_crops_device_store, DESIGN.md section 3, "ragged crops").  Nothing here touches the GPU.

The models are written from the contract in include/glc.h, not from the kernel.  With n the stored length of the
selected clip, s the start and w the wanted length (`length` where none is given), a selection is usable when the index
is in range, n is a length the encoder accepts and at most max_length, 0 <= s < n and 1 <= w <= length; its valid
length is v = min(w, n - s).  A crop owns the table rows and block slots of the fixed draw (store_draw_cases.slots) and
max_descs descriptors: the hops of its valid part - glc_plan_crop's for {s, v} - then one silent descriptor per
1024 ch positions of the padding [v ch, length ch) of its row, then null ones."""
from __future__ import annotations

import crop_cases as CC
import store_draw_cases as S

HOP, DELAY = S.HOP, S.DELAY
NO_BLOB, BAD_CROP, BAD_HEADER, NULL_DESC, U64 = S.NO_BLOB, S.BAD_CROP, S.BAD_HEADER, S.NULL_DESC, S.U64


def valid_of(n, start, want, length):
    """v of a usable selection"""
    return min(length if want is None else want, n - start)


def verdict_of(entries, lengths, arena_bytes, max_length, clip, start, want, length):
    """0, BAD_CROP or NO_BLOB for one selection; entries / lengths as the int64 the tensors hold."""
    if clip < 0 or clip >= len(entries):
        return BAD_CROP
    n = lengths[clip]
    w = length if want is None else want
    if n < 0 or n > max_length or n <= 512 or not 0 <= start < n or not 1 <= w <= length:
        return BAD_CROP
    off, size, _, raw_stored = (v & U64 for v in entries[clip])
    if (raw_stored >> 32) == 0 or off % 64 or off > arena_bytes or size > arena_bytes - off:
        return NO_BLOB
    return 0


def pads_of(v, length, ch):
    """descriptors of the padding behind a valid part of v samples per channel"""
    return -(-(length - v) * ch // (HOP * ch))


def descs_needed(p_hops, v, length, ch):
    return p_hops + pads_of(v, length, ch)


def plan_model(g, max_descs, arena, arena_bytes, entries, lengths, max_length, clips, starts, wants, length, ch, planar, clip_stride,
               channel_stride):
    """-> (dir rows, descriptor rows [n][max_descs], verdicts, valid lengths) as the ragged planner must write them.
    wants: None, or one wanted length per crop."""
    max_frames = S.slots(length, ch)[1]
    rounds_of = S.per_round(length, ch)
    planes = planar and ch > 1
    per_hop, span = HOP * ch, length * ch
    dirs, descs, verdicts, valids = [], [], [], []

    def silent(j0, dst):
        return (-1, -1, 0, min(per_hop, span - j0), dst if planes else dst + j0, channel_stride if planes else 0, j0)

    for i, (clip, start) in enumerate(zip(clips, starts)):
        want = None if wants is None else wants[i]
        k = i % rounds_of
        slot0, dst = k * max_frames, i * clip_stride
        verdict = verdict_of(entries, lengths, arena_bytes, max_length, clip, start, want, length)
        verdicts.append(verdict)
        if verdict:
            dirs.append((arena, 0, slot0 * ch, 0, 0, 0))
            descs.append([silent(s * per_hop, dst) if s * per_hop < span else NULL_DESC for s in range(max_descs)])
            valids.append(0)
            continue
        n = lengths[clip]
        v = valid_of(n, start, want, length)
        assert 1 <= v <= length
        valids.append(v)
        nf = S.frames_of(n)
        p = g.plan_crop(n * ch, ch, start, v)
        assert p.n_frames <= max_frames and descs_needed(p.n_hops, v, length, ch) <= max_descs
        dirs.append((arena + (entries[clip][0] & U64), entries[clip][1] & U64, slot0 * ch, nf * ch, p.first_frame * ch, p.n_frames * ch))
        t0 = DELAY + start * ch                           # the valid part in the un-trimmed stream: [t0, t0 + v ch)
        base = slot0 - p.first_frame
        row = []
        for s in range(max_descs):
            if s < p.n_hops:
                h = p.first_hop + s
                lo, hi = max(t0, h * per_hop), min(t0 + v * ch, (h + 1) * per_hop)
                assert hi > lo
                j0 = lo - t0
                row.append((base + h - 1 if h >= 1 else -1, base + h if h < nf else -1, lo - h * per_hop, hi - lo,
                            dst if planes else dst + j0, channel_stride if planes else 0, j0))
                continue
            j0 = v * ch + (s - p.n_hops) * per_hop
            row.append(silent(j0, dst) if j0 < span else NULL_DESC)
        descs.append(row)
    return dirs, descs, verdicts, valids


def boundary_selections(n, ch, length):
    """(start, want) of a clip of n samples per channel for an output row of `length`: starts on both sides of every hop
    boundary and at the clip's ends, each wanting the whole row (cut by the clip's end where it is nearer), one sample
    and a part that ends on either side of the next hop boundary."""
    starts = {0, n - 1, max(0, n - length), max(0, n - length - 1), min(n - 1, max(0, n - length) + 1)}
    bounds = [CC.boundary_sample(h, ch) for h in range(1, CC.hop_of(n - 1, ch - 1, ch) + 1)]
    for b in bounds:
        starts.update(s for s in (b - 1, b, b + 1) if 0 <= s < n)
    sels = set()
    for s in sorted(starts):
        sels.update({(s, length), (s, 1), (s, min(2, length))})
        for b in bounds:
            for e in (b - 1, b, b + 1, b + 2):           # the valid part's last sample
                if s <= e and 1 <= e - s + 1 <= length:
                    sels.add((s, e - s + 1))
    return sorted(sels)
