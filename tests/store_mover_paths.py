"""Which paths of the store's byte movers a case reaches, by geometry alone: no GPU, no kernel code.

Written from DESIGN.md section 3 (the blob layout, the join, the cut, eviction) and the "where a destination unit comes
from" paragraphs of section 4.  A join or a cut fills a packed destination space that starts at the rounded-up cursor:
blob after blob, each a 64-byte header and five sections - is_raw, scale, cnt, pairs, raw -, each section a run of data
followed by zeros up to the next multiple of 64.  A run is made of parts, each one contiguous range of the source arena:
the segments' runs in a join (a seam is where one part ends and the next begins), one part in a cut.  The movers work on
tiles of 16 KiB and units of 16 bytes of that space, and what they have to do for a tile or a unit follows from where it
lies.  This module computes the space from the models' layout functions and names where every tile and unit lies.

Tile classes (a tile is [TILE k, min(TILE (k + 1), limit))):
  A  wholly inside the data of one run, no seam in it
  B  wholly inside the data of one run, at least one seam in it ("B_empty": an empty part between two of its seams)
  C  begins in a run's data, its last unit begins at or behind the run's end, in the same section's padding
  D  covers parts of two or more sections (the header is one) of one blob
  E  covers parts of two or more blobs
  F  begins exactly on a header
  G  the call's last tile, shorter than TILE
  H  tile index GRID or above: a second pass of the grid-stride loop
Unit classes, per section, each with the kind of its tile ("narrow": A, B or C; "wide": D or E):
  phase  (source address - destination address) mod 16 of a unit that lies inside one part
  seam   the position mod 16, in the destination run, of a seam that falls inside a unit
  end    the bytes of the run in its last unit, where the run does not end on 16

reached() returns labels:
  ("tile", section, "A" | "B" | "B_empty" | "C"), ("tile", "D" | "E" | "F" | "G" | "H"),
  ("phase" | "seam" | "end", section, value, "narrow" | "wide"),
  ("H", "D" | "E" | "F" | "G"), ("H", "seam" | "end", section): what lies at or behind tile GRID (any seam and any
  run's end there, inside a unit or on its edge)."""
import bisect

import numpy as np

import store_compact_cases as M
import store_join_cases as J

TILE, GRID = J.TILE, J.GRID
SECTIONS = ("is_raw", "scale", "cnt", "pairs", "raw")


# ------------------------------------------------------------------------------------------ the destination blobs of a call
# A destination blob is (ch, n_frames, parts): parts[s] is the list of (source offset inside its blob, bytes) of
# section s.  Source blobs lie on multiples of 64 of the arena, so the offset inside the blob is the address mod 16.

def _section_starts(ch, nf, n_pairs):
    return J.layout(ch, nf) + (J.raw_offset(ch, nf, n_pairs),)


def join_blobs(case):
    """The destination blobs of a join case: one per clip, a part per segment."""
    ch, out = case["ch"], []
    for blobs in case["clips"]:
        parts, F = [[] for _ in SECTIONS], 0
        for b in blobs:
            _, _, nf, n_pairs, n_raw, _ = J.parse_header(b)
            starts = _section_starts(ch, nf, n_pairs)
            for s, n in enumerate((nf, 4 * nf * ch, 4 * nf * ch, 4 * n_pairs, 2 * J.FRAME * n_raw)):
                parts[s].append((starts[s], n))
            F += nf
        out.append((ch, F, parts))
    return out


def cut_blobs(case):
    """The destination blobs of a cut case: one per cut, one part per section."""
    ch, out, sums = case["ch"], [], {}
    for clip, f0, nf in case["cuts"]:
        if clip not in sums:
            b = np.frombuffer(case["clips"][clip], np.uint8)
            _, _, F, n_pairs, _, _ = J.parse_header(b)
            starts = _section_starts(ch, F, n_pairs)
            cnt = b[starts[2]:starts[2] + 4 * F * ch].view(np.uint32).astype(np.uint64)
            raw = (b[starts[0]:starts[0] + F] != 0).astype(np.uint64) * ch
            sums[clip] = (starts, np.concatenate([[0], np.cumsum(cnt)]), np.concatenate([[0], np.cumsum(raw)]))
        starts, pairs, rows = sums[clip]
        m0, m1 = f0 * ch, (f0 + nf) * ch
        P0, P, R0, R = int(pairs[m0]), int(pairs[m1] - pairs[m0]), int(rows[f0]), int(rows[f0 + nf] - rows[f0])
        parts = [[(starts[0] + f0, nf)], [(starts[1] + 4 * m0, 4 * (m1 - m0))], [(starts[2] + 4 * m0, 4 * (m1 - m0))],
                 [(starts[3] + 4 * P0, 4 * P)], [(starts[4] + 2 * J.FRAME * R0, 2 * J.FRAME * R)]]
        out.append((ch, nf, parts))
    return out


# ------------------------------------------------------------------------------------------ tiles and units

def reached(blobs):
    """The labels (module docstring) the packed space of `blobs` reaches."""
    # the regions of the space in order: [start, end) of a header or of a section with its padding
    regions, at = [], 0                                  # (start, end, blob, section or -1, data bytes, parts)
    for b, (ch, nf, parts) in enumerate(blobs):
        lens = [sum(n for _, n in p) for p in parts]
        starts = _section_starts(ch, nf, lens[3] // 4)
        size = J.blob_bytes(ch, nf, lens[3] // 4, lens[4] // (2 * J.FRAME))
        regions.append((at, at + 64, b, -1, 64, ()))
        for s in range(5):
            end = at + (starts[s + 1] if s < 4 else size)
            assert end - (at + starts[s]) == J.a64(lens[s])
            if lens[s]:
                regions.append((at + starts[s], end, b, s, lens[s], parts[s]))
        at += size
    limit, first = at, [r[0] for r in regions]
    out, kinds = set(), {}
    n_tiles = (limit + TILE - 1) // TILE

    def seams_of(region):
        """(position, the part in front is empty) of every seam strictly inside the run's data."""
        start, _, _, _, data, parts = region
        pos, found = start, []
        for i, (_, n) in enumerate(parts[:-1]):
            pos += n
            if start < pos < start + data:
                found.append((pos, n == 0))
        return found

    seams = [seams_of(r) if r[3] >= 0 else [] for r in regions]
    for k in range(n_tiles):
        lo, hi = TILE * k, min(TILE * (k + 1), limit)
        i0, i1 = bisect.bisect_right(first, lo) - 1, bisect.bisect_right(first, hi - 1) - 1
        cls = set()
        if regions[i0][2] != regions[i1][2]:
            cls.add("E")
        elif i0 != i1:
            cls.add("D")
        if regions[i0][3] < 0 and regions[i0][0] == lo:
            cls.add("F")
        if k == n_tiles - 1 and hi - lo < TILE:
            cls.add("G")
        if k >= GRID:
            cls.add("H")
        start, _, _, sec, data, _ = regions[i0]
        one = set()
        if i0 == i1 and sec >= 0 and lo < start + data:
            if hi <= start + data:
                inside = [(p, empty) for p, empty in seams[i0] if lo < p < hi]
                one.add("B" if inside else "A")
                if any(empty for _, empty in inside):
                    one.add("B_empty")
            elif hi - 16 >= start + data:
                one.add("C")
        out |= {("tile", c) for c in cls} | {("tile", SECTIONS[sec], c) for c in one}
        if "H" in cls:
            out |= {("H", c) for c in cls - {"H"}}
        kinds[k] = "narrow" if one else "wide" if cls & {"D", "E"} else None

    def unit(what, sec, value, p):
        if kinds[p // TILE]:
            out.add((what, SECTIONS[sec], value, kinds[p // TILE]))

    for i, (start, _, _, sec, data, parts) in enumerate(regions):
        if sec < 0:
            continue
        pos = start
        for src, n in parts:
            u0, u1 = (pos + 15) // 16 * 16, (pos + n) // 16 * 16          # the units that lie inside the part
            if u1 - u0 >= 16:
                for k in range(u0 // TILE, (u1 - 1) // TILE + 1):
                    unit("phase", sec, (src - pos) % 16, max(u0, k * TILE))
            pos += n
        for p, _ in seams[i]:
            if p % 16:
                unit("seam", sec, p % 16, p)
            if p // TILE >= GRID:                                         # any seam, on a unit's edge or inside one
                out.add(("H", "seam", SECTIONS[sec]))
        if data % 16:
            unit("end", sec, data % 16, start + data)
        if (start + data - 1) // TILE >= GRID:
            out.add(("H", "end", SECTIONS[sec]))
    return out


# ------------------------------------------------------------------------------------------ eviction

def evict_reached(case, rnd=None):
    """The labels an eviction case reaches when it runs with the in-place round `rnd` (None: the default round):
    "one_blob" / "several_blobs" (a tile inside one kept blob / over several), "tile_ge_grid" (tile index GRID or above),
    and in place "round_boundary" (a 16 KiB tile of the packed space that a round boundary cuts), "short_round_tile" (the
    last tile of a round that is no multiple of TILE, all of it moved), "job_ge_grid" (a job of index GRID or above out
    of the 2 * tiles of a round launch); "tail_ge_cap": more than TAIL_CAP entries behind n_out to zero."""
    ab, entries = case["arena_bytes"], case["entries"]
    _, kept = M.verdicts(ab, entries, case["keep"])
    in_place = case["dst_bytes"] is None
    dst_bytes = ab if in_place else case["dst_bytes"]
    new_off, place, limit, first = [], 0, 0, None
    for i in kept:
        new_off.append(place)
        if place <= dst_bytes and entries[i][1] <= dst_bytes - place:
            limit = place + entries[i][1]
        if first is None and entries[i][0] != place:
            first = place
        place += entries[i][1]
    total = place
    first = total if first is None else first
    out = set()
    if len(entries) - len(kept) > M.TAIL_CAP:
        out.add("tail_ge_cap")

    def blobs_in(lo, hi):
        return bisect.bisect_right(new_off, hi - 1) - bisect.bisect_right(new_off, lo) + 1

    if not in_place:
        for k in range((limit + TILE - 1) // TILE):
            lo, hi = TILE * k, min(TILE * (k + 1), limit)
            out.add("one_blob" if blobs_in(lo, hi) == 1 else "several_blobs")
            if k >= GRID:
                out.add("tile_ge_grid")
        return out
    rs = min(rnd or M.DEFAULT_ROUND, (ab + 63) // 64 * 64)
    tiles = (rs + TILE - 1) // TILE
    for r in range((total + rs - 1) // rs if rs else 0):
        base = r * rs
        for j in range(tiles):
            lo, hi = max(base + j * TILE, first), min(base + min((j + 1) * TILE, rs), total)
            if lo >= hi:
                continue
            out.add("one_blob" if blobs_in(lo, hi) == 1 else "several_blobs")
            if j >= GRID:
                out.add("tile_ge_grid")
            if tiles + j >= GRID:
                out.add("job_ge_grid")
            if j == tiles - 1 and rs % TILE and hi == base + rs:
                out.add("short_round_tile")
            g = lo // TILE * TILE                                        # the 16 KiB tile of the packed space that holds lo
            b = (g // rs + 1) * rs                                       # the first round boundary behind its start
            if g < b < min(g + TILE, total):
                out.add("round_boundary")
    return out
