"""Cases and the numpy model of the cut (include/glc.h glc_store_cut_device / glc_compact_cut), written from DESIGN.md
section 3, "cutting a stored clip": judge the entry, the header and the window, sum the rows in front of the window and
in it, take the window's slice of each of the five sections behind a fresh header with zero padding; then the encoder's
placement rule over the pieces.

The blobs are made by the builder of tests/store_join_cases.py: the cut is structural, like the join, and never looks at
what a list or a plane means."""
import functools
import struct

import numpy as np

import store_join_cases as J

PATTERN = J.PATTERN
HOP, FRAME = J.HOP, J.FRAME
TILE, GRID = J.TILE, J.GRID
BAD_HEADER, ROW_BOUNDS, RAW_RANGE, NO_BLOB, BAD_CROP = 1, 2, 8, 64, 128


# ------------------------------------------------------------------------------------------ the model

def cut(blob, ch: int, f0: int, nf: int):
    """(status bits, the piece's blob or None) of frames [f0, f0 + nf) of `blob`, all of whose bytes are available."""
    b = np.frombuffer(bytes(blob), np.uint8)
    if b.size < 64:
        return BAD_HEADER, None
    magic, chs, F, n_pairs, n_raw, nbytes = J.parse_header(b)
    # the frame count is bounded before any size is formed from it
    if magic != J.MAGIC or chs != ch or F == 0 or F > 0xFFFFFFFF // ch or F > b.size - 64:
        return BAD_HEADER, None
    if n_pairs > F * ch * HOP or n_raw > F * ch or n_raw % ch:
        return BAD_HEADER, None
    need = J.blob_bytes(ch, F, n_pairs, n_raw)
    if nbytes != need or b.size < need:
        return BAD_HEADER, None
    if f0 + nf > F:
        return BAD_CROP, None
    o_israw, o_scale, o_cnt, o_pairs = J.layout(ch, F)
    m0, m1 = f0 * ch, (f0 + nf) * ch
    cnt = b[o_cnt:o_cnt + 4 * m1].view(np.uint32).astype(np.uint64)       # nothing behind the window is looked at
    israw = b[o_israw:o_israw + f0 + nf]
    P0, P = int(cnt[:m0].sum()), int(cnt[m0:].sum())
    R0, R = int(np.count_nonzero(israw[:f0])) * ch, int(np.count_nonzero(israw[f0:])) * ch
    bits = 0
    if (cnt > HOP).any() or P0 + P > n_pairs:
        bits |= ROW_BOUNDS
    if R0 + R > n_raw:
        bits |= RAW_RANGE
    if bits:
        return bits, None
    out = np.zeros(J.blob_bytes(ch, nf, P, R), np.uint8)
    out[:64] = np.frombuffer(J.header(ch, nf, P, R, out.size), np.uint8)
    d_israw, d_scale, d_cnt, d_pairs = J.layout(ch, nf)
    d_raw, s_raw = J.raw_offset(ch, nf, P), J.raw_offset(ch, F, n_pairs)
    for dst, src, n in ((d_israw, o_israw + f0, nf), (d_scale, o_scale + 4 * m0, 4 * (m1 - m0)), (d_cnt, o_cnt + 4 * m0, 4 * (m1 - m0)),
                        (d_pairs, o_pairs + 4 * P0, 4 * P), (d_raw, s_raw + 2 * FRAME * R0, 2 * FRAME * R)):
        out[dst:dst + n] = b[src:src + n]
    return 0, out.tobytes()


def cut_store(arena, arena_bytes: int, entries, cuts, lengths, ch: int, dst, dst_bytes: int, cursor: int):
    """The device call.  arena: uint8 array; entries: rows [offset, bytes, n_pairs, n_raw_rows, stored]; cuts: [(clip,
    first_frame, n_frames)]; lengths: per cut, or None; dst: uint8 array, a copy of which is written.  Returns a dict of
    the destination arena, entries_out (rows of 5), lengths_out, status and the cursor."""
    dst = np.array(dst, np.uint8)
    at = J.a64(cursor)
    status, entries_out, lengths_out = [], [], []
    for i, (clip, f0, nf) in enumerate(cuts):
        bits, blob = BAD_CROP, None
        if clip < len(entries):
            off, nb, _, _, stored = entries[clip]
            if stored == 0 or off % 64 or off > arena_bytes or nb > arena_bytes - off:
                bits = NO_BLOB | BAD_HEADER
            else:
                bits, blob = cut(arena[off:off + nb], ch, f0, nf)
        status.append(bits)
        if bits:
            entries_out.append([0, 0, 0, 0, 0])
            lengths_out.append(0)
            continue
        blob = np.frombuffer(blob, np.uint8)
        _, _, _, n_pairs, n_raw, _ = J.parse_header(blob)
        stored = at <= dst_bytes and blob.size <= dst_bytes - at
        if stored:
            dst[at:at + blob.size] = blob
        entries_out.append([at, blob.size, n_pairs, n_raw, int(stored)])
        lengths_out.append(lengths[i] if lengths is not None else HOP * nf)
        at += blob.size
    return {"dst": dst, "entries": entries_out, "lengths": lengths_out, "status": status, "cursor": at}


# ------------------------------------------------------------------------------------------ damage

def damaged(blob: bytes, kind: str, ch: int, f0: int, nf: int):
    """(the blob damaged in the named way, the status bits the cut [f0, f0 + nf) of it gets, a word of the host twin's
    message).  The header kinds are the join's; the others touch what the cut itself reads."""
    if kind in ("magic", "channels", "frames", "bytes"):
        bad, bits = J.damaged(blob, kind, ch)
        return bad, bits, "magic" if kind in ("magic", "channels") else "size"   # a frame count of its own only moves the sizes
    b = np.frombuffer(blob, np.uint8).copy()
    magic, chs, F, n_pairs, n_raw, nbytes = J.parse_header(b)
    o_israw, _, o_cnt, _ = J.layout(ch, F)
    cnt = b[o_cnt:o_cnt + 4 * F * ch].view(np.uint32)

    def put(n_pairs=n_pairs, n_raw=n_raw, nbytes=nbytes):
        b[:40] = np.frombuffer(struct.pack("<IIQQQQ", magic, chs, F, n_pairs, n_raw, nbytes), np.uint8)
    if kind == "cnt_front":                        # a row in front of the window: needs f0 > 0
        cnt[0] = HOP + 1
        return b.tobytes(), ROW_BOUNDS, "1024"
    if kind == "cnt_in":
        cnt[f0 * ch + (nf * ch) // 2] = HOP + 1
        return b.tobytes(), ROW_BOUNDS, "1024"
    if kind == "pairs_low":
        # the header says one pair fewer than the rows up to the window's end hold, with the size that goes with that
        # count: it passes the header rule (a blob may lie in more bytes than it needs)
        low = int(cnt[:(f0 + nf) * ch].astype(np.uint64).sum()) - 1
        assert 0 <= low < n_pairs
        put(n_pairs=low, nbytes=J.blob_bytes(ch, F, low, n_raw))
        return b.tobytes(), ROW_BOUNDS, "n_pairs"
    if kind == "raw_low":
        # one raw frame fewer in the header and in the bytes; the window holds the clip's last raw frame
        assert n_raw >= ch and b[o_israw:o_israw + f0 + nf].astype(bool).sum() * ch == n_raw
        put(n_raw=n_raw - ch, nbytes=nbytes - 2 * FRAME * ch)
        return b.tobytes(), RAW_RANGE, "n_raw_rows"
    if kind == "cnt_behind":                       # behind the window: not looked at
        assert f0 + nf < F
        cnt[(f0 + nf) * ch] = HOP + 1
        return b.tobytes(), 0, ""
    if kind == "raw_behind":
        assert f0 + nf < F
        b[o_israw + f0 + nf] ^= 1
        return b.tobytes(), 0, ""
    raise KeyError(kind)


HEADER_DAMAGE = ("magic", "channels", "frames", "bytes")
WINDOW_DAMAGE = ("cnt_front", "cnt_in", "pairs_low", "raw_low")
BEHIND = ("cnt_behind", "raw_behind")


def damage_clip(rng, ch=2):
    """A clip for the damage kinds and the window they are judged on: 9 frames, raw frames in front of the window and in
    it, none behind; every other row holds pairs."""
    f0, nf, F = 3, 4, 9
    return J.make_blob(rng, ch, F, raw=(2, 5), cnt=rng.integers(1, 30, F * ch)), f0, nf


# ------------------------------------------------------------------------------------------ the cases

def case(name, ch, clips, cuts):
    """clips: one blob per stored clip; cuts: [(clip, first_frame, n_frames)]."""
    return {"name": name, "ch": ch, "clips": clips, "cuts": cuts}


def edge_cases():
    rng = np.random.default_rng(20240911)
    cases = []
    # every channel count: the whole clip, one frame (first, middle, last), f0 in {1, 3, 17} (the is_raw window starts
    # at an odd byte), clips of 1, 2, 7 and 40 frames
    for ch in (1, 2, 3):
        clips = [J.make_blob(rng, ch, 40, raw=(2, 17, 39)), J.make_blob(rng, ch, 1), J.make_blob(rng, ch, 2, raw=(1,)), J.make_blob(rng, ch, 7)]
        cuts = [(0, 0, 40), (0, 0, 1), (0, 20, 1), (0, 39, 1), (0, 1, 5), (0, 3, 30), (0, 17, 23), (0, 17, 1),
                (1, 0, 1), (2, 0, 2), (2, 1, 1), (2, 0, 1), (3, 0, 7), (3, 3, 4), (3, 1, 5)]
        cases.append(case(f"windows_ch{ch}", ch, clips, cuts))
    # every dword phase of the funnel: ch f0 mod 4 and P0 mod 4 each take 0..3, and not only together
    cnt = [1, 1, 1, 1, 2, 1, 1, 1, 1, 3, 1, 1]
    cases.append(case("dword_phases", 1, [J.make_blob(rng, 1, 12, cnt=cnt)], [(0, f0, nf) for f0 in range(11) for nf in (1, 12 - f0)]))
    cases.append(case("dword_phases_ch3", 3, [J.make_blob(rng, 3, 9, cnt=[1] * 27)], [(0, f0, 9 - f0) for f0 in range(9)]))
    # a window with no pairs between rows that have some; a window whose rows are all raw; raw frames only in front
    cnt = [5, 6, 7, 8, 0, 0, 0, 0, 0, 0, 9, 10, 11, 12]
    cases.append(case("no_pairs_in_window", 2, [J.make_blob(rng, 2, 7, cnt=cnt)], [(0, 2, 3), (0, 2, 1), (0, 1, 5)]))
    cases.append(case("raw_windows", 2, [J.make_blob(rng, 2, 10, raw=(0, 1, 4, 5, 6))],
                      [(0, 4, 3), (0, 5, 1), (0, 7, 3), (0, 2, 2), (0, 0, 2), (0, 3, 5)]))
    # mono pieces of 16 and 64 frames: the is_raw run ends exactly on 16 and on 64 bytes, the dword runs on 64 and 256
    cases.append(case("runs_end_on_16_and_64", 1, [J.make_blob(rng, 1, 70, raw=(9, 66))], [(0, 3, 16), (0, 5, 64), (0, 0, 64), (0, 54, 16)]))
    # 8 full rows (32 KiB of pairs) and 8 raw rows (32 KiB of planes): more than one tile holds a single run
    full = J.make_blob(rng, 1, 10, cnt=[3] + [HOP] * 8 + [5])
    planes = J.make_blob(rng, 1, 10, raw=range(1, 9))
    cases.append(case("runs_longer_than_a_tile", 1, [full, planes], [(0, 1, 8), (1, 1, 8), (0, 0, 10), (1, 0, 10)]))
    # many one-frame pieces in one tile
    cases.append(case("one_frame_pieces", 2, [J.make_blob(rng, 2, 40, raw=(11, 12))], [(0, f, 1) for f in range(40)]))
    # 1, 2 and 1025 cuts: 1025 crosses the scan's chunk
    small = [J.make_blob(rng, 1, 5, raw=(3,)), J.make_blob(rng, 1, 3)]
    for n in (1, 2, 1025):
        cuts = [(int(c), int(f0), int(rng.integers(1, (5, 3)[c] - f0 + 1))) for c, f0 in
                ((c, rng.integers(0, (5, 3)[c])) for c in rng.integers(0, 2, n))]
        cases.append(case(f"cuts_{n}", 1, small, cuts))
    # duplicate, overlapping and descending cuts
    cases.append(case("any_order", 3, [J.make_blob(rng, 3, 12, raw=(6,)), J.make_blob(rng, 3, 4)],
                      [(1, 2, 2), (0, 8, 4), (0, 4, 6), (0, 4, 6), (0, 0, 5), (1, 0, 4), (0, 6, 1), (1, 2, 2)]))
    return cases


def partitions():
    """(name, channels, blob, the frame counts of a partition of it)."""
    rng = np.random.default_rng(20240912)
    return [("stereo", 2, J.make_blob(rng, 2, 23, raw=(4, 5, 22)), [1, 3, 1, 7, 2, 9]),
            ("mono", 1, J.make_blob(rng, 1, 17, raw=(0,)), [16, 1]),
            ("three", 3, J.make_blob(rng, 3, 9), [4, 5]),
            ("whole", 2, J.make_blob(rng, 2, 6, raw=(2,)), [6])]


def store_of(c, rng, gap=True):
    """The source store of a case: (arena bytes, entries rows) - the clips' blobs at multiples of 64, the pattern between and
    around them."""
    chunks, entries, at = [], [], 0
    for b in c["clips"]:
        pad = 64 * int(rng.integers(1, 4)) if gap else 0
        chunks.append(np.full(pad, PATTERN, np.uint8))
        at += pad
        _, _, _, n_pairs, n_raw, _ = J.parse_header(b)
        entries.append([at, len(b), n_pairs, n_raw, 1])
        chunks.append(np.frombuffer(b, np.uint8))
        at += len(b)
    chunks.append(np.full(192, PATTERN, np.uint8))
    return np.concatenate(chunks), entries


# ------------------------------------------------------------------------------------------ tile, section and grid edges
# Cases laid out against the mover's 16 KiB tiles of the packed destination space (tests/store_mover_paths.py names
# what each reaches, tests/test_store_mover_paths.py holds the union of all case lists to it).  Built on first use and
# kept, not at import.

def aligned_case(name, ch, clips, filler_clip, targets):
    """A case whose pieces lie where the tiles are.  targets: ((clip, f0, nf), anchor, want): one-frame pieces of
    `filler_clip` - whose frame k has 16 k pairs in its first row and none else, a piece of 256 + 64 k bytes - in front
    of the piece put its byte `anchor` on a packed offset that is `want` mod TILE (anchor None: no fillers).  Packed
    offsets count from the rounded-up cursor."""
    cuts, at = [], 0
    for (clip, f0, nf), anchor, want in targets:
        if anchor is not None:
            for k in J.fill((want - at - anchor) % TILE):
                cuts.append((filler_clip, k, 1))
                at += 256 + 64 * k
            assert (at + anchor) % TILE == want % TILE
        cuts.append((clip, f0, nf))
        at += len(cut(clips[clip], ch, f0, nf)[1])
    return case(name, ch, clips, cuts)


def _tiles_mono(rng):
    """A mono clip of 32800 frames: frames 32744..32759 hold one pair each, 32760..32770 are full rows (44 KiB of pairs),
    32790..32799 are raw (40 KiB of planes), everything in front is empty, so that long windows stay small."""
    F = 32800
    clip = J.make_blob(rng, 1, F, range(32790, 32800), J._rows(F, full=range(32760, 32771), some=[(f, 1) for f in range(32744, 32760)]))
    fill_clip = J.make_blob(rng, 1, 65, cnt=[16 * k for k in range(65)])
    # the whole clip with its is_raw run on a tile boundary: tiles inside one run in every section, source and
    # destination co-aligned
    targets = [((0, 0, F), 64, 0)]
    # the piece on a tile boundary and 32640 + e frames: tile 1 begins in the is_raw run and its last unit in the padding,
    # e bytes in the run's last unit; f0 = e gives the source phase
    for e in (1, 7, 15):
        targets.append(((0, e, 32640 + e), 0, 0))
    # the same with the run on the boundary and 16320 + e frames
    for e in (2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14):
        targets.append(((0, e, 16320 + e), 64, 0))
    # the scale run, then the cnt run, ends TILE - 64 + 4 q in a tile (4112 + q frames: 16 KiB and more)
    for which in (0, 1):
        for q in (1, 2, 3):
            n = 4112 + q
            targets.append(((0, 4 * which + q, n), 64 + J.a64(n) + which * J.a64(4 * n) + 4 * n - 4 * q, TILE - 64))
    # the pairs run: P0 = 12..15 pairs in front, 11264 + 4..1 in the window; where that is no multiple of 4, the run ends
    # TILE - 64 + 4 q in a tile
    for j in (12, 13, 14, 15):
        q = (16 - j) % 4
        targets.append(((0, 32744 + j, 30), J.layout(1, 30)[3] + 4 * (11 * HOP + 16 - j - q) if q else None, TILE - 64))
    # the planes
    targets.append(((0, 32780, 20), None, 0))
    return aligned_case("tiles_mono", 1, [clip, fill_clip], 1, targets)


def _tiles_three(rng):
    """Three channels: the dword windows start on dword 3 f0."""
    F = 14001
    clip = J.make_blob(rng, 3, F, (5, 6, 7000, 14000), J._rows(F, 3, full=(20, 21, 9000), some=[(f, 1 + f % 3) for f in range(16)]))
    cuts = [(0, f0, nf) for f0, nf in ((0, F), (1, 5500), (2, 9001), (3, 13998), (7, 6990), (6999, 7002), (9000, 1), (13990, 11))]
    return case("tiles_three_channels", 3, [clip], cuts)


def _small_phases(rng):
    """Small pieces, whose tiles hold many runs: every source phase f0 = 0..15 against every count of bytes in the last
    unit of the is_raw run, and the dword phases and counts that go with them."""
    clip = J.make_blob(rng, 1, 48, raw=(5, 20, 21), cnt=rng.integers(0, 4, 48))
    return case("small_phases", 1, [clip], [(0, i, 17 + i) for i in range(16)] + [(0, 15 - i, 1 + i) for i in range(15)])


def _grid_stride(rng):
    """The joined clips of the join's grid-stride case as the store: the 40 MiB of planes in the three pieces of its
    seams (2550 tiles, the grid is 2048), then pieces of the two small clips, one of them on a tile boundary: headers, run
    ends of every section and the call's short last tile all behind tile 2048."""
    c = J.heavy_case(J.GRID_CASE)
    clips = [J.join(blobs, 2) for blobs in c["clips"] if len(blobs) > 1]
    clips.append(J.make_blob(rng, 2, 65, cnt=[n for k in range(65) for n in (16 * k, 0)]))
    cuts = [(0, 0, 2000), (0, 2000, 2200), (0, 4200, 900), (1, 0, 51), (1, 3, 5), (2, 8, 1), (2, 0, 20), (2, 20, 31), (1, 40, 11), (2, 5, 3), (1, 17, 30)]
    return aligned_case("grid_stride", 2, clips, 3, [(c, 0 if c == (2, 0, 20) else None, 0) for c in cuts])


_HEAVY = {"tiles_mono": (_tiles_mono, 41), "tiles_three_channels": (_tiles_three, 42), "small_phases": (_small_phases, 43)}
TILE_CASES = tuple(_HEAVY)             # names: heavy_case(name) builds
GRID_CASE = "grid_stride"
_HEAVY[GRID_CASE] = (_grid_stride, 44)


@functools.lru_cache(maxsize=None)
def heavy_case(name):
    make, seed = _HEAVY[name]
    return make(np.random.default_rng(20250300 + seed))
