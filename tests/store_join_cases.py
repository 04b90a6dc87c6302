"""Cases and the numpy model of the segment join (include/glc.h glc_store_join_segments_device / glc_compact_join),
written from DESIGN.md section 3, "joining a clip's segments": parse every segment blob, judge it, concatenate the five
sections, write the header of the sums and zero padding; then the encoder's placement rule over the clips.

A blob here is made by the builder below, not by the codec: the join is structural and never looks at what a list or a
plane means.  The builder makes raw frames too (stream_decode_cases.compact_blob makes none)."""
import functools
import struct

import numpy as np

MAGIC = 0x42434C47
FRAME = 2048
HOP = 1024
PATTERN = 0xA5
TILE = 16384                          # bytes one workgroup moves at a time (csrc/glc_kernels.h kStoreMoveTile)
GRID = 2048                           # workgroups of a move launch at most (kStoreMoveGrid): tile GRID is a second pass
BAD_HEADER, PAIR_SUM, RAW_SUM, NO_BLOB = 1, 16, 32, 64


def a64(v: int) -> int:
    return (v + 63) & ~63


def layout(ch: int, nf: int):
    """(o_israw, o_scale, o_cnt, o_pairs) of a blob of nf frames."""
    m = nf * ch
    o_israw = 64
    o_scale = o_israw + a64(nf)
    o_cnt = o_scale + a64(4 * m)
    return o_israw, o_scale, o_cnt, o_cnt + a64(4 * m)


def raw_offset(ch: int, nf: int, n_pairs: int) -> int:
    return a64(layout(ch, nf)[3] + 4 * n_pairs)


def blob_bytes(ch: int, nf: int, n_pairs: int, n_raw_rows: int) -> int:
    return raw_offset(ch, nf, n_pairs) + n_raw_rows * FRAME * 2


def header(ch: int, nf: int, n_pairs: int, n_raw_rows: int, nbytes: int) -> bytes:
    return struct.pack("<IIQQQQ", MAGIC, ch, nf, n_pairs, n_raw_rows, nbytes) + bytes(24)


def parse_header(blob):
    return struct.unpack("<IIQQQQ", bytes(blob[:40]))


def make_blob(rng, ch: int, nf: int, raw=(), cnt=None) -> bytes:
    """A blob of nf frames.  raw: the frames (0-based, of this blob) that are raw; cnt: the list length of every row
    (nf * ch values; the rows of raw frames are forced to 0), default random 0..40.  Lists ascend strictly below 1024,
    the scales and planes are random bits."""
    m = nf * ch
    raw = set(raw)
    cnt = np.array(rng.integers(0, 41, m) if cnt is None else cnt, np.uint32).reshape(m).copy()
    israw = np.zeros(nf, np.uint8)
    for f in raw:
        israw[f] = 1
        cnt[f * ch:(f + 1) * ch] = 0
    scale = rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32)
    for f in raw:
        scale[f * ch:(f + 1) * ch] = 0
    pairs = []
    for n in cnt:
        if n == 0:                    # an empty row draws nothing from the generator: skipped, the bytes stay the same
            continue
        idx = np.sort(rng.choice(HOP, int(n), replace=False)).astype(np.uint32)
        q = rng.integers(0, 2 ** 16, int(n), dtype=np.uint32)
        pairs.append(idx | (q << 16))
    pairs = np.concatenate(pairs) if pairs else np.empty(0, np.uint32)
    n_pairs, n_raw = int(pairs.size), len(raw) * ch
    o_israw, o_scale, o_cnt, o_pairs = layout(ch, nf)
    out = np.zeros(blob_bytes(ch, nf, n_pairs, n_raw), np.uint8)
    out[:64] = np.frombuffer(header(ch, nf, n_pairs, n_raw, out.size), np.uint8)
    out[o_israw:o_israw + nf] = israw
    out[o_scale:o_scale + 4 * m] = scale.view(np.uint8)
    out[o_cnt:o_cnt + 4 * m] = cnt.view(np.uint8)
    out[o_pairs:o_pairs + 4 * n_pairs] = pairs.astype(np.uint32).view(np.uint8)
    out[raw_offset(ch, nf, n_pairs):] = rng.integers(0, 256, n_raw * FRAME * 2, dtype=np.uint8)
    return out.tobytes()


# ------------------------------------------------------------------------------------------ the model

def segment_status(blob, ch: int, n_frames: int) -> int:
    """The status word of a segment whose entry is usable and names the bytes `blob` (all of entry.bytes)."""
    blob = np.frombuffer(bytes(blob), np.uint8)
    if blob.size < 64:
        return BAD_HEADER
    magic, chs, nf, n_pairs, n_raw, nbytes = parse_header(blob)
    if magic != MAGIC or chs != ch or nf != n_frames:
        return BAD_HEADER
    m = nf * ch
    if n_pairs > m * HOP or n_raw > m or n_raw % ch:
        return BAD_HEADER
    need = blob_bytes(ch, nf, n_pairs, n_raw)
    if nbytes != need or blob.size < need:
        return BAD_HEADER
    o_israw, _, o_cnt, _ = layout(ch, nf)
    bits = 0
    if int(blob[o_cnt:o_cnt + 4 * m].view(np.uint32).astype(np.uint64).sum()) != n_pairs:
        bits |= PAIR_SUM
    if int(np.count_nonzero(blob[o_israw:o_israw + nf])) * ch != n_raw:
        bits |= RAW_SUM
    return bits


def join(blobs, ch: int) -> bytes:
    """The blob of the clip whose segments are `blobs`, in frame order.  ValueError("segment j") for an unusable one."""
    parts = [[] for _ in range(5)]
    F = P = R = 0
    for j, b in enumerate(blobs):
        b = np.frombuffer(bytes(b), np.uint8)
        nf = parse_header(b)[2] if b.size >= 64 else 0
        if nf == 0 or segment_status(b, ch, nf):
            raise ValueError(f"segment {j}")
        _, _, _, n_pairs, n_raw, _ = parse_header(b)
        o_israw, o_scale, o_cnt, o_pairs = layout(ch, nf)
        m = nf * ch
        o_raw = raw_offset(ch, nf, n_pairs)
        for k, (at, n) in enumerate(((o_israw, nf), (o_scale, 4 * m), (o_cnt, 4 * m), (o_pairs, 4 * n_pairs), (o_raw, n_raw * FRAME * 2))):
            parts[k].append(b[at:at + n])
        F, P, R = F + nf, P + n_pairs, R + n_raw
    out = np.zeros(blob_bytes(ch, F, P, R), np.uint8)
    out[:64] = np.frombuffer(header(ch, F, P, R, out.size), np.uint8)
    starts = layout(ch, F) + (raw_offset(ch, F, P),)
    for at, runs in zip(starts, parts):
        run = np.concatenate(runs) if runs else np.empty(0, np.uint8)
        out[at:at + run.size] = run
    return out.tobytes()


def join_store(arena, arena_bytes: int, entries, segs, lengths, ch: int, dst, dst_bytes: int, cursor: int):
    """The device call.  arena: uint8 array; entries: per segment [offset, bytes, n_pairs, n_raw_rows, stored]; segs:
    [(stream, first_frame, n_frames)]; dst: uint8 array, a copy of which is written.  Returns a dict of the destination
    arena, entries_out (rows of 5), lengths_out (or None), status and the cursor."""
    dst = np.array(dst, np.uint8)
    status, clips = [], []
    for j, ((stream, _, nf), (off, nb, _, _, stored)) in enumerate(zip(segs, entries)):
        if stored == 0 or off % 64 or off > arena_bytes or nb > arena_bytes - off:
            status.append(NO_BLOB | BAD_HEADER)
        else:
            status.append(segment_status(arena[off:off + nb], ch, nf))
        if not clips or clips[-1][0] != stream:
            clips.append((stream, []))
        clips[-1][1].append(j)
    at = a64(cursor)
    entries_out, lengths_out = [], []
    for c, (_, js) in enumerate(clips):
        if any(status[j] for j in js):
            entries_out.append([0, 0, 0, 0, 0])
            lengths_out.append(0)
            continue
        blob = np.frombuffer(join([arena[entries[j][0]:entries[j][0] + entries[j][1]] for j in js], ch), np.uint8)
        _, _, _, n_pairs, n_raw, _ = parse_header(blob)
        stored = at <= dst_bytes and blob.size <= dst_bytes - at
        if stored:
            dst[at:at + blob.size] = blob
        entries_out.append([at, blob.size, n_pairs, n_raw, int(stored)])
        lengths_out.append(lengths[c] if lengths is not None else 0)
        at += blob.size
    return {"dst": dst, "entries": entries_out, "lengths": lengths_out if lengths is not None else None, "status": status,
            "cursor": at}


def entry_words(rows) -> np.ndarray:
    """Rows [offset, bytes, n_pairs, n_raw_rows, stored] as the (n, 4) int64 words of glc_store_entry."""
    out = np.zeros((len(rows), 4), np.uint64)
    for i, (off, nb, p, r, stored) in enumerate(rows):
        out[i] = (off, nb, p, r | (stored << 32))
    return out.view(np.int64)


def clip_length(nf: int) -> int:
    """A length (samples per channel) whose clip has nf frames: glc_plan_encode(1024 nf, 1).n_frames == nf."""
    return HOP * nf


# ------------------------------------------------------------------------------------------ damage

def damaged(blob: bytes, kind: str, ch: int):
    """(the blob damaged in the named way, the status bits the join gives it)."""
    b = np.frombuffer(blob, np.uint8).copy()
    magic, chs, nf, n_pairs, n_raw, nbytes = parse_header(b)
    o_israw, _, o_cnt, _ = layout(ch, nf)

    def put(**kw):
        f = dict(magic=magic, chs=chs, nf=nf, n_pairs=n_pairs, n_raw=n_raw, nbytes=nbytes)
        f.update(kw)
        b[:40] = np.frombuffer(struct.pack("<IIQQQQ", f["magic"], f["chs"], f["nf"], f["n_pairs"], f["n_raw"], f["nbytes"]), np.uint8)
    if kind == "magic":
        put(magic=magic ^ 0x100)
    elif kind == "channels":
        put(chs=ch + 1)
    elif kind == "frames":
        put(nf=nf + 64)
    elif kind == "bytes":
        put(nbytes=nbytes + 64)
    elif kind == "cnt_sum":
        b[o_cnt:o_cnt + 4].view(np.uint32)[0] += 1
        return b.tobytes(), PAIR_SUM
    elif kind == "raw_count":
        f = int(np.flatnonzero(b[o_israw:o_israw + nf] == 0)[0])
        b[o_israw + f] = 1
        return b.tobytes(), RAW_SUM
    else:
        raise KeyError(kind)
    return b.tobytes(), BAD_HEADER


DAMAGE = ("magic", "channels", "frames", "cnt_sum", "raw_count", "bytes")


# ------------------------------------------------------------------------------------------ the cases

def case(name, ch, clips):
    """clips: per clip the list of its segment blobs."""
    return {"name": name, "ch": ch, "clips": clips}


def clip_of(rng, ch, seg_frames, raw=(), cnt=None):
    """The segments of one clip: seg_frames[k] frames each; raw: the CLIP's raw frames; cnt: a function (first frame,
    frames) -> the rows' list lengths, or None."""
    out, f0 = [], 0
    for nf in seg_frames:
        out.append(make_blob(rng, ch, nf, [f - f0 for f in raw if f0 <= f < f0 + nf], cnt(f0, nf) if cnt else None))
        f0 += nf
    return out


def edge_cases():
    rng = np.random.default_rng(20240607)
    cases = []
    # every channel count against segments of 1, 63, 64 and 65 frames: the is_raw run of a segment lands on bytes 0, 1,
    # 2, 3, 66, 130, 194 (every residue mod 16 that a one-frame step, a 63 and a 65 reach); first_frame * ch takes the
    # residues 0..3 mod 4 dwords for mono and 3 channels, 0 and 2 for stereo, 0 for 8
    for ch in (1, 2, 3, 8):
        frames = [1, 1, 1, 63, 64, 65]
        cases.append(case(f"frames_ch{ch}", ch, [clip_of(rng, ch, frames, raw=(2, 70)), clip_of(rng, ch, frames[::-1])]))
    # pairs per segment 0, 1, 15, 16, 17: one-frame mono segments whose one row has that many pairs
    cases.append(case("pairs_per_segment", 1, [[make_blob(rng, 1, 1, cnt=[n]) for n in (0, 1, 15, 16, 17, 0, 0, 16, 1)]]))
    # the pair section ends exactly on a 64-byte boundary (32 pairs), and one dword past it (33)
    cases.append(case("pairs_end_on_64", 2, [[make_blob(rng, 2, 1, cnt=[7, 9]), make_blob(rng, 2, 1, cnt=[16, 0])],
                                             [make_blob(rng, 2, 1, cnt=[7, 9]), make_blob(rng, 2, 1, cnt=[16, 1])]]))
    # a segment that is all raw, between two that are not; a clip that is all raw
    cases.append(case("all_raw_segment", 2, [clip_of(rng, 2, [3, 2, 3], raw=(3, 4)), clip_of(rng, 2, [1, 2], raw=(0, 1, 2))]))
    # the clip's raw frames are the last frame of one segment and the first of the next
    cases.append(case("raw_across_a_seam", 3, [clip_of(rng, 3, [5, 4], raw=(4, 5))]))
    # one segment: the join is the segment itself
    cases.append(case("one_segment", 2, [clip_of(rng, 2, [17], raw=(9,))]))
    # 1, 2 and 20 segments per clip, rows with no pairs at all among them
    cases.append(case("segments_1_2_20", 2, [clip_of(rng, 2, [4]), clip_of(rng, 2, [3, 5]),
                                             clip_of(rng, 2, [1 + k % 3 for k in range(20)], raw=(7, 8, 30),
                                                     cnt=lambda f0, nf: [0] * (2 * nf) if f0 % 4 == 0 else None)]))
    # 1, 3 and 1500 clips of one-frame mono segments: 1500 crosses the scan block of 1024
    for n in (1, 3, 1500):
        cases.append(case(f"clips_{n}", 1, [[make_blob(rng, 1, 1, cnt=[int(rng.integers(0, 20))])] for _ in range(n)]))
    # 1500 segments in few clips: the segment scan crosses its block too
    cases.append(case("segments_1500", 1, [[make_blob(rng, 1, 1, cnt=[int(rng.integers(0, 5))]) for _ in range(n)] for n in (700, 1, 799)]))
    # long rows: a clip of more than one move tile whose seams fall inside tiles
    cases.append(case("long_rows", 2, [clip_of(rng, 2, [9, 7, 11], raw=(10,), cnt=lambda f0, nf: rng.integers(200, 700, 2 * nf))]))
    return cases


def store_of(c, rng, gap=True):
    """The source store of a case: (arena bytes, entries rows, segs, lengths) - the blobs at multiples of 64 in segment
    order, random bytes between and around them."""
    chunks, entries, segs, lengths, at = [], [], [], [], 0
    for s, blobs in enumerate(c["clips"]):
        f0 = 0
        for b in blobs:
            pad = 64 * int(rng.integers(1, 4)) if gap else 0
            chunks.append(rng.integers(0, 256, pad, dtype=np.uint8))
            at += pad
            _, _, nf, n_pairs, n_raw, _ = parse_header(b)
            entries.append([at, len(b), n_pairs, n_raw, 1])
            segs.append((10 * s + 3, f0, nf))         # stream values ascend, they need not be 0, 1, ..
            chunks.append(np.frombuffer(b, np.uint8))
            at += len(b)
            f0 += nf
        lengths.append(clip_length(f0))
    chunks.append(rng.integers(0, 256, 192, dtype=np.uint8))
    return np.concatenate(chunks), entries, segs, lengths


# ------------------------------------------------------------------------------------------ tile, section and grid edges
# Cases laid out against the mover's 16 KiB tiles of the packed destination space (tests/store_mover_paths.py names
# what each reaches, tests/test_store_mover_paths.py holds the union of all case lists to it).  They are heavy - tens of
# thousands of rows, tens of MiB - so they are built on first use and kept, not at import.

def filler(ch: int, k: int) -> bytes:
    """A one-frame blob of 256 + 64 k bytes (k in 0..64; ch <= 16): what stands between two clips to move the next."""
    assert 0 <= k <= 64 and ch <= 16
    return _filler(ch, k)


@functools.lru_cache(maxsize=None)
def _filler(ch, k):
    return make_blob(np.random.default_rng(7000 + 100 * ch + k), ch, 1, cnt=[16 * k] + [0] * (ch - 1))


def fill(gap: int):
    """The k of fillers whose sizes sum to `gap` bytes (a multiple of 64) or, where gap < 256, to gap + TILE."""
    assert gap % 64 == 0 and 0 <= gap < TILE
    if gap == 0:
        return []
    if gap < 256:
        gap += TILE
    out = []
    while gap:
        size = gap if gap <= 4352 else min(4352, gap - 256)
        out.append((size - 256) // 64)
        gap -= size
    return out


def joined_bytes(blobs, ch: int) -> int:
    F, P, R = (sum(parse_header(b)[k] for b in blobs) for k in (2, 3, 4))
    return blob_bytes(ch, F, P, R)


def aligned_case(name, ch, targets):
    """A case whose clips lie where the tiles are.  targets: (segment blobs, anchor, want): one-frame filler clips in
    front of the clip put byte `anchor` of its joined blob on a packed offset that is `want` mod TILE (anchor None: no
    fillers).  Packed offsets count from the rounded-up cursor."""
    clips, at = [], 0
    for blobs, anchor, want in targets:
        if anchor is not None:
            for k in fill((want - at - anchor) % TILE):
                clips.append([filler(ch, k)])
                at += 256 + 64 * k
            assert (at + anchor) % TILE == want % TILE
        clips.append(blobs)
        at += joined_bytes(blobs, ch)
    return case(name, ch, clips)


def _rows(nf, ch=1, full=(), some=()):
    """List lengths of nf frames: 1024 in the frames `full` (every channel), n pairs in frame f for (f, n) of `some`;
    frames at or behind nf are passed over."""
    cnt = np.zeros(nf * ch, np.uint32)
    for f in full:
        cnt[f * ch:(f + 1) * ch] = HOP
    for f, n in some:
        cnt[f * ch:f * ch + 1] = n
    return cnt


def _tiles_mono(rng):
    """One long mono clip for the one-run tiles with and without seams, then clips whose runs end 16 to 63 bytes in
    front of a tile boundary, in every section and with every count of bytes in the run's last unit."""
    # 15 segments of 1025 frames and one of 25000: the is_raw run starts on a tile; its seams lie at 1025 k, on every
    # residue 1..15, all inside the first tile, and the next tile has none; the dword runs have seams at 4100 k.  Every
    # segment but the 8th has two full rows and k mod 4 pairs more (the pairs seams take every dword residue, the 8th
    # is an empty part between two seams); the last has nine full rows: 36 KiB of pairs without a seam.  Raw frames:
    # the last six of segment 3, none in segment 4, the first six of segment 5 (an empty part between two seams inside
    # 48 KiB of planes), and nine in the last segment.
    segs, f0 = [], 0
    for k in range(15):
        raw = range(1019, 1025) if k == 3 else range(6) if k == 5 else ()
        cnt = _rows(1025) if k == 7 else _rows(1025, full=(10, 11), some=((12, k % 4),))
        segs.append(make_blob(rng, 1, 1025, raw, cnt))
    segs.append(make_blob(rng, 1, 25000, range(14625, 14634), _rows(25000, full=range(100, 109))))
    targets = [(segs, 64, 0)]
    # the is_raw run ends 16320 + e bytes behind a tile boundary, e = 1..15: the tile begins in the run and its last unit
    # in the padding; a seam nine frames in front of the end
    for e in range(1, 16):
        F = 16320 + e
        targets.append(([make_blob(rng, 1, F - 9, cnt=_rows(F - 9)), make_blob(rng, 1, 9, cnt=_rows(9, some=((0, 3),)))], 64, 0))
    # the scale run, then the cnt run, ends TILE - 64 + e in a tile, e = 4, 8, 12 (4113 .. 4115 frames: 16 KiB and more)
    for which in (0, 1):
        for q in (1, 2, 3):
            F = 4112 + q
            end = 64 + a64(F) + which * a64(4 * F) + 4 * F
            targets.append(([make_blob(rng, 1, 4000, cnt=_rows(4000)), make_blob(rng, 1, F - 4000, (5,), _rows(F - 4000))], end - 4 * q, TILE - 64))
    # the pairs run likewise: five full rows and q pairs
    for q in (1, 2, 3):
        blobs = [make_blob(rng, 1, 5, cnt=_rows(5, full=(0, 1, 2))), make_blob(rng, 1, 3, cnt=_rows(3, full=(0, 2), some=((1, q),)))]
        targets.append((blobs, layout(1, 8)[3] + 4 * 5 * HOP, TILE - 64))
    return aligned_case("tiles_mono", 1, targets)


def _tiles_three(rng):
    """Three channels, odd frame counts, one segment of one frame: the dword runs' seams at 12 first_frame."""
    frames = [4673, 4661, 1, 4666]
    segs = clip_of(rng, 3, frames, raw=(4672, 4673, 9000, 9335), cnt=lambda f0, nf: _rows(nf, 3, full=(7, 8), some=((9, 1 + f0 % 3),)))
    small = clip_of(rng, 3, [2, 1, 5, 3], raw=(3,))
    return aligned_case("tiles_three_channels", 3, [(segs, None, 0), (small, None, 0), (small[::-1], 64, 0)])


def _small_phases(rng):
    """Small clips, whose tiles hold many runs: sixteen segments of 33 frames (seams and source phases on every residue),
    and a clip of 16 + e frames for every e = 1..15 (every count of bytes in a run's last unit)."""
    clips = [clip_of(rng, 1, [33] * 16, raw=(32, 33, 70), cnt=lambda f0, nf: rng.integers(0, 4, nf))]
    clips += [clip_of(rng, 1, [16, e], cnt=lambda f0, nf: rng.integers(0, 4, nf)) for e in range(1, 16)]
    clips += [clip_of(rng, 1, [3, 2, 4], cnt=lambda f0, nf: [q] + [0] * (nf - 1)) for q in (1, 2, 3)]
    return case("small_phases", 1, clips)


def _grid_stride(rng):
    """Stereo, 5100 raw frames in three segments - 40 MiB of planes, 2550 tiles, the grid is 2048 -, the second seam of
    the planes behind tile 2048; then two small clips of twelve segments each, the second on a tile boundary: headers, seams
    of every section and the call's short last tile all behind tile 2048."""
    big = [make_blob(rng, 2, nf, range(nf), _rows(nf, 2)) for nf in (2000, 2200, 900)]
    frames = [3, 5, 1, 7, 2, 9, 4, 1, 6, 2, 8, 3]
    small = [clip_of(rng, 2, frames[k:] + frames[:k], raw=(4, 5, 20, 21, 40), cnt=lambda f0, nf: rng.integers(100, 700, 2 * nf)) for k in (0, 5)]
    return aligned_case("grid_stride", 2, [(big, None, 0), (small[0], None, 0), (small[1], 0, 0)])


_HEAVY = {"tiles_mono": (_tiles_mono, 31), "tiles_three_channels": (_tiles_three, 32), "small_phases": (_small_phases, 33)}
TILE_CASES = tuple(_HEAVY)             # names: heavy_case(name) builds
GRID_CASE = "grid_stride"
_HEAVY[GRID_CASE] = (_grid_stride, 34)


@functools.lru_cache(maxsize=None)
def heavy_case(name):
    make, seed = _HEAVY[name]
    return make(np.random.default_rng(20250300 + seed))
