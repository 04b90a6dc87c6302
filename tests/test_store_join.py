"""Joining a streamed clip's segments into one store blob on the device: glc_store_join_segments_device and
join_segments_tensor (include/glc.h "joining a streamed clip's segments").

Every comparison is exact - bytes and integers.  The synthetic tests run on blobs the builder of
tests/store_join_cases.py makes (held to the host twin by tests/test_store_join_model.py): the whole destination arena,
both output arrays, the status words and the cursor are held to the numpy model, and every byte that must stay untouched
to the 0xA5 pattern.  The codec tests push clips through the streaming encoder in random chunkings, join, and demand
the bytes the batch encode stores and the bits it decodes to.  Damaged blobs and entries are those of the case lists
(every count inside its buffer): the tests pin the defined result, they provoke nothing."""
import ctypes as C

import numpy as np
import pytest

import store_join_cases as J

pytestmark = pytest.mark.gpu

EINVAL = -1
SR = 44100
HOP = 1024
MARGIN = 256                       # pattern bytes behind every buffer


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    assert hasattr(g.lib, "glc_store_join_segments_device")
    yield g
    _ctx.clear()             # contexts: released while the library is still loaded


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


_ctx = {}


def ctx(g, kind, ch=2):
    key = (kind, ch)
    if key not in _ctx:
        _ctx[key] = g.Decoder(ch, SR) if kind in ("dec", "mover") else g.Encoder(SR)
    return _ctx[key]


def dev(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


def padded(data, margin=MARGIN):
    return np.concatenate([np.ascontiguousarray(data).view(np.uint8).reshape(-1), np.full(margin, J.PATTERN, np.uint8)])


def seg_array(g, segs):
    return (g._lib.GlcStreamSeg * max(len(segs), 1))(*[g._lib.GlcStreamSeg(*s) for s in segs])


def run_join(g, torch, arena_h, arena_bytes, entries, segs, lengths, ch, dst_h, dst_bytes, cursor, name="", mover=None):
    """One call on buffers with pattern margins, then everything the call may have touched against the model.  arena_h
    may be longer than arena_bytes (a guard the call must not read); dst_h is the destination as it is before the call."""
    mover = mover or ctx(g, "mover")
    n, n_clips = len(segs), len({s[0] for s in segs})
    want = J.join_store(arena_h, arena_bytes, entries, segs, lengths, ch, dst_h, dst_bytes, cursor)
    arena = dev(torch, padded(arena_h))
    dst = dev(torch, padded(dst_h))
    assert arena.data_ptr() % 64 == 0 and dst.data_ptr() % 64 == 0
    ent_in = dev(torch, padded(J.entry_words(entries)))
    ent_out = dev(torch, np.full(32 * n_clips + MARGIN, J.PATTERN, np.uint8))
    len_out = dev(torch, np.full(8 * n_clips + MARGIN, J.PATTERN, np.uint8)) if lengths is not None else None
    status = dev(torch, np.full(4 * n + MARGIN, J.PATTERN, np.uint8))
    cur = dev(torch, padded(np.array([cursor], np.uint64)))
    lens = (C.c_uint64 * n_clips)(*lengths) if lengths is not None else None
    torch.cuda.synchronize()
    rc = g.lib.glc_store_join_segments_device(
        mover._h, arena.data_ptr(), arena_bytes, ent_in.data_ptr(), seg_array(g, segs), n, lens, ch, dst.data_ptr(), dst_bytes,
        cur.data_ptr(), ent_out.data_ptr(), len_out.data_ptr() if lengths is not None else None, status.data_ptr())
    assert rc == 0, g.lib.glc_last_error(mover._h)
    mover.synchronize()
    # ---- the host enters here
    got = status.cpu().numpy()
    assert got[:4 * n].view(np.uint32).tolist() == want["status"], name
    assert np.all(got[4 * n:] == J.PATTERN)
    got = cur.cpu().numpy()
    assert int(got[:8].view(np.uint64)[0]) == want["cursor"], name
    assert np.all(got[8:] == J.PATTERN)
    got = ent_out.cpu().numpy()
    assert np.array_equal(got[:32 * n_clips].view(np.int64).reshape(n_clips, 4), J.entry_words(want["entries"])), name
    assert np.all(got[32 * n_clips:] == J.PATTERN)
    if lengths is not None:
        got = len_out.cpu().numpy()
        assert got[:8 * n_clips].view(np.int64).tolist() == want["lengths"], name
        assert np.all(got[8 * n_clips:] == J.PATTERN)
    got = dst.cpu().numpy()
    diff = np.nonzero(got[:dst_h.size] != want["dst"])[0]
    assert diff.size == 0, (name, "first differing byte", int(diff[0]), "of", dst_h.size, "clip entries", want["entries"][:4])
    assert np.all(got[dst_h.size:] == J.PATTERN), name
    assert np.array_equal(arena.cpu().numpy(), padded(arena_h)) and np.array_equal(ent_in.cpu().numpy(), padded(J.entry_words(entries)))
    return want


# ------------------------------------------------------------------------------------------ 1: synthetic

CASES = J.edge_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_synthetic_against_the_model(glc_amd, torch, case):
    synthetic(glc_amd, torch, case)


@pytest.mark.parametrize("name", J.TILE_CASES + (J.GRID_CASE,))
def test_tile_section_and_grid_edges(glc_amd, torch, name):
    """The cases laid out against the mover's tiles (tests/store_join_cases.py "tile, section and grid edges"): tiles
    inside one run with and without seams, tiles that end in a run's padding, every source phase and seam position on
    both kinds of tile, and 40 MiB whose tiles outnumber the grid.  tests/test_store_mover_paths.py names what they reach."""
    synthetic(glc_amd, torch, J.heavy_case(name))


def synthetic(glc_amd, torch, case):
    rng = np.random.default_rng(11)
    arena_h, entries, segs, lengths = J.store_of(case, rng)
    total = sum(J.joined_bytes(blobs, case["ch"]) for blobs in case["clips"])
    dst_h = np.full(128 + total + 512, J.PATTERN, np.uint8)
    want = run_join(glc_amd, torch, arena_h, arena_h.size, entries, segs, lengths, case["ch"], dst_h, dst_h.size, 100, case["name"])
    assert all(e[4] == 1 for e in want["entries"]) and want["entries"][0][0] == 128 and want["cursor"] == 128 + total
    assert not any(want["status"])


def test_without_lengths_and_python_binding(glc_amd, torch):
    g = glc_amd
    case = next(c for c in CASES if c["name"] == "segments_1_2_20")
    arena_h, entries, segs, lengths = J.store_of(case, np.random.default_rng(12))
    dst_h = np.full(1 << 16, J.PATTERN, np.uint8)
    run_join(g, torch, arena_h, arena_h.size, entries, segs, None, case["ch"], dst_h, dst_h.size, 0, "no lengths")
    want = J.join_store(arena_h, arena_h.size, entries, segs, lengths, case["ch"], dst_h, dst_h.size, 64)
    out_arena, cursor = dev(torch, dst_h), torch.full((1,), 64, dtype=torch.int64, device="cuda")
    for obj in (ctx(g, "enc"), ctx(g, "dec")):
        cursor.fill_(64)
        ent, lens, status = obj.join_segments_tensor(dev(torch, arena_h), dev(torch, J.entry_words(entries)), segs, out_arena, cursor,
                                                     lengths=lengths, channels=case["ch"])
        torch.cuda.synchronize()
        assert np.array_equal(ent.cpu().numpy(), J.entry_words(want["entries"])) and lens.cpu().tolist() == want["lengths"]
        assert status.cpu().tolist() == want["status"] and int(cursor.cpu()[0]) == want["cursor"]
        assert np.array_equal(out_arena.cpu().numpy(), want["dst"])


MIB, FAR = 1 << 20, 1 << 32


def test_offsets_beyond_4_gib(glc_amd, torch):
    """Source and destination arenas of 2^32 + 4 MiB bytes, allocated and never filled: every segment lies above 2^32,
    the cursor just below it, so that the first clip lands below 2^32, the second across it and the others above.  Only
    the two windows are written and compared (the model runs on them, its offsets shifted); the first MiB of either
    arena, where an offset cut to 32 bits would land, keeps its pattern."""
    g = glc_amd
    rng = np.random.default_rng(31)
    ch = 2
    case = J.case("far", ch, next(c for c in CASES if c["name"] == "long_rows")["clips"] + three_clips(rng)["clips"])
    arena_h, entries, segs, lengths = J.store_of(case, rng)
    sizes = [J.joined_bytes(blobs, ch) for blobs in case["clips"]]
    size, base, win = FAR + 4 * MIB, FAR + MIB, FAR - MIB
    cursor = FAR - sizes[0] - 100
    dst_h = np.full(2 * MIB, J.PATTERN, np.uint8)
    want = J.join_store(arena_h, arena_h.size, entries, segs, lengths, ch, dst_h, size - win, cursor - win)
    assert want["entries"][1][0] + win < FAR < want["entries"][1][0] + win + sizes[1] and want["cursor"] < 2 * MIB
    arena = torch.empty(size, dtype=torch.uint8, device="cuda")
    dst = torch.empty(size, dtype=torch.uint8, device="cuda")
    arena[:3 * MIB] = J.PATTERN
    arena[base:base + arena_h.size] = dev(torch, arena_h)
    dst[:MIB] = J.PATTERN
    dst[win:win + 2 * MIB] = J.PATTERN
    n, n_clips = len(segs), len(sizes)
    far = [[e[0] + base] + e[1:] for e in entries]
    ent_in = dev(torch, J.entry_words(far))
    ent_out = dev(torch, np.full(32 * n_clips + MARGIN, J.PATTERN, np.uint8))
    len_out = dev(torch, np.full(8 * n_clips + MARGIN, J.PATTERN, np.uint8))
    status = dev(torch, np.full(4 * n + MARGIN, J.PATTERN, np.uint8))
    cur = dev(torch, np.array([cursor], np.uint64))
    torch.cuda.synchronize()
    mover = ctx(g, "mover")
    rc = g.lib.glc_store_join_segments_device(mover._h, arena.data_ptr(), size, ent_in.data_ptr(), seg_array(g, segs), n,
                                              (C.c_uint64 * n_clips)(*lengths), ch, dst.data_ptr(), size, cur.data_ptr(),
                                              ent_out.data_ptr(), len_out.data_ptr(), status.data_ptr())
    assert rc == 0, g.lib.glc_last_error(mover._h)
    mover.synchronize()
    got = status.cpu().numpy()
    assert got[:4 * n].view(np.uint32).tolist() == want["status"] == [0] * n and np.all(got[4 * n:] == J.PATTERN)
    assert int(cur.cpu()[0]) == want["cursor"] + win
    got = ent_out.cpu().numpy()
    assert np.array_equal(got[:32 * n_clips].view(np.int64).reshape(n_clips, 4), J.entry_words([[e[0] + win] + e[1:] for e in want["entries"]]))
    assert np.all(got[32 * n_clips:] == J.PATTERN)
    got = len_out.cpu().numpy()
    assert got[:8 * n_clips].view(np.int64).tolist() == want["lengths"] and np.all(got[8 * n_clips:] == J.PATTERN)
    got = dst[win:win + 2 * MIB].cpu().numpy()
    diff = np.nonzero(got != want["dst"])[0]
    assert diff.size == 0, ("first differing byte", int(diff[0]), "entries", want["entries"])
    assert bool((dst[:MIB] == J.PATTERN).all()) and bool((arena[:3 * MIB] == J.PATTERN).all())
    assert np.array_equal(arena[base:base + arena_h.size].cpu().numpy(), arena_h)
    del arena, dst
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ 2: end to end

def tone(ch, L, seed):
    t = np.arange(L, dtype=np.float64)[:, None]
    f = 180.0 * (1 + seed % 5) * (1 + 0.37 * np.arange(ch)[None, :])
    return (0.4 * np.sin(2 * np.pi * f * t / SR) + 0.1 * np.sin(2 * np.pi * 3.1 * f * t / SR)).astype(np.float32)


def batch_tensor(torch, clips, ch, dtype):
    """(B, C, T) planar, NaN (or a loud integer) behind every clip's length."""
    T = max(c.shape[0] for c in clips)
    x = np.full((len(clips), ch, T), np.nan if dtype == np.float32 else 12345, dtype)
    for i, c in enumerate(clips):
        x[i, :, :c.shape[0]] = c.T
    return dev(torch, x)


@pytest.mark.parametrize("ch,integer", ((2, False), (3, True)), ids=("stereo_f32", "3ch_int16"))
def test_streamed_clips_join_to_the_batch_encode(glc_amd, torch, ch, integer):
    g = glc_amd
    rng = np.random.default_rng(77 + ch)
    lens = [5000, 30000, 1537]
    clips = [tone(ch, lens[0], 1), (rng.standard_normal((lens[1], ch)) * 0.3).astype(np.float32), tone(ch, lens[2], 2)]
    dtype = np.int16 if integer else np.float32
    if integer:
        clips = [np.clip(np.round(c * 32767.0), -32768, 32767).astype(np.int16) for c in clips]
    bits = 16 if integer else None
    # the store the batch encode fills
    b_arena, b_cursor, b_entries = ctx(g, "enc").encode_compact_batch_tensor(batch_tensor(torch, clips, ch, dtype), lengths=lens, bits=bits)
    # the live arena the streaming encoder fills, every lane in its own random chunking
    se = g.StreamEncoder(SR, ch, n_streams=3)
    arena = torch.zeros(1 << 21, dtype=torch.uint8, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    sent, seg_list, ent_list = [0, 0, 0], [], []
    while any(s < n for s, n in zip(sent, lens)):
        take = [min(n - s, int(rng.integers(0, 9000))) for s, n in zip(sent, lens)]
        chunk = [c[s:s + k] for c, s, k in zip(clips, sent, take)]
        sent = [s + k for s, k in zip(sent, take)]
        x = batch_tensor(torch, [c if c.shape[0] else np.zeros((1, ch), dtype) for c in chunk], ch, dtype)
        # a lane finishes with the push that brings its last sample; a finished lane sends nothing more
        fin = [k > 0 and s == n for k, s, n in zip(take, sent, lens)]
        entries, segs = se.push_tensor(x, take, fin, arena, cursor, bits=bits)
        seg_list += segs
        ent_list.append(entries)
    order = sorted(range(len(seg_list)), key=lambda j: seg_list[j][:2])
    segs = [seg_list[j] for j in order]
    entries = torch.cat(ent_list)[torch.tensor(order, device="cuda")].contiguous()
    assert max(sum(1 for s in segs if s[0] == lane) for lane in range(3)) >= 2
    out_arena = torch.full((b_arena.numel() + 4096,), J.PATTERN, dtype=torch.uint8, device="cuda")
    out_cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    j_entries, j_lens, status = se.join_segments_tensor(arena, entries, segs, out_arena, out_cursor, lengths=lens)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(segs) and j_lens.cpu().tolist() == lens
    be, je = b_entries.cpu().numpy(), j_entries.cpu().numpy()
    assert np.array_equal(be[:, 1:], je[:, 1:]) and np.all(je[:, 3] >> 32 == 1)             # bytes, n_pairs, n_raw_rows | stored
    assert (be[1, 3] & 0xFFFFFFFF) > 0                                                       # the noise clip has raw frames
    joined, whole = ([b.cpu().numpy().tobytes() for b in g.store_blobs(a, e)] for a, e in ((out_arena, j_entries), (b_arena, b_entries)))
    assert joined == whole
    assert int(out_cursor.cpu()[0]) == int(b_cursor.cpu()[0])
    assert np.all(out_arena.cpu().numpy()[int(out_cursor.cpu()[0]):] == J.PATTERN)
    # a draw from the joined store is the draw from the batch-encoded store
    dec = ctx(g, "dec", ch)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")
    pick, starts = i64([0, 1, 2, 1]), i64([0, 100, 10, 20000])
    a = dec.decode_store_crops_tensor(b_arena, b_entries, i64(lens), pick, starts, HOP, max(lens))
    b = dec.decode_store_crops_tensor(out_arena, j_entries, j_lens, pick, starts, HOP, max(lens))
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    assert all(s.flags == 0 for s in dec.last_compact_status())


# ------------------------------------------------------------------------------------------ 3: damage and placement

def three_clips(rng, ch=2):
    return J.case("three", ch, [J.clip_of(rng, ch, [3, 2]), J.clip_of(rng, ch, [2, 4, 3], raw=(1, 7)), J.clip_of(rng, ch, [5])])


@pytest.mark.parametrize("kind", J.DAMAGE + ("not_stored", "offset_odd", "outside"))
def test_a_damaged_segment_refuses_its_clip_alone(glc_amd, torch, kind):
    g = glc_amd
    rng = np.random.default_rng(21)
    case = three_clips(rng)
    which = 3                                                   # the middle segment of the middle clip
    bits = J.NO_BLOB | J.BAD_HEADER
    if kind in J.DAMAGE:
        case["clips"][1][1], bits = J.damaged(case["clips"][1][1], kind, 2)
    arena_h, entries, segs, lengths = J.store_of(case, rng)
    arena_bytes = arena_h.size
    if kind == "not_stored":
        entries[which][4] = 0
    elif kind == "offset_odd":
        entries[which][0] += 32
    elif kind == "outside":
        # the entry points behind arena_bytes, into a guard of NaN bits that belongs to the tensor but not to the arena
        arena_bytes = arena_h.size
        arena_h = np.concatenate([arena_h, np.full(8192, 0xFF, np.uint8)])
        entries[which][0] = arena_bytes + 64
    dst_h = np.full(1 << 16, J.PATTERN, np.uint8)
    want = run_join(g, torch, arena_h, arena_bytes, entries, segs, lengths, 2, dst_h, dst_h.size, 0, kind)
    assert want["status"] == [0, 0, 0, bits, 0, 0]
    assert want["entries"][1] == [0, 0, 0, 0, 0] and want["lengths"][1] == 0
    assert want["entries"][2][0] == want["entries"][0][0] + want["entries"][0][1]        # as if the refused clip had size 0
    # a draw that selects the refused clip: +0.0 and GLC_COMPACT_NO_BLOB
    dec = ctx(g, "dec", 2)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")
    ent = dev(torch, J.entry_words(want["entries"]))
    out = dec.decode_store_crops_tensor(dev(torch, want["dst"]), ent, i64(lengths), i64([1]), i64([0]), 64, max(lengths))
    torch.cuda.synchronize()
    assert not out.cpu().numpy().view(np.uint32).any()
    assert dec.last_compact_status()[0].flags == J.NO_BLOB | J.BAD_HEADER


def test_placement_a_clip_that_does_not_fit_and_an_append(glc_amd, torch):
    g = glc_amd
    rng = np.random.default_rng(22)
    case = three_clips(rng, 3)
    arena_h, entries, segs, lengths = J.store_of(case, rng)
    sizes = [len(J.join(blobs, 3)) for blobs in case["clips"]]
    # too small for the last clip by one byte: not stored, nothing written, the cursor at the size that would have sufficed
    dst_bytes = 64 + sum(sizes) - 1
    dst_h = np.full(dst_bytes, J.PATTERN, np.uint8)
    want = run_join(g, torch, arena_h, arena_h.size, entries, segs, lengths, 3, dst_h, dst_bytes, 1, "does not fit")
    assert [e[4] for e in want["entries"]] == [1, 1, 0] and want["cursor"] == 64 + sum(sizes)
    assert np.all(want["dst"][64 + sizes[0] + sizes[1]:] == J.PATTERN)
    # a second join with the cursor of the first appends behind it
    dst_h = np.full(3 * sum(sizes), J.PATTERN, np.uint8)
    first = run_join(g, torch, arena_h, arena_h.size, entries, segs, lengths, 3, dst_h, dst_h.size, 0, "first")
    second = run_join(g, torch, arena_h, arena_h.size, entries, segs, lengths, 3, first["dst"], dst_h.size, first["cursor"], "append")
    assert second["entries"][0][0] == sum(sizes) and second["cursor"] == 2 * sum(sizes)
    assert np.array_equal(second["dst"][:sum(sizes)], second["dst"][sum(sizes):2 * sum(sizes)])


# ------------------------------------------------------------------------------------------ 4: family rules

def live(g):
    c = (C.c_uint64 * 4)()
    assert g.lib.glc_debug_live_resources(c) == 0
    return tuple(int(v) for v in c)


def test_host_rules_and_what_the_call_leaves(glc_amd, torch):
    g = glc_amd
    rng = np.random.default_rng(23)
    ch = 2
    stream = ctx(g, "enc").encode(tone(ch, 9 * HOP + 77, 3).reshape(-1), ch)      # by the shared encoder, before the count
    torch.cuda.synchronize()
    before = live(g)
    case = three_clips(rng, ch)
    arena_h, entries, segs, lengths = J.store_of(case, rng)
    dec = g.Decoder(ch, SR)
    # a resident stream and a completed compact decode on the context
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")
    good = J.join_store(arena_h, arena_h.size, entries, segs, lengths, ch, np.zeros(1 << 16, np.uint8), 1 << 16, 0)
    dec.decode_store_crops_tensor(dev(torch, good["dst"]), dev(torch, J.entry_words(good["entries"])), i64(lengths), i64([0, 2]),
                                  i64([5, 0]), 200, max(lengths))
    status = [(s.flags, s.n_bad_rows, s.first_bad_row) for s in dec.last_compact_status()]
    dec.decode(stream)                                               # behind the draw, which is a decode and forgets the stream
    resident = dec.resident_stream()
    assert resident != 0
    dst_h = np.full(1 << 16, J.PATTERN, np.uint8)
    run_join(g, torch, arena_h, arena_h.size, entries, segs, lengths, ch, dst_h, dst_h.size, 0, "family", mover=dec)
    assert dec.resident_stream() == resident
    assert [(s.flags, s.n_bad_rows, s.first_bad_row) for s in dec.last_compact_status()] == status

    # ---- the host rules: GLC_EINVAL before anything is queued, nothing changed
    n, n_clips = len(segs), 3
    arena, dst = dev(torch, padded(arena_h)), dev(torch, padded(dst_h))
    ent_in = dev(torch, J.entry_words(entries))
    ent_out = dev(torch, np.full(32 * n_clips + 64, J.PATTERN, np.uint8))
    len_out = dev(torch, np.full(8 * n_clips + 64, J.PATTERN, np.uint8))
    stat = dev(torch, np.full(4 * n + 64, J.PATTERN, np.uint8))
    cur = dev(torch, np.array([192, 0], np.uint64))
    A, D, EI, EO, LO, ST, CU = (t.data_ptr() for t in (arena, dst, ent_in, ent_out, len_out, stat, cur))

    def call(a=A, ab=arena_h.size, ei=EI, sg=segs, ns=None, ln=lengths, c=ch, d=D, db=dst_h.size, cu=CU, eo=EO, lo=LO, st=ST):
        ns = len(sg) if ns is None else ns
        lens = (C.c_uint64 * max(len(ln), 1))(*ln) if ln is not None else None
        return g.lib.glc_store_join_segments_device(dec._h, a, ab, ei, seg_array(g, sg), ns, lens, c, d, db, cu, eo, lo, st)

    def with_seg(j, **kw):
        out = list(segs)
        f = dict(zip(("stream", "first_frame", "n_frames"), out[j]))
        f.update(kw)
        out[j] = (f["stream"], f["first_frame"], f["n_frames"])
        return out

    assert call(ns=0) == 0                                                     # n_segs == 0: GLC_OK, the cursor stays
    refused = [
        call(a=None), call(ei=None), call(d=None), call(cu=None), call(eo=None), call(st=None), call(c=0),
        call(ln=None), call(lo=None),                                          # lengths and d_lengths_out: both or neither
        call(a=A + 32), call(d=D + 16), call(ei=EI + 4), call(cu=CU + 4), call(eo=EO + 4), call(lo=LO + 4), call(st=ST + 2),
        call(sg=with_seg(0, first_frame=1)),                                   # a clip's first segment starts at frame 0
        call(sg=with_seg(1, n_frames=0)),
        call(sg=with_seg(1, first_frame=segs[1][1] + 1)),                      # a gap
        call(sg=[segs[2], segs[3], segs[4], segs[0], segs[1], segs[5]]),       # streams do not ascend
        call(sg=[segs[0], segs[2], segs[1], segs[3], segs[4], segs[5]]),       # a clip's segments are not consecutive
        call(ln=[lengths[0], lengths[1] + HOP, lengths[2]]),                   # frames that are not the length's
        call(sg=with_seg(5, n_frames=1 << 31), ln=None, lo=None),              # rows past 32 bits
        call(d=A + 64, db=64), call(eo=A + 128), call(lo=D + 8), call(st=D + 64), call(cu=A + 8), call(eo=EI), call(st=EO),
        call(lo=EO + 8), call(cu=ST),
    ]
    assert refused == [EINVAL] * len(refused), refused
    dec.synchronize()
    torch.cuda.synchronize()
    assert cur.cpu().tolist() == [192, 0] and np.array_equal(dst.cpu().numpy(), padded(dst_h))
    for t in (ent_out, len_out, stat):
        assert np.all(t.cpu().numpy() == J.PATTERN)
    del arena, dst
    dec.close()
    assert live(g) == before
