"""Cutting stored clips into frame ranges on the device: glc_store_cut_device and cut_clips_tensor (include/glc.h
"cutting stored clips into frame ranges").

Every comparison is exact - bytes and integers.  The synthetic tests run on blobs the builder of
tests/store_join_cases.py makes (held to the host twin by tests/test_store_cut_model.py): the arena's gaps and all of the
destination are the 0xA5 pattern before the call, and the whole destination arena, the three output arrays and the
cursor are held to the numpy model afterwards, every byte that must stay untouched to the pattern.  The codec tests cut
what the batch encode stored at the seams a streaming encode of the same clips has, and demand the streaming encoder's
segment blobs, the original back from the join and the bits of the whole from the streaming decoder.  Damaged blobs and
entries are those of the case lists (every count inside its buffer): the tests pin the defined result, they provoke
nothing."""
import ctypes as C

import numpy as np
import pytest

import store_cut_cases as K
import store_join_cases as J

pytestmark = pytest.mark.gpu

EINVAL = -1
SR = 44100
HOP = 1024
MARGIN = 256                       # pattern bytes behind every buffer


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    assert hasattr(g.lib, "glc_store_cut_device")
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
    return np.concatenate([np.ascontiguousarray(data).view(np.uint8).reshape(-1), np.full(margin, K.PATTERN, np.uint8)])


def cut_array(g, cuts):
    return (g._lib.GlcStoreCut * max(len(cuts), 1))(*[g._lib.GlcStoreCut(*c) for c in cuts])


def run_cut(g, torch, arena_h, arena_bytes, entries, cuts, lengths, ch, dst_h, dst_bytes, cursor, name="", mover=None, n_entries=None):
    """One call on buffers with pattern margins, then everything the call may have touched against the model.  arena_h
    may be longer than arena_bytes (a guard the call must not read); dst_h is the destination as it is before the call."""
    mover = mover or ctx(g, "mover")
    n = len(cuts)
    n_entries = len(entries) if n_entries is None else n_entries
    want = K.cut_store(arena_h, arena_bytes, entries[:n_entries], cuts, lengths, ch, dst_h, dst_bytes, cursor)
    arena = dev(torch, padded(arena_h))
    dst = dev(torch, padded(dst_h))
    assert arena.data_ptr() % 64 == 0 and dst.data_ptr() % 64 == 0
    ent_in = dev(torch, padded(J.entry_words(entries)))
    ent_out = dev(torch, np.full(32 * n + MARGIN, K.PATTERN, np.uint8))
    len_out = dev(torch, np.full(8 * n + MARGIN, K.PATTERN, np.uint8))
    status = dev(torch, np.full(4 * n + MARGIN, K.PATTERN, np.uint8))
    cur = dev(torch, padded(np.array([cursor], np.uint64)))
    lens = (C.c_uint64 * n)(*lengths) if lengths is not None else None
    torch.cuda.synchronize()
    rc = g.lib.glc_store_cut_device(
        mover._h, arena.data_ptr(), arena_bytes, ent_in.data_ptr(), n_entries, cut_array(g, cuts), n, lens, ch, dst.data_ptr(), dst_bytes,
        cur.data_ptr(), ent_out.data_ptr(), len_out.data_ptr(), status.data_ptr())
    assert rc == 0, g.lib.glc_last_error(mover._h)
    mover.synchronize()
    # ---- the host enters here
    got = status.cpu().numpy()
    assert got[:4 * n].view(np.uint32).tolist() == want["status"], name
    assert np.all(got[4 * n:] == K.PATTERN)
    got = cur.cpu().numpy()
    assert int(got[:8].view(np.uint64)[0]) == want["cursor"], name
    assert np.all(got[8:] == K.PATTERN)
    got = ent_out.cpu().numpy()
    assert np.array_equal(got[:32 * n].view(np.int64).reshape(n, 4), J.entry_words(want["entries"])), name
    assert np.all(got[32 * n:] == K.PATTERN)
    got = len_out.cpu().numpy()
    assert got[:8 * n].view(np.int64).tolist() == want["lengths"], name
    assert np.all(got[8 * n:] == K.PATTERN)
    got = dst.cpu().numpy()
    diff = np.nonzero(got[:dst_h.size] != want["dst"])[0]
    assert diff.size == 0, (name, "first differing byte", int(diff[0]), "of", dst_h.size, "entries", want["entries"][:4])
    assert np.all(got[dst_h.size:] == K.PATTERN), name
    assert np.array_equal(arena.cpu().numpy(), padded(arena_h)) and np.array_equal(ent_in.cpu().numpy(), padded(J.entry_words(entries)))
    return want


# ------------------------------------------------------------------------------------------ 1: synthetic

CASES = K.edge_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_synthetic_against_the_model(glc_amd, torch, case):
    synthetic(glc_amd, torch, case)


@pytest.mark.parametrize("name", K.TILE_CASES + (K.GRID_CASE,))
def test_tile_section_and_grid_edges(glc_amd, torch, name):
    """The cases laid out against the mover's tiles (tests/store_cut_cases.py "tile, section and grid edges"): tiles
    inside one run and tiles that end in its padding, in every section, every source phase and every count of bytes in
    a run's last unit on both kinds of tile, and 40 MiB whose tiles outnumber the grid.  tests/test_store_mover_paths.py
    names what they reach."""
    synthetic(glc_amd, torch, K.heavy_case(name))


def synthetic(glc_amd, torch, case):
    rng = np.random.default_rng(11)
    arena_h, entries = K.store_of(case, rng)
    ch, cuts = case["ch"], case["cuts"]
    total = sum(len(K.cut(case["clips"][c], ch, f0, nf)[1]) for c, f0, nf in cuts)
    dst_h = np.full(128 + total + 512, K.PATTERN, np.uint8)
    lengths = [HOP * nf - (i % 3) for i, (_, _, nf) in enumerate(cuts)]          # each plans to nf frames
    want = run_cut(glc_amd, torch, arena_h, arena_h.size, entries, cuts, lengths, ch, dst_h, dst_h.size, 100, case["name"])
    assert all(e[4] == 1 for e in want["entries"]) and want["entries"][0][0] == 128 and want["cursor"] == 128 + total
    assert not any(want["status"]) and want["lengths"] == lengths


def test_without_lengths_and_python_binding(glc_amd, torch):
    g = glc_amd
    case = next(c for c in CASES if c["name"] == "any_order")
    arena_h, entries = K.store_of(case, np.random.default_rng(12))
    ch, cuts = case["ch"], case["cuts"]
    dst_h = np.full(1 << 17, K.PATTERN, np.uint8)
    want = run_cut(g, torch, arena_h, arena_h.size, entries, cuts, None, ch, dst_h, dst_h.size, 0, "no lengths")
    assert want["lengths"] == [HOP * nf for _, _, nf in cuts]
    want = K.cut_store(arena_h, arena_h.size, entries, cuts, None, ch, dst_h, dst_h.size, 64)
    out_arena, cursor = dev(torch, dst_h), torch.full((1,), 64, dtype=torch.int64, device="cuda")
    for obj, given in ((ctx(g, "enc"), cuts), (ctx(g, "dec"), np.array(cuts, np.int64))):
        cursor.fill_(64)
        out_arena.fill_(K.PATTERN)
        ent, lens, status = obj.cut_clips_tensor(dev(torch, arena_h), dev(torch, J.entry_words(entries)), given, out_arena, cursor, channels=ch)
        torch.cuda.synchronize()
        assert np.array_equal(ent.cpu().numpy(), J.entry_words(want["entries"])) and lens.cpu().tolist() == want["lengths"]
        assert status.cpu().tolist() == want["status"] and int(cursor.cpu()[0]) == want["cursor"]
        assert np.array_equal(out_arena.cpu().numpy(), want["dst"])


MIB, FAR = 1 << 20, 1 << 32


def test_offsets_beyond_4_gib(glc_amd, torch):
    """Source and destination arenas of 2^32 + 4 MiB bytes, allocated and never filled: both clips lie above 2^32, the
    cursor just below it, so that the first piece lands below 2^32, the second across it and the others above.  Only the
    two windows are written and compared (the model runs on them, its offsets shifted); the first MiB of either arena,
    where an offset cut to 32 bits would land, keeps its pattern."""
    g = glc_amd
    case = next(c for c in CASES if c["name"] == "runs_longer_than_a_tile")
    ch, cuts = case["ch"], [(0, 1, 8), (1, 1, 8), (0, 0, 10), (1, 0, 10), (0, 3, 5), (1, 9, 1)]
    arena_h, entries = K.store_of(case, np.random.default_rng(31))
    sizes = [len(K.cut(case["clips"][c], ch, f0, nf)[1]) for c, f0, nf in cuts]
    size, base, win = FAR + 4 * MIB, FAR + MIB, FAR - MIB
    cursor = FAR - sizes[0] - 100
    dst_h = np.full(2 * MIB, K.PATTERN, np.uint8)
    lengths = [HOP * nf - 1 for _, _, nf in cuts]
    want = K.cut_store(arena_h, arena_h.size, entries, cuts, lengths, ch, dst_h, size - win, cursor - win)
    assert want["entries"][1][0] + win < FAR < want["entries"][1][0] + win + sizes[1] and want["cursor"] < 2 * MIB
    arena = torch.empty(size, dtype=torch.uint8, device="cuda")
    dst = torch.empty(size, dtype=torch.uint8, device="cuda")
    arena[:3 * MIB] = K.PATTERN
    arena[base:base + arena_h.size] = dev(torch, arena_h)
    dst[:MIB] = K.PATTERN
    dst[win:win + 2 * MIB] = K.PATTERN
    n = len(cuts)
    ent_in = dev(torch, J.entry_words([[e[0] + base] + e[1:] for e in entries]))
    ent_out = dev(torch, np.full(32 * n + MARGIN, K.PATTERN, np.uint8))
    len_out = dev(torch, np.full(8 * n + MARGIN, K.PATTERN, np.uint8))
    status = dev(torch, np.full(4 * n + MARGIN, K.PATTERN, np.uint8))
    cur = dev(torch, np.array([cursor], np.uint64))
    torch.cuda.synchronize()
    mover = ctx(g, "mover")
    rc = g.lib.glc_store_cut_device(mover._h, arena.data_ptr(), size, ent_in.data_ptr(), len(entries), cut_array(g, cuts), n,
                                    (C.c_uint64 * n)(*lengths), ch, dst.data_ptr(), size, cur.data_ptr(), ent_out.data_ptr(),
                                    len_out.data_ptr(), status.data_ptr())
    assert rc == 0, g.lib.glc_last_error(mover._h)
    mover.synchronize()
    got = status.cpu().numpy()
    assert got[:4 * n].view(np.uint32).tolist() == want["status"] == [0] * n and np.all(got[4 * n:] == K.PATTERN)
    assert int(cur.cpu()[0]) == want["cursor"] + win
    got = ent_out.cpu().numpy()
    assert np.array_equal(got[:32 * n].view(np.int64).reshape(n, 4), J.entry_words([[e[0] + win] + e[1:] for e in want["entries"]]))
    assert np.all(got[32 * n:] == K.PATTERN)
    got = len_out.cpu().numpy()
    assert got[:8 * n].view(np.int64).tolist() == want["lengths"] == lengths and np.all(got[8 * n:] == K.PATTERN)
    got = dst[win:win + 2 * MIB].cpu().numpy()
    diff = np.nonzero(got != want["dst"])[0]
    assert diff.size == 0, ("first differing byte", int(diff[0]), "entries", want["entries"])
    assert bool((dst[:MIB] == K.PATTERN).all()) and bool((arena[:3 * MIB] == K.PATTERN).all())
    assert np.array_equal(arena[base:base + arena_h.size].cpu().numpy(), arena_h)
    del arena, dst
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ 2: real blobs

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
def test_pieces_of_real_blobs_are_the_stream_encoders_segments(glc_amd, torch, ch, integer):
    g = glc_amd
    rng = np.random.default_rng(91 + ch)
    lens = [9000, 14000]
    clips = [tone(ch, lens[0], 1), (rng.standard_normal((lens[1], ch)) * 0.3).astype(np.float32)]
    dtype = np.int16 if integer else np.float32
    if integer:
        clips = [np.clip(np.round(c * 32767.0), -32768, 32767).astype(np.int16) for c in clips]
    bits = 16 if integer else None
    b_arena, b_cursor, b_entries = ctx(g, "enc").encode_compact_batch_tensor(batch_tensor(torch, clips, ch, dtype), lengths=lens, bits=bits)
    # the same clips through the streaming encoder, every lane in its own chunking: its segments are the seams
    se = g.StreamEncoder(SR, ch, n_streams=2)
    arena = torch.zeros(1 << 21, dtype=torch.uint8, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    sent, seg_list, ent_list = [0, 0], [], []
    while any(s < n for s, n in zip(sent, lens)):
        take = [min(n - s, int(rng.integers(0, 5000))) for s, n in zip(sent, lens)]
        chunk = [c[s:s + k] for c, s, k in zip(clips, sent, take)]
        sent = [s + k for s, k in zip(sent, take)]
        x = batch_tensor(torch, [c if c.shape[0] else np.zeros((1, ch), dtype) for c in chunk], ch, dtype)
        fin = [k > 0 and s == n for k, s, n in zip(take, sent, lens)]
        entries, segs = se.push_tensor(x, take, fin, arena, cursor, bits=bits)
        seg_list += segs
        ent_list.append(entries)
    order = sorted(range(len(seg_list)), key=lambda j: seg_list[j][:2])
    segs = [seg_list[j] for j in order]
    s_entries = torch.cat(ent_list)[torch.tensor(order, device="cuda")].contiguous()
    assert min(sum(1 for s in segs if s[0] == lane) for lane in range(2)) >= 2
    # the cut of the batch encode's blobs at those seams
    out_arena = torch.full((2 * b_arena.numel() + 4096,), K.PATTERN, dtype=torch.uint8, device="cuda")
    out_cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    c_entries, c_lens, status = se.cut_clips_tensor(b_arena, b_entries, segs, out_arena, out_cursor)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(segs) and c_lens.cpu().tolist() == [HOP * s[2] for s in segs]
    assert (b_entries.cpu().numpy()[1, 3] & 0xFFFFFFFF) > 0                                  # the noise clip has raw frames
    pieces, segments = ([b.cpu().numpy().tobytes() for b in g.store_blobs(a, e)] for a, e in ((out_arena, c_entries), (arena, s_entries)))
    assert pieces == segments
    assert np.all(out_arena.cpu().numpy()[int(out_cursor.cpu()[0]):] == K.PATTERN)
    # the join of the pieces is the original
    j_arena = torch.full((b_arena.numel() + 4096,), K.PATTERN, dtype=torch.uint8, device="cuda")
    j_cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    j_entries, j_lens, j_status = se.join_segments_tensor(out_arena, c_entries, segs, j_arena, j_cursor, lengths=lens)
    torch.cuda.synchronize()
    assert j_status.cpu().tolist() == [0] * len(segs)
    joined, whole = ([b.cpu().numpy().tobytes() for b in g.store_blobs(a, e)] for a, e in ((j_arena, j_entries), (b_arena, b_entries)))
    assert joined == whole and int(j_cursor.cpu()[0]) == int(b_cursor.cpu()[0])
    # a receiver fed the pieces hears the whole clips
    sd = g.StreamDecoder(SR, ch, n_streams=2)
    out, emitted = sd.push_tensor(out_arena, c_entries, segs, finish=[True, True], total_len=lens)
    dec = ctx(g, "dec", ch)
    want = [dec.decode_compact_tensor(b, n * ch).clone() for b, n in zip(g.store_blobs(b_arena, b_entries), lens)]
    torch.cuda.synchronize()
    assert emitted == lens and all(s.flags == 0 for s in sd.last_compact_status())
    o = out.cpu().numpy()
    for i, n in enumerate(lens):
        assert np.array_equal(o[i, :, :n].T.reshape(-1).view(np.uint32), want[i].cpu().numpy().view(np.uint32)), i


@pytest.mark.parametrize("ch", (1, 2, 3))
def test_a_piece_is_a_clip_to_the_crop_decode(glc_amd, torch, ch):
    """A crop of a piece that stays a frame away from both of the piece's ends decodes from frames inside the piece, and
    the interleaved delay shifts both sides alike: bit for bit the whole clip's crop at 1024 f0 + start."""
    g = glc_amd
    rng = np.random.default_rng(40 + ch)
    L = 12 * HOP + 300
    nfw = g.plan_encode(L * ch, ch).n_frames
    clip = tone(ch, L, 3) + (rng.standard_normal((L, ch)) * 0.01).astype(np.float32)
    b_arena, _, b_entries = ctx(g, "enc").encode_compact_batch_tensor(batch_tensor(torch, [clip], ch, np.float32), lengths=[L])
    cuts = [(0, 4, 5), (0, 0, 4), (0, nfw - 3, 3), (0, 1, nfw - 1)]
    out_arena = torch.full((4 * b_arena.numel() + 4096,), K.PATTERN, dtype=torch.uint8, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    dec = ctx(g, "dec", ch)
    c_entries, c_lens, status = dec.cut_clips_tensor(b_arena, b_entries, cuts, out_arena, cursor)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(cuts)
    pieces = g.store_blobs(out_arena, c_entries)
    whole = g.store_blobs(b_arena, b_entries)[0]
    picks = []                                                          # (piece, start in the piece, length)
    for k, (_, f0, nf) in enumerate(cuts):
        lo, hi = HOP, HOP * (nf - 1)
        for start, length in ((lo, hi - lo), (lo, 1), (hi - 1, 1), (lo + 1, hi - lo - 1), (lo + 477, min(1000, hi - lo - 477)), ((lo + hi) // 2, 2)):
            if length >= 1 and start + length <= hi:
                picks.append((k, start, length))
    assert len(picks) >= 20
    a = dec.decode_compact_crops_tensor([pieces[k] for k, _, _ in picks], [HOP * cuts[k][2] * ch for k, _, _ in picks],
                                        [s for _, s, _ in picks], [n for _, _, n in picks])
    assert all(s.flags == 0 for s in dec.last_compact_status())
    b = dec.decode_compact_crops_tensor([whole] * len(picks), [L * ch] * len(picks), [HOP * cuts[k][1] + s for k, s, _ in picks],
                                        [n for _, _, n in picks])
    assert all(s.flags == 0 for s in dec.last_compact_status())
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    assert a.cpu().numpy().any()


# ------------------------------------------------------------------------------------------ 3: damage and placement

def three_clips(rng, ch=2):
    """The damage clip between two others, and one cut of each: the middle cut is the window the damage is judged on."""
    blob, f0, nf = K.damage_clip(rng, ch)
    return K.case("three", ch, [J.make_blob(rng, ch, 5, raw=(1,)), blob, J.make_blob(rng, ch, 6)], [(0, 1, 3), (1, f0, nf), (2, 0, 6)])


@pytest.mark.parametrize("kind", K.HEADER_DAMAGE + K.WINDOW_DAMAGE + ("not_stored", "offset_odd", "outside", "window_beyond", "no_such_clip"))
def test_a_damaged_source_refuses_its_cut_alone(glc_amd, torch, kind):
    g = glc_amd
    rng = np.random.default_rng(21)
    case = three_clips(rng)
    _, f0, nf = case["cuts"][1]
    bits = K.NO_BLOB | K.BAD_HEADER
    if kind in K.HEADER_DAMAGE + K.WINDOW_DAMAGE:
        case["clips"][1], bits, _ = K.damaged(case["clips"][1], kind, 2, f0, nf)
    arena_h, entries = K.store_of(case, rng)
    arena_bytes, n_entries = arena_h.size, 3
    if kind == "not_stored":
        entries[1][4] = 0
    elif kind == "offset_odd":
        entries[1][0] += 32
    elif kind == "outside":
        # the entry points behind arena_bytes, into a guard of NaN bits that belongs to the tensor but not to the arena
        arena_h = np.concatenate([arena_h, np.full(8192, 0xFF, np.uint8)])
        entries[1][0] = arena_bytes + 64
    elif kind == "window_beyond":
        case["cuts"][1], bits = (1, 6, 4), K.BAD_CROP
    elif kind == "no_such_clip":
        # clip == n_entries: a fourth entry lies behind the index and is not read
        entries.append(list(entries[1]))
        case["cuts"][1], bits = (3, f0, nf), K.BAD_CROP
    dst_h = np.full(1 << 16, K.PATTERN, np.uint8)
    want = run_cut(g, torch, arena_h, arena_bytes, entries, case["cuts"], None, 2, dst_h, dst_h.size, 0, kind, n_entries=n_entries)
    assert want["status"] == [0, bits, 0]
    assert want["entries"][1] == [0, 0, 0, 0, 0] and want["lengths"][1] == 0
    assert want["entries"][2][0] == want["entries"][0][0] + want["entries"][0][1]        # as if the refused cut had size 0


@pytest.mark.parametrize("kind", K.BEHIND)
def test_damage_behind_the_window_does_not_refuse(glc_amd, torch, kind):
    rng = np.random.default_rng(24)
    case = three_clips(rng)
    _, f0, nf = case["cuts"][1]
    case["clips"][1], bits, _ = K.damaged(case["clips"][1], kind, 2, f0, nf)
    arena_h, entries = K.store_of(case, rng)
    dst_h = np.full(1 << 16, K.PATTERN, np.uint8)
    want = run_cut(glc_amd, torch, arena_h, arena_h.size, entries, case["cuts"], None, 2, dst_h, dst_h.size, 0, kind)
    assert bits == 0 and want["status"] == [0, 0, 0] and all(e[4] == 1 for e in want["entries"])


def test_placement_a_piece_that_does_not_fit_and_an_append(glc_amd, torch):
    g = glc_amd
    rng = np.random.default_rng(22)
    case = three_clips(rng, 3)
    arena_h, entries = K.store_of(case, rng)
    cuts = case["cuts"]
    sizes = [len(K.cut(case["clips"][c], 3, f0, nf)[1]) for c, f0, nf in cuts]
    # too small for the last piece by one byte: not stored, nothing written, the cursor at the size that would have sufficed
    dst_bytes = 64 + sum(sizes) - 1
    dst_h = np.full(dst_bytes, K.PATTERN, np.uint8)
    want = run_cut(g, torch, arena_h, arena_h.size, entries, cuts, None, 3, dst_h, dst_bytes, 1, "does not fit")
    assert [e[4] for e in want["entries"]] == [1, 1, 0] and want["cursor"] == 64 + sum(sizes)
    assert np.all(want["dst"][64 + sizes[0] + sizes[1]:] == K.PATTERN)
    # a second call appends from the first one's cursor, which the caller moved off the 64-byte grid
    dst_h = np.full(3 * sum(sizes), K.PATTERN, np.uint8)
    first = run_cut(g, torch, arena_h, arena_h.size, entries, cuts, None, 3, dst_h, dst_h.size, 0, "first")
    assert first["cursor"] == sum(sizes)
    second = run_cut(g, torch, arena_h, arena_h.size, entries, cuts, None, 3, first["dst"], dst_h.size, first["cursor"] + 5, "append")
    assert second["entries"][0][0] == sum(sizes) + 64 and second["cursor"] == 2 * sum(sizes) + 64
    assert np.array_equal(second["dst"][:sum(sizes)], second["dst"][sum(sizes) + 64:2 * sum(sizes) + 64])


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
    arena_h, entries = K.store_of(case, rng)
    cuts = case["cuts"]
    lengths = [HOP * nf for _, _, nf in cuts]
    dec = g.Decoder(ch, SR)
    # a completed compact decode, then a resident stream on the context
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")
    good = K.cut_store(arena_h, arena_h.size, entries, cuts, lengths, ch, np.zeros(1 << 16, np.uint8), 1 << 16, 0)
    dec.decode_store_crops_tensor(dev(torch, good["dst"]), dev(torch, J.entry_words(good["entries"])), i64(lengths), i64([0, 2]),
                                  i64([5, 0]), 200, max(lengths))
    status = [(s.flags, s.n_bad_rows, s.first_bad_row) for s in dec.last_compact_status()]
    dec.decode(stream)                                               # behind the draw, which is a decode and forgets the stream
    resident = dec.resident_stream()
    assert resident != 0
    dst_h = np.full(1 << 16, K.PATTERN, np.uint8)
    run_cut(g, torch, arena_h, arena_h.size, entries, cuts, lengths, ch, dst_h, dst_h.size, 0, "family", mover=dec)
    assert dec.resident_stream() == resident
    assert [(s.flags, s.n_bad_rows, s.first_bad_row) for s in dec.last_compact_status()] == status
    # an open decode session stays open and goes on where it was
    sd = g.StreamDecoder(SR, ch)
    pieces_h = K.cut_store(arena_h, arena_h.size, entries, [(1, 0, 4), (1, 4, 5)], None, ch, np.zeros(1 << 16, np.uint8), 1 << 16, 0)
    p_arena, p_entries = dev(torch, pieces_h["dst"]), dev(torch, J.entry_words(pieces_h["entries"]))
    sd.push_tensor(p_arena, p_entries[0:1], [(0, 0, 4)])
    assert sd.frames_done(0) == 4
    run_cut(g, torch, arena_h, arena_h.size, entries, cuts, lengths, ch, dst_h, dst_h.size, 0, "session", mover=sd)
    assert sd.frames_done(0) == 4
    sd.push_tensor(p_arena, p_entries[1:2], [(0, 4, 5)], finish=True, total_len=9 * HOP)
    assert sd.frames_done(0) == 0 and all(s.flags == 0 for s in sd.last_compact_status())
    sd.close()

    # ---- the host rules: GLC_EINVAL before anything is queued, nothing changed
    n = len(cuts)
    arena, dst = dev(torch, padded(arena_h)), dev(torch, padded(dst_h))
    ent_in = dev(torch, J.entry_words(entries))
    ent_out = dev(torch, np.full(32 * n + 64, K.PATTERN, np.uint8))
    len_out = dev(torch, np.full(8 * n + 64, K.PATTERN, np.uint8))
    stat = dev(torch, np.full(4 * n + 64, K.PATTERN, np.uint8))
    cur = dev(torch, np.array([192, 0], np.uint64))
    A, D, EI, EO, LO, ST, CU = (t.data_ptr() for t in (arena, dst, ent_in, ent_out, len_out, stat, cur))

    def call(a=A, ab=arena_h.size, ei=EI, ne=3, cu_=cuts, nc=None, ln=lengths, c=ch, d=D, db=dst_h.size, cu=CU, eo=EO, lo=LO, st=ST):
        nc = len(cu_) if nc is None and cu_ is not None else nc
        lens = (C.c_uint64 * max(len(ln), 1))(*ln) if ln is not None else None
        return g.lib.glc_store_cut_device(dec._h, a, ab, ei, ne, cut_array(g, cu_) if cu_ is not None else None, nc, lens, c, d, db, cu, eo, lo, st)

    def with_cut(i, **kw):
        out = list(cuts)
        f = dict(zip(("clip", "first_frame", "n_frames"), out[i]))
        f.update(kw)
        out[i] = (f["clip"], f["first_frame"], f["n_frames"])
        return out

    assert call(nc=0) == 0                                                     # n_cuts == 0: GLC_OK, the cursor stays
    refused = [
        call(a=None), call(ei=None), call(cu_=None, nc=3), call(d=None), call(cu=None), call(eo=None), call(lo=None), call(st=None),
        call(c=0),
        call(a=A + 32), call(d=D + 16), call(ei=EI + 4), call(cu=CU + 4), call(eo=EO + 4), call(lo=LO + 4), call(st=ST + 2),
        call(cu_=with_cut(1, n_frames=0)),
        call(cu_=with_cut(2, n_frames=1 << 31), ln=None),                      # rows past 32 bits
        call(ln=[lengths[0], lengths[1] + HOP, lengths[2]]),                   # frames that are not the length's
        call(ln=[lengths[0], lengths[1], 0]),
        call(d=A + 64, db=64), call(eo=A + 128), call(lo=D + 8), call(st=D + 64), call(cu=A + 8), call(eo=EI), call(st=EO),
        call(lo=EO + 8), call(cu=ST),
    ]
    assert refused == [EINVAL] * len(refused), refused
    dec.synchronize()
    torch.cuda.synchronize()
    assert cur.cpu().tolist() == [192, 0] and np.array_equal(dst.cpu().numpy(), padded(dst_h))
    for t in (ent_out, len_out, stat):
        assert np.all(t.cpu().numpy() == K.PATTERN)
    del arena, dst
    dec.close()
    assert live(g) == before
