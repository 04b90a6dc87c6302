"""Eviction from the compact store: glc_store_compact_device and _Ctx.compact_store_tensor (include/glc.h "evicting clips
from the store").

Every comparison is exact - bytes and integers.  The byte movers run on arenas of seeded random bytes with entries the
host makes: the whole destination arena, both output arrays, new_index, n_out and the cursor are held to the numpy model
of tests/store_compact_cases.py (itself held to the header's invariants by tests/test_store_compact_model.py), and every
byte that must stay untouched - behind the cursor, a margin behind every buffer, the source of an out-of-place call -
to the 0xA5 pattern or to what it held.  The codec tests draw crops before and after an eviction and demand equal bits.
Damaged entries are those of the case lists (every count inside its buffer): the tests pin the defined result, they
provoke nothing."""
import numpy as np
import pytest

import compact_decode_cases as K
import crop_cases as CC
import roundtrip_cases as RC
import store_compact_cases as M
from crop_cases import NAN_BITS

pytestmark = pytest.mark.gpu

F32 = np.float32
EINVAL = -1
SR = 44100
MARGIN = 256                       # pattern bytes behind every arena
NO_BLOB, BAD_CROP, BAD_HEADER = 64, 128, 1


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    assert hasattr(g.lib, "glc_store_compact_device") and hasattr(g.lib, "glc_debug_set_store_compact_round")
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


def entries_np(entries):
    return np.array(entries, dtype=np.uint64).reshape(-1, 4).view(np.int64)


def padded(data, margin=MARGIN):
    """`data` with a margin of pattern bytes behind it."""
    return np.concatenate([np.ascontiguousarray(data).view(np.uint8).reshape(-1), np.full(margin, M.PATTERN, np.uint8)])


def run_case(g, torch, case, alias=False, with_lengths=True, rnd=None, mover=None):
    """One call on buffers with pattern margins, then everything the call may have touched against the model."""
    mover = mover or ctx(g, "mover")
    n, ab = len(case["entries"]), case["arena_bytes"]
    in_place = case["dst_bytes"] is None
    arena_h = M.arena_of(case)
    lengths = case["lengths"] if with_lengths else None
    dst_h = None if in_place else np.full(case["dst_bytes"], M.PATTERN, np.uint8)
    want = M.compact(arena_h, ab, case["entries"], lengths, case["keep"], dst_h, case["dst_bytes"])

    arena = dev(torch, padded(arena_h))
    dst = arena if in_place else dev(torch, padded(dst_h))
    assert arena.data_ptr() % 64 == 0 and dst.data_ptr() % 64 == 0
    ent_in = dev(torch, padded(entries_np(case["entries"])))
    len_in = dev(torch, padded(np.array(lengths, np.int64))) if with_lengths else None
    keep = dev(torch, padded(np.array(case["keep"], np.uint8)))
    ent_out = ent_in if alias else dev(torch, np.full(32 * n + MARGIN, M.PATTERN, np.uint8))
    len_out = None if not with_lengths else len_in if alias else dev(torch, np.full(8 * n + MARGIN, M.PATTERN, np.uint8))
    new_index = dev(torch, np.full(8 * n + MARGIN, M.PATTERN, np.uint8))
    counts = dev(torch, np.full(16 + MARGIN, M.PATTERN, np.uint8))
    torch.cuda.synchronize()
    assert g.lib.glc_debug_set_store_compact_round(mover._h, rnd or 0) == 0
    rc = g.lib.glc_store_compact_device(
        mover._h, arena.data_ptr(), ab, ent_in.data_ptr(), len_in.data_ptr() if with_lengths else None, n, keep.data_ptr(),
        dst.data_ptr(), ab if in_place else case["dst_bytes"], ent_out.data_ptr(), len_out.data_ptr() if with_lengths else None,
        new_index.data_ptr(), counts.data_ptr(), counts.data_ptr() + 8)
    assert rc == 0, g.lib.glc_last_error(mover._h)
    mover.synchronize()
    assert g.lib.glc_debug_set_store_compact_round(mover._h, 0) == 0
    # ---- the host enters here
    name = case["name"]
    got_counts = counts.cpu().numpy()
    assert got_counts[:16].view(np.uint64).tolist() == [want["n_out"], want["cursor"]], name
    assert np.all(got_counts[16:] == M.PATTERN)
    got_index = new_index.cpu().numpy()
    assert got_index[:8 * n].view(np.int64).tolist() == want["new_index"], name
    assert np.all(got_index[8 * n:] == M.PATTERN)
    got_ent = ent_out.cpu().numpy()
    assert np.array_equal(got_ent[:32 * n].view(np.int64).reshape(n, 4), entries_np(want["entries"])), name
    assert np.all(got_ent[32 * n:] == M.PATTERN)
    if with_lengths:
        got_len = len_out.cpu().numpy()
        assert got_len[:8 * n].view(np.int64).tolist() == want["lengths"], name
        assert np.all(got_len[8 * n:] == M.PATTERN)
    if not alias:                                                       # the inputs are inputs
        assert np.array_equal(ent_in.cpu().numpy(), padded(entries_np(case["entries"])))
        if with_lengths:
            assert np.array_equal(len_in.cpu().numpy(), padded(np.array(lengths, np.int64)))
    assert np.array_equal(keep.cpu().numpy(), padded(np.array(case["keep"], np.uint8)))
    got_dst = dst.cpu().numpy()
    size = ab if in_place else case["dst_bytes"]
    diff = np.nonzero(got_dst[:size] != want["arena"][:size])[0]
    assert diff.size == 0, (name, "first differing byte", int(diff[0]), "of", size)
    assert np.all(got_dst[size:] == M.PATTERN), name
    if not in_place:
        assert np.array_equal(arena.cpu().numpy(), padded(arena_h)), name       # the source is not written at all
    return want


# ------------------------------------------------------------------------------------------ 1: the byte movers

@pytest.mark.parametrize("group", ("keep_patterns", "own_source_overlap", "unusable_entries", "out_of_order", "out_of_place"))
def test_byte_movers_against_the_model(glc_amd, torch, group):
    cases = getattr(M, group)()
    seen = set()
    for i, case in enumerate(cases):
        want = run_case(glc_amd, torch, case, alias=bool(i % 2))
        seen |= {v if v < 0 else 0 for v in want["new_index"]}
    assert 0 in seen or group == "unusable_entries"
    if group == "out_of_order":
        assert seen == {0, M.DROPPED, M.UNUSABLE, M.OUT_OF_ORDER}


@pytest.mark.parametrize("rnd", (1024, 4096, None), ids=("1KiB", "4KiB", "default"))
def test_round_edges_in_place(glc_amd, torch, rnd):
    """Blobs that end on, begin on and span round boundaries of the packed space; totals of whole rounds and 64 bytes
    more.  The cases laid out for 1 KiB and 4 KiB rounds also run at the default round, and the small cases at 1 KiB."""
    g = glc_amd
    cases = M.round_edges(rnd) if rnd else [c for r in M.ROUNDS for c in M.round_edges(r)]
    for i, case in enumerate(cases):
        want = run_case(g, torch, case, alias=bool(i % 2), rnd=rnd)
        assert want["n_out"] >= 2
    if rnd == 1024:
        for case in M.own_source_overlap() + M.keep_patterns():
            run_case(g, torch, case, rnd=rnd)
        for case in M.round_edges(4096):                          # ... and rounds that no boundary of the layout respects
            run_case(g, torch, case, rnd=1024 + 64)


@pytest.mark.parametrize("name", tuple(M.GRID_RUNS))
def test_grid_stride_edges(glc_amd, torch, name):
    """Arenas of tens of MiB (tests/store_compact_cases.py "grid-stride edges"): more tiles than the movers' grid, out of
    place and in place; in place with a round whose 2 * tiles jobs exceed the grid and which is no multiple of the tile,
    with a round of three tiles and 64 bytes, and as one round; and a tail of the output arrays longer than one pass."""
    make, rnd = M.GRID_RUNS[name]
    want = run_case(glc_amd, torch, make(), alias=name.endswith("64"), rnd=rnd)
    assert want["n_out"] >= 7


MIB, FAR = 1 << 20, 1 << 32


def far_call(g, torch, mover, arena, ab, entries, lengths, keep, dst, dst_bytes):
    """glc_store_compact_device on arenas the caller holds: (entries_out, lengths_out, new_index, n_out, cursor), every
    array checked for its pattern margin."""
    n = len(entries)
    ent_in, len_in = dev(torch, entries_np(entries)), dev(torch, np.array(lengths, np.int64))
    keep_d = dev(torch, np.array(keep, np.uint8))
    outs = [dev(torch, np.full(k * n + MARGIN, M.PATTERN, np.uint8)) for k in (32, 8, 8)] + [dev(torch, np.full(16 + MARGIN, M.PATTERN, np.uint8))]
    torch.cuda.synchronize()
    assert g.lib.glc_debug_set_store_compact_round(mover._h, 0) == 0
    rc = g.lib.glc_store_compact_device(mover._h, arena.data_ptr(), ab, ent_in.data_ptr(), len_in.data_ptr(), n, keep_d.data_ptr(), dst.data_ptr(),
                                        dst_bytes, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                                        outs[3].data_ptr() + 8)
    assert rc == 0, g.lib.glc_last_error(mover._h)
    mover.synchronize()
    got = [o.cpu().numpy() for o in outs]
    for o, k in zip(got, (32 * n, 8 * n, 8 * n, 16)):
        assert np.all(o[k:] == M.PATTERN)
    counts = got[3][:16].view(np.uint64).tolist()
    return (got[0][:32 * n].view(np.uint64).reshape(n, 4).tolist(), got[1][:8 * n].view(np.int64).tolist(),
            got[2][:8 * n].view(np.int64).tolist(), counts[0], counts[1])


def far_case():
    ent, end = M.laid([64, 5 * M.TILE + 320, 64, 2 * M.TILE, 192, 64])
    return M.case("far", ent, [0, 1, 0, 1, 1, 0], end)


def test_in_place_beyond_4_gib(glc_amd, torch):
    """A kept first blob of exactly 4 GiB at offset 0, which does not move; 64 dropped bytes behind it; kept blobs behind
    those, whose new offsets lie above 2^32 and shift by 64.  Only the window behind 2^32 is written and compared (the
    model runs on that window, its offsets shifted); the arena's first MiB, where an offset cut to 32 bits would land,
    keeps its pattern."""
    g = glc_amd
    case = far_case()
    small_h = M.arena_of(case)
    want = M.compact(small_h, case["arena_bytes"], case["entries"], case["lengths"], case["keep"])
    arena = torch.empty(FAR + 4 * MIB, dtype=torch.uint8, device="cuda")
    arena[:MIB] = M.PATTERN
    arena[FAR:FAR + 2 * MIB] = M.PATTERN
    arena[FAR:FAR + small_h.size] = dev(torch, small_h)
    ab = FAR + case["arena_bytes"]
    entries = [M.entry(0, FAR, n_pairs=5)] + [M.entry(e[0] + FAR, e[1], e[2], e[3] & 0xFFFFFFFF) for e in case["entries"]]
    got = far_call(g, torch, ctx(g, "mover"), arena, ab, entries, [77] + case["lengths"], [1] + case["keep"], arena, ab)
    n_out = want["n_out"]
    shifted = [[e[0] + FAR] + e[1:] for e in want["entries"][:n_out]]
    assert got[0] == [M.entry(0, FAR, n_pairs=5)] + shifted + [[0] * 4] * (len(entries) - 1 - n_out)
    assert got[1] == [77] + want["lengths"]
    assert got[2] == [0] + [v + 1 if v >= 0 else v for v in want["new_index"]]
    assert got[3:] == (n_out + 1, want["cursor"] + FAR) and want["cursor"] + 64 < case["arena_bytes"]
    assert all(e[0] > FAR for e in shifted[1:]) and shifted[0][0] == FAR
    assert np.array_equal(arena[FAR:FAR + small_h.size].cpu().numpy(), want["arena"])
    assert bool((arena[FAR + small_h.size:FAR + 2 * MIB] == M.PATTERN).all()) and bool((arena[:MIB] == M.PATTERN).all())
    del arena
    torch.cuda.empty_cache()


def test_out_of_place_from_beyond_4_gib(glc_amd, torch):
    """The same store with every source above 2^32, gathered into a small destination: a source offset cut to 32 bits
    would read the pattern of the arena's first MiBs."""
    g = glc_amd
    case = far_case()
    small_h = M.arena_of(case)
    total = sum(e[1] for e, k in zip(case["entries"], case["keep"]) if k)
    dst_h = np.full(total + 64, M.PATTERN, np.uint8)
    want = M.compact(small_h, case["arena_bytes"], case["entries"], case["lengths"], case["keep"], dst_h, total)
    arena = torch.empty(FAR + 4 * MIB, dtype=torch.uint8, device="cuda")
    arena[:3 * MIB] = M.PATTERN
    base = FAR + MIB
    arena[base:base + small_h.size] = dev(torch, small_h)
    dst = dev(torch, padded(dst_h))
    entries = [M.entry(e[0] + base, e[1], e[2], e[3] & 0xFFFFFFFF) for e in case["entries"]]
    got = far_call(g, torch, ctx(g, "mover"), arena, FAR + 4 * MIB, entries, case["lengths"], case["keep"], dst, total)
    assert got == (want["entries"], want["lengths"], want["new_index"], want["n_out"], want["cursor"]) and want["cursor"] == total
    assert np.array_equal(dst.cpu().numpy(), padded(want["arena"]))
    assert np.array_equal(arena[base:base + small_h.size].cpu().numpy(), small_h) and bool((arena[:3 * MIB] == M.PATTERN).all())
    del arena
    torch.cuda.empty_cache()


def test_scan_edges(glc_amd, torch):
    for i, case in enumerate(M.scan_edges()):
        run_case(glc_amd, torch, case, alias=bool(i % 2), with_lengths=i % 3 != 2)


def test_aliased_and_separate_outputs_give_the_same_words(glc_amd, torch):
    """run_case holds both forms to the model; here side by side on one case with every verdict, with and without
    lengths."""
    g = glc_amd
    case = next(c for c in M.out_of_order() if c["name"] == "all_three_codes")
    for with_lengths in (True, False):
        a = run_case(g, torch, case, alias=True, with_lengths=with_lengths)
        b = run_case(g, torch, case, alias=False, with_lengths=with_lengths)
        assert a["entries"] == b["entries"] and a["lengths"] == b["lengths"] and (a["lengths"] is None) == (not with_lengths)
    big = next(c for c in M.scan_edges() if c["name"] == "scan_2050")
    run_case(g, torch, big, alias=True)
    run_case(g, torch, big, alias=False, with_lengths=False)


def test_arguments_refused_before_anything_is_queued(glc_amd, torch):
    g = glc_amd
    mover = g.Decoder(2, SR)
    case = M.keep_patterns()[4]
    n, ab = len(case["entries"]), case["arena_bytes"]
    arena_h = M.arena_of(case)
    arena, other = dev(torch, padded(arena_h)), dev(torch, np.full(2 * ab, M.PATTERN, np.uint8))
    room = dev(torch, np.full(4096, M.PATTERN, np.uint8))               # every small array lives here, 256 bytes apart
    ent = dev(torch, entries_np(case["entries"]))
    lens = dev(torch, np.array(case["lengths"], np.int64))
    keep = dev(torch, np.array(case["keep"], np.uint8))
    torch.cuda.synchronize()
    A, D, R, E, L, Kp = arena.data_ptr(), other.data_ptr(), room.data_ptr(), ent.data_ptr(), lens.data_ptr(), keep.data_ptr()
    EO, LO, NI, NO, CU = R, R + 512, R + 1024, R + 1536, R + 1600

    def call(arena=A, ab=ab, entries=E, lengths=L, n=n, keep=Kp, dst=None, dst_bytes=None, eo=EO, lo=LO, ni=NI, no=NO, cu=CU):
        dst = arena if dst is None else dst
        dst_bytes = ab if dst_bytes is None else dst_bytes
        return g.lib.glc_store_compact_device(mover._h, arena, ab, entries, lengths, n, keep, dst, dst_bytes, eo, lo, ni, no, cu)

    refused = [
        g.lib.glc_store_compact_device(None, A, ab, E, L, n, Kp, A, ab, EO, LO, NI, NO, CU),
        g.lib.glc_store_compact_device(mover._h, None, ab, E, L, n, Kp, A, ab, EO, LO, NI, NO, CU),
        g.lib.glc_store_compact_device(mover._h, A, ab, E, L, n, Kp, None, ab, EO, LO, NI, NO, CU),
        call(entries=None), call(keep=None), call(eo=None), call(ni=None), call(no=None), call(cu=None),
        call(lengths=None), call(lo=None),                                # the lengths pair: both or neither
        call(arena=A + 32, ab=ab - 64), call(dst=D + 32, dst_bytes=ab),   # an arena that is not 64-byte aligned
        call(entries=E + 4), call(lengths=L + 4), call(eo=EO + 4), call(lo=LO + 4), call(ni=NI + 4), call(no=NO + 4), call(cu=CU + 4),
        call(n=0),
        call(dst_bytes=ab - 64), call(dst_bytes=ab + 64),                 # in place with dst_bytes != arena_bytes
        call(dst=A + 64, dst_bytes=ab), call(dst=A + ab - 64, dst_bytes=64),      # a destination inside the source
        call(arena=D + 64, ab=ab, dst=D, dst_bytes=2 * ab),               # ... and around it
        call(eo=A), call(lo=A + 64), call(ni=A + 128), call(no=A + ab - 8), call(cu=A),       # an array inside the arena
        call(dst=D, dst_bytes=2 * ab, ni=D + ab), call(dst=D, dst_bytes=2 * ab, cu=D + 2 * ab - 8),   # ... inside the destination
        call(eo=E + 32), call(eo=E + 32 * (n - 1)),                       # a shifted alias of the entries
        call(lo=L + 8), call(ni=E), call(ni=L), call(eo=L), call(lo=E),
        call(ni=Kp - Kp % 8), call(eo=Kp - Kp % 8),                       # the keep bytes
        call(no=CU), call(no=NI), call(cu=NI + 8 * (n - 1)), call(cu=EO + 8), call(no=LO), call(lo=EO + 8), call(ni=EO + 32 * n - 8),
    ]
    assert refused == [EINVAL] * len(refused)
    assert g.lib.glc_debug_set_store_compact_round(mover._h, 1000) == EINVAL          # no multiple of 64
    mover.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(arena.cpu().numpy(), padded(arena_h))
    assert np.all(other.cpu().numpy() == M.PATTERN) and np.all(room.cpu().numpy() == M.PATTERN)
    assert np.array_equal(ent.cpu().numpy(), entries_np(case["entries"])) and lens.cpu().tolist() == case["lengths"]
    # ... and the same buffers accepted: in place, then out of place
    want = M.compact(arena_h, ab, case["entries"], case["lengths"], case["keep"])
    assert call() == 0
    mover.synchronize()
    got = room.cpu().numpy()
    assert [int(got[o:o + 8].view(np.uint64)[0]) for o in (1536, 1600)] == [want["n_out"], want["cursor"]]
    assert got[1024:1024 + 8 * n].view(np.int64).tolist() == want["new_index"]
    assert np.array_equal(arena.cpu().numpy()[:ab], want["arena"])
    mover.close()


# ------------------------------------------------------------------------------------------ 2: with the codec

def batch_of(torch, ch, clips):
    lens = [c.size // ch for c in clips]
    x = np.full((len(clips), ch, max(lens)), NAN_BITS, np.uint32).view(F32)
    for i, c in enumerate(clips):
        x[i, :, :lens[i]] = np.ascontiguousarray(c, F32).reshape(-1, ch).T
    return torch.from_numpy(x).cuda(), lens


def encode_store(g, torch, ch, clips, arena=None, cursor=None):
    x, lens = batch_of(torch, ch, clips)
    arena, cursor, entries = ctx(g, "enc").encode_compact_batch_tensor(x, lengths=lens, planar=True, arena=arena, cursor=cursor)
    return arena, cursor, entries, lens


def i64(torch, values):
    return torch.tensor(list(values), dtype=torch.int64).reshape(-1).cuda()


def draw(g, torch, ch, arena, entries, lengths_t, clips, starts, length, max_length):
    dec = ctx(g, "dec", ch)
    out = dec.decode_store_crops_tensor(arena, entries, lengths_t, i64(torch, clips), i64(torch, starts), length, max_length)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32), [(s.flags, s.n_bad_rows, s.first_bad_row) for s in dec.last_compact_status()]


def clips_of(ch, lens, seed=0):
    """Tones, silence and noise, 1 to 6 frames each."""
    kinds = (lambda n, s: RC.chord(SR, ch, n, seed=s), lambda n, s: RC.lcg_noise(n * ch, seed=s + 1), lambda n, s: np.zeros(n * ch, F32))
    return [np.ascontiguousarray(kinds[i % 3 if i % 5 else 0](n, seed + i), F32) for i, n in enumerate(lens)]


LENS8 = (600, 6000, 1025, 2049, 3100, 5000, 777, 4096)
KEEP8 = (0, 1, 1, 0, 1, 1, 0, 1)
LENGTH = 500


def crops_for(lens, idx):
    """Per clip of `idx` the first, the last and a middle window of LENGTH samples."""
    clips = [i for i in idx for _ in range(3)]
    starts = [s for i in idx for s in (0, lens[i] - LENGTH, (lens[i] - LENGTH) // 2)]
    return clips, starts


def test_draws_are_the_same_bits_through_new_index(glc_amd, torch):
    g = glc_amd
    ch = 2
    clips8 = clips_of(ch, LENS8)
    arena, cursor, entries, lens = encode_store(g, torch, ch, clips8)
    lengths_t = i64(torch, lens)
    every = list(range(8))
    sel, starts = crops_for(lens, every)
    before, st_before = draw(g, torch, ch, arena, entries, lengths_t, sel, starts, LENGTH, max(lens))
    assert all(w == (0, 0, 0) for w in st_before)
    old = arena.clone()
    keep = torch.tensor(KEEP8, dtype=torch.bool).cuda()
    ents, lens_out, new_index, n_out, cur = ctx(g, "dec", ch).compact_store_tensor(arena, entries, lengths_t, keep)
    torch.cuda.synchronize()
    idx = new_index.cpu().tolist()
    kept = [i for i in every if KEEP8[i]]
    assert [idx[i] for i in kept] == list(range(5)) and all(idx[i] == M.DROPPED for i in every if not KEEP8[i])
    assert int(n_out.item()) == 5 and lens_out.cpu().tolist() == [lens[i] for i in kept] + [0] * 3
    e_old, e_new = entries.cpu().tolist(), ents.cpu().tolist()
    assert int(cur.item()) == sum(e_old[i][1] for i in kept) == e_new[4][0] + e_new[4][1]
    assert e_new[5:] == [[0] * 4] * 3
    assert torch.equal(arena[int(cur.item()):], old[int(cur.item()):])           # nothing at or above the cursor is written
    # the same crops through new_index: every sample and every status word
    sel_k, starts_k = crops_for(lens, kept)
    rows = [3 * i + j for i in kept for j in range(3)]
    after, st_after = draw(g, torch, ch, arena, ents, lens_out, [idx[c] for c in sel_k], starts_k, LENGTH, max(lens))
    assert np.array_equal(after, before[rows]) and st_after == [st_before[r] for r in rows]
    # a stale index: the old number of a clip, now at or beyond n_out, or a dropped clip's -1
    stale, st = draw(g, torch, ch, arena, ents, lens_out, [5, 7, idx[0]], [0, 0, 0], LENGTH, max(lens))
    assert not stale.any()                                                      # +0.0
    assert all(w[0] & BAD_HEADER and w[0] & (NO_BLOB | BAD_CROP) and w[1:] == (0, 0) for w in st)
    # out of place from the original bytes gives the same store
    other = torch.full((int(cur.item()) + 128,), M.PATTERN, dtype=torch.uint8, device="cuda")
    ents2, lens2, idx2, n2, cur2 = ctx(g, "enc").compact_store_tensor(old, entries, lengths_t, keep.to(torch.uint8), out_arena=other)
    torch.cuda.synchronize()
    assert torch.equal(ents2, ents) and torch.equal(lens2, lens_out) and torch.equal(idx2, new_index) and torch.equal(cur2, cur)
    assert torch.equal(other[:int(cur.item())], arena[:int(cur.item())]) and bool((other[int(cur.item()):] == M.PATTERN).all())
    # a bound on the bytes in use: the same result from fewer rounds
    again = old.clone()
    ents3, _, idx3, _, cur3 = ctx(g, "dec", ch).compact_store_tensor(again, entries, None, keep, used_bytes=int(cursor.item()))
    torch.cuda.synchronize()
    assert torch.equal(ents3, ents) and torch.equal(idx3, new_index) and torch.equal(cur3, cur) and torch.equal(again, arena)


def test_a_damaged_blob_stays_exactly_as_damaged(glc_amd, torch):
    g = glc_amd
    base = CC.stereo_stream()
    good, _ = K.pack(2, base)
    bad_magic, _ = K.pack(2, base, magic=K.MAGIC ^ 0x100)
    bad_list, _ = K.pack(2, CC.with_bad_list(base, 7))
    blobs = [good, bad_magic, good, bad_list]
    parts, ent, off = [], [], 0
    for b in blobs:
        size = K.align64(b.size)
        parts.append(np.concatenate([b, np.zeros(size - b.size, np.uint8)]))
        ent.append(M.entry(off, size))
        off += size
    arena = dev(torch, np.concatenate(parts))
    entries, n = dev(torch, entries_np(ent)), len(base) * K.HOP
    lengths_t = i64(torch, [n] * 4)
    start, length = CC.first_sample_of_hop(3, 2), 2 * K.HOP
    before, st_before = draw(g, torch, 2, arena, entries, lengths_t, [1, 2, 3], [start] * 3, length, n)
    assert st_before[0][0] & BAD_HEADER and st_before[1] == (0, 0, 0) and st_before[2][0] == K.NOT_CANONICAL
    keep = torch.tensor([0, 1, 1, 1], dtype=torch.uint8).cuda()
    ents, lens_out, new_index, n_out, cur = ctx(g, "dec").compact_store_tensor(arena, entries, lengths_t, keep)
    assert new_index.cpu().tolist() == [M.DROPPED, 0, 1, 2]
    after, st_after = draw(g, torch, 2, arena, ents, lens_out, [0, 1, 2], [start] * 3, length, n)
    assert np.array_equal(after, before) and st_after == st_before


def test_append_after_compaction(glc_amd, torch):
    g = glc_amd
    ch = 2
    clips8, more = clips_of(ch, LENS8), clips_of(ch, (1500, 513, 3000), seed=40)
    bound = g.compact_store_bound(ch, [c.size // ch for c in clips8 + more])
    arena = torch.full((bound,), M.PATTERN, dtype=torch.uint8, device="cuda")
    arena, cursor, entries, lens = encode_store(g, torch, ch, clips8, arena=arena)
    keep = torch.tensor(KEEP8, dtype=torch.bool).cuda()
    ents, lens_out, new_index, n_out, cur = ctx(g, "enc").compact_store_tensor(arena, entries, i64(torch, lens), keep)
    at = int(cur.item())
    arena, cur, e2, l2 = encode_store(g, torch, ch, more, arena=arena, cursor=cur)
    ents[5:8] = e2                                                  # behind n_out
    lens_out[5:8] = i64(torch, l2)
    torch.cuda.synchronize()
    e2h = e2.cpu().tolist()
    assert e2h[0][0] == at and all(e[3] >> 32 == 1 for e in e2h)    # the new blobs start at the cursor, and are stored
    kept = [c for c, k in zip(clips8, KEEP8) if k]
    fresh, fcur, fent, flens = encode_store(g, torch, ch, kept + more, arena=torch.full((bound,), M.PATTERN, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    end = int(fcur.item())
    assert int(cur.item()) == end and torch.equal(ents, fent) and lens_out.cpu().tolist() == flens
    assert torch.equal(arena[:end], fresh[:end])                    # byte for byte the store that got the 5 + 3 clips in one go
    sel, starts = crops_for(flens, range(8))
    a, st_a = draw(g, torch, ch, arena, ents, lens_out, sel, starts, LENGTH, max(flens))
    b, st_b = draw(g, torch, ch, fresh, fent, i64(torch, flens), sel, starts, LENGTH, max(flens))
    assert np.array_equal(a, b) and st_a == st_b and all(w == (0, 0, 0) for w in st_a)


def test_overflow_and_recover(glc_amd, torch):
    g = glc_amd
    ch = 2
    clips = [RC.chord(SR, ch, n, seed=3) for n in (5000, 3000, 2500, 2000)]
    _, _, full, lens = encode_store(g, torch, ch, clips)
    sizes = [e[1] for e in full.cpu().tolist()]
    assert sizes[2] <= sizes[0] + 64                                # clip 2 fits once clip 0 has gone
    small = torch.full((sizes[0] + sizes[1] + 64,), M.PATTERN, dtype=torch.uint8, device="cuda")
    arena, cursor, entries, lens = encode_store(g, torch, ch, clips, arena=small)
    torch.cuda.synchronize()
    assert int(cursor.item()) == sum(sizes) > small.numel() and [e[3] >> 32 for e in entries.cpu().tolist()] == [1, 1, 0, 0]
    keep = torch.tensor([0, 1, 1, 1], dtype=torch.bool).cuda()
    ents, lens_out, new_index, n_out, cur = ctx(g, "enc").compact_store_tensor(arena, entries, i64(torch, lens), keep)
    torch.cuda.synchronize()
    assert new_index.cpu().tolist() == [M.DROPPED, 0, M.UNUSABLE, M.UNUSABLE]
    assert int(n_out.item()) == 1 and int(cur.item()) == sizes[1]
    arena, cur, e2, l2 = encode_store(g, torch, ch, clips[2:3], arena=arena, cursor=cur)
    ents[1:2] = e2
    lens_out[1:2] = i64(torch, l2)
    torch.cuda.synchronize()
    assert e2.cpu().tolist()[0][0] == sizes[1] and e2.cpu().tolist()[0][3] >> 32 == 1      # an append that fits is stored
    sel, starts = [0, 1, 0, 1], [0, 0, lens[1] - LENGTH, lens[2] - LENGTH]
    a, st = draw(g, torch, ch, arena, ents, lens_out, sel, starts, LENGTH, max(lens))
    ref_arena, _, ref_ent, ref_lens = encode_store(g, torch, ch, clips[1:3])
    b, st_b = draw(g, torch, ch, ref_arena, ref_ent, i64(torch, ref_lens), sel, starts, LENGTH, max(lens))
    assert np.array_equal(a, b) and st == st_b == [(0, 0, 0)] * 4


def test_context_state_is_left_alone(glc_amd, torch):
    g = glc_amd
    ch = 2
    case = M.keep_patterns()[4]
    arena_h = M.arena_of(case)

    def compact_on(c):
        arena = dev(torch, arena_h)
        out = c.compact_store_tensor(arena, dev(torch, entries_np(case["entries"])), i64(torch, case["lengths"]),
                                     dev(torch, np.array(case["keep"], np.uint8)))
        torch.cuda.synchronize()
        want = M.compact(arena_h, case["arena_bytes"], case["entries"], case["lengths"], case["keep"])
        assert out[2].cpu().tolist() == want["new_index"] and np.array_equal(arena.cpu().numpy(), want["arena"])

    # a Decoder with a resident stream, an open streaming session and a status record
    dec = g.Decoder(ch, SR)
    x = RC.chord(SR, ch, 600 * K.HOP + 100)                          # two chunks of the streaming decode
    stream = ctx(g, "enc").encode(x, ch)
    whole = np.concatenate([np.asarray(c.samples, F32) for c in ctx(g, "dec", ch).decode_streaming(stream)])     # an undisturbed session
    dec.decode(stream)
    clips8 = clips_of(ch, LENS8[:3])
    s_arena, _, s_ent, s_lens = encode_store(g, torch, ch, clips8)
    dec.decode_store_crops_tensor(s_arena, s_ent, i64(torch, s_lens), i64(torch, [0, 1]), i64(torch, [0, 5]), LENGTH, max(s_lens))
    status = dec.last_compact_status()
    dec.decode(stream)
    resident = dec.resident_stream()
    assert resident != 0
    chunks = dec.decode_streaming(stream)
    first = next(chunks)
    compact_on(dec)
    assert dec.resident_stream() == resident
    rest = list(chunks)                                              # the next chunk of the session, and its last
    assert len(rest) >= 1
    got = np.concatenate([np.asarray(c.samples, F32) for c in [first] + rest])
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))
    again = dec.last_compact_status()
    assert [(s.flags, s.n_bad_rows, s.first_bad_row) for s in again] == [(s.flags, s.n_bad_rows, s.first_bad_row) for s in status]
    dec.close()
    # a round-trip context after a batch round trip
    rt = g.RoundTrip(SR)
    xb, lens = batch_of(torch, ch, clips8)
    rt.apply_batch_tensor(xb, lengths=lens)
    info = rt.last_batch_info()
    compact_on(rt)
    assert rt.last_batch_info() == info and rt.resident_stream() == 0
    rt.close()


@pytest.mark.parametrize("ch,keep", ((1, (0, 1, 1)), (6, (1, 0, 1))), ids=("mono", "6ch"))
def test_mono_and_six_channel_stores(glc_amd, torch, ch, keep):
    g = glc_amd
    clips = clips_of(ch, (2049, 600, 3100), seed=ch)
    arena, _, entries, lens = encode_store(g, torch, ch, clips)
    lengths_t = i64(torch, lens)
    sel, starts = crops_for(lens, range(3))
    before, st_before = draw(g, torch, ch, arena, entries, lengths_t, sel, starts, LENGTH, max(lens))
    ents, lens_out, new_index, n_out, cur = ctx(g, "dec", ch).compact_store_tensor(arena, entries, lengths_t,
                                                                                  torch.tensor(keep, dtype=torch.bool).cuda())
    idx = new_index.cpu().tolist()
    kept = [i for i in range(3) if keep[i]]
    assert [idx[i] for i in kept] == [0, 1] and int(n_out.item()) == 2
    sel_k, starts_k = crops_for(lens, kept)
    rows = [3 * i + j for i in kept for j in range(3)]
    after, st_after = draw(g, torch, ch, arena, ents, lens_out, [idx[c] for c in sel_k], starts_k, LENGTH, max(lens))
    assert np.array_equal(after, before[rows]) and st_after == [st_before[r] for r in rows]
