"""The batch drivers, the device round trip, the compressed clip store, crops and draws across the channel axis: 4, 5, 7,
9, 16, 17, 257 and 513 channels (tests/channel_axis_cases.py says what each is there for), where every suite of these
paths stopped at eight.

Every comparison is bit for bit - encoded bytes, blob bytes, decoded float32 viewed as uint32, int16 against the
restated narrowing of test_int_pcm - and the reference is the CPU oracle, per clip, computed once.  Every output buffer is
pre-filled with and surrounded by a pattern nothing computes, and everything outside the clips' samples must still hold
it afterwards.  A selection that cannot be served (an entry that holds no blob, a clip index outside the store) and a
blob whose header is damaged are part of every store read: +0.0 and the status bit.  The pointer calls
(glc_decode_batch_device_compact, glc_decode_crops_device_compact) refuse a bad selection on the host before anything
is queued, so there the unusable blob stands alone.

The CPU part holds the cases to their edges and shows that the model of "what a batch call writes where" notices ten
single edits, five of them at the new channel counts only."""
import ctypes as C

import numpy as np
import pytest

import channel_axis_cases as Q
import compact_decode_cases as K
import compact_edges as E
import compact_store_cases as CS
import crop_cases as CC
import store_draw_cases as S
from channel_axis_cases import CHANNELS, OLD

HOP = Q.HOP
F32 = np.float32
EINVAL = -1
NAN_BITS, I16_PATTERN = Q.NAN_BITS, Q.I16_PATTERN
GUARD = 8                    # pattern elements in front of and behind a flat output
TAIL = 4096                  # pattern bytes behind what an arena needs
FAKE_ARENA, FAKE_OUT = 1 << 44, 1 << 52      # numbers the planner hook never dereferences


# ----------------------------------------------------------------------------------------------------
# CPU: the cases reach their edges, the model is the definition, and every slip shows
# ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    import glc_amd as g
    return g


def test_the_channel_counts_take_the_paths_they_are_there_for():
    assert CHANNELS == (4, 5, 7, 9, 16, 17, 257, 513) and not set(CHANNELS) & set(OLD)
    assert [512 % ch for ch in CHANNELS] == [0, 2, 1, 8, 0, 2, 255, 512]
    assert [ch for ch in CHANNELS if ch & (ch - 1) == 0] == [4, 16]
    assert sum(ch > 256 for ch in CHANNELS) == 2 and min(ch for ch in CHANNELS if ch > 256) == 257
    assert 512 < 513                                   # the whole delay lies inside sample frame 0


@pytest.mark.parametrize("ch", [c for c in CHANNELS if not Q.is_wide(c)])
def test_the_pool_shows_both_frame_kinds_on_the_oracle(ch):
    raw = Q.item(ch, "mixed").raw
    assert any(raw) and not all(raw) and any(raw[i] != raw[i + 1] for i in range(len(raw) - 1))
    assert not any(Q.item(ch, "chord1537").raw)
    assert sorted({it.nf for it in Q.pool(ch)}) == [1, 2, 17]


@pytest.mark.parametrize("ch", CHANNELS)
def test_the_crops_hold_the_edges(host, ch):
    g = host
    lens = dict(zip(Q.batch_names(ch), Q.pool_lengths(ch)))
    per_hop, r = HOP * ch, 512 % ch
    last_start = full = straddles = False
    for name in Q.names(ch):
        n = lens[name]
        for start, length in Q.crops(ch, name):
            assert 0 <= start and length >= 1 and start + length <= n
            at = 512 + start * ch
            p = g.plan_crop(n * ch, ch, start, length)
            if at % per_hop == per_hop - ch + r:       # the last position of a hop that a start can take
                last_start = True
                full = full or p.n_hops == Q.slots(length, ch)[0]
            first, last = at, 512 + (start + length - 1) * ch
            straddles = straddles or any(a // per_hop != (a + ch - 1) // per_hop for a in (first, last))
    assert last_start and full
    assert straddles == (r != 0)
    assert (0, 1) in Q.crops(ch, Q.names(ch)[0])
    if not Q.is_wide(ch):
        for length in Q.CROP_LENGTHS:
            assert sum(c[1] == length for c in Q.crops(ch, "chord2049")) >= 3
    # some planar hop of a pool clip starts its planes at different times exactly where a sample frame can straddle
    j0 = per_hop - 512                                 # hop 1 of a whole clip
    t_lo = {(j0 - c + ch - 1) // ch for c in range(ch)}
    assert (len(t_lo) > 1) == (r != 0)


@pytest.mark.parametrize("ch", CHANNELS)
def test_the_layouts_start_at_every_alignment(ch):
    lens = Q.pool_lengths(ch)
    for planar in (True, False):
        assert Q.start_offsets(ch, len(lens), max(lens), planar) == {0, 1, 2, 3}, planar
        kw = Q.layout_kw(ch, max(lens), planar)
        assert kw["lead"] == 1 and kw["clip_stride"] % 2 == 1 and kw.get("channel_stride", 1) % 2 == 1


@pytest.mark.parametrize("ch", OLD + CHANNELS)
def test_the_model_is_the_definition(ch):
    """Un-mutated, `writes` puts sample t of channel c - position 512 + t ch + c - where the layout says, every element
    once; `slots` is the tight formula of store_draw_cases."""
    for n, start, length, planar in Q.model_cases(ch):
        cs = Q.odd_up(length)
        got = Q.writes(ch, n, start, length, planar, dst=3, cstride=cs)
        want = Q.closed_form(ch, n, start, length, planar, dst=3, cstride=cs)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, start, length, planar)
    for length in (1, 2, 1023, 1024, 1025, 2049):
        assert Q.slots(length, ch) == S.slots(length, ch)


_outcomes = {}


def outcome(ch, mut=None):
    if (ch, mut) not in _outcomes:
        _outcomes[(ch, mut)] = Q.outcome(ch, mut)
    return _outcomes[(ch, mut)]


def seen_at(mut, counts):
    return {ch for ch in counts if outcome(ch, mut) != outcome(ch)}


@pytest.mark.parametrize("mut", Q.MUTATIONS)
def test_every_slip_shows_at_a_new_channel_count(mut):
    assert seen_at(mut, CHANNELS), mut


@pytest.mark.parametrize("mut", Q.NEW_ONLY)
def test_five_slips_show_at_the_new_counts_only(mut):
    """What the suites of 1, 2, 3, 6 and 8 channels could not have seen: nothing changes there."""
    assert len(Q.NEW_ONLY) >= 5
    assert seen_at(mut, OLD) == set(), mut
    want = {"delay_at_least_a_frame": {513}, "plane_index_in_8_bits": {257, 513}, "pow2_takes_the_widest_shift": {16},
            "slot_residue_exclusive": {7}, "hop_index_in_16_bits": {257, 513}}[mut]
    assert seen_at(mut, CHANNELS) == want, mut


@pytest.mark.parametrize("mut", Q.LITERAL)
def test_the_plain_slips_were_visible_before(mut):
    """The slips in their plain form change something at 2, 3 or 6 channels already (the arithmetic of
    channel_axis_cases.SEEN_BEFORE): they are no gap of the old suites, which is why NEW_ONLY exists."""
    assert seen_at(mut, OLD) == Q.SEEN_BEFORE[mut], mut


# ----------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    import glc_amd
    yield torch, glc_amd
    _ctx.clear()             # contexts: released while the library is still loaded
    _dev.clear()


_ctx = {}
_dev = {}


def ctx(g, kind, ch=0):
    if (kind, ch) not in _ctx:
        _ctx[(kind, ch)] = {"enc": lambda: g.Encoder(Q.SR), "rt": lambda: g.RoundTrip(Q.SR)}.get(kind, lambda: g.Decoder(ch, Q.SR))()
    return _ctx[(kind, ch)]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def guarded(n, dtype):
    """A flat host buffer of n elements with GUARD pattern elements on either side -> (whole buffer, the n in the middle)."""
    if dtype == F32:
        buf = np.full(n + 2 * GUARD, NAN_BITS, np.uint32).view(F32)
    else:
        buf = np.full(n + 2 * GUARD, I16_PATTERN, np.int16)
    return buf, buf[GUARD:]


def guard_intact(buf, n):
    w = buf.view(np.uint32) if buf.dtype == F32 else buf
    pat = NAN_BITS if buf.dtype == F32 else I16_PATTERN
    return bool(np.all(w[:GUARD] == pat) and np.all(w[GUARD + n:] == pat))


def nan_tensor(torch, shape):
    return torch.from_numpy(np.full(shape, NAN_BITS, np.uint32).view(F32)).cuda()


def pattern(n, seed=0):
    """A byte pattern with no period a misplaced blob could hide behind."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(seed)
    return ((i * np.uint64(167) + (i >> np.uint64(8)) * np.uint64(13)) % np.uint64(251) + np.uint64(3)).astype(np.uint8)


def refused_cleanly(g, c, rc):
    """An entry point may refuse a channel count, but only like this: GLC_EINVAL and a message (the callers check that
    nothing was written)."""
    assert rc == EINVAL and g.lib.glc_last_error(c._h)
    return True


# ------------------------------------------------------------------------------------------ single stream

@pytest.mark.gpu
@pytest.mark.parametrize("ch", CHANNELS)
def test_single_stream(gpu, ch):
    """Encoder.encode, Decoder.decode (float32 and int16) and glc_roundtrip_device of every pool clip."""
    torch, g = gpu
    enc, dec, rt = ctx(g, "enc"), ctx(g, "dec", ch), ctx(g, "rt")
    for it in Q.pool(ch):
        stream = enc.encode(it.x, ch)
        assert stream.to_bytes() == it.glc, it.name
        for dtype, ref in ((F32, it.dec), (np.int16, it.dec16)):
            buf, out = guarded(it.n, dtype)
            got = dec.decode(stream, out=out, dtype=dtype)
            assert got.size == it.n and guard_intact(buf, it.n), (it.name, dtype)
            assert np.array_equal(bits(got), bits(ref)) if dtype == F32 else np.array_equal(got, ref), (it.name, dtype)
        x = torch.from_numpy(it.x).cuda()
        y = nan_tensor(torch, it.n + 2 * GUARD)
        torch.cuda.synchronize()
        n = rt.apply_device(x.data_ptr(), it.n, ch, y.data_ptr() + 4 * GUARD, it.n)
        rt.synchronize()
        a = y.cpu().numpy()
        assert n == it.n and guard_intact(a, it.n) and np.array_equal(bits(a[GUARD:GUARD + it.n]), bits(it.dec)), it.name
        assert np.array_equal(bits(x.cpu().numpy()), bits(it.x))


# ------------------------------------------------------------------------------------------ host batch

@pytest.mark.gpu
@pytest.mark.parametrize("ch", CHANNELS)
def test_host_batch(gpu, ch):
    """glc_encode_batch and glc_decode_batch (and its int16 form) on the ragged pool."""
    torch, g = gpu
    enc, dec = ctx(g, "enc"), ctx(g, "dec", ch)
    its = [Q.item(ch, n) for n in Q.batch_names(ch)]
    streams = enc.encode_batch([it.x for it in its], ch)
    assert [s.to_bytes() for s in streams] == [it.glc for it in its]
    total = sum(it.n for it in its)
    for dtype in (F32, np.int16):
        buf, out = guarded(total, dtype)
        got = dec.decode_batch(streams, out=out[:total], dtype=dtype)
        assert guard_intact(buf, total) and [a.size for a in got] == [it.n for it in its]
        for a, it in zip(got, its):
            assert np.array_equal(bits(a), bits(it.dec)) if dtype == F32 else np.array_equal(a, it.dec16), (it.name, dtype)


# ------------------------------------------------------------------------------------------ device round trip of a batch

PAIRS = [(True, True), (True, False), (False, True), (False, False)]


def batch(ch, planar):
    import test_roundtrip_batch as RB
    its = [Q.item(ch, n) for n in Q.batch_names(ch)]
    T = max(it.pc for it in its)
    return RB.Batch([it.x for it in its], ch, planar, **Q.layout_kw(ch, T, planar)), its


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS + ["in-place-planar", "in-place-interleaved"],
                         ids=["planar-planar", "planar-interleaved", "interleaved-planar", "interleaved-interleaved", "in-place-planar",
                              "in-place-interleaved"])
@pytest.mark.parametrize("ch", CHANNELS)
def test_roundtrip_batch(gpu, ch, pair):
    """glc_roundtrip_batch_device from and to strided layouts that start planes and clips at every alignment: every
    word of the output buffer, and the input unchanged."""
    import test_roundtrip_batch as RB
    torch, g = gpu
    rt = ctx(g, "rt")
    if isinstance(pair, str):
        src, its = batch(ch, pair == "in-place-planar")
        RB.run(torch, rt, src, src, [it.dec for it in its], in_place=True)
    else:
        src, its = batch(ch, pair[0])
        dst, _ = batch(ch, pair[1])
        RB.run(torch, rt, src, dst, [it.dec for it in its])
    infos = rt.last_batch_info()
    assert [i.n_frames for i in infos] == [it.nf for it in its]
    assert [i.n_raw_frames for i in infos] == [sum(it.raw) for it in its]
    assert [i.serialized_bytes for i in infos] == [len(it.glc) for it in its]


# ------------------------------------------------------------------------------------------ the store, written

def blob_counts(blob):
    import struct
    _, _, _, n_pairs, n_raw, nbytes = struct.unpack_from("<IIQQQQ", blob.tobytes()[:64], 0)
    assert nbytes == blob.size and nbytes % 64 == 0
    return n_pairs, n_raw


@pytest.mark.gpu
@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
@pytest.mark.parametrize("ch", CHANNELS)
def test_store_write(gpu, ch, planar):
    """glc_encode_batch_device_compact: entries, cursor and EVERY byte of a pattern-filled arena against the model of
    compact_store_cases over the host twin's blobs of the oracle's records; a blob cut from the arena is the oracle's
    stream."""
    torch, g = gpu
    enc = ctx(g, "enc")
    src, its = batch(ch, planar)
    in_words = src.fill(src.clips)
    store, x = src.tensor(torch, in_words)
    cursor0 = 77
    blobs = [(it.blob_enc,) + blob_counts(it.blob_enc) for it in its]
    need = CS.store_model(None, None, cursor0, 1 << 62, blobs=blobs)[2]
    entries, bl, cur = CS.store_model(None, None, cursor0, need, blobs=blobs)
    image = pattern(need + TAIL, seed=ch)
    arena = torch.from_numpy(image).cuda()
    cursor = torch.tensor([cursor0], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    a, c, ent = enc.encode_compact_batch_tensor(x, lengths=src.lens, planar=planar, arena=arena, cursor=cursor)
    torch.cuda.synchronize()
    assert a is arena and c is cursor and g.lib.glc_ctx_resident_stream(enc._h) == 0
    assert np.array_equal(ent.cpu().numpy(), CS.entry_rows(entries))
    assert int(cursor.item()) == cur == need and all(e[4] == 1 for e in entries)
    have, want = arena.cpu().numpy(), CS.arena_image(image.size, entries, bl, image)
    bad = np.flatnonzero(have != want)
    assert bad.size == 0, f"{bad.size} arena bytes differ, first at {bad[0]} (entries {entries[:3]})"
    assert np.array_equal(store.cpu().numpy().view(np.uint32), in_words)
    assert need <= g.compact_store_bound(ch, src.lens)
    for (off, nbytes, _, _, _), it in zip(entries, its):
        assert g.EncodedAudio.from_compact(Q.SR, it.n, ch, [have[off:off + nbytes]]).to_bytes() == it.glc, it.name


# ------------------------------------------------------------------------------------------ the store, read

class HostStore:
    """A store the HOST builds from the oracle's streams (glc_frames_to_compact), on the device: the pool's blobs back
    to back, then a copy of the longest chord's blob with a damaged magic, then an entry that holds nothing."""

    def __init__(self, torch, ch):
        self.ch = ch
        self.its = Q.pool(ch)
        off, entries, parts = 0, [], []
        self.src = self.its[-1] if Q.is_wide(ch) else self.its[4]      # long enough for every crop length
        damaged = self.src.blob.copy()
        damaged[:4] = np.frombuffer(np.uint32(K.MAGIC ^ 0x100).tobytes(), np.uint8)
        for b in [it.blob for it in self.its] + [damaged]:
            assert b.size % 64 == 0
            entries.append(S.entry(off, b.size))
            parts.append(b)
            off += b.size
        entries.append(S.entry(0, self.src.blob.size, stored=0))
        self.host_entries = entries
        self.host_lengths = [it.pc for it in self.its] + [self.src.pc, self.src.pc]
        self.n_good, self.i_damaged, self.i_empty = len(self.its), len(self.its), len(self.its) + 1
        self.arena = torch.from_numpy(np.concatenate(parts)).cuda()
        assert self.arena.data_ptr() % 64 == 0
        self.entries = torch.tensor(entries, dtype=torch.int64).cuda()
        self.lengths = torch.tensor(self.host_lengths, dtype=torch.int64).cuda()
        self.max_length = max(self.host_lengths)

    def blob(self, e):
        off, nbytes = self.host_entries[e][:2]
        return self.arena[off:off + nbytes]

    def ref(self, e):
        """The whole-clip decode an entry's crops are slices of (+0.0 for the damaged blob)."""
        return self.its[e].dec if e < self.n_good else np.zeros(self.src.n, F32)


def host_store(torch, ch):
    if ("store", ch) not in _dev:
        _dev.clear()             # one channel count's store at a time
        _dev[("store", ch)] = HostStore(torch, ch)
    return _dev[("store", ch)]


def status_words(st):
    return [(s.flags, s.n_bad_rows, s.first_bad_row) for s in st]


@pytest.mark.gpu
@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
@pytest.mark.parametrize("ch", CHANNELS)
def test_store_read_whole_clips(gpu, ch, planar):
    """glc_decode_batch_device_compact of the host-built store into a strided batch; the damaged blob is silence."""
    import test_roundtrip_batch as RB
    torch, g = gpu
    dec = ctx(g, "dec", ch)
    st = host_store(torch, ch)
    order = list(range(st.n_good)) + [st.i_damaged] + ([0, 1] if Q.is_wide(ch) else [])
    refs = [st.ref(e) for e in order]
    T = max(r.size // ch for r in refs)
    dst = RB.Batch(refs, ch, planar, **Q.layout_kw(ch, T, planar))
    out_store, out = dst.tensor(torch, np.full(dst.size, NAN_BITS, np.uint32))
    torch.cuda.synchronize()
    got = dec.decode_compact_batch_tensor([st.blob(e) for e in order], [r.size for r in refs], lengths=dst.lens, planar=planar, out=out)
    torch.cuda.synchronize()
    assert got is out and g.lib.glc_ctx_resident_stream(dec._h) == 0
    have, want = out_store.cpu().numpy().view(np.uint32), dst.fill(refs)
    bad = np.flatnonzero(have != want)
    assert bad.size == 0, f"{bad.size} words differ, first at {bad[0]} of {have.size}"
    words = status_words(dec.last_compact_status())
    m = st.src.nf * ch
    assert words == [(0, 0, 0) if e != st.i_damaged else (K.BAD_HEADER, m, 0) for e in order]


def decode_crops(g, torch, dec, ch, st, sels, planar):
    """sels: (entry, start, length).  One glc_decode_crops_device_compact call into the leading slice of a bigger
    pattern tensor: every element against the slices / the pattern -> status words."""
    b = len(sels)
    l_max = max(s[2] for s in sels)
    shape = (b + 1, ch + 1, l_max + 3) if planar else (b + 1, l_max + 1, ch)
    big = nan_tensor(torch, shape)
    out = big[:b, :ch, 1:1 + l_max] if planar else big[:b, :l_max, :]
    torch.cuda.synchronize()
    got = dec.decode_compact_crops_tensor([st.blob(e) for e, _, _ in sels], [st.host_lengths[e] * ch for e, _, _ in sels],
                                          [s for _, s, _ in sels], [l for _, _, l in sels], planar=planar, out=out)
    torch.cuda.synchronize()
    assert got is out and g.lib.glc_ctx_resident_stream(dec._h) == 0
    want = CC.want_crops(shape, planar, 1, ch, [(st.ref(e), s, l) for e, s, l in sels])
    host = big.cpu().numpy().view(np.uint32)
    if not np.array_equal(host, want):
        rows = sorted({int(i) for i in np.argwhere(host != want)[:, 0]})
        raise AssertionError(f"crops {rows[:8]} differ: {[sels[i] for i in rows[:8] if i < b]}")
    return status_words(dec.last_compact_status())


@pytest.mark.gpu
@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
@pytest.mark.parametrize("ch", CHANNELS)
def test_store_read_crops_by_pointer(gpu, ch, planar):
    """glc_decode_crops_device_compact: every crop of channel_axis_cases.crops is the slice of the oracle's decode."""
    torch, g = gpu
    dec = ctx(g, "dec", ch)
    st = host_store(torch, ch)
    sels = [(e, s, l) for e, it in enumerate(st.its) for s, l in Q.crops(ch, it.name)]
    p = g.plan_crop(st.src.n, ch, 0, 1)
    damaged = (st.i_damaged, 0, 1)
    short = [s for s in sels if s[2] <= 1025]
    long = [s for s in sels if s[2] > 1025]
    assert short and (long or Q.is_wide(ch))
    for group in (short + [damaged], long[:len(long) // 2] + [damaged], long[len(long) // 2:]):
        if not group:
            continue
        words = decode_crops(g, torch, dec, ch, st, group, planar)
        assert words == [(0, 0, 0) if s != damaged else (K.BAD_HEADER, p.n_frames * ch, p.first_frame * ch) for s in group]


def draw(g, torch, dec, ch, st, sels, length, planar):
    """sels: (clip index, start).  One glc_decode_crops_device_store call -> (status words, verdicts of the model)."""
    b = len(sels)
    shape = (b + 1, ch + 1, length + 3) if planar else (b + 1, length + 1, ch)
    big = nan_tensor(torch, shape)
    out = big[:b, :ch, 1:1 + length] if planar else big[:b, :length, :]
    cl = torch.tensor([c for c, _ in sels], dtype=torch.int64).cuda()
    stt = torch.tensor([s for _, s in sels], dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    got = dec.decode_store_crops_tensor(st.arena, st.entries, st.lengths, cl, stt, length, st.max_length, planar=planar, out=out)
    torch.cuda.synchronize()
    assert got is out and g.lib.glc_ctx_resident_stream(dec._h) == 0
    verdicts = [S.verdict_of(st.host_entries, st.host_lengths, st.arena.numel(), st.max_length, c, s, length) for c, s in sels]
    want = CC.want_crops(shape, planar, 1, ch, [(np.zeros(length * ch, F32), 0, length) if v else (st.ref(c), s, length)
                                                for v, (c, s) in zip(verdicts, sels)])
    host = big.cpu().numpy().view(np.uint32)
    if not np.array_equal(host, want):
        rows = sorted({int(i) for i in np.argwhere(host != want)[:, 0]})
        raise AssertionError(f"draws {rows[:8]} of length {length} differ: {[sels[i] for i in rows[:8] if i < b]}")
    return status_words(dec.last_compact_status()), verdicts


def draw_selections(ch, st, length):
    """The boundary starts of every pool clip, then the damaged blob, the empty entry and a clip index outside the store."""
    return Q.draws(ch, length) + [(st.i_damaged, 0), (st.i_empty, 0), (st.i_empty + 5, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
@pytest.mark.parametrize("ch", CHANNELS)
def test_store_read_draws(gpu, ch, planar):
    """glc_decode_crops_device_store at every boundary start of lengths 1, 1024 and 1025 (1 and 2 for the wide counts)."""
    torch, g = gpu
    dec = ctx(g, "dec", ch)
    st = host_store(torch, ch)
    for length in (Q.WIDE_DRAW_LENGTHS if Q.is_wide(ch) else Q.CROP_LENGTHS):
        sels = draw_selections(ch, st, length)
        assert len(sels) >= 3 + 2 * len(st.its)
        words, verdicts = draw(g, torch, dec, ch, st, sels, length, planar)
        assert verdicts[-3:] == [0, S.NO_BLOB, S.BAD_CROP] and not any(verdicts[:-3])
        pd = g.plan_crop(st.src.n, ch, 0, length)
        assert words[-3:] == [(K.BAD_HEADER, pd.n_frames * ch, pd.first_frame * ch), (S.NO_BLOB | S.BAD_HEADER, 0, 0),
                              (S.BAD_CROP | S.BAD_HEADER, 0, 0)]
        assert all(w == (0, 0, 0) for w in words[:-3])


# ------------------------------------------------------------------------------------------ the hooks

@pytest.mark.gpu
@pytest.mark.parametrize("ch", CHANNELS)
def test_hook_store_plan(gpu, ch):
    """glc_debug_store_plan_device against store_draw_cases.plan_model, planar and interleaved."""
    torch, g = gpu
    dec = ctx(g, "dec", ch)
    st = host_store(torch, ch)
    f = g.lib.glc_debug_store_plan_device
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                  C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ab = st.arena.numel()
    for length in (Q.WIDE_DRAW_LENGTHS if Q.is_wide(ch) else Q.CROP_LENGTHS):
        sels = draw_selections(ch, st, length)
        n = len(sels)
        clips, starts = [c for c, _ in sels], [s for _, s in sels]
        cl, stt = torch.tensor(clips, dtype=torch.int64).cuda(), torch.tensor(starts, dtype=torch.int64).cuda()
        max_hops = S.slots(length, ch)[0]
        assert g.store_crop_slots(length, ch)[0] == max_hops
        for planar in (True, False):
            chs = length + 3 if planar else 0
            cs = ch * (length + 3) + 5 if planar else length * ch + 7
            lay = g._lib.GlcClipLayout(n, ch, 1 if planar else 0, cs, chs, length, None)
            dirs, descs, verd = np.zeros(n, S.DIR_DTYPE), np.zeros(n * max_hops, S.DESC_DTYPE), np.zeros(n, np.uint32)
            torch.cuda.synchronize()
            rc = f(dec._h, FAKE_ARENA, ab, st.entries.data_ptr(), st.lengths.data_ptr(), st.entries.shape[0], st.max_length,
                   cl.data_ptr(), stt.data_ptr(), length, FAKE_OUT, C.addressof(lay), dirs.ctypes.data, descs.ctypes.data,
                   verd.ctypes.data)
            assert rc == 0, g.lib.glc_last_error(dec._h)
            want = S.plan_model(g, FAKE_ARENA, ab, st.host_entries, st.host_lengths, st.max_length, clips, starts, length, ch,
                                planar, cs, chs)
            got = (dirs.tolist(), descs.reshape(n, max_hops).tolist(), verd.tolist())
            for what, a, b in zip(("directory", "descriptors", "verdicts"), got, want):
                for i, (x, y) in enumerate(zip(a, b)):
                    assert x == y or [tuple(r) for r in x] == y, (what, "crop", i, sels[i], length, planar, x, y)
            assert want[2][-3:] == [0, S.NO_BLOB, S.BAD_CROP]


@pytest.mark.gpu
@pytest.mark.parametrize("ch", CHANNELS)
def test_hook_rows_of_a_window(gpu, ch):
    """glc_debug_rows_from_compact_window against the whole-blob tables, one window per clip that starts inside it."""
    torch, g = gpu
    dec = ctx(g, "dec", ch)
    st = host_store(torch, ch)
    f = g.lib.glc_debug_rows_from_compact_window
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint16, C.c_uint64, C.c_uint64] + [C.c_void_p] * 6
    inside = 0
    for e, it in enumerate(st.its):
        full = Q.tables_of_blob(it.blob, ch)
        start = 5 * HOP + 100 if it.name == "mixed" else it.pc - 1      # the last sample of a short clip: its last hop
        p = g.plan_crop(it.n, ch, start, min(it.pc - start, 1500))
        f0, frames = p.first_frame, p.n_frames
        inside += f0 > 0
        m = frames * ch
        begin, cnt, raw = np.empty(m, np.uint64), np.empty(m, np.uint32), np.empty(m, np.int64)
        words = (C.c_uint64 * 3)()
        d_blob = st.blob(e)
        torch.cuda.synchronize()
        rc = f(dec._h, d_blob.data_ptr(), d_blob.numel(), it.nf, ch, f0, frames, begin.ctypes.data, cnt.ctypes.data, None,
               raw.ctypes.data, None, C.addressof(words))
        assert rc == 0, g.lib.glc_last_error(dec._h)
        assert (words[0] & 0xFFFFFFFF, words[1], words[2]) == (0, 0, 0), it.name
        for got, whole in zip((begin, cnt, raw), full):
            assert np.array_equal(got, whole[f0 * ch:(f0 + frames) * ch]), (it.name, f0, frames)
    assert inside >= 2 or Q.is_wide(ch)                # (the two wide clips end inside hop 1: every window has frame 0)


def pack_case(ch):
    """Three clips of 3, 1 and 2 frames with a junk record behind each: raw frames first and last in a clip."""
    kind = lambda i, f: "raw" if (i == 0 and f in (0, 2)) or (i == 2 and f == 1) else "sparse"
    return CS._build(ch, [3, 1, 2], kind, CS._alt, 9100 + ch, hi=4), (3, 1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("ch", CHANNELS)
def test_hook_pack_with_junk_between_clips(gpu, ch):
    """glc_debug_compact_store_device on records built by hand, a junk record behind every clip: entries, cursor and
    every byte of the arena against compact_store_cases.store_model."""
    torch, g = gpu
    enc = ctx(g, "enc")
    desc, clips = pack_case(ch)
    assert ch % 2 == 0 or (clips[0] * ch) % 4 != 0     # rows per clip: no multiple of 4 wherever ch allows it
    f = g.lib.glc_debug_compact_store_device
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint16, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    cursor0 = 100
    need = CS.store_model(desc, clips, cursor0, 1 << 62)[2]
    entries, blobs, cur = CS.store_model(desc, clips, cursor0, need)
    image = pattern(need + TAIL, seed=3 * ch)
    arena = torch.from_numpy(image).cuda()
    d_rec = E.materialise_torch(desc, torch)
    d_cursor = torch.tensor([cursor0], dtype=torch.int64, device="cuda")
    d_entries = torch.full((len(clips), 4), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = f(enc._h, d_rec.data_ptr(), (C.c_uint64 * len(clips))(*clips), len(clips), ch, arena.data_ptr(), need, d_cursor.data_ptr(),
           d_entries.data_ptr())
    assert rc == 0, g.lib.glc_last_error(enc._h)
    enc.synchronize()
    assert np.array_equal(d_entries.cpu().numpy(), CS.entry_rows(entries)) and int(d_cursor.item()) == cur
    have, want = arena.cpu().numpy(), CS.arena_image(image.size, entries, blobs, image)
    bad = np.flatnonzero(have != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[0]} (entries {entries})"
