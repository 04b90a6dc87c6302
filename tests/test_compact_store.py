"""glc_encode_batch_device_compact: a batch of device-resident clips into one self-describing compact blob per clip,
placed back to back in an arena by a cursor the device keeps (tests/compact_store_cases.py holds the model).

Every arena is prefilled with a byte pattern; after the call EVERY byte of it is compared - the stored blobs where the
model puts them, the pattern everywhere else, in front of the initial cursor and behind the final one.  The pack
kernels A1-A3 run alone through glc_debug_compact_store_device on records built by hand; the driver is held to
Encoder.encode_compact_tensor clip by clip (the same bytes), to Encoder.encode and the CPU oracle through
EncodedAudio.from_compact, and to the round trip through the compact batch decode.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import compact_edges as E
import compact_store_cases as S
import roundtrip_cases as RC
from conftest import O
import conftest as cf

HOP = RC.HOP
F32 = np.float32
SR = 48000
EINVAL = -1
NAN_BITS = 0x7FC00ABC
TAIL = 8192                  # pattern bytes behind what the clips need


# ----------------------------------------------------------------------------------------------------
# CPU: the cases reach their edges, and every rule of the model bites
# ----------------------------------------------------------------------------------------------------

def _expected(c, arena_bytes=None, mutation=None):
    need = S.store_model(c.desc, c.clip_frames, c.cursor0, 1 << 62)[2]
    cap = need if arena_bytes is None else arena_bytes
    return S.store_model(c.desc, c.clip_frames, c.cursor0, cap, mutation), need


def test_cases_reach_their_edges():
    names = {c.name for c in S.cases()}
    assert {f"edges-ch{ch}" for ch in (1, 2, 3, 6)} <= names
    assert S.case("one-clip-one-frame").clip_frames == (1,) and S.case("three-one-frame-clips").clip_frames == (1, 1, 1)
    for ch in (1, 2, 3, 6):
        c = S.case(f"edges-ch{ch}")
        assert c.clip_frames == (3, 1, 64, 65)
        descs = S.clip_descs(c.desc, c.clip_frames)
        assert descs[0].flags[0] and descs[3].flags[-1] and descs[2].flags[0]          # a raw frame first and last in a clip
        o = E.layout(ch, 64), E.layout(ch, 65)
        assert o[0][1] - (o[0][0] + 64) == 0 and o[1][1] - (o[1][0] + 65) == 63          # no raw-flag gap, then one of 63 bytes
    assert len({4 * 3 * ch % 64 for ch in (1, 2, 3, 6)}) == 4                              # 4 M mod 64 of the first clip varies
    assert any(c.cursor0 % 64 for c in S.cases()) and any(c.cursor0 % 64 == 0 for c in S.cases())
    c = S.case("all-raw-and-silent")
    (entries, blobs, _), _ = _expected(c)
    descs = S.clip_descs(c.desc, c.clip_frames)
    assert descs[0].flags.all() and entries[0][2] == 0 and entries[0][3] == 2 * 2
    assert entries[1][1] == E.layout(2, 3)[3] and entries[1][2] == 0 and entries[1][3] == 0   # silent: bytes == o_pairs
    c = S.case("nnz-disagrees")
    assert not c.desc.consistent()
    for c in S.cases():                                                                   # junk that would show if it leaked
        slot = 0
        for n in c.clip_frames:
            j = slot + n
            assert c.desc.flags[j] != 0 or (c.desc.nnz[j * c.desc.ch:(j + 1) * c.desc.ch] == HOP).all()
            slot += n + 1
    c = S.case("clip-across-a-scan-block")
    assert 5 < 1024 < 5 + 1030 and c.clip_frames[1] * c.desc.ch > 1024
    assert S.case("clip-of-1200-rows-ch3").clip_frames[0] * 3 > 1024
    assert len(S.case("1100-mono-clips").clip_frames) == 1100 > 1024                       # the second chunk of A2's clip scan


def test_every_blob_is_a_multiple_of_64_and_offsets_ascend():
    for c in S.cases():
        (entries, blobs, cursor), need = _expected(c)
        assert all(e[1] % 64 == 0 and e[0] % 64 == 0 and e[4] == 1 for e in entries), c.name
        offs = [e[0] for e in entries]
        assert offs == sorted(offs) and offs[0] == S.align64(c.cursor0)
        assert cursor == need == offs[-1] + entries[-1][1]


def _outcome(c, cap, mutation):
    entries, blobs, cursor = S.store_model(c.desc, c.clip_frames, c.cursor0, cap, mutation)
    size = max(cursor, max(e[0] + e[1] for e in entries)) + TAIL
    return S.entry_rows(entries).tobytes(), S.arena_image(size, entries, blobs).tobytes(), cursor


@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_every_rule_bites(mutation):
    """One rule of the store changed at a time: the expected arena, entries or cursor of some case differs."""
    hit = []
    for c in S.cases():
        if len(c.clip_frames) > 100:
            continue
        need = S.store_model(c.desc, c.clip_frames, c.cursor0, 1 << 62)[2]
        caps = [need]
        if len(c.clip_frames) > 1:                    # the capacity rules show only where something does not fit
            e = S.store_model(c.desc, c.clip_frames, c.cursor0, need)[0]
            caps.append(e[1][0] + e[1][1] - 64)       # cut inside clip 1
        for cap in caps:
            if _outcome(c, cap, None) != _outcome(c, cap, mutation):
                hit.append((c.name, cap))
    assert hit, mutation


# ----------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    import glc_amd
    f = glc_amd.lib.glc_debug_compact_store_device
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint16, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    yield torch, glc_amd
    _ctx.clear()


_ctx = {}


def ctx(g, kind, ch=2):
    key = (kind, ch)
    if key not in _ctx:
        _ctx[key] = {"enc": lambda: g.Encoder(SR), "dec": lambda: g.Decoder(ch, SR), "rt": lambda: g.RoundTrip(SR)}[kind]()
    return _ctx[key]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _pattern(n, seed=0):
    """A byte pattern with no period a misplaced blob could hide behind."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(seed)
    return ((i * np.uint64(167) + (i >> np.uint64(8)) * np.uint64(13)) % np.uint64(251) + np.uint64(3)).astype(np.uint8)


_records = {}


def _upload(torch, c):
    if c.name not in _records:
        _records[c.name] = E.materialise_torch(c.desc, torch)
    return _records[c.name]


def _hook(gpu, c, arena, arena_bytes, cursor):
    torch, g = gpu
    enc = ctx(g, "enc")
    clips, d_rec = c.clip_frames, _upload(torch, c)
    entries = torch.full((len(clips), 4), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = g.lib.glc_debug_compact_store_device(enc._h, d_rec.data_ptr(), (C.c_uint64 * len(clips))(*clips), len(clips), c.desc.ch,
                                              arena.data_ptr(), arena_bytes, cursor.data_ptr(), entries.data_ptr())
    assert rc == 0, (c.name, g.lib.glc_last_error(enc._h))
    return entries


def _run_hook(gpu, c, arena_bytes=None, what=None):
    """The pack alone over case `c` into a pattern-filled arena of which `arena_bytes` are offered (default: exactly
    what the clips need): entries, cursor and every byte of the arena against the model."""
    torch, g = gpu
    (entries, blobs, cursor), need = _expected(c, arena_bytes)
    cap = need if arena_bytes is None else arena_bytes
    image = _pattern(max(need, cap) + TAIL)
    arena = torch.from_numpy(image).cuda()
    d_cursor = torch.tensor([c.cursor0], dtype=torch.int64, device="cuda")
    got = _hook(gpu, c, arena, cap, d_cursor)
    ctx(g, "enc").synchronize()
    what = what or c.name
    print(f"{what}: {len(entries)} clips, need {need} bytes, offered {cap}, stored {sum(e[4] for e in entries)}")
    assert np.array_equal(got.cpu().numpy(), S.entry_rows(entries)), what
    assert int(d_cursor.item()) == cursor, what
    want = S.arena_image(image.size, entries, blobs, image)
    have = arena.cpu().numpy()
    bad = np.flatnonzero(have != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[0]} (cursor0 {c.cursor0}, entries {entries[:4]})"
    return entries


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in S.cases()])
def test_pack_kernels_at_their_edges(gpu, name):
    _run_hook(gpu, S.case(name))


@pytest.mark.gpu
def test_capacity(gpu):
    """A fixed set of clips against arenas that hold all of them, all but the last, a prefix, and nothing."""
    torch, g = gpu
    c = S.case("edges-ch2")
    (full, _, need), _ = _expected(c)
    assert all(e[4] for e in _run_hook(gpu, c, need, "exactly the sum"))
    e = _run_hook(gpu, c, need - 64, "64 bytes less")
    assert [x[4] for x in e] == [1, 1, 1, 0] and e[3][:2] == full[3][:2]                  # the would-be offset and size
    for k in (1, 2):
        e = _run_hook(gpu, c, full[k][0] + full[k][1] // 2, f"cut inside clip {k}")
        assert [x[4] for x in e] == [1] * k + [0] * (4 - k) and [x[:4] for x in e] == [x[:4] for x in full]
    assert not any(x[4] for x in _run_hook(gpu, c, 0, "arena_bytes == 0"))
    # a further call after an overflow stores nothing and still advances the cursor
    cap = full[2][0] + 64
    image = _pattern(2 * need + TAIL, seed=5)
    arena = torch.from_numpy(image).cuda()
    d_cursor = torch.tensor([c.cursor0], dtype=torch.int64, device="cuda")
    e1 = _hook(gpu, c, arena, cap, d_cursor)
    e2 = _hook(gpu, c, arena, cap, d_cursor)
    ctx(g, "enc").synchronize()
    m1, blobs, c1 = S.store_model(c.desc, c.clip_frames, c.cursor0, cap)
    m2, _, c2 = S.store_model(c.desc, c.clip_frames, c1, cap)
    assert [x[4] for x in m1] == [1, 1, 0, 0] and not any(x[4] for x in m2) and c2 == c1 + (need - S.align64(c.cursor0))
    assert np.array_equal(e1.cpu().numpy(), S.entry_rows(m1)) and np.array_equal(e2.cpu().numpy(), S.entry_rows(m2))
    assert int(d_cursor.item()) == c2
    assert np.array_equal(arena.cpu().numpy(), S.arena_image(image.size, m1, blobs, image))


# ------------------------------------------------------------------------------------------ the driver

_pool = {}


def clip_pool(g, torch, ch):
    """Clips of mixed kinds with what the single path makes of each: (samples, blob bytes of encode_compact_tensor)."""
    if ch not in _pool:
        enc = ctx(g, "enc")
        tone = cf.gen_tone("sine", 440.0, SR, ch, 0.1)
        xs = [tone,
              np.concatenate([RC.lcg_noise(2 * HOP * ch, seed=9), cf.gen_tone("sine", 1000.0, SR, ch, 0.07)]),   # raw then compressed
              np.zeros(700 * ch, F32),
              RC.chord(SR, ch, 513),
              RC.chord(SR, ch, 2 * HOP + 77, seed=2), RC.chord(SR, ch, 5 * HOP, seed=5), RC.chord(SR, ch, 3 * HOP + 1, seed=6)]
        pool = []
        for x in xs:
            x = np.ascontiguousarray(x, F32)
            blob, info = enc.encode_compact_tensor(torch.from_numpy(x).cuda(), ch)
            pool.append((x, blob.cpu().numpy().copy()))
        _pool[ch] = pool
    return _pool[ch]


def padded(torch, clips, ch, planar, margin=0):
    """The clips in a NaN-pattern batch tensor (a slice of a bigger one when margin > 0) -> (storage, x, lengths)."""
    lens = [x.size // ch for x in clips]
    b, t = len(clips), max(lens)
    shape = (b + margin, ch + margin, t + 3 * margin) if planar else (b + margin, t + margin, ch)
    host = np.full(shape, NAN_BITS, np.uint32)
    for i, x in enumerate(clips):
        a = bits(x).reshape(lens[i], ch)
        if planar:
            host[i, :ch, margin:margin + lens[i]] = a.T
        else:
            host[i, :lens[i], :] = a
    big = torch.from_numpy(host.view(F32)).cuda()
    x = big[:b, :ch, margin:margin + t] if planar else big[:b, :t, :]
    return big, x, lens


def run_driver(gpu, clips, want_blobs, ch, planar, margin=0, cursor0=0, slack=TAIL, what=""):
    """One call over `clips`; the arena (pattern, cursor0 bytes in use) must hold want_blobs back to back from the
    rounded cursor and the pattern everywhere else; the input is unchanged."""
    torch, g = gpu
    enc = ctx(g, "enc")
    big, x, lens = padded(torch, clips, ch, planar, margin)
    before = big.clone()
    at = S.align64(cursor0)
    entries = []
    for bl in want_blobs:
        hdr = np.frombuffer(bl[:64].tobytes(), np.uint64)
        assert int(hdr[4]) == bl.size and bl.size % 64 == 0
        entries.append((at, bl.size, int(hdr[2]), int(hdr[3]), 1))
        at += bl.size
    image = _pattern(at + slack, seed=11)
    arena = torch.from_numpy(image).cuda()
    cursor = torch.tensor([cursor0], dtype=torch.int64, device="cuda")
    a, cur, ent = enc.encode_compact_batch_tensor(x, lengths=lens, planar=planar, arena=arena, cursor=cursor)
    assert a is arena and cur is cursor and g.lib.glc_ctx_resident_stream(enc._h) == 0
    torch.cuda.synchronize()
    print(f"{what}: {len(clips)} clips, {at - S.align64(cursor0)} blob bytes against a bound of {g.compact_store_bound(ch, lens)}")
    assert np.array_equal(ent.cpu().numpy(), S.entry_rows(entries)), what
    assert int(cur.item()) == at
    have, want = arena.cpu().numpy(), S.arena_image(image.size, entries, want_blobs, image)
    bad = np.flatnonzero(have != want)
    assert bad.size == 0, f"{what}: {bad.size} arena bytes differ, first at {bad[0]}"
    assert torch.equal(big.view(torch.int32), before.view(torch.int32))
    return arena, ent, lens, x


@pytest.mark.gpu
@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
@pytest.mark.parametrize("n_clips", (1, 2, 64, 300))
def test_driver_equals_the_single_path(gpu, n_clips, planar):
    torch, g = gpu
    pool = clip_pool(g, torch, 2)
    pick = [pool[(i * 5 + 1) % len(pool)] for i in range(n_clips)]
    run_driver(gpu, [p[0] for p in pick], [p[1] for p in pick], 2, planar, cursor0=n_clips, what=f"{n_clips} clips")


@pytest.mark.gpu
@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
def test_driver_on_a_slice_of_a_bigger_tensor(gpu, planar):
    torch, g = gpu
    pool = clip_pool(g, torch, 3)
    pick = [pool[i % len(pool)] for i in range(9)]
    run_driver(gpu, [p[0] for p in pick], [p[1] for p in pick], 3, planar, margin=2, what="slice")


@pytest.mark.gpu
@pytest.mark.parametrize("ch", (1, 2))
def test_blobs_are_the_streams_of_encode_and_of_the_oracle(gpu, ch):
    """EncodedAudio.from_compact of a blob cut from the arena serialises to Encoder.encode's bytes and the oracle's."""
    torch, g = gpu
    pool = clip_pool(g, torch, ch)
    arena, ent, lens, _ = run_driver(gpu, [p[0] for p in pool], [p[1] for p in pool], ch, True, what="pool")
    blobs = g.store_blobs(arena, ent)
    assert len(blobs) == len(pool) and all(b is not None for b in blobs)
    for (x, _), blob in zip(pool, blobs):
        data = g.EncodedAudio.from_compact(SR, x.size, ch, [blob.cpu().numpy()]).to_bytes()
        assert data == ctx(g, "enc").encode(x, ch).to_bytes()
        assert data == O.encode(x, SR, ch).glc


@pytest.mark.gpu
def test_append(gpu):
    """Two calls over the halves of a batch with one cursor leave what one call over the whole batch leaves."""
    torch, g = gpu
    enc = ctx(g, "enc")
    pool = clip_pool(g, torch, 2)
    pick = [pool[(i * 3 + 2) % len(pool)] for i in range(10)]
    arena_w, ent_w, lens, x = run_driver(gpu, [p[0] for p in pick], [p[1] for p in pick], 2, True, cursor0=77, what="whole")
    arena = torch.from_numpy(_pattern(arena_w.numel(), seed=11)).cuda()
    cursor = torch.tensor([77], dtype=torch.int64, device="cuda")
    _, _, e1 = enc.encode_compact_batch_tensor(x[:4], lengths=lens[:4], arena=arena, cursor=cursor)
    _, _, e2 = enc.encode_compact_batch_tensor(x[4:], lengths=lens[4:], arena=arena, cursor=cursor)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([e1, e2]), ent_w) and torch.equal(arena, arena_w)
    assert int(cursor.item()) == int(ent_w[-1, 0] + ent_w[-1, 1])


@pytest.mark.gpu
def test_batch_of_several_rounds(gpu):
    """More virtual frames than a stereo round of 4096 holds: 1300 clips of up to 6 frames."""
    torch, g = gpu
    pool = clip_pool(g, torch, 2)
    pick = [pool[(i * 4 + 3) % len(pool)] for i in range(1300)]
    assert sum(RC.frames_of(p[0].size // 2) + 1 for p in pick) > 4096
    run_driver(gpu, [p[0] for p in pick], [p[1] for p in pick], 2, True, cursor0=5, what="rounds")


@pytest.mark.gpu
def test_a_clip_longer_than_a_round_in_the_middle(gpu):
    """A mono clip of one frame more than a round between short ones: packed as a round of its own, and the offsets
    still ascend with the clip index."""
    torch, g = gpu
    enc = ctx(g, "enc")
    pool = clip_pool(g, torch, 1)
    per = 8193 * HOP - 100
    assert RC.frames_of(per) == 8193
    t = np.arange(per, dtype=np.float64) / SR
    long = (0.3 * np.sin(2 * np.pi * 523.25 * t) + 0.1 * np.sin(2 * np.pi * 3111.0 * t)).astype(F32)
    long[40 * HOP:42 * HOP] = RC.lcg_noise(2 * HOP, seed=3)                    # raw frames inside it
    blob, _ = enc.encode_compact_tensor(torch.from_numpy(long).cuda(), 1)
    clips = [pool[1][0], pool[4][0], long, pool[0][0], pool[3][0]]
    wants = [pool[1][1], pool[4][1], blob.cpu().numpy().copy(), pool[0][1], pool[3][1]]
    _, ent, _, _ = run_driver(gpu, clips, wants, 1, True, cursor0=1, what="long clip")
    offs = ent[:, 0].cpu().numpy()
    assert (np.diff(offs) > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
def test_closed_loop(gpu, planar):
    """Decoding the store gives the batch round trip bit for bit, with a clean status."""
    torch, g = gpu
    enc, dec, rt = ctx(g, "enc"), ctx(g, "dec", 2), ctx(g, "rt")
    pool = clip_pool(g, torch, 2)
    clips = [pool[(i * 2 + 1) % len(pool)][0] for i in range(12)]
    _, x, lens = padded(torch, clips, 2, planar)
    arena, cursor, ent = enc.encode_compact_batch_tensor(x, lengths=lens, planar=planar)
    y = dec.decode_compact_batch_tensor(g.store_blobs(arena, ent), [2 * n for n in lens], lengths=lens, planar=planar)
    want = rt.apply_batch_tensor(x, lengths=lens, planar=planar)
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))
    st = dec.last_compact_status()
    assert len(st) == 12 and all(s.flags == 0 and s.n_bad_rows == 0 for s in st)
    assert int(cursor.item()) == int(ent[:, 1].sum()) <= arena.numel() == g.compact_store_bound(2, lens)


@pytest.mark.gpu
def test_beyond_4_gib(gpu):
    """A real arena of 2^32 + 1 MiB bytes and a cursor just below 2^32: the blobs land there, and an offset cut to 32
    bits would land in the arena's first MiB, which must be untouched."""
    torch, g = gpu
    enc = ctx(g, "enc")
    MIB = 1 << 20
    size = (1 << 32) + MIB
    arena = torch.empty(size, dtype=torch.uint8, device="cuda")
    lo, hi = (1 << 32) - MIB // 2, (1 << 32) + MIB // 2
    head, mid = _pattern(MIB, seed=1), _pattern(MIB, seed=2)
    arena[:MIB] = torch.from_numpy(head).cuda()
    arena[lo:hi] = torch.from_numpy(mid).cuda()
    pool = clip_pool(g, torch, 2)
    pick = [pool[0], pool[1], pool[3], pool[4], pool[6]]
    cursor0 = (1 << 32) - 4096
    _, x, lens = padded(torch, [p[0] for p in pick], 2, True)
    cursor = torch.tensor([cursor0], dtype=torch.int64, device="cuda")
    _, _, ent = enc.encode_compact_batch_tensor(x, lengths=lens, arena=arena, cursor=cursor)
    torch.cuda.synchronize()
    entries, at = [], cursor0
    for _, bl in pick:
        hdr = np.frombuffer(bl[:64].tobytes(), np.uint64)
        entries.append((at, bl.size, int(hdr[2]), int(hdr[3]), 1))
        at += bl.size
    assert cursor0 < (1 << 32) < at < hi and entries[-1][0] > (1 << 32)
    assert np.array_equal(ent.cpu().numpy(), S.entry_rows(entries)) and int(cursor.item()) == at
    want = mid.copy()
    for (off, n, _, _, _), (_, bl) in zip(entries, pick):
        want[off - lo:off - lo + n] = bl
    assert np.array_equal(arena[lo:hi].cpu().numpy(), want)
    assert np.array_equal(arena[:MIB].cpu().numpy(), head)


@pytest.mark.gpu
def test_arguments_refused_before_anything_is_queued(gpu):
    torch, g = gpu
    enc = ctx(g, "enc")
    L = g._lib.GlcClipLayout
    pool = clip_pool(g, torch, 2)
    clips = [pool[4][0], pool[0][0]]                  # clip 1 is the longer one: a stride one short of it faults clip 1 alone
    big, x, lens = padded(torch, clips, 2, True)
    T = x.shape[2]
    assert lens[1] - 1 >= lens[0]
    image = _pattern(1 << 16, seed=3)
    arena = torch.from_numpy(image).cuda()
    cursor = torch.tensor([128], dtype=torch.int64, device="cuda")
    ent = torch.full((4, 4), -1, dtype=torch.int64, device="cuda")
    arr = (C.c_uint64 * 2)(*lens)
    lp = C.cast(arr, C.POINTER(C.c_uint64))
    good = L(2, 2, 1, x.stride(0), x.stride(1), T, lp)
    f = g.lib.glc_encode_batch_device_compact

    def call(lay=good, pcm=None, a=None, n=image.size, cu=None, e=None):
        vp = lambda v, d: C.c_void_p(d if v is None else v)
        return f(enc._h, vp(pcm, x.data_ptr()), C.byref(lay) if lay is not None else None, vp(a, arena.data_ptr()), n,
                 vp(cu, cursor.data_ptr()), vp(e, ent.data_ptr()))

    torch.cuda.synchronize()
    short = (C.c_uint64 * 2)(lens[0], 512)
    in_words = x.data_ptr()
    refused = {
        "null layout": lambda: call(lay=None),
        "null pcm": lambda: call(pcm=0),
        "null arena": lambda: call(a=0),
        "null cursor": lambda: call(cu=0),
        "null entries": lambda: call(e=0),
        "arena not 64-byte aligned": lambda: call(a=arena.data_ptr() + 32, n=image.size - 32),
        "cursor not 8-byte aligned": lambda: call(cu=cursor.data_ptr() + 4),
        "entries not 8-byte aligned": lambda: call(e=ent.data_ptr() + 4),
        "channels == 0": lambda: call(lay=L(2, 0, 1, x.stride(0), x.stride(1), T, lp)),
        "a clip the encoder refuses": lambda: call(lay=L(2, 2, 1, x.stride(0), x.stride(1), T, C.cast(short, C.POINTER(C.c_uint64)))),
        "channel_stride smaller than a plane": lambda: call(lay=L(2, 2, 1, x.stride(0), lens[1] - 1, T, lp)),
        "clip_stride smaller than the clip": lambda: call(lay=L(2, 2, 1, x.stride(1) + lens[1] - 1, x.stride(1), T, lp)),
        "the arena overlaps the input": lambda: call(a=(in_words + 4 * lens[0] + 63) // 64 * 64, n=64),
        "the entries overlap the input": lambda: call(e=in_words + 8),
    }
    for what, fn in refused.items():
        assert fn() == EINVAL, what
        msg = g.lib.glc_last_error(enc._h).decode()
        assert "glc_encode_batch_device_compact" in msg, (what, msg)
        if what in ("a clip the encoder refuses", "channel_stride smaller than a plane", "clip_stride smaller than the clip"):
            assert "clip 1" in msg, (what, msg)
    assert f(None, None, None, None, 0, None, None) == EINVAL
    # the A1-A3 hook holds the same four pointers to the same alignments: the arena to 64 bytes (32 is not enough), the
    # records, the cursor and the entries to 8
    one_each = (C.c_uint64 * 2)(1, 1)
    hook = lambda rec=0, a=0, cu=0, e=0: g.lib.glc_debug_compact_store_device(
        enc._h, x.data_ptr() + rec, one_each, 2, 2, arena.data_ptr() + a, image.size - a, cursor.data_ptr() + cu, ent.data_ptr() + e)
    for what, fn in {"arena": lambda: hook(a=32), "records": lambda: hook(rec=4), "cursor": lambda: hook(cu=4),
                     "entries": lambda: hook(e=4)}.items():
        assert fn() == EINVAL, what
        msg = g.lib.glc_last_error(enc._h).decode()
        assert "glc_debug_compact_store_device" in msg and "aligned" in msg, (what, msg)
    # nothing was queued: the arena, the cursor and the entries are what they were
    enc.synchronize()
    assert np.array_equal(arena.cpu().numpy(), image) and int(cursor.item()) == 128 and bool((ent == -1).all())
    # n_clips == 0 is fine and leaves the cursor alone, whatever the other arguments
    assert call(lay=L(0, 2, 1, 0, 0, 0, None)) == 0 and f(enc._h, None, C.byref(L(0, 2, 1, 0, 0, 0, None)), None, 0, None, None) == 0
    enc.synchronize()
    assert int(cursor.item()) == 128 and np.array_equal(arena.cpu().numpy(), image)
    assert g.compact_store_bound(2, lens) == sum(g.compact_bound(2, RC.frames_of(n)) for n in lens)
    assert g.compact_store_bound(2, [512]) == 0 and g.compact_store_bound(2, []) == 0


@pytest.mark.gpu
def test_context_state_afterwards(gpu):
    """No stream is resident, an open decode session is closed, and an encode that follows is what it always was."""
    torch, g = gpu
    dec = ctx(g, "dec", 2)
    pool = clip_pool(g, torch, 2)
    x = pool[4][0]
    stream = ctx(g, "enc").encode(x, 2)
    before = dec.decode(stream).copy()
    assert g.lib.glc_ctx_resident_stream(dec._h) != 0
    _, xs, lens = padded(torch, [pool[0][0], pool[1][0]], 2, True)
    arena, cursor, ent = g.Encoder.encode_compact_batch_tensor(dec, xs, lengths=lens)      # the C call on a context with a resident stream
    torch.cuda.synchronize()
    assert g.lib.glc_ctx_resident_stream(dec._h) == 0
    blobs = g.store_blobs(arena, ent)
    assert [b.cpu().numpy().tobytes() for b in blobs] == [pool[0][1].tobytes(), pool[1][1].tobytes()]
    assert np.array_equal(bits(dec.decode(stream)), bits(before))
    assert ctx(g, "enc").encode(x, 2).to_bytes() == stream.to_bytes()
