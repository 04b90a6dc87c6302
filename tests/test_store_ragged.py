"""Ragged crops drawn from the compact store: glc_decode_ragged_crops_device_store and its _i16 twin, the ragged form of
the draw planner behind them (k_store_plan_crops<true> through glc_debug_store_plan_ragged_device) and
Decoder.decode_store_ragged_crops_tensor (DESIGN.md sections 3 and 4).

Every sample comparison is bit for bit - float32 viewed as int32, int16 as it is - on every element of the output
tensor, a margin of a pattern nothing computes (a NaN payload, 0x7ABC for int16) around the slice written included.
The valid part of a usable crop is what Decoder.decode_compact_crops_tensor (glc_decode_crops_device_compact) writes for
{start, v} with v resolved on the host AFTER the draw; the padding behind it and every unusable crop are +0.0 / 0 (as
bits: -0.0 fails); `valid` and every status word are compared.  The models are store_ragged_cases', written from the
contract.  Damaged blobs are the existing ones of crop_cases / compact_decode_cases (every count inside its buffer):
the tests pin the defined result, they provoke nothing."""
import ctypes as C

import numpy as np
import pytest

import compact_decode_cases as K
import crop_cases as CC
import roundtrip_cases as RC
import store_draw_cases as S
import store_ragged_cases as R
from crop_cases import NAN_BITS

pytestmark = pytest.mark.gpu

HOP = K.HOP
F32 = np.float32
EINVAL = -1
SR = 44100
SENT16, SENT64 = 0x7ABC, -7777               # what int16 outputs and `valid` hold where nothing may be written
FAKE_ARENA, FAKE_OUT = 1 << 44, 1 << 52      # numbers the planner hook never dereferences
POOL = (513, 1024, 1025, 1536, 2049, 3000)   # tonal clips, samples per channel; one noise clip (raw frames) of 2500 follows


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    assert hasattr(g.lib, "glc_decode_ragged_crops_device_store")
    yield g
    _ctx.clear()             # contexts: released while the library is still loaded
    _cache.clear()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


_ctx = {}
_cache = {}


def ctx(g, kind, ch=2):
    key = (kind, ch)
    if key not in _ctx:
        _ctx[key] = g.Encoder(SR) if kind == "enc" else g.Decoder(ch, SR)
    return _ctx[key]


def pattern(torch, shape, dtype):
    if dtype == torch.int16:
        return torch.full(shape, SENT16, dtype=torch.int16, device="cuda")
    return torch.from_numpy(np.full(shape, NAN_BITS, np.uint32).view(F32)).cuda()


def as_bits(torch, t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def i64(torch, values):
    return torch.tensor(list(values), dtype=torch.int64).reshape(-1).cuda()


class Store:
    """A store as a caller holds it: everything on the device, plus what the TEST knows about it on the host."""

    def __init__(self, torch, ch, arena, entries, lengths):
        self.ch, self.arena, self.entries = ch, arena, entries
        self.host_lengths = [int(v) for v in lengths]
        self.lengths = i64(torch, self.host_lengths)
        self.max_length = max(self.host_lengths)
        self.host_entries = entries.cpu().tolist()


def pool(g, torch, ch):
    """The store of the pool, encoded in one call: six tonal clips of 513 to 3000 samples and one of noise."""
    key = ("pool", ch)
    if key not in _cache:
        clips = [RC.chord(SR, ch, n, seed=n % 13) for n in POOL] + [RC.lcg_noise(2500 * ch, seed=5)]
        lens = [c.size // ch for c in clips]
        x = np.full((len(clips), ch, max(lens)), NAN_BITS, np.uint32).view(F32)
        for i, c in enumerate(clips):
            x[i, :, :lens[i]] = np.ascontiguousarray(c, F32).reshape(-1, ch).T
        arena, _, entries = ctx(g, "enc").encode_compact_batch_tensor(torch.from_numpy(x).cuda(), lengths=lens, planar=True)
        _cache[key] = Store(torch, ch, arena, entries, lens)
    return _cache[key]


def host_store(torch, ch, blobs):
    """blobs: [(uint8 array, capacity the entry names, samples per channel)] back to back in an arena the host builds"""
    off, entries, parts = 0, [], []
    for buf, cap, _ in blobs:
        buf = np.ascontiguousarray(buf, np.uint8)
        entries.append(S.entry(off, cap))
        parts.append(buf)
        pad = (-buf.size) % 64
        if pad:
            parts.append(np.zeros(pad, np.uint8))
        off += buf.size + pad
    arena = torch.from_numpy(np.concatenate(parts)).cuda()
    assert arena.data_ptr() % 64 == 0
    return Store(torch, ch, arena, torch.tensor(entries, dtype=torch.int64).cuda(), [b[2] for b in blobs])


def status_words(st):
    return [(s.flags, s.n_bad_rows, s.first_bad_row) for s in st]


def clean(words):
    return all(w == (0, 0, 0) for w in words)


def check_ragged(g, torch, store, clips, starts, wants, length, planar=True, margin=0, dtype=None, dec=None, max_length=None,
                 stream=None):
    """One ragged draw into the leading slice of a pattern tensor - on `stream` when given, with the selection made on that
    stream and nothing synchronised in front of the call - then, and only then, the selection is resolved on the host.
    Every element of the tensor, every `valid` (and the words around them) and every status word is held to the contract.
    wants: None (d_want == NULL), or one wanted length per crop.  -> (status words, verdicts, valid lengths)."""
    ch = store.ch
    dtype = dtype or torch.float32
    dec = dec or ctx(g, "ragged", ch)
    b = len(clips)
    shape = (b + margin, ch + margin, length + 3 * margin) if planar else (b + margin, length + margin, ch)
    ml = store.max_length if max_length is None else max_length
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        big = pattern(torch, shape, dtype)
        out = big[:b, :ch, margin:margin + length] if planar else big[:b, :length, :]
        valid_big = torch.full((b + 2,), SENT64, dtype=torch.int64, device="cuda")
        clips_t, starts_t = i64(torch, clips) + 0, i64(torch, starts) + 0          # (the additions run on this stream)
        want_t = None if wants is None else i64(torch, wants) + 0
        got, valid = dec.decode_store_ragged_crops_tensor(store.arena, store.entries, store.lengths, clips_t, starts_t, length, ml,
                                                          want=want_t, planar=planar, out=out, valid=valid_big[1:b + 1])
    assert got is out and valid.data_ptr() == valid_big.data_ptr() + 8
    assert g.lib.glc_ctx_resident_stream(dec._h) == 0
    if stream is not None:
        stream.synchronize()
    # ---- the host enters here
    entries, lens = store.host_entries, store.host_lengths
    wl = [None] * b if wants is None else wants
    verdicts = [R.verdict_of(entries, lens, store.arena.numel(), ml, c, s, w, length) for c, s, w in zip(clips, starts, wl)]
    good = [i for i, v in enumerate(verdicts) if not v]
    valids = [0 if verdicts[i] else R.valid_of(lens[clips[i]], starts[i], wl[i], length) for i in range(b)]
    want = pattern(torch, shape, dtype)
    view = want[:b, :ch, margin:margin + length] if planar else want[:b, :length, :]
    view[:] = 0                                                   # +0.0 / 0: unusable crops, and the padding of the others
    want_st = [(v | S.BAD_HEADER, 0, 0) for v in verdicts]
    if good:
        pdec = ctx(g, "pointer", ch)
        blobs = [store.arena[entries[clips[i]][0]:entries[clips[i]][0] + entries[clips[i]][1]] for i in good]
        ref = torch.zeros((len(good), ch, length) if planar else (len(good), length, ch), dtype=dtype, device="cuda")
        pdec.decode_compact_crops_tensor(blobs, [lens[clips[i]] * ch for i in good], [starts[i] for i in good], [valids[i] for i in good],
                                         planar=planar, out=ref)
        view[torch.tensor(good).cuda()] = ref
        for i, s in zip(good, status_words(pdec.last_compact_status())):
            want_st[i] = s
    torch.cuda.synchronize()
    same = as_bits(torch, big) == as_bits(torch, want)
    if not bool(same.all()):
        rows = sorted({int(i) for i in torch.nonzero(~same)[:, 0].cpu().tolist()})
        raise AssertionError(f"crops {rows[:8]} differ: {[(clips[i], starts[i], wl[i], length) for i in rows[:8] if i < b]}")
    assert valid_big.cpu().tolist() == [SENT64] + valids + [SENT64]
    st = status_words(dec.last_compact_status())
    assert st == want_st
    return st, verdicts, valids


# ------------------------------------------------------------------------------------------ 1: the planner against its model

HOOK_ARGS = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
             C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def plan_hook(g, dec, arena, arena_bytes, entries_t, lengths_t, max_length, clips_t, starts_t, want_t, length, lay):
    f = g.lib.glc_debug_store_plan_ragged_device
    f.restype, f.argtypes = C.c_int, HOOK_ARGS
    n = clips_t.shape[0]
    max_descs = g.store_ragged_slots(length, lay.channels)[0]
    dirs, descs = np.zeros(n, S.DIR_DTYPE), np.zeros(n * max_descs, S.DESC_DTYPE)
    verdicts, valids = np.zeros(n, np.uint32), np.full(n, SENT64, np.int64)
    rc = f(dec._h, arena, arena_bytes, entries_t.data_ptr(), lengths_t.data_ptr(), entries_t.shape[0], max_length,
           clips_t.data_ptr(), starts_t.data_ptr(), None if want_t is None else want_t.data_ptr(), length, FAKE_OUT, C.addressof(lay),
           dirs.ctypes.data, descs.ctypes.data, verdicts.ctypes.data, valids.ctypes.data)
    assert rc == 0, g.lib.glc_last_error(dec._h)
    return dirs.tolist(), descs.reshape(n, max_descs).tolist(), verdicts.tolist(), valids.tolist()


def check_plan(g, torch, ch, entries, lengths, max_length, sels, length, arena_bytes=1 << 40, no_want=False):
    """sels: (clip, start, want).  The hook against the model, planar and interleaved.  -> (verdicts, valids)"""
    L = g._lib
    dec = ctx(g, "ragged", ch)
    entries_t = torch.tensor(entries, dtype=torch.int64).cuda()
    lengths_t = i64(torch, lengths)
    clips, starts, wants = ([s[k] for s in sels] for k in range(3))
    clips_t, starts_t, want_t = i64(torch, clips), i64(torch, starts), None if no_want else i64(torch, wants)
    n = len(sels)
    max_descs = g.store_ragged_slots(length, ch)[0]
    want = None
    for planar in (True, False):
        chs = length + 3 if planar else 0
        cs = ch * (length + 3) + 5 if planar else length * ch + 7
        lay = L.GlcClipLayout(n, ch, 1 if planar else 0, cs, chs, length, None)
        got = plan_hook(g, dec, FAKE_ARENA, arena_bytes, entries_t, lengths_t, max_length, clips_t, starts_t, want_t, length, lay)
        want = R.plan_model(g, max_descs, FAKE_ARENA, arena_bytes, entries, lengths, max_length, clips, starts, None if no_want else wants,
                            length, ch, planar, cs, chs)
        for what, a, b in zip(("directory", "descriptors", "verdicts", "valid"), got, want):
            for i, (x, y) in enumerate(zip(a, b)):
                assert x == y or [tuple(r) for r in x] == y, (what, "crop", i, sels[i], x, y)
    return want[2], want[3]


@pytest.mark.parametrize("ch", (1, 2, 3, 6))
def test_planner_equals_the_model_at_every_hop_boundary(glc_amd, torch, ch):
    """Clips shorter than, as long as and longer than the row; starts on both sides of every hop boundary and at n - 1;
    valid parts that end on both sides of every hop boundary."""
    g = glc_amd
    lengths = [513, 1024, 1536, 2049, 3000]
    entries = [S.entry(64 * 1000 * i, 64 * (100 + i)) for i in range(len(lengths))]
    full = 0
    for length in (1, 2, 1024, 1536, 2500):
        sels = [(e, s, w) for e in reversed(range(len(lengths))) for s, w in R.boundary_selections(lengths[e], ch, length)]
        assert all((e, lengths[e] - 1, length) in sels and (e, 0, 1) in sels for e in range(len(lengths)))
        verdicts, valids = check_plan(g, torch, ch, entries, lengths, 3000, sels, length)
        assert not any(verdicts) and min(valids) == 1 and max(valids) == min(length, 3000)
        assert length == 1 or any(v < w for v, (_, _, w) in zip(valids, sels))       # the clip's end cut a wanted length
        max_descs = g.store_ragged_slots(length, ch)[0]
        for (e, s, _), v in zip(sels, valids):
            full += R.descs_needed(g.plan_crop(lengths[e] * ch, ch, s, v).n_hops, v, length, ch) == max_descs
        # d_want == NULL: every crop wants the row
        v2, valids2 = check_plan(g, torch, ch, entries, lengths, 3000, sels[::3], length, no_want=True)
        assert not any(v2) and valids2 == [min(length, lengths[e] - s) for e, s, _ in sels[::3]]
    assert full > 0                          # some crop used every descriptor of its slot


def test_planner_verdicts(glc_amd, torch):
    g = glc_amd
    ab, ml, length = 1 << 40, 40000, 100
    table = [                                                   # (entry, stored length, what the planner must say)
        (S.entry(0, 4096), 5000, 0),
        (S.entry((1 << 32) + 64, 8192), 1536, 0),               # an offset beyond 2^32
        (S.entry(ab - 4096, 4096), 2049, 0),                    # offset + bytes exactly arena_bytes
        (S.entry(ab - 4096, 4097), 2049, S.NO_BLOB),            # ... one byte over: a range outside the arena
        (S.entry((1 << 64) - 64, 4096), 2049, S.NO_BLOB),       # the sum wraps
        (S.entry(96, 4096), 2049, S.NO_BLOB),                   # a misaligned offset
        (S.entry(128, 4096, stored=0), 2049, S.NO_BLOB),
        (S.entry(0, 4096), 512, S.BAD_CROP),                    # a length the encoder refuses
        (S.entry(0, 4096), 0, S.BAD_CROP),
        (S.entry(0, 4096), -5, S.BAD_CROP),
        (S.entry(0, 4096), ml, 0),
        (S.entry(0, 4096), ml + 1, S.BAD_CROP),
        (S.entry(0, 4096), (1 << 63) - 1, S.BAD_CROP),
    ]
    entries, lengths = [t[0] for t in table], [t[1] for t in table]
    n_e = len(table)
    sels = [(e, 0, length) for e in range(n_e)] + [(e, max(0, lengths[e] - 1), 7) for e in range(n_e)]
    expect = [t[2] for t in table] * 2
    extra = [  # (clip, start, want) -> verdict
        ((0, 0, 1), 0), ((0, 0, length), 0), ((0, 0, 0), S.BAD_CROP), ((0, 0, length + 1), S.BAD_CROP), ((0, 0, -1), S.BAD_CROP),
        ((0, 0, -(1 << 63)), S.BAD_CROP), ((0, 0, (1 << 63) - 1), S.BAD_CROP),
        ((0, 4999, length), 0), ((0, 5000, length), S.BAD_CROP), ((0, 5001, 1), S.BAD_CROP), ((0, -1, 1), S.BAD_CROP),
        ((0, (1 << 63) - 1, 1), S.BAD_CROP), ((0, -(1 << 63), 1), S.BAD_CROP),
        ((-1, 0, 1), S.BAD_CROP), ((n_e, 0, 1), S.BAD_CROP), ((1 << 62, 0, 1), S.BAD_CROP), ((-(1 << 63), 0, 1), S.BAD_CROP),
        ((6, -1, 1), S.BAD_CROP), ((6, 0, 0), S.BAD_CROP), ((6, 0, 1), S.NO_BLOB),        # BAD_CROP wins over an unusable entry
        ((0, 4950, length), 0),
    ]
    verdicts, valids = check_plan(g, torch, 2, entries, lengths, ml, sels + [x[0] for x in extra], length, arena_bytes=ab)
    assert verdicts == expect + [x[1] for x in extra]
    assert valids[len(sels) + 7] == 1 and valids[-1] == 50 and valids[len(sels) + 1] == length
    # max_length below the row: every clip is short
    verdicts, valids = check_plan(g, torch, 2, [S.entry(0, 4096)] * 2, [600, 601], 600, [(0, 0, 5000), (1, 0, 5000), (0, 599, 4000)], 5000)
    assert verdicts == [0, S.BAD_CROP, 0] and valids == [600, 0, 1]


def test_planner_over_two_rounds(glc_amd, torch):
    g = glc_amd
    length = 600
    assert S.slots(length, 1) == (2, 3) and S.per_round(length, 1) == 1024 and g.store_ragged_slots(length, 1) == (3, 3)
    lengths = [513, 700, 3000]
    entries = [S.entry(64 * 1000 * i, 64 * (100 + i)) for i in range(3)]
    rng = np.random.RandomState(3)
    sels = []
    for _ in range(1025):                                        # per_round + 1 crops
        e = int(rng.randint(3))
        sels.append((e, int(rng.randint(lengths[e])), int(rng.randint(1, length + 1))))
    sels[1023], sels[1024] = (2, 2999, length), (0, 511, 2)       # the last crop of a round and the first of the next
    verdicts, valids = check_plan(g, torch, 1, entries, lengths, 3000, sels, length)
    assert not any(verdicts) and valids[1023:] == [1, 2]


# ------------------------------------------------------------------------------------------ 2: the draw

def mixed_selections(store, length, rng, per_clip=10):
    """Usable selections at the edges of every clip and a few in the middle, with unusable ones in between."""
    ch, sels = store.ch, []
    for e, n in enumerate(store.host_lengths):
        edge = R.boundary_selections(n, ch, length)
        take = [edge[int(k)] for k in rng.choice(len(edge), min(per_clip, len(edge)), replace=False)]
        take += [(n - 1, length), (0, length), (0, 1), (max(0, n - length), length)]
        sels += [(e, s, w) for s, w in take]
    n_e = len(store.host_lengths)
    bad = [(0, store.host_lengths[0], 1), (1, -1, 1), (2, 0, 0), (3, 0, length + 1), (4, 0, -3), (-1, 0, 1), (n_e, 0, 1)]
    for k, x in enumerate(bad):
        sels.insert(3 + 5 * k, x)
    return sels


@pytest.mark.parametrize("ch", (1, 2, 3, 6))
@pytest.mark.parametrize("planar,margin", ((True, 0), (False, 2), (True, 2)), ids=("planar", "interleaved-slice", "planar-slice"))
def test_ragged_draw_float_and_int16(glc_amd, torch, ch, planar, margin):
    """A row longer than three of the clips, as long as none: valid parts cut by the clip's end, by the wanted length and
    by neither, unusable selections between them - as float32 and as int16."""
    g = glc_amd
    store = pool(g, torch, ch)
    length = 1200
    sels = mixed_selections(store, length, np.random.RandomState(ch))
    for dtype in (torch.float32, torch.int16):
        st, verdicts, valids = check_ragged(g, torch, store, *([s[k] for s in sels] for k in range(3)), length, planar=planar,
                                            margin=margin, dtype=dtype)
        assert verdicts.count(S.BAD_CROP) == 7 and verdicts.count(0) == len(sels) - 7
        assert clean([w for w, v in zip(st, verdicts) if not v])
        assert any(0 < v < w for v, (_, _, w) in zip(valids, sels)) and length in valids and 1 in valids


@pytest.mark.parametrize("ch", (2, 3))
def test_rows_of_one_hop_and_of_one_sample(glc_amd, torch, ch):
    """length 1024: every usable crop's slot has one descriptor more than the fixed draw's; length 1 and 2: no padding
    or one sample of it."""
    g = glc_amd
    store = pool(g, torch, ch)
    for k, length in enumerate((1024, 1, 2)):
        assert g.store_ragged_slots(1024, ch)[0] == S.slots(1024, ch)[0] + 1
        sels = mixed_selections(store, length, np.random.RandomState(10 + k), per_clip=6)
        st, verdicts, valids = check_ragged(g, torch, store, *([s[k2] for s in sels] for k2 in range(3)), length, planar=bool(k % 2),
                                            margin=1, dtype=torch.int16 if k == 1 else torch.float32)
        assert verdicts.count(0) >= len(sels) - 7


def test_every_clip_is_shorter_than_the_row(glc_amd, torch):
    """max_length < length is legal here: a row of 4000 samples from clips of at most 3000."""
    g = glc_amd
    store = pool(g, torch, 2)
    length = 4000
    assert store.max_length < length
    n_e = len(store.host_lengths)
    sels = [(e, s, length) for e in range(n_e) for s in (0, 100, store.host_lengths[e] - 1)]
    for planar in (True, False):
        st, verdicts, valids = check_ragged(g, torch, store, *([s[k] for s in sels] for k in range(3)), length, planar=planar, margin=1)
        assert not any(verdicts) and clean(st)
        assert valids == [store.host_lengths[e] - s for e, s, _ in sels] and max(valids) == 3000
    # ... and with a max_length below some of the clips: those are unusable, the others as before
    st, verdicts, _ = check_ragged(g, torch, store, *([s[k] for s in sels] for k in range(3)), length, max_length=2049)
    assert [v for v in verdicts[::3]] == [0 if n <= 2049 else S.BAD_CROP for n in store.host_lengths]


@pytest.mark.parametrize("dtype", ("float32", "int16"))
def test_without_wanted_lengths_inside_the_clips_it_is_the_fixed_draw(glc_amd, torch, dtype):
    """want=None and every crop inside its clip: bit for bit decode_store_crops_tensor, statuses included."""
    g = glc_amd
    dtype = getattr(torch, dtype)
    store = pool(g, torch, 2)
    length = 500
    rng = np.random.RandomState(8)
    clips = [int(k) for k in rng.randint(0, len(store.host_lengths), 60)]
    starts = [int(rng.randint(0, store.host_lengths[e] - length + 1)) for e in clips]
    starts[:3] = [store.host_lengths[e] - length for e in clips[:3]]
    for planar in (True, False):
        st, verdicts, valids = check_ragged(g, torch, store, clips, starts, None, length, planar=planar, dtype=dtype)
        assert not any(verdicts) and valids == [length] * 60
        dec = ctx(g, "ragged", 2)
        a, valid = dec.decode_store_ragged_crops_tensor(store.arena, store.entries, store.lengths, i64(torch, clips), i64(torch, starts),
                                                        length, store.max_length, planar=planar, dtype=dtype)
        st_a = status_words(dec.last_compact_status())
        b = dec.decode_store_crops_tensor(store.arena, store.entries, store.lengths, i64(torch, clips), i64(torch, starts), length,
                                          store.max_length, planar=planar, dtype=dtype)
        torch.cuda.synchronize()
        assert a.dtype == b.dtype == dtype and a.shape == b.shape and torch.equal(as_bits(torch, a), as_bits(torch, b))
        assert valid.dtype == torch.int64 and valid.cpu().tolist() == [length] * 60
        assert st_a == status_words(dec.last_compact_status()) == st


def test_one_clip_drawn_many_times(glc_amd, torch):
    g = glc_amd
    store = pool(g, torch, 3)
    length, e = 900, 2                                           # the clip of 1025 samples
    n = store.host_lengths[e]
    rng = np.random.RandomState(21)
    sels = [(e, int(rng.randint(n)), int(rng.randint(1, length + 1))) for _ in range(150)] + [(e, 0, length)] * 20 + [(e, n - 1, 5)] * 20
    st, verdicts, valids = check_ragged(g, torch, store, *([s[k] for s in sels] for k in range(3)), length, planar=False)
    assert not any(verdicts) and clean(st) and len(set(valids)) > 50


def test_two_rounds(glc_amd, torch):
    g = glc_amd
    store = pool(g, torch, 1)
    length = 600
    assert S.per_round(length, 1) == 1024
    rng = np.random.RandomState(7)
    n_e = len(store.host_lengths)
    sels = []
    for _ in range(1030):
        e = int(rng.randint(n_e))
        sels.append((e, int(rng.randint(store.host_lengths[e])), int(rng.randint(1, length + 1))))
    sels[1023], sels[1024], sels[5] = (5, 2999, length), (0, 512, length), (n_e, 0, 1)
    dec = g.Decoder(1, SR)
    st, verdicts, valids = check_ragged(g, torch, store, *([s[k] for s in sels] for k in range(3)), length, dec=dec)
    assert verdicts.count(S.BAD_CROP) == 1 and valids[1023:1025] == [1, 1]
    # a second, smaller call on the same context: workspaces reused, one status and one valid length per crop of THAT call
    st, _, valids = check_ragged(g, torch, store, [5, 0], [2500, 0], [length, 3], length, dec=dec, dtype=torch.int16)
    assert len(st) == 2 and clean(st) and valids == [500, 3]
    dec.close()


def test_damaged_blobs_in_an_arena(glc_amd, torch):
    """The crafted streams and the damaged blobs of crop_cases in one arena: samples and status words of the valid parts
    are the pointer call's (check_ragged compares both)."""
    g = glc_amd
    base = CC.stereo_stream()
    n_true = sum(len(r.idx) for _, body in base for r in body)
    o_pairs = K.layout(2, len(base))[3]
    crafted = [c for c in CC.crafted() if c[1] == 2]
    blobs = [(buf[:nbytes], nbytes, len(frames) * HOP) for (buf, nbytes), (_, _, frames) in zip([K.pack(2, c[2]) for c in crafted], crafted)]
    n_crafted = len(blobs)
    damaged = [dict(magic=K.MAGIC ^ 0x100), dict(cnt_set={1: HOP}), dict(n_pairs=n_true + 1, bytes_field=K.align64(o_pairs + 4 * (n_true + 1)))]
    for over in damaged:
        buf, _ = K.pack(2, base, **over)
        blobs.append((buf, buf.size, len(base) * HOP))            # the entry names the whole buffer, as the pointer tests do
    for row in (7, 4, 3, 10):
        buf, _ = K.pack(2, CC.with_bad_list(base, row))
        blobs.append((buf, buf.size, len(base) * HOP))
    store = host_store(torch, 2, blobs)
    start = CC.first_sample_of_hop(3, 2)
    want = CC.first_sample_of_hop(5, 2) - start                   # frames 2 .. 4
    length = want + 700
    sels = [(e, s, w) for e in range(len(blobs)) for s, w in ((start, want), (0, 300), (store.host_lengths[e] - 200, length))]
    st, verdicts, valids = check_ragged(g, torch, store, *([s[k] for s in sels] for k in range(3)), length, planar=False, margin=1)
    assert not any(verdicts) and valids[:3] == [want, 300, 200]
    of = lambda e: st[3 * e]                                      # the crop of frames 2 .. 4 of entry e
    assert all(clean(st[3 * e:3 * e + 3]) for e in range(n_crafted))
    assert of(n_crafted) == (K.BAD_HEADER, 3 * 2, 2 * 2)          # bad magic: the window's rows
    assert of(n_crafted + 1) == (K.ROW_BOUNDS, 6, 4)              # an inflated cnt in front of the window
    assert of(n_crafted + 2) == (0, 0, 0)                         # the pair sum is not a crop's business
    assert [of(n_crafted + 3 + k) for k in range(4)] == [(K.NOT_CANONICAL, 1, 7), (K.NOT_CANONICAL, 1, 4), (0, 0, 0), (0, 0, 0)]


def test_on_another_stream_with_nothing_synchronised_in_front(glc_amd, torch):
    g = glc_amd
    store = pool(g, torch, 2)
    torch.cuda.synchronize()
    length = 1100
    sels = mixed_selections(store, length, np.random.RandomState(33), per_clip=4)
    side = torch.cuda.Stream()
    for planar in (True, False):
        st, verdicts, _ = check_ragged(g, torch, store, *([s[k] for s in sels] for k in range(3)), length, planar=planar, margin=1,
                                       stream=side)
        assert verdicts.count(0) == len(sels) - 7


def test_context_state_afterwards(glc_amd, torch):
    """No stream is resident afterwards and an open decode session is closed; a glc_decode that follows is what it always
    was; the pointer call and the ragged draw alternate on one context."""
    g = glc_amd
    dec = g.Decoder(2, SR)
    x = RC.chord(SR, 2, 4 * HOP + 100)
    stream = ctx(g, "enc").encode(x, 2)
    before = dec.decode(stream).copy()
    assert g.lib.glc_ctx_resident_stream(dec._h) != 0
    store = pool(g, torch, 2)
    st, _, _ = check_ragged(g, torch, store, [3, 4, 0], [0, 2000, 500], [700, 700, 700], 700, dec=dec)
    assert g.lib.glc_ctx_resident_stream(dec._h) == 0 and clean(st)
    assert np.array_equal(CC.bits(dec.decode(stream)), CC.bits(before))
    e = store.host_entries
    for _ in range(2):
        ref = pattern(torch, (2, 2, 500), torch.float32)
        dec.decode_compact_crops_tensor([store.arena[e[k][0]:e[k][0] + e[k][1]] for k in (3, 4)],
                                        [store.host_lengths[k] * 2 for k in (3, 4)], [5, 6], 500, out=ref)
        st, _, _ = check_ragged(g, torch, store, [3, 4], [5, 2040], [500, 500], 500, dec=dec)
        assert clean(st)
    assert g.lib.glc_decode_stream_begin(dec._h, stream._h) == 0
    check_ragged(g, torch, store, [3], [0], [9], 500, dec=dec)
    out, last, buf = C.c_uint64(), C.c_int(), np.empty(16, F32)
    assert g.lib.glc_decode_stream_next(dec._h, buf.ctypes.data, 16, C.byref(out), C.byref(last)) == EINVAL
    dec.close()


# ------------------------------------------------------------------------------------------ 3: the call's edges

def test_arguments_refused_before_anything_is_queued(glc_amd, torch):
    g = glc_amd
    L = g._lib
    dec = g.Decoder(2, SR)
    store = pool(g, torch, 2)
    length, ml, n_e = 600, store.max_length, len(store.host_lengths)
    clips_t, starts_t, want_t = i64(torch, [3, 4]), i64(torch, [10, 2000]), i64(torch, [600, 600])
    out = pattern(torch, (2, 600, 2), torch.float32)
    valid_t = torch.full((4,), SENT64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    A, E, Ln = store.arena.data_ptr(), store.entries.data_ptr(), store.lengths.data_ptr()
    Cl, St, W, V, o = clips_t.data_ptr(), starts_t.data_ptr(), want_t.data_ptr(), valid_t.data_ptr() + 8, out.data_ptr()

    def lay(n_clips=2, ch=2, planar=0, cs=1200, chs=0, lengths=None, one=600):
        return L.GlcClipLayout(n_clips, ch, planar, cs, chs, one, C.cast(lengths, C.POINTER(C.c_uint64)) if lengths is not None else None)

    def call(arena=A, ab=None, entries=E, lengths=Ln, n=n_e, max_length=ml, clips=Cl, starts=St, want=W, length=length, d_out=o,
             layout=None, valid=V, f=g.lib.glc_decode_ragged_crops_device_store):
        layout = layout or lay()
        return f(dec._h, arena, store.arena.numel() if ab is None else ab, entries, lengths, n, max_length, clips, starts, want, length,
                 d_out, C.byref(layout), valid)

    big_frames = (1 << 41) + 1024                                # 2^31 + 1 stereo frames: more than 32 bits of rows
    refused = [
        # what the fixed draw refuses ...
        call(arena=None), call(entries=None), call(lengths=None), call(clips=None), call(starts=None), call(d_out=None),
        g.lib.glc_decode_ragged_crops_device_store(dec._h, A, 64, E, Ln, n_e, ml, Cl, St, W, length, o, None, V),
        call(layout=lay(ch=0)),
        call(arena=A + 32),                                       # the arena is not 64-byte aligned
        call(entries=E + 4), call(lengths=Ln + 4), call(clips=Cl + 4), call(starts=St + 4),
        call(d_out=o + 2),
        call(length=0, layout=lay(one=0)),
        call(max_length=512),                                     # a max_length the encoder refuses
        call(max_length=0),
        call(max_length=big_frames),                              # ... whose rows exceed 32 bits
        call(max_length=1 << 62),
        call(length=1 << 62, layout=lay(n_clips=1, one=1 << 62)),     # length * channels wraps
        call(layout=lay(lengths=(C.c_uint64 * 2)(600, 599))),     # lengths given and not all `length`
        call(layout=lay(one=599)),
        call(layout=lay(cs=1199)),                                # a clip overlaps the next
        call(layout=lay(planar=1, cs=1200, chs=599)),             # a plane overlaps the next
        call(n=0),
        call(length=4095 * HOP + 2, max_length=1 << 23, layout=lay(n_clips=1, one=4095 * HOP + 2)),     # max_frames + 1 > 4097
        call(d_out=A + 64),                                       # the output overlaps the arena
        call(d_out=E - 4 * 1199 + 8, layout=lay(n_clips=1)),      # ... the entries
        call(d_out=Ln), call(d_out=Cl), call(d_out=St - 4 * 2399),
        # ... and what is new
        call(want=W + 4), call(valid=V + 4),                      # not 8-byte aligned
        call(d_out=W), call(d_out=W - 4 * 2399),                  # want overlaps the output extent
        call(d_out=V), call(valid=o + 8), call(valid=o + 4 * 2392),       # valid overlaps it
        call(valid=A + 64), call(valid=A + store.arena.numel() - 8),      # valid overlaps the arena
        call(valid=E + 8), call(valid=Ln), call(valid=Cl), call(valid=St + 8), call(valid=W), call(valid=W + 8),
        call(f=g.lib.glc_decode_ragged_crops_device_store_i16, d_out=o + 1),
        call(f=g.lib.glc_decode_ragged_crops_device_store_i16, valid=o + 8),
    ]
    assert refused == [EINVAL] * len(refused)
    # the planner hook checks what the call checks
    hook = g.lib.glc_debug_store_plan_ragged_device
    hook.restype, hook.argtypes = C.c_int, HOOK_ARGS
    plan = np.zeros(4096, np.uint8)
    for arena_at, want_at, layout, what in ((A, W, lay(cs=1199), b"clip_stride"), (A + 32, W, lay(), b"64-byte"), (A, W + 4, lay(), b"want")):
        assert hook(dec._h, arena_at, store.arena.numel(), E, Ln, n_e, ml, Cl, St, want_at, length, o, C.addressof(layout), plan.ctypes.data,
                    plan.ctypes.data, plan.ctypes.data, plan.ctypes.data) == EINVAL
        assert b"glc_debug_store_plan_ragged_device" in g.lib.glc_last_error(dec._h) and what in g.lib.glc_last_error(dec._h)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy().view(np.uint32) == NAN_BITS)                  # nothing was written by a refused call
    assert valid_t.cpu().tolist() == [SENT64] * 4
    assert g.lib.glc_decode_compact_last_status(dec._h, (L.GlcCompactStatus * 2)(), 2) == EINVAL      # nothing has completed
    # no clips: nothing to do, whatever else is passed
    assert g.lib.glc_decode_ragged_crops_device_store(dec._h, None, 0, None, None, 0, 0, None, None, None, 0, None,
                                                      C.byref(lay(n_clips=0)), None) == 0
    # ... and the accepted forms: one length for all or a lengths array, with and without want and valid
    lens2 = (C.c_uint64 * 2)(600, 600)
    e, hl = store.host_entries, store.host_lengths
    ref = torch.zeros((2, 600, 2), dtype=torch.float32, device="cuda")
    ctx(g, "pointer", 2).decode_compact_crops_tensor([store.arena[e[k][0]:e[k][0] + e[k][1]] for k in (3, 4)], [hl[3] * 2, hl[4] * 2],
                                                     [10, 2000], [600, hl[4] - 2000], planar=False, out=ref)
    for layout, want, valid in ((lay(), W, V), (lay(lengths=lens2), None, V), (lay(), W, None)):
        out.fill_(float("nan"))
        valid_t.fill_(SENT64)
        assert call(layout=layout, want=want, valid=valid) == 0, g.lib.glc_last_error(dec._h)
        dec.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
        assert valid_t.cpu().tolist() == ([SENT64, 600, hl[4] - 2000, SENT64] if valid else [SENT64] * 4)
    st = (L.GlcCompactStatus * 2)()
    assert g.lib.glc_decode_compact_last_status(dec._h, st, 2) == 0
    assert g.lib.glc_decode_compact_last_status(dec._h, st, 1) == EINVAL          # one status per crop
    dec.close()


def test_tensor_call_allocates_and_checks_its_tensors(glc_amd, torch):
    g = glc_amd
    dec = ctx(g, "ragged", 2)
    store = pool(g, torch, 2)
    clips_t, starts_t, want_t = i64(torch, [3, 0, 5]), i64(torch, [0, 500, 2900]), i64(torch, [800, 800, 300])
    args = (store.arena, store.entries, store.lengths, clips_t, starts_t)
    for planar in (True, False):
        out, valid = dec.decode_store_ragged_crops_tensor(*args, 800, store.max_length, want=want_t, planar=planar)
        torch.cuda.synchronize()
        assert tuple(out.shape) == ((3, 2, 800) if planar else (3, 800, 2)) and out.dtype == torch.float32
        assert valid.dtype == torch.int64 and valid.cpu().tolist() == [800, 13, 100]
        tail = out[1, :, 13:] if planar else out[1, 13:, :]
        assert bool((tail.view(torch.int32) == 0).all())
    assert len(dec.last_compact_status()) == 3
    out16, _ = dec.decode_store_ragged_crops_tensor(*args, 800, store.max_length, dtype=torch.int16)
    assert out16.dtype == torch.int16 and tuple(out16.shape) == (3, 2, 800)
    with pytest.raises(g.GlcError) as err:
        dec.decode_store_ragged_crops_tensor(*args, 0, store.max_length)
    assert err.value.code == EINVAL
    with pytest.raises(TypeError):
        dec.decode_store_ragged_crops_tensor(*args, 800, store.max_length, want=want_t.int())
    with pytest.raises(TypeError):
        dec.decode_store_ragged_crops_tensor(*args, 800, store.max_length, want=want_t[:2])
    with pytest.raises(TypeError):
        dec.decode_store_ragged_crops_tensor(*args, 800, store.max_length, valid=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        dec.decode_store_ragged_crops_tensor(*args, 800, store.max_length, valid=torch.zeros(3, dtype=torch.int64))
    empty = i64(torch, [])
    out, valid = dec.decode_store_ragged_crops_tensor(store.arena, store.entries, store.lengths, empty, empty, 800, store.max_length)
    assert tuple(out.shape) == (0, 2, 800) and tuple(valid.shape) == (0,)
    assert g.store_ragged_slots(800, 2) == (3, 3)
