"""Crops drawn from the compact store by device-side index and start: glc_decode_crops_device_store, the draw planner
behind it (k_store_plan_crops through glc_debug_store_plan_device) and Decoder.decode_store_crops_tensor (DESIGN.md
sections 3 and 4).

Every sample comparison is bit for bit - float32 viewed as int32, tolerance 0 - on every element of the output: the
expectation is what Decoder.decode_compact_crops_tensor (glc_decode_crops_device_compact, held to the whole-clip decode
and the oracle by tests/test_compact_crops.py) writes for the same selections resolved on the host, +0.0 for a crop whose
entry or selection is unusable, and a NaN payload nothing computes everywhere else.  One test goes to the oracle-backed
host decode directly.  The status words are compared crop by crop.  Damaged blobs are those of crop_cases /
compact_decode_cases (every count inside its buffer): the tests pin the defined result, they provoke nothing."""
import ctypes as C

import numpy as np
import pytest

import compact_decode_cases as K
import conftest as cf
import crop_cases as CC
import roundtrip_cases as RC
import store_draw_cases as S
from conftest import O
from crop_cases import NAN_BITS, bits

pytestmark = pytest.mark.gpu

HOP = K.HOP
F32 = np.float32
EINVAL = -1
SR = 44100
FAKE_ARENA, FAKE_OUT = 1 << 44, 1 << 52      # numbers the planner hook never dereferences


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    assert hasattr(g.lib, "glc_decode_crops_device_store")
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


def nan_tensor(torch, shape):
    return torch.from_numpy(np.full(shape, NAN_BITS, np.uint32).view(F32)).cuda()


def i64(torch, values):
    return torch.tensor(list(values), dtype=torch.int64).reshape(-1).cuda()


class Store:
    """A store as a caller holds it: everything on the device, plus what the TEST knows about it on the host."""

    def __init__(self, torch, ch, arena, entries, lengths):
        self.ch, self.arena, self.entries = ch, arena, entries
        self.host_lengths = [int(v) for v in lengths]
        self.lengths = i64(torch, self.host_lengths)
        self.max_length = max(self.host_lengths)
        self._host_entries = None

    def host_entries(self):
        if self._host_entries is None:
            self._host_entries = self.entries.cpu().tolist()
        return self._host_entries


def batch_of(torch, ch, clips):
    """Interleaved clips -> a padded planar (B, C, T) device tensor (NaN behind every clip) and the lengths."""
    lens = [c.size // ch for c in clips]
    x = np.full((len(clips), ch, max(lens)), NAN_BITS, np.uint32).view(F32)
    for i, c in enumerate(clips):
        x[i, :, :lens[i]] = np.ascontiguousarray(c, F32).reshape(-1, ch).T
    return torch.from_numpy(x).cuda(), lens


def encode_store(g, torch, ch, clips, arena=None, cursor=None):
    x, lens = batch_of(torch, ch, clips)
    arena, cursor, entries = ctx(g, "enc").encode_compact_batch_tensor(x, lengths=lens, planar=True, arena=arena, cursor=cursor)
    return arena, cursor, entries, lens


def host_store(torch, ch, blobs):
    """blobs: [(bytes-like uint8 array, capacity the entry names, samples per channel)] laid back to back in an arena
    the HOST builds, with entries the host makes."""
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


def check_draw(g, torch, store, clips, starts, length, planar=True, margin=0, dec=None, clips_t=None, starts_t=None, max_length=None):
    """One draw into the leading slice of a NaN-pattern tensor, then - and only then - the selection is resolved on the
    host: every element and every status word is held to the pointer call on the usable crops, to +0.0 and the
    verdict on the others, to the pattern elsewhere.  -> (status words, verdicts)."""
    ch = store.ch
    dec = dec or ctx(g, "draw", ch)
    clips_t = i64(torch, clips) if clips_t is None else clips_t
    starts_t = i64(torch, starts) if starts_t is None else starts_t
    b = clips_t.shape[0]
    shape = (b + margin, ch + margin, length + 3 * margin) if planar else (b + margin, length + margin, ch)
    big = nan_tensor(torch, shape)
    out = big[:b, :ch, margin:margin + length] if planar else big[:b, :length, :]
    got = dec.decode_store_crops_tensor(store.arena, store.entries, store.lengths, clips_t, starts_t, length,
                                        store.max_length if max_length is None else max_length, planar=planar, out=out)
    assert got is out
    assert g.lib.glc_ctx_resident_stream(dec._h) == 0
    # ---- the host enters here
    clips, starts = clips_t.cpu().tolist(), starts_t.cpu().tolist()
    entries, lens = store.host_entries(), store.host_lengths
    ml = store.max_length if max_length is None else max_length
    verdicts = [S.verdict_of(entries, lens, store.arena.numel(), ml, c, s, length) for c, s in zip(clips, starts)]
    good = [i for i, v in enumerate(verdicts) if not v]
    bad = [i for i, v in enumerate(verdicts) if v]
    want = nan_tensor(torch, shape)
    view = want[:b, :ch, margin:margin + length] if planar else want[:b, :length, :]
    want_st = [(v | S.BAD_HEADER, 0, 0) for v in verdicts]
    if good:
        pdec = ctx(g, "pointer", ch)
        blobs = [store.arena[entries[clips[i]][0]:entries[clips[i]][0] + entries[clips[i]][1]] for i in good]
        ref = nan_tensor(torch, (len(good), ch, length) if planar else (len(good), length, ch))
        pdec.decode_compact_crops_tensor(blobs, [lens[clips[i]] * ch for i in good], [starts[i] for i in good], length,
                                         planar=planar, out=ref)
        view[torch.tensor(good).cuda()] = ref
        for i, s in zip(good, status_words(pdec.last_compact_status())):
            want_st[i] = s
    if bad:
        view[torch.tensor(bad).cuda()] = 0.0
    torch.cuda.synchronize()
    same = big.view(torch.int32) == want.view(torch.int32)
    if not bool(same.all()):
        rows = sorted({int(i) for i in torch.nonzero(~same)[:, 0].cpu().tolist()})
        raise AssertionError(f"crops {rows[:8]} differ: {[(clips[i], starts[i], length) for i in rows[:8] if i < b]}")
    st = status_words(dec.last_compact_status())
    assert st == want_st
    return st, verdicts


def clean(words):
    return all(w == (0, 0, 0) for w in words)


# ------------------------------------------------------------------------------------------ 1: the planner against a model

def plan_hook(g, torch, dec, arena, arena_bytes, entries_t, lengths_t, max_length, clips_t, starts_t, length, lay):
    f = g.lib.glc_debug_store_plan_device
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                  C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    n = clips_t.shape[0]
    max_hops = S.slots(length, lay.channels)[0]
    dirs, descs, verdicts = np.zeros(n, S.DIR_DTYPE), np.zeros(n * max_hops, S.DESC_DTYPE), np.zeros(n, np.uint32)
    rc = f(dec._h, arena, arena_bytes, entries_t.data_ptr(), lengths_t.data_ptr(), entries_t.shape[0], max_length,
           clips_t.data_ptr(), starts_t.data_ptr(), length, FAKE_OUT, C.addressof(lay), dirs.ctypes.data, descs.ctypes.data,
           verdicts.ctypes.data)
    assert rc == 0, g.lib.glc_last_error(dec._h)
    return dirs.tolist(), descs.reshape(n, max_hops).tolist(), verdicts.tolist()


def check_plan(g, torch, ch, entries, lengths, max_length, sels, length, arena_bytes=1 << 40):
    L = g._lib
    dec = ctx(g, "draw", ch)
    entries_t = torch.tensor(entries, dtype=torch.int64).cuda()
    lengths_t, clips_t, starts_t = i64(torch, lengths), i64(torch, [s[0] for s in sels]), i64(torch, [s[1] for s in sels])
    n = len(sels)
    verdicts = None
    for planar in (True, False):
        chs = length + 3 if planar else 0
        cs = ch * (length + 3) + 5 if planar else length * ch + 7
        lay = L.GlcClipLayout(n, ch, 1 if planar else 0, cs, chs, length, None)
        got = plan_hook(g, torch, dec, FAKE_ARENA, arena_bytes, entries_t, lengths_t, max_length, clips_t, starts_t, length, lay)
        want = S.plan_model(g, FAKE_ARENA, arena_bytes, entries, lengths, max_length, [s[0] for s in sels], [s[1] for s in sels],
                            length, ch, planar, cs, chs)
        for what, a, b in zip(("directory", "descriptors", "verdicts"), got, want):
            for i, (x, y) in enumerate(zip(a, b)):
                assert x == y or [tuple(r) for r in x] == y, (what, "crop", i, sels[i], x, y)
        verdicts = want[2]
    return verdicts


@pytest.mark.parametrize("ch", (1, 2, 3, 6))
def test_planner_equals_the_model_at_every_hop_boundary(glc_amd, torch, ch):
    g = glc_amd
    lengths = [513, 1536, 2049, 5000, 12345]
    entries = [S.entry(64 * 1000 * i, 64 * (100 + i)) for i in range(len(lengths))]
    for length in (1, 300, 2049, 12345):
        sels = []
        for e in reversed(range(len(lengths))):                      # descending clip indices, each many times over
            pts = S.boundary_starts(lengths[e], ch, length)
            sels += [(e, s) for s in pts] + [(e, 0)] * (2 if pts else 1)
        assert (4, 0) in sels and (4, lengths[4] - length) in sels
        rounds_of = S.per_round(length, ch)
        if rounds_of < 700:
            sels = (sels * (rounds_of // len(sels) + 2))[:rounds_of + 9]      # ... and into a second round
        verdicts = check_plan(g, torch, ch, entries, lengths, 12345, sels, length)
        assert verdicts.count(0) >= 3 and (length <= 513 or S.BAD_CROP in verdicts)     # clips shorter than the crop


def test_planner_verdicts_and_64_bit_arithmetic(glc_amd, torch):
    g = glc_amd
    ab, ml, length = 1 << 40, 40000, 100
    table = [                                                   # (entry, stored length, what the planner must say)
        (S.entry(0, 4096), 5000, 0),
        (S.entry((1 << 32) + 64, 8192), 1536, 0),               # an offset beyond 2^32
        (S.entry(ab - 4096, 4096), 2049, 0),                    # offset + bytes exactly arena_bytes
        (S.entry(ab - 4096, 4097), 2049, S.NO_BLOB),            # ... one byte over
        (S.entry((1 << 64) - 64, 4096), 2049, S.NO_BLOB),       # the sum wraps
        (S.entry(64, (1 << 64) - 1), 2049, S.NO_BLOB),
        (S.entry(96, 4096), 2049, S.NO_BLOB),                   # an offset that is no multiple of 64
        (S.entry(128, 4096, stored=0), 2049, S.NO_BLOB),
        (S.entry(0, 4096), 512, S.BAD_CROP),                    # a length the encoder refuses
        (S.entry(0, 4096), 0, S.BAD_CROP),
        (S.entry(0, 4096), -5, S.BAD_CROP),
        (S.entry(0, 4096), ml, 0),
        (S.entry(0, 4096), ml + 1, S.BAD_CROP),
        (S.entry(0, 4096), (1 << 63) - 1, S.BAD_CROP),
        (S.entry(ab, 0), 2049, 0),                              # an empty blob at the arena's end: inside (R2 fails its header)
        (S.entry(ab + 64, 0), 2049, S.NO_BLOB),
    ]
    entries, lengths = [t[0] for t in table], [t[1] for t in table]
    n_e = len(table)
    sels = [(e, 0) for e in range(n_e)] + [(e, max(0, lengths[e] - length)) for e in range(n_e)]
    expect = [t[2] for t in table] * 2
    extra = [(-1, 0), (n_e, 0), (1 << 62, 0), (-(1 << 63), 0), (0, -1), (0, 5000 - length + 1), (0, (1 << 63) - 1), (0, -(1 << 63)),
             (7, -1), (-1, -1), (n_e - 1, 0), (0, 5000 - length)]
    expect += [S.BAD_CROP] * 10 + [S.NO_BLOB, 0]                 # BAD_CROP wins over an unusable entry
    assert check_plan(g, torch, 2, entries, lengths, ml, sels + extra, length, arena_bytes=ab) == expect
    # lengths near the 32-bit row limit: 2^31 - 1 stereo frames
    big = (1 << 41) - 512
    assert S.frames_of(big) * 2 == (1 << 32) - 2
    entries, lengths = [S.entry(1 << 39, 1 << 38), S.entry(0, 64)], [big, big + 1]
    sels = [(0, 0), (0, big - length), (0, big - length + 1), (1, 0), (0, big // 2)]
    assert check_plan(g, torch, 2, entries, lengths, big, sels, length, arena_bytes=ab) == [0, 0, S.BAD_CROP, S.BAD_CROP, 0]


# ------------------------------------------------------------------------------------------ pools

def kinds(ch, n, seed):
    """tone, silence, noise (raw frames) of n samples per channel"""
    return [cf.gen_tone("sine", 440.0 + seed, SR, ch, (n + 1) / SR)[:n * ch], np.zeros(n * ch, F32), RC.lcg_noise(n * ch, seed=seed + 1)]


POOLS = {2: (513, 1536, 2049, 5000, 12345, 40000), 1: (513, 2049, 5000), 3: (513, 1536, 5000), 6: (513, 2049, 3100)}


def pool(g, torch, ch):
    """The store of a pool of clips, encoded in one call: tone, silence and noise of every length of POOLS[ch]."""
    key = ("pool", ch)
    if key not in _cache:
        clips = [c for i, n in enumerate(POOLS[ch]) for c in kinds(ch, n, 10 * i)]
        arena, _, entries, lens = encode_store(g, torch, ch, clips)
        _cache[key] = Store(torch, ch, arena, entries, lens)
    return _cache[key]


# ------------------------------------------------------------------------------------------ 2: the closed loop

@pytest.mark.parametrize("planar,margin", ((True, 0), (False, 0), (True, 2), (False, 2)),
                         ids=("planar", "interleaved", "planar-slice", "interleaved-slice"))
def test_closed_loop_with_no_host_in_it(glc_amd, torch, planar, margin):
    """Encode into an arena, draw with torch.randint selections on the same stream; the entries are read on the host
    only afterwards (check_draw resolves the selection behind the draw)."""
    g = glc_amd
    ch, length, b = 2, 1000, 96
    clips = [RC.chord(SR, ch, n, seed=n % 17) for n in (1100, 2049, 5000, 7777)] + [RC.lcg_noise(3000 * ch, seed=5)]
    arena, _, entries, lens = encode_store(g, torch, ch, clips)
    store = Store(torch, ch, arena, entries, lens)
    assert store._host_entries is None
    gen = torch.Generator(device="cuda").manual_seed(1234)
    clips_t = torch.randint(0, len(clips), (b,), device="cuda", generator=gen)
    starts_t = torch.randint(0, 1 << 30, (b,), device="cuda", generator=gen) % (store.lengths[clips_t] - length + 1)
    st, verdicts = check_draw(g, torch, store, None, None, length, planar=planar, margin=margin, clips_t=clips_t, starts_t=starts_t)
    assert not any(verdicts) and clean(st)
    assert len(set(clips_t.cpu().tolist())) == len(clips)


# ------------------------------------------------------------------------------------------ 3: window edges

@pytest.mark.parametrize("ch", (2, 1, 3, 6))
def test_window_edges_of_every_clip(glc_amd, torch, ch):
    """Per clip of the pool: the windows crop_cases.edge_windows gives, a crop without a halo frame, one that reaches the
    bare tail hop, single samples - grouped by length, one call per length with every clip that has such a window."""
    g = glc_amd
    store = pool(g, torch, ch)
    by_length, tails, no_halo = {}, 0, 0
    for e, n in enumerate(store.host_lengths):
        nf = S.frames_of(n)
        assert 1 <= nf <= 40
        for start, length in S.edge_draws(n, ch, nf):
            by_length.setdefault(length, []).append((e, start))
            p = g.plan_crop(n * ch, ch, start, length)
            tails += p.first_hop + p.n_hops == nf + 1
            no_halo += p.first_hop == 0
            hops, frames = S.slots(length, ch)
            assert p.n_hops <= hops and p.n_frames <= frames
    assert tails > 10 and no_halo > 10 and 1 in by_length
    unused = 0
    for i, (length, sels) in enumerate(sorted(by_length.items())):
        st, verdicts = check_draw(g, torch, store, [s[0] for s in sels], [s[1] for s in sels], length, planar=bool(i % 2))
        assert not any(verdicts) and clean(st), length
        frames = S.slots(length, ch)[1]
        unused += sum(frames - g.plan_crop(store.host_lengths[e] * ch, ch, s, length).n_frames for e, s in sels)
    assert unused > 50                   # slots with unused rows and descriptors were there, and changed nothing


# ------------------------------------------------------------------------------------------ 4: scan and round edges

def test_unused_rows_straddle_the_scan_blocks(glc_amd, torch):
    """Crops of one sample of a 3-channel pool own 3 frames = 9 table rows each, of which those at a clip's start use 3
    and most others 6: the 1024-row scan blocks begin inside slots, on used and on unused rows."""
    g = glc_amd
    store = pool(g, torch, 3)
    assert S.slots(1, 3) == (2, 3)
    rng = np.random.RandomState(4)
    n_e = len(store.host_lengths)
    sels = [(e, s) for e in range(n_e) for s in (0, CC.boundary_sample(1, 3), CC.boundary_sample(2, 3), store.host_lengths[e] - 1)
            if s < store.host_lengths[e]]
    sels += [(int(rng.randint(n_e)), 0) for _ in range(200)]
    sels += [(e, int(rng.randint(store.host_lengths[e]))) for e in rng.randint(0, n_e, 250)]
    assert len(sels) * 9 > 4 * K.SCAN_BLOCK
    used = [g.plan_crop(store.host_lengths[e] * 3, 3, s, 1).n_frames for e, s in sels]
    assert set(used) == {1, 2, 3}
    for planar in (True, False):
        st, verdicts = check_draw(g, torch, store, [s[0] for s in sels], [s[1] for s in sels], 1, planar=planar)
        assert not any(verdicts) and clean(st)
    # ... and stereo single samples (2 frames a slot), more than a scan block of rows
    store = pool(g, torch, 2)
    sels = [(e, int(rng.randint(store.host_lengths[e]))) for e in rng.randint(0, len(store.host_lengths), 300)] + [(0, 0), (3, 0)]
    st, verdicts = check_draw(g, torch, store, [s[0] for s in sels], [s[1] for s in sels], 1)
    assert not any(verdicts) and clean(st)


def test_700_crops_take_two_rounds(glc_amd, torch):
    g = glc_amd
    store = pool(g, torch, 2)
    length = 3000
    assert S.slots(length, 2) == (4, 5) and S.per_round(length, 2) == 682
    rng = np.random.RandomState(7)
    fits = [e for e, n in enumerate(store.host_lengths) if n >= length]
    clips = [fits[int(k)] for k in rng.randint(0, len(fits), 700)]
    starts = [int(rng.randint(0, store.host_lengths[e] - length + 1)) for e in clips]
    for i in (0, 681, 682, 699):                                 # the last crop of a round and the first of the next
        starts[i] = store.host_lengths[clips[i]] - length
    dec = glc_amd.Decoder(2, SR)
    for planar in (True, False):
        st, verdicts = check_draw(g, torch, store, clips, starts, length, planar=planar, dec=dec)
        assert not any(verdicts) and clean(st)
    # a second, smaller call on the same context: workspaces reused, one status per crop of THAT call
    st, _ = check_draw(g, torch, store, clips[:3], starts[:3], length, dec=dec)
    assert len(st) == 3 and clean(st)
    st, _ = check_draw(g, torch, store, [0, 5], [1, 2], 17, dec=dec)
    assert len(st) == 2 and clean(st)
    dec.close()


def test_window_behind_more_than_4096_rows(glc_amd, torch):
    """A clip of about 2100 stereo frames: windows with more than one prefix chunk of rows in front, with max_length
    equal to the clip and far above it (the prefix launch is sized by it)."""
    g = glc_amd
    n = 2100 * HOP + 17
    t = np.arange(n, dtype=np.float64)
    mono = (0.3 * np.sin(2 * np.pi * 440.0 / SR * t) + 0.1 * np.sin(2 * np.pi * 1234.5 / SR * t)).astype(F32)
    x = np.stack([mono, mono[::-1]], 1).reshape(-1)
    short = RC.chord(SR, 2, 3000, seed=3)
    arena, _, entries, lens = encode_store(g, torch, 2, [short, x])
    store = Store(torch, 2, arena, entries, lens)
    length = 2500
    starts = [n - length, 2060 * HOP, CC.PREFIX_ROWS // 2 * HOP, 0, 500, 12 * HOP + 3]
    clips = [1, 1, 1, 1, 0, 1]
    p = g.plan_crop(n * 2, 2, starts[0], length)
    assert p.first_frame * 2 > CC.PREFIX_ROWS
    for max_length in (n, 1 << 30):
        st, verdicts = check_draw(g, torch, store, clips, starts, length, max_length=max_length)
        assert not any(verdicts) and clean(st)


# ------------------------------------------------------------------------------------------ 5: appending, and a host-built store

def test_entries_of_two_encode_calls_with_one_cursor(glc_amd, torch):
    g = glc_amd
    ch = 2
    first = [RC.chord(SR, ch, n, seed=n % 13) for n in (1300, 4000)]
    second = [RC.lcg_noise(2500 * ch, seed=8), RC.chord(SR, ch, 6000, seed=2), np.zeros(1025 * ch, F32)]
    arena = torch.empty(g.compact_store_bound(ch, [c.size // ch for c in first + second]), dtype=torch.uint8, device="cuda")
    arena, cursor, e1, l1 = encode_store(g, torch, ch, first, arena=arena)
    arena, cursor, e2, l2 = encode_store(g, torch, ch, second, arena=arena, cursor=cursor)
    store = Store(torch, ch, arena, torch.cat([e1, e2]), l1 + l2)
    rng = np.random.RandomState(12)
    clips = [int(k) for k in rng.randint(0, 5, 40)] + [4, 3, 2, 1, 0]
    starts = [int(rng.randint(0, store.host_lengths[e] - 1000 + 1)) for e in clips]
    st, verdicts = check_draw(g, torch, store, clips, starts, 1000)
    assert not any(verdicts) and clean(st)
    offs = [e[0] for e in store.host_entries()]
    assert offs == sorted(offs) and all(e[3] >> 32 == 1 for e in store.host_entries())
    assert int(cursor.item()) == offs[-1] + store.host_entries()[-1][1]


def test_host_built_store_against_the_oracle(glc_amd, torch):
    """Blobs of glc_frames_to_compact uploaded by the host, entries made by the host; the expectation of this test is
    the slice of the host decode, which must be the oracle's."""
    g = glc_amd
    ch = 2
    xs = [np.ascontiguousarray(x, F32) for x in (RC.chord(SR, ch, 3 * HOP + 300), RC.mixed_clip(SR, ch), RC.chord(SR, ch, 513, seed=9))]
    blobs, refs = [], []
    for x in xs:
        stream = ctx(g, "enc").encode(x, ch)
        blob = np.frombuffer(g.frames_to_compact(stream), np.uint8)
        ref = ctx(g, "host", ch).decode(stream).copy()
        assert np.array_equal(bits(ref), bits(O.decode(O.encode(x, SR, ch).glc)[0]))
        blobs.append((blob, blob.size, x.size // ch))
        refs.append(ref)
    store = host_store(torch, ch, blobs)
    length = 400
    sels = [(e, s) for e, n in enumerate(store.host_lengths) for s in S.boundary_starts(n, ch, length)]
    sels = sels[::-1]
    dec = ctx(g, "draw", ch)
    for planar in (True, False):
        out = dec.decode_store_crops_tensor(store.arena, store.entries, store.lengths, i64(torch, [s[0] for s in sels]),
                                            i64(torch, [s[1] for s in sels]), length, store.max_length, planar=planar)
        torch.cuda.synchronize()
        want = CC.want_crops(tuple(out.shape), planar, 0, ch, [(refs[e], s, length) for e, s in sels])
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
        assert clean(status_words(dec.last_compact_status()))
    st, verdicts = check_draw(g, torch, store, [s[0] for s in sels], [s[1] for s in sels], length)      # ... and the pointer call
    assert not any(verdicts) and clean(st)


# ------------------------------------------------------------------------------------------ 6: untrusted data

def test_crafted_and_damaged_blobs_in_an_arena(glc_amd, torch):
    """The crafted streams and the damaged blobs of crop_cases side by side in one arena: samples and status words are
    the pointer call's (check_draw compares both), and the damaged ones report what that call reports."""
    g = glc_amd
    base = CC.stereo_stream()
    n_true = sum(len(r.idx) for _, body in base for r in body)
    o_pairs = K.layout(2, len(base))[3]
    packed = [K.pack(2, frames) for name, ch, frames in CC.crafted() if ch == 2]
    blobs = [(buf[:nbytes], nbytes, len(frames) * HOP) for (buf, nbytes), (_, ch, frames) in
             zip(packed, [c for c in CC.crafted() if c[1] == 2])]
    n_crafted = len(blobs)
    damaged = [dict(magic=K.MAGIC ^ 0x100), dict(cnt_set={1: HOP}), dict(n_pairs=n_true + 1, bytes_field=K.align64(o_pairs + 4 * (n_true + 1)))]
    for over in damaged:
        buf, _ = K.pack(2, base, **over)
        blobs.append((buf, buf.size, len(base) * HOP))            # the entry names the whole buffer, as the pointer tests do
    for row in (7, 4, 3, 10):
        buf, _ = K.pack(2, CC.with_bad_list(base, row))
        blobs.append((buf, buf.size, len(base) * HOP))
    store = host_store(torch, 2, blobs)
    start, length = CC.first_sample_of_hop(3, 2), CC.first_sample_of_hop(5, 2) - CC.first_sample_of_hop(3, 2)     # frames 2 .. 4
    p = g.plan_crop(len(base) * HOP * 2, 2, start, length)
    assert (p.first_frame, p.n_frames) == (2, 3)
    sels = [(e, s) for e in range(len(blobs)) for s in (start, 0, store.host_lengths[e] - length)]
    st, verdicts = check_draw(g, torch, store, [s[0] for s in sels], [s[1] for s in sels], length, planar=False)
    assert not any(verdicts)
    of = lambda e: st[3 * e]                                      # the crop of frames 2 .. 4 of entry e
    assert all(clean(st[3 * e:3 * e + 3]) for e in range(n_crafted))
    assert of(n_crafted) == (K.BAD_HEADER, 3 * 2, 2 * 2)          # bad magic: the window's rows
    assert of(n_crafted + 1) == (K.ROW_BOUNDS, 6, 4)              # an inflated cnt in front of the window
    assert of(n_crafted + 2) == (0, 0, 0)                         # the pair sum is not a crop's business
    assert [of(n_crafted + 3 + k) for k in range(4)] == [(K.NOT_CANONICAL, 1, 7), (K.NOT_CANONICAL, 1, 4), (0, 0, 0), (0, 0, 0)]


def test_arena_too_small_for_the_last_clips(glc_amd, torch):
    g = glc_amd
    ch = 2
    clips = [RC.chord(SR, ch, n, seed=n % 11) for n in (2000, 3000, 2500, 4000)]
    arena, cursor, entries, lens = encode_store(g, torch, ch, clips)
    full = Store(torch, ch, arena, entries, lens)
    sizes = [e[1] for e in full.host_entries()]
    small = torch.empty(sizes[0] + sizes[1] + 64, dtype=torch.uint8, device="cuda")        # the third clip does not fit
    arena, cursor, entries, lens = encode_store(g, torch, ch, clips, arena=small)
    store = Store(torch, ch, arena, entries, lens)
    sels = [(0, 0), (2, 0), (1, 7), (3, 100), (1, 2000), (2, 1500)]
    st, verdicts = check_draw(g, torch, store, [s[0] for s in sels], [s[1] for s in sels], 1000)
    assert verdicts == [0, S.NO_BLOB, 0, S.NO_BLOB, 0, S.NO_BLOB]
    assert [e[3] >> 32 for e in store.host_entries()] == [1, 1, 0, 0]
    assert st[1] == (S.NO_BLOB | S.BAD_HEADER, 0, 0) and clean([st[0], st[2], st[4]])
    assert int(cursor.item()) == sum(sizes)


@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
def test_bad_entries_and_selections_between_good_crops(glc_amd, torch, planar):
    """Entries a host made, some unusable, and selections some of which are: exact status words, +0.0, neighbours bit
    for bit (check_draw holds every element of the batch)."""
    g = glc_amd
    ch = 2
    good = pool(g, torch, ch)
    ent = [list(e) for e in good.host_entries()]
    lens = list(good.host_lengths)
    n_e = len(ent)
    ab = good.arena.numel()
    ent[1][0] += 32                                               # misaligned
    ent[2][3] &= 0xFFFFFFFF                                       # stored == 0
    ent[4] = S.entry(ab - 64, 128)                                # leaves the arena
    ent[5] = S.entry((1 << 64) - 64, ent[5][1])                   # the sum wraps
    lens[7] = 512                                                 # a length the encoder refuses
    lens[8] = good.max_length + 1
    store = Store(torch, ch, good.arena, torch.tensor(ent, dtype=torch.int64).cuda(), lens)
    length = 300
    clips = [0, 1, 3, 2, 6, 4, 9, 5, 10, 7, 11, 8, 12, -1, 13, n_e, 14, 1 << 40, 15, 16, 17, 16, 17, 1, 3]
    starts = [0, 0, 5, 0, 9, 0, 100, 0, 7, 0, 3, 0, 50, 0, 11, 0, 13, 0, -1, lens[16] - length + 1, lens[17] - length, -(1 << 63), 0, -1, 213]
    st, verdicts = check_draw(g, torch, store, clips, starts, length, planar=planar, margin=1, max_length=good.max_length)
    n, b = S.NO_BLOB, S.BAD_CROP
    assert verdicts == [0, n, 0, n, 0, n, 0, n, 0, b, 0, b, 0, b, 0, b, 0, b, b, b, 0, b, 0, b, 0]
    assert [w for w, v in zip(st, verdicts) if v] == [(v | S.BAD_HEADER, 0, 0) for v in verdicts if v]
    assert clean([w for w, v in zip(st, verdicts) if not v])


# ------------------------------------------------------------------------------------------ 7: the call's edges

def test_arguments_refused_before_anything_is_queued(glc_amd, torch):
    g = glc_amd
    L = g._lib
    dec = glc_amd.Decoder(2, SR)
    store = pool(g, torch, 2)
    length, ml, n_e = 600, store.max_length, len(store.host_lengths)
    clips_t, starts_t = i64(torch, [3, 4]), i64(torch, [10, 20])
    out = nan_tensor(torch, (2, 600, 2))
    room = torch.zeros(64 * 1024, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    A, E, Ln, Cl, St, o = store.arena.data_ptr(), store.entries.data_ptr(), store.lengths.data_ptr(), clips_t.data_ptr(), starts_t.data_ptr(), out.data_ptr()
    lens2 = (C.c_uint64 * 2)(600, 600)

    def lay(n_clips=2, ch=2, planar=0, cs=1200, chs=0, lengths=None, one=600):
        return L.GlcClipLayout(n_clips, ch, planar, cs, chs, one, C.cast(lengths, C.POINTER(C.c_uint64)) if lengths is not None else None)

    def call(arena=A, ab=None, entries=E, lengths=Ln, n=n_e, max_length=ml, clips=Cl, starts=St, length=length, d_out=o, layout=None):
        layout = layout or lay()
        return g.lib.glc_decode_crops_device_store(dec._h, arena, store.arena.numel() if ab is None else ab, entries, lengths, n,
                                                   max_length, clips, starts, length, d_out, C.byref(layout))

    big_frames = (1 << 41) + 1024                                # 2^31 + 1 stereo frames: more than 32 bits of rows
    refused = [
        call(arena=None), call(entries=None), call(lengths=None), call(clips=None), call(starts=None), call(d_out=None),
        g.lib.glc_decode_crops_device_store(dec._h, A, 64, E, Ln, n_e, ml, Cl, St, length, o, None),
        call(layout=lay(ch=0)),
        call(arena=A + 32),                                       # the arena is not 64-byte aligned
        call(entries=E + 4), call(lengths=Ln + 4), call(clips=Cl + 4), call(starts=St + 4),
        call(d_out=o + 2),
        call(length=0, layout=lay(one=0)),
        call(max_length=length - 1),
        call(max_length=512, length=512, layout=lay(one=512)),    # a max_length the encoder refuses
        call(max_length=big_frames),                              # ... whose rows exceed 32 bits
        call(max_length=1 << 62),
        call(layout=lay(lengths=(C.c_uint64 * 2)(600, 599))),     # lengths given and not all `length`
        call(layout=lay(one=599)),                                # ... one length for all that is not `length`
        call(layout=lay(cs=1199)),                                # a clip overlaps the next
        call(layout=lay(planar=1, cs=1200, chs=599)),             # a plane overlaps the next
        call(n=0),
        call(length=4095 * HOP + 2, max_length=1 << 23, layout=lay(n_clips=1, one=4095 * HOP + 2)),     # max_frames + 1 > 4097
        call(d_out=A + 64),                                       # the output overlaps the arena
        call(d_out=A + store.arena.numel() - 4),
        call(d_out=E - 4 * 1199 + 8, layout=lay(n_clips=1)),      # ... the entries
        call(d_out=Ln), call(d_out=Cl), call(d_out=St - 4 * 2399),
    ]
    assert refused == [EINVAL] * len(refused)
    # the planner hook checks what the call checks: a clip that overlaps the next, an arena that is not aligned
    hook = g.lib.glc_debug_store_plan_device
    hook.restype = C.c_int
    hook.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                     C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    plan = np.zeros(4096, np.uint8)
    for arena_at, layout, what in ((A, lay(cs=1199), b"clip_stride"), (A + 32, lay(), b"64-byte")):
        assert hook(dec._h, arena_at, store.arena.numel(), E, Ln, n_e, ml, Cl, St, length, o, C.addressof(layout), plan.ctypes.data,
                    plan.ctypes.data, plan.ctypes.data) == EINVAL
        assert b"glc_debug_store_plan_device" in g.lib.glc_last_error(dec._h) and what in g.lib.glc_last_error(dec._h)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy().view(np.uint32) == NAN_BITS)
    assert g.lib.glc_decode_compact_last_status(dec._h, (L.GlcCompactStatus * 2)(), 2) == EINVAL      # nothing has completed
    # no clips: nothing to do, whatever else is passed
    assert g.lib.glc_decode_crops_device_store(dec._h, None, 0, None, None, 0, 0, None, None, 0, None, C.byref(lay(n_clips=0))) == 0
    # ... and the accepted forms of the same call: one length for all, and a lengths array
    for layout in (lay(), lay(lengths=lens2)):
        assert call(layout=layout) == 0
        dec.synchronize()
        ref = nan_tensor(torch, (2, 600, 2))
        blobs = [store.arena[e[0]:e[0] + e[1]] for e in (store.host_entries()[3], store.host_entries()[4])]
        ctx(g, "pointer", 2).decode_compact_crops_tensor(blobs, [store.host_lengths[3] * 2, store.host_lengths[4] * 2], [10, 20], 600,
                                                         planar=False, out=ref)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    st = (L.GlcCompactStatus * 2)()
    assert g.lib.glc_decode_compact_last_status(dec._h, st, 2) == 0
    assert g.lib.glc_decode_compact_last_status(dec._h, st, 1) == EINVAL          # one status per crop
    dec.close()


def test_context_state_afterwards(glc_amd, torch):
    """No stream is resident afterwards and an open decode session is closed; a glc_decode that follows is what it always
    was; the pointer call and the draw alternate on one context (the draw leaves the pinned table image alone)."""
    g = glc_amd
    dec = g.Decoder(2, SR)
    x = RC.chord(SR, 2, 4 * HOP + 100)
    stream = ctx(g, "enc").encode(x, 2)
    before = dec.decode(stream).copy()
    assert g.lib.glc_ctx_resident_stream(dec._h) != 0
    store = pool(g, torch, 2)
    st, _ = check_draw(g, torch, store, [3, 4, 5], [0, 100, 200], 500, dec=dec)
    assert g.lib.glc_ctx_resident_stream(dec._h) == 0 and clean(st)
    assert np.array_equal(bits(dec.decode(stream)), bits(before))
    e = store.host_entries()
    for _ in range(2):
        ref = nan_tensor(torch, (2, 2, 500))
        dec.decode_compact_crops_tensor([store.arena[e[k][0]:e[k][0] + e[k][1]] for k in (3, 4)],
                                        [store.host_lengths[k] * 2 for k in (3, 4)], [5, 6], 500, out=ref)
        st, _ = check_draw(g, torch, store, [3, 4], [5, 6], 500, dec=dec)
        assert clean(st)
    # a decode session that is open is closed by the draw
    assert g.lib.glc_decode_stream_begin(dec._h, stream._h) == 0
    check_draw(g, torch, store, [3], [0], 500, dec=dec)
    out = C.c_uint64()
    last = C.c_int()
    buf = np.empty(16, F32)
    assert g.lib.glc_decode_stream_next(dec._h, buf.ctypes.data, 16, C.byref(out), C.byref(last)) == EINVAL
    dec.close()


def test_tensor_call_allocates_and_checks_its_tensors(glc_amd, torch):
    g = glc_amd
    dec = ctx(g, "draw", 2)
    store = pool(g, torch, 2)
    clips_t, starts_t = i64(torch, [3, 9, 4]), i64(torch, [0, 700, 1])
    e, lens = store.host_entries(), store.host_lengths
    for planar in (True, False):
        out = dec.decode_store_crops_tensor(store.arena, store.entries, store.lengths, clips_t, starts_t, 800, store.max_length, planar=planar)
        ref = ctx(g, "pointer", 2).decode_compact_crops_tensor([store.arena[e[k][0]:e[k][0] + e[k][1]] for k in (3, 9, 4)],
                                                              [lens[k] * 2 for k in (3, 9, 4)], [0, 700, 1], 800, planar=planar)
        torch.cuda.synchronize()
        assert tuple(out.shape) == ((3, 2, 800) if planar else (3, 800, 2))
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    assert len(dec.last_compact_status()) == 3
    with pytest.raises(g.GlcError) as err:
        dec.decode_store_crops_tensor(store.arena, store.entries, store.lengths, clips_t, starts_t, 0, store.max_length)
    assert err.value.code == EINVAL
    with pytest.raises(TypeError):
        dec.decode_store_crops_tensor(store.arena, store.entries, store.lengths, clips_t.int(), starts_t, 800, store.max_length)
    with pytest.raises(TypeError):
        dec.decode_store_crops_tensor(store.arena, store.entries.cpu(), store.lengths, clips_t, starts_t, 800, store.max_length)
    with pytest.raises(g.GlcError):
        dec.decode_store_crops_tensor(store.arena, store.entries, store.lengths, clips_t, starts_t[:2], 800, store.max_length)
    empty = i64(torch, [])
    out = dec.decode_store_crops_tensor(store.arena, store.entries, store.lengths, empty, empty, 800, store.max_length)
    assert tuple(out.shape) == (0, 2, 800)
