"""Windows of stored clips: glc_decode_crops_device_compact, R2 of windows behind it (launch_rows_from_compact through
glc_debug_rows_from_compact_window; the whole blob, glc_debug_rows_from_compact, is the window of all frames plus the
totals check) and Decoder.decode_compact_crops_tensor (DESIGN.md sections 3 and 4).

Every sample comparison is bit for bit - float32 viewed as uint32, tolerance 0.  The expectation is always the slice
of a path that existed before: Decoder.decode_compact_tensor (glc_decode_device_compact) of the same bytes, which
tests/test_compact_decode.py holds to glc_decode of glc_frames_from_compact, and that host path itself for the crafted
blobs; for the small natural clips also the oracle's decode.  Outputs are pre-filled with a NaN payload nothing
computes and every element outside the crops must keep it.  Damaged blobs sit in buffers of glc_compact_bound bytes
with every count inside the buffer (compact_decode_cases.pack): the tests pin the defined result, they provoke
nothing."""
import ctypes as C
import struct

import numpy as np
import pytest

import compact_decode_cases as K
import conftest as cf
import crop_cases as CC
import roundtrip_cases as RC
from conftest import O
from crop_cases import NAN_BITS, ROUND, bits

pytestmark = pytest.mark.gpu

HOP, FRAME = K.HOP, K.FRAME
F32 = np.float32
EINVAL = -1
SR = 44100


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    assert hasattr(g.lib, "glc_decode_crops_device_compact")
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


def upload(torch, buf):
    t = torch.from_numpy(np.ascontiguousarray(buf, np.uint8)).cuda()
    assert t.data_ptr() % 64 == 0
    return t


def whole_decode(g, torch, d_blob, n_samples, ch):
    """The whole clip through the call that existed before (glc_decode_device_compact) -> (samples, status)."""
    dec = ctx(g, "whole", ch)
    y = dec.decode_compact_tensor(d_blob, n_samples)
    torch.cuda.synchronize()
    return y.cpu().numpy().copy(), dec.last_compact_status()[0]


def host_decode(g, blob, n_samples, ch):
    enc = g.EncodedAudio.from_compact(SR, n_samples, ch, [np.ascontiguousarray(blob, np.uint8)])
    return ctx(g, "host", ch).decode(enc).copy()


def decode_crops(g, torch, ch, entries, planar=True, margin=0):
    """entries: [(device blob, n_samples, whole clip's samples, start, length)].  One call into a NaN-pattern tensor
    (a slice of a bigger one when margin > 0); every element is held to the slices / to the pattern.  -> statuses."""
    dec = ctx(g, "dec", ch)
    b = len(entries)
    l_max = max(e[4] for e in entries)
    shape = (b + margin, ch + margin, l_max + 3 * margin) if planar else (b + margin, l_max + margin, ch)
    big = nan_tensor(torch, shape)
    out = big[:b, :ch, margin:margin + l_max] if planar else big[:b, :l_max, :]
    got = dec.decode_compact_crops_tensor([e[0] for e in entries], [e[1] for e in entries], [e[3] for e in entries],
                                          [e[4] for e in entries], planar=planar, out=out)
    assert got is out
    torch.cuda.synchronize()
    assert g.lib.glc_ctx_resident_stream(dec._h) == 0
    want = CC.want_crops(shape, planar, margin, ch, [(e[2], e[3], e[4]) for e in entries])
    host = big.cpu().numpy().view(np.uint32)
    if not np.array_equal(host, want):
        bad = sorted({int(i) for i in np.argwhere(host != want)[:, 0]})
        raise AssertionError(f"crops {bad[:8]} differ: {[(entries[i][3], entries[i][4]) for i in bad[:8] if i < b]}")
    st = dec.last_compact_status()
    assert len(st) == b
    return st


def clean(st):
    return (st.flags, st.n_bad_rows, st.first_bad_row) == (0, 0, 0)


# ------------------------------------------------------------------------------------------ 1: window edges

def noise_then_tone(ch):
    """white noise, then a tone: raw frames, then compressed ones"""
    return np.concatenate([RC.lcg_noise(5 * HOP * ch), cf.gen_tone("sine", 440.0, SR, ch, 6 * HOP / SR)[:6 * HOP * ch]])


NATURAL = [
    ("chord-mono", 1, lambda: RC.chord(SR, 1, 5 * HOP + 300)),
    ("chord-stereo", 2, lambda: RC.chord(SR, 2, 5 * HOP + 1)),
    ("chord-stereo-short-of-the-tail", 2, lambda: RC.chord(SR, 2, 5 * HOP + 600, seed=3)),
    ("chord-3ch", 3, lambda: RC.chord(SR, 3, 5 * HOP + 300)),
    ("chord-6ch", 6, lambda: RC.chord(SR, 6, 5 * HOP)),
    ("noise-then-tone-stereo", 2, lambda: noise_then_tone(2)),
]


def natural(g, torch, name):
    """(device blob, n_samples, whole decode, frames, is_raw per frame) of a natural clip, made once."""
    if name not in _cache:
        _, ch, make = next(c for c in NATURAL if c[0] == name)
        x = np.ascontiguousarray(make(), F32)
        assert x.size % ch == 0
        d_blob, info = ctx(g, "enc").encode_compact_tensor(torch.from_numpy(x).cuda(), ch)
        d_blob = d_blob.clone()
        ref, st = whole_decode(g, torch, d_blob, x.size, ch)
        assert clean(st) and ref.size == x.size
        oracle = O.decode(O.encode(x, SR, ch).glc)[0]
        assert np.array_equal(bits(ref), bits(oracle))
        nf = int(info.n_frames)
        israw = d_blob[64:64 + nf].cpu().numpy().astype(bool)
        _cache[name] = (d_blob, x.size, ref, nf, israw)
    return _cache[name]


@pytest.mark.parametrize("name,ch", [(c[0], c[1]) for c in NATURAL], ids=[c[0] for c in NATURAL])
def test_window_edges_of_natural_clips(glc_amd, torch, name, ch):
    g = glc_amd
    d_blob, n_samples, ref, nf, israw = natural(g, torch, name)
    n = n_samples // ch
    assert 5 <= nf <= 12
    windows = CC.edge_windows(n, ch, nf)
    assert (0, 1) in windows and (0, n) in windows and (n - 1, 1) in windows
    if ch in (3, 6):                 # the hop boundary falls inside a sample frame: windows of that one frame
        b = CC.boundary_sample(1, ch)
        assert CC.hop_of(b, 0, ch) == 0 and CC.hop_of(b, ch - 1, ch) == 1 and (b, 1) in windows
    if name == "chord-stereo-short-of-the-tail":
        assert not CC.reaches_tail(n, ch, nf)
    if name in ("chord-stereo", "chord-mono"):
        assert CC.reaches_tail(n, ch, nf)
    if name == "noise-then-tone-stereo":
        # a raw halo frame in front of a raw and of a compressed own frame: the one-hop windows of hops f + 1
        assert israw[0] and israw[1] and not israw[-1]
        f = int(np.flatnonzero(~israw)[0])
        assert israw[f - 1]
        for h in (1, f):             # own frame h, halo frame h - 1
            a = CC.first_sample_of_hop(h, ch)
            assert (a, CC.first_sample_of_hop(h + 1, ch) - a) in windows
            p = g.plan_crop(n_samples, ch, a, CC.first_sample_of_hop(h + 1, ch) - a)
            assert (p.first_frame, p.n_frames) == (h - 1, 2)
    entries = [(d_blob, n_samples, ref, s, l) for s, l in windows]
    for planar in (True, False):     # all windows of the clip in one call: the same blob many times over
        st = decode_crops(g, torch, ch, entries, planar=planar)
        assert all(clean(s) for s in st)
    for s, l in ((0, 1), (n - 1, 1), (0, n), windows[len(windows) // 2]):     # ... and alone
        st = decode_crops(g, torch, ch, [(d_blob, n_samples, ref, s, l)])
        assert clean(st[0])


# ------------------------------------------------------------------------------------------ 2: crafted blobs

CRAFTED = CC.crafted()


@pytest.mark.parametrize("name,ch,frames", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_windows_of_crafted_blobs(glc_amd, torch, name, ch, frames):
    g = glc_amd
    buf, nbytes = K.pack(ch, frames)
    nf = len(frames)
    n_samples = K.n_samples_of(ch, nf)
    ref = host_decode(g, buf[:nbytes], n_samples, ch)            # glc_decode of glc_frames_from_compact
    d_blob = upload(torch, buf[:nbytes])
    dev, st = whole_decode(g, torch, d_blob, n_samples, ch)
    assert clean(st) and np.array_equal(bits(dev), bits(ref))
    windows = CC.crafted_windows(nf, ch)
    p = g.plan_crop(n_samples, ch, *windows[0])
    assert (p.first_frame, p.n_frames) == (0, 1)                 # only the first frame
    p = g.plan_crop(n_samples, ch, *windows[1])
    assert (p.first_frame, p.n_frames) == (nf - 1, 1)            # only the last frame
    st = decode_crops(g, torch, ch, [(d_blob, n_samples, ref, s, l) for s, l in windows], planar=False)
    assert all(clean(s) for s in st)
    if "inf" in name:
        assert np.isnan(ref).any()


# ------------------------------------------------------------------------------------------ 3: the scans, at table level

def rows_window(g, torch, d_blob, cap_bytes, nf, ch, f0, frames):
    """(row_begin, row_cnt, row_raw, status) of a window through glc_debug_rows_from_compact_window."""
    f = g.lib.glc_debug_rows_from_compact_window
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint16, C.c_uint64, C.c_uint64] + [C.c_void_p] * 6
    m = frames * ch
    begin, cnt, raw = np.empty(m, np.uint64), np.empty(m, np.uint32), np.empty(m, np.int64)
    st = (C.c_uint64 * 3)()
    rc = f(ctx(g, "dec", ch)._h, d_blob.data_ptr(), cap_bytes, nf, ch, f0, frames, begin.ctypes.data, cnt.ctypes.data, None,
           raw.ctypes.data, None, C.addressof(st))
    assert rc == 0
    return begin, cnt, raw, (st[0] & 0xFFFFFFFF, st[1], st[2])


def check_table_windows(g, torch, buf, nbytes, nf, ch, want, windows):
    d_blob = upload(torch, buf[:nbytes])
    torch.cuda.synchronize()
    for f0, frames in windows:
        begin, cnt, raw, st = rows_window(g, torch, d_blob, nbytes, nf, ch, f0, frames)
        r0, r1 = f0 * ch, (f0 + frames) * ch
        assert st == (0, 0, 0), (f0, frames, st)
        for got, full in zip((begin, cnt, raw), want):
            assert np.array_equal(got, full[r0:r1]), (f0, frames)


SCAN_SHAPES = [(K.SCAN_BLOCK - 1, 1), (K.SCAN_BLOCK, 1), (K.SCAN_BLOCK + 1, 1), (2 * K.SCAN_BLOCK + 1, 1), (1026, 3)]


@pytest.mark.parametrize("rows,ch", SCAN_SHAPES, ids=[f"rows-{r}-{c}ch" for r, c in SCAN_SHAPES])
def test_window_tables_at_the_scan_edges(glc_amd, torch, rows, ch):
    frames = CC.scan_blob(rows, ch)
    buf, nbytes = K.pack(ch, frames)
    windows = CC.table_windows(rows, ch)
    firsts = {w[0] * ch for w in windows}
    if ch == 1:
        assert firsts >= {r for r in (0, 1, K.SCAN_BLOCK - 1, K.SCAN_BLOCK, K.SCAN_BLOCK + 1, rows - 1) if r < rows}
        assert {w[1] for w in windows} >= {1, 3, 4, 5}
    else:
        assert firsts >= {0, 3, 1020, 1023}
    check_table_windows(glc_amd, torch, buf, nbytes, rows // ch, ch, K.tables(ch, frames), windows)


def test_window_tables_at_the_prefix_chunk_edges(glc_amd, torch):
    """Rows in front of a window are summed in chunks of PREFIX_ROWS per workgroup: windows with one row less, exactly,
    and one row more than a chunk in front, and at the end of a blob of more than one chunk."""
    nf = CC.PREFIX_ROWS + 1100
    P = CC.PREFIX_ROWS
    buf, nbytes, want = K.big_mono(nf, (0, 3, P - 2, P - 1, P, P + 1, nf - 1), seed=7)
    windows = [(f0, n) for f0 in (P - 1, P, P + 1, P + 2, nf - 1) for n in (1, 4) if f0 + n <= nf] + [(2, nf - 2), (P - 3, 1030)]
    check_table_windows(glc_amd, torch, buf, nbytes, nf, 1, want, windows)


def test_window_tables_behind_a_million_rows(glc_amd, torch):
    """A blob of more than 1024 * 1024 rows: a short window behind row 1024 * 1024 (257 chunks of rows in front of it),
    and a window of more than 1024 * 1024 rows - more than 1024 scan blocks, so the one-workgroup scan of the window's
    block sums takes a second chunk and carries the first one's total into it.  Tables only."""
    edge = K.SCAN_BLOCK * K.SCAN_BLOCK
    nf = edge + K.SCAN_BLOCK + 7
    buf, nbytes, want = K.big_mono(nf, (0, 5, edge - 1, edge, edge + 1, edge + 3, nf - 1))
    check_table_windows(glc_amd, torch, buf, nbytes, nf, 1, want, [(edge + 1, 5), (edge - 2, 9), (nf - 1, 1), (3, edge + 1025)])


def all_tables(g, d_blob, cap_bytes, nf, ch, window):
    """The five row tables (the scales as bits) and (flags, n_bad_rows, first_bad_row) of a blob through
    glc_debug_rows_from_compact (window None), or of the window (first_frame, frames) through its window twin."""
    tail = [C.c_void_p] * 6
    if window is None:
        f, mid, frames = g.lib.glc_debug_rows_from_compact, (), nf
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint16] + tail
    else:
        f, mid, frames = g.lib.glc_debug_rows_from_compact_window, tuple(window), window[1]
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint16, C.c_uint64, C.c_uint64] + tail
    f.restype = C.c_int
    m = frames * ch
    arrays = [np.empty(m, t) for t in (np.uint64, np.uint32, np.uint32, np.int64, np.uint64)]   # begin, cnt, scale, raw, raw_len
    st = (C.c_uint64 * 3)()
    rc = f(ctx(g, "dec", ch)._h, d_blob.data_ptr(), cap_bytes, nf, ch, *mid, *[a.ctypes.data for a in arrays], C.addressof(st))
    assert rc == 0
    return arrays, (st[0] & 0xFFFFFFFF, st[1], st[2])


def whole_and_window(g, torch, buf, cap_bytes, nf, ch):
    """Both hooks over all frames of one blob: the tables must be bit-equal.  -> (tables, whole status, window status)."""
    d_blob = upload(torch, buf)
    torch.cuda.synchronize()
    whole, st_whole = all_tables(g, d_blob, cap_bytes, nf, ch, None)
    win, st_win = all_tables(g, d_blob, cap_bytes, nf, ch, (0, nf))
    for name, a, b in zip(("row_begin", "row_cnt", "row_scale", "row_raw", "row_raw_len"), whole, win):
        assert np.array_equal(a, b), name
    return whole, st_whole, st_win


@pytest.mark.parametrize("rows,ch", SCAN_SHAPES, ids=[f"rows-{r}-{c}ch" for r, c in SCAN_SHAPES])
def test_whole_blob_is_the_window_of_all_frames_at_the_scan_edges(glc_amd, torch, rows, ch):
    """The whole-blob R2 is the window {0, rows} plus the totals check: same five tables, same status, both K.tables."""
    frames = CC.scan_blob(rows, ch)
    buf, nbytes = K.pack(ch, frames)
    (begin, cnt, _, raw, raw_len), st_whole, st_win = whole_and_window(glc_amd, torch, buf[:nbytes], nbytes, rows // ch, ch)
    assert st_whole == st_win == (0, 0, 0)
    want = K.tables(ch, frames)
    assert np.array_equal(begin, want[0]) and np.array_equal(cnt, want[1]) and np.array_equal(raw, want[2])
    assert np.array_equal(raw_len, np.where(want[2] >= 0, FRAME * ch, 0).astype(np.uint64))


def header_fields(buf):
    """(magic, channels, n_frames, n_pairs, n_raw_rows, bytes) of a packed blob."""
    return struct.unpack("<IIQQQQ", buf[:40].tobytes())


def test_whole_blob_and_window_agree_on_damaged_blobs(glc_amd, torch):
    g = glc_amd
    base, ch, nf = CC.stereo_stream(), 2, 8
    clean_buf, clean_bytes = K.pack(ch, base)
    want = K.tables(ch, base)
    n_true = int(want[1].sum())

    # a non-canonical list at row 7: one row rejected, by both, and every other row as in the clean blob
    frames = CC.with_bad_list(base, 7)
    assert all(frames[i // ch][1][i % ch] is base[i // ch][1][i % ch] for i in range(nf * ch) if i != 7)
    assert list(frames[3][1][1].idx) == [3, 40, 40, 900]
    buf, nbytes = K.pack(ch, frames)
    (begin, cnt, _, raw, _), st_whole, st_win = whole_and_window(g, torch, buf, nbytes, nf, ch)
    assert st_whole == st_win == (K.NOT_CANONICAL, 1, 7)
    others = np.arange(nf * ch) != 7                      # the lists in the blob are those of `frames`: row 7 holds 4 pairs
    assert (begin[7], cnt[7]) == (0, 0) and np.all(raw == -1)
    assert np.array_equal(begin[others], K.tables(ch, frames)[0][others]) and np.array_equal(cnt[others], want[1][others])

    # n_pairs one too large with a consistent `bytes`: the totals are the whole-blob launch's business alone
    o_pairs = K.layout(ch, nf)[3]
    buf, nbytes = K.pack(ch, base, n_pairs=n_true + 1, bytes_field=K.align64(o_pairs + 4 * (n_true + 1)))
    hc, hd = header_fields(clean_buf), header_fields(buf)
    assert hd[3] == hc[3] + 1 and hd[5] == K.align64(o_pairs + 4 * hd[3]) and (hd[:3], hd[4]) == (hc[:3], hc[4])
    assert np.array_equal(buf[64:], clean_buf[64:])
    (begin, cnt, _, raw, _), st_whole, st_win = whole_and_window(g, torch, buf, buf.size, nf, ch)
    assert st_whole == (K.PAIR_SUM, 0, 0) and st_win == (0, 0, 0)
    assert np.array_equal(begin, want[0]) and np.array_equal(cnt, want[1]) and np.array_equal(raw, want[2])

    # a bad magic: every row rejected and empty, by both
    buf, nbytes = K.pack(ch, base, magic=K.MAGIC ^ 0x100)
    assert header_fields(buf)[0] != K.MAGIC and header_fields(buf)[1:] == hc[1:] and np.array_equal(buf[64:], clean_buf[64:])
    tables, st_whole, st_win = whole_and_window(g, torch, buf, nbytes, nf, ch)
    assert st_whole == st_win == (K.BAD_HEADER, nf * ch, 0)
    begin, cnt, scale, raw, raw_len = tables
    assert not begin.any() and not cnt.any() and not scale.any() and np.all(raw == -1) and not raw_len.any()


# ------------------------------------------------------------------------------------------ 4: batches

def pool(g, torch, ch):
    """About 8 clips of 5 to 12 frames, raw frames among them (and, mono, one of 70 frames so that 300 crops fill
    more than a round): [(device blob, n_samples, whole decode)]."""
    key = ("pool", ch)
    if key not in _cache:
        enc = ctx(g, "enc")
        xs = [RC.chord(SR, ch, 5 * HOP + 300), RC.chord(SR, ch, 6 * HOP + 77, seed=2), RC.lcg_noise((5 * HOP + 5) * ch),
              RC.chord(SR, ch, 9 * HOP, seed=5), np.concatenate([RC.lcg_noise(4 * HOP * ch, seed=9), RC.chord(SR, ch, 7 * HOP + 1, seed=6)]),
              np.zeros(5 * HOP * ch, F32), RC.chord(SR, ch, 12 * HOP - 9, seed=8), RC.chord(SR, ch, 7 * HOP + 513, seed=11)]
        if ch == 1:
            xs.append(RC.chord(SR, 1, 70 * HOP, seed=12))
        clips = []
        for x in xs:
            x = np.ascontiguousarray(x, F32)
            d_blob, _ = enc.encode_compact_tensor(torch.from_numpy(x).cuda(), ch)
            d_blob = d_blob.clone()
            y, st = whole_decode(g, torch, d_blob, x.size, ch)
            assert clean(st) and y.size == x.size
            clips.append((d_blob, x.size, y))
        _cache[key] = clips[::-1]                        # allocated in this order: the addresses do not ascend
    return _cache[key]


def draw(clips, ch, n_crops, seed, long_bias=False):
    rng = np.random.RandomState(seed)
    entries = []
    for _ in range(n_crops):
        k = 0 if long_bias and rng.rand() < 0.5 else rng.randint(len(clips))       # long_bias: clips[0], whole, every other time
        d_blob, n_samples, y = clips[k]
        n = n_samples // ch
        length = n if long_bias and k == 0 else int(rng.randint(1, n + 1))
        start = int(rng.randint(0, n - length + 1))
        entries.append((d_blob, n_samples, y, start, length))
    return entries


@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
@pytest.mark.parametrize("n_crops", (1, 2, 64))
def test_batch_of_crops(glc_amd, torch, n_crops, planar):
    g = glc_amd
    entries = draw(pool(g, torch, 2), 2, n_crops, seed=100 + n_crops)
    st = decode_crops(g, torch, 2, entries, planar=planar)
    assert all(clean(s) for s in st)
    if n_crops == 64:
        ptrs = [e[0].data_ptr() for e in entries]
        assert len(set(ptrs)) < len(ptrs) and ptrs != sorted(ptrs)      # blobs repeat, addresses do not ascend
        for i in (0, 17, 63):                                          # ... and each crop equals the single-entry call
            assert clean(decode_crops(g, torch, 2, [entries[i]], planar=planar)[0])


@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
def test_batch_of_300_crops_spans_rounds(glc_amd, torch, planar):
    g = glc_amd
    clips = pool(g, torch, 1)
    assert clips[0][1] == 70 * HOP
    entries = draw(clips, 1, 300, seed=300, long_bias=True)
    hops = sum(g.plan_crop(e[1], 1, e[3], e[4]).n_frames + 1 for e in entries)
    assert hops > ROUND + 1                                             # more than one round's budget
    st = decode_crops(g, torch, 1, entries, planar=planar)
    assert all(clean(s) for s in st)


@pytest.mark.parametrize("planar", (True, False), ids=("planar", "interleaved"))
def test_batch_into_a_slice_of_a_bigger_tensor(glc_amd, torch, planar):
    g = glc_amd
    for ch in (2, 3):
        entries = draw(pool(g, torch, ch), ch, 9, seed=9 + ch)
        st = decode_crops(g, torch, ch, entries, planar=planar, margin=2)
        assert all(clean(s) for s in st)


def test_batch_with_a_window_longer_than_a_round(glc_amd, torch):
    """A window of ROUND + 1 frames in the middle of a mono clip takes the long path (the windowed R2 once, then the
    ring rounds), between crops that are packed into ordinary rounds."""
    g = glc_amd
    nf = ROUND + 9
    n = nf * HOP
    t = np.arange(n, dtype=np.float64)
    x = (0.3 * np.sin(2 * np.pi * 440.0 / SR * t) + 0.1 * np.sin(2 * np.pi * 1234.5 / SR * t)).astype(F32)
    d_blob, info = ctx(g, "enc").encode_compact_tensor(torch.from_numpy(x).cuda(), 1)
    assert info.n_frames == nf
    ref, st = whole_decode(g, torch, d_blob, n, 1)
    assert clean(st)
    start, length = 3 * HOP + 100, (ROUND - 1) * HOP + 50
    p = g.plan_crop(n, 1, start, length)
    assert p.n_frames == ROUND + 1 and p.first_frame > 0 and p.first_frame + p.n_frames < nf
    clips = pool(g, torch, 1)
    small = draw(clips, 1, 4, seed=41)
    entries = small[:2] + [(d_blob, n, ref, start, length)] + small[2:]
    for planar in (True, False):
        st = decode_crops(g, torch, 1, entries, planar=planar)
        assert all(clean(s) for s in st)
    # a window of exactly a round's frames stays in an ordinary round
    assert g.plan_crop(n, 1, start, length - HOP).n_frames == ROUND
    assert clean(decode_crops(g, torch, 1, [(d_blob, n, ref, start, length - HOP)])[0])


# ------------------------------------------------------------------------------------------ 5: untrusted blobs

def damaged(g, torch, frames, ch=2, **over):
    """(device buffer of glc_compact_bound bytes, n_samples, the whole-blob call's samples and status) of a blob packed
    with overrides."""
    buf, nbytes = K.pack(ch, frames, **over)
    assert buf.size == g.compact_bound(ch, len(frames))
    d = upload(torch, buf)
    n_samples = K.n_samples_of(ch, len(frames))
    y, st = whole_decode(g, torch, d, n_samples, ch)
    return d, n_samples, y, st


def window_of_frames(g, n_samples, ch, f0, f1):
    """A crop whose window is exactly the frames [f0, f1) (f0 >= 1: f0 is the halo frame of hop f0 + 1)."""
    start = CC.first_sample_of_hop(f0 + 1, ch)
    length = CC.first_sample_of_hop(f1, ch) - start
    p = g.plan_crop(n_samples, ch, start, length)
    assert (p.first_frame, p.n_frames) == (f0, f1 - f0)
    return start, length


def test_bad_magic_gives_silence_and_reports_the_window(glc_amd, torch):
    g = glc_amd
    d, n_samples, y, st = damaged(g, torch, CC.stereo_stream(), magic=K.MAGIC ^ 0x100)
    assert st.flags == K.BAD_HEADER and not bits(y).any()
    start, length = window_of_frames(g, n_samples, 2, 2, 5)
    got = decode_crops(g, torch, 2, [(d, n_samples, y, start, length)])[0]
    assert (got.flags, got.n_bad_rows, got.first_bad_row) == (K.BAD_HEADER, 3 * 2, 2 * 2)


def test_bad_list_inside_in_front_of_and_behind_the_window(glc_amd, torch):
    g = glc_amd
    base = CC.stereo_stream()
    for row, where in ((7, "inside"), (4, "halo"), (3, "in front"), (10, "behind")):
        d, n_samples, y, st = damaged(g, torch, CC.with_bad_list(base, row))
        assert (st.flags, st.n_bad_rows, st.first_bad_row) == (K.NOT_CANONICAL, 1, row)
        start, length = window_of_frames(g, n_samples, 2, 2, 5)      # rows 4 .. 9
        got = decode_crops(g, torch, 2, [(d, n_samples, y, start, length)])[0]   # the slice of the whole-blob call
        if where in ("inside", "halo"):
            assert (got.flags, got.n_bad_rows, got.first_bad_row) == (K.NOT_CANONICAL, 1, row), where
        else:
            assert clean(got), where


def test_inflated_cnt_in_front_pushes_the_window_behind_n_pairs(glc_amd, torch):
    g = glc_amd
    base = CC.stereo_stream()
    n_true = sum(len(r.idx) for _, body in base for r in body)
    assert n_true < HOP
    d, n_samples, y, st = damaged(g, torch, base, cnt_set={1: HOP})     # every later row now begins behind n_pairs
    assert st.flags & K.ROW_BOUNDS
    start, length = window_of_frames(g, n_samples, 2, 2, 5)
    got = decode_crops(g, torch, 2, [(d, n_samples, y, start, length)])[0]
    assert (got.flags, got.n_bad_rows, got.first_bad_row) == (K.ROW_BOUNDS, 6, 4)
    # ... and a window of frame 0 alone sees the inflated row itself, and nothing of what it does behind it
    got = decode_crops(g, torch, 2, [(d, n_samples, y, 0, 100)])[0]
    assert (got.flags, got.n_bad_rows, got.first_bad_row) == (K.ROW_BOUNDS, 1, 1)


def test_pair_sum_is_not_reported_by_crops(glc_amd, torch):
    g = glc_amd
    base = CC.stereo_stream()
    n_true = sum(len(r.idx) for _, body in base for r in body)
    o_pairs = K.layout(2, len(base))[3]
    d, n_samples, y, st = damaged(g, torch, base, n_pairs=n_true + 1, bytes_field=K.align64(o_pairs + 4 * (n_true + 1)))
    assert (st.flags, st.n_bad_rows) == (K.PAIR_SUM, 0)
    for start, length in ((0, n_samples // 2), window_of_frames(g, n_samples, 2, 2, 5)):
        assert clean(decode_crops(g, torch, 2, [(d, n_samples, y, start, length)])[0])


def test_damaged_entry_leaves_its_neighbours_alone(glc_amd, torch):
    g = glc_amd
    clips = pool(g, torch, 2)
    d, n_samples, y, _ = damaged(g, torch, CC.with_bad_list(CC.stereo_stream(), 7))
    start, length = window_of_frames(g, n_samples, 2, 2, 5)
    good = draw(clips, 2, 4, seed=55)
    entries = good[:2] + [(d, n_samples, y, start, length)] + good[2:]
    st = decode_crops(g, torch, 2, entries, planar=False)
    assert [clean(s) for s in st] == [True, True, False, True, True]
    assert (st[2].flags, st[2].n_bad_rows, st[2].first_bad_row) == (K.NOT_CANONICAL, 1, 7)


# ------------------------------------------------------------------------------------------ 6: the call's edges

def raw_call(g, dec, blobs, sizes, ns, crops, d_out, lay):
    b = len(sizes)
    L = g._lib
    return g.lib.glc_decode_crops_device_compact(
        dec._h, (C.c_void_p * b)(*blobs) if blobs is not None else None, (C.c_uint64 * b)(*sizes), (C.c_uint64 * b)(*ns),
        (L.GlcCrop * b)(*[L.GlcCrop(s, l) for s, l in crops]) if crops is not None else None, C.c_void_p(d_out), C.byref(lay))


def test_arguments_refused_before_anything_is_queued(glc_amd, torch):
    g = glc_amd
    L = g._lib
    dec = ctx(g, "dec", 2)
    buf, nbytes = K.pack(2, CC.stereo_stream())
    store = torch.zeros(buf.size + 4 * 3000, dtype=torch.uint8, device="cuda")     # the blob, and room behind it
    store[:buf.size] = torch.from_numpy(buf).cuda()
    d = store[:nbytes]
    n_samples = K.n_samples_of(2, 8)
    n = n_samples // 2
    out = nan_tensor(torch, (2, 600, 2))
    torch.cuda.synchronize()
    lens = (C.c_uint64 * 2)(500, 600)
    lay = lambda n_clips=2, ch=2, planar=0, cs=1200, chs=0, lengths=lens: L.GlcClipLayout(
        n_clips, ch, planar, cs, chs, 600, C.cast(lengths, C.POINTER(C.c_uint64)) if lengths is not None else None)
    P, S, N = [d.data_ptr()] * 2, [nbytes] * 2, [n_samples] * 2
    ok_crops = [(10, 500), (n - 600, 600)]
    o = out.data_ptr()
    o_pairs = K.layout(2, 8)[3]
    refused = [
        raw_call(g, dec, P, S, N, [(10, 0), (0, 600)], o, lay(lengths=(C.c_uint64 * 2)(0, 600))),      # length == 0
        raw_call(g, dec, P, S, N, [(10, 500), (n - 599, 600)], o, lay()),                              # ends behind the clip
        raw_call(g, dec, P, S, N, [(10, 500), (2 ** 64 - 300, 600)], o, lay()),                        # the sum wraps
        raw_call(g, dec, P, S, N, [(10, 499), (n - 600, 600)], o, lay()),                              # the layout's length differs
        raw_call(g, dec, P, S, N, [(10, 500), (0, 600)], o, lay(lengths=None, cs=1200)),               # ... with one length for all
        raw_call(g, dec, P, S, N, ok_crops, store.data_ptr() + 64, lay()),                             # the output overlaps a blob
        raw_call(g, dec, P, S, N, ok_crops, store.data_ptr() + nbytes - 4, lay()),
        raw_call(g, dec, None, S, N, ok_crops, o, lay()),                                              # what the batch call refuses
        raw_call(g, dec, P, S, N, None, o, lay()),
        raw_call(g, dec, [P[0], 0], S, N, ok_crops, o, lay()),
        raw_call(g, dec, [P[0], P[1] + 32], S, N, ok_crops, o, lay()),
        raw_call(g, dec, P, [nbytes, o_pairs - 1], N, ok_crops, o, lay()),
        raw_call(g, dec, P, S, [n_samples, 2 * 512], ok_crops, o, lay()),
        raw_call(g, dec, P, S, N, ok_crops, o, lay(ch=0)),
        raw_call(g, dec, P, S, N, ok_crops, o + 2, lay()),
        raw_call(g, dec, P, S, N, ok_crops, o, lay(cs=1199)),                                          # a clip overlaps the next
        raw_call(g, dec, P, S, N, ok_crops, o, lay(planar=1, cs=1200, chs=599)),                       # a plane overlaps the next
        g.lib.glc_decode_crops_device_compact(dec._h, None, None, None, None, C.c_void_p(o), None),
    ]
    assert refused == [EINVAL] * len(refused)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy().view(np.uint32) == NAN_BITS)
    # no clips: nothing to do
    assert g.lib.glc_decode_crops_device_compact(dec._h, None, None, None, None, None, C.byref(L.GlcClipLayout(0, 2, 1, 0, 0, 0, None))) == 0
    # ... and the accepted form of the same call
    assert raw_call(g, dec, P, S, N, ok_crops, o, lay()) == 0
    dec.synchronize()
    y, _ = whole_decode(g, torch, d, n_samples, 2)
    want = CC.want_crops((2, 600, 2), False, 0, 2, [(y, 10, 500), (y, n - 600, 600)])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    st = (L.GlcCompactStatus * 2)()
    assert g.lib.glc_decode_compact_last_status(dec._h, st, 2) == 0
    assert g.lib.glc_decode_compact_last_status(dec._h, st, 1) == EINVAL          # one status per crop


def test_context_state_and_a_smaller_second_call(glc_amd, torch):
    """No stream is resident afterwards; a glc_decode that follows is what it always was; a second call with a smaller
    batch on the same context (workspaces reused, one status per crop of THAT call)."""
    g = glc_amd
    dec = g.Decoder(2, SR)
    x = RC.chord(SR, 2, 4 * HOP + 100)
    stream = ctx(g, "enc").encode(x, 2)
    before = dec.decode(stream).copy()
    assert g.lib.glc_ctx_resident_stream(dec._h) != 0
    clips = pool(g, torch, 2)
    for n_crops in (40, 3):
        entries = draw(clips, 2, n_crops, seed=70 + n_crops)
        out = nan_tensor(torch, (n_crops, 2, max(e[4] for e in entries)))
        dec.decode_compact_crops_tensor([e[0] for e in entries], [e[1] for e in entries], [e[3] for e in entries],
                                        [e[4] for e in entries], out=out)
        torch.cuda.synchronize()
        assert g.lib.glc_ctx_resident_stream(dec._h) == 0
        want = CC.want_crops(tuple(out.shape), True, 0, 2, [(e[2], e[3], e[4]) for e in entries])
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
        st = dec.last_compact_status()
        assert len(st) == n_crops and all(clean(s) for s in st)
    assert np.array_equal(bits(dec.decode(stream)), bits(before))
    dec.close()


def test_tensor_call_allocates_and_takes_one_length(glc_amd, torch):
    g = glc_amd
    dec = ctx(g, "dec", 2)
    clips = pool(g, torch, 2)[:3]
    starts = [0, 700, 1]
    for planar in (True, False):
        out = dec.decode_compact_crops_tensor([c[0] for c in clips], [c[1] for c in clips], starts, 2000, planar=planar)
        torch.cuda.synchronize()
        assert tuple(out.shape) == ((3, 2, 2000) if planar else (3, 2000, 2))
        want = CC.want_crops(tuple(out.shape), planar, 0, 2, [(c[2], s, 2000) for c, s in zip(clips, starts)])
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    # lengths that differ: the padding of a tensor the call allocated is +0.0
    out = dec.decode_compact_crops_tensor([c[0] for c in clips], [c[1] for c in clips], starts, [5, 2000, 1])
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert tuple(host.shape) == (3, 2, 2000) and not host[0, :, 5:].view(np.uint32).any() and not host[2, :, 1:].view(np.uint32).any()
    assert np.array_equal(bits(host[0, :, :5].T).reshape(-1), bits(clips[0][2])[:10])
    with pytest.raises(g.GlcError) as e:
        dec.decode_compact_crops_tensor([clips[0][0]], [clips[0][1]], [0], 0)
    assert e.value.code == EINVAL
    with pytest.raises(g.GlcError):
        dec.decode_compact_crops_tensor([clips[0][0]], [clips[0][1]], [0, 1], 5)
    assert len(dec.last_compact_status()) == 3
