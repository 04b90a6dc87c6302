"""Every round driver ON the edge of a round: a batch whose slots add up to exactly the round's budget - one round -
and the same batch with its last clip one frame longer - two.  The multi-round tests of the other suites overshoot a
round by a wide margin; an off-by-one in how a driver sizes or addresses what pack_rounds (csrc/glc_rounds.hpp)
returns would show here.  tests/test_round_plan.py pins the packer itself on the host.

A clip of n frames costs n + 1 slots.  Stereo budgets: 4096 slots for the encode-side drivers,
kDecodeChunkFrames + 1 = 4097 for the decode-side ones, and 4096 with one slot in front of every round for the
streaming push.  64 clips, 63 of them of 63 frames; the last one is varied.  Frame counts are the oracle's
(O.num_frames), and each test first asserts the slot sums it relies on.

The expectation is the library's own: every clip's output is byte-equal - no tolerance - to that of the same clip sent
through a call of its own, which the other suites hold to the oracle.  tests/test_batch.py has no batch at this edge
for glc_encode_batch / glc_decode_batch (its only round-sized clip is 37 frames longer than a round), so they are
pinned here as well.  The test cannot see how many rounds ran and need not."""
import numpy as np
import pytest

import conftest as cf
import roundtrip_cases as RC
from conftest import O

pytestmark = pytest.mark.gpu

SR, CH, HOP = 44100, 2, 1024
F32 = np.float32
N_CLIPS, FRAMES = 64, 63
ENCODE_BUDGET, DECODE_BUDGET, STREAM_FRONT = 4096, 4097, 1
EDGES = ("one-round", "one-frame-more")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    import glc_amd
    yield torch, glc_amd
    _ctx.clear()             # contexts: released while the library is still loaded
    _own.clear()


_ctx, _clips, _own = {}, {}, {}


def ctx(g, kind):
    if kind not in _ctx:
        _ctx[kind] = {"enc": lambda: g.Encoder(SR), "dec": lambda: g.Decoder(CH, SR), "rt": lambda: g.RoundTrip(SR)}[kind]()
    return _ctx[kind]


def clip(n_frames, seed):
    """`n_frames` frames of chord and noise segments (compressed and raw frames), made once per (frames, seed)."""
    if (n_frames, seed) not in _clips:
        seg = np.concatenate([cf.gen_chord(SR, CH, 3 * HOP, seed=seed), RC.lcg_noise(2 * HOP * CH, seed=seed)])
        x = np.resize(seg, (n_frames * HOP - 100) * CH).astype(F32)
        assert O.num_frames(x.size, CH) == n_frames
        _clips[(n_frames, seed)] = x
    return _clips[(n_frames, seed)]


def batch(budget, front, edge):
    """[(key, samples)]: 63 clips of 63 frames of three kinds and a last one that fills `budget` slots behind `front`
    exactly, or is one frame longer."""
    last = budget - front - (N_CLIPS - 1) * (FRAMES + 1) - 1 + EDGES.index(edge)
    keys = [(FRAMES, 1 + i % 3) for i in range(N_CLIPS - 1)] + [(last, 4)]
    slots = front + sum(O.num_frames(clip(*k).size, CH) + 1 for k in keys)
    assert slots == budget + EDGES.index(edge), "the batch does not sit on the edge of a round"
    return [(k, clip(*k)) for k in keys]


def own(driver, key, make):
    """What `driver` gives for the clip `key` in a call of its own, computed once."""
    if (driver, key) not in _own:
        _own[(driver, key)] = make()
    return _own[(driver, key)]


def padded(torch, clips):
    """The clips as one planar (B, C, T) device tensor, NaN behind the short ones -> (x, lengths)."""
    lens = [x.size // CH for x in clips]
    host = np.full((len(clips), CH, max(lens)), np.nan, F32)
    for i, x in enumerate(clips):
        host[i, :, :lens[i]] = x.reshape(lens[i], CH).T
    return torch.from_numpy(host).cuda(), lens


def words(t):
    return t.contiguous().cpu().numpy().view(np.uint32)


def blobs_of(torch, arena, entries):
    """The bytes of every stored blob of `entries`, in their order."""
    torch.cuda.synchronize()
    a, out = arena.cpu().numpy(), []
    for e in entries.cpu().numpy():
        assert e[3] >> 32 == 1, "a blob was not stored"
        out.append(a[int(e[0]):int(e[0] + e[1])].tobytes())
    return out


@pytest.mark.parametrize("edge", EDGES)
def test_roundtrip_batch_device(gpu, edge):
    torch, g = gpu
    rt = ctx(g, "rt")
    b = batch(ENCODE_BUDGET, 0, edge)

    def alone(x):
        t, lens = padded(torch, [x])
        return words(rt.apply_batch_tensor(t, lengths=lens))

    x, lens = padded(torch, [c for _, c in b])
    got = rt.apply_batch_tensor(x, lengths=lens)
    torch.cuda.synchronize()
    for i, (key, c) in enumerate(b):
        assert np.array_equal(words(got[i:i + 1, :, :lens[i]]), own("rtb", key, lambda: alone(c))), i
    assert not got[:, :, min(lens):].isnan().any()           # the padding of a new output is zero, never the input's


@pytest.mark.parametrize("edge", EDGES)
def test_encode_batch_device_compact(gpu, edge):
    torch, g = gpu
    enc = ctx(g, "enc")
    b = batch(ENCODE_BUDGET, 0, edge)

    def alone(x):
        t, lens = padded(torch, [x])
        arena, _, entries = enc.encode_compact_batch_tensor(t, lengths=lens)
        return blobs_of(torch, arena, entries)[0]

    x, lens = padded(torch, [c for _, c in b])
    arena, cursor, entries = enc.encode_compact_batch_tensor(x, lengths=lens)
    got = blobs_of(torch, arena, entries)
    assert len(got) == len(b)
    for i, (key, c) in enumerate(b):
        assert got[i] == own("ebc", key, lambda: alone(c)), i
    e = entries.cpu().numpy()
    assert int(cursor.item()) == int(e[-1, 0] + e[-1, 1]) and np.all(e[1:, 0] == e[:-1, 0] + e[:-1, 1])  # back to back


@pytest.mark.parametrize("edge", EDGES)
def test_decode_batch_device_compact(gpu, edge):
    torch, g = gpu
    enc, dec = ctx(g, "enc"), ctx(g, "dec")
    b = batch(DECODE_BUDGET, 0, edge)
    blob = {key: own("blob", key, lambda: enc.encode_compact_tensor(torch.from_numpy(c).cuda(), CH)[0]) for key, c in b}

    def alone(key, x):
        return words(dec.decode_compact_batch_tensor([blob[key]], [x.size]))

    got = dec.decode_compact_batch_tensor([blob[key] for key, _ in b], [c.size for _, c in b])
    torch.cuda.synchronize()
    for i, (key, c) in enumerate(b):
        assert np.array_equal(words(got[i:i + 1, :, :c.size // CH]), own("cdb", key, lambda: alone(key, c))), i
    assert all((s.flags, s.n_bad_rows) == (0, 0) for s in dec.last_compact_status())


@pytest.mark.parametrize("edge", EDGES)
def test_encode_batch_and_decode_batch(gpu, edge):
    """The host calls: glc_encode_batch packs 4096 slots, glc_decode_batch 4097 - one batch each."""
    torch, g = gpu
    enc, dec = ctx(g, "enc"), ctx(g, "dec")
    b = batch(ENCODE_BUDGET, 0, edge)
    got = enc.encode_batch([c for _, c in b], CH)
    assert len(got) == len(b)
    for i, (key, c) in enumerate(b):
        assert got[i].to_bytes() == own("encode", key, lambda: enc.encode(c, CH).to_bytes()), i
    b = batch(DECODE_BUDGET, 0, edge)
    streams = [own("stream", key, lambda: enc.encode(c, CH)) for key, c in b]
    out = dec.decode_batch(streams)
    assert len(out) == len(b)
    for i, (key, c) in enumerate(b):
        assert np.array_equal(out[i].view(np.uint32), own("decode", key, lambda: dec.decode(streams[i]).copy().view(np.uint32))), i


@pytest.mark.parametrize("edge", EDGES)
def test_stream_push_device(gpu, edge):
    """One push that finishes 64 fresh lanes: a segment per lane, every round with its one slot in front."""
    torch, g = gpu
    b = batch(ENCODE_BUDGET, STREAM_FRONT, edge)

    def push(clips):
        se = g.StreamEncoder(SR, CH, n_streams=len(clips))
        x, lens = padded(torch, clips)
        arena = torch.zeros(g.compact_store_bound(CH, lens) + 4096 * len(clips), dtype=torch.uint8, device="cuda")
        cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
        entries, segs = se.push_tensor(x, lens, [True] * len(clips), arena, cursor)
        return blobs_of(torch, arena, entries), segs

    got, segs = push([c for _, c in b])
    assert [(lane, f0) for lane, f0, _ in segs] == [(i, 0) for i in range(len(b))]
    assert STREAM_FRONT + sum(nf + 1 for _, _, nf in segs) == ENCODE_BUDGET + EDGES.index(edge)
    for i, (key, c) in enumerate(b):
        assert got[i] == own("push", key, lambda: push([c])[0][0]), i
