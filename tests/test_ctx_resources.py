"""What a context holds of the device is released with it (csrc/glc_resources.hpp; include/glc_debug.h
glc_debug_live_resources): device buffers, pinned buffers, streams of the library's own and events are counted where
they are created and destroyed, and after glc_stream_enc_close + glc_ctx_destroy the four counts are EXACTLY what they
were before glc_ctx_create - whatever ran in between, and also when the only call was a refused one.

One fresh 48 kHz context per cycle is driven through every family that creates handles lazily: a screened range encode
that takes the edge path (side stream, its events, the edge coefficients), a glc_encode of several rounds (helper threads,
stream_b, the copy and download streams, slot 1), a decode, a streaming decode session left open, the batch round trip,
the batch encode into a store, the store's compaction, and two stream encoders - one session takes host pushes or device
pushes, not both, so there is one of each on the context.  While the context lives every count must have gone up: that is
what shows the cycle reaches the handles."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctx_sequence_cases as Q  # noqa: E402

SR, HOP = 48000, Q.HOP
EINVAL = -1
KINDS = ("device buffers", "pinned buffers", "streams", "events")


def tone(ch, frames):
    """Interleaved float32 of `frames` frames (frames * 1024 + 100 samples per channel): a chord, one pitch per channel."""
    n = frames * HOP + 100
    t = np.arange(n, dtype=np.float64) / SR
    x = np.stack([0.3 * np.sin(2 * np.pi * (440.0 + 97.0 * c) * t) + 0.1 * np.sin(2 * np.pi * (3001.0 + 13.0 * c) * t) for c in range(ch)], 1)
    return np.ascontiguousarray(x.astype(np.float32).reshape(-1))


_inputs = {}


def inputs():
    """Computed once, shared by the cycles, never written."""
    if not _inputs:
        _inputs.update(range300=tone(2, 300), rounds=tone(2, 4 * 1024 + 300),
                       clips=[Q.item(2, n).x for n in ("tonal9", "noise5", "mixed13", "tonal130")])
    return _inputs


def live(g):
    c = (C.c_uint64 * 4)()
    assert g.lib.glc_debug_live_resources(c) == 0
    return tuple(int(v) for v in c)


def view(cls, owner, **kw):
    """The context of `owner` seen as another class of the package: the same handle, nothing of its own."""
    v = object.__new__(cls)
    v.__dict__.update(_h=owner._h, sample_rate=owner.sample_rate, device=owner.device, **kw)
    return v


def padded(torch, clips, ch):
    """(B, T, C) float32 CUDA tensor of the clips, zero behind each, and their samples per channel."""
    lens = [c.size // ch for c in clips]
    x = np.zeros((len(clips), max(lens), ch), np.float32)
    for i, c in enumerate(clips):
        x[i, :lens[i]] = c.reshape(-1, ch)
    return torch.from_numpy(x).cuda(), lens


def use_everything(torch, g, ctx):
    """Every family once on `ctx`; returns the open stream encoders (handles) and what must stay alive until they close."""
    L, h, I = g.lib, ctx._h, inputs()
    views = []

    def as_(cls, **kw):
        views.append(view(cls, ctx, **kw))
        return views[-1]
    enc, dec, rt = as_(g.Encoder), as_(g.Decoder, channels=2), as_(g.RoundTrip)

    # screened range encode, forced on: 300 stereo frames hold 4 edge rows, so the launch takes the side stream
    assert L.glc_debug_set_encode_screen(h, 2) == 0
    x = torch.from_numpy(I["range300"]).cuda()
    rec = torch.zeros(300 * int(L.glc_record_bytes(2)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    enc.encode_range_device(x.data_ptr(), 0, x.numel() // 2, x.numel(), 2, 0, 300, rec.data_ptr())
    ctx.synchronize()
    launches, rows = C.c_uint64(), C.c_uint64()
    assert L.glc_debug_encode_edge_stats(h, C.byref(launches), C.byref(rows)) == 0
    assert (launches.value, rows.value) == (1, 4), "the range encode did not take the edge path"
    assert L.glc_debug_set_encode_screen(h, 0) == 0

    # glc_encode of several rounds: the helper threads and the three other streams
    whole = enc.encode(I["rounds"], 2)
    assert whole.info().n_frames == 4 * 1024 + 300

    # decode, and a streaming session that is never finished
    stream = enc.encode(I["clips"][3], 2)
    assert dec.decode(stream).size == I["clips"][3].size
    assert L.glc_decode_stream_begin(h, stream._h) == 0

    # batch round trip, batch encode into a store, the store's compaction
    xb, lens = padded(torch, I["clips"], 2)
    rt.apply_batch_tensor(xb, lengths=lens, planar=False)
    arena, cursor, entries = enc.encode_compact_batch_tensor(xb, lengths=lens, planar=False)
    keep = torch.tensor([1, 0, 1, 1], dtype=torch.uint8, device="cuda")
    ctx.compact_store_tensor(arena, entries, None, keep)

    # two stream encoders on the context: host pushes, device pushes
    sessions = []
    for _ in range(2):
        s = C.c_void_p()
        assert L.glc_stream_enc_open(h, 2, 1, C.byref(s)) == 0
        sessions.append(s)
    host = as_(g.StreamEncoder, channels=2, n_streams=1, _s=sessions[0])
    host.push(I["clips"][0], finish=True)
    assert host.encoded().info().n_frames == 9
    devp = as_(g.StreamEncoder, channels=2, n_streams=1, _s=sessions[1])
    chunk = xb[0:1, :lens[0]].contiguous()
    arena2 = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    _, segs = devp.push_tensor(chunk, None, [1], arena2, torch.zeros(1, dtype=torch.int64, device="cuda"), planar=False)
    assert segs == [(0, 0, 9)]
    ctx.synchronize()
    torch.cuda.synchronize()
    for v in views:  # a view owns nothing: its finaliser must find nothing to close
        v.__dict__.update(_h=None, _s=None)
    return sessions


@pytest.mark.gpu
def test_a_context_releases_everything_it_created():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    g = Q.G()
    inputs()
    gc.collect()  # no forgotten context of an earlier test may be finalised in the middle of this one
    before = live(g)
    for cycle in range(3):
        ctx = g.Encoder(SR)
        sessions = use_everything(torch, g, ctx)
        alive = live(g)
        for k, name in enumerate(KINDS):
            assert alive[k] > before[k], f"cycle {cycle}: the context holds no {name}: {alive} against {before}"
        for s in sessions:
            g.lib.glc_stream_enc_close(s)
        ctx.close()
        assert live(g) == before, f"cycle {cycle}: (device, pinned, streams, events) {live(g)} after destroy, {before} before create"


@pytest.mark.gpu
def test_a_refused_call_leaves_nothing_behind():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    g = Q.G()
    gc.collect()
    before = live(g)
    ctx = g.Encoder(SR)
    created = live(g)
    x = torch.zeros(2 * (9 * HOP + 100), dtype=torch.float32, device="cuda")
    rec = torch.zeros(9 * int(g.lib.glc_record_bytes(2)), dtype=torch.uint8, device="cuda")
    rc = g.lib.glc_encode_range_device(ctx._h, C.c_void_p(x.data_ptr()), 0, x.numel() // 2, x.numel(), 2, 0, 10,
                                       C.c_void_p(rec.data_ptr()), None)  # 10 frames of a stream of 9
    assert rc == EINVAL
    assert live(g) == created, "a refused call allocated"
    ctx.close()
    assert live(g) == before
