"""The host twin of the cut, glc_compact_cut (include/glc.h), against the numpy model of tests/store_cut_cases.py: the
same bytes on every edge case, the pieces of a partition join back to the clip, the codec reads a piece as the frames it
was cut from, and the same refusals.  No GPU: everything here is a host call.  (The argument rules of the device call
need a context, which needs a device: tests/test_store_cut.py holds them.)"""
import ctypes as C
import struct

import numpy as np
import pytest

import store_cut_cases as K
import store_join_cases as J


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    assert hasattr(g.lib, "glc_compact_cut") and hasattr(g.lib, "glc_store_cut_device")
    return g


CASES = K.edge_cases()
PARTS = K.partitions()


def pieces_of(g, blob, ch, frames):
    out, f0 = [], 0
    for nf in frames:
        out.append(g.compact_cut(blob, f0, nf, ch))
        f0 += nf
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cut_equals_the_model(glc_amd, case):
    seen = set()
    for clip, f0, nf in case["cuts"]:
        if (clip, f0, nf) in seen:
            continue
        seen.add((clip, f0, nf))
        bits, want = K.cut(case["clips"][clip], case["ch"], f0, nf)
        assert bits == 0
        got = glc_amd.compact_cut(case["clips"][clip], f0, nf, case["ch"])
        assert got == want, (case["name"], clip, f0, nf)
        assert K.cut(got, case["ch"], 0, nf) == (0, got)                    # the whole of a piece is the piece
        assert J.segment_status(got, case["ch"], nf) == 0                   # the join's segment rule
    blob = case["clips"][0]
    assert glc_amd.compact_cut(blob, 0, J.parse_header(blob)[2]) == blob    # the channel count from the header; the whole clip


@pytest.mark.parametrize("part", PARTS, ids=[p[0] for p in PARTS])
def test_cut_then_join_is_the_clip(glc_amd, part):
    _, ch, blob, frames = part
    pieces = pieces_of(glc_amd, blob, ch, frames)
    assert glc_amd.compact_join(pieces, ch) == blob
    assert J.join(pieces, ch) == blob


def glc_frame_spans(data: bytes, ch: int):
    """The byte range of every frame of a serialised stream (the container format: a 22-byte head, the frames, a 16-byte
    tail; a frame is its lists, its scales, the raw tag and, behind a set tag, its samples)."""
    n_frames = struct.unpack_from("<Q", data, 14)[0]
    at, spans = 22, []
    for _ in range(n_frames):
        start = at
        n_lists = struct.unpack_from("<Q", data, at)[0]
        at += 8
        for _ in range(n_lists):
            at += 8 + 4 * struct.unpack_from("<Q", data, at)[0]
        at += 8 + 4 * struct.unpack_from("<Q", data, at)[0]
        tag = data[at]
        at += 1
        if tag:
            at += 8 + 2 * struct.unpack_from("<Q", data, at)[0]
        spans.append((start, at))
    assert at + 16 == len(data)
    return spans


@pytest.mark.parametrize("part", PARTS, ids=[p[0] for p in PARTS])
def test_the_codec_reads_a_piece(glc_amd, part):
    """EncodedAudio.from_compact of a piece serialises to the bytes of the same frames of the whole clip's .glc, and the
    pieces in frame order assemble to the stream the whole blob assembles to."""
    g = glc_amd
    _, ch, blob, frames = part
    F = sum(frames)
    n = J.clip_length(F) * ch
    assert g.plan_encode(n, ch).n_frames == F
    whole = g.EncodedAudio.from_compact(44100, n, ch, [blob]).to_bytes()
    spans = glc_frame_spans(whole, ch)
    pieces = pieces_of(g, blob, ch, frames)
    assert g.EncodedAudio.from_compact(44100, n, ch, pieces).to_bytes() == whole
    f0 = 0
    for nf, piece in zip(frames, pieces):
        n_piece = J.clip_length(nf) * ch
        assert g.plan_encode(n_piece, ch).n_frames == nf
        got = g.EncodedAudio.from_compact(44100, n_piece, ch, [piece]).to_bytes()
        assert got[22:-16] == whole[spans[f0][0]:spans[f0 + nf - 1][1]], (part[0], f0, nf)
        f0 += nf


def _raw_call(g, blob, ch, f0, nf, cap=1 << 20):
    """glc_compact_cut itself: (rc, info.bytes, message, the output buffer's bytes)."""
    held = np.frombuffer(blob + bytes(-len(blob) % 8), np.uint64)
    info = g._lib.GlcCompactInfo()
    out = np.zeros(cap // 8 + 1, np.uint64)
    rc = g.lib.glc_compact_cut(held.ctypes.data_as(C.c_void_p), len(blob), ch, f0, nf, out.ctypes.data_as(C.c_void_p), cap, C.byref(info))
    return rc, int(info.bytes), (g.lib.glc_last_error(None) or b"").decode(), out.view(np.uint8)


@pytest.mark.parametrize("kind", K.HEADER_DAMAGE + K.WINDOW_DAMAGE)
def test_damage_is_refused_by_name(glc_amd, kind):
    g = glc_amd
    blob, f0, nf = K.damage_clip(np.random.default_rng(5))
    assert K.cut(blob, 2, f0, nf)[0] == 0
    bad, bits, word = K.damaged(blob, kind, 2, f0, nf)
    assert K.cut(bad, 2, f0, nf) == (bits, None) and bits != 0
    rc, size, msg, out = _raw_call(g, bad, 2, f0, nf)
    assert rc == g._lib.GLC_EINVAL and size == 0 and msg.startswith("glc_compact_cut: ") and word in msg, msg
    assert not out.any()
    with pytest.raises(g.GlcError):
        g.compact_cut(bad, f0, nf, 2)


def test_a_window_beyond_the_frames_and_no_frames_are_refused(glc_amd):
    g = glc_amd
    blob, _, _ = K.damage_clip(np.random.default_rng(5))
    for f0, nf in ((0, 10), (9, 1), (5, 5), (10, 0x7FFFFFFF), (2 ** 64 - 1, 2), (3, 2 ** 64 - 2)):
        assert K.cut(blob, 2, f0, nf)[0] == K.BAD_CROP
        rc, size, msg, _ = _raw_call(g, blob, 2, f0, nf)
        assert rc == g._lib.GLC_EINVAL and size == 0 and "window" in msg, (f0, nf, msg)
    rc, size, msg, _ = _raw_call(g, blob, 2, 3, 0)
    assert rc == g._lib.GLC_EINVAL and size == 0 and "no frames" in msg


@pytest.mark.parametrize("kind", K.BEHIND)
def test_damage_behind_the_window_does_not_refuse(glc_amd, kind):
    g = glc_amd
    blob, f0, nf = K.damage_clip(np.random.default_rng(5))
    bad, bits, _ = K.damaged(blob, kind, 2, f0, nf)
    assert bits == 0 and bad != blob
    want = K.cut(blob, 2, f0, nf)
    assert K.cut(bad, 2, f0, nf) == want
    assert g.compact_cut(bad, f0, nf, 2) == want[1]
    with pytest.raises(g.GlcError):                                  # a window that reaches the damage is refused
        g.compact_cut(bad, f0, nf + 1, 2)
    assert K.cut(bad, 2, f0, nf + 1)[0] == (K.ROW_BOUNDS if kind == "cnt_behind" else K.RAW_RANGE)


def test_a_frame_count_that_wraps_the_sizes_is_refused(glc_amd):
    """A 64-byte blob whose header says n_frames = 2^64 - 64 (mono, 144 pairs, bytes = 64): every section offset formed
    from that count wraps, the size comes out as 64 and the header rule alone would pass it - and the sums over cnt and
    is_raw would then run far outside the blob.  The frame count is bounded before the rule is asked."""
    g = glc_amd
    for F, n_pairs in ((2 ** 64 - 64, 144), (2 ** 64 - 1, 0), (2 ** 32, 0), (2 ** 63, 0), (0, 0)):
        crafted = struct.pack("<IIQQQQ", J.MAGIC, 1, F, n_pairs, 0, 64) + bytes(24)
        assert K.cut(crafted, 1, 0, 1)[0] == K.BAD_HEADER
        for f0, nf in ((0, 1), (5, 3), (2 ** 63, 2 ** 62)):
            rc, size, msg, out = _raw_call(g, crafted, 1, f0, nf, cap=1 << 16)
            assert rc == g._lib.GLC_EINVAL and size == 0 and "frame count" in msg, (F, msg)
            assert not out.any()
        with pytest.raises(g.GlcError):
            g.compact_cut(crafted, 0, 1)


def test_a_cap_one_short_is_refused_with_the_size(glc_amd):
    g = glc_amd
    blob, f0, nf = K.damage_clip(np.random.default_rng(6), 3)
    need = len(K.cut(blob, 3, f0, nf)[1])
    rc, size, msg, out = _raw_call(g, blob, 3, f0, nf, cap=need - 1)
    assert rc == g._lib.GLC_EINVAL and size == need and "smaller" in msg and not out.any()
    rc, size, _, out = _raw_call(g, blob, 3, f0, nf, cap=need)
    assert rc == 0 and size == need and out[:need].tobytes() == K.cut(blob, 3, f0, nf)[1]


def test_the_signatures_are_declared(glc_amd):
    for name in ("glc_store_cut_device", "glc_compact_cut"):
        assert name in glc_amd._lib.SIGNATURES
    for cls in (glc_amd.Encoder, glc_amd.Decoder, glc_amd.StreamEncoder):
        assert callable(getattr(cls, "cut_clips_tensor"))
    assert callable(glc_amd.compact_cut)
