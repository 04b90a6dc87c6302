"""The host twin of the segment join, glc_compact_join (include/glc.h), against the numpy model of
tests/store_join_cases.py: the same bytes on every edge case, the same refusals, and the same stream out of
glc_frames_from_compact whether it is given the segments or their join.  No GPU: everything here is a host call.
(The argument rules of the device call need a context, which needs a device: tests/test_store_join.py holds them.)"""
import ctypes as C

import numpy as np
import pytest

import store_join_cases as J


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    assert hasattr(g.lib, "glc_compact_join") and hasattr(g.lib, "glc_store_join_segments_device")
    return g


CASES = J.edge_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_join_equals_the_model(glc_amd, case):
    for k, blobs in enumerate(case["clips"]):
        want = J.join(blobs, case["ch"])
        got = glc_amd.compact_join(blobs, case["ch"])
        assert got == want, (case["name"], "clip", k)
        assert glc_amd.compact_join(blobs) == want          # the channel count from the first header
        if len(blobs) == 1:
            assert got == blobs[0]                      # one segment: the join is the segment itself


def test_model_blobs_are_what_the_codec_reads(glc_amd):
    """The builder's blobs are blobs: glc_frames_from_compact takes them, and the stream it assembles from the
    segments serialises to the bytes of the stream it assembles from their join."""
    for case in CASES:
        if case["name"].startswith("clips_1500") or case["name"] == "segments_1500":
            continue
        ch = case["ch"]
        for blobs in case["clips"]:
            nf = sum(J.parse_header(b)[2] for b in blobs)
            n = J.clip_length(nf) * ch
            assert glc_amd.plan_encode(n, ch).n_frames == nf
            from_segments = glc_amd.EncodedAudio.from_compact(44100, n, ch, blobs).to_bytes()
            from_join = glc_amd.EncodedAudio.from_compact(44100, n, ch, [glc_amd.compact_join(blobs, ch)]).to_bytes()
            assert from_join == from_segments, case["name"]


def _raw_call(g, blobs, ch, cap=None):
    """glc_compact_join itself: (rc, info.bytes, message)."""
    held = [np.frombuffer(b + bytes(-len(b) % 8), np.uint64) for b in blobs]
    ptrs = (C.c_void_p * len(held))(*[h.ctypes.data for h in held])
    sizes = (C.c_uint64 * len(held))(*[len(b) for b in blobs])
    info = g._lib.GlcCompactInfo()
    need = len(J.join(blobs, ch)) if cap is None else cap
    out = np.zeros(need // 8 + 1, np.uint64)
    rc = g.lib.glc_compact_join(ptrs, sizes, len(held), ch, out.ctypes.data_as(C.c_void_p), need, C.byref(info))
    return rc, int(info.bytes), (g.lib.glc_last_error(None) or b"").decode()


@pytest.mark.parametrize("kind", J.DAMAGE)
@pytest.mark.parametrize("which", (0, 2))
def test_an_unusable_segment_is_refused_by_name(glc_amd, kind, which):
    rng = np.random.default_rng(5)
    blobs = J.clip_of(rng, 2, [3, 4, 2], raw=(1, 8))
    bad, bits = J.damaged(blobs[which], kind, 2)
    assert J.segment_status(bad, 2, J.parse_header(blobs[which])[2]) == bits != 0
    blobs[which] = bad
    with pytest.raises(ValueError, match=f"segment {which}"):
        J.join(blobs, 2)
    rc, _, msg = _raw_call(glc_amd, blobs, 2, cap=1 << 20)
    assert rc == glc_amd._lib.GLC_EINVAL and f"segment {which}:" in msg, msg
    with pytest.raises(glc_amd.GlcError):
        glc_amd.compact_join(blobs, 2)


def test_a_frame_count_that_wraps_the_sizes_is_refused(glc_amd):
    """A 64-byte blob whose header says n_frames = 2^64 - 64 (mono, 144 pairs, bytes = 64): every section offset formed
    from that count wraps, the size comes out as 64 and the header rule alone would pass it - and the sums over cnt and
    is_raw would then run far outside the blob.  The frame count is bounded before the rule is asked: refused by name,
    with nothing read behind the 64 bytes (tools/host_fuzz.cpp holds the same blob under the address sanitizer)."""
    import struct
    g = glc_amd
    good = J.make_blob(np.random.default_rng(8), 1, 3)
    for nf, n_pairs in ((2 ** 64 - 64, 144), (2 ** 64 - 1, 0), (2 ** 32, 0), (2 ** 63, 0)):
        crafted = struct.pack("<IIQQQQ", J.MAGIC, 1, nf, n_pairs, 0, 64) + bytes(24)
        for blobs, which in (([crafted], 0), ([good, crafted], 1)):
            rc, size, msg = _raw_call(g, blobs, 1, cap=1 << 16)
            assert rc == g._lib.GLC_EINVAL and size == 0 and f"segment {which}:" in msg, (nf, msg)
            with pytest.raises(g.GlcError):
                g.compact_join(blobs)


def test_no_segments_is_refused(glc_amd):
    g = glc_amd
    info = g._lib.GlcCompactInfo()
    out = np.zeros(16, np.uint64)
    assert g.lib.glc_compact_join(None, None, 0, 2, out.ctypes.data_as(C.c_void_p), 128, C.byref(info)) == g._lib.GLC_EINVAL
    assert info.bytes == 0 and not out.any()
    with pytest.raises(g.GlcError):
        g.compact_join([])
    with pytest.raises(g.GlcError):
        g.compact_join([], 2)


def test_a_cap_one_short_is_refused_with_the_size(glc_amd):
    rng = np.random.default_rng(6)
    blobs = J.clip_of(rng, 3, [2, 5], raw=(3,))
    need = len(J.join(blobs, 3))
    rc, size, msg = _raw_call(glc_amd, blobs, 3, cap=need - 1)
    assert rc == glc_amd._lib.GLC_EINVAL and size == need and "smaller" in msg
    rc, size, _ = _raw_call(glc_amd, blobs, 3, cap=need)
    assert rc == 0 and size == need


def test_the_signature_is_declared(glc_amd):
    for name in ("glc_store_join_segments_device", "glc_compact_join"):
        assert name in glc_amd._lib.SIGNATURES
    for cls in (glc_amd.Encoder, glc_amd.Decoder, glc_amd.StreamEncoder):
        assert callable(getattr(cls, "join_segments_tensor"))
