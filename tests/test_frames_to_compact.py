"""glc_frames_to_compact (host only): the compact blob of a whole EncodedAudio, the inverse of
glc_frames_from_compact - the bytes glc_compact_records gives for the stream's records - and what it refuses."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import compact_decode_cases as K
import roundtrip_cases as RC

EINVAL = -1
HOP, FRAME = K.HOP, K.FRAME
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    assert hasattr(g.lib, "glc_frames_to_compact")
    return g


def streams():
    rng = np.random.RandomState(4)
    for ch in (1, 2, 3, 6):
        yield f"edge-stream-{ch}ch", ch, RC.edge_stream(ch)
    for where in ("first", "last", "every-other", "all", "none"):
        yield f"raw-{where}", 2, RC.raw_placement(2, 6, where)
    yield "one-frame-mono", 1, [("c", [(0.5, RC.dense_row(rng, 1024), None)])]
    yield "all-empty", 2, [("c", [(0.0, np.zeros(HOP, np.int16), None)] * 2)] * 3


STREAMS = list(streams())


def canonical_records(ch, frames):
    """Records as a STREAM describes them: an nnz field that counts its row, nothing on the rows of raw frames."""
    fixed = []
    for kind, body in frames:
        if kind == "raw":
            fixed.append((kind, body))
        else:
            fixed.append((kind, [(s, q, min(int(np.count_nonzero(q)), n if n is not None else HOP)) for s, q, n in body]))
    for i, (kind, body) in enumerate(fixed):      # a short nnz field keeps the first nnz non-zeros: say so in the row
        if kind == "c":
            rows = []
            for s, q, n in body:
                q = q.copy()
                q[np.flatnonzero(q)[n:]] = 0
                rows.append((s, q, None))
            fixed[i] = (kind, rows)
    return RC.build_records(ch, fixed)


@pytest.mark.parametrize("name,ch,frames", STREAMS, ids=[s[0] for s in STREAMS])
def test_equals_compact_records_and_inverts_from_compact(glc_amd, name, ch, frames):
    g = glc_amd
    records, per_channel = canonical_records(ch, frames)
    n = per_channel * ch
    want = g.compact_records(records, ch)
    stream = g.EncodedAudio.from_records(44100, n, ch, records)
    blob = np.frombuffer(g.frames_to_compact(stream), np.uint8)
    assert blob.size == want.size and np.array_equal(blob, want)
    back = g.EncodedAudio.from_compact(44100, n, ch, [blob])
    assert back.to_bytes() == stream.to_bytes()
    # ... and the model of DESIGN.md section 3 reads the same header
    nf = len(frames)
    hdr = np.frombuffer(blob[:40].tobytes(), np.uint32)
    assert hdr[0] == K.MAGIC and hdr[1] == ch and int(np.frombuffer(blob[8:16].tobytes(), np.uint64)[0]) == nf
    assert int(np.frombuffer(blob[32:40].tobytes(), np.uint64)[0]) == blob.size


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.glc"))), ids=os.path.basename)
def test_round_trip_is_the_identity_on_the_golden_streams(glc_amd, path):
    g = glc_amd
    data = open(path, "rb").read()
    stream = g.EncodedAudio.from_bytes(data)
    h, gi = stream.header, stream.gapless_info
    blob = g.frames_to_compact(stream)
    back = g.EncodedAudio.from_compact(h.sample_rate, gi.original_length, h.channels, [blob])
    assert back.to_bytes() == data
    assert g.frames_to_compact(back) == blob


def test_golden_streams_exist():
    assert glob.glob(os.path.join(GOLDEN, "*.glc"))


def view_parts(g, ch, frames):
    records, per_channel = canonical_records(ch, frames)
    return g.EncodedAudio.from_records(44100, per_channel * ch, ch, records).parts()


def refuse(g, parts, what):
    stream = g.EncodedAudio.from_parts(parts)
    info = g._lib.GlcCompactInfo()
    buf = np.zeros(g.compact_bound(parts["channels"], parts["n_frames"]) + 4096 * 4, np.uint8)
    rc = g.lib.glc_frames_to_compact(stream._h, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(info))
    assert rc == EINVAL
    msg = g.lib.glc_last_error(None).decode()
    assert "glc_frames_to_compact" in msg and what in msg, msg
    with pytest.raises(g.GlcError) as e:
        g.frames_to_compact(stream)
    assert e.value.code == EINVAL


def test_refuses_a_frame_with_another_number_of_lists(glc_amd):
    p = view_parts(glc_amd, 2, RC.raw_placement(2, 3, "none"))
    # frame 1 gives its second list to frame 2: 2, 1, 3 lists per frame
    lb = p["list_begin"].copy()
    lb[2] -= 1
    p["list_begin"] = lb
    refuse(glc_amd, p, "frame 1")


def test_refuses_a_frame_with_another_number_of_scales(glc_amd):
    p = view_parts(glc_amd, 2, RC.raw_placement(2, 3, "none"))
    sb = p["scale_begin"].copy()
    sb[1] += 1
    p["scale_begin"] = sb
    refuse(glc_amd, p, "frame 0")


def test_refuses_a_raw_frame_of_another_length(glc_amd):
    p = view_parts(glc_amd, 2, RC.raw_placement(2, 3, "last"))
    rb = p["raw_begin"].copy()
    rb[-1] -= 2
    p["raw_begin"] = rb
    p["raw"] = p["raw"][:-2].copy()
    p["n_raw"] = int(p["n_raw"]) - 2
    refuse(glc_amd, p, "2048 * channels")


@pytest.mark.parametrize("kind", ("repeated", "descending", "bin-1024"))
def test_refuses_a_list_that_is_not_canonical(glc_amd, kind):
    p = view_parts(glc_amd, 1, [("c", [(0.1, RC.dense_row(np.random.RandomState(1), 3, [5, 6, 7], [1, 2, 3]), None)])])
    pairs = p["pairs"].copy()
    q = pairs & np.uint32(0xFFFF0000)
    idx = {"repeated": [5, 6, 6], "descending": [5, 7, 6], "bin-1024": [5, 6, 1024]}[kind]
    p["pairs"] = (q | np.array(idx, np.uint32)).astype(np.uint32)
    refuse(glc_amd, p, "strictly ascending")


def test_cap_too_small_fills_the_size(glc_amd):
    g = glc_amd
    records, per_channel = canonical_records(2, RC.raw_placement(2, 4, "first"))
    stream = g.EncodedAudio.from_records(44100, per_channel * 2, 2, records)
    want = g.compact_records(records, 2)
    info = g._lib.GlcCompactInfo()
    buf = np.full(want.size, 0xAB, np.uint8)
    rc = g.lib.glc_frames_to_compact(stream._h, buf.ctypes.data_as(C.c_void_p), want.size - 1, C.byref(info))
    assert rc == EINVAL and info.bytes == want.size and np.all(buf == 0xAB)
    rc = g.lib.glc_frames_to_compact(stream._h, buf.ctypes.data_as(C.c_void_p), want.size, C.byref(info))     # exactly enough
    assert rc == 0 and np.array_equal(buf, want)
    assert (info.n_frames, info.bytes) == (4, want.size)
