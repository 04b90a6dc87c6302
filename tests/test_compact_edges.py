"""The compaction kernels P1-P3 at their scan and packing edges (tests/compact_edges.py builds the records).

CPU: the generator is deterministic; the model of the blob, written from DESIGN.md section 3, equals the host twin
glc_compact_records byte for byte on every case with a dense image; the families reach the edges they claim
(computed from the descriptions and the expected blobs, so that an edit of the generator cannot silently drop
one); records an encode could have left give the same EncodedAudio bytes through the blob as through
glc_frames_from_records; and every single-rule mutation of the model changes at least one expected blob - so the
GPU tests below would notice that edit of a kernel.  GPU: every case through glc_compact_device_records (the batch
cases through glc_debug_compact_batch_device, include/glc_debug.h) into a 0xAB-filled buffer: sizes, every byte
of the blob, and every byte behind it still 0xAB; the 1026-block case with its records built on the device; one
context through compactions of different sizes; ranges that start inside a record array; refused arguments."""
import ctypes as C
import time

import numpy as np
import pytest

import compact_edges as E
from compact_edges import BLOCK, FRAME, HOP, SENTINEL

SR = 48000
TAIL = 4096            # sentinel bytes behind the capacity the entry point asks for


@pytest.fixture(scope="module")
def cases():
    return E.cases()


def _by_name(cs):
    return {c.name: c for c in cs}


def _family(cs, fam):
    return [c for c in cs if c.family == fam]


_expected = {}


def _model(c):
    """The expected blob of a case, computed once and shared (read-only)."""
    if c.name not in _expected:
        blob, info = E.model_batch(c.desc, c.clip_frames) if c.family == "batch" else E.model(c.desc)
        blob.setflags(write=False)
        _expected[c.name] = (blob, info)
    return _expected[c.name]


def _sections(c):
    """(is_raw, cnt, pairs, raw planes, gap bytes) of a case's expected blob."""
    d = c.desc
    blob, (nf, n_pairs, n_raw, total) = _model(c)
    o_israw, o_scale, o_cnt, o_pairs, _ = E.layout(d.ch, nf, len(c.clip_frames))
    raw_off = E.align64(o_pairs + 4 * n_pairs)
    return (blob[o_israw:o_israw + nf], blob[o_cnt:o_cnt + 4 * nf * d.ch].view(np.uint32),
            blob[o_pairs:o_pairs + 4 * n_pairs].view(np.uint32), blob[raw_off:total].view(np.int16).reshape(-1, FRAME),
            blob[o_pairs + 4 * n_pairs:raw_off])


# ----------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------

def test_generator_is_deterministic(cases):
    assert E.digest(E.build_cases()) == E.digest(cases)
    assert len({c.name for c in cases}) == len(cases)


def test_model_equals_the_host_twin_on_every_case(cases):
    """glc_compact_records on the dense records against the model on the description; a batch case as the plain
    compaction of its virtual stream (junk records included - the twin knows no clips).  The chunks case has no
    dense image."""
    import glc_amd
    n = 0
    for c in cases:
        if not c.dense:
            assert c.family == "chunks"
            continue
        d = c.desc
        want, info = E.model(d)
        got = glc_amd.compact_records(E.materialise(d), d.ch)
        assert got.size == info[3] == want.size, c.name
        assert np.array_equal(got, want), f"{c.name}: first difference at byte {int(np.flatnonzero(got != want)[0])}"
        n += 1
    assert n == len(cases) - 1


def test_families_cover_what_they_claim(cases):
    by = _by_name(cases)
    assert {c.family for c in cases} == {"counts", "disagree", "raw", "blocks", "chunks", "batch"}

    # counts: every count, every placement, q at both ends under an undisturbed index, scale bits copied
    for c in _family(cases, "counts"):
        d = c.desc
        marks = c.info["marks"]
        assert d.consistent()
        assert {n for _, kind, n in marks if kind == "spread"} == set(E.NNZ_COUNTS) == {0, 1, 2, 63, 64, 65, 127, 128, 1023, 1024}
        assert {kind for _, kind, _ in marks} == {"spread", "low", "high", "one_per_group", "63_64", "every_other"}
        for m, kind, n in marks:
            ks = d.e_k[d.e_row == m]
            assert ks.size == n == d.nnz[m]
            if kind == "low":
                assert (ks < 64).all()
            elif kind == "high":
                assert (ks >= 960).all() and (ks < HOP).all()
            elif kind == "one_per_group":
                assert sorted(ks // 64) == list(range(16))
            elif kind == "63_64":
                assert ks.tolist() == [63, 64]
            elif kind == "every_other":
                assert n == 512 and len(set(ks % 2)) == 1
        assert {n for _, kind, n in marks if kind in ("low", "high")} >= {1, 2, 63, 64}
        assert {int(ks[0]) % 64 for m, kind, _ in marks if kind == "one_per_group" for ks in [d.e_k[d.e_row == m]]} >= {0, 63}
        assert set(d.e_q.tolist()) == {1, -1, 32767, -32767, -32768} == set(E.Q_VALUES)
        _, _, pairs, _, _ = _sections(c)
        neg = d.e_q < 0                                 # every entry is kept: pair j is entry j
        assert pairs.size == d.e_q.size and ((pairs[neg] >> 16) & 0x8000 == 0x8000).all()
        assert np.array_equal(pairs & 0xFFFF, d.e_k.astype(np.uint32))
        w = pairs[d.e_q == -32768]
        assert w.size and np.array_equal(w, (d.e_k[d.e_q == -32768] | 0x8000 << 16).astype(np.uint32))
        assert set(E.SCALE_BITS) <= set(d.scale_bits.tolist())
        blob, (nf, _, _, _) = _model(c)
        o_scale = E.layout(d.ch, nf)[1]
        assert np.array_equal(blob[o_scale:o_scale + 4 * d.rows].view(np.uint32), d.scale_bits)
    f = np.array(E.SCALE_BITS, np.uint32).view(np.float32)
    assert f[0] == 0 and np.signbit(f[0]) and 0 < f[1] < np.finfo(np.float32).tiny and np.isinf(f[2]) and np.isnan(f[3])
    assert E.SCALE_BITS[3] & 0x3FFFFF not in (0, 0x3FFFFF)                 # a payload, not the default NaN

    # disagree: the field above and below the truth, past 1024, on raw rows; junk above bin 1023
    tf = by["disagree-over"].info["true_field"]
    assert all(t < fl <= 1024 for t, fl in tf) and {t for t, _ in tf} >= {0, 63, 64, 1023}
    _, cnt, pairs, _, _ = _sections(by["disagree-over"])
    assert cnt.tolist() == [fl for _, fl in tf] and int((pairs == E.FILLER).sum()) == sum(fl - t for t, fl in tf)
    tf = by["disagree-under"].info["true_field"]
    assert all(fl < t for t, fl in tf) and {fl for _, fl in tf} >= {0, 1, 63, 64, 65, 1023}
    _, cnt, pairs, _, _ = _sections(by["disagree-under"])
    assert cnt.tolist() == [fl for _, fl in tf] and not (pairs == E.FILLER).any()
    tf = by["disagree-clamp"].info["true_field"]
    assert {fl for _, fl in tf if fl > 1024} == set(E.CLAMPED_FIELDS) == {1025, 0xFFFFFFFF}
    _, cnt, pairs, _, _ = _sections(by["disagree-clamp"])
    assert cnt.tolist() == [min(fl, 1024) for _, fl in tf]
    c = by["disagree-rawnnz"]
    israw, cnt, _, _, _ = _sections(c)
    assert set(c.info["fields"].values()) == {7, 1024, 0xFFFFFFFF}
    for fr, v in c.info["fields"].items():
        assert israw[fr] == 1 and (c.desc.nnz[2 * fr:2 * fr + 2] == v).all() and not cnt[2 * fr:2 * fr + 2].any()
    c = by["disagree-upper"]
    up = c.desc.e_k >= HOP
    assert np.bincount(c.desc.e_row[up], minlength=c.desc.rows).tolist() == [HOP] * c.desc.rows
    _, cnt, pairs, _, _ = _sections(c)
    assert c.desc.consistent() and pairs.size == int((~up).sum()) and ((pairs & 0xFFFF) < HOP).all()
    c = by["disagree-upper-over"]
    up = c.desc.e_k >= HOP
    assert np.bincount(c.desc.e_row[up], minlength=c.desc.rows).tolist() == [HOP] * c.desc.rows
    _, cnt, pairs, _, _ = _sections(c)
    assert (cnt > c.desc.true_counts()).all() and int((pairs == E.FILLER).sum()) == int((cnt - c.desc.true_counts()).sum())
    assert [c.desc.consistent() for c in _family(cases, "disagree")] == [False, False, False, False, True, False]

    # raw: flag words, placements, a raw frame across the block edge, extremes, gaps
    fam = _family(cases, "raw")
    flags = set()
    for c in fam:
        flags |= set(c.desc.flags.tolist())
        assert c.desc.consistent()
    assert flags == {0, 1, 2, 0x100, 0x80000000} == {0, *E.FLAG_WORDS}
    assert {c.info.get("flag") for c in fam} >= set(E.FLAG_WORDS)
    assert {c.info["placement"] for c in fam} >= {"all", "none", "alternating", "first", "last"}
    for kind, want in (("all", lambda nf: [1] * nf), ("none", lambda nf: [0] * nf), ("alternating", lambda nf: [f % 2 for f in range(nf)]),
                       ("first", lambda nf: [1] + [0] * (nf - 1)), ("last", lambda nf: [0] * (nf - 1) + [1])):
        for c in fam:
            if c.info["placement"] == kind:
                assert _sections(c)[0].tolist() == want(c.desc.nf), c.name
    assert {c.desc.ch for c in fam if "straddle" in c.info} == set(E.RAW_CHANNELS) == {3, 5, 7}
    for c in fam:
        if "straddle" in c.info:
            f0, ch = c.info["straddle"], c.desc.ch
            assert c.desc.flags[f0] != 0 and f0 * ch < BLOCK < (f0 + 1) * ch and c.desc.rows > BLOCK
        vals = set().union(*[set(p.reshape(-1).tolist()) for p in c.desc.planes.values()]) if c.desc.planes else set()
        assert not c.desc.planes or vals >= set(E.I16_EXTREMES) >= {-32768, 32767}
    gaps = {}
    for c in fam:
        if "gap" in c.info:
            _, _, pairs, raw, gap = _sections(c)
            assert raw.shape[0] >= 1 and gap.size == c.info["gap"] and not gap.any()
            gaps[pairs.size % 16] = gap.size
    assert gaps == {0: 0, 1: 60, 15: 4}

    # blocks: the row counts, and the packed scan word at both limits
    fam = _family(cases, "blocks")
    assert {c.desc.rows for c in fam if c.desc.ch == 1} >= set(E.BLOCK_ROWS) == {1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 4097}
    for ch in (3, 8):
        have = {c.desc.nf for c in fam if c.desc.ch == ch}
        assert have == {E.block_frames(ch, M) for M in E.BLOCK_ROWS}
        assert all(abs(E.block_frames(ch, M) * ch - M) <= max(ch / 2, ch - M) for M in E.BLOCK_ROWS)
    assert {c.desc.ch for c in fam} == set(E.BLOCK_CHANNELS) == {1, 3, 8}
    assert any(c.desc.flags.any() for c in fam if c.desc.rows > BLOCK)
    c = by["blocks-dense-then-one"]
    _, cnt, pairs, _, _ = _sections(c)
    assert cnt.tolist() == [HOP] * BLOCK + [1] and pairs.size == (1 << 20) + 1
    assert pairs[1 << 20] == (77 | 0x8000 << 16) and not (pairs == E.FILLER).any()        # the row's offset is exactly 2^20
    c = by["blocks-raw-block"]
    israw, cnt, pairs, raw, _ = _sections(c)
    assert israw.tolist() == [1] * BLOCK + [0, 1] and cnt[BLOCK] == 4 and raw.shape[0] == BLOCK + 1
    assert raw[:BLOCK, 0].tolist() == list(range(1, BLOCK + 1)) and np.array_equal(raw[BLOCK], c.desc.planes[BLOCK + 1][0])
    c = by["blocks-1023-dense-1-raw"]
    israw, cnt, pairs, raw, _ = _sections(c)
    assert cnt.tolist() == [HOP] * (BLOCK - 1) + [0, 2, 0] and israw.tolist() == [0] * (BLOCK - 1) + [1, 0, 1]
    assert (pairs[-2:] & 0xFFFF).tolist() == [5, 900] and raw.shape[0] == 2

    # chunks: more than 1024 scan blocks, 0..3 pairs per row, raw frames in the blocks around the chunk edge
    c = by["chunks"]
    d = c.desc
    assert d.ch == 1 and d.nf == BLOCK * (BLOCK + 1) + 7 and -(-d.rows // BLOCK) == BLOCK + 2 and d.consistent()
    assert set(d.nnz.tolist()) == {0, 1, 2, 3}
    per_block = np.add.reduceat(d.nnz.astype(np.int64), np.arange(0, d.rows, BLOCK))
    assert len(set(per_block[:BLOCK + 1].tolist())) > 500 and per_block[BLOCK:].all()
    assert tuple(np.flatnonzero(d.flags) // BLOCK) == E.CHUNK_RAW_BLOCKS == (0, 1023, 1024, 1025)

    # batch: the clip shapes, both kinds of junk, and nothing of a junk record in the blob
    fam = _family(cases, "batch")
    assert any(set(c.clip_frames) == {1} and 1 < len(c.clip_frames) < 700 for c in fam)
    assert {c.clip_frames[0] for c in fam if c.name.startswith("batch-edge")} == {1023, 1024, 1025}
    assert all(c.desc.ch == 1 for c in fam if c.name.startswith("batch-edge"))           # frames are rows
    assert any(len(c.clip_frames) == 1 for c in fam) and any(c.clip_frames == (1,) * 700 for c in fam)
    kinds = set()
    for c in fam:
        d, ch = c.desc, c.desc.ch
        real = E.real_frames(c.clip_frames)
        junk = np.setdiff1d(np.arange(d.nf), real)
        assert junk.size == len(c.clip_frames) == len(c.info["junk"])
        for j, kind in zip(junk, c.info["junk"]):
            kinds.add(kind)
            if kind == "rawflag":
                assert d.flags[j] != 0 and np.count_nonzero(d.planes[int(j)]) > 1900 * ch
            else:
                assert d.flags[j] == 0 and (d.nnz[j * ch:(j + 1) * ch] == HOP).all()
                assert int(((d.e_row // ch) == j).sum()) == HOP * ch
        israw, cnt, pairs, raw, _ = _sections(c)
        sub = E.take_frames(d, real)
        assert sub.consistent() and pairs.size == int(sub.nnz.sum()) == sub.e_q.size and raw.shape[0] == int((sub.flags != 0).sum()) * ch
        blob, _ = _model(c)
        dirv = blob[64:64 + 16 * len(c.clip_frames)].view(np.uint64).reshape(-1, 2)
        first = np.cumsum((0,) + c.clip_frames[:-1])
        assert dirv[:, 0].tolist() == [int(sub.nnz[:f * ch].sum()) for f in first]
        assert dirv[:, 1].tolist() == [int((sub.flags[:f] != 0).sum()) * ch for f in first]
    assert kinds == {"rawflag", "dense"}
    c = by["batch-first-raw"]
    first = np.cumsum((0,) + c.clip_frames[:-1])
    assert (_sections(c)[0][first] != 0).tolist() == [False, True, False, True]
    assert _sections(by["batch-all-raw"])[0].all() and _sections(by["batch-all-raw"])[2].size == 0


def test_consistent_cases_give_the_bytes_of_the_records(cases):
    """Records whose nnz fields say what their rows hold: EncodedAudio through the expected blob
    (glc_frames_from_compact) and through the records (glc_frames_from_records) serialise to the same bytes."""
    import glc_amd
    n = 0
    for c in cases:
        d = c.desc
        if not (c.dense and c.family != "batch" and d.consistent()):
            continue
        n_samples = d.nf * HOP * d.ch
        assert glc_amd.plan_encode(n_samples, d.ch).n_frames == d.nf
        blob, _ = _model(c)
        via_blob = glc_amd.EncodedAudio.from_compact(SR, n_samples, d.ch, [np.array(blob)]).to_bytes()
        assert via_blob == glc_amd.EncodedAudio.from_records(SR, n_samples, d.ch, E.materialise(d)).to_bytes(), c.name
        n += 1
    assert n >= 40


_HINT = {"scan_inclusive": "counts", "block_carry_dropped": "blocks", "chunk_carry_dropped": "chunks",
         "raw_counted_as_pairs": "disagree", "raw_flag_low_byte": "raw", "nnz_unclamped": "disagree",
         "filler_missing": "disagree", "keep_last_not_first": "disagree", "descending_k": "counts",
         "idx_q_swapped": "counts", "upper_bins_counted": "disagree", "raw_gap_unaligned": "raw",
         "raw_gap_not_zeroed": "raw", "raw_rows_by_block_not_global": "blocks", "dir_off_by_one_clip": "batch",
         "junk_frame_counted": "batch"}


def _mutated_differs(c, mut):
    want, _ = _model(c)
    got, _ = E.model_batch(c.desc, c.clip_frames, mut) if c.family == "batch" else E.model(c.desc, mut)
    return got.size != want.size or not np.array_equal(got, want)


def test_power_every_mutation_of_the_model_changes_an_expected_blob(cases):
    """Each single-rule edit of the packing changes the expected blob of some case of the family built for it -
    which is what makes the GPU tests below able to catch that edit of a kernel."""
    assert set(_HINT) == set(E.MUTATIONS) and len(E.MUTATIONS) == 16
    caught = {}
    for mut in E.MUTATIONS:
        hit = [c.name for c in _family(cases, _HINT[mut]) if _mutated_differs(c, mut)]
        if hit:
            caught[mut] = set(hit)
    missed = [m for m in E.MUTATIONS if m not in caught]
    assert not missed, f"mutations no expected blob notices: {missed}"
    print("detected:", {m: sorted(v)[:4] for m, v in caught.items()})
    by = _by_name(cases)
    # only a range of more than 1024 scan blocks can show a lost chunk carry
    assert not any(_mutated_differs(c, "chunk_carry_dropped") for c in cases if c.dense and c.family != "batch")
    assert caught["raw_flag_low_byte"] >= {"raw-flag-0x100", "raw-first", "raw-last"}
    assert "raw-flag-0x1" not in caught["raw_flag_low_byte"]
    assert caught["raw_gap_unaligned"] >= {"raw-gap60", "raw-gap4"} and "raw-gap0" not in caught["raw_gap_unaligned"]
    assert caught["raw_gap_not_zeroed"] >= {"raw-gap60", "raw-gap4"}
    assert caught["nnz_unclamped"] == {"disagree-clamp"} and caught["upper_bins_counted"] == {"disagree-upper-over"}
    assert caught["raw_counted_as_pairs"] == {"disagree-rawnnz"}
    assert caught["keep_last_not_first"] == {"disagree-under"} and caught["filler_missing"] >= {"disagree-over", "disagree-clamp"}
    assert caught["block_carry_dropped"] >= {"blocks-dense-then-one", "blocks-ch1-nf1025", "blocks-ch3-nf342", "blocks-ch8-nf256"}
    assert "blocks-ch1-nf1024" not in caught["block_carry_dropped"]
    assert caught["raw_rows_by_block_not_global"] >= {"blocks-raw-block", "blocks-1023-dense-1-raw"}
    assert caught["junk_frame_counted"] == {c.name for c in _family(cases, "batch") if len(c.clip_frames) > 1}
    assert caught["dir_off_by_one_clip"] == {c.name for c in _family(cases, "batch")}
    # a junk record is in no one's sections however it is filled: a single clip shows it through the sizes alone
    assert _model(by["batch-single-dense-junk"])[1][1] < HOP


# ----------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    import glc_amd
    f = glc_amd.lib.glc_debug_compact_batch_device
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint16, C.c_void_p, C.c_uint64,
                  C.POINTER(glc_amd._lib.GlcCompactInfo)]
    return torch, glc_amd


def _sentinel_blob(torch, n):
    t = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 64 == 0
    return t


def _upload(torch, d):
    t = torch.from_numpy(E.materialise(d).reshape(-1)).cuda()
    assert t.data_ptr() % 64 == 0
    return t


def _explain(got, want, c, n_clips=0):
    d = c.desc
    nf = len(E.real_frames(c.clip_frames)) if c.clip_frames else d.nf
    o_israw, o_scale, o_cnt, o_pairs, _ = E.layout(d.ch, nf, n_clips)
    bad = np.flatnonzero(got != want)
    at = int(bad[0])
    names = [(64, "header"), (o_israw, "directory"), (o_scale, "is_raw"), (o_cnt, "scale"), (o_pairs, "cnt")]
    sec = next((n for end, n in names if at < end), "pairs / raw planes")
    return (f"{bad.size} of {want.size} bytes differ, first at byte {at} ({sec}; pairs start at {o_pairs}): "
            f"got {got[at:at + 8].tolist()} want {want[at:at + 8].tolist()}; last at byte {int(bad[-1])}")


def _check(got_info, buf, c, want, info, what, n_clips=0):
    """info and every byte: the blob, then the sentinel to the end of the buffer."""
    assert (got_info.n_frames, got_info.n_pairs, got_info.n_raw_rows, got_info.bytes) == info, what
    n = info[3]
    assert np.array_equal(buf[:n], want), f"{what}: {_explain(buf[:n], want, c, n_clips)}"
    rest = buf[n:]
    assert (rest == SENTINEL).all(), \
        f"{what}: {int((rest != SENTINEL).sum())} bytes behind the blob were written, first at +{int(np.flatnonzero(rest != SENTINEL)[0])}"


def _compact(gpu, enc, c, what=None, d_rec=None):
    """One plain case through glc_compact_device_records, everything compared."""
    torch, glc_amd = gpu
    d = c.desc
    want, info = _model(c)
    d_rec = _upload(torch, d) if d_rec is None else d_rec
    cap = glc_amd.compact_bound(d.ch, d.nf)
    assert cap == E.layout(d.ch, d.nf)[4]
    d_blob = _sentinel_blob(torch, cap + TAIL)
    torch.cuda.synchronize()
    got = enc.compact_device_records(d_rec.data_ptr(), d.nf, d.ch, d_blob.data_ptr(), cap)
    _check(got, d_blob.cpu().numpy(), c, want, info, what or c.name)
    return d_rec


def _compact_batch(gpu, enc, c, what=None):
    torch, glc_amd = gpu
    d, clips = c.desc, c.clip_frames
    want, info = _model(c)
    d_rec = _upload(torch, d)
    cap = E.layout(d.ch, sum(clips), len(clips))[4]
    d_blob = _sentinel_blob(torch, cap + TAIL)
    torch.cuda.synchronize()
    got = glc_amd._lib.GlcCompactInfo()
    rc = glc_amd.lib.glc_debug_compact_batch_device(enc._h, d_rec.data_ptr(), (C.c_uint64 * len(clips))(*clips), len(clips), d.ch,
                                                    d_blob.data_ptr(), cap, C.byref(got))
    assert rc == 0, (c.name, glc_amd.lib.glc_last_error(enc._h))
    _check(got, d_blob.cpu().numpy(), c, want, info, what or c.name, len(clips))


def _case_ids(*families):
    return [c.name for c in E.cases() if c.family in families]


@pytest.mark.gpu
@pytest.mark.parametrize("name", _case_ids("counts", "disagree", "raw", "blocks"))
def test_gpu_every_case_byte_for_byte(gpu, cases, name):
    c = _by_name(cases)[name]
    glc_amd = gpu[1]
    enc = glc_amd.Encoder(SR)
    d = c.desc
    d_rec = _compact(gpu, enc, c)
    if d.consistent():
        n_samples = d.nf * HOP * d.ch
        ea = enc.frames_from_device_records(d_rec.data_ptr(), d.nf, n_samples, d.ch)
        assert ea.to_bytes() == glc_amd.EncodedAudio.from_records(SR, n_samples, d.ch, E.materialise(d)).to_bytes()


@pytest.mark.gpu
def test_gpu_more_than_1024_scan_blocks(gpu, cases):
    """1026 scan blocks: the chunk loop and the carry of k_pack_scan_blocks.  The records (4.3 GB) are built on the
    device, zero fill plus indexed stores; the blob buffer is as large again.  Only the blob itself comes back:
    header, fixed sections, pairs and the four raw planes, and the MiB behind them."""
    torch, glc_amd = gpu
    t0 = time.perf_counter()
    c = _by_name(cases)["chunks"]
    d = c.desc
    want, info = _model(c)
    d_rec = E.materialise_torch(d, torch)
    assert d_rec.data_ptr() % 64 == 0 and d_rec.numel() * 2 == d.nf * E.record_bytes(1)
    probe = np.concatenate([np.arange(64), np.arange(d.e_row.size - 64, d.e_row.size)])      # the stores landed, at both ends
    col = E.header_bytes(1) // 2 + d.e_k[probe]
    assert [int(d_rec[int(r), int(k)]) for r, k in zip(d.e_row[probe], col)] == d.e_q[probe].tolist()
    assert int(torch.count_nonzero(d_rec.view(torch.int32)[:, 0])) == 4
    cap = glc_amd.compact_bound(1, d.nf)
    d_blob = _sentinel_blob(torch, cap)
    enc = glc_amd.Encoder(SR)
    torch.cuda.synchronize()
    got = enc.compact_device_records(d_rec.data_ptr(), d.nf, 1, d_blob.data_ptr(), cap)
    assert (got.n_frames, got.n_pairs, got.n_raw_rows, got.bytes) == info
    n = info[3]
    buf = d_blob[:n + (1 << 20)].cpu().numpy()
    assert np.array_equal(buf[:n], want), _explain(buf[:n], want, c)
    assert (buf[n:] == SENTINEL).all()
    print(f"chunks case: {time.perf_counter() - t0:.2f} s wall, {n} blob bytes, {d.nf} rows")


@pytest.mark.gpu
@pytest.mark.parametrize("name", _case_ids("batch"))
def test_gpu_batch_compaction_byte_for_byte(gpu, cases, name):
    _compact_batch(gpu, gpu[1].Encoder(SR), _by_name(cases)[name])


@pytest.mark.gpu
def test_gpu_reuse_sequence(gpu, cases):
    """One context through compactions of different sizes and kinds, each step against its model, not against the
    step before: loc, blk or totals left in the scratch by a longer call must not show in a shorter one."""
    by = _by_name(cases)
    enc = gpu[1].Encoder(SR)
    _compact(gpu, enc, by["blocks-ch1-nf4097"], "reuse step 0")
    _compact(gpu, enc, by["blocks-ch1-nf1"], "reuse step 1")
    _compact(gpu, enc, by["blocks-dense-then-one"], "reuse step 2")
    _compact_batch(gpu, enc, by["batch-edge-1024"], "reuse step 3")
    _compact(gpu, enc, by["blocks-ch1-nf4097"], "reuse step 4")


@pytest.mark.gpu
@pytest.mark.parametrize("name,a", [("blocks-ch1-nf2049", 1), ("blocks-ch1-nf4097", 1029), ("blocks-ch3-nf1366", 1),
                                    ("blocks-ch3-nf1366", 2), ("raw-ch3-alternating", 341)])
def test_gpu_sub_range_of_a_record_array(gpu, cases, name, a):
    """Frames [a, n) of a case, from d_records + a * record_bytes: one channel makes that start 16-byte aligned and
    no more (4112 = 16 * 257); three channels put every block edge of the range inside a frame."""
    torch, glc_amd = gpu
    c = _by_name(cases)[name]
    d = c.desc
    rec = E.record_bytes(d.ch)
    sub = E.take_frames(d, np.arange(a, d.nf))
    want, info = E.model(sub)
    d_rec = _upload(torch, d)
    start = d_rec.data_ptr() + a * rec
    assert start % 8 == 0 and (d.ch != 1 or start % 32 == 16) and (d.ch != 3 or BLOCK % 3)
    cap = glc_amd.compact_bound(d.ch, sub.nf)
    d_blob = _sentinel_blob(torch, cap + TAIL)
    torch.cuda.synchronize()
    got = glc_amd.Encoder(SR).compact_device_records(start, sub.nf, d.ch, d_blob.data_ptr(), cap)
    _check(got, d_blob.cpu().numpy(), E.Case(name, c.family, sub), want, info, f"{name} from frame {a}")


@pytest.mark.gpu
def test_gpu_refused_arguments_leave_the_blob_untouched(gpu, cases):
    """glc_compact_device_records and the batch hook check before any device work: misaligned d_records or d_blob
    (include/glc.h: 8 bytes), a capacity one byte short, no channels, no clips, a clip of no frames."""
    torch, glc_amd = gpu
    c = _by_name(cases)["blocks-ch1-nf5"]
    d = c.desc
    enc = glc_amd.Encoder(SR)
    d_rec = _upload(torch, d)
    cap = glc_amd.compact_bound(d.ch, d.nf)
    bc = _by_name(cases)["batch-single"]
    bcap = E.layout(bc.desc.ch, 5, 1)[4]
    d_blob = _sentinel_blob(torch, max(cap, bcap) + TAIL)
    torch.cuda.synchronize()
    r, b = d_rec.data_ptr(), d_blob.data_ptr()
    for what, args in (("misaligned d_records", (r + 4, d.nf - 1, d.ch, b, cap)), ("misaligned d_records", (r + 2, d.nf - 1, d.ch, b, cap)),
                       ("misaligned d_blob", (r, d.nf, d.ch, b + 4, cap)), ("misaligned d_blob", (r, d.nf, d.ch, b + 1, cap)),
                       ("cap one byte short", (r, d.nf, d.ch, b, cap - 1)), ("channels == 0", (r, d.nf, 0, b, cap)),
                       ("null blob", (r, d.nf, d.ch, 0, cap))):
        with pytest.raises(glc_amd.GlcError) as e:
            enc.compact_device_records(*args)
        assert e.value.code == glc_amd._lib.GLC_EINVAL, what
    hook = glc_amd.lib.glc_debug_compact_batch_device
    info = glc_amd._lib.GlcCompactInfo()
    d_vrec = _upload(torch, bc.desc)
    v, ch = d_vrec.data_ptr(), bc.desc.ch
    assert bc.clip_frames == (5,)
    one, none, two = (C.c_uint64 * 1)(5), (C.c_uint64 * 1)(0), (C.c_uint64 * 2)(4, 0)
    for what, args in (("n_clips == 0", (v, one, 0, ch, b, bcap)), ("a clip of 0 frames", (v, none, 1, ch, b, bcap)),
                       ("a clip of 0 frames", (v, two, 2, ch, b, bcap)), ("misaligned d_records", (v + 4, one, 1, ch, b, bcap)),
                       ("misaligned d_blob", (v, one, 1, ch, b + 4, bcap)), ("cap one byte short", (v, one, 1, ch, b, bcap - 1)),
                       ("channels == 0", (v, one, 1, 0, b, bcap)), ("null clip_frames", (v, None, 1, ch, b, bcap))):
        assert hook(enc._h, *args, C.byref(info)) == glc_amd._lib.GLC_EINVAL, what
    enc.synchronize()
    assert (d_blob.cpu().numpy() == SENTINEL).all()          # a refused call writes nothing
    # and the bounds themselves are accepted: capacity exact, an empty range
    _compact(gpu, enc, c, "cap exact", d_rec)
    got = enc.compact_device_records(0, 0, 2, d_blob.data_ptr(), glc_amd.compact_bound(2, 0))
    assert (got.n_frames, got.n_pairs, got.n_raw_rows, got.bytes) == (0, 0, 0, 64)
