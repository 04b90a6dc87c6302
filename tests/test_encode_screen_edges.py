"""The screened encode path at its channel, tile and driver edges (tests/encode_screen_edges.py builds the cases and the
models; tests/test_encode_screen.py is the path's first suite; the helpers both use are in encode_screen_cases.py).

CPU: every case reaches the outcome it is built for, by a margin (no row too close to call) and by row number; the
families together hold what they claim - every loader, both quantiser forms, a failing and a passing row on each side
of every row cut, energy in one octet only; a numpy model of the path's RECORDS equals the oracle on every case, and
each single-edit mutation of it - a plane read one row off, an octet skipped, a flag read from the neighbouring
tile ... - changes a byte or a count of a named case; the bound holds on the new value shapes.
GPU: every case through glc_encode_range_device with the screen forced on and off - record bytes against the
oracle, guard pages, the counts exactly the model's; sequences on one context (a smaller launch after a larger, the
channel count changing, the same launch twice, 255 and 256 rows); and the other four drivers of encode_range_on -
glc_encode (both workspace slots), glc_encode_batch (junk frames), the single and the batch round trip - against
oracle.encode / oracle.decode, under the automatic bound kind and with the matrix form forced.  (The store encode, the
stream push and the PCM round trip: tests/test_encode_screen_drivers.py.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_screen_edges as E  # noqa: E402
from encode_screen_edges import SR  # noqa: E402
from oracle import oracle as O  # noqa: E402

F32 = np.float32
CASES = {c.name: c for c in E.all_cases()}
RANGE_NAMES = [c.name for c in CASES.values() if c.family != "reuse"]

_expected = {}


def expected(case):
    """(oracle records, taps, model) of a case, computed once per session."""
    if case.name not in _expected:
        rec, taps = E.expected(case)
        _expected[case.name] = (rec, taps, E.decide(case, taps))
    return _expected[case.name]


def family(fam):
    return [c for c in CASES.values() if c.family == fam]


def fails(case):
    return np.flatnonzero(expected(case)[2] == -1).tolist()


# ----------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------

def test_every_row_of_every_case_is_decided_and_fails_where_it_was_built_to():
    for name, c in CASES.items():
        _, taps, v = expected(c)
        assert 255 <= c.M <= 800
        assert (v != 0).all(), f"{name}: rows {np.flatnonzero(v == 0)[:8].tolist()} are too close to the floor to call"
        got = fails(c)
        if c.fail_rows is not None:
            assert got == c.fail_rows, f"{name}: rows {got[:12]} fail, built for {c.fail_rows[:12]}"
        else:
            assert set(c.must_fail) <= set(got) and not set(c.must_pass) & set(got), name
    # channels: the sizes the family promises
    for c in family("channels"):
        assert c.M % 256 and (c.ch not in (5, 6) or c.M % 16), c.name
        if "raw" in c.tags:
            assert expected(c)[1].is_raw.all() == c.tags["raw"] and expected(c)[1].is_raw.any() == c.tags["raw"], c.name
    assert {c.ch for c in family("channels")} == {4, 5, 6, 8, 16}
    for ch in (5, 6, 8, 16):            # unfused: three single rows, in the first, the last and a middle channel, one frame
        f = np.array(CASES[f"ch{ch}-clicks"].fail_rows)
        assert f.size == 3 + ch and {0, ch - 1, ch // 2} <= set((f % ch).tolist())
    assert len(CASES["ch4-clicks"].fail_rows) == 16          # fused: four whole frames
    # boundaries: by number
    assert (E.M_MONO, E.M_STEREO) == (309, 310) and E.boundary_patterns(309)["r288"] == [288]
    for r in (0, 3, 4, 15, 16, 31, 32, 255, 256, 308, 288):
        assert fails(CASES[f"b1-r{r}"]) == [r]
    for r in (0, 3, 4, 15, 16, 31, 32, 255, 256, 309, 288):
        assert fails(CASES[f"b2-r{r}"]) == [r // 2 * 2, r // 2 * 2 + 1]
    assert fails(CASES["b1-tile1-fails"]) == list(range(32, 64)) == fails(CASES["b2-tile1-fails"])
    assert fails(CASES["b1-tile1-passes"]) == list(range(32)) + list(range(64, 96)) == fails(CASES["b2-tile1-passes"])
    assert fails(CASES["b1-alternate"]) == list(range(0, 309, 2))
    assert fails(CASES["b2-alternate"]) == [r for r in range(310) if r // 2 % 2 == 0]
    # octets: the stretches; which condition fails a row
    for c in family("octets"):
        L, c0, _ = E.shape(c.sr)
        k, db = c.tags["k"], c.tags["db"]
        a, b = E.conditions(c, expected(c)[1])
        got = np.array(fails(c))
        assert ((got + c.f0) // 8 % 2 == 1).all() or db == E.LOUD, c.name       # only frames that hold the line throughout
        assert np.array_equal(np.flatnonzero(a | b), got), c.name
        q_last = (expected(c)[1].dense_q[got][:, L:] != 0).any(1)
        if db == E.SUBFLOOR:
            # Decided by the emulated fused sums, not by model(), which cannot call these rows: B is 1.055 nfl on
            # the 48 rows that fail and at most 0.95 nfl without the term kScreenCErr A - 5 % to either side on
            # every row of the case, where two orders of fused accumulation differ by parts in 10^6 of B.
            r = E.conditions(c, expected(c)[1], ratio=True)[1]
            r4 = E.conditions(c, expected(c)[1], 4, ratio=True)[1]
            assert got.size == 48 and (r[got] > 1.05).all() and (np.delete(r, got) < 0.95).all() and (r4 < 0.95).all(), c.name
            assert (E.model(c, expected(c)[1])[got] == 0).all() and not q_last.any() and not a.any(), c.name
            continue
        assert q_last.all(), f"{c.name}: a failing row whose record has nothing in the last band"
        if k < c0:             # L, C0 - 1: condition (a) alone, on exact bins
            assert db == E.LONE and a[got].all() and not b.any(), c.name
            assert got.size == 64 and ((got + c.f0) % 2 == 0).all()
        elif k >= c0 + 1:      # nothing reaches down to the exact bins
            assert b[got].all() and not a.any(), c.name
        if db == E.CONFINED:   # energy over the floor in ONE octet, below it everywhere else from L on
            mag = np.abs(expected(c)[1].coeffs[got])
            nfl = E.NOISE_FLOOR * mag[:, :c0].max(1)
            over = (mag[:, L:] > nfl[:, None]).any(0)
            lo = np.flatnonzero(over)[0] + L, np.flatnonzero(over)[-1] + L
            assert (lo[0] - c0) // 8 == (lo[1] - c0) // 8 == (k - c0) // 8 and lo[0] >= c0, (c.name, lo)
    # reuse
    assert len(fails(CASES["reuse-fail-768"])) == 768 and CASES["reuse-pass-290"].M % 32 and not fails(CASES["reuse-pass-290"])
    assert CASES["reuse-m255"].M == 255 and CASES["reuse-m256"].M == 256
    for seq in E.SEQUENCES.values():
        assert all(n in CASES for n in seq)
    assert [CASES[n].ch for n in E.SEQUENCES["channels"]] == [2, 8, 3, 2]


def test_the_families_cover_what_they_claim():
    cs = [c for c in CASES.values()]
    assert {c.ch for c in cs} >= {1, 2, 4, 8} and {c.ch for c in cs} & {3, 5, 6, 16}           # every loader
    assert any(c.ch in (1, 2, 4) and fails(c) for c in cs) and any(c.ch not in (1, 2, 4) and fails(c) for c in cs)
    # a failing last row where M is no multiple of 4, 16 or 32
    assert any(c.M - 1 in fails(c) and c.M % 4 and c.M % 16 and c.M % 32 for c in cs)
    # single failing rows (mono) and frames (stereo) on each side of every cut, passing rows beside them
    for ch in (1, 2):
        for cut in E.CUTS:
            below, above = fails(CASES[f"b{ch}-r{cut - 1}"]), fails(CASES[f"b{ch}-r{cut}"])
            assert cut - 1 in below and cut not in below and cut in above and cut - 1 not in above
    # 32-tiles: exactly one failing row; none failing between two that fail everywhere; all failing between two clean ones
    def tiles(c):
        v = np.zeros((c.M + 31) // 32 * 32, int)
        v[fails(c)] = 1
        return v.reshape(-1, 32).sum(1)
    assert any((tiles(c) == 1).any() for c in family("boundaries"))
    assert tiles(CASES["b1-tile1-passes"])[:3].tolist() == [32, 0, 32] and tiles(CASES["b1-tile1-fails"])[:3].tolist() == [0, 32, 0]
    assert tiles(CASES["b1-r288"])[-1] == 1 and tiles(CASES["b1-r308"])[-1] == 1 and 309 - 288 < 32
    # energy confined to the first and to the last octet
    conf = {(c.sr, (c.tags["k"] - E.shape(c.sr)[1]) // 8) for c in family("octets") if c.tags["db"] == E.CONFINED}
    for sr in (44100, 48000):
        assert {(sr, 0), (sr, (1023 - E.shape(sr)[1]) // 8)} <= conf
    assert {c.sr for c in family("octets")} == set(E.RATES)
    # raw and compressed frames among the repaired rows; no raw frame among the passing ones
    raw_rep = comp_rep = raw_pass = 0
    for c in cs:
        _, taps, v = expected(c)
        fr_fail = (v.reshape(-1, c.ch) == -1).any(1)
        raw = taps.is_raw.astype(bool)
        raw_rep += int((raw & fr_fail).sum())
        comp_rep += int((~raw & fr_fail).sum())
        raw_pass += int((raw & ~fr_fail).sum())
    assert raw_rep > 0 and comp_rep > 0
    assert raw_pass == 0, "a frame whose rows all pass is raw: the claim that MODE 1 rows carry no last band would not cover it"
    for ch in (4, 8):          # K3 at 8 channels and the fused decision at 4 see repaired rows of both kinds
        assert expected(CASES[f"ch{ch}-noise-raw"])[1].is_raw.all() and not expected(CASES[f"ch{ch}-noise"])[1].is_raw.any()


# -------------------------------------------------------------------------------------- the drivers' rows (CPU)

_driver = {}
# rows the model leaves undecided per driver input: what opens the GPU tests' lo..hi window of repaired rows, and no more
UNDECIDED = {"encode": 1, "encode16": 1, "batch": 4, "rt-planar-ch2": 4, "rt-interleaved-ch3": 5, "rt-clip": 0}


def driver(name):
    """name -> (Case of the rows the driver launches, oracle taps, model), once."""
    if name not in _driver:
        if name == "encode":
            c = E.whole_case("encode", SR, E.ENCODE_CH, E.encode_clip())
        elif name == "encode16":       # the same clip as 16-bit integers, widened as the device widens them
            c = E.whole_case("encode16", SR, E.ENCODE_CH, E.encode_clip_i16().astype(F32) / F32(32768.0))
        elif name == "batch":
            c = E.virtual_case("batch", SR, 2, E.encode_batch_clips())
        elif name == "rt-clip":
            c = E.whole_case("rt-clip", SR, 2, E.roundtrip_clip().reshape(-1, 2))
        else:
            _, sr, ch, _, clips = next(b for b in E.roundtrip_batches() if b[0] == name)
            c = E.virtual_case(name, sr, ch, clips)
        _, taps = E.expected(c)
        _driver[name] = (c, taps, E.model(c, taps))
    return _driver[name]


def frame_view(c, v):
    return v.reshape(-1, c.ch)


def test_driver_rows_are_decided_where_the_cases_rely_on_them():
    # glc_encode: 8 channels, rounds of 256 / 256 / rest frames, every one of them at least 256 rows
    c, taps, v = driver("encode")
    nf = c.f1
    rounds = E.encode_rounds(nf, c.ch)
    assert len(rounds) == 3 and [r[1] for r in rounds[:2]] == [256, 256] and all(n * c.ch >= 256 for _, n in rounds)
    fv = frame_view(c, v)
    # only rows of the frames that touch the zero padding - the first, the last two - may be undecided: 1 row is
    und = np.flatnonzero((fv == 0).any(1))
    assert set(und.tolist()) <= {0, nf - 2, nf - 1} and (v == 0).sum() <= UNDECIDED["encode"]
    a, b = E.ENCODE_NOISE
    assert (fv[a:b] == -1).all()                                               # the noise, all of it in round 1 (slot 1)
    assert rounds[1][0] <= a - 1 and b + 1 <= rounds[1][0] + rounds[1][1]
    for f in E.ENCODE_CLICKS:
        assert fv[f].tolist() == [1] * 5 + [-1] + [1] * 2                          # the clicked row of 8
    quiet = np.ones(nf, bool)
    quiet[[0, nf - 2, nf - 1, *E.ENCODE_CLICKS]] = False
    quiet[a - 1:b + 1] = False
    assert (fv[quiet] == 1).all()
    assert rounds[0][0] <= E.ENCODE_CLICKS[0] < rounds[1][0] and rounds[2][0] <= E.ENCODE_CLICKS[1]
    c16, _, v16 = driver("encode16")
    assert c16.f1 == nf and (v16 == 0).sum() <= UNDECIDED["encode16"] and (frame_view(c16, v16)[a:b] == -1).all()
    for f in E.ENCODE_CLICKS:
        assert frame_view(c16, v16)[f].tolist() == [1] * 5 + [-1] + [1] * 2
    # the batch drivers: the virtual stream.  Its junk frames are rows of the launch like any other: each holds the
    # tail of one clip and the head of the next under the window's two halves, or zeros, and the model decides it
    # from the stream's samples as it decides every row.  Undecided: only rows of the frames that touch a clip's
    # padding - its first, its last two, the junk frame behind it - and of those 4, 4 and 5 rows (UNDECIDED).
    for name in ("batch", "rt-planar-ch2", "rt-interleaved-ch3"):
        c, taps, v = driver(name)
        assert c.M >= 256
        fv = frame_view(c, v)
        und = set(np.flatnonzero((fv == 0).any(1)).tolist())
        may = set()
        for i, (at, n) in enumerate(c.slots):
            may |= {at, at + n - 2, at + n - 1, at + n}
            kind = i % 5
            inner = fv[at + 1:at + n - 2]
            if kind == 1:
                assert (inner == -1).all(), (name, i)
            elif kind == 2:
                assert (fv[at:at + n] == 1).all(), (name, i)             # silence passes, padding or not
            else:
                lo = 2 if kind == 3 else 1                               # (a click at sample 512 is in frame 1's window too)
                assert (fv[at + lo:at + n - 2] == 1).all(), (name, i)
            if kind == 3:
                assert (fv[at] == -1).all(), (name, i)
            if kind == 4:
                assert (fv[at + n - 1] == -1).all(), (name, i)
        assert und <= may and (v == 0).sum() <= UNDECIDED[name], (name, sorted(und - may), int((v == 0).sum()))
    c, taps, v = driver("rt-clip")
    fv = frame_view(c, v)
    assert c.M >= 256 and (fv[70] == -1).all() and (np.delete(fv, [0, 70, c.f1 - 2, c.f1 - 1], 0) == 1).all()
    assert (v == 0).sum() == UNDECIDED["rt-clip"] == 0


# -------------------------------------------------------------------------------------- power

_rows = {}


def model_records(c, mut=None, stale=None):
    rec, taps, _ = expected(c)
    if c.name not in _rows:
        _rows[c.name] = E.Rows(c, taps)
    return E.screen_records(c, _rows[c.name], rec, E.flags(c, taps, mut), mut, stale)


def test_the_record_model_equals_the_oracle_and_every_mutation_of_it_is_seen():
    """The model is the proof restated: a passing row quantised from the columns below C0 with the last band's base
    at 0, a failing row from the oracle.  Unmutated it gives the oracle's bytes for every case.  Mutated - one edit
    at a time - it must differ from the oracle in a byte of a case of the family the edit is aimed at, or, where
    the bytes provably cannot differ, in the count of repaired rows, which the GPU tests compare exactly."""
    for name, c in CASES.items():
        got, count, stray = model_records(c)
        assert np.array_equal(got, expected(c)[0]), f"{name}: the unmutated model differs from the oracle"
        assert count == len(fails(c)) and not stray
    aimed = {1: "octets", 2: "octets", 3: "octets", 4: "octets", 5: "octets", 6: "octets", 7: "boundaries", 8: "boundaries",
             9: "boundaries", 11: "channels"}
    by_bytes, by_count = {}, {}
    for mut, fam in aimed.items():
        for c in family(fam):
            got, count, _ = model_records(c, mut)
            if not np.array_equal(got, expected(c)[0]):
                by_bytes.setdefault(mut, []).append(c.name)
            elif count != len(fails(c)):
                by_count.setdefault(mut, []).append(c.name)
    # 10 is a sequence: the flags the all-fail launch of 768 rows left behind row 290 of the next one.  MODE 2's
    # group of rows 288..303 would write rows 290..303 - records behind the launch's last, which the GPU tests
    # catch as guard bytes (the count is formed from wave_fail, which the launch writes afresh: it does not move)
    big, small = CASES["reuse-fail-768"], CASES["reuse-pass-290"]
    stale = E.flags(big, expected(big)[1])
    got, count, stray = model_records(small, 10, stale)
    assert count == 0 and stray == list(range(290, 304))
    by_bytes[10] = [f"{small.name} after {big.name} (rows {stray[0]}..{stray[-1]} written behind the records: guard bytes)"]
    neutral = {
        4: "count: a row that only kScreenCErr A fails has nothing over the floor (the bound without A is still an upper "
           "bound of the oracle's |c| up to the distance A covers), so its record is the same from either path",
        5: "count: a lone bin L over the floor is quantised by MODE 1 as by the oracle (the last band's base is 0 there "
           "and the oracle's threshold, 0.003 pf indiv scale rms, is at most half the bin at 44.1 / 48 kHz: DESIGN section 6)",
        6: "count: as 5, for bin C0 - 1",
        11: "count: the sibling row passes on its own, so MODE 1 writes the oracle's bytes for it; 1 row per clicked frame instead of 4",
    }
    report = {m: ("bytes", by_bytes[m][:3]) if m in by_bytes else ("count", by_count.get(m, [])[:3]) for m in sorted(E.MUTATIONS)}
    msg = "; ".join(f"{m} ({E.MUTATIONS[m]}): {how} {names}" for m, (how, names) in report.items())
    for m in (1, 2, 3, 7, 8, 9, 10):
        assert m in by_bytes, f"mutation {m} ({E.MUTATIONS[m]}) changes no byte of any case - {msg}"
    for m in (4, 5, 6, 11):
        assert m not in by_bytes and by_count.get(m), f"mutation {m} ({E.MUTATIONS[m]}): {neutral[m]} - but {msg}"
    # the cases DESIGN section 6 names for a reviewer's two hand edits of the kernels
    assert "b1-r32" in by_bytes[7] and "oct-48000-k1020" in by_bytes[3] and "oct-48000-k387" in by_bytes[2], msg
    assert "b1-r308" in by_bytes[8] and "b1-r15" in by_bytes[9], msg
    assert by_count[5] == ["oct-44100-k371", "oct-48000-k341"] and by_count[6] == ["oct-44100-k383", "oct-48000-k383"], msg
    assert by_count[11] == ["ch4-clicks"], msg
    assert by_count[4] == ["sub-44100-k387", "sub-48000-k1020"], msg       # 48 rows repaired with A, none without


def test_bound_holds_for_the_new_value_shapes():
    """Eight rows per case, the failing ones first: the octet lines and the clicks at 4 .. 16 channels."""
    for c in CASES.values():
        if c.tags.get("values") not in ("line", "click"):
            continue
        v = expected(c)[2]
        pick = np.concatenate([np.flatnonzero(v == -1)[:4], np.flatnonzero(v == 1)[:4]])
        E.S.assert_bound(E.windowed_rows(c)[pick], c.name)


# ----------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    import glc_amd
    E.S.bind(glc_amd)
    encoders = {}

    def encoder(key):
        if key not in encoders:
            encoders[key] = glc_amd.Encoder(key if isinstance(key, int) else SR)
        return encoders[key]
    yield torch, glc_amd, encoder
    for e in encoders.values():
        e.close()


def _launch_and_check(gpu, enc, c, label=""):
    """The case in mode 2 and in mode 1: bytes, guard pages (in _records), counts."""
    exp, _, v = expected(c)
    name = label + c.name
    on, screened, repaired = E.S.records(gpu[0], gpu[1], enc, c, 2)
    off, screened_off, repaired_off = E.S.records(gpu[0], gpu[1], enc, c, 1)
    print(f"{name}: M {c.M}, screened {screened}, repaired {repaired}, model {int((v == -1).sum())}")
    assert (screened_off, repaired_off) == (0, 0), f"{name}: mode 1 took the screened path"
    assert np.array_equal(off, exp), f"{name}, screen off: {E.S.explain(off, exp, c.ch)}"
    assert np.array_equal(on, exp), f"{name}, screen on: {E.S.explain(on, exp, c.ch)}"
    assert np.array_equal(on, off)
    if c.M < 256:
        assert (screened, repaired) == (0, 0), f"{name}: a launch of {c.M} rows was screened"
    else:
        assert screened == c.M, f"{name}: {screened} of {c.M} rows went through the screened path"
        assert repaired == int((v == -1).sum()), f"{name}: {repaired} rows repaired, the model has {int((v == -1).sum())}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", RANGE_NAMES)
def test_gpu_range_cases_equal_the_oracle_and_repair_exactly_the_models_rows(gpu, name):
    c = CASES[name]
    _launch_and_check(gpu, gpu[2](c.sr), c)


@pytest.mark.gpu
@pytest.mark.parametrize("seq", list(E.SEQUENCES))
def test_gpu_one_workspace_reused_by_a_sequence_of_launches(gpu, seq):
    """All sequences on ONE context, whose workspace was sized by the largest launch so far: stale hf planes, flags
    and wave counts lie behind every smaller one.  After the 768-row launch that failed everywhere, the 290-row
    launch that passes everywhere must report 0 repaired rows and leave its guard pages alone: no flag at an index
    >= M was consulted."""
    enc = gpu[2]("reuse")
    for i, name in enumerate(E.SEQUENCES[seq]):
        _launch_and_check(gpu, enc, CASES[name], f"{seq}[{i}] ")


@pytest.mark.gpu
# the FMA form (k_mdct_mix_st) with either PCM loader, the matrix form (k_mdct_mx_st: built for 1 / 2 / 4 / 8 channels)
@pytest.mark.parametrize("ch, bound", ((2, 1), (2, 2), (3, 1)))
def test_gpu_tight_shard_with_nan_on_both_sides_under_both_forms_and_both_repairs(gpu, ch, bound):
    """The mixed-role transforms and the latency repair (k_mdct_fwd_small_rows) read their PCM through the same
    descriptor rules as the exact kernels, whose guards cases tests/test_k1_edges.py holds: a shard with t0 > 0 that
    ends inside the stream, NaN in front of it and behind it, a last tile that is not full.  Records byte for byte."""
    torch, glc_amd, encoder = gpu
    c = E.guarded_shard_case(ch)
    exp, taps = E.expected(c)
    v = E.model(c, taps)
    _, t0, tc = c.shard()
    assert t0 > 0 and (t0 + tc) * c.ch < c.n_samples and c.M % 256 and c.M % 128 and 0 < int((v == -1).sum())
    enc = encoder("guarded")
    lib = glc_amd.lib
    try:
        assert lib.glc_debug_set_encode_bound(enc._h, bound) == 0
        for repair in (2, 1):                   # k_mdct_fwd_small_rows, k_mdct_fwd_small_cols
            assert lib.glc_debug_set_encode_repair(enc._h, repair) == 0
            got, screened, repaired = E.S.records(torch, glc_amd, enc, c, 2, nan_pad=16384)
            assert np.array_equal(got, exp), f"bound {bound}, repair {repair}: {E.S.explain(got, exp, c.ch)}"
            assert screened == c.M and int((v == -1).sum()) <= repaired <= int((v != 1).sum()), (bound, repair, screened, repaired)
    finally:
        assert lib.glc_debug_set_encode_bound(enc._h, 0) == 0 and lib.glc_debug_set_encode_repair(enc._h, 0) == 0


def _set(glc_amd, ctx, mode):
    assert glc_amd.lib.glc_debug_set_encode_screen(ctx._h, mode) == 0


def _delta(glc_amd, ctx, s0):
    s1 = E.S.stats(glc_amd, ctx)
    return s1[0] - s0[0], s1[1] - s0[1]


BOUND_KINDS = (0, 2)      # automatic - the FMA form at these row counts - and the matrix form forced wherever it is built


def _set_bound(glc_amd, ctx, kind):
    assert glc_amd.lib.glc_debug_set_encode_bound(ctx._h, kind) == 0


_oracle = {}


def oracle_stream(key, x, sr, ch):
    if key not in _oracle:
        glc = O.encode(x, sr, ch).glc
        _oracle[key] = (glc, O.decode(glc)[0])
    return _oracle[key]


def _bounds(name):
    v = driver(name)[2]
    return int((v == -1).sum()), int((v != 1).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("bound", BOUND_KINDS)
def test_gpu_glc_encode_screens_every_round_on_both_workspace_slots(gpu, bound):
    """Encoder.encode of 690 frames of 8 channels: three rounds, the middle one - on the second stream, workspace
    slot 1 - with 40 frames of noise; float32, and the same clip as int16.  Bound kind 2: the rounds take the matrix
    form's 8-channel segment loader (the kind outlives the screen's setter)."""
    torch, glc_amd, _ = gpu
    c = driver("encode")[0]
    x = E.encode_clip().reshape(-1)
    ref = oracle_stream("encode", x, SR, c.ch)[0]
    x16 = E.encode_clip_i16().reshape(-1)
    ref16 = oracle_stream("encode16", (x16.astype(F32) / F32(32768.0)), SR, c.ch)[0]
    lo, hi = _bounds("encode")
    lo16, hi16 = _bounds("encode16")
    enc = glc_amd.Encoder(SR)
    try:
        _set_bound(glc_amd, enc, bound)
        _set(glc_amd, enc, 2)
        s0 = E.S.stats(glc_amd, enc)
        on = enc.encode(x, c.ch).to_bytes()
        screened, repaired = _delta(glc_amd, enc, s0)
        print(f"glc_encode: screened {screened} of {c.M}, repaired {repaired}, model {lo}..{hi}")
        assert on == ref, "mode 2: the stream differs from the oracle's"
        assert screened == c.M and lo <= repaired <= hi
        s0 = E.S.stats(glc_amd, enc)
        on16 = enc.encode(x16, c.ch, bits=16).to_bytes()
        screened, repaired = _delta(glc_amd, enc, s0)
        assert on16 == ref16, "mode 2, int16: the stream differs from the oracle's of the widened samples"
        print(f"glc_encode, int16: screened {screened} of {c.M}, repaired {repaired}, model {lo16}..{hi16}")
        assert screened == c.M and lo16 <= repaired <= hi16
        _set(glc_amd, enc, 1)
        s0 = E.S.stats(glc_amd, enc)
        off = enc.encode(x, c.ch).to_bytes()
        assert _delta(glc_amd, enc, s0) == (0, 0)
        assert off == ref, "mode 1: the stream differs from the oracle's"
    finally:
        _set_bound(glc_amd, enc, 0)
        enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bound", BOUND_KINDS)
def test_gpu_encode_batch_screens_the_virtual_stream_junk_frames_included(gpu, bound):
    """20 stereo clips of 5..9 frames in one round: 160 virtual frames, 320 rows, the 20 junk frames among them.
    They count as screened - they are rows of the launch - and the repaired bound treats them like every row: the
    model, run on the virtual stream of DESIGN section 3, decides them."""
    torch, glc_amd, _ = gpu
    clips = E.encode_batch_clips()
    refs = [oracle_stream(("batch", i), x, SR, 2)[0] for i, x in enumerate(clips)]
    c = driver("batch")[0]
    lo, hi = _bounds("batch")
    enc = glc_amd.Encoder(SR)
    try:
        _set_bound(glc_amd, enc, bound)
        _set(glc_amd, enc, 2)
        s0 = E.S.stats(glc_amd, enc)
        on = [e.to_bytes() for e in enc.encode_batch(clips, 2)]
        screened, repaired = _delta(glc_amd, enc, s0)
        print(f"glc_encode_batch: screened {screened} of {c.M}, repaired {repaired}, model {lo}..{hi}")
        for i, (got, ref) in enumerate(zip(on, refs)):
            assert got == ref, f"mode 2: clip {i} differs from the oracle's encode of it alone"
        assert screened == c.M == 320 and lo <= repaired <= hi
        _set(glc_amd, enc, 1)
        s0 = E.S.stats(glc_amd, enc)
        off = [e.to_bytes() for e in enc.encode_batch(clips, 2)]
        assert _delta(glc_amd, enc, s0) == (0, 0)
        assert off == on
    finally:
        _set_bound(glc_amd, enc, 0)
        enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bound", BOUND_KINDS)
def test_gpu_round_trips_decode_the_records_the_screen_and_the_repair_left(gpu, bound):
    """RoundTrip on one clip (298 rows, a clicked frame repaired in front of the decode of the same round) and
    apply_batch_tensor on a planar stereo and an interleaved 3-channel batch (278 / 285 rows of virtual stream):
    the output words are the oracle's decode of its own encode per clip, the NaN pattern everywhere else.  Bound kind 2:
    the stereo launches take the matrix form; the 3-channel batch, which the form is not built for, keeps the FMA one."""
    import test_roundtrip_batch as RB
    torch, glc_amd, _ = gpu
    rt = glc_amd.RoundTrip(SR)
    try:
        _set_bound(glc_amd, rt, bound)
        for mode in (2, 1):
            _set(glc_amd, rt, mode)
            x = E.roundtrip_clip()
            c = driver("rt-clip")[0]
            lo, hi = _bounds("rt-clip")
            s0 = E.S.stats(glc_amd, rt)
            y = rt.apply_tensor(torch.from_numpy(x).cuda(), 2)
            rt.synchronize()
            got = y.cpu().numpy()
            screened, repaired = _delta(glc_amd, rt, s0)
            assert np.array_equal(RB.bits(got), RB.bits(oracle_stream("rt-clip", x, SR, 2)[1])), f"mode {mode}: single clip"
            assert (screened, repaired) == (0, 0) if mode == 1 else (screened == c.M and lo <= repaired <= hi), (mode, screened, repaired)
            for name, sr, ch, planar, clips in E.roundtrip_batches():
                c = driver(name)[0]
                lo, hi = _bounds(name)
                refs = [oracle_stream((name, i), xc, sr, ch)[1] for i, xc in enumerate(clips)]
                b = RB.Batch(clips, ch, planar, lead=5, tail=3)
                s0 = E.S.stats(glc_amd, rt)
                RB.run(torch, rt, b, b.like(planar, lead=2, tail=7), refs)
                screened, repaired = _delta(glc_amd, rt, s0)
                print(f"{name}, mode {mode}: screened {screened} of {c.M}, repaired {repaired}, model {lo}..{hi}")
                assert (screened, repaired) == (0, 0) if mode == 1 else (screened == c.M and lo <= repaired <= hi), (name, mode, screened, repaired)
    finally:
        _set_bound(glc_amd, rt, 0)
        rt.close()
