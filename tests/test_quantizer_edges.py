"""The quantiser kernels at their decision boundaries (tests/quant_edges.py builds the rows).

CPU: the two oracles agree on every generated row, the families cover what they claim, the expected
records hold the hand-derived answers, and mutated copies of the numpy quantiser (one edit each, the kind
of edit a kernel change could make) all change at least one expected record - so the GPU test below would
notice them.  GPU: K2 / K3 through glc_debug_quantize_device (include/glc_debug.h), record bytes against
the expected ones, sentinel bytes where no kernel may write; and the records of the raw-decision family
assembled into a .glc stream and parsed back."""
import ctypes as C

import numpy as np
import pytest

import quant_edges as Q
from oracle import glc_oracle_np as N
from oracle import oracle as O

F32 = np.float32
GLC_EINVAL = -1  # include/glc.h


@pytest.fixture(scope="module")
def cases():
    return Q.cases()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _by_name(cs):
    return {c.name: c for c in cs}


# ----------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------

def test_generator_is_deterministic(cases):
    assert Q.digest(Q.build_cases()) == Q.digest(cases)


def test_c_oracle_and_numpy_oracle_agree_on_every_row(cases):
    for c in cases:
        w, edges = Q.perceptual(c.sr)
        with np.errstate(all="ignore"):
            thr, gmax = N.thresholds_rows(c.coeffs, w, edges)
            q = N.quantise_rows(c.coeffs, gmax, thr)
        assert np.array_equal(_bits(gmax), _bits(c.scale)), c.name
        assert np.array_equal(q, c.q), f"{c.name}: {(q != c.q).sum()} q differ"
        thr_c = Q.oracle_rows(c.coeffs, c.sr)[1]
        assert np.array_equal(_bits(thr), _bits(thr_c)), f"{c.name}: thresholds differ"
        s2, q2 = Q.quantise(c.coeffs, c.sr)  # the restatement the power check mutates
        assert np.array_equal(_bits(s2), _bits(c.scale)) and np.array_equal(q2, c.q), c.name


def test_families_cover_what_they_claim(cases):
    by = _by_name(cases)
    assert {c.family for c in cases} == {"thresholds", "noise_floor", "peak_gate", "rounding", "extremes", "raw"}
    # K2 phase 2: the rates between them take every body-loop step count 0..8 plus the long bands
    steps = set()
    for sr in Q.RATES:
        _, e = Q.perceptual(sr)
        steps |= {Q.body_steps(int(e[b]), int(e[b + 1])) for b in range(len(e) - 1)}
    assert steps == Q.BODY_STEPS
    assert list(Q.perceptual(100)[1]) == [0, 1024]  # one band spans the row
    regimes = set()
    for sr in Q.RATES:
        c = by[f"thresholds-{sr}-ch1"]
        _, e = Q.perceptual(sr)
        band_of = np.searchsorted(e, np.arange(Q.HOP), side="right") - 1
        seen = {}
        for r, k, side, regime in c.info["flips"]:
            seen.setdefault(int(band_of[k]), set()).add((r % 16, side))
            regimes.add(regime)
        for b in range(len(e) - 1):
            got = seen.get(b, set())
            assert {p for p, _ in got} == set(range(16)), f"{sr} Hz band {b}: flips at row positions {sorted(got)}"
            assert {s for _, s in got} == {0, 1}, f"{sr} Hz band {b}: one side of the edge only"
    assert regimes == {"thr", "floor"}
    for ch in Q.CHANNELS:
        c = by[f"raw-44100-ch{ch}"]
        flip, totals = c.info["flip"], c.info["totals"]
        assert {t - flip for t in totals[Q.RAW_LEAD:]} == {-1, 0, 1}
        launched = c.is_raw[Q.RAW_LEAD:]
        assert (np.diff(launched.astype(int)) != 0).sum() >= 4  # neighbouring frames decide differently
        if ch > 1:
            nnz = (c.q != 0).sum(axis=1)[Q.RAW_LEAD * ch:]
            assert (nnz == 1024).any() and ((nnz > 0) & (nnz < 1024)).any()
            if Q.HOP * (ch - 1) > flip + 1:  # an empty channel fits beside the others (7, 8 and 16 channels)
                assert (nnz == 0).any()
        assert np.isnan(c.stream).any() and np.isinf(c.stream).any() and (np.abs(c.stream[np.isfinite(c.stream)]) > 1).any()
    assert len(by["peak_gate-192000-ch2"].info["marks"]) >= 2


def test_expected_records_hold_the_known_answers(cases):
    by = _by_name(cases)
    # raw-or-compressed flip points (src/codec.rs:505-521 in f32); 5 channels flips on an exact equality
    assert {ch: Q.flip_point(ch) for ch in Q.CHANNELS} == \
        {1: 850, 2: 1717, 3: 2585, 4: 3452, 5: 4319, 6: 5187, 7: 6054, 8: 6922, 16: 13861}
    assert F32(8 * 5 + 4 * 4319 + 8 + 4 * 5 + 64) == Q.raw_threshold(5) == F32(17408)
    for c in cases:
        nnz = (c.q != 0).sum(axis=1)
        if c.family == "raw":
            totals = np.array(c.info["totals"])
            assert np.array_equal(nnz.reshape(-1, c.ch).sum(axis=1), totals)
            assert np.array_equal(c.is_raw, totals >= c.info["flip"])
        if c.family == "thresholds":
            for r, k, side, _ in c.info["flips"]:
                assert (c.q[r, k] != 0) == bool(side), f"{c.name} row {r} bin {k}"
        if c.family == "noise_floor":
            assert Q.NOISE_FLOOR.view(np.uint32) == 0x3B8273A5
            for r, x, y in c.info["marks"]:
                assert abs(c.coeffs[r, x]) == F32(Q.NOISE_FLOOR * c.scale[r])
                assert c.q[r, x] == 0 and c.q[r, y] != 0, f"{c.name} row {r}"
        if c.family == "peak_gate":
            for r, k in c.info["marks"][0::2]:
                assert c.coeffs[r, k] == F32(c.scale[r] * F32(0.3)) and c.q[r, k] == 0
            for r, k in c.info["marks"][1::2]:
                assert c.coeffs[r, k] == np.nextafter(F32(c.scale[r] * F32(0.3)), F32(np.inf)) and c.q[r, k] != 0
        if c.family == "rounding":
            for r, k, qv in c.info["expect"]:
                assert c.scale[r] == 1.0 and c.q[r, k] == qv, f"row {r} bin {k}: {c.q[r, k]} != {qv}"
        if c.family == "extremes" and c.ch == 1:
            names = c.info["names"]
            w, edges = Q.perceptual(c.sr)
            for r, name in enumerate(names):
                row, thr = c.coeffs[r], O.thresholds(c.coeffs[r], w, edges)
                if name in ("zero", "subnormal"):
                    assert c.scale[r] == F32(1e-10) and nnz[r] == 0
                if name == "negative_max":
                    at = row == row.min()
                    assert at.sum() == 5 and c.scale[r] == -row.min() and np.all(c.q[r, at] == -32768)
                if name == "overflow":
                    peak = np.abs(row) > c.scale[r] * F32(0.3)
                    assert np.isinf(thr[~peak]).any() and np.isfinite(thr[peak]).all() and nnz[r] == 0
                if name.startswith("nan"):
                    k = int(np.flatnonzero(np.isnan(row))[0])
                    b = np.searchsorted(edges, k, side="right") - 1
                    band = slice(int(edges[b]), int(edges[b + 1]))
                    peak = np.abs(row[band]) > c.scale[r] * F32(0.3)
                    assert c.scale[r] == np.nanmax(np.abs(row)) and c.q[r, k] == 0
                    assert np.isnan(thr[band][~peak]).all() and np.isfinite(thr[band][peak]).all() and peak.any()
                    assert np.all(c.q[r, band][peak] != 0) and np.all(c.q[r, band][~peak] == 0)
                if name == "inf":
                    assert np.isinf(c.scale[r]) and nnz[r] == 0


def _records_under(c, mut):
    scale, q = Q.quantise(c.coeffs, c.sr, mut)
    is_raw = Q.decide((q != 0).sum(axis=1), c.ch, mut)
    return Q.build_records(c.ch, scale, q, is_raw, c.planes)


def test_power_every_mutation_changes_an_expected_record(cases):
    """Each mutated copy of the quantiser must change at least one expected record, and the band-sum ones
    must do so at every sample rate: this is what makes the GPU test below able to catch such an edit of
    K2 / K3."""
    for c in cases:
        assert np.array_equal(_records_under(c, None), c.expected), c.name
    caught = {}
    for mut in Q.MUTATIONS:
        caught[mut] = {c.name for c in cases if not np.array_equal(_records_under(c, mut), c.expected)}
    missed = [m for m, names in caught.items() if not names]
    assert not missed, f"mutations no expected record notices: {missed}"
    for mut in ("sum_two_acc", "sum_descending"):
        rates = {c.sr for c in cases if c.family == "thresholds" and c.name in caught[mut]}
        assert rates == set(Q.RATES), f"{mut} goes unnoticed at {sorted(set(Q.RATES) - rates)} Hz"


# ----------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    import glc_amd
    f = glc_amd.lib.glc_debug_quantize_device
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint16,
                  C.c_uint64, C.c_uint64, C.c_void_p]
    return torch, glc_amd


_NAN_ROWS = 16


def _launch(gpu, sr, ch, rows, stream, n_samples, frame_begin, t0, expect_rc=0):
    """K2 / K3 on `rows` (the frames [frame_begin, n_frames) of the stream) -> the records of those frames
    plus one spare record, all of which started as sentinel bytes."""
    torch, glc_amd = gpu
    L = n_samples // ch
    nf = rows.shape[0] // ch
    rec = Q.record_bytes(ch)
    d_coef = torch.full((rows.shape[0] + _NAN_ROWS, Q.HOP), float("nan"), dtype=torch.float32, device="cuda")
    d_coef[:rows.shape[0]] = torch.from_numpy(np.ascontiguousarray(rows))
    if stream is None:
        d_pcm = torch.zeros((L - t0) * ch, dtype=torch.float32, device="cuda")
    else:
        d_pcm = torch.from_numpy(np.ascontiguousarray(stream[t0 * ch:])).cuda()
    d_rec = torch.full(((nf + 1) * rec,), Q.SENTINEL, dtype=torch.uint8, device="cuda")
    enc = glc_amd.Encoder(sr)
    torch.cuda.synchronize()
    rc = glc_amd.lib.glc_debug_quantize_device(enc._h, d_coef.data_ptr(), d_pcm.data_ptr(), t0, L - t0, n_samples, ch,
                                               frame_begin, frame_begin + nf, d_rec.data_ptr())
    assert rc == expect_rc, glc_amd.lib.glc_last_error(enc._h)
    enc.synchronize()
    return d_rec.cpu().numpy().reshape(nf + 1, rec)


def _explain(got, exp, ch):
    hdr = Q.header_bytes(ch)
    bad = np.flatnonzero((got != exp).any(axis=1))
    f = int(bad[0])
    cols = np.flatnonzero(got[f] != exp[f])
    where = "header" if cols[0] < hdr else f"payload channel {(cols[0] - hdr) // 4096} i16 {((cols[0] - hdr) % 4096) // 2}"
    return f"{bad.size} records differ; first: record {f}, {cols.size} bytes, from byte {cols[0]} ({where})"


def _check(got, exp, ch, what):
    spare = np.full((1, Q.record_bytes(ch)), Q.SENTINEL, np.uint8)
    exp = np.concatenate([exp, spare])
    assert np.array_equal(got, exp), f"{what}: {_explain(got, exp, ch)}"


def _case_ids():
    return [c.name for c in Q.cases()]


@pytest.mark.gpu
@pytest.mark.parametrize("name", _case_ids())
def test_gpu_records_at_the_edges(gpu, cases, name):
    c = _by_name(cases)[name]
    fb = c.frame_begin
    got = _launch(gpu, c.sr, c.ch, c.coeffs[fb * c.ch:], c.stream, c.n_samples, fb, c.t0)
    _check(got, c.expected[fb:], c.ch, name)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 3, 4, 5, 15, 16, 17, 4095, 4097, (1 << 16) + 5])
def test_gpu_launch_sizes(gpu, cases, M):
    c = _by_name(cases)["thresholds-44100-ch1"]
    pick = np.arange(M) % c.n_frames
    got = _launch(gpu, c.sr, 1, c.coeffs[pick], None, M * Q.HOP, 0, 0)
    _check(got, c.expected[pick], 1, f"M={M}")


@pytest.mark.gpu
def test_gpu_entry_point_checks_its_arguments(gpu, cases):
    torch, glc_amd = gpu
    c = _by_name(cases)["raw-44100-ch3"]
    enc = glc_amd.Encoder(c.sr)
    d = torch.zeros(c.n_samples + 8 * Q.HOP, dtype=torch.float32, device="cuda")
    f = glc_amd.lib.glc_debug_quantize_device
    L, fb = c.n_samples // c.ch, c.frame_begin
    ok = (enc._h, d.data_ptr(), d.data_ptr(), c.t0, L - c.t0, c.n_samples, c.ch, fb, c.n_frames, d.data_ptr())
    bad = [dict(i=1, v=None), dict(i=2, v=None), dict(i=9, v=None),        # null coefficients / PCM / records
           dict(i=3, v=c.t0 + 1), dict(i=4, v=L - c.t0 - 1),               # shard misses the halo
           dict(i=8, v=c.n_frames + 1), dict(i=7, v=c.n_frames + 1),       # frame range out of bounds
           dict(i=6, v=0), dict(i=5, v=100)]                               # no channels / the reference panics
    for b in bad:
        args = list(ok)
        args[b["i"]] = b["v"]
        assert f(*args) == GLC_EINVAL, (b, glc_amd.lib.glc_last_error(enc._h))
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("ch", Q.CHANNELS)
def test_gpu_records_make_the_expected_glc(gpu, cases, ch):
    """The GPU records of the raw-decision family, whole stream, through EncodedAudio.from_records and the
    .glc serialiser, parsed back: index / value lists, scales and raw planes as expected."""
    _, glc_amd = gpu
    from conftest import parse_glc
    c = _by_name(cases)[f"raw-44100-ch{ch}"]
    got = _launch(gpu, c.sr, ch, c.coeffs, c.stream, c.n_samples, 0, 0)
    _check(got, c.expected, ch, c.name)
    g = parse_glc(glc_amd.EncodedAudio.from_records(c.sr, c.n_samples, ch, got[:-1]).to_bytes())
    assert (g["sample_rate"], g["channels"], g["total_samples"]) == (c.sr, ch, c.n_samples)
    assert len(g["frames"]) == c.n_frames
    for f, fr in enumerate(g["frames"]):
        if c.is_raw[f]:
            assert fr["lists"] == [] and fr["scales"].size == 0
            assert np.array_equal(fr["raw"], c.planes[f].reshape(-1)), f"frame {f}: raw plane"
            continue
        assert fr["raw"] is None and len(fr["lists"]) == ch
        assert np.array_equal(_bits(fr["scales"]), _bits(c.scale[f * ch:(f + 1) * ch])), f"frame {f}: scales"
        for k, (idx, q) in enumerate(fr["lists"]):
            row = c.q[f * ch + k]
            assert np.array_equal(idx, np.flatnonzero(row)) and np.array_equal(q, row[row != 0]), f"frame {f} ch {k}"
