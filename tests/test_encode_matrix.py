"""The matrix form of the screened transform on the device (k_mdct_mx_st; DESIGN.md sections 2 and 4).

The instruction against the error model the budget rests on; H and A as the quantiser reads them, against the real sums;
record bytes against the oracle with the matrix form, the FMA form and no screen, and the repaired rows against the
model's window - so a form that is silently off, or that repairs everything, does not pass; the value edges; the
setter's rules."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_matrix_cases as X  # noqa: E402
import encode_screen_cases as S  # noqa: E402
from encode_screen_cases import C_ERR, F32, FRAME, GAMMA, HOP, SLACK, TINY, Case  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
LOW = ([220.0, 1234.5, 3100.0, 6900.0], [0.3, 0.2, 0.1, 0.05])


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    import glc_amd
    S.bind(glc_amd)
    lib = glc_amd.lib
    lib.glc_debug_set_encode_bound.restype, lib.glc_debug_set_encode_bound.argtypes = C.c_int, [C.c_void_p, C.c_int]
    lib.glc_debug_encode_bound_tap.restype = C.c_int
    lib.glc_debug_encode_bound_tap.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.glc_debug_mfma_bf16.restype = C.c_int
    lib.glc_debug_mfma_bf16.argtypes = [C.c_void_p, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    encoders = {}

    def encoder(sr):
        if sr not in encoders:
            encoders[sr] = glc_amd.Encoder(sr)
        return encoders[sr]
    yield torch, glc_amd, encoder
    for e in encoders.values():
        e.close()


_expected = {}


def expected(case):
    """(oracle records, taps, model) of a case, computed once per session."""
    if case.name not in _expected:
        rec, taps = S.expected(case)
        _expected[case.name] = (rec, taps, S.model(case, taps))
    return _expected[case.name]


def records(gpu, enc, c, bound, mode):
    """One launch of the case with the bound's form and the screen's mode set -> (bytes, screened, repaired)."""
    lib = gpu[1].lib
    assert lib.glc_debug_set_encode_bound(enc._h, bound) == 0
    try:
        return S.records(gpu[0], gpu[1], enc, c, mode)
    finally:
        assert lib.glc_debug_set_encode_bound(enc._h, 0) == 0


# ---------------------------------------------------------------------------------------------------- the instruction

def _bf16_bits(x):
    return (np.ascontiguousarray(x, F32).view(np.uint32) >> 16).astype(np.uint16)


def _mfma(gpu, enc, a, b, c):
    """D = C + A B of one v_mfma_f32_32x32x16_bf16: a [32, 16], b [16, 32] f32 holding bf16 values, c [32, 32] f32."""
    lane = np.arange(64)
    ks = 8 * (lane // 32)[:, None] + np.arange(8)[None, :]
    fa = _bf16_bits(a[(lane % 32)[:, None], ks]).copy()
    fb = _bf16_bits(b[ks, (lane % 32)[:, None]]).copy()
    e = np.arange(16)
    rows = 8 * (e // 4)[None, :] + 4 * (lane // 32)[:, None] + (e % 4)[None, :]
    cols = np.broadcast_to((lane % 32)[:, None], rows.shape)
    fc = np.ascontiguousarray(c[rows, cols], F32)
    fd = np.zeros_like(fc)
    p16, pf = C.POINTER(C.c_uint16), C.POINTER(C.c_float)
    rc = gpu[1].lib.glc_debug_mfma_bf16(enc._h, fa.ctypes.data_as(p16), fb.ctypes.data_as(p16), fc.ctypes.data_as(pf), fd.ctypes.data_as(pf))
    assert rc == 0
    d = np.zeros((32, 32), F32)
    d[rows, cols] = fd
    return d


def test_the_instruction_stays_within_the_error_model(gpu):
    """|D - exact| <= kappa (|C| + sum |p|), kappa = 17 * 2^-23, on same-sign products (nothing cancels) spread over
    binades, with C much larger and much smaller than the products, and with subnormal pieces beside a normal C."""
    k = X.constants()
    enc = gpu[2](48000)
    rng = np.random.default_rng(3)
    worst, flushed = 0.0, None

    def operand(shape, spread):
        m = 1.0 + rng.integers(0, 128, shape) / 128.0                 # 8 significant bits: bf16 values
        return (m * 2.0 ** rng.integers(-spread, spread + 1, shape)).astype(F32)
    for spread in (0, 3, 12, 30):
        for c_scale in (0.0, 2.0 ** 20, 2.0 ** -20, 1.0, -1.0):
            a, b = operand((32, 16), spread), operand((16, 32), spread)
            p = a.astype(np.float64)[:, :, None] * b.astype(np.float64)[None, :, :]    # [i, k, j], each exact
            sp = p.sum(1)
            c = (c_scale * sp * (1.0 + rng.integers(0, 2 ** 20, sp.shape) / 2.0 ** 20)).astype(F32)
            d = _mfma(gpu, enc, a, b, c).astype(np.float64)
            exact = np.array([[math.fsum([float(c[i, j])] + p[i, :, j].tolist()) for j in range(32)] for i in range(32)])
            ratio = np.abs(d - exact) / (np.abs(c.astype(np.float64)) + np.abs(p).sum(1))
            worst = max(worst, float(ratio.max()))
    # subnormal pieces (2^-130 .. 2^-127 times values near 1) beside C = 2^-100: flushed or not, they are far inside kappa |C|
    a = (operand((32, 16), 0).astype(np.float64) * 2.0 ** rng.integers(-130, -126, (32, 16))).astype(F32)
    b = operand((16, 32), 0)
    p = a.astype(np.float64)[:, :, None] * b.astype(np.float64)[None, :, :]
    c = np.full((32, 32), 2.0 ** -100, F32)
    d = _mfma(gpu, enc, a, b, c).astype(np.float64)
    exact = c.astype(np.float64) + p.sum(1)
    ratio = np.abs(d - exact) / (np.abs(c.astype(np.float64)) + np.abs(p).sum(1))
    worst = max(worst, float(ratio.max()))
    d0 = _mfma(gpu, enc, a, b, np.zeros((32, 32), F32)).astype(np.float64)
    flushed = bool((d0 == 0).all())
    assert (np.abs(d0 - p.sum(1)) <= 16 * 2.0 ** -126).all(), "a subnormal piece is off by more than the smallest normal"
    print(f"largest |D - exact| / (|C| + sum |p|): {worst:.3e} = {worst / k['kappa']:.3f} kappa; subnormal bf16 inputs flushed: {flushed}")
    assert worst <= k["kappa"]


# ---------------------------------------------------------------------------------------------------- H and A

def _pattern_case(M):
    """M mono frames at 48 kHz: low tones, and every fifth frame's window overwritten with a sign pattern of a bound column
    (every product of that column on one side) at an amplitude from full scale down to 1e-3; the frames beside one see
    half of it."""
    T, _, _ = O.tables()
    n = (M + 3) * HOP
    x = (0.5 * S.tones(48000, 1, n, *LOW)[:, 0]).astype(F32)
    cols, amps = (384, 385, 500, 640, 1023), (1.0, -1.0, 1e-3, 0.25)
    for q, f in enumerate(range(2, M, 5)):
        lo = f * HOP - HOP // 2
        x[lo:lo + FRAME] = np.sign(T[cols[q % 5]]).astype(F32) * F32(amps[q % 4])
    return Case(f"matrix-tap-{M}", "matrix", 48000, 1, x[:, None], 1, 1 + M)


@pytest.mark.parametrize("M", [128, 129, 257])
def test_h_and_a_of_the_matrix_form_against_the_real_sums(gpu, M):
    """|H - max_k |sum xw T|| <= gamma_2048 A (1 + 1e-3) per row over the bound columns, A within the slack the bound
    gives its order, and the bound formed from them covers every oracle |c_k| it is there to cover (k >= C0; the columns
    [L, C0) are exact ones, checked by the pass rule's other condition)."""
    c = _pattern_case(M)
    enc = gpu[2](c.sr)
    exp, taps, v = expected(c)
    rec, screened, repaired = records(gpu, enc, c, 2, 2)
    assert screened == c.M and np.array_equal(rec, exp), S.explain(rec, exp, c.ch)
    h, a = np.zeros(M, F32), np.zeros(M, F32)
    pf = C.POINTER(C.c_float)
    assert gpu[1].lib.glc_debug_encode_bound_tap(enc._h, M, h.ctypes.data_as(pf), a.ctypes.data_as(pf)) == 0
    T, _, norm = O.tables()
    _, c0, _ = S.shape(c.sr)
    xw = S.windowed_rows(c).astype(np.float64)
    real = np.abs(xw @ T[c0:].astype(np.float64).T).max(1)
    A = np.abs(xw).sum(1)
    err = np.abs(h.astype(np.float64) - real)
    print(f"M {M}: largest |H - real| / A {np.max(err / np.maximum(A, 1e-300)):.3e} (gamma_2048 {GAMMA:.3e}), "
          f"largest |A - sum| / sum {np.max(np.abs(a - A) / np.maximum(A, 1e-300)):.3e}, repaired {repaired}")
    assert (err <= GAMMA * A * (1 + 1e-3)).all(), np.flatnonzero(err > GAMMA * A * (1 + 1e-3))[:8].tolist()
    assert (np.abs(a.astype(np.float64) - A) <= GAMMA * A).all()
    B = ((h + C_ERR * a) * F32(norm)) * SLACK + TINY
    assert (np.abs(taps.coeffs[:, c0:]) <= B[:, None]).all()
    lo, hi = int((v == -1).sum()), int((v != 1).sum())
    assert lo <= repaired <= hi and lo > 0 and hi < M, (repaired, lo, hi)


# ---------------------------------------------------------------------------------------------------- records

def _shape_cases():
    """Rows 128 .. 301 around the 128-row tile, mono; two tiles and a partial one at 2 / 4 / 8 channels; 3 channels, which
    the form is not built for and which therefore keeps the FMA form under the same setting."""
    out = []
    for ch, frames in ((1, 128), (1, 129), (1, 255), (1, 256), (1, 257), (1, 301), (2, 128), (2, 129), (4, 64), (4, 65), (8, 32), (8, 33), (3, 100)):
        x = S.tones(48000, ch, (frames + 8) * HOP, *LOW)
        S._click(x, 3 + frames // 2, ch_sel=ch - 1)
        S._click(x, 3 + frames - 2)
        out.append(Case(f"matrix-ch{ch}-m{frames * ch}", "matrix", 48000, ch, x, 3, 3 + frames))
    return out


RECORD_CASES = {c.name: c for c in [c for c in S.cases() if c.sr in (44100, 48000)] + _shape_cases()}


@pytest.mark.parametrize("name", list(RECORD_CASES))
def test_records_equal_the_oracle_under_both_forms_and_without_the_screen(gpu, name):
    c = RECORD_CASES[name]
    enc = gpu[2](c.sr)
    exp, taps, v = expected(c)
    built = c.ch in (1, 2, 4, 8)
    lo, hi = int((v == -1).sum()), int((v != 1).sum())
    out = {}
    for label, bound, mode in (("matrix", 2, 2), ("fma", 1, 2), ("off", 0, 1)):
        rec, screened, repaired = records(gpu, enc, c, bound, mode)
        out[label] = rec
        print(f"{name} [{label}]: M {c.M}, screened {screened}, repaired {repaired}, model {lo}..{hi}")
        assert np.array_equal(rec, exp), f"{name} [{label}]: {S.explain(rec, exp, c.ch)}"
        takes = mode == 2 and c.M >= (128 if bound == 2 and built else 256)
        assert screened == (c.M if takes else 0), f"{name} [{label}]: {screened} of {c.M} rows went through the screened path"
        if takes:
            assert lo <= repaired <= hi, f"{name} [{label}]: {repaired} rows repaired, the model has {lo}..{hi}"
        else:
            assert repaired == 0
    assert np.array_equal(out["matrix"], out["fma"]) and np.array_equal(out["matrix"], out["off"])


def test_value_rows_fail_or_pass_as_the_model_says(gpu):
    """NaN, Inf, 3e38 (whose bf16 rounding overflows: the totals are not finite and H is written as infinity) and 1e-40
    (pieces the matrix pipe may flush: under kScreenTiny) under the matrix form."""
    c = RECORD_CASES["values"]
    enc = gpu[2](c.sr)
    exp, taps, v = expected(c)
    assert (v != 0).all()
    rec, screened, repaired = records(gpu, enc, c, 2, 2)
    assert np.array_equal(rec, exp) and screened == c.M
    assert repaired == int((v == -1).sum()), "exactly the model's rows: 3e38, the NaN and Inf frames, energy above C0 only"
    h, a = np.zeros(c.M, F32), np.zeros(c.M, F32)
    pf = C.POINTER(C.c_float)
    assert gpu[1].lib.glc_debug_encode_bound_tap(enc._h, c.M, h.ctypes.data_as(pf), a.ctypes.data_as(pf)) == 0
    f0 = c.f0
    assert (h[81 - f0:119 - f0] > 1e36).all(), "3e38 rows: sums that overflow leave a huge or infinite H, never a NaN"
    assert (h[42 - f0:78 - f0] <= 2048 * 1e-40).all() and (a[42 - f0:78 - f0] > 0).all()
    assert not np.isfinite(a[150 - f0]) and not np.isfinite(a[170 - f0])
    # one sample of 3.4e38 at the centre of frame 60's window: finite, but its bf16 rounding is infinite and a - a1 is
    # not a number any more - the row's H must come out infinite (fmaxf in the quantiser would drop a NaN)
    x = S.tones(48000, 1, 140 * HOP, *LOW)
    x[61 * HOP - HOP // 2, 0] = 3.4e38
    c = Case("matrix-overflow", "matrix", 48000, 1, x, 2, 130)
    exp, taps, v = expected(c)
    rec, screened, repaired = records(gpu, enc, c, 2, 2)
    assert np.array_equal(rec, exp) and screened == c.M and int((v == -1).sum()) <= repaired <= int((v != 1).sum())
    h, a = np.zeros(c.M, F32), np.zeros(c.M, F32)
    assert gpu[1].lib.glc_debug_encode_bound_tap(enc._h, c.M, h.ctypes.data_as(pf), a.ctypes.data_as(pf)) == 0
    assert np.isinf(h[60 - c.f0]) and np.isfinite(a[60 - c.f0]) and v[60 - c.f0] == -1
    assert np.isfinite(h[[50 - c.f0, 70 - c.f0]]).all()


# ---------------------------------------------------------------------------------------------------- context rules

def test_the_setter_survives_the_screen_setter_and_rejects_unknown_kinds(gpu):
    torch, glc_amd, _ = gpu
    lib = glc_amd.lib
    c = RECORD_CASES["matrix-ch1-m128"]            # 128 rows: screened only while the matrix form is forced
    exp = expected(c)[0]
    enc = glc_amd.Encoder(c.sr)
    try:
        assert lib.glc_debug_set_encode_bound(enc._h, 3) != 0 and lib.glc_debug_set_encode_bound(enc._h, -1) != 0
        assert lib.glc_debug_set_encode_bound(enc._h, 2) == 0
        for mode in (2, 0, 2):                      # S.records sets the mode, launches, and sets mode 0 again
            rec, screened, _ = S.records(torch, glc_amd, enc, c, mode)
            assert np.array_equal(rec, exp) and screened == (c.M if mode == 2 else 0), mode
        assert lib.glc_debug_set_encode_bound(enc._h, 1) == 0
        rec, screened, _ = S.records(torch, glc_amd, enc, c, 2)
        assert np.array_equal(rec, exp) and screened == 0
    finally:
        enc.close()


def test_a_fresh_context_and_a_long_lived_one_give_the_same_bytes(gpu):
    torch, glc_amd, encoder = gpu
    old = encoder(48000)                            # has run every case above it
    for name in ("mixed-partial-tile", "matrix-ch2-m258", "matrix-ch8-m264"):
        c = RECORD_CASES[name]
        fresh = glc_amd.Encoder(c.sr)
        try:
            a = records(gpu, fresh, c, 2, 2)
            b = records(gpu, old, c, 2, 2)
        finally:
            fresh.close()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], expected(c)[0]) and a[1:] == b[1:], name
