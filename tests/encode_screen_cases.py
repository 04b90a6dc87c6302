"""Cases for tests/test_encode_screen.py: streams that drive the screened encode path to every
outcome - all rows pass, all rows fail, one frame / one channel / one row of the partial tile fails, a last-band
line that crosses the noise floor below and above C0, the value edges, the layouts - and a CPU model of the screen
that says, from the oracle's coefficients, which rows MUST pass, which MUST fail and which are too close to call.

The model is not the code under test: the exact columns of the device are the oracle's bit for bit, so condition (a)
is evaluated on the oracle's coefficients; the bound waves' fused sums e_k are only known to lie within
2 gamma_2048 A of the oracle's unnormalised sums, which brackets B from both sides."""
import ctypes as C

import numpy as np

from oracle import oracle as O

HOP, FRAME = 1024, 2048
F32 = np.float32
U = 2.0 ** -24
GAMMA = 2048 * U / (1 - 2048 * U)
# the kernel's constants (glc_kernels.hip kScreenCErr / kScreenSlack / kScreenTiny), restated
C_ERR, SLACK, TINY = F32(2.45e-4), F32(1.001), F32(1e-33)
NOISE_FLOOR = F32(10.0) ** F32(-48.0 / 20.0)


def shape(sr):
    """(L, C0, ne) of a rate: start of the last band, rounded up to 64, exact waves."""
    _, e = O.perceptual(sr)
    L = int(e[-2])
    c0 = (L + 63) // 64 * 64
    return L, c0, c0 // 64


class Case:
    def __init__(self, name, family, sr, ch, pcm, f0, f1, halo=0, expect=None):
        self.name, self.family, self.sr, self.ch = name, family, sr, ch
        self.pcm = np.ascontiguousarray(pcm, F32).reshape(-1)
        self.n_samples = self.pcm.size
        self.f0, self.f1, self.halo = f0, f1, halo
        self.expect = expect          # "pass": no row repaired, "fail": every row repaired, None: the model decides
        self.M = (f1 - f0) * ch

    def shard(self):
        """-> (shard, t0, t_count): the per-channel samples frames [f0, f1) read, `halo` more in front."""
        per = -(-self.n_samples // self.ch)
        lo = max(0, self.f0 * HOP - HOP // 2 - self.halo)
        hi = min(per, (self.f1 - 1) * HOP + FRAME - HOP // 2)
        return self.pcm[lo * self.ch:hi * self.ch], lo, hi - lo


def tones(sr, ch, n, freqs, amps, phase=0.3):
    t = np.arange(n, dtype=np.float64) / sr
    x = np.zeros((n, ch))
    for c in range(ch):
        for j, (f, a) in enumerate(zip(freqs, amps)):
            x[:, c] += a * np.sin(2 * np.pi * f * (1 + 0.013 * c) * t + phase * (j + 1) + c)
    return x


def lcg_noise(n, ch, seed=12345, amp=0.9):
    out = np.empty(n * ch)
    s = seed
    for i in range(n * ch):
        s = (1103515245 * s + 12345) & 0x7FFFFFFF
        out[i] = (s / 2 ** 30 - 1.0) * amp
    return out.reshape(n, ch)


def _click(x, frame, ch_sel=None, amp=2.0):
    """A click at the first sample of `frame + 1`'s window: the centre of `frame`'s, weight ~4e-4 in the neighbour's."""
    t = (frame + 1) * HOP - HOP // 2
    if ch_sel is None:
        x[t, :] += amp
    else:
        x[t, ch_sel] += amp


def cases():
    out = []
    low = ([220.0, 1234.5, 3100.0, 6900.0], [0.3, 0.2, 0.1, 0.05])

    def stream(sr, ch, frames):
        return tones(sr, ch, frames * HOP, *low)

    # all rows pass: interior frames of tones below 7 kHz (frame 0 and the last frames see the zero padding)
    out.append(Case("pass-ch2", "pass", 48000, 2, stream(48000, 2, 140), 4, 132, expect="pass"))
    # all rows fail: noise, loud enough for raw frames and quiet enough for compressed ones
    out.append(Case("fail-noise-raw", "fail", 48000, 2, lcg_noise(130 * HOP, 2), 1, 129, expect="fail"))
    out.append(Case("fail-noise", "fail", 48000, 2, lcg_noise(130 * HOP, 2, seed=99, amp=0.05) +
                    tones(48000, 2, 130 * HOP, [440.0], [0.5]), 1, 129, expect="fail"))
    # mixed
    x = stream(48000, 2, 140)
    _click(x, 70)
    out.append(Case("mixed-one-frame", "mixed", 48000, 2, x, 4, 132))
    x = stream(48000, 2, 140)
    _click(x, 70, ch_sel=1)
    out.append(Case("mixed-one-channel", "mixed", 48000, 2, x, 4, 132))
    x = stream(48000, 2, 160)
    _click(x, 4 + 140)                      # rows 280, 281 of 300: the second, partial tile
    out.append(Case("mixed-partial-tile", "mixed", 48000, 2, x, 4, 154))
    # crossings: a line at bin 362.5 (inside [L, C0)) / 400.5 (just above C0 = 384) ramped from -66 to -30 dB under a
    # full-scale 1 kHz tone: |c| / nfl crosses 1 once, slowly (0.14 dB per frame)
    for name, k in (("cross-below-c0", 362.5), ("cross-above-c0", 400.5)):
        n = 262 * HOP
        t = np.arange(n, dtype=np.float64) / 48000
        ramp = 10.0 ** ((-66.0 + 36.0 * np.arange(n) / n) / 20.0)
        x = 0.5 * np.sin(2 * np.pi * 1000.0 * t) + 0.5 * ramp * np.sin(2 * np.pi * k * 48000 / 2048 * t)
        out.append(Case(name, "cross", 48000, 1, x[:, None], 3, 259))
    # value edges, mono, 40 frames each: zeros, 1e-40, 3e38, a NaN and an Inf in one row each, energy only in S
    n = 262 * HOP
    x = np.zeros((n, 1), F32)
    x[40 * HOP:80 * HOP, 0] = 1e-40
    x[80 * HOP:120 * HOP:2, 0] = 3e38
    x[80 * HOP + 1:120 * HOP:2, 0] = -3e38
    x[120 * HOP:200 * HOP, 0] = tones(48000, 1, 80 * HOP, *low)[:, 0].astype(F32)
    x[150 * HOP + 17, 0] = np.nan
    x[170 * HOP + 900, 0] = np.inf
    x[200 * HOP:, 0] = tones(48000, 1, 62 * HOP, [15000.0], [0.4])[:, 0].astype(F32)
    out.append(Case("values", "values", 48000, 1, x, 2, 258))
    # layouts
    x = stream(48000, 2, 150)
    _click(x, 100)
    out.append(Case("layout-halo", "layout", 48000, 2, x, 7, 135, halo=333))
    x = stream(48000, 1, 300)[:299 * HOP - 77]             # ragged end: the last frames read the trailing padding
    out.append(Case("layout-ragged-end", "layout", 48000, 1, x, 299 - 257, 299))
    x = stream(48000, 1, 310)
    _click(x, 200)
    out.append(Case("layout-m-301", "layout", 48000, 1, x, 2, 303))
    x = stream(48000, 3, 110)
    _click(x, 50, ch_sel=2)
    out.append(Case("layout-ch3", "layout", 48000, 3, x, 3, 103))      # 300 rows: K3 and the per-row loader
    for sr in (44100, 96000, 192000):
        x = stream(sr, 2, 140)
        _click(x, 70)
        out.append(Case(f"layout-sr{sr}", "layout", sr, 2, x, 4, 132))
    return out


def guard_case():
    """4098 rows of noise (the 130-frame LCG stream, repeated): 17 row tiles, the fewest the automatic mode screens (the
    16-wave transform takes a launch whose last round of 32 tiles is more than half full), and every row fails -
    what the guard exists for."""
    x = np.tile(lcg_noise(130 * HOP, 2), (16, 1))
    return Case("guard-noise", "guard", 48000, 2, x, 1, 2050, expect="fail")


class FlagshipRank(Case):
    """Rank `rank` of `world` of the benchmark's workload (bench.py make_shard_pcm): 4096 stereo frames of the chord,
    a frame range of a stream of 4096 * world frames.  Only the shard's samples are ever generated."""

    def __init__(self, bench, rank, world):
        self._bench = bench
        n = bench.FRAMES_PER_GPU
        self.name = self.family = f"flagship-{rank}-of-{world}"
        self.sr, self.ch, self.halo, self.expect = bench.SR, bench.CH, 0, None
        self.n_samples = n * world * HOP * bench.CH
        self.f0, self.f1 = n * rank, n * (rank + 1)
        self.M = n * bench.CH

    def shard(self):
        per = self.n_samples // self.ch
        lo = max(0, self.f0 * HOP - HOP // 2)
        hi = min(per, (self.f1 - 1) * HOP + FRAME - HOP // 2)
        return self._bench.chord(np, lo, hi - lo), lo, hi - lo


def expected(case):
    """-> (record bytes, oracle taps) of the case's frames."""
    sh, t0, tc = case.shard()
    return O.encode_range_records(sh, t0, tc, case.n_samples, case.sr, case.ch, case.f0, case.f1, taps=True)


def windowed_rows(case):
    """fl(x w) of every row of the case, [M, 2048] f32 (from the shard the case hands the encoder)."""
    _, w, _ = O.tables()
    per = -(-case.n_samples // case.ch)
    sh, t0, tc = case.shard()
    x = np.zeros((tc * case.ch,), F32)
    x[:sh.size] = sh
    x = x.reshape(tc, case.ch)
    rows = np.zeros((case.M, FRAME), F32)
    for f in range(case.f0, case.f1):
        lo = f * HOP - HOP // 2
        a, b = max(lo, t0), min(lo + FRAME, per, t0 + tc)
        if b > a:
            rows[(f - case.f0) * case.ch:(f - case.f0 + 1) * case.ch, a - lo:b - lo] = x[a - t0:b - t0].T
    with np.errstate(all="ignore"):
        return rows * w[None, :]


def model(case, taps):
    """Per row: +1 must pass, -1 must fail, 0 too close to call (or order-dependent).  Frame-level for 1 / 2 / 4 channels
    (one failing channel fails its frame), as the fused quantiser decides."""
    L, c0, _ = shape(case.sr)
    _, _, norm = O.tables()
    with np.errstate(all="ignore"):
        a = np.abs(taps.coeffs.astype(np.float64))
        xw = windowed_rows(case).astype(np.float64)
        A = np.abs(xw).sum(1)
        scale = np.maximum(np.fmax.reduce(a[:, :c0], axis=1, initial=0.0), 1e-10)
        nfl = float(NOISE_FLOOR) * scale
        cond_a = (a[:, L:c0] > nfl[:, None] * (1 + 1e-5)).any(1)
        cond_a_maybe = (a[:, L:c0] > nfl[:, None] * (1 - 1e-5)).any(1)
        hs = np.fmax.reduce(a[:, c0:], axis=1, initial=0.0) / float(norm)
        e_hi, e_lo = hs + 2.0 * GAMMA * A * 1.001, np.maximum(hs - 2.0 * GAMMA * A * 1.001, 0.0)
        b_hi = (e_hi + float(C_ERR) * A) * float(norm) * float(SLACK) * (1 + 1e-4) + float(TINY)
        b_lo = (e_lo + float(C_ERR) * A) * float(norm) * float(SLACK) * (1 - 1e-4)
        finite = np.isfinite(A) & np.isfinite(taps.coeffs).all(1)
        must_fail = cond_a | ~finite | (b_lo > nfl)
        must_pass = ~cond_a_maybe & finite & (b_hi <= nfl)
    v = np.where(must_fail, -1, np.where(must_pass, 1, 0))
    if case.ch in (1, 2, 4):
        fr = v.reshape(-1, case.ch)
        frame = np.where((fr == -1).any(1), -1, np.where((fr == 1).all(1), 1, 0))
        v = np.repeat(frame, case.ch)
    return v


def fma_sums(xw, T, cols):
    """e_k = the running f32 sum of fused multiply-adds xw_i T_ki, i ascending, for k in cols -> [rows, len(cols)] f32.
    (The f64 product of two f32 is exact; the one f64 rounding in front of the f32 one moves a tie by 2^-29 ulp.)"""
    acc = np.zeros((xw.shape[0], len(cols)), F32)
    Tt = np.ascontiguousarray(T[cols].T).astype(np.float64)
    x64 = xw.astype(np.float64)
    with np.errstate(all="ignore"):
        for i in range(FRAME):
            acc = (acc.astype(np.float64) + x64[:, i:i + 1] * Tt[i][None, :]).astype(F32)
    return acc


def bound_per_bin(e, A):
    """The kernel's B with |e_k| in place of the row maximum, in f32 as the kernel computes it."""
    with np.errstate(all="ignore"):
        _, _, norm = O.tables()
        return ((np.abs(e) + (C_ERR * A)[:, None]) * F32(norm)) * SLACK + TINY


def assert_bound(xw, what):
    """|c| of the oracle never exceeds the kernel's bound formed from the emulated fused sums, for the rows `xw` over
    the columns 128..1023 (S at 192 kHz: the widest) -> the largest |c| / B seen."""
    T, _, norm = O.tables()
    cols = np.arange(128, 1024)
    e = fma_sums(xw, T, cols)
    with np.errstate(all="ignore"):
        A = np.cumsum(np.abs(xw), axis=1, dtype=F32)[:, -1]       # ascending f32 sum, as the wave forms it
        B = bound_per_bin(e, A)
        c = np.stack([np.abs(O.mdct_block(r))[cols] for r in xw])
        ok = (c <= B) | ~np.isfinite(B)                # a non-finite bound fails the row: nothing is claimed
    assert ok.all(), f"{what}: |c| exceeds the bound at (row, k) {np.argwhere(~ok)[:4].tolist()}"
    with np.errstate(all="ignore"):
        return float(np.nanmax(np.where(np.isfinite(B) & (B > 0), c / B, 0.0)))


# ---------------------------------------------------------------------------------------------------- GPU helpers

def bind(glc_amd):
    """The two debug hooks of include/glc_debug.h the screen's suites drive."""
    f = glc_amd.lib.glc_debug_set_encode_screen
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int]
    g = glc_amd.lib.glc_debug_encode_screen_stats
    g.restype, g.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]


def stats(glc_amd, ctx):
    """(rows screened, rows repaired) of a context so far."""
    a, b = C.c_uint64(), C.c_uint64()
    assert glc_amd.lib.glc_debug_encode_screen_stats(ctx._h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def records(torch, glc_amd, enc, c, mode, nan_pad=0):
    """One glc_encode_range_device of the case with the screen in `mode` (None: as the context stands, which is the
    automatic mode) -> (record bytes, rows screened, rows repaired).  nan_pad: that many NaN words in front of and
    behind the shard on the device."""
    sh, t0, tc = c.shard()
    host = np.full(sh.size + 2 * nan_pad, 0x7FC00000, np.uint32)
    host[nan_pad:nan_pad + sh.size] = sh.view(np.uint32)          # as words: NaN payloads travel untouched
    d_pcm = torch.from_numpy(host.view(np.int32)).cuda()
    rb = glc_amd.lib.glc_record_bytes(c.ch) * (c.f1 - c.f0)
    d_rec = torch.full((rb + 8192,), 0xA5, dtype=torch.uint8, device="cuda")
    d_rec[4096:4096 + rb] = 0     # zeroed, as the oracle's are: header padding and the upper half of a compressed row are nobody's
    torch.cuda.synchronize()
    s0 = stats(glc_amd, enc)
    if mode is not None:      # (setting a mode, the automatic one too, clears the guard's state: None leaves it alone)
        assert glc_amd.lib.glc_debug_set_encode_screen(enc._h, mode) == 0
    try:
        enc.encode_range_device(d_pcm.data_ptr() + 4 * nan_pad, t0, tc, c.n_samples, c.ch, c.f0, c.f1, d_rec.data_ptr() + 4096)
        enc.synchronize()
    finally:
        if mode is not None:
            assert glc_amd.lib.glc_debug_set_encode_screen(enc._h, 0) == 0
    s1 = stats(glc_amd, enc)
    r = d_rec.cpu().numpy()
    assert (r[:4096] == 0xA5).all() and (r[4096 + rb:] == 0xA5).all(), f"{c.name}: bytes around the records were written"
    return r[4096:4096 + rb], s1[0] - s0[0], s1[1] - s0[1]


def explain(got, exp, ch):
    bad = np.flatnonzero(got != exp)
    rec = O.record_bytes(ch)
    return f"{bad.size} record bytes differ in frames {np.unique(bad // rec)[:8].tolist()}, first at byte {bad[0] % rec} of its record"
