"""Cases for tests/test_encode_edge.py: streams and frame ranges that put the stream's edge frames - the frames whose
2048-sample window reaches into the zero padding, csrc/glc_kernels.h edge_frames - at every place of a screened launch
the edge path treats differently, and a Python restatement of which frames and rows those are.

The restatement is not the code under test: edge_frames() below is the closed form the library uses, brute_edge() the
window test it stands for, and tests/test_encode_edge.py holds one to the other."""
import numpy as np

import encode_screen_cases as S
from encode_screen_cases import HOP, FRAME, Case, _click, tones, lcg_noise

F32 = np.float32
EDGE_ROWS_MAX = 32  # csrc/glc_kernels.h kEdgeRowsMax
LOW = ([220.0, 1234.5, 3100.0, 6900.0], [0.3, 0.2, 0.1, 0.05])


def plan(n_samples, ch):
    """(per_channel, n_frames) of include/glc.h glc_plan_encode, restated (src/codec.rs:433-455)."""
    per = -(-n_samples // ch)
    padded = (HOP // 2 + per + HOP - 1) // HOP * HOP + HOP // 2
    return per, (1 if padded < FRAME else (padded - FRAME) // HOP + 1)


def edge_frames(per, n_frames):
    """(a, b): the edge frames are [0, a) and [b, n_frames)."""
    tail = FRAME - HOP // 2
    a = min(1, n_frames)
    b = (per - tail) // HOP + 1 if per >= tail else 0
    b = min(b, n_frames)
    return a, max(a, b)


def brute_edge(per, n_frames):
    """The frames whose window [hop f - hop/2, hop f - hop/2 + frame) is not wholly inside [0, per)."""
    return [f for f in range(n_frames) if f * HOP - HOP // 2 < 0 or f * HOP - HOP // 2 + FRAME > per]


def edge_rows(case):
    """The rows of the case's launch (row = (frame - f0) * ch + c) that belong to edge frames."""
    per, nf = plan(case.n_samples, case.ch)
    a, b = edge_frames(per, nf)
    return [(f - case.f0) * case.ch + c for f in range(case.f0, case.f1) if f < a or f >= b for c in range(case.ch)]


def _stream(ch, frames, cut=0):
    x = tones(48000, ch, frames * HOP, *LOW)
    return x[:frames * HOP - cut] if cut else x


def cases():
    """name -> Case, 48 kHz.  `family` names what the case is for; c.bounds the forms of K1 it reaches the screen with
    (the forced screen takes launches from 128 rows with the matrix form, from 256 with the FMA form)."""
    out = []

    def add(name, ch, x, f0, f1, bounds=(1, 2)):
        c = Case(name, "edge", 48000, ch, x, f0, f1)
        c.bounds = bounds
        assert c.M >= (256 if 1 in bounds else 128)
        out.append(c)

    # mono, 140 rows at the most: one 128-row matrix tile and a ragged one.  Both edges, one, the other, none.
    x = _stream(1, 140)
    add("mono-whole", 1, x, 0, 140, (2,))
    add("mono-head", 1, x, 0, 135, (2,))
    add("mono-tail", 1, x, 5, 140, (2,))
    add("mono-middle", 1, x, 3, 137, (2,))
    # ... and with the FMA form, which starts at 256 rows
    add("mono-whole-262", 1, _stream(1, 262), 0, 262)
    # stereo, M = 550: the end's edge rows sit in a partial last quantiser wave (550 = 34 * 16 + 6)
    add("stereo-whole", 2, _stream(2, 275), 0, 275)
    # lengths that end inside a hop.  Whatever the length, the plan has exactly one trailing edge frame - or none: with
    # per_channel = 1024 q + r the last frame ends at 1024 q + 512 (r <= 512) or 1024 q + 1536 (r > 512), the one before
    # it 1024 earlier, inside the stream - so "two trailing edge frames" cannot be built (test_encode_edge.py asserts it
    # for every length it tries).  r = 300: the last frame holds 812 samples; r = 512: the last frame's window ends
    # where the stream does, and the stream has NO trailing edge frame; r = 513: the last frame holds one hop less.
    for r, ch, bounds in ((300, 1, (2,)), (512, 1, (2,)), (513, 2, (1, 2))):
        x = _stream(ch, 141)[:139 * HOP + r]
        nf = plan(x.size, ch)[1]
        add(f"ch{ch}-ends-at-r{r}", ch, x, 2 if ch == 2 else 0, nf, bounds)
    # a click in frame 1: rows 2-3 of the first quantiser wave are the serial repair's, rows 0-1 the side stream's
    x = _stream(2, 140)
    _click(x, 1)
    add("stereo-click-frame-1", 2, x, 0, 140)
    # 4 channels: the edge frame is a whole quantiser wave, the fused decision takes all four rows from the side path
    add("ch4-whole", 4, _stream(4, 66), 0, 66)
    # 3 and 8 channels: flags per row, K3 behind the join
    add("ch3-whole", 3, _stream(3, 88), 0, 88)
    add("ch8-whole", 8, _stream(8, 34), 0, 34)
    # silence over frame 0's window: the edge frame passes its screen
    x = _stream(2, 140)
    x[:FRAME - HOP // 2] = 0.0
    add("stereo-silent-head", 2, x, 0, 140)
    # a NaN inside frame 0, an infinity inside the last frame
    x = _stream(1, 262).astype(F32)
    x[100, 0] = np.nan
    x[261 * HOP + 40, 0] = np.inf
    add("mono-nan-inf", 1, x, 0, 262)
    # full-scale noise in the edge frames: they go raw through the side path
    x = _stream(2, 140)
    x[:FRAME - HOP // 2] = lcg_noise(FRAME - HOP // 2, 2)
    x[138 * HOP:] = lcg_noise(2 * HOP, 2, seed=7)
    add("stereo-noise-edges", 2, x, 0, 140)
    return out


def two_chunk_case():
    """Stereo, 4096 + 300 frames: the range is two chunks of the encoder, the start edge in chunk 0 on the caller's
    stream, the end edge in chunk 1 on the second one."""
    c = Case("stereo-two-chunks", "edge", 48000, 2, _stream(2, 4396), 0, 4396)
    c.bounds = (1, 2)
    return c


def bind(glc_amd):
    S.bind(glc_amd)
