"""Inputs of tests/test_roundtrip.py: the clips of the oracle comparison, and frame records built by hand
in the layout of glc_record_bytes (include/glc.h) for the edges of the records -> row-tables kernel."""
import numpy as np

import conftest as cf

HOP, FRAME = 1024, 2048
F32 = np.float32


def frames_of(per_channel):
    return -(-(512 + per_channel) // HOP) - 1       # src/codec.rs:433-455


def lcg_noise(n, seed=12345, amp=0.5):
    """Uniform noise from a 32-bit LCG (Numerical Recipes constants): no structure a tonal model could keep."""
    out = np.empty(n, np.float64)
    s = seed & 0xFFFFFFFF
    for i in range(n):
        s = (1664525 * s + 1013904223) & 0xFFFFFFFF
        out[i] = s / 2147483648.0 - 1.0
    return (amp * out).astype(F32)


def chord(sr, ch, per_channel, seed=7):
    return cf.gen_chord(sr, ch, per_channel, seed=seed)


def mixed_clip(sr, ch):
    """chord, then LCG noise, then chord: compressed and raw frames next to each other."""
    a = chord(sr, ch, 6 * HOP, seed=3)
    n = lcg_noise(6 * HOP * ch)
    b = chord(sr, ch, 5 * HOP + 300, seed=4)
    return np.concatenate([a, n, b])


# (name, sample rate, channels, samples, what the oracle's stream must show: "tonal" = no raw frame,
#  "noise" = at least one raw frame, "mixed" = both kinds and a raw frame next to a compressed one, None = either)
def oracle_cases():
    c = []
    c.append(("sine-44k-stereo", 44100, 2, cf.gen_tone("sine", 440.0, 44100, 2, 0.2), "tonal"))
    c.append(("sweep-48k-mono", 48000, 1, cf.gen_tone("sweep", 200.0, 48000, 1, 0.2, 4000.0), None))
    for d in (-1, 0, 1):      # one short of a hop, exactly on it, one past it
        c.append((f"chord-48k-mono-hop{d:+d}", 48000, 1, chord(48000, 1, 6 * HOP + d), "tonal"))
        c.append((f"chord-44k-stereo-hop{d:+d}", 44100, 2, chord(44100, 2, 5 * HOP + d), "tonal"))
        # ... and around the length at which the padding arithmetic adds a frame (src/codec.rs:433-455)
        c.append((f"chord-96k-mono-frame-edge{d:+d}", 96000, 1, chord(96000, 1, 4 * HOP + 512 + d), "tonal"))
    c.append(("chord-96k-6ch", 96000, 6, chord(96000, 6, 4 * HOP + 300), "tonal"))
    c.append(("chord-44k-6ch-hop", 44100, 6, chord(44100, 6, 3 * HOP), "tonal"))
    c.append(("noise-48k-stereo", 48000, 2, cf.gen_noise(48000, 2, 0.15, 11), "noise"))
    c.append(("noise-96k-mono", 96000, 1, cf.gen_noise(96000, 1, 0.08, 5), "noise"))
    c.append(("shortest-44k-mono", 44100, 1, chord(44100, 1, 513), None))
    c.append(("shortest-96k-6ch", 96000, 6, chord(96000, 6, 513), None))
    c.append(("mixed-48k-stereo", 48000, 2, mixed_clip(48000, 2), "mixed"))
    c.append(("mixed-44k-mono", 44100, 1, mixed_clip(44100, 1), "mixed"))
    return c


# ------------------------------------------------------------------------------------------ records by hand

def record_layout(ch):
    hdr = ((8 + 8 * ch) + 15) // 16 * 16
    return hdr, hdr + 2 * FRAME * ch


def build_records(ch, frames):
    """frames: per frame either ("raw", planes int16 [ch][2048]) or ("c", [(scale, dense_q int16 [1024], nnz or
    None = count the row) per channel]) -> (records uint8, per-channel samples of a stream of that many frames)."""
    hdr, rec = record_layout(ch)
    buf = np.zeros((len(frames), rec), np.uint8)
    for f, (kind, body) in enumerate(frames):
        r = buf[f]
        if kind == "raw":
            r[0:4] = np.frombuffer(np.uint32(1).tobytes(), np.uint8)
            r[hdr:] = np.ascontiguousarray(body, np.int16).reshape(-1).view(np.uint8)
            continue
        assert len(body) == ch
        for c, (scale, q, nnz) in enumerate(body):
            q = np.ascontiguousarray(q, np.int16)
            assert q.shape == (HOP,)
            n = int(np.count_nonzero(q)) if nnz is None else nnz
            r[8 + 8 * c:12 + 8 * c] = np.frombuffer(np.float32(scale).tobytes(), np.uint8)
            r[12 + 8 * c:16 + 8 * c] = np.frombuffer(np.uint32(n).tobytes(), np.uint8)
            r[hdr + c * 4096: hdr + c * 4096 + 2048] = q.view(np.uint8)
    assert frames_of(len(frames) * HOP) == len(frames)
    return buf.reshape(-1), len(frames) * HOP


def dense_row(rng, nnz, positions=None, values=None):
    """A dense quantised row with `nnz` non-zero entries (random places and values unless given)."""
    q = np.zeros(HOP, np.int16)
    k = np.sort(rng.choice(HOP, nnz, replace=False)) if positions is None else np.asarray(positions)
    v = values
    if v is None:
        v = rng.randint(-3000, 3000, k.size)
        v[v == 0] = 7
    q[k] = np.asarray(v, np.int16)
    assert np.count_nonzero(q) == k.size
    return q


def edge_rows(seed=1):
    """(name, scale, dense row, nnz field or None) for every structural edge of a compressed row."""
    rng = np.random.RandomState(seed)
    rows = []
    for n in (0, 1, 63, 64, 65, 1023, 1024):        # around the wave width, and a full row
        rows.append((f"nnz{n}", 0.01 + 0.001 * (n % 7), dense_row(rng, n), None))
    rows.append(("only-k0", 0.02, dense_row(rng, 1, [0], [1234]), None))
    rows.append(("only-k1023", 0.02, dense_row(rng, 1, [1023], [-4321]), None))
    rows.append(("k0-and-k1023", 0.02, dense_row(rng, 2, [0, 1023], [5, -5]), None))
    rows.append(("alternating-even", 0.005, dense_row(rng, 512, np.arange(0, HOP, 2)), None))
    rows.append(("alternating-odd", 0.005, dense_row(rng, 512, np.arange(1, HOP, 2)), None))
    rows.append(("lane-edges", 0.01, dense_row(rng, 128, np.sort(np.r_[np.arange(0, HOP, 16), np.arange(15, HOP, 16)])), None))
    rows.append(("q-extremes", 0.03, dense_row(rng, 4, [3, 500, 501, 1020], [-32768, 32767, -32768, 32767]), None))
    rows.append(("full-extremes", 0.001, dense_row(rng, HOP, np.arange(HOP), np.where(np.arange(HOP) % 2, -32768, 32767)), None))
    rows.append(("scale-zero", 0.0, dense_row(rng, 40), None))                 # scale.max(1e-12), src/codec.rs:653
    rows.append(("scale-denormal", np.float32(1e-40), dense_row(rng, 40), None))
    rows.append(("scale-below-floor", np.float32(1e-13), dense_row(rng, 40), None))
    rows.append(("scale-negative", -0.5, dense_row(rng, 40), None))
    rows.append(("nnz-field-short", 0.01, dense_row(rng, 100), 37))           # the first 37 non-zeros count
    return rows


def raw_planes(rng, ch):
    p = rng.randint(-32768, 32768, (ch, FRAME)).astype(np.int16)
    p[0, 0], p[-1, -1] = -32768, 32767
    return p


def edge_stream(ch, seed=2):
    """Every edge row in every channel position of a stream of `ch` channels (+ a raw frame in the middle)."""
    rng = np.random.RandomState(seed)
    rows = edge_rows(seed)
    frames = []
    for i in range(len(rows)):
        frames.append(("c", [rows[(i + c * 5) % len(rows)][1:] for c in range(ch)]))
        if i == len(rows) // 2:
            frames.append(("raw", raw_planes(rng, ch)))
    return frames


def raw_placement(ch, n_frames, where, seed=3):
    rng = np.random.RandomState(seed)
    is_raw = {"first": lambda f: f == 0, "last": lambda f: f == n_frames - 1, "every-other": lambda f: f % 2 == 1,
              "all": lambda f: True, "none": lambda f: False}[where]
    frames = []
    for f in range(n_frames):
        if is_raw(f):
            frames.append(("raw", raw_planes(rng, ch)))
        else:
            frames.append(("c", [(0.01 * (c + 1), dense_row(rng, 30 + 11 * c + f), None) for c in range(ch)]))
    return frames
