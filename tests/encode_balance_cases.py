"""Cases for tests/test_encode_balance.py: the balanced wave layout of the mixed-role transform (DESIGN.md section 4;
csrc/glc_mdct_fwd.hpp mix_wave), restated here, and streams whose rows put a line on chosen columns of it.

wave_map() is the restatement: which columns and which hf plane a wave of workgroup n_tile owns.  aims() picks from it the
columns a mis-dealt run would lose - the ends of an exact wave's run, of a hybrid wave's exact and bound runs, of the
neighbouring bound wave's run, of the first and last bound run, in workgroups 0 and 7 - and aimed_case() builds a stream
that holds one of them per (stretch of frames, channel): a loud line below C0 (the records hold it: a coefficient stored
in the wrong place or not at all changes their bytes) or, from C0 on, the CONFINED construction of
encode_screen_edges.py (energy over the noise floor in ONE bin, so in one run; such a row must be repaired, and its
record holds the line, so an unrepaired one changes bytes as well)."""
import numpy as np

import encode_screen_edges as E
from encode_screen_cases import F32, HOP, NOISE_FLOOR, shape

BALANCED_MAX = 11      # largest ne with a balanced layout (above it a SIMD has no wave left that is only bound)


def hybrid_pairs(ne):
    """Exact column pairs of a hybrid wave in the balanced layout of `ne`: ne % 4 (0: whole waves balance already, or
    ne > 11 and no balanced layout exists)."""
    return ne % 4 if ne <= BALANCED_MAX else 0


def shipped_pairs(ne):
    """... and what a launch takes: the balanced layout where it measured faster than whole waves - 2 pairs (44.1, 48
    and 192 kHz) - and whole waves elsewhere (3 pairs, 96 kHz: measured no faster; 1 pair: no rate has it)."""
    return 2 if hybrid_pairs(ne) == 2 else 0


def first_bound(ne, hp):
    return ne // 4 * 4 if hp else ne


def planes(ne, hp):
    return 8 * (16 - first_bound(ne, hp))


def a_wave(ne, hp):
    return ne // 4 * 4 + 4 if hp else ne


def wave_map(ne, hp, n_tile, wave):
    """-> (kind, plane, exact runs, bound runs): kind 'exact' / 'hybrid' / 'bound', runs as (first column, columns)."""
    xb, bb = 8 * ne * n_tile, 64 * ne + 8 * (16 - ne) * n_tile
    fb = first_bound(ne, hp)
    plane = (16 - fb) * n_tile + wave - fb
    if hp == 0:
        if wave < ne:
            return "exact", None, [(xb + 8 * wave, 8)], []
        return "bound", plane, [], [(bb + 8 * (wave - ne), 8)]
    q, k, sd = ne // 4, wave // 4, wave % 4
    if k < q:
        return "exact", None, [(xb + 8 * wave, 8)], []
    if k > q:
        return "bound", plane, [], [(bb + 4 * (8 - 2 * hp) + 8 * (wave - 4 * q - 4), 8)]
    return "hybrid", plane, [(xb + 32 * q + 2 * hp * sd, 2 * hp)], [(bb + (8 - 2 * hp) * sd, 8 - 2 * hp)]


def aims(ne, hp):
    """-> [(column, 'exact' | 'bound', the run (first, columns) that holds it, what it is)] of a rate."""
    out = []
    q = ne // 4

    def ends(run, side, what):
        out.append((run[0], side, run, what + " first"))
        out.append((run[0] + run[1] - 1, side, run, what + " last"))

    for j in (0, 7):
        hy0, hy3 = wave_map(ne, hp, j, 4 * q), wave_map(ne, hp, j, 4 * q + 3)
        nb, last = wave_map(ne, hp, j, a_wave(ne, hp)), wave_map(ne, hp, j, 15)
        if q or not hp:
            ends(wave_map(ne, hp, j, 0)[2][0], "exact", f"wg{j} exact wave 0")
        if not hp:          # whole waves: the last exact wave's last column (workgroup 7: C0 - 1)
            r = wave_map(ne, hp, j, ne - 1)[2][0]
            out.append((r[0] + 7, "exact", r, f"wg{j} last exact wave last"))
        if hp:
            out.append((hy0[2][0][0], "exact", hy0[2][0], f"wg{j} hybrid wave on SIMD 0, exact run first"))
            r = hy3[2][0]
            out.append((r[0] + r[1] - 1, "exact", r, f"wg{j} hybrid wave on SIMD 3, exact run last"))   # wg 7: C0 - 1
            ends(hy0[3][0], "bound", f"wg{j} first bound run (hybrid wave on SIMD 0)")
            if j == 0:
                ends(hy3[3][0], "bound", f"wg{j} hybrid wave on SIMD 3, bound run")
            else:
                out.append((hy3[3][0][0] + hy3[3][0][1] - 1, "bound", hy3[3][0], f"wg{j} hybrid wave on SIMD 3, bound run last"))
        if j == 0:
            ends(nb[3][0], "bound", f"wg{j} first bound-only wave, beside the hybrid ones")
            ends(last[3][0], "bound", f"wg{j} last bound run")
        else:
            out.append((nb[3][0][0], "bound", nb[3][0], f"wg{j} first bound-only wave first"))
            out.append((last[3][0][0] + 7, "bound", last[3][0], f"wg{j} last bound run last"))               # column 1023
    return out


# ---------------------------------------------------------------------------------------------------- streams

ON = 4                  # hops a line is on, then off: frames 5 and 6 of every 8 hold it throughout
LOUD, CONFINED = E.LOUD, E.CONFINED


def _at_bin(t, k, theta0):
    return np.cos(np.pi * (k + 0.5) / HOP * (t + 1024.5) + theta0)


def aimed_stream(sr, ch, frames, targets):
    """A tone at about 1 kHz in every channel (the phase that gives every frame the same scale) and, in hops 4..7 of
    every 8, the line of targets[(hop // 8) * ch + channel] = (column, dB over the noise floor) - encode_screen_edges
    line_stream with one line per stretch and channel.  The line is alone in its bin in the EVEN frames."""
    n = frames * HOP
    t = np.arange(n, dtype=np.float64)
    kt = int(round(1000.0 * 2048 / sr - 0.5))
    at = 0.5
    x = np.repeat((at * _at_bin(t, kt, np.pi / 4))[:, None], ch, axis=1)
    hop = np.arange(n) // HOP
    for i, (k, db) in enumerate(targets):
        s, c = divmod(i, ch)
        on = (hop >= 8 * s + ON) & (hop < 8 * s + 2 * ON)
        al = at * np.cos(np.pi / 4) * float(NOISE_FLOOR) * 10.0 ** (db / 20.0)
        x[:, c] += on * al * _at_bin(t, k, 0.0)
    return x


F0 = 2      # first frame of every case: clear of the leading zero padding, and even, so row parity is frame parity


def aimed_case(sr, ch, M):
    """M rows from frame F0 on; aim i sits in channel i % ch of the stretch (i // ch): its row is that of frame
    8 (i // ch) + 6 - the even frame that holds the line throughout.  -> Edge with .aimed = [(row, column, side, run, what)]."""
    assert M % ch == 0
    nf = M // ch
    _, _, ne = shape(sr)
    hp = shipped_pairs(ne)
    picks = aims(ne, hp)
    n_str = (F0 + nf - 7) // 8 + 1          # stretches whose frame 8 s + 6 is inside [F0, F0 + nf)
    assert len(picks) <= n_str * ch, (sr, ch, M, len(picks), n_str)
    targets = [(k, LOUD if side == "exact" else CONFINED) for k, side, _, _ in picks]
    x = aimed_stream(sr, ch, F0 + nf + 4, targets)
    c = E.Edge(f"aim-{sr}-ch{ch}-m{M}", "balance", sr, ch, x, F0, F0 + nf, values="line")
    c.aimed = [((8 * (i // ch) + 6 - F0) * ch + i % ch, k, side, run, what) for i, (k, side, run, what) in enumerate(picks)]
    assert all(0 <= a[0] < M for a in c.aimed)
    return c


RATES = (48000, 96000, 192000)            # (pairs, q) of the balanced layout (2, 1), (3, 0), (2, 0); 96 kHz takes whole waves
# Rows are whole frames, so a row count is a multiple of the channel count: 256 (one full tile), 257 (a second tile
# with one row) and 515 (no multiple of 4) exist as such for mono; the other channel counts take the nearest counts
# with the same property - a second tile that holds one frame, a count that is no multiple of 4 where one exists
# (none does for 8 channels).
SHAPES = ((1, 256), (1, 257), (1, 515), (2, 256), (2, 514), (3, 258), (3, 513), (8, 256), (8, 264))


def aimed_cases():
    return [aimed_case(sr, ch, M) for sr in RATES for ch, M in SHAPES]


def a_cases():
    """Rows that ONLY the A term fails (encode_screen_edges SUBFLOOR: the line half a dB under the floor), at 48 kHz:
    the even frames of the stretches.  From frame 2 on they are rows 4 lane + 0 and + 2 of the tile, from frame 3 on
    rows 4 lane + 1 and + 3 - the four quarters of the A plane, each written by another workgroup."""
    out = []
    for f0 in (2, 3):
        nf = 260
        x = E.line_stream(48000, 1020, E.SUBFLOOR, f0 + nf + 4)
        whole = [f for f in range(f0, f0 + nf) if (f // 8) % 2 == 1 and f % 8 not in (0, 7)]
        out.append(E.Edge(f"a-rows-f{f0}", "balance-a", 48000, 1, x, f0, f0 + nf,
                          fail_rows=[f - f0 for f in whole if f % 2 == 0], decide="fma", k=1020, db=E.SUBFLOOR, values="line"))
    return out


def reuse_pairs():
    """(larger, smaller) per rate, for one fresh context each: after the 515-row launch the workspace of the 256-row
    one lies inside planes the larger launch wrote at another stride."""
    return [(f"aim-{sr}-ch1-m515", f"aim-{sr}-ch1-m256") for sr in (48000, 96000)]


def all_cases():
    return aimed_cases() + a_cases()
