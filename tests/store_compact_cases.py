"""A numpy model of glc_store_compact_device, written from the text of include/glc.h ("evicting clips from the store"),
and the case lists tests/test_store_compact_model.py (CPU) and tests/test_store_compact.py (GPU) share.

An entry is [offset, bytes, n_pairs, n_raw_rows | stored << 32] in Python ints (unsigned 64-bit values): the model
never wraps.  A case is a dict:
  name, arena_bytes, entries, lengths (a list, one per entry), keep (bytes 0..255),
  dst_bytes (None: in place; else the capacity of a disjoint destination arena),
  round (None: any round size; else the in-place round, in bytes, the case was laid out for),
  big (only the grid-stride cases: the arena's bytes are drawn as bytes)."""
import numpy as np

DROPPED, UNUSABLE, OUT_OF_ORDER = -1, -2, -3
U64 = 1 << 64
PATTERN = 0xA5                        # what the GPU tests fill every byte with that must not be written
TILE = 16384                          # bytes one workgroup moves at a time (csrc/glc_kernels.h kStoreMoveTile)
CHUNK = 1024                          # entries of one chunk of the scan
GRID = 2048                           # workgroups of a move launch at most (kStoreMoveGrid): tile GRID is a second pass
TAIL_CAP = 1024 * 256                 # entries one pass of k_store_evict_tail zeroes
DEFAULT_ROUND = 64 << 20              # the in-place round where none is set (csrc/glc_api.hip kStoreCompactRound)


def entry(offset, size, n_pairs=0, n_raw_rows=0, stored=1):
    return [offset % U64, size % U64, n_pairs, (n_raw_rows & 0xFFFFFFFF) | (stored << 32)]


def usable(e, arena_bytes):
    offset, size, _, word3 = e
    return (word3 >> 32) != 0 and offset % 64 == 0 and size % 64 == 0 and size != 0 and offset <= arena_bytes \
        and size <= arena_bytes - offset


def verdicts(arena_bytes, entries, keep):
    """(new_index, the indices of the kept entries in order): the keep byte, the entry rule and the order rule."""
    new_index, kept = [0] * len(entries), []
    ends = 0                                                  # E_i: the maximum of offset + bytes over the candidates in front
    for i, e in enumerate(entries):
        if not keep[i]:
            new_index[i] = DROPPED
            continue
        if not usable(e, arena_bytes):
            new_index[i] = UNUSABLE
            continue
        if e[0] < ends:
            new_index[i] = OUT_OF_ORDER
        else:
            new_index[i] = len(kept)
            kept.append(i)
        ends = max(ends, e[0] + e[1])
    return new_index, kept


def compact(arena, arena_bytes, entries, lengths, keep, dst=None, dst_bytes=None):
    """-> dict(arena: the destination afterwards (the source arena itself in place), entries (n, 4) of Python ints,
    lengths (or None), new_index, n_out, cursor).  `arena` / `dst` are uint8 arrays at least arena_bytes / dst_bytes
    long; neither is modified."""
    n = len(entries)
    in_place = dst is None
    if in_place:
        dst_bytes = arena_bytes
    out = np.array(arena if in_place else dst, np.uint8, copy=True)
    new_index, kept = verdicts(arena_bytes, entries, keep)
    entries_out = [[0, 0, 0, 0] for _ in range(n)]
    lengths_out = None if lengths is None else [0] * n
    place = 0
    for k, i in enumerate(kept):
        offset, size, n_pairs, word3 = entries[i]
        stored = place <= dst_bytes and size <= dst_bytes - place
        entries_out[k] = [place, size, n_pairs, (word3 & 0xFFFFFFFF) | (int(stored) << 32)]
        if lengths is not None:
            lengths_out[k] = lengths[i]
        if stored:
            out[place:place + size] = arena[offset:offset + size]       # from the arena as it was
        place += size
    return dict(arena=out, entries=entries_out, lengths=lengths_out, new_index=new_index, n_out=len(kept), cursor=place)


def arena_of(case, seed=0):
    """The seeded random bytes of a case's source arena (arena_bytes of them)."""
    if case.get("big"):               # tens of MiB: bytes drawn as bytes
        return np.random.default_rng(0x5eed + seed + case["arena_bytes"] % 9973).integers(0, 256, case["arena_bytes"], dtype=np.uint8)
    rng = np.random.RandomState(0x5eed + seed + case["arena_bytes"] % 9973)
    return rng.randint(0, 256, case["arena_bytes"]).astype(np.uint8)


# ------------------------------------------------------------------------------------------ building cases

def laid(sizes, gaps=None, start=0):
    """Entries back to back in index order (gaps[i] unused bytes in front of blob i), and the end of the last."""
    off, out = start, []
    for i, s in enumerate(sizes):
        off += gaps[i] if gaps else 0
        out.append(entry(off, s, n_pairs=7 * i + 1, n_raw_rows=i % 3))
        off += s
    return out, off


def case(name, entries, keep, arena_bytes, dst_bytes=None, rnd=None, lengths=None):
    n = len(entries)
    assert len(keep) == n
    return dict(name=name, arena_bytes=arena_bytes, entries=entries, keep=[int(k) for k in keep],
                lengths=lengths if lengths is not None else [600 + 13 * i for i in range(n)], dst_bytes=dst_bytes, round=rnd)


def keep_patterns():
    sizes = [64, 192, 4096, 64, 1024, 320, 2048, 64]
    ent, end = laid(sizes)
    n = len(sizes)
    pats = dict(all=[1] * n, none=[0] * n, first=[1] + [0] * (n - 1), last=[0] * (n - 1) + [1],
                alternating=[i % 2 for i in range(n)], alternating_even=[1 - i % 2 for i in range(n)],
                front_dropped=[0] + [1] * (n - 1), bytes_2_and_255=[2, 0, 255, 0, 1, 128, 0, 2])
    return [case("keep_" + k, ent, v, end) for k, v in pats.items()]


def own_source_overlap():
    out = []
    ent, end = laid([64, 5 * TILE + 320])                    # a blob of many tiles shifts by 64: it overlaps itself
    out.append(case("shift_64_many_tiles", ent, [0, 1], end))
    ent, end = laid([1024, 1024])
    out.append(case("shift_one_blob", ent, [0, 1], end))
    ent, end = laid([4096, 256])
    out.append(case("shift_larger_than_blob", ent, [0, 1], end))
    ent, end = laid([64, 3 * TILE, 128, 2 * TILE + 64, 64], gaps=[0, 0, 64, 0, 192])
    out.append(case("shifts_grow_along_the_arena", ent, [0, 1, 0, 1, 1], end + 128))
    return out


def round_edges(r):
    """Laid out for an in-place round of r bytes: kept blobs that end on a round boundary of the packed space, begin on
    one, span three rounds; packed totals of exactly 4 r and 4 r + 64; the last blob ending at arena_bytes."""
    half = r // 2
    sizes = [64, half, half, 2 * r + half, 128, half, 64]
    keep = [0, 1, 1, 1, 0, 1, 0]                            # packed: [0, r/2) [r/2, r) [r, 3.5 r) [3.5 r, 4 r)
    ent, end = laid(sizes)
    a = case(f"round_{r}_total_4_rounds", ent, keep, end, rnd=r)
    keep = [0, 1, 1, 1, 0, 1, 1]                            # ... and 64 bytes into a fifth round; the last blob ends the arena
    b = case(f"round_{r}_total_64_over", ent, keep, end, rnd=r)
    ent, end = laid([r, 64, 3 * r])                         # the shift is 64 for a blob of three rounds, from a boundary on
    c = case(f"round_{r}_three_rounds_shift_64", ent, [1, 0, 1], end, rnd=r)
    ent, end = laid([64, 64, r - 64, r], gaps=[0, 0, 0, 5 * r])      # sources far behind their rounds
    d = case(f"round_{r}_far_source", ent, [0, 1, 1, 1], end, rnd=r)
    return [a, b, c, d]


def scan_edges():
    out = []
    ent, end = laid([192])
    out += [case("one_entry_kept", ent, [1], end), case("one_entry_dropped", ent, [0], end)]
    for n in (1023, 1024, 1025, 2050):
        ent, end = laid([64] * n)
        drop = {0, 1022, 1023, 1024, 1025, 2046, 2047, 2048, 2049} | set(range(5, n, 7))
        out.append(case(f"scan_{n}", ent, [0 if i in drop else 1 for i in range(n)], end))
        out.append(case(f"scan_{n}_edges_kept", ent, [1 if i in (0, 1023, 1024, 2047, 2048, n - 1) else i % 3 == 0 for i in range(n)], end))
    # a prefix maximum carried across the chunk edge: entry 1020 reaches to where entry 1040 begins, and the entries
    # between them - the first four in its chunk, the others in the next - begin inside it
    n = 1045
    ent, end = laid([64] * n)
    ent[1020] = entry(1020 * 64, 20 * 64, n_pairs=5)
    c = case("scan_carried_maximum", ent, [1] * n, end)
    out.append(c)
    return out


def damages(arena_bytes):
    return dict(not_stored=lambda e: entry(e[0], e[1], stored=0),
                offset_plus_32=lambda e: entry(e[0] + 32, e[1]),
                bytes_plus_32=lambda e: entry(e[0], e[1] + 32),
                bytes_zero=lambda e: entry(e[0], 0),
                offset_at_end=lambda e: entry(arena_bytes, 64),
                end_outside=lambda e: entry(arena_bytes - 64, 128),
                offset_wraps=lambda e: entry(U64 - 64, e[1]),
                bytes_wrap=lambda e: entry(e[0], U64 - 64))


def unusable_entries():
    out = []
    sizes = [128, 256, 512, 64, 1024, 192]
    for keep_it in (1, 0):
        for name in damages(0):
            ent, end = laid(sizes)
            ent[2] = damages(end)[name](ent[2])
            out.append(case(f"unusable_{name}_keep_{keep_it}", ent, [1, 0, keep_it, 1, 1, 1], end))
    return out


def out_of_order():
    out = []
    ent = [entry(1024, 256, 1), entry(0, 256, 2), entry(2048, 64, 3)]
    out.append(case("descending_pair", ent, [1, 1, 1], 4096))
    ent = [entry(0, 256, 1), entry(512, 512, 2), entry(512, 512, 3), entry(1024, 64, 4)]
    out.append(case("same_blob_twice", ent, [1, 1, 1, 1], 4096))
    ent = [entry(0, 1024, 1), entry(512, 1024, 2), entry(1024, 512, 3), entry(1536, 64, 4)]
    out.append(case("begins_inside_its_predecessor", ent, [1, 1, 1, 1], 4096))     # entry 2 begins below entry 1's end, too
    ent = [entry(0, 1024, 1), entry(512, 3072, 2), entry(1024, 1024, 3), entry(3584, 64, 4)]
    out.append(case("unkept_out_of_order_entry_knocks_nothing_out", ent, [1, 0, 1, 1], 4096))
    ent = [entry(64, 64, 1), entry(0, 64, 2, stored=0), entry(0, 64, 3), entry(128, 64, 4)]
    out.append(case("all_three_codes", ent, [1, 1, 1, 0], 4096))
    return out


def out_of_place():
    sizes = [64, 192, 4096, 64, 1024, 320, 2048, 64]
    ent, end = laid(sizes, gaps=[0, 64, 0, 0, 128, 0, 0, 0])
    keep = [1, 0, 1, 1, 0, 1, 1, 1]
    total = sum(s for s, k in zip(sizes, keep) if k)
    out = [case("out_exact", ent, keep, end, dst_bytes=total), case("out_64_under", ent, keep, end, dst_bytes=total - 64),
           case("out_zero", ent, keep, end, dst_bytes=0), case("out_roomy", ent, keep, end, dst_bytes=total + 4096),
           case("out_half", ent, keep, end, dst_bytes=64 + 4096 + 64),
           case("out_keep_all", ent, [1] * len(sizes), end, dst_bytes=end),
           case("out_keep_none", ent, [0] * len(sizes), end, dst_bytes=end)]
    ent, end = laid([64, 5 * TILE + 320, 64, 2 * TILE])
    out.append(case("out_many_tiles", ent, [0, 1, 0, 1], end, dst_bytes=7 * TILE + 320))
    return out


def small_cases():
    """Every case but the round-edge ones (those take the round they were laid out for)."""
    return keep_patterns() + own_source_overlap() + scan_edges() + unusable_entries() + out_of_order() + out_of_place()


ROUNDS = (1024, 4096)


def all_cases():
    return small_cases() + [c for r in ROUNDS for c in round_edges(r)]


# ------------------------------------------------------------------------------------------ grid-stride edges
# Arenas of tens of MiB: more than GRID tiles, so that the movers' grid-stride loops run a second pass (tests/
# store_mover_paths.py names what a case reaches).  Cheap to describe - the bytes are drawn when a test asks for them.

MIB = 1 << 20
BIG_ROUNDS = (17 * MIB + 64, 3 * TILE + 64, None)         # 2 * tiles above GRID and no multiple of the tile; a few tiles; one round


def big(c):
    c["big"] = True
    return c


def grid_out_of_place():
    """36 MiB of kept blobs out of an arena of 38: large and small ones on both sides of tile GRID, which a large one spans."""
    sizes = [64, 20 * MIB + 320, 128, 9 * MIB + 64, 4096, 64, 5 * MIB + 192, 3 * TILE, 64, 2 * MIB + 64, 192, 64, 320]
    keep = [0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0, 1]
    ent, end = laid(sizes, gaps=[0, 64, 0, 0, 128, 0, 0, 0, 0, 64, 0, 0, 0])
    total = sum(s for s, k in zip(sizes, keep) if k)
    assert total > (GRID + 64) * TILE
    return big(case("grid_out_of_place", ent, keep, end + 64, dst_bytes=total + 128))


def grid_in_place():
    """40 MiB in place: a dropped 64 bytes in front, so every blob shifts by 64 and overlaps its own source; blobs that span
    the boundaries of a 17 MiB + 64 round; a second dropped blob far behind; the last kept blob ends the arena."""
    sizes = [64, 12 * MIB + 320, 9 * MIB + 192, 64, 11 * MIB + 64, 6 * MIB + 128, 4096, 2 * MIB - 4096 - 64 * 9, 64]
    keep = [0, 1, 1, 1, 1, 1, 0, 1, 1]
    ent, end = laid(sizes)
    assert end > 2 * BIG_ROUNDS[0] and end > (GRID + 64) * TILE
    return big(case("grid_in_place", ent, keep, end))


def long_tail():
    """TAIL_CAP + 300 entries of 64 bytes, most dropped, some of the last 300 kept: the zeroed tail of the output arrays is
    longer than one pass of k_store_evict_tail."""
    n = TAIL_CAP + 300
    ent, end = laid([64] * n)
    keep = [1 if i in (3, 1024, 70000, TAIL_CAP - 1, TAIL_CAP, TAIL_CAP + 7, n - 2, n - 1) or i % 50021 == 11 else 0 for i in range(n)]
    return big(case("long_tail", ent, keep, end))


GRID_RUNS = {"grid_out_of_place": (grid_out_of_place, None), "grid_in_place_round_17_mib_64": (grid_in_place, BIG_ROUNDS[0]),
             "grid_in_place_round_3_tiles_64": (grid_in_place, BIG_ROUNDS[1]), "grid_in_place_one_round": (grid_in_place, BIG_ROUNDS[2]),
             "long_tail": (long_tail, None)}


def grid_runs():
    """(case, in-place round) of every run of the grid-stride cases."""
    return [(make(), rnd) for make, rnd in GRID_RUNS.values()]


def small_runs():
    """(case, in-place round) of every run tests/test_store_compact.py makes of the small cases."""
    runs = [(c, None) for c in all_cases()] + [(c, r) for r in ROUNDS for c in round_edges(r)]
    return runs + [(c, 1024) for c in own_source_overlap() + keep_patterns()] + [(c, 1024 + 64) for c in round_edges(4096)]
