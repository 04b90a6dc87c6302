"""The paths of the store's byte movers that the case lists reach, and the models at the new shapes.  No GPU.

tests/store_mover_paths.py names, by geometry alone, where every 16 KiB tile and 16-byte unit of a call's packed
destination space lies.  The first tests hold the UNION of all case lists the GPU modules run (tests/test_store_join.py,
tests/test_store_cut.py, tests/test_store_compact.py) to a fixed set of those names: a class no case reaches fails by
name, so a change to a case list - or to a mover, with the cases it then needs - cannot reopen a hole silently.  The last
tests hold the numpy models to the host twins glc_compact_join / glc_compact_cut on the new cases, byte for byte."""
import pytest

import store_compact_cases as M
import store_cut_cases as K
import store_join_cases as J
import store_mover_paths as P

SECTIONS = P.SECTIONS
KINDS = ("narrow", "wide")                       # a tile of class A, B or C / of class D or E: the movers' two code paths


def universe():
    """Every class of the map, for either mover."""
    out = {("tile", c) for c in "DEFGH"} | {("H", c) for c in "DEFG"}
    for sec in SECTIONS:
        step = 1 if sec == "is_raw" else 4
        out |= {("tile", sec, c) for c in "ABC"} | {("H", "seam", sec), ("H", "end", sec)}
        out |= {("phase", sec, v, k) for v in range(0, 16, step) for k in KINDS}
        out |= {(what, sec, v, k) for what in ("seam", "end") for v in range(step, 16, step) for k in KINDS}
    return out | {("tile", "pairs", "B_empty"), ("tile", "raw", "B_empty")}


# What cannot occur, each with its reason.  Everything else of universe() must be reached.
PLANES = "a plane is 4096 bytes and the raw run starts on a multiple of 64: "
IMPOSSIBLE = {
    "join": [
        (lambda l: l[:2] == ("phase", "raw") and l[2] != 0, PLANES + "source and destination are co-aligned, the phase is 0"),
        (lambda l: l[:2] in (("seam", "raw"), ("end", "raw")), PLANES + "no seam and no end falls inside a unit"),
        (lambda l: l == ("tile", "raw", "C"), PLANES + "the raw run has no padding"),
    ],
    "cut": [
        (lambda l: l[:2] == ("phase", "raw") and l[2] != 0, PLANES + "source and destination are co-aligned, the phase is 0"),
        (lambda l: l[:2] in (("seam", "raw"), ("end", "raw")), PLANES + "no seam and no end falls inside a unit"),
        (lambda l: l == ("tile", "raw", "C"), PLANES + "the raw run has no padding"),
        (lambda l: l[0] == "seam" or l[:2] == ("H", "seam") or (l[0] == "tile" and l[-1] in ("B", "B_empty")),
         "a run of a piece is one contiguous range of the source: the cut has no seams"),
    ],
}


def required(mover):
    return {l for l in universe() if not any(rule(l) for rule, _ in IMPOSSIBLE[mover])}


def join_reached():
    cases = J.edge_cases() + [J.heavy_case(n) for n in J.TILE_CASES + (J.GRID_CASE,)]
    return set().union(*(P.reached(P.join_blobs(c)) for c in cases))


def cut_reached():
    cases = K.edge_cases() + [K.heavy_case(n) for n in K.TILE_CASES + (K.GRID_CASE,)]
    return set().union(*(P.reached(P.cut_blobs(c)) for c in cases))


@pytest.mark.parametrize("mover", ("join", "cut"))
def test_the_case_lists_reach_every_path(mover):
    got = join_reached() if mover == "join" else cut_reached()
    missing = sorted(required(mover) - got, key=str)
    assert not missing, (mover, "no case reaches", missing)
    # the impossible set is impossible: the map finds none of it anywhere
    assert not {l for l in got if any(rule(l) for rule, _ in IMPOSSIBLE[mover])}
    assert all(reason for _, reason in IMPOSSIBLE[mover])


def test_the_old_lists_alone_did_not():
    """What this map was written for: the small cases reach no one-run tile outside pairs and raw, and no second pass."""
    old = set().union(*(P.reached(P.join_blobs(c)) for c in J.edge_cases()))
    assert not {l for l in old if l[0] == "tile" and l[1] in ("is_raw", "scale", "cnt")} and ("tile", "H") not in old
    old = set().union(*(P.reached(P.cut_blobs(c)) for c in K.edge_cases()))
    assert not {l for l in old if l[0] == "tile" and l[1] in ("is_raw", "scale", "cnt")} and ("tile", "H") not in old


EVICT = ("one_blob", "several_blobs", "round_boundary", "short_round_tile", "tile_ge_grid", "job_ge_grid", "tail_ge_cap")


def test_the_eviction_runs_reach_every_path():
    got = set().union(*(P.evict_reached(c, r) for c, r in M.small_runs() + M.grid_runs()))
    missing = [name for name in EVICT if name not in got]
    assert not missing and got <= set(EVICT), ("no run reaches", missing)
    small = set().union(*(P.evict_reached(c, r) for c, r in M.small_runs()))
    assert not small & {"tile_ge_grid", "job_ge_grid", "tail_ge_cap"}
    # the second pass is reached on both sides: out of place, in one 40 MiB round, and by the jobs of a 17 MiB round
    out_of_place, in_place = M.grid_out_of_place(), M.grid_in_place()
    assert "tile_ge_grid" in P.evict_reached(out_of_place) and "tile_ge_grid" in P.evict_reached(in_place, None)
    assert {"job_ge_grid", "short_round_tile", "round_boundary"} <= P.evict_reached(in_place, M.BIG_ROUNDS[0])
    assert "tile_ge_grid" not in P.evict_reached(in_place, M.BIG_ROUNDS[0])
    assert {"short_round_tile", "round_boundary", "several_blobs"} <= P.evict_reached(in_place, M.BIG_ROUNDS[1])


def test_the_map_on_a_hand_made_space():
    """One blob of 40 mono frames in two parts of 23 and 17, no pairs, no planes: 64 + 64 + 192 + 192 bytes, one tile.
    The second part's 17 is_raw bytes, packed 87 .. 104, hold no whole unit, so it has no phase there."""
    parts = [[(64, 23), (64, 17)], [(128, 92), (128, 68)], [(256, 92), (256, 68)], [(384, 0), (320, 0)], [(384, 0), (320, 0)]]
    got = P.reached([(1, 40, parts)])
    assert got == {("tile", "D"), ("tile", "F"), ("tile", "G"),
                   ("phase", "is_raw", 0, "wide"), ("seam", "is_raw", 7, "wide"), ("end", "is_raw", 8, "wide"),
                   ("phase", "scale", 0, "wide"), ("phase", "scale", 4, "wide"), ("seam", "scale", 12, "wide"),
                   ("phase", "cnt", 0, "wide"), ("phase", "cnt", 4, "wide"), ("seam", "cnt", 12, "wide")}


# ------------------------------------------------------------------------------------------ the models at the new shapes

@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    assert hasattr(g.lib, "glc_compact_join") and hasattr(g.lib, "glc_compact_cut")
    return g


@pytest.mark.parametrize("name", J.TILE_CASES + (J.GRID_CASE,))
def test_join_model_equals_the_host_twin(glc_amd, name):
    case = J.heavy_case(name)
    seen = set()
    for k, blobs in enumerate(case["clips"]):
        if len(blobs) == 1 and blobs[0] in seen:              # a filler that has been held already
            continue
        seen.add(blobs[0])
        assert glc_amd.compact_join(blobs, case["ch"]) == J.join(blobs, case["ch"]), (name, "clip", k)


@pytest.mark.parametrize("name", K.TILE_CASES + (K.GRID_CASE,))
def test_cut_model_equals_the_host_twin(glc_amd, name):
    case = K.heavy_case(name)
    for clip, f0, nf in sorted(set(case["cuts"])):
        bits, want = K.cut(case["clips"][clip], case["ch"], f0, nf)
        assert bits == 0
        assert glc_amd.compact_cut(case["clips"][clip], f0, nf, case["ch"]) == want, (name, clip, f0, nf)
