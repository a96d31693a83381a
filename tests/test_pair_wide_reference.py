"""The scenes of tests/pair_wide_scene.py held on the CPU to what tests/test_gpu_pair_wide.py needs of them: that they reach
the loop structure of fes_pair_kernels.hpp the 16^3 box never reaches (the arithmetic is done with the header's own constants,
read by regex), which crafted cells share a run of the pairing pass and where the runs are cut, that the cell of a particle
is floor(position) in fp32 and fp64, that 0 < strong < pairs, and the pair reference against its 50-digit twin
(test_pair_reference.exact_parts) on the crafted cells and a fixed sample of about 2000 spread cells.

Measured here (printed by the test, asserted against the constants below):
  the double reference against its 50-digit twin on the wide scenes, as a share of value_bound(out, REF_ULPS): single-stage
      particles 0.451, chains and triples 0.218 -> WIDE_AMPLIFICATION = 4 x 0.218 = 0.88, the margin and derivation of
      test_pair_reference.AMPLIFICATION, which stays 0.16 for the 16^3 scenes.  The largest share belongs to the particles
      of two or three pairs (0.218 among 2240 protons, 0.172 among the 1236 members of triples), of which these scenes hold
      a hundred times as many as the 16^3 ones; it falls with the length of the chain, whose errors do not line up: 0.042
      for 4 .. 20 pairs, 0.0006 for the 410 pairs of the (5, 2048) and (2048, 5) cells;
  fp32: none of the 42875 sampled stored particles differs from the twin, the 410-pair chains included, so the (5, 2048)
      cells stay at their full length (the GPU test's condition is a share below FP32_SHARE = 1e-3 of chains and triples)."""
import math
import os
import re

import numpy as np

import pair_reference as ref
import pair_wide_scene as wide
from helpers import ROOT
from test_pair_reference import FP32_SHARE, REF_ULPS, exact_parts, value_bound

# chains and triples on the wide scenes: 4 x the largest share measured below (0.218), rounded up, as test_pair_reference.AMPLIFICATION
WIDE_AMPLIFICATION = 0.88
SEEDS = wide.SEEDS
SAMPLE = 2000


def constants():
    """the constants of fes_pair_kernels.hpp the scenes are sized against"""
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_pair_kernels.hpp")).read()
    get = lambda name: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))
    k = {name: get(name) for name in ("kPairThreads", "kPairBlocks", "kPairCollideBlocks", "kPairCellMax", "kPairChunk", "kPairScanPer", "kPairCountTurn", "kPairTileCellsMax")}
    assert re.search(r"constexpr\s+int\s+kPairEntries\s*=\s*2\s*\*\s*kPairCellMax\s*;", text)
    k["kPairEntries"] = 2 * k["kPairCellMax"]
    assert re.search(r"__launch_bounds__\(1024\)\s+void\s+pair_scan_kernel", text)
    k["scan_turn"] = 1024 * k["kPairScanPer"]
    return k


def runs_of(k, na, nb=None):
    """The runs of the pairing pass as DESIGN 4.17 states them, per chunk of kPairChunk cells: from c0 the longest stretch of
    cells that are not overfull and whose entries, both species together, fit kPairEntries; an overfull cell is a run of its
    own with length 0.  Returns [(c0, len)]."""
    nb = np.zeros_like(na) if nb is None else nb
    out = []
    for lo in range(0, len(na), k["kPairChunk"]):
        end = min(lo + k["kPairChunk"], len(na))
        c0 = lo
        while c0 < end:
            n, tot = 0, 0
            while c0 + n < end and max(na[c0 + n], nb[c0 + n]) <= k["kPairCellMax"] and tot + na[c0 + n] + nb[c0 + n] <= k["kPairEntries"]:
                tot += na[c0 + n] + nb[c0 + n]
                n += 1
            out.append((c0, n))
            c0 += max(n, 1)
    return out


def test_the_grid_reaches_the_loops():
    k = constants()
    n = wide.NCELLS
    assert n == 37 * 33 * 29 == 35409 and len(set(wide.SHAPE)) == 3 and wide.DV == np.prod(wide.L) / n == 1.0
    assert n % k["kPairScanPer"] == 1                                             # the scan's ragged tail
    assert 2 * k["scan_turn"] < n <= 3 * k["scan_turn"]                           # three turns: the carry is used twice
    chunks = -(-n // k["kPairChunk"])
    assert chunks == 554 > k["kPairCollideBlocks"] == 512 and chunks - k["kPairCollideBlocks"] == 42     # workgroups 0 .. 41 take a second chunk
    assert n - (chunks - 1) * k["kPairChunk"] == 17                               # the clipped last chunk
    for tile, want in (((16, 16, 8), (3, 3, 4)), ((8, 8, 8), (5, 5, 4))):
        assert tuple(-(-s // t) for s, t in zip(wide.SHAPE, tile)) == want and all(s % t for s, t in zip(wide.SHAPE, tile))
        assert tile[0] * tile[1] * tile[2] <= k["kPairTileCellsMax"]              # the LDS forms serve both tilings
    # the crafted cells against the turns and the chunks
    assert sorted(wide.LIKE_TURNS) == [k["scan_turn"] - 1, k["scan_turn"], 2 * k["scan_turn"] - 1, 2 * k["scan_turn"]]
    assert len(set(wide.LIKE_TURNS.values())) == 4 and any(v % 2 for v in wide.LIKE_TURNS.values()) and not all(v % 2 for v in wide.LIKE_TURNS.values())
    assert 2 * k["scan_turn"] == k["kPairCollideBlocks"] * k["kPairChunk"]        # cell 32768 opens chunk 512: workgroup 0's second
    chunk_of = lambda c: c // k["kPairChunk"]
    assert len({chunk_of(wide.LIKE_RUN_AT + i) for i in range(len(wide.LIKE_RUN))}) == 1
    assert [chunk_of(wide.LIKE_STRADDLE_AT + i) for i in range(4)] == [199, 199, 200, 200]
    assert len({chunk_of(wide.UNLIKE_RUN_AT + i) for i in range(len(wide.UNLIKE_RUN))}) == 1
    assert k["kPairCellMax"] == ref.CELL_MAX == 2048
    # the index passes of big_like: the plain forms repeat above kPairBlocks x kPairThreads slots, the LDS forms above
    # kPairBlocks x kPairCountTurn; the wide scenes stay below one trip of either and take many turns of the LDS forms
    lds_trip = k["kPairBlocks"] * k["kPairCountTurn"]
    assert lds_trip == 4194304 and wide.N_BIG == lds_trip + 2 * k["kPairCountTurn"] + 1 > 8 * k["kPairBlocks"] * k["kPairThreads"]
    assert wide.N_BIG < 2 ** 31


def counts_of_scene(pos):
    return np.bincount(wide.cell_index(pos), minlength=wide.NCELLS)


def test_the_crafted_cells_and_where_the_runs_are_cut():
    k = constants()
    s = wide.wide_like()
    na = counts_of_scene(s["pos"])
    assert all(na[c] == n for c, n in wide.LIKE_CRAFTED.items()) and na[0] >= 2 and na[-1] >= 3
    spread = np.delete(na, list(wide.LIKE_CRAFTED))
    assert all((spread == m).sum() > 100 for m in range(6)) and spread.max() < 20       # counts 0, 1, 2, 3, ... everywhere
    runs = dict(runs_of(k, na))
    at = wide.LIKE_RUN_AT
    lo = at - at % k["kPairChunk"]
    # [1500, 1500 | 1500, 2048 | 2049 | 600 ...]: cut by the total, cut at the overfull cell, the overfull cell alone, the rest
    assert runs[lo] == at + 2 - lo and runs[at + 2] == 2 and runs[at + 4] == 0 and runs[at + 5] == lo + k["kPairChunk"] - (at + 5)
    assert na[lo:at + 3].sum() > k["kPairEntries"] >= na[lo:at + 2].sum() and na[at + 2:at + 4].sum() <= k["kPairEntries"]
    # 900, 900 | 900, 900: the chunk boundary cuts, not the total
    at = wide.LIKE_STRADDLE_AT
    c, n = next((c, n) for c, n in runs.items() if c <= at < c + n)
    assert c + n == at + 2 and (at + 2) % k["kPairChunk"] == 0 and na[c:at + 3].sum() <= k["kPairEntries"] and runs[at + 2] == k["kPairChunk"]
    # the last chunk is one run of 17 cells
    assert runs[553 * k["kPairChunk"]] == 17
    assert sum(1 for n in runs.values() if n == 0) == 1

    s = wide.wide_unlike()
    na, nb = counts_of_scene(s["pos_a"]), counts_of_scene(s["pos_b"])
    assert all((na[c], nb[c]) == n for c, n in wide.UNLIKE_CRAFTED.items()) and min(na[0], nb[0], na[-1], nb[-1]) >= 2
    runs = dict(runs_of(k, na, nb))
    at = wide.UNLIKE_RUN_AT
    lo = at - at % k["kPairChunk"]
    # ... | (2048, 2048) | (2048, 2049) | (5, 2048) | (2048, 5) (1300, 700) | (1300, 700) (1300, 700) | (0, 500) (500, 0) ...
    # the cell that fills the LDS alone; the overfull one; two cells that are not overfull and do not fit together; cuts by the total
    assert [runs.get(at + i) for i in range(9)] == [1, 0, 1, 2, None, 2, None, lo + k["kPairChunk"] - (at + 7), None]
    assert runs[lo] == at - lo and na[at] + nb[at] == k["kPairEntries"]
    assert sum(1 for n in runs.values() if n == 0) == 1
    # every cut above is by the total: no other cell of either scene is overfull
    assert (np.maximum(na, nb) > k["kPairCellMax"]).sum() == 1

    b = wide.big_like()
    nbig = np.bincount(b["cell"], minlength=wide.NCELLS)
    assert np.array_equal(b["cell"], wide.cell_index(b["pos"])) and len(b["pos"]) == wide.N_BIG
    assert nbig.max() <= k["kPairCellMax"] and nbig.min() >= 2 and 110 < nbig.mean() < 125
    assert all(n > 1 for _, n in runs_of(k, nbig))                                      # and no run of one cell: every chunk is cut by the total


def test_the_cell_is_floor_of_the_position_in_both_precisions():
    """the library stores position / L and takes the cell as int(stored x n); whether the division is done in the stored type
    or in double and then cast, the product lies within 37 x 2^-23 of i + f, an eighth away from the next integer"""
    s, u, b = wide.wide_like(), wide.wide_unlike(), wide.big_like()
    for pos in (s["pos"], u["pos_a"], u["pos_b"], b["pos"]):
        want = np.floor(pos).astype(np.int64)
        frac = pos - want
        assert frac.min() == 0.125 and frac.max() == 0.875 and np.array_equal(frac * 8, np.round(frac * 8))
        assert want.min() == 0 and np.array_equal(want.max(axis=0), np.array(wide.SHAPE) - 1)
        for dtype in (np.float32, np.float64):
            n, length = np.array(wide.SHAPE, dtype=dtype), np.array(wide.L, dtype=dtype)
            for stored in ((pos / np.array(wide.L)).astype(dtype), pos.astype(dtype) / length):
                assert stored.dtype == dtype
                g = stored * n
                assert g.dtype == dtype and np.array_equal(g.astype(np.int64), want)
                assert np.abs(g.astype(np.float64) - pos).max() <= 37 * 2.0 ** -23


def like_request(W):
    return ref.request(wide.LOG_LAMBDA, wide.TAU, wide.ME, wide.QE, wide.ME, wide.QE, W, wide.DV, like=True, **SEEDS)


def unlike_request(W):
    return ref.request(wide.LOG_LAMBDA, wide.TAU, wide.ME, wide.QE, wide.MP, -wide.QE, W, wide.DV, **SEEDS)


def every_counted_pair_moves_both_members(out, *stored):
    """what test_gpu_pair.check_values takes for granted of a scene: a particle changed if and only if a counted pair held it"""
    return all(np.array_equal(out["stages_" + side] > 0, (out["v" + side] != v).any(axis=1)) for side, v in zip("ab", stored))


def test_some_pairs_are_strong_and_some_are_not():
    """on the requests of the GPU test (the scene's SEEDS), with the velocities stored in either precision"""
    for dtype in (np.float32, np.float64):
        s = wide.wide_like()
        out = ref.apply(like_request(s["W"]), wide.cell_index(s["pos"]), np.arange(len(s["pos"])), s["vel"].astype(dtype))
        na = counts_of_scene(s["pos"])
        print("wide_like: %s" % {key: out[key] for key in ("pairs", "strong", "cells", "overfull_cells", "overfull_particles")})
        assert 0 < out["strong"] < out["pairs"] and (out["pairs"], out["cells"]) == wide.like_pairs(na)
        assert (out["overfull_cells"], out["overfull_particles"]) == (1, 2049)
        assert every_counted_pair_moves_both_members(out, s["vel"].astype(dtype))
        s = wide.wide_unlike()
        out = ref.apply(unlike_request(s["W"]), wide.cell_index(s["pos_a"]), np.arange(len(s["pos_a"])), s["vel_a"].astype(dtype),
                        wide.cell_index(s["pos_b"]), np.arange(len(s["pos_b"])), s["vel_b"].astype(dtype))
        na, nb = counts_of_scene(s["pos_a"]), counts_of_scene(s["pos_b"])
        print("wide_unlike: %s" % {key: out[key] for key in ("pairs", "strong", "cells", "overfull_cells", "overfull_particles")})
        live = (np.minimum(na, nb) > 0) & (np.maximum(na, nb) <= 2048)
        assert 0 < out["strong"] < out["pairs"] == np.maximum(na, nb)[live].sum() and out["cells"] == live.sum()
        assert (out["overfull_cells"], out["overfull_particles"]) == (1, 4097)
        assert out["stages_a"].max() == 410 == out["stages_b"].max()                  # the chains of (2048, 5) and (5, 2048): ceil(2048 / 5)
        assert every_counted_pair_moves_both_members(out, s["vel_a"].astype(dtype), s["vel_b"].astype(dtype))
    b = wide.big_like()
    ids = np.flatnonzero(b["cell"] % wide.BIG_EVERY == 0)
    out = ref.apply(like_request(b["W"]), b["cell"][ids], ids, b["vel"][ids])
    print("big_like, every %dth cell: %s" % (wide.BIG_EVERY, {key: out[key] for key in ("pairs", "strong", "cells")}))
    assert 0 < out["strong"] < out["pairs"] and out["cells"] == -(-wide.NCELLS // wide.BIG_EVERY)
    assert every_counted_pair_moves_both_members(out, b["vel"][ids])


# ---- the reference against its 50-digit twin on the crafted cells and a sample of the spread ones
_parts = {}


def twin_parts(req, owners):
    """exact_parts, every owner's 50-digit values computed once per request (they do not depend on the stored type)"""
    memo = _parts.setdefault((req["seed_lo"], req["seed_hi"], req["stream"], req["epoch"]), {})
    owners = np.atleast_1d(owners)
    new = np.array(sorted(set(int(i) for i in owners) - set(memo)), dtype=np.uint64)
    if len(new):
        for i, a, b, c in zip(new, *exact_parts(req, new)):
            memo[int(i)] = (a, b, c)
    got = np.array([memo[int(i)] for i in owners]).reshape(-1, 3)
    return got[:, 0], got[:, 1], got[:, 2]


def sampled(cell, crafted, rng):
    """the particles of the crafted cells and of SAMPLE spread cells (the cells are independent: a subset is a valid request)"""
    spread = np.setdiff1d(np.unique(cell), list(crafted))
    chosen = np.concatenate([rng.choice(spread, SAMPLE, replace=False), list(crafted), [0, wide.NCELLS - 1]])
    return np.flatnonzero(np.isin(cell, chosen))


def sample_runs(dtype, parts=None):
    rng = np.random.default_rng(7)
    s = wide.wide_like()
    cell = wide.cell_index(s["pos"])
    ids = sampled(cell, wide.LIKE_CRAFTED, rng)
    like = ref.apply(like_request(s["W"]), cell[ids], ids, s["vel"][ids].astype(dtype), parts=parts)
    s = wide.wide_unlike()
    ca, cb = wide.cell_index(s["pos_a"]), wide.cell_index(s["pos_b"])
    both = np.concatenate([ca, cb])
    chosen = sampled(both, wide.UNLIKE_CRAFTED, rng)
    ia, ib = chosen[chosen < len(ca)], chosen[chosen >= len(ca)] - len(ca)
    unlike = ref.apply(unlike_request(s["W"]), ca[ia], ia, s["vel_a"][ia].astype(dtype), cb[ib], ib, s["vel_b"][ib].astype(dtype), parts=parts)
    return like, unlike


def test_the_reference_against_its_fifty_digit_twin_on_the_wide_scenes():
    single = chained = 0.0
    for dtype in (np.float64, np.float32):
        differing = total = longest = 0
        for mine, twin in zip(sample_runs(dtype), sample_runs(dtype, twin_parts)):
            assert (mine["pairs"], mine["strong"], mine["cells"]) == (twin["pairs"], twin["strong"], twin["cells"]) and 0 < mine["strong"] < mine["pairs"]
            for side in ("a", "b"):
                if mine["v" + side] is None:
                    continue
                stages = mine["stages_" + side]
                longest = max(longest, int(stages.max()))
                if dtype is np.float32:
                    differing += int((mine["v" + side] != twin["v" + side]).any(axis=1).sum())
                    total += len(mine["v" + side])
                    continue
                share = np.abs(mine["v" + side] - twin["v" + side]) / np.maximum(value_bound(mine, REF_ULPS, side), np.finfo(np.float64).tiny)
                single = max(single, float(share[stages == 1].max()))
                chained = max(chained, float(share[stages > 1].max()))
        assert longest == 410
        if dtype is np.float32:
            print("fp32: %d of %d sampled stored particles differ from the 50-digit twin (the longest chain has %d pairs)" % (differing, total, longest))
            assert differing == 0 and total > 20000 and FP32_SHARE == 1e-3
    print("double reference against its 50-digit twin on the wide scenes, share of value_bound(REF_ULPS): single-stage %.3f, chains and triples %.3f "
          "-> amplification 4 x %.3f = %.3f" % (single, chained, chained, 4 * chained))
    assert single <= 1
    assert 4 * chained <= WIDE_AMPLIFICATION < 4 * chained * 1.5 and math.isfinite(chained)     # the constant is the measurement, rounded up
