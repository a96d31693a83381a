"""The generator of tests/sequence_model.py on the CPU: it is deterministic in the seed, its steps are well formed, and over the
committed seeds the sequences reach the states the GPU tests are there for — asserted here, not hoped for."""
import json

import numpy as np

import sequence_model as model


def plain(x):
    """a step or a scene as JSON text (arrays as lists): equal text, equal draws"""
    def enc(o):
        if isinstance(o, np.ndarray):
            return o.tolist()
        if isinstance(o, (np.integer, np.floating, np.bool_)):
            return o.item()
        raise TypeError(type(o))
    return json.dumps(x, default=enc, sort_keys=True)


def runs():
    return [(model.scene(seed), model.sequence(seed)) for seed in model.SEEDS]


def test_the_generator_is_deterministic_in_the_seed():
    for seed in model.SEEDS:
        assert plain(model.scene(seed)) == plain(model.scene(seed)) and plain(model.sequence(seed)) == plain(model.sequence(seed))
        a, b = model.particles(seed, 3, 100), model.particles(seed, 3, 100)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert not np.array_equal(a[0], model.particles(seed, 4, 100)[0]) and not np.array_equal(a[0], model.particles(seed + 1, 3, 100)[0])
    assert plain(model.sequence(model.SEEDS[0])) != plain(model.sequence(model.SEEDS[1]))
    for index in range(len(model.GROUP_CASES)):
        assert plain(model.group_sequence(index)) == plain(model.group_sequence(index))


def test_the_scenes_are_the_small_ones_of_the_issue():
    assert len(model.SEEDS) == len(set(model.SEEDS)) == 12
    for sc, steps in runs():
        nx, ny, nz = sc["shape"]
        assert nx > 16 and ny > 16 and nz > 8 and nx % 16 and ny % 16 and nz % 8 and nz % 2 == 0 and nz % 3 == 0
        assert 2000 <= sc["counts"][0] <= 9000 and sc["counts"][1] * 4 == sc["counts"][0] and (len(sc["counts"]) == 2 or 1 <= sc["counts"][2] <= 7)
        assert sc["masses"][1] != sc["masses"][0] and sc["charges"][1] != sc["charges"][0]
        assert sc["staged"] == (sc["seed"] % 3 == 0) and 0 <= sc["sort_interval"] <= 3
        assert sc["dt"] == (model.em_dt(sc["shape"], sc["L"]) if sc["solver"] == "yee" else 5e-12)
        # a fast particle crosses more than a cell per electrostatic sub-step
        pos, vel = model.particles(sc["seed"], 0, sc["counts"][0])
        assert sc["solver"] == "yee" or (np.abs(vel).max(axis=1) * model.C * sc["dt"] > sc["L"][0] / nx).sum() > 10
        assert 12 <= len(steps) <= 16 and steps[0]["kind"] == "substeps"
        saved = 0
        for st in steps:
            assert st["kind"] in model.STATE_KINDS and len(st["reads"]) == 4 and len({r["kind"] for r in st["reads"]}) == 4
            if st["kind"] == "substeps":
                assert st["k"] in (1, 2, 3, 5)
            if st["kind"] in ("setRange", "load"):      # a strict sub-range
                assert 0 < st["first"] and st["count"] >= 1 and st["first"] + st["count"] < sc["counts"][st["species"]]
            if st["kind"] in model.POSITION_KINDS and st["what"] != "velocity" and sc["solver"] != "none":
                assert st["precalc"]                    # the library requires it after positions changed
            if st["kind"] == "loadCheckpoint":
                assert st["file"] < saved               # a file saved earlier in the same sequence
            saved += sum(r["kind"] == "saveCheckpoint" for r in st["reads"])
        if sc["registered"]:
            assert sc["collide_every"]["every"] in (1, 2, 3) and sc["pair_every"]["every"] in (1, 2, 3)
            rec = sc["recorders"]
            assert len({rec[k]["every"] for k in rec}) == 3
            total = sum(st["k"] for st in steps if st["kind"] == "substeps")
            assert all(total // rec[k]["every"] > rec[k]["capacity"] for k in rec), "every ring must wrap"


def test_every_state_changing_kind_meets_a_reordered_handle():
    """every kind directly after a substeps that can have re-binned, and before another substeps"""
    met = set()
    for sc, steps in runs():
        re = model.can_have_rebinned(sc, steps)
        for i in range(1, len(steps)):
            if re[i - 1] and any(st["kind"] == "substeps" for st in steps[i + (steps[i]["kind"] != "substeps"):]):
                met.add(steps[i]["kind"])
    assert met == set(model.STATE_KINDS), set(model.STATE_KINDS) - met


def test_every_reading_kind_follows_every_state_changing_kind():
    met = {(st["kind"], r["kind"]) for _, steps in runs() for st in steps for r in st["reads"]}
    missing = [(s, r) for s in model.STATE_KINDS for r in model.READ_KINDS if (s, r) not in met]
    assert not missing, missing


def test_solvers_precisions_and_the_staged_binning_with_and_without_registered_operators():
    met = set()
    for sc, _ in runs():
        met |= {(sc["solver"], sc["registered"]), (sc["precision"], sc["registered"])}
        if sc["staged"]:
            met.add(("staged", sc["registered"]))
    want = {(x, r) for x in model.SOLVERS + ("fp32", "fp64", "staged") for r in (False, True)}
    assert met == want, want - met


def test_an_odd_save_under_full_em_is_followed_by_more_sub_steps():
    """a saveCheckpoint directly after an odd number of sub-steps with the chained lattice step still open — the comparison of
    that step does not read B of the integer time, and no read before the save does —, and more sub-steps later"""
    found = 0
    for sc, steps in runs():
        if sc["solver"] != "yee":
            continue
        for i, st in enumerate(steps):
            kinds = [r["kind"] for r in st["reads"]]
            if st["kind"] == "substeps" and st["k"] % 2 and "saveCheckpoint" in kinds and not model.compares_face_b(i):
                if "readField" not in kinds[:kinds.index("saveCheckpoint")]:
                    found += any(later["kind"] == "substeps" for later in steps[i + 1:])
    assert found > 0
    # and the twins of full-EM sequences are filled from an open step as often as from a closed one
    assert sum(model.compares_face_b(i) for i in range(16)) == 8


def test_a_strict_sub_range_is_rewritten_on_a_sorted_species_for_every_solver():
    met = set()
    for sc, steps in runs():
        seen_substeps = False
        for st in steps:
            seen_substeps |= st["kind"] == "substeps"
            if st["kind"] in ("setRange", "load") and sc["sort_interval"] > 0 and seen_substeps:
                met.add((sc["solver"], st["kind"]))
    assert {s for s, _ in met} == set(model.SOLVERS) and {k for _, k in met} == {"setRange", "load"}, met


def test_the_collisions_take_both_passes_and_every_load_form():
    sides, loads, elastic = set(), set(), set()
    for sc, steps in runs():
        for st in steps:
            if "side" in st:
                sides.add((st["what"], st["side"]))
            if st["kind"] == "load":
                loads |= {("what", st["what"]), ("lattice", st["lattice"]), ("paired", st["paired"])}
            if st["kind"] == "collide_elastic":
                elastic.add("sigma_tau" in st["kw"])
    assert {s for _, s in sides} == {"below_lo", "above_lo", "below_hi", "above_hi"} and {w for w, _ in sides} == {"exchange", "elastic"}
    assert loads == {("what", "position"), ("what", "velocity"), ("what", "both"), ("lattice", False), ("lattice", True), ("paired", False), ("paired", True)}
    assert elastic == {False, True}


def test_the_group_cases():
    assert len(model.GROUP_CASES) == 6
    cases = [model.group_case(i) for i in range(6)]
    assert {c["world"] for c in cases} == {2, 3} and {c["every"] for c in cases} == {1, 2, 3} and all(c["ghost"] == 2 for c in cases)
    assert {(c["em"], c["distributed_solve"]) for c in cases} == {(False, 0), (False, 1), (True, 0), (True, 1)}
    for i, c in enumerate(cases):
        nx, ny, nz = c["shape"]
        assert nz % c["world"] == 0
        if c["distributed_solve"]:      # bit-identical on the library's own transforms only
            assert all(s & (s - 1) == 0 and s >= 8 for s in c["shape"]) and ny % c["world"] == 0
        if c["em"]:
            assert 2 * (c["ghost"] + 2) <= nz // c["world"]
        steps = model.group_sequence(i)
        kinds = [st["kind"] for st in steps]
        assert 12 <= len(steps) <= 16 and set(kinds) == set(model.GROUP_STATE_KINDS) and kinds.count("pair_refused") == 1 and kinds.count("reload") == 1
        assert kinds.index("reload") < len(kinds) - 1 - kinds[::-1].index("step")          # frames after the reload
    reads = {r["kind"] for i in range(6) for st in model.group_sequence(i) for r in st["reads"]}
    assert reads == set(model.GROUP_READ_KINDS)


def test_the_named_sequences_are_well_formed():
    sc, steps = model.NAMED["pending_rebinning"]()
    assert sc["staged"] and sc["solver"] == "poisson_fft" and not sc["registered"]
    assert plain(steps) == plain(model.NAMED["pending_rebinning"]()[1])
    kinds = [st["kind"] for st in steps]
    pending = [i for i, st in enumerate(steps) if st.get("expect_sort_pass")]
    # a binning precalc() follows sub-steps (the other species holds a fresh census), and before the next sub-steps come a save
    # and a load; the file saved while pending is loaded later
    first = pending[0]
    assert kinds[first - 1] == "substeps" and steps[first]["precalc"] and steps[first]["species"] == 1
    upto = kinds.index("substeps", first)
    assert any(r["kind"] == "saveCheckpoint" for st in steps[first:upto] for r in st["reads"]) and "loadCheckpoint" in kinds[first:upto]
    file_pending = [r["file"] for r in steps[first]["reads"] if r["kind"] == "saveCheckpoint"][0]
    assert any(st["kind"] == "loadCheckpoint" and st["file"] == file_pending for st in steps[upto:])
    saved = 0
    for st in steps:
        assert st["kind"] in model.STATE_KINDS and all(r["kind"] in model.READ_KINDS for r in st["reads"])
        if st["kind"] == "loadCheckpoint":
            assert st["file"] < saved
        saved += sum(r["kind"] == "saveCheckpoint" for r in st["reads"])
