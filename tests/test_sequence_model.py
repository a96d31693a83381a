"""The generator of tests/sequence_model.py on the CPU: it is deterministic in the seed, its steps are well formed, and over the
committed seeds the sequences reach the states the GPU tests are there for — asserted here, not hoped for."""
import hashlib
import json

import numpy as np

import decomp_scene
import gas_reference as gasref
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


# ================================================================================================ generation 1 is pinned
# sha256 (first 16 hex digits) of plain(scene) + plain(steps), computed at the commit before generation 2 was added: the
# scenes and step lists the generation-1 GPU tests replay are what they were.
DIGESTS = {
    "seeds": {0: "b88e361c004645aa", 1: "fa3a421e3aaab58d", 2: "8bf4aa2f5883c5ff", 4: "fc50f0b443bab06e", 5: "2850973631f0dc94", 6: "c20067328dbbd7b4",
              8: "4cd5b3074dae8a8b", 16: "0cdcb9a9c16a6747", 21: "ad9b1dd47dce9b55", 22: "22ea5a20f207999d", 46: "291e5839731051f5", 54: "835d249252043344"},
    "group": ["9add0b9a8791ade5", "8f0273c3d2933819", "61ebd40b7d1f99c9", "39009e2f49291aa5", "9973ebda2bf5c3b2", "4215902dee52dce2"],
    "resume": ["453c8ac7de05169f", "d7a0362d61c5dac3"],
    "pending_rebinning": "23834c3031e82a50",
}


def digest(sc, steps):
    return hashlib.sha256((plain(sc) + plain(steps)).encode()).hexdigest()[:16]


def test_generation_1_is_what_it_was():
    assert model.SEEDS == list(DIGESTS["seeds"])
    assert {seed: digest(model.scene(seed), model.sequence(seed)) for seed in model.SEEDS} == DIGESTS["seeds"]
    assert [digest(model.group_case(i), model.group_sequence(i)) for i in range(len(model.GROUP_CASES))] == DIGESTS["group"]
    assert [digest(model.resume_scene(*r), []) for r in model.RESUME] == DIGESTS["resume"]
    assert digest(*model.pending_rebinning()) == DIGESTS["pending_rebinning"]
    assert (model.RESUME_EVERY, model.RESUME_T, model.RESUME_N) == ((2, 3), 6, 11)


# ================================================================================================ generation 2
def window_side(kw, lengths=model.L):
    """whole, or the side of kGasWindowFirstMax the window's share of the volume lies on"""
    if "lo" not in kw:
        return "whole"
    assert all(0 <= kw["lo"][a] < kw["hi"][a] <= lengths[a] for a in range(3)) and model.window_volume(kw, lengths) < 1
    return "first" if model.window_volume(kw, lengths) < model.gas_window_first_max() else "after"


def facts2(seed):
    """(bad, cover) of a generation-2 seed: the conditions it breaks that every seed must meet (well-formed steps, no vacuous
    request on the scene's initial particles, the registered operators' windows), and what it adds to the coverage"""
    sc, steps = model.scene2(seed), model.sequence2(seed)
    state = model.initial_state(sc)
    bad, cover = [], set()
    total = model.substeps_of(steps)
    nx, ny, nz = sc["shape"]
    ok = (sc["shape"] == model.SHAPE and sc["counts"][:2] == [model.N0, model.N1] and (len(sc["counts"]) == 2 or 1 <= sc["counts"][2] <= 7)
          and sc["staged"] == (seed % 3 == 0) and 0 <= sc["sort_interval"] <= 3 and 14 <= len(steps) <= 17 and steps[0]["kind"] == "substeps")
    if not ok:
        bad.append("scene")
    cover |= {("scene", sc["solver"], sc["registered"]), ("scene", sc["precision"], sc["registered"])} | ({("scene", "staged", sc["registered"])} if sc["staged"] else set())

    def gas(what, kw, where):
        got = model.gas_want(sc, state, what, kw)
        if not 0 < got["collided"] < got["candidates"]:
            bad.append(("gas", where, got))
        if got["below"] + got["above"] > 0:
            cover.add(("gas outside the table",))

    def fusion(a, b, kw, where, spectrum):
        out = model.spectrum_want(sc, state, a, b, kw) if spectrum else model.fusion_want(sc, state, a, b, kw)[1]
        if not (out["pairs"] > 0 and out["reactions_exact"] > 0):
            bad.append(("fusion", where, out["pairs"]))
        if out["below"] + out["above"] > 0:
            cover.add(("pairs outside the table",))
        if spectrum:
            if np.count_nonzero(out["bins"]) < 2:
                bad.append(("spectrum", where, out["bins"]))
            if out["under"] + out["over"] > 0:
                cover.add(("yield outside the axis",))

    re = model.can_have_rebinned(sc, steps, model.POSITION_KINDS2)
    saved, t, seen_substeps = 0, 0, False
    for i, st in enumerate(steps):
        kind = st["kind"]
        reads = [r["kind"] for r in st["reads"]]
        want_reads = model.READS2 + (len(model.STATS_KINDS2) if sc["registered"] else 0)
        if kind not in model.STATE_KINDS2 or len(reads) != want_reads or len(set(reads)) != want_reads or not set(reads) <= set(model.READ_KINDS2 + model.STATS_KINDS2):
            bad.append(("reads", i))
        cover |= {("follows", kind, r) for r in reads}
        if i and re[i - 1] and any(later["kind"] == "substeps" for later in steps[i + (kind != "substeps"):]):
            cover.add(("rebinned", kind))
        seen_substeps |= kind == "substeps"
        if kind in ("setRange", "load", "load_profile", "load_radial"):
            if not (0 < st["first"] and st["count"] >= 1 and st["first"] + st["count"] < sc["counts"][st["species"]]):
                bad.append(("sub-range", i))
            if sc["sort_interval"] > 0 and seen_substeps:
                cover.add(("sub-range on a sorted species", sc["solver"], kind))
        if kind in model.POSITION_KINDS2 and st["what"] != "velocity" and sc["solver"] != "none" and not st["precalc"]:
            bad.append(("precalc", i))
        if kind == "loadCheckpoint" and not st["file"] < saved:
            bad.append(("file", i))
        saved += reads.count("saveCheckpoint")
        if kind == "substeps":
            t += st["k"]
        if "side" in st and kind.startswith("collide_"):
            cover |= {("collide", st["what"]), ("collide side", st["side"])}
        if kind.startswith("force_"):
            kw = st["kw"]
            env = kw.get("envelope")
            active = env is None or env["start"] <= t + kw["epoch"] <= env["stop"]
            if st["t"] != t or st["active"] != active or (env is not None and not env["start"] < env["stop"]) or not all(w["nu"] != 0 and any(w["mode"]) for w in kw["waves"]):
                bad.append(("force", i))
            if active and model.force_inside(sc, state, kw) == 0:
                bad.append(("force kicks nobody", i))
            cover |= {("force", st["what"]), ("waves", len(kw["waves"])), ("force window", window_side(kw) != "whole"), ("force taper", any(x is not None for x in kw["taper"])),
                      ("envelope", "none" if env is None else "active" if active else "inactive"), ("force species", kw["species"])}
            if env is not None and env.get("values"):
                cover.add(("envelope table", active))
        if kind.startswith("gas_"):
            gas(st["what"], st["kw"], i)
            K = gasref.request(sc["L"], 0, **{k: v for k, v in st["kw"].items() if k != "species"})["K"]
            lo, hi = model.gas_compact_range()
            if st["side"] != ("below_lo" if K < lo else "above_lo" if K < (lo * hi) ** 0.5 else "below_hi" if K <= hi else "above_hi") or not 0.85 < K / {"below_lo": lo, "above_lo": lo, "below_hi": hi, "above_hi": hi}[st["side"]] < 1.15:
                bad.append(("gas side", i, K))
            cover |= {("gas", st["what"]), ("gas side", st["side"]), ("gas window", window_side(st["kw"])), ("gas species", st["kw"]["species"]),
                      ("gas taper", any(x is not None for x in st["kw"]["taper"]))}
        if kind == "load_profile":
            cover |= {("density axes", sum(x is not None for x in st["density"])), ("thermal", st["thermal"] is not None), ("shear", st["shear"] is not None),
                      ("profile lattice", st["lattice"]), ("profile what", st["what"])}
        if kind == "load_radial":
            r = st["radial"]
            cover |= {("body", r["geometry"]), ("across", model.radial_is_across(r)), ("radial what", st["what"]), ("radial lattice", st["lattice"])}
            if r["geometry"] == "cylinder":
                cover.add(("cylinder axis", r["axis"]))
            if not all(r.get(k) is not None for k in ("density", "thermal", "flow_radial")):
                bad.append(("radial tables", i))
        for r in st["reads"]:
            if r["kind"] in ("fusionYield", "fusionSpectrum"):
                fusion(r["a"], r["b"], r["kw"], (i, r["kind"]), r["kind"] == "fusionSpectrum")
                cover.add((r["kind"], "like" if r["b"] is None else "unlike") if r["kind"] == "fusionYield" else (r["kind"], r["form"]))
    if sc["registered"]:
        rec = sc["recorders"]
        if not all(total // rec[k]["every"] > rec[k]["capacity"] for k in rec):
            bad.append("a ring does not wrap")
        a, b = sc["force_window"]
        env = sc["force_on"][0]["envelope"]
        # the envelope of the first force opens after the first sub-step and closes before the last one; every family is due three times
        if not (1 < a and b < total and b - a + 1 >= 3 and (env["start"], env["stop"]) == (sc["force_on"][0]["epoch"] + a, sc["force_on"][0]["epoch"] + b)):
            bad.append(("envelope", a, b, total))
        if "envelope" in sc["force_on"][1] or sc["force_on"][0]["species"] == sc["force_on"][1]["species"]:
            bad.append("forces")
        for key in ("collide_every", "pair_every", "gas_every", "fusion_every", "spectrum_every"):
            if not (1 <= sc[key]["every"] <= 3 and total // sc[key]["every"] >= 3):
                bad.append(("due", key))
        for kw in sc["force_on"]:
            if model.force_inside(sc, state, kw) == 0:
                bad.append("a registered force kicks nobody")
        gas(sc["gas_every"]["kind"], sc["gas_every"]["kw"], "registered")
        fusion(sc["fusion_every"]["a"], sc["fusion_every"]["b"], sc["fusion_every"]["kw"], "registered", False)
        fusion(sc["spectrum_every"]["a"], sc["spectrum_every"]["b"], sc["spectrum_every"]["kw"], "registered", True)
    return bad, cover


def required2():
    """what the committed generation-2 seeds must reach together"""
    want = {("rebinned", k) for k in model.STATE_KINDS2}
    want |= {("follows", s, r) for s in model.STATE_KINDS2 for r in model.READ_KINDS2 + model.STATS_KINDS2}
    want |= {("scene", x, r) for x in model.SOLVERS + ("fp32", "fp64", "staged") for r in (False, True)}
    want |= {("force", k) for k in ("field", "accel")} | {("waves", 1), ("waves", 4), ("force window", True), ("force window", False), ("force taper", True), ("force taper", False),
                                                         ("envelope", "none"), ("envelope", "active"), ("envelope", "inactive"), ("force species", 2),
                                                         ("envelope table", True), ("envelope table", False)}
    want |= {("gas", k) for k in ("exchange", "elastic")} | {("gas side", s) for s in ("below_lo", "above_lo", "below_hi", "above_hi")}
    want |= {("gas window", s) for s in ("whole", "first", "after")} | {("gas species", 0), ("gas species", 1), ("gas taper", True), ("gas taper", False), ("gas outside the table",)}
    want |= {("density axes", n) for n in (1, 2, 3)} | {(k, v) for k in ("thermal", "shear", "profile lattice", "radial lattice") for v in (False, True)}
    want |= {(k, w) for k in ("profile what", "radial what") for w in ("position", "velocity", "both")}
    want |= {("body", "sphere"), ("body", "cylinder"), ("across", True), ("across", False)} | {("cylinder axis", a) for a in range(3)}
    want |= {("fusionYield", "like"), ("fusionYield", "unlike"), ("pairs outside the table",), ("yield outside the axis",)} | {("fusionSpectrum", f) for f in ("product", "los", "cm")}
    want |= {("sub-range on a sorted species", s, k) for s in model.SOLVERS for k in ("load_profile", "load_radial")}
    want |= {("collide", w) for w in ("exchange", "elastic")} | {("collide side", s) for s in ("below_lo", "above_lo", "below_hi", "above_hi")}
    return want


_facts2 = {}


def facts_of(seed):
    if seed not in _facts2:
        _facts2[seed] = facts2(seed)
    return _facts2[seed]


def test_generation_2_is_deterministic_and_leaves_generation_1_alone():
    assert len(model.SEEDS2) == len(set(model.SEEDS2)) == 12
    for seed in model.SEEDS2[:3]:
        assert plain(model.scene2(seed)) == plain(model.scene2(seed)) and plain(model.sequence2(seed)) == plain(model.sequence2(seed))
        base = model.scene(seed)
        assert all(plain(model.scene2(seed)[k]) == plain(base[k]) for k in base)          # the scene family is generation 1's
    assert plain(model.sequence2(model.SEEDS2[0])) != plain(model.sequence2(model.SEEDS2[1]))
    assert model.STATE_KINDS2[:len(model.STATE_KINDS)] == model.STATE_KINDS and model.READ_KINDS2[:len(model.READ_KINDS)] == model.READ_KINDS
    assert set(model.POSITION_KINDS2) == set(model.POSITION_KINDS) | {"load_profile", "load_radial"}


def test_no_generation_2_seed_breaks_a_condition_every_seed_must_meet():
    """well-formed steps; on the scene's initial particles every gas request has 0 < collided < candidates (gas_reference),
    every fusion request pairs > 0 and a positive yield (fusion_reference), every spectrum two non-empty bins
    (fusion_spectrum_reference), every active force a particle inside its window; the first registered force's envelope opens
    after the first sub-step and closes before the last; every registered family is due at least three times"""
    for seed in model.SEEDS2:
        assert facts_of(seed)[0] == [], (seed, facts_of(seed)[0])


def test_generation_2_reaches_what_it_is_there_for():
    """every state-changing kind meets a reordered handle; every reading kind follows every state-changing kind (the stats
    reads on scenes with registered operators); solvers x precisions x staged with and without registration; and the forms
    of the new operators the issue names"""
    cover = set().union(*[facts_of(seed)[1] for seed in model.SEEDS2])
    missing = required2() - cover
    assert not missing, sorted(missing, key=str)
    # inside its envelope more often than outside
    forces = [st for seed in model.SEEDS2 for st in model.sequence2(seed) if st["kind"].startswith("force_") and "envelope" in st["kw"]]
    assert 0 < sum(not st["active"] for st in forces) < sum(st["active"] for st in forces)
    seed, index = model.epoch_control()
    st = model.sequence2(seed)[index]
    assert st["t"] > 0 and st["active"] and "envelope" not in st["kw"]


def test_the_named_sequence_of_the_resets():
    sc, steps = model.NAMED2["resets"]()
    assert sc["registered"] and sc["fusion_every"]["every"] == 1 and sc["spectrum_every"]["every"] == 1
    kinds = [st["kind"] for st in steps]
    at = [i for i, st in enumerate(steps) if st.get("reset")]
    assert len(at) == 3 and kinds[at[0]] == "substeps" and kinds[at[1]].startswith("collide_") and kinds[at[2]] == "loadCheckpoint"
    # every piece holds sub-steps: between two resets, before the first and after the last
    cuts = [0] + [i + 1 for i in at] + [len(steps)]
    assert all(model.substeps_of(steps[x:y]) > 0 for x, y in zip(cuts, cuts[1:]))
    state = model.initial_state(sc)
    assert model.fusion_want(sc, state, sc["fusion_every"]["a"], sc["fusion_every"]["b"], sc["fusion_every"]["kw"])[1]["reactions_exact"] > 0
    assert np.count_nonzero(model.spectrum_want(sc, state, sc["spectrum_every"]["a"], sc["spectrum_every"]["b"], sc["spectrum_every"]["kw"])["bins"]) >= 2
    total, rec = model.substeps_of(steps), sc["recorders"]
    assert all(total // rec[k]["every"] > rec[k]["capacity"] for k in rec)
    a, b = sc["force_window"]
    assert 1 < a and b < total
    saved = 0
    for st in steps:
        assert st["kind"] in model.STATE_KINDS2 and all(r["kind"] in model.READ_KINDS2 + model.STATS_KINDS2 for r in st["reads"])
        assert st["kind"] != "loadCheckpoint" or st["file"] < saved
        saved += sum(r["kind"] == "saveCheckpoint" for r in st["reads"])


def test_the_generation_2_group_cases():
    for i in range(len(model.GROUP_CASES)):
        case, steps = model.group_case2(i), model.group_sequence2(i)
        assert plain(steps) == plain(model.group_sequence2(i)) and all(plain(case[k]) == plain(v) for k, v in model.group_case(i).items())
        kinds = [st["kind"] for st in steps]
        assert set(kinds) == set(model.GROUP_STATE_KINDS2) and all(kinds.count(k) == 1 for k in model.GROUP_STATE_KINDS2 if k != "step")
        last = len(kinds) - 1 - kinds[::-1].index("step")
        assert all(kinds.index(k) < last for k in ("reload_profile", "reload_radial"))         # frames after the reloads
        lengths, dt = model.group_lengths(i), model.group_dt(i)
        forces = [case["force_on"]] + [st["kw"] for st in steps if st["kind"].startswith("force_")]
        for kw in forces:      # no application may push a particle beyond the ghost planes between two migrations
            assert kw["species"] == 0 and 0 < model.kick_bound(kw, dt) < model.GROUP_KICK_MAX, (i, model.kick_bound(kw, dt))
            assert all(w["nu"] != 0 and any(w["mode"]) for w in kw["waves"]) and window_side(kw, lengths) in ("whole", "first", "after")
        assert min(model.GROUP_BACKGROUND["vth"]) >= model.GROUP_KICK_MAX
        # no windowed collision request is vacuous on the scene's first particles (gas_reference)
        import fusionpic
        sc = decomp_scene.build(fusionpic, case)
        state = [dict(frac=sc["pos"] / np.array(lengths), vel=sc["vel"], ids=np.arange(sc["n"]))]
        for what, kw in [(case["gas_every"]["kind"], case["gas_every"]["kw"])] + [(st["what"], st["kw"]) for st in steps if st["kind"].startswith("gas_")]:
            got = model.gas_want(dict(L=lengths), state, what, kw)
            assert 0 < got["collided"] <= got["candidates"] and got["candidates"] >= 5, (i, what, got)
        for st in steps:
            if st["kind"].startswith("reload_"):
                assert st["population"]["first"] == 0 and st["population"]["count"] == 3000
            if st["kind"] == "reload_radial":
                r = st["population"]["radial"]
                assert all(2 * r["r_max"] <= lengths[a] for a in range(3) if r["geometry"] == "sphere" or a != r["axis"])
    sides = {st["side"] for i in range(6) for st in model.group_sequence2(i) if "side" in st}
    assert len(sides) >= 3
    assert {model.group_case2(i)["force_on"]["kind"] for i in range(6)} == {"field", "accel"} and {model.group_case2(i)["gas_every"]["kind"] for i in range(6)} == {"exchange", "elastic"}
    bodies = [model.group_sequence2(i)[[st["kind"] for st in model.group_sequence2(i)].index("reload_radial")]["population"]["radial"] for i in range(6)]
    assert {b["geometry"] for b in bodies} == {"sphere", "cylinder"}


def test_the_second_resume_scene():
    for solver, precision in model.RESUME:
        sc = model.resume_scene2(solver, precision)
        every = model.RESUME2_EVERY
        assert (sc["collide_every"]["every"], sc["pair_every"]["every"], sc["gas_every"]["every"], sc["fusion_every"]["every"], sc["spectrum_every"]["every"]) == \
            (every["collide"], every["pair"], every["gas"], every["fusion"], every["spectrum"])
        assert all(model.RESUME_T % e == 0 for e in every.values())
        a, b = sc["force_window"]
        assert 0 < a < model.RESUME_T < b < model.RESUME_N and len(sc["force_on"]) == 2      # the envelope straddles the cut
        assert sc["gas_every"]["kw"]["tau"] == every["gas"] * sc["dt"] and sc["fusion_every"]["kw"]["tau"] == every["fusion"] * sc["dt"]
        state = model.initial_state(sc)
        got = model.gas_want(sc, state, sc["gas_every"]["kind"], sc["gas_every"]["kw"])
        assert 0 < got["collided"] < got["candidates"]
        assert model.fusion_want(sc, state, sc["fusion_every"]["a"], sc["fusion_every"]["b"], sc["fusion_every"]["kw"])[1]["reactions_exact"] > 0
        assert np.count_nonzero(model.spectrum_want(sc, state, sc["spectrum_every"]["a"], sc["spectrum_every"]["b"], sc["spectrum_every"]["kw"])["bins"]) >= 2
