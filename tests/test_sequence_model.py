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


# ================================================================================================ generation 3
def facts3(seed):
    """(bad, cover) of a generation-3 seed: the conditions it breaks that every seed must meet (well-formed steps, the forced
    opening, no vacuous removal on the scene's initial particles, the registered operators' windows and periods), and what it
    adds to the coverage"""
    import remove_reference as rr
    sc, steps = model.scene3(seed), model.sequence3(seed)
    state = model.initial_state3(sc)
    bad, cover = [], set()
    total = model.substeps_of(steps)
    ok = (sc["shape"] == model.SHAPE and sc["L"] == (1.0, 1.0, 1.0) and sc["counts"][:2] == [model.N0, model.N1] and sc["staged"] == (seed % 3 == 0)
          and sc["dt"] == (model.em_dt(model.SHAPE, model.L3) if sc["solver"] == "yee" else 5e-9) and 14 <= len(steps) <= 18 and steps[0]["kind"] == "substeps"
          and sc["macro_weight"] == model.DENSITY3 / model.N0 and sc["dv"] == 1.0 / np.prod(model.SHAPE))
    if not ok:
        bad.append("scene")
    cover |= {("scene", sc["solver"], sc["registered"]), ("scene", sc["precision"], sc["registered"])} | ({("scene", "staged", sc["registered"])} if sc["staged"] else set())
    re = model.can_have_rebinned3(sc, steps)
    kinds = [st["kind"] for st in steps]
    want_reads = (6 + len(model.STATS_KINDS3)) if sc["registered"] else model.READS3
    saved, thinned = 0, set()
    for i, st in enumerate(steps):
        kind = st["kind"]
        reads = [r["kind"] for r in st["reads"]]
        if kind not in model.STATE_KINDS3 or len(reads) != want_reads or len(set(reads)) != want_reads or not set(reads) <= set(model.READ_KINDS2 + model.STATS_KINDS3):
            bad.append(("reads", i))
        if st["thinned"] != sorted(thinned):
            bad.append(("thinned", i))
        if kind in model.NEW_KINDS3:
            cover |= {("new", kind, sc["solver"]), ("new", kind, sc["precision"]), ("new", kind, sc["registered"])} | ({("new", kind, "staged")} if sc["staged"] else set())
            if i and re[i - 1]:
                cover.add(("rebinned", kind))
        if st["thinned"] and kind in model.STATE_KINDS2:
            cover.add(("on a thinned handle", kind))
        if st["refused"]:
            cover.add(("refused", kind))
            if not (kind in model.CALLER_ORDER_KINDS3 and st["species"] in thinned or kind == "renumber" and sc["registered"] and thinned) or st["precalc"]:
                bad.append(("refused", i))
        if st["thinned_after"]:
            cover |= {("read of a thinned handle", r) for r in reads}
        if kind in model.INJECT_KINDS3:
            cover |= {("read after an injection", r) for r in reads}
            if thinned & ({0, 1} if kind == "inject_pair" else {st["species"]}):      # (new ids from the id span on, not from n)
                cover.add(("into a thinned species", kind))
        for r in st["reads"]:
            if r.get("refused"):
                cover.add(("refused read", r["kind"]))
            want = (r["kind"] in model.CALLER_ORDER_READS3 and r["species"] in st["thinned_after"]) or (r["kind"] == "saveCheckpoint" and bool(st["thinned_after"]))
            if bool(r.get("refused")) != want:
                bad.append(("refused read", i, r["kind"]))
        if kind == "loadCheckpoint" and not st["file"] < saved:
            bad.append(("file", i))
        saved += sum("file" in r for r in st["reads"])
        if kind in model.POSITION_KINDS2 and st["what"] != "velocity" and sc["solver"] != "none" and not (st["precalc"] or st["refused"]):
            bad.append(("precalc", i))
        # no vacuous removal, as far as the CPU can tell: on the initial particles
        if kind in model.REMOVE_KINDS3 + ("remove_nothing",):
            s = state[st["species"]]
            share = rr.removed_mask(s["ids"], s["frac"], s["vel"], st["where"], st["every"], st["outside"]).mean()
            if not (share == 0 if kind == "remove_nothing" else 0.05 <= share <= 0.8):
                bad.append(("share", i, kind, float(share)))
        if kind == "remove_thinned_by_id":
            cover.add(("by id with a window", st["where"] is not None))
        if kind == "reserve" and st["extra"] >= 1024:
            cover.add(("reserve across a stride",))
        if kind in ("inject_volume", "inject_pair") and st["kw"]["kind"] == "volume":
            cover |= {("volume lattice", st["kw"]["lattice"]), ("volume paired", st["kw"].get("paired", False))}
        if kind in ("inject_flux", "inject_pair") and st["kw"]["kind"] == "flux":
            cover |= {("flux plane on a face", st["kw"]["plane"] in (0.0, 1.0)), ("flux axis", st["kw"]["axis"]), ("flux side", st["kw"]["side"])}
        if kind in model.INJECT_KINDS3:
            cover |= {("reserve first", st["reserve_first"]), ("pair kind", st["kw"]["kind"])} if kind == "inject_pair" else {("reserve first", st["reserve_first"])}
        if kind.startswith("force_") and st["t"] != model.substeps_of(steps[:i]):
            bad.append(("force t", i))
        thinned = set(st["thinned_after"])
    # the forced opening
    first = next(i for i, k in enumerate(kinds) if k in model.REMOVE_KINDS3)
    after = steps[first + 1]
    end = next((i for i in range(first + 1, len(steps)) if kinds[i] in ("renumber", "loadCheckpoint") and not steps[i]["refused"]), len(steps))
    within = kinds[first + 2:end]
    reads_within = {r["kind"] for st in steps[first + 2:end] for r in st["reads"]}
    if not (after["kind"] == "substeps" and after["k"] >= sc["sort_interval"] + 1 and all(any(k.startswith(f) for k in within) for f in ("collide_", "gas_", "pair_", "force_"))
            and {"fusionYield", "fusionSpectrum"} <= reads_within and not any(k in model.REMOVE_KINDS3 + ("renumber",) for k in kinds[:first])):
        bad.append("opening")
    if re[first + 1]:      # the forced substeps IS a re-binning push on the thinned species (not on every scene: full EM, sort_interval 0, a hook that un-bins)
        cover.add(("the opening re-bins", seed))
    if sc["registered"]:
        rec = sc["recorders"]
        if not all(total // rec[k]["every"] > rec[k]["capacity"] for k in rec):
            bad.append("a ring does not wrap")
        a, b = sc["force_window"]
        if not (1 < a and b < total and b - a + 1 >= 3):
            bad.append(("envelope", a, b, total))
        for key in ("collide_every", "pair_every", "gas_every", "fusion_every", "spectrum_every"):
            if not total // sc[key]["every"] >= 3:
                bad.append(("due", key))
        for op in sc["remove_every"]:      # the hook's sinks take somebody at their first application, on the initial particles
            s = state[op["species"]]
            share = rr.removed_mask(s["ids"], s["frac"], s["vel"], op["where"], op["every_id"], op["outside"]).mean()
            if not 0.05 <= share <= 0.8:
                bad.append(("sink", float(share)))
        if any(k == "loadCheckpoint" for k, st in zip(kinds, steps) if st["thinned"]):
            bad.append("a rewind of a registered, thinned scene")
        if model.reserved3(sc, total)[0] != sc["counts"][0] + sum(op["kw"]["count"] * -(-total // op["every"]) for op in sc["inject_every"] if op["species"] == 0):
            bad.append("reserved")
    return bad, cover


def required3():
    want = {("scene", x, r) for x in model.SOLVERS + ("fp32", "fp64", "staged") for r in (False, True)}
    want |= {("new", k, x) for k in model.NEW_KINDS3 for x in model.SOLVERS + ("fp32", "fp64", "staged", False, True)}
    want |= {("rebinned", k) for k in model.NEW_KINDS3}
    want |= {("on a thinned handle", k) for k in model.STATE_KINDS2}
    want |= {("read of a thinned handle", r) for r in model.READ_KINDS2} | {("read after an injection", r) for r in model.READ_KINDS2}
    want |= {("refused", k) for k in model.CALLER_ORDER_KINDS3 + ("renumber",)} | {("refused read", r) for r in model.CALLER_ORDER_READS3 + ("saveCheckpoint",)}
    want |= {("into a thinned species", k) for k in model.INJECT_KINDS3}
    want |= {("by id with a window", False), ("by id with a window", True), ("reserve across a stride",), ("volume lattice", False), ("volume lattice", True),
             ("volume paired", False), ("volume paired", True), ("flux plane on a face", False), ("flux plane on a face", True), ("reserve first", False),
             ("reserve first", True), ("pair kind", "volume"), ("pair kind", "flux"), ("flux side", -1), ("flux side", 1)} | {("flux axis", a) for a in range(3)}
    return want


_facts3 = {}


def facts3_of(seed):
    if seed not in _facts3:
        _facts3[seed] = facts3(seed)
    return _facts3[seed]


# sha256 (first 16 hex digits) of plain(scene3) + plain(sequence3) per committed seed, and of the named scenes: generation 3
# is deterministic, and a change of its generator shows here before it silently moves what the GPU tests replay
DIGESTS3 = {
    "seeds": {8: "5d1a7a11c8472116", 24: "816da214419a390e", 82: "4489ae55c586e536", 89: "6675709e3e59e77f", 176: "b83eb494f3315852", 648: "f05884e5226d9abb", 1986: "e52f62a156fe11e0", 2568: "689e1a35ea5eb2a0", 3060: "8ca50ee9cfe9f3a5", 3317: "44e40433fba138da", 3975: "93292da8640468f5", 4778: "7bfe50ae4007d435"},
    "turnover": ["b55346484b3c4002", "95130b3e002d33c8", "279e4fd4b0cae3bc"],
    "named": ["751abf78466dfaa9", "a54dc107abaa0519"],
    "resume": ["b7c49928a6f52434", "adb5290959fc370d", "9f29a2d7d2272552", "2a84f9a9c0dd626f"],
}


def test_generation_3_is_deterministic_and_leaves_generations_1_and_2_alone():
    assert len(model.SEEDS3) == len(set(model.SEEDS3)) == 12
    for seed in model.SEEDS3[:3]:
        assert plain(model.scene3(seed)) == plain(model.scene3(seed)) and plain(model.sequence3(seed)) == plain(model.sequence3(seed))
    assert plain(model.sequence3(model.SEEDS3[0])) != plain(model.sequence3(model.SEEDS3[1]))
    assert {seed: digest(model.scene3(seed), model.sequence3(seed)) for seed in model.SEEDS3} == DIGESTS3["seeds"]
    assert [digest(*model.turnover(*case)) for case in model.TURNOVER_CASES] == DIGESTS3["turnover"]
    assert [digest(model.rewinds(), []), digest(model.hook_overflow(), [])] == DIGESTS3["named"]
    assert [digest(model.resume_scene3(*r, sink), []) for r in model.RESUME for sink in (False, True)] == DIGESTS3["resume"]
    assert model.STATE_KINDS3[:len(model.STATE_KINDS2)] == model.STATE_KINDS2 and len(set(model.STATE_KINDS3)) == len(model.STATE_KINDS2) + 10
    # the scene is generation 2's but for what follows from the edge lengths
    for seed in model.SEEDS3[:3]:
        base, sc = model.scene2(seed), model.scene3(seed)
        assert all(plain(sc[k]) == plain(base[k]) for k in ("seed", "solver", "precision", "sort_interval", "staged", "counts", "masses", "charges", "shape", "addB", "registered"))
    # a fast particle still crosses more than a cell per electrostatic sub-step; omega_p dt is what it was on the millimetre box
    pos, vel = model.particles3(model.SEEDS3[0], 0, model.N0)
    assert np.all((pos >= 0) & (pos < 1)) and (np.abs(vel).max(axis=1) * model.C * model.DT3 > 1.0 / model.SHAPE[0]).sum() > 10
    assert abs(np.sqrt(model.DENSITY3) * model.DT3 / (np.sqrt(1e15) * 5e-12) - 1) < 1e-12


def test_no_generation_3_seed_breaks_a_condition_every_seed_must_meet():
    """well-formed steps; the model's own account of which species are thinned and which calls are refused; the forced
    opening (the first removal, a re-binning substeps on the thinned species, one of each old family and both fusion reads
    before the next renumber); on the scene's initial particles every remove_window / remove_outside / remove_thinned_by_id
    takes between 5 % and 80 % of its species and every remove_nothing nobody (remove_reference.removed_mask); the hook's
    sinks likewise; every ring wraps, every registered family is due three times"""
    for seed in model.SEEDS3:
        assert facts3_of(seed)[0] == [], (seed, facts3_of(seed)[0])


def test_generation_3_reaches_what_it_is_there_for():
    """every new kind under every solver, both precisions, with and without registered operators, with the staged binning
    forced, and directly after a substeps that can have re-binned; every generation-1 and generation-2 state-changing kind
    and every read kind on a handle that is thinned; every read kind after an injection; every caller-order call refused"""
    cover = set().union(*[facts3_of(seed)[1] for seed in model.SEEDS3])
    missing = required3() - cover
    assert not missing, sorted(missing, key=str)
    # ("rebinned", kind) can only come from a scene without registered operators, electrostatic or `none`, with sort_interval > 0:
    # the hook's sources un-bin their species every sub-step (can_have_rebinned3).  On more than a quarter of the seeds the
    # forced opening is a re-binning push on the species that was just thinned
    for seed in model.SEEDS3:
        sc, steps = model.scene3(seed), model.sequence3(seed)
        if any(model.can_have_rebinned3(sc, steps)):
            assert not sc["registered"] and sc["solver"] != "yee" and sc["sort_interval"] > 0
    assert sum(1 for c in cover if c[0] == "the opening re-bins") * 4 > len(model.SEEDS3)


def test_the_arithmetic_of_the_generation_3_named_sequences():
    import inject_reference as ir
    # turnover: forty sub-steps in pieces of 1, 2, 3 and 5; the id span ends at three times the capacity
    assert sum(model.TURNOVER_PIECES) == 40 and set(model.TURNOVER_PIECES) == {1, 2, 3, 5}
    for case in model.TURNOVER_CASES:
        sc, reads = model.turnover(*case)
        tv = sc["turnover"]
        assert model.N1 + 40 * tv["count"] == 4590 >= 3 * tv["capacity"] and sc["capacities"][1] == tv["capacity"] == 1500 and tv["sink_every"] == 2
        assert tv["feeds"] == ([0, 1] if case[0] == "yee" else [1]) and sc["capacities"][0] >= model.N0 + (40 * tv["count"] if case[0] == "yee" else 0)
        assert (sc["solver"], sc["precision"]) == case and not sc["registered"] and (case[0] != "none" or (sc["addB"] is None and sc["zero_field"]))
        assert len(reads) == len(tv["pieces"]) and all({r["kind"] for r in row} == set(model.READ_KINDS2) for row in reads)
        lo, hi = tv["source"]["lo"][0], tv["source"]["hi"][0]      # nine tenths of the source's window lie inside the sink's
        assert (min(hi, 0.5) - lo) / (hi - lo) >= 0.9
    # the scenes with registered operators: the capacity reserved up front covers every application even if no sink took anybody
    for seed in model.SEEDS3:
        sc, steps = model.scene3(seed), model.sequence3(seed)
        if not sc["registered"]:
            continue
        total = model.substeps_of(steps)
        cap, n = model.reserved3(sc, total), list(sc["counts"])
        for t in range(1, total + 1):
            for op in sc["inject_every"]:
                if t % op["every"] == 0:
                    assert ir.fits(n[op["species"]], cap[op["species"]], n[op["species"]], op["kw"]["count"]), (seed, t)
                    n[op["species"]] += op["kw"]["count"]
        assert all(n[s] <= cap[s] < n[s] + sum(op["kw"]["count"] for op in sc["inject_every"] if op["species"] == s) + 1 for s in range(2))
        pair = [op["kw"] for op in sc["inject_every"] if op["every"] == 1]
        assert len(pair) == 2 and plain(pair[0]) == plain(pair[1]) and [op["species"] for op in sc["inject_every"]] == [0, 1, 0] and sc["inject_every"][2]["kw"]["kind"] == "flux"
        assert [(op["every"], op["species"]) for op in sc["remove_every"]] == [(2, 0), (3, 1)] and sc["remove_every"][1]["every_id"][0] == 3
    # hook_overflow: the third application is the first that does not fit
    sc = model.hook_overflow()
    src = sc["hook"]["sources"][1]
    n = model.N1
    fits = []
    for k in range(3):
        fits.append(ir.fits(n, sc["capacities"][1], n, src["kw"]["count"]))
        n += src["kw"]["count"] if fits[-1] else 0
    assert fits == [True, True, False] and src["species"] == 1 and sc["hook"]["sink"]["species"] == 0 and sc["hook"]["sources"][0]["species"] == 0
    assert sc["capacities"][0] >= model.N0 + 5 * sc["hook"]["sources"][0]["kw"]["count"]
    # rewinds: unregistered, electrostatic fp32, sort_interval 2, the staged binning forced
    sc = model.rewinds()
    assert (sc["solver"], sc["precision"], sc["sort_interval"], sc["staged"], sc["registered"]) == ("poisson_fft", "fp32", 2, True, False)
    # the resumes: the cut is a multiple of every period, the capacities hold the whole run
    for solver, precision in model.RESUME:
        for sink in (False, True):
            sc = model.resume_scene3(solver, precision, sink)
            assert all(model.RESUME_T % op["every"] == 0 for op in sc["inject_every"] + sc["remove_every"]) and len(sc["remove_every"]) == int(sink)
            assert sc["capacities"][:2] == [sc["counts"][s] + sc["inject_every"][s]["kw"]["count"] * -(-model.RESUME_N // sc["inject_every"][s]["every"]) for s in range(2)]
            assert plain(sc["inject_every"][0]["kw"]) == plain(sc["inject_every"][1]["kw"])


# ================================================================================================ generation 4
def facts4(seed):
    """(bad, cover) of a generation-4 seed: the conditions it breaks that every seed must meet, and what it adds to the
    coverage.  The events are the references' on the scene's initial particles (ionize_reference.application,
    burn_reference.application with the cells of cells_of)."""
    import burn_reference as bref
    import ionize_reference as iref
    import remove_reference as rr
    sc, steps = model.scene4(seed), model.sequence4(seed)
    base = model.scene3(seed)
    state = model.initial_state3(sc)
    roles = sc["roles"]
    bad, cover = [], set()
    total = model.substeps_of(steps)
    nb = len(base["counts"])
    ok = (sc["counts"][:nb] == base["counts"] and sc["masses"][:nb] == base["masses"] and set(sc["counts"][nb:]) == {1} and steps[0]["kind"] == "substeps"
          and (sc["masses"][roles["p3"]], sc["charges"][roles["p3"]]) == (4 * model.MP, -2 * model.QE) and (sc["masses"][roles["p4"]], sc["charges"][roles["p4"]]) == (model.MP, -model.QE)
          and (roles["electron"] == 0 or (sc["masses"][roles["electron"]], sc["charges"][roles["electron"]]) == (model.ME, model.QE))
          and all(plain(sc[k]) == plain(base[k]) for k in ("seed", "solver", "precision", "sort_interval", "staged", "shape", "L", "dt", "macro_weight", "addB", "registered"))
          and any(r["kind"] == "saveCheckpoint" for r in steps[0]["reads"]) and sc["empty"] == ([roles["p3"]] if sc["registered"] else []))
    if not ok:
        bad.append("scene")
    cover |= {("scene", sc["solver"], sc["registered"]), ("scene", sc["precision"], sc["registered"])} | ({("scene", "staged", sc["registered"])} if sc["staged"] else set())
    re = model.can_have_rebinned4(sc, steps)
    kinds = [st["kind"] for st in steps]
    want_reads = (6 + len(model.STATS_KINDS4)) if sc["registered"] else model.READS3
    saved, thinned, t = 0, set(sc["empty"]), 0
    burnt = grown = thins_product = False      # since the last rewind or renumber: a burn has thinned somebody, an ionisation has grown somebody
    first_removal = next(i for i, k in enumerate(kinds) if k in model.REMOVE_KINDS3)
    for i, st in enumerate(steps):
        kind = st["kind"]
        reads = [r["kind"] for r in st["reads"]]
        if kind not in model.STATE_KINDS4 or len(reads) != want_reads or len(set(reads)) != want_reads or not set(reads) <= set(model.READ_KINDS2 + model.STATS_KINDS4):
            bad.append(("reads", i))
        if st["thinned"] != sorted(thinned):
            bad.append(("thinned", i))
        if st["refused"] != ((kind in model.CALLER_ORDER_KINDS3 and st["species"] in thinned) or (kind == "renumber" and sc["registered"] and bool(thinned))) or (st["refused"] and st["precalc"]):
            bad.append(("refused", i))
        if kind in model.NEW_KINDS4:
            cover |= {("new", kind, sc["solver"]), ("new", kind, sc["precision"]), ("new", kind, sc["registered"])} | ({("new", kind, "staged")} if sc["staged"] else set())
            if i and re[i - 1]:
                cover.add(("rebinned", kind))
        elif burnt and grown:
            cover.add(("burnt and grown", kind))
        # the events, on the initial particles
        if kind in model.IONIZE_KINDS4:
            req, app = model.ionize_want(sc, state, st)
            share = app["m"] / model.N0
            if not iref.margins_hold(req, app) or not (app["m"] == 0 if kind == "ionize_nothing" else app["m"] >= 2 if kind == "ionize_refused" else 1 <= app["m"] and share <= 0.5):
                bad.append(("ionised", i, kind, app["m"]))
            if kind != "ionize_nothing" and not (st["g_threshold"] <= st["kw"]["g_lo"] < st["kw"]["g_hi"]):
                bad.append(("threshold", i))
            if kind == "ionize":
                cover.add(("ionize into", "a separate species" if st["electron"] != 0 else "its projectiles, thinned" if 0 in thinned else "its projectiles"))
                cover.add(("ionize at the threshold", st["g_threshold"] == st["kw"]["g_lo"]))
        elif kind in model.BURN_KINDS4 + ("burn_nothing", "burn_refused"):
            req, app = model.burn_want(sc, state, st)
            left = [int(app["keep_a"].sum())] + ([int(app["keep_b"].sum())] if st["b"] is not None else [])
            if not bref.conditions_hold(app) or not (app["m"] == 0 if kind == "burn_nothing" else app["m"] >= 2 if kind == "burn_refused" else app["m"] >= 4 and min(left) >= 1):
                bad.append(("burnt", i, kind, app["m"]))
            if st["saturated"] and not (app["accepted"] > app["burnt"] > 0 and app["saturated"] > 0 and app["blocked"] > 0):
                bad.append(("saturated", i, app["accepted"], app["burnt"], app["saturated"]))
            if kind in model.BURN_KINDS4:
                cover |= {("burn", st["form"]), ("burn tracked", st["products"][1] is not None)}
            if kind == "burn_nothing":
                cover.add(("burn_nothing", st["nothing"]))
        if kind == "reserve" and st["extra"] >= 1024 and st["species"] in (roles["p3"], roles["p4"]):
            cover.add(("reserve across a stride on a product",))
        if kind == "loadCheckpoint" and burnt:
            cover.add(("loadCheckpoint after a burn",))
        if kind == "loadCheckpoint" and not st["file"] < saved:
            bad.append(("file", i))
        if kind in model.POSITION_KINDS2 and st["what"] != "velocity" and sc["solver"] != "none" and not (st["precalc"] or st["refused"]):
            bad.append(("precalc", i))
        if kind in model.REMOVE_KINDS3 + ("remove_nothing",) and st["species"] != roles["p3"]:
            s = state[st["species"]]
            share = rr.removed_mask(s["ids"], s["frac"], s["vel"], st["where"], st["every"], st["outside"]).mean()
            if not (share == 0 if kind == "remove_nothing" else 0.05 <= share <= 0.8):
                bad.append(("share", i, kind, float(share)))
        if kind in model.REMOVE_KINDS3 and st["species"] == roles["p3"]:      # (the product's removal: one of two of the consecutive ids the block's burn has made)
            if not (i == first_removal + 6 and st["where"] is None and st["every"][0] == 2 and not st["outside"]):
                bad.append(("the product's removal", i))
            thins_product = True
        if kind in model.BURN_KINDS4 and roles["p3"] in thinned:
            cover.add(("burn into a thinned product", sc["registered"]))
        if kind.startswith("force_") and st["t"] != model.substeps_of(steps[:i]):
            bad.append(("force t", i))
        # the model's account, restated
        t += st.get("k", 0)
        if kind in model.REMOVE_KINDS3:
            thinned.add(st["species"])
        elif kind in model.BURN_KINDS4:
            thinned |= {st["a"]} | ({st["b"]} if st["b"] is not None else set())
            burnt = True
        elif kind == "ionize":
            grown = True
        elif kind == "loadCheckpoint" or (kind == "renumber" and not st["refused"]):
            thinned.clear()
            burnt = grown = False
        elif kind == "substeps" and sc["registered"]:
            thinned |= {op["species"] for op in sc["remove_every"] if t >= op["every"]}
            bu = sc["burn_every"][0]
            if t >= bu["every"]:
                thinned |= {bu["a"]} | ({bu["b"]} if bu["b"] is not None else set())
                burnt = True
            grown = grown or t >= sc["ionize_every"][0]["every"]
        if st["thinned_after"] != sorted(thinned):
            bad.append(("thinned after", i))
        if burnt and grown:
            cover |= {("read burnt and grown", r) for r in reads}
        for r in st["reads"]:
            want = (r["kind"] in model.CALLER_ORDER_READS3 and r["species"] in thinned) or (r["kind"] == "saveCheckpoint" and bool(thinned))
            if bool(r.get("refused")) != want:
                bad.append(("refused read", i, r["kind"]))
        saved += sum("file" in r for r in st["reads"])
    if not set(model.NEW_KINDS4) <= set(kinds) or not thins_product:
        bad.append("a new kind is missing")
    # the forced block: the first removal, a re-binning substeps, an ionize, such a substeps, the saturated burn, such a substeps; both fusion reads behind each
    first = next(i for i, k in enumerate(kinds) if k in model.REMOVE_KINDS3)
    block = steps[first:first + 6]
    pushes = [block[1], block[3], block[5]]
    end = next((i for i in range(first + 1, len(steps)) if kinds[i] in ("renumber", "loadCheckpoint") and not steps[i]["refused"]), len(steps))
    if not (first <= 2 and [b["kind"] for b in block[::2]][1] == "ionize" and block[4]["kind"] in model.BURN_KINDS4 and block[4]["saturated"] and end >= first + 7
            and all(p["kind"] == "substeps" and p["k"] >= sc["sort_interval"] + 1 and {"fusionYield", "fusionSpectrum"} <= {r["kind"] for r in p["reads"]} for p in pushes)
            and not any(k in model.REMOVE_KINDS3 + ("renumber", "loadCheckpoint") for k in kinds[:first])):
        bad.append("block")
    if re[first + 3] and re[first + 5]:      # the block's burn and the substeps behind it meet a handle that a fused re-binning push has reordered
        cover.add(("the block re-bins", seed))
    if sc["registered"]:
        rec = sc["recorders"]
        if not all(total // rec[k]["every"] > rec[k]["capacity"] for k in rec):
            bad.append("a ring does not wrap")
        a, b = sc["force_window"]
        if not (1 < a and b < total and b - a + 1 >= 3):
            bad.append(("envelope", a, b, total))
        ops = [sc[key] for key in ("collide_every", "pair_every", "gas_every", "fusion_every", "spectrum_every")] + sc["ionize_every"] + sc["burn_every"]
        if not all(total // op["every"] >= 3 for op in ops):
            bad.append("due")
        for op in sc["remove_every"]:
            s = state[op["species"]]
            share = rr.removed_mask(s["ids"], s["frac"], s["vel"], op["where"], op["every_id"], op["outside"]).mean()
            if not 0.05 <= share <= 0.8:
                bad.append(("sink", float(share)))
        ionised, burnt0 = model.hook_events4(sc)
        if not (ionised > 0 and burnt0 > 0):
            bad.append(("the hook's first applications", ionised, burnt0))
        # the chain: the first burner's product_a species is a reactant of the second, which is due behind the every-third sink of species 1
        b1, b2 = sc["burn_every"]
        if not (b1["products"] == [roles["p3"], roles["p4"]] and b2["a"] == roles["p3"] and b2["b"] == 1 and b2["products"] == [roles["p4"], None] and b2["every"] == 3
                and any(op["species"] == 1 and op["every"] == 3 for op in sc["remove_every"]) and b1["a"] == 0 and sc["ionize_every"][0]["species"] == 0):
            bad.append("chain")
        # the capacities: generation 3's, and HOOK_GROWTH4 times the events on the initial particles per application
        cap, cap3 = model.reserved4(sc, total), model.reserved3(sc, total)
        gi = max(model.HOOK_GROWTH4 * ionised, model.HOOK_FLOOR4) * (total // sc["ionize_every"][0]["every"])
        gb = max(model.HOOK_GROWTH4 * burnt0, model.HOOK_FLOOR4) * (total // b1["every"])
        want = list(cap3)
        want[roles["electron"]] += gi
        want[1] += gi
        want[roles["p3"]] += gb
        want[roles["p4"]] += 2 * gb
        if cap != want:
            bad.append("reserved")
    return bad, cover


def required4():
    want = {("scene", x, r) for x in model.SOLVERS + ("fp32", "fp64", "staged") for r in (False, True)}
    want |= {("new", k, x) for k in model.NEW_KINDS4 for x in model.SOLVERS + ("fp32", "fp64", "staged", False, True)}
    want |= {("rebinned", k) for k in model.NEW_KINDS4}
    want |= {("burnt and grown", k) for k in model.STATE_KINDS3} | {("read burnt and grown", r) for r in model.READ_KINDS2 + model.STATS_KINDS4}
    want |= {("ionize into", "a separate species"), ("ionize into", "its projectiles, thinned"), ("ionize at the threshold", False), ("ionize at the threshold", True),
             ("burn", "like"), ("burn", "unlike"), ("burn tracked", False), ("burn tracked", True), ("burn_nothing", "above"), ("burn_nothing", "tau"),
             ("loadCheckpoint after a burn",), ("reserve across a stride on a product",), ("burn into a thinned product", False), ("burn into a thinned product", True)}
    return want


_facts4 = {}


def facts4_of(seed):
    if seed not in _facts4:
        _facts4[seed] = facts4(seed)
    return _facts4[seed]


# sha256 (first 16 hex digits) of plain(scene4) + plain(sequence4) per committed seed, of the named scenes and of the resumes
DIGESTS4 = {
    "seeds": {0: "7e1f27ab466ef938", 2: "4b048f5426925b42", 12: "c82d412f9be55d7d", 13: "5a817ebf65a2f483", 21: "1fc9060b0082b6ed", 59: "4bf89f4c4cd757ed", 111: "6e5907555f46c56e", 129: "a085ce7c92bc6aa4", 131: "be127c67cb049395", 149: "aa9f56720c424ae9", 165: "9ce0e4507a5942a4", 187: "f47df5e105e67d2d"},
    "chain": ["2c3afeb18b441edc", "0204019995dd81b2"],
    "named": ["acaf39bfe0d4abaf", "255d8faa414e2e42", "5731d5cadbb794f6"],
    "resume": ["6f5cf24cf89d3af5", "157131ec783851d1", "33c067b578e6f1dc", "236a096cf98ac261"],
}


def digests4():
    return {"seeds": {seed: digest(model.scene4(seed), model.sequence4(seed)) for seed in model.SEEDS4},
            "chain": [digest(model.chain(*case), []) for case in model.CHAIN_CASES],
            "named": [digest(model.reserve_after_register(), []), digest(model.hook_order(), []), digest(model.burner_fails_behind_an_ioniser(), [])],
            "resume": [digest(model.resume_scene4(*r, burner), []) for r in model.RESUME for burner in (False, True)]}


def test_generation_4_is_deterministic_and_leaves_generations_1_to_3_alone():
    assert len(model.SEEDS4) == len(set(model.SEEDS4)) == 12
    for seed in model.SEEDS4[:3]:
        assert plain(model.scene4(seed)) == plain(model.scene4(seed)) and plain(model.sequence4(seed)) == plain(model.sequence4(seed))
    assert plain(model.sequence4(model.SEEDS4[0])) != plain(model.sequence4(model.SEEDS4[1]))
    assert digests4() == DIGESTS4
    # generations 1 to 3 digest as before (generation 3's scenes are generation 2's on the unit box, its steps use generation 2's draws)
    assert {seed: digest(model.scene(seed), model.sequence(seed)) for seed in model.SEEDS} == DIGESTS["seeds"]
    assert {seed: digest(model.scene3(seed), model.sequence3(seed)) for seed in model.SEEDS3} == DIGESTS3["seeds"]
    assert model.STATE_KINDS4[:len(model.STATE_KINDS3)] == model.STATE_KINDS3 and len(set(model.STATE_KINDS4)) == len(model.STATE_KINDS3) + 8
    assert model.STATS_KINDS4[:len(model.STATS_KINDS3)] == model.STATS_KINDS3
    # the scene is generation 3's with more species behind its own
    for seed in model.SEEDS4[:3]:
        base, sc = model.scene3(seed), model.scene4(seed)
        n = len(base["counts"])
        assert all(plain(sc[k]) == plain(base[k]) for k in base if k not in ("counts", "masses", "charges", "generation"))
        assert sc["counts"][:n] == base["counts"] and sorted(sc["roles"].values()) == ([0] if sc["roles"]["electron"] == 0 else []) + list(range(n, len(sc["counts"])))


def test_no_generation_4_seed_breaks_a_condition_every_seed_must_meet():
    """well-formed steps; the model's own account of which species are thinned and which calls are refused, restated; the forced
    block; on the scene's initial particles every ionize has between 1 event and 50 % of its projectiles as events, every burn
    kind with events at least 4 and a survivor of every reactant, every *_nothing exactly none, every *_refused at least 2
    (its target can be one slot short), the saturated burn accepted > burnt > 0 and saturated > 0, with
    burn_reference.conditions_hold and ionize_reference.margins_hold; every registered family due three times, the hook's
    ioniser and first burner with events at their first application, the chain's shape, the capacities by reserved4's rule"""
    for seed in model.SEEDS4:
        assert facts4_of(seed)[0] == [], (seed, facts4_of(seed)[0])


def test_generation_4_reaches_what_it_is_there_for():
    """every new kind under every solver, both precisions, with and without registered operators, with the staged binning
    forced, and directly after a substeps that can have re-binned; every state-changing kind of generations 1 to 3 and every
    read kind on a handle that a burn has thinned and an ionisation has grown; ionize into a thinned electron target and into a
    separate species; a loadCheckpoint after a burn; like, unlike and untracked burns; a reserve across a stride on a product"""
    cover = set().union(*[facts4_of(seed)[1] for seed in model.SEEDS4])
    missing = required4() - cover
    assert not missing, sorted(missing, key=str)
    assert sum(1 for c in cover if c[0] == "the block re-bins") * 4 > len(model.SEEDS4)


def test_the_arithmetic_of_the_generation_4_named_scenes():
    import burn_reference as bref
    import ionize_reference as iref
    # chain: twenty sub-steps in pieces of 1, 2, 3 and 5; species 2 is the first burner's product, the second's reactant and the ioniser's projectile
    assert sum(model.CHAIN_PIECES) == 20 and set(model.CHAIN_PIECES) == {1, 2, 3, 5}
    for case in model.CHAIN_CASES:
        sc = model.chain(*case)
        b1, b2 = sc["burn_every"]
        io = sc["ionize_every"][0]
        assert (sc["solver"], sc["precision"]) == case and (b1["a"], b1["b"], b1["products"]) == (0, None, [2, 3]) and (b2["a"], b2["b"], b2["products"]) == (2, 1, [3, None])
        assert (io["species"], io["kw"]["species"], io["electron"], io["ion"]) == (2, 2, 4, 1) and (case[0] != "none" or (sc["addB"] is None and sc["zero_field"]))
        assert model.burn_want(sc, model.initial_state3(sc), b1)[1]["m"] >= 20
    # reserve_after_register: every reserve crosses a stride of 1024; all four families on species 0 and 1, due every sub-step
    sc = model.reserve_after_register()
    plan = sc["plan"]
    assert plan["reserve"] == [0, sc["roles"]["p3"], 1] and all(sc["capacities"][sp] // 1024 != (sc["capacities"][sp] + plan["extra"]) // 1024 for sp in plan["reserve"])
    assert all(op["every"] == 1 for op in [sc["pair_every"], sc["fusion_every"]] + sc["ionize_every"] + sc["burn_every"])
    assert (sc["pair_every"]["a"], sc["pair_every"]["b"]) == (sc["fusion_every"]["a"], sc["fusion_every"]["b"]) == (sc["burn_every"][0]["a"], sc["burn_every"][0]["b"]) == (0, 1)
    state = model.initial_state3(sc)
    ionised, burnt = model.hook_events4(sc)
    # the room up front holds the applications before the reserves at HOOK_GROWTH4 times the first one's events, the room afterwards all five
    g, p3 = model.HOOK_GROWTH4, sc["roles"]["p3"]
    assert 0 < plan["before"] * g * ionised <= 400 and 0 < plan["before"] * g * burnt <= sc["capacities"][p3] - 1, (ionised, burnt)
    assert (plan["before"] + plan["after"]) * g * max(ionised, burnt) <= min(400, sc["capacities"][p3] - 1) + plan["extra"]
    assert model.fusion_want(sc, state, 0, 1, sc["fusion_every"]["kw"])[1]["reactions_exact"] > 0
    # hook_order: on the initial particles (no beam yet) the ioniser finds only the fast fifth, and the burner's species holds one particle
    for precision in ("fp32", "fp64"):
        sc = model.hook_order(precision)
        io, bu, src = sc["ionize_every"][0], sc["burn_every"][0], sc["inject_every"][0]
        assert (src["every"], io["every"], bu["every"], src["species"], io["species"]) == (1, 1, 1, 0, 0) and bu["a"] == io["electron"] == sc["roles"]["electron"] != 0 and bu["b"] is None
        assert sc["counts"][bu["a"]] == 1 and src["kw"]["drift"][2] == 0.8 and io["kw"]["g_lo"] == io["g_threshold"] == 0.6 and bu["p"] >= 1
        req, app = model.ionize_want(sc, model.initial_state3(sc), io)
        assert 0 < app["m"] < 300 and iref.margins_hold(req, app)
        assert sc["capacities"][0] == model.N0 + sc["substeps"] * src["kw"]["count"]
    # burner_fails_behind_an_ioniser: on the initial particles the first two applications fit the room of three but one slot and
    # the third does not; the replay takes the events from the mate, and asserts the same
    sc = model.burner_fails_behind_an_ioniser()
    req, app = model.burn_want(sc, model.initial_state3(sc), sc["burn_every"][0])
    m0 = app["m"]
    room = model.room_of(1, [m0] * 3)
    assert m0 >= 20 and bref.fits(1, room, 1, m0) and bref.fits(1 + m0, room, 1 + m0, m0) and not bref.fits(1 + 2 * m0, room, 1 + 2 * m0, m0)
    assert sc["fails_at"] == 3 and sc["ionize_every"][0]["every"] == sc["burn_every"][0]["every"] == 1 and sc["capacities"][sc["roles"]["p3"]] >= 1 + 5 * 4 * m0
    # the resumes: the cut is a multiple of every period
    for solver, precision in model.RESUME:
        for burner in (False, True):
            sc = model.resume_scene4(solver, precision, burner)
            ops = sc["inject_every"] + sc["ionize_every"] + sc["burn_every"]
            assert all(model.RESUME_T % op["every"] == 0 for op in ops) and len(sc["burn_every"]) == int(burner) and not sc["remove_every"]
            assert len(sc["capacities"]) == len(sc["counts"]) and sc["roles"]["electron"] != 0
