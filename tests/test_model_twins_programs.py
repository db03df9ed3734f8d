"""The host-side checks of the state-machine programs (tests/model_twins.py): every program the GPU test runs contains the orderings
the caches depend on, and generating one twice gives the same text.  No GPU."""
import pytest

import model_twins as mt


@pytest.mark.parametrize("name", sorted(mt.PROGRAMS))
def test_every_program_contains_what_it_was_built_for(name):
    spec = mt.PROGRAMS[name]
    prog = mt.program_of(name)
    assert prog == mt.program_of(name)                                 # seeded: the same text every time
    stats = mt.check_program(prog, spec["kind"])
    assert 150 <= len(prog) <= 260, len(prog)
    ops = {a.op for a in prog}
    common = {"eval", "eval25", "propagate", "hold", "release", "eval_mode", "manual_seed", "snapshot", "load_snapshot", "year_new",
              "year_fill", "size", "emb_ratio", "to_cpu_and_back", "check_indices"}
    assert common <= ops, common - ops
    assert {a.arg[0] for a in prog if a.op == "size"} | {96} == set(mt.SIZES)
    assert {a.arg[0] for a in prog if a.op in ("year_new", "year_fill")} == set(mt.YEARS)
    assert {a.arg[0] for a in prog if a.op == "hold"} == set(mt.HOLD_WHAT)
    if spec["kind"] == "inference":
        assert {a.arg[0] for a in prog if a.op == "replace"} == set(mt.REPLACE_WHAT)
        assert not ops & {"train", "fwd_drop", "train_mode", "modes"}
    else:
        assert {"train", "fwd_drop", "train_mode"} <= ops and "replace" not in ops
        assert {a.arg[1] for a in prog if a.op == "train"} == set(mt.TRAIN_VARIANTS)
        assert {a.arg[0] for a in prog if a.op == "train"} == {True, False}
        assert ("modes" in ops) == (spec["kind"] == "mixed")
        # two forwards, then a backward through the first only: with node masks and without, in train mode and in eval mode
        sim, seen = mt._Sim(), set()
        for a in prog:
            if a.op == "train" and a.arg[1] == "two_fwd":
                seen.add((a.arg[0], sim.training))
            sim.apply(a)
        assert {(True, True), (True, False), (False, True)} <= seen, seen
        assert mt.expected_training_replays(prog) >= 20
        if spec["kind"] == "training":
            # experiment.py:72: eval() is never undone, and every eval-mode step asks for node dropout - the reference-mode run of
            # this text then never reaches a forward that could be captured
            first_eval = next(i for i, a in enumerate(prog) if a.op == "eval_mode")
            assert not any(a.op == "train_mode" for a in prog[first_eval:])
            assert all(a.arg[0] for a in prog[first_eval:] if a.op in ("train", "fwd_drop"))
    print(name, len(prog), stats)


def test_the_two_single_mode_training_programs_are_one_text():
    assert mt.program_of("training_device") == mt.program_of("training_reference")
    assert mt.PROGRAMS["training_device"]["modes"] == ("device", "device")
    assert mt.PROGRAMS["training_reference"]["modes"] == ("reference", "reference")


def test_the_checks_notice_a_program_that_lacks_an_ordering():
    prog = mt.program_of("training_device")
    no_seed = [a for a in prog if a.op != "manual_seed"]
    with pytest.raises(AssertionError, match="manual_seed"):
        mt.check_program(no_seed, "training")
    cut = [a for i, a in enumerate(prog) if not (a.op == "eval25" and i < 60)]
    with pytest.raises(AssertionError):
        mt.check_program(cut, "training")
    with pytest.raises(AssertionError, match="never released"):
        mt.check_program([a for a in prog if a.op != "release"], "training")
