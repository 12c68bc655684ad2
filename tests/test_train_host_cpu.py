"""CPU (no GPU): the host side of the any-size train steps (csrc/train_generic.hip, train_info.hip, train_classifier.hip over the shared
csrc/train_step_host.hpp and train_tables.hip) gives, call by call, what it gave before the three copies of that host code became one.

tests/train_host_cases.py lists the calls -- the planners at valid sizes (the plan's bytes) and every refusal the entry points have, with
the two-fault calls that pin which check runs first --; tests/train_host_refusals.json holds the return code and the full text of
dvae_last_error recorded with the library of the commit before the move.  The comparison is exact, and no case is skipped."""
import importlib
import json
import os

import train_host_cases as hc

native = importlib.import_module("disentangled-vae_amd.native")

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_host_refusals.json")) as f:
    RECORDED = hc.unpack(json.load(f))
CASES = hc.cases()


def test_the_recorded_cases_are_the_listed_cases():
    assert sorted(RECORDED) == sorted(CASES)


def test_every_entry_point_has_a_case():
    covered = {entry for entry, _ in CASES.values()}
    assert covered == set(hc.ENTRY_POINTS), (sorted(set(hc.ENTRY_POINTS) - covered), sorted(covered - set(hc.ENTRY_POINTS)))
    exported = {n for n in native.SIGNATURES if n.startswith(("dvae_train_generic_", "dvae_train_info_", "dvae_train_clf_", "dvae_module_generic_",
                                                              "dvae_train_gradnorm_"))}
    assert exported == set(hc.ENTRY_POINTS)


def test_every_recorded_call_past_the_planners_is_a_refusal():
    # nothing here may reach the device: the pointers of these calls are made up
    for k, want in RECORDED.items():
        if not hc.is_planner_case(k):
            assert want[0] in (hc.BADARG, hc.UNSUPPORTED) and want[1], k


def test_replay():
    lib = native.load()
    differ = {}
    for k, (_, run) in CASES.items():
        got = run(lib)
        if got != RECORDED[k]:
            differ[k] = (got, RECORDED[k])
    assert not differ, f"{len(differ)} of {len(CASES)} calls differ: {json.dumps(dict(list(differ.items())[:5]), indent=1)}"
