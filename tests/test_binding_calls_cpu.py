"""CPU: what the Python binding passes down to the library -- every flight and check method of multiagent_planning_amd/_lib.py driven through
the recording stand-in of tests/bindingcalls.py, against tests/binding_calls.json, the record of the binding before it was last changed.
No library and no GPU: the stand-in takes the library's place, transition_sharded()'s partition() included."""
import json

from multiagent_planning_amd import _lib
import bindingcalls as bc


def test_the_binding_passes_down_what_the_record_holds():
    want = json.load(open(bc.JSON_PATH))
    got = bc.record(_lib)
    for part in ("cases", "errors"):
        assert list(got[part]) == list(want[part]), f"the {part} of tests/bindingcalls.py are not those of the record"
        for name in want[part]:
            assert got[part][name] == want[part][name], f"{part[:-1]} {name}"
    assert got == want


def test_every_refusal_of_the_methods_is_reached_by_an_error_case():
    """every `raise DmpcError` of the flight and check methods and of the private helpers they use, found in the source as it stands"""
    refusals, lines = bc.refusals(_lib), bc.raised_at(_lib)
    stray = [n for n in lines if not any(lo <= n <= hi for _, lo, hi in refusals)]
    assert refusals and not stray, f"error cases end on lines {stray} of _lib.py, which the search of the source does not cover"
    missed = [(name, lo) for name, lo, hi in refusals if not any(lo <= n <= hi for n in lines)]
    assert not missed, f"no error case of tests/bindingcalls.py reaches {missed}"
