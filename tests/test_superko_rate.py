"""tools/superko_rate.py without a device: the windows recorded in profiles/superko_rate.json give, through measure(), the
summary and the measured block recorded beside them (keys and rounding, not the device); and the recorded off-path A/B
against the parent commit says what DESIGN.md section 5x quotes."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_recorded_windows_give_the_recorded_summary():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import superko_rate as sr
    rec = json.load(open(os.path.join(ROOT, "profiles", "superko_rate.json")))
    assert set(rec["windows"]) == set(sr.MODES) and len({len(w) for w in rec["windows"].values()}) == 1
    res, measured = sr.measure(rec["windows"])
    assert res == rec["summary"] and measured == rec["measured"]
    assert all(w["counts_per_step"] == [0.0, 0.0] for w in rec["windows"]["off"])
    assert all(w["k_expand_share"] > 0 for ws in rec["windows"].values() for w in ws)
    for mode in sr.MODES:
        assert rec["data"][mode]["games"] == rec["data"]["shape"]["games"]
    assert rec["data"]["off"]["counters"] == [0, 0]


def test_recorded_bench_ab_is_inside_the_parents_spread():
    ab = json.load(open(os.path.join(ROOT, "profiles", "superko_bench_ab.json")))
    assert ab["dump_outputs_byte_equal_to_parent"] is True and ab["within_parent_spread"] is True
    assert len(ab["parent"]["ms_per_step"]) == len(ab["this"]["ms_per_step"]) == 3
    assert abs(ab["this_minus_parent_median"]) <= ab["parent"]["spread"]
