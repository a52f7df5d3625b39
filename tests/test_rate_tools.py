"""The parent A/B harness of tools/rate_windows.py and the three tools on it (puct_rate.py, explore_rate.py,
surprise_rate.py), without a device: the windows recorded in profiles/ give, through each tool's measure(), the summary
and the measured block recorded beside them -- which pins the keys, the rounding and the bar, not the device -- and the
rounds alternate as documented."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rate_windows as rw  # noqa: E402


@pytest.mark.parametrize("tool,part,count", [("puct_rate", None, 3), ("explore_rate", None, 3), ("surprise_rate", "train", 10)])
def test_recorded_windows_give_the_recorded_summary(tool, part, count):
    rec = json.load(open(os.path.join(ROOT, "profiles", tool + ".json")))
    rec = rec[part] if part else rec
    assert {m: len(w) for m, w in rec["windows"].items()} == dict(parent_off=count, off=count, on=count)
    res, measured = __import__(tool).measure(rec["windows"])
    assert res == rec["summary"]
    assert measured == rec["measured"] and measured["off_within_parent_spread"] is True
    # without the parent's windows: no parent keys, the rest unchanged
    res1, m1 = __import__(tool).measure(dict(rec["windows"], parent_off=[]))
    assert "parent_off" not in res1 and not [k for k in m1 if k.startswith(("off_minus_parent", "parent_spread", "off_within"))]
    assert all(measured[k] == v for k, v in m1.items() if k != "parent")


def test_the_bar_is_every_key_inside_the_parents_spread():
    res = dict(off=dict(a=dict(median=10.06, spread=0.0), b=dict(median=5.0, spread=0.0)),
               parent_off=dict(a=dict(median=10.0, spread=0.05), b=dict(median=5.126, spread=0.2)))
    out = rw.off_against_parent(res, dict(a=("a", 4), kb=("b", 2)))
    assert out == dict(off_minus_parent_a=0.06, off_minus_parent_kb=-0.13, parent_spread_a=0.05, parent_spread_kb=0.2,
                       off_within_parent_spread=False)
    res["parent_off"]["a"]["spread"] = 0.06
    assert rw.off_against_parent(res, dict(a=("a", 4), kb=("b", 2)))["off_within_parent_spread"] is True


def test_rounds_alternate_and_skip_a_missing_parent():
    calls = []

    def run_parent(tree):
        calls.append("parent:" + tree)
        return [dict(k=len(calls))]

    def run_this(k):
        calls.append("this:%d" % k)
        return dict(off=[dict(k=k)], on=[dict(k=k), dict(k=-k)])

    w = rw.parent_rounds(3, "P", run_parent, run_this)
    assert calls == ["parent:P", "this:0", "this:1", "parent:P", "parent:P", "this:2"]
    assert w == dict(parent_off=[dict(k=1), dict(k=4), dict(k=5)], off=[dict(k=0), dict(k=1), dict(k=2)],
                     on=[dict(k=0), dict(k=0), dict(k=1), dict(k=-1), dict(k=2), dict(k=-2)])
    del calls[:]
    w = rw.parent_rounds(3, None, run_parent, run_this)
    assert calls == ["this:0", "this:1", "this:2"] and w["parent_off"] == [] and len(w["off"]) == 3
