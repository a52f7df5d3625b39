"""Reanalysis, CPU side (include/agz.h agz_replay_reanalyze_start / _commit): the two entry points
declared, exported and bound (C / ctypes / Julia); the twin (tests/reanalyze_twin.py) on the golden self-play games under
another network -- every row a distribution over the legal moves of its position, the squash rule switching at n = tau;
and the commit rule in numpy against hand-written cases."""
import inspect
import os

import numpy as np
import pytest

import alphago_jl_amd as ag
import orc
import reanalyze_twin as rt
import selfplay_twin as tw
from test_abi import _julia_ccalls, declared_functions
from test_hostsim_selfplay import OracleNet, bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "alphago.jl_amd", "julia", "AlphaGoMI.jl")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("agz_replay_reanalyze_start", "agz_replay_reanalyze_commit")
OK, BAD_ARGUMENT, POOL_EXHAUSTED = ag._lib.OK, ag._lib.BAD_ARGUMENT, ag._lib.POOL_EXHAUSTED


def test_entry_points_are_declared_exported_and_bound():
    L = ag.load()
    jl = open(JL).read()
    calls = {c[0] for c in _julia_ccalls(jl)}
    for name in NAMES:
        assert name in declared_functions(), name
        assert hasattr(L, name) and name in L._agz_signatures, name
        assert name in calls, name
    assert "function reanalyze!(" in jl and "review, reanalyze!," in jl
    assert L.agz_version() == 103
    assert "reanalyze" in ag.__all__ and callable(ag.reanalyze)
    for name in ("reanalyze_start", "reanalyze_commit"):
        assert callable(getattr(ag.Engine, name))
    p = inspect.signature(ag.reanalyze).parameters
    assert [k for k in p][:7] == ["engine", "first", "count", "game_id_base", "commit", "lines", "pv_depth"]
    assert p["first"].default == 0 and p["count"].default is None and p["commit"].default is True
    # one stepping loop behind review() and reanalyze()
    for fn in (ag.review, ag.reanalyze):
        src = inspect.getsource(fn)
        assert "_review_rows(" in src and ".step(" not in src, fn.__name__


def check_rows(N, R, t, moves, start=None):
    """every row of twin game t: a distribution over the legal moves of its position, children_as_pi of the visits under
    the squash rule of its ply.  -> (rows only the squashed form gives, rows only the plain form gives)"""
    only = [0, 0]
    pos = orc.make_pos(N) if start is None else start.copy()
    for k, m in enumerate(moves):
        row, vis = t["pis"][k], t["visits"][k]
        legal = orc.legal_moves(pos).astype(bool)
        assert (row >= 0).all() and (row[~legal] == 0).all(), k
        # every entry is one float32 rounding of its exact quotient: the sum is 1 within 2^-24 relative
        assert abs(float(row.astype(np.float64).sum()) - 1.0) <= 2.0 ** -23, k
        assert vis.sum() >= R - 1 and (vis[~legal] == 0).all(), k
        squash = bool(pos.n <= t["tau"])
        assert bits_equal(row, tw.pi_of(vis.astype(np.float64), squash)), (k, squash)
        if not bits_equal(row, tw.pi_of(vis.astype(np.float64), not squash)):
            only[0 if squash else 1] += 1
        assert -1.0 <= t["qs"][k] <= 1.0
        rc, pos = orc.play(pos, int(m))
        assert rc == orc.OK
    return only


@pytest.mark.parametrize("name,net_seed", [("selfplay_5x5_t1_r16_resign", 7), ("selfplay_9x9_t1_r24", 3)])
def test_twin_rows_on_the_golden_games(name, net_seed):
    """the recorded games searched again under another network: what the new targets must look like"""
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    N, tower, R, seed = (int(x) for x in d["config"])
    A, P = N * N + 1, N * N
    net = OracleNet(N, tower, seed=net_seed)
    plain = moved = 0
    for g in (int(x) for x in d["games"]):
        moves = d[f"g{g}_moves"]
        t = rt.twin_rows(N, net.cb, R, seed, g, moves)
        assert t["tau"] == (P // 12) // 2 * 2 and t["n0"] == 0
        assert t["pis"].shape == (len(moves), A) and t["qs"].shape == (len(moves),)
        plain += check_rows(N, R, t, moves)[1]
        moved += int(not bits_equal(t["pis"], d[f"g{g}_pis"])) + int(not bits_equal(t["qs"], d[f"g{g}_qs"]))
    net.close()
    print(f"{name}: {plain} rows past tau that the squashed form would not give; {moved} tables moved")
    assert plain > 0
    assert moved > 0, "another network moved no target"


def test_squash_rule_switches_at_tau():
    """At R = 16 the early plies spread their readouts one per move, where x^0.98 changes nothing.  R = 64 on a 5x5 board
    visits some moves twice from the first ply on: plies n = 0, 1, 2 <= tau = 2 are rows only the squashed form gives,
    and from n = 3 on there are rows only the plain form gives"""
    d = np.load(os.path.join(GOLDEN, "selfplay_5x5_t1_r16_resign.npz"))
    N, R, moves = 5, 64, d["g3_moves"]
    net = OracleNet(N, 1, seed=2)
    t = rt.twin_rows(N, net.cb, R, 5, 9, moves)
    net.close()
    assert t["tau"] == 2
    squashed, plain = check_rows(N, R, t, moves)
    print(f"{len(moves)} plies: {squashed} only squashed, {plain} only plain")
    assert squashed == 3 and plain >= 1


def _record(pis, qs):
    return dict(pis=np.array(pis, np.float32), qs=np.array(qs, np.float32))


def test_refresh_rule_on_hand_written_cases():
    old = _record([[0.5, 0.5, 0], [0, 0, 0], [0, 1, 0], [0.25, 0.25, 0.5]], [0.1, 0.2, 0.3, 0.4])
    new_pi = np.array([[1, 0, 0], [0.5, 0, 0.5], [0, 0, 1], [0, 0, 1]], np.float32)
    new_q = np.array([-0.1, -0.2, -0.3, -0.4], np.float32)
    # every row OK: the zero row stays zero and still takes its q
    pis, qs, counts = rt.refresh(old, (new_pi, new_q), [OK] * 4)
    assert bits_equal(pis, [[1, 0, 0], [0, 0, 0], [0, 0, 1], [0, 0, 1]]) and bits_equal(qs, new_q)
    assert counts == (4, 3, 0)
    # a short and an invalid row: neither q nor pi moves; the other rows of the game are committed
    pis, qs, counts = rt.refresh(old, (new_pi, new_q), [OK, OK, POOL_EXHAUSTED, BAD_ARGUMENT])
    assert bits_equal(pis, [[1, 0, 0], [0, 0, 0], [0, 1, 0], [0.25, 0.25, 0.5]])
    assert bits_equal(qs, [-0.1, -0.2, 0.3, 0.4]) and counts == (2, 1, 2)
    # nothing OK, and an empty game
    pis, qs, counts = rt.refresh(old, (new_pi, new_q), [POOL_EXHAUSTED] * 4)
    assert bits_equal(pis, old["pis"]) and bits_equal(qs, old["qs"]) and counts == (0, 0, 4)
    pis, qs, counts = rt.refresh(_record(np.zeros((0, 3)), []), (np.zeros((0, 3), np.float32), np.zeros(0, np.float32)), [])
    assert pis.shape == (0, 3) and counts == (0, 0, 0)
    # the inputs are not written to
    assert bits_equal(old["qs"], [0.1, 0.2, 0.3, 0.4]) and bits_equal(old["pis"][2], [0, 1, 0])
    # zero rows before and after: the targets-only index (a ply is a target iff its row is not all zero) holds
    for status in ([OK] * 4, [OK, BAD_ARGUMENT, OK, POOL_EXHAUSTED]):
        pis, _, _ = rt.refresh(old, (new_pi, new_q), status)
        assert ((pis != 0).any(axis=1) == (old["pis"] != 0).any(axis=1)).all()
