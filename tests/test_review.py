"""Batched game review, CPU side: the new entry point declared, exported and bound (C / ctypes / Julia), review()'s
argument checks, and the conversion of move lists, record dicts and selfplay() players to agz_review_start's arrays."""
import os

import numpy as np
import pytest

import alphago_jl_amd as ag
from test_abi import _julia_ccalls, declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "alphago.jl_amd", "julia", "AlphaGoMI.jl")


def test_review_entry_point_is_declared_exported_and_bound():
    L = ag.load()
    jl = open(JL).read()
    assert "agz_review_start" in declared_functions()
    assert hasattr(L, "agz_review_start") and "agz_review_start" in L._agz_signatures
    assert "agz_review_start" in {c[0] for c in _julia_ccalls(jl)}
    assert "function review(" in jl and "analyze, review," in jl
    assert L.agz_version() == 103
    for name in ("review", "review_arrays"):
        assert name in ag.__all__ and callable(getattr(ag, name))
    for name in ("review_start", "review_progress", "review_results"):
        assert callable(getattr(ag.Engine, name))


def test_review_argument_checks():
    env = ag.GoEnv(5)
    nn = object()
    with pytest.raises(TypeError):
        ag.review(env, nn, [object()])                           # not a game
    with pytest.raises(TypeError):
        ag.review(env, nn, [[12, 1.5]])                          # not a move
    with pytest.raises(TypeError):
        ag.review(env, nn, [{"result": 1}])                      # a dict without moves
    for bad in ([26], [-1], [(5, 0)], [(0, -1)]):
        with pytest.raises(ValueError):
            ag.review(env, nn, [[12] + bad])
    with pytest.raises(ValueError):
        ag.review(env, nn, [[12]], starts=[ag.Position(ag.GoEnv(9))])
    with pytest.raises(TypeError):
        ag.review(env, nn, [[12]], starts=["empty"])
    with pytest.raises(ValueError):
        ag.review(env, nn, [[12], [7]], starts=[None])
    for r in (0, -4, 2.5, True):
        with pytest.raises(ValueError):
            ag.review(env, nn, [[12]], num_readouts=r)
    with pytest.raises(ValueError):
        ag.review(env, nn, [[12]], slots=0)
    with pytest.raises(TypeError):                               # a network of this package is needed
        ag.review(env, nn, [[12]])
    assert ag.review(env, nn, []) == []


def _fake_record(moves, A, game_id=0):
    n = len(moves)
    return dict(index=0, game_id=game_id, num_moves=n, result=1, was_resign=0, resign_disabled=0, final_score=2.5,
                short_searches=0, moves=np.array(moves, np.int16), pis=np.zeros((n, A), np.float32),
                qs=np.zeros(n, np.float32))


@pytest.mark.parametrize("N", [5, 9, 19])
def test_move_lists_records_and_players_convert_alike(N):
    env = ag.GoEnv(N)
    P = N * N
    rng = np.random.RandomState(N)
    flat = [list(rng.randint(0, P + 1, size=k)) for k in (0, 1, 7, 30)]
    flat[2][3] = P                                                # passes
    want_moves = np.array([a for g in flat for a in g], np.int16)
    want_off = np.array([0, 0, 1, 8, 38], np.int64)
    coords = [[ag.from_flat(int(a), env) for a in g] for g in flat]
    records = [_fake_record(g, P + 1, j) for j, g in enumerate(flat)]
    players = [ag.SelfPlayPlayer(env, None, 16, r) for r in records]
    mixed = [flat[0], records[1], players[2], coords[3]]
    as_arrays = [np.array(g, np.int64) for g in flat]
    for games in (flat, coords, records, players, mixed, as_arrays):
        moves, off = ag.review_arrays(env, games)
        assert moves.dtype == np.int16 and off.dtype == np.int64
        assert (moves == want_moves).all() and (off == want_off).all()
    # board coordinates go through to_flat: (row, col) -> row + N * col
    moves, _ = ag.review_arrays(env, [[(1, 2), None, (N - 1, 0)]])
    assert list(moves) == [1 + N * 2, P, N - 1]
