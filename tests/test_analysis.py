"""Batched analysis, CPU side: the agz_analysis layout (C / ctypes / Julia), the new entry points exported and bound,
analyze()'s argument checks, and the Position -> (board, info, history) conversion MCTSPlayer and analyze() share."""
import ctypes as C
import os

import numpy as np
import pytest

import alphago_jl_amd as ag
from test_abi import _c_layout, _julia_ccalls, _julia_struct_layout, declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "alphago.jl_amd", "julia", "AlphaGoMI.jl")
NEW = ("agz_analyze_start", "agz_analyze_progress", "agz_analyze_results")


def test_analysis_layout_agrees_between_c_ctypes_and_julia():
    ct = ag._lib.Analysis
    size, offs = _c_layout("agz_analysis", len(ct._fields_))
    assert C.sizeof(ct) == size == 24
    assert [getattr(ct, f[0]).offset for f in ct._fields_] == offs
    jsize, joffs, _ = _julia_struct_layout(open(JL).read(), "AgzAnalysis")
    assert (jsize, joffs) == (size, offs)


def test_analysis_entry_points_are_exported_and_bound():
    L = ag.load()
    declared = declared_functions()
    jl_calls = {c[0] for c in _julia_ccalls(open(JL).read())}
    for name in NEW:
        assert name in declared and hasattr(L, name) and name in L._agz_signatures, name
        assert name in jl_calls, name
    assert L.agz_version() == 103


def test_analyze_argument_checks():
    env = ag.GoEnv(5)
    pos = ag.Position(env)
    with pytest.raises(TypeError):
        ag.analyze(env, object(), [object()])
    with pytest.raises(ValueError):
        ag.analyze(env, object(), [ag.Position(ag.GoEnv(9))])
    with pytest.raises(ValueError):
        ag.analyze(env, object(), [pos], num_readouts=0)
    with pytest.raises(ValueError):
        ag.analyze(env, object(), [pos], slots=0)
    with pytest.raises(TypeError):                      # a network of this package is needed
        ag.analyze(env, object(), [pos])
    assert ag.analyze(env, object(), []) == []


class _RecordingEngine:
    """stands in for the device engine: records what initialize_game hands to agz_tree_init"""

    def tree_init(self, g, board, **kw):
        self.call = (g, np.array(board), kw)

    def set_draw(self, g, game_id, sel=0):
        pass


def _inline_initialize_game_args(pos):
    """what MCTSPlayer.initialize_game computed before the conversion was factored out"""
    env = pos.env
    last = -1 if not pos.recent else ag.to_flat(pos.recent[-1].move, env)
    hist, b = [], pos._flat()[0].astype(np.int16)
    for k in range(min(7, pos.board_deltas.shape[0])):
        b = b - np.ascontiguousarray(pos.board_deltas[k].T).reshape(-1)
        hist.append(b.astype(np.int8))
    return pos._flat()[0], dict(n=pos.n, to_play=pos.to_play, ko=pos._ko0(), caps=pos.caps, last_move=last,
                                komi=pos.komi, history=np.stack(hist) if hist else None)


def _positions(env, rng):
    N = env.N
    out = [ag.Position(env)]
    for k in range(8):
        board = rng.randint(-1, 2, size=(N, N)).astype(np.int8)
        nd = k                                        # 0..7 deltas, some beyond the 7 the planes use
        deltas = rng.randint(-1, 2, size=(nd, N, N)).astype(np.int8)
        recent = [ag.PlayerMove(1 if i % 2 == 0 else -1, None if rng.rand() < 0.2 else (rng.randint(N), rng.randint(N)))
                  for i in range(k % 4)]
        ko = None if k % 3 else (rng.randint(N), rng.randint(N))
        out.append(ag.Position(env, board=board, n=3 + k, komi=5.5, caps=(k, 2 * k), ko=ko, recent=recent,
                               board_deltas=deltas, to_play=1 if k % 2 else -1))
    return out


@pytest.mark.parametrize("N", [5, 9, 19])
def test_position_arrays_reproduce_initialize_game(N):
    env = ag.GoEnv(N)
    P = N * N
    for pos in _positions(env, np.random.RandomState(N)):
        player = object.__new__(ag.MCTSPlayer)
        player.env, player.engine, player._game_id = env, _RecordingEngine(), 0
        player.initialize_game(pos)
        g, board, kw = player.engine.call
        want_board, want = _inline_initialize_game_args(pos)
        assert g == 0 and (board == want_board).all()
        for k in ("n", "to_play", "ko", "caps", "last_move", "komi"):
            assert kw[k] == want[k], k
        assert (kw["history"] is None) == (want["history"] is None)
        if want["history"] is not None:
            assert (kw["history"] == want["history"]).all()
        # the same arrays through position_arrays, as analyze() sends them to agz_analyze_start
        b, info, hist = ag.position_arrays(pos)
        assert b.dtype == np.int8 and b.shape == (P,) and (b == want_board).all()
        assert hist.dtype == np.int8 and hist.shape == (info.history_len, P)
        assert (info.n, info.to_play, info.ko, (info.caps_black, info.caps_white), info.last_move) == \
            (want["n"], want["to_play"], want["ko"], tuple(want["caps"]), want["last_move"])
        assert info.komi == np.float32(pos.komi)
        assert info.prev_move == (-1 if len(pos.recent) < 2 else ag.to_flat(pos.recent[-2].move, env))
        if want["history"] is not None:
            assert (hist == want["history"]).all()
