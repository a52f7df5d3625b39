"""Start positions for self-play and the arena (agz_selfplay_set_starts), on the host simulator: game `gid` begins at entry
gid mod S of the table (arena game g at g mod S) and is, from there, the reference's game -- bit for bit the twins of
tests/selfplay_twin.py in moves, pi, q, result, resign flag and final score.  CPU only."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import alphago_jl_amd as ag
import hs
import orc
import selfplay_twin as tw
from test_hostsim_arena import oracle_eval_game
from test_hostsim_selfplay import OracleNet, bits_equal, oracle_game, run_engine

L = orc.lib()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLIES = (1, 4, 7, 12, 2, 9)            # S = 6 starts: both colours to move, history of 1..7 boards
THRESHOLD = dict(resign_threshold=-0.9, resign_disable_fraction=0.0)      # resignation never disabled


def starts_5x5():
    return tw.random_starts(5, PLIES, seed=0)


def run_sim(N, net, R, seed, games, slots, starts, arena=False, white=None, max_steps=400000, **cfg):
    sim = hs.Sim(board_size=N, games=slots, num_readouts=R, seed=seed, game_id_base=0, game_id_stride=1,
                 record_capacity_games=games + 8, arena_mode=1 if arena else 0, **cfg)
    sim.set_starts(starts)
    sim.start(games)
    steps = 0
    while sim.counters()["finished"] < games and steps < max_steps:
        if arena:
            sim.step(net.on_feats, white.on_feats)
        else:
            sim.step(net.on_feats)
        steps += 1
    recs, ct = sim.records(), sim.counters()
    sim.close()
    return recs, ct


def assert_selfplay_equal(r, o, what):
    assert r["num_moves"] == o["num_moves"], (what, r["num_moves"], o["num_moves"])
    assert (r["moves"] == o["moves"]).all(), what
    assert r["result"] == o["result"] and r["was_resign"] == o["was_resign"], what
    assert r["resign_disabled"] == o["resign_disabled"], what
    assert np.float32(r["final_score"]) == np.float32(o["final_score"]), what
    assert bits_equal(r["qs"], o["qs"]) and bits_equal(r["pis"], o["pis"]), what
    assert r["short_searches"] == 0, what


def assert_records_identical(got, want):
    assert len(got) == len(want)
    for x, y in zip(got, want):
        for k in ("game_id", "num_moves", "result", "was_resign", "resign_disabled", "short_searches"):
            assert x[k] == y[k], k
        assert np.float32(x["final_score"]) == np.float32(y["final_score"])
        assert (x["moves"] == y["moves"]).all() and bits_equal(x["pis"], y["pis"]) and bits_equal(x["qs"], y["qs"])


def assert_arena_equal(r, o, what):
    assert r["num_moves"] == o["num_moves"], (what, r["num_moves"], o["num_moves"])
    assert (r["moves"] == o["moves"]).all(), what
    assert bits_equal(r["qs"], o["qs"]), what
    assert r["result"] == o["result"] and bool(r["was_resign"]) == bool(o["was_resign"]), what
    assert np.float32(r["final_score"]) == np.float32(o["final_score"]), what
    assert int(r["game_id"]) == o["ender"], what
    assert r["short_searches"] == 0, what


# ---------------------------------------------------------------- the twins are the reference loops

@pytest.mark.parametrize("N,R,games", [(5, 16, 4), (9, 16, 1)])
def test_twin_selfplay_from_the_empty_board_is_or_selfplay_ex(N, R, games):
    net = OracleNet(N, 1, seed=0)
    for gid in range(games):
        o = oracle_game(N, net, R, 3, gid, -0.9, 0.05)
        t = tw.twin_selfplay(N, net.cb, R, 3, gid, None, -0.9, 0.05)
        assert t["num_moves"] == o["num_moves"] and (t["moves"] == o["moves"][: t["num_moves"]]).all()
        assert t["result"] == o["result"] and t["evals"] == o["evals"]
        assert t["was_resign"] == (o["result_string"] in (b"B+R", b"W+R"))
        assert bits_equal(t["pis"], o["pis"]) and bits_equal(t["qs"], o["qs"])
    net.close()


def test_twin_arena_from_the_empty_board_is_or_evaluate_game():
    N, R = 5, 16
    black, white = OracleNet(N, 1, seed=0), OracleNet(N, 1, seed=5)
    for g in range(4):
        o = oracle_eval_game(N, black, white, R, 1, g)
        t = tw.twin_arena(N, black.cb, white.cb, R, -0.9, 1, g, None)
        assert t["num_moves"] == o["num_moves"] and (t["moves"] == o["moves"]).all()
        assert bits_equal(t["qs"], o["qs"]) and t["result"] == o["result"] and t["was_resign"] == o["was_resign"]
        assert np.float32(t["final_score"]) == np.float32(o["final_score"])
        assert (t["evals_black"], t["evals_white"]) == o["evals"]
    black.close()
    white.close()


def test_generated_starts_are_legal_unfinished_and_varied():
    for N in (5, 9):
        starts = tw.random_starts(N, PLIES, seed=0) + [tw.setup_start(N), tw.ko_start(N)]
        for p in starts:
            assert not p.done and p.n < tw.max_game_length(N)
            if p.recent_len >= 2:
                assert not (p.recent_move[p.recent_len - 1] == N * N and p.recent_move[p.recent_len - 2] == N * N)
        assert {p.to_play for p in starts} == {1, -1}
        assert {p.ndeltas for p in starts} >= {0, 7}
        assert starts[-1].ko >= 0
        assert starts[-2].n == 0 and starts[-2].to_play == -1 and starts[-2].ndeltas == 0


# ---------------------------------------------------------------- self-play from a table

@pytest.mark.parametrize("games,slots", [(12, 4), (4, 3)])        # more games than S = 6 entries, and S > games
def test_selfplay_from_a_table_equals_the_twin(games, slots):
    N, R, seed = 5, 16, 2
    net = OracleNet(N, 1, seed=0)
    starts = starts_5x5()
    recs, ct = run_sim(N, net, R, seed, games, slots, starts, **THRESHOLD)
    assert len(recs) == games and ct["pool_exhausted"] == 0 and ct["started"] == games
    assert [int(r["game_id"]) for r in recs] == list(range(games))
    moves = evals = 0
    ends = set()
    for r in recs:
        gid = int(r["game_id"])
        o = tw.twin_selfplay(N, net.cb, R, seed, gid, starts[gid % len(starts)], **{
            "threshold": THRESHOLD["resign_threshold"], "disable": THRESHOLD["resign_disable_fraction"]})
        assert_selfplay_equal(r, o, gid)
        moves += o["num_moves"]
        evals += o["evals"]
        ends.add("resign" if r["was_resign"] else "score")
    assert ct["positions"] == moves and ct["evals"] == evals
    if games >= 12:
        assert ends == {"resign", "score"}, ends          # the parity set ends both ways
    net.close()


def test_game_to_start_follows_the_index_rule():
    """the first recorded move of game gid is legal on entry gid mod S and the record's length ends at that entry's
    n + num_moves <= max_game_length; a table of ONE entry gives every game that start"""
    N, R, seed = 5, 16, 4
    net = OracleNet(N, 1, seed=0)
    starts = starts_5x5()
    recs, _ = run_sim(N, net, R, seed, 8, 4, starts[3:4], **THRESHOLD)
    for r in recs:
        o = tw.twin_selfplay(N, net.cb, R, seed, int(r["game_id"]), starts[3], -0.9, 0.0)
        assert_selfplay_equal(r, o, r["game_id"])
        assert starts[3].n + r["num_moves"] <= tw.max_game_length(N)
    # with base / stride (a rank of a multi-GPU run) the index is still the GLOBAL id mod S
    sim = hs.Sim(board_size=N, games=2, num_readouts=R, seed=seed, game_id_base=3, game_id_stride=4,
                 record_capacity_games=16, **THRESHOLD)
    sim.set_starts(starts)
    sim.start(5)
    while sim.counters()["finished"] < 5:
        sim.step(net.on_feats)
    recs = sim.records()
    sim.close()
    assert [int(r["game_id"]) for r in recs] == [3, 7, 11, 15, 19]
    for r in recs:
        gid = int(r["game_id"])
        assert_selfplay_equal(r, tw.twin_selfplay(N, net.cb, R, seed, gid, starts[gid % 6], -0.9, 0.0), gid)
    net.close()


def test_the_slot_count_is_invisible():
    N, R, seed, games = 5, 16, 6, 7
    net = OracleNet(N, 1, seed=0)
    starts = starts_5x5()
    a, _ = run_sim(N, net, R, seed, games, 2, starts, **THRESHOLD)
    b, _ = run_sim(N, net, R, seed, games, 5, starts, **THRESHOLD)
    assert len(a) == len(b) == games
    for x, y in zip(a, b):
        assert x["game_id"] == y["game_id"] and x["num_moves"] == y["num_moves"] and x["result"] == y["result"]
        assert (x["moves"] == y["moves"]).all() and bits_equal(x["pis"], y["pis"]) and bits_equal(x["qs"], y["qs"])
        assert np.float32(x["final_score"]) == np.float32(y["final_score"])
    net.close()


def test_setup_and_ko_starts():
    """a handicap-style set-up (n = 0, White to move, no history, komi 0.5) and a start with the ko point set"""
    N, R, seed = 5, 16, 7
    net = OracleNet(N, 1, seed=0)
    starts = [tw.setup_start(N), tw.ko_start(N)]
    recs, _ = run_sim(N, net, R, seed, 4, 2, starts, **THRESHOLD)
    for r in recs:
        gid = int(r["game_id"])
        assert_selfplay_equal(r, tw.twin_selfplay(N, net.cb, R, seed, gid, starts[gid % 2], -0.9, 0.0), gid)
    net.close()


def test_a_start_beyond_tau_is_argmax_from_its_first_move():
    """9x9: tau_threshold = 6; the start of 12 plies picks by arg-max, so its recorded pi's are the sharpened ones
    (children_as_pi(squash) only while n <= tau) -- implied by twin parity, asserted here on the twin's own rows"""
    N, R, seed = 9, 16, 8
    net = OracleNet(N, 1, seed=0)
    start = tw.random_start(N, 12, 77)
    recs, _ = run_sim(N, net, R, seed, 1, 1, [start], resign_threshold=-2.0, resign_disable_fraction=0.0)
    o = tw.twin_selfplay(N, net.cb, R, seed, 0, start, -2.0, 0.0)
    assert_selfplay_equal(recs[0], o, 0)
    assert start.n >= (N * N // 12) // 2 * 2 and o["num_moves"] > 0
    for k in range(o["num_moves"]):          # unsquashed: pi = child_N / sum, so its smallest positive entry is k / R'
        assert np.isclose(o["pis"][k].sum(), 1.0, atol=1e-5)
    net.close()


# ---------------------------------------------------------------- the arena from a table

@pytest.mark.parametrize("games,slots", [(12, 4), (4, 6)])
def test_arena_from_a_table_equals_the_twin(games, slots):
    N, R, seed = 5, 16, 1
    black, white = OracleNet(N, 1, seed=0), OracleNet(N, 1, seed=5)
    starts = starts_5x5() + [tw.setup_start(N)]
    recs, ct = run_sim(N, black, R, seed, games, slots, starts, arena=True, white=white)
    assert len(recs) == games and ct["pool_exhausted"] == 0
    assert sorted(int(r["game_id"]) // 2 for r in recs) == list(range(games))
    evals = 0
    first_movers = set()
    for r in recs:
        g = int(r["game_id"]) // 2
        start = starts[g % len(starts)]
        o = tw.twin_arena(N, black.cb, white.cb, R, -0.9, seed, g, start)
        assert_arena_equal(r, o, g)
        evals += o["evals_black"] + o["evals_white"]
        first_movers.add(start.to_play)
    assert ct["evals"] == evals
    assert first_movers == {1, -1}
    black.close()
    white.close()


# ---------------------------------------------------------------- no table: today's engine

def test_without_a_table_the_records_are_todays():
    N, R, seed, games = 5, 16, 2, 5
    net = OracleNet(N, 1, seed=0)
    want, wct, _ = run_engine(N, net, R, seed, games, 3)
    for starts in ([], None):
        if starts is None:          # a table set and cleared again
            sim = hs.Sim(board_size=N, games=3, num_readouts=R, seed=seed, record_capacity_games=games + 8)
            sim.set_starts(starts_5x5())
            assert sim.L.hs_starts_count(sim.h) == 6
            sim.set_starts([])
            assert sim.L.hs_starts_count(sim.h) == 0
            sim.start(games)
            while sim.counters()["finished"] < games:
                sim.step(net.on_feats)
            got, gct = sim.records(), sim.counters()
            sim.close()
        else:
            got, gct = run_sim(N, net, R, seed, games, 3, starts)
        assert len(got) == games
        assert_records_identical(got, want)
        assert gct == wct
    net.close()


def test_the_empty_board_is_the_one_entry_table_of_the_empty_position():
    """what lets game_start make one root_install call: no table and a table of the empty position alone are one run"""
    for N, R, seed, games, slots in ((5, 16, 2, 5, 3), (9, 16, 4, 2, 2)):
        net = OracleNet(N, 1, seed=0)
        want, wct, _ = run_engine(N, net, R, seed, games, slots)
        got, gct = run_sim(N, net, R, seed, games, slots, [tw.random_start(N, 0, 0)])
        net.close()
        assert len(want) == games
        assert_records_identical(got, want)
        assert gct == wct


def test_board_check_of_the_table():
    """root_board_valid, the check k_starts_valid runs over a table: a point outside {-1, 0, 1}, a group without a
    liberty, a stone on the ko point"""
    sim = hs.Sim(board_size=5, games=1, num_readouts=4)
    good = tw.ko_start(5)
    assert sim.board_valid(good.board_np(), good.ko)
    b = good.board_np()
    b[int(np.flatnonzero(b == 0)[0])] = 2
    assert not sim.board_valid(b, -1)
    b = np.zeros(25, np.int8)
    b[0], b[1], b[5] = -1, 1, 1                     # the corner stone has no liberty
    assert not sim.board_valid(b, -1)
    b = good.board_np()
    stone = int(np.flatnonzero(b != 0)[0])
    assert not sim.board_valid(b, stone)
    sim.close()


# ---------------------------------------------------------------- the ABI

def test_header_declares_the_new_calls_and_keeps_the_abi():
    hdr = open(os.path.join(ROOT, "include", "agz.h")).read()
    assert re.search(r"#define AGZ_VERSION 103\b", hdr)
    for name in ("agz_selfplay_set_starts", "agz_selfplay_starts_count", "agz_replay_features_starts"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert C.sizeof(ag._lib.Config) == 112 and C.sizeof(ag._lib.GameHeader) == 32
    lib = ag.load()
    assert lib.agz_version() == 103
    for name in ("agz_selfplay_set_starts", "agz_selfplay_starts_count", "agz_replay_features_starts"):
        assert name in lib._agz_signatures and hasattr(lib, name)
    sz = (C.c_int32 * 64)()
    assert lib.agz_abi_layout(b"agz_config", sz, 64) > 0 and sz[0] == 112
    for who in ("selfplay", "evaluate", "train"):
        assert "starts" in inspect.signature(getattr(ag, who)).parameters, who
