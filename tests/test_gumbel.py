"""The Gumbel root search (agz_selfplay_set_gumbel) on the host simulator: Gumbel-top-k candidates at the
root of a full self-play search, Sequential Halving over them, the survivor with the largest s(a) as the move and
softmax(logit + sigma(q)) as the recorded row.  tests/selfplay_twin.py restates all of it over the oracle's primitives.
Here: off is the cap simulator byte for byte, the schedules, the worked row, hand rows for the root pick, whole games
against the twin bit for bit, and the properties of the rows.  CPU only."""
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
from test_hostsim_selfplay import OracleNet, bits_equal
from test_playout_cap import run_cap_sim

L = orc.lib()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = (8, 0.5)
THR = -0.1


def run_gumbel_sim(N, net, R, cap, m, seed, games, slots, starts=None, reset=False, c_visit=50.0, c_scale=1.0,
                   max_steps=400000, **cfg):
    sim = hs.Sim(board_size=N, games=slots, num_readouts=R, seed=seed, game_id_base=0, game_id_stride=1,
                 record_capacity_games=games + 8, **cfg)
    if starts:
        sim.set_starts(starts)
    if cap:
        sim.set_playout_cap(*cap)
    if m is not None:
        sim.set_gumbel(m, c_visit, c_scale)
    if reset:
        sim.set_gumbel(0)
    sim.start(games)
    steps = 0
    while sim.counters()["finished"] < games and steps < max_steps:
        sim.step(net.on_feats)
        steps += 1
    out = sim.records(), sim.counters(), sim.all_counters(), sim.gumbel_counts()
    sim.close()
    return out


# ---------------------------------------------------------------- (a) off is the cap simulator, byte for byte

@pytest.mark.parametrize("cap", [None, CAP])
def test_off_and_reset_are_the_cap_twin_and_simulator(cap):
    N, R, seed, games, slots = 5, 16, 3, 4, 3
    net = OracleNet(N, 1, seed=0)
    starts = tw.random_starts(N, (4, 7, 1), seed=0)
    kw = dict(resign_threshold=THR, resign_disable_fraction=0.0)
    r, p = cap if cap else (0, 1.0)
    want, wct, wcaps = run_cap_sim(N, net, R, r, p, seed, games, slots, starts=starts, **kw)
    ran = [run_gumbel_sim(N, net, R, cap, None, seed, games, slots, starts=starts, **kw),
           run_gumbel_sim(N, net, R, cap, 0, seed, games, slots, starts=starts, **kw),
           run_gumbel_sim(N, net, R, cap, 16, seed, games, slots, starts=starts, reset=True, **kw)]
    for got, gct, allc, gc in ran:
        assert len(got) == len(want) == games
        for x, y in zip(got, want):
            assert sorted(x) == sorted(y)
            for key in x:
                a, b = np.asarray(x[key]), np.asarray(y[key])
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
        assert gct == wct
        assert (allc["CT_CAP_FULL"], allc["CT_CAP_FAST"]) == wcaps
        assert allc == ran[0][2] and gc == (0, 0)
    for rec in want:                                    # ... and the cap twin's
        gid = int(rec["game_id"])
        o = tw.twin_selfplay(N, net.cb, R, seed, gid, starts[gid % 3], THR, 0.0, cap=(r if cap else 4, p))
        assert (rec["moves"] == o["moves"]).all() and bits_equal(rec["qs"], o["qs"])
        assert bits_equal(np.ascontiguousarray(rec["pis"], np.float32).reshape(-1, N * N + 1), o["pis"])
    net.close()


# ---------------------------------------------------------------- (b) the schedules

SCHEDULES = [
    (32, 16, [(16, 16), (8, 8), (4, 8)]),
    (32, 4, [(4, 16), (2, 16)]),
    (32, 5, [(5, 10), (2, 10), (2, 10), (2, 2)]),
    (400, 16, [(16, 96), (8, 96), (4, 100), (2, 100), (2, 8)]),
]


@pytest.mark.parametrize("n,m0,want", SCHEDULES)
def test_schedules(n, m0, want):
    sim = hs.Sim(board_size=5, games=1, num_readouts=8, seed=1)
    assert sim.schedule(n, m0) == want == tw.schedule(n, m0)
    assert sum(q for _, q in want) == n
    sim.close()


def test_schedule_of_one_candidate_and_small_budgets():
    sim = hs.Sim(board_size=5, games=1, num_readouts=8, seed=1)
    assert sim.schedule(16, 1) == [(1, 16)] == tw.schedule(16, 1)
    for n in (1, 2, 3, 7, 16, 33):
        for m0 in range(1, 17):
            s = sim.schedule(n, m0)
            assert s == tw.schedule(n, m0) and sum(q for _, q in s) == n
    sim.close()


@pytest.mark.parametrize("R,m", [(32, 16), (32, 4), (32, 5)])
def test_schedule_of_a_running_search(R, m):
    """the phase ends and survivor counts the slot's state goes through in the first search of a game"""
    N = 5
    net = OracleNet(N, 1, seed=0)
    sim = hs.Sim(board_size=N, games=1, num_readouts=R, seed=4, resign_threshold=-2.0, resign_disable_fraction=0.0)
    sim.set_gumbel(m)
    sim.start(1)
    seen = []
    for _ in range(200):
        sim.step(net.on_feats)
        st = sim.gumbel_state(0)
        if st.n == 0 and (st.cnt, st.end) not in seen:
            seen.append((st.cnt, st.end))
        if st.n > 0:
            break
    want, end = [], 1.0                                  # the pre-expansion is the root's first visit
    for mp, q in tw.schedule(R, m):
        end += q
        want.append((mp, end))
    assert seen == want
    assert sim.gumbel_counts()[1] >= len(want) - 1
    sim.close()
    net.close()


# ---------------------------------------------------------------- (c) the worked row

EX_N = [60, 20, 12, 1, 6, 0]
EX_P = [0.50, 0.20, 0.10, 0.05, 0.10, 0.05]
EX_W = [30.5, 0, 6.25, 0, 3.5, 0.45]
EX_X = [7.556853, 3.890562, 5.841646, 2.504268, 5.947415, 4.979268]
EX_PI = [0.672112, 0.017187, 0.120931, 0.004297, 0.134422, 0.051052]
EX_PI_MINUS = [0.106663, 0.667399, 0.023713, 0.166850, 0.021333, 0.014043]


def example_tree(rows=(EX_N, EX_W, EX_P), at=(0, 1, 2, 3, 4, 5), to_play=1, board=None, last_move=-1, N=5, sim=None):
    """a single tree on the simulator whose expanded root has the given child rows at actions `at`, zero elsewhere"""
    sim = sim or hs.Sim(board_size=N, games=1, num_readouts=8, seed=1, c_puct=1.0)
    b = np.zeros(N * N, np.int8) if board is None else board
    root = sim.tree_init(0, b, n=sim.tau + 1, to_play=to_play, last_move=last_move)
    st, leaf = sim.op(hs.TOP_SELECT, node=root)
    assert st == 0 and leaf == root
    st, _ = sim.op(hs.TOP_INCORPORATE, node=root, up_to=root, probs=np.full(sim.A, 1.0 / sim.A, np.float32), value=0.0)
    assert st == 0
    for field, vals in enumerate(rows):
        row = sim.row(0, root, field)
        row[:] = 0
        row[list(at)] = np.asarray(vals, np.float32)
    return sim, root


def rows_of(sim, root):
    return [sim.row(0, root, f).copy() for f in range(3)]


def legal_of(sim, root):
    return np.asarray(sim.legal(0, root), np.int8)


@pytest.mark.parametrize("at", [(0, 1, 2, 3, 4, 5), (3, 7, 2, 9, 24, 25)])
def test_worked_row(at):
    sim, root = example_tree(at=at)
    at = list(at)
    got = sim.gumbel_pi(0, root, 50.0, 0.1)
    want, x = tw.gumbel_pi(*rows_of(sim, root), legal_of(sim, root), 1, 50.0, 0.1)
    assert bits_equal(got, want)
    assert np.abs(x[at] - EX_X).max() < 1e-6
    assert np.abs(got[at].astype(np.float64) - EX_PI).max() < 1e-6
    rest = np.setdiff1d(np.arange(sim.A), at)
    assert (got[rest] == 0).all()                       # legal, P = 0: logit -1e30, no mass
    assert abs(float(got.astype(np.float64).sum()) - 1.0) < 1e-6
    # c_scale = 1.0
    got1 = sim.gumbel_pi(0, root, 50.0, 1.0)
    want1, _ = tw.gumbel_pi(*rows_of(sim, root), legal_of(sim, root), 1, 50.0, 1.0)
    assert bits_equal(got1, want1)
    assert abs(float(got1[at[0]]) - 0.783795) < 1e-6 and abs(float(got1[at[5]]) - 0.00501063) < 1e-6
    sim.close()


def test_worked_row_white_to_play():
    sim, root = example_tree(to_play=-1)
    got = sim.gumbel_pi(0, root, 50.0, 0.1)
    want, _ = tw.gumbel_pi(*rows_of(sim, root), legal_of(sim, root), -1, 50.0, 0.1)
    assert bits_equal(got, want)
    assert np.abs(got[:6].astype(np.float64) - EX_PI_MINUS).max() < 1e-6
    sim.close()


def test_worked_row_illegal_action_and_zero_prior():
    board = np.zeros(25, np.int8)
    board[2] = 1                                         # a2 is occupied: illegal
    sim, root = example_tree(board=board)
    lg = legal_of(sim, root)
    assert lg[2] == 0 and lg[[0, 1, 3, 4, 5]].all()
    got = sim.gumbel_pi(0, root, 50.0, 0.1)
    want, _ = tw.gumbel_pi(*rows_of(sim, root), lg, 1, 50.0, 0.1)
    assert bits_equal(got, want) and got[2] == 0.0
    keep = [0, 1, 3, 4, 5]
    renorm = np.array(EX_PI)[keep] / np.array(EX_PI)[keep].sum()
    assert np.abs(got[keep].astype(np.float64) - renorm).max() < 2e-6
    sim.close()
    # P = 0 on a legal action with visits and value: no mass, the rest renormalised
    P0 = list(EX_P)
    P0[1] = 0.0
    sim, root = example_tree(rows=(EX_N, EX_W, P0))
    got = sim.gumbel_pi(0, root, 50.0, 0.1)
    want, _ = tw.gumbel_pi(*rows_of(sim, root), legal_of(sim, root), 1, 50.0, 0.1)
    assert bits_equal(got, want) and got[1] == 0.0
    keep = [0, 2, 3, 4, 5]
    renorm = np.array(EX_PI)[keep] / np.array(EX_PI)[keep].sum()
    assert np.abs(got[keep].astype(np.float64) - renorm).max() < 2e-6
    sim.close()


# ---------------------------------------------------------------- (d) hand rows for the root pick

def root_action_of(sim, root, leaf):
    a = np.flatnonzero(sim.children(0, root) == leaf)
    assert len(a) == 1
    return int(a[0])


def test_root_pick_least_visited_survivor():
    sim, root = example_tree()
    before = sim.gumbel_counts()
    sel = sim.game(0).sel
    assert root_action_of(sim, root, sim.gumbel_descend(0, [0, 1, 2, 4])) == 4        # N = 60, 20, 12, 6
    assert sim.row(0, root, 0)[4] == 7.0 and sim.game(0).sel == sel + 1
    assert root_action_of(sim, root, sim.gumbel_descend(0, [0, 3, 2])) == 3           # N = 60, 1, 12
    assert root_action_of(sim, root, sim.gumbel_descend(0, [0])) == 0                 # a lone survivor
    assert root_action_of(sim, root, sim.gumbel_descend(0, [1, 5])) == 5              # an unvisited survivor
    assert sim.gumbel_counts() == before
    sim.close()


def test_root_pick_ties_go_to_the_first_stored():
    Nv = [5, 3, 3, 3, 9, 3]
    for order, want in (([0, 2, 1, 3], 2), ([3, 5, 1], 3), ([4, 1, 2], 1)):
        sim, root = example_tree(rows=(Nv, EX_W, EX_P))
        assert root_action_of(sim, root, sim.gumbel_descend(0, order)) == want
        # the visit in flight counts: the next descent goes to the next of the tie
        nxt = [a for a in order if Nv[a] == 3 and a != want]
        if nxt:
            assert root_action_of(sim, root, sim.gumbel_descend(0, order)) == nxt[0]
        sim.close()


def test_root_pick_pass_hack_keeps_its_precedence():
    P = 25
    sim, root = example_tree(last_move=P)
    assert sim.row(0, root, 0)[P] == 0.0
    assert root_action_of(sim, root, sim.gumbel_descend(0, [0, 1, 4])) == P           # mcts.jl:119-126 first
    assert root_action_of(sim, root, sim.gumbel_descend(0, [0, 1, 4])) == 4           # the pass has a visit now
    sim.close()


def test_below_the_root_is_puct():
    sim, root = example_tree()
    child = sim.gumbel_descend(0, [3])
    assert root_action_of(sim, root, child) == 3
    st, _ = sim.op(hs.TOP_INCORPORATE, node=child, up_to=root, probs=np.full(sim.A, 1.0 / sim.A, np.float32), value=0.0)
    assert st == 0
    FN, FP, FW = [60, 20, 12, 1, 6], [0.50, 0.20, 0.10, 0.05, 0.15], [30.5, 0, 6.25, 0, 3.5]
    for field, vals in enumerate((FN, FW, FP)):
        row = sim.row(0, child, field)
        row[:] = 0
        row[:5] = np.asarray(vals, np.float32)
    sim.row(0, root, 0)[3] = 98.0                                  # the child's own N: 99 with the visit, scale 10
    leaf = sim.gumbel_descend(0, [3])
    pick = int(np.flatnonzero(sim.children(0, child) == leaf)[0])
    Nc, Wc, Pc = [sim.row(0, child, f).copy() for f in range(3)]
    Nc[pick] -= 1                                                  # the rows the descent saw
    score, _, scale = tw.action_scores(Nc, Wc, Pc, sim.meta(0, child).to_play, 99.0, 1.0)
    lg = sim.legal(0, child) != 0
    assert not lg[3] and scale == 10.0
    best = np.flatnonzero(lg & (score == score[lg].max()))
    assert len(best) == 1 and pick == int(best[0]) and Nc[pick] > 0     # the PUCT arg-max, not the least visited
    sim.close()


# ---------------------------------------------------------------- (e) whole games against the twin

# N, R, m, cap, seed, games, slots: seeds and starts chosen so that the twin alone meets the conditions asserted below
GAME_SETS = [
    (5, 32, 4, None, 3, 3, 2),
    (5, 32, 16, CAP, 3, 4, 3),
    (9, 32, 16, None, 9, 2, 2),
    (9, 32, 4, CAP, 10, 2, 2),
]
_games = {}


def set_starts_of(N):
    return tw.random_starts(N, (4, 7, 1), seed=0)


def game_set(i):
    """(records of the simulator, twins, counters, all counters, gumbel counts) of GAME_SETS[i], computed once"""
    if i not in _games:
        N, R, m, cap, seed, games, slots = GAME_SETS[i]
        net = OracleNet(N, 1, seed=0)
        starts = set_starts_of(N)
        recs, cnt, allc, gc = run_gumbel_sim(N, net, R, cap, m, seed, games, slots, starts=starts,
                                             resign_threshold=THR, resign_disable_fraction=0.0)
        r, p = cap if cap else (0, 1.0)
        twins = [tw.twin_selfplay(N, net.cb, R, seed, int(rec["game_id"]), starts[int(rec["game_id"]) % len(starts)], THR,
                                  0.0, cap=(r, p), gumbel=(m, 50.0, 1.0)) for rec in recs]
        net.close()
        _games[i] = (recs, twins, cnt, allc, gc)
    return _games[i]


def assert_set_conditions(twins):
    """what the inputs of a set guarantee, on the twin alone"""
    for o in twins:
        for n, q0, halvings in o["halvings_per_search"]:
            assert n <= q0 or halvings >= 1, "a full search with n > Q_0 has no halving"
    assert sum(o["begun"] for o in twins) >= 1
    assert sum(o["reused"] for o in twins) >= 1, "no search begins at a reused root"
    assert sum(o["off_max"] for o in twins) >= 1, "every move is the most visited child"
    assert sum(o["dups"] for o in twins) >= 1, "no duplicate is reverted inside a Gumbel search"
    assert sum(o["cuts"] for o in twins) >= 1, "no select phase is cut short at a phase end"


@pytest.mark.parametrize("i", range(len(GAME_SETS)))
def test_sim_games_equal_the_twin(i):
    N, R, m, cap, seed, games, slots = GAME_SETS[i]
    recs, twins, cnt, allc, gc = game_set(i)
    assert len(recs) == games and cnt["pool_exhausted"] == 0
    assert_set_conditions(twins)
    for rec, o in zip(recs, twins):
        gid = int(rec["game_id"])
        assert rec["num_moves"] == o["num_moves"] and (rec["moves"] == o["moves"]).all(), gid
        assert rec["result"] == o["result"] and rec["was_resign"] == o["was_resign"], gid
        assert np.float32(rec["final_score"]) == np.float32(o["final_score"]), gid
        assert bits_equal(rec["qs"], o["qs"]), gid
        full = o["full"]
        got = np.ascontiguousarray(rec["pis"], np.float32).reshape(-1, N * N + 1)
        assert (got[~full].view(np.uint32) == 0).all(), (gid, "a fast row is not all zero")
        assert bits_equal(got[full], o["pis"][full]), gid
        assert rec["short_searches"] == 0
    assert cnt["evals"] == sum(o["evals"] for o in twins)
    assert cnt["positions"] == sum(o["num_moves"] for o in twins)
    assert gc == (sum(o["begun"] for o in twins), sum(o["halved"] for o in twins))
    if cap:
        assert allc["CT_CAP_FULL"] == sum(int(o["full"].sum()) for o in twins)
        assert allc["CT_CAP_FAST"] == sum(int((~o["full"]).sum()) for o in twins)
        assert any((~o["full"]).any() for o in twins) and any(o["full"].any() for o in twins)
    assert allc["CT_FORCED_SEL"] == 0 and allc["CT_PRUNED_ROWS"] == 0


# ---------------------------------------------------------------- (f) the rows

@pytest.mark.parametrize("i", range(len(GAME_SETS)))
def test_row_properties(i):
    N = GAME_SETS[i][0]
    A = N * N + 1
    recs, twins, _, _, _ = game_set(i)
    legal = np.zeros(A, np.int8)
    nrows = 0
    for rec, o in zip(recs, twins):
        full = o["full"]
        got = np.ascontiguousarray(rec["pis"], np.float32).reshape(len(full), A)
        assert (got[~full] == 0).all(), "a fast row is not all zero"
        for k in np.flatnonzero(full):
            L.or_all_legal_moves(C.byref(o["positions"][k]), legal.ctypes.data_as(C.POINTER(C.c_int8)))
            row = got[k]
            assert abs(float(row.astype(np.float64).sum()) - 1.0) < 1e-6
            assert (row[legal == 0] == 0).all(), "mass on an illegal action"
            nrows += 1
        # P > 0 on every legal action of these networks (a softmax): every legal entry of a full row is positive unless
        # its exponent underflows, which x - max x > -745 excludes here: |logit| < 40 and sigma in [0, 82]
        for k in np.flatnonzero(full):
            L.or_all_legal_moves(C.byref(o["positions"][k]), legal.ctypes.data_as(C.POINTER(C.c_int8)))
            assert (got[k][legal != 0] > 0).all(), "a legal action with P > 0 has no mass"
    assert nrows >= len(recs)


# ---------------------------------------------------------------- the ABI

NEW_CALLS = ("agz_selfplay_set_gumbel", "agz_selfplay_gumbel_counts", "agz_tree_gumbel_pi")


def test_header_declares_the_new_calls_and_keeps_the_abi():
    hdr = open(os.path.join(ROOT, "include", "agz.h")).read()
    assert re.search(r"#define AGZ_VERSION 103\b", hdr)
    for name in NEW_CALLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    draws = open(os.path.join(ROOT, "include", "agz_draws.h")).read()
    assert re.search(r"#define AGZ_SITE_GUMBEL 12u", draws) and re.search(r"#define AGZ_SITE_PLAYOUT_CAP 11u", draws)
    assert C.sizeof(ag._lib.Config) == 112 and C.sizeof(ag._lib.GameHeader) == 32 and C.sizeof(hs.GameState) == 112
    assert C.sizeof(hs.GumbelStateC) == 56
    lib = ag.load()
    assert lib.agz_version() == 103
    for name in NEW_CALLS:
        assert name in lib._agz_signatures and hasattr(lib, name)
    for who in ("selfplay", "train"):
        sig = inspect.signature(getattr(ag, who)).parameters
        assert sig["gumbel"].default is None and sig["gumbel_c_visit"].default == 50.0, who
        assert sig["gumbel_c_scale"].default == 1.0, who
    for m in ("set_gumbel", "gumbel_counts", "tree_gumbel_pi"):
        assert hasattr(ag.Engine, m), m
    from alphago_jl_amd.api import NodeView
    assert hasattr(NodeView, "gumbel_pi")
    jl = open(os.path.join(ROOT, "alphago.jl_amd", "julia", "AlphaGoMI.jl")).read()
    for name in NEW_CALLS:
        assert ":%s" % name in jl, name
    state = open(os.path.join(ROOT, "alphago.jl_amd", "csrc", "agz_state.h")).read()
    assert re.search(r"CT_GUMBEL_BEGUN = CT_COUNT, CT_GUMBEL_HALVED = CT_COUNT \+ 1;", state)
