"""The analysis and review driver of agz_search.h (analysis_pre / analysis_finish / review_claim / review_next_ply /
review_play under the host wave simulator) against the player loop on the single-tree ops of a second simulator:
per game TOP_INIT on its start with draw key (seed, game_id_base + j), per ply TOP_SEARCH_SELECT / TOP_SEARCH_POST until
N(root) >= N0 + R, then TOP_PICK, then TOP_PLAY of the recorded move.  Every row must be the loop's bit for bit, which
runs play_move through two of its callers (review_play, TOP_PLAY) in one assertion.  tests/test_gpu_review.py::
test_internal_network_matches_mcts_player on the CPU; the pool recovery of review_play stays with
test_small_pool_moves_early_and_the_game_goes_on there (a full pool changes the search).  CPU only."""
import numpy as np
import pytest

import alphago_jl_amd as ag
import hs
import orc
from selfplay_twin import opos_arrays, random_start
from test_hostsim_selfplay import OracleNet, bits_equal

N, R, PAR, SEED, BASE = 5, 16, 8, 7, 300
P, A = N * N, N * N + 1
OK, BAD_ARGUMENT, SOFTPICK = ag._lib.OK, ag._lib.BAD_ARGUMENT, orc.ASSERT_SOFTPICK
FIELDS = ("move", "status", "N", "W", "Q", "nodes_used", "child_N", "child_W", "prior")


@pytest.fixture(scope="module")
def net():
    n = OracleNet(N, 1, seed=0)
    yield n
    n.close()


def random_game(start, nmoves, seed, pass_at=()):
    """nmoves seeded random legal moves from `start` (flat actions), a pass at the plies of pass_at"""
    rng = np.random.RandomState(seed)
    pos, out = start, []
    for k in range(nmoves):
        cand = np.flatnonzero(orc.legal_moves(pos)[:P])
        a = P if k in pass_at or len(cand) == 0 else int(rng.choice(cand))
        rc, pos = orc.play(pos, a)
        assert rc == orc.OK
        out.append(a)
    return out


def run(net_fn, positions, games, slots, two_player, max_steps=2000):
    """the batched run on `slots` slots: (rows finished, rows)"""
    sim = hs.Sim(board_size=N, games=slots, num_readouts=R, parallel_readouts=PAR, seed=SEED, two_player_mode=two_player)
    sim.analysis_start(positions, games, game_id_base=BASE)
    for _ in range(max_steps):
        if sim.analysis_results()[0] >= sim.an_rows:
            break
        sim.step(net_fn)
    out = sim.analysis_results()
    assert all(sim.game(g).phase in (0, 5) for g in range(slots))       # G_IDLE or G_RETIRED: nothing left searching
    sim.close()
    return out


def player_rows(net_fn, arrays, j, moves, two_player, plies=None):
    """the rows of the player loop over game j: one per ply, `plies` of them (all by default; 1 with no moves is
    suggest_move alone)"""
    boards, infos, hist = arrays
    sim = hs.Sim(board_size=N, games=1, num_readouts=R, parallel_readouts=PAR, seed=SEED, two_player_mode=two_player)
    st, _ = sim.op(hs.TOP_INIT, board=boards[j], info=hs.PositionInfo.from_buffer_copy(infos[j]),
                   history=hist[j][: infos[j].history_len] if infos[j].history_len else None)
    assert st == OK
    sim.L.hs_game_set(sim.h, 0, 0, float(BASE + j))
    rows = []
    for k in range(len(moves) if plies is None else plies):
        target = np.float32(sim.game(0).rootN) + np.float32(R)
        while np.float32(sim.game(0).rootN) < target:
            st, ns = sim.op(hs.TOP_SEARCH_SELECT, par=PAR)
            assert st == OK
            if ns:
                feats = np.zeros((ns, 17 * P), np.float32)
                sim.L.hs_tree_leaf_features(sim.h, 0, hs.pf(feats))
                pi, v = net_fn(feats)
                sim.L.hs_set_batch_outputs(sim.h, hs.pf(np.ascontiguousarray(pi, np.float32)),
                                           hs.pf(np.ascontiguousarray(v, np.float32)), ns)
                assert sim.op(hs.TOP_SEARCH_POST)[0] == OK
        st, a = sim.op(hs.TOP_PICK)
        assert st in (OK, SOFTPICK)                      # the soft pick's assertion is a row too
        G, root = sim.game(0), sim.game(0).root
        rows.append(dict(move=a if st == OK else -1, status=st, N=np.float32(G.rootN), W=np.float32(G.rootW),
                         Q=np.float32(G.rootW) / (np.float32(1) + np.float32(G.rootN)), nodes_used=G.nodes_used,
                         child_N=sim.row(0, root, 0).copy(), child_W=sim.row(0, root, 1).copy(),
                         prior=sim.row(0, root, 2).copy()))
        if k < len(moves):
            assert sim.op(hs.TOP_PLAY, a=moves[k]) == (OK, 1)
    sim.close()
    return rows


def assert_row(r, i, o, what):
    for f in FIELDS:
        if f in ("move", "status", "nodes_used"):
            assert int(r[f][i]) == int(o[f]), (what, f, int(r[f][i]), int(o[f]))
        else:
            assert bits_equal(r[f][i], o[f]), (what, f)


def unsearched(status):
    z = np.zeros(A, np.float32)
    return dict(move=-1, status=status, N=0.0, W=0.0, Q=0.0, nodes_used=0, child_N=z, child_W=z, prior=z)


def offsets(games):
    return np.concatenate([[0], np.cumsum([len(g) for g in games])]).astype(np.int64)


@pytest.mark.parametrize("two_player", [0, 1])
def test_review_equals_the_player_loop(net, two_player):
    mid = random_start(N, 9, 41, komi=5.5)               # a mid-game start: history, captures state, its own komi
    assert mid.ndeltas > 0
    starts = [orc.make_pos(N), mid, orc.make_pos(N, komi=6.5)]
    games = [random_game(starts[0], 6, 11, pass_at=(3,)), random_game(mid, 7, 12), []]
    assert P in games[0] and [len(g) for g in games] == [6, 7, 0]
    arrays = opos_arrays(starts)
    done, r = run(net.on_feats, arrays, games, slots=2, two_player=two_player)    # 2 slots: one takes a second game
    off = offsets(games)
    assert done == off[-1] == 13 and len(r["move"]) == 13                 # the empty game has no rows
    inherited = False
    for j, g in enumerate(games):
        rows = player_rows(net.on_feats, arrays, j, g, two_player)
        for k, o in enumerate(rows):
            assert_row(r, off[j] + k, o, f"game {j} ply {k}")
            if k:
                inherited |= bool(r["N"][off[j] + k] > R)                 # the re-rooted tree kept the child's visits
    assert inherited, "no ply searched a reused tree"
    assert (r["status"] == OK).sum() >= 11


def test_analysis_equals_the_first_ply_of_the_loop(net):
    positions = [orc.make_pos(N), random_start(N, 5, 21), random_start(N, 8, 22, komi=5.5), random_start(N, 12, 23),
                 random_start(N, 3, 24)]
    boards, infos, hist = opos_arrays(positions)
    bad = 2
    boards[bad][:] = 0
    boards[bad][0] = 1                                   # a black stone in the corner with both liberties white:
    boards[bad][1] = boards[bad][N] = -1                 # a group without a liberty is no position
    arrays = (boards, infos, hist)
    done, r = run(net.on_feats, arrays, None, slots=2, two_player=1)
    assert done == 5 and len(r["move"]) == 5
    for i in range(5):
        o = unsearched(BAD_ARGUMENT) if i == bad else player_rows(net.on_feats, arrays, i, [], 1, plies=1)[0]
        assert_row(r, i, o, f"position {i}")
        assert i == bad or (o["status"] == OK and o["N"] >= R)


def test_an_unplayable_recorded_move_gives_up_the_rest_of_its_game(net):
    starts = [orc.make_pos(N), orc.make_pos(N), random_start(N, 6, 31)]
    bad_game = [12, 6, 12, 7, 8]                         # ply 2 plays on the stone of ply 0
    games = [random_game(starts[0], 5, 51), bad_game, random_game(starts[2], 4, 52)]
    arrays = opos_arrays(starts)
    done, r = run(net.on_feats, arrays, games, slots=2, two_player=1)
    off = offsets(games)
    assert done == off[-1] == 14                          # the progress counter reaches the total
    for j, g in enumerate(games):
        rows = player_rows(net.on_feats, arrays, j, g[:2] if j == 1 else g, 1)
        rows += [unsearched(BAD_ARGUMENT)] * (len(g) - len(rows))
        for k, o in enumerate(rows):
            assert_row(r, off[j] + k, o, f"game {j} ply {k}")
    assert list(r["status"][off[1]: off[2]]) == [OK, OK] + [BAD_ARGUMENT] * 3
    assert list(r["move"][off[1] + 2: off[2]]) == [-1] * 3
