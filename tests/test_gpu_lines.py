"""Analysis lines on the device (agz_analyze_set_lines / agz_analyze_lines / agz_tree_lines; analyze() / review() with
lines > 0; NodeView.lines / most_visited_path / mvp_gg): everything is compared exactly -- moves, lengths, the bits of
every float -- with the numpy walk of lines_twin.py over rows read through Engine.node_floats / node_children."""
import numpy as np
import pytest

import alphago_jl_amd as ag
import lines_twin
from test_gpu_analysis import api_positions, opos_arrays, run_analysis
from test_gpu_review import api_game
from test_hostsim_selfplay import bits_equal

import orc

pytestmark = pytest.mark.gpu
OK, BAD_ARGUMENT, POOL_EXHAUSTED, NOT_READY = ag._lib.OK, ag._lib.BAD_ARGUMENT, ag._lib.POOL_EXHAUSTED, ag._lib.NOT_READY
K, D = 4, 16
POLICY_SCALE = 30.0        # the policy FC weights x 30: a peaked policy, so that the searches go deep (see peaked_net)


def peaked_net(env, tower, seed, scale=POLICY_SCALE):
    """a synthetic network whose policy is peaked: the glorot policy FC weights scaled up (the value head is untouched).
    The synthetic towers feed the policy FC very small inputs, so x 10 leaves the policy flat (pi max 0.025 at 9x9 /
    tower 2, 0.0035 at 19x19 / tower 1, against 0.012 and 0.0028 uniform).  Measured on the MCTSPlayer twin of
    test_analyze_lines_equal_the_walk_over_mcts_player, rows with >= 2 lines and a first PV of >= 3 moves:
      9x9 / tower 2 / R 64, 10 positions: x 10: 5, x 30: 10 (pi max 0.07), x 100: 8, x 200: 7, x 400: 7 (one child takes
        nearly every visit);  19x19 / tower 1 / R 32, 5 positions: x 10: 0, x 30: 0, x 100: 4, x 200: 5 (pi max 0.10),
        x 400: 5.  Hence x 30 at 9x9 and x 200 at 19x19."""
    nn = ag.NeuralNet(env, tower_height=tower, seed=seed)
    w = nn.engine.get_weights(ag._lib.L_POLICY_FC, ag._lib.K_WEIGHT)
    nn.set_weights(ag._lib.L_POLICY_FC, ag._lib.K_WEIGHT, w * np.float32(scale))
    return nn


def player_walk(p, node, k=K, d=D, mv=1):
    """the twin's tables for `node` of MCTSPlayer p's tree"""
    e = p.engine
    return lines_twin.walk(lambda n, f: e.node_floats(0, n, f), lambda n: e.node_children(0, n), node, k, d, mv)


def as_lines(env, t):
    """the twin's tables as the list of Line analyze() / review() / NodeView.lines() must return"""
    out, one = [], np.float32(1)
    for k in range(len(t["move"])):
        n = int(t["pv_len"][k])
        if t["move"][k] < 0:
            assert n == 0
            continue
        out.append(ag.Line(ag.from_flat(int(t["move"][k]), env), t["N"][k], t["W"][k], t["W"][k] / (one + t["N"][k]),
                           t["prior"][k], [ag.from_flat(int(a), env) for a in t["pv"][k, :n]], t["pv_N"][k, :n],
                           t["end_W"][k] / (one + t["pv_N"][k, n - 1])))
    return out


def assert_lines_equal(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.move == b.move and a.pv == b.pv, (what, i, a.move, b.move, a.pv, b.pv)
        for f in ("N", "W", "Q", "prior", "pv_N", "end_Q"):
            assert bits_equal(np.asarray(getattr(a, f), np.float32), np.asarray(getattr(b, f), np.float32)), (what, i, f)


def assert_plain_rows_equal(a, b, what):
    assert a.move == b.move and a.status == b.status and a.game_id == b.game_id and a.nodes_used == b.nodes_used, what
    for f in ("N", "W", "Q", "child_N", "child_W", "child_Q", "prior"):
        assert bits_equal(getattr(a, f), getattr(b, f)), (what, f)


def suggest_twin(env, nn, pos, R, seed, game_id, **kw):
    p = ag.MCTSPlayer(env, nn, num_readouts=R, seed=seed, game_id=game_id, **kw)
    p.initialize_game(pos)
    p.suggest_move()
    t = player_walk(p, p.root.id)
    p.engine.close()
    return t


# ---------------------------------------------------------------- 4. / 5. analyze with lines

@pytest.mark.parametrize("N,tower,R,count,slots,scale", [(9, 2, 64, 10, 3, 30.0), (19, 1, 32, 5, 2, 200.0)])
def test_analyze_lines_equal_the_walk_over_mcts_player(N, tower, R, count, slots, scale):
    env = ag.GoEnv(N)
    nn = peaked_net(env, tower, 1, scale)
    positions = api_positions(env, 3, count, 3 * N)
    seed, base = 4, 100
    res = ag.analyze(env, nn, positions, num_readouts=R, seed=seed, game_id_base=base, slots=slots, lines=K, pv_depth=D)
    deep = 0
    for i, pos in enumerate(positions):
        t = suggest_twin(env, nn, pos, R, seed, base + i)
        print(f"{N}x{N} row {i}: twin lines {int((t['move'] >= 0).sum())}, pv_len {list(t['pv_len'])}")
        deep += int((t["move"] >= 0).sum() >= 2 and t["pv_len"][0] >= 3)
        assert isinstance(res[i], ag.AnalysisLines) and res[i].status == OK
        assert_lines_equal(res[i].lines, as_lines(env, t), (N, i))
    assert 10 * deep >= 9 * len(positions), (deep, len(positions))        # not a comparison of empty tables
    # 5. everything else in the rows is what the same run with lines off gives, and that one returns plain Analysis
    plain = ag.analyze(env, nn, positions, num_readouts=R, seed=seed, game_id_base=base, slots=slots)
    for i, (a, b) in enumerate(zip(res, plain)):
        assert type(b) is ag.Analysis and len(b) == 11
        assert_plain_rows_equal(ag.Analysis(*a[:11]), b, (N, i))


# ---------------------------------------------------------------- 6. independence of scheduling

def test_lines_do_not_depend_on_slots_or_splitting():
    N, R = 5, 32
    env = ag.GoEnv(N)
    nn = peaked_net(env, 1, 2)
    positions = api_positions(env, 8, 10, 12)
    B = len(positions)
    kw = dict(num_readouts=R, seed=1, lines=K, pv_depth=D, pv_min_visits=2)
    runs = [ag.analyze(env, nn, positions, game_id_base=50, slots=s, **kw) for s in (1, 3, 64)]
    half = B // 2
    split = (ag.analyze(env, nn, positions[:half], game_id_base=50, **kw)
             + ag.analyze(env, nn, positions[half:], game_id_base=50 + half, **kw))
    assert any(len(a.lines) >= 2 for a in runs[0])
    for other in runs[1:] + [split]:
        for i, (a, b) in enumerate(zip(runs[0], other)):
            assert_plain_rows_equal(ag.Analysis(*a[:11]), ag.Analysis(*b[:11]), i)
            assert_lines_equal(a.lines, b.lines, i)


# ---------------------------------------------------------------- 7. review with lines

def test_review_lines_equal_the_walk_before_the_recorded_move():
    N, tower, R = 9, 2, 32
    env = ag.GoEnv(N)
    nn = peaked_net(env, tower, 1)
    games = [api_game(env, 10 + j, 8) for j in range(3)]
    seed, base = 4, 100
    res = ag.review(env, nn, games, num_readouts=R, seed=seed, game_id_base=base, slots=2, lines=K, pv_depth=D)
    kept = 0
    for j, g in enumerate(games):
        p = ag.MCTSPlayer(env, nn, num_readouts=R, seed=seed, game_id=base + j, two_player_mode=True)
        p.initialize_game(None)
        assert len(res[j]) == len(g)
        for k, m in enumerate(g):
            n_before = p.root.N
            p.suggest_move()
            t = player_walk(p, p.root.id)                          # after the k-th suggest_move, before play_move(m_k)
            assert res[j][k].status == OK
            assert_lines_equal(res[j][k].lines, as_lines(env, t), (j, k))
            kept += int(k >= 1 and n_before > 0 and len(res[j][k].lines) > 0)
            assert p.play_move(m)
        p.engine.close()
    assert kept >= 1                                               # some compared row started from a kept subtree
    plain = ag.review(env, nn, games, num_readouts=R, seed=seed, game_id_base=base, slots=2)
    for ga, gb in zip(res, plain):
        for a, b in zip(ga, gb):
            assert type(b) is ag.Analysis
            assert_plain_rows_equal(ag.Analysis(*a[:11]), b, "review")


# ---------------------------------------------------------------- 8. rows that are not searched, short rows, readiness

def test_unsearched_rows_keep_unused_slots():
    N, R = 5, 16
    env = ag.GoEnv(N)
    nn = peaked_net(env, 1, 6)
    good = api_positions(env, 10, 2, 8)
    dead = np.zeros((N, N), np.int8)
    dead[0, 0], dead[0, 1], dead[1, 0] = 1, -1, -1                # a Black stone without a liberty
    positions = [good[0], ag.Position(env, board=dead, n=3), good[1]]
    res = ag.analyze(env, nn, positions, num_readouts=R, seed=3, slots=2, lines=K, pv_depth=D)
    assert res[1].status == BAD_ARGUMENT and res[1].lines == []
    assert res[0].lines and res[2].lines
    # the raw tables of such a row: move -1, pv_len 0, pv -1, floats +0
    eng = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=R, seed=3)
    nn.engine.copy_weights_to(eng)
    eng.analyze_set_lines(K, D, 1)
    boards, hist, infos = np.zeros((3, N * N), np.int8), np.zeros((3, 7, N * N), np.int8), []
    for k, pos in enumerate(positions):
        boards[k], f, h = ag.position_arrays(pos)
        hist[k, :len(h)] = h
        infos.append(f)
    run_analysis(eng, boards, infos, hist)
    t = eng.analyze_lines()
    assert (t["move"][1] == -1).all() and (t["pv_len"][1] == 0).all() and (t["pv"][1] == -1).all()
    for f in ("N", "W", "prior", "end_W", "pv_N"):
        assert not t[f][1].view(np.uint32).any(), f
    assert (t["move"][0] >= 0).any() and (t["pv"][0][t["move"][0] < 0] == -1).all()
    eng.close()
    # an invalid record from ply 2 on: rows 2.. of that game have no lines, the earlier ones and the other game do
    games = [[12, 7, 12, 13], [6, 18, 8]]
    rv = ag.review(env, nn, games, num_readouts=R, seed=3, slots=2, lines=K, pv_depth=D)
    assert [r.status for r in rv[0]] == [OK, OK, BAD_ARGUMENT, BAD_ARGUMENT]
    assert all(r.lines for r in rv[0][:2]) and all(r.lines == [] for r in rv[0][2:]) and all(r.lines for r in rv[1])


def test_short_rows_have_lines_and_readiness_is_reported():
    N, R = 5, 64
    env = ag.GoEnv(N)
    nn = peaked_net(env, 1, 7)
    positions = api_positions(env, 12, 4, 6)
    res = ag.analyze(env, nn, positions, num_readouts=R, seed=1, slots=2, max_nodes_per_game=24, lines=K, pv_depth=D)
    short = [a for a in res if a.status == POOL_EXHAUSTED]
    assert short
    for a in short:                                               # a short row is a valid row: so are its lines
        assert a.N < R and a.lines and a.lines[0].N == a.child_N.max() and a.lines[0].pv[0] == a.lines[0].move
        order = [(-float(l.N), -float(l.prior), ag.to_flat(l.move, env)) for l in a.lines]
        assert order == sorted(order)
    # readiness
    eng = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=32)
    eng.init_synthetic(0)
    eng.analyze_set_lines(K, D, 1)
    eng.analyze_start(*opos_arrays([orc.make_pos(N)] * 3))
    eng.step(1)
    assert eng.analyze_progress() < 3
    with pytest.raises(ag.AgzError) as ex:
        eng.analyze_lines()
    assert ex.value.status == NOT_READY
    while eng.analyze_progress() < 3:
        eng.step(4)
    t = eng.analyze_lines()
    assert (t["move"][:, 0] >= 0).all()
    eng.analyze_set_lines(0)                                      # off again: takes effect at the next start
    assert (eng.analyze_lines()["move"][:, 0] >= 0).all()
    run_analysis(eng, *opos_arrays([orc.make_pos(N)] * 2))
    with pytest.raises(ag.AgzError) as ex:
        eng.analyze_lines()
    assert ex.value.status == BAD_ARGUMENT
    for bad in ((-1, 16, 1), (17, 16, 1), (4, 0, 1), (4, 65, 1), (4, 16, 0)):
        with pytest.raises(ag.AgzError) as ex:
            eng.analyze_set_lines(*bad)
        assert ex.value.status == BAD_ARGUMENT, bad
    eng.close()


# ---------------------------------------------------------------- 9. the single-tree call

def test_tree_lines_equal_the_walk_and_print_it():
    N, R = 9, 64
    env = ag.GoEnv(N)
    nn = peaked_net(env, 2, 1)
    p = ag.MCTSPlayer(env, nn, num_readouts=R, seed=2, game_id=5, two_player_mode=True)
    p.initialize_game(None)
    p.suggest_move()
    root = p.root
    e = p.engine
    for k, d, mv in ((4, 16, 1), (16, 64, 1), (4, 4, 2), (1, 1, 1)):
        t = player_walk(p, root.id, k, d, mv)
        assert lines_twin.same(e.tree_lines(0, root.id, k, d, mv), t) is None, (k, d, mv)
        assert_lines_equal(root.lines(k, d, mv), as_lines(env, t), (k, d, mv))
    t = player_walk(p, root.id)
    assert (t["move"] >= 0).sum() >= 2 and t["pv_len"][0] >= 2
    inner = int(e.node_children(0, root.id)[t["move"][0]])          # an inner node: the first line's first child
    assert inner >= 0
    ti = player_walk(p, inner)
    assert ti["move"][0] == t["pv"][0, 1]
    assert lines_twin.same(e.tree_lines(0, inner, K, D, 1), ti) is None
    # the strings of mcts.jl:267-293 over the first line of the walk
    t1 = player_walk(p, root.id, 1, 64, 1)
    n = int(t1["pv_len"][0])
    want = "".join(f"{ag.to_kgs(ag.from_flat(int(a), env), env)} ({float(v):.1f}) ==> "
                   for a, v in zip(t1["pv"][0, :n], t1["pv_N"][0, :n]))
    want += "Q: %.5f\n" % (t1["end_W"][0] / (np.float32(1) + t1["pv_N"][0, n - 1]))
    assert root.most_visited_path() == want
    t2 = player_walk(p, root.id, 1, 64, 2)
    assert root.mvp_gg() == " ".join(ag.to_kgs(ag.from_flat(int(a), env), env) for a in t2["pv"][0, :t2["pv_len"][0]])
    assert root.mvp_gg() != ""
    d = root.describe()
    assert d.startswith("%.4f\n" % root.Q) and want in d and "P-Dir" not in d
    assert d.count("\n") == 2 + min(15, int((root.child_N > 0).sum()))
    # the tie cases on the device: rows set by node_set_floats over the searched tree's nodes
    A = env.action_space
    kids = {int(a): int(c) for a, c in enumerate(e.node_children(0, root.id)) if c >= 0}
    a1, a2 = sorted(kids)[:2]
    free = next(a for a in range(A) if a not in kids)
    rows = [np.zeros(A, np.float32) for _ in range(3)]
    rows[0][[a1, a2, free]] = (7, 7, 7)
    rows[2][[a1, a2, free]] = (0.25, 0.5, 0.125)
    rows[1][[a1, a2, free]] = (1.5, -2.5, 0.75)
    for f in range(3):
        e.node_set_floats(0, root.id, f, rows[f])
    got = e.tree_lines(0, root.id, 4, 8, 1)
    assert lines_twin.same(got, player_walk(p, root.id, 4, 8, 1)) is None
    assert list(got["move"]) == [a2, a1, free, -1] and got["pv_len"][2] == 1        # prior decides; no node: alone
    rows[2][[a1, a2, free]] = 0.5
    e.node_set_floats(0, root.id, 2, rows[2])
    got = e.tree_lines(0, root.id, 4, 8, 1)
    assert lines_twin.same(got, player_walk(p, root.id, 4, 8, 1)) is None
    assert list(got["move"]) == sorted([a1, a2, free]) + [-1]                        # equal priors: the lower action
    cn = np.zeros(A, np.float32)
    cn[[3, 40, 77]] = 5                                                              # a shared maximum one level down
    e.node_set_floats(0, kids[a1], 0, cn)
    got = e.tree_lines(0, root.id, 4, 8, 1)
    assert lines_twin.same(got, player_walk(p, root.id, 4, 8, 1)) is None
    k1 = list(got["move"]).index(a1)
    assert got["pv"][k1, 1] == 3 and got["pv_N"][k1, 1] == 5
    with pytest.raises(ag.AgzError):
        e.tree_lines(0, 10 ** 6, 4, 8, 1)
    e.close()


# ---------------------------------------------------------------- 10. self-play is not changed

def test_selfplay_after_analysis_with_lines_is_unchanged():
    from test_gpu_analysis import case_positions
    N, games = 5, 4
    kw = dict(board_size=N, tower_height=1, games=3, num_readouts=16, seed=2, record_capacity_games=games + 8)

    def play(eng):
        eng.start(games)
        for _ in range(20000):
            eng.step(8)
            if eng.stats()["games_finished"] >= games:
                break
        return sorted(eng.records(), key=lambda r: int(r["game_id"]))

    eng = ag.Engine(**kw)
    eng.init_synthetic(0)
    first = play(eng)
    st0 = eng.stats()
    eng.analyze_set_lines(K, D, 1)
    run_analysis(eng, *opos_arrays(case_positions(N)))
    assert (eng.analyze_lines()["move"][:, 0] >= 0).any()
    st1 = eng.stats()
    assert eng.records_count() == games
    for f in ("positions", "games_started", "games_finished", "resigned_games", "abandoned_games"):
        assert st1[f] == st0[f], f
    second = play(eng)
    fresh = ag.Engine(**kw)
    fresh.init_synthetic(0)
    ref = play(fresh)
    for recs in (first, second):
        assert len(recs) == len(ref)
        for a, b in zip(recs, ref):
            assert a["game_id"] == b["game_id"] and a["num_moves"] == b["num_moves"]
            assert (a["moves"] == b["moves"]).all() and bits_equal(a["pis"], b["pis"]) and bits_equal(a["qs"], b["qs"])
    eng.close()
    fresh.close()
