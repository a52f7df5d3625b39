"""Superko on the device (agz_search_set_ko_rule).  All values are integers or records held to the
bit: agz_go_keys and agz_go_legal_seen on every fixture position of tests/test_superko.py, one launch per board size and
rule, against the twin (superko_twin.Line: flood fill and a set of boards, no keys); single trees at four board sizes, the
masks and keys of the walked nodes against the twin and the host simulator; self-play, engine against simulator, records
and both counters; and one analyze, one review and one arena case at 5x5, and the review of a game that breaks the rule; the off path: records
byte-equal to an engine on which the setter was never called."""
import numpy as np
import pytest

import alphago_jl_amd as ag
import gpu_options as go
import hs
import superko_twin as sk
from gpu_options import RECORD, api_game, api_positions, peaked_engine, play, same_game, sharpen
from test_hostsim_selfplay import bits_equal

pytestmark = pytest.mark.gpu
u64 = np.uint64
POS, SIT = sk.POSITIONAL, sk.SITUATIONAL
NAME = sk.RULE_NAMES


def rules_engine(N):
    """an engine for the rules kernels and single trees alone: no network of its own"""
    return ag.Engine(board_size=N, tower_height=0, games=1, num_readouts=8, external_network=1, two_player_mode=1,
                     max_nodes_per_game=4096 if N < 19 else 2600)


# ---------------------------------------------------------------- a. the two batched entries

@pytest.fixture(scope="module")
def fixture_rows():
    """{(N, rule): [(board, to_play, ko, seen keys, twin's mask)]}: the random games and the hand-built cycles"""
    rows = {}
    for rule in sk.RULES:
        for N in sorted(sk.RANDOM_PLAY):
            rows.setdefault((N, rule), []).extend(
                (p["board"], p["to_play"], p["ko"], p["keys"], p["legal"]) for p in sk.random_games(N, rule))
        for f in sk.fixtures():
            rows.setdefault((f.N, rule), []).extend(sk.fixture_positions(f, rule)[0])
    return rows


@pytest.mark.parametrize("N", (2, 3, 4, 5, 9, 19))
def test_batched_entries_equal_the_twin(N, fixture_rows):
    eng = rules_engine(N)
    for rule in sk.RULES:
        rows = fixture_rows[(N, rule)]
        b, tp, ko = sk.soa(rows)
        got = eng.legal_moves(b, tp, ko, seen=[r[3] for r in rows], rule=NAME[rule])
        want = np.stack([r[4] for r in rows])
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (N, rule, len(rows), bad[:5])
        keys = eng.position_keys(b, tp, NAME[rule])
        assert keys.dtype == u64 and (keys == np.array([sk.np_key(x, t, rule) for x, t in zip(b, tp)], u64)).all()
        assert (keys == np.array([r[3][-1] for r in rows], u64)).all(), "a position's own key closes its seen list"
        # no seen keys: all_legal_moves
        assert (eng.legal_moves(b, tp, ko, seen=[[] for _ in rows], rule=NAME[rule]) == eng.go_legal(b, tp, ko)).all()
    assert ag.position_key(b[0], int(tp[0]), "situational") == sk.np_key(b[0], int(tp[0]), SIT)
    with pytest.raises(ag.AgzError):
        eng.position_keys(b[:1], tp[:1], 7)
    eng.close()


# ---------------------------------------------------------------- b. single trees

def tree_case(N):
    """(board, moves): a hand-built cycle at this size; the first two moves are played at the root (the log), the rest
    walked down the tree"""
    name = {3: "two_groups_3", 5: "send_two_return_one_5", 9: "triple_ko_9", 19: "triple_ko_19"}[N]
    pick = [f for f in sk.fixtures() if f.name == name + "/s3/swap"]
    if not pick:                                    # (the two-group fixture is named after the size random play found)
        pick = [f for f in sk.fixtures() if f.name.startswith("two_groups") and f.name.endswith("/s3/swap")]
    return pick[0]


def both_add(eng, sim, node, a):
    """maybe_add_child on both: the child, or -1 where both refuse"""
    st, c = sim.op(hs.TOP_ADD_CHILD, node=node, a=a)
    try:
        e = eng.maybe_add_child(0, node, a)
    except ag.AgzError:
        e = -1
    assert (c if st == 0 else -1) == e, (node, a, st, c, e)
    return e


@pytest.mark.parametrize("rule", sk.RULES)
@pytest.mark.parametrize("N", (3, 5, 9, 19))
def test_single_tree_nodes_equal_the_twin_and_the_simulator(N, rule):
    f = tree_case(N)
    if f.N != N:
        pytest.skip(f"the two-group fixture lies at {f.N}x{f.N}")
    eng = rules_engine(N)
    sim = hs.Sim(board_size=N, games=1, num_readouts=8, two_player_mode=1, max_nodes_per_game=4096 if N < 19 else 2600)
    go.configure(eng, dict(ko_rule=rule))
    go.configure(sim, dict(ko_rule=rule))
    assert eng.tree_init(0, f.board, to_play=f.to_play) == sim.tree_init(0, f.board, to_play=f.to_play)
    line = sk.Line(N, rule, f.board, f.to_play)
    walked = 0

    def check(node):
        want = line.legal()
        assert (eng.node_legal(0, node) == want).all() and (sim.legal(0, node) == want).all(), (N, rule, node)
        key = sk.np_key(line.board, line.to_play, rule)
        assert eng.node_key(0, node) == key == sim.node_key(node)
        assert (eng.node_board(0, node) == line.board).all()
        return want

    split = min(2, len(f.moves) - 1)
    for a in f.moves[:split]:                       # at the root: play_move, the log
        assert eng.play_move(0, a) == 1 and sim.op(hs.TOP_PLAY, a=a) == (0, 1)
        line.play(a)
    node = eng.tree_root(0)
    assert node == sim.game(0).root
    for i, a in enumerate(f.moves[split:]):
        want = check(node)
        kids = {}
        step = 1 if N <= 9 else 7                   # 19x19: every seventh action, and the cycle's own
        for x in sorted(set(range(0, N * N + 1, step)) | {a, N * N}):
            c = both_add(eng, sim, node, x)
            assert (c >= 0) == bool(want[x]), (N, rule, node, x)
            kids[x] = c
            walked += 1
        last = i + 1 == len(f.moves) - split
        if last:
            assert (kids[a] < 0) == (rule in f.refused), "the move that closes the cycle"
            break
        assert kids[a] >= 0
        line.play(a)
        node = kids[a]
    assert walked > N
    # with no rule set, the key read-out is the position key computed on demand
    plain = rules_engine(N)
    root = plain.tree_init(0, f.board, to_play=f.to_play)
    assert plain.node_key(0, root) == sk.np_key(f.board, f.to_play, POS)
    assert (plain.node_legal(0, root) == sk.Line(N, sk.SIMPLE, f.board, f.to_play).legal()).all()
    for x in (eng, plain):
        x.close()
    sim.close()


# ---------------------------------------------------------------- c. self-play, engine against simulator

FIELDS = RECORD + ("resign_disabled", "final_score")


def lockstep_games(N, rule, games, readouts=16, seed=3, options=None):
    """-> (the engine's records, the simulator's, superko counts of both; with options, the uncertainty counts of both)"""
    cfg = dict(games=games, num_readouts=readouts, seed=seed, record_capacity_games=games + 8, c_puct=0.96,
               resign_threshold=-2.0, resign_disable_fraction=1.0)
    eng = peaked_engine(N, 1, **cfg)
    fwd = peaked_engine(N, 1, games=1, num_readouts=8, max_nodes_per_game=16)
    sim = hs.Sim(board_size=N, **cfg)
    go.configure(eng, dict(options or {}, ko_rule=rule))
    go.configure(sim, dict(options or {}, ko_rule=rule))
    eng.start(games)
    sim.start(games)
    for step in range(20000):
        eng.step(1)
        sim.step(fwd.forward_features)
        if sim.L.hs_records_count(sim.h) >= games:
            break
    assert eng.records_count() == games
    out = (sorted(eng.records(), key=lambda r: r["game_id"]), sim.records(), eng.superko_counts(), sim.superko_counts())
    if options:
        out += (eng.uncertainty_counts(), sim.uncertainty_counts())
    for x in (eng, fwd):
        x.close()
    sim.close()
    return out


@pytest.mark.parametrize("rule", sk.RULES)
@pytest.mark.parametrize("N,games", ((3, 8), (4, 6), (5, 4)))
def test_selfplay_equals_the_simulator(N, games, rule):
    recs, want, counts, wcounts = lockstep_games(N, rule, games)
    print(f"{N}x{N} {NAME[rule]}: counters {counts}")
    assert counts == wcounts
    assert len(recs) == len(want) == games
    for r, o in zip(recs, want):
        assert same_game(r, o, FIELDS), (N, rule, r["game_id"])
        line = sk.Line(N, rule)
        for a in r["moves"]:
            assert line.legal()[int(a)], "a recorded move the rule refuses"
            line.play(int(a))


def test_counters_are_positive_somewhere():
    """the positional rule at 3x3 removes moves in these searches (the simulator's run of tests/test_superko.py does)"""
    recs, want, counts, wcounts = lockstep_games(3, POS, 8)
    assert counts == wcounts and counts[0] > 0 and counts[1] >= counts[0]


def test_selfplay_with_lcb_variance_and_puct_options_equals_the_simulator():
    """the combined case of tests/test_superko.py (3x3, 8 games, 16 readouts, seed 3: the positional rule with lcb,
    puct_variance and the PUCT option) on the engine's own forward: records bit for bit, both sets of counters equal,
    and every option exercised"""
    recs, want, counts, wcounts, unc, wunc = lockstep_games(3, POS, 8, options=sk.COMBINED)
    print(f"combined: superko {counts} / {wcounts}, uncertainty {unc} / {wunc}")
    assert len(recs) == len(want) == 8
    assert all(same_game(r, o, RECORD) for r, o in zip(recs, want))
    assert counts == wcounts and unc == wunc
    assert counts[0] > 0
    assert unc[0] > 0 and unc[2] > 0


# ---------------------------------------------------------------- c2. analyze, review, the arena at 5x5

OK, BAD_ARGUMENT = ag._lib.OK, ag._lib.BAD_ARGUMENT
f32 = np.float32


def rows_equal(a, root):
    return (bits_equal(a.N, f32(root.N)) and bits_equal(a.W, f32(root.W)) and bits_equal(a.child_N, root.child_N) and
            bits_equal(a.child_W, root.child_W) and bits_equal(a.prior, root.child_prior))


def test_analyze_equals_the_player_under_the_rule():
    env = ag.GoEnv(5)
    nn = ag.NeuralNet(env, tower_height=1, seed=1)
    sharpen(nn.engine, 5)
    positions = api_positions(env, 3, 5, 10)
    kw = dict(num_readouts=48, seed=4, two_player_mode=True, ko_rule="positional")
    res = ag.analyze(env, nn, positions, game_id_base=100, slots=2, **kw)
    for k, pos in enumerate(positions):
        p = ag.MCTSPlayer(env, nn, game_id=100 + k, **kw)
        p.initialize_game(pos)
        mv = p.suggest_move()
        a = res[k]
        assert a.status == OK and ag.to_flat(a.move, env) == ag.to_flat(mv, env), k
        assert rows_equal(a, p.root), k
        assert (p.root.legal() == p.engine.node_legal(0, p.root.id)).all() and p.root.key == p.engine.node_key(0, p.root.id)
        p.engine.close()


def test_review_equals_the_player_under_the_rule():
    env = ag.GoEnv(5)
    nn = ag.NeuralNet(env, tower_height=1, seed=1)
    sharpen(nn.engine, 5)
    games = [api_game(env, 10 + j, 6) for j in range(2)]
    kw = dict(num_readouts=16, seed=4, ko_rule="situational")
    res = ag.review(env, nn, games, game_id_base=100, slots=2, **kw)
    for j, g in enumerate(games):
        p = ag.MCTSPlayer(env, nn, game_id=100 + j, two_player_mode=True, **kw)
        p.initialize_game(None)
        for k, m in enumerate(g):
            mv = p.suggest_move()
            a = res[j][k]
            assert a.status == OK and a.move == mv, (j, k)
            assert rows_equal(a, p.root), (j, k)
            assert p.play_move(m)
        p.engine.close()


def test_review_gives_up_a_game_that_breaks_the_rule():
    """a game recorded without the rule: the stones of the send-two-return-one corner, then its three moves.  The ninth
    move recreates the board two plies back: under the positional rule its row and the later ones carry the give-up
    status of a move that cannot be played; with no rule, and under the situational one, every row is searched"""
    N = 5
    pt = lambda r, c: r + N * c
    game = [pt(0, 1), pt(1, 0), pt(1, 2), pt(1, 1), pt(0, 3), pt(4, 4), pt(0, 0), pt(0, 2), pt(0, 1), pt(3, 3)]
    for rule, bad in ((sk.SIMPLE, None), (POS, 8), (SIT, None)):          # (what the twin says of this game)
        line, first = sk.Line(N, rule), None
        for k, a in enumerate(game):
            if not line.legal()[a]:
                first = k
                break
            line.play(a)
        assert first == bad
    env = ag.GoEnv(N)
    nn = ag.NeuralNet(env, tower_height=1, seed=1)
    for rule, bad in ((None, None), ("positional", 8), ("situational", None)):
        rows = ag.review(env, nn, [game], num_readouts=16, seed=4, slots=1, ko_rule=rule)[0]
        assert len(rows) == len(game)
        status = [r.status for r in rows]
        if bad is None:
            assert status == [OK] * len(game), (rule, status)
        else:
            assert status == [OK] * bad + [BAD_ARGUMENT] * (len(game) - bad), (rule, status)
            assert all(r.move is None for r in rows[bad:])


def test_evaluate_equals_the_simulator_arena_under_the_rule():
    env = ag.GoEnv(5)
    a, b = ag.NeuralNet(env, tower_height=1, seed=0), ag.NeuralNet(env, tower_height=1, seed=5)
    games = 2
    ok, st = ag.evaluate(env, a, b, num_games=games, ro=16, seed=2, return_stats=True, ko_rule="positional", c_puct=0.96)
    sim = hs.Sim(board_size=5, games=2 * games, num_readouts=16, seed=2, arena_mode=1, record_capacity_games=games + 8,
                 c_puct=0.96)
    go.configure(sim, dict(ko_rule=POS))
    sim.start(games)
    for _ in range(20000):
        sim.step(a.engine.forward_features, b.engine.forward_features)
        if sim.L.hs_records_count(sim.h) >= games:
            break
    want = sim.records()
    got = sorted(st.records, key=lambda r: r["game_id"])
    assert len(want) == len(got) == games
    for r, o in zip(got, want):
        assert r["game_id"] // 2 == o["game_id"] // 2 and r["num_moves"] == o["num_moves"], r["game_id"]
        assert (r["moves"] == o["moves"]).all() and bits_equal(r["qs"], o["qs"]) and r["result"] == o["result"]
    sim.close()


# ---------------------------------------------------------------- d. off

def test_off_is_the_engine_the_setter_never_touched():
    cfg = dict(games=4, num_readouts=16, seed=3, record_capacity_games=12, c_puct=0.96)
    runs = []
    for mode in ("never", "simple", "on_then_simple"):
        eng = peaked_engine(5, 1, **cfg)
        if mode == "simple":
            eng.set_ko_rule("simple")
        if mode == "on_then_simple":
            eng.set_ko_rule("positional")
            eng.set_ko_rule("simple")
        recs, st = play(eng, 4)
        assert eng.superko_counts() == (0, 0)
        runs.append((recs, st))
        eng.close()
    for recs, st in runs[1:]:
        assert len(recs) == len(runs[0][0])
        assert all(same_game(r, o, FIELDS) for r, o in zip(recs, runs[0][0]))
        assert st == runs[0][1], "every figure of agz_stats"


def test_refusals_keep_the_setting():
    eng = peaked_engine(3, 1, games=2, num_readouts=8, seed=1)
    eng.set_ko_rule("positional")
    root = eng.tree_init(0, np.zeros(9, np.int8))
    key = eng.node_key(0, root)
    for bad in (-1, 3):
        with pytest.raises(ag.AgzError):
            eng.set_ko_rule(bad)
    with pytest.raises(ValueError):
        eng.set_ko_rule("super")
    n = eng.tree_search_select(0, 4)
    assert n > 0
    with pytest.raises(ag.AgzError):                 # inside the select / incorporate window
        eng.set_ko_rule("situational")
    eng.tree_search_incorporate(0)
    eng.start(2)
    eng.step(1)
    with pytest.raises(ag.AgzError):                 # games in flight
        eng.set_ko_rule("simple")
    assert key == 0
    eng.close()
