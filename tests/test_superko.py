"""Superko on the host (agz_search_set_ko_rule): the keys of include/agz_superko.h against a numpy
restatement bit for bit, and the rule -- run by the host simulator (hs.Sim: agz_search.h lane-serial) -- against
its independent statement, go_shapes.ff_legal / ff_play plus a Python set of boards (superko_twin.Line), which uses no
keys: random legal play with a census of what it reaches, hand-built cycles in every image and both colourings, single
trees, whole self-play games with their counters, the refusals, and a stand-alone sanitizer program."""
import numpy as np
import pytest

import go_shapes as gs
import gpu_options
import hs
import superko_twin as sk
from test_explore import run_sanitizer_part

u64 = np.uint64
POS, SIT = sk.POSITIONAL, sk.SITUATIONAL
G_SEARCH = 3


# ---------------------------------------------------------------- the header

def test_keys_equal_the_restatement_bit_for_bit():
    L = hs.lib()
    assert L.hs_white_to_play() == sk.WHITE_TO_PLAY
    pts = np.arange(0, 19 * 19 + 40)
    for colour in (1, -1):
        want = sk.zobrist(pts, np.full(len(pts), colour))
        got = np.array([L.hs_zobrist(int(p), colour) for p in pts], u64)
        assert (got == want).all()
    both = np.concatenate([sk.zobrist(pts, np.ones(len(pts))), sk.zobrist(pts, -np.ones(len(pts)))])
    assert len(set(both.tolist()) | {sk.WHITE_TO_PLAY, 0}) == 2 * len(pts) + 2, "the stone keys are distinct"
    rng = np.random.RandomState(5)
    for N in (2, 3, 9, 19):
        sim = hs.Sim(board_size=N, games=1, num_readouts=4, max_nodes_per_game=8)
        boards = rng.randint(-1, 2, size=(24, N * N)).astype(np.int8)
        boards[0] = 0
        tp = np.where(rng.rand(24) < 0.5, 1, -1).astype(np.int8)
        for rule in (sk.SIMPLE, POS, SIT):
            want = np.array([sk.np_key(b, t, rule) for b, t in zip(boards, tp)], u64)
            assert (sim.position_keys(boards, tp, rule) == want).all(), (N, rule)
            host = np.array([L.hs_position_key(hs.p8(np.ascontiguousarray(b)), N * N, int(t), rule)
                             for b, t in zip(boards, tp)], u64)
            assert (host == want).all(), (N, rule)
        assert sim.position_keys(boards[:1], tp[:1], POS)[0] == 0, "the empty board"
        sim.close()


def test_child_key_identity_on_the_capture_family():
    """node key XOR the stone XOR the captured groups (each once) XOR the side constant = the key of the board after
    ff_play, on every move of the ko_and_captures family; the family has moves that take 2, 3 and 4 groups at once"""
    groups_seen = set()
    for case in gs.ko_and_captures():
        N, tp = case.N, case.to_play
        legal = gs.ff_legal(case.board, N, tp, case.ko)
        index, groups = gs.ff_groups(case.board, N)
        for a in np.nonzero(legal[:-1])[0]:
            a = int(a)
            st, after, _, ncap = gs.ff_play(case.board, N, tp, case.ko, a)
            assert st == gs.OK
            dead = {int(index[q]) for q in gs.neighbours(N, a) if case.board[q] == -tp and groups[index[q]][1] == {a}}
            groups_seen.add(len(dead))
            for rule in (POS, SIT):
                k = sk.np_key(case.board, tp, rule) ^ int(sk.zobrist([a], [tp])[0])
                for gi in dead:
                    stones = sorted(groups[gi][0])
                    k ^= int(np.bitwise_xor.reduce(sk.zobrist(stones, case.board[stones])))
                if rule == SIT:
                    k ^= sk.WHITE_TO_PLAY
                assert k == sk.np_key(after, -tp, rule), (case.name, a, rule)
            assert sum(len(groups[gi][0]) for gi in dead) == ncap
    assert {2, 3, 4} <= groups_seen, groups_seen


# ---------------------------------------------------------------- random legal play

def sim_masks(sim, positions, rule):
    b, tp, ko = sk.soa([(p["board"], p["to_play"], p["ko"]) for p in positions])
    return sim.legal_moves(b, tp, ko, [p["keys"] for p in positions], rule)


@pytest.mark.parametrize("rule", sk.RULES)
@pytest.mark.parametrize("N", sorted(sk.RANDOM_PLAY))
def test_random_play_masks_equal_the_twin(N, rule):
    positions = sk.random_games(N, rule)
    sim = hs.Sim(board_size=N, games=1, num_readouts=4, max_nodes_per_game=8)
    got = sim_masks(sim, positions, rule)
    want = np.stack([p["legal"] for p in positions])
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (N, rule, bad[:5])
    # with no seen keys, and under the simple rule with them, the entry is all_legal_moves
    simple = np.stack([p["simple"] for p in positions])
    b, tp, ko = sk.soa([(p["board"], p["to_play"], p["ko"]) for p in positions])
    assert (sim.legal_moves(b, tp, ko, [[] for _ in positions], rule) == simple).all()
    assert (sim.legal_moves(b, tp, ko, [p["keys"] for p in positions], sk.SIMPLE) == simple).all()
    assert (got[:, -1] == 1).all(), "pass is always legal"
    sim.close()


def test_census_of_the_random_fixtures():
    """what the random games reach under the positional rule, seed 7, pass probability 0.1 (printed), held to the floors:
    positions that lose a move at N = 2 >= 50, at N = 3 >= 10; positions where the two rules' masks differ >= 10; removed
    moves that capture nothing >= 10"""
    c = {N: sk.census(sk.random_games(N, POS)) for N in sorted(sk.RANDOM_PLAY)}
    for N, row in c.items():
        print(f"{N}x{N}: {row}")
        games, plies = sk.RANDOM_PLAY[N]
        assert row["positions"] > games
    assert (sk.RANDOM_PLAY[2], sk.RANDOM_PLAY[3], sk.RANDOM_PLAY[4]) == ((40, 60), (40, 80), (30, 100))
    assert c[2]["lost"] >= 50 and c[3]["lost"] >= 10
    assert sum(row["differ"] for row in c.values()) >= 10
    assert sum(row["free"] for row in c.values()) >= 10
    assert all(row["removed"] >= row["lost"] for row in c.values())


# ---------------------------------------------------------------- hand-built cycles

def test_the_fixture_set_is_what_it_says():
    names = {f.name.split("/")[0] for f in sk.fixtures()}
    N0 = sk.smallest_triple_ko()[0]
    assert names == {f"triple_ko_{N0}", "triple_ko_9", "triple_ko_19", "send_two_return_one_5", "send_two_return_one_9",
                     "send_two_pass_pass_return_one_5", "send_two_pass_pass_return_one_9",
                     f"two_groups_{sk.two_group_closing()[0]}"}
    assert len(sk.fixtures()) == 16 * len(names), "eight images, two colourings"
    assert N0 < 9
    for n in range(4, N0):      # no smaller board holds three of these kos
        from itertools import combinations
        places = [(s, c) for s in range(8) for c in range(n - 3)]
        assert all(sk.triple_ko(n, list(t)) is None for t in combinations(places, 3))
    board, cycle = sk.triple_ko_19()
    assert sorted({a // 32 for a in cycle}) == [0, 1, 3, 4, 6, 7], "the kos' points lie on both sides of 32, 128 and 224"
    # the closing move of the two-group fixture does take two groups
    f = [x for x in sk.fixtures() if x.name.startswith("two_groups") and x.name.endswith("/s0")][0]
    line = sk.Line(f.N, POS, f.board, f.to_play)
    for a in f.moves[:-1]:
        line.play(a)
    assert gs.captured_groups(line.board, f.N, line.to_play, f.moves[-1]) >= 2


@pytest.mark.parametrize("rule", sk.RULES)
def test_hand_built_cycles(rule):
    """every fixture, move by move: the simulator's mask equals the twin's at every position, every move of the cycle but
    the last is legal, and the last is refused exactly under the rules the fixture names"""
    sims = {}
    by_size = {}
    for f in sk.fixtures():
        positions, refused = sk.fixture_positions(f, rule)
        assert refused == (rule in f.refused), (f.name, rule)
        by_size.setdefault(f.N, []).extend((f.name, i, p) for i, p in enumerate(positions))
    for N, rows in by_size.items():
        sim = sims.setdefault(N, hs.Sim(board_size=N, games=1, num_readouts=4, max_nodes_per_game=8))
        b, tp, ko = sk.soa([p for _, _, p in rows])
        got = sim.legal_moves(b, tp, ko, [p[3] for _, _, p in rows], rule)
        want = np.stack([p[4] for _, _, p in rows])
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (rule, [rows[i][:2] for i in bad[:5]])
    for sim in sims.values():
        sim.close()


def test_a_pass_between_the_repetitions_splits_the_rules():
    """send two, capture, pass, pass, return one: the board of the start with the other side to move -- the positional rule
    refuses the return, the situational rule allows it"""
    f = [x for x in sk.fixtures() if x.name == "send_two_pass_pass_return_one_5/s0"][0]
    sim = hs.Sim(board_size=5, games=1, num_readouts=4, max_nodes_per_game=8)
    last = {}
    for rule in sk.RULES:
        positions, refused = sk.fixture_positions(f, rule)
        b, tp, ko = sk.soa(positions[-1:])
        last[rule] = int(sim.legal_moves(b, tp, ko, [positions[-1][3]], rule)[0][f.moves[-1]])
        assert refused == (rule == POS)
    assert last == {POS: 0, SIT: 1}
    sim.close()


# ---------------------------------------------------------------- single trees

def check_node(sim, node, line, g=0):
    """the node's mask and key against the twin's line that leads to it"""
    assert (sim.board(g, node) == line.board).all()
    assert (sim.legal(g, node) == line.legal()).all(), (node, line.board.reshape(line.N, line.N).T, line.to_play)
    assert sim.node_key(node, g) == sk.np_key(line.board, line.to_play, line.rule)


def walk(sim, node, line, rng, depth, g=0):
    """maybe_add_child over every action of `node`: a refused action takes no node, an allowed one gives a child whose
    mask and key are the twin's; then down `depth` levels along one allowed action"""
    legal = line.legal()
    kids = {}
    for a in range(sim.A):
        st, c = sim.op(hs.TOP_ADD_CHILD, g=g, node=node, a=a)
        if legal[a]:
            assert st == 0 and c >= 0, (node, a)
            kids[a] = c
        else:
            assert st == sk.ag._lib.ILLEGAL_MOVE and sim.children(g, node)[a] == -1, (node, a, st)
    for a, c in kids.items():
        nxt = line.copy()
        nxt.play(a)
        check_node(sim, c, nxt, g)
    if depth > 0:
        board_moves = [a for a in kids if a != sim.P] or list(kids)
        a = board_moves[rng.randint(len(board_moves))]
        nxt = line.copy()
        nxt.play(a)
        walk(sim, kids[a], nxt, rng, depth - 1, g)


def tree_fixture(N):
    """a start for the trees: 3x3 -- a few random moves; 5x5 -- the send-two-return-one corner"""
    if N == 5:
        return sk.send_two_return_one(5)[0]
    return np.array([1, -1, 0, 0, 1, -1, 0, 0, 0], np.int8)


@pytest.mark.parametrize("rule", sk.RULES)
@pytest.mark.parametrize("N", (3, 5))
def test_single_tree_nodes_equal_the_twin(N, rule):
    rng = np.random.RandomState(N)
    sim = hs.Sim(board_size=N, games=1, num_readouts=8, max_nodes_per_game=512, two_player_mode=1)
    gpu_options.configure(sim, dict(ko_rule=rule))
    board = tree_fixture(N)
    root = sim.tree_init(0, board)
    line = sk.Line(N, rule, board)
    check_node(sim, root, line)
    assert sim.game_log() == []
    walk(sim, root, line, rng, depth=2 * N)
    if N == 5:      # the cycle of the fixture, down the tree: the third move takes no node under the positional rule
        cyc = sk.send_two_return_one(5)[1]
        n1 = sim.children(0, root)[cyc[0]]
        n2 = sim.children(0, n1)[cyc[1]] if n1 >= 0 else -1
        if n2 < 0:
            st, n1 = sim.op(hs.TOP_ADD_CHILD, node=root, a=cyc[0])
            st, n2 = sim.op(hs.TOP_ADD_CHILD, node=n1, a=cyc[1])
        st, n3 = sim.op(hs.TOP_ADD_CHILD, node=n2, a=cyc[2])
        assert (st != 0) == (rule == POS)
    sim.close()


@pytest.mark.parametrize("rule", sk.RULES)
def test_new_nodes_see_the_log_after_play_move(rule):
    """play_move re-roots: the old roots' keys go to the slot's log, and nodes made afterwards are refused what repeats
    them.  The send-two-return-one cycle, played at the root, then searched one level down."""
    N = 5
    board, cyc = sk.send_two_return_one(N)
    sim = hs.Sim(board_size=N, games=1, num_readouts=8, max_nodes_per_game=256, two_player_mode=1)
    gpu_options.configure(sim, dict(ko_rule=rule))
    root = sim.tree_init(0, board)
    line = sk.Line(N, rule, board)
    for k, a in enumerate(cyc[:2]):
        st, ok = sim.op(hs.TOP_PLAY, a=a)
        assert st == 0 and ok == 1
        line.play(a)
        root = sim.game(0).root
        check_node(sim, root, line)
        assert sim.game_log() == line.seen_keys()[:-1], "the log holds every position the root has left behind"
    rng = np.random.RandomState(1)
    walk(sim, root, line, rng, depth=3)
    assert bool(line.legal()[cyc[2]]) == (rule == SIT)
    st, ok = sim.op(hs.TOP_PLAY, a=cyc[2])
    assert (ok == 1) == (rule == SIT)
    sim.close()


@pytest.mark.parametrize("rule", sk.RULES)
@pytest.mark.parametrize("H", (1, 3, 7))
def test_new_nodes_see_the_history_boards(H, rule):
    """agz_tree_init with H history boards: a game played outside the tree for H plies, installed at its last position.
    The log is the boards' keys with their sides to move, and the masks of the tree are the twin's."""
    N = 3
    rng = np.random.RandomState(10 * H + rule)
    for attempt in range(6):
        line = sk.Line(N, rule)
        for _ in range(6):          # earlier positions the install does not hand over: unknown to the rule
            moves = np.nonzero(line.legal()[:-1])[0]
            line.play(int(moves[rng.randint(len(moves))]))
        known = sk.Line(N, rule, line.board, line.to_play, line.ko)
        boards = [line.board.copy()]
        for _ in range(H):
            moves = np.nonzero(known.legal()[:-1])[0]
            if len(moves) == 0:
                break
            known.play(int(moves[rng.randint(len(moves))]))
            boards.append(known.board.copy())
        if len(boards) == H + 1:
            break
    assert len(boards) == H + 1
    history = boards[:-1][::-1]                      # newest first
    sim = hs.Sim(board_size=N, games=1, num_readouts=8, max_nodes_per_game=512, two_player_mode=1)
    gpu_options.configure(sim, dict(ko_rule=rule))
    root = sim.tree_init(0, known.board, n=6 + H, to_play=known.to_play, ko=known.ko, history=np.stack(history))
    tw = sk.Line(N, rule, known.board, known.to_play, known.ko, history=history)
    assert sorted(sim.game_log()) == sorted(tw.seen_keys()[:-1]) and len(sim.game_log()) == H
    assert sorted(tw.seen_keys()) == sorted(known.seen_keys()), "the sides to move of the history boards"
    check_node(sim, root, tw)
    walk(sim, root, tw, rng, depth=4)
    sim.close()


# ---------------------------------------------------------------- whole self-play games

def replay_repeats(rec, N, rule):
    """how many positions of the recorded game repeat an earlier one under `rule` (a pass is not a repetition)"""
    line = sk.Line(N, rule)
    seen, rep = {sk.situation(line.board, line.to_play, rule)}, 0
    for a in rec["moves"]:
        a = int(a)
        if a != N * N:
            assert line.legal()[a], "a recorded move the rule refuses"
        line.play(a)
        s = sk.situation(line.board, line.to_play, rule)
        if a != N * N:
            rep += s in seen
        seen.add(s)
    return rep


def play_games(N, rule, games=8, slots=4, readouts=16, seed=3, tally=True, options=None, **cfg):
    """self-play on the simulator under `rule`; the tally: every node, when it first shows up live, adds what its mask
    lacks against all_legal_moves of its own board"""
    sim = hs.Sim(board_size=N, games=slots, num_readouts=readouts, seed=seed, record_capacity_games=games + 8,
                 resign_threshold=-2.0, resign_disable_fraction=1.0, max_nodes_per_game=384, **cfg)
    gpu_options.configure(sim, dict(options or {}, ko_rule=rule))
    net = hs.PeakedNet(N)
    sim.start(games)
    known, nodes, moves = [dict() for _ in range(slots)], 0, 0
    for _ in range(40000):
        sim.step(net)
        if tally:
            for g in range(slots):
                live = {}
                for i in sim.live_nodes(g):
                    m = sim.meta(g, i)
                    live[i] = (m.fmove, m.n, sim.board(g, i).tobytes())      # (re-rooting rewrites meta.parent)
                for i, ident in live.items():
                    if known[g].get(i) != ident:
                        m = sim.meta(g, i)
                        gone = int((gs.ff_legal(sim.board(g, i), N, m.to_play, m.ko) != sim.legal(g, i)).sum())
                        nodes += gone > 0
                        moves += gone
                known[g] = live
        if sim.L.hs_records_count(sim.h) >= games:
            break
    recs, counts, cnt = sim.records(), sim.superko_counts(), sim.all_counters()
    cnt["uncertainty"], cnt["puct"] = sim.uncertainty_counts(), sim.puct_counts()
    sim.close()
    assert len(recs) == games and cnt["CT_POOL_EXHAUSTED"] == 0
    return recs, counts, (nodes, moves), cnt


@pytest.mark.parametrize("rule", sk.RULES)
def test_selfplay_games_repeat_no_position(rule):
    """8 games, 16 readouts, the peaked network, resignation off, at 3x3 and 4x4: replayed, no recorded game repeats a
    position under its rule; both counters equal the tally over the nodes; both are positive over the two sizes.  (At
    3x3 a game ends after 12 plies: the positional rule removes moves there -- (4, 4) at this seed -- but no search of
    six seeds tried met a situational repetition beyond the simple ko, so the situational counters are positive through
    the 4x4 games alone.)"""
    total = np.zeros(2, np.int64)
    for N in (3, 4):
        recs, counts, tally, _ = play_games(N, rule)
        print(f"{N}x{N} {sk.RULE_NAMES[rule]}: counters {counts}, tally {tally}")
        assert all(replay_repeats(r, N, rule) == 0 for r in recs)
        assert counts == tally
        total += counts
    assert total[0] > 0 and total[1] >= total[0]


def same_records(a, b):
    bits = hs.bits32
    return len(a) == len(b) and all(
        x["game_id"] == y["game_id"] and x["num_moves"] == y["num_moves"] and (x["moves"] == y["moves"]).all() and
        x["result"] == y["result"] and (bits(x["pis"]) == bits(y["pis"])).all() and (bits(x["qs"]) == bits(y["qs"])).all()
        for x, y in zip(a, b))


@pytest.mark.parametrize("rule", sk.RULES)
def test_a_run_whose_counters_stay_zero_is_the_run_without_the_rule(rule):
    """9x9, 4 games, 16 readouts, the first 12 plies: no search of these meets a repetition (both counters stay zero), so
    the run is the run with no rule set, byte for byte: every slot's GameState and live root rows after every step, and
    every counter of the enum at the end"""
    import ctypes as C
    cfg = dict(board_size=9, games=4, num_readouts=16, seed=3, resign_threshold=-2.0, resign_disable_fraction=1.0,
               max_nodes_per_game=768)
    off, on = hs.Sim(**cfg), hs.Sim(**cfg)
    gpu_options.configure(on, dict(ko_rule=rule))
    nets = hs.PeakedNet(9), hs.PeakedNet(9)
    off.start(4)
    on.start(4)
    for step in range(4000):
        off.step(nets[0])
        on.step(nets[1])
        done = True
        for g in range(4):
            a, b = off.game(g), on.game(g)
            assert bytes(a) == bytes(b), (step, g)
            if a.phase == G_SEARCH:
                for field in range(3):
                    assert (hs.bits32(off.row(g, a.root, field)) == hs.bits32(on.row(g, b.root, field))).all(), (step, g)
                assert (off.legal(g, a.root) == on.legal(g, b.root)).all()
            done = done and a.move_count >= 12
        if done:
            break
    assert done and on.superko_counts() == (0, 0) and off.superko_counts() == (0, 0)
    assert off.all_counters() == on.all_counters(), "every counter of the enum"
    off.close()
    on.close()


def start_table(N):
    """two oracle positions a few plies in (their history boards go to the rule's log)"""
    import orc
    out, pos = [], orc.make_pos(N)
    for a in (5, 6, 9, 10, 1):
        _, pos = orc.play(pos, a)
        if a in (9, 1):
            out.append(pos.copy())
    return out


@pytest.mark.parametrize("options", ("cap_forced", "gumbel_starts"))
def test_the_rule_under_the_other_search_options(options):
    """the 4x4 games with the playout cap and forced playouts, and with the Gumbel root search from a start table,
    through gpu_options.configure: the records are stable run to run, and both counters equal
    the tally"""
    opt = (dict(cap=(6, 0.5), forced=(2.0, True)) if options == "cap_forced" else
           dict(gumbel=4, starts=start_table(4)))
    runs = [play_games(4, POS, options=opt, tally=(k == 0)) for k in range(2)]
    print(options, runs[0][1], runs[0][2])
    assert same_records(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert runs[0][1] == runs[0][2]
    assert runs[0][1][0] > 0


def test_the_rule_with_lcb_variance_and_puct_options():
    """The positional rule together with lcb, puct_variance and the PUCT option on one simulator: 3x3, 8 games on 4
    slots, 16 readouts, seed 3, hs.PeakedNet -- the first shape of the superko tests at which all three counts are
    positive.  The records are stable run to run, the superko counters equal the key-free tally, and the options were
    exercised: measured superko counts (4, 4), uncertainty counts (96 LCB picks, 23 off the most visited child, 4482
    levels under a variance factor, 3422 of them raised), all 4482 levels under the PUCT option."""
    runs = [play_games(3, POS, options=sk.COMBINED, tally=(k == 0)) for k in range(2)]
    (recs, counts, tally, cnt), again = runs[0], runs[1]
    unc = cnt["uncertainty"]
    print("combined:", counts, tally, unc)
    assert same_records(recs, again[0]) and counts == again[1] and unc == again[3]["uncertainty"]
    assert counts == tally
    assert counts[0] > 0
    assert unc[0] > 0 and unc[2] > 0 and cnt["puct"][0] > 0
    assert all(replay_repeats(r, 3, POS) == 0 for r in recs)


# ---------------------------------------------------------------- refusals

def test_refusals_keep_the_setting():
    sim = hs.Sim(board_size=3, games=2, num_readouts=8, max_nodes_per_game=64)
    assert sim.ko_rule() == sk.SIMPLE
    assert sim.set_ko_rule(POS) == sk.OK and sim.ko_rule() == POS
    for bad in (-1, 3, 99):
        assert sim.set_ko_rule(bad) == sk.BAD_ARGUMENT and sim.ko_rule() == POS
    # inside the select / incorporate window of a single tree
    sim.tree_init(0, np.zeros(9, np.int8))
    st, n = sim.op(hs.TOP_SEARCH_SELECT, g=0, par=4)
    assert st == 0 and n > 0
    assert sim.set_ko_rule(SIT) == sk.BAD_ARGUMENT and sim.ko_rule() == POS
    sim.L.hs_set_batch_outputs(sim.h, hs.pf(np.full((n, sim.A), 0.1, np.float32)), hs.pf(np.zeros(n, np.float32)), n)
    assert sim.op(hs.TOP_SEARCH_POST, g=0)[0] == 0
    assert sim.set_ko_rule(SIT) == sk.OK and sim.ko_rule() == SIT
    # while games are being played
    sim.start(2)
    sim.step(hs.PeakedNet(3))
    assert any(sim.game(g).phase == G_SEARCH for g in range(2))
    assert sim.set_ko_rule(sk.SIMPLE) == sk.BAD_ARGUMENT and sim.ko_rule() == SIT
    sim.close()


# ---------------------------------------------------------------- sanitizers

def test_sanitizer_build_plays_the_rule():
    """the `superko` part of the stand-alone sanitizer program (tests/hostsim/hostsim_sanitize.cpp, built once per
    process by test_explore.run_sanitizer_part): the 2x2 random games, one triple ko, and 3x3 self-play under the rule"""
    run_sanitizer_part("superko")
