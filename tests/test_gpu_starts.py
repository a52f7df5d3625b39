"""Start positions for self-play, the arena and replay on the device (agz_selfplay_set_starts).

Game gid of a run with a table of S entries must be, bit for bit, the twin's game (tests/selfplay_twin.py: the reference's
loops with initialize_game!(player, start)) from entry gid mod S -- arena game g from entry g mod S -- and every
consumer of its record must rebuild or_get_feats of the twin's positions.  Refusals leave the table in force."""
import numpy as np
import pytest

import alphago_jl_amd as ag
import orc
import selfplay_twin as tw
from alphago_jl_amd import symmetry
from gpu_common import GpuNetForOracle
from gpu_options import assert_game_equals_twin as assert_selfplay_equal, assert_train_equals_twin, host_schedule
from gpu_options import play as play_sorted
from test_hostsim_selfplay import OracleNet, bits_equal

pytestmark = pytest.mark.gpu
L = orc.lib()
BAD_ARGUMENT = ag._lib.BAD_ARGUMENT
PLIES = (1, 4, 7, 12, 2, 9)
NEVER = dict(resign_threshold=-0.9, resign_disable_fraction=0.0)        # resignation never disabled


def table(N):
    """S = 8: six starts of random play (both colours to move, 1..7 history boards, passes in some), a set-up position
    (stones placed, n = 0, White to move, no history, komi 0.5) and a start with the ko point set"""
    return tw.random_starts(N, PLIES, seed=0) + [tw.setup_start(N), tw.ko_start(N)]


def set_table(eng, starts):
    b, i, h = tw.opos_arrays(starts)
    eng.set_starts(boards=b, info=i, history=h)


def play(eng, games, network=None, white=None):
    return play_sorted(eng, games, network, white, sort=False)          # the order of the record ring is asserted here


def assert_arena_equal(r, o, what):
    print(f"arena game {what}: start {r['start']}, {r['num_moves']} moves, result {r['result']}, "
          f"resign {r['was_resign']}, score {r['final_score']}")
    assert r["num_moves"] == o["num_moves"], what
    assert (r["moves"] == o["moves"]).all(), what
    assert bits_equal(r["qs"], o["qs"]), what
    assert r["result"] == o["result"] and bool(r["was_resign"]) == bool(o["was_resign"]), what
    assert np.float32(r["final_score"]) == np.float32(o["final_score"]), what
    assert int(r["game_id"]) == o["ender"] and r["short_searches"] == 0, what


def check_selfplay(recs, st, starts, N, R, seed, cb):
    moves = evals = 0
    twins = {}
    for r in recs:
        gid = int(r["game_id"])
        assert r["start"] == gid % len(starts)
        o = tw.twin_selfplay(N, cb, R, seed, gid, starts[gid % len(starts)], -0.9, 0.0)
        assert_selfplay_equal(r, o, gid)
        moves += o["num_moves"]
        evals += o["evals"]
        twins[gid] = o
    assert st["positions"] == moves and st["evals"] == evals
    return twins


def assert_parity_set_is_varied(recs, starts):
    """the conditions that keep a green run from proving little"""
    used = [starts[r["start"]] for r in recs]
    assert {bool(r["was_resign"]) for r in recs} == {True, False}, "one game ends by resignation, one by score"
    assert {p.to_play for p in used} == {1, -1}
    assert {p.ndeltas for p in used} >= {0, 7}
    assert all(r["short_searches"] == 0 for r in recs)


# ---------------------------------------------------------------- self-play

@pytest.mark.parametrize("N,R,games,slots,seed", [(5, 16, 12, 4, 2), (9, 16, 8, 4, 2)])
def test_selfplay_external_network_equals_the_twin(N, R, games, slots, seed):
    net = OracleNet(N, 1, seed=0)
    starts = table(N)
    eng = ag.Engine(board_size=N, tower_height=0, games=slots, num_readouts=R, seed=seed, external_network=1,
                    record_capacity_games=games + 8, **NEVER)
    set_table(eng, starts)
    assert eng.starts_count() == len(starts)
    recs, st = play(eng, games, net.on_feats)
    assert [int(r["game_id"]) for r in recs] == list(range(games))
    check_selfplay(recs, st, starts, N, R, seed, net.cb)
    assert_parity_set_is_varied(recs, starts)
    eng.close()
    net.close()


@pytest.mark.parametrize("N,tower,R,games,slots,seed", [(5, 1, 16, 12, 4, 2), (9, 1, 16, 4, 4, 2)])
def test_selfplay_internal_network_equals_the_twin(N, tower, R, games, slots, seed):
    starts = table(N)
    eng = ag.Engine(board_size=N, tower_height=tower, games=slots, num_readouts=R, seed=seed, game_id_base=4,
                    record_capacity_games=games + 8, **NEVER)
    eng.init_synthetic(0)
    set_table(eng, starts)
    recs, st = play(eng, games)
    assert [int(r["game_id"]) for r in recs] == list(range(4, 4 + games))       # the index is the id, not the order
    fwd = ag.Engine(board_size=N, tower_height=tower, games=1, num_readouts=8, max_nodes_per_game=16)
    fwd.init_synthetic(0)
    check_selfplay(recs, st, starts, N, R, seed, GpuNetForOracle(fwd).cb)
    eng.close()
    fwd.close()


def test_one_entry_and_slot_count_is_invisible():
    """S = 1: every game has that start; 2 slots and 5 slots play the same games"""
    N, R, seed, games = 5, 16, 6, 6
    starts = table(N)
    out = []
    for slots, tbl in ((2, starts), (5, starts), (3, starts[3:4])):
        eng = ag.Engine(board_size=N, tower_height=1, games=slots, num_readouts=R, seed=seed,
                        record_capacity_games=games + 8, **NEVER)
        eng.init_synthetic(0)
        set_table(eng, tbl)
        out.append(play(eng, games)[0])
        eng.close()
    for x, y in zip(out[0], out[1]):
        assert x["game_id"] == y["game_id"] and x["num_moves"] == y["num_moves"] and x["result"] == y["result"]
        assert (x["moves"] == y["moves"]).all() and bits_equal(x["pis"], y["pis"]) and bits_equal(x["qs"], y["qs"])
    fwd = ag.Engine(board_size=N, tower_height=1, games=1, num_readouts=8, max_nodes_per_game=16)
    fwd.init_synthetic(0)
    cb = GpuNetForOracle(fwd).cb
    for r in out[2]:
        assert r["start"] == 0
        assert_selfplay_equal(r, tw.twin_selfplay(N, cb, R, seed, int(r["game_id"]), starts[3], -0.9, 0.0), r["game_id"])
    fwd.close()


def test_the_empty_board_is_the_one_entry_table_of_the_empty_position():
    """what lets game_start make one root_install call: no table and a table of the empty position alone are one run"""
    N, R, seed, games = 5, 16, 2, 5
    out = []
    for tbl in (None, [tw.random_start(N, 0, 0)]):
        eng = ag.Engine(board_size=N, tower_height=1, games=3, num_readouts=R, seed=seed, record_capacity_games=games + 8)
        eng.init_synthetic(0)
        if tbl:
            set_table(eng, tbl)
        assert eng.starts_count() == (1 if tbl else 0)
        out.append(play_sorted(eng, games))
        eng.close()
    (want, wst), (got, gst) = out
    assert gst["positions"] == wst["positions"] and gst["evals"] == wst["evals"]
    for x, y in zip(got, want):
        for k in ("game_id", "num_moves", "result", "was_resign", "resign_disabled", "short_searches"):
            assert x[k] == y[k], k
        assert np.float32(x["final_score"]) == np.float32(y["final_score"])
        assert (x["moves"] == y["moves"]).all() and bits_equal(x["pis"], y["pis"]) and bits_equal(x["qs"], y["qs"])


# ---------------------------------------------------------------- the arena

@pytest.mark.parametrize("N,R,games,slots", [(5, 16, 8, 4), (9, 16, 2, 4)])
def test_arena_external_networks_equal_the_twin(N, R, games, slots):
    black, white = OracleNet(N, 1, seed=0), OracleNet(N, 1, seed=5)
    starts = table(N)[2:]                # entries: White, Black, Black, White, set-up (White), ko
    eng = ag.Engine(board_size=N, tower_height=0, games=slots, num_readouts=R, seed=1, arena_mode=1,
                    external_network=1, record_capacity_games=games + 8)
    set_table(eng, starts)
    recs, st = play(eng, games, black.on_feats, white.on_feats)
    assert sorted(int(r["game_id"]) // 2 for r in recs) == list(range(games))
    evals = 0
    for r in recs:
        g = int(r["game_id"]) // 2
        assert r["start"] == g % len(starts)
        o = tw.twin_arena(N, black.cb, white.cb, R, -0.9, 1, g, starts[g % len(starts)])
        assert_arena_equal(r, o, g)
        evals += o["evals_black"] + o["evals_white"]
    assert st["evals"] == evals
    assert {starts[r["start"]].to_play for r in recs} == {1, -1}
    eng.close()
    black.close()
    white.close()


@pytest.mark.parametrize("N,tower,R,games,slots", [(5, 1, 16, 8, 6), (9, 1, 16, 2, 4)])
def test_arena_internal_networks_equal_the_twin(N, tower, R, games, slots):
    starts = table(N)
    eng = ag.Engine(board_size=N, tower_height=tower, games=slots, num_readouts=R, seed=3, arena_mode=1,
                    record_capacity_games=games + 8)
    eng.init_synthetic(0)
    eng.net_select(1)
    eng.init_synthetic(5)
    eng.net_select(0)
    set_table(eng, starts)
    recs, st = play(eng, games)
    fb = ag.Engine(board_size=N, tower_height=tower, games=1, num_readouts=8, max_nodes_per_game=16)
    fw = ag.Engine(board_size=N, tower_height=tower, games=1, num_readouts=8, max_nodes_per_game=16)
    fb.init_synthetic(0)
    fw.init_synthetic(5)
    bcb, wcb = GpuNetForOracle(fb).cb, GpuNetForOracle(fw).cb
    evals = 0
    for r in recs:
        g = int(r["game_id"]) // 2
        o = tw.twin_arena(N, bcb, wcb, R, -0.9, 3, g, starts[g % len(starts)])
        assert_arena_equal(r, o, g)
        evals += o["evals_black"] + o["evals_white"]
    assert st["evals"] == evals
    for e in (eng, fb, fw):
        e.close()


# ---------------------------------------------------------------- refusals

def test_refusals_leave_the_previous_table_in_force():
    N, R, seed = 5, 16, 9
    net = OracleNet(N, 1, seed=0)
    starts = table(N)
    eng = ag.Engine(board_size=N, tower_height=0, games=3, num_readouts=R, seed=seed, external_network=1,
                    record_capacity_games=16, **NEVER)
    set_table(eng, starts[:5])
    P, mgl = N * N, tw.max_game_length(N)

    def refused(boards, infos, hist, word):
        with pytest.raises(ag.AgzError) as e:
            eng.set_starts(boards=boards, info=infos, history=hist)
        assert e.value.status == BAD_ARGUMENT and word in str(e.value), str(e.value)
        assert "AGZ_" not in str(e.value).split(":", 1)[1]
        assert eng.starts_count() == 5

    def fresh():
        return tw.opos_arrays(starts[:3])

    # a bad scalar field (the checks of agz_analyze_start), naming the entry
    for field, value in (("to_play", 0), ("history_len", 8), ("n", -1), ("ko", P), ("last_move", P + 1), ("prev_move", -2)):
        b, i, h = fresh()
        setattr(i[1], field, value)
        refused(b, i, h, "entry 1")
    b, i, h = fresh()
    refused(b, i, None, "entry")                       # history_len > 0 without history boards
    # a finished start: two passes, or n >= max_game_length
    b, i, h = fresh()
    i[2].last_move = i[2].prev_move = P
    refused(b, i, h, "entry 2")
    b, i, h = fresh()
    i[0].n = mgl
    refused(b, i, h, "entry 0")
    # a bad board: a point outside {-1, 0, 1}, a group without a liberty, a stone on the ko point
    b, i, h = fresh()
    b[1, int(np.flatnonzero(b[1] == 0)[0])] = 2
    refused(b, i, h, "entry 1")
    b, i, h = fresh()
    b[2] = 0
    b[2, 0], b[2, 1], b[2, N] = -1, 1, 1
    refused(b, i, h, "entry 2")
    b, i, h = fresh()
    i[0].ko = int(np.flatnonzero(b[0] != 0)[0])
    refused(b, i, h, "entry 0")
    # the table that was in force all along still is: its games are the twin's
    recs, st = play(eng, 3, net.on_feats)
    for r in recs:
        gid = int(r["game_id"])
        assert_selfplay_equal(r, tw.twin_selfplay(N, net.cb, R, seed, gid, starts[gid % 5], -0.9, 0.0), gid)
    # the record ring holds games: neither setting nor clearing
    b, i, h = fresh()
    refused(b, i, h, "record ring")
    # ... nor while games of a run are being played (nothing recorded yet)
    other = ag.Engine(board_size=N, tower_height=1, games=2, num_readouts=R, seed=seed, record_capacity_games=8)
    other.init_synthetic(0)
    set_table(other, starts[:5])
    other.start(2)
    other.step(3)
    assert other.records_count() == 0
    with pytest.raises(ag.AgzError) as e:
        other.set_starts(boards=b, info=i, history=h)
    assert e.value.status == BAD_ARGUMENT and "still being played" in str(e.value) and other.starts_count() == 5
    other.close()
    with pytest.raises(ag.AgzError):
        eng.set_starts(None)
    assert eng.starts_count() == 5
    # ... nor while the replay arena holds them
    assert eng.replay_ingest_records(0, 3) == 3
    eng.records_clear()
    refused(b, i, h, "replay arena")
    eng.replay_clear()
    # together with the bench stagger: refused both ways round
    with pytest.raises(ag.AgzError):
        eng._ck(eng.L.agz_debug_set_stagger(eng.h, 3))
    eng.set_starts(boards=b, info=i, history=h)
    assert eng.starts_count() == 3
    eng.set_starts(None)
    assert eng.starts_count() == 0
    eng.start(1)
    eng._ck(eng.L.agz_debug_set_stagger(eng.h, 3))
    with pytest.raises(ag.AgzError) as e:
        eng.set_starts(boards=b, info=i, history=h)
    assert e.value.status == BAD_ARGUMENT and eng.starts_count() == 0
    eng.close()
    net.close()


# ---------------------------------------------------------------- replay

def twin_rows(o):
    """(features, pi, z) of every recorded ply of a twin game: or_get_feats of the positions it moved from"""
    f = np.stack([orc.feats(p).astype(np.float32).reshape(-1) for p in o["positions"]])
    return f, o["pis"], np.full(len(o["positions"]), o["result"], np.float32)


def test_replay_rebuilds_the_twins_positions():
    N, R, seed, games = 5, 16, 2, 8
    starts = table(N)
    eng = ag.Engine(board_size=N, tower_height=1, games=4, num_readouts=R, seed=seed, record_capacity_games=games + 8,
                    **NEVER)
    eng.init_synthetic(0)
    set_table(eng, starts)
    recs, st = play(eng, games)
    fwd = ag.Engine(board_size=N, tower_height=1, games=1, num_readouts=8, max_nodes_per_game=16)
    fwd.init_synthetic(0)
    twins = check_selfplay(recs, st, starts, N, R, seed, GpuNetForOracle(fwd).cb)
    recs = [r for r in recs if r["num_moves"] > 0]
    assert len(recs) >= 6
    want = {int(r["game_id"]): twin_rows(twins[int(r["game_id"])]) for r in recs}
    # agz_records_features
    for r in recs:
        got = eng.record_features(r["index"], r["num_moves"])
        assert bits_equal(got, want[int(r["game_id"])][0]), r["game_id"]
    # the arena: agz_replay_batch, agz_replay_batch_sym, agz_replay_sample
    packed = eng.records_packed().copy()
    assert eng.replay_ingest_records(0, games) == games
    order = [int(eng.replay_record(k)["game_id"]) for k in range(eng.replay_count())]

    def all_rows(e):
        g = np.concatenate([np.full(e.replay_record(k)["num_moves"], k, np.int64) for k in range(e.replay_count())])
        p = np.concatenate([np.arange(e.replay_record(k)["num_moves"], dtype=np.int32) for k in range(e.replay_count())])
        return g, p

    def expect(g, p, ids):
        rows = [(want[ids[a]][0][b], want[ids[a]][1][b], want[ids[a]][2][b]) for a, b in zip(g, p)]
        return (np.stack([x[0] for x in rows]), np.stack([x[1] for x in rows]), np.array([x[2] for x in rows], np.float32))

    g, p = all_rows(eng)
    wf, wp, wz = expect(g, p, order)
    f, pi, z = eng.replay_batch(g, p)
    assert bits_equal(f, wf) and bits_equal(pi, wp) and bits_equal(z, wz)
    sym = (np.arange(len(g)) % 8).astype(np.int32)
    f, pi, z = eng.replay_batch_sym(g, p, sym)
    for b in range(len(g)):
        assert bits_equal(f[b], symmetry.apply_features(wf[b], int(sym[b]), N))
        assert bits_equal(pi[b], symmetry.apply_policy(wp[b], int(sym[b]), N))
    assert bits_equal(z, wz)
    B = min(64, len(g))
    f, pi, z, sg, sp = eng.replay_sample(B, 1)
    eng.sync()
    sg, sp = sg.cpu().numpy(), sp.cpu().numpy()
    assert len({(int(a), int(b)) for a, b in zip(sg, sp)}) == B
    wf2, wp2, wz2 = expect(sg, sp, order)
    assert bits_equal(f.cpu().numpy(), wf2) and bits_equal(pi.cpu().numpy(), wp2) and bits_equal(z.cpu().numpy(), wz2)
    # hosts that keep the move lists: agz_replay_features_starts, directly and through ReplayBuffer
    byid = {int(r["game_id"]): r for r in recs}
    moves = np.concatenate([byid[i]["moves"] for i in sorted(byid)])
    offs, o = {}, 0
    for i in sorted(byid):
        offs[i] = o
        o += byid[i]["num_moves"]
    pairs = [(i, j) for i in sorted(byid) for j in range(byid[i]["num_moves"])]
    got = eng.replay_features(moves, [offs[i] for i, _ in pairs], [j for _, j in pairs],
                              start=[byid[i]["start"] for i, _ in pairs])
    assert bits_equal(got, np.stack([want[i][0][j] for i, j in pairs]))
    empty = eng.replay_features(moves[:1], [0], [0], start=[-1])            # -1: the empty board
    assert bits_equal(empty, orc.feats(orc.make_pos(N)).astype(np.float32).reshape(1, -1))
    with pytest.raises(ag.AgzError):
        eng.replay_features(moves[:1], [0], [0], start=[len(starts)])
    buf = ag.ReplayBuffer(ag.GoEnv(N), memory_size=10 ** 6)
    buf.extend([byid[i] for i in sorted(byid)])
    ids = sorted(byid)
    picked, _ = buf.sample_indices(40, np.random.default_rng(0))               # the (game slot, ply) pairs of the draw
    bf, bpi, bz = buf.sample(40, np.random.default_rng(0), eng)
    assert len(set(picked)) == 40
    for b, (gi, j) in enumerate(picked):
        f, p_, z_ = want[ids[gi]]
        assert bits_equal(bf[b], f[j]) and bits_equal(bpi[:, b], p_[j]) and bz[b] == z_[j], (b, gi, j)
    # pack -> agz_replay_ingest_packed on another engine with the same table: the same rows
    other = ag.Engine(board_size=N, tower_height=1, games=1, num_readouts=8, max_nodes_per_game=16)
    set_table(other, starts)
    assert other.replay_ingest(packed) == games
    order2 = [int(other.replay_record(k)["game_id"]) for k in range(other.replay_count())]
    g2, p2 = all_rows(other)
    wf3, wp3, wz3 = expect(g2, p2, order2)
    f, pi, z = other.replay_batch(g2, p2)
    assert bits_equal(f, wf3) and bits_equal(pi, wp3) and bits_equal(z, wz3)
    for e in (eng, fwd, other):
        e.close()


# ---------------------------------------------------------------- the Python loops

def api_position(env, opos):
    """the api.Position of an oracle position of random play: the same moves, played through the package"""
    pos = ag.Position(env, komi=opos.komi)
    for k in range(opos.recent_len):
        a = int(opos.recent_move[k])
        pos = pos.play_move(None if a == env.N * env.N else ag.from_flat(a, env))
    b, i, h = ag.api.position_arrays(pos)
    wb, wi, wh = tw.opos_arrays([opos])
    assert (b == wb[0]).all() and (h == wh[0][: len(h)]).all() and len(h) == opos.ndeltas
    for name, _ in ag._lib.PositionInfo._fields_:
        assert getattr(i, name) == getattr(wi[0], name), name
    return pos


def test_selfplay_and_evaluate_take_positions():
    N, R = 5, 16
    env = ag.GoEnv(N)
    ostarts = tw.random_starts(N, PLIES, seed=0)
    starts = [api_position(env, p) for p in ostarts]
    nn = ag.NeuralNet(env, tower_height=1, seed=0)
    players = ag.selfplay(env, nn, R, games=6, seed=2, game_id_base=0, starts=starts, **NEVER)
    cb = GpuNetForOracle(nn.engine).cb
    for gid, pl in enumerate(players):
        o = tw.twin_selfplay(N, cb, R, 2, gid, ostarts[gid % 6], -0.9, 0.0)
        assert pl.game_id == gid and pl.start is starts[gid % 6]
        assert [ag.to_flat(c, env) for c in pl.moves] == list(o["moves"]) and pl.result == o["result"]
        assert pl.root.position.n == ostarts[gid % 6].n + o["num_moves"]
        positions, pis, res = pl.extract_data()
        assert len(positions) == len(pis) == len(res) == o["num_moves"]
        for q, w in zip(positions, o["positions"]):
            assert (q._flat()[0] == w.board_np()).all() and q.n == w.n and q.to_play == w.to_play
    # the reference's path into the replay buffer: selfplay -> (extract_data) -> ReplayBuffer.  The buffer keeps each
    # player's table index and samples (features, pi, z) of the twin's positions through agz_replay_features_starts
    twins = [tw.twin_selfplay(N, cb, R, 2, gid, ostarts[gid % 6], -0.9, 0.0) for gid in range(6)]
    assert [pl.start_index for pl in players] == [gid % 6 for gid in range(6)]
    kept = [g for g in range(6) if twins[g]["num_moves"] > 0]
    buf = ag.ReplayBuffer(env, memory_size=10 ** 6)
    buf.extend([players[g] for g in kept])
    eng = ag.Engine(board_size=N, tower_height=1, games=1, num_readouts=8, max_nodes_per_game=16)
    eng.set_starts(starts)
    B = min(48, len(buf))
    picked, _ = buf.sample_indices(B, np.random.default_rng(3))
    bf, bpi, bz = buf.sample(B, np.random.default_rng(3), eng)
    for b, (gi, j) in enumerate(picked):
        o = twins[kept[gi]]
        assert bits_equal(bf[b], orc.feats(o["positions"][j]).astype(np.float32).reshape(-1)), (b, gi, j)
        assert bits_equal(bpi[:, b], o["pis"][j]) and bz[b] == o["result"], (b, gi, j)
    assert any(twins[kept[gi]]["positions"][j].n > j for gi, j in picked)        # rows that differ from an empty-board replay
    no_index = ag.SelfPlayPlayer.__new__(ag.SelfPlayPlayer)
    no_index.__dict__.update(players[kept[0]].__dict__)
    no_index.start_index = -1
    with pytest.raises(ValueError):
        ag.ReplayBuffer(env).push_record(no_index)
    eng.close()
    wn = ag.NeuralNet(env, tower_height=1, seed=5)
    ok, st = ag.evaluate(env, nn, wn, num_games=6, ro=R, seed=1, starts=starts, return_stats=True)
    wcb = GpuNetForOracle(wn.engine).cb
    assert len(st.records) == 6
    for r in st.records:
        g = int(r["game_id"]) // 2
        assert_arena_equal(r, tw.twin_arena(N, cb, wcb, R, -0.9, 1, g, ostarts[g % 6]), g)


TRAIN = dict(N=5, TOWER=1, R=16, SEED=3, num_games=8, slots=4, memory=60, B=8, start_after=8)


def test_train_with_starts_plays_the_twins_games():
    """train(..., starts=..., slots=4): every logged record is the twin's game from its start on the weights in force
    round by round -- games overlap training with 4 slots, so round r of a game (engine step start_step + r) runs on
    the weights left by the trainings of the steps before it.  The weights after each training come from the same
    schedule composed of single calls (the method of tests/test_gpu_train_batched.py), which train() must equal."""
    N, R, SEED = TRAIN["N"], TRAIN["R"], TRAIN["SEED"]
    env = ag.GoEnv(N)
    ostarts = tw.random_starts(N, PLIES, seed=0)
    starts = [api_position(env, p) for p in ostarts]
    nn0 = ag.NeuralNet(env, tower_height=TRAIN["TOWER"], seed=1)
    ref, snaps, start_step, _ = host_schedule(nn0, TRAIN, lambda eng: eng.set_starts(starts), targets_only=False)
    _, log = assert_train_equals_twin(
        env, nn0, TRAIN, (ref, snaps, start_step),
        lambda cb, gid, on_round: tw.twin_selfplay(N, cb, R, SEED, gid, ostarts[gid % 6], -0.9, 0.05, on_round=on_round),
        masked=False, starts=starts)
    for x, y in zip(log, ref):
        assert x["record"]["start"] == y["record"]["start"] == int(x["record"]["game_id"]) % 6
