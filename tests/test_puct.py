"""PUCT rule options (agz_search_set_puct) on the host simulator, CPU only: (1) the scores of
hand-written nodes against the numpy restatement, bit for bit; (2) every descent of a 200-readout search predicted from
the rows before it runs; (3) the rule changes self-play and clearing it restores the unset run; (4) self-play under the
rule with each of the other search options."""
import numpy as np
import pytest

import hs
import puct_twin as pt
import selfplay_twin as tw

f32 = np.float32
C_PUCT = 0.96
SETTINGS = {"off": pt.OFF, "growth": (0, 0.0, 0.0, 19652.0), "growth1": (0, 0.0, 0.0, 1.0), "fpu": (1, 0.2, 0.05, 0.0),
            "fpu0": (1, 0.0, 0.0, 0.0), "both": (1, 0.2, 0.05, 19652.0)}


# ---------------------------------------------------------------- 1. scores

def hand_rows(A, kind, seed):
    rng = np.random.RandomState(seed)
    P = rng.rand(A).astype(f32)
    P = (P / P.sum()).astype(f32)
    N = np.zeros(A, f32)
    W = rng.uniform(-1, 1, A).astype(f32)
    if kind == "all":
        N[:] = rng.randint(1, 9, A)
    elif kind != "none":
        idx = rng.choice(A, max(2, A // 5), replace=False)
        N[idx] = rng.randint(1, 9, len(idx))
        N[A - 1] = 2                                  # the last action (the last lane of the last register row)
    W = (W * (1 + N)).astype(f32)
    if kind == "tiny":
        P[np.flatnonzero(N > 0)[0]] = f32(1e-12)      # (int64)(P * 2^30) truncates to 0
        P[np.flatnonzero(N == 0)[0]] = f32(1e-12)
    if kind == "negzero":
        W[np.flatnonzero(N > 0)[1]] = f32(-0.0)
        W[np.flatnonzero(N == 0)[0]] = f32(-0.0)
    return N, W, P


def hand_node(sim, is_root, tp, N, W, P, N_s, W_s):
    """a node of the simulator's tree with these rows, side to move and own statistics -> (node, W_s as stored)"""
    A = sim.A
    root = sim.tree_init(0, np.zeros(sim.P, np.int8), to_play=tp if is_root else -tp)
    node = root
    if not is_root:
        st, node = sim.op(hs.TOP_ADD_CHILD, node=root, a=3)
        assert st == 0 and node >= 0
    st, _ = sim.op(hs.TOP_INCORPORATE, node=node, probs=P, value=float(W_s) if is_root else 0.0, up_to=root)
    assert st == 0
    for k, row in enumerate((N, W, P)):
        sim.row(0, node, k)[:] = row
    if is_root:
        sim.L.hs_node_set_N(sim.h, 0, root, float(N_s))
    else:
        sim.row(0, root, 0)[3] = N_s
        sim.row(0, root, 1)[3] = W_s
    assert sim.meta(0, node).to_play == tp and sim.N_(0, node) == N_s
    return node, f32(sim.W_(0, node))


@pytest.mark.parametrize("N", [5, 9, 19])
def test_scores_equal_the_restatement(N):
    A = N * N + 1
    assert {5: 26, 9: 82, 19: 362}[N] == A
    sim = hs.Sim(board_size=N, games=1, num_readouts=8, max_nodes_per_game=16, c_puct=C_PUCT)
    checked = 0
    for ci, kind in enumerate(("none", "all", "mixed", "tiny", "negzero")):
        for is_root in (True, False):
            for tp in (1, -1):
                rows = hand_rows(A, kind, 100 * N + ci)
                N_s = f32(rows[0].sum() + 1)
                W_s = f32(-0.0) if (kind == "negzero" and not is_root) else f32(0.37 * N_s * (1 if ci % 2 else -1))
                node, W_st = hand_node(sim, is_root, tp, *rows, N_s, W_s)
                assert is_root or W_st.view(np.uint32) == W_s.view(np.uint32)
                off = None
                for name, setting in SETTINGS.items():
                    sim.set_puct(*setting)
                    got = sim.scores(node)
                    want = pt.puct_scores(*rows, N_s, W_st, tp, is_root, C_PUCT, setting)
                    assert (pt.bits64(got) == pt.bits64(want)).all(), (kind, is_root, tp, name)
                    if name == "off":
                        off = got
                        ref, _, _ = tw.action_scores(*rows, tp, N_s, C_PUCT)      # today's rule, as the other twins state it
                        assert (pt.bits64(got) == pt.bits64(ref)).all()
                    visited = rows[0] > 0
                    if setting[3] == 0:             # no growth: visited children keep their scores, bit for bit
                        assert (pt.bits64(got)[visited] == pt.bits64(off)[visited]).all()
                    elif visited.any():
                        assert (got[visited] != off[visited]).any()
                    if setting[0] and not visited.all() and name != "fpu0":
                        assert (got[~visited] != off[~visited]).any(), (kind, name)
                    checked += 1
    sim.set_puct(1, 0.2, 0.05, 0.0)              # r and r_root are told apart
    rows = hand_rows(A, "mixed", 7)
    node, W_st = hand_node(sim, True, 1, *rows, f32(40), f32(10))
    as_root = sim.scores(node)
    assert (pt.bits64(as_root) != pt.bits64(pt.puct_scores(*rows, f32(40), W_st, 1, False, C_PUCT, sim.setting))).any()
    assert checked == 5 * 2 * 2 * len(SETTINGS)
    sim.close()


def test_log_and_sqrt_restated():
    """the two restated functions against the library's own (the oracle exports them)"""
    import ctypes as C
    L = tw.L
    L.or_det_sqrt.restype = C.c_double
    L.or_det_sqrt.argtypes = [C.c_double]
    rng = np.random.RandomState(0)
    for x in list(rng.uniform(1e-9, 4.0, 200)) + [1.0, 2.0, 0.5, 1.0 + 1.0 / 19652.0, (801.0 + 19652.0) / 19652.0, 2.0 ** -30]:
        assert pt.agz_log(x) == L.or_det_log(float(x))
        assert pt.agz_sqrt(x) == L.or_det_sqrt(float(x))
    assert pt.agz_sqrt(0.0) == 0.0


# ---------------------------------------------------------------- 2. descents, predicted then checked

def searched_tree(par, setting, noise, readouts=200, seed=7, game_id=5):
    sim = hs.Sim(board_size=5, games=1, num_readouts=readouts, parallel_readouts=8, seed=seed, max_nodes_per_game=1024,
                 c_puct=C_PUCT)
    net = hs.PeakedNet(5)
    root = sim.tree_init(0, np.zeros(sim.P, np.int8))
    sim.L.hs_game_set(sim.h, 0, 0, float(game_id))
    sim.set_puct(*setting)
    total = dict(levels=0, unvisited=0, ties=0, terminal=0, phases=0, depth=0)
    noised = False
    while sim.game(0).rootN < readouts:
        want, counts, sh = pt.predict_phase(sim, par, C_PUCT, seed)
        st, n = sim.op(hs.TOP_SEARCH_SELECT, par=par)
        assert st == 0 and n == len(want)
        pt.assert_phase(sim, want, sh)
        for k in ("levels", "unvisited", "ties", "terminal"):
            total[k] += counts[k]
        total["phases"] += 1
        total["depth"] = max([total["depth"]] + [len(p) for p in want])
        if n:
            feats = np.zeros((n, 17 * sim.P), f32)
            sim.L.hs_tree_leaf_features(sim.h, 0, hs.pf(feats))
            pi, v = net(feats)
            sim.L.hs_set_batch_outputs(sim.h, hs.pf(pi), hs.pf(v), n)
        st, _ = sim.op(hs.TOP_SEARCH_POST)
        assert st == 0
        if noise and not noised:
            assert sim.op(hs.TOP_NOISE, node=root)[0] == 0
            noised = True
    return sim, total


@pytest.mark.parametrize("par", [1, 8])
@pytest.mark.parametrize("name,noise", [("both", False), ("growth1", False), ("fpu", True)])
def test_descents_are_predicted(par, name, noise):
    setting = SETTINGS[name]
    sim, total = searched_tree(par, setting, noise)
    print(f"par {par} {name} noise {noise}: {total}, nodes {sim.game(0).nodes_used}")
    assert total["depth"] >= 4 and total["levels"] > 200
    assert sim.puct_counts() == (total["levels"], total["unvisited"])
    assert 0 < total["unvisited"] < total["levels"] and total["ties"] > 0
    sim.close()


def test_the_rule_changes_the_tree():
    """the same search with and without the rule: another tree (so the predictions above are not the unchanged rule's)"""
    rows = {}
    for name in ("off", "fpu", "growth1"):
        sim, total = searched_tree(8, SETTINGS[name], False, readouts=96)
        rows[name] = sim.row(0, sim.game(0).root, 0).copy()
        assert (sim.puct_counts() == (0, 0)) == (name == "off")
        sim.close()
    assert (rows["fpu"] != rows["off"]).any() and (rows["growth1"] != rows["off"]).any()


# ---------------------------------------------------------------- 3 / 4. self-play

def selfplay(setting=None, clear=False, games=3, R=16, seed=3, configure=None):
    sim = hs.Sim(board_size=5, games=games, num_readouts=R, seed=seed, c_puct=C_PUCT, record_capacity_games=games + 4)
    net = hs.PeakedNet(5)
    if configure:
        configure(sim)
    if setting is not None:
        sim.set_puct(*setting)
    if clear:
        sim.set_puct(*pt.OFF)
    sim.start(games)
    for _ in range(20000):
        sim.step(net)
        if sim.L.hs_records_count(sim.h) >= games:
            break
    recs, counts, ctr = sim.records(), sim.puct_counts(), sim.counters()
    sim.close()
    assert len(recs) == games and ctr["pool_exhausted"] == 0
    return recs, counts


def same_records(a, b):
    return len(a) == len(b) and all(
        x["num_moves"] == y["num_moves"] and (x["moves"] == y["moves"]).all() and x["result"] == y["result"]
        and x["was_resign"] == y["was_resign"] and (x["pis"].view(np.uint32) == y["pis"].view(np.uint32)).all()
        and (x["qs"].view(np.uint32) == y["qs"].view(np.uint32)).all() for x, y in zip(a, b))


def test_the_rule_is_live_and_off_is_off():
    unset, c0 = selfplay()
    assert c0 == (0, 0)
    on, c1 = selfplay((1, 0.2, 0.0, 0.0))
    assert not same_records(on, unset), "the rule changed no move, pi or q"
    assert any(len(x["moves"]) != len(y["moves"]) or (x["moves"] != y["moves"]).any() for x, y in zip(on, unset))
    assert c1[0] > 0 and c1[1] > 0 and c1[1] < c1[0]
    cleared, c2 = selfplay((1, 0.2, 0.0, 19652.0), clear=True)
    assert same_records(cleared, unset) and c2 == (0, 0)
    # (1, 0, 0, 0) is not off: an unvisited child has its parent's value, not 0
    fpu0, c3 = selfplay((1, 0.0, 0.0, 0.0))
    assert not same_records(fpu0, unset) and c3[0] > 0
    growth, c4 = selfplay((0, 0.0, 0.0, 1.0))
    assert not same_records(growth, unset) and c4[0] > 0


@pytest.mark.parametrize("option", ["playout_cap", "forced_playouts", "gumbel", "starts"])
def test_selfplay_under_the_rule_with_each_option(option):
    def configure(sim):
        if option == "playout_cap":
            sim.set_playout_cap(4, 0.5)
        elif option == "forced_playouts":
            sim.set_forced_playouts(2.0, True)
        elif option == "gumbel":
            sim.set_gumbel(4, 50.0, 1.0)
        else:
            sim.set_starts(tw.random_starts(5, [0, 3, 6]))
    plain, _ = selfplay(configure=configure)
    recs, counts = selfplay((1, 0.2, 0.05, 19652.0), configure=configure)
    assert counts[0] > 0 and counts[1] > 0
    assert all(r["num_moves"] > 0 for r in recs)
    assert not same_records(recs, plain)
