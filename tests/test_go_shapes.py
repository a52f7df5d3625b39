"""The Go rules on hand-built shapes (tests/go_shapes.py): long groups, captures of more than one and two waves' worth
of stones, ko at corner, edge and centre, chosen bits of the legal mask, boards of every size class.  CPU only.

Three parties: the oracle (oracle/agz_oracle_go.c), a flood-fill restatement of the rules (go_shapes.ff_*) that the
oracle is held to on these boards, and the engine's rules (csrc/agz_search.h) run lane-serially by the host simulator,
held to the oracle.  Everything is integer and compared for equality.  tests/test_gpu_go_shapes.py runs the same
cases through the HIP kernels: the simulator cannot stand in for the wave primitives."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import go_shapes as gs
import hs
import orc

L = orc.lib()
KOMI = 7.5
FAMILY_NAMES = list(gs.FAMILIES)


# ---------------------------------------------------------------- the oracle's answers, computed once

def oracle_pos(case):
    return orc.make_pos(case.N, board=case.board, ko=case.ko, to_play=case.to_play, komi=KOMI)


def oracle_play(pos, a):
    """(status, board, ko, captured) of move a, in the engine's convention: an illegal move changes nothing"""
    rcode, nxt = orc.play(pos, int(a))
    if rcode != orc.OK:
        return 1, pos.board_np(), pos.ko, 0
    return 0, nxt.board_np(), nxt.ko, (nxt.caps[0] - pos.caps[0]) + (nxt.caps[1] - pos.caps[1])


@lru_cache(None)
def expected(name):
    """per case of the family: (legal int8[A], [(status, board, ko, captured) per tried move], score)"""
    out = []
    for c in gs.family(name):
        pos = oracle_pos(c)
        out.append((orc.legal_moves(pos), [oracle_play(pos, a) for a in c.moves], np.float32(L.or_score(C.byref(pos)))))
    return out


_sims = {}


def sim_of(N):
    if N not in _sims:
        _sims[N] = hs.Sim(board_size=N, games=1, num_readouts=8, max_nodes_per_game=16)
    return _sims[N]


def assert_rules_equal(backend_of, cases, want):
    """go_legal / go_play / go_score of backend_of(N) on every case, one call per entry and size, against `want`"""
    checked = 0
    for N in sorted({c.N for c in cases}):
        idx = [k for k, c in enumerate(cases) if c.N == N]
        be = backend_of(N)
        boards = np.stack([cases[k].board for k in idx])
        tp = np.array([cases[k].to_play for k in idx], np.int8)
        ko = np.array([cases[k].ko for k in idx], np.int32)
        legal = be.go_legal(boards, tp, ko)
        score = be.go_score(boards, np.full(len(idx), KOMI, np.float32))
        rows = [(j, m) for j, k in enumerate(idx) for m in range(len(cases[k].moves))]
        sel = [j for j, _ in rows]
        moves = np.array([cases[idx[j]].moves[m] for j, m in rows], np.int32)
        bo, ko_o, nc, st = be.go_play(boards[sel], tp[sel], ko[sel], moves)
        for j, k in enumerate(idx):
            assert (legal[j] == want[k][0]).all(), (cases[k].name, np.flatnonzero(legal[j] != want[k][0]))
            assert score[j] == want[k][2], (cases[k].name, score[j], want[k][2])
        for r, (j, m) in enumerate(rows):
            w, name = want[idx[j]][1][m], (cases[idx[j]].name, int(moves[r]))
            assert st[r] == w[0], name
            assert (bo[r] == w[1]).all(), name
            assert ko_o[r] == w[2] and nc[r] == w[3], (name, ko_o[r], nc[r], w[2:])
            checked += 1
    return checked


# ---------------------------------------------------------------- the oracle against the restatement

@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_oracle_matches_flood_fill(name):
    cases, want = gs.family(name), expected(name)
    assert len(cases) > 0
    for c, (legal, plays, score) in zip(cases, want):
        assert (legal == gs.ff_legal(c.board, c.N, c.to_play, c.ko)).all(), c.name
        assert score == gs.ff_score(c.board, c.N, KOMI), c.name
        for a, (st, board, ko, ncap) in zip(c.moves, plays):
            fst, fboard, fko, fcap = gs.ff_play(c.board, c.N, c.to_play, c.ko, a)
            assert (st, ko, ncap) == (fst, fko, fcap) and (board == fboard).all(), (c.name, a)
            if a < c.N * c.N:
                assert legal[a] == (st == 0), (c.name, a)


# ---------------------------------------------------------------- the simulator against the oracle

@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_hostsim_matches_oracle(name):
    cases = gs.family(name)
    assert assert_rules_equal(sim_of, cases, expected(name)) == sum(len(c.moves) for c in cases)


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_hostsim_root_mask_matches_oracle(name):
    """every case as a tree root: the packed legal mask node_init_from_scratch writes, word by word"""
    for c, (legal, _, _) in zip(gs.family(name), expected(name)):
        sim = sim_of(c.N)
        root = sim.tree_init(0, c.board, to_play=c.to_play, ko=c.ko, komi=KOMI)
        assert (sim.legal(0, root) == legal).all(), c.name
        assert (sim.board(0, root) == c.board).all(), c.name


def validity_boards(N):
    """[(board, ko, valid)]: the spiral whose groups keep their one liberty, the same with the inner end filled by
    either colour, with a 2 on the inner end, and with the ko point on a stone"""
    out = []
    for colour in (-1, 1):
        board, inner = gs.spiral_board(N, colour)
        out.append((board, -1, True))
        out.append((board, inner, True))                   # (a ko point that is empty)
        for v in (1, -1, 2):
            b = board.copy()
            b[inner] = v
            out.append((b, -1, False))
        out.append((board, 0, False))
    return out


@pytest.mark.parametrize("N", gs.SPIRAL_SIZES)
def test_hostsim_root_validation(N):
    for board, ko, ok in validity_boards(N):
        assert gs.valid(board, N) == (ok or ko >= 0)
        assert sim_of(N).board_valid(board, ko) == ok, (N, ko, ok)


# ---------------------------------------------------------------- the census: what the fixtures reach, asserted

def census():
    cap, groups, ko_sites, refused, mask = {}, set(), set(), 0, {}
    for name in FAMILY_NAMES:
        cases, want = gs.family(name), expected(name)
        by_name = {c.name: k for k, c in enumerate(cases)}
        for k, c in enumerate(cases):
            for m, (a, (st, _, ko, ncap)) in enumerate(zip(c.moves, want[k][1])):
                if st == 0 and ncap:
                    cap[c.N] = max(cap.get(c.N, 0), ncap)
                    groups.add(gs.captured_groups(c.board, c.N, c.to_play, a))
                if st == 0 and ko >= 0:
                    ko_sites.add((len(gs.neighbours(c.N, a)), c.to_play))
                if st == 1 and a == c.ko and by_name.get(c.name + "-noko") is not None:
                    twin = by_name[c.name + "-noko"]
                    assert cases[twin].moves[m] == a and (cases[twin].board == c.board).all()
                    refused += want[twin][1][m][0] == 0        # the same retake without the ko: legal
            if name == "mask_edges":
                for a in gs.edge_actions(c.N) + [c.N * c.N]:
                    mask.setdefault((c.N, a), set()).add(int(want[k][0][a]))
    depth = {}
    for name, stones in (("spirals", True), ("spiral_scores", False)):
        for c in gs.family(name):
            key = (c.N, "stones" if stones else "empty")
            depth[key] = max(depth.get(key, 0), max(gs.component_depths(c.board, c.N, stones)))
    return dict(cap=cap, groups=groups, ko_sites=ko_sites, refused=refused, mask=mask, depth=depth)


def test_census():
    got = census()
    total = sum(len(gs.family(n)) for n in FAMILY_NAMES)
    tried = sum(len(c.moves) for n in FAMILY_NAMES for c in gs.family(n))
    print(f"\ncensus of tests/go_shapes.py: {total} positions, {tried} tried moves")
    for n in FAMILY_NAMES:
        sizes = sorted({c.N for c in gs.family(n)})
        print(f"  {n:16s} {len(gs.family(n)):5d} positions, N = {sizes}")
    print("  largest capture by a tried move, per size:", dict(sorted(got["cap"].items())))
    print("  component depth from the smallest point:", dict(sorted(got["depth"].items())))
    print("  groups captured by one move:", sorted(got["groups"]))
    print("  ko set by a move with (neighbours, colour):", sorted(got["ko_sites"]))
    print("  retakes refused by ko (legal without it):", got["refused"])
    flags = {N: sum(v == {0, 1} for (n, a), v in got["mask"].items() if n == N and a < N * N) for N in gs.MASK_SIZES}
    print("  mask-edge actions seen both legal and illegal, per size:", flags)
    assert max(got["cap"].values()) > 128 and any(64 < v <= 128 for v in got["cap"].values())
    assert got["cap"][19] == 198 and got["cap"][9] >= 48
    assert got["depth"][(19, "stones")] >= 190 and got["depth"][(19, "empty")] >= 190
    assert got["ko_sites"] == {(k, colour) for k in (2, 3, 4) for colour in (1, -1)}
    assert got["refused"] > 0
    assert {1, 2, 3, 4} <= got["groups"]
    for N in gs.MASK_SIZES:
        P = N * N
        assert flags[N] == len(gs.edge_actions(N)), (N, flags)
        assert got["mask"][(N, P)] == {1}                   # pass: always legal
        for m in range(32, P, 32):
            assert got["mask"][(N, m - 1)] == got["mask"][(N, m)] == {0, 1}
    for N, (path, comp) in gs.SPIRAL_STONES.items():
        board, inner = gs.spiral_board(N, -1)
        assert int((board == -1).sum()) == path and int((board == 1).sum()) == comp and board[inner] == 0


# ---------------------------------------------------------------- the scripted games

@lru_cache(None)
def game_positions(N):
    """the oracle's positions of the scripted game, the start included: every move legal, no capture before the one
    at the inner end, never two passes in a row"""
    moves, capture = gs.scripted_game(N)
    pos = orc.make_pos(N, komi=KOMI)
    out = [pos.copy()]
    for k, a in enumerate(moves):
        rcode, nxt = orc.play(pos, a)
        assert rcode == orc.OK, (N, k, a)
        taken = (nxt.caps[0] - pos.caps[0]) + (nxt.caps[1] - pos.caps[1])
        assert taken == (gs.SPIRAL_STONES[N][0] if k == capture else 0), (N, k)
        assert not nxt.done
        pos = nxt
        out.append(pos.copy())
    assert capture == 2 * gs.SPIRAL_STONES[N][0] and moves.count(N * N) > 1 and len(moves) == capture + 13
    return out


@pytest.mark.parametrize("N", [9, 19])
def test_scripted_game_on_hostsim(N):
    """the game move by move through go_play / go_legal / go_score, and along one line of the tree (node_expand_child,
    node_init_from_scratch, the packed mask).  The simulator has no entry for replay features: that path is
    tests/test_gpu_go_shapes.py's."""
    moves, capture = gs.scripted_game(N)
    pos = game_positions(N)
    P = N * N
    sim = sim_of(N)
    boards = np.stack([p.board_np() for p in pos])
    tp = np.array([p.to_play for p in pos], np.int8)
    ko = np.array([p.ko for p in pos], np.int32)
    legal = sim.go_legal(boards, tp, ko)
    score = sim.go_score(boards, np.full(len(pos), KOMI, np.float32))
    bo, ko_o, nc, st = sim.go_play(boards[:-1], tp[:-1], ko[:-1], np.array(moves, np.int32))
    for k, p in enumerate(pos):
        assert (legal[k] == orc.legal_moves(p)).all(), k
        assert score[k] == L.or_score(C.byref(p)), k
    assert (st == 0).all() and (bo == boards[1:]).all() and (ko_o == ko[1:]).all()
    assert nc[capture] == gs.SPIRAL_STONES[N][0] and nc.sum() == nc[capture]
    tree = hs.Sim(board_size=N, games=1, num_readouts=8, max_nodes_per_game=len(moves) + 2)
    node = tree.tree_init(0, np.zeros(P, np.int8), komi=KOMI)
    for k, a in enumerate(moves):
        status, node = tree.op(hs.TOP_ADD_CHILD, node=node, a=a)
        assert status == 0 and node >= 0, k
        m, p = tree.meta(0, node), pos[k + 1]
        assert (tree.board(0, node) == boards[k + 1]).all(), k
        assert (m.ko, m.caps_b, m.caps_w, m.to_play, m.n) == (p.ko, p.caps[0], p.caps[1], p.to_play, p.n), k
        assert (tree.legal(0, node) == legal[k + 1]).all(), k
    tree.close()
