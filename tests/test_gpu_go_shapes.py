"""The hand-built shapes of tests/go_shapes.py on the device: the HIP rules kernels, the tree's child expansion with
its packed legal mask, device replay across the big captures, and root validation, against the oracle.  Integers,
compared for equality.  tests/test_go_shapes.py holds the oracle to a second reference on the same cases and runs them
through the host simulator, which shares agz_search.h but not the wave primitives of agz_engine.hip: 64-lane strides,
shuffle reductions, ballots and LDS atomics are what this file is about."""
import ctypes as C

import numpy as np
import pytest

import alphago_jl_amd as ag
import go_shapes as gs
import orc
from test_go_shapes import (FAMILY_NAMES, KOMI, assert_rules_equal, expected, game_positions, oracle_play, oracle_pos,
                            validity_boards)

pytestmark = pytest.mark.gpu
L = orc.lib()

_engines = {}


def engine_of(N):
    """one engine per board size for the whole file: no network to speak of, one tree slot of 2A + 2 nodes"""
    if N not in _engines:
        _engines[N] = ag.Engine(board_size=N, games=1, tower_height=0, num_readouts=8,
                                max_nodes_per_game=max(16, 2 * (N * N + 1) + 2))
    return _engines[N]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


# ---------------------------------------------------------------- go_legal / go_play / go_score

@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_rules_match_oracle(name):
    cases = gs.family(name)
    assert assert_rules_equal(engine_of, cases, expected(name)) == sum(len(c.moves) for c in cases)


@pytest.mark.parametrize("N", [9, 19])
def test_scripted_game_by_rules(N):
    moves, capture = gs.scripted_game(N)
    pos = game_positions(N)
    cases = [gs.Case(f"game/N{N}/{k}", N, p.board_np(), int(p.to_play), int(p.ko), moves[k:k + 1] or [N * N])
             for k, p in enumerate(pos)]
    want = [(orc.legal_moves(p), [oracle_play(p, a) for a in c.moves], np.float32(L.or_score(C.byref(p))))
            for p, c in zip(pos, cases)]
    assert want[capture][1][0][3] == gs.SPIRAL_STONES[N][0]
    assert assert_rules_equal(engine_of, cases, want) == len(cases)


# ---------------------------------------------------------------- the tree path

def walk(eng, node, pos):
    """maybe_add_child for every action of `node`, whose position is `pos`: a legal action yields the oracle's next
    position, every other is refused and adds no node.  -> {action: (child, its position)}"""
    A = pos.A
    legal = orc.legal_moves(pos)
    out, made = {}, []
    for a in range(A):
        if not legal[a]:
            with pytest.raises(ag.IllegalMove):
                eng.maybe_add_child(0, node, a)
            continue
        child = eng.maybe_add_child(0, node, a)
        rcode, nxt = orc.play(pos, a)
        assert rcode == orc.OK
        info = eng.node_info(0, child)
        assert (eng.node_board(0, child) == nxt.board_np()).all(), a
        assert (info.parent, info.fmove, info.pos.n) == (node, a, nxt.n), a
        assert (info.pos.ko, info.pos.caps_black, info.pos.caps_white, info.pos.to_play) == \
            (nxt.ko, nxt.caps[0], nxt.caps[1], nxt.to_play), a
        made.append(child)
        out[a] = (child, nxt)
    children = eng.node_children(0, node)
    assert ((children >= 0) == (legal != 0)).all()
    assert [int(children[a]) for a in out] == made
    assert made == list(range(made[0], made[0] + len(made))), "a refused action took a node"
    return out


def walk_root(case, then=None):
    """the walk over the root of `case`; then = an action: the same walk over the child behind it"""
    eng = engine_of(case.N)
    pos = oracle_pos(case)
    root = eng.tree_init(0, case.board, to_play=case.to_play, ko=case.ko, komi=KOMI)
    kids = walk(eng, root, pos)
    if then is not None:
        child, nxt = kids[then]
        return kids, walk(eng, child, nxt)
    return kids, None


@pytest.mark.parametrize("N", [9, 19])
def test_tree_children_of_spirals(N):
    """the un-rotated spiral, both colourings, both sides to move: the root has two children, the pass and the capture
    of the other arm; behind the capture every action of the child is walked"""
    path, comp, inner = gs.spiral_arms(N)
    picked = [c for c in gs.spirals((N,), images=(0,))]
    assert len(picked) == 4
    for c in picked:
        kids, grand = walk_root(c, then=inner)
        assert sorted(kids) == [inner, N * N]
        taken = kids[inner][1].caps[0] + kids[inner][1].caps[1]
        assert taken in gs.SPIRAL_STONES[N] and len(grand) == taken + 1


@pytest.mark.parametrize("N", gs.MASK_SIZES)
def test_tree_children_of_mask_edges(N):
    """the eye boards: the children are the eyes with Black to move and the pass alone with White to move, so every bit
    next to a word edge of the packed mask is read both set and clear"""
    for c in gs.mask_edges((N,)):
        if "swap" in c.name:
            continue
        kids, _ = walk_root(c)
        eyes = [int(p) for p in np.flatnonzero(c.board == 0)]
        assert sorted(kids) == (eyes if c.to_play == 1 else []) + [N * N], c.name


def test_tree_children_of_ko():
    """a ko at the corner, the edge and the centre: behind the capture the child's mask has the ko point clear, and
    the grandchildren are the oracle's"""
    cases = {c.name: c for c in gs.family("ko_and_captures")}
    for name in ("shape/N9/corner/ko/tp+1/s0", "shape/N9/edge/ko/tp+1/s5/swap", "shape/N5/centre/ko/tp+1/s3"):
        c = cases[name]
        a = c.moves[0]
        kids, grand = walk_root(c, then=a)
        ko = kids[a][1].ko
        assert ko >= 0 and c.board[ko] == -c.to_play and ko not in grand


# ---------------------------------------------------------------- replay across the captures

@pytest.mark.parametrize("N", [9, 19])
def test_replay_features_of_scripted_game(N):
    """device replay of the scripted game, every ply from eight before the capture to the end: the history planes
    straddle the capture of 48 / 198 stones"""
    moves, capture = gs.scripted_game(N)
    pos = game_positions(N)
    plies = list(range(capture - 8, len(moves) + 1))
    got = engine_of(N).replay_features(np.array(moves, np.int16), [0] * len(plies), plies)
    for row, j in zip(got, plies):
        assert (row.reshape(17, -1) == orc.feats(pos[j])).all(), j


# ---------------------------------------------------------------- root validation

@pytest.mark.parametrize("N", [9, 19])
def test_root_validation(N):
    """set_starts runs root_board_valid per entry on the device: the spiral with its one liberty is taken, the spiral
    with the inner end filled (no liberty 47 / 197 points from the smallest point), a 2, or the ko on a stone is not"""
    eng = engine_of(N)
    for board, ko, ok in validity_boards(N):
        info = ag._lib.PositionInfo()
        info.n, info.to_play, info.ko, info.last_move, info.prev_move, info.komi = 0, 1, ko, -1, -1, KOMI
        if ok:
            eng.set_starts(boards=board[None], info=[info])
            assert eng.starts_count() == 1
            eng.set_starts(None)
        else:
            with pytest.raises(ag.AgzError) as e:
                eng.set_starts(boards=board[None], info=[info])
            assert e.value.status == ag._lib.BAD_ARGUMENT and "entry 0" in str(e.value)
        assert eng.starts_count() == 0
