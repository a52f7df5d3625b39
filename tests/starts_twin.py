"""Twins of the two reference loops for games that begin at a start position (TEST INFRASTRUCTURE).

twin_selfplay is selfplay.jl:1-45 with initialize_game!(player, start) at :14, twin_arena is the body of evaluate's loop
(neural_net.jl:113-148) with both players initialised on the start.  Both are written over the oracle's primitives
(or_player_*, or_select_leaf, or_incorporate_results, or_inject_noise, ...): the search rounds are spelled out here so
that the draw key (seed, game, position.n, select attempt) is in this file's hands -- or_player_initialize_game sets
draw.move = pos.n, and so does every twin below.  From the empty board they must equal or_selfplay_ex /
or_evaluate_game (tests/test_starts.py holds them to that)."""
import ctypes as C
import os
import shlex
import subprocess
import tempfile

import numpy as np

import alphago_jl_amd as ag
import hs
import orc

L = orc.lib()
L.or_draw_u64.restype = C.c_uint64
L.or_draw_u64.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64]
L.or_draw_u01.restype = C.c_double
L.or_draw_u01.argtypes = [C.c_uint64]
SITE_RESIGN = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- start positions

def max_game_length(N):
    return (N * N * 7) // 5


def random_start(N, plies, seed, komi=7.5, pass_every=0):
    """the position after `plies` seeded random legal moves from the empty board; pass_every = k > 0 makes every k-th
    ply a pass (never two in a row, so the position is not finished); plies < max_game_length"""
    assert 0 <= plies < max_game_length(N)
    rng = np.random.RandomState(seed)
    pos = orc.make_pos(N, komi=komi)
    legal = np.zeros(N * N + 1, np.int8)
    last_pass = False
    for k in range(plies):
        L.or_all_legal_moves(C.byref(pos), legal.ctypes.data_as(C.POINTER(C.c_int8)))
        cand = np.flatnonzero(legal[:N * N])
        want_pass = pass_every > 0 and (k + 1) % pass_every == 0 and not last_pass
        if len(cand) == 0 or want_pass:
            assert not last_pass, "the generator never passes twice in a row"
            a = N * N
        else:
            a = int(rng.choice(cand))
        rcode, pos = orc.play(pos, a)
        assert rcode == orc.OK
        last_pass = a == N * N
    assert not pos.done and pos.n == plies
    return pos.copy()


def random_starts(N, plies_list, seed=0, komi=7.5):
    """one start per entry of plies_list; every third one has passes in its history"""
    return [random_start(N, p, seed * 1000 + i, komi=komi, pass_every=5 if i % 3 == 2 else 0)
            for i, p in enumerate(plies_list)]


def setup_start(N, komi=0.5):
    """a set-up position: stones placed, n = 0, White to move, no history (a handicap game)"""
    b = np.zeros(N * N, np.int8)
    for r, c in ((1, 1), (N - 2, N - 2), (1, N - 2), (N - 2, 1)):
        b[r + N * c] = 1
    return orc.make_pos(N, board=b, n=0, komi=komi, to_play=orc.WHITE)


def ko_start(N, min_n=0):
    """a position of seeded random play with the ko point set"""
    for s in range(400):
        for plies in range(4, max_game_length(N) - 2):
            p = random_start(N, plies, 5000 + s)
            if p.ko >= 0 and p.n >= min_n:
                return p
            if p.n > 3 * N:
                break
    raise AssertionError("no ko position found")


def opos_arrays(positions):
    """oracle positions -> the (boards, info, history) of agz_analyze_start / agz_selfplay_set_starts"""
    N = positions[0].N
    P, B = N * N, len(positions)
    boards = np.zeros((B, P), np.int8)
    hist = np.zeros((B, 7, P), np.int8)
    infos = (ag._lib.PositionInfo * B)()
    for k, p in enumerate(positions):
        boards[k] = p.board_np()
        cur = boards[k].astype(np.int16)
        for d in range(p.ndeltas):
            cur = cur - np.frombuffer(p.deltas[d], np.int8, count=P)
            hist[k, d] = cur
        f = infos[k]
        f.n, f.to_play, f.ko = p.n, p.to_play, p.ko
        f.caps_black, f.caps_white = p.caps[0], p.caps[1]
        f.last_move = p.recent_move[p.recent_len - 1] if p.recent_len > 0 else -1
        f.prev_move = p.recent_move[p.recent_len - 2] if p.recent_len > 1 else -1
        f.history_len = p.ndeltas
        f.komi = p.komi
    return boards, infos, hist


# ---------------------------------------------------------------- the search round, with the draw key in our hands

def _net_call(net_cb, leaves, A):
    B = len(leaves)
    arr = (C.POINTER(orc.OPos) * B)(*[L.or_node_pos(x) for x in leaves])
    pi = np.zeros((B, A), np.float32)
    v = np.zeros(B, np.float32)
    net_cb(None, arr, B, orc.fptr(pi), orc.fptr(v))
    return pi, v


def _tree_search(env, root, draw, net_cb, A, par=8):
    """tree_search!, mcts_play.jl:73-98, on `root` with the draw stream `draw`"""
    leaves, failsafe = [], 0
    while len(leaves) < par and failsafe < 2 * par:
        failsafe += 1
        leaf = L.or_select_leaf(env, root, C.byref(draw))
        if L.or_node_is_done(env, leaf):
            L.or_backup_value(leaf, float(L.or_result(L.or_node_pos(leaf))), root)
            continue
        L.or_add_virtual_loss(leaf, root)
        leaves.append(leaf)
    if leaves:
        pi, v = _net_call(net_cb, leaves, A)
        for k, leaf in enumerate(leaves):
            L.or_revert_virtual_loss(leaf, root)
            L.or_incorporate_results(env, leaf, orc.fptr(pi[k]), A, float(v[k]), root)
    return len(leaves)


def _readouts(env, p, draw, net_cb, A, R, on_round=None):
    root = L.or_player_root(p)
    current = np.float32(L.or_node_N(root))
    evals = 0
    while np.float32(L.or_node_N(root)) < current + np.float32(R):
        if on_round:
            on_round()
        evals += _tree_search(env, root, draw, net_cb, A)
    return evals


def _new_draw(seed, game, p):
    pos = L.or_node_pos(L.or_player_root(p)).contents
    return orc.ODraw(seed, game, pos.n, 0)


def _root_pos(p):
    return L.or_node_pos(L.or_player_root(p)).contents


# ---------------------------------------------------------------- selfplay.jl:1-45 from a start

def twin_selfplay(N, net_cb, R, seed, game, start=None, threshold=-0.9, disable=0.05, on_round=None):
    """one self-play game of `game` from `start` (an OPos; None = the empty board with komi 7.5).  on_round() is called
    before every network round of the game, the pre-expansion included: round r of a game is the engine step r after
    the one its slot claimed it in, which lets a caller change the weights where train() changed them"""
    A = N * N + 1
    u = L.or_draw_u01(L.or_draw_u64(seed, game, 0, SITE_RESIGN, 0))          # selfplay.jl:9, keyed by the game alone
    disabled = u < disable
    p = L.or_player_new(N, net_cb, None, R, 0, -1.0 if disabled else threshold, seed, game)
    L.or_player_initialize_game(p, C.byref(start) if start is not None else None)
    env = L.or_player_env(p)
    start_n = _root_pos(p).n
    draw = _new_draw(seed, game, p)
    evals = 1
    if on_round:
        on_round()
    first = L.or_select_leaf(env, L.or_player_root(p), C.byref(draw))         # :16-20: the unexpanded root itself
    pi, v = _net_call(net_cb, [first], A)
    L.or_incorporate_results(env, first, orc.fptr(pi[0]), A, float(v[0]), first)
    positions, moves = [], []
    was_resign = 0
    while True:
        root = L.or_player_root(p)
        L.or_inject_noise(env, root, C.byref(draw))
        evals += _readouts(env, p, draw, net_cb, A, R, on_round)
        if L.or_player_should_resign(p):
            L.or_player_set_result(p, -_root_pos(p).to_play, 1)
            was_resign = 1
            break
        a = C.c_int(-1)
        if L.or_player_pick_move(p, C.byref(a)) != orc.OK:
            a = C.c_int(A - 1)
        positions.append(_root_pos(p).copy())
        assert L.or_player_play_move(p, a.value) == 1
        moves.append(a.value)
        draw = _new_draw(seed, game, p)
        if L.or_node_is_done(env, L.or_player_root(p)):
            L.or_player_set_result(p, L.or_result(L.or_node_pos(L.or_player_root(p))), 0)
            break
    n = L.or_player_num_moves(p)
    assert n == len(moves) == _root_pos(p).n - start_n
    fin = _root_pos(p).copy()
    rec = dict(num_moves=n, result=L.or_player_result(p), was_resign=was_resign, resign_disabled=int(disabled),
               final_score=0.0 if was_resign else float(L.or_score(C.byref(fin))),
               moves=np.array(moves, np.int16),
               pis=np.stack([orc.node_arr(L.or_player_search_pi(p, k), A).copy() for k in range(n)]) if n else None,
               qs=np.array([L.or_player_q(p, k) for k in range(n)], np.float32),
               evals=evals, positions=positions, final=fin)
    L.or_player_free(p)
    return rec


# ---------------------------------------------------------------- neural_net.jl:113-148 from a start

def twin_arena(N, black_cb, white_cb, R, threshold, seed, game, start=None):
    """one evaluate() game from `start`: the player whose colour is to move searches first"""
    A = N * N + 1
    black = L.or_player_new(N, black_cb, None, R, 1, threshold, seed, 2 * game)
    white = L.or_player_new(N, white_cb, None, R, 1, threshold, seed, 2 * game + 1)
    for p in (black, white):
        L.or_player_initialize_game(p, C.byref(start) if start is not None else None)
    env = L.or_player_env(black)
    moves, qs, positions = [], [], []
    evals = {1: 0, -1: 0}
    was_resign = 0
    while True:
        tp = _root_pos(black).to_play
        active, inactive = (black, white) if tp == 1 else (white, black)
        cb, gid = (black_cb, 2 * game) if tp == 1 else (white_cb, 2 * game + 1)
        draw = _new_draw(seed, gid, active)
        evals[tp] += _readouts(L.or_player_env(active), active, draw, cb, A, R)
        if L.or_player_should_resign(active):
            winner = -_root_pos(active).to_play
            L.or_player_set_result(active, winner, 1)
            L.or_player_set_result(inactive, winner, 1)
            was_resign = 1
            ender = gid
            break
        a = C.c_int(-1)
        if L.or_player_pick_move(active, C.byref(a)) != orc.OK:
            a = C.c_int(A - 1)
        qs.append(L.or_node_Q(L.or_player_root(active)))
        positions.append(_root_pos(active).copy())
        assert L.or_player_play_move(active, a.value) == 1
        assert L.or_player_play_move(inactive, a.value) == 1
        moves.append(a.value)
        if L.or_node_is_done(env, L.or_player_root(active)):
            winner = L.or_result(L.or_node_pos(L.or_player_root(active)))
            L.or_player_set_result(active, winner, 0)
            L.or_player_set_result(inactive, winner, 0)
            ender = gid
            break
    fin = _root_pos(black).copy()
    rec = dict(num_moves=len(moves), result=L.or_player_result(black), was_resign=was_resign,
               final_score=float(L.or_score(C.byref(fin))), moves=np.array(moves, np.int16),
               qs=np.array(qs, np.float32), evals_black=evals[1], evals_white=evals[-1], positions=positions,
               final=fin, ender=ender)
    L.or_player_free(black)
    L.or_player_free(white)
    return rec


# ---------------------------------------------------------------- the host simulator with a table

_sl = None


def starts_lib():
    """tests/hostsim/hostsim_starts.cpp (hostsim.cpp + hs_set_starts), built with the flags of the Makefile next to it"""
    global _sl
    if _sl is not None:
        return _sl
    base = hs.lib()
    d = os.path.join(ROOT, "tests", "hostsim")
    recipe = [ln for ln in open(os.path.join(d, "Makefile")).read().split("\n") if ln.startswith("\tg++")]
    assert len(recipe) == 1
    flags = [t for t in shlex.split(recipe[0])[1:] if t not in ("$<", "-o", "$@")]
    src = os.path.join(d, "hostsim_starts.cpp")
    deps = [src, os.path.join(d, "hostsim.cpp")] + [os.path.join(ROOT, "alphago.jl_amd", "csrc", h) for h in
                                                    ("agz_search.h", "agz_state.h", "agz_layout.h")]
    deps += [os.path.join(ROOT, "include", h) for h in ("agz.h", "agz_draws.h")]
    out = os.path.join(d, "libhostsim_starts.so")
    if not os.access(d, os.W_OK):
        out = os.path.join(tempfile.mkdtemp(prefix="hostsim_starts_"), "libhostsim_starts.so")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
        subprocess.run(["g++"] + flags + [src, "-o", out], check=True)
    S = C.CDLL(out)
    for name, fn in list(vars(base).items()):           # the prototypes hs.lib() declared, on this library's symbols
        if name.startswith("hs_"):
            g = getattr(S, name)
            g.restype, g.argtypes = fn.restype, fn.argtypes
    S.hs_set_starts.restype = None
    S.hs_set_starts.argtypes = [C.c_void_p, C.POINTER(C.c_int8), C.POINTER(ag._lib.PositionInfo), C.POINTER(C.c_int8),
                                C.c_int]
    S.hs_starts_count.restype = C.c_int
    S.hs_starts_count.argtypes = [C.c_void_p]
    S.hs_start_board_valid.restype = C.c_int
    S.hs_start_board_valid.argtypes = [C.c_void_p, C.POINTER(C.c_int8), C.c_int]
    _sl = S
    return S


class StartsSim(hs.Sim):
    """hs.Sim on the library that can set a table of start positions"""

    def __init__(self, **cfg):
        self.L = starts_lib()
        self.cfg = hs.default_config(**cfg)
        self.h = self.L.hs_create(C.byref(self.cfg))
        d = (C.c_int32 * 10)()
        self.L.hs_dims(self.h, d)
        (self.N, self.P, self.A, self.AP, self.cap, self.games, self.par, self.mgl, self.tau, self.maxd) = list(d)

    def set_starts(self, positions):
        if not positions:
            self.L.hs_set_starts(self.h, None, None, None, 0)
            return
        boards, infos, hist = opos_arrays(positions)
        self.L.hs_set_starts(self.h, hs.p8(boards), infos, hs.p8(hist), len(positions))

    def board_valid(self, board, ko=-1):
        b = np.ascontiguousarray(board, np.int8)
        return bool(self.L.hs_start_board_valid(self.h, hs.p8(b), ko))
