"""Twin of the self-play loop under the Gumbel root search (TEST INFRASTRUCTURE; agz_selfplay_set_gumbel).

The scores, the Sequential Halving schedule, the halving, the root pick, the move and the target row are restated here in
numpy float64, with float32 exactly where the definitions say float32, over the oracle's or_det_log / or_det_exp /
or_draw_u64 / or_draw_u01.  The descent is forced_twin.select_leaf's restatement of mcts.jl:108-138 with a root action
given by the caller.  twin_selfplay_gumbel is cap_twin.twin_selfplay_cap with those: no noise in a Gumbel search, select
phases that stop at the phase end, the survivor with the largest s as the move, gumbel_pi as the row.  Also here: the
host simulator with the setter, the counters, the slot state and the single-node gumbel_pi entry."""
import ctypes as C
import os
import re
import shlex
import subprocess
import tempfile

import numpy as np

import cap_twin as ct
import forced_twin as ft
import hs
import orc
import starts_twin as tw
from starts_twin import L, _net_call, _new_draw, _root_pos

ROOT = tw.ROOT
f32, f64 = np.float32, np.float64
NO_LOGIT = -1.0e30
PAR = 8

L.or_det_log.restype = C.c_double
L.or_det_log.argtypes = [C.c_double]
L.or_det_exp.restype = C.c_double
L.or_det_exp.argtypes = [C.c_double]


def _site_gumbel():
    hdr = open(os.path.join(ROOT, "include", "agz_draws.h")).read()
    return int(re.search(r"#define AGZ_SITE_GUMBEL (\d+)u", hdr).group(1))


SITE_GUMBEL = _site_gumbel()


# ---------------------------------------------------------------- the scores, restated

def logit(p):
    p = f32(p)
    return L.or_det_log(float(p)) if p > 0 else NO_LOGIT


def gumbel_g(seed, game, n_root, a):
    u = L.or_draw_u01(L.or_draw_u64(seed, game, n_root, SITE_GUMBEL, a))
    return -L.or_det_log(-L.or_det_log(u))


def sigma(N, W, tp, c_visit, c_scale):
    """sigma(a) for every action: float32 qs, the rest float64 in the stated order"""
    N, W = np.asarray(N, f32), np.asarray(W, f32)
    qs = (W / (f32(1) + N)) * f32(tp)
    assert qs.dtype == np.float32
    maxN = f64(N.max())
    return ((f64(c_visit) + maxN) * f64(c_scale)) * (f64(0.5) + f64(0.5) * qs.astype(f64))


def score(seed, game, n_root, a, N, W, P, tp, c_visit, c_scale):
    """s(a) = (g(a) + logit(a)) + sigma(a)"""
    return (gumbel_g(seed, game, n_root, a) + logit(P[a])) + float(sigma(N, W, tp, c_visit, c_scale)[a])


def gumbel_pi(N, W, P, legal, tp, c_visit, c_scale):
    """the target row: softmax over the legal actions of logit + sigma, float32[A]"""
    A = len(N)
    sg = sigma(N, W, tp, c_visit, c_scale)
    lg = np.asarray(legal) != 0
    x = [logit(P[a]) + float(sg[a]) if lg[a] else None for a in range(A)]
    mx = max(v for v in x if v is not None)
    e = [L.or_det_exp(v - mx) if v is not None else 0.0 for v in x]
    s = 0.0
    for v in e:
        s += v
    return (np.array(e, f64) / f64(s)).astype(f32), np.array([v if v is not None else np.nan for v in x])


def schedule(n, m0):
    """[(m_p, Q_p)] of a search of budget n with m0 survivors"""
    P = 1
    while (1 << P) < m0:
        P += 1
    out, m, left = [], m0, n
    while left > 0:
        q = min(max(1, n // (P * m)) * m, left)
        out.append((m, q))
        left -= q
        m = 1 if m == 1 else max(2, m // 2)
    return out


class State:
    """the Sequential Halving state of one search"""

    def __init__(self, act, n, rootN, target):
        self.act = list(act)
        self.m0 = len(act)
        self.budget = n
        self.P = 1
        while (1 << self.P) < len(act):
            self.P += 1
        self.halvings = 0
        self.end = self.phase_end(rootN, target)

    def phase_end(self, rootN, target):
        m = len(self.act)
        q = max(1, self.budget // (self.P * m)) * m
        return f32(rootN) + f32(min(q, int(f32(target) - f32(rootN))))


def begin(seed, game, n_root, P, legal, m, rootN, target):
    """the m_0 legal actions with the largest g + logit, the lower action on ties, in that order"""
    cand = [(-(gumbel_g(seed, game, n_root, a) + logit(P[a])), a) for a in range(len(P)) if legal[a]]
    cand.sort()
    act = [a for _, a in cand[:min(m, len(cand))]]
    return State(act, int(f32(target) - f32(rootN)), rootN, target)


def halve(st, seed, game, n_root, N, W, P, tp, c_visit, c_scale, rootN, target):
    sc = sorted((-score(seed, game, n_root, a, N, W, P, tp, c_visit, c_scale), a) for a in st.act)
    m = len(st.act)
    keep = 1 if m == 1 else max(2, m // 2)
    st.act = [a for _, a in sc[:keep]]
    st.halvings += 1
    st.end = st.phase_end(rootN, target)


def root_pick(st, N):
    """the survivor with the fewest visits, in flight included; the first in stored order on ties"""
    best = st.act[0]
    for a in st.act[1:]:
        if N[a] < N[best]:
            best = a
    return best


def best_survivor(st, seed, game, n_root, N, W, P, tp, c_visit, c_scale):
    return min((-score(seed, game, n_root, a, N, W, P, tp, c_visit, c_scale), a) for a in st.act)[1]


# ---------------------------------------------------------------- the descent

def select_leaf(env, root, draw, root_action=-1):
    """forced_twin.select_leaf (k = 0) with the root action given: after the pass-first rule, depth 0 takes it -- no
    score, no tie draw there; draw.sel advances once per descent all the same"""
    A = env.contents.A
    ps = A - 1
    cur, depth = root, 0
    cas = np.zeros(A, f64)
    legal = np.zeros(A, np.int8)
    while True:
        L.or_node_set_N(cur, f32(L.or_node_N(cur)) + f32(1))
        if not L.or_node_is_expanded(cur):
            break
        pos = L.or_node_pos(cur)
        cN = orc.node_arr(L.or_node_child_N(cur), A)
        rl = pos.contents.recent_len
        if rl != 0 and pos.contents.recent_move[rl - 1] == ps and cN[ps] == 0:
            pick = ps
        elif depth == 0 and root_action >= 0:
            pick = root_action
        else:
            L.or_child_action_score(env, cur, cas.ctypes.data_as(C.POINTER(C.c_double)))
            L.or_all_legal_moves(pos, legal.ctypes.data_as(C.POINTER(C.c_int8)))
            lg = legal != 0
            best = cas[lg].max()
            possible = np.flatnonzero(lg & (cas == best))
            pick = int(possible[0])
            if len(possible) > 1:
                bits = L.or_draw_u64(draw.seed, draw.game, draw.move, ft.SITE_PUCT_TIE, draw.sel * 1024 + depth)
                pick = int(possible[ft._index(bits, len(possible))])
        nx = C.c_void_p()
        assert L.or_maybe_add_child(env, cur, pick, C.byref(nx)) == orc.OK
        cur = nx.value
        depth += 1
    draw.sel += 1
    return cur


def _rows(root, A):
    return (orc.node_arr(L.or_node_child_N(root), A), orc.node_arr(L.or_node_child_W(root), A),
            orc.node_arr(L.or_node_child_prior(root), A))


def _legal(root, A):
    legal = np.zeros(A, np.int8)
    L.or_all_legal_moves(L.or_node_pos(root), legal.ctypes.data_as(C.POINTER(C.c_int8)))
    return legal


def _gumbel_readouts(env, pl, draw, net_cb, A, R, m, cv, cs, seed, game, info, on_round=None):
    """one Gumbel search of the player's root: R root visits by Sequential Halving.  Returns (evals, state)"""
    root = L.or_player_root(pl)
    pos = _root_pos(pl)
    n_root, tp = pos.n, pos.to_play
    start = f32(L.or_node_N(root))
    target = start + f32(R)
    st, evals = None, 0
    while f32(L.or_node_N(root)) < target:
        if on_round:
            on_round()
        rootN = f32(L.or_node_N(root))
        if L.or_node_is_expanded(root):
            N, W, P = _rows(root, A)
            if st is None:
                st = begin(seed, game, n_root, P, _legal(root, A), m, rootN, target)
                info["begun"] += 1
                info["reused"] += bool(rootN > 0)
                info["sched"].append((int(target - rootN), len(st.act)))
            elif not rootN < st.end and st.end < target:
                halve(st, seed, game, n_root, N, W, P, tp, cv, cs, rootN, target)
                info["halved"] += 1
        leaves, failsafe = [], 0
        while len(leaves) < PAR and failsafe < 2 * PAR and (st is None or f32(L.or_node_N(root)) < st.end):
            failsafe += 1
            ra = root_pick(st, orc.node_arr(L.or_node_child_N(root), A)) if st is not None else -1
            leaf = select_leaf(env, root, draw, ra)
            if L.or_node_is_done(env, leaf):
                L.or_backup_value(leaf, float(L.or_result(L.or_node_pos(leaf))), root)
                continue
            L.or_add_virtual_loss(leaf, root)
            leaves.append(leaf)
        if st is not None and len(leaves) < PAR and failsafe < 2 * PAR:
            info["cuts"] += 1
        if leaves:
            pi, v = _net_call(net_cb, leaves, A)
            for i, leaf in enumerate(leaves):
                L.or_revert_virtual_loss(leaf, root)
                info["dups"] += bool(st is not None and L.or_node_is_expanded(leaf))
                L.or_incorporate_results(env, leaf, orc.fptr(pi[i]), A, float(v[i]), root)
        evals += len(leaves)
    if st is not None:
        assert f32(L.or_node_N(root)) == target, "a Gumbel search makes exactly n root visits"
        info["halvings_per_search"].append((st.budget, schedule(st.budget, st.m0)[0][1], st.halvings))
    return evals, st


def twin_selfplay_gumbel(N, net_cb, R, r, p, m, c_visit, c_scale, seed, game, start=None, threshold=-0.9,
                         disable=0.05, on_round=None):
    """cap_twin.twin_selfplay_cap (r = 0: the cap is off, every search full) with the Gumbel root search in the full
    searches (m >= 2).  The record also has `visit_pis` (children_as_pi of the raw visits, fast rows zeroed), `begun`,
    `halved` (the two counters), and what the conditions of a game set are asserted on: `reused` (searches begun at a
    root with visits), `dups` (duplicates reverted inside a Gumbel search), `cuts` (select phases cut short at a phase
    end), `off_max` (moves that are not the most visited child), `halvings_per_search` [(n, Q_0, halvings)]"""
    assert m >= 2
    A = N * N + 1
    u = L.or_draw_u01(L.or_draw_u64(seed, game, 0, tw.SITE_RESIGN, 0))
    disabled = u < disable
    pl = L.or_player_new(N, net_cb, None, R, 0, -1.0 if disabled else threshold, seed, game)
    L.or_player_initialize_game(pl, C.byref(start) if start is not None else None)
    env = L.or_player_env(pl)
    start_n = _root_pos(pl).n
    draw = _new_draw(seed, game, pl)
    evals = 1
    if on_round:
        on_round()
    first = select_leaf(env, L.or_player_root(pl), draw)
    pi, v = _net_call(net_cb, [first], A)
    L.or_incorporate_results(env, first, orc.fptr(pi[0]), A, float(v[0]), first)
    positions, moves, full, searched, rows = [], [], [], [], []
    info = dict(begun=0, halved=0, reused=0, dups=0, cuts=0, off_max=0, halvings_per_search=[], sched=[])
    was_resign = 0
    while True:
        root = L.or_player_root(pl)
        is_full = True if r <= 0 else bool(ct.coin_full(seed, game, _root_pos(pl).n, p))
        searched.append(is_full)
        st = None
        if is_full:                                      # no noise: a Gumbel search
            e, st = _gumbel_readouts(env, pl, draw, net_cb, A, R, m, c_visit, c_scale, seed, game, info, on_round)
        else:
            e = tw._readouts(env, pl, draw, net_cb, A, r, on_round)
        evals += e
        if L.or_player_should_resign(pl):
            L.or_player_set_result(pl, -_root_pos(pl).to_play, 1)
            was_resign = 1
            break
        rp = _root_pos(pl)
        Nr, Wr, Pr = _rows(root, A)
        row = None
        if is_full and st is not None:
            a = best_survivor(st, seed, game, rp.n, Nr, Wr, Pr, rp.to_play, c_visit, c_scale)
            info["off_max"] += bool(a != int(np.argmax(Nr)))
        else:
            a = C.c_int(-1)
            if L.or_player_pick_move(pl, C.byref(a)) != orc.OK:
                a = C.c_int(A - 1)
            a = a.value
        if is_full:
            row, _ = gumbel_pi(Nr, Wr, Pr, _legal(root, A), rp.to_play, c_visit, c_scale)
        positions.append(rp.copy())
        rows.append(row)
        assert L.or_player_play_move(pl, a) == 1
        moves.append(a)
        full.append(is_full)
        draw = _new_draw(seed, game, pl)
        if L.or_node_is_done(env, L.or_player_root(pl)):
            L.or_player_set_result(pl, L.or_result(L.or_node_pos(L.or_player_root(pl))), 0)
            break
    n = L.or_player_num_moves(pl)
    assert n == len(moves) == _root_pos(pl).n - start_n
    fin = _root_pos(pl).copy()
    full = np.array(full, bool)
    raw = np.stack([orc.node_arr(L.or_player_search_pi(pl, i), A).copy() for i in range(n)]) if n else None
    pis = None
    if n:
        raw[~full] = 0.0
        pis = raw.copy()
        for i, row in enumerate(rows):
            if row is not None:
                pis[i] = row
    rec = dict(num_moves=n, result=L.or_player_result(pl), was_resign=was_resign, resign_disabled=int(disabled),
               final_score=0.0 if was_resign else float(L.or_score(C.byref(fin))),
               moves=np.array(moves, np.int16), pis=pis, visit_pis=raw,
               qs=np.array([L.or_player_q(pl, i) for i in range(n)], np.float32),
               evals=evals, positions=positions, final=fin, full=full, searched_full=np.array(searched, bool),
               start_n=start_n, **info)
    L.or_player_free(pl)
    return rec


# ---------------------------------------------------------------- the host simulator with the setting

class GumbelStateC(C.Structure):
    _fields_ = [("n", C.c_int32), ("cnt", C.c_int32), ("budget", C.c_int32), ("P", C.c_int32), ("end", C.c_float),
                ("pad", C.c_int32), ("act", C.c_int16 * 16)]


_gl = None


def gumbel_lib():
    """tests/hostsim/hostsim_gumbel.cpp, built with the flags of the Makefile next to it"""
    global _gl
    if _gl is not None:
        return _gl
    base = ft.forced_lib()
    d = os.path.join(ROOT, "tests", "hostsim")
    recipe = [ln for ln in open(os.path.join(d, "Makefile")).read().split("\n") if ln.startswith("\tg++")]
    assert len(recipe) == 1
    flags = [t for t in shlex.split(recipe[0])[1:] if t not in ("$<", "-o", "$@")]
    src = os.path.join(d, "hostsim_gumbel.cpp")
    deps = [src] + [os.path.join(d, f) for f in ("hostsim_forced.cpp", "hostsim_cap.cpp", "hostsim_starts.cpp",
                                                 "hostsim.cpp")]
    deps += [os.path.join(ROOT, "alphago.jl_amd", "csrc", h) for h in ("agz_search.h", "agz_state.h", "agz_layout.h")]
    deps += [os.path.join(ROOT, "include", h) for h in ("agz.h", "agz_draws.h")]
    out = os.path.join(d, "libhostsim_gumbel.so")
    if not os.access(d, os.W_OK):
        out = os.path.join(tempfile.mkdtemp(prefix="hostsim_gumbel_"), "libhostsim_gumbel.so")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
        subprocess.run(["g++"] + flags + [src, "-o", out], check=True)
    S = C.CDLL(out)
    for name, fn in list(vars(base).items()):           # the prototypes declared so far, on this library's symbols
        if name.startswith("hs_"):
            g = getattr(S, name)
            g.restype, g.argtypes = fn.restype, fn.argtypes
    S.hs_set_gumbel.restype = None
    S.hs_set_gumbel.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
    S.hs_gumbel_counts.restype = None
    S.hs_gumbel_counts.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    S.hs_gumbel_state.restype = None
    S.hs_gumbel_state.argtypes = [C.c_void_p, C.c_int, C.POINTER(GumbelStateC)]
    S.hs_gumbel_pi.restype = None
    S.hs_gumbel_pi.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_float)]
    S.hs_gumbel_descend.restype = C.c_int
    S.hs_gumbel_descend.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int16), C.c_int]
    S.hs_gumbel_schedule.restype = C.c_int
    S.hs_gumbel_schedule.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]
    _gl = S
    return S


class GumbelSim(ft.ForcedSim):
    """ForcedSim on the library that can also set the Gumbel root search and run gumbel_pi on a node"""

    def __init__(self, **cfg):
        self.L = gumbel_lib()
        self.cfg = hs.default_config(**cfg)
        self.h = self.L.hs_create(C.byref(self.cfg))
        d = (C.c_int32 * 10)()
        self.L.hs_dims(self.h, d)
        (self.N, self.P, self.A, self.AP, self.cap, self.games, self.par, self.mgl, self.tau, self.maxd) = list(d)

    def set_gumbel(self, m=0, c_visit=50.0, c_scale=1.0):
        self.L.hs_set_gumbel(self.h, int(m), float(c_visit), float(c_scale))

    def gumbel_counts(self):
        out = (C.c_ulonglong * 2)()
        self.L.hs_gumbel_counts(self.h, out)
        return int(out[0]), int(out[1])

    def gumbel_state(self, g):
        st = GumbelStateC()
        self.L.hs_gumbel_state(self.h, g, C.byref(st))
        return st

    def gumbel_pi(self, g, node, c_visit, c_scale):
        out = np.zeros(self.A, np.float32)
        self.L.hs_gumbel_pi(self.h, g, node, float(c_visit), float(c_scale), hs.pf(out))
        return out

    def gumbel_descend(self, g, survivors):
        act = (C.c_int16 * len(survivors))(*survivors)
        return int(self.L.hs_gumbel_descend(self.h, g, act, len(survivors)))

    def schedule(self, n, m0):
        out = (C.c_int32 * 128)()
        k = self.L.hs_gumbel_schedule(int(n), int(m0), out, 64)
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(k)]
