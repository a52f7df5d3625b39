"""Twin of the self-play loop under forced playouts and policy target pruning (TEST INFRASTRUCTURE).

The oracle's or_select_leaf cannot force, so the descent (mcts.jl:108-138) is restated here over the oracle's primitives
(or_node_set_N, or_child_action_score, or_all_legal_moves, or_maybe_add_child, or_draw_u64) with the same ODraw.sel
bookkeeping and the same tie key sel * 1024 + depth; at depth 0 of a forced search every under-forced child scores one
common value above all real scores.  The pruned target is restated in numpy float64 with float32 exactly where the rule
says float32.  twin_selfplay_forced is cap_twin.twin_selfplay_cap with that descent and that target; with k = 0 it must
be twin_selfplay_cap bit for bit (tests/test_forced_playouts.py holds it to that before anything rests on it).  Also
here: the host simulator with the setter and the single-node pruned_pi entry."""
import ctypes as C
import os
import shlex
import subprocess
import tempfile

import numpy as np

import cap_twin as ct
import hs
import orc
import starts_twin as tw
from starts_twin import L, _net_call, _new_draw, _root_pos

ROOT = tw.ROOT
SITE_PUCT_TIE = 1
FORCED_SCORE = 1.0e300
f32, f64 = np.float32, np.float64

L.or_det_pow.restype = C.c_double
L.or_det_pow.argtypes = [C.c_double, C.c_double]


def _site_puct_tie():
    import re
    hdr = open(os.path.join(ROOT, "include", "agz_draws.h")).read()
    return int(re.search(r"#define AGZ_SITE_PUCT_TIE (\d+)u", hdr).group(1))


SITE_PUCT_TIE = _site_puct_tie()


# ---------------------------------------------------------------- the rules, restated

def under_forced(k, N, P, T):
    """the children a visited root child is forced ahead of the arg-max: N^2 < (k P) T in float64, in this order"""
    N64, P64 = np.asarray(N, f32).astype(f64), np.asarray(P, f32).astype(f64)
    return (N64 > 0) & (N64 * N64 < (f64(k) * P64) * f64(T))


def action_scores(N, W, P, tp, rootN, c_puct):
    """child_action_score (mcts.jl:86-92): Float32 Q times to_play plus Float64 U; also the Float32 Q * to_play"""
    N, W, P = (np.asarray(x, f32) for x in (N, W, P))
    scale = f64(c_puct) * f64(np.sqrt(f32(1) + f32(rootN)))
    denom = f32(1) + N
    qs = (W / denom) * f32(tp)
    assert qs.dtype == np.float32
    return qs.astype(f64) + (scale * P.astype(f64)) / denom.astype(f64), qs, scale


def pruned_visits(N, W, P, tp, rootN, c_puct, k):
    """N' of the pruned target: float64[A]"""
    N = np.asarray(N, f32)
    P = np.asarray(P, f32)
    T = f64(f32(N.astype(f64).sum()))
    score, qs, scale = action_scores(N, W, P, tp, rootN, c_puct)
    cs = int(np.argmax(N))                      # the first maximum: the lowest index on ties
    out = N.astype(f64)
    for a in range(len(N)):
        if a == cs or not N[a] > 0:
            continue
        n, p = f64(N[a]), f64(P[a])
        nf = np.sqrt((f64(k) * p) * T)
        gap = score[cs] - f64(qs[a])
        n_min = n if gap <= 0 else (scale * p) / gap - f64(1)
        m = min(n, max(n - nf, n_min, f64(0)))
        if m < n and m <= 1:
            m = f64(0)
        out[a] = m
    return out


def pi_of(visits, squash):
    """children_as_pi's transform of float64 visits: x (x^0.98 under the squash) over the sum in ascending index order"""
    x = [L.or_det_pow(float(v), 0.98) if squash else float(v) for v in visits]
    s = 0.0
    for v in x:
        s += v
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.array(x, f64) / f64(s)).astype(f32)


def pruned_pi(N, W, P, tp, rootN, c_puct, k, squash):
    """(row float32[A], changed)"""
    Np = pruned_visits(N, W, P, tp, rootN, c_puct, k)
    return pi_of(Np, squash), bool((Np < np.asarray(N, f32).astype(f64)).any())


# ---------------------------------------------------------------- the descent

def _index(bits, n):
    return ((int(bits) >> 32) * int(n)) >> 32


def select_leaf(env, root, draw, k=0.0):
    """or_select_leaf restated; k > 0 applies the forced rule at depth 0.  Returns (leaf, forced): forced = the root
    level of this descent was decided among under-forced children"""
    A = env.contents.A
    ps = A - 1
    cur, depth, forced = root, 0, False
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
        else:
            L.or_child_action_score(env, cur, cas.ctypes.data_as(C.POINTER(C.c_double)))
            L.or_all_legal_moves(pos, legal.ctypes.data_as(C.POINTER(C.c_int8)))
            lg = legal != 0
            if k > 0 and depth == 0:
                T = f32(cN.astype(f64).sum())
                uf = under_forced(k, cN, orc.node_arr(L.or_node_child_prior(cur), A), T)
                cas[uf] = FORCED_SCORE
                forced = bool((uf & lg).any())
            best = cas[lg].max()
            possible = np.flatnonzero(lg & (cas == best))
            pick = int(possible[0])
            if len(possible) > 1:
                bits = L.or_draw_u64(draw.seed, draw.game, draw.move, SITE_PUCT_TIE, draw.sel * 1024 + depth)
                pick = int(possible[_index(bits, len(possible))])
        nx = C.c_void_p()
        assert L.or_maybe_add_child(env, cur, pick, C.byref(nx)) == orc.OK
        cur = nx.value
        depth += 1
    draw.sel += 1
    return cur, forced


def _tree_search(env, root, draw, net_cb, A, k, par=8):
    """starts_twin._tree_search on the restated descent; also the number of forced root selections"""
    leaves, failsafe, nforced = [], 0, 0
    while len(leaves) < par and failsafe < 2 * par:
        failsafe += 1
        leaf, forced = select_leaf(env, root, draw, k)
        nforced += forced
        if L.or_node_is_done(env, leaf):
            L.or_backup_value(leaf, float(L.or_result(L.or_node_pos(leaf))), root)
            continue
        L.or_add_virtual_loss(leaf, root)
        leaves.append(leaf)
    if leaves:
        pi, v = _net_call(net_cb, leaves, A)
        for i, leaf in enumerate(leaves):
            L.or_revert_virtual_loss(leaf, root)
            L.or_incorporate_results(env, leaf, orc.fptr(pi[i]), A, float(v[i]), root)
    return len(leaves), nforced


def _readouts(env, p, draw, net_cb, A, R, k, on_round=None):
    root = L.or_player_root(p)
    current = f32(L.or_node_N(root))
    evals = nforced = 0
    while f32(L.or_node_N(root)) < current + f32(R):
        if on_round:
            on_round()
        e, nf = _tree_search(env, root, draw, net_cb, A, k)
        evals += e
        nforced += nf
    return evals, nforced


def twin_selfplay_forced(N, net_cb, R, r, p, k, prune, seed, game, start=None, threshold=-0.9, disable=0.05,
                         on_round=None):
    """cap_twin.twin_selfplay_cap (r = 0: the cap is off, every search full) with the forced descent in the full
    searches and, with prune, the pruned target in their rows.  The record also has `raw_pis` (children_as_pi of the
    raw visits, fast rows zeroed), `forced_sel` (root descents the forced rule decided) and `pruned_rows` (bool per
    ply: pruning changed the row)"""
    A = N * N + 1
    u = L.or_draw_u01(L.or_draw_u64(seed, game, 0, tw.SITE_RESIGN, 0))
    disabled = u < disable
    pl = L.or_player_new(N, net_cb, None, R, 0, -1.0 if disabled else threshold, seed, game)
    L.or_player_initialize_game(pl, C.byref(start) if start is not None else None)
    env = L.or_player_env(pl)
    tau = L.or_player_tau_threshold(pl)
    start_n = _root_pos(pl).n
    draw = _new_draw(seed, game, pl)
    evals = 1
    if on_round:
        on_round()
    first, _ = select_leaf(env, L.or_player_root(pl), draw)
    pi, v = _net_call(net_cb, [first], A)
    L.or_incorporate_results(env, first, orc.fptr(pi[0]), A, float(v[0]), first)
    positions, moves, full, searched, rows, changed = [], [], [], [], [], []
    was_resign, forced_sel = 0, 0
    while True:
        root = L.or_player_root(pl)
        is_full = True if r <= 0 else bool(ct.coin_full(seed, game, _root_pos(pl).n, p))
        searched.append(is_full)
        if is_full:
            L.or_inject_noise(env, root, C.byref(draw))
        e, nf = _readouts(env, pl, draw, net_cb, A, R if is_full else r, k if is_full else 0.0, on_round)
        evals += e
        forced_sel += nf
        if L.or_player_should_resign(pl):
            L.or_player_set_result(pl, -_root_pos(pl).to_play, 1)
            was_resign = 1
            break
        a = C.c_int(-1)
        if L.or_player_pick_move(pl, C.byref(a)) != orc.OK:
            a = C.c_int(A - 1)
        rp = _root_pos(pl)
        positions.append(rp.copy())
        row, ch = None, False
        if is_full and prune and k > 0:
            row, ch = pruned_pi(orc.node_arr(L.or_node_child_N(root), A), orc.node_arr(L.or_node_child_W(root), A),
                                orc.node_arr(L.or_node_child_prior(root), A), rp.to_play, L.or_node_N(root),
                                env.contents.c_puct, k, rp.n <= tau)
        rows.append(row)
        changed.append(ch)
        assert L.or_player_play_move(pl, a.value) == 1
        moves.append(a.value)
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
               moves=np.array(moves, np.int16), pis=pis, raw_pis=raw,
               qs=np.array([L.or_player_q(pl, i) for i in range(n)], np.float32),
               evals=evals, positions=positions, final=fin, full=full, searched_full=np.array(searched, bool),
               start_n=start_n, forced_sel=forced_sel, pruned_rows=np.array(changed, bool))
    L.or_player_free(pl)
    return rec


# ---------------------------------------------------------------- the host simulator with the setting

_fl = None


def forced_lib():
    """tests/hostsim/hostsim_forced.cpp, built with the flags of the Makefile next to it"""
    global _fl
    if _fl is not None:
        return _fl
    base = ct.cap_lib()
    d = os.path.join(ROOT, "tests", "hostsim")
    recipe = [ln for ln in open(os.path.join(d, "Makefile")).read().split("\n") if ln.startswith("\tg++")]
    assert len(recipe) == 1
    flags = [t for t in shlex.split(recipe[0])[1:] if t not in ("$<", "-o", "$@")]
    src = os.path.join(d, "hostsim_forced.cpp")
    deps = [src] + [os.path.join(d, f) for f in ("hostsim_cap.cpp", "hostsim_starts.cpp", "hostsim.cpp")]
    deps += [os.path.join(ROOT, "alphago.jl_amd", "csrc", h) for h in ("agz_search.h", "agz_state.h", "agz_layout.h")]
    deps += [os.path.join(ROOT, "include", h) for h in ("agz.h", "agz_draws.h")]
    out = os.path.join(d, "libhostsim_forced.so")
    if not os.access(d, os.W_OK):
        out = os.path.join(tempfile.mkdtemp(prefix="hostsim_forced_"), "libhostsim_forced.so")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
        subprocess.run(["g++"] + flags + [src, "-o", out], check=True)
    S = C.CDLL(out)
    for name, fn in list(vars(base).items()):           # the prototypes declared so far, on this library's symbols
        if name.startswith("hs_"):
            g = getattr(S, name)
            g.restype, g.argtypes = fn.restype, fn.argtypes
    S.hs_set_forced_playouts.restype = None
    S.hs_set_forced_playouts.argtypes = [C.c_void_p, C.c_double, C.c_int]
    S.hs_pruned_pi.restype = C.c_int
    S.hs_pruned_pi.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_float)]
    _fl = S
    return S


class ForcedSim(ct.CapSim):
    """CapSim on the library that can also set forced playouts and run pruned_pi on a node"""

    def __init__(self, **cfg):
        self.L = forced_lib()
        self.cfg = hs.default_config(**cfg)
        self.h = self.L.hs_create(C.byref(self.cfg))
        d = (C.c_int32 * 10)()
        self.L.hs_dims(self.h, d)
        (self.N, self.P, self.A, self.AP, self.cap, self.games, self.par, self.mgl, self.tau, self.maxd) = list(d)

    def set_forced_playouts(self, k, prune=True):
        self.L.hs_set_forced_playouts(self.h, float(k), 1 if prune else 0)

    def all_counters(self):
        """every counter of enum Counter by its name"""
        out = (C.c_ulonglong * 64)()
        self.L.hs_counters(self.h, out)
        return dict(zip(ct.counter_names(), list(out)))

    def forced_counts(self):
        c = self.all_counters()
        names = ct.counter_names()
        assert names.index("CT_PRUNED_ROWS") == names.index("CT_FORCED_SEL") + 1 == names.index("CT_CAP_FAST") + 2
        return int(c["CT_FORCED_SEL"]), int(c["CT_PRUNED_ROWS"])

    def pruned_pi(self, g, node, k):
        out = np.zeros(self.A, np.float32)
        ch = self.L.hs_pruned_pi(self.h, g, node, float(k), hs.pf(out))
        return out, bool(ch)
