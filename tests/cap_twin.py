"""Twin of the self-play loop under playout cap randomization (TEST INFRASTRUCTURE).

twin_selfplay_cap is starts_twin.twin_selfplay -- selfplay.jl:1-45 over the oracle's primitives -- with one change per
loop iteration: before the search of the root of ply n it draws the coin
    full = u01(draw_u64(seed, game, n, AGZ_SITE_PLAYOUT_CAP = 11, 0)) < p
and searches in full (or_inject_noise, R readouts) or fast (no noise, r readouts).  The rows of fast plies are zeroed in
the returned record ("no policy target").  Also here: the coin in Python, the host simulator with the cap setter, and a
numpy restatement of the targets-only replay sampler (agz_replay_set_targets_only + agz_replay_sample)."""
import ctypes as C
import os
import shlex
import subprocess
import tempfile

import numpy as np

import alphago_jl_amd as ag
import hs
import orc
import starts_twin as tw
from starts_twin import L, _net_call, _new_draw, _readouts, _root_pos

SITE_PLAYOUT_CAP = 11
SITE_REPLAY_SAMPLE = 9
SITE_REPLAY_SYM = 10
ROOT = tw.ROOT


def coin_full(seed, game, n, p):
    """the full / fast decision for the root of ply n of game `game`"""
    return L.or_draw_u01(L.or_draw_u64(seed, game, n, SITE_PLAYOUT_CAP, 0)) < p


def pattern(seed, game, start_n, num_moves, p):
    """the decisions of the plies a game of num_moves moves from position.n = start_n played"""
    return np.array([coin_full(seed, game, start_n + k, p) for k in range(num_moves)], bool)


def twin_selfplay_cap(N, net_cb, R, r, p, seed, game, start=None, threshold=-0.9, disable=0.05, on_round=None):
    """one self-play game under the cap (r fast readouts, full with probability p); see twin_selfplay for the rest.
    The record also has `full` (bool per ply) and `searched_full` (one more entry when the game ended by resignation:
    the search that resigned was decided too, and played no move)"""
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
    first = L.or_select_leaf(env, L.or_player_root(pl), C.byref(draw))
    pi, v = _net_call(net_cb, [first], A)
    L.or_incorporate_results(env, first, orc.fptr(pi[0]), A, float(v[0]), first)
    positions, moves, full, searched = [], [], [], []
    was_resign = 0
    while True:
        root = L.or_player_root(pl)
        is_full = bool(coin_full(seed, game, _root_pos(pl).n, p))
        searched.append(is_full)
        if is_full:
            L.or_inject_noise(env, root, C.byref(draw))
        evals += _readouts(env, pl, draw, net_cb, A, R if is_full else r, on_round)
        if L.or_player_should_resign(pl):
            L.or_player_set_result(pl, -_root_pos(pl).to_play, 1)
            was_resign = 1
            break
        a = C.c_int(-1)
        if L.or_player_pick_move(pl, C.byref(a)) != orc.OK:
            a = C.c_int(A - 1)
        positions.append(_root_pos(pl).copy())
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
    pis = np.stack([orc.node_arr(L.or_player_search_pi(pl, k), A).copy() for k in range(n)]) if n else None
    if n:
        pis[~full] = 0.0
    rec = dict(num_moves=n, result=L.or_player_result(pl), was_resign=was_resign, resign_disabled=int(disabled),
               final_score=0.0 if was_resign else float(L.or_score(C.byref(fin))),
               moves=np.array(moves, np.int16), pis=pis, qs=np.array([L.or_player_q(pl, k) for k in range(n)], np.float32),
               evals=evals, positions=positions, final=fin, full=full, searched_full=np.array(searched, bool),
               start_n=start_n)
    L.or_player_free(pl)
    return rec


# ---------------------------------------------------------------- the host simulator with the cap

_cl = None


def cap_lib():
    """tests/hostsim/hostsim_cap.cpp, built with the flags of the Makefile next to it"""
    global _cl
    if _cl is not None:
        return _cl
    base = tw.starts_lib()
    d = os.path.join(ROOT, "tests", "hostsim")
    recipe = [ln for ln in open(os.path.join(d, "Makefile")).read().split("\n") if ln.startswith("\tg++")]
    assert len(recipe) == 1
    flags = [t for t in shlex.split(recipe[0])[1:] if t not in ("$<", "-o", "$@")]
    src = os.path.join(d, "hostsim_cap.cpp")
    deps = [src, os.path.join(d, "hostsim_starts.cpp"), os.path.join(d, "hostsim.cpp")]
    deps += [os.path.join(ROOT, "alphago.jl_amd", "csrc", h) for h in ("agz_search.h", "agz_state.h", "agz_layout.h")]
    deps += [os.path.join(ROOT, "include", h) for h in ("agz.h", "agz_draws.h")]
    out = os.path.join(d, "libhostsim_cap.so")
    if not os.access(d, os.W_OK):
        out = os.path.join(tempfile.mkdtemp(prefix="hostsim_cap_"), "libhostsim_cap.so")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
        subprocess.run(["g++"] + flags + [src, "-o", out], check=True)
    S = C.CDLL(out)
    for name, fn in list(vars(base).items()):           # the prototypes declared so far, on this library's symbols
        if name.startswith("hs_"):
            g = getattr(S, name)
            g.restype, g.argtypes = fn.restype, fn.argtypes
    S.hs_set_playout_cap.restype = None
    S.hs_set_playout_cap.argtypes = [C.c_void_p, C.c_int, C.c_double]
    _cl = S
    return S


def counter_names():
    """enum Counter of agz_state.h, in order (without CT_COUNT)"""
    import re
    src = open(os.path.join(ROOT, "alphago.jl_amd", "csrc", "agz_state.h")).read()
    body = re.search(r"enum Counter : int \{(.*?)\};", src, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = re.findall(r"\bCT_\w+", body)
    assert names[-1] == "CT_COUNT" and len(names) - 1 <= 64
    return names[:-1]


class CapSim(tw.StartsSim):
    """StartsSim on the library that can also set the playout cap"""

    def __init__(self, **cfg):
        self.L = cap_lib()
        self.cfg = hs.default_config(**cfg)
        self.h = self.L.hs_create(C.byref(self.cfg))
        d = (C.c_int32 * 10)()
        self.L.hs_dims(self.h, d)
        (self.N, self.P, self.A, self.AP, self.cap, self.games, self.par, self.mgl, self.tau, self.maxd) = list(d)

    def set_playout_cap(self, r, p):
        self.L.hs_set_playout_cap(self.h, int(r), float(p))

    def cap_counts(self):
        out = (C.c_ulonglong * 64)()
        self.L.hs_counters(self.h, out)
        names = counter_names()
        at = names.index("CT_CAP_FULL")
        assert names[at + 1] == "CT_CAP_FAST" and names.index("CT_PEAK_NODES") == len(hs.CT) - 1
        return int(out[at]), int(out[at + 1])


# ---------------------------------------------------------------- the targets-only sampler, restated

def _index(bits, n):
    """agz_index (include/agz_draws.h): uniform in [0, n) from the high 32 bits"""
    return ((int(bits) >> 32) * int(n)) >> 32


def floyd_entries(seed, call, B, Lw):
    """agz_replay_sample's draw as include/agz.h states it: B distinct entries of 0..Lw-1"""
    taken, out = set(), []
    for b in range(B):
        j = Lw - B + b
        t = _index(L.or_draw_u64(seed, call, 0, SITE_REPLAY_SAMPLE, j), j + 1)
        e = j if t in taken else t
        taken.add(e)
        out.append(e)
    return out


def target_entries(pis_per_game):
    """every target ply of an arena (a list of [num_moves][A] pi arrays, oldest game first) as (game, ply), in order"""
    out = []
    for g, pis in enumerate(pis_per_game):
        for k in range(len(pis)):
            if np.any(np.asarray(pis[k]) != 0):
                out.append((g, k))
    return out


def sample_targets(seed, call, B, pis_per_game, window=None):
    """(game, ply) of the B samples a targets-only arena draws: the live entries are the newest `window` target plies
    (None: all of them), entry e the e-th of them, oldest first"""
    ent = target_entries(pis_per_game)
    if window is not None:
        ent = ent[max(0, len(ent) - window):]
    pick = floyd_entries(seed, call, B, len(ent))
    return [ent[e] for e in pick], len(ent)
