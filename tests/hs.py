"""ctypes binding of tests/hostsim/libhostsim.so -- the host wave simulator over the engine's
search templates (TEST INFRASTRUCTURE; see tests/hostsim/hostsim.cpp)."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np

import alphago_jl_amd as ag
from alphago_jl_amd import symmetry as sy

HERE = os.path.dirname(os.path.abspath(__file__))
CT = ["steps", "positions", "started", "finished", "evals", "dup", "terminal", "rootvisits",
      "pool_exhausted", "resigned", "claimed", "recorded",
      "t_free", "t_pick", "t_child", "t_reroot", "t_noise", "t_move_select", "n_move", "t_select", "n_select", "t_move_max",
      "t_create", "n_create", "pool_short", "peak_nodes"]          # enum Counter of agz_state.h, in order


class AgzConfig(C.Structure):
    _fields_ = [
        ("board_size", C.c_int32), ("tower_height", C.c_int32), ("games", C.c_int32),
        ("num_readouts", C.c_int32), ("parallel_readouts", C.c_int32), ("two_player_mode", C.c_int32),
        ("komi", C.c_float), ("reserved0", C.c_float),
        ("c_puct", C.c_double), ("dirichlet_noise_weight", C.c_double), ("resign_threshold", C.c_double),
        ("resign_disable_fraction", C.c_double),
        ("seed", C.c_uint64), ("game_id_base", C.c_uint64), ("game_id_stride", C.c_uint64),
        ("max_nodes_per_game", C.c_int32), ("device", C.c_int32), ("external_network", C.c_int32),
        ("pool_policy", C.c_int32), ("record_capacity_games", C.c_int32), ("arena_mode", C.c_int32),
    ]


def default_config(**kw):
    c = AgzConfig()
    c.board_size = 19
    c.tower_height = 19
    c.games = 1
    c.num_readouts = 800
    c.parallel_readouts = 8
    c.two_player_mode = 0
    c.komi = 7.5
    c.c_puct = 0.96
    c.dirichlet_noise_weight = 0.25
    c.resign_threshold = -0.9
    c.resign_disable_fraction = 0.05
    c.seed = 0
    c.game_id_base = 0
    c.game_id_stride = 1
    for k, v in kw.items():
        setattr(c, k, v)
    return c


class PositionInfo(C.Structure):
    _fields_ = [("n", C.c_int32), ("to_play", C.c_int32), ("ko", C.c_int32), ("caps_black", C.c_int32),
                ("caps_white", C.c_int32), ("last_move", C.c_int32), ("prev_move", C.c_int32),
                ("history_len", C.c_int32), ("komi", C.c_float)]


class GameHeader(C.Structure):
    _fields_ = [("game_id", C.c_uint64), ("num_moves", C.c_int32), ("result", C.c_int32),
                ("was_resign", C.c_int32), ("resign_disabled", C.c_int32), ("final_score", C.c_float),
                ("short_searches", C.c_int32)]


class NodeMeta(C.Structure):
    _fields_ = [("parent", C.c_int32), ("n", C.c_int32), ("ko", C.c_int32), ("caps_b", C.c_int32),
                ("caps_w", C.c_int32), ("fmove", C.c_int16), ("last_move", C.c_int16), ("losses", C.c_int16),
                ("to_play", C.c_int8), ("flags", C.c_uint8), ("pad", C.c_int32)]


class GameState(C.Structure):
    _fields_ = [("game_id", C.c_uint64), ("resign_threshold", C.c_double), ("rootN", C.c_float),
                ("rootW", C.c_float), ("target", C.c_float), ("komi", C.c_float), ("root", C.c_int32),
                ("phase", C.c_int32), ("sel", C.c_int32), ("move_count", C.c_int32), ("nqs", C.c_int32),
                ("hist_len", C.c_int32), ("free_top", C.c_int32), ("nleaves", C.c_int32),
                ("leaf_base", C.c_int32), ("resign_disabled", C.c_int32), ("err", C.c_int32),
                ("result", C.c_int32), ("was_resign", C.c_int32), ("nodes_used", C.c_int32),
                ("short_first", C.c_int32), ("arena_k", C.c_int32), ("garbage", C.c_int32), ("npend", C.c_int32),
                ("short_searches", C.c_int32), ("stalled", C.c_int32)]


class TreeArgs(C.Structure):
    _fields_ = [("op", C.c_int32), ("g", C.c_int32), ("node", C.c_int32), ("a", C.c_int32),
                ("up_to", C.c_int32), ("par", C.c_int32), ("value", C.c_float), ("info", PositionInfo),
                ("probs", C.POINTER(C.c_float)), ("board", C.POINTER(C.c_int8)),
                ("history", C.POINTER(C.c_int8)), ("iout", C.POINTER(C.c_int32)),
                ("dout", C.POINTER(C.c_double))]


class GumbelStateC(C.Structure):
    _fields_ = [("n", C.c_int32), ("cnt", C.c_int32), ("budget", C.c_int32), ("P", C.c_int32), ("end", C.c_float),
                ("pad", C.c_int32), ("act", C.c_int16 * 16)]


(TOP_INIT, TOP_SELECT, TOP_ADD_CHILD, TOP_VLOSS_ADD, TOP_VLOSS_REVERT, TOP_INCORPORATE, TOP_NOISE,
 TOP_SEARCH_SELECT, TOP_SEARCH_POST, TOP_PICK, TOP_PLAY, TOP_RESIGN, TOP_SCORES, TOP_PENDING) = range(14)

_lib = None
sig = None                   # name -> (restype, argtypes) of every export of hostsim.cpp, once lib() has run


def lib():
    global _lib, sig
    if _lib is not None:
        return _lib
    d = os.path.join(HERE, "hostsim")
    try:          # always: make is incremental, and a library older than its sources would test stale code
        subprocess.run(["make", "-s", "-C", d], check=True)
    except Exception:
        if not os.path.exists(os.path.join(d, "libhostsim.so")):
            raise
    L = C.CDLL(os.path.join(d, "libhostsim.so"))
    vp, i, f, dbl, ull = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_ulonglong
    P = C.POINTER
    i8p, i32p = P(C.c_int8), P(C.c_int32)
    sig = {
        "hs_create": (vp, [P(AgzConfig)]), "hs_destroy": (None, [vp]), "hs_dims": (None, [vp, P(C.c_int32)]),
        "hs_start": (None, [vp, C.c_int64]), "hs_pre": (i, [vp]), "hs_leaf_features": (None, [vp, P(f)]),
        "hs_post": (None, [vp, P(f), P(f)]), "hs_counters": (None, [vp, P(C.c_ulonglong)]),
        "hs_arena_counts": (None, [vp, P(C.c_int32)]),
        "hs_live_games": (i, [vp]), "hs_records_count": (C.c_long, [vp]),
        "hs_record_header": (None, [vp, C.c_long, P(GameHeader)]),
        "hs_record_game": (None, [vp, C.c_long, P(C.c_int16), P(f), P(f)]),
        "hs_go_play": (None, [vp, P(C.c_int8), P(C.c_int8), P(C.c_int32), P(C.c_int32), i, P(C.c_int8),
                              P(C.c_int32), P(C.c_int32), P(C.c_int32)]),
        "hs_go_legal": (None, [vp, P(C.c_int8), P(C.c_int8), P(C.c_int32), i, P(C.c_int8)]),
        "hs_go_score": (None, [vp, P(C.c_int8), P(f), i, P(f)]),
        "hs_tree_op": (i, [vp, P(TreeArgs), P(C.c_int32)]),
        "hs_set_batch_outputs": (None, [vp, P(f), P(f), i]),
        "hs_tree_leaf_features": (None, [vp, i, P(f)]),
        "hs_game_state": (None, [vp, i, P(GameState)]), "hs_game_set": (None, [vp, i, i, C.c_double]),
        "hs_node_meta": (None, [vp, i, i, P(NodeMeta)]), "hs_node_set_n": (None, [vp, i, i, i]),
        "hs_node_N": (f, [vp, i, i]), "hs_node_W": (f, [vp, i, i]), "hs_node_set_N": (None, [vp, i, i, f]),
        "hs_node_row": (P(f), [vp, i, i, i]), "hs_node_children": (P(C.c_int32), [vp, i, i]),
        "hs_node_board": (P(C.c_int8), [vp, i, i]), "hs_node_legal": (None, [vp, i, i, P(C.c_int8)]),
        # the settings of self-play and what the tests read back of them
        "hs_set_starts": (None, [vp, P(C.c_int8), P(ag._lib.PositionInfo), P(C.c_int8), i]),
        "hs_starts_count": (i, [vp]), "hs_start_board_valid": (i, [vp, P(C.c_int8), i]),
        "hs_set_playout_cap": (None, [vp, i, dbl]),
        "hs_set_forced_playouts": (None, [vp, dbl, i]), "hs_pruned_pi": (i, [vp, i, i, dbl, P(f)]),
        "hs_set_gumbel": (None, [vp, i, dbl, dbl]), "hs_gumbel_counts": (None, [vp, P(C.c_ulonglong)]),
        "hs_gumbel_state": (None, [vp, i, P(GumbelStateC)]), "hs_gumbel_pi": (None, [vp, i, i, dbl, dbl, P(f)]),
        "hs_gumbel_descend": (i, [vp, i, P(C.c_int16), i]), "hs_gumbel_schedule": (i, [i, i, P(C.c_int32), i]),
        "hs_set_puct": (None, [vp, i, dbl, dbl, dbl]), "hs_puct_counts": (None, [vp, P(C.c_ulonglong)]),
        "hs_leaf_paths": (i, [vp, i, P(C.c_int32), P(C.c_int32), P(C.c_int32)]),
        "hs_set_symmetry": (None, [vp, i]), "hs_leaf_syms": (None, [vp, P(C.c_int32)]),
        "hs_set_root_policy_temperature": (i, [vp, i, dbl, dbl, dbl]), "hs_set_root_noise": (i, [vp, dbl, i]),
        "hs_set_move_temperature": (i, [vp, i, dbl, dbl, dbl]), "hs_explore_counts": (None, [vp, P(C.c_ulonglong)]),
        "hs_explore_rows": (None, [vp, i, i, P(f), P(dbl), P(f)]), "hs_temperature": (dbl, [i, dbl, dbl, dbl]),
        "hs_set_pick_case": (None, [vp, i, P(f), C.c_ulonglong, i]),
        "hs_node_lines": (None, [vp, i, i, i, i, i, P(ag._lib.Line), P(C.c_int16), P(f)]),
        "hs_analysis_start": (None, [vp, P(C.c_int8), P(ag._lib.PositionInfo), P(C.c_int8), C.c_int64, P(C.c_int16),
                                     P(C.c_int64), C.c_uint64]),
        "hs_analysis_results": (C.c_longlong, [vp, P(ag._lib.Analysis), P(f), P(f), P(f)]),
        # value uncertainty
        "hs_set_value_moments": (i, [vp, i]), "hs_set_lcb": (i, [vp, dbl, i, dbl]),
        "hs_set_puct_variance": (i, [vp, dbl, dbl, dbl]), "hs_uncertainty_setting": (None, [vp, P(dbl)]),
        "hs_uncertainty_counts": (None, [vp, P(ull)]), "hs_node_S": (f, [vp, i, i]),
        "hs_node_row_S": (P(f), [vp, i, i]), "hs_child_lcb": (i, [vp, i, i, dbl, P(dbl), P(dbl), P(dbl)]),
        "hs_root_set": (None, [vp, i, f, f]), "hs_sqrt": (dbl, [dbl]), "hs_value_lcb": (None, [f, f, f, i, dbl, P(dbl)]),
        "hs_variance_factor": (dbl, [f, f, f, dbl, dbl, dbl]),
        # superko
        "hs_set_ko_rule": (i, [vp, i]), "hs_ko_rule": (i, [vp]),
        "hs_superko_counts": (None, [vp, P(ull)]), "hs_node_key": (ull, [vp, i, i]), "hs_game_log": (i, [vp, i, P(ull)]),
        "hs_node_flags": (None, [vp, i, P(C.c_uint8)]), "hs_go_keys": (None, [vp, i8p, i8p, i, i, P(ull)]),
        "hs_go_legal_seen": (None, [vp, i8p, i8p, i32p, P(ull), P(C.c_int64), i, i, i8p]),
        "hs_zobrist": (ull, [i, i]), "hs_white_to_play": (ull, []), "hs_position_key": (ull, [i8p, i, i, i]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def counter_names():
    """enum Counter of agz_state.h, in order (without CT_COUNT)"""
    src = open(os.path.join(os.path.dirname(HERE), "alphago.jl_amd", "csrc", "agz_state.h")).read()
    body = re.search(r"enum Counter : int \{(.*?)\};", src, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = re.findall(r"\bCT_\w+", body)
    assert names[-1] == "CT_COUNT" and len(names) - 1 <= 64
    return names[:-1]


def p8(a):
    return a.ctypes.data_as(C.POINTER(C.c_int8))


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def pf(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def pu64(a):
    return a.ctypes.data_as(C.POINTER(C.c_ulonglong))


def bits32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class Sim:
    """A hostsim engine plus the helpers the parity tests need."""

    def __init__(self, **cfg):
        self.L = lib()
        self.cfg = default_config(**cfg)
        self.h = self.L.hs_create(C.byref(self.cfg))
        d = (C.c_int32 * 10)()
        self.L.hs_dims(self.h, d)
        (self.N, self.P, self.A, self.AP, self.cap, self.games, self.par, self.mgl, self.tau, self.maxd) = list(d)
        self.setting = (0, 0.0, 0.0, 0.0)          # the PUCT rule options: off

    def close(self):
        if self.h:
            self.L.hs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- batched self-play
    def start(self, total_games):
        self.L.hs_start(self.h, total_games)

    def step(self, net, white_net=None):
        """one self-play step; net(feats [B,17*P] float32) -> (pi [B,A], v [B]).  Arena mode:
        `net` answers the Black players' leaves, `white_net` the White players'."""
        B = self.L.hs_pre(self.h)
        if B == 0:
            if white_net is not None:      # a step may consist of terminal leaves only: moves happen in post
                z = np.zeros((1, self.A), np.float32)
                self.L.hs_post(self.h, pf(z), pf(np.zeros(1, np.float32)))
            return 0
        feats = np.zeros((B, 17 * self.P), np.float32)
        self.L.hs_leaf_features(self.h, pf(feats))
        if white_net is not None:
            cnt = (C.c_int32 * 2)()
            self.L.hs_arena_counts(self.h, cnt)
            pi, v = np.zeros((B, self.A), np.float32), np.zeros(B, np.float32)
            if cnt[0]:
                pi[:cnt[0]], v[:cnt[0]] = net(feats[:cnt[0]])
            if cnt[1]:
                pi[cnt[0]:], v[cnt[0]:] = white_net(feats[cnt[0]:])
        else:
            pi, v = net(feats)
        pi = np.ascontiguousarray(pi, np.float32)
        v = np.ascontiguousarray(v, np.float32)
        self.L.hs_post(self.h, pf(pi), pf(v))
        return B

    def counters(self):
        out = (C.c_ulonglong * 64)()            # enum Counter of agz_state.h is longer than the names kept here
        self.L.hs_counters(self.h, out)
        return dict(zip(CT, list(out)))

    def all_counters(self):
        """every counter of enum Counter by its name"""
        out = (C.c_ulonglong * 64)()
        self.L.hs_counters(self.h, out)
        return dict(zip(counter_names(), list(out)))

    def records(self):
        out = []
        for k in range(self.L.hs_records_count(self.h)):
            hd = GameHeader()
            self.L.hs_record_header(self.h, k, C.byref(hd))
            nm = hd.num_moves
            moves = np.zeros(max(nm, 1), np.int16)
            pis = np.zeros((max(nm, 1), self.A), np.float32)
            qs = np.zeros(max(nm, 1), np.float32)
            self.L.hs_record_game(self.h, k, moves.ctypes.data_as(C.POINTER(C.c_int16)), pf(pis), pf(qs))
            out.append(dict(game_id=hd.game_id, num_moves=nm, result=hd.result, was_resign=hd.was_resign,
                            resign_disabled=hd.resign_disabled, final_score=hd.final_score,
                            short_searches=hd.short_searches, moves=moves[:nm].copy(), pis=pis[:nm].copy(), qs=qs[:nm].copy()))
        return sorted(out, key=lambda r: r["game_id"])

    # ---- the settings of self-play (agz_selfplay_set_*)
    def set_starts(self, positions):
        """the table of start positions, from oracle positions; an empty list clears it"""
        if not positions:
            self.L.hs_set_starts(self.h, None, None, None, 0)
            return
        from selfplay_twin import opos_arrays          # (the twin module imports this one)
        boards, infos, hist = opos_arrays(positions)
        self.L.hs_set_starts(self.h, p8(boards), infos, p8(hist), len(positions))

    def board_valid(self, board, ko=-1):
        b = np.ascontiguousarray(board, np.int8)
        return bool(self.L.hs_start_board_valid(self.h, p8(b), ko))

    def set_playout_cap(self, r, p):
        self.L.hs_set_playout_cap(self.h, int(r), float(p))

    def cap_counts(self):
        c, names = self.all_counters(), counter_names()
        assert names.index("CT_CAP_FAST") == names.index("CT_CAP_FULL") + 1
        assert names.index("CT_PEAK_NODES") == len(CT) - 1
        return int(c["CT_CAP_FULL"]), int(c["CT_CAP_FAST"])

    def set_forced_playouts(self, k, prune=True):
        self.L.hs_set_forced_playouts(self.h, float(k), 1 if prune else 0)

    def forced_counts(self):
        c, names = self.all_counters(), counter_names()
        assert names.index("CT_PRUNED_ROWS") == names.index("CT_FORCED_SEL") + 1 == names.index("CT_CAP_FAST") + 2
        return int(c["CT_FORCED_SEL"]), int(c["CT_PRUNED_ROWS"])

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

    def schedule(self, n, m0):
        """the Sequential Halving schedule [(m_p, Q_p)] of a search of budget n with m0 survivors"""
        out = (C.c_int32 * 128)()
        k = self.L.hs_gumbel_schedule(int(n), int(m0), out, 64)
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(k)]

    # ---- the PUCT rule options (agz_search_set_puct) and the symmetry mode
    def set_puct(self, fpu_on=0, r=0.0, r_root=0.0, c_base=0.0):
        self.L.hs_set_puct(self.h, int(fpu_on), float(r), float(r_root), float(c_base))
        self.setting = (int(fpu_on), float(r), float(r_root), float(c_base))      # (puct_twin.predict_phase reads it)

    def puct_counts(self):
        out = (C.c_ulonglong * 2)()
        self.L.hs_puct_counts(self.h, out)
        return int(out[0]), int(out[1])

    def set_symmetry(self, mode):
        """-1 none, 0..7 fixed, 8 random (agz_selfplay_set_symmetry)"""
        self.L.hs_set_symmetry(self.h, int(mode))

    def step_sym(self, forward):
        """one self-play step whose leaves are evaluated under their recorded symmetries: forward(feats) -> (pi, v) is the
        plain network; the features go in under T_s and the policy comes back under its inverse"""
        def net(feats):
            B = len(feats)
            s = np.zeros(B, np.int32)
            self.L.hs_leaf_syms(self.h, p32(s))
            x = np.stack([sy.apply_features(feats[k], int(s[k]), self.N) for k in range(B)]).astype(np.float32)
            pi, v = forward(x)
            pi = np.stack([sy.apply_policy(pi[k], sy.inverse(int(s[k])), self.N) for k in range(B)]).astype(np.float32)
            return pi, v
        return self.step(net)

    def scores(self, node, g=0):
        out = np.zeros(self.A, np.float64)
        st, _ = self.op(TOP_SCORES, g=g, node=node, dout=out)
        assert st == 0
        return out

    def leaf_paths(self, g=0):
        """the leaves of the last select phase of slot g: [(leaf, [root .. leaf])]"""
        nodes = np.zeros(self.par, np.int32)
        plen = np.zeros(self.par, np.int32)
        paths = np.zeros((self.par, self.maxd), np.int32)
        n = self.L.hs_leaf_paths(self.h, g, p32(nodes), p32(plen), p32(paths))
        return [(int(nodes[k]), [int(x) for x in paths[k, :plen[k]]]) for k in range(n)]

    # ---- root exploration and the move temperature (a setting: explore_twin.setting)
    def apply(self, st):
        """the three setters from a setting; an off part is set off"""
        from explore_twin import schedule_of           # (the twin module imports this one)
        pt, (total, shaped), mt = st["pt"], st["noise"], st["mt"]
        off = (0, 1.0, 1.0, 1.0)
        assert self.L.hs_set_root_policy_temperature(self.h, *(off if pt is None else (1,) + schedule_of(pt, self.N))) == 0
        assert self.L.hs_set_root_noise(self.h, float(total), 1 if shaped else 0) == 0
        assert self.L.hs_set_move_temperature(self.h, *(off if mt is None else (1,) + schedule_of(mt, self.N))) == 0

    def explore_counts(self):
        out = (C.c_ulonglong * 4)()
        self.L.hs_explore_counts(self.h, out)
        return tuple(int(x) for x in out)

    def explore_rows(self, node, g=0):
        t, al, nz = np.zeros(self.A, np.float32), np.zeros(self.A, np.float64), np.zeros(self.A, np.float32)
        self.L.hs_explore_rows(self.h, g, node, pf(t), al.ctypes.data_as(C.POINTER(C.c_double)), pf(nz))
        return t, al, nz

    def set_pick_case(self, Nrow, game_id, n, g=0):
        row = np.ascontiguousarray(Nrow, np.float32)
        self.L.hs_set_pick_case(self.h, g, pf(row), int(game_id), int(n))

    # ---- value uncertainty (agz_search_set_value_moments / _set_lcb / _set_puct_variance).  The setters return the
    # status; gpu_options.configure asserts it
    def set_value_moments(self, on=True):
        return self.L.hs_set_value_moments(self.h, int(on))

    def set_lcb(self, z=0.0, min_visits=1, min_ratio=0.0):
        return self.L.hs_set_lcb(self.h, float(z), int(min_visits), float(min_ratio))

    def set_puct_variance(self, k=0.0, prior=0.4, weight=2.0):
        return self.L.hs_set_puct_variance(self.h, float(k), float(prior), float(weight))

    def uncertainty_setting(self):
        """(moments on, z, min_visits, min_ratio, k, prior, weight)"""
        out = np.zeros(8, np.float64)
        self.L.hs_uncertainty_setting(self.h, pd(out))
        return (int(out[0]), out[1], int(out[2]), out[3], out[4], out[5], out[6])

    def uncertainty_counts(self):
        out = (C.c_ulonglong * 4)()
        self.L.hs_uncertainty_counts(self.h, out)
        return tuple(int(x) for x in out)

    def S_(self, g, node):
        return self.L.hs_node_S(self.h, g, node)

    def row_S(self, g, node):
        return np.ctypeslib.as_array(self.L.hs_node_row_S(self.h, g, node), shape=(self.AP,))[: self.A]

    def child_lcb(self, node, z, g=0):
        m, sd, l = np.zeros(self.A, np.float64), np.zeros(self.A, np.float64), np.zeros(self.A, np.float64)
        assert self.L.hs_child_lcb(self.h, g, node, float(z), pd(m), pd(sd), pd(l)) == ag._lib.OK
        return m, sd, l

    # ---- superko (agz_search_set_ko_rule)
    def set_ko_rule(self, rule):
        """the status; gpu_options.configure asserts it"""
        return self.L.hs_set_ko_rule(self.h, int(rule))

    def ko_rule(self):
        return self.L.hs_ko_rule(self.h)

    def superko_counts(self):
        out = (C.c_ulonglong * 2)()
        self.L.hs_superko_counts(self.h, out)
        return int(out[0]), int(out[1])

    def node_key(self, node, g=0):
        return int(self.L.hs_node_key(self.h, g, node))

    def game_log(self, g=0):
        out = np.zeros(7 + self.mgl, np.uint64)
        n = self.L.hs_game_log(self.h, g, pu64(out))
        return [int(x) for x in out[:n]]

    def live_nodes(self, g=0):
        out = np.zeros(self.cap, np.uint8)
        self.L.hs_node_flags(self.h, g, out.ctypes.data_as(C.POINTER(C.c_uint8)))
        return [int(i) for i in np.nonzero(out & 4)[0]]

    def position_keys(self, boards, to_play, rule):
        B = len(to_play)
        out = np.zeros(B, np.uint64)
        self.L.hs_go_keys(self.h, p8(np.ascontiguousarray(boards, np.int8)), p8(np.ascontiguousarray(to_play, np.int8)), B,
                          int(rule), pu64(out))
        return out

    def legal_moves(self, boards, to_play, ko, seen, rule):
        """seen: one list of keys per position"""
        B = len(to_play)
        off = np.zeros(B + 1, np.int64)
        off[1:] = np.cumsum([len(k) for k in seen])
        flat = np.array([x for k in seen for x in k] + [0], np.uint64)
        out = np.zeros((B, self.A), np.int8)
        self.L.hs_go_legal_seen(self.h, p8(np.ascontiguousarray(boards, np.int8)), p8(np.ascontiguousarray(to_play, np.int8)),
                                p32(np.ascontiguousarray(ko, np.int32)), pu64(flat), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                B, int(rule), p8(out))
        return out

    # ---- batched analysis and game review
    def analysis_start(self, positions, games=None, game_id_base=0):
        """agz_analyze_start on oracle positions (or their opos_arrays, which a caller may have spoilt); with `games` (one
        list of flat moves per position) agz_review_start: the positions are the games' starts, and ply k of game j is
        row offsets[j] + k.  Step the run with step()."""
        from selfplay_twin import opos_arrays          # (the twin module imports this one)
        boards, infos, hist = positions if isinstance(positions, tuple) else opos_arrays(positions)
        B = len(infos)
        moves = off = None
        self.an_rows = B
        if games is not None:
            assert len(games) == B
            mv = np.array([m for g in games for m in g] + [0], np.int16)        # (never empty)
            of = np.concatenate([[0], np.cumsum([len(g) for g in games])]).astype(np.int64)
            moves, off = mv.ctypes.data_as(C.POINTER(C.c_int16)), of.ctypes.data_as(C.POINTER(C.c_int64))
            self.an_rows = int(of[-1])
        self.L.hs_analysis_start(self.h, p8(boards), infos, p8(hist), B, moves, off, game_id_base)

    def analysis_results(self):
        """(rows finished, the fields of the run's rows: move, status, N, W, Q, nodes_used, child_N / child_W / prior)"""
        n = self.an_rows
        res = (ag._lib.Analysis * max(n, 1))()
        rows = [np.zeros((max(n, 1), self.A), np.float32) for _ in range(3)]
        done = self.L.hs_analysis_results(self.h, res, *(pf(r) for r in rows))
        out = {f: np.array([getattr(res[k], f) for k in range(n)], np.int32 if t is C.c_int32 else np.float32)
               for f, t in ag._lib.Analysis._fields_}
        out.update(child_N=rows[0][:n], child_W=rows[1][:n], prior=rows[2][:n])
        return int(done), out

    # ---- Go rules
    def go_play(self, boards, to_play, ko, moves):
        B = len(moves)
        boards = np.ascontiguousarray(boards, np.int8)
        to_play = np.ascontiguousarray(to_play, np.int8)
        ko = np.ascontiguousarray(ko, np.int32)
        moves = np.ascontiguousarray(moves, np.int32)
        bo = np.zeros_like(boards)
        ko_o = np.zeros(B, np.int32)
        nc = np.zeros(B, np.int32)
        st = np.zeros(B, np.int32)
        self.L.hs_go_play(self.h, p8(boards), p8(to_play), p32(ko), p32(moves), B, p8(bo), p32(ko_o), p32(nc), p32(st))
        return bo, ko_o, nc, st

    def go_legal(self, boards, to_play, ko):
        B = len(to_play)
        boards = np.ascontiguousarray(boards, np.int8)
        out = np.zeros((B, self.A), np.int8)
        self.L.hs_go_legal(self.h, p8(boards), p8(np.ascontiguousarray(to_play, np.int8)),
                           p32(np.ascontiguousarray(ko, np.int32)), B, p8(out))
        return out

    def go_score(self, boards, komi):
        B = len(komi)
        out = np.zeros(B, np.float32)
        self.L.hs_go_score(self.h, p8(np.ascontiguousarray(boards, np.int8)),
                           pf(np.ascontiguousarray(komi, np.float32)), B, pf(out))
        return out

    # ---- single-tree ops
    def op(self, op, g=0, node=0, a=0, up_to=-1, par=0, value=0.0, probs=None, board=None, info=None,
           history=None, dout=None):
        T = TreeArgs()
        T.op, T.g, T.node, T.a, T.up_to, T.par, T.value = op, g, node, a, up_to, par, value
        keep = []
        if probs is not None:
            pr = np.ascontiguousarray(probs, np.float32)
            keep.append(pr)
            T.probs = pf(pr)
        if board is not None:
            bd = np.ascontiguousarray(board, np.int8)
            keep.append(bd)
            T.board = p8(bd)
        if history is not None:
            hh = np.ascontiguousarray(history, np.int8)
            keep.append(hh)
            T.history = p8(hh)
        if info is not None:
            T.info = info
        if dout is not None:
            T.dout = dout.ctypes.data_as(C.POINTER(C.c_double))
        r0 = C.c_int32()
        st = self.L.hs_tree_op(self.h, C.byref(T), C.byref(r0))
        return st, r0.value

    def tree_init(self, g, board, n=0, to_play=1, ko=-1, caps=(0, 0), last_move=-1, komi=7.5, history=None):
        info = PositionInfo()
        info.n, info.to_play, info.ko = n, to_play, ko
        info.caps_black, info.caps_white = caps
        info.last_move, info.prev_move = last_move, -1
        info.history_len = 0 if history is None else len(history)
        info.komi = komi
        st, root = self.op(TOP_INIT, g=g, board=board, info=info, history=history)
        assert st == 0
        return root

    def pruned_pi(self, g, node, k):
        """agz_tree_pruned_pi: (row float32[A], whether pruning changed it)"""
        out = np.zeros(self.A, np.float32)
        ch = self.L.hs_pruned_pi(self.h, g, node, float(k), pf(out))
        return out, bool(ch)

    def gumbel_pi(self, g, node, c_visit, c_scale):
        out = np.zeros(self.A, np.float32)
        self.L.hs_gumbel_pi(self.h, g, node, float(c_visit), float(c_scale), pf(out))
        return out

    def gumbel_descend(self, g, survivors):
        """one descent from the root of slot g with `survivors` as its Gumbel state -> the leaf"""
        act = (C.c_int16 * len(survivors))(*survivors)
        return int(self.L.hs_gumbel_descend(self.h, g, act, len(survivors)))

    def lines(self, node, K, D, mv, g=0):
        """node_lines on `node`: the fields of the K lines, pv [K][D] and pv_N [K][D]"""
        ln = (ag._lib.Line * K)()
        pv = np.full((K, D), 7, np.int16)               # (junk: every entry has to be written)
        pvn = np.full((K, D), 7, np.float32)
        self.L.hs_node_lines(self.h, g, node, K, D, mv, ln, pv.ctypes.data_as(C.POINTER(C.c_int16)), pf(pvn))
        out = {f: np.array([getattr(x, f) for x in ln], np.int32 if f in ("move", "pv_len") else np.float32)
               for f in ("move", "pv_len", "N", "W", "prior", "end_W")}
        out.update(pv=pv, pv_N=pvn)
        return out

    def game(self, g):
        s = GameState()
        self.L.hs_game_state(self.h, g, C.byref(s))
        return s

    def meta(self, g, node):
        m = NodeMeta()
        self.L.hs_node_meta(self.h, g, node, C.byref(m))
        return m

    def row(self, g, node, field):
        return np.ctypeslib.as_array(self.L.hs_node_row(self.h, g, node, field), shape=(self.AP,))[: self.A]

    def children(self, g, node):
        return np.ctypeslib.as_array(self.L.hs_node_children(self.h, g, node), shape=(self.AP,))[: self.A]

    def board(self, g, node):
        return np.ctypeslib.as_array(self.L.hs_node_board(self.h, g, node), shape=(self.P,)).copy()

    def legal(self, g, node):
        out = np.zeros(self.A, np.int8)
        self.L.hs_node_legal(self.h, g, node, p8(out))
        return out

    def N_(self, g, node):
        return self.L.hs_node_N(self.h, g, node)

    def W_(self, g, node):
        return self.L.hs_node_W(self.h, g, node)

    def Q_(self, g, node):
        return np.float32(self.W_(g, node)) / (np.float32(1) + np.float32(self.N_(g, node)))


class PeakedNet:
    """pi and v from a hash of the features: one board point holds `peak` of the mass, the rest is spread over all
    actions in four levels (equal priors: unvisited children tie under the FPU, so the tie draw is exercised); v is
    spread over +-0.9"""

    def __init__(self, N, peak=0.6, salt=0):
        self.N, self.A, self.peak, self.salt = N, N * N + 1, peak, salt
        self.calls = 0

    def __call__(self, feats):
        feats = np.ascontiguousarray(feats, np.float32)
        B = feats.shape[0]
        pi = np.zeros((B, self.A), np.float32)
        v = np.zeros(B, np.float32)
        for b in range(B):
            h = zlib.crc32(feats[b].tobytes(), self.salt)
            rng = np.random.RandomState(h)
            rest = np.floor(rng.rand(self.A) * 4.0) / 4.0 + 0.05
            rest[-1] *= 0.25                            # a pass is rarely the network's idea
            row = (1.0 - self.peak) * rest / rest.sum()
            row[h % (self.A - 1)] += self.peak
            pi[b] = row.astype(np.float32)
            v[b] = np.float32(((h >> 8) % 1801) / 1000.0 - 0.9)
        self.calls += B
        return pi, v
