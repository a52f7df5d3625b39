"""Host-side mirror of the reference's call surface for the hot path, over the C ABI.

Same names, argument meaning and error behaviour as tejank10/AlphaGo.jl so that the parity tests
read like the reference's own tests -- GoEnv, Position, play_move / pass_move / all_legal_moves /
score / result, NeuralNet, MCTSPlayer (initialize_game, tree_search, pick_move, play_move,
should_resign, is_done, set_result, extract_data), selfplay -- with Python conventions: 0-based
(row, col) coordinates, `None` for a pass, snake_case instead of `!`.  No arithmetic happens here:
every method marshals arrays and makes one call into libagz (HIP, gfx950)."""
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import IllegalMove
from .engine import Engine, value_targets

BLACK, WHITE, EMPTY = 1, -1, 0
_KGS = "ABCDEFGHJKLMNOPQRST"
_SGF = "abcdefghijklmnopqrstuvwxyz"

PlayerMove = namedtuple("PlayerMove", "color move")       # board.jl:17-20

_rules = {}


def _rules_engine(N):
    """a 1-slot engine used only for the batched rule kernels (agz_go_*) with B = 1"""
    if N not in _rules:
        _rules[N] = Engine(board_size=N, tower_height=0, games=1, num_readouts=1, max_nodes_per_game=8)
    return _rules[N]


class GoEnv:
    """GoEnv(N, planes=17), src/game/go/go.jl:1-26"""

    def __init__(self, board_size=19, planes=17):
        assert planes % 2 == 1
        self.N = board_size
        self.action_space = board_size * board_size + 1
        self.planes = (planes - 1) // 2
        self.max_action_space = 361          # go.jl:24 (hard-coded in the reference)


def to_flat(c, env):                          # coords.jl:5-7
    return env.N * env.N if c is None else c[0] + env.N * c[1]


def from_flat(f, env):                        # coords.jl:10-12
    return None if f == env.N * env.N else (f % env.N, f // env.N)


def from_kgs(s, env):                         # coords.jl:26-34
    if s == "pass":
        return None
    return env.N - int(s[1:]), _KGS.index(s[0].upper())


def to_kgs(c, env):                           # coords.jl:37
    return "pass" if c is None else f"{_KGS[c[1]]}{env.N - c[0]}"


def from_sgf(s):                              # coords.jl:14-20
    return None if not s else (_SGF.index(s[1]), _SGF.index(s[0]))


def to_sgf(c):                                # coords.jl:23
    return "" if c is None else _SGF[c[1]] + _SGF[c[0]]


class Position:
    """GoPosition, src/game/go/board.jl:271-306.  board[row, col] in {-1, 0, +1}."""

    def __init__(self, env, board=None, n=0, komi=7.5, caps=(0, 0), ko=None, recent=(), board_deltas=None,
                 to_play=BLACK):
        self.env = env
        N = env.N
        self.board = np.zeros((N, N), np.int8) if board is None else np.array(board, np.int8).reshape(N, N)
        self.n = n
        self.komi = float(np.float32(komi))
        self.caps = tuple(caps)
        self.ko = ko
        self.recent = list(recent)
        self.board_deltas = np.zeros((0, N, N), np.int8) if board_deltas is None else np.array(board_deltas, np.int8)
        self.to_play = to_play
        self.done = False

    # flat views in the ABI's point order p = row + N*col
    def _flat(self):
        return np.ascontiguousarray(self.board.T).reshape(1, -1)

    def _ko0(self):
        return -1 if self.ko is None else to_flat(self.ko, self.env)

    def soa(self):
        """(board [P], deltas [7, P], ndeltas, to_play) for agz_net_forward / agz_features"""
        N = self.env.N
        d = np.zeros((7, N * N), np.int8)
        k = self.board_deltas.shape[0]
        for i in range(k):
            d[i] = np.ascontiguousarray(self.board_deltas[i].T).reshape(-1)
        return self._flat()[0], d, k, self.to_play

    def all_legal_moves(self):                # board.jl:393-424
        return _rules_engine(self.env.N).go_legal(self._flat(), [self.to_play], [self._ko0()])[0]

    def is_move_legal(self, c):               # board.jl:376-391
        return bool(self.all_legal_moves()[to_flat(c, self.env)])

    def score(self):                          # board.jl:511-533
        return float(_rules_engine(self.env.N).go_score(self._flat(), [self.komi])[0])

    def result(self):                         # board.jl:535-544
        s = self.score()
        return 1 if s > 0 else -1 if s < 0 else 0

    def result_string(self):                  # board.jl:546-555
        s = self.score()
        return f"B+{s:.1f}" if s > 0 else f"W+{-s:.1f}" if s < 0 else "DRAW"

    def _copy(self):
        p = Position(self.env, self.board.copy(), self.n, self.komi, self.caps, self.ko, list(self.recent),
                     self.board_deltas.copy(), self.to_play)
        return p                              # like deepcopy(GoPosition): done resets (board.jl:308-315)

    def pass_move(self, mutate=False):        # board.jl:426-440
        return self.play_move(None, mutate=mutate)

    def flip_playerturn(self, mutate=False):  # board.jl:442-447
        p = self if mutate else self._copy()
        p.ko = None
        p.to_play = -p.to_play
        return p

    def play_move(self, c, mutate=False):     # board.jl:451-509
        env, N = self.env, self.env.N
        a = to_flat(c, env)
        bo, ko_o, nc, st = _rules_engine(N).go_play(self._flat(), [self.to_play], [self._ko0()], [a])
        if st[0] == _lib.ILLEGAL_MOVE:
            raise IllegalMove(_lib.ILLEGAL_MOVE, f"illegal move {c}")
        new_board = bo[0].reshape(N, N).T.copy()
        color = self.to_play
        # delta = +color at the played point and wherever an opponent stone vanished (board.jl:479-481)
        delta = np.where(new_board != self.board, color, 0).astype(np.int8)
        p = self if mutate else self._copy()
        was_pass_before = bool(self.recent) and self.recent[-1].move is None
        p.board = new_board
        p.n = self.n + 1
        cap = int(nc[0])
        p.caps = (self.caps[0] + cap, self.caps[1]) if color == BLACK else (self.caps[0], self.caps[1] + cap)
        p.ko = None if ko_o[0] < 0 else from_flat(int(ko_o[0]), env)
        p.recent = list(self.recent) + [PlayerMove(color, c)]
        keep = self.board_deltas[: env.planes - 2]
        p.board_deltas = np.concatenate([delta[None], keep], axis=0)
        p.to_play = -color
        p.done = c is None and was_pass_before
        return p


class NeuralNet:
    """NeuralNet(env; tower_height), src/neural_net.jl:13-33 -- inference only"""

    def __init__(self, env, tower_height=19, seed=0):
        self.env = env
        self.tower_height = tower_height
        self.engine = Engine(board_size=env.N, tower_height=tower_height, games=1, num_readouts=1,
                             max_nodes_per_game=8)
        self.engine.init_synthetic(seed)      # Flux-default-equivalent init (glorot uniform, BN identity)

    def set_weights(self, layer, kind, data):
        self.engine.set_weights(layer, kind, data)

    def set_precision(self, precision="f32"):
        """tower arithmetic of nn(positions): "f32" (default) or "f16" (fp16 operands, f32 accumulate)"""
        self.engine.set_precision(precision)

    def __call__(self, positions, symmetry=None):            # neural_net.jl:57-73
        """symmetry (ours, DESIGN.md "Board symmetries"): None = the reference's one orientation; s in 0..7 or an
        array of one s per position = each position evaluated under T_s, pi back in board orientation; "average" =
        the mean pi and v over all eight symmetries"""
        single = isinstance(positions, Position)
        plist = [positions] if single else list(positions)
        if plist and not isinstance(plist[0], Position):
            feats = np.stack([np.asarray(p.feats, np.float32).reshape(-1) for p in plist])
            pi, v = self.forward_features(feats, symmetry)
        elif symmetry is not None:
            soa = [p.soa() for p in plist]
            feats = self.engine.features(np.stack([s[0] for s in soa]), np.stack([s[1] for s in soa]),
                                         [s[2] for s in soa], [s[3] for s in soa])
            pi, v = self.forward_features(feats, symmetry)
        else:
            soa = [p.soa() for p in plist]
            pi, v = self.engine.forward(np.stack([s[0] for s in soa]), np.stack([s[1] for s in soa]),
                                        [s[2] for s in soa], [s[3] for s in soa])
        return (pi[0], float(v[0])) if single else (pi.T.copy(), v)      # pi is A x B like the reference

    def forward_features(self, feats, symmetry=None):
        """feats [B, 17*N*N] -> (pi [B, A], v [B]); symmetry as in __call__"""
        if symmetry is None:
            return self.engine.forward_features(feats)
        feats = np.ascontiguousarray(feats, np.float32)
        B = feats.shape[0]
        if isinstance(symmetry, str):
            if symmetry != "average":
                raise ValueError(f"symmetry {symmetry!r}: None, 0..7, an array of those, or 'average'")
            pi, v = self.engine.forward_features_sym(np.repeat(feats, 8, axis=0), np.tile(np.arange(8, dtype=np.int32), B))
            return pi.reshape(B, 8, -1).mean(axis=1, dtype=np.float64).astype(np.float32), \
                v.reshape(B, 8).mean(axis=1, dtype=np.float64).astype(np.float32)
        return self.engine.forward_features_sym(feats, symmetry)


def load_model(model_dir, env, bn_field="auto"):
    """load_model(str, env), src/play.jl:3-21: BSON parameter lists (and BatchNorm statistics when the
    struct dumps are present) -> NeuralNet; the tower height is read off the base parameter list.
    bn_field says what the 5th field of a dumped Flux.BatchNorm is: "std" (Flux <= 0.7, the files the
    reference ships: forward (x - mu) / sigma), "var" (Flux >= 0.8: sigma^2, eps under the root) or
    "auto" (decide per layer from the dump: Float64 eps = 1e-8 / TrackedArray parameters => "std")."""
    from . import bson_weights as bw
    ck = bw.read_checkpoint(model_dir, bn_field)
    nn = NeuralNet(env, tower_height=bw.tower_height_of(ck["base"]))
    bw.apply_param_lists(nn.engine, ck["base"], ck["value"], ck["policy"], ck.get("base_stats"),
                         ck.get("value_stats"), ck.get("policy_stats"))
    return nn


def save_model(nn, model_dir):
    """save_model(nn), src/train.jl:14-35 (the reference hard-codes <repo>/models; here the directory
    is an argument): writes weights/agz_{base,value,policy}.bson readable by Flux.loadparams!"""
    from . import bson_weights as bw
    bw.write_checkpoint(model_dir, bw.extract_param_lists(nn.engine))


def get_feats(pos):                           # features.jl:24-26 -> [17, N, N] indexed [plane, row, col]
    N = pos.env.N
    b, d, k, tp = pos.soa()
    f = _rules_engine(N).features(b[None], d[None], [k], [tp])[0]
    return f.reshape(17, N, N).transpose(0, 2, 1).copy()


class LeafPosition(Position):
    """One element of the `Vector{Position}` a duck-typed network receives (`mcts_player.network([leaf.position for leaf
    in leaves])`, mcts_play.jl:89): the leaf's GoPosition fields materialised from the device tree by
    agz_tree_leaf_positions -- board, board_deltas (newest first), to_play, n, ko, caps, the last two moves -- so that
    `len(positions)` is the batch size (DummyNet, test/test_mcts_player.jl:25-32) and get_feats(position) /
    NeuralNet(positions) work on it like on any Position.  `.node` is the leaf's handle; `.feats` the 17 planes
    (plane-major, p = row + N*col), computed on demand by agz_features."""

    node = None

    @property
    def feats(self):
        b, d, k, tp = self.soa()
        return _rules_engine(self.env.N).features(b[None], d[None], [k], [tp])[0].reshape(-1)


LeafView = LeafPosition       # round <= 5 name


def _leaf_positions(player, lp):
    env, N = player.env, player.env.N
    out = []
    for k in range(len(lp["nodes"])):
        i = lp["info"][k]
        nd = int(lp["ndeltas"][k])
        recent = []
        if i.prev_move >= 0:
            recent.append(PlayerMove(int(i.to_play), from_flat(int(i.prev_move), env)))
        if i.last_move >= 0:
            recent.append(PlayerMove(-int(i.to_play), from_flat(int(i.last_move), env)))
        pos = LeafPosition(env, lp["boards"][k].reshape(N, N).T, int(i.n), i.komi, (int(i.caps_black), int(i.caps_white)),
                           None if i.ko < 0 else from_flat(int(i.ko), env), recent,
                           lp["deltas"][k, :nd].reshape(nd, N, N).transpose(0, 2, 1), int(i.to_play))
        pos.node = NodeView(player, int(lp["nodes"][k]))
        out.append(pos)
    return out


class NodeView:
    """read-only view of an MCTSNode (src/mcts.jl:41-82) living on the device"""

    def __init__(self, player, node):
        self._p, self.id = player, node

    @property
    def _info(self):
        return self._p.engine.node_info(0, self.id)

    N = property(lambda s: s._info.N)
    W = property(lambda s: s._info.W)
    Q = property(lambda s: s._info.Q)
    is_expanded = property(lambda s: bool(s._info.is_expanded))
    losses_applied = property(lambda s: s._info.losses_applied)
    fmove = property(lambda s: s._info.fmove)
    child_N = property(lambda s: s._p.engine.node_floats(0, s.id, _lib.F_CHILD_N))
    child_W = property(lambda s: s._p.engine.node_floats(0, s.id, _lib.F_CHILD_W))
    child_prior = property(lambda s: s._p.engine.node_floats(0, s.id, _lib.F_CHILD_PRIOR))
    child_action_score = property(lambda s: s._p.engine.node_scores(0, s.id))
    # (ours) value uncertainty, with the moments on (lcb= / puct_variance= or Engine.set_value_moments)
    child_S = property(lambda s: s._p.engine.node_floats(0, s.id, _lib.F_CHILD_S))
    child_stdev = property(lambda s: s._p.engine.tree_child_lcb(0, s.id, 0.0)[1])

    # (ours) superko: the node's key under the rule in force, and its legal mask as the search reads it
    key = property(lambda s: s._p.engine.node_key(0, s.id))

    def legal(self):
        """the node's legal mask int8[A] (agz_tree_node_legal): under ko_rule= the moves that repeat a position are off"""
        return self._p.engine.node_legal(0, self.id)

    def child_lcb(self, z):
        """the lower confidence bounds of the children under z, from the side to move (agz_tree_child_lcb)"""
        return self._p.engine.tree_child_lcb(0, self.id, z)[2]

    @property
    def child_Q(self):
        return self.child_W / (np.float32(1) + self.child_N)

    @property
    def child_U(self):                        # mcts.jl:91-92: c_puct (Float64) x Float32 sqrt x prior / (1 + N)
        # Julia evaluates left to right: Float64 c_puct x the Float32 square root, then Float64 throughout
        scale = np.float64(self._p.engine.cfg.c_puct) * np.float64(np.sqrt(np.float32(1) + np.float32(self.N)))
        return scale * self.child_prior.astype(np.float64) / (np.float32(1) + self.child_N).astype(np.float64)

    def __eq__(self, other):
        return isinstance(other, NodeView) and other._p is self._p and other.id == self.id

    def __hash__(self):
        return hash((id(self._p), self.id))

    # ---- the node-level operations test/test_mcts.jl:2-5 imports, one agz_tree_* call each
    def select_leaf(self):                    # mcts.jl:108-138
        return NodeView(self._p, self._p.engine.select_leaf(0, self.id))

    def maybe_add_child(self, f):             # mcts.jl:140-149 (f: 0-based flat move, N*N = pass)
        return NodeView(self._p, self._p.engine.maybe_add_child(0, self.id, int(f)))

    def add_virtual_loss(self, up_to):        # mcts.jl:151-163
        self._p.engine.add_virtual_loss(0, self.id, up_to.id)

    def revert_virtual_loss(self, up_to):     # mcts.jl:165-177
        self._p.engine.revert_virtual_loss(0, self.id, up_to.id)

    def incorporate_results(self, move_probs, value, up_to):      # mcts.jl:187-214
        e = self._p.engine
        st = e.incorporate_results(0, self.id, np.asarray(move_probs, np.float32), float(value), up_to.id)
        if st in (_lib.ASSERT_DONE_NODE, _lib.BAD_SHAPE):
            raise AssertionError(e.L.agz_last_error(e.h).decode())      # mcts.jl:190,196
        e._ck(st)

    def inject_noise(self):                   # mcts.jl:232-239
        self._p.engine.inject_noise(0, self.id)

    def set_N(self, value):                   # mcts.jl:99
        self._p.engine.node_set_N(0, self.id, float(value))

    def is_done(self):                        # mcts.jl:227-229
        return bool(self._p.engine.is_done(0, self.id))

    @property
    def children(self):
        ch = self._p.engine.node_children(0, self.id)
        return {int(a): NodeView(self._p, int(c)) for a, c in enumerate(ch) if c >= 0}

    def pruned_pi(self, k=2.0):
        """children_as_pi of this node with policy target pruning under k (ours, Engine.set_forced_playouts): the
        forced visits the search did not agree with are left out; squashed iff the node's n <= tau"""
        return self._p.engine.tree_pruned_pi(0, self.id, k)

    def gumbel_pi(self, c_visit=50.0, c_scale=1.0):
        """the improved-policy row of this node (ours, Engine.set_gumbel): softmax over its legal actions of
        log(prior) + sigma(q), sigma = (c_visit + max child_N) * c_scale * (0.5 + 0.5 q); an unvisited child's q is the
        node's own network value"""
        return self._p.engine.tree_gumbel_pi(0, self.id, c_visit, c_scale)

    # ---- analysis lines (ours; the commented-out most_visited_path / mvp_gg / describe of mcts.jl:255-327 are the
    # definition): one agz_tree_lines call each, the walk runs on the device
    def lines(self, k=4, depth=16, min_visits=1):
        """the top k candidate moves of this node (child_N, then child_prior descending, then the action ascending)
        with their principal variations: a list of Line"""
        _check_lines(k, depth, min_visits)
        if k == 0:
            return []
        return _line_rows(self._p.env, self._p.engine.tree_lines(0, self.id, k, depth, min_visits))

    def most_visited_path(self):              # mcts.jl:267-281
        """the first line's principal variation as "<kgs> (<N>) ==> ... Q: <Q of its end>"; a tie of child_N at this
        node is decided by the prior (the candidate order), below it by findmax as in the reference.  "GAME END" (a
        most visited child that is no node) is not printed: the walk ends there."""
        ln = self.lines(1, 64, 1)
        if not ln:
            return "Q: %.5f\n" % self.Q
        env = self._p.env
        return "".join(f"{to_kgs(c, env)} ({_jl_f32(n)}) ==> " for c, n in zip(ln[0].pv, ln[0].pv_N)) + "Q: %.5f\n" % ln[0].end_Q

    def mvp_gg(self):                         # mcts.jl:283-293
        """the most visited path in go-gui VAR format while maximum(child_N) > 1, e.g. 'D4 Q16 ...'"""
        ln = self.lines(1, 64, 2)
        if not ln or not ln[0].N > 1:
            return ""
        return " ".join(to_kgs(c, self._p.env) for c in ln[0].pv)

    def describe(self):                       # mcts.jl:295-327, without the P-Dir column (original_prior is not stored)
        env = self._p.env
        cn, prior = self.child_N, self.child_prior
        score, cq, cu = self.child_action_score, self.child_Q, self.child_U
        soft_n = cn / max(np.float32(1), cn.sum())
        p_delta = soft_n - prior
        p_rel = np.zeros_like(p_delta)
        mask = prior != 0
        p_rel[mask] = p_delta[mask] / prior[mask]
        out = ["%.4f\n" % self.Q, self.most_visited_path(),
               "move : action    Q     U     P    N  soft-N  p-delta  p-rel"]
        for ln in self.lines(15, 1, 1):       # the rows in candidate order (the reference: child_N, then action score)
            a = to_flat(ln.move, env)
            out.append("\n%s   : % .3f % .3f %.3f %.3f %5d %.4f % .5f % .2f" % (
                to_kgs(ln.move, env), score[a], cq[a], cu[a], prior[a], int(cn[a]), soft_n[a], p_delta[a], p_rel[a]))
        return "".join(out)

    @property
    def position(self):
        info = self._info
        N = self._p.env.N
        board = self._p.engine.node_board(0, self.id).reshape(N, N).T
        pos = Position(self._p.env, board, info.pos.n, info.pos.komi, (info.pos.caps_black, info.pos.caps_white),
                       None if info.pos.ko < 0 else from_flat(info.pos.ko, self._p.env), to_play=info.pos.to_play)
        pos.done = bool(info.done)
        # `recent`: the whole move list when this node is the player's root (what extract_data / replay_position need,
        # board.jl:557-578); for any other node the moves played since the root, behind the root's
        moves, node, inf = [], self.id, info
        while inf.parent >= 0:
            moves.append(inf.fmove)
            node = inf.parent
            inf = self._p.engine.node_info(0, node)
        base = getattr(self._p, "_recent", None)
        if base is not None and node == self._p.engine.tree_root(0):
            rec, tp = list(base), -info.pos.to_play if len(moves) % 2 else info.pos.to_play
            for a in reversed(moves):
                rec.append(PlayerMove(tp, from_flat(int(a), self._p.env)))
                tp = -tp
            pos.recent = rec
        return pos


def _jl_f32(x):
    """a Float32 as Julia's string interpolation prints it"""
    x = np.float32(x)
    return str(int(x)) + ".0" if x == np.floor(x) and abs(x) < 1e7 else np.format_float_positional(x, unique=True)


def position_arrays(pos):
    """A Position in the C ABI's terms (agz_tree_init, agz_analyze_start): board [P] int8 in point order, a PositionInfo
    (n, to_play, ko, caps, last two moves, history_len, komi) and history [history_len][P] int8.  initialize_game!
    keeps pos.board_deltas (board.jl:505-506): the up-to-7 older boards the history planes need are
    B_{k+1} = B_k - delta_k (features.jl:8-14), newest first."""
    env = pos.env
    board = pos._flat()[0]
    hist, b = [], board.astype(np.int16)
    for k in range(min(7, pos.board_deltas.shape[0])):
        b = b - np.ascontiguousarray(pos.board_deltas[k].T).reshape(-1)
        hist.append(b.astype(np.int8))
    info = _lib.PositionInfo()
    info.n, info.to_play, info.ko = pos.n, pos.to_play, pos._ko0()
    info.caps_black, info.caps_white = pos.caps
    info.last_move = -1 if not pos.recent else to_flat(pos.recent[-1].move, env)
    info.prev_move = -1 if len(pos.recent) < 2 else to_flat(pos.recent[-2].move, env)
    info.history_len = len(hist)
    info.komi = pos.komi
    return board, info, np.stack(hist) if hist else np.zeros((0, env.N * env.N), np.int8)


class MCTSPlayer:
    """MCTSPlayer(env, network; num_readouts, two_player_mode, resign_threshold), mcts_play.jl:3-24.
    `network` is any callable positions -> (pi A x B, v B) (the duck-typed field of mcts_play.jl:5): a NeuralNet of this
    package is evaluated on the device; anything else receives a list of B Position objects (LeafPosition) exactly as
    the reference's `mcts_player.network([leaf.position for leaf in leaves])` (mcts_play.jl:89) and may answer with
    plain arrays or Tracker-style objects carrying `.data` (mcts_play.jl:90)."""

    def __init__(self, env, network, num_readouts=800, two_player_mode=False, resign_threshold=-0.9, seed=0,
                 game_id=0, symmetry=None, fpu=None, c_base=0.0, root_policy_temperature=None, root_noise=None,
                 move_temperature=None, lcb=None, puct_variance=None, ko_rule=None):
        self.env = env
        self.network = network
        self.num_readouts = num_readouts
        self.two_player_mode = two_player_mode
        self.tau_threshold = -1 if two_player_mode else (env.N * env.N // 12) // 2 * 2
        self.resign_threshold = resign_threshold
        internal = isinstance(network, NeuralNet)
        self.engine = Engine(board_size=env.N, tower_height=network.tower_height if internal else 0, games=1,
                             num_readouts=num_readouts, parallel_readouts=64, two_player_mode=int(two_player_mode),
                             resign_threshold=resign_threshold, seed=seed, external_network=0 if internal else 1)
        if internal:
            network.engine.copy_weights_to(self.engine)
        if symmetry is not None:
            # (ours) leaf evaluation under board symmetries: None, "random" or a fixed s in 0..7 (Engine.set_symmetry)
            if not internal:
                raise ValueError("symmetry needs a NeuralNet of this package: a caller's network receives Positions")
            self.engine.set_symmetry(symmetry)
        _apply_puct(self.engine, fpu, c_base)      # (ours) the PUCT rule options of Engine.set_puct
        _apply_uncertainty(self.engine, lcb, puct_variance)
        _apply_ko_rule(self.engine, ko_rule)
        # (ours) root exploration in inject_noise and the move temperature in pick_move, as selfplay() takes them
        _apply_explore(self.engine, root_policy_temperature, root_noise, move_temperature)
        self._game_id = game_id
        self.qs, self.searches_pi = [], []
        self.result, self.result_string = 0, ""
        self._start = None

    def initialize_game(self, pos=None):      # mcts_play.jl:110-118
        pos = Position(self.env) if pos is None else pos
        board, info, hist = position_arrays(pos)
        self.engine.tree_init(0, board, n=pos.n, to_play=pos.to_play, ko=info.ko, caps=pos.caps,
                              last_move=info.last_move, komi=pos.komi, history=hist if len(hist) else None)
        self.engine.set_draw(0, self._game_id, 0)
        self.qs, self.searches_pi = [], []
        self.result, self.result_string = 0, ""
        self._start = pos
        self._moves = []
        self._recent = list(pos.recent)

    @property
    def root(self):
        return NodeView(self, self.engine.tree_root(0))

    def tree_search(self, parallel_readouts=8):    # mcts_play.jl:73-98; returns the leaves like the reference
        e = self.engine
        n = e.tree_search_select(0, parallel_readouts)
        if isinstance(self.network, NeuralNet):
            nodes = e.tree_leaf_positions(0, n, nodes_only=True)["nodes"]
            e.tree_search_incorporate(0)
            return [NodeView(self, int(i)) for i in nodes]
        if n == 0:
            e.tree_search_incorporate(0)
            return []
        positions = _leaf_positions(self, e.tree_leaf_positions(0, n))
        move_probs, values = self.network(positions)             # mcts_play.jl:89
        move_probs = np.asarray(getattr(move_probs, "data", move_probs), np.float32)      # :90
        values = np.asarray(getattr(values, "data", values), np.float32).reshape(-1)
        if move_probs.shape != (self.env.action_space, n) or values.shape != (n,):
            raise AssertionError(f"network returned {move_probs.shape} / {values.shape} for {n} positions "
                                 f"(expected ({self.env.action_space}, {n}) / ({n},))")      # mcts.jl:190
        e.tree_search_incorporate(0, np.ascontiguousarray(move_probs.T), values)          # column i = leaf i (:91)
        return [p.node for p in positions]

    def pick_move(self):                      # mcts_play.jl:52-71
        st, a = self.engine.pick_move(0)
        if st == _lib.ASSERT_SOFTPICK:
            raise AssertionError("child_N[fcoord] != 0 (mcts_play.jl:67)")
        return from_flat(a, self.env)

    def play_move(self, c):                   # mcts_play.jl:26-50
        root = self.root
        info = root._info
        if not self.two_player_mode:
            cn = root.child_N
            with np.errstate(invalid="ignore", divide="ignore"):
                if info.pos.n <= self.tau_threshold:
                    pr = cn.astype(np.float64) ** 0.98
                    self.searches_pi.append((pr / pr.sum()).astype(np.float32))
                else:
                    self.searches_pi.append(cn / cn.sum())
        self.qs.append(np.float32(info.Q))
        if not self.engine.play_move(0, to_flat(c, self.env)):
            print("Illegal move")
            if not self.two_player_mode:
                self.searches_pi.pop()
            self.qs.pop()
            return False
        self._moves.append(c)
        self._recent.append(PlayerMove(info.pos.to_play, c))
        return True

    def get_position(self):                   # mcts_play.jl:141-142
        return self.root.position

    def suggest_move(self):                   # mcts_play.jl:144-151
        current_readouts = self.root.N
        while self.root.N < current_readouts + self.num_readouts:
            self.tree_search()
        return self.pick_move()

    def should_resign(self):                  # mcts_play.jl:124
        return bool(self.engine.should_resign(0))

    def is_done(self):                        # mcts_play.jl:120
        return self.result != 0 or bool(self.engine.is_done(0, self.engine.tree_root(0)))

    def set_result(self, winner, was_resign):  # mcts_play.jl:100-108
        self.result = winner
        self.result_string = ("B+R" if winner == BLACK else "W+R") if was_resign else self.root.position.result_string()

    def extract_data(self, value_target=None):                   # mcts_play.jl:126-139
        assert len(self.searches_pi) == self.root._info.pos.n, "GoPosition history is incomplete"
        pos = Position(self.env, komi=self._start.komi)
        positions = []
        for c in self._moves:
            positions.append(pos)
            pos = pos.play_move(c)
        return positions, [p.copy() for p in self.searches_pi], _results(self, len(positions), value_target)


# A bare finished-game tuple (what records look like before they are wrapped; tests and the replay buffer build them by
# hand).  short_searches: moves played on fewer than num_ro readouts because the node pool was full (0 = the game is the
# reference's game; agz_config.pool_policy, include/agz.h)
GameRecord = namedtuple("GameRecord", "game_id moves searches_pi qs result result_string was_resign short_searches",
                        defaults=[0])


class _FinishedRoot:
    """`player.root` of a finished self-play game: the one thing train() reads from it is `.position`
    (train.jl:72: player.root.position.n; mcts_play.jl:127,132: extract_data replays root.position.recent)"""

    def __init__(self, player):
        self._player = player

    @property
    def position(self):
        return self._player._replay()[1]


class SelfPlayPlayer:
    """What `selfplay(env, nn, num_ro)` returns (selfplay.jl:44): the MCTSPlayer of ONE finished game, read-only --
    `.result`, `.result_string`, `.qs`, `.searches_pi` (mcts_play.jl:3-15) as the device recorded them,
    `.root.position` (the final GoPosition with its whole `recent` list: `.n`, `.board`, `.caps`, ...) and
    `extract_data(player)`.  The tree itself stayed on the device and was recycled with its slot.  Also carries the
    record's fields (`game_id`, `moves` as board coordinates / None, `was_resign`, `short_searches`).  `start` (ours) is
    the Position the game began at -- an entry of selfplay(..., starts=...) -- or None for the empty board: the moves,
    searches_pi and qs cover the plies played from there; `start_index` is that entry's index in the table (-1: none),
    which is what ReplayBuffer keeps to replay the game on the device.  `full_search` (ours) is one bool per move:
    False for the plies of a fast search under selfplay(..., playout_cap=...), whose searches_pi row is all zero (no
    policy target); all True without the cap."""

    def __init__(self, env, network, num_readouts, rec, start=None):
        self.env, self.network, self.num_readouts = env, network, num_readouts
        self.start = start
        self.start_index = int(rec.get("start", -1)) if start is not None else -1
        if start is not None and self.start_index < 0:
            raise ValueError("a start position needs the record's `start` index (Engine.records())")
        self.two_player_mode = False
        self.tau_threshold = (env.N * env.N // 12) // 2 * 2
        self.game_id = int(rec["game_id"])
        self.resign_threshold = -1.0 if rec.get("resign_disabled") else -0.9       # selfplay.jl:9
        self.moves = [from_flat(int(a), env) for a in rec["moves"]]
        self.searches_pi = [np.array(p, np.float32) for p in rec["pis"]]
        self.full_search = [bool(np.any(p != 0)) for p in self.searches_pi]
        self.qs = np.array(rec["qs"], np.float32)
        self.result = int(rec["result"])
        self.was_resign = bool(rec["was_resign"])
        self.short_searches = int(rec.get("short_searches", 0))
        if self.was_resign:                                                         # mcts_play.jl:100-108
            self.result_string = "B+R" if self.result == BLACK else "W+R"
        else:
            sc = float(rec["final_score"])                                          # board.jl:546-555
            self.result_string = f"B+{sc:.1f}" if sc > 0 else f"W+{-sc:.1f}" if sc < 0 else "DRAW"
        self.root = _FinishedRoot(self)
        self._replayed = None

    def _replay(self):
        """replay_position (board.jl:557-578): the positions before each move and the final one, by agz_go_play"""
        if self._replayed is None:
            pos, before = (Position(self.env) if self.start is None else self.start), []
            for c in self.moves:
                before.append(pos)
                pos = pos.play_move(c)
            self._replayed = (before, pos)
        return self._replayed

    @property
    def position(self):                        # mcts_play.jl:14
        return self.root.position

    def get_position(self):                    # mcts_play.jl:141-142
        return self.root.position

    def is_done(self):                         # mcts_play.jl:120
        return True

    def extract_data(self, targets_only=False, value_target=None):                    # mcts_play.jl:126-139
        start_n = 0 if self.start is None else self.start.n
        assert len(self.searches_pi) == self.root.position.n - start_n, "GoPosition history is incomplete"
        before, _ = self._replay()
        keep = [k for k in range(len(before)) if self.full_search[k] or not targets_only]
        results = _results(self, len(before), value_target)       # over every ply: a target sums the fast plies behind it
        return [before[k] for k in keep], [self.searches_pi[k].copy() for k in keep], [results[k] for k in keep]


def _results(player, n, value_target):
    """the results list of extract_data: the constant fill of mcts_play.jl:138, or with value_target = (alpha, lam) the
    per-ply value targets of the player's qs and result (value_targets, include/agz_value_target.h) as float32"""
    if value_target is None:
        return [player.result] * n
    alpha, lam = value_target
    y = value_targets(np.asarray(player.qs, np.float32), player.result, alpha, lam)
    assert len(y) == n, "one recorded q per position"
    return list(y)


# The reference draws from Julia's global RNG (selfplay.jl:9, mcts.jl:133,235, mcts_play.jl:61,66): successive selfplay
# calls see successive random numbers.  Here every draw is a function of (seed, game id, move, site) (include/agz_draws.h):
# `seed(s)` is Random.seed!(s), and each selfplay call plays the next unused game ids of that stream.
_stream = {"seed": 0, "next_game": 0}


def _refuse_two_root_rules(gumbel, forced_playouts):      # before selfplay() / train() create anything
    if gumbel and forced_playouts:
        raise ValueError("gumbel and forced_playouts are two rules for the same decision: ask for one")


def _apply_puct(eng, fpu, c_base):
    """the PUCT rule options (Engine.set_puct) on a fresh engine; nothing asked for, nothing set"""
    if fpu is not None or c_base:
        eng.set_puct(fpu, c_base)


def _apply_ko_rule(eng, ko_rule=None):
    """(ours) the superko rule of a fresh engine: "simple" | "positional" | "situational" (Engine.set_ko_rule); nothing
    asked for, nothing set"""
    if ko_rule is not None:
        eng.set_ko_rule(ko_rule)


def _apply_uncertainty(eng, lcb=None, puct_variance=None):
    """(ours) value uncertainty on a fresh engine: lcb = z | (z, min_visits, min_ratio) -- the move is the child with the
    largest lower confidence bound (Engine.set_lcb); puct_variance = k | (k, prior, weight) -- exploration scaled by the
    spread of a node's values (Engine.set_puct_variance).  Either switches the value moments on; nothing asked for,
    nothing set"""
    if lcb is None and puct_variance is None:
        return
    eng.set_value_moments(True)
    if lcb is not None:
        eng.set_lcb(lcb)
    if puct_variance is not None:
        eng.set_puct_variance(puct_variance)


def _apply_explore(eng, root_policy_temperature=None, root_noise=None, move_temperature=None):
    """root exploration and the move temperature (Engine.set_root_policy_temperature / set_root_noise /
    set_move_temperature) on a fresh engine; nothing asked for, nothing set"""
    if root_policy_temperature is not None:
        eng.set_root_policy_temperature(root_policy_temperature)
    if root_noise is not None:
        total_alpha, shaped = root_noise if isinstance(root_noise, (tuple, list)) else (root_noise, False)
        eng.set_root_noise(total_alpha, shaped)
    if move_temperature is not None:
        eng.set_move_temperature(move_temperature)


def _apply_search_options(eng, starts, playout_cap, forced_playouts, prune_targets, gumbel, gumbel_c_visit, gumbel_c_scale,
                          targets_only_arena=False, fpu=None, c_base=0.0, root_policy_temperature=None, root_noise=None,
                          move_temperature=None, lcb=None, puct_variance=None, ko_rule=None):
    """selfplay()'s and train()'s search options on a fresh engine (train(): a targets-only arena under the cap)"""
    _refuse_two_root_rules(gumbel, forced_playouts)
    _apply_puct(eng, fpu, c_base)
    _apply_uncertainty(eng, lcb, puct_variance)
    _apply_ko_rule(eng, ko_rule)
    _apply_explore(eng, root_policy_temperature, root_noise, move_temperature)
    if starts:
        eng.set_starts(starts)
    if playout_cap is not None:
        eng.set_playout_cap(*playout_cap)
        if targets_only_arena:
            eng.replay_set_targets_only(playout_cap[0] > 0)
    if forced_playouts:
        eng.set_forced_playouts(forced_playouts, prune_targets)
    if gumbel:
        eng.set_gumbel(gumbel, gumbel_c_visit, gumbel_c_scale)


def seed(s):
    """Random.seed!(s) for selfplay(): restarts the game-id stream at 0 under draw-stream seed `s`"""
    _stream["seed"], _stream["next_game"] = int(s), 0


def selfplay(env, nn, num_ro=800, games=None, seed=None, slots=None, precision="f32", game_id_base=None, symmetry=None,
             starts=None, playout_cap=None, forced_playouts=None, prune_targets=True, gumbel=None, gumbel_c_visit=50.0,
             gumbel_c_scale=1.0, fpu=None, c_base=0.0, root_policy_temperature=None, root_noise=None,
             move_temperature=None, lcb=None, puct_variance=None, ko_rule=None, **cfg):
    """selfplay(env, nn, num_ro) (src/selfplay.jl:1-45) -> the finished game's player (SelfPlayPlayer), exactly the
    call train() makes (train.jl:57).  `games=G` (ours) plays G games concurrently on the device and returns a list of
    G such players ordered by game id.  Game ids continue from the previous call (module stream, `seed()`), unless
    `seed` / `game_id_base` pin them.  precision="f16" plays with the fp16-operand tower; default exact f32.
    symmetry (ours): None (the reference's search), "random" (every leaf evaluated under a drawn board symmetry) or a
    fixed s in 0..7 (Engine.set_symmetry).  starts (ours): a list of Positions; the game with id gid begins at
    starts[gid % len(starts)] (initialize_game!(player, pos), mcts_play.jl:110-118) instead of the empty board, and its
    player carries that Position as `.start` (Engine.set_starts).  playout_cap (ours): (r, p) -- playout cap
    randomization (Engine.set_playout_cap): a move is searched in full (noise, num_ro readouts) with probability p and
    otherwise fast (no noise, r readouts, an all-zero searches_pi row); the player's `full_search` tells which.
    forced_playouts (ours): k -- forced playouts (Engine.set_forced_playouts; KataGo plays 2): in a full search a visited
    root child below sqrt(k P sum(N)) visits is searched first; prune_targets (default on with k) records the searches_pi
    row with the forced visits the search did not agree with left out.
    gumbel (ours): m -- the Gumbel root search (Engine.set_gumbel) in the full searches: up to m root candidates by
    Gumbel-top-k, Sequential Halving, the searches_pi row is softmax(log prior + sigma(q)); gumbel_c_visit and
    gumbel_c_scale are sigma's constants.  It composes with playout_cap, starts and symmetry, not with forced_playouts.
    fpu and c_base (ours): the PUCT rule options of Engine.set_puct -- first-play urgency reduction, r or (r, r_root),
    and the c_puct growth constant -- at every level of every search; they compose with all of the above.
    root_policy_temperature, root_noise, move_temperature (ours): T or (early, late, halflife) -- a softmax temperature on
    the root prior of a full search; (total_alpha, shaped) -- its Dirichlet noise over the legal moves only, shaped by the
    prior as in KataGo; T or (early, late, halflife) -- the move is sampled in proportion to N^(1/T(n)) (Engine.set_root_
    policy_temperature / set_root_noise / set_move_temperature).  Gumbel and fast searches get no root rule."""
    _refuse_two_root_rules(gumbel, forced_playouts)
    single = games is None
    games = 1 if single else int(games)
    if seed is None:
        seed = _stream["seed"]
        if game_id_base is None:
            game_id_base = _stream["next_game"]
            _stream["next_game"] += games
    if game_id_base is None:
        game_id_base = 0
    slots = min(games, 1024) if slots is None else slots
    eng = Engine(board_size=env.N, tower_height=nn.tower_height, games=slots, num_readouts=num_ro, seed=seed,
                 game_id_base=game_id_base, record_capacity_games=games + 8, **cfg)
    nn.engine.copy_weights_to(eng)
    eng.set_precision(precision)
    if symmetry is not None:
        eng.set_symmetry(symmetry)
    _apply_search_options(eng, starts, playout_cap, forced_playouts, prune_targets, gumbel, gumbel_c_visit, gumbel_c_scale,
                          fpu=fpu, c_base=c_base, lcb=lcb, puct_variance=puct_variance, ko_rule=ko_rule, root_policy_temperature=root_policy_temperature, root_noise=root_noise,
                          move_temperature=move_temperature)
    eng.start(games)
    while eng.records_count() < games:
        eng.step(16)
        if eng.stats()["stalled_games"]:      # only with pool_policy = AGZ_POOL_STALL: a game waits on its full pool
            eng.close()
            raise _lib.AgzError(_lib.POOL_EXHAUSTED, "a game is waiting on a full node pool (pool_policy = stall): raise "
                                                     "max_nodes_per_game or use the default policy")
    out = [SelfPlayPlayer(env, nn, num_ro, r, starts[r["start"]] if starts else None) for r in eng.records()]
    eng.close()
    return out[0] if single else out


# One position's result of analyze(): the move suggest_move would pick (board coordinates, None = pass; also None when
# status is not OK and no move was picked), the root's N, W, Q and its child rows, status (_lib.OK, BAD_ARGUMENT,
# POOL_EXHAUSTED, ASSERT_SOFTPICK; include/agz.h agz_analysis), the tree's size and the draw-stream game id
Analysis = namedtuple("Analysis", "move N W Q child_N child_W child_Q prior status nodes_used game_id")


# One candidate move of an analysed node with its principal variation (include/agz.h agz_line): move and
# the pv entries as board coordinates (None = pass, pv[0] = move), N / W / prior = the candidate's entries of the node's
# rows, Q = W / (1 + N), pv_N[d] = the child_N entry pv[d] was chosen by, end_Q = Q of the line's last move
Line = namedtuple("Line", "move N W Q prior pv pv_N end_Q")
# a row of analyze() / review() with lines > 0: Analysis's fields, then the list of Line (at most `lines` of them)
AnalysisLines = namedtuple("AnalysisLines", Analysis._fields + ("lines",))


# a row of analyze() / review() with the value moments on (lcb= / puct_variance=): the same tuple, and beside it the
# attributes child_S (the root's row of squared-value sums) and root_S (the root's own)
class AnalysisS(Analysis):
    pass


class AnalysisLinesS(AnalysisLines):
    pass


def _with_S(row, child_S, root_S):
    out = (AnalysisLinesS if isinstance(row, AnalysisLines) else AnalysisS)(*row)
    out.child_S, out.root_S = child_S, root_S
    return out


def _check_lines(lines, pv_depth, pv_min_visits):
    for name, v in (("lines", lines), ("pv_depth", pv_depth), ("pv_min_visits", pv_min_visits)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer")
    if not 0 <= lines <= 16:
        raise ValueError("lines must be in 0..16")
    if not 1 <= pv_depth <= 64:
        raise ValueError("pv_depth must be in 1..64")
    if pv_min_visits < 1:
        raise ValueError("pv_min_visits must be >= 1")


def _line_rows(env, t):
    """the Line list of one row of the tables Engine.analyze_lines / tree_lines return ([K], [K][D])"""
    out = []
    one = np.float32(1)
    for k in range(len(t["move"])):
        n = int(t["pv_len"][k])
        if t["move"][k] < 0 or n < 1:
            continue
        pvn = t["pv_N"][k, :n].copy()
        out.append(Line(from_flat(int(t["move"][k]), env), t["N"][k], t["W"][k], t["W"][k] / (one + t["N"][k]),
                        t["prior"][k], [from_flat(int(a), env) for a in t["pv"][k, :n]], pvn,
                        t["end_W"][k] / (one + pvn[-1])))
    return out


def analyze(env, nn, positions, num_readouts=800, seed=0, game_id_base=0, slots=None, two_player_mode=False,
            symmetry=None, precision="f32", lines=0, pv_depth=16, pv_min_visits=1, fpu=None, c_base=0.0,
            move_temperature=None, lcb=None, puct_variance=None, ko_rule=None, **cfg):
    """suggest_move over many positions in one device run (ours).  Record i is what
    `MCTSPlayer(env, nn, num_readouts, two_player_mode, seed=seed, game_id=game_id_base + i, symmetry=symmetry)`,
    `initialize_game(positions[i])`, `suggest_move()` computes (mcts_play.jl:110-118,144-151), bit for bit, except that
    an invalid board gives status BAD_ARGUMENT instead of a search, and that a position whose last two moves were passes
    is a finished root, as in the reference (MCTSNode keeps pos.done).  `slots` trees search at once (default
    min(len(positions), 1024)); a slot that finishes a position takes the next.  `cfg`: further agz_config fields
    (parallel_readouts = tree_search!'s 8 by default, max_nodes_per_game, pool_policy, ...).
    lines > 0 (at most 16): the rows are AnalysisLines, i.e. Analysis plus `lines`, the root's top candidates with
    principal variations of at most pv_depth moves taken when the search ended (pv_min_visits 1 walks
    like most_visited_path, 2 like mvp_gg); everything else in the row is what lines = 0 gives.
    move_temperature (ours): T or (early, late, halflife), with two_player_mode off -- the suggested move is sampled in
    proportion to N^(1/T(n)) as Engine.set_move_temperature states it; record i is then what the MCTSPlayer above computes
    when it is given the same move_temperature.  The search and the rows do not change."""
    _check_lines(lines, pv_depth, pv_min_visits)
    positions = list(positions)
    for k, p in enumerate(positions):
        if not isinstance(p, Position):
            raise TypeError(f"positions[{k}] is {type(p).__name__}, not a Position")
        if p.env.N != env.N:
            raise ValueError(f"positions[{k}] is a {p.env.N}x{p.env.N} position, env is {env.N}x{env.N}")
    if int(num_readouts) < 1:
        raise ValueError("num_readouts must be >= 1")
    if not positions:
        return []
    B, P = len(positions), env.N * env.N
    slots = min(B, 1024) if slots is None else int(slots)
    if slots < 1:
        raise ValueError("slots must be >= 1")
    if not isinstance(nn, NeuralNet):
        raise TypeError("analyze needs a NeuralNet of this package (the search runs on the device with its weights)")
    boards = np.zeros((B, P), np.int8)
    hist = np.zeros((B, 7, P), np.int8)
    infos = (_lib.PositionInfo * B)()
    for k, p in enumerate(positions):
        boards[k], infos[k], h = position_arrays(p)
        hist[k, :len(h)] = h
    # one search per tree, no re-rooting: a tree holds at most 1 + R + 2 * parallel_readouts nodes
    cfg.setdefault("max_nodes_per_game", 2 * int(num_readouts) + 256)
    eng = Engine(board_size=env.N, tower_height=nn.tower_height, games=slots, num_readouts=int(num_readouts),
                 seed=seed, two_player_mode=int(two_player_mode), **cfg)
    try:
        nn.engine.copy_weights_to(eng)
        eng.set_precision(precision)
        if symmetry is not None:
            eng.set_symmetry(symmetry)
        _apply_puct(eng, fpu, c_base)      # the PUCT rule options of Engine.set_puct, as MCTSPlayer(fpu=, c_base=)
        _apply_uncertainty(eng, lcb, puct_variance)
        _apply_ko_rule(eng, ko_rule)
        _apply_explore(eng, move_temperature=move_temperature)      # pick_move's, as MCTSPlayer(move_temperature=)
        if lines:
            eng.analyze_set_lines(lines, pv_depth, pv_min_visits)
        eng.analyze_start(boards, infos, hist, game_id_base)
        while eng.analyze_progress() < B:
            eng.step(16)
            if eng.stats()["stalled_games"]:      # pool_policy = AGZ_POOL_STALL: a slot waits on its full pool
                raise _lib.AgzError(_lib.POOL_EXHAUSTED, "a search is waiting on a full node pool (pool_policy = "
                                                         "stall): raise max_nodes_per_game or use the default policy")
        r = eng.analyze_results()
        t = eng.analyze_lines() if lines else None
        S = eng.analyze_child_S() if (lcb is not None or puct_variance is not None) else None
    finally:
        eng.close()
    out = []
    for k in range(B):
        cn, cw = r["child_N"][k], r["child_W"][k]
        a = Analysis(None if r["move"][k] < 0 else from_flat(int(r["move"][k]), env), r["N"][k], r["W"][k],
                     r["Q"][k], cn, cw, cw / (np.float32(1) + cn), r["prior"][k], int(r["status"][k]),
                     int(r["nodes_used"][k]), int(game_id_base) + k)
        a = AnalysisLines(*a, _line_rows(env, {f: v[k] for f, v in t.items()})) if lines else a
        out.append(a if S is None else _with_S(a, S[0][k], S[1][k]))
    return out


def review_arrays(env, games):
    """Recorded games in agz_review_start's terms: (moves int16 [total], game_offset int64 [G+1]).  A game is a move list
    (board coordinates, None = pass, or flat actions 0..N*N), a record dict of Engine.records() (its "moves") or a
    player selfplay() returned (its .moves)."""
    P = env.N * env.N
    flat, off = [], [0]
    for j, g in enumerate(games):
        if isinstance(g, SelfPlayPlayer):
            seq = g.moves
        elif isinstance(g, dict):
            if "moves" not in g:
                raise TypeError(f"games[{j}] is a dict without 'moves'")
            seq = g["moves"]
        elif isinstance(g, (list, tuple, np.ndarray)):
            seq = g
        else:
            raise TypeError(f"games[{j}] is {type(g).__name__}, not a move list, a record dict or a selfplay() player")
        for k, m in enumerate(seq):
            if m is None:
                a = P
            elif isinstance(m, (int, np.integer)) and not isinstance(m, bool):
                a = int(m)
            elif isinstance(m, (tuple, list, np.ndarray)) and len(m) == 2:
                r, c = int(m[0]), int(m[1])
                if not (0 <= r < env.N and 0 <= c < env.N):
                    raise ValueError(f"games[{j}] move {k}: {tuple(m)} is off the {env.N}x{env.N} board")
                a = to_flat((r, c), env)
            else:
                raise TypeError(f"games[{j}] move {k}: {m!r} is neither a coordinate pair, None nor a flat action")
            if not 0 <= a <= P:
                raise ValueError(f"games[{j}] move {k}: action {a} is not in 0..{P}")
            flat.append(a)
        off.append(len(flat))
    return np.array(flat, np.int16), np.array(off, np.int64)


def review(env, nn, games, num_readouts=800, starts=None, two_player_mode=True, seed=0, game_id_base=0, slots=None,
           symmetry=None, precision="f32", lines=0, pv_depth=16, pv_min_visits=1, fpu=None, c_base=0.0,
           move_temperature=None, lcb=None, puct_variance=None, ko_rule=None, **cfg):
    """Batched game review (ours; the loop of play(), src/play.jl:25-77, over recorded games): for game j, what
    `p = MCTSPlayer(env, nn, num_readouts, two_player_mode, seed=seed, game_id=game_id_base + j, symmetry=symmetry)`,
    `p.initialize_game(starts[j])`, then for every recorded move m_k `p.suggest_move()` and `p.play_move(m_k)` compute,
    bit for bit: one list of Analysis per game, entry k taken at the k-th suggest_move (the move picked, the root's N, W,
    Q and rows).  The recorded move, not the suggested one, re-roots the tree, so its subtree is kept.  games: move lists
    (coordinates / None / flat actions), Engine.records() dicts or selfplay() players.  starts: None (every game from the
    empty board with agz_config.komi) or one Position (or None) per game.  A recorded move that cannot be played (illegal,
    or after the game ended) gives its ply and every later one of that game status BAD_ARGUMENT, move None; the earlier
    plies and the other games are not affected.  `slots` trees search at once (default min(len(games),
    1024)).  `cfg`: further agz_config fields (parallel_readouts, max_nodes_per_game, pool_policy, komi, ...).
    lines > 0: the rows are AnalysisLines as in analyze(); the lines of ply k are taken when its search ended, before
    the recorded move re-roots the tree.
    move_temperature (ours): T or (early, late, halflife); with two_player_mode=False the suggested move of every ply is
    sampled in proportion to N^(1/T(n)) (Engine.set_move_temperature), as the MCTSPlayer above suggests it when it is
    given the same move_temperature; under the default two_player_mode=True it changes nothing."""
    _check_lines(lines, pv_depth, pv_min_visits)
    games = list(games)
    moves, off = review_arrays(env, games)
    if starts is not None:
        starts = list(starts)
        if len(starts) != len(games):
            raise ValueError(f"{len(starts)} starts for {len(games)} games")
        for k, p in enumerate(starts):
            if p is not None and not isinstance(p, Position):
                raise TypeError(f"starts[{k}] is {type(p).__name__}, not a Position")
            if p is not None and p.env.N != env.N:
                raise ValueError(f"starts[{k}] is a {p.env.N}x{p.env.N} position, env is {env.N}x{env.N}")
    if isinstance(num_readouts, bool) or not isinstance(num_readouts, (int, np.integer)) or int(num_readouts) < 1:
        raise ValueError("num_readouts must be an integer >= 1")
    if not games:
        return []
    G, P = len(games), env.N * env.N
    slots = min(G, 1024) if slots is None else int(slots)
    if slots < 1:
        raise ValueError("slots must be >= 1")
    if not isinstance(nn, NeuralNet):
        raise TypeError("review needs a NeuralNet of this package (the search runs on the device with its weights)")
    boards = infos = hist = None
    if starts is not None:
        boards = np.zeros((G, P), np.int8)
        hist = np.zeros((G, 7, P), np.int8)
        infos = (_lib.PositionInfo * G)()
        for k, p in enumerate(starts):
            p = Position(env, komi=cfg.get("komi", 7.5)) if p is None else p
            boards[k], infos[k], h = position_arrays(p)
            hist[k, :len(h)] = h
    # trees are re-rooted and kept, as in self-play: the engine's default pool (agz_config.max_nodes_per_game)
    eng = Engine(board_size=env.N, tower_height=nn.tower_height, games=slots, num_readouts=int(num_readouts),
                 seed=seed, two_player_mode=int(two_player_mode), **cfg)
    try:
        nn.engine.copy_weights_to(eng)
        eng.set_precision(precision)
        if symmetry is not None:
            eng.set_symmetry(symmetry)
        _apply_puct(eng, fpu, c_base)      # the PUCT rule options of Engine.set_puct, as MCTSPlayer(fpu=, c_base=)
        _apply_uncertainty(eng, lcb, puct_variance)
        _apply_ko_rule(eng, ko_rule)
        _apply_explore(eng, move_temperature=move_temperature)      # pick_move's, as MCTSPlayer(move_temperature=)
        if lines:
            eng.analyze_set_lines(lines, pv_depth, pv_min_visits)
        eng.review_start(moves, off, boards, infos, hist, game_id_base)
        return _review_rows(env, eng, off, [int(game_id_base) + j for j in range(G)], lines,
                            with_S=lcb is not None or puct_variance is not None)
    finally:
        eng.close()


def _review_rows(env, eng, off, game_ids, lines, with_S=False):
    """The loop behind review() and reanalyze(): step the review run on `eng` until its off[-1] rows are finished, then
    read them as one list of Analysis (AnalysisLines with lines on) per game: game j's rows off[j] .. off[j + 1] - 1."""
    total = int(off[-1])
    while eng.review_progress() < total:
        eng.step(16)
        if eng.stats()["stalled_games"]:      # pool_policy = AGZ_POOL_STALL: a slot waits on its full pool
            raise _lib.AgzError(_lib.POOL_EXHAUSTED, "a search is waiting on a full node pool (pool_policy = "
                                                     "stall): raise max_nodes_per_game or use the default policy")
    r = eng.review_results()
    t = eng.analyze_lines() if lines else None
    S = eng.analyze_child_S() if with_S else None
    out = []
    for j, gid in enumerate(game_ids):
        rows = []
        for i in range(int(off[j]), int(off[j + 1])):
            cn, cw = r["child_N"][i], r["child_W"][i]
            a = Analysis(None if r["move"][i] < 0 else from_flat(int(r["move"][i]), env), r["N"][i], r["W"][i],
                         r["Q"][i], cn, cw, cw / (np.float32(1) + cn), r["prior"][i], int(r["status"][i]),
                         int(r["nodes_used"][i]), gid)
            a = AnalysisLines(*a, _line_rows(env, {f: v[i] for f, v in t.items()})) if lines else a
            rows.append(a if S is None else _with_S(a, S[0][i], S[1][i]))
        out.append(rows)
    return out


def reanalyze(engine, first=0, count=None, game_id_base=0, commit=True, lines=0, pv_depth=0, pv_min_visits=1):
    """Reanalyse (ours; MuZero's): search games first .. first + count - 1 of `engine`'s replay arena
    again on its current network and write the new targets over the records.  The search is review()'s, on the engine's
    own num_readouts, network and pool, with the games gathered on the device: game j from its entry of the start table,
    draw-stream game id game_id_base + its record's game_id, so the rows of a game depend neither on its place in the
    arena nor on the range.  commit: every row with status OK writes qs[k] = Q and -- unless the record's row is all
    zero, which means "no policy target" and stays so -- its pi row children_as_pi(root, n <= tau_threshold); short,
    invalid and given-up rows leave the record alone.  Moves, results, the arena's order and its window stay.  The run
    takes over the engine's slots: self-play games in flight are dropped.  lines > 0: AnalysisLines rows, as in review()
    (pv_depth 0: review()'s default of 16); the call leaves the engine's analyze_set_lines setting at these values.
    Returns (counts, rows): counts = dict(committed, pi_rows, skipped) in rows (None with commit=False), rows = one list
    of Analysis per game as review() gives them."""
    pv_depth = pv_depth or 16
    _check_lines(lines, pv_depth, pv_min_visits)
    engine.analyze_set_lines(lines, pv_depth, pv_min_visits)
    engine.reanalyze_start(first, count, game_id_base)
    ids = [int(game_id_base) + int(g) for g in engine.reanalyze_game_ids()]
    rows = _review_rows(GoEnv(engine.N), engine, engine.reanalyze_offsets(), ids, lines)
    return (engine.reanalyze_commit() if commit else None), rows


EvalStats = namedtuple("EvalStats", "games_won num_games win_rate resigned moves records")


def evaluate(env, black_net, white_net, num_games=400, ro=800, verbose=False, seed=0, slots=None,
             return_stats=False, symmetry=None, starts=None, fpu=None, c_base=0.0, lcb=None, puct_variance=None, ko_rule=None, **cfg):
    """evaluate(env, black_net, white_net; num_games, ro) (src/neural_net.jl:103-158): black_net plays
    Black and white_net White in `num_games` games of two two_player_mode MCTSPlayers (arg-max moves,
    no noise, resign at -0.9); True iff Black's win rate reaches 0.55.  All games run concurrently on
    the device (arena_mode: one slot pair per game, both networks resident).  The tally follows the
    reference literally: a game counts for Black when `result(black.root.position) == BLACK`, i.e.
    by the Tromp-Taylor score of the final position, also after a resignation (:147).  symmetry (ours): as for
    selfplay(), applied to both networks' evaluations.  starts (ours): an opening suite -- game g begins at the Position
    starts[g % len(starts)] with komi, stones and side to move as given there; the player of the colour to move searches
    first, black_net still plays Black.  The records (return_stats) carry the entry as `start`.  fpu and c_base (ours):
    the PUCT rule options of Engine.set_puct, for both players."""
    if black_net.tower_height != white_net.tower_height:
        raise ValueError("the arena keeps both networks in one engine: tower heights must match")
    pairs = min(num_games, 512) if slots is None else slots
    eng = Engine(board_size=env.N, tower_height=black_net.tower_height, games=2 * pairs, num_readouts=ro, seed=seed,
                 arena_mode=1, record_capacity_games=num_games + 8, **cfg)
    black_net.engine.copy_weights_to(eng)
    eng.net_select(1)
    white_net.engine.copy_weights_to(eng)
    eng.net_select(0)
    if symmetry is not None:
        eng.set_symmetry(symmetry)
    _apply_puct(eng, fpu, c_base)
    _apply_uncertainty(eng, lcb, puct_variance)
    _apply_ko_rule(eng, ko_rule)
    if starts:
        eng.set_starts(starts)
    eng.start(num_games)
    while eng.records_count() < num_games:
        eng.step(16)
        if eng.stats()["pool_exhausted"]:
            eng.close()
            raise _lib.AgzError(_lib.POOL_EXHAUSTED, "node pool exhausted; raise max_nodes_per_game")
    recs = eng.records()
    st = eng.stats()
    eng.close()
    if st["pool_exhausted"]:
        raise _lib.AgzError(_lib.POOL_EXHAUSTED, "node pool exhausted; raise max_nodes_per_game")
    games_won = sum(1 for r in recs if r["final_score"] > 0)
    rate = games_won / num_games
    if verbose:
        print(f"Won {games_won} / {num_games}. Win rate: {rate}. ", end="")
    ok = rate >= 0.55
    if return_stats:
        return ok, EvalStats(games_won, num_games, rate, sum(int(r["was_resign"]) for r in recs),
                             sum(int(r["num_moves"]) for r in recs), recs)
    return ok


def extract_data(player, record=None, targets_only=False, value_target=None):
    """extract_data(player) -> (positions, pis, results), mcts_play.jl:126-139: one argument, the player selfplay()
    returned or a live MCTSPlayer (train.jl:58).  The round <= 5 form extract_data(env, record) for a bare GameRecord
    is still accepted.  targets_only=True (ours, for selfplay(..., playout_cap=...) players) drops the plies of fast
    searches -- the all-zero pi rows -- from all three lists; the default keeps every ply, zero rows included.
    value_target=(alpha, lam) (ours): `results` is the per-ply vector of value targets y_t (float32) -- the result blended
    with the TD(lam) return of the player's recorded qs from that ply on (Engine.replay_set_value_target; a kept ply sums
    the qs of the dropped plies behind it) -- instead of the constant fill; None: the result, as the reference."""
    if record is None:
        kw = {} if value_target is None else dict(value_target=value_target)
        return player.extract_data(targets_only=True, **kw) if targets_only else player.extract_data(**kw)
    env, pos, positions = player, Position(player), []
    for c in record.moves:
        positions.append(pos)
        pos = pos.play_move(c)
    return positions, [np.array(p) for p in record.searches_pi], [record.result] * len(positions)


def get_replay_batch(pos_buffer, pi_buffer, res_buffer, batch_size=32, rng=None):
    """get_replay_batch(pos_buffer, pi_buffer, res_buffer; batch_size), src/train.jl:4-12: `batch_size` distinct
    entries (sample(..., replace=false)); pi_replay = hcat(...) is A x B.  (alphago.jl_amd.ReplayBuffer is the same
    contract with positions kept as move lists and rebuilt on the device.)"""
    rng = np.random.default_rng() if rng is None else rng
    idxs = rng.choice(len(pos_buffer), size=batch_size, replace=False)
    return ([pos_buffer[i] for i in idxs], np.stack([pi_buffer[i] for i in idxs], axis=1),
            [res_buffer[i] for i in idxs])


class Momentum:
    """Flux.Momentum(eta, rho = 0.9) (train.jl:54): the state lives in the network's engine (agz_train_step)"""

    def __init__(self, eta=0.01, rho=0.9):
        self.eta, self.rho = float(eta), float(rho)


def _train(nn, input_data, opt, epochs=1):
    """_train(nn, (positions, pi A x B, z), opt; epochs) (src/neural_net.jl:85-101; call train.jl:70) as intended (the
    reference's does not run at HEAD): minibatches of 32 positions (a short tail is its own batch; a single
    left-over position joins the batch before it: BatchNorm needs two), each one agz_train_step on the device --
    training-mode forward, 0.01 crossentropy + 0.01 mse + 1e-4 sum(theta^2), backward, Momentum update.  Returns the
    summed minibatch loss / epochs (:98-100).  Features come from agz_features on the positions' own fields."""
    positions, pi, z = input_data
    pi = np.asarray(pi, np.float32)
    z = np.asarray(z, np.float32)
    e = nn.engine
    soa = [p.soa() for p in positions]
    feats = e.features(np.stack([s[0] for s in soa]), np.stack([s[1] for s in soa]), [s[2] for s in soa],
                       [s[3] for s in soa])
    n = len(positions)
    cuts = list(range(0, n, 32)) + [n]
    if len(cuts) > 2 and cuts[-1] - cuts[-2] == 1:
        del cuts[-2]
    loss_avg = 0.0
    for _ in range(epochs):
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            loss_avg += float(e.train_step(feats[lo:hi], pi[:, lo:hi].T, z[lo:hi], eta=opt.eta, rho=opt.rho)[0])
    return loss_avg / epochs


def _result_string(h):
    """player.result_string of a finished game from its record header (mcts_play.jl:100-108, board.jl:546-555)"""
    if h["was_resign"]:
        return "B+R" if h["result"] == BLACK else "W+R"
    sc = float(h["final_score"])
    return f"B+{sc:.1f}" if sc > 0 else f"W+{-sc:.1f}" if sc < 0 else "DRAW"


def _minibatch_cuts(n):
    """_train's chunking (api._train): 32-position minibatches, a single left-over position joins the one before it"""
    cuts = list(range(0, n, 32)) + [n]
    if len(cuts) > 2 and cuts[-1] - cuts[-2] == 1:
        del cuts[-2]
    return cuts


def train(env, num_games=25000, memory_size=500000, batch_size=32, epochs=1, ckp_freq=1000, readouts=800,
          tower_height=19, model=None, start_training_after=50000, slots=None, seed=0, game_id_base=0, symmetry=None,
          augment=False, precision="f32", checkpoint_dir=None, callback=print, return_log=False, profile=None, starts=None,
          playout_cap=None, forced_playouts=None, prune_targets=True, gumbel=None, gumbel_c_visit=50.0,
          gumbel_c_scale=1.0, value_target=None, fpu=None, c_base=0.0, surprise=0.0, root_policy_temperature=None,
          root_noise=None, move_temperature=None, lcb=None, puct_variance=None, ko_rule=None, **cfg):
    """train(env; num_games, memory_size, batch_size, epochs, ckp_freq, readouts, tower_height, model,
    start_training_after) (src/train.jl:38-92) with `slots` games in flight on the device.  One engine
    plays, keeps the replay arena and trains; per step: agz_selfplay_step(1), one read of how many games finished, and
    for each of them in game-id order: its record into the arena (device to device), the window set to the newest
    memory_size entries, the game counter i advanced, then -- once the window holds start_training_after entries --
    _train on a device-drawn get_replay_batch(batch_size) (agz_replay_sample with draw key (seed, i)) in `epochs` passes of
    32-position agz_train_step minibatches, Momentum(2f-2); every ckp_freq games a checkpoint.  Finished slots are held
    until the step's training is done, so every game starts on the weights the games finished before it left; slots = 1
    is the reference's sequential loop.  Ours: seed / game_id_base (the draw stream of the games: they are game ids
    game_id_base .. game_id_base + num_games - 1), symmetry (as in selfplay), augment (each sample under a drawn board symmetry), precision,
    checkpoint_dir (save_model into checkpoint_dir/game_<i> every ckp_freq games; None: no checkpoints), callback (what
    the reference prints goes here), return_log (also return one dict per game), profile (a dict filled with steps,
    wall_s, train_s, train_steps, positions and host_syncs: the library calls of the loop that synchronise the engine's
    stream, each at least once; tools/train_rate.py), starts (a list of Positions: the game with id gid begins at
    starts[gid % len(starts)], and the replay arena rebuilds its training positions from there; as in selfplay),
    playout_cap ((r, p): playout cap randomization as in selfplay, with a targets-only arena -- memory_size and
    start_training_after then count target entries, the plies of full searches, and only those are sampled),
    forced_playouts (k) and prune_targets (forced playouts and policy target pruning in the full searches, as in selfplay),
    gumbel (m), gumbel_c_visit and gumbel_c_scale (the Gumbel root search in the full searches, as in selfplay),
    value_target ((alpha, lam): the z of every training batch is (1 - alpha) * result + alpha * TD(lam) of the game's
    recorded root values from the sampled ply on, Engine.replay_set_value_target; None: the result, as the reference),
    fpu and c_base (the PUCT rule options of Engine.set_puct, as in selfplay), surprise (rho: policy surprise weighting --
    each game is scored right after it is filed, on the weights of that moment, and every training batch is drawn by
    weight, with replacement: per game a share 1 - rho of the sampling mass evenly over its target plies and rho in
    proportion to KL(pi || prior), Engine.replay_score / replay_set_surprise; 0: the uniform draw, as the reference),
    root_policy_temperature, root_noise and move_temperature (root exploration and the move temperature, as in selfplay).
    Returns the trained NeuralNet (model itself when given)."""
    import time
    import torch
    from . import bson_weights as bw
    import os
    num_games, batch_size, epochs = int(num_games), int(batch_size), int(epochs)
    if num_games < 1 or batch_size < 2 or epochs < 1 or int(ckp_freq) < 1:
        raise ValueError("num_games, epochs, ckp_freq >= 1 and batch_size >= 2 (BatchNorm needs two positions)")
    _refuse_two_root_rules(gumbel, forced_playouts)
    cur_nn = NeuralNet(env, tower_height=tower_height) if model is None else model       # train.jl:43
    slots = min(num_games, 1024) if slots is None else int(slots)
    if slots < 1:
        raise ValueError("slots must be >= 1")
    callback = callback or (lambda line: None)
    eng = Engine(board_size=env.N, tower_height=cur_nn.tower_height, games=slots, num_readouts=int(readouts), seed=seed,
                 game_id_base=game_id_base, record_capacity_games=slots + 8, **cfg)
    log = []
    try:
        cur_nn.engine.copy_weights_to(eng)
        eng.set_precision(precision)
        if symmetry is not None:
            eng.set_symmetry(symmetry)
        opt = Momentum(2e-2)                                                            # train.jl:54
        dev = torch.device("cuda", eng.cfg.device)
        feats = torch.empty((batch_size, 17 * eng.P), dtype=torch.float32, device=dev)
        pi = torch.empty((batch_size, eng.A), dtype=torch.float32, device=dev)
        z = torch.empty(batch_size, dtype=torch.float32, device=dev)
        cuts = _minibatch_cuts(batch_size)
        _apply_search_options(eng, starts, playout_cap, forced_playouts, prune_targets, gumbel, gumbel_c_visit,
                              gumbel_c_scale, targets_only_arena=True, fpu=fpu, c_base=c_base, lcb=lcb, puct_variance=puct_variance, ko_rule=ko_rule,
                              root_policy_temperature=root_policy_temperature, root_noise=root_noise,
                              move_temperature=move_temperature)
        if value_target is not None:
            eng.replay_set_value_target(*value_target)
        surprise = float(surprise)
        eng.replay_set_surprise(surprise)
        eng.set_hold(True)
        eng.start(num_games)
        eng.release()
        i = step = trained = claimed = 0
        started = {}                                   # game index -> (step of its first network call, trainings before)
        parked = slots
        t0, t_train, n_steps, n_pos, syncs = time.perf_counter(), 0.0, 0, 0, 0
        while i < num_games:
            take = min(parked, num_games - claimed)
            for k in range(claimed, claimed + take):
                started[k] = (step + 1, trained)
            claimed += take
            eng.step(1)
            step += 1
            n = eng.records_count()                    # the step's one synchronising read
            syncs += 1
            if n == 0:
                parked = 0
                if step % 256 == 0 and eng.stats()["stalled_games"]:
                    raise _lib.AgzError(_lib.POOL_EXHAUSTED, "a game is waiting on a full node pool (pool_policy = "
                                                             "stall): raise max_nodes_per_game or use the default policy")
                continue
            heads = sorted(((eng.record_header(k), k) for k in range(n)), key=lambda hk: hk[0]["game_id"])
            recs = {r["index"]: r for r in eng.records()} if return_log else None
            syncs += 2 * n + 1                         # n headers, n ingests, records_clear
            for h, k in heads:
                n_pos += int(h["num_moves"])
                eng.replay_ingest_records(k, 1)                                          # push_data, train.jl:60-61
                if surprise > 0.0:
                    eng.replay_score(eng.replay_count() - 1, 1)                          # on the weights of this moment
                    syncs += 1
                eng.replay_set_window(memory_size)                                       # shrink, train.jl:63-65
                i += 1
                loss = None
                if eng.replay_live_positions() >= start_training_after:                  # train.jl:67
                    t1 = time.perf_counter()
                    eng.replay_sample(batch_size, i, 8 if augment else -1, feats, pi, z)  # train.jl:68-69
                    loss = 0.0
                    for _ in range(epochs):                                              # _train, train.jl:70
                        for lo, hi in zip(cuts[:-1], cuts[1:]):
                            loss += float(eng.train_step_device(feats[lo:hi], pi[lo:hi], z[lo:hi], hi - lo, eta=opt.eta,
                                                                rho=opt.rho)[0])
                    loss /= epochs
                    t_train += time.perf_counter() - t1
                    n_steps += epochs * (len(cuts) - 1)
                    syncs += epochs * (len(cuts) - 1)     # each step returns its losses
                    trained += 1
                    callback(f"Episode {i} over. Loss: {loss}. Winner: {_result_string(h)}. "
                             f"Moves: {h['num_moves']}.")                                 # train.jl:71-73
                if i % int(ckp_freq) == 0 and checkpoint_dir is not None:              # train.jl:86-89
                    bw.write_checkpoint(os.path.join(checkpoint_dir, f"game_{i}"), bw.extract_param_lists(eng))
                    callback("Model saved. ")
                if return_log:
                    gi = int(h["game_id"]) - int(game_id_base)
                    log.append(dict(i=i, game_id=int(h["game_id"]), step=step, start_step=started[gi][0],
                                    trained_before_start=started[gi][1], trained_after=trained, loss=loss,
                                    live=eng.replay_live_positions(), record=recs[k]))
            eng.records_clear()
            eng.release()
            parked = n
        if profile is not None:
            profile.update(steps=step, wall_s=time.perf_counter() - t0, train_s=t_train, train_steps=n_steps,
                           positions=n_pos, host_syncs=syncs)
        eng.copy_weights_to(cur_nn.engine)
    finally:
        eng.close()
    return (cur_nn, log) if return_log else cur_nn
