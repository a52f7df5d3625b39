"""The PUCT rule options (agz_search_set_puct) restated in Python (TEST INFRASTRUCTURE).

puct_scores is the rule of include/agz.h in numpy: float32 exactly where the definition says Float32, Python floats
(float64) elsewhere, agz_log and agz_sqrt of include/agz_draws.h restated operation for operation (both use only + * /
and the exponent bits).  predict_phase walks a tree's rows from the root as one select phase does (mcts.jl:108-138 with
the pass-first rule and the tie draw of select_leaf, virtual losses between the descents) and says which leaves it must
return.  The oracle's select_leaf is the reference's rule and cannot stand in here.

The simulator it is compared with is hs.Sim (set_puct, puct_counts, scores, leaf_paths); the peaked deterministic network
the tests search with is hs.PeakedNet."""
import struct

import numpy as np

from alphago_jl_amd import symmetry as sy
from hs import bits64
from selfplay_twin import SITE_PUCT_TIE

f32, f64 = np.float32, np.float64
OFF = (0, 0.0, 0.0, 0.0)
TWO30 = 1073741824.0


# ---------------------------------------------------------------- agz_log / agz_sqrt, restated

def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def agz_log(x):
    """include/agz_draws.h agz_log: natural log of a finite x > 0"""
    x = float(x)
    e = 0
    b = _bits(x)
    if (b >> 52) == 0:
        x = x * 18014398509481984.0
        e = -54
        b = _bits(x)
    e += ((b >> 52) & 0x7FF) - 1023
    m = _from_bits((b & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000)
    if m > 1.4142135623730951:
        m = m * 0.5
        e += 1
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = 1.0 / 23.0
    for d in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = p * z + 1.0 / d
    p = p * z + 1.0
    lm = 2.0 * s * p
    return float(e) * 0.6931471805599453 + lm


def agz_sqrt(x):
    """include/agz_draws.h agz_sqrt: Newton on y = sqrt(x) from a power of two"""
    x = float(x)
    if x <= 0.0:
        return 0.0
    e = ((_bits(x) >> 52) & 0x7FF) - 1023
    y = 2.0 ** int(e / 2)               # C's e / 2 truncates towards zero
    if y * y > x:
        y = y * 0.5
    y = y * 1.2
    for _ in range(8):
        y = 0.5 * (y + x / y)
    return y


# ---------------------------------------------------------------- the rule

def puct_scale(n, c_puct, c_base):
    one = f32(1) + f32(n)
    root = float(np.sqrt(one))          # sqrtf: correctly rounded in float32
    if c_base > 0:
        c = float(c_puct) + agz_log((float(one) + float(c_base)) / float(c_base))
        return c * root
    return float(c_puct) * root


def fpu_mass(N_row, P_row):
    """M: the integer policy mass of the visited children, in units of 2^-30"""
    return sum(int(float(p) * TWO30) for n, p in zip(N_row, P_row) if n > 0)


def puct_scores(N_row, W_row, P_row, N_s, W_s, to_play, is_root, c_puct, setting):
    """the score of every action of a node with own statistics (N_s, W_s) under setting = (fpu_on, r, r_root, c_base):
    float64[A]"""
    fpu_on, r, r_root, c_base = setting
    N, W, P = (np.asarray(x, f32) for x in (N_row, W_row, P_row))
    tp = f32(to_play)
    scale = puct_scale(N_s, c_puct, c_base)
    denom = f32(1) + N
    qs = (W / denom) * tp
    assert qs.dtype == np.float32
    out = qs.astype(f64) + (f64(scale) * P.astype(f64)) / denom.astype(f64)
    if fpu_on:
        m = float(fpu_mass(N, P)) * (1.0 / TWO30)
        q_s = f32(W_s) / (f32(1) + f32(N_s))
        qp = q_s * tp
        assert type(qp) is np.float32
        rho = r_root if is_root else r
        f = f32(float(qp) - float(rho) * agz_sqrt(m))
        un = N == 0
        out[un] = (f64(f) + (f64(scale) * P.astype(f64)) / f64(f32(1)))[un]
    return out


# ---------------------------------------------------------------- one select phase, predicted from the rows

PASS_DONE, NEW = "done", "new"


class Shadow:
    """a copy-on-touch image of one simulator tree (slot g) that the predicted descents of one phase write to"""

    def __init__(self, sim, g=0):
        self.sim, self.g = sim, g
        G = sim.game(g)
        self.root = G.root
        self.own = {self.root: [f32(G.rootN), f32(G.rootW)]}       # node -> own [N, W]; other nodes: the parent's rows
        self.rows, self.kids, self.metas, self.new = {}, {}, {}, {}

    def meta(self, node):
        if node not in self.metas:
            m = self.sim.meta(self.g, node)
            self.metas[node] = dict(parent=m.parent, fmove=m.fmove, n=m.n, to_play=m.to_play, last_move=m.last_move,
                                    expanded=bool(m.flags & 1), done=bool(m.flags & 2) or m.n >= self.sim.mgl)
        return self.metas[node]

    def row(self, node):
        if node not in self.rows:
            self.rows[node] = [self.sim.row(self.g, node, k).copy() for k in range(3)]
            self.kids[node] = [int(c) for c in self.sim.children(self.g, node)]
        return self.rows[node]

    def stat(self, node):
        """(the list, the index) holding N of `node`; W is at the same place of the W list"""
        if node in self.own:
            return None
        m = self.meta(node)
        return m["parent"], m["fmove"]

    def get(self, node, k):
        where = self.stat(node)
        return self.own[node][k] if where is None else self.row(where[0])[k][where[1]]

    def add(self, node, k, x):
        where = self.stat(node)
        if where is None:
            self.own[node][k] = f32(self.own[node][k] + f32(x))
        else:
            r = self.row(where[0])[k]
            r[where[1]] = f32(r[where[1]] + f32(x))

    def child(self, node, a):
        """the child of `node` under a, created (as a key) when it is not there"""
        self.row(node)
        c = self.kids[node][a]
        if c >= 0:
            return c
        key = (NEW, node, a)
        if key not in self.metas:
            pm = self.meta(node)
            ps = self.sim.A - 1
            n = pm["n"] + 1
            self.metas[key] = dict(parent=node, fmove=a, n=n, to_play=-pm["to_play"], last_move=a, expanded=False,
                                   done=(a == ps and pm["last_move"] == ps) or n >= self.sim.mgl)
        return key


def descend(sh, c_puct, setting, seed, game_id, move_key, sel, counts):
    """one select_leaf from the root of the shadow tree -> the path [root .. leaf]"""
    sim, g = sh.sim, sh.g
    ps = sim.A - 1
    cur, depth, path = sh.root, 0, []
    while True:
        sh.add(cur, 0, 1.0)
        path.append(cur)
        m = sh.meta(cur)
        if not m["expanded"]:
            break
        N, W, P = sh.row(cur)
        if m["last_move"] == ps and N[ps] == 0:
            pick = ps
        else:
            sc = puct_scores(N, W, P, sh.get(cur, 0), sh.get(cur, 1), m["to_play"], cur == sh.root, c_puct, setting)
            lg = sim.legal(g, cur) != 0
            best = sc[lg].max()
            possible = np.flatnonzero(lg & (sc == best))
            pick = int(possible[0])
            if len(possible) > 1:
                bits = sy.draw_u64(seed, game_id, move_key, SITE_PUCT_TIE, sel * 1024 + depth)
                pick = int(possible[((bits >> 32) * len(possible)) >> 32])
                counts["ties"] += 1
            if setting != OFF:
                counts["levels"] += 1
                counts["unvisited"] += bool(N[pick] == 0)
        cur = sh.child(cur, pick)
        depth += 1
    return path


def predict_phase(sim, par, c_puct, seed, g=0):
    """the select phase the simulator is about to run on slot g (game_select_phase with no root rule): up to par leaves
    in 2 * par attempts, a virtual loss along each path, a finished leaf's result backed up at once.
    -> ([path [root .. leaf]] of the leaves in order, counts)"""
    sh = Shadow(sim, g)
    G = sim.game(g)
    move_key = sh.meta(sh.root)["n"]
    sel = G.sel
    counts = dict(levels=0, unvisited=0, ties=0, terminal=0)
    leaves, failsafe = [], 0
    while len(leaves) < par and failsafe < 2 * par:
        failsafe += 1
        path = descend(sh, c_puct, sim.setting, seed, G.game_id, move_key, sel, counts)
        sel += 1
        leaf = path[-1]
        lm = sh.meta(leaf)
        if lm["done"]:
            # only a double pass ends a game inside these small trees: the leaf's board is its parent's
            assert lm["last_move"] == sim.A - 1 and lm["n"] < sim.mgl and isinstance(lm["parent"], int)
            board = sim.board(g, lm["parent"]) if isinstance(leaf, tuple) else sim.board(g, leaf)
            score = sim.go_score(board[None, :], np.array([G.komi], f32))[0]
            value = 1.0 if score > 0 else -1.0 if score < 0 else 0.0
            for x in path:
                sh.add(x, 1, value)
            counts["terminal"] += 1
            continue
        for x in path:
            sh.add(x, 1, float(sh.meta(x)["to_play"]))
        leaves.append(path)
    return leaves, counts, sh


def assert_phase(sim, predicted, sh, g=0):
    """the leaves the simulator's select phase returned are the predicted ones: the leaf (a node that was there, or the
    new child of the predicted parent under the predicted action) and its parent chain; and every statistic the
    prediction touched is the simulator's, bit for bit"""
    got = sim.leaf_paths(g)
    assert len(got) == len(predicted), (len(got), len(predicted))
    ids = {}
    for (leaf, chain), want in zip(got, predicted):
        assert len(chain) == len(want) and chain[-1] == leaf, (chain, want)
        for x, y in zip(chain, want):
            if isinstance(y, tuple):
                m = sim.meta(g, x)
                parent = ids.get(y[1], y[1])
                assert (m.parent, m.fmove) == (parent, y[2]), (chain, want)
                assert ids.setdefault(y, x) == x
            else:
                assert x == y, (chain, want)
    for node, rows in sh.rows.items():
        for k in range(2):
            assert (sim.row(g, node, k).view(np.uint32) == rows[k].view(np.uint32)).all(), (node, k)
    G = sim.game(g)
    assert f32(G.rootN) == sh.own[sh.root][0] and f32(G.rootW).view(np.uint32) == sh.own[sh.root][1].view(np.uint32)
