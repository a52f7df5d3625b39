"""Value uncertainty (agz_search_set_value_moments / _set_lcb / _set_puct_variance) for the tests
(TEST INFRASTRUCTURE): the arithmetic of include/agz_uncertainty.h restated in numpy from the text of include/agz.h, a dict
mirror of the moment rule for trees driven one call at a time, and one select phase predicted from the rows.  The simulator
is hs.Sim, which has the three setters; gpu_options.configure sets them from a dict."""
import numpy as np

import alphago_jl_amd as ag
import hs
import puct_twin as pt

f32, f64 = np.float32, np.float64
OK, BAD_ARGUMENT = ag._lib.OK, ag._lib.BAD_ARGUMENT


# ---------------------------------------------------------------- the arithmetic, restated from include/agz.h

def lib_sqrt(x):
    return hs.lib().hs_sqrt(float(x))


def _sqrt_each(v, sqrt):
    return np.array([sqrt(float(x)) for x in np.atleast_1d(v)], f64)


def child_stats(N, W, S, sqrt=pt.agz_sqrt):
    """rule 1 on rows: (cnt, mean, var, sd), float64 each, every operation rounded on its own"""
    N, W, S = (np.atleast_1d(np.asarray(x, f32)) for x in (N, W, S))
    cnt = (f32(1) + N).astype(f64)
    mean = W.astype(f64) / cnt
    m2 = S.astype(f64) / cnt
    var = m2 - mean * mean
    var = np.where(var > 0, var, 0.0)
    return cnt, mean, var, _sqrt_each(var, sqrt)


def child_lcb(N, W, S, tp, z, sqrt=pt.agz_sqrt):
    """rule 2 on rows: (mean, sd, lcb)"""
    cnt, mean, var, sd = child_stats(N, W, S, sqrt)
    q = mean * f64(f32(tp))
    return mean, sd, q - f64(z) * _sqrt_each(var / cnt, sqrt)


def variance_factor(n, W_s, S_s, k, prior, pw, sqrt=pt.agz_sqrt):
    """rule 3 of a node with own (n, W_s, S_s)"""
    cnt = f64(f32(1) + f32(n))
    mean = f64(f32(W_s)) / cnt
    m2 = f64(f32(S_s)) / cnt
    k, prior, pw = f64(k), f64(prior), f64(pw)
    var = ((((mean * mean) + (prior * prior)) * pw) + (m2 * cnt)) / (pw + cnt) - (mean * mean)
    if not var > 0:
        var = f64(0)
    return float(f64(1) + k * ((f64(sqrt(float(var))) / prior) - f64(1)))


def lcb_pick(N, W, S, tp, lcb, sqrt=pt.agz_sqrt):
    """the LCB rule on a root's rows: the action, or None where the arg-max branch runs as it is (max N < min_visits)"""
    z, mv, ratio = lcb
    N = np.asarray(N, f32)
    mx = N.max()
    if mx < mv:
        return None
    el = (N >= mv) & (N.astype(f64) >= f64(ratio) * f64(mx))
    _, _, l = child_lcb(N, W, S, tp, z, sqrt)
    best = l[el].max()
    cand = np.flatnonzero(el & (l == best))
    top = N[cand].max()
    return int(cand[N[cand] == top][0])


def scores(N_row, W_row, P_row, N_s, W_s, S_s, to_play, is_root, c_puct, setting, pv, sqrt=pt.agz_sqrt):
    """pt.puct_scores with the scale multiplied by the variance factor pv = (k, prior, weight) of the node's own
    (N_s, W_s, S_s); pv = None: pt.puct_scores"""
    if pv is None or not pv[0] > 0:
        return pt.puct_scores(N_row, W_row, P_row, N_s, W_s, to_play, is_root, c_puct, setting)
    fpu_on, r, r_root, c_base = setting
    N, W, P = (np.asarray(x, f32) for x in (N_row, W_row, P_row))
    tp = f32(to_play)
    scale = f64(pt.puct_scale(N_s, c_puct, c_base)) * f64(variance_factor(N_s, W_s, S_s, *pv, sqrt=sqrt))
    denom = f32(1) + N
    qs = (W / denom) * tp
    out = qs.astype(f64) + (scale * P.astype(f64)) / denom.astype(f64)
    if fpu_on:
        m = float(pt.fpu_mass(N, P)) * (1.0 / pt.TWO30)
        qp = (f32(W_s) / (f32(1) + f32(N_s))) * tp
        f = f32(float(qp) - float(r_root if is_root else r) * pt.agz_sqrt(m))
        un = N == 0
        out[un] = (f64(f) + (scale * P.astype(f64)) / f64(f32(1)))[un]
    return out


# ---------------------------------------------------------------- the moment rule on a dict

class MomentMirror:
    """The S of one simulator tree (slot g) kept by rule 1 of include/agz.h in float32, in the order the engine stores:
    rows[node] = the S row of the node's children (a node's own S is its entry in its parent's row), root_S the root's
    own.  The caller reports every call it makes on the tree; `check` holds the simulator to the mirror bit for bit."""

    def __init__(self, sim, g=0):
        self.sim, self.g = sim, g
        self.rows, self.root, self.root_S = {}, -1, f32(0)

    def init(self, root):
        self.rows, self.root, self.root_S = {root: np.zeros(self.sim.A, f32)}, root, f32(0)

    def created(self, node):
        """a node that select_leaf or add_child made (or a pool entry used again): its row is zeroed"""
        self.rows[node] = np.zeros(self.sim.A, f32)

    def chain(self, node, up_to=-1):
        """node .. up_to (or the root), as walk_path collects it"""
        out, x = [], node
        while True:
            out.append(x)
            p = self.sim.meta(self.g, x).parent
            if x == up_to or p < 0:
                return out
            x = p

    def add(self, node, x):
        m = self.sim.meta(self.g, node)
        if m.parent < 0:
            self.root_S = f32(self.root_S + f32(x))
        else:
            r = self.rows[m.parent]
            r[m.fmove] = f32(r[m.fmove] + f32(x))

    def virtual_loss(self, node, up_to, sign):
        for x in self.chain(node, up_to):
            self.add(x, f32(sign))

    def incorporate(self, node, up_to, value):
        """a first expansion: value * value in every child entry, then along the path"""
        sq = f32(f32(value) * f32(value))
        self.rows[node][:] = sq
        for x in self.chain(node, up_to):
            self.add(x, sq)

    def reroot(self, a, child):
        self.root_S = f32(self.rows[self.root][a])
        self.root = child

    def live(self):
        out, todo = [], [self.root]
        while todo:
            x = todo.pop()
            out.append(x)
            todo += [int(c) for c in self.sim.children(self.g, x) if c >= 0]
        return out

    def check(self, what):
        nodes = self.live()
        for x in nodes:
            if x not in self.rows:
                self.created(x)
            got = self.sim.row_S(self.g, x)
            assert (got.view(np.uint32) == self.rows[x].view(np.uint32)).all(), (what, x)
            own = f32(self.sim.S_(self.g, x))
            m = self.sim.meta(self.g, x)
            want = self.root_S if m.parent < 0 else self.rows[m.parent][m.fmove]
            assert own.view(np.uint32) == f32(want).view(np.uint32), (what, x, "own")
        return len(nodes)


# ---------------------------------------------------------------- one select phase, predicted from the rows

class ShadowS(pt.Shadow):
    """pt.Shadow with the S row beside N, W and P: rows[node] = [N, W, P, S], a root's own = [N, W, -, S]"""

    def __init__(self, sim, g=0):
        super().__init__(sim, g)
        self.own[self.root] = self.own[self.root] + [None, f32(sim.S_(g, self.root))]

    def row(self, node):
        if node not in self.rows:
            super().row(node)
            self.rows[node].append(self.sim.row_S(self.g, node).copy())
        return self.rows[node]


def descend(sh, c_puct, setting, pv, seed, game_id, move_key, sel, counts):
    """pt.descend under the variance factor pv: one select_leaf from the root of the shadow tree -> the path; every
    level it scores is counted with the factor of the node's own (n, W, S) as this descent sees them"""
    sim, g = sh.sim, sh.g
    ps = sim.A - 1
    cur, depth, path = sh.root, 0, []
    while True:
        sh.add(cur, 0, 1.0)
        path.append(cur)
        m = sh.meta(cur)
        if not m["expanded"]:
            break
        N, W, P, _ = sh.row(cur)
        if m["last_move"] == ps and N[ps] == 0:
            pick = ps
        else:
            own = (sh.get(cur, 0), sh.get(cur, 1), sh.get(cur, 3))
            sc = scores(N, W, P, *own, m["to_play"], cur == sh.root, c_puct, setting, pv)
            lg = sim.legal(g, cur) != 0
            best = sc[lg].max()
            possible = np.flatnonzero(lg & (sc == best))
            pick = int(possible[0])
            if len(possible) > 1:
                bits = pt.sy.draw_u64(seed, game_id, move_key, pt.SITE_PUCT_TIE, sel * 1024 + depth)
                pick = int(possible[((bits >> 32) * len(possible)) >> 32])
                counts["ties"] += 1
            if pv is not None and pv[0] > 0:
                counts["levels"] += 1
                counts["raised"] += variance_factor(*own, *pv) > 1.0
        cur = sh.child(cur, pick)
        depth += 1
    return path


def leaf_board(sim, g, sh, leaf):
    """the board of a leaf of the shadow tree: a node's own, or for a child that is not made yet its parent's board with
    the move played"""
    if not isinstance(leaf, tuple):
        return sim.board(g, leaf)
    _, parent, a = leaf
    assert isinstance(parent, int)
    board = sim.board(g, parent)
    if a == sim.A - 1:
        return board
    m = sim.meta(g, parent)
    out, _, _, st = sim.go_play(board[None, :], [m.to_play], [m.ko], [a])
    assert st[0] == 0
    return out[0]


def predict_phase(sim, par, c_puct, seed, pv, g=0):
    """pt.predict_phase with the moments and the variance factor: the select phase the simulator is about to run on slot
    g (game_select_phase with no root rule) -- up to par leaves in 2 * par attempts, a virtual loss in W and S along each
    path, a finished leaf's result backed up at once in W and S.
    -> ([path [root .. leaf]] of the leaves in order, counts with levels / raised, the shadow)"""
    sh = ShadowS(sim, g)
    G = sim.game(g)
    move_key = sh.meta(sh.root)["n"]
    sel = G.sel
    counts = dict(levels=0, raised=0, ties=0, terminal=0, in_flight=0)
    leaves, failsafe = [], 0
    while len(leaves) < par and failsafe < 2 * par:
        failsafe += 1
        counts["in_flight"] += bool(leaves)
        path = descend(sh, c_puct, sim.setting, pv, seed, G.game_id, move_key, sel, counts)
        sel += 1
        leaf = path[-1]
        if sh.meta(leaf)["done"]:
            score = sim.go_score(leaf_board(sim, g, sh, leaf)[None, :], np.array([G.komi], f32))[0]
            value = f32(1.0 if score > 0 else -1.0 if score < 0 else 0.0)
            for x in path:
                sh.add(x, 1, value)
                sh.add(x, 3, f32(value * value))
            counts["terminal"] += 1
            continue
        for x in path:
            sh.add(x, 1, float(sh.meta(x)["to_play"]))
            sh.add(x, 3, 1.0)
        leaves.append(path)
    return leaves, counts, sh


def assert_phase(sim, predicted, sh, g=0):
    """pt.assert_phase, and the S of everything the prediction touched"""
    pt.assert_phase(sim, predicted, sh, g)
    for node, rows in sh.rows.items():
        assert (sim.row_S(g, node).view(np.uint32) == rows[3].view(np.uint32)).all(), (node, "S")
    assert f32(sim.S_(g, sh.root)).view(np.uint32) == f32(sh.own[sh.root][3]).view(np.uint32)
