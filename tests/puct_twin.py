"""The PUCT rule options (agz_search_set_puct) restated in Python (TEST INFRASTRUCTURE).

puct_scores is the rule of include/agz.h in numpy: float32 exactly where the definition says Float32, Python floats
(float64) elsewhere, agz_log and agz_sqrt of include/agz_draws.h restated operation for operation (both use only + * /
and the exponent bits).  predict_phase walks a tree's rows from the root as one select phase does (mcts.jl:108-138 with
the pass-first rule and the tie draw of select_leaf, virtual losses between the descents) and says which leaves it must
return.  The oracle's select_leaf is the reference's rule and cannot stand in here.

Also here: the host simulator with the setter -- tests/hostsim/hostsim_puct.cpp, built to a library of its own with the
flags of the Makefile next to it and bound like hs.lib() -- and the peaked deterministic network the tests search with."""
import ctypes as C
import os
import re
import shlex
import struct
import subprocess
import zlib

import numpy as np

import hs
from alphago_jl_amd import symmetry as sy

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
f32, f64 = np.float32, np.float64
OFF = (0, 0.0, 0.0, 0.0)
TWO30 = 1073741824.0


def _site(name):
    hdr = open(os.path.join(ROOT, "include", "agz_draws.h")).read()
    return int(re.search(r"#define AGZ_SITE_%s (\d+)u" % name, hdr).group(1))


SITE_PUCT_TIE = _site("PUCT_TIE")


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


def bits64(x):
    return np.ascontiguousarray(x, f64).view(np.uint64)


# ---------------------------------------------------------------- the simulator with the setter

_lib = None


def _sources():
    c = os.path.join(ROOT, "alphago.jl_amd", "csrc")
    return [os.path.join(HERE, "hostsim", "hostsim_puct.cpp"), os.path.join(HERE, "hostsim", "hostsim.cpp"),
            os.path.join(c, "agz_search.h"), os.path.join(c, "agz_state.h"), os.path.join(c, "agz_layout.h"),
            os.path.join(ROOT, "include", "agz_draws.h"), os.path.join(ROOT, "include", "agz.h")]


def lib():
    """tests/hostsim/libhostsim_puct.so: hostsim.cpp + hs_set_puct / hs_puct_counts, with hs.lib()'s prototypes"""
    global _lib
    if _lib is not None:
        return _lib
    base = hs.lib()
    d = os.path.join(HERE, "hostsim")
    out = os.path.join(d, "libhostsim_puct.so")
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in _sources()):
        mk = open(os.path.join(d, "Makefile")).read()
        cmd = shlex.split(re.search(r"^\t(g\+\+ .*)$", mk, flags=re.M).group(1))
        cmd = [os.path.join(d, "hostsim_puct.cpp") if t == "$<" else out + ".tmp" if t == "$@" else t for t in cmd]
        subprocess.run(cmd + ["-Wno-unknown-pragmas"], check=True)
        os.replace(out + ".tmp", out)
    L = C.CDLL(out)
    for name, fn in list(vars(base).items()):
        if name.startswith("hs_") and hasattr(fn, "argtypes"):
            g = getattr(L, name)
            g.restype, g.argtypes = fn.restype, fn.argtypes
    vp, i, dbl = C.c_void_p, C.c_int, C.c_double
    P = C.POINTER
    for name, (res, args) in {"hs_set_puct": (None, [vp, i, dbl, dbl, dbl]),
                              "hs_puct_counts": (None, [vp, P(C.c_ulonglong)]),
                              "hs_leaf_paths": (i, [vp, i, P(C.c_int32), P(C.c_int32), P(C.c_int32)]),
                              "hs_set_symmetry": (None, [vp, i]), "hs_leaf_syms": (None, [vp, P(C.c_int32)])}.items():
        g = getattr(L, name)
        g.restype, g.argtypes = res, args
    _lib = L
    return L


class Sim(hs.Sim):
    """hs.Sim on the library with the setter"""

    def __init__(self, **cfg):
        self.L = lib()
        self.cfg = hs.default_config(**cfg)
        self.h = self.L.hs_create(C.byref(self.cfg))
        d = (C.c_int32 * 10)()
        self.L.hs_dims(self.h, d)
        (self.N, self.P, self.A, self.AP, self.cap, self.games, self.par, self.mgl, self.tau, self.maxd) = list(d)
        self.setting = OFF

    def set_puct(self, fpu_on=0, r=0.0, r_root=0.0, c_base=0.0):
        self.L.hs_set_puct(self.h, int(fpu_on), float(r), float(r_root), float(c_base))
        self.setting = (int(fpu_on), float(r), float(r_root), float(c_base))

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
            self.L.hs_leaf_syms(self.h, hs.p32(s))
            x = np.stack([sy.apply_features(feats[k], int(s[k]), self.N) for k in range(B)]).astype(f32)
            pi, v = forward(x)
            pi = np.stack([sy.apply_policy(pi[k], sy.inverse(int(s[k])), self.N) for k in range(B)]).astype(f32)
            return pi, v
        return self.step(net)

    def scores(self, node, g=0):
        out = np.zeros(self.A, f64)
        st, _ = self.op(hs.TOP_SCORES, g=g, node=node, dout=out)
        assert st == 0
        return out

    def leaf_paths(self, g=0):
        """the leaves of the last select phase of slot g: [(leaf, [root .. leaf])]"""
        nodes = np.zeros(self.par, np.int32)
        plen = np.zeros(self.par, np.int32)
        paths = np.zeros((self.par, self.maxd), np.int32)
        n = self.L.hs_leaf_paths(self.h, g, hs.p32(nodes), hs.p32(plen), hs.p32(paths))
        return [(int(nodes[k]), [int(x) for x in paths[k, :plen[k]]]) for k in range(n)]


# ---------------------------------------------------------------- a peaked deterministic network

class PeakedNet:
    """pi and v from a hash of the features: one board point holds `peak` of the mass, the rest is spread over all
    actions in four levels (equal priors: unvisited children tie under the FPU, so the tie draw is exercised); v is
    spread over +-0.9"""

    def __init__(self, N, peak=0.6, salt=0):
        self.N, self.A, self.peak, self.salt = N, N * N + 1, peak, salt
        self.calls = 0

    def __call__(self, feats):
        feats = np.ascontiguousarray(feats, f32)
        B = feats.shape[0]
        pi = np.zeros((B, self.A), f32)
        v = np.zeros(B, f32)
        for b in range(B):
            h = zlib.crc32(feats[b].tobytes(), self.salt)
            rng = np.random.RandomState(h)
            rest = np.floor(rng.rand(self.A) * 4.0) / 4.0 + 0.05
            rest[-1] *= 0.25                            # a pass is rarely the network's idea
            row = (1.0 - self.peak) * rest / rest.sum()
            row[h % (self.A - 1)] += self.peak
            pi[b] = row.astype(f32)
            v[b] = f32(((h >> 8) % 1801) / 1000.0 - 0.9)
        self.calls += B
        return pi, v


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
