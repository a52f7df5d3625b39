"""Hand-built Go positions for the rules kernels, and a flood-fill restatement of the rules to hold the oracle to.

Random legal play (tests/test_hostsim_go.py, tests/test_gpu_go.py) never reaches a group deeper than a few dozen
points, a capture of more than one wave's worth of stones, or a chosen bit of the packed legal mask.  The generators
here do, by construction.  Each returns a list of Case(name, N, board int8[P], to_play, ko, moves): the board with
p = row + N * col, the side to move, the ko point (-1: none) and the actions to try by play; every case is also a case
for the legality vector and for the score.  Numpy only: nothing here calls the oracle, the simulator or the engine
(random_boards borrows the oracle's random play from test_hostsim_go when it is called).

The restatement (ff_legal, ff_play, ff_score) is the rules by flood fill and nothing more: legality with suicide and
ko, play with captures and the ko rule "exactly one stone captured and the point played was surrounded by the
opponent", Tromp-Taylor area score.  DESIGN.md §8."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from alphago_jl_amd.symmetry import transform_points

Case = namedtuple("Case", "name N board to_play ko moves")

OK, ILLEGAL = 0, 1
SPIRAL_SIZES = (5, 8, 9, 13, 16, 19)
# stones of (the path, its complement)
SPIRAL_STONES = {5: (16, 8), 8: (38, 25), 9: (48, 32), 13: (96, 72), 16: (142, 113), 19: (198, 162)}
MASK_SIZES = (8, 15, 16, 19)
RANDOM_SIZES = (3, 4, 8, 11, 14, 16, 17)


# ---------------------------------------------------------------- the rules by flood fill

def neighbours(N, p):
    row, col = p % N, p // N
    return [r + N * c for r, c in ((row - 1, col), (row + 1, col), (row, col - 1), (row, col + 1))
            if 0 <= r < N and 0 <= c < N]


def ff_region(board, N, p):
    """the points connected to p through points of p's own value, and every other point next to them"""
    v = board[p]
    inside, border, todo = {p}, set(), [p]
    while todo:
        for q in neighbours(N, todo.pop()):
            if board[q] != v:
                border.add(q)
            elif q not in inside:
                inside.add(q)
                todo.append(q)
    return inside, border


def ff_groups(board, N):
    """(group index per point or -1, [(stones, liberties)] per group)"""
    index = np.full(N * N, -1, np.int64)
    groups = []
    for p in range(N * N):
        if board[p] != 0 and index[p] < 0:
            stones, border = ff_region(board, N, p)
            index[list(stones)] = len(groups)
            groups.append((stones, {q for q in border if board[q] == 0}))
    return index, groups


def ff_play(board, N, to_play, ko, a):
    """(status, board after, ko after, stones captured); an illegal move leaves the board and the ko as they were"""
    P = N * N
    board = np.asarray(board, np.int8)
    if a == P:
        return OK, board.copy(), -1, 0
    if a < 0 or a > P or board[a] != 0 or a == ko:
        return ILLEGAL, board.copy(), ko, 0
    after = board.copy()
    after[a] = to_play
    captured = []
    for q in neighbours(N, a):
        if after[q] == -to_play:
            stones, border = ff_region(after, N, q)
            if not any(after[e] == 0 for e in border):
                captured += sorted(stones)
                after[list(stones)] = 0
    _, border = ff_region(after, N, a)
    if not any(after[e] == 0 for e in border):
        return ILLEGAL, board.copy(), ko, 0
    surrounded = all(board[q] == -to_play for q in neighbours(N, a))
    return OK, after, captured[0] if len(captured) == 1 and surrounded else -1, len(captured)


def ff_legal(board, N, to_play, ko):
    """int8[P + 1]: an empty point other than the ko point is legal if it has an empty neighbour, joins a friendly group
    that keeps another liberty, or takes the last liberty of an enemy group; pass always is"""
    P = N * N
    index, groups = ff_groups(board, N)
    out = np.zeros(P + 1, np.int8)
    out[P] = 1
    for a in range(P):
        if board[a] != 0 or a == ko:
            continue
        for q in neighbours(N, a):
            if board[q] == 0:
                out[a] = 1
            elif board[q] == to_play:
                out[a] |= len(groups[index[q]][1]) > 1
            else:
                out[a] |= len(groups[index[q]][1]) == 1
    return out


def ff_score(board, N, komi):
    """Tromp-Taylor: stones plus the empty regions that border one colour only, Black minus White minus komi"""
    diff, seen = int((board == 1).sum()) - int((board == -1).sum()), set()
    for p in range(N * N):
        if board[p] == 0 and p not in seen:
            region, border = ff_region(board, N, p)
            seen |= region
            colours = {int(board[q]) for q in border}
            if len(colours) == 1:
                diff += len(region) * colours.pop()
    return np.float32(np.float32(diff) - np.float32(komi))


def captured_groups(board, N, to_play, a):
    """how many distinct enemy groups a stone of to_play at a takes off the board"""
    index, groups = ff_groups(board, N)
    return len({index[q] for q in neighbours(N, a) if board[q] == -to_play and groups[index[q]][1] == {a}})


def component_depths(board, N, stones):
    """the depth of every stone group (stones) or empty region (not stones): the largest BFS distance, inside the
    component, from its smallest point -- the sweeps plain min-label propagation needs"""
    out, seen = [], set()
    for p in range(N * N):
        if (board[p] != 0) != stones or p in seen:
            continue
        dist, ring = {p: 0}, [p]
        while ring:
            nxt = []
            for q in ring:
                for r in neighbours(N, q):
                    if board[r] == board[p] and r not in dist:
                        dist[r] = dist[q] + 1
                        nxt.append(r)
            ring = nxt
        seen |= set(dist)
        out.append(max(dist.values()))
    return out


def valid(board, N):
    """every point in {-1, 0, 1} and no group without a liberty"""
    return bool(np.isin(board, (-1, 0, 1)).all()) and all(libs for _, libs in ff_groups(board, N)[1])


# ---------------------------------------------------------------- images and followers of a case

def image(case, s):
    """the case under the board symmetry T_s"""
    t = transform_points(s, case.N)
    board = np.zeros_like(case.board)
    board[t[:-1]] = case.board
    ko = int(t[case.ko]) if case.ko >= 0 else -1
    return Case(f"{case.name}/s{s}", case.N, board, case.to_play, ko, [int(t[a]) for a in case.moves])


def swapped(case):
    """the case with the colours exchanged"""
    return Case(f"{case.name}/swap", case.N, (-case.board).astype(np.int8), -case.to_play, case.ko, list(case.moves))


def follow(case, a, moves, tag):
    """the case after move a (legal by the restatement), with `moves` to try"""
    st, board, ko, _ = ff_play(case.board, case.N, case.to_play, case.ko, a)
    assert st == OK, (case.name, a)
    return Case(f"{case.name}/{tag}", case.N, board, -case.to_play, ko, list(moves))


def dedupe(moves):
    return list(dict.fromkeys(int(a) for a in moves))


# ---------------------------------------------------------------- 1. spirals

@lru_cache(None)
def spiral_cells(N):
    """(row, col) of the pitch-2 spiral from the corner: walk on, turning right whenever the next cell is off the board,
    visited, or next to an earlier part of the path"""
    path, step = [(0, 0)], (0, 1)
    on_path = {(0, 0)}

    def blocked(cell):
        r, c = cell
        if not (0 <= r < N and 0 <= c < N) or cell in on_path:
            return True
        return any(n in on_path and n != path[-1] for n in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)))

    while True:
        nxt = (path[-1][0] + step[0], path[-1][1] + step[1])
        if blocked(nxt):
            step = (step[1], -step[0])
            nxt = (path[-1][0] + step[0], path[-1][1] + step[1])
            if blocked(nxt):
                return path
        path.append(nxt)
        on_path.add(nxt)


@lru_cache(None)
def spiral_arms(N):
    """(path points without the inner end, complement points, inner end), both arms from the outer end inwards"""
    pts = [r + N * c for r, c in spiral_cells(N)]
    inner, path = pts[-1], pts[:-1]
    rest = set(range(N * N)) - set(pts)
    dist, ring = {inner: 0}, [inner]
    while ring:
        nxt = []
        for q in ring:
            for r in neighbours(N, q):
                if r in rest and r not in dist:
                    dist[r] = dist[q] + 1
                    nxt.append(r)
        ring = nxt
    assert set(dist) == rest | {inner}, "the complement of the spiral is one group that touches the inner end"
    comp = sorted(rest, key=lambda p: (-dist[p], p))
    assert (len(path), len(comp)) == SPIRAL_STONES[N], (N, len(path), len(comp))
    return tuple(path), tuple(comp), inner


def spiral_board(N, path_colour):
    path, comp, inner = spiral_arms(N)
    board = np.zeros(N * N, np.int8)
    board[list(path)] = path_colour
    board[list(comp)] = -path_colour
    return board, inner


def spirals(sizes=SPIRAL_SIZES, images=range(8)):
    """both colourings and both sides to move, in every image: each group's one liberty is the inner end, and the move
    there is legal only because it captures the other arm"""
    out = []
    for N in sizes:
        path, comp, inner = spiral_arms(N)
        for colour in (-1, 1):
            board, _ = spiral_board(N, colour)
            for tp in (1, -1):
                base = Case(f"spiral/N{N}/path{'W' if colour < 0 else 'B'}/tp{tp:+d}", N, board, tp, -1,
                            [inner, N * N, path[0], comp[0]])
                out += [image(base, s) for s in images]
    return out


def spiral_scores(sizes=SPIRAL_SIZES, images=range(8)):
    """the boards after the capture of either arm: the emptied arm as it is, and with one stone of the captured colour
    at its outer end, its middle and its inner end (the region neutral, or split in two)"""
    out = []
    for N in sizes:
        path, comp, inner = spiral_arms(N)
        for colour in (-1, 1):
            board, _ = spiral_board(N, colour)
            for arm, taken in (("path", path), ("comp", comp)):
                tc = colour if arm == "path" else -colour            # the colour of the captured arm
                st, after, ko, ncap = ff_play(board, N, -tc, -1, inner)
                assert st == OK and ncap == len(taken) and ko == -1
                spots = {"open": None, "outer": taken[0], "middle": taken[len(taken) // 2], "inner": taken[-1]}
                for tag, spot in spots.items():
                    b = after.copy()
                    if spot is not None:
                        b[spot] = tc
                    base = Case(f"spiral-score/N{N}/path{'W' if colour < 0 else 'B'}/{arm}/{tag}", N, b, tc, -1,
                                [taken[1], taken[len(taken) // 2 + 1], taken[-2], N * N])
                    out += [image(base, s) for s in images]
    return out


# ---------------------------------------------------------------- 2. ko and capture counts

class _Clash(Exception):
    pass


class _Shape:
    """stones by (row, col) around an anchor; X = +1 moves first, O = -1"""

    def __init__(self, N, where):
        m = N // 2
        self.N, self.where = N, where
        self.a = {"corner": (0, 0), "edge": (0, m), "centre": (m, m)}[where]
        self.stones = {}

    def on(self, rc):
        return 0 <= rc[0] < self.N and 0 <= rc[1] < self.N

    def orth(self, rc=None):
        """the neighbours of rc (the anchor), clockwise from the north, as one run of the circle"""
        r, c = rc or self.a
        ring = [(r - 1, c), (r, c + 1), (r + 1, c), (r, c - 1)]
        keep = [self.on(x) for x in ring]
        k = next((i for i in range(4) if keep[i] and not keep[i - 1]), 0)
        return [ring[(k + i) % 4] for i in range(4) if keep[(k + i) % 4]]

    def ring8(self, cells):
        """the points a king's move from one of `cells`, without them"""
        out = {(r + dr, c + dc) for r, c in cells for dr in (-1, 0, 1) for dc in (-1, 0, 1)}
        return {x for x in out if self.on(x)} - set(cells)

    def put(self, cells, colour):
        for rc in cells:
            if not self.on(rc):
                continue
            if self.stones.get(rc, colour) != colour:
                raise _Clash(rc)
            self.stones[rc] = colour

    def around(self, cells, colour, keep_free):
        """a stone of `colour` on every neighbour of `cells` outside them and outside keep_free"""
        self.put([n for rc in cells for n in self.orth(rc) if n not in cells and n not in keep_free], colour)

    def pt(self, rc):
        return rc[0] + self.N * rc[1]

    def board(self):
        b = np.zeros(self.N * self.N, np.int8)
        for rc, v in self.stones.items():
            b[self.pt(rc)] = v
        return b


def _capture(N, where, ncap, friendly=False, long=False):
    """X at the anchor takes ncap of its neighbours, each a group of its own whose last liberty the anchor is; the
    other neighbours are O (the anchor surrounded), or the first of them X (friendly).  long: the first group has a
    second stone behind it.  ncap = 1, not friendly, not long: a ko."""
    s = _Shape(N, where)
    orth = s.orth()
    if ncap > len(orth) or (friendly and ncap == len(orth)):
        return None
    groups = [[q] for q in orth[:ncap]]
    if long:
        q = groups[0][0]
        groups[0].append((2 * q[0] - s.a[0], 2 * q[1] - s.a[1]))
        if not s.on(groups[0][1]):
            return None
    for g in groups:
        s.put(g, -1)
    for k, r in enumerate(orth[ncap:]):
        s.put([r], 1 if friendly and k == 0 else -1)
    for g in groups:
        s.around(g, 1, {s.a})
    return s, [s.a] + orth


def _surrounded(N, where):
    """every neighbour of the anchor O and alive: single-stone suicide for X"""
    s = _Shape(N, where)
    s.put(s.orth(), -1)
    return s, [s.a] + s.orth()


def _ring(N, where, fill, wall):
    """an O ring around the anchor a and the point b next to it.  wall: X all around the ring, so a and b are its only
    liberties.  fill: an X stone on b, whose one liberty is a.
      wall, no fill: a snapback -- X throws in at a, O takes one stone at b (no ko: b joins the ring), X takes the lot
      fill, no wall: X at a is a two-stone suicide;  fill and wall: the same point, legal, because it takes the ring"""
    s = _Shape(N, where)
    b = (s.a[0], s.a[1] + 1)
    ring = s.ring8([s.a, b])
    s.put(ring, -1)
    if wall:
        s.around(ring, 1, {s.a, b})
    if fill:
        s.put([b], 1)
    return s, [s.a, b]


def _touch(N, where, sides):
    """one O group, its only liberty the anchor, next to the anchor on `sides` sides: captured once, not per side"""
    s = _Shape(N, where)
    orth = s.orth()
    if sides > len(orth):
        return None
    ring = s.ring8([s.a]) - set(orth[sides:])
    group, todo = {orth[0]}, [orth[0]]
    while todo:
        for n in s.orth(todo.pop()):
            if n in ring and n not in group:
                group.add(n)
                todo.append(n)
    if not set(orth[:sides]) <= group:
        return None
    s.put(group, -1)
    s.put(s.ring8([s.a]) - group, 1)
    s.around(group, 1, {s.a})
    return s, [s.a]


def _liberties(N, where, free):
    """one O stone on the anchor with exactly `free` liberties (the first `free` neighbours), X on the others"""
    s = _Shape(N, where)
    orth = s.orth()
    if free > len(orth):
        return None
    s.put([s.a], -1)
    s.put(orth[free:], 1)
    return s, orth


def _patterns(N, where):
    """(name, board, moves, line): line = the moves X and O play on from there, each position on the way a case"""
    made = []

    def add(name, build, *args, line=(), **kw):
        try:
            got = build(N, where, *args, **kw)
        except _Clash:
            return
        if got is None:
            return
        s, moves = got
        board = s.board()
        if valid(board, N):
            made.append((name, board, dedupe([s.pt(rc) for rc in moves] + [N * N]), [s.pt(rc) for rc in line]))

    s0 = _Shape(N, where)
    a, orth = s0.a, s0.orth()
    add("ko", _capture, 1, line=[a])                                # (the retake is the first neighbour, a tried move)
    add("one-friendly", _capture, 1, friendly=True, line=[a])
    add("one-long", _capture, 1, long=True, line=[a])              # two stones captured by a surrounded move: no ko
    for n in (2, 3, 4):
        add(f"groups{n}", _capture, n, line=[a])
        add(f"groups{n}-long", _capture, n, long=True, line=[a])
        add(f"groups{n}-friendly", _capture, n, friendly=True, line=[a])
    add("suicide1", _surrounded)
    b = (a[0], a[1] + 1)
    add("snapback", _ring, fill=False, wall=True, line=[a, b, a])
    add("suicide2", _ring, fill=True, wall=False)
    add("suicide2-capture", _ring, fill=True, wall=True, line=[a])
    for n in (2, 3, 4):
        add(f"touch{n}", _touch, n, line=[a])
    for n in (1, 2, 3, 4):
        add(f"libs{n}", _liberties, n)
    return made


def _whole_board(N):
    """one X group with exactly one, two and three liberties; the two are points 0 and P - 1, the ends of the
    smallest / largest liberty summary"""
    P = N * N
    made = []
    for name, holes in (("full1", [0]), ("full2", [0, P - 1]), ("full3", [0, P // 2, P - 1]), ("full1-last", [P - 1])):
        board = np.ones(P, np.int8)
        board[holes] = 0
        made.append((name, board, dedupe(holes + [1, P - 2, P]), []))
    return made


def ko_and_captures(sizes=(5, 9), images=range(8)):
    out = []
    for N in sizes:
        pats = [(f"{w}/{n}", b, m, l) for w in ("corner", "edge", "centre") for n, b, m, l in _patterns(N, w)]
        pats += [(f"board/{n}", b, m, l) for n, b, m, l in _whole_board(N)]
        for name, board, moves, line in pats:
            for s in images:
                for swap in (False, True):
                    for tp in (1, -1):
                        c = image(Case(f"shape/N{N}/{name}/tp{tp:+d}", N, board, tp, -1, moves), s)
                        t = transform_points(s, N)
                        c = swapped(c) if swap else c
                        out.append(c)
                        if tp != 1:
                            continue
                        for k, a in enumerate(line):        # the line of play; each ko on it once more without the ko
                            nxt = line[k + 1:k + 2] or [a]
                            c = follow(c, int(t[a]), dedupe([int(t[x]) for x in nxt] + list(c.moves)), f"m{k}")
                            out.append(c)
                            if c.ko >= 0:
                                out.append(c._replace(name=c.name + "-noko", ko=-1))
    return out


# ---------------------------------------------------------------- 3. mask and stride edges

def edge_actions(N):
    """both sides of every multiple of 32 (and so of 64) below P, plus 0 and P - 1"""
    P = N * N
    return sorted({0, P - 1} | {m + d for m in range(32, P, 32) for d in (-1, 0)})


def _eye_board(N, eyes):
    board = np.ones(N * N, np.int8)
    board[list(eyes)] = 0
    return board


def _eyes_fit(N, eyes):
    """single-point eyes in one connected group"""
    board = _eye_board(N, eyes)
    if any(board[q] == 0 for e in eyes for q in neighbours(N, e)):
        return False
    return len(ff_groups(board, N)[1]) == 1


def mask_edges(sizes=MASK_SIZES):
    """one Black group over the whole board but for single-point eyes at chosen actions: with Black to move every eye
    is legal, with White to move none is, and pass always is.  `first` takes the edge actions that fit together,
    `second` those left over (neighbours of the first), `lattice` every second point of every second line that is no eye
    of the first.  And the same with the colours exchanged."""
    out = []
    for N in sizes:
        P = N * N
        want = edge_actions(N)
        first, second = [], []
        for e in want:
            if _eyes_fit(N, first + [e]):
                first.append(e)
            elif _eyes_fit(N, second + [e]):
                second.append(e)
        assert sorted(first + second) == want, (N, want, first, second)
        lattice = []
        for p in range(P):
            near = {p + dr + N * dc for dr in (-1, 0, 1) for dc in (-1, 0, 1)
                    if 0 <= p % N + dr < N and 0 <= p // N + dc < N}
            if p not in first and not near & set(lattice) and _eyes_fit(N, lattice + [p]):
                lattice.append(p)
        for tag, eyes in (("first", first), ("second", second), ("lattice", lattice)):
            if not eyes:
                continue
            board = _eye_board(N, eyes)
            moves = dedupe(list(eyes) + want + [P])
            for tp in (1, -1):
                c = Case(f"mask/N{N}/{tag}/tp{tp:+d}", N, board, tp, -1, moves)
                out += [c, swapped(c)]
    return out


# ---------------------------------------------------------------- 4. small and odd boards

def tiny_tree(N=2, depth=7):
    """every position of the game tree of the N x N board to `depth` plies, each once, with every action to try"""
    P = N * N
    start = (bytes(P), 1, -1, False)
    seen, ring, out = {start[:3]}, [start], []
    for d in range(depth + 1):
        nxt = []
        for raw, tp, ko, passed in ring:
            board = np.frombuffer(raw, np.int8).copy()
            out.append(Case(f"tiny/N{N}/d{d}/{len(out)}", N, board, tp, ko, list(range(P + 1))))
            for a in range(P + 1):
                st, b, k, _ = ff_play(board, N, tp, ko, a)
                if st != OK or (a == P and passed):
                    continue
                key = (b.tobytes(), -tp, k)
                if key not in seen:
                    seen.add(key)
                    nxt.append(key + (a == P,))
        ring = nxt
    return out


def random_boards(sizes=RANDOM_SIZES, games=3, seed=7):
    """positions of uniformly random legal play on the sizes no other test uses, four drawn actions and pass to try"""
    from test_hostsim_go import random_positions
    out = []
    rng = np.random.RandomState(seed)
    for N in sizes:
        P = N * N
        for k, pos in enumerate(random_positions(N, games if N < 14 else 2, min(3 * P // 2, 220), seed=seed + N)):
            moves = dedupe(list(rng.randint(0, P, size=4)) + [P])
            out.append(Case(f"random/N{N}/{k}", N, pos.board_np(), int(pos.to_play), int(pos.ko), moves))
    return out


# ---------------------------------------------------------------- 5. a scripted game into the spiral

def scripted_game(N):
    """(moves, ply of the capture): Black plays the complement from its outer end, White the spiral path from its outer
    end, the side that has run out passes; then Black takes the path at the inner end, and twelve more moves go into the
    emptied path three points apart, one of them a pass"""
    path, comp, inner = spiral_arms(N)
    P = N * N
    moves = []
    for k in range(len(path)):
        moves += [comp[k] if k < len(comp) else P, path[k]]
    capture = len(moves)
    moves.append(inner)
    moves += [P if k == 5 else path[3 * k] for k in range(12)]
    return moves, capture


FAMILIES = {"spirals": spirals, "spiral_scores": spiral_scores, "ko_and_captures": ko_and_captures,
            "mask_edges": mask_edges, "tiny_tree": tiny_tree, "random_boards": random_boards}


@lru_cache(None)
def family(name):
    return tuple(FAMILIES[name]())


def all_cases():
    return [c for name in FAMILIES for c in family(name)]
