"""Superko (agz_search_set_ko_rule) for the tests (TEST INFRASTRUCTURE): the independent statement
of the rule, which is go_shapes.ff_legal / ff_play plus a Python set of board bytes (positional) or of (board bytes,
to_play) pairs (situational) and uses no keys at all; the keys of include/agz_superko.h restated in numpy from the
header's text; and the fixtures both test files play: random legal games and hand-built cycles.  The simulator is hs.Sim,
which has the setter; gpu_options.configure sets it from a dict."""
from functools import lru_cache

import numpy as np

import alphago_jl_amd as ag
import go_shapes as gs
from alphago_jl_amd.symmetry import transform_points

OK, BAD_ARGUMENT = ag._lib.OK, ag._lib.BAD_ARGUMENT
SIMPLE, POSITIONAL, SITUATIONAL = 0, 1, 2
RULES = (POSITIONAL, SITUATIONAL)
RULE_NAMES = {SIMPLE: "simple", POSITIONAL: "positional", SITUATIONAL: "situational"}
u64 = np.uint64
# for gpu_options.configure: the options that steer the same descent and the same pick_move as the rule -- the LCB pick,
# the variance-scaled PUCT (both need the moments, which configure switches on) and the PUCT option (FPU reduction, c_base)
COMBINED = dict(lcb=(5.0, 3, 0.15), pv=(0.85, 0.4, 2.0), puct=((0.2, 0.05), 19652.0))


def soa(positions):
    """(boards int8[B][P], to_play int8[B], ko int32[B]) of a list of (board, to_play, ko, ...) tuples"""
    return (np.ascontiguousarray(np.stack([p[0] for p in positions]), np.int8),
            np.array([p[1] for p in positions], np.int8), np.array([p[2] for p in positions], np.int32))


# ---------------------------------------------------------------- the keys, restated from the text of include/agz_superko.h

WHITE_TO_PLAY = 0x8A5CD789635D2DFF


def zobrist(points, colours):
    """agz_zobrist on arrays: uint64, every operation modulo 2^64"""
    with np.errstate(over="ignore"):
        p = np.asarray(points).astype(u64)
        z = (p * u64(2) + (np.asarray(colours) < 0).astype(u64) + u64(1)) * u64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u64(32))) * u64(0xD6E8FEB86659FD93)
        z = (z ^ (z >> u64(29))) * u64(0xA0761D6478BD642F)
        return z ^ (z >> u64(32))


def np_key(board, to_play, rule):
    """the key of a position under `rule` (SIMPLE: the position key), a Python int"""
    board = np.asarray(board)
    pts = np.nonzero(board)[0]
    k = int(np.bitwise_xor.reduce(zobrist(pts, board[pts]))) if len(pts) else 0
    return k ^ (WHITE_TO_PLAY if rule == SITUATIONAL and to_play < 0 else 0)


# ---------------------------------------------------------------- the rule, stated without keys

def situation(board, to_play, rule):
    b = np.asarray(board, np.int8).tobytes()
    return b if rule == POSITIONAL else (b, int(to_play))


def sk_legal(board, N, to_play, ko, seen, rule):
    """all_legal_moves under `rule`: a move the simple rules allow is refused when the position after it is in `seen`"""
    out = gs.ff_legal(board, N, to_play, ko)
    if rule == SIMPLE:
        return out
    for a in np.nonzero(out[:-1])[0]:
        st, after, _, _ = gs.ff_play(board, N, to_play, ko, int(a))
        assert st == gs.OK
        if situation(after, -to_play, rule) in seen:
            out[a] = 0
    return out


class Line:
    """one game under a rule, played move by move: its position, the exact seen set, and every seen position once more
    as (board, to_play) for the callers that need keys"""

    def __init__(self, N, rule, board=None, to_play=1, ko=-1, history=()):
        """history: older boards, newest first; board h had (-1)^(h+1) * to_play to move"""
        self.N, self.P, self.rule = N, N * N, rule
        self.board = np.zeros(self.P, np.int8) if board is None else np.asarray(board, np.int8).copy()
        self.to_play, self.ko = to_play, ko
        self.past = [(np.asarray(b, np.int8).copy(), to_play if h & 1 else -to_play) for h, b in enumerate(history)]
        self.past.append((self.board.copy(), to_play))

    def seen(self):
        return {situation(b, tp, self.rule) for b, tp in self.past} if self.rule != SIMPLE else set()

    def seen_keys(self):
        return [np_key(b, tp, self.rule) for b, tp in self.past]

    def legal(self, rule=None):
        rule = self.rule if rule is None else rule
        seen = {situation(b, tp, rule) for b, tp in self.past} if rule != SIMPLE else set()
        return sk_legal(self.board, self.N, self.to_play, self.ko, seen, rule)

    def position(self):
        """(board, to_play, ko, seen keys under the line's rule)"""
        return self.board.copy(), self.to_play, self.ko, self.seen_keys()

    def play(self, a):
        st, board, ko, ncap = gs.ff_play(self.board, self.N, self.to_play, self.ko, int(a))
        assert st == gs.OK, (a, self.board.reshape(self.N, self.N).T)
        self.board, self.ko, self.to_play = board, ko, -self.to_play
        self.past.append((board.copy(), self.to_play))
        return ncap

    def copy(self):
        o = Line(self.N, self.rule, self.board, self.to_play, self.ko)
        o.past = list(self.past)
        return o


# ---------------------------------------------------------------- fixtures: random legal play

RANDOM_PLAY = {2: (40, 60), 3: (40, 80), 4: (30, 100)}      # N -> (games, plies at most)


@lru_cache(None)
def random_games(N, rule, seed=7, pass_prob=0.1):
    """random legal play under `rule`: a list of dicts per position -- board, to_play, ko, keys (the seen set as keys under
    the rule), legal (the twin's mask), simple (ff_legal), other (the mask under the other superko rule, same history),
    free (removed moves that capture nothing), moves (the game's moves up to here)"""
    games, plies = RANDOM_PLAY[N]
    rng = np.random.RandomState(seed)
    other = SITUATIONAL if rule == POSITIONAL else POSITIONAL
    out = []
    for _ in range(games):
        line, passes, played = Line(N, rule), 0, []
        for _ in range(plies):
            legal = line.legal()
            simple = gs.ff_legal(line.board, N, line.to_play, line.ko)
            gone = np.nonzero(simple[:-1] & ~legal[:-1].astype(bool))[0]
            free = sum(1 for a in gone if gs.ff_play(line.board, N, line.to_play, line.ko, int(a))[3] == 0)
            b, tp, ko, keys = line.position()
            out.append(dict(board=b, to_play=tp, ko=ko, keys=keys, legal=legal, simple=simple, other=line.legal(other),
                            free=free, moves=tuple(played)))
            moves = np.nonzero(legal[:-1])[0]
            a = N * N if len(moves) == 0 or rng.rand() < pass_prob else int(moves[rng.randint(len(moves))])
            passes = passes + 1 if a == N * N else 0
            line.play(a)
            played.append(a)
            if passes == 2:
                break
    return out


def census(positions):
    lost = sum(1 for p in positions if (p["legal"] != p["simple"]).any())
    removed = sum(int((p["legal"] != p["simple"]).sum()) for p in positions)
    differ = sum(1 for p in positions if (p["legal"] != p["other"]).any())
    free = sum(p["free"] for p in positions)
    return dict(positions=len(positions), lost=lost, removed=removed, differ=differ, free=free)


# ---------------------------------------------------------------- fixtures: hand-built cycles

def pt(N, row, col):
    return row + N * col


def board_of(N, black, white):
    b = np.zeros(N * N, np.int8)
    for r, c in black:
        assert b[pt(N, r, c)] == 0
        b[pt(N, r, c)] = 1
    for r, c in white:
        assert b[pt(N, r, c)] == 0
        b[pt(N, r, c)] = -1
    return b


def edge_ko(N, s, c, black_to_take):
    """An edge ko under the board symmetry T_s, on rows 0..1 and columns c..c+3 of the untransformed frame:

        row 0:   B  W  .  W          black_to_take: the White stone (0, c+1) has the single liberty (0, c+2); Black plays
        row 1:   .  B  W  .          there, captures it and stands in atari, and White retakes at (0, c+1)

    (not black_to_take: the other phase -- a Black stone on (0, c+2), (0, c+1) empty).  Returns (black cells, white cells,
    Black's point, White's point) as points p = row + N*col, or None when the shape leaves the board."""
    if c < 0 or c + 3 >= N or N < 2:
        return None
    t = transform_points(s, N)
    black = [(0, c), (1, c + 1)] + ([] if black_to_take else [(0, c + 2)])
    white = [(0, c + 3), (1, c + 2)] + ([(0, c + 1)] if black_to_take else [])
    at = lambda rc: int(t[pt(N, *rc)])
    return [at(x) for x in black], [at(x) for x in white], at((0, c + 2)), at((0, c + 1))


def triple_ko(N, places):
    """three edge kos at places = [(s, c)] * 3: kos 0 and 1 are Black's to take, ko 2 is White's to retake, Black to play.
    The cycle: B takes 0, W retakes 2, B takes 1, W retakes 0, B takes 2, W retakes 1 -- the sixth move recreates the
    start with the same side to move.  Returns (board, cycle), or None when the kos collide or the cycle does not run."""
    board = np.zeros(N * N, np.int8)
    kos = []
    for i, (s, c) in enumerate(places):
        k = edge_ko(N, s, c, i < 2)
        if k is None:
            return None
        for cells, colour in ((k[0], 1), (k[1], -1)):
            for p in cells:
                if board[p] != 0:
                    return None
                board[p] = colour
        kos.append(k)
    if any(board[k[2]] != 0 and board[k[3]] != 0 for k in kos) or not gs.valid(board, N):
        return None
    cycle = [kos[0][2], kos[2][3], kos[1][2], kos[0][3], kos[2][2], kos[1][3]]
    b, tp, ko = board, 1, -1
    for a in cycle:
        st, b, ko, ncap = gs.ff_play(b, N, tp, ko, a)
        if st != gs.OK or ncap != 1:
            return None
        tp = -tp
    return (board, cycle) if (b == board).all() else None


@lru_cache(None)
def smallest_triple_ko():
    """(N, board, cycle) of the first board size on which three edge kos fit, in a fixed search order"""
    from itertools import combinations
    for N in range(4, 10):
        places = [(s, c) for s in range(8) for c in range(N - 3)]
        for trio in combinations(places, 3):
            got = triple_ko(N, list(trio))
            if got is not None:
                return N, got[0], got[1]
    raise AssertionError("no triple ko up to 9x9")


@lru_cache(None)
def triple_ko_9():
    from itertools import combinations
    places = [(s, c) for s in range(8) for c in range(6)]
    for trio in combinations(places, 3):
        got = triple_ko(9, list(trio))
        if got is not None:
            return got
    raise AssertionError("no triple ko on 9x9")


def triple_ko_19():
    """on one edge of 19x19, the kos' two points on either side of a multiple of 32: the take and retake points are
    19 (c + 2) and 19 (c + 1), i.e. 38 | 19, 133 | 114 and 228 | 209 around 32, 128 and 224 (the mask-word edges)"""
    got = triple_ko(19, [(0, 0), (0, 5), (0, 10)])
    assert got is not None
    for k in range(3):
        a, b = sorted(got[1][i] for i in range(6) if i in ((0, 3), (2, 5), (4, 1))[k])
        assert a // 32 != b // 32, (a, b)
    return got


def send_two_return_one(N):
    """in the corner of an N x N board, N >= 5: Black (0,1) with White below it and Black stones around (0,2).  Black
    sends two at (0,0), White captures both at (0,2) and stands in atari, Black returns one at (0,1): the board of the
    start, White to move.  The positional rule refuses the third move, the situational rule does not."""
    board = board_of(N, [(0, 1), (1, 2), (0, 3)], [(1, 0), (1, 1)])
    return board, [pt(N, 0, 0), pt(N, 0, 2), pt(N, 0, 1)]


def two_group_closing(rule=POSITIONAL):
    """a position of the random games (2x2, 3x3) whose refused move takes two groups off the board at once, as the move
    list that leads to it from the empty board: (N, moves, closing move)"""
    for N in (2, 3):
        for p in random_games(N, rule):
            gone = np.nonzero(p["simple"][:-1] & ~p["legal"][:-1].astype(bool))[0]
            for a in gone:
                if gs.captured_groups(p["board"], N, p["to_play"], int(a)) >= 2:
                    return N, list(p["moves"]), int(a)
    raise AssertionError("random play reaches no refused move that captures two groups")


Fixture = __import__("collections").namedtuple("Fixture", "name N board to_play moves refused")


def _images(f, sizes_all=True):
    """the fixture in all eight images and both colourings"""
    out = []
    for s in range(8):
        t = transform_points(s, f.N)
        board = np.zeros_like(f.board)
        board[t[:-1]] = f.board
        moves = [int(t[a]) for a in f.moves]
        out.append(Fixture(f"{f.name}/s{s}", f.N, board, f.to_play, moves, f.refused))
        out.append(Fixture(f"{f.name}/s{s}/swap", f.N, (-board).astype(np.int8), -f.to_play, moves, f.refused))
    return out


@lru_cache(None)
def fixtures():
    """The hand-built lines: each a start position and the moves of its cycle, the last of which closes it.  refused:
    the rules under which the twin must refuse that last move (the twin is asked, this only guards the fixture)."""
    both = (POSITIONAL, SITUATIONAL)
    base = []
    N, board, cycle = smallest_triple_ko()
    base.append(Fixture(f"triple_ko_{N}", N, board, 1, cycle, both))
    board, cycle = triple_ko_9()
    base.append(Fixture("triple_ko_9", 9, board, 1, cycle, both))
    board, cycle = triple_ko_19()
    base.append(Fixture("triple_ko_19", 19, board, 1, cycle, both))
    for n in (5, 9):
        board, cycle = send_two_return_one(n)
        base.append(Fixture(f"send_two_return_one_{n}", n, board, 1, cycle, (POSITIONAL,)))
        # the same with two passes between the capture and the return: still an odd number of board moves
        base.append(Fixture(f"send_two_pass_pass_return_one_{n}", n, board, 1, cycle[:2] + [n * n, n * n] + cycle[2:],
                            (POSITIONAL,)))
    N, moves, closing = two_group_closing()
    base.append(Fixture(f"two_groups_{N}", N, np.zeros(N * N, np.int8), 1, moves + [closing], (POSITIONAL,)))
    return [g for f in base for g in _images(f)]


def fixture_positions(f, rule):
    """every position of fixture f played under `rule` up to its closing move: [(board, to_play, ko, seen keys, twin's
    mask)], and whether the twin refuses the closing move"""
    line = Line(f.N, rule, f.board, f.to_play)
    out = []
    for i, a in enumerate(f.moves):
        legal = line.legal()
        out.append(line.position() + (legal,))
        if i + 1 == len(f.moves):
            return out, not legal[a]
        assert legal[a], (f.name, RULE_NAMES[rule], i, a)
        line.play(a)
