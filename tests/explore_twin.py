"""Root exploration and the move temperature (agz_selfplay_set_root_policy_temperature, agz_selfplay_set_root_noise,
agz_search_set_move_temperature) restated in Python (TEST INFRASTRUCTURE).

The rules of include/agz.h in numpy: Python floats where the definition says Float64, np.float32 where it says Float32,
every sum a loop in ascending action order, the elementary functions and the draws through the oracle's exported
or_det_log, or_det_exp, or_dirichlet_gamma, or_draw_u64 and or_draw_u01.  twin_selfplay_explore is the loop of
selfplay_twin.twin_selfplay with two steps replaced by the restatement: the noise of a full search, written into the
oracle root's prior row in place, and the pick of the move.

Also here: a callback that lets a network of feature rows (such as hs.PeakedNet) answer the oracle's positions, a run of
the host simulator (hs.Sim: apply, explore_counts, explore_rows, set_pick_case) under a setting, and the settings, game
sets, rows and positions that the CPU tests (tests/test_explore.py) and the device tests (tests/test_gpu_explore.py) share."""
import ctypes as C

import numpy as np

import hs
import orc
import selfplay_twin as tw
from hs import bits32, bits64

L = tw.L
L.or_dirichlet_gamma.restype = C.c_double
L.or_dirichlet_gamma.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_double]
f32, f64 = np.float32, np.float64
LN2 = 0.6931471805599453
ARGMAX_T = 0.01
SITE_PICK_TIE, SITE_SOFTPICK = tw._site("PICK_TIE"), tw._site("SOFTPICK")
OFF = dict(pt=None, noise=(0.0, False), mt=None)
KATAGO = dict(pt=(1.25, 1.1, None), noise=(10.83, True), mt=(0.75, 0.15, None))     # None: the board size


def setting(pt=None, noise=(0.0, False), mt=None):
    return dict(pt=pt, noise=noise, mt=mt)


# ---------------------------------------------------------------- the rules

def temperature(n, early, late, halflife):
    """agz_temperature: late + ((early - late) * agz_exp(-((n * ln 2) / halflife)))"""
    return late + ((early - late) * L.or_det_exp(-((float(n) * LN2) / halflife)))


def legacy_alpha(A):
    """View::alpha, mcts.jl:22 with go.jl:24: one Float32 constant for all A actions"""
    return float(f32(0.03 * 361.0 / float(A)))


def temper_row(P, legal, T):
    """rule 1 -> (row float32[A], whether a legal positive entry existed)"""
    P = np.array(P, f32)
    on = [a for a in range(len(P)) if legal[a] and P[a] > 0]
    if not on:
        return P, False
    x = {a: L.or_det_log(float(P[a])) / T for a in on}
    M = max(x.values())
    e = {a: L.or_det_exp(x[a] - M) for a in on}
    E = mass = 0.0
    for a in on:
        E += e[a]
    for a in on:
        mass += float(P[a])
    for a in on:
        P[a] = f32((e[a] / E) * mass)
    return P, True


def noise_alpha(P, legal, total_alpha, shaped):
    """alpha_a of rule 2: float64[A], 0 for an illegal action"""
    A = len(P)
    on = [a for a in range(A) if legal[a]]
    u = 1.0 / float(len(on))
    alpha = np.zeros(A, f64)
    S, s = 0.0, {}
    if shaped:
        l = {a: L.or_det_log(min(0.01, float(P[a])) + 1e-20) for a in on}
        tot = 0.0
        for a in on:
            tot += l[a]
        mean = tot / float(len(on))
        s = {a: max(0.0, l[a] - mean) for a in on}
        for a in on:
            S += s[a]
    for a in on:
        alpha[a] = total_alpha * u if (not shaped or S <= 0.0) else total_alpha * (0.5 * ((s[a] / S) + u))
    return alpha


def noise_row(P, legal, alpha, seed, game, n, w):
    """the mix of rule 2 under the concentrations alpha: float32[A]"""
    P = np.array(P, f32)
    on = [a for a in range(len(P)) if legal[a]]
    u = 1.0 / float(len(on))
    g = {a: L.or_dirichlet_gamma(seed, game, n, a, float(alpha[a])) for a in on}
    G = 0.0
    for a in on:
        G += g[a]
    for a in on:
        d = g[a] / G if G > 0.0 else u
        P[a] = f32((float(P[a]) * (1.0 - w)) + (d * w))
    return P


def legacy_noise_row(P, seed, game, n, w):
    """inject_noise! as the engine runs it with rule 2 off: one alpha, all A actions (mcts.jl:233-239)"""
    P = np.array(P, f32)
    A = len(P)
    al = legacy_alpha(A)
    g = [L.or_dirichlet_gamma(seed, game, n, a, al) for a in range(A)]
    G = 0.0
    for x in g:
        G += x
    for a in range(A):
        d = g[a] / G if G > 0.0 else 1.0 / float(A)
        P[a] = f32(float(P[a]) * (1.0 - w) + d * w)
    return P


def schedule_of(t, N):
    """(early, late, halflife) with halflife None = the board size"""
    early, late, half = t
    return float(early), float(late), float(N if half is None else half)


def explore_rows(P, legal, n, seed, game, w, st, N):
    """what root_explore does to a root's prior row under setting st -> (tempered, alpha, noised, was tempered)"""
    P = np.array(P, f32)
    did = False
    if st["pt"] is not None:
        P, did = temper_row(P, legal, temperature(n, *schedule_of(st["pt"], N)))
    tempered = P.copy()
    total, shaped = st["noise"]
    if total > 0:
        alpha = noise_alpha(P, legal, float(total), bool(shaped))
        noised = noise_row(P, legal, alpha, seed, game, n, w)
    else:
        alpha = np.full(len(P), legacy_alpha(len(P)), f64)
        noised = legacy_noise_row(P, seed, game, n, w)
    return tempered, alpha, noised, did


def argmax_pick(Nrow, n, seed, game):
    """the arg-max branch of pick_move (mcts_play.jl:58-62): the most visited child, the tie draw among several"""
    Nrow = np.asarray(Nrow, f32)
    idx = np.flatnonzero(Nrow == Nrow.max())
    if len(idx) > 1:
        return int(idx[tw._index(L.or_draw_u64(seed, game, n, SITE_PICK_TIE, 0), len(idx))])
    return int(idx[0])


def pick_move(Nrow, n, seed, game, mt, N):
    """rule 3 -> (ok, action, sampled, off_max); ok False = AGZ_ASSERT_SOFTPICK"""
    Nrow = np.asarray(Nrow, f32)
    T = temperature(n, *schedule_of(mt, N))
    if T <= ARGMAX_T:
        return True, argmax_pick(Nrow, n, seed, game), False, False
    mx = Nrow.max()
    if not mx > 0:
        return False, -1, False, False
    wts = [L.or_det_exp(L.or_det_log(float(c) / float(mx)) / T) if c > 0 else 0.0 for c in Nrow]
    S = 0.0
    for x in wts:
        S += x
    r = L.or_draw_u01(L.or_draw_u64(seed, game, n, SITE_SOFTPICK, 0)) * S
    acc, pick, last = 0.0, None, None
    for a, x in enumerate(wts):
        acc += x
        if x > 0:
            last = a
            if acc > r:
                pick = a
                break
    if pick is None:
        pick = last
    return True, int(pick), True, bool(Nrow[pick] != mx)


# ---------------------------------------------------------------- a feature-row network in front of the oracle

class FeatsNet:
    """net(feats [B, 17 * P] float32) -> (pi, v), such as hs.PeakedNet, as the oracle's network callback: the
    positions go through or_get_feats, so the simulator (hs_leaf_features) and the oracle ask the same rows"""

    def __init__(self, net, N):
        self.net, self.A = net, N * N + 1

        def _fn(ctx, positions, B, pi, v):
            feats = np.stack([orc.feats(positions[b].contents).reshape(-1) for b in range(B)]).astype(f32)
            p, val = self.net(feats)
            np.ctypeslib.as_array(pi, shape=(B * self.A,))[:] = np.ascontiguousarray(p, f32).reshape(-1)
            np.ctypeslib.as_array(v, shape=(B,))[:] = np.ascontiguousarray(val, f32)

        self.cb = orc.NET_FN(_fn)

    def on_feats(self, feats):
        return self.net(feats)


# ---------------------------------------------------------------- selfplay.jl:1-45 with the rules

def twin_selfplay_explore(N, net_cb, R, seed, game, st, start=None, threshold=-0.9, disable=0.05, on_round=None,
                          cap=None, forced=None, noise_w=0.25):
    """selfplay_twin.twin_selfplay (no Gumbel search) under the setting st: the noise of a full search is explore_rows
    written into the oracle root's prior row, the move is pick_move when the move temperature is on.  cap, forced and
    start as in the original.  The record also has tempered / noised (roots), sampled / off_max (moves of the sampling
    branch), argmax_plies (moves of the T <= 0.01 branch) and illegal_roots (noised roots with an illegal point)."""
    r, p = cap if cap else (0, 1.0)
    k, prune = forced if forced else (0.0, False)
    A = N * N + 1
    u = L.or_draw_u01(L.or_draw_u64(seed, game, 0, tw.SITE_RESIGN, 0))
    disabled = u < disable
    pl = L.or_player_new(N, net_cb, None, R, 0, -1.0 if disabled else threshold, seed, game)
    L.or_player_initialize_game(pl, C.byref(start) if start is not None else None)
    env = L.or_player_env(pl)
    tau = L.or_player_tau_threshold(pl)
    start_n = tw._root_pos(pl).n
    draw = tw._new_draw(seed, game, pl)
    evals = 1
    if on_round:
        on_round()
    first = L.or_select_leaf(env, L.or_player_root(pl), C.byref(draw))
    pi, v = tw._net_call(net_cb, [first], A)
    L.or_incorporate_results(env, first, orc.fptr(pi[0]), A, float(v[0]), first)
    positions, moves, full, searched, rows, changed = [], [], [], [], [], []
    info = dict(forced_sel=0, tempered=0, noised=0, sampled=0, off_max=0, argmax_plies=0, illegal_roots=0)
    was_resign = 0
    while True:
        root = L.or_player_root(pl)
        rp = tw._root_pos(pl)
        is_full = r <= 0 or bool(tw.coin_full(seed, game, rp.n, p))
        searched.append(is_full)
        rule = tw._forced_rule(env, draw, k if is_full else 0.0, info) if forced else None
        if is_full:
            Pr = orc.node_arr(L.or_node_child_prior(root), A)
            legal = tw._legal(root, A)
            _, _, noised, did = explore_rows(Pr, legal, rp.n, seed, game, noise_w, st, N)
            Pr[:] = noised
            info["tempered"] += did
            info["noised"] += st["noise"][0] > 0
            info["illegal_roots"] += bool((legal[:A - 1] == 0).any())
        evals += tw._readouts(env, pl, draw, net_cb, A, R if is_full else r, on_round, rule)
        if L.or_player_should_resign(pl):
            L.or_player_set_result(pl, -tw._root_pos(pl).to_play, 1)
            was_resign = 1
            break
        rp = tw._root_pos(pl)
        Nr, Wr, Pr = tw._rows(root, A)
        if st["mt"] is not None:
            ok, a, sampled, off = pick_move(Nr, rp.n, seed, game, st["mt"], N)
            info["sampled"] += sampled
            info["off_max"] += off
            info["argmax_plies"] += ok and not sampled
            if not ok:
                a = A - 1
        else:
            a = C.c_int(-1)
            if L.or_player_pick_move(pl, C.byref(a)) != orc.OK:
                a = C.c_int(A - 1)
            a = a.value
        row, ch = None, False
        if is_full and prune and k > 0:
            row, ch = tw.pruned_pi(Nr, Wr, Pr, rp.to_play, L.or_node_N(root), env.contents.c_puct, k, rp.n <= tau)
        positions.append(rp.copy())
        rows.append(row)
        changed.append(ch)
        assert L.or_player_play_move(pl, a) == 1
        moves.append(a)
        full.append(is_full)
        draw = tw._new_draw(seed, game, pl)
        if L.or_node_is_done(env, L.or_player_root(pl)):
            L.or_player_set_result(pl, L.or_result(L.or_node_pos(L.or_player_root(pl))), 0)
            break
    n = L.or_player_num_moves(pl)
    assert n == len(moves) == tw._root_pos(pl).n - start_n
    fin = tw._root_pos(pl).copy()
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
               start_n=start_n, pruned_rows=np.array(changed, bool), **info)
    L.or_player_free(pl)
    return rec


def tallies(twins):
    """the four counters of agz_search_explore_counts over a set of twin games"""
    return tuple(int(sum(o[k] for o in twins)) for k in ("tempered", "noised", "sampled", "off_max"))


# ---------------------------------------------------------------- the simulator under a setting

def run_sim(N, net, R, seed, games, slots, st, cap=None, forced=None, starts=None, max_steps=400000, **cfg):
    """self-play of `games` games on the simulator under setting st (None: no setter is called) -> (records, counters,
    the four explore counters)"""
    sim = hs.Sim(board_size=N, games=slots, num_readouts=R, seed=seed, game_id_base=0, game_id_stride=1,
              record_capacity_games=games + 8, **cfg)
    if starts:
        sim.set_starts(starts)
    if cap:
        sim.set_playout_cap(*cap)
    if forced:
        sim.set_forced_playouts(*forced)
    if st is not None:
        sim.apply(st)
    sim.start(games)
    steps = 0
    while sim.counters()["finished"] < games and steps < max_steps:
        sim.step(net)
        steps += 1
    out = sim.records(), sim.all_counters(), sim.explore_counts()
    sim.close()
    return out


# ---------------------------------------------------------------- rows and positions the tests look at

def prior_kinds(A, legal, seed):
    """prior rows that take every branch of the rules: {name: float32[A]}"""
    rng = np.random.RandomState(seed)
    rand = rng.rand(A).astype(f32)
    rand = (rand / rand.sum()).astype(f32)
    big = rand.copy()
    lg = np.flatnonzero(legal)
    big[lg[: max(2, len(lg) // 6)]] = f32(0.05)                      # entries above 0.01
    big[lg[-3:-1]] = f32(0.0)                                        # exact zeros on legal points
    peaked = np.full(A, (1.0 - 0.6) / A, f32)
    peaked[lg[len(lg) // 2]] += f32(0.6)
    return {"random": rand, "constant": np.full(A, 1.0 / A, f32), "big_and_zero": big, "peaked": peaked}


def ko_position(N):
    """tw.ko_start(N); on the boards where seeded random play meets no ko early enough, the textbook shape played out"""
    try:
        return tw.ko_start(N)
    except AssertionError:
        pass
    b = np.zeros(N * N, np.int8)
    for (r, c), s in {(0, 1): 1, (1, 0): 1, (2, 1): 1, (1, 1): -1, (0, 2): -1, (2, 2): -1, (1, 3): -1}.items():
        b[r + N * c] = s
    rcode, pos = orc.play(orc.make_pos(N, board=b, n=8), 1 + N * 2)
    assert rcode == orc.OK and pos.ko == 1 + N * 1
    return pos.copy()


def positions(N):
    cap = tw.random_start(N, (N * N * 6) // 5, 40 + N)
    assert cap.caps[0] + cap.caps[1] > 0, "the random start has captures"
    return {"empty": orc.make_pos(N), "ko": ko_position(N), "captures": cap}


def pick_rows(A, seed):
    rng = np.random.RandomState(seed)
    one = np.zeros(A, f32)
    one[A // 3] = 5
    ties = np.zeros(A, f32)
    ties[[1, A // 2, A - 2]] = 7
    ties[2] = 3
    only_pass = np.zeros(A, f32)
    only_pass[A - 1] = 4
    big = np.zeros(A, f32)
    idx = rng.choice(A, min(A, 12), replace=False)
    big[idx] = rng.randint(1, 1601, len(idx))
    big[idx[0]] = 1600
    dense = rng.randint(0, 40, A).astype(f32)
    ones = np.ones(A, f32)
    return {"one": one, "ties": ties, "only_pass": only_pass, "big": big, "dense": dense, "ones": ones}


# ---------------------------------------------------------------- settings and game sets

GAME_SETTING = setting(pt=(1.25, 1.1, None), noise=(10.83, True), mt=(0.75, 0.0, 2.0))
SETTINGS = {
    "all": GAME_SETTING,
    "katago": KATAGO,
    "temper_only": setting(pt=(0.8, 1.3, 4.0)),
    "unit_temper": setting(pt=(1.0, 1.0, 7.0)),
    "unshaped": setting(noise=(3.0, False)),
    "shaped": setting(noise=(10.83, True)),
    "off": OFF,
}
GAME_SETS = {5: dict(R=24, seed=21, games=8, slots=4), 9: dict(R=32, seed=22, games=8, slots=4)}
COMPOSE = {"plain": {}, "cap": dict(cap=(8, 0.5)), "forced": dict(forced=(2.0, True)), "starts": dict(starts=True)}


def starts_of(N):
    return tw.random_starts(N, (4, 7, 1), seed=0)
