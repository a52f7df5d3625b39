"""Root exploration and the move temperature on the host simulator, CPU only: the rows of
agz_tree_explore_rows, the schedule, the picks and whole self-play games against the Python restatement of
tests/explore_twin.py, bit for bit; off against the simulator that never made the calls; and the same game set on a
stand-alone address + undefined sanitizer build of the simulator (the same boards, readouts, options and counts, on a
network and starts of its own); and the argument refusals, which the simulator's setters share with the engine (the
refusals that depend on an engine's state are in tests/test_gpu_explore.py)."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import alphago_jl_amd as ag
import explore_twin as ex
import hs
import orc
import selfplay_twin as tw
from explore_twin import COMPOSE, GAME_SETS, GAME_SETTING, SETTINGS, pick_rows, positions, starts_of
from gpu_options import assert_game_equals_twin

f32 = np.float32


# ---------------------------------------------------------------- rows

def root_at(sim, pos, game_id):
    """slot 0 of the simulator as a single tree on oracle position pos, its root expanded -> the root"""
    info = hs.PositionInfo()
    _, infos, hist = tw.opos_arrays([pos])
    for name, _ in hs.PositionInfo._fields_:
        setattr(info, name, getattr(infos[0], name))
    st, root = sim.op(hs.TOP_INIT, board=pos.board_np(), info=info, history=hist[0] if info.history_len else None)
    assert st == 0
    sim.L.hs_game_set(sim.h, 0, 0, float(game_id))
    st, leaf = sim.op(hs.TOP_SELECT, node=root)
    assert st == 0 and leaf == root
    st, _ = sim.op(hs.TOP_INCORPORATE, node=root, up_to=root, probs=np.full(sim.A, 1.0 / sim.A, f32), value=0.0)
    assert st == 0
    return root


def check_rows(sim, root, P, legal, n, seed, game, w, st, N, what):
    sim.row(0, root, 2)[:] = P
    sim.apply(st)
    t, al, nz = sim.explore_rows(root)
    wt, wal, wnz, _ = ex.explore_rows(P, legal, n, seed, game, w, st, N)
    assert (ex.bits32(t) == ex.bits32(wt)).all(), (what, "tempered")
    assert (ex.bits64(al) == ex.bits64(wal)).all(), (what, "alpha")
    assert (ex.bits32(nz) == ex.bits32(wnz)).all(), (what, "noised")
    assert (ex.bits32(sim.row(0, root, 2)) == ex.bits32(P)).all(), (what, "the read left the tree alone")
    return t, al, nz


def test_rows_equal_the_restatement():
    seed, game, w = 11, 6, 0.25
    flat_branch = shaped_branch = 0
    for N in (5, 9, 13, 19):
        A = N * N + 1
        assert {5: 26, 9: 82, 13: 170, 19: 362}[N] == A
        sim = hs.Sim(board_size=N, games=1, num_readouts=8, max_nodes_per_game=16, seed=seed)
        for pname, pos in positions(N).items():
            root = root_at(sim, pos, game)
            legal = sim.legal(0, root)
            assert (legal == orc.legal_moves(pos)).all()
            if pname != "empty":
                assert (legal[:A - 1] == 0).any(), "illegal points exist"
            kinds = ex.prior_kinds(A, legal, 7 * N)
            kinds["net"] = hs.PeakedNet(N)(orc.feats(pos).reshape(1, -1))[0][0]
            for kname, P in kinds.items():
                for sname, st in SETTINGS.items():
                    t, al, nz = check_rows(sim, root, P, legal, pos.n, seed, game, w, st, N, (N, pname, kname, sname))
                    lg = legal != 0
                    assert (ex.bits32(t)[~lg] == ex.bits32(P)[~lg]).all() and (t[lg & (P == 0)] == 0).all()
                    if st["noise"][0] > 0:
                        assert (al[~lg] == 0).all() and (ex.bits32(nz)[~lg] == ex.bits32(t)[~lg]).all()
                        assert abs(al.sum() - st["noise"][0]) < 1e-9 * st["noise"][0]
                        if st["noise"][1]:
                            flat = np.ptp(al[lg]) == 0
                            flat_branch += flat
                            shaped_branch += not flat
                    else:
                        assert (al == ex.legacy_alpha(A)).all()
                    if st["pt"] is not None and sname != "unit_temper" and kname != "constant":
                        assert (t != P).any(), (N, pname, kname, sname)
                    if st["pt"] is None:
                        assert (ex.bits32(t) == ex.bits32(P)).all()
        sim.close()
    assert flat_branch > 0 and shaped_branch > 0, (flat_branch, shaped_branch)


def test_off_rows_are_the_stored_noise():
    """with both root rules off TOP_NOISE stores what it stored before: the row the reference's rule gives, and the rows
    read says the same"""
    N, seed, game = 5, 3, 9
    sim = hs.Sim(board_size=N, games=1, num_readouts=8, max_nodes_per_game=16, seed=seed)
    pos = tw.random_start(N, 9, 1)
    root = root_at(sim, pos, game)
    P = ex.prior_kinds(sim.A, sim.legal(0, root), 1)["random"]
    sim.row(0, root, 2)[:] = P
    _, _, nz = sim.explore_rows(root)
    assert sim.op(hs.TOP_NOISE, node=root)[0] == 0
    assert (ex.bits32(sim.row(0, root, 2)) == ex.bits32(nz)).all()
    assert (ex.bits32(nz) == ex.bits32(ex.legacy_noise_row(P, seed, game, pos.n, 0.25))).all()
    assert sim.explore_counts() == (0, 0, 0, 0)
    # and under the rules TOP_NOISE stores the noised row and counts the root
    sim.row(0, root, 2)[:] = P
    sim.apply(GAME_SETTING)
    _, _, nz = sim.explore_rows(root)
    assert sim.explore_counts() == (0, 0, 0, 0)
    assert sim.op(hs.TOP_NOISE, node=root)[0] == 0
    assert (ex.bits32(sim.row(0, root, 2)) == ex.bits32(nz)).all()
    assert sim.explore_counts() == (1, 1, 0, 0)
    sim.close()


# ---------------------------------------------------------------- schedule

def test_schedule():
    Lx = hs.lib()
    for early, late, half in ((1.25, 1.1, 19.0), (0.75, 0.15, 9.0), (0.1, 10.0, 1.0), (3.0, 3.0, 5.0), (0.75, 0.0, 2.0)):
        # T(0) = late + (early - late) * 1.0: early exactly wherever the subtraction is exact (Sterbenz: late / 2 <= early
        # <= 2 late, and late = 0), which covers KataGo's schedules; elsewhere the two roundings leave at most an ulp of
        # the larger temperature each
        t0 = Lx.hs_temperature(0, early, late, half)
        if late == 0.0 or late / 2 <= early <= 2 * late:
            assert t0 == early
        else:
            assert abs(t0 - early) <= 2.0 ** -51 * max(early, late)
        ts =[Lx.hs_temperature(n, early, late, half) for n in range(0, 400)]
        assert ts == [ex.temperature(n, early, late, half) for n in range(0, 400)]
        d = np.diff(ts)
        assert (d <= 0).all() if early >= late else (d >= 0).all()
        if early == late:
            assert all(t == late for t in ts)
        else:
            assert abs(ts[int(half)] - (late + 0.5 * (early - late))) < 1e-12 or half != int(half)
            assert ts[-1] != early
    assert Lx.hs_temperature(10 ** 6, 2.0, 0.5, 1.0) == 0.5


# ---------------------------------------------------------------- picks

@pytest.mark.parametrize("N", [5, 9])
def test_picks_equal_the_restatement(N):
    seed, mt = 5, (0.75, 0.0, 2.0)
    sim = hs.Sim(board_size=N, games=1, num_readouts=8, max_nodes_per_game=16, seed=seed)
    off = hs.Sim(board_size=N, games=1, num_readouts=8, max_nodes_per_game=16, seed=seed)
    for s in (sim, off):
        root_at(s, orc.make_pos(N), 0)
    sim.apply(ex.setting(mt=mt))
    sampled = off_max = argmax = picked = 0
    for name, row in pick_rows(sim.A, N).items():
        picks = set()
        for key in range(200):
            n = key % 13 if key < 170 else 13 + key % 20           # T(12) = 0.0117 samples, T(13) = 0.0083 does not
            sim.set_pick_case(row, key, n)
            st, a = sim.op(hs.TOP_PICK)
            ok, wa, smp, om = ex.pick_move(row, n, seed, key, mt, N)
            assert ok and st == 0 and a == wa, (name, key, n, a, wa)
            assert row[a] > 0
            picks.add(a)
            sampled += smp
            off_max += om
            if not smp:
                assert n >= 13 >= off.tau
                off.set_pick_case(row, key, n)
                assert off.op(hs.TOP_PICK) == (0, a), (name, key)
                argmax += 1
        if name in ("ties", "dense", "ones"):
            assert len(picks) > 1, name
        picked += 1
    assert sim.explore_counts() == (0, 0, sampled, off_max) and sampled == 170 * picked and off_max > 0
    assert argmax == 30 * picked and off.explore_counts() == (0, 0, 0, 0)
    # no visited child at all: the soft pick's assertion
    sim.set_pick_case(np.zeros(sim.A, f32), 1, 0)
    assert sim.op(hs.TOP_PICK)[0] == ag._lib.ASSERT_SOFTPICK
    assert not ex.pick_move(np.zeros(sim.A, f32), 0, seed, 1, mt, N)[0]
    sim.close()
    off.close()


# ---------------------------------------------------------------- games

def play_set(N, how, st=GAME_SETTING, setting_for_sim="same"):
    c = GAME_SETS[N]
    kw = dict(COMPOSE[how])
    starts = starts_of(N) if kw.pop("starts", False) else None
    net = hs.PeakedNet(N)
    recs, cnt, counts = ex.run_sim(N, net, c["R"], c["seed"], c["games"], c["slots"],
                                   st if setting_for_sim == "same" else setting_for_sim, starts=starts, **kw)
    return recs, cnt, counts, starts, kw


@pytest.mark.parametrize("how", list(COMPOSE))
@pytest.mark.parametrize("N", [5, 9])
def test_games_equal_the_twin(N, how):
    c = GAME_SETS[N]
    recs, cnt, counts, starts, kw = play_set(N, how)
    assert len(recs) == c["games"] and cnt["CT_POOL_EXHAUSTED"] == 0
    cb = ex.FeatsNet(hs.PeakedNet(N), N).cb
    twins = []
    for rec in recs:
        gid = int(rec["game_id"])
        o = ex.twin_selfplay_explore(N, cb, c["R"], c["seed"], gid, GAME_SETTING,
                                     start=starts[gid % len(starts)] if starts else None, **kw)
        assert_game_equals_twin(rec, o, (N, how, gid), o["full"] if "cap" in kw else None)
        twins.append(o)
    print(N, how, "counters", counts, "argmax plies", sum(o["argmax_plies"] for o in twins))
    assert counts == ex.tallies(twins)
    assert cnt["CT_EVALS"] == sum(o["evals"] for o in twins)
    # the conditions of the set, on the twin's own games
    assert counts[2] > 0 and counts[3] > 0, "moves were sampled, some off the most visited child"
    assert sum(o["argmax_plies"] for o in twins) > 0, "a ply in the T <= 0.01 branch"
    assert sum(o["illegal_roots"] for o in twins) > 0, "a noised root with an illegal point"
    assert counts[0] == counts[1] > 0
    if "cap" in kw:
        assert any((~o["full"]).any() for o in twins) and counts[1] == sum(int(o["searched_full"].sum()) for o in twins)
    if "forced" in kw:
        assert sum(o["forced_sel"] for o in twins) > 0


@pytest.mark.parametrize("N", [5])
def test_the_rules_change_the_games_and_off_is_the_unset_simulator(N):
    on = play_set(N, "plain")
    never = play_set(N, "plain", setting_for_sim=None)
    off = play_set(N, "plain", setting_for_sim=ex.OFF)
    assert off[2] == never[2] == (0, 0, 0, 0)
    assert off[1] == never[1], "all counters"
    assert len(off[0]) == len(never[0])
    for a, b in zip(off[0], never[0]):
        assert a["game_id"] == b["game_id"] and (a["moves"] == b["moves"]).all() and a["result"] == b["result"]
        assert (ex.bits32(a["pis"]) == ex.bits32(b["pis"])).all() and (ex.bits32(a["qs"]) == ex.bits32(b["qs"])).all()
    assert any(len(a["moves"]) != len(b["moves"]) or (a["moves"] != b["moves"]).any() for a, b in zip(on[0], never[0]))


# ---------------------------------------------------------------- refusals

REFUSED = {
    "hs_set_root_policy_temperature": ((2, 1.0, 1.0, 1.0), (-1, 1.0, 1.0, 1.0), (1, float("nan"), 1.0, 1.0),
                                       (1, 1.0, float("nan"), 1.0), (1, 1.0, 1.0, float("nan")), (1, 0.0999, 1.0, 1.0),
                                       (1, 1.0, 10.001, 1.0), (1, 1.0, 1.0, 0.0), (1, 1.0, 1.0, -1.0),
                                       (1, 1.0, 1.0, 1.0000001e6), (0, 0.05, 1.0, 1.0)),
    "hs_set_move_temperature": ((2, 1.0, 1.0, 1.0), (1, float("nan"), 1.0, 1.0), (1, -1e-9, 1.0, 1.0),
                                (1, 1.0, 10.001, 1.0), (1, 1.0, 1.0, 0.0), (1, 1.0, 1.0, float("nan")),
                                (1, 1.0, 1.0, 1.0000001e6), (1, 11.0, 1.0, 1.0)),
    "hs_set_root_noise": ((float("nan"), 0), (-1e-9, 0), (1000.001, 0), (1.0, 2), (1.0, -1), (0.0, 1)),
}
TAKEN = (("hs_set_root_policy_temperature", (1, 0.1, 10.0, 1.0e6)), ("hs_set_move_temperature", (1, 0.0, 10.0, 1.0e6)),
         ("hs_set_root_noise", (1000.0, 1)), ("hs_set_root_noise", (0.0, 0)))


def test_refusals_keep_the_setting():
    """the argument checks the engine and the simulator share (explore_*_refusal, agz_state.h): every refusal leaves
    the setting in force, shown by the rows read before and after and, for the move temperature, by the pick.  (Games in
    flight and a pending select phase are states of the engine alone: tests/test_gpu_explore.py.)"""
    N, seed, game = 5, 1, 3
    kept = ex.setting(pt=(1.3, 0.9, 4.0), noise=(5.0, True), mt=(0.8, 0.2, 3.0))
    sim = hs.Sim(board_size=N, games=1, num_readouts=8, max_nodes_per_game=16, seed=seed)
    pos = tw.random_start(N, 6, 2)
    root = root_at(sim, pos, game)
    legal = sim.legal(0, root)
    P = ex.prior_kinds(sim.A, legal, 3)["big_and_zero"]
    sim.row(0, root, 2)[:] = P
    visits = np.zeros(sim.A, f32)
    visits[np.flatnonzero(legal)[[1, 4, 6]]] = (5, 9, 2)
    sim.apply(kept)

    def in_force(what):
        t, al, nz = sim.explore_rows(root)
        wt, wal, wnz, _ = ex.explore_rows(P, legal, pos.n, seed, game, 0.25, kept, N)
        assert (ex.bits32(t) == ex.bits32(wt)).all() and (ex.bits64(al) == ex.bits64(wal)).all(), what
        assert (ex.bits32(nz) == ex.bits32(wnz)).all(), what
        for key in range(8):
            sim.set_pick_case(visits, key, pos.n)
            assert sim.op(hs.TOP_PICK) == (0, ex.pick_move(visits, pos.n, seed, key, kept["mt"], N)[1]), what
        sim.L.hs_game_set(sim.h, 0, 0, float(game))

    for fn, cases in REFUSED.items():
        for args in cases:
            in_force(("before", fn, args))
            assert getattr(sim.L, fn)(sim.h, *args) == ag._lib.BAD_ARGUMENT, (fn, args)
            in_force((fn, args))
    for fn, args in TAKEN:                            # the bounds themselves are in range
        assert getattr(sim.L, fn)(sim.h, *args) == 0, (fn, args)
    sim.close()
    arena = hs.Sim(board_size=N, games=2, num_readouts=8, max_nodes_per_game=16, arena_mode=1)
    for fn, args in TAKEN + (("hs_set_root_policy_temperature", (0, 1.0, 1.0, 1.0)), ("hs_set_move_temperature", (0, 1.0, 1.0, 1.0))):
        assert getattr(arena.L, fn)(arena.h, *args) == ag._lib.BAD_ARGUMENT, ("arena", fn, args)
    arena.close()


# ---------------------------------------------------------------- sanitizers

def _static_sanitizer_runtimes():
    """are libasan.a and libubsan.a where g++ looks for them?"""
    if not shutil.which("g++"):
        return False
    for name in ("libasan.a", "libubsan.a"):
        r = subprocess.run(["g++", "-print-file-name=" + name], capture_output=True, text=True)
        if r.returncode != 0 or not os.path.isabs(r.stdout.strip()) or not os.path.exists(r.stdout.strip()):
            return False
    return True


@functools.lru_cache(None)
def _sanitizer_program():
    """hostsim.cpp with the main of hostsim_sanitize.cpp under -fsanitize=address,undefined (the `sanitize` target of
    tests/hostsim/Makefile), built once per test process into a directory of its own -> (the program, make's result)"""
    d = tempfile.mkdtemp(prefix="hostsim_sanitize_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "hostsim_sanitize")
    return exe, subprocess.run(["make", "-s", "-C", os.path.join(hs.HERE, "hostsim"), "sanitize", "SANITIZE_OUT=" + exe],
                               capture_output=True, text=True)


def run_sanitizer_part(part):
    """one part of the sanitizer program (explore, uncertainty, superko): a program of its own with both runtimes linked
    into it (so it starts in whatever environment the suite runs in, which is left as it is).  Skipped where g++ or its
    static sanitizer runtimes are missing."""
    if not _static_sanitizer_runtimes():
        pytest.skip("no g++ with static libasan / libubsan")
    exe, r = _sanitizer_program()
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, part], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "games played" in r.stdout and "ERROR" not in r.stderr


def test_sanitizer_build_plays_the_game_set():
    """The `explore` part.  A check of memory and undefined behaviour, not of results: it plays the boards, readouts,
    setting, cap, forced playouts, a table of three starts and the game counts of the sets above, but on a hash network
    and walk starts of its own, not on PeakedNet and tw.random_starts."""
    run_sanitizer_part("explore")
