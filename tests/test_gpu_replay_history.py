"""The replay arena through one history of calls against a host model: a targets-only arena is filled,
scored in part, windowed without and with a physical drop, scored again, filled, trimmed, cleared and filled once more.
After every step the arena's counts, every game (agz_replay_game), every game's scores (agz_replay_surprise: the KL bits
and the scored flag) and a batch over every live entry (agz_replay_batch) are what a model says that is built from the
packed bytes on the host: a list of games with their byte sizes, the window as (first game, first target) and the rules
of agz_replay_set_window / agz_replay_trim restated over that list.  The expected scores come from the engine-free
agz_surprise_weights on priors evaluated game by game, the expected features from an arena that is never changed."""
import numpy as np
import pytest

import alphago_jl_amd as ag
import surprise_twin as st
from gpu_options import play
from test_gpu_surprise import priors
from test_hostsim_selfplay import bits_equal

pytestmark = pytest.mark.gpu

N, TOWER, R, GAMES, SLOTS, SEED = 5, 1, 8, 12, 4, 3
A = N * N + 1
HEADER = ("game_id", "num_moves", "result", "was_resign", "resign_disabled", "short_searches")


def engine():
    e = ag.Engine(board_size=N, tower_height=TOWER, games=SLOTS, num_readouts=R, seed=SEED, record_capacity_games=GAMES + 8)
    e.init_synthetic(0)
    return e


class Model:
    """the arena as a list of games (targets-only): g = dict(rec, orig, bytes, targets, scored)"""

    def __init__(self):
        self.games, self.first_game, self.first_entry = [], 0, 0

    def tcum(self):
        return np.concatenate([[0], np.cumsum([int(g["targets"].sum()) for g in self.games])]).astype(np.int64)

    def offsets(self):
        return np.concatenate([[0], np.cumsum([g["bytes"] for g in self.games])]).astype(np.int64)

    def positions(self):
        return sum(g["rec"]["num_moves"] for g in self.games)

    def live(self):
        return int(self.tcum()[-1] - self.tcum()[self.first_game] - self.first_entry)

    def live_entries(self):
        out = []
        for k in range(self.first_game, len(self.games)):
            t = np.flatnonzero(self.games[k]["targets"])
            out += [(k, int(p)) for p in (t[self.first_entry:] if k == self.first_game else t)]
        return out

    def ingest(self, games):
        self.games += [dict(g, scored=False) for g in games]

    def drop_front(self, n):
        del self.games[:n]
        if self.first_game >= n:
            self.first_game -= n
        else:
            self.first_game = self.first_entry = 0

    def clear(self):
        self.games, self.first_game, self.first_entry = [], 0, 0

    def set_window(self, max_entries):
        """-> the number of games dropped physically"""
        ec, off = self.tcum(), self.offsets()
        first = max(int(ec[self.first_game]) + self.first_entry, int(ec[-1]) - max_entries)
        k = self.first_game
        while k < len(self.games) and ec[k + 1] <= first:
            k += 1
        if k == len(self.games):
            self.clear()
            return k
        self.first_game, self.first_entry = k, first - int(ec[k])
        if k > 0 and off[k] > off[-1] // 2:
            self.drop_front(k)
            return k
        return 0

    def trim(self, max_positions):
        drop, pos = 0, self.positions()
        while drop < len(self.games) and pos > max_positions:
            pos -= self.games[drop]["rec"]["num_moves"]
            drop += 1
        if drop == len(self.games):
            self.clear()
        elif drop:
            self.drop_front(drop)
        return drop


def check(e, m, ref, want_kl, what):
    n = len(m.games)
    assert (e.replay_count(), e.replay_positions(), e.replay_live_positions()) == (n, m.positions(), m.live()), what
    for k, g in enumerate(m.games):
        got, rec = e.replay_record(k), g["rec"]
        assert all(got[f] == rec[f] for f in HEADER) and np.float32(got["final_score"]) == np.float32(rec["final_score"])
        assert (got["moves"] == rec["moves"]).all() and bits_equal(got["pis"], rec["pis"]), (what, k)
        assert bits_equal(got["qs"], rec["qs"]), (what, k)
        kl, _, scored = e.replay_surprise(k)
        assert scored == g["scored"], (what, k)
        want = want_kl[g["orig"]] if scored else np.zeros(rec["num_moves"])
        assert (st.bits(kl) == st.bits(want)).all(), (what, k)
    entries = m.live_entries()
    assert len(entries) == m.live()
    if entries:
        game, ply = np.array([a for a, _ in entries], np.int64), np.array([b for _, b in entries], np.int32)
        f, p, z = e.replay_batch(game, ply)
        orig = np.array([m.games[a]["orig"] for a in game], np.int64)
        wf, wp, wz = ref.replay_batch(orig, ply)
        assert bits_equal(f, wf) and bits_equal(p, wp) and bits_equal(z, wz), what
        assert bits_equal(p, np.stack([m.games[a]["rec"]["pis"][b] for a, b in entries])), what
        assert (p != 0).any(axis=1).all() and (z == [m.games[a]["rec"]["result"] for a in game]).all(), what
    print(f"{what}: {n} games, {m.positions()} plies, {m.live()} live, window ({m.first_game}, {m.first_entry}), "
          f"scored {[int(g['scored']) for g in m.games]}")


def test_history_of_a_targets_only_arena_equals_the_host_model():
    src = engine()
    src.set_playout_cap(2, 0.5)
    assert len(play(src, GAMES)[0]) == GAMES
    packed = src.records_packed().copy()
    src.close()
    recs = ag.distributed.unpack_records(packed, A)
    pack = lambda rs: ag.distributed.pack_records(rs, A)
    games = [dict(rec=r, orig=k, bytes=len(pack([r])), targets=(r["pis"] != 0).any(axis=1)) for k, r in enumerate(recs)]
    assert sum(g["bytes"] for g in games) == len(packed)
    print("games (moves, targets):", [(g["rec"]["num_moves"], int(g["targets"].sum())) for g in games])
    assert any((~g["targets"]).any() for g in games), "the playout cap left no zero row"
    ref = engine()                                               # every game in an arena that is never changed
    assert ref.replay_ingest(packed) == GAMES
    want_kl = [ag.surprise_weights(g["rec"]["pis"], priors(ref, k), 0.0)[0] for k, g in enumerate(games)]

    e, m = engine(), Model()
    e.replay_set_targets_only(True)

    def ingest(lo, hi, what):
        assert e.replay_ingest(pack(recs[lo:hi])) == hi - lo
        m.ingest(games[lo:hi])
        check(e, m, ref, want_kl, what)

    def score(first, count, what):
        want = sum(int(g["targets"].sum()) for g in m.games[first:first + count])
        assert e.replay_score(first, count) == want
        for g in m.games[first:first + count]:
            g["scored"] = True
        check(e, m, ref, want_kl, what)

    ingest(0, 4, "ingest 4")
    score(0, 2, "score games 0-1")
    ingest(4, 8, "ingest 4 more")

    # a window that begins at the second target of a game and leaves less than half of the bytes dead: nothing dropped
    tc, off = m.tcum(), m.offsets()
    g1 = next(k for k in range(1, 8) if tc[k + 1] - tc[k] >= 2)
    assert off[g1] <= off[-1] // 2, "the first game with two targets lies behind half of the bytes"
    e.replay_set_window(int(tc[-1] - tc[g1]) - 1)
    assert m.set_window(int(tc[-1] - tc[g1]) - 1) == 0 and (m.first_game, m.first_entry) == (g1, 1)
    check(e, m, ref, want_kl, "window inside a game")

    # a smaller one whose dead games hold more than half of the bytes: they go, the scored ones among them
    g2 = next(k for k in range(g1 + 1, 8) if off[k] > off[-1] // 2)
    inside = 1 if tc[g2 + 1] - tc[g2] >= 2 else 0
    assert g2 < 7 or inside, "the window would be empty"
    e.replay_set_window(int(tc[-1] - tc[g2]) - inside)
    assert m.set_window(int(tc[-1] - tc[g2]) - inside) == g2 and len(m.games) == 8 - g2
    assert (m.first_game, m.first_entry) == (0, inside)
    check(e, m, ref, want_kl, "window with a physical drop")

    score(len(m.games) - 1, 1, "score the newest game")
    ingest(8, 12, "ingest 4 more")
    first_len = m.games[0]["rec"]["num_moves"]
    e.replay_trim(m.positions() - first_len)
    assert m.trim(m.positions() - first_len) == 1
    check(e, m, ref, want_kl, "trim by one game")
    assert any(g["scored"] for g in m.games) and not all(g["scored"] for g in m.games)
    e.replay_clear()
    m.clear()
    check(e, m, ref, want_kl, "clear")
    ingest(0, 2, "ingest 2")
    assert not any(g["scored"] for g in m.games)
    for x in (e, ref):
        x.close()
