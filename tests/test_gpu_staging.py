"""The host staging buffers of the engine (the s_* scratch behind the C ABI) are reused across calls, batch sizes and
roles: s_f32a_ is x32 in one call and features in the next, s_i32a_ is ndeltas, then ko, then a carved block of four
arrays.  What can go wrong there is a pointer that is stale after a regrow, a size taken from a buffer's capacity, or
one buffer serving two roles in one call.  So ONE long-lived engine runs the batch sizes 1, 6, 2 (grow, regrow, shrink
into an oversize buffer), and at each size every entry point below in turn, so that the shared buffers change roles
between consecutive calls.  Expected: for each entry point an engine of its own (same config, same weights, arena filled
from the same packed records) that is called exactly once, at B = 6.  Rows do not depend on batch composition
(DESIGN.md section 4), so the long-lived engine's outputs at size B are the first B rows of that, bit for bit."""
import numpy as np
import pytest

import alphago_jl_amd as ag
from gpu_common import pos_soa
from test_hostsim_go import random_positions

pytestmark = pytest.mark.gpu

CFG = dict(board_size=5, tower_height=1, games=2, num_readouts=8, max_nodes_per_game=16)
N, P, A = 5, 25, 26
SIZES = (1, 6, 2)
BMAX = 6
GAMES = 3
CALLS = ("forward", "go_play", "forward_features", "go_legal", "forward_features_sym", "go_score", "features",
         "replay_features", "replay_batch", "replay_batch_sym", "debug_math")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def engine():
    eng = ag.Engine(seed=3, record_capacity_games=GAMES + 4, **CFG)
    eng.init_synthetic(11)
    return eng


def inputs(records):
    """the size-6 inputs; size B takes their first B rows"""
    rng = np.random.RandomState(5)
    reached = random_positions(N, 2, 30, seed=17)
    positions = [reached[i] for i in rng.choice(len(reached), BMAX, replace=False)]
    boards, deltas, nd, tp = pos_soa(positions)
    x = dict(boards=boards, deltas=deltas, nd=nd, tp=tp)
    x["ko"] = np.array([p.ko for p in positions], np.int32)
    x["moves"] = rng.randint(0, A, BMAX).astype(np.int32)
    x["komi"] = rng.choice([0.5, 5.5, 6.5, 7.5], BMAX).astype(np.float32)
    x["feats"] = (rng.rand(BMAX, 17 * P) < 0.3).astype(np.float32)
    x["sym"] = rng.randint(0, 8, BMAX).astype(np.int32)
    # replay: sample b is ply[b] of arena game game[b]; for agz_replay_features the games' move lists back to back
    played = [k for k, r in enumerate(records) if r["num_moves"] > 0]
    x["game"] = rng.choice(played, BMAX).astype(np.int64)
    x["ply"] = np.array([rng.randint(0, records[g]["num_moves"]) for g in x["game"]], np.int32)
    x["all_moves"] = np.concatenate([r["moves"] for r in records]).astype(np.int16)
    starts = np.concatenate([[0], np.cumsum([r["num_moves"] for r in records])])
    x["off"] = starts[x["game"]].astype(np.int32)
    x["mx"] = rng.uniform(0.1, 40.0, BMAX)
    x["my"] = rng.uniform(0.0, 30.0, BMAX)
    return x


def call(eng, name, x, B):
    """entry point `name` on the first B rows of the inputs; its outputs as a tuple of arrays"""
    r = lambda k: x[k][:B]
    if name == "forward":
        return eng.forward(r("boards"), r("deltas"), r("nd"), r("tp"))
    if name == "go_play":
        return eng.go_play(r("boards"), r("tp"), r("ko"), r("moves"))
    if name == "forward_features":
        return eng.forward_features(r("feats"))
    if name == "go_legal":
        return (eng.go_legal(r("boards"), r("tp"), r("ko")),)
    if name == "forward_features_sym":
        return eng.forward_features_sym(r("feats"), r("sym"))
    if name == "go_score":
        return (eng.go_score(r("boards"), r("komi")),)
    if name == "features":
        return (eng.features(r("boards"), r("deltas"), r("nd"), r("tp")),)
    if name == "replay_features":
        return (eng.replay_features(x["all_moves"], r("off"), r("ply")),)
    if name == "replay_batch":
        return eng.replay_batch(r("game"), r("ply"))
    if name == "replay_batch_sym":
        return eng.replay_batch_sym(r("game"), r("ply"), r("sym"))
    if name == "debug_math":
        return (eng.debug_math(5, r("mx"), r("my")),)
    raise KeyError(name)


@pytest.fixture(scope="module")
def runs():
    """(got[(B, name)], want[name]): the long-lived engine at every size, and the one-call engines at B = 6"""
    eng = engine()
    eng.start(GAMES)
    for _ in range(2000):
        if eng.records_count() >= GAMES:
            break
        eng.step(8)
    assert eng.records_count() == GAMES
    packed = eng.records_packed().copy()
    assert eng.replay_ingest(packed) == GAMES
    records = [eng.replay_record(k) for k in range(GAMES)]
    x = inputs(records)
    got = {(B, name): call(eng, name, x, B) for B in SIZES for name in CALLS}
    eng.close()
    want = {}
    for name in CALLS:
        ref = engine()
        assert ref.replay_ingest(packed) == GAMES
        want[name] = call(ref, name, x, BMAX)
        ref.close()
    return got, want


@pytest.mark.parametrize("name", CALLS)
def test_reused_staging_buffers_answer_as_fresh_ones(runs, name):
    got, want = runs
    for B in SIZES:
        assert len(got[(B, name)]) == len(want[name])
        for k, (g, w) in enumerate(zip(got[(B, name)], want[name])):
            assert g.shape[0] == B and g.dtype == w.dtype, (name, B, k)
            assert bits_equal(g, w[:B]), (name, B, k)


def test_the_inputs_exercise_the_calls(runs):
    """the comparison above means something: outputs differ from row to row and the rule calls hit their branches"""
    _, want = runs
    pi, v = want["forward"]
    assert len({r.tobytes() for r in pi}) == BMAX and np.isfinite(pi).all() and np.isfinite(v).all()
    assert len({r.tobytes() for r in want["features"][0]}) == BMAX
    assert len({r.tobytes() for r in want["replay_batch"][0]}) > 1
    assert not bits_equal(want["replay_batch"][0], want["replay_batch_sym"][0])
    assert not bits_equal(want["forward_features"][0], want["forward_features_sym"][0])
    assert want["go_legal"][0].any() and np.isfinite(want["debug_math"][0]).all()
