"""The fp16-operand tower (agz_net_set_precision(F16), BASELINE.json configs[4]: "fp16 MFMA path,
mixed-precision inference") against the oracle.

Two bars, both written here:
  * TOL16 = 5e-4 against the oracle's restatement of THIS arithmetic (precision 16: weights and tower
    activations rounded to IEEE half at the points where the GPU stores them, sums in float64).  What
    is left is f32-vs-f64 accumulation, which now and then moves a value across a half rounding
    boundary (one half ulp = 4.9e-4 relative of that activation).
  * TOLMIX = 1e-2 against the exact f64 network: the price of half storage itself -- this mode does
    NOT meet the 1e-4 bar of the default f32 path and is not what bench.py measures.
Both bars have to let through the half roundings that f32 and f64 sums place differently, and one such flip is as large as
a small structural defect (a truncating store in one epilogue passes every test of this file).  Structural defects of the
fp16 kernels -- a tap, a halo row, a tile edge, the late flush of the output image, a rounding mode -- are caught in
tests/test_gpu_exact_tower.py, on networks whose every rounded value is an integer: there the trunk has to agree exactly.
Integer/tree work stays bit-exact in this mode too: self-play games equal the oracle's when the
oracle's network callable is this same HIP network."""
import numpy as np
import pytest

import alphago_jl_amd as ag
import orc
from gpu_common import GpuNetForOracle, copy_weights_from_oracle, pos_soa
from test_gpu_nn import oracle_forward64
from test_gpu_selfplay import check_against_oracle, run
from test_hostsim_go import random_positions
from test_oracle_nn import randomize_bn

pytestmark = pytest.mark.gpu
L = orc.lib()
TOL16, TOLMIX = 5e-4, 1e-2


@pytest.mark.parametrize("N,tower,B", [(5, 1, 7), (9, 2, 37), (9, 10, 16), (19, 3, 5), (7, 2, 70)])
def test_f16_forward_matches_oracle(N, tower, B):
    A = N * N + 1
    rng = np.random.RandomState(N + tower)
    onet = L.or_net_new(N, tower)
    L.or_net_init_synthetic(onet, 3)
    randomize_bn(onet, list(range(0, 1 + 2 * tower)) + [orc.L_VALUE_CONV, orc.L_POLICY_CONV], rng)
    eng = ag.Engine(board_size=N, games=1, tower_height=tower, num_readouts=8, max_nodes_per_game=16)
    copy_weights_from_oracle(eng, onet, tower)
    positions = random_positions(N, 4, 80, seed=7)
    positions = [positions[i] for i in rng.choice(len(positions), B, replace=False)]
    feats = np.stack([orc.feats(p).reshape(-1) for p in positions]).astype(np.float32)
    pi32, v32 = eng.forward(*pos_soa(positions))                 # default path, before the switch
    eng.set_precision("f16")
    gpi, gv = eng.forward(*pos_soa(positions))
    pi16, v16 = np.zeros((B, A), np.float32), np.zeros(B, np.float32)
    L.or_net_forward_feats(onet, orc.fptr(feats), B, orc.fptr(pi16), orc.fptr(v16), 16)
    pi64, v64 = oracle_forward64(onet, feats, A)
    d16 = max(np.abs(gpi - pi16).max(), np.abs(gv - v16).max())
    dmix = max(np.abs(gpi - pi64).max(), np.abs(gv - v64).max())
    print(f"N={N} tower={tower}: vs fp16 restatement {d16:.2e}, vs f64 {dmix:.2e}")
    assert d16 <= TOL16, d16
    assert dmix <= TOLMIX, dmix
    assert np.allclose(gpi.sum(1), 1, atol=1e-5)
    if tower >= 2:
        assert (gpi != pi32).any() or (gv != v32).any()          # it really is a different arithmetic
    # entry points agree, outputs do not depend on batch neighbours (tree parity relies on it)
    fpi, fv = eng.forward_features(feats)
    assert (fpi == gpi).all() and (fv == gv).all()
    perm = rng.permutation(B)
    ppi, pv = eng.forward(*pos_soa([positions[i] for i in perm]))
    assert (ppi == gpi[perm]).all() and (pv == gv[perm]).all()
    spi, sv = eng.forward(*pos_soa(positions[:1]))
    assert (spi[0] == gpi[0]).all() and sv[0] == gv[0]
    # and back: the switch is not sticky
    eng.set_precision("f32")
    bpi, bv = eng.forward(*pos_soa(positions))
    assert (bpi == pi32).all() and (bv == v32).all()
    L.or_net_free(onet)
    eng.close()


@pytest.mark.parametrize("N,B", [(3, 25), (4, 14), (4, 15), (6, 70), (13, 9), (16, 8), (9, 300)])
def test_f16_tile_geometry(N, B):
    """the persistent fp16 convolution works on 224-row tiles of consecutive board points: batches that end exactly
    on a tile (4x4 x 14 = 224 rows), one row past it, well inside one, across several workgroups' second tiles
    (9x9 x 300 = 108 tiles... of 256 CUs: one each; the full batch of test_gpu_nn.py gives every workgroup 11-12),
    and halos of every size class (N + 1 = 4 .. 17 rows).  Bars as in test_f16_forward_matches_oracle."""
    tower = 2
    A = N * N + 1
    rng = np.random.RandomState(100 + N)
    onet = L.or_net_new(N, tower)
    L.or_net_init_synthetic(onet, 3)
    randomize_bn(onet, list(range(0, 1 + 2 * tower)) + [orc.L_VALUE_CONV, orc.L_POLICY_CONV], rng)
    eng = ag.Engine(board_size=N, games=1, tower_height=tower, num_readouts=8, max_nodes_per_game=16)
    copy_weights_from_oracle(eng, onet, tower)
    eng.set_precision("f16")
    feats = (rng.rand(B, 17 * N * N) < 0.3).astype(np.float32)
    feats[:, 16 * N * N:] = np.where(rng.rand(B, 1) < 0.5, 1.0, -1.0)
    pi16, v16 = np.zeros((B, A), np.float32), np.zeros(B, np.float32)
    L.or_net_forward_feats(onet, orc.fptr(feats), B, orc.fptr(pi16), orc.fptr(v16), 16)
    gpi, gv = eng.forward_features(feats)
    d16 = max(np.abs(gpi - pi16).max(), np.abs(gv - v16).max())
    assert d16 <= TOL16, d16
    for k in (0, B // 2, B - 1):                                   # a row's result does not depend on its tile
        spi, sv = eng.forward_features(feats[k:k + 1])
        assert (spi[0] == gpi[k]).all() and sv[0] == gv[k], k
    L.or_net_free(onet)
    eng.close()


@pytest.mark.parametrize("N,tower,readouts,games,slots", [(5, 2, 16, 4, 4), (9, 2, 24, 2, 2)])
def test_f16_selfplay_games_match_oracle(N, tower, readouts, games, slots):
    eng = ag.Engine(board_size=N, tower_height=tower, games=slots, num_readouts=readouts, seed=6,
                    record_capacity_games=games + 8)
    eng.init_synthetic(0)
    eng.set_precision("f16")
    recs, st = run(eng, games)
    assert len(recs) == games and st["pool_exhausted"] == 0
    fwd = ag.Engine(board_size=N, tower_height=tower, games=1, num_readouts=8, max_nodes_per_game=16)
    fwd.init_synthetic(0)
    fwd.set_precision("f16")
    moves, evals = check_against_oracle(recs, GpuNetForOracle(fwd), N, readouts, 6)
    assert st["positions"] == moves and st["evals"] == evals
    fwd.close()
    eng.close()


def test_precision_argument_is_checked():
    eng = ag.Engine(board_size=5, tower_height=1, games=1, num_readouts=8, max_nodes_per_game=16)
    with pytest.raises(ag.AgzError):
        eng._ck(eng.L.agz_net_set_precision(eng.h, 7))
    eng.close()


def test_api_precision_switch():
    env = ag.GoEnv(5)
    nn = ag.NeuralNet(env, tower_height=2, seed=0)
    f32 = ag.selfplay(env, nn, 16, games=3, seed=4)
    f16 = ag.selfplay(env, nn, 16, games=3, seed=4, precision="f16")
    again = ag.selfplay(env, nn, 16, games=3, seed=4, precision="f16")
    assert [r.moves for r in f16] == [r.moves for r in again]              # deterministic in either arithmetic
    assert len(f32) == len(f16) == 3 and all(len(r.moves) > 0 for r in f16)
    nn.set_precision("f16")
    pi, v = nn(ag.Position(env))
    assert abs(pi.sum() - 1) < 1e-5 and -1 <= v <= 1
    nn.engine.close()
