"""The twin of reanalysis (include/agz.h agz_replay_reanalyze_start / _commit).  TEST INFRASTRUCTURE.

What a reanalysis run must compute for one arena game is a plain loop over interfaces that exist:

    p = MCTSPlayer(env, nn, R, seed=seed, game_id=base + gid);  initialize_game!(p, start)
    for each recorded move m_k:  suggest_move(p);  play_move!(p, m_k)

and the expected rows are p.searches_pi[k] and p.qs[k], which play_move! itself appends (mcts_play.jl:26-50).  twin_rows is
that loop on the oracle's player (or_player_*), whose network is any or_net_fn: the CPU oracle network, or the HIP forward
behind gpu_common.GpuNetForOracle, so that the rows are bit for bit what the device must give.  refresh is the commit rule
in numpy."""
import ctypes as C

import numpy as np

import alphago_jl_amd as ag
import orc

L = orc.lib()
PAR = 8                      # tree_search!'s parallel_readouts, agz_config's default
OK = ag._lib.OK


def twin_rows(N, net_cb, R, seed, game_id, moves, start=None, threshold=-0.9):
    """The loop above on the oracle's player; start: an oracle position or None.  -> dict(pis float32 [n][A], qs float32
    [n], visits float32 [n][A]: the root's child_N when ply k's search ended, n0: position.n of the start, tau: the
    player's tau_threshold)"""
    A = N * N + 1
    visits = []
    op = L.or_player_new(N, net_cb, None, R, 0, threshold, seed, game_id)
    L.or_player_initialize_game(op, None if start is None else C.byref(start))
    for m in moves:
        root = L.or_player_root(op)
        n0 = L.or_node_N(root)
        while L.or_node_N(L.or_player_root(op)) < n0 + R:               # suggest_move, mcts_play.jl:144-151
            L.or_player_tree_search(op, PAR)
        a = C.c_int(-1)
        L.or_player_pick_move(op, C.byref(a))
        visits.append(orc.node_arr(L.or_node_child_N(L.or_player_root(op)), A).copy())
        assert L.or_player_play_move(op, int(m)) == 1, (game_id, int(m))
    n = len(moves)
    assert L.or_player_num_moves(op) == n and L.or_player_nqs(op) == n
    pis = np.stack([orc.node_arr(L.or_player_search_pi(op, k), A).copy() for k in range(n)]) if n else \
        np.zeros((0, A), np.float32)
    qs = np.array([L.or_player_q(op, k) for k in range(n)], np.float32)
    tau = L.or_player_tau_threshold(op)
    L.or_player_free(op)
    return dict(pis=pis, qs=qs, visits=np.array(visits, np.float32).reshape(n, A), n0=0 if start is None else start.n,
                tau=tau)


def refresh(record, rows, status):
    """The commit rule.  record: dict with pis [n][A] and qs [n]; rows = (pis [n][A], qs [n]) of the run; status [n].
    -> (new pis, new qs, (rows committed, pi rows overwritten, rows skipped)).  A row is committed iff its status is OK:
    its q is written, and its pi row unless the record's row is all zero, which stays all zero."""
    pis = np.array(record["pis"], np.float32, copy=True)
    qs = np.array(record["qs"], np.float32, copy=True)
    new_pi, new_q = rows
    committed = written = skipped = 0
    for k, st in enumerate(status):
        if int(st) != OK:
            skipped += 1
            continue
        committed += 1
        qs[k] = new_q[k]
        if (pis[k] != 0).any():
            pis[k] = new_pi[k]
            written += 1
    return pis, qs, (committed, written, skipped)
