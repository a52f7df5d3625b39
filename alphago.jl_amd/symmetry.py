"""The eight symmetries of the Go board (DESIGN.md "Board symmetries").

The host mirror of `sym_point` / `sym_inverse` in csrc/agz_layout.h, which every kernel uses.  Points follow
`api.to_flat`: p = row + N*col, p == N*N is pass.  For s in 0..7, T_s(row, col) does, in order:
  1. s & 4: swap row and col;  2. s & 2: row = N-1-row;  3. s & 1: col = N-1-col.
T_0 is the identity and pass maps to pass.  A position under T_s has X'[plane][T_s(p)] = X[plane][p]; the prior of move
p is then net(X').pi[T_s(p)] (`apply_policy(pi, inverse(s), N)` brings a policy back), the value is net(X').v.
The quarter turns 5 and 6 are each other's inverse; every other T_s is its own.
"""
import numpy as np

RANDOM = 8           # AGZ_SYMMETRY_RANDOM
NONE = -1            # AGZ_SYMMETRY_NONE
SITE_SYMMETRY = 8    # AGZ_SITE_SYMMETRY (include/agz_draws.h)

_M64 = (1 << 64) - 1


def transform_points(s, N):
    """int64[N*N + 1]: t[p] = T_s(p), pass included"""
    p = np.arange(N * N)
    r, c = p % N, p // N
    if s & 4:
        r, c = c, r
    if s & 2:
        r = N - 1 - r
    if s & 1:
        c = N - 1 - c
    return np.concatenate([r + N * c, [N * N]]).astype(np.int64)


def inverse(s):
    """the index of T_s^-1"""
    return s if s < 4 else 4 | ((s & 1) << 1) | ((s >> 1) & 1)


def apply_features(feats, s, N):
    """feature rows [..., planes*N*N] (agz_features order, [plane][p] per row) under T_s: out[plane][T_s(p)] = in[plane][p]"""
    f = np.asarray(feats)
    t = transform_points(s, N)[:-1]
    x = f.reshape(f.shape[:-1] + (-1, N * N))
    out = np.empty_like(x)
    out[..., t] = x
    return out.reshape(f.shape)


def apply_policy(pi, s, N):
    """policy rows [..., N*N + 1] under T_s: out[T_s(p)] = pi[p], pass unchanged.  The policy a network returns for a
    position under T_s comes back to board orientation with apply_policy(pi, inverse(s), N)."""
    x = np.asarray(pi)
    out = np.empty_like(x)
    out[..., transform_points(s, N)] = x
    return out


def _mix64(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw_u64(seed, game, move, site, idx):
    """agz_draw_u64 (include/agz_draws.h)"""
    h = _mix64((seed + 0x9E3779B97F4A7C15) & _M64)
    h = _mix64(h ^ ((game + 0xD1B54A32D192ED03) & _M64))
    h = _mix64(h ^ (((move << 8) | site) & _M64))
    return _mix64(h ^ ((idx + 0x8CB92BA72F3D8DD7) & _M64))


def draw_symmetry(seed, game_id, e):
    """the s of network evaluation e (0-based) of game `game_id` under AGZ_SYMMETRY_RANDOM"""
    return ((draw_u64(seed, game_id, 0, SITE_SYMMETRY, e) >> 32) * 8) >> 32


def mode_of(symmetry):
    """None | "random" | int 0..7 -> the agz_selfplay_set_symmetry mode"""
    if symmetry is None:
        return NONE
    if isinstance(symmetry, str):
        if symmetry.lower() != "random":
            raise ValueError(f"symmetry {symmetry!r}: None, 'random' or 0..7")
        return RANDOM
    s = int(symmetry)
    if not 0 <= s < 8:
        raise ValueError(f"symmetry {symmetry!r}: None, 'random' or 0..7")
    return s
