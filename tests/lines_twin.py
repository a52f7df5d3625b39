"""The twin of the analysis-lines walk (include/agz.h "analysis lines"): a plain numpy walk over node
rows read through interfaces that exist without the feature (hs_node_row / hs_node_children on the host simulator,
Engine.node_floats / node_children on the device).  It shares no code with the wave templates of agz_search.h; the
tests compare its output with theirs exactly (moves, lengths, the bits of every float)."""
import numpy as np


def walk(row, children, X, K, D, min_visits):
    """row(node, field) -> float32 [A] (field 0 child_N, 1 child_W, 2 child_prior), children(node) -> int32 [A].
    Returns the tables node_lines writes: dict of move, pv_len int32 [K]; N, W, prior, end_W float32 [K]; pv int16
    [K][D] (-1 beyond pv_len); pv_N float32 [K][D] (0 beyond pv_len)."""
    N, W, Pr = (np.array(row(X, f), np.float32) for f in (0, 1, 2))
    ch = np.array(children(X), np.int32)
    A = len(N)
    cand = [a for a in range(A) if N[a] > 0]
    cand.sort(key=lambda a: (-float(N[a]), -float(Pr[a]), a))        # float32 -> float is exact, so is the order
    out = dict(move=np.full(K, -1, np.int32), pv_len=np.zeros(K, np.int32), N=np.zeros(K, np.float32),
               W=np.zeros(K, np.float32), prior=np.zeros(K, np.float32), end_W=np.zeros(K, np.float32),
               pv=np.full((K, D), -1, np.int16), pv_N=np.zeros((K, D), np.float32))
    for k, a in enumerate(cand[:K]):
        pv, pvn, end_w, c = [a], [N[a]], W[a], int(ch[a])
        while len(pv) < D and c >= 0:
            cn = np.array(row(c, 0), np.float32)
            m = cn.max()
            if m < np.float32(min_visits):
                break
            b = int(np.flatnonzero(cn == m)[0])                        # findmax: the lowest index, no draw
            pv.append(b)
            pvn.append(cn[b])
            end_w = np.array(row(c, 1), np.float32)[b]
            c = int(np.array(children(c), np.int32)[b])
        out["move"][k], out["pv_len"][k] = a, len(pv)
        out["N"][k], out["W"][k], out["prior"][k], out["end_W"][k] = N[a], W[a], Pr[a], end_w
        out["pv"][k, :len(pv)] = pv
        out["pv_N"][k, :len(pv)] = pvn
    return out


FIELDS = ("move", "pv_len", "N", "W", "prior", "end_W", "pv", "pv_N")


def same(a, b):
    """exact equality of two line tables: integers by value, floats by their bits; returns the first field that
    differs (None when equal)"""
    for f in FIELDS:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return f
    return None
