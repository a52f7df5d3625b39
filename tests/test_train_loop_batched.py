"""Batched train(), CPU side: the draw agz_replay_sample makes, as a host twin compiled from
include/agz_draws.h (Floyd's algorithm, one step after the other), is B distinct entries of the window for every window
shape; a second, pure-Python twin agrees with it; the library and the package export the new entry points."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import alphago_jl_amd as ag
from alphago_jl_amd import symmetry as sy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SITE_REPLAY_SAMPLE, SITE_REPLAY_SYM = 9, 10

_TWIN = r"""
#include <stdint.h>
#include <stdlib.h>
#include "agz_draws.h"
/* agz_replay_sample's draw, sequentially: out[b] = entry of the window [0, L) taken by Floyd's step b */
int twin_sample(uint64_t seed, uint64_t call, int64_t L, int32_t B, int64_t* out) {
  if (B < 1 || B > L) return 1;
  char* taken = (char*)calloc((size_t)L, 1);
  for (int32_t b = 0; b < B; ++b) {
    const uint64_t j = (uint64_t)(L - B + b);
    const int64_t t = (int64_t)agz_index(agz_draw_u64(seed, call, 0, AGZ_SITE_REPLAY_SAMPLE, j), (uint32_t)(j + 1));
    out[b] = taken[t] ? (int64_t)j : t;
    taken[out[b]] = 1;
  }
  free(taken);
  return 0;
}
int32_t twin_sym(uint64_t seed, uint64_t call, int32_t b) {
  return (int32_t)agz_index(agz_draw_u64(seed, call, 0, AGZ_SITE_REPLAY_SYM, (uint64_t)b), 8u);
}
"""
_twin_lib = None


def twin():
    """the host twin of the draw (compiled once per session into a scratch directory of the build)"""
    global _twin_lib
    if _twin_lib is None:
        import tempfile
        d = tempfile.mkdtemp(prefix="agz_twin_")
        src, so = os.path.join(d, "twin.c"), os.path.join(d, "libtwin.so")
        open(src, "w").write(_TWIN)
        subprocess.run(["gcc", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src, "-o", so], check=True)
        lib = C.CDLL(so)
        lib.twin_sample.restype = C.c_int
        lib.twin_sample.argtypes = [C.c_uint64, C.c_uint64, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        lib.twin_sym.restype = C.c_int32
        lib.twin_sym.argtypes = [C.c_uint64, C.c_uint64, C.c_int32]
        _twin_lib = lib
    return _twin_lib


def sample_entries(seed, call, L, B):
    """window entries 0..L-1 drawn for samples b = 0..B-1"""
    out = np.zeros(B, np.int64)
    assert twin().twin_sample(seed, call, L, B, out.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    return out


def sample_syms(seed, call, B):
    return np.array([twin().twin_sym(seed, call, b) for b in range(B)], np.int32)


def window_pairs(lengths, first_game, first_ply, entries):
    """window entry e -> (arena game, ply): the entries are the plies from (first_game, first_ply) on, game after game"""
    cum = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    a = cum[first_game] + first_ply + np.asarray(entries, np.int64)
    g = np.searchsorted(cum, a, side="right") - 1
    return g.astype(np.int64), (a - cum[g]).astype(np.int32)


def window_of(lengths, max_entries):
    """(first_game, first_ply, live) of the newest max_entries entries (shrink, train.jl:52)"""
    total = int(sum(lengths))
    first = max(0, total - max_entries)
    k = 0
    while k < len(lengths) and sum(lengths[:k + 1]) <= first:
        k += 1
    return k, first - int(sum(lengths[:k])), total - first


def _py_floyd(seed, call, L, B):
    out, taken = [], set()
    for b in range(B):
        j = L - B + b
        t = ((sy.draw_u64(seed, call, 0, SITE_REPLAY_SAMPLE, j) >> 32) * (j + 1)) >> 32      # agz_index
        v = j if t in taken else t
        taken.add(v)
        out.append(v)
    return out


def test_twin_matches_a_python_floyd_and_the_index_rule():
    for seed, call, L, B in ((0, 1, 10, 3), (7, 12, 500, 32), (2**63 + 1, 5, 33, 33), (3, 2**40, 100000, 256)):
        assert sample_entries(seed, call, L, B).tolist() == _py_floyd(seed, call, L, B)
    for seed, call in ((0, 0), (5, 77)):
        want = [int(((sy.draw_u64(seed, call, 0, SITE_REPLAY_SYM, b) >> 32) * 8) >> 32) for b in range(64)]
        assert sample_syms(seed, call, 64).tolist() == want


def test_index_rule_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "agz_draws.h")).read()
    body = re.search(r"agz_index\(uint64_t bits, uint32_t n\) \{(.*?)\n\}", hdr, flags=re.S).group(1)
    assert "(((bits >> 32) * (uint64_t)n) >> 32)" in body
    assert re.search(r"#define AGZ_SITE_REPLAY_SAMPLE 9u", hdr) and re.search(r"#define AGZ_SITE_REPLAY_SYM 10u", hdr)
    # the sites stay distinct
    sites = [int(v) for v in re.findall(r"#define AGZ_SITE_\w+ (\d+)u", hdr)]
    assert len(sites) == len(set(sites))


# (arena game lengths, memory_size, B): one game; the oldest game cut partway; B = window size; many games
SHAPES = [((23,), 100, 8), ((23,), 23, 23), ((12, 17, 9), 30, 16), ((12, 17, 9), 30, 30), ((5, 5, 5, 5), 7, 7),
          (tuple(range(20, 84)), 1000, 256), ((40, 1, 40), 41, 41)]


@pytest.mark.parametrize("lengths,memory,B", SHAPES)
def test_draw_gives_distinct_live_entries(lengths, memory, B):
    fg, fp, live = window_of(list(lengths), memory)
    assert live == min(memory, sum(lengths))
    for call in (1, 2, 99):
        e = sample_entries(11, call, live, B)
        assert len(set(e.tolist())) == B and e.min() >= 0 and e.max() < live
        if B == live:
            assert sorted(e.tolist()) == list(range(live))      # the whole window, once each
        g, p = window_pairs(lengths, fg, fp, e)
        assert ((g >= fg) & (g < len(lengths))).all()
        assert (p >= 0).all() and (p < np.asarray(lengths)[g]).all()
        assert ((g > fg) | (p >= fp)).all()                      # nothing before the window's first live ply
        assert len(set(zip(g.tolist(), p.tolist()))) == B


def test_partly_cut_game_keeps_exactly_its_newest_plies():
    lengths = [12, 17, 9]
    fg, fp, live = window_of(lengths, 30)
    assert (fg, fp, live) == (0, 8, 30)                          # 38 entries, the oldest 8 gone: game 0 keeps plies 8..11
    g, p = window_pairs(lengths, fg, fp, np.arange(live))
    assert list(zip(g.tolist(), p.tolist()))[:5] == [(0, 8), (0, 9), (0, 10), (0, 11), (1, 0)]


def test_draws_are_roughly_uniform():
    L, B = 50, 10
    hits = np.zeros(L)
    for call in range(2000):
        hits[sample_entries(3, call, L, B)] += 1
    assert np.abs(hits / hits.sum() - 1 / L).max() < 0.006


def test_library_and_package_export_the_train_surface():
    L = ag.load()
    for name in ("agz_replay_sample", "agz_selfplay_release", "agz_selfplay_set_hold", "agz_replay_set_window",
                 "agz_replay_live_positions", "agz_replay_ingest_records"):
        assert hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "agz.h")).read()
    for name in ("agz_replay_sample", "agz_selfplay_release", "agz_replay_set_window"):
        assert name + "(" in hdr
    from alphago_jl_amd import train
    sig = inspect.signature(train)
    want = dict(num_games=25000, memory_size=500000, batch_size=32, epochs=1, ckp_freq=1000, readouts=800,
                tower_height=19, model=None, start_training_after=50000)                 # train.jl:38-40
    for k, v in want.items():
        assert sig.parameters[k].default == v, k
    for k in ("slots", "seed", "game_id_base", "symmetry", "augment", "precision", "checkpoint_dir", "callback"):
        assert k in sig.parameters, k


def test_julia_stub_has_train():
    jl = open(os.path.join(ROOT, "alphago.jl_amd", "julia", "AlphaGoMI.jl")).read()
    assert re.search(r"^function train\(env::GoEnv;", jl, flags=re.M)
    for name in (":agz_replay_sample", ":agz_selfplay_release", ":agz_selfplay_set_hold", ":agz_replay_set_window",
                 ":agz_replay_ingest_records"):
        assert name in jl, name


def test_calls_without_an_engine_are_refused():
    L = ag.load()
    assert L.agz_replay_sample(None, 4, 0, -1, None, None, None, None, None) == ag._lib.BAD_ARGUMENT
    assert L.agz_selfplay_release(None) == ag._lib.BAD_ARGUMENT
    assert L.agz_replay_live_positions(None) == -1
