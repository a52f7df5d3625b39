"""Board symmetries (DESIGN.md "Board symmetries"), CPU side: the Python maps form the dihedral group D4, agree with the
C++ helper every kernel uses (csrc/agz_layout.h), commute with the feature planes of the oracle, and the draw key has a
mirror; the library exports the new entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alphago_jl_amd as ag
import orc
from alphago_jl_amd import symmetry as sy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (5, 9, 19)


def _compose(a, b, N):
    """the index c with T_c = T_a after T_b"""
    ta, tb = sy.transform_points(a, N), sy.transform_points(b, N)
    both = ta[tb]
    hits = [c for c in range(8) if (sy.transform_points(c, N) == both).all()]
    assert len(hits) == 1
    return hits[0]


@pytest.mark.parametrize("N", SIZES)
def test_eight_distinct_permutations_pass_fixed(N):
    perms = [sy.transform_points(s, N) for s in range(8)]
    A = N * N + 1
    for t in perms:
        assert sorted(t.tolist()) == list(range(A))      # a permutation of the actions
        assert t[N * N] == N * N                           # pass maps to pass
    assert len({tuple(t) for t in perms}) == 8
    assert (perms[0] == np.arange(A)).all()


@pytest.mark.parametrize("N", SIZES)
def test_group_closure_and_inverse(N):
    ident = np.arange(N * N + 1)
    for a in range(8):
        for b in range(8):
            _compose(a, b, N)                              # closed: the composite is one of the eight
        ia = sy.inverse(a)
        assert (sy.transform_points(a, N)[sy.transform_points(ia, N)] == ident).all()
        assert (sy.transform_points(ia, N)[sy.transform_points(a, N)] == ident).all()
    # the two quarter turns are each other's inverse, not their own
    assert sy.inverse(5) == 6 and sy.inverse(6) == 5
    assert not (sy.transform_points(5, N)[sy.transform_points(5, N)] == ident).all()


@pytest.mark.parametrize("N", SIZES)
def test_policy_round_trip(N):
    rng = np.random.RandomState(N)
    pi = rng.rand(3, N * N + 1).astype(np.float32)
    for s in range(8):
        t = sy.apply_policy(pi, s, N)
        assert (t[:, N * N] == pi[:, N * N]).all()
        assert (sy.apply_policy(t, sy.inverse(s), N) == pi).all()


def test_cpp_helper_matches_python(tmp_path):
    """sym_point / sym_inverse of csrc/agz_layout.h (compiled by the host compiler) == transform_points / inverse"""
    src = tmp_path / "sym.cpp"
    src.write_text('#include "agz_layout.h"\n#include <cstdio>\n#include <initializer_list>\nint main() {\n'
                   '  for (int N : {5, 9, 19}) for (int s = 0; s < 8; ++s) {\n'
                   '    std::printf("%d %d %d", N, s, agz::sym_inverse(s));\n'
                   '    for (int p = 0; p <= N * N; ++p) std::printf(" %d", agz::sym_point(s, N, p));\n'
                   '    std::printf("\\n");\n  }\n}\n')
    exe = tmp_path / "sym"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "alphago.jl_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == 3 * 8
    for line in lines:
        v = [int(x) for x in line.split()]
        N, s, inv = v[:3]
        assert inv == sy.inverse(s)
        assert v[3:] == sy.transform_points(s, N).tolist()


@pytest.mark.parametrize("N", (5, 9))
def test_features_commute_with_the_transform(N):
    """get_feats of the transformed game == the transformed get_feats: playing T_s of every move from the empty board
    gives the transformed position (the rules are symmetric), history planes and captures included"""
    rng = np.random.RandomState(N)
    P = N * N
    moves, pos = [], orc.make_pos(N)
    while len(moves) < 3 * N:
        legal = np.nonzero(orc.legal_moves(pos)[:P])[0]
        a = int(rng.choice(legal))
        rc, pos = orc.play(pos, a)
        assert rc == 0
        moves.append(a)
    base = orc.feats(pos)
    assert base.shape == (17, P)
    for s in range(8):
        t = sy.transform_points(s, N)
        tpos = orc.make_pos(N)
        for a in moves:
            rc, tpos = orc.play(tpos, int(t[a]))
            assert rc == 0
        got = orc.feats(tpos)
        want = sy.apply_features(base.reshape(-1), s, N).reshape(17, P)
        assert (got == want).all(), s


def test_draw_mirror_matches_the_shared_header():
    L = orc.lib()
    L.or_draw_u64.restype = C.c_uint64
    L.or_draw_u64.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64]
    L.or_draw_index.restype = C.c_uint32
    L.or_draw_index.argtypes = [C.c_uint64, C.c_uint32]
    for seed, game, e in ((0, 0, 0), (1, 7, 3), (2**63 + 5, 2**40 + 1, 999), (12345, 3, 2**33)):
        d = L.or_draw_u64(seed, game, 0, sy.SITE_SYMMETRY, e)
        assert sy.draw_u64(seed, game, 0, sy.SITE_SYMMETRY, e) == d
        assert sy.draw_symmetry(seed, game, e) == L.or_draw_index(d, 8)
    hdr = open(os.path.join(ROOT, "include", "agz_draws.h")).read()
    assert re.search(r"#define AGZ_SITE_SYMMETRY 8u", hdr)
    counts = np.bincount([sy.draw_symmetry(1, g, e) for g in range(64) for e in range(128)], minlength=8)
    assert (np.abs(counts / counts.sum() - 1 / 8) < 0.01).all()


def test_mode_parsing():
    assert sy.mode_of(None) == -1 and sy.mode_of("random") == 8 and sy.mode_of(3) == 3
    for bad in (8, -1, "avg", 9):
        with pytest.raises(ValueError):
            sy.mode_of(bad)


def test_library_exports_the_symmetry_entry_points():
    L = ag.load()
    for name in ("agz_selfplay_set_symmetry", "agz_net_forward_features_sym", "agz_replay_batch_sym"):
        assert hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "agz.h")).read()
    assert "#define AGZ_SYMMETRY_NONE (-1)" in hdr and "#define AGZ_SYMMETRY_RANDOM 8" in hdr
