// agz_search.h -- Go rules, PUCT search, virtual loss, backup, noise and the per-move phase of
// the self-play hot path, written ONCE as wave-level templates.
//
// One 64-lane wavefront owns one game tree (DESIGN.md "Search kernels").  The template
// parameter W supplies the wave primitives:
//   * agz::HipWave  (agz_engine.hip)   -- the product: lanes = threadIdx, LDS scratch, DPP/shuffle
//                                         reductions, LDS atomics.  This is what runs on gfx950.
//   * a host wave simulator (tests/hostsim) -- TEST INFRASTRUCTURE that executes the same source
//     lane-serially on the CPU so that tree/rules logic can be diffed against the oracle in
//     this GPU-less container.  It is never linked into libagz.so.
//
// Discipline that makes the two agree: data-parallel work goes through w.for_each (pure per-index
// bodies), every cross-lane flow through memory is separated by w.sync(), per-lane partials are
// combined with w.reduce_*, and all other control flow is wave-uniform.  The descent keeps rows in registers across the
// W::kLanes lanes (64; the simulator is a wave of one) and reads single elements by shuffle: both run that one form.
//
// Reference semantics restated here (file:line under /root/reference):
//   select_leaf mcts.jl:108-138 | maybe_add_child! :140-147 | virtual loss :149-171 |
//   revert_visits! :173-186 | incorporate_results! :188-213 | backup_value! :215-225 |
//   inject_noise! :233-239 | children_as_pi :241-252 | PUCT :84-92
//   tree_search! mcts_play.jl:73-98 | pick_move :52-71 | play_move! :26-50 | should_resign :124
//   selfplay loop selfplay.jl:1-45
//   play_move! board.jl:451-509 | pass_move! :426-440 | all_legal_moves :393-424 |
//   is_move_suicidal :354-374 | is_koish :47-56 | score :511-533
// Float types follow the reference exactly: Float32 statistics, Float64 c_puct
// and action score, Float32 values; this header must be compiled with FP contraction off.
#pragma once
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/agz_draws.h"
#include "../../include/agz_explore.h"
#include "../../include/agz_superko.h"
#include "../../include/agz_uncertainty.h"
#include "agz_state.h"

#if defined(__HIPCC__)
#define AGZ_FN __host__ __device__ __forceinline__
#else
#define AGZ_FN inline
#endif

// k_pre phase clocks (timing builds only; see CT_T_* in agz_state.h)
#ifdef AGZ_TIMING_EXPERIMENTS
#define AGZ_STAMP_BEGIN(w) unsigned long long agz_t_prev = (w).clock()
#define AGZ_STAMP_BEGIN_AGAIN(w) agz_t_prev = (w).clock()
#define AGZ_STAMP_TO(w, V, slot, t)                             \
  do {                                                          \
    const unsigned long long agz_t_now = (w).clock();           \
    (w).count(&(V).counters[slot], agz_t_now - (t));             \
    (t) = agz_t_now;                                            \
  } while (0)
#define AGZ_STAMP(w, V, slot) AGZ_STAMP_TO(w, V, slot, agz_t_prev)
#define AGZ_STAMP_AT(w, V, slot, clk) do { if (clk) AGZ_STAMP_TO(w, V, slot, *(clk)); } while (0)   // a caller's clock, if any
#else
#define AGZ_STAMP_BEGIN(w) unsigned long long agz_t_prev = 0
#define AGZ_STAMP_BEGIN_AGAIN(w) (void)agz_t_prev
#define AGZ_STAMP(w, V, slot) (void)agz_t_prev
#define AGZ_STAMP_AT(w, V, slot, clk) (void)(clk)
#endif


#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace agz {

// the largest board the scratch is sized for (19x19): bounds on View::PP, AP and maxd
constexpr int kPPMax = 368, kAPMax = 368, kMaxdMax = 528;

// The widths R (row elements per lane of a 64-lane wave) that the register-row templates -- the descent and the lines
// walk -- are instantiated at; f gets R as a std::integral_constant.  A row of n elements with no width of its own (4 or
// 5 per lane, N = 14..17) takes the next one up: the templates mask what lies past the row's end.
template <class F>
AGZ_FN auto with_row_width(int n, F f) {
  static_assert(6 * kWave >= kAPMax, "the widest instantiation covers the largest row");
  switch ((n + kWave - 1) / kWave) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});     // 9x9
    case 3: return f(std::integral_constant<int, 3>{});     // 13x13
    default: return f(std::integral_constant<int, 6>{});    // 19x19, and N = 14..17 rounded up
  }
}

// The width of a wave type: W::kLanes lanes (HipWave: 64; the host simulator: 1).  A wave type that states none is taken
// as lane-serial, a wave of one lane.  That one lane is lane 0 and holds whole rows, so it reads an element out of its
// own registers and is asked for neither w.lane nor w.shfl: wave_lane and wave_shfl are those two for any wave.
template <class W, class = void>
struct wave_lanes : std::integral_constant<int, 1> {};
template <class W>
struct wave_lanes<W, std::void_t<decltype(W::kLanes)>> : std::integral_constant<int, W::kLanes> {};
template <class W>
AGZ_FN int wave_lane(const W& w) {
  if constexpr (wave_lanes<W>::value > 1) return w.lane; else return 0;
}
template <class W, class T>
AGZ_FN T wave_shfl(const W& w, T v, int src) {
  if constexpr (wave_lanes<W>::value > 1) return w.shfl(v, src); else return v;
}

struct Scratch {
  int8_t* sb;        // [PP] working board
  int32_t* label;    // [PP]
  int32_t* minlib;   // [PP]
  int32_t* maxlib;   // [PP]
  int8_t* flag;      // [AP]
  double* dbuf;      // [AP]
  int32_t* path;     // [maxd]
  // superko (View::sk_key): [AP] keys -- a stone group's at its label, a candidate move's child key at its empty point --
  // then one chunk of kSkChunk seen keys.  Last, so that an initialiser of the seven above leaves it null: a lane-serial
  // wave then works in a buffer of its own (sk_keybuf)
  uint64_t* key;     // [AP + kSkChunk]
};
constexpr int kSkChunk = 64;

// The 64-bit wave operations of the superko filter, for any wave: the XOR of v over the lanes (a butterfly of shuffles; a
// wave of one lane has folded its whole range into v already) and an XOR into a cell that several lanes may hit (the LDS
// atomic; one lane alone has no one to race with).
template <class W>
AGZ_FN uint64_t wave_xor64(const W& w, uint64_t v) {
  if constexpr (wave_lanes<W>::value > 1) {
    int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    for (int o = wave_lanes<W>::value / 2; o > 0; o >>= 1) {
      lo ^= w.shfl(lo, w.lane ^ o);
      hi ^= w.shfl(hi, w.lane ^ o);
    }
    return ((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo;
  } else {
    return v;
  }
}
template <class W>
AGZ_FN void wave_axor64(const W& w, uint64_t* p, uint64_t v) {
  if constexpr (wave_lanes<W>::value > 1) w.axor64(p, v); else *p ^= v;
}
template <class W>
AGZ_FN uint64_t* sk_keybuf(const W& w, const Scratch& S) {
#if !defined(__HIPCC__)
  if constexpr (wave_lanes<W>::value == 1) {
    static thread_local uint64_t buf[kAPMax + kSkChunk];
    return S.key ? S.key : buf;
  }
#endif
  return S.key;
}

constexpr int kIntMax = 0x7fffffff;

// ------------------------------------------------------------------ small helpers

template <class W>
AGZ_FN int nbrs(int N, int p, int out[4]) {
  const int i = p % N, j = p / N;
  int k = 0;
  if (i + 1 < N) out[k++] = p + 1;
  if (i - 1 >= 0) out[k++] = p - 1;
  if (j + 1 < N) out[k++] = p + N;
  if (j - 1 >= 0) out[k++] = p - N;
  return k;
}

AGZ_FN long node_index(const View& V, int g, int node) { return (long)g * V.cap + node; }

AGZ_FN bool legal_bit(const View& V, long ni, int a) {
  return (V.legal[ni * V.LW + (a >> 5)] >> (a & 31)) & 1u;
}

// N(x) / W(x): a node's own statistics live in its parent's child rows (mcts.jl:96-102); the
// root's live in the game record (the DummyNode of mcts.jl:27-39).
AGZ_FN float* slotN(const View& V, int g, int node) {
  const NodeMeta& m = V.meta[node_index(V, g, node)];
  return m.parent < 0 ? &V.gs[g].rootN : &V.childN[node_index(V, g, m.parent) * V.AP + m.fmove];
}
AGZ_FN float* slotW(const View& V, int g, int node) {
  const NodeMeta& m = V.meta[node_index(V, g, node)];
  return m.parent < 0 ? &V.gs[g].rootW : &V.childW[node_index(V, g, m.parent) * V.AP + m.fmove];
}

// S(x), the sum of squared values beside W(x) (View::childS / rootS, agz_search_set_value_moments): only with moments on
AGZ_FN float* slotS(const View& V, int g, int node) {
  const NodeMeta& m = V.meta[node_index(V, g, node)];
  return m.parent < 0 ? &V.rootS[g] : &V.childS[node_index(V, g, m.parent) * V.AP + m.fmove];
}

AGZ_FN bool node_is_done(const View& V, int g, int node) {
  const NodeMeta& m = V.meta[node_index(V, g, node)];
  return (m.flags & NF_DONE) || m.n >= V.max_game_length;   // mcts.jl:230-231
}

// ------------------------------------------------------------------ rules on a board in scratch

// Connected components by min-label propagation with pointer jumping.  stones=true labels
// stone groups, stones=false labels empty regions.  The fixed point (label = smallest point
// of the component) does not depend on the order in which lanes update.
template <class W>
AGZ_FN void label_components(W& w, const View& V, Scratch& S, bool stones) {
  const int P = V.P, N = V.N;
  w.for_each(P, [&](int p) {
    const bool in = stones ? (S.sb[p] != 0) : (S.sb[p] == 0);
    S.label[p] = in ? p : -1;
    S.minlib[p] = kIntMax;
    S.maxlib[p] = -1;
  });
  w.sync();
  for (int iter = 0; iter < 4 * P; ++iter) {
    bool changed = false;
    w.for_each(P, [&](int p) {
      const int l = S.label[p];
      if (l < 0) return;
      const int c = S.sb[p];
      int m = l, nb[4];
      const int k = nbrs<W>(N, p, nb);
      for (int t = 0; t < k; ++t)
        if (S.sb[nb[t]] == c) { const int lq = S.label[nb[t]]; m = lq < m ? lq : m; }
      const int lm = S.label[m];
      m = lm < m ? lm : m;
      if (m < l) { S.label[p] = m; changed = true; }
    });
    changed = w.any(changed);
    w.sync();
    if (!changed) break;
  }
}

// distinct-liberty summary per stone group: minlib/maxlib over the group's empty neighbours.
//   none  <=> maxlib < 0 ; exactly one <=> minlib == maxlib ; two or more <=> minlib < maxlib
template <class W>
AGZ_FN void group_liberties(W& w, const View& V, Scratch& S) {
  const int P = V.P, N = V.N;
  w.for_each(P, [&](int e) {
    if (S.sb[e] != 0) return;
    int nb[4];
    const int k = nbrs<W>(N, e, nb);
    for (int t = 0; t < k; ++t)
      if (S.sb[nb[t]] != 0) {
        const int gl = S.label[nb[t]];
        w.amin(&S.minlib[gl], e);
        w.amax(&S.maxlib[gl], e);
      }
  });
  w.sync();
}

// all_legal_moves (board.jl:393-424) for the side `tp` into S.flag[0..AP).
// An empty, non-ko point is legal iff it has an empty neighbour, or joins a friendly group that
// keeps another liberty, or captures an enemy group in atari (is_move_suicidal :354-374).
// Needs label_components(stones) + group_liberties on the board in S.sb.
template <class W>
AGZ_FN void compute_legal_flags(W& w, const View& V, Scratch& S, int tp, int ko) {
  const int P = V.P, N = V.N, A = V.A;
  w.for_each(V.AP, [&](int a) {
    bool ok = false;
    if (a == P) ok = true;
    else if (a < P && S.sb[a] == 0 && a != ko) {
      int nb[4];
      const int k = nbrs<W>(N, a, nb);
      for (int t = 0; t < k; ++t) {
        const int c = S.sb[nb[t]];
        if (c == 0) { ok = true; continue; }
        const int gl = S.label[nb[t]];
        if (c == tp) { if (S.minlib[gl] < S.maxlib[gl]) ok = true; }
        else if (S.minlib[gl] == S.maxlib[gl]) ok = true;
      }
    }
    S.flag[a] = ok && a < A;
  });
  w.sync();
}

// ---- superko (include/agz_superko.h): the filter behind compute_legal_flags

// the key under `rule` of board b [P] with tp to move
template <class W>
AGZ_FN uint64_t board_key(W& w, const View& V, const int8_t* b, int tp, int rule) {
  uint64_t k = 0;
  w.for_each(V.P, [&](int p) { const int c = b[p]; if (c != 0) k ^= agz_zobrist(p, c); });
  return wave_xor64(w, k) ^ agz_ko_side_key(tp, rule);
}

// K[a] := the key of the position after move a, for every flagged board move a of the side tp on the board in S.sb
// (labels, liberties and flags current), node_key being the board's own key under `rule`.  The stone groups' keys are
// built in K at the groups' labels first: a label is a stone and a candidate an empty point, so the two never share a cell.
template <class W>
AGZ_FN void sk_child_keys(W& w, const View& V, Scratch& S, uint64_t* K, int tp, int rule, uint64_t node_key) {
  const int P = V.P, N = V.N;
  w.for_each(V.AP, [&](int a) { K[a] = 0; });
  w.sync();
  w.for_each(P, [&](int p) {
    const int c = S.sb[p];
    if (c != 0) wave_axor64(w, &K[S.label[p]], agz_zobrist(p, c));
  });
  w.sync();
  const uint64_t flip = rule == AGZ_KO_SITUATIONAL ? AGZ_ZOBRIST_WHITE_TO_PLAY : 0ull;   // the side to move changes
  w.for_each(P, [&](int a) {
    if (!S.flag[a]) return;
    uint64_t k = node_key ^ agz_zobrist(a, tp) ^ flip;
    int nb[4], dead[4];
    const int n = nbrs<W>(N, a, nb);
    for (int t = 0; t < n; ++t) {
      dead[t] = -1;
      if (S.sb[nb[t]] != -tp) continue;
      const int gl = S.label[nb[t]];
      if (S.minlib[gl] != a || S.maxlib[gl] != a) continue;
      bool dup = false;
      for (int u = 0; u < t; ++u) dup = dup || dead[u] == gl;
      if (dup) continue;
      dead[t] = gl;
      k ^= K[gl];
    }
    K[a] = k;
  });
  w.sync();
}

// clear the flag of every board move whose child key is one of seen[0 .. cnt); returns this lane's count of them
template <class W>
AGZ_FN int sk_strike(W& w, const View& V, Scratch& S, const uint64_t* K, const uint64_t* seen, int cnt) {
  int struck = 0;
  w.sync();
  w.for_each(V.P, [&](int a) {
    if (!S.flag[a]) return;
    const uint64_t k = K[a];
    bool hit = false;
    for (int i = 0; i < cnt; ++i) hit = hit || seen[i] == k;
    if (hit) { S.flag[a] = 0; struck++; }
  });
  w.sync();
  return struck;
}

// The filter of a tree node: `key` is node id's own key, its seen set the keys of the node, of its ancestors (from
// `parent` up) and of the slot's log.  Counts the node and its removed moves.
template <class W>
AGZ_FN void superko_filter_node(W& w, const View& V, Scratch& S, int g, int parent, int tp, uint64_t key) {
  uint64_t* K = sk_keybuf(w, S);
  uint64_t* seen = K + V.AP;
  sk_child_keys(w, V, S, K, tp, V.ko_rule, key);
  int struck = 0, c = 1;
  if (w.leader()) seen[0] = key;
  for (int n = parent; n >= 0;) {
    const long ni = node_index(V, g, n);
    if (w.leader()) seen[c] = V.sk_key[ni];
    n = V.meta[ni].parent;
    if (++c == kSkChunk) { struck += sk_strike(w, V, S, K, seen, c); c = 0; }
  }
  const int len = V.sk_len[g];
  const uint64_t* log = V.sk_log + (long)g * sk_log_stride(V);
  for (int at = 0; c > 0 || at < len;) {
    const int take = kSkChunk - c < len - at ? kSkChunk - c : len - at;
    w.for_each(take, [&](int i) { seen[c + i] = log[at + i]; });
    c += take;
    at += take;
    struck += sk_strike(w, V, S, K, seen, c);
    c = 0;
  }
  struck = w.reduce_sum(struck);
  if (struck > 0) {
    w.count(&V.counters[CT_SK_NODES], 1);
    w.count(&V.counters[CT_SK_MOVES], (unsigned long long)struck);
  }
}

// S.flag -> the packed mask words of node index ni
template <class W>
AGZ_FN void pack_legal_mask(W& w, const View& V, Scratch& S, long ni) {
  const int A = V.A;
  w.for_each(V.LW, [&](int wi) {
    uint32_t bits = 0;
    for (int b = 0; b < 32; ++b) {
      const int a = wi * 32 + b;
      if (a < A && S.flag[a]) bits |= 1u << b;
    }
    V.legal[ni * V.LW + wi] = bits;
  });
  w.sync();
}

// Place a stone of `color` at point a on the board in S.sb (labels + liberties of the PRE-move
// board must be current): removes the enemy groups whose only liberty was a (add_stone!
// board.jl:251-259) and reports the capture count and the ko point (board.jl:472,483-487).
template <class W>
AGZ_FN void apply_move_in_scratch(W& w, const View& V, Scratch& S, int a, int color, int* ncap_out, int* ko_out) {
  const int P = V.P, N = V.N;
  int nb[4];
  const int k = nbrs<W>(N, a, nb);
  // is_koish on the pre-move board (board.jl:47-56)
  int koish = S.sb[nb[0]];
  for (int t = 1; t < k; ++t)
    if (S.sb[nb[t]] != koish) koish = 0;
  int dead[4];
  for (int t = 0; t < 4; ++t) dead[t] = -1;
  for (int t = 0; t < k; ++t)
    if (S.sb[nb[t]] == -color) {
      const int gl = S.label[nb[t]];
      if (S.minlib[gl] == a && S.maxlib[gl] == a) dead[t] = gl;
    }
  w.sync();
  int ncap = 0, lastcap = -1;
  w.for_each(P, [&](int p) {
    if (S.sb[p] != -color) return;
    const int gl = S.label[p];
    if (gl == dead[0] || gl == dead[1] || gl == dead[2] || gl == dead[3]) {
      S.sb[p] = 0;
      ncap += 1;
      lastcap = p > lastcap ? p : lastcap;
    }
  });
  ncap = w.reduce_sum(ncap);
  lastcap = w.reduce_max(lastcap);
  if (w.leader()) S.sb[a] = (int8_t)color;
  w.sync();
  *ncap_out = ncap;
  *ko_out = (ncap == 1 && koish == -color) ? lastcap : -1;
}

// Tromp-Taylor area score minus komi (board.jl:511-533), Black-positive.
template <class W>
AGZ_FN float area_score(W& w, const View& V, Scratch& S, float komi) {
  const int P = V.P, N = V.N;
  label_components(w, V, S, false);
  // minlib doubles as the "touches" bitmask per empty region (1 = black border, 2 = white)
  w.for_each(P, [&](int p) { S.maxlib[p] = 0; });
  w.sync();
  w.for_each(P, [&](int e) {
    if (S.sb[e] != 0) return;
    int nb[4];
    const int k = nbrs<W>(N, e, nb);
    int bits = 0;
    for (int t = 0; t < k; ++t) {
      const int c = S.sb[nb[t]];
      if (c == 1) bits |= 1;
      if (c == -1) bits |= 2;
    }
    if (bits) w.aor(&S.maxlib[S.label[e]], bits);
  });
  w.sync();
  int diff = 0;
  w.for_each(P, [&](int p) {
    const int c = S.sb[p];
    if (c == 1) diff += 1;
    else if (c == -1) diff -= 1;
    else {
      const int t = S.maxlib[S.label[p]];
      if (t == 1) diff += 1;
      else if (t == 2) diff -= 1;
    }
  });
  diff = w.reduce_sum(diff);
  w.sync();
  return (float)diff - komi;
}

AGZ_FN int result_of(float score) { return score > 0.f ? 1 : score < 0.f ? -1 : 0; }

// ------------------------------------------------------------------ node pool

template <class W>
AGZ_FN int free_pending(W& w, const View& V, Scratch& S, int g, int budget);

template <class W>
AGZ_FN int pool_alloc(W& w, const View& V, Scratch& S, int g) {
  GameState& G = V.gs[g];
  int top = G.free_top;
  if (top <= 0 && G.garbage > 0) {      // nothing free but releases pending: do them now
    free_pending(w, V, S, g, V.cap);
    top = G.free_top;
  }
  if (top <= 0) {
    w.count(&V.counters[CT_POOL_EXHAUSTED], 1);
    if (w.leader()) G.err = AGZ_POOL_EXHAUSTED;
    w.sync();
    return -1;
  }
  const int id = V.freelist[(long)g * V.cap + top - 1];
  w.sync();
  if (w.leader()) { G.free_top = top - 1; G.nodes_used += 1; }
  w.sync();
  return id;
}

template <class W>
AGZ_FN void pool_free(W& w, const View& V, int g, int node) {
  GameState& G = V.gs[g];
  const int top = G.free_top;
  w.sync();
  if (w.leader()) {
    V.freelist[(long)g * V.cap + top] = node;
    G.free_top = top + 1;
    G.nodes_used -= 1;
  }
  w.sync();
}

// Deferred release of discarded subtrees.  play_move! drops the siblings of the chosen child
// (`root.parent.children = Dict()`, mcts_play.jl:48); walking them at once put a serial walk over
// thousands of nodes on the critical path of the ~2 % of games that move in a given step (k_pre took
// as long as its slowest wave: 2.9 ms).  Instead the detached old root is pushed on a per-game
// garbage stack -- it lives in the unused tail of the slot's free list and grows downward, while free
// entries grow upward; they cannot collide because every stacked node is an allocated node and
// #allocated + #free == cap -- and every k_pre releases at most `budget` nodes of it, children pushed
// in ascending action order (a deterministic order: node ids never depend on timing).
template <class W>
AGZ_FN int free_pending(W& w, const View& V, Scratch& S, int g, int budget) {
  GameState& G = V.gs[g];
  int32_t* fl = V.freelist + (long)g * V.cap;
  int sp = V.cap - G.garbage;
  int done = 0;
  w.sync();
  while (sp < V.cap && done < budget) {
    const int node = fl[sp];
    ++sp;
    const long ni = node_index(V, g, node);
    const bool expanded = V.meta[ni].flags & NF_EXPANDED;
    w.sync();
    if (expanded) sp = w.push_desc(V.A, [&](int a) { return V.child[ni * V.AP + a]; }, fl, sp);
    const int top = G.free_top;
    w.sync();
    if (w.leader()) { fl[top] = node; G.free_top = top + 1; G.nodes_used -= 1; V.meta[ni].flags = 0; }
    w.sync();
    ++done;
  }
  if (w.leader()) G.garbage = V.cap - sp;
  w.sync();
  return done;
}

// nodes released per step and game: a move creates <= R+7 nodes over ~R/8 steps, i.e. ~8 per step
// in steady state; 32 keeps up with 4x headroom and costs ~30 us of a wave per step
constexpr int kFreeBudget = 32;

// detach `keep` from `start` and hand `start` (with everything else below it) to the garbage stack
template <class W>
AGZ_FN void discard_except(W& w, const View& V, int g, int start, int keep_action) {
  GameState& G = V.gs[g];
  w.sync();
  if (w.leader()) {
    if (keep_action >= 0) V.child[node_index(V, g, start) * V.AP + keep_action] = -1;
    V.freelist[(long)g * V.cap + V.cap - G.garbage - 1] = start;
    G.garbage = G.garbage + 1;
  }
  w.sync();
}

// ------------------------------------------------------------------ node creation

template <class W>
AGZ_FN void load_board(W& w, const View& V, Scratch& S, long ni) {
  w.for_each(V.P, [&](int p) { S.sb[p] = V.board[ni * V.PP + p]; });
  w.sync();
}

// The Tromp-Taylor score of `node`'s board under the game's komi; result_of gives its sign (`result`, board.jl:535-545)
template <class W>
AGZ_FN float position_score(W& w, const View& V, Scratch& S, int g, int node) {
  load_board(w, V, S, node_index(V, g, node));
  return area_score(w, V, S, V.gs[g].komi);
}

// Initialise node `id` from the board currently in S.sb (rows zeroed, legal mask for `tp`).
template <class W>
AGZ_FN void node_init_from_scratch(W& w, const View& V, Scratch& S, int g, int id, const NodeMeta& m) {
  const long ni = node_index(V, g, id);
  w.for_each(V.AP, [&](int a) {
    V.childN[ni * V.AP + a] = 0.f;
    V.childW[ni * V.AP + a] = 0.f;
    V.childP[ni * V.AP + a] = 0.f;
    V.child[ni * V.AP + a] = -1;
    if (V.childS) V.childS[ni * V.AP + a] = 0.f;
  });
  w.for_each(V.P, [&](int p) { V.board[ni * V.PP + p] = S.sb[p]; });
  if (w.leader()) { V.meta[ni] = m; V.meta[ni].flags = (uint8_t)(m.flags | NF_ALLOC); }
  label_components(w, V, S, true);
  group_liberties(w, V, S);
  compute_legal_flags(w, V, S, m.to_play, m.ko);
  if (V.sk_key) {      // a superko rule is in force (wave-uniform)
    const uint64_t key = board_key(w, V, S.sb, m.to_play, V.ko_rule);
    if (w.leader()) V.sk_key[ni] = key;
    superko_filter_node(w, V, S, g, m.parent, m.to_play, key);
  }
  pack_legal_mask(w, V, S, ni);
}

// The board half of node_create_child: play the node's move (meta.fmove) on its parent's board in scratch and
// initialise the node's rows, board and legal mask from the result (board.jl:451-509 / pass_move! :426-440).
template <class W>
AGZ_FN void node_expand_child(W& w, const View& V, Scratch& S, int g, int id) {
  const long ni = node_index(V, g, id);
  NodeMeta m = V.meta[ni];
  const long pi = node_index(V, g, m.parent);
  const NodeMeta pm = V.meta[pi];
  const int a = m.fmove;
  load_board(w, V, S, pi);
  if (a != V.P) {
    const int color = pm.to_play;
    label_components(w, V, S, true);
    group_liberties(w, V, S);
    int ncap = 0, ko = -1;
    apply_move_in_scratch(w, V, S, a, color, &ncap, &ko);
    m.ko = ko;
    if (pm.to_play == 1) m.caps_b += ncap; else m.caps_w += ncap;
  }
  node_init_from_scratch(w, V, S, g, id, m);
}

// play_move!(position, a) into a fresh node.  Returns the new node id, -1 on pool exhaustion, -2 on an illegal move.
// defer (View::defer_expand, the engine's select phase): only allocate the node and link it -- nothing in the rest of
// the select phase looks at a new, unexpanded leaf's board, rows or legal mask -- and leave node_expand_child to
// k_expand, which runs one wave per new leaf instead of eight expansions in a row per game (21.7 us each: 62 % of the
// select phase).  Terminal children are finished at once: their board is scored right after the descent.
template <class W>
AGZ_FN int node_create_child(W& w, const View& V, Scratch& S, int g, int parent, int a, bool defer = false) {
  const long pi = node_index(V, g, parent);
  const NodeMeta pm = V.meta[pi];
  const int P = V.P;
  if (a < 0 || a >= V.A || !legal_bit(V, pi, a)) return -2;
  AGZ_STAMP_BEGIN(w);
  const int id = pool_alloc(w, V, S, g);
  if (id < 0) return -1;
  NodeMeta m;
  m.parent = parent;
  m.n = pm.n + 1;
  m.fmove = (int16_t)a;
  m.last_move = (int16_t)a;
  m.losses = 0;
  m.to_play = (int8_t)-pm.to_play;
  m.flags = NF_ALLOC;
  m.caps_b = pm.caps_b;
  m.caps_w = pm.caps_w;
  m.ko = -1;
  m.pad = 0;
  if (a == P && pm.last_move == P) m.flags |= NF_DONE;     // pass: done iff the previous move was a pass too
  GameState& G = V.gs[g];
  const bool terminal = (m.flags & NF_DONE) || m.n >= V.max_game_length;
  const bool later = defer && !terminal && G.npend < kMaxPend;
  w.sync();
  if (w.leader()) {
    V.meta[node_index(V, g, id)] = m;
    V.child[pi * V.AP + a] = id;
    if (later) { V.pend_node[(long)g * kMaxPend + G.npend] = id; G.npend = G.npend + 1; }
  }
  w.sync();
  if (!later) node_expand_child(w, V, S, g, id);
  AGZ_STAMP(w, V, CT_T_CREATE);
#ifdef AGZ_TIMING_EXPERIMENTS
  w.count(&V.counters[CT_N_CREATE], 1);
#endif
  return id;
}

// k_expand: the i-th deferred expansion of game g's select phase
template <class W>
AGZ_FN void game_expand(W& w, const View& V, Scratch& S, int g, int i) {
  if (i >= V.gs[g].npend) return;
  node_expand_child(w, V, S, g, V.pend_node[(long)g * kMaxPend + i]);
}

// ------------------------------------------------------------------ PUCT and select_leaf

// child_Q[a] from the side to move (mcts.jl:86-92): Float32
AGZ_FN float action_q(float n, float wv, float to_play) {
  const float denom = 1.0f + n;
  const float q = wv / denom;
  return q * to_play;
}
// child_action_score[a] (mcts.jl:86-92) of a child's N, W and prior: Float32 Q times to_play, plus Float64 U
AGZ_FN double action_score(float n, float wv, float p, float to_play, double scale) {
  const float denom = 1.0f + n;
  const double u = (scale * (double)p) / (double)denom;
  return (double)action_q(n, wv, to_play) + u;
}

// c_base > 0 (agz_search_set_puct): c_puct grows with the logarithm of the node's visits
AGZ_FN double puct_scale(const View& V, float n_node) {
  const float one_plus_n = 1.0f + n_node;
  if (V.c_base > 0.0) {
    const double c = V.c_puct + agz_log(((double)one_plus_n + V.c_base) / V.c_base);
    return c * (double)sqrtf(one_plus_n);
  }
  return V.c_puct * (double)sqrtf(one_plus_n);
}

// pv_k > 0 (agz_search_set_puct_variance): that scale times the variance factor of the node's own (n, W, S); the factor
// goes out through `factor` when asked for
AGZ_FN double puct_scale(const View& V, float n_node, float w_node, float s_node, double* factor = nullptr) {
  const double scale = puct_scale(V, n_node);
  if (!(V.pv_k > 0.0)) return scale;
  const double f = agz_variance_factor(n_node, w_node, s_node, V.pv_k, V.pv_prior, V.pv_weight);
  if (factor) *factor = f;
  return scale * f;
}

// PUCT rule options (View::fpu_on / c_base, agz_search_set_puct): is either part on?
AGZ_FN bool puct_rule_on(const View& V) { return V.fpu_on != 0 || V.c_base > 0.0; }

// First-play urgency.  A lane's share of M, the policy mass of the node's visited children in units of 2^-30: an
// integer sum, so order-free and exact
AGZ_FN long long fpu_mass(float n, float p) { return n > 0.0f ? (long long)((double)p * 1073741824.0) : 0ll; }
// the sum of a wave's shares, through the int reductions every wave has (the low 24 bits and the rest apart)
template <class W>
AGZ_FN long long reduce_sum_i64(W& w, long long v) {
  const int lo = w.reduce_sum((int)(v & 0xffffffll));
  const int hi = w.reduce_sum((int)(v >> 24));
  return (long long)hi * 16777216ll + (long long)lo;
}
// f, the Q of every unvisited child of a node with own statistics (n_s, w_s): the node's value from the side to move,
// less rho * sqrt(m); rho = fpu_r_root at the game's root
AGZ_FN float fpu_value(const View& V, bool is_root, float n_s, float w_s, float to_play, long long M) {
  const double m = (double)M * (1.0 / 1073741824.0);
  const float q_s = w_s / (1.0f + n_s);
  const float qp = q_s * to_play;
  const double rho = is_root ? V.fpu_r_root : V.fpu_r;
  return (float)((double)qp - rho * agz_sqrt(m));
}
// the score of an unvisited child under the FPU: f for its Q, its U as action_score writes it with N_a = 0
AGZ_FN double fpu_score(float f, float p, double scale) {
  const double u = (scale * (double)p) / (double)1.0f;
  return (double)f + u;
}
// the score of a child under the current rule: with the FPU on an unvisited child has f for its Q
AGZ_FN double child_score(bool fpu, float f, float n, float wv, float p, float to_play, double scale) {
  const double s = action_score(n, wv, p, to_play, scale);
  return fpu && n == 0.0f ? fpu_score(f, p, scale) : s;
}

// k-th (0-based) set flag in ascending index order; every lane scans (LDS broadcast reads)
AGZ_FN int kth_flag(const int8_t* flag, int n, int k) {
  for (int a = 0; a < n; ++a)
    if (flag[a]) { if (k == 0) return a; --k; }
  return -1;
}

// Forced playouts (View::forced_k = k > 0).  At the root level of a descent a legal child that has been
// visited at all is UNDER-FORCED while N_a < sqrt(k * P_a * T), T = sum of the root's child visits; stated without the
// root, in f64, in this order of operations.  Under-forced children all score kForcedScore, above every real score, so
// the unchanged arg-max and tie rule picks among them.
constexpr double kForcedScore = 1.0e300;
AGZ_FN bool under_forced(double k, float n, float p, float total) {
  return n > 0.0f && (double)n * (double)n < (k * (double)p) * (double)total;
}

// Does a descent of game slot g from its root run under the forced rule?  Self-play full searches do (every search
// with the playout cap off); fast searches, the arena, analysis and review never; a single tree (G_MANUAL) follows the
// setting.  root_n = position.n of the root about to be searched.
AGZ_FN bool forced_search(const View& V, const GameState& G, int root_n);

// select_leaf (mcts.jl:108-138), the one descent of the device and the host simulator.  A wave of W::kLanes lanes keeps
// a node's child rows in registers, R >= ceil(AP / kLanes) elements a = lane + kLanes * r per lane; what lies past AP or
// A is loaded from a clamped index and masked out of every sum, arg-max and flag.  Everything that depends only on the
// node id -- meta, N / W / P / child-id rows, the legal words -- is requested at once, the node's own N comes along from
// the parent's row of the level above, and the chosen child's id and N come out of the registers by shuffle: one memory
// round trip per level.
// Mode, the root level (depth 0) of the descent alone: kSelForced -- the descent starts at the root of a search under the
// forced rule; kSelGiven -- the caller chose the root action (root_pick, the Gumbel root search); the pass-first rule
// keeps its precedence, nothing is scored and no tie draw is made there.
constexpr int kSelPlain = 0, kSelForced = 1, kSelGiven = 2;
template <int R, int Mode, class W>
AGZ_FN int descend(W& w, const View& V, Scratch& S, int g, int from, int* plen_out, bool defer, int root_pick) {
  constexpr bool Forced = Mode == kSelForced;
  constexpr int L = wave_lanes<W>::value;
  // element a >= 0 of a row sits in lane a % L, row a / L: unsigned, so that at L = 64 these are a & 63 and a >> 6
  auto lane_of = [](int a) { return (int)((unsigned)a % (unsigned)L); };
  auto row_of = [](int a) { return (int)((unsigned)a / (unsigned)L); };
  GameState& G = V.gs[g];
  const int A = V.A, AP = V.AP, pass = V.P;
  const uint32_t move_key = (uint32_t)V.meta[node_index(V, g, G.root)].n;
  const uint32_t sel = (uint32_t)G.sel;
  // the PUCT rule options (agz_search_set_puct): uniform branches on the View, so that off nothing below is new work
  const bool rule = puct_rule_on(V), fpu = V.fpu_on != 0;
  // the variance factor (agz_search_set_puct_variance): uniform too; off, no S row is loaded
  const bool pv = V.pv_k > 0.0;
  const int root = G.root;
  int cur = from, depth = 0, plen = 0;
  int levels = 0, unvisited = 0;                               // CT_PUCT_LEVELS / CT_PUCT_UNVISITED of this descent
  int pv_levels = 0, pv_raised = 0;                            // CT_UNC_LEVELS / CT_UNC_RAISED of this descent
  w.sync();
  float* np = slotN(V, g, cur);
  float n_cur = *np;
  float w_cur = 0.f;                                           // the node's own W: its parent's row, like n_cur
  float s_cur = 0.f;                                           // ... and its own S, under the variance factor
  if (fpu || pv) w_cur = *slotW(V, g, cur);
  if (pv) s_cur = *slotS(V, g, cur);
  for (;;) {
    const long ni = node_index(V, g, cur);
    const NodeMeta m = V.meta[ni];
    float cn[R], cw[R], cp[R], cs[R];
    int cc[R];
    bool lg[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int a = wave_lane(w) + L * r;
      const bool in = a < AP;
      const long o = ni * AP + (in ? a : 0);
      cn[r] = V.childN[o];
      cw[r] = V.childW[o];
      cp[r] = V.childP[o];
      cs[r] = pv ? V.childS[o] : 0.f;
      cc[r] = in ? V.child[o] : -1;
      lg[r] = a < A && legal_bit(V, ni, a);
    }
    const float n_new = n_cur + 1.0f;
    w.sync();
    if (w.leader()) { *np = n_new; if (plen < V.maxd) S.path[plen] = cur; }
    plen++;
    w.sync();
    if (!(m.flags & NF_EXPANDED)) break;
    auto row_f = [&](const float* v, int a) {              // element a of a row held across the lanes
      float x = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r) { const float t = wave_shfl(w, v[r], lane_of(a)); if (r == row_of(a)) x = t; }
      return x;
    };
    int pick;
    bool given = false, scored = false;
    if constexpr (Mode == kSelGiven) given = depth == 0;
    if (m.last_move == pass && row_f(cn, pass) == 0.0f) {
      pick = pass;    // HACK of mcts.jl:119-126: look at the double pass first
    } else if (given) {
      pick = root_pick;
    } else {
      double factor = 1.0;
      const double scale = pv ? puct_scale(V, n_new, w_cur, s_cur, &factor) : puct_scale(V, n_new);
      if (pv) { pv_levels++; pv_raised += factor > 1.0; }
      const float tp = (float)m.to_play;
      double sc[R];
      double best = -1.0e300;
      bool have = false;
      float total = 0.f;
      if constexpr (Forced) {
        if (depth == 0) {
#pragma unroll
          for (int r = 0; r < R; ++r) total += wave_lane(w) + L * r < A ? cn[r] : 0.f;
          total = w.reduce_sum_f(total);   // visit counts are integers: order-free and exact
        }
      }
      float f = 0.f;
      if (fpu) {
        long long M = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) M += wave_lane(w) + L * r < A ? fpu_mass(cn[r], cp[r]) : 0ll;
        f = fpu_value(V, cur == root, n_new, w_cur, tp, reduce_sum_i64(w, M));
      }
      scored = rule;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        sc[r] = child_score(fpu, f, cn[r], cw[r], cp[r], tp, scale);
        if constexpr (Forced) {
          if (depth == 0 && under_forced(V.forced_k, cn[r], cp[r], total)) sc[r] = kForcedScore;
        }
        if (lg[r] && (!have || sc[r] > best)) { best = sc[r]; have = true; }
      }
      best = w.reduce_max(have ? best : -1.0e300);
      if constexpr (Forced) {
        if (depth == 0 && best == kForcedScore) w.count(&V.counters[CT_FORCED_SEL], 1);
      }
      int cnt = 0, idx = kIntMax;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int a = wave_lane(w) + L * r;
        const bool f = lg[r] && sc[r] == best;
        if (a < AP) S.flag[a] = f;
        if (f) { cnt++; idx = a < idx ? a : idx; }
      }
      cnt = w.reduce_sum(cnt);
      idx = w.reduce_min(idx);
      w.sync();
      if (cnt > 1) {
        const uint64_t bits = agz_draw_u64(V.seed, G.game_id, move_key, AGZ_SITE_PUCT_TIE,
                                           (uint64_t)sel * 1024u + (uint64_t)depth);
        idx = kth_flag(S.flag, A, (int)agz_index(bits, (uint32_t)cnt));
      }
      if (cnt == 0) idx = pass;   // cannot happen: pass is always legal
      pick = idx;
      w.sync();
    }
    int nx = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) { const int t = wave_shfl(w, cc[r], lane_of(pick)); if (r == row_of(pick)) nx = t; }
    const float n_next = row_f(cn, pick);
    if (scored) { levels++; unvisited += n_next == 0.0f; }
    if (fpu || pv) w_cur = row_f(cw, pick);
    if (pv) s_cur = row_f(cs, pick);
    if (nx < 0) nx = node_create_child(w, V, S, g, cur, pick, defer);
    if (nx < 0) break;   // pool exhausted: hand back the current node (flagged in the counters)
    np = &V.childN[ni * AP + pick];      // the child's own N lives in this row (slotN)
    n_cur = n_next;
    cur = nx;
    depth++;
  }
  if (w.leader()) G.sel = (int32_t)(sel + 1);
  if (rule) {
    w.count(&V.counters[CT_PUCT_LEVELS], (unsigned long long)levels);
    w.count(&V.counters[CT_PUCT_UNVISITED], (unsigned long long)unvisited);
  }
  if (pv) {
    w.count(&V.counters[CT_UNC_LEVELS], (unsigned long long)pv_levels);
    w.count(&V.counters[CT_UNC_RAISED], (unsigned long long)pv_raised);
  }
  w.sync();
  *plen_out = plen < V.maxd ? plen : V.maxd;
  return cur;
}

// descend<R, Mode> at the wave's row width for this board: a 64-lane wave takes one of the instantiated widths, any
// other wave (the host simulator's single lane) the one width that covers the largest board
template <int Mode, class W>
AGZ_FN int descend_of(W& w, const View& V, Scratch& S, int g, int from, int* plen_out, bool defer, int root_pick) {
  constexpr int L = wave_lanes<W>::value;
  if constexpr (L == kWave) {
    return with_row_width(V.AP, [&](auto r) {
      return descend<decltype(r)::value, Mode>(w, V, S, g, from, plen_out, defer, root_pick);
    });
  } else {
    return descend<(kAPMax + L - 1) / L, Mode>(w, V, S, g, from, plen_out, defer, root_pick);
  }
}

// select_leaf from `from`; the visited nodes are left in S.path[0..len).  Returns the leaf.
template <class W>
AGZ_FN int select_leaf(W& w, const View& V, Scratch& S, int g, int from, int* plen_out, bool defer = false,
                       bool forced = false, int root_pick = -1) {
  return root_pick >= 0 ? descend_of<kSelGiven>(w, V, S, g, from, plen_out, defer, root_pick)
         : forced       ? descend_of<kSelForced>(w, V, S, g, from, plen_out, defer, -1)
                        : descend_of<kSelPlain>(w, V, S, g, from, plen_out, defer, -1);
}

// walk parents from `node` up to and including `up_to` (or the root); path[0] = topmost
template <class W>
AGZ_FN int walk_path(W& w, const View& V, Scratch& S, int g, int node, int up_to) {
  int len = 0, x = node;
  for (;;) {
    ++len;
    if (x == up_to) break;
    const int p = V.meta[node_index(V, g, x)].parent;
    if (p < 0) break;
    x = p;
  }
  if (len > V.maxd) len = V.maxd;
  x = node;
  w.sync();
  for (int i = len - 1; i >= 0; --i) {
    if (w.leader()) S.path[i] = x;
    x = V.meta[node_index(V, g, x)].parent;
    if (x < 0) x = 0;
  }
  w.sync();
  return len;
}

// W(node) += sign * to_play(node) and losses_applied += sign along the path (mcts.jl:149-171)
template <class W>
AGZ_FN void path_virtual_loss(W& w, const View& V, int g, const int32_t* path, int len, int sign) {
  w.for_each(len, [&](int i) {
    const int node = path[i];
    NodeMeta& m = V.meta[node_index(V, g, node)];
    float* wp = slotW(V, g, node);
    *wp = *wp + (float)(sign * m.to_play);
    if (V.childS) { float* sp = slotS(V, g, node); *sp = *sp + (float)sign; }   // a virtual loss is a value of +-1
    m.losses = (int16_t)(m.losses + sign);
  });
  w.sync();
}

// W(node) += value along the path (backup_value!, mcts.jl:215-225)
template <class W>
AGZ_FN void path_backup(W& w, const View& V, int g, const int32_t* path, int len, float value) {
  w.for_each(len, [&](int i) {
    float* wp = slotW(V, g, path[i]);
    *wp = *wp + value;
    if (V.childS) { float* sp = slotS(V, g, path[i]); const float sq = value * value; *sp = *sp + sq; }
  });
  w.sync();
}

// N(node) -= 1 along the path (revert_visits!, mcts.jl:173-186)
template <class W>
AGZ_FN void path_revert_visits(W& w, const View& V, int g, const int32_t* path, int len) {
  w.for_each(len, [&](int i) {
    float* np = slotN(V, g, path[i]);
    *np = *np - 1.0f;
  });
  w.sync();
}

// incorporate_results!(node, probs, value, up_to) with the path root..node in `path`
template <class W>
AGZ_FN int incorporate(W& w, const View& V, int g, int node, const float* probs, float value,
                       const int32_t* path, int len) {
  const long ni = node_index(V, g, node);
  const uint8_t flags = V.meta[ni].flags;
  if (flags & NF_DONE) return AGZ_ASSERT_DONE_NODE;
  if (flags & NF_EXPANDED) {
    path_revert_visits(w, V, g, path, len);
    w.count(&V.counters[CT_DUP], 1);
    return AGZ_OK;
  }
  w.sync();
  if (w.leader()) V.meta[ni].flags = flags | NF_EXPANDED;
  w.for_each(V.A, [&](int a) {
    V.childP[ni * V.AP + a] = probs[a];
    V.childW[ni * V.AP + a] = value;   // initialise child Q as the parent's value, mcts.jl:203-211
    if (V.childS) V.childS[ni * V.AP + a] = value * value;
  });
  w.sync();
  path_backup(w, V, g, path, len, value);
  return AGZ_OK;
}

// inject_noise!(node) (mcts.jl:233-239): Dirichlet(alpha) over ALL actions from the draw stream, mixed into `row` (the
// node's prior row)
template <class W>
AGZ_FN void inject_noise(W& w, const View& V, Scratch& S, int g, int node, float* row) {
  const GameState& G = V.gs[g];
  const long ni = node_index(V, g, node);
  const uint32_t move_key = (uint32_t)V.meta[ni].n;
  const int A = V.A;
  w.for_each(A, [&](int a) {
    S.dbuf[a] = agz_dirichlet_gamma(V.seed, G.game_id, move_key, (uint32_t)a, V.alpha);
  });
  w.sync();
  double sum = 0.0;
  for (int a = 0; a < A; ++a) sum += S.dbuf[a];   // fixed ascending order on every lane
  w.for_each(A, [&](int a) {
    const double d = sum > 0.0 ? S.dbuf[a] / sum : 1.0 / (double)A;
    const double mixed = (double)row[a] * (1.0 - V.noise_w) + d * V.noise_w;
    row[a] = (float)mixed;
  });
  w.sync();
}

// ------------------------------------------------------------------ root exploration
// The root policy temperature and the noise over the legal moves (include/agz_explore.h states the arithmetic, include/agz.h
// the rule).  The per-element values go through S.dbuf and every sum is taken over it in ascending action order on
// every lane, as inject_noise sums.

// the sum of S.dbuf over the flagged actions, ascending
AGZ_FN double sum_flagged(const Scratch& S, int A) {
  double s = 0.0;
  for (int a = 0; a < A; ++a)
    if (S.flag[a]) s += S.dbuf[a];
  return s;
}

// Rule 1 on `row`: the legal, positive entries re-softmaxed at T and scaled to the mass they had.  Returns whether there
// was such an entry (a row without one is left alone).
template <class W>
AGZ_FN bool temper_row(W& w, const View& V, Scratch& S, long ni, int n_root, float* row) {
  const int A = V.A;
  const double T = agz_temperature(n_root, V.pt_early, V.pt_late, V.pt_half);
  int cnt = 0;
  w.for_each(V.AP, [&](int a) {
    const bool on = a < A && legal_bit(V, ni, a) && row[a] > 0.0f;
    S.flag[a] = on;
    S.dbuf[a] = on ? (double)row[a] : 0.0;
    if (on) cnt++;
  });
  cnt = w.reduce_sum(cnt);
  w.sync();
  if (cnt == 0) return false;
  const double mass = sum_flagged(S, A);
  w.sync();
  double mx = -__builtin_huge_val();
  w.for_each(A, [&](int a) {
    if (!S.flag[a]) return;
    const double x = agz_explore_temper_x(row[a], T);
    S.dbuf[a] = x;
    if (x > mx) mx = x;
  });
  mx = w.reduce_max(mx);
  w.for_each(A, [&](int a) { if (S.flag[a]) S.dbuf[a] = agz_exp(S.dbuf[a] - mx); });
  w.sync();
  const double E = sum_flagged(S, A);
  w.for_each(A, [&](int a) { if (S.flag[a]) row[a] = agz_explore_temper_p(S.dbuf[a], E, mass); });
  w.sync();
  return true;
}

// Rule 2 on `row`: Dirichlet noise of total concentration V.noise_total over the legal actions, the concentration of
// each shaped by the row under V.noise_shaped; alpha (may be null) receives alpha_a, 0 for an illegal action
template <class W>
AGZ_FN void legal_noise(W& w, const View& V, Scratch& S, int g, long ni, int n_root, float* row, double* alpha) {
  const GameState& G = V.gs[g];
  const int A = V.A;
  const int shaped = V.noise_shaped;
  int L = 0;
  w.for_each(V.AP, [&](int a) {
    const bool lg = a < A && legal_bit(V, ni, a);
    S.flag[a] = lg;
    if (lg) L++;
  });
  L = w.reduce_sum(L);
  w.sync();
  if (L == 0) return;   // cannot happen: pass is always legal
  const double u = 1.0 / (double)L;
  double ssum = 0.0;
  if (shaped) {
    w.for_each(A, [&](int a) { S.dbuf[a] = S.flag[a] ? agz_explore_shape_l(row[a]) : 0.0; });
    w.sync();
    const double mean = sum_flagged(S, A) / (double)L;
    w.sync();
    w.for_each(A, [&](int a) { S.dbuf[a] = S.flag[a] ? agz_explore_shape_s(S.dbuf[a], mean) : 0.0; });
    w.sync();
    ssum = sum_flagged(S, A);
    w.sync();
  }
  w.for_each(A, [&](int a) {
    double al = 0.0, gm = 0.0;
    if (S.flag[a]) {
      al = agz_explore_alpha(V.noise_total, u, shaped, shaped ? S.dbuf[a] : 0.0, ssum);
      gm = agz_dirichlet_gamma(V.seed, G.game_id, (uint32_t)n_root, (uint32_t)a, al);
    }
    if (alpha) alpha[a] = al;
    S.dbuf[a] = gm;
  });
  w.sync();
  const double gsum = sum_flagged(S, A);
  w.for_each(A, [&](int a) {
    if (!S.flag[a]) return;
    const double d = gsum > 0.0 ? S.dbuf[a] / gsum : u;
    row[a] = agz_explore_mix(row[a], d, V.noise_w);
  });
  w.sync();
}

// What a search that gets noise does to its root's prior before it begins: the temperature first, the noise second.
// With both rules off this is inject_noise.  row = null: the node's stored row, and the roots are counted; otherwise
// a copy of it [AP] (agz_tree_explore_rows), with `tempered` [A] = the row between the two rules and `alpha` [A] = the
// concentration of each action (either may be null).
template <class W>
AGZ_FN void root_explore(W& w, const View& V, Scratch& S, int g, int node, float* row = nullptr, float* tempered = nullptr,
                         double* alpha = nullptr) {
  const long ni = node_index(V, g, node);
  const bool stored = row == nullptr;
  if (stored) row = V.childP + ni * V.AP;
  const int n_root = V.meta[ni].n;
  if (V.pt_on) {
    const bool did = temper_row(w, V, S, ni, n_root, row);
    if (did && stored) w.count(&V.counters[CT_EXP_TEMPERED], 1);
  }
  if (tempered) {
    w.for_each(V.A, [&](int a) { tempered[a] = row[a]; });
    w.sync();
  }
  if (V.noise_total > 0.0) {
    legal_noise(w, V, S, g, ni, n_root, row, alpha);
    if (stored) w.count(&V.counters[CT_EXP_NOISED], 1);
  } else {
    if (alpha) w.for_each(V.A, [&](int a) { alpha[a] = V.alpha; });
    inject_noise(w, V, S, g, node, row);
  }
}

// children_as_pi(root, squash) into out[A] (mcts.jl:241-252)
template <class W>
AGZ_FN void children_as_pi(W& w, const View& V, Scratch& S, long ni, bool squash, float* out) {
  const int A = V.A;
  if (!squash) {
    float part = 0.f;
    w.for_each(A, [&](int a) { part += V.childN[ni * V.AP + a]; });
    const float s = w.reduce_sum_f(part);   // visit counts are integers: order-free and exact
    w.for_each(A, [&](int a) { out[a] = V.childN[ni * V.AP + a] / s; });
  } else {
    w.for_each(A, [&](int a) { S.dbuf[a] = agz_pow((double)V.childN[ni * V.AP + a], 0.98); });
    w.sync();
    double s = 0.0;
    for (int a = 0; a < A; ++a) s += S.dbuf[a];
    w.for_each(A, [&](int a) { out[a] = (float)(S.dbuf[a] / s); });
  }
  w.sync();
}

// Policy target pruning: children_as_pi of the node's visits with the forced playouts (k = V.forced_k)
// that the search did not agree with taken out.  c* = the most visited child, lowest index on ties; S* = its PUCT score
// under scale = puct_scale(rootN).  Every other visited child a keeps
//   N'_a = min(N_a, max(N_a - sqrt(k P_a T), N_min, 0)),   N_min = scale P_a / (S* - q_a) - 1  (N_a when S* <= q_a),
// the visits at which its score would still not pass S*, and none at all when what is left of a reduced child is <= 1.
// All f64 but q_a, which is action_q's f32.  The row is N' (squash: N'^0.98) over its f64 sum in ascending index
// order, narrowed to f32 last -- for an unchanged row bit for bit children_as_pi's.  Returns whether some N'_a < N_a.
template <class W>
AGZ_FN bool pruned_pi(W& w, const View& V, Scratch& S, long ni, float rootN, bool squash, float* out) {
  const int A = V.A;
  const float* cN = V.childN + ni * V.AP;
  float mx = -1.0f, part = 0.f;
  w.for_each(A, [&](int a) { const float c = cN[a]; mx = c > mx ? c : mx; part += c; });
  mx = w.reduce_max_f(mx);
  const float total = w.reduce_sum_f(part);   // visit counts are integers: order-free and exact
  int cs = kIntMax;
  w.for_each(A, [&](int a) { if (cN[a] == mx && a < cs) cs = a; });
  cs = w.reduce_min(cs);
  const float tp = (float)V.meta[ni].to_play;
  // (under the variance factor, with the node's own W and S: node ni is node ni % cap of slot ni / cap)
  const int pg = (int)(ni / V.cap), pnode = (int)(ni % V.cap);
  const double scale =
      V.pv_k > 0.0 ? puct_scale(V, rootN, *slotW(V, pg, pnode), *slotS(V, pg, pnode)) : puct_scale(V, rootN);
  const float* cW = V.childW + ni * V.AP;
  const float* cP = V.childP + ni * V.AP;
  const double s_star = action_score(cN[cs], cW[cs], cP[cs], tp, scale);
  const double k = V.forced_k;
  bool changed = false;
  w.sync();
  w.for_each(A, [&](int a) {
    const float n = cN[a];
    double keep = (double)n;
    if (a != cs && n > 0.0f) {
      const double p = (double)cP[a];
      const double nf = sqrt((k * p) * (double)total);
      const double gap = s_star - (double)action_q(n, cW[a], tp);
      const double n_min = gap <= 0.0 ? (double)n : (scale * p) / gap - 1.0;
      double m = (double)n - nf;
      m = n_min > m ? n_min : m;
      m = m > 0.0 ? m : 0.0;
      m = m < (double)n ? m : (double)n;
      if (m < (double)n) {
        if (m <= 1.0) m = 0.0;
        changed = true;
      }
      keep = m;
    }
    S.dbuf[a] = squash ? agz_pow(keep, 0.98) : keep;
  });
  changed = w.any(changed);
  w.sync();
  double s = 0.0;
  for (int a = 0; a < A; ++a) s += S.dbuf[a];   // fixed ascending order on every lane
  w.for_each(A, [&](int a) { out[a] = (float)(S.dbuf[a] / s); });
  w.sync();
  return changed;
}

// The value statistics of a node's children under z (agz_tree_child_lcb; include/agz_uncertainty.h rules 1 and 2), from the
// node's side to move, whatever the setting of the LCB rule: mean, sd and lcb [A] each.  Needs the moments on.
template <class W>
AGZ_FN void child_lcb_rows(W& w, const View& V, int g, int node, double z, double* mean, double* sd, double* lcb) {
  const long ni = node_index(V, g, node);
  const float tp = (float)V.meta[ni].to_play;
  w.for_each(V.A, [&](int a) {
    const long o = ni * V.AP + a;
    const agz_value_stats st = agz_child_stats(V.childN[o], V.childW[o], V.childS[o]);
    mean[a] = st.mean;
    sd[a] = st.sd;
    lcb[a] = agz_stats_lcb(st, tp, z);
  });
  w.sync();
}

// pick_move (mcts_play.jl:52-71).  Returns AGZ_OK / AGZ_ASSERT_SOFTPICK.
template <class W>
AGZ_FN int pick_move(W& w, const View& V, Scratch& S, int g, int* a_out) {
  const GameState& G = V.gs[g];
  const long ni = node_index(V, g, G.root);
  const int A = V.A, n = V.meta[ni].n;
  const int tau = V.two_player ? -1 : V.tau;
  // the move temperature (agz_search_set_move_temperature, two_player off): at T <= 0.01 the arg-max branch, verbatim
  const bool tempered = V.mt_on != 0 && !V.two_player;
  const double T = tempered ? agz_temperature(n, V.mt_early, V.mt_late, V.mt_half) : 0.0;
  if (tempered ? T <= AGZ_EXPLORE_ARGMAX_T : n >= tau) {
    float mx = -1.0f;
    w.for_each(A, [&](int a) { const float c = V.childN[ni * V.AP + a]; mx = c > mx ? c : mx; });
    mx = w.reduce_max_f(mx);
    // the LCB rule (agz_search_set_lcb): among the children with enough visits the largest lower confidence bound,
    // ties to the larger N, then to the lower action; no draw.  Below min_visits at the top, today's branch
    if (V.lcb_z > 0.0 && !(mx < (float)V.lcb_min_visits)) {
      const float tp = (float)V.meta[ni].to_play;
      const double floor_n = V.lcb_min_ratio * (double)mx;
      double best = -1.0e300;
      w.for_each(V.AP, [&](int a) {
        const long o = ni * V.AP + a;
        const float c = a < A ? V.childN[o] : -1.0f;
        const bool el = a < A && c >= (float)V.lcb_min_visits && (double)c >= floor_n;
        S.flag[a] = el;
        if (!el) return;
        const double l = agz_child_lcb(c, V.childW[o], V.childS[o], tp, V.lcb_z);
        S.dbuf[a] = l;
        if (l > best) best = l;
      });
      best = w.reduce_max(best);
      w.sync();
      float bn = -1.0f;
      w.for_each(A, [&](int a) {
        if (S.flag[a] && S.dbuf[a] == best) { const float c = V.childN[ni * V.AP + a]; bn = c > bn ? c : bn; }
      });
      bn = w.reduce_max_f(bn);
      int pick = kIntMax;
      w.for_each(A, [&](int a) {
        if (S.flag[a] && S.dbuf[a] == best && V.childN[ni * V.AP + a] == bn && a < pick) pick = a;
      });
      pick = w.reduce_min(pick);
      w.sync();
      w.count(&V.counters[CT_UNC_LCB], 1);
      w.count(&V.counters[CT_UNC_LCB_OFF_MAX], bn != mx ? 1 : 0);
      *a_out = pick;
      return AGZ_OK;
    }
    int cnt = 0, idx = kIntMax;
    w.for_each(V.AP, [&](int a) {
      const bool f = a < A && V.childN[ni * V.AP + a] == mx;
      S.flag[a] = f;
      if (f) { cnt++; idx = a < idx ? a : idx; }
    });
    cnt = w.reduce_sum(cnt);
    idx = w.reduce_min(idx);
    w.sync();
    if (cnt > 1) {
      const uint64_t bits = agz_draw_u64(V.seed, G.game_id, (uint32_t)n, AGZ_SITE_PICK_TIE, 0);
      idx = kth_flag(S.flag, A, (int)agz_index(bits, (uint32_t)cnt));
    }
    w.sync();
    *a_out = idx;
    return AGZ_OK;
  }
  if (tempered) {
    // sample in proportion to (N_a / max N)^(1/T), pass included, with the soft pick's draw
    float mx = 0.0f;
    w.for_each(A, [&](int a) { const float c = V.childN[ni * V.AP + a]; mx = c > mx ? c : mx; });
    mx = w.reduce_max_f(mx);
    if (!(mx > 0.0f)) return AGZ_ASSERT_SOFTPICK;
    w.for_each(A, [&](int a) { S.dbuf[a] = agz_explore_pick_weight(V.childN[ni * V.AP + a], mx, T); });
    w.sync();
    double sum = 0.0;
    for (int a = 0; a < A; ++a) sum += S.dbuf[a];   // fixed ascending order on every lane
    const double r = agz_u01(agz_draw_u64(V.seed, G.game_id, (uint32_t)n, AGZ_SITE_SOFTPICK, 0)) * sum;
    int pick = -1, last = -1;
    double acc = 0.0;
    for (int a = 0; a < A && pick < 0; ++a) {
      const double wa = S.dbuf[a];
      acc += wa;
      if (wa > 0.0) { last = a; if (acc > r) pick = a; }
    }
    if (pick < 0) pick = last;                      // rounding left r at or past the sum: the highest weighted action
    const bool off_max = V.childN[ni * V.AP + pick] != mx;
    w.sync();
    w.count(&V.counters[CT_EXP_SAMPLED], 1);
    w.count(&V.counters[CT_EXP_OFF_MAX], off_max ? 1 : 0);
    *a_out = pick;
    return AGZ_OK;
  }
  // soft pick: cdf = cumsum(child_N) ./ cdf[end-1]; first index with !(cdf < u)
  float denom = 0.f;
  {
    float part = 0.f;
    w.for_each(A - 1, [&](int a) { part += V.childN[ni * V.AP + a]; });
    denom = w.reduce_sum_f(part);
  }
  const double u = agz_u01(agz_draw_u64(V.seed, G.game_id, (uint32_t)n, AGZ_SITE_SOFTPICK, 0));
  w.for_each(A, [&](int a) { S.dbuf[a] = (double)V.childN[ni * V.AP + a]; });
  w.sync();
  int f = A;
  float acc = 0.f;
  for (int a = 0; a < A; ++a) {
    acc += (float)S.dbuf[a];
    const float c = acc / denom;
    if (!((double)c < u)) { f = a; break; }
  }
  w.sync();
  if (f >= A || S.dbuf[f] == 0.0) return AGZ_ASSERT_SOFTPICK;
  *a_out = f;
  return AGZ_OK;
}

// ------------------------------------------------------------------ per-move phase / lifecycle

template <class W>
AGZ_FN void push_history(W& w, const View& V, int g, long ni_board) {
  GameState& G = V.gs[g];
  int8_t* h = V.hist + (long)g * 7 * V.PP;
  const int keep = G.hist_len < 6 ? G.hist_len : 6;
  for (int k = keep; k >= 1; --k) {
    w.for_each(V.P, [&](int p) { h[k * V.PP + p] = h[(k - 1) * V.PP + p]; });
    w.sync();
  }
  w.for_each(V.P, [&](int p) { h[p] = V.board[ni_board * V.PP + p]; });
  w.sync();
  if (w.leader()) G.hist_len = keep + 1;
  w.sync();
}

// Make `child` (a child of the current root via action a) the new root; everything else in
// the old tree is released (play_move!(player, c) mcts_play.jl:40-48: siblings dropped).
template <class W>
AGZ_FN void reroot(W& w, const View& V, Scratch& S, int g, int a, int child) {
  GameState& G = V.gs[g];
  const int old_root = G.root;
  const long oi = node_index(V, g, old_root);
  const float cn = V.childN[oi * V.AP + a], cw = V.childW[oi * V.AP + a];
  const float cs = V.childS ? V.childS[oi * V.AP + a] : 0.f;
  push_history(w, V, g, oi);
  discard_except(w, V, g, old_root, a);
  if (V.sk_key && w.leader()) {      // the old root's position stays seen
    const int len = V.sk_len[g];
    if (len < sk_log_stride(V)) { V.sk_log[(long)g * sk_log_stride(V) + len] = V.sk_key[oi]; V.sk_len[g] = len + 1; }
  }
  if (w.leader()) {
    G.rootN = cn;
    G.rootW = cw;
    if (V.childS) V.rootS[g] = cs;
    G.root = child;
    G.sel = 0;
    NodeMeta& cm = V.meta[node_index(V, g, child)];
    cm.parent = -1;
  }
  w.sync();
}

// (defined below, behind root_board_valid)
template <class W>
AGZ_FN bool root_install(W& w, const View& V, Scratch& S, int g, const int8_t* board, const int8_t* hist,
                         const agz_position_info& info, int phase, bool analysis);

// the selfplay.jl:9 resign coin of game `game_id` (move 0 of its draw stream, wherever the game starts)
AGZ_FN void game_resign_coin(const View& V, GameState& G, uint64_t game_id) {
  const double u = agz_u01(agz_draw_u64(V.seed, game_id, 0, AGZ_SITE_RESIGN, 0));
  G.resign_disabled = u < V.resign_disable_frac;
  G.resign_threshold = G.resign_disabled ? -1.0 : V.resign_threshold;
}

// initialize_game! on an empty board (mcts_play.jl:110-118) + the selfplay.jl:9 resign coin.  With a table of start
// positions set (View::st_*), initialize_game!(player, start) on entry start_key mod st_count instead: the root, the
// history ring, komi and position.n are the entry's, so every draw of the game is keyed by the entry's n onwards.
template <class W>
AGZ_FN void game_start(W& w, const View& V, Scratch& S, int g, uint64_t game_id, uint64_t start_key) {
  GameState& G = V.gs[g];
  const bool table = V.st_count > 0;
  const long s = table ? (long)(start_key % (uint64_t)V.st_count) : 0;
  const agz_position_info info = table ? V.st_info[s] : empty_position_info(V.komi);
  // one install: the empty board is a null `board` and `hist` (no history, S.sb all zero)
  root_install(w, V, S, g, table ? V.st_board + s * V.P : nullptr, table ? V.st_hist + s * 7 * V.P : nullptr, info, G_INIT,
               false);
  if (w.leader()) {
    G.game_id = game_id;
    game_resign_coin(V, G, game_id);
    G.short_first = 0;
    V.gumbel[g].n = -1;
  }
  w.sync();
  w.count(&V.counters[CT_STARTED], 1);
  if (table) return;
  // bench-only: a random opening prefix so that concurrent games are at mixed stages, and a
  // shortened first search so that they are also at mixed phases of their readout budget
  if (V.stagger > 0) {
    if (w.leader()) G.short_first = 1;
    w.sync();
    const int want = (int)agz_index(agz_draw_u64(V.seed, game_id, 0, AGZ_SITE_STAGGER, 0), (uint32_t)V.stagger + 1u);
    for (int t = 0; t < want; ++t) {
      const long ni = node_index(V, g, G.root);
      int cnt = 0;
      w.for_each(V.AP, [&](int a) {
        const bool f = a < V.P && legal_bit(V, ni, a);
        S.flag[a] = f;
        if (f) cnt++;
      });
      cnt = w.reduce_sum(cnt);
      w.sync();
      if (cnt == 0) break;
      const uint64_t bits = agz_draw_u64(V.seed, game_id, 0, AGZ_SITE_STAGGER, (uint64_t)t + 1u);
      const int a = kth_flag(S.flag, V.P, (int)agz_index(bits, (uint32_t)cnt));
      w.sync();
      const int ch = node_create_child(w, V, S, g, G.root, a);
      if (ch < 0) break;
      reroot(w, V, S, g, a, ch);
      if (w.leader()) { G.rootN = 0.f; G.rootW = 0.f; if (V.childS) V.rootS[g] = 0.f; }
      w.sync();
    }
  }
}

// A caller's position before it becomes a root (analysis mode): every point in {-1, 0, +1}, no stone group without a
// liberty (the LDS labelling of the move rules), the ko point, if set, empty.  The board is left in S.sb.
template <class W>
AGZ_FN bool root_board_valid(W& w, const View& V, Scratch& S, const int8_t* board, int ko) {
  int bad = 0;
  w.for_each(V.P, [&](int p) {
    const int c = board[p];
    S.sb[p] = (int8_t)c;
    if (c < -1 || c > 1) bad++;
  });
  bad = w.reduce_sum(bad);
  w.sync();
  if (bad) return false;
  if (ko >= 0 && ko < V.P && S.sb[ko] != 0) return false;
  label_components(w, V, S, true);
  group_liberties(w, V, S);
  int dead = 0;
  w.for_each(V.P, [&](int p) { if (S.sb[p] != 0 && S.maxlib[S.label[p]] < 0) dead++; });
  dead = w.reduce_sum(dead);
  w.sync();
  return dead == 0;
}

// initialize_game!(player, pos) (mcts_play.jl:110-118) on slot g: an empty pool, `board` [P] (null: empty) as the root, the
// info.history_len boards of `hist` ([.][P], newest first) as the history ring, the slot in `phase`.  The one install of
// agz_tree_init (TOP_INIT, analysis = false, unchanged) and of the analysis mode (analysis = true): there an invalid
// board returns false before the slot is touched, and a position whose last two moves were passes is a finished root
// -- MCTSNode(pos) keeps pos.done (mcts.jl:66-80, board.jl:437), which agz_position_info carries as those two moves.
// The draw key (G.game_id, G.sel) and the readout target are the caller's.
template <class W>
AGZ_FN bool root_install(W& w, const View& V, Scratch& S, int g, const int8_t* board, const int8_t* hist,
                         const agz_position_info& info, int phase, bool analysis) {
  GameState& G = V.gs[g];
  if (analysis && !root_board_valid(w, V, S, board, info.ko)) return false;
  w.for_each(V.cap, [&](int i) { V.freelist[(long)g * V.cap + i] = V.cap - 1 - i; });
  w.sync();
  if (w.leader()) {
    G.rootN = 0.f; G.rootW = 0.f; G.target = 0.f; G.komi = info.komi;
    if (V.childS) V.rootS[g] = 0.f;
    G.sel = 0; G.move_count = 0; G.nqs = 0; G.hist_len = info.history_len;
    G.free_top = V.cap; G.garbage = 0; G.nleaves = 0; G.err = 0; G.result = 0; G.was_resign = 0; G.nodes_used = 0;
    G.short_searches = 0;
    G.phase = phase;
    V.eval_ord[g] = 0;
    G.resign_threshold = V.resign_threshold; G.resign_disabled = 0;
  }
  w.sync();
  for (int h = 0; hist && h < info.history_len && h < 7; ++h)
    w.for_each(V.P, [&](int p) { V.hist[((long)g * 7 + h) * V.PP + p] = hist[(long)h * V.P + p]; });
  if (V.sk_key) {      // the key log begins with the history boards: board h had (-1)^(h+1) * to_play to move
    int len = 0;
    for (int h = 0; hist && h < info.history_len && h < 7; ++h, ++len) {
      const uint64_t k = board_key(w, V, hist + (long)h * V.P, (h & 1) ? info.to_play : -info.to_play, V.ko_rule);
      if (w.leader()) V.sk_log[(long)g * sk_log_stride(V) + h] = k;
    }
    if (w.leader()) V.sk_len[g] = len;
    w.sync();
  }
  const int id = pool_alloc(w, V, S, g);
  w.for_each(V.P, [&](int p) { S.sb[p] = board ? board[p] : (int8_t)0; });
  w.sync();
  NodeMeta m;
  m.parent = -1; m.n = info.n; m.ko = info.ko; m.caps_b = info.caps_black; m.caps_w = info.caps_white;
  m.fmove = -1; m.last_move = (int16_t)info.last_move; m.losses = 0; m.to_play = (int8_t)info.to_play;
  m.flags = analysis && info.last_move == V.P && info.prev_move == V.P ? NF_DONE : 0;
  m.pad = 0;
  node_init_from_scratch(w, V, S, g, id, m);
  if (w.leader()) G.root = id;
  w.sync();
  return true;
}

// set_result! + extract_data (mcts_play.jl:100-108,126-139): copy the finished game into the
// record arena and release the slot.
template <class W>
AGZ_FN void game_finish(W& w, const View& V, Scratch& S, int g, int winner, int was_resign, float score) {
  GameState& G = V.gs[g];
  const int nm = G.move_count;
  const long slot = (long)(w.fetch_add(&V.counters[CT_RECORDED], 1ull) % (unsigned long long)V.fin_cap);
  w.count(&V.counters[CT_FINISHED], 1);
  const int mgl = V.max_game_length;
  if (w.leader()) {
    agz_game_header h;
    h.game_id = G.game_id; h.num_moves = nm; h.result = winner; h.was_resign = was_resign;
    h.resign_disabled = G.resign_disabled; h.final_score = score; h.short_searches = G.short_searches;
    V.fin_hdr[slot] = h;
    G.result = winner; G.was_resign = was_resign; G.phase = G_IDLE;
  }
  w.for_each(nm, [&](int k) {
    V.fin_moves[slot * mgl + k] = V.rec_moves[(long)g * mgl + k];
    V.fin_q[slot * mgl + k] = V.rec_q[(long)g * mgl + k];
  });
  w.for_each(nm * V.A, [&](int i) { V.fin_pi[slot * mgl * V.A + i] = V.rec_pi[(long)g * mgl * V.A + i]; });
  w.sync();
  if (was_resign) w.count(&V.counters[CT_RESIGNED], 1);
}

// A game whose node pool refused an allocation in the last select phase (G.err).  The reference's tree is unbounded
// (mcts.jl:140-147: a child is a fresh heap object); a fixed pool has to answer "and when it is full?".  With
// AGZ_POOL_MOVE_EARLY the search of this move ends here: the move phase runs on the visits the root has -- re-rooting
// hands the siblings' subtrees back -- and the shortened search is counted (agz_stats, game header).  That needs a
// child to play: an expanded root with a visited board move (the soft pick normalises by the non-pass visits,
// mcts_play.jl:64-67), or any visited child once the pick is the arg-max.  Otherwise, and always with AGZ_POOL_STALL,
// the slot waits for the host (agz_slot_status / agz_slot_abandon); the other slots are not affected.
template <class W>
AGZ_FN bool pool_full_can_move(W& w, const View& V, int g) {
  const GameState& G = V.gs[g];
  if (G.err != AGZ_POOL_EXHAUSTED || V.pool_policy != AGZ_POOL_MOVE_EARLY) return false;
  const long ri = node_index(V, g, G.root);
  const NodeMeta rm = V.meta[ri];
  if (!(rm.flags & NF_EXPANDED)) return false;
  float s = 0.f;
  w.for_each(V.P, [&](int a) { s += V.childN[ri * V.AP + a]; });
  s = w.reduce_sum_f(s);
  // (under the move temperature every visited child has a weight, pass included, in either branch)
  const bool argmax = V.two_player || V.mt_on != 0 || rm.n >= V.tau;
  return s > 0.f || (argmax && V.childN[ri * V.AP + V.P] > 0.f);
}

// Playout cap randomization (View::cap_fast > 0): is the search of this game's root of ply n a full one?  The coin is
// a function of (seed, game, n) alone, so the move phase that ends a search asks again what the phase that began it
// was told.  Off: every search is full.
AGZ_FN bool playout_cap_full(const View& V, uint64_t game_id, int n) {
  if (V.cap_fast <= 0) return true;
  return agz_u01(agz_draw_u64(V.seed, game_id, (uint32_t)n, AGZ_SITE_PLAYOUT_CAP, 0)) < V.cap_full_prob;
}

// Is the search of self-play game G's root of ply root_n a full one?  The bench stagger's short first search keeps its
// own budget and counts as full, whatever its coin.
AGZ_FN bool full_search(const View& V, const GameState& G, int root_n) {
  return G.short_first || playout_cap_full(V, G.game_id, root_n);
}

AGZ_FN bool forced_search(const View& V, const GameState& G, int root_n) {
  if (!(V.forced_k > 0.0) || V.arena || V.analysis) return false;
  if (G.phase == G_MANUAL) return true;
  return full_search(V, G, root_n);
}


// ------------------------------------------------------------------ Gumbel root search
// "Policy improvement by planning with Gumbel" (Danihelka et al., ICLR 2022) at the root of a full self-play search
// (View::gumbel_m = m > 0).  THE DEFINITIONS, for the root with rows N, W, P, tp = to_play, position.n =
// n_root, and a legal action a:
//   logit(a) = agz_log((double)P[a]) when P[a] > 0, else -1.0e30
//   g(a)     = -agz_log(-agz_log(agz_u01(agz_draw_u64(seed, game_id, n_root, AGZ_SITE_GUMBEL, a))))
//   qs(a)    = the f32 (W[a] / (1.0f + N[a])) * tp of action_score.  incorporate initialises every child's W to the
//              parent's value, so an unvisited child's qs is the root's own network value: the "completed Q"
//   sigma(a) = ((c_visit + (double)maxN) * c_scale) * (0.5 + 0.5 * (double)qs(a)),  maxN = max of N[.] over all A
//              actions; f64, in this order
//   s(a)     = (g(a) + logit(a)) + sigma(a)
// BEGIN (the first select phase with the root expanded and the slot's state not this root's): n = G.target - G.rootN;
// the survivors are the m_0 = min(m, #legal) legal actions with the largest g + logit, ties to the lower action, stored
// in that order; P = the smallest integer >= 1 with 2^P >= m_0.  PHASES: phase p with m_p survivors ends when G.rootN
// reaches its start plus Q_p = max(1, floor(n / (P m_p))) m_p, cut to what remains of n; reverted duplicates do not
// count.  HALVE (start of a select phase, phase over, budget left): order the survivors by s descending, ties to the
// lower action, keep the first m_{p+1} = max(2, floor(m_p / 2)) (1 if m_p = 1).  ROOT LEVEL of a descent: after the
// pass-first rule, the survivor with the smallest child_N, visits in flight included, the first in stored order on ties;
// no score, no tie draw.  Below the root: PUCT, unchanged.  A select phase stops collecting at the phase end.
// MOVE: the survivor with the largest s, ties to the lower action.  TARGET: gumbel_pi.  No Dirichlet noise.
constexpr double kGumbelNoLogit = -1.0e30;

// Is the search of game slot g's root a Gumbel search?  forced_search's test: self-play full searches only (every search
// with the playout cap off); fast searches, the arena, analysis, review and single trees (G_MANUAL) never.
AGZ_FN bool gumbel_search(const View& V, const GameState& G, int root_n) {
  if (V.gumbel_m <= 0 || V.arena || V.analysis || G.phase == G_MANUAL) return false;
  return full_search(V, G, root_n);
}

AGZ_FN double gumbel_logit(float p) { return p > 0.0f ? agz_log((double)p) : kGumbelNoLogit; }

AGZ_FN double gumbel_g(const View& V, uint64_t game_id, int n_root, int a) {
  return -agz_log(-agz_log(agz_u01(agz_draw_u64(V.seed, game_id, (uint32_t)n_root, AGZ_SITE_GUMBEL, (uint64_t)a))));
}

AGZ_FN double gumbel_sigma(const View& V, long ni, int a, float tp, float maxN) {
  const float denom = 1.0f + V.childN[ni * V.AP + a];
  const float q = V.childW[ni * V.AP + a] / denom;
  const float qs = q * tp;
  return ((V.gumbel_cvisit + (double)maxN) * V.gumbel_cscale) * (0.5 + 0.5 * (double)qs);
}

template <class W>
AGZ_FN float row_max_N(W& w, const View& V, long ni) {
  float mx = 0.f;
  w.for_each(V.A, [&](int a) { const float c = V.childN[ni * V.AP + a]; mx = c > mx ? c : mx; });
  return w.reduce_max_f(mx);
}

AGZ_FN int gumbel_quota(int n, int P, int m) {
  const int per = n / (P * m);
  return (per < 1 ? 1 : per) * m;
}

// the end of a phase of m survivors that starts now
AGZ_FN float gumbel_phase_end(const GameState& G, int n, int P, int m) {
  const int left = (int)(G.target - G.rootN), q = gumbel_quota(n, P, m);
  return G.rootN + (float)(q < left ? q : left);
}

template <class W>
AGZ_FN void gumbel_begin(W& w, const View& V, Scratch& S, int g) {
  GameState& G = V.gs[g];
  GumbelState& T = V.gumbel[g];
  const long ri = node_index(V, g, G.root);
  const int A = V.A, n_root = V.meta[ri].n;
  int nlegal = 0;
  w.for_each(V.AP, [&](int a) {
    const bool lg = a < A && legal_bit(V, ri, a);
    S.flag[a] = lg;                                        // legal and not yet taken
    S.dbuf[a] = lg ? gumbel_g(V, G.game_id, n_root, a) + gumbel_logit(V.childP[ri * V.AP + a]) : 0.0;
    if (lg) nlegal++;
  });
  nlegal = w.reduce_sum(nlegal);
  w.sync();
  int m0 = V.gumbel_m < nlegal ? V.gumbel_m : nlegal;
  const double ninf = -__builtin_huge_val();
  for (int k = 0; k < m0; ++k) {
    double best = ninf;
    w.for_each(A, [&](int a) { if (S.flag[a] && S.dbuf[a] > best) best = S.dbuf[a]; });
    best = w.reduce_max(best);
    int idx = kIntMax;
    w.for_each(A, [&](int a) { if (S.flag[a] && S.dbuf[a] == best && a < idx) idx = a; });
    idx = w.reduce_min(idx);
    w.sync();
    if (idx >= A) { m0 = k; break; }                       // (a NaN prior: nothing compares equal to the maximum)
    if (w.leader()) { S.flag[idx] = 0; T.act[k] = (int16_t)idx; }
    w.sync();
  }
  if (m0 < 1) {                                            // (every prior NaN: search the pass alone)
    if (w.leader()) T.act[0] = (int16_t)V.P;
    m0 = 1;
  }
  int P = 1;
  while ((1 << P) < m0) ++P;
  const int n = (int)(G.target - G.rootN);
  if (w.leader()) {
    T.n = n_root; T.cnt = m0; T.budget = n; T.P = P;
    T.end = gumbel_phase_end(G, n, P, m0);
  }
  w.sync();
  w.count(&V.counters[CT_GUMBEL_BEGUN], 1);
}

// s(a) of survivor i into S.dbuf[i], i < cnt; returns the largest
template <class W>
AGZ_FN double gumbel_scores(W& w, const View& V, Scratch& S, int g) {
  const GameState& G = V.gs[g];
  const GumbelState& T = V.gumbel[g];
  const long ri = node_index(V, g, G.root);
  const int n_root = V.meta[ri].n;
  const float tp = (float)V.meta[ri].to_play;
  const float maxN = row_max_N(w, V, ri);
  double best = -__builtin_huge_val();
  w.sync();
  w.for_each(T.cnt, [&](int i) {
    const int a = T.act[i];
    const double s = (gumbel_g(V, G.game_id, n_root, a) + gumbel_logit(V.childP[ri * V.AP + a])) +
                     gumbel_sigma(V, ri, a, tp, maxN);
    S.dbuf[i] = s;
    if (s > best) best = s;
  });
  best = w.reduce_max(best);
  w.sync();
  return best;
}

template <class W>
AGZ_FN void gumbel_halve(W& w, const View& V, Scratch& S, int g) {
  GameState& G = V.gs[g];
  GumbelState& T = V.gumbel[g];
  const int cnt = T.cnt, half = cnt / 2;
  const int keep = cnt == 1 ? 1 : (half > 2 ? half : 2);
  gumbel_scores(w, V, S, g);
  w.for_each(cnt, [&](int i) {                             // rank by s descending, the lower action first on ties
    const double s = S.dbuf[i];
    const int a = T.act[i];
    int rank = 0;
    for (int j = 0; j < cnt; ++j) {
      const double sj = S.dbuf[j];
      const int aj = T.act[j];
      if (sj > s || (sj == s && aj < a)) rank++;
    }
    S.label[rank] = a;
  });
  w.sync();
  w.for_each(keep, [&](int i) { T.act[i] = (int16_t)S.label[i]; });
  if (w.leader()) { T.cnt = keep; T.end = gumbel_phase_end(G, T.budget, T.P, keep); }
  w.sync();
  w.count(&V.counters[CT_GUMBEL_HALVED], 1);
}

// The start of a select phase of a Gumbel search: begin, or halve, when due.  Returns whether the slot's state is set
// up for this root (an unexpanded root has none yet: its descents end at the root).
template <class W>
AGZ_FN bool gumbel_select_start(W& w, const View& V, Scratch& S, int g) {
  const GameState& G = V.gs[g];
  const long ri = node_index(V, g, G.root);
  if (!(V.meta[ri].flags & NF_EXPANDED)) return false;
  const GumbelState& T = V.gumbel[g];
  if (T.n != V.meta[ri].n) gumbel_begin(w, V, S, g);
  else if (!(G.rootN < T.end) && T.end < G.target) gumbel_halve(w, V, S, g);
  return true;
}

// the root action of the next descent
AGZ_FN int gumbel_root_pick(const View& V, int g) {
  const GumbelState& T = V.gumbel[g];
  const float* cN = V.childN + node_index(V, g, V.gs[g].root) * V.AP;
  int pick = T.act[0];
  float best = cN[pick];
  for (int i = 1; i < T.cnt; ++i) {
    const int a = T.act[i];
    const float c = cN[a];
    if (c < best) { best = c; pick = a; }
  }
  return pick;
}

// the move of a Gumbel search: the survivor with the largest s, the lower action on ties
template <class W>
AGZ_FN int gumbel_move(W& w, const View& V, Scratch& S, int g) {
  const GumbelState& T = V.gumbel[g];
  const double best = gumbel_scores(w, V, S, g);
  int idx = kIntMax;
  w.for_each(T.cnt, [&](int i) { const int a = T.act[i]; if (S.dbuf[i] == best && a < idx) idx = a; });
  idx = w.reduce_min(idx);
  w.sync();
  return idx < V.A ? idx : T.act[0];                       // (NaN scores: nothing compares equal to the maximum)
}

// The improved policy of node row ri into out[A] under V.gumbel_cvisit / V.gumbel_cscale: over legal a,
// x(a) = logit(a) + sigma(a), out[a] = (float)(agz_exp(x(a) - max x) / sum), the f64 sum over S.dbuf in ascending index
// order; illegal actions get 0; no squash.
template <class W>
AGZ_FN void gumbel_pi(W& w, const View& V, Scratch& S, long ri, float* out) {
  const int A = V.A;
  const float tp = (float)V.meta[ri].to_play;
  const float maxN = row_max_N(w, V, ri);
  double mx = -__builtin_huge_val();
  w.sync();
  w.for_each(A, [&](int a) {
    if (!legal_bit(V, ri, a)) return;
    const double x = gumbel_logit(V.childP[ri * V.AP + a]) + gumbel_sigma(V, ri, a, tp, maxN);
    S.dbuf[a] = x;
    if (x > mx) mx = x;
  });
  mx = w.reduce_max(mx);
  w.for_each(A, [&](int a) { S.dbuf[a] = legal_bit(V, ri, a) ? agz_exp(S.dbuf[a] - mx) : 0.0; });
  w.sync();
  double s = 0.0;
  for (int a = 0; a < A; ++a) s += S.dbuf[a];   // fixed ascending order on every lane
  w.for_each(A, [&](int a) { out[a] = (float)(S.dbuf[a] / s); });
  w.sync();
}

// ------------------------------------------------------------------ the player's methods, once for every driver
// MCTSPlayer's play_move!, should_resign, suggest_move and is_done (mcts_play.jl:26-50, :124, :144-151, :120): self-play
// (game_*), the evaluate() arena (arena_*), analysis / review (analysis_* / review_*) and tree_op are loops over these.

// Q(root) (mcts.jl:96-102 on the DummyNode entries): Float32
AGZ_FN float root_q(const GameState& G) { return G.rootW / (1.0f + G.rootN); }

// should_resign: Q_perspective(root) < resign_threshold (mcts_play.jl:124) -- the Float32 Q from the side to move,
// widened for the comparison with the Float64 threshold
AGZ_FN bool should_resign(const View& V, int g) {
  const GameState& G = V.gs[g];
  const float qp = root_q(G) * (float)V.meta[node_index(V, g, G.root)].to_play;
  return (double)qp < G.resign_threshold;
}

// suggest_move's budget (mcts_play.jl:145-146): `budget` more visits of the root, and the slot searches
template <class W>
AGZ_FN void search_budget(W& w, GameState& G, int budget) {
  if (w.leader()) { G.target = G.rootN + (float)budget; G.phase = G_SEARCH; }
}

// Begin the search of self-play game g's root `node`: root_explore (Dirichlet noise, selfplay.jl:23) unless the search is fast or a
// Gumbel search, which gets none, and the budget: R more root visits, cap_fast for a fast search.
template <class W>
AGZ_FN void search_begin(W& w, const View& V, Scratch& S, int g, int node, bool full) {
  if (full && V.gumbel_m <= 0) root_explore(w, V, S, g, node);
  search_budget(w, V.gs[g], full ? V.R : V.cap_fast);
}

// Is the search of slot g over: its budget spent, or the pool full and the game able to move early?  Sets G.stalled,
// what agz_stats.stalled_games / agz_slot_status report: the pool is full and the slot cannot move (AGZ_POOL_STALL: it
// waits for agz_slot_abandon).  (The arena asks in game_post and looks at the target alone: it never moves early.)
template <class W>
AGZ_FN bool search_over(W& w, const View& V, int g) {
  GameState& G = V.gs[g];
  const bool full = G.err == AGZ_POOL_EXHAUSTED;
  const bool over = !(G.rootN < G.target) || pool_full_can_move(w, V, g);
  if (w.leader()) G.stalled = full && !over;
  w.sync();
  return over;
}

// the pi row a ply's record gets (play_move): none; all zero (a fast search, the arena); children_as_pi of the visits;
// pruned_pi (counts CT_PRUNED_ROWS where pruning changed the row); gumbel_pi
enum PiRow : int { kPiNone = 0, kPiZero, kPiVisits, kPiPruned, kPiGumbel };

// play_move!(player, a) (mcts_play.jl:26-50), in the reference's order: record the ply -- the pi row `kind` at index
// G.move_count (length(searches_pi)), with `qs` the move and q at index G.nqs (length(qs)) -- then find or create the
// root's child for `a`, re-root on it (the dropped siblings go to the garbage stack) and advance move_count with `plies`,
// nqs with `qs`.  Returns the child, or what node_create_child returned (-2 too for an action out of range, before
// anything is written).  A failed play leaves both counts where they were, so the row it stored lies past the end of the
// record (the reference's push!, catch, pop!) until the slot's next play overwrites it; what follows is the caller's.
// clk: the phase clock of self-play's move phase (timing builds).
template <class W>
AGZ_FN int play_move(W& w, const View& V, Scratch& S, int g, int a, float q, int kind, bool plies, bool qs,
                     unsigned long long* clk = nullptr) {
  GameState& G = V.gs[g];
  if (a < 0 || a >= V.A) return -2;
  const int root = G.root, mgl = V.max_game_length;
  const long ri = node_index(V, g, root);
  const int k = G.move_count, kq = G.nqs;
  if (kind != kPiNone && k < mgl) {
    float* row = V.rec_pi + ((long)g * mgl + k) * V.A;
    const bool squash = V.meta[ri].n <= V.tau;
    if (kind == kPiZero) {
      w.for_each(V.A, [&](int i) { row[i] = 0.f; });
    } else if (kind == kPiGumbel) {
      gumbel_pi(w, V, S, ri, row);
    } else if (kind == kPiPruned) {                          // the forced playouts do not belong in the target
      if (pruned_pi(w, V, S, ri, G.rootN, squash, row)) w.count(&V.counters[CT_PRUNED_ROWS], 1);
    } else {
      children_as_pi(w, V, S, ri, squash, row);
    }
  }
  if (qs && kq < mgl && w.leader()) {
    V.rec_moves[(long)g * mgl + kq] = (int16_t)a;
    V.rec_q[(long)g * mgl + kq] = q;
  }
  w.sync();
  AGZ_STAMP_AT(w, V, CT_T_PICK, clk);
  int child = V.child[ri * V.AP + a];
  if (child < 0) child = node_create_child(w, V, S, g, root, a);
  if (child < 0) return child;
  AGZ_STAMP_AT(w, V, CT_T_CHILD, clk);
  reroot(w, V, S, g, a, child);
  if (w.leader()) { if (plies) G.move_count = k + 1; if (qs) G.nqs = kq + 1; }
  w.sync();
  return child;
}

// The selfplay.jl:22-43 loop body between two readout phases, for a game whose budget is spent:
// resign check -> pick -> play (record pi and Q, re-root) -> done check -> noise for the next move.
template <class W>
AGZ_FN void game_move_phase(W& w, const View& V, Scratch& S, int g) {
  GameState& G = V.gs[g];
  const NodeMeta rm = V.meta[node_index(V, g, G.root)];
  w.count_max(&V.counters[CT_PEAK_NODES], (unsigned long long)G.nodes_used);
  const bool early = G.rootN < G.target;          // only game_pre's full-pool rule sends a game here before its budget is spent
  if (early) {
    w.count(&V.counters[CT_POOL_SHORT], 1);
    if (w.leader()) { G.short_searches = G.short_searches + 1; G.err = 0; }
    w.sync();
  }
  if (should_resign(V, g)) { game_finish(w, V, S, g, -rm.to_play, 1, 0.f); return; }
  AGZ_STAMP_BEGIN(w);
  // a fast search (playout cap) leaves no policy target: its row is all zero
  const bool fast = !full_search(V, G, rm.n);
  const bool gumbel = V.gumbel_m > 0 && !fast;       // the search that ends here was a Gumbel search
  int a = V.P;
  if (gumbel && V.gumbel[g].n == rm.n) {             // (state never set up: the pool filled before the root was expanded)
    a = gumbel_move(w, V, S, g);
  } else if (pick_move(w, V, S, g, &a) != AGZ_OK) {
    a = V.P;  // the reference dies on its assertion; we pass
  }
  if (V.cap_fast > 0) w.count(&V.counters[fast ? CT_CAP_FAST : CT_CAP_FULL], 1);
  const int kind = fast ? kPiZero : gumbel ? kPiGumbel : (V.forced_prune && V.forced_k > 0.0) ? kPiPruned : kPiVisits;
  const int child = play_move(w, V, S, g, a, root_q(G), kind, true, true, &agz_t_prev);
  if (child < 0) { game_finish(w, V, S, g, 0, 0, 0.f); return; }      // the pool cannot hold the child: the game is void
  if (!G.short_first) w.count(&V.counters[CT_POSITIONS], 1);
  w.sync();
  if (w.leader()) G.short_first = 0;
  w.sync();
  AGZ_STAMP(w, V, CT_T_REROOT);
  if (node_is_done(V, g, child)) {
    const float sc = position_score(w, V, S, g, child);
    game_finish(w, V, S, g, result_of(sc), 0, sc);
    return;
  }
  search_begin(w, V, S, g, child, playout_cap_full(V, G.game_id, V.meta[node_index(V, g, child)].n));
  w.sync();
  AGZ_STAMP(w, V, CT_T_NOISE);
}

// Record which boards feed the eight history planes of leaf `k` (features.jl:8-14): path
// nodes newest first, then the game's history ring, then "repeat the oldest available".
template <class W>
AGZ_FN void record_leaf(W& w, const View& V, Scratch& S, int g, int k, int leaf, int plen) {
  const GameState& G = V.gs[g];
  const long li = (long)g * V.par + k;
  const int d = plen - 1;   // path[0] is the root when the descent started there
  int avail = d + G.hist_len;
  if (avail > 7) avail = 7;
  w.for_each(8, [&](int s) {
    const int t = s <= avail ? s : avail;
    V.leaf_featsrc[li * 8 + s] = t <= d ? S.path[d - t] : -(t - d - 1) - 1;
  });
  w.for_each(plen, [&](int i) { V.leaf_path[li * V.maxd + i] = S.path[i]; });
  if (w.leader()) {
    V.leaf_node[li] = leaf;
    V.leaf_plen[li] = plen;
    V.leaf_tp[li] = V.meta[node_index(V, g, leaf)].to_play;
    // e = ordinal of this evaluation among all the game has sent to the network, counted whether or not a symmetry
    // mode is on, so that switching the mode mid-game leaves the draw key of later evaluations what it would have been
    const int e = V.eval_ord[g];
    V.eval_ord[g] = e + 1;
    if (V.symmetry) {
      // the transform this evaluation is made under (DESIGN.md "Board symmetries"): fixed, or the e-th draw of the game
      V.leaf_sym[li] = (int8_t)(V.symmetry <= 8 ? V.symmetry - 1
                                                 : (int)agz_index(agz_draw_u64(V.seed, G.game_id, 0, AGZ_SITE_SYMMETRY,
                                                                               (uint64_t)e), 8u));
    }
  }
  w.sync();
}

// One tree_search! select phase (mcts_play.jl:73-87): up to `par` leaves, `2*par` attempts.
template <class W>
AGZ_FN void game_select_phase(W& w, const View& V, Scratch& S, int g, int par, bool defer = false) {
  GameState& G = V.gs[g];
  int nleaves = 0, failsafe = 0, terminal = 0;
  const float n_before = G.rootN;
  // (G.err says what THIS select phase ran into: a refused allocation of an earlier phase must not shorten a later search --
  // the tree may have been re-rooted, or its garbage released, since)
  if (w.leader()) { G.npend = 0; G.err = 0; }
  w.sync();
  // one decision per phase: the root does not change inside it
  const bool forced = V.forced_k > 0.0 && forced_search(V, G, V.meta[node_index(V, g, G.root)].n);
  // Gumbel root search: begin or halve as due; then the caller's root action per descent, up to the phase end
  bool gumbel = false;
  if (V.gumbel_m > 0 && gumbel_search(V, G, V.meta[node_index(V, g, G.root)].n)) gumbel = gumbel_select_start(w, V, S, g);
  while (nleaves < par && failsafe < 2 * par && (!gumbel || G.rootN < V.gumbel[g].end)) {
    failsafe++;
    int plen = 0;
    const int leaf = select_leaf(w, V, S, g, G.root, &plen, defer, forced, gumbel ? gumbel_root_pick(V, g) : -1);
    if (node_is_done(V, g, leaf)) {
      const float value = (float)result_of(position_score(w, V, S, g, leaf));
      path_backup(w, V, g, S.path, plen, value);
      terminal++;
      continue;
    }
    path_virtual_loss(w, V, g, S.path, plen, +1);
    record_leaf(w, V, S, g, nleaves, leaf, plen);
    nleaves++;
  }
  if (w.leader()) G.nleaves = nleaves;
  w.sync();
  w.count(&V.counters[CT_TERMINAL], (unsigned long long)terminal);
  w.count(&V.counters[CT_EVALS], (unsigned long long)nleaves);
  w.count(&V.counters[CT_ROOTVISITS], (unsigned long long)(G.rootN - n_before));
}

// ---------------------------------------------------------------- evaluate() arena ----
// neural_net.jl:103-158 for many games at once.  Slots come in pairs: slot 2i is the Black
// player of game i (network 0), slot 2i+1 the White player (network 1), each with its own tree
// (`black` / `white` MCTSPlayers, two_player_mode: arg-max picks, no noise, no pi).  The side to
// move searches; when its budget is spent it moves at the END of k_post and publishes the move in
// the pair's mailbox; the partner reads the mailbox at the START of the next k_pre, plays the same
// move on its tree and takes over.  Writer and reader therefore always run in different kernel
// launches: no intra-kernel communication, deterministic.

// arena mailbox words of a slot pair: ar_hdr[4 * pair .. +3] = {local game index, plies played, done, result};
// after the (games/2 + 1) headers, one abort word per pair = 1 + local game index of a game one side had to drop
constexpr int kArenaWordsPerPair = 5;
AGZ_FN int32_t* arena_abort_word(const View& V, int pair) { return V.ar_hdr + 4 * (V.games / 2 + 1) + pair; }

template <class W>
AGZ_FN void arena_finish(W& w, const View& V, Scratch& S, int g, bool emit, int winner, int was_resign) {
  GameState& G = V.gs[g];
  // `result(black.root.position)` (:147) is the Tromp-Taylor result of the final position
  if (emit) game_finish(w, V, S, g, winner, was_resign, position_score(w, V, S, g, G.root));
  if (w.leader()) { G.phase = G_IDLE; G.arena_k = G.arena_k + 1; G.nleaves = 0; }
  w.sync();
}

template <class W>
AGZ_FN void arena_start(W& w, const View& V, Scratch& S, int g, uint64_t index) {
  GameState& G = V.gs[g];
  const int k = G.arena_k;
  game_start(w, V, S, g, 2 * index + (uint64_t)(g & 1), index);
  // the player whose colour is to move searches first: `num_move % 2` (:118-119) on the empty start is Black, slot
  // parity 0; a start from the table may have White to move
  int waits = g & 1;
  if (V.st_count > 0) waits = (g & 1) != (V.meta[node_index(V, g, G.root)].to_play == 1 ? 0 : 1);
  if (w.leader()) {
    G.arena_k = k;
    G.resign_disabled = 0;
    G.resign_threshold = V.resign_threshold;     // MCTSPlayer default, evaluate passes none (:110-111)
    if (waits) G.phase = G_ARENA_WAIT;
  }
  if (!waits) search_budget(w, G, V.R);            // :121-126, root not pre-expanded
  w.sync();
}

// play_move!(active, move) (:138) and, with the partner's move, play_move!(inactive, move) (:139) on this slot's tree:
// two_player_mode records no pi, so the ply's row is all zero
template <class W>
AGZ_FN bool arena_apply(W& w, const View& V, Scratch& S, int g, int a, float q) {
  return play_move(w, V, S, g, a, q, kPiZero, true, true) >= 0;
}

// the pair's mailbox: this slot's game, its plies played, whether the game is over and how (arena_pre reads it)
template <class W>
AGZ_FN void arena_publish(W& w, const View& V, int g, int done, int result) {
  const GameState& G = V.gs[g];
  int32_t* hdr = V.ar_hdr + 4 * (g >> 1);
  if (w.leader()) { hdr[0] = G.arena_k; hdr[1] = G.move_count; hdr[2] = done; hdr[3] = result; }
  w.sync();
}

template <class W>
AGZ_FN void arena_pre(W& w, const View& V, Scratch& S, int g) {
  GameState& G = V.gs[g];
  const int pair = g >> 1, npairs = V.games >> 1;
  if (G.phase == G_MANUAL || G.phase == G_RETIRED) {
    if (w.leader()) G.nleaves = 0;
    w.sync();
    return;
  }
  if (G.phase == G_IDLE) {
    if (w.leader()) G.nleaves = 0;
    w.sync();
    const long long idx = (long long)pair + (long long)G.arena_k * npairs;    // both slots derive the same sequence
    if (V.total_games > 0 && idx >= V.total_games) {
      if (w.leader()) G.phase = G_RETIRED;
      w.sync();
      return;
    }
    arena_start(w, V, S, g, V.id_base + (uint64_t)idx * V.id_stride);
  }
  if (G.phase == G_ARENA_WAIT) {
    if (w.leader()) G.nleaves = 0;
    w.sync();
    const int32_t* hdr = V.ar_hdr + 4 * pair;
    const int hk = hdr[0], hply = hdr[1], hdone = hdr[2], hres = hdr[3];
    if (hk != G.arena_k) return;                            // nothing published for this game yet
    if (hply > G.move_count) {
      const long pg = (long)(g ^ 1) * V.max_game_length + G.move_count;
      const int a = V.rec_moves[pg];
      const float q = V.rec_q[pg];
      if (!arena_apply(w, V, S, g, a, q)) {
        // node pool exhausted while following the partner's move: the partner is parked in G_ARENA_WAIT for
        // this slot's reply and would wait forever.  Raise the pair's abort word; the partner reads it in
        // k_post (a different launch, so still no intra-kernel communication) and files the game as void.
        if (w.leader()) arena_abort_word(V, pair)[0] = G.arena_k + 1;
        w.sync();
        arena_finish(w, V, S, g, false, 0, 0);
        return;
      }
    } else if (!hdone) {
      return;
    }
    if (hdone) {                                            // set_result!(inactive, ...) (:131,144)
      if (w.leader()) { G.result = (hres & 3) - 1; G.was_resign = hres >> 2; }
      w.sync();
      arena_finish(w, V, S, g, false, 0, 0);
      return;
    }
    search_budget(w, G, V.R);                               // :121-126
    w.sync();
  }
  if (G.phase == G_SEARCH) game_select_phase(w, V, S, g, V.par, V.defer_expand != 0);
}

// the active player's budget is spent: :128-146
template <class W>
AGZ_FN void arena_move_phase(W& w, const View& V, Scratch& S, int g) {
  GameState& G = V.gs[g];
  if (should_resign(V, g)) {                                // should_resign(active) (:129-133)
    const int winner = -V.meta[node_index(V, g, G.root)].to_play;
    arena_publish(w, V, g, 1, (winner + 1) | 4);
    arena_finish(w, V, S, g, true, winner, 1);
    return;
  }
  int a = V.P;
  if (pick_move(w, V, S, g, &a) != AGZ_OK) a = V.P;
  if (!arena_apply(w, V, S, g, a, root_q(G))) {             // the pool cannot hold the child: the game is void
    arena_publish(w, V, g, 1, 1);
    arena_finish(w, V, S, g, true, 0, 0);
    return;
  }
  w.count(&V.counters[CT_POSITIONS], 1);
  if (node_is_done(V, g, G.root)) {                         // :140-145
    const int winner = result_of(position_score(w, V, S, g, G.root));
    arena_publish(w, V, g, 1, winner + 1);
    arena_finish(w, V, S, g, true, winner, 0);
    return;
  }
  if (w.leader()) G.phase = G_ARENA_WAIT;
  arena_publish(w, V, g, 0, 0);
}

// ---------------------------------------------------------------- analysis lines ----
// The top-K candidates of a node and the principal variation (PV) behind each: most_visited_path, mvp_gg and describe
// of mcts.jl:255-327 (commented out there; their text is the definition).  Every value is an exact read of a stored
// row, no arithmetic, so a host walk over the same rows gives the same bits.  For a node X:
//   * candidates of X: the actions a with child_N[a] > 0, by child_N descending, then child_prior descending, then a
//     ascending; the first K are the lines.  (describe sorts by the action score second; the prior is a stored value.)
//   * PV of candidate a, depth limit D >= 1, min_visits >= 1: pv[0] = a, c = child[X][a].  While len < D and c is a
//     node: m = max of c's child_N; stop if m < min_visits; b = the lowest action with child_N == m (findmax, no draw);
//     append b; c = child[c][b].  min_visits 1 is most_visited_path, 2 is mvp_gg (maximum(child_N) > 1).
//   * pv_N[d] = the child_N entry pv[d] was chosen by.  Per line: the candidate's N, W, prior at X, end_W = the child_W
//     entry of the last PV move, pv_len.
//   * unused line slots: move -1, pv_len 0, floats 0; pv beyond pv_len: -1, pv_N 0.
// The walk is level by level over groups of up to four lines: at one depth the group's rows are requested together
// (R = ceil(A / 64) values per lane and line), then reduced, so a group costs about two dependent memory round trips
// per level (the rows; then child / child_W of the chosen entries) whatever its size.

constexpr int kLineGroup = 4;

// One wave item per lane slot l (for_each over kWave: a lane of the GPU wave takes exactly its own l), R row entries
// a = l + 64 r each; per-slot partials are combined by the reductions below.
// The best untaken candidate of node row xi: (child_N, child_prior, a) in the candidate order, or -1 when none is left.
template <int R, class W>
AGZ_FN int lines_next_candidate(W& w, const View& V, const Scratch& S, long xi) {
  const int A = V.A;
  const float ninf = -__builtin_huge_valf();
  float bn = ninf, bp = ninf;
  int bi = kIntMax;
  w.for_each(kWave, [&](int l) {
    float vn[R], vp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {                     // both rows first (clamped, not predicated), then the compares
      const int a = l + kWave * r, aa = a < A ? a : A - 1;
      vn[r] = V.childN[xi * V.AP + aa];
      vp[r] = V.childP[xi * V.AP + aa];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int a = l + kWave * r;
      const float n = vn[r], p = vp[r];
      const bool open = (a < A) & !S.flag[a < A ? a : 0] & (n > 0.0f);      // (& and |: nothing short-circuits a load)
      const bool better = (n > bn) | ((n == bn) & ((p > bp) | ((p == bp) & (a < bi))));
      if (open & better) { bn = n; bp = p; bi = a; }
    }
  });
  const float mn = w.reduce_max_f(bn);
  const float mp = w.reduce_max_f(bn == mn ? bp : ninf);
  const int idx = w.reduce_min(bn == mn && bp == mp ? bi : kIntMax);
  return idx == kIntMax ? -1 : idx;
}

// One PV level of a group: m[j] = max of child_N row[j], b[j] = its lowest action.  Every row is a valid node row (a
// finished line passes any; its result is ignored), so all loads are issued before the first value is used.
template <int R, class W>
AGZ_FN void lines_level(W& w, const View& V, const long (&row)[kLineGroup], float (&m)[kLineGroup], int (&b)[kLineGroup]) {
  const int A = V.A;
  const float ninf = -__builtin_huge_valf();
  float mx[kLineGroup];
  int ix[kLineGroup];
#pragma unroll
  for (int j = 0; j < kLineGroup; ++j) { mx[j] = ninf; ix[j] = kIntMax; }
  w.for_each(kWave, [&](int l) {
    float v[kLineGroup][R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int a = l + kWave * r, aa = a < A ? a : A - 1;
#pragma unroll
      for (int j = 0; j < kLineGroup; ++j) v[j][r] = V.childN[row[j] * V.AP + aa];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int a = l + kWave * r;
      if (a >= A) continue;
#pragma unroll
      for (int j = 0; j < kLineGroup; ++j) {
        const float c = v[j][r];
        if (c > mx[j] || (c == mx[j] && a < ix[j])) { mx[j] = c; ix[j] = a; }
      }
    }
  });
#pragma unroll
  for (int j = 0; j < kLineGroup; ++j) {
    m[j] = w.reduce_max_f(mx[j]);
    b[j] = w.reduce_min(mx[j] == m[j] ? ix[j] : kIntMax);
  }
}

template <int R, class W>
AGZ_FN void node_lines_rows(W& w, const View& V, Scratch& S, int g, int node, int K, int D, int min_visits,
                            agz_line* out, int16_t* pv, float* pv_N) {
  const long xi = node_index(V, g, node);
  const int AP = V.AP;
  const float need = (float)min_visits;
  w.for_each(AP, [&](int a) { S.flag[a] = 0; });           // the "taken" mask of the candidates
  w.for_each(K * D, [&](int i) { pv[i] = -1; pv_N[i] = 0.f; });
  w.for_each(K, [&](int k) {
    agz_line e;
    e.move = -1; e.pv_len = 0; e.N = 0.f; e.W = 0.f; e.prior = 0.f; e.end_W = 0.f;
    out[k] = e;
  });
  w.sync();
  bool more = true;
  for (int k0 = 0; k0 < K && more; k0 += kLineGroup) {
    agz_line ln[kLineGroup];
    int cur[kLineGroup];
#pragma unroll
    for (int j = 0; j < kLineGroup; ++j) {
      ln[j].move = -1; ln[j].pv_len = 0; ln[j].N = 0.f; ln[j].W = 0.f; ln[j].prior = 0.f; ln[j].end_W = 0.f;
      cur[j] = -1;
      if (k0 + j >= K || !more) continue;
      const int a = lines_next_candidate<R>(w, V, S, xi);
      if (a < 0) { more = false; continue; }
      ln[j].move = a; ln[j].pv_len = 1;
      ln[j].N = V.childN[xi * AP + a]; ln[j].W = V.childW[xi * AP + a]; ln[j].prior = V.childP[xi * AP + a];
      ln[j].end_W = ln[j].W;
      cur[j] = V.child[xi * AP + a];
      if (w.leader()) { S.flag[a] = 1; pv[(long)(k0 + j) * D] = (int16_t)a; pv_N[(long)(k0 + j) * D] = ln[j].N; }
      w.sync();
    }
    for (int d = 1; d < D; ++d) {
      long row[kLineGroup];
      bool live[kLineGroup], any = false;
#pragma unroll
      for (int j = 0; j < kLineGroup; ++j) {
        live[j] = cur[j] >= 0 && cur[j] < V.cap;
        row[j] = live[j] ? node_index(V, g, cur[j]) : xi;
        any = any || live[j];
      }
      if (!any) break;
      float m[kLineGroup];
      int b[kLineGroup];
      lines_level<R>(w, V, row, m, b);
#pragma unroll
      for (int j = 0; j < kLineGroup; ++j) {
        if (!live[j]) continue;
        if (m[j] < need) { cur[j] = -1; continue; }
        ln[j].pv_len = d + 1;
        ln[j].end_W = V.childW[row[j] * AP + b[j]];
        cur[j] = V.child[row[j] * AP + b[j]];
        if (w.leader()) { pv[(long)(k0 + j) * D + d] = (int16_t)b[j]; pv_N[(long)(k0 + j) * D + d] = m[j]; }
      }
    }
    if (w.leader()) {
#pragma unroll
      for (int j = 0; j < kLineGroup; ++j)
        if (ln[j].move >= 0) out[k0 + j] = ln[j];
    }
  }
  w.sync();
}

// the K lines of `node` of slot g into out [K], pv [K][D], pv_N [K][D] (all entries are written)
template <class W>
AGZ_FN void node_lines(W& w, const View& V, Scratch& S, int g, int node, int K, int D, int min_visits, agz_line* out,
                       int16_t* pv, float* pv_N) {
  with_row_width(V.A, [&](auto r) {
    node_lines_rows<decltype(r)::value>(w, V, S, g, node, K, D, min_visits, out, pv, pv_N);
  });
}

// ---------------------------------------------------------------- batched analysis ----
// suggest_move (mcts_play.jl:144-151) for caller positions i = 0..an_count-1, any number per slot (DESIGN.md "Batched
// analysis").  G_IDLE: claim the next index, install position i as the root with draw key (seed, an_id_base + i) and
// target R -- initialize_game! -- or retire the slot.  G_SEARCH: game_select_phase, i.e. tree_search!.  Budget spent, or
// a full pool under AGZ_POOL_MOVE_EARLY: pick_move, the row of position i in the result tables, back to G_IDLE.  No
// noise, no pre-expansion, no record, no re-rooting: the next install resets the pool.

// the result row of the slot's current search: position an_slot[g], or in review mode ply G.move_count of game an_slot[g]
AGZ_FN long long analysis_row(const View& V, int g) {
  const long long j = V.an_slot[g];
  return V.review ? V.rv_off[j] + V.gs[g].move_count : j;
}

// the row of a position or ply that was not searched: no move, `status`
AGZ_FN agz_analysis unsearched_row(int status) { return agz_analysis{-1, status, 0.f, 0.f, 0.f, 0}; }

// the slot is done with its position or game: idle, to claim the next one in analysis_pre
template <class W>
AGZ_FN void slot_idle(W& w, GameState& G) {
  if (w.leader()) { G.phase = G_IDLE; G.nleaves = 0; G.err = 0; G.stalled = 0; }
  w.sync();
}

// the slot's row of the result tables: the header, and the root's three A-wide rows in consecutive stores
template <class W>
AGZ_FN void analysis_finish(W& w, const View& V, Scratch& S, int g) {
  GameState& G = V.gs[g];
  const long long i = analysis_row(V, g);
  const long ri = node_index(V, g, G.root);
  int status = G.rootN < G.target ? AGZ_POOL_EXHAUSTED : AGZ_OK;     // only the full-pool rule ends a search early
  int a = -1;
  if (pick_move(w, V, S, g, &a) != AGZ_OK) { status = AGZ_ASSERT_SOFTPICK; a = -1; }
  const int A = V.A;
  w.for_each(A, [&](int k) {
    V.an_childN[i * A + k] = V.childN[ri * V.AP + k];
    V.an_childW[i * A + k] = V.childW[ri * V.AP + k];
    V.an_prior[i * A + k] = V.childP[ri * V.AP + k];
    if (V.an_childS) V.an_childS[i * A + k] = V.childS[ri * V.AP + k];
  });
  if (V.an_childS && w.leader()) V.an_rootS[i] = V.rootS[g];
  // reanalysis: the pi row the self-play move phase records at this root, under the same squash rule
  if (V.an_pi) children_as_pi(w, V, S, ri, V.meta[ri].n <= V.tau, V.an_pi + i * A);
  if (V.an_lines > 0) {                                 // (review mode: before review_play re-roots)
    const long long kd = (long long)V.an_lines * V.an_pv_depth;
    node_lines(w, V, S, g, G.root, V.an_lines, V.an_pv_depth, V.an_pv_min, V.an_line + i * V.an_lines, V.an_pv + i * kd,
               V.an_pvN + i * kd);
  }
  if (w.leader()) {
    agz_analysis r;
    r.move = a; r.status = status; r.N = G.rootN; r.W = G.rootW; r.Q = root_q(G);
    r.nodes_used = G.nodes_used;
    V.an_res[i] = r;
  }
  slot_idle(w, G);
  w.count(&V.an_ctr[1], 1);
}

// ---------------------------------------------------------------- batched game review ----
// play() (src/play.jl:25-77) over recorded games (DESIGN.md "Batched game review"): game j's ply k is suggest_move on the
// tree, then play_move!(player, m_k) with the recorded move, which re-roots the same tree.  The slot's ply is G.move_count.

// rows k .. n-1 of game j (k = G.move_count) get `status` and move -1 with nothing searched; the slot goes idle
template <class W>
AGZ_FN void review_give_up(W& w, const View& V, int g, int status) {
  GameState& G = V.gs[g];
  const long long j = V.an_slot[g];
  const long long r0 = V.rv_off[j] + G.move_count, r1 = V.rv_off[j + 1];
  w.for_each((int)(r1 - r0), [&](int t) { V.an_res[r0 + t] = unsearched_row(status); });
  w.sync();
  slot_idle(w, G);
  w.count(&V.an_ctr[1], (unsigned long long)(r1 - r0));
}

// Before ply k's search: the game is over (k = n), or m_k must be playable at the root -- legal there (legal_bit: an
// empty point, not the ko point, no suicide; a pass always) and the root not finished (two passes, max_game_length).  An
// invalid record gives up the rest of the game (rows k.. BAD_ARGUMENT).  Otherwise suggest_move's target.
template <class W>
AGZ_FN void review_next_ply(W& w, const View& V, int g) {
  GameState& G = V.gs[g];
  const long long j = V.an_slot[g];
  const long long off = V.rv_off[j], n = V.rv_off[j + 1] - off;
  if (G.move_count >= n) { slot_idle(w, G); return; }
  const int a = V.rv_moves[off + G.move_count];
  const long ri = node_index(V, g, G.root);
  if (node_is_done(V, g, G.root) || a < 0 || a > V.P || !legal_bit(V, ri, a)) {   // (arena records: no host check)
    review_give_up(w, V, g, AGZ_BAD_ARGUMENT);
    return;
  }
  search_budget(w, G, V.R);                                 // N(root) >= N0 + R
  if (w.leader()) G.stalled = 0;
  w.sync();
}

// play_move!(player, m_k) without the record -- the ply count alone advances -- then the next ply (the dropped siblings
// go to the garbage stack game_pre drains).  A child the full pool cannot hold is made room for by discarding the
// root's other subtrees first: the re-root drops them anyway, so the result is the unbounded tree's.
template <class W>
AGZ_FN void review_play(W& w, const View& V, Scratch& S, int g) {
  GameState& G = V.gs[g];
  const long long j = V.an_slot[g];
  const int a = V.rv_moves[V.rv_off[j] + G.move_count];
  const long ri = node_index(V, g, G.root);
  int child = play_move(w, V, S, g, a, 0.f, kPiNone, true, false);
  if (child == -1) {
    if (w.leader()) {
      for (int b = 0; b < V.A; ++b) {
        const int c = V.child[ri * V.AP + b];
        if (c < 0) continue;
        V.child[ri * V.AP + b] = -1;
        V.freelist[(long)g * V.cap + V.cap - G.garbage - 1] = c;
        G.garbage = G.garbage + 1;
      }
      G.err = 0;
    }
    w.sync();
    free_pending(w, V, S, g, V.cap);
    child = play_move(w, V, S, g, a, 0.f, kPiNone, true, false);
  }
  if (child < 0) {                                      // (a pool of fewer than two nodes)
    if (w.leader()) G.move_count = G.move_count + 1;
    w.sync();
    review_give_up(w, V, g, AGZ_POOL_EXHAUSTED);
    return;
  }
  if (w.leader()) G.err = 0;
  w.sync();
  review_next_ply(w, V, g);
}

// G_IDLE in review mode: claim game j, install its start (an invalid board gives up all its rows), ply 0
template <class W>
AGZ_FN void review_claim(W& w, const View& V, Scratch& S, int g, long long j) {
  GameState& G = V.gs[g];
  const agz_position_info info = V.an_info[j];
  if (w.leader()) V.an_slot[g] = j;
  w.sync();
  if (V.rv_off[j + 1] == V.rv_off[j]) return;          // no moves, no rows
  const bool ok = root_install(w, V, S, g, V.an_board + j * V.P, V.an_hist + j * 7 * V.P, info, G_SEARCH, true);
  if (w.leader()) {
    G.move_count = 0;
    if (ok) { G.game_id = V.an_gid ? V.an_gid[j] : V.an_id_base + (uint64_t)j; G.short_first = 0; }
  }
  w.sync();
  if (!ok) { review_give_up(w, V, g, AGZ_BAD_ARGUMENT); return; }
  review_next_ply(w, V, g);
}

template <class W>
AGZ_FN void analysis_pre(W& w, const View& V, Scratch& S, int g) {
  GameState& G = V.gs[g];
  if (G.phase == G_RETIRED) {
    if (w.leader()) G.nleaves = 0;
    w.sync();
    return;
  }
  if (G.phase == G_SEARCH && search_over(w, V, g)) {
    analysis_finish(w, V, S, g);
    if (V.review) review_play(w, V, S, g);
  }
  while (G.phase == G_IDLE) {
    if (w.leader()) G.nleaves = 0;
    w.sync();
    const long long i = (long long)w.fetch_add(&V.an_ctr[0], 1ull);
    if (i >= V.an_count) {
      if (w.leader()) G.phase = G_RETIRED;
      w.sync();
      return;
    }
    if (V.review) {
      review_claim(w, V, S, g, i);
      continue;
    }
    const agz_position_info info = V.an_info[i];
    if (!root_install(w, V, S, g, V.an_board + i * V.P, V.an_hist + i * 7 * V.P, info, G_SEARCH, true)) {
      if (w.leader()) V.an_res[i] = unsearched_row(AGZ_BAD_ARGUMENT);
      w.sync();
      w.count(&V.an_ctr[1], 1);
      continue;                                         // nothing searched: claim the next position in this k_pre
    }
    if (w.leader()) {
      V.an_slot[g] = i;
      G.game_id = V.an_id_base + (uint64_t)i;
      G.short_first = 0; G.stalled = 0;
    }
    search_budget(w, G, V.R);                           // suggest_move: N(root) >= N0 + num_readouts
    w.sync();
  }
  if (G.phase == G_SEARCH) game_select_phase(w, V, S, g, V.par, V.defer_expand != 0);
}

// Phase A+B of a self-play step for game slot g: lifecycle, per-move phase, select.
template <class W>
AGZ_FN void game_pre(W& w, const View& V, Scratch& S, int g) {
  GameState& G = V.gs[g];
  if (w.leader()) G.npend = 0;       // k_expand looks at every game, whether it selects this step or not
  AGZ_STAMP_BEGIN(w);
  const unsigned long long agz_t_start = agz_t_prev;
  (void)agz_t_start;
  if (G.garbage > 0 && G.phase != G_MANUAL) free_pending(w, V, S, g, kFreeBudget);
  AGZ_STAMP(w, V, CT_T_FREE);
  if (V.arena && G.phase != G_MANUAL) { arena_pre(w, V, S, g); return; }
  if (V.analysis && G.phase != G_MANUAL) { analysis_pre(w, V, S, g); return; }
  if (G.phase == G_MANUAL || G.phase == G_RETIRED) {
    if (w.leader() && G.phase == G_RETIRED) G.nleaves = 0;
    w.sync();
    return;
  }
  bool agz_moved = false;
  if (G.phase == G_SEARCH) {
    if (search_over(w, V, g)) { game_move_phase(w, V, S, g); agz_moved = true; }
  } else if (G.stalled) {
    if (w.leader()) G.stalled = 0;
    w.sync();
  }
  (void)agz_moved;
  AGZ_STAMP_BEGIN_AGAIN(w);
  if (G.phase == G_IDLE) {
    if (w.leader()) G.nleaves = 0;
    w.sync();
    if (V.hold) {
      // parked until the host releases the slot: train() trains between its games' finish and the next game's start
      const int32_t rel = V.released[g];
      w.sync();
      if (!rel) return;
      if (w.leader()) V.released[g] = 0;
      w.sync();
    }
    // claim the next global game index; retire the slot when the quota is used up
    const long long idx = (long long)w.fetch_add(&V.counters[CT_CLAIMED], 1ull);
    if (V.total_games > 0 && idx >= V.total_games) {
      if (w.leader()) G.phase = G_RETIRED;
      w.sync();
      return;
    }
    const uint64_t gid = V.id_base + (uint64_t)idx * V.id_stride;
    game_start(w, V, S, g, gid, gid);
  }
  if (G.phase == G_INIT) {
    // selfplay.jl:16-20: the very first select_leaf returns the unexpanded root; it is sent to
    // the network alone, without virtual loss, and incorporated with up_to = itself.
    int plen = 0;
    const int leaf = select_leaf(w, V, S, g, G.root, &plen);
    record_leaf(w, V, S, g, 0, leaf, plen);
    if (w.leader()) { G.nleaves = 1; G.phase = G_INIT_WAIT; }
    w.sync();
    w.count(&V.counters[CT_EVALS], 1);
    return;
  }
  if (G.phase == G_SEARCH) {
    game_select_phase(w, V, S, g, V.par, V.defer_expand != 0);
#ifdef AGZ_TIMING_EXPERIMENTS
    const unsigned long long t = w.clock();
    w.count(&V.counters[agz_moved ? CT_T_MOVE_SELECT : CT_T_SELECT], t - agz_t_prev);
    w.count(&V.counters[agz_moved ? CT_N_MOVE : CT_N_SELECT], 1);
    if (agz_moved) w.count_max(&V.counters[CT_T_MOVE_MAX], t - agz_t_start);
#endif
  }
}

// Phase C: revert virtual losses and incorporate the network outputs in collection order
// (mcts_play.jl:89-96), or finish the selfplay.jl:16-20 pre-expansion.
template <class W>
AGZ_FN void game_post(W& w, const View& V, Scratch& S, int g) {
  GameState& G = V.gs[g];
  const int nl = G.nleaves;
  if (V.arena && G.phase == G_ARENA_WAIT) {                 // the partner dropped this game in k_pre (pool exhausted)
    if (arena_abort_word(V, g >> 1)[0] == G.arena_k + 1) arena_finish(w, V, S, g, true, 0, 0);
    return;
  }
  if (V.arena && G.phase == G_SEARCH && nl <= 0) {          // a select phase of terminal leaves only
    if (!(G.rootN < G.target)) arena_move_phase(w, V, S, g);
    return;
  }
  if (nl <= 0 || (G.phase != G_SEARCH && G.phase != G_INIT_WAIT && G.phase != G_MANUAL)) return;
  for (int k = 0; k < nl; ++k) {
    const long li = (long)g * V.par + k;
    const int leaf = V.leaf_node[li], plen = V.leaf_plen[li];
    const long b = (long)G.leaf_base + k;
    const int32_t* path = V.leaf_path + li * V.maxd;
    if (G.phase != G_INIT_WAIT) path_virtual_loss(w, V, g, path, plen, -1);
    incorporate(w, V, g, leaf, V.pi + b * V.A, V.v[b], path, plen);
  }
  if (G.phase == G_INIT_WAIT) {
    search_begin(w, V, S, g, G.root, full_search(V, G, V.meta[node_index(V, g, G.root)].n));
    if (G.short_first) {            // the bench stagger: a short first search of its own budget
      const double u = agz_u01(agz_draw_u64(V.seed, G.game_id, 0, AGZ_SITE_STAGGER, 1000000u));
      search_budget(w, G, 1 + (int)(u * (double)(V.R - 1)));
    }
  }
  if (w.leader()) G.nleaves = 0;
  w.sync();
  // (the arena's "search over" is the target alone, here and above: search_over's full-pool rule is game_pre's)
  if (V.arena && G.phase == G_SEARCH && !(G.rootN < G.target)) arena_move_phase(w, V, S, g);
}

// Feature planes of one leaf slot into the stem-input layout [P][32] (features.jl:3-26)
// Sym: the planes of the leaf's position under T_s, s = V.leaf_sym[leaf] -- X'[plane][p] = X[plane][T_s^-1(p)]: the remap
// is on the read side, so the store pattern below is the same (Sym = false is the instantiation without symmetries)
template <bool Sym = false, class W>
// part / parts: this wave does the part-th of `parts` equal shares of the leaf's items (k_leaf_features gives a leaf four waves)
AGZ_FN void leaf_features(W& w, const View& V, int g, int k, float* x32, float* whcn, int part = 0, int parts = 1) {
  const long li = (long)g * V.par + k;
  const int tp = V.leaf_tp[li];
  const int P = V.P;
  int src[8];
  for (int s = 0; s < 8; ++s) src[s] = V.leaf_featsrc[li * 8 + s];
  int sinv = 0;
  if constexpr (Sym) sinv = sym_inverse(V.leaf_sym[li]);
  auto stone = [&](int s, int p) -> int {
    if constexpr (Sym) p = sym_point(sinv, V.N, p);
    return src[s] >= 0 ? V.board[node_index(V, g, src[s]) * V.PP + p] : V.hist[((long)g * 7 + (-src[s] - 1)) * V.PP + p];
  };
  if (x32) {
    // The stem input row of point p is 32 floats = eight 16-byte quads: quad c < 4 holds the planes of history boards
    // 2c and 2c + 1 (own / opponent stones each), quad 4 the colour plane, quads 5..7 the padding.  Item = (point, quad),
    // quad fastest: the 64 lanes of a wave write 1 KB of consecutive bytes per store instruction, and a lane reads the two
    // board bytes its quad needs instead of all eight.  (Round 6 tried, and timed, four things on this kernel -- this store
    // pattern against lane = point, four leaves per workgroup, four waves per leaf, streaming stores: 35-39 us per 8192
    // leaves of 9x9 every time, 0.3 of the HBM rate in bytes.  What it waits for is the chain leaf record -> eight node
    // boards scattered over a 14 GB pool -> store, three dependent round trips with a TLB miss each, not bandwidth.)
    struct alignas(16) Quad { float a, b, c, d; };
    Quad* dst = reinterpret_cast<Quad*>(x32);
    const int per = (P * 8 + parts - 1) / parts, lo = part * per, hi = lo + per < P * 8 ? lo + per : P * 8;
    w.for_each(hi - lo, [&](int j) {
      const int i = lo + j;
      const int p = i >> 3, c = i & 7;
      Quad q{0.f, 0.f, 0.f, 0.f};
      if (c < 4) {
        const int s0 = stone(2 * c, p), s1 = stone(2 * c + 1, p);
        q.a = s0 == tp ? 1.f : 0.f;
        q.b = s0 == -tp ? 1.f : 0.f;
        q.c = s1 == tp ? 1.f : 0.f;
        q.d = s1 == -tp ? 1.f : 0.f;
      } else if (c == 4) {
        q.a = (float)tp;
      }
      dst[i] = q;
    });
  }
  if (whcn) {
    const int per = (P + parts - 1) / parts, lo = part * per, hi = lo + per < P ? lo + per : P;
    w.for_each(hi - lo, [&](int j) {
      const int p = lo + j;
      for (int s = 0; s < 8; ++s) {
        const int c = stone(s, p);
        whcn[(long)P * (2 * s) + p] = c == tp ? 1.f : 0.f;
        whcn[(long)P * (2 * s + 1) + p] = c == -tp ? 1.f : 0.f;
      }
      whcn[(long)P * 16 + p] = (float)tp;
    });
  }
}


// ------------------------------------------------------------------ batched Go-rule entry points
// (agz_go_play / agz_go_legal / agz_go_score): one wave per position, no tree involved.

template <class W>
AGZ_FN void go_legal_one(W& w, const View& V, Scratch& S, const int8_t* board, int tp, int ko, int8_t* out) {
  w.for_each(V.P, [&](int p) { S.sb[p] = board[p]; });
  w.sync();
  label_components(w, V, S, true);
  group_liberties(w, V, S);
  compute_legal_flags(w, V, S, tp, ko);
  w.for_each(V.A, [&](int a) { out[a] = S.flag[a]; });
  w.sync();
}

// agz_go_keys: the key under `rule` of one position
template <class W>
AGZ_FN void go_key_one(W& w, const View& V, const int8_t* board, int tp, int rule, uint64_t* out) {
  const uint64_t k = board_key(w, V, board, tp, rule);
  if (w.leader()) *out = k;
  w.sync();
}

// agz_go_legal_seen: all_legal_moves under `rule` with the caller's seen set seen[0 .. cnt)
template <class W>
AGZ_FN void go_legal_seen_one(W& w, const View& V, Scratch& S, const int8_t* board, int tp, int ko, const uint64_t* seen,
                              int cnt, int rule, int8_t* out) {
  w.for_each(V.P, [&](int p) { S.sb[p] = board[p]; });
  w.sync();
  label_components(w, V, S, true);
  group_liberties(w, V, S);
  compute_legal_flags(w, V, S, tp, ko);
  if (rule != AGZ_KO_SIMPLE) {
    uint64_t* K = sk_keybuf(w, S);
    uint64_t* chunk = K + V.AP;
    sk_child_keys(w, V, S, K, tp, rule, board_key(w, V, S.sb, tp, rule));
    for (int at = 0; at < cnt; at += kSkChunk) {
      const int take = cnt - at < kSkChunk ? cnt - at : kSkChunk;
      w.for_each(take, [&](int i) { chunk[i] = seen[at + i]; });
      sk_strike(w, V, S, K, chunk, take);
    }
  }
  w.for_each(V.A, [&](int a) { out[a] = S.flag[a]; });
  w.sync();
}

template <class W>
AGZ_FN void go_play_one(W& w, const View& V, Scratch& S, const int8_t* board, int tp, int ko, int move,
                        int8_t* board_out, int32_t* ko_out, int32_t* ncap_out, int32_t* status_out) {
  const int P = V.P;
  w.for_each(P, [&](int p) { S.sb[p] = board[p]; });
  w.sync();
  int ncap = 0, nko = -1, status = AGZ_OK;
  if (move == P) {
    // pass_move!: board unchanged, ko cleared
  } else if (move < 0 || move > P) {
    status = AGZ_ILLEGAL_MOVE;
  } else {
    label_components(w, V, S, true);
    group_liberties(w, V, S);
    compute_legal_flags(w, V, S, tp, ko);
    const bool ok = S.flag[move];
    w.sync();
    if (!ok) status = AGZ_ILLEGAL_MOVE;
    else apply_move_in_scratch(w, V, S, move, tp, &ncap, &nko);
  }
  if (status != AGZ_OK) {
    w.for_each(P, [&](int p) { board_out[p] = board[p]; });
    nko = ko;
    ncap = 0;
  } else {
    w.for_each(P, [&](int p) { board_out[p] = S.sb[p]; });
  }
  if (w.leader()) { *ko_out = nko; *ncap_out = ncap; *status_out = status; }
  w.sync();
}

template <class W>
AGZ_FN void go_score_one(W& w, const View& V, Scratch& S, const int8_t* board, float komi, float* out) {
  w.for_each(V.P, [&](int p) { S.sb[p] = board[p]; });
  w.sync();
  const float sc = area_score(w, V, S, komi);
  if (w.leader()) *out = sc;
  w.sync();
}

// ------------------------------------------------------------------ single-tree compat ops
// The reference's MCTSNode / MCTSPlayer calls, one at a time, on game slot g (agz_tree_*).

enum TreeOpCode : int32_t {
  TOP_INIT = 0, TOP_SELECT, TOP_ADD_CHILD, TOP_VLOSS_ADD, TOP_VLOSS_REVERT, TOP_INCORPORATE, TOP_NOISE,
  TOP_SEARCH_SELECT, TOP_SEARCH_POST, TOP_PICK, TOP_PLAY, TOP_RESIGN, TOP_SCORES, TOP_PENDING
};

struct TreeArgs {
  int32_t op, g, node, a, up_to, par;
  float value;
  agz_position_info info;
  const float* probs;      // [A]
  const int8_t* board;     // [P]
  const int8_t* history;   // [history_len][P]
  int32_t* iout;           // [4]
  double* dout;            // [A]
};

template <class W>
AGZ_FN void tree_op(W& w, const View& V, Scratch& S, const TreeArgs& T) {
  const int g = T.g;
  GameState& G = V.gs[g];
  int status = AGZ_OK, r0 = 0;
  switch (T.op) {
    case TOP_INIT: {
      // initialize_game!(player, pos), mcts_play.jl:110-118
      root_install(w, V, S, g, T.board, T.history, T.info, G_MANUAL, false);
      r0 = G.root;
    } break;
    case TOP_SELECT: {
      int plen = 0;
      r0 = select_leaf(w, V, S, g, T.node, &plen, false,
                       T.node == G.root && forced_search(V, G, V.meta[node_index(V, g, G.root)].n));
    } break;
    case TOP_ADD_CHILD: {
      const long ni = node_index(V, g, T.node);
      int c = (T.a >= 0 && T.a < V.A) ? V.child[ni * V.AP + T.a] : -2;
      if (c == -1) c = node_create_child(w, V, S, g, T.node, T.a);
      if (c == -2) status = AGZ_ILLEGAL_MOVE;
      else if (c < 0) status = AGZ_POOL_EXHAUSTED;
      r0 = c;
    } break;
    case TOP_VLOSS_ADD:
    case TOP_VLOSS_REVERT: {
      const int len = walk_path(w, V, S, g, T.node, T.up_to);
      path_virtual_loss(w, V, g, S.path, len, T.op == TOP_VLOSS_ADD ? +1 : -1);
    } break;
    case TOP_INCORPORATE: {
      const int len = walk_path(w, V, S, g, T.node, T.up_to);
      status = incorporate(w, V, g, T.node, T.probs, T.value, S.path, len);
    } break;
    case TOP_NOISE: root_explore(w, V, S, g, T.node); break;
    case TOP_SEARCH_SELECT: {
      game_select_phase(w, V, S, g, T.par);
      r0 = G.nleaves;
      if (w.leader()) G.leaf_base = 0;
      w.sync();
    } break;
    case TOP_SEARCH_POST: game_post(w, V, S, g); break;
    case TOP_PICK: status = pick_move(w, V, S, g, &r0); break;
    case TOP_PLAY: {
      // play_move!(player, c), mcts_play.jl:26-50: two_player_mode keeps qs and no searches_pi.  An illegal move is
      // the reference's "Illegal move ... return false": AGZ_OK with r0 = 0
      const int c = play_move(w, V, S, g, T.a, root_q(G), V.two_player ? kPiNone : kPiVisits, !V.two_player, true);
      if (c < 0) { r0 = 0; status = c == -2 ? AGZ_OK : AGZ_POOL_EXHAUSTED; break; }
      free_pending(w, V, S, g, V.cap);      // single-tree API: release the dropped siblings right away
      r0 = 1;
    } break;
    case TOP_RESIGN: r0 = should_resign(V, g); break;
    case TOP_SCORES: {
      const long ni = node_index(V, g, T.node);
      const NodeMeta m = V.meta[ni];
      const float n_s = *slotN(V, g, T.node), tp = (float)m.to_play;
      const double scale =
          V.pv_k > 0.0 ? puct_scale(V, n_s, *slotW(V, g, T.node), *slotS(V, g, T.node)) : puct_scale(V, n_s);
      float f = 0.f;
      if (V.fpu_on) {
        long long M = 0;
        w.for_each(V.A, [&](int a) { M += fpu_mass(V.childN[ni * V.AP + a], V.childP[ni * V.AP + a]); });
        f = fpu_value(V, T.node == G.root, n_s, *slotW(V, g, T.node), tp, reduce_sum_i64(w, M));
      }
      w.for_each(V.A, [&](int a) {
        const long o = ni * V.AP + a;
        T.dout[a] = child_score(V.fpu_on != 0, f, V.childN[o], V.childW[o], V.childP[o], tp, scale);
      });
      w.sync();
    } break;
    case TOP_PENDING: {
      int cnt = 0;
      w.for_each(V.cap, [&](int i) {
        const NodeMeta& m = V.meta[node_index(V, g, i)];
        if ((m.flags & NF_ALLOC) && m.losses != 0) cnt++;
      });
      r0 = w.reduce_sum(cnt);
    } break;
    default: status = AGZ_BAD_ARGUMENT;
  }
  w.sync();
  if (w.leader()) { T.iout[0] = status; T.iout[1] = r0; }
  w.sync();
}

}  // namespace agz
