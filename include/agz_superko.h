/*
 * agz_superko.h -- position keys and the superko rules: positional and situational repetition (agz_search_set_ko_rule,
 * agz_go_keys, agz_go_legal_seen, agz_tree_node_key, agz_go_position_key; include/agz.h).
 *
 * 1. STONE KEYS.  agz_zobrist(point, colour), colour = +1 (Black) or -1 (White), point = row + N*col >= 0, is a fixed
 *    64-bit integer mix, every operation modulo 2^64:
 *
 *     x = (uint64)point * 2 + (colour < 0 ? 1 : 0) + 1
 *     z = x * 0x9E3779B97F4A7C15
 *     z = (z ^ (z >> 32)) * 0xD6E8FEB86659FD93
 *     z = (z ^ (z >> 29)) * 0xA0761D6478BD642F
 *     key = z ^ (z >> 32)
 *
 *    It is a finaliser of its own, not a draw site of agz_draws.h: no seed enters it, and its values are part of the
 *    contract (tests/test_superko.py restates it in numpy).  AGZ_ZOBRIST_WHITE_TO_PLAY is one more constant.
 *
 * 2. KEYS OF A POSITION.  The position key is the XOR of agz_zobrist(p, board[p]) over the stones (0 for the empty
 *    board).  The situation key is the position key, XORed with AGZ_ZOBRIST_WHITE_TO_PLAY when White is to play.  The
 *    key "under a rule" is the situation key under AGZ_KO_SITUATIONAL and the position key otherwise.
 *
 * 3. THE RULE.  The seen set of a node X holds the keys, under the rule in force, of X's own position and of every
 *    earlier position of its game that the engine knows: X's ancestors in the tree up to the root, the positions the
 *    root has left behind through re-rooting since the slot was installed, and the history_len (at most 7) boards handed
 *    to the install (board h is h + 1 plies before the root, so its side to move is to_play * (-1)^(h+1)).  A board move
 *    a that the simple rules allow at X is refused when the key of the position after a -- captures removed, the other
 *    side to move -- is in the seen set:
 *
 *     child = key(X) ^ agz_zobrist(a, to_play) ^ (XOR of the stones of the DISTINCT enemy groups whose only liberty is a)
 *             ^ (AGZ_ZOBRIST_WHITE_TO_PLAY under the situational rule: the side to move always changes)
 *
 *    Pass is always legal.  The simple-ko clause stays (both rules imply it).  Positions older than a supplied history
 *    are unknown to the rule: a game installed from a position with h history boards can repeat a position that lies
 *    more than h plies before that install.  A 64-bit key collision forbids a legal move.
 *
 * Plain C99; also valid C++ and HIP device code.
 */
#ifndef AGZ_SUPERKO_H
#define AGZ_SUPERKO_H

#include <stdint.h>

#if defined(__HIPCC__)
#define AGZ_SK_FN __host__ __device__ static inline
#else
#define AGZ_SK_FN static inline
#endif

#define AGZ_KO_SIMPLE 0        /* one ko point (the default: the reference's rule) */
#define AGZ_KO_POSITIONAL 1    /* no board may be recreated */
#define AGZ_KO_SITUATIONAL 2   /* no board may be recreated with the same side to move */

#define AGZ_ZOBRIST_WHITE_TO_PLAY 0x8A5CD789635D2DFFull

AGZ_SK_FN uint64_t agz_zobrist(int32_t point, int32_t colour) {
  uint64_t z = ((uint64_t)(uint32_t)point * 2u + (colour < 0 ? 1u : 0u) + 1u) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 32)) * 0xD6E8FEB86659FD93ull;
  z = (z ^ (z >> 29)) * 0xA0761D6478BD642Full;
  return z ^ (z >> 32);
}

/* what the side to move adds to a position key under `rule` */
AGZ_SK_FN uint64_t agz_ko_side_key(int32_t to_play, int32_t rule) {
  return (rule == AGZ_KO_SITUATIONAL && to_play < 0) ? AGZ_ZOBRIST_WHITE_TO_PLAY : 0ull;
}

AGZ_SK_FN int agz_ko_rule_valid(int32_t rule) { return rule >= AGZ_KO_SIMPLE && rule <= AGZ_KO_SITUATIONAL; }

/* The key of board[P] (+1 Black, -1 White, 0 empty) with to_play to move, under `rule` (AGZ_KO_SIMPLE gives the
 * position key).  For the host: the kernels fold a board over the lanes of a wave (board_key, agz_search.h). */
AGZ_SK_FN uint64_t agz_position_key(const int8_t* board, int32_t P, int32_t to_play, int32_t rule) {
  uint64_t k = agz_ko_side_key(to_play, rule);
  for (int32_t p = 0; p < P; ++p)
    if (board[p] != 0) k ^= agz_zobrist(p, board[p]);
  return k;
}

#endif /* AGZ_SUPERKO_H */
