// mz_2048.h -- the rules of 2048 on one 64-bit board ("Device 2048"): integer arithmetic in registers, no
// table in memory, nothing of HIP -- the kernels of mz_env2048.cuh include it for the device, tests/rules2048_main.cpp
// for the host compiler, and both run the same text.
//
// Board: nibble i (bits 4 i .. 4 i + 3) is the exponent of cell i, row-major, cell 0 top-left, so row r is the 16 bits
// at 16 r and column c of it the nibble at 4 c.  Exponent 0 is empty, exponent k is tile 2^k.
// Moves: 0 up, 1 right, 2 down, 3 left; any other value changes nothing.  A move slides every line toward its edge and
// merges equal neighbours once per tile, starting from that edge (2 2 2 2 -> 4 4 . ., 2 2 4 . -> 4 4 . .); two tiles of
// exponent 15 do not merge.  `gained` is the sum of the tiles the merges created (at most 8 x 2^15).
// A move is legal when it changes the board.  The mask of a board has byte a = 1 where move a is illegal -- except that
// a board with no tile at all reports every move as legal (zero-padded reanalysis rows: an all-invalid root must never
// reach the search).  A board is dead when no move changes it; by that rule the empty board is dead as well.
// Spawn: with n empty cells enumerated in ascending cell index and one threefry block (x0, x1), the cell is number
// k = (uint64(x0) * n) >> 32 of them and the exponent 2 where x1 < 0x1999999A (one in ten), else 1.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MZ_2048_FN __host__ __device__ __forceinline__
#else
#define MZ_2048_FN inline
#endif

namespace mz2048 {

constexpr uint32_t kFourBelow = 0x1999999Au;   // x1 below this spawns exponent 2
constexpr uint32_t kAllIllegal = 0x01010101u;  // the mask word of a dead board

// rows <-> columns of the 4 x 4 nibbles (its own inverse): 2 x 2 blocks of nibbles, then 2 x 2 blocks of bytes
MZ_2048_FN uint64_t transpose(uint64_t x) {
  const uint64_t a = (x & 0xF0F00F0FF0F00F0Full) | ((x & 0x0000F0F00000F0F0ull) << 12) |
                     ((x & 0x0F0F00000F0F0000ull) >> 12);
  return (a & 0xFF00FF0000FF00FFull) | ((a & 0x00FF00FF00000000ull) >> 24) | ((a & 0x00000000FF00FF00ull) << 24);
}

// every row's four nibbles in reverse order (its own inverse)
MZ_2048_FN uint64_t mirror(uint64_t x) {
  x = ((x & 0x00FF00FF00FF00FFull) << 8) | ((x >> 8) & 0x00FF00FF00FF00FFull);
  return ((x & 0x0F0F0F0F0F0F0F0Full) << 4) | ((x >> 4) & 0x0F0F0F0F0F0F0F0Full);
}

// one line of four nibbles slid toward nibble 0 and merged from there; adds the created tiles to `gained`
MZ_2048_FN uint32_t slide_line(uint32_t line, uint32_t& gained) {
  uint32_t out = 0, at = 0, held = 0;  // held: the tile that may still merge with the next one
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint32_t v = (line >> (4 * c)) & 15u;
    if (v == 0) continue;
    if (held == v && v != 15u) {
      out |= (v + 1u) << at;
      at += 4;
      gained += 2u << v;
      held = 0;
    } else {
      if (held != 0) {
        out |= held << at;
        at += 4;
      }
      held = v;
    }
  }
  return out | (held << at);  // (held == 0 adds nothing; at <= 12 whenever held != 0)
}

// THE slide and merge: the board after move `a`; `gained` = the sum of the tiles its merges created
MZ_2048_FN uint64_t move(uint64_t board, int a, uint32_t& gained) {
  gained = 0;
  if ((unsigned)a > 3u) return board;
  const bool columns = a == 0 || a == 2, far_edge = a == 1 || a == 2;
  uint64_t x = board;
  if (columns) x = transpose(x);
  if (far_edge) x = mirror(x);
  uint64_t y = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) y |= (uint64_t)slide_line((uint32_t)(x >> (16 * r)) & 0xFFFFu, gained) << (16 * r);
  if (far_edge) y = mirror(y);
  if (columns) y = transpose(y);
  return y;
}

// THE legality rule: does move `a` change this board
MZ_2048_FN bool move_changes(uint64_t board, int a) {
  uint32_t gained;
  return move(board, a, gained) != board;
}

// byte a = 1 where move a does not change the board (kAllIllegal: dead), the empty board included
MZ_2048_FN uint32_t unchanged_word(uint64_t board) {
  uint32_t w = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a) w |= (move_changes(board, a) ? 0u : 1u) << (8 * a);
  return w;
}

MZ_2048_FN bool dead(uint64_t board) { return unchanged_word(board) == kAllIllegal; }

// the mask the search gets: unchanged_word, but 0 for a board with no tile at all
MZ_2048_FN uint32_t mask_word(uint64_t board) { return board == 0 ? 0u : unchanged_word(board); }

MZ_2048_FN int empty_cells(uint64_t board) {
  uint64_t x = board | (board >> 1);
  x |= x >> 2;
  return 16 - __builtin_popcountll(x & 0x1111111111111111ull);
}

// one spawn from the block (x0, x1); a full board is returned as it is
MZ_2048_FN uint64_t spawn(uint64_t board, uint32_t x0, uint32_t x1) {
  const int n = empty_cells(board);
  const int k = (int)(((uint64_t)x0 * (uint64_t)n) >> 32);  // 0 .. n - 1 (0 for n == 0, where nothing is empty)
  const uint64_t v = x1 < kFourBelow ? 2u : 1u;
  uint64_t out = board;
  int seen = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const bool empty = ((board >> (4 * i)) & 15u) == 0;
    if (empty && seen == k) out |= v << (4 * i);
    seen += empty ? 1 : 0;
  }
  return out;
}

}  // namespace mz2048
