// The rules header of the device 2048 (muax_amd/csrc/mz_2048.h) under the host compiler, for
// tests/test_env_2048_rules_cpu.py.  Every line of standard input is "board action x0 x1" (decimal); the answer is one
// line: the board after the move, the tiles its merges created, the unchanged word, the mask word, the number of empty
// cells of the moved board, the moved board after a spawn from (x0, x1), and the board transposed and mirrored.
#include <cinttypes>
#include <cstdio>

#include "mz_2048.h"

int main() {
  uint64_t board;
  int a;
  uint32_t x0, x1;
  while (std::scanf("%" SCNu64 " %d %" SCNu32 " %" SCNu32, &board, &a, &x0, &x1) == 4) {
    uint32_t gained;
    const uint64_t moved = mz2048::move(board, a, gained);
    std::printf("%" PRIu64 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %d %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", moved, gained,
                mz2048::unchanged_word(board), mz2048::mask_word(board), mz2048::empty_cells(moved),
                mz2048::spawn(moved, x0, x1), mz2048::transpose(board), mz2048::mirror(board));
  }
  return 0;
}
