// keys_main.cpp -- runs the library's host integer code (muax_amd/csrc/mz_keys.h: the JAX threefry key walk and mctx's
// sequential-halving table) on the CPU, with no GPU or HIP runtime call, so that tests/test_keys_cpu.py can build it with
// the host sanitizers and compare every word with the oracle.  One command per argument group, one output line each:
//   split K0 K1 N ROW   -> h_split(key, N, ROW): 2 words
//   walk K0 K1 S        -> derive_keys(key, S): k_sample (2 words), then sim_keys (2 S words)
//   gumbel K0 K1        -> the Gumbel policy's root key split(key, 2)[1]: 2 words
//   visits M S          -> considered_visits(M, S): S words
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mz_keys.h"

int main(int argc, char** argv) {
  int i = 1;
  auto num = [&]() -> unsigned long long {
    if (i >= argc) {
      fprintf(stderr, "keys_main: missing argument\n");
      exit(2);
    }
    return strtoull(argv[i++], nullptr, 0);
  };
  auto key = [&](uint32_t k[2]) {
    k[0] = (uint32_t)num();
    k[1] = (uint32_t)num();
  };
  while (i < argc) {
    const char* cmd = argv[i++];
    uint32_t k[2], out[2];
    std::vector<uint32_t> words;
    if (!strcmp(cmd, "split")) {
      key(k);
      const uint64_t n = num(), row = num();
      mzh::h_split(k, n, row, out);
      words = {out[0], out[1]};
    } else if (!strcmp(cmd, "walk")) {
      key(k);
      const int S = (int)num();
      words.assign(2 + 2 * (size_t)S, 0u);
      mzh::derive_keys(k, S, words.data(), words.data() + 2);
    } else if (!strcmp(cmd, "gumbel")) {
      key(k);
      mzh::h_split(k, 2, 1, out);
      words = {out[0], out[1]};
    } else if (!strcmp(cmd, "visits")) {
      const int m = (int)num(), S = (int)num();
      std::vector<int32_t> seq((size_t)S, -1);
      mzh::considered_visits(m, S, seq.data());
      words.assign(seq.begin(), seq.end());
    } else {
      fprintf(stderr, "keys_main: unknown command %s\n", cmd);
      return 2;
    }
    for (size_t w = 0; w < words.size(); ++w) printf(w ? " %u" : "%u", words[w]);
    printf("\n");
  }
  return 0;
}
