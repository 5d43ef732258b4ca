// mz_keys.h -- the host's integer code: JAX threefry key bookkeeping and mctx's sequential-halving table.  These decide
// every PRNG stream of every search.  Plain C++ (no HIP include), so tests/keys_main.cpp runs them on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mzh {

// ---- host-side JAX threefry (key bookkeeping only: 3 blocks per simulation) ----
inline uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
inline void h_threefry(const uint32_t key[2], uint32_t x0, uint32_t x1, uint32_t out[2]) {
  static const int R[2][4] = {{13, 15, 26, 6}, {17, 29, 16, 24}};
  const uint32_t ks[3] = {key[0], key[1], key[0] ^ key[1] ^ 0x1BD11BDAu};
  x0 += ks[0];
  x1 += ks[1];
  for (int g = 0; g < 5; ++g) {
    for (int i = 0; i < 4; ++i) {
      x0 += x1;
      x1 = rotl32(x1, R[g & 1][i]) ^ x0;
    }
    x0 += ks[(g + 1) % 3];
    x1 += ks[(g + 2) % 3] + (uint32_t)(g + 1);
  }
  out[0] = x0;
  out[1] = x1;
}
inline uint32_t h_bits(const uint32_t key[2], uint64_t size, uint64_t i) {
  uint64_t half = (size + 1) / 2;
  uint64_t blk = i < half ? i : i - half;
  uint64_t c1 = half + blk;
  uint32_t out[2];
  h_threefry(key, (uint32_t)blk, c1 < size ? (uint32_t)c1 : 0u, out);
  return i < half ? out[0] : out[1];
}
inline void h_split(const uint32_t key[2], uint64_t n, uint64_t row, uint32_t out[2]) {
  out[0] = h_bits(key, 2 * n, 2 * row);
  out[1] = h_bits(key, 2 * n, 2 * row + 1);
}

// mctx seq_halving.get_table_of_considered_visits (host integers, uploaded once per handle)
inline void considered_visits(int m, int S, int32_t* seq) {
  if (m <= 1) {
    for (int i = 0; i < S; ++i) seq[i] = i;
    return;
  }
  int log2max = 0;
  while ((1 << log2max) < m) ++log2max;
  std::vector<int32_t> visits(m, 0);
  int n = 0, nc = m;
  while (n < S) {
    int extra = S / (log2max * nc);
    if (extra < 1) extra = 1;
    for (int e = 0; e < extra; ++e) {
      for (int i = 0; i < nc && n < S; ++i) seq[n++] = visits[i];
      for (int i = 0; i < nc; ++i) visits[i] += 1;
    }
    nc = nc / 2 > 2 ? nc / 2 : 2;
  }
}
// ... for every m in 0..max_considered: the [max_considered + 1][S] table the Gumbel kernels read
inline std::vector<int32_t> visit_table(int max_considered, int S) {
  std::vector<int32_t> table((size_t)(max_considered + 1) * S);
  for (int m = 0; m <= max_considered; ++m) considered_visits(m, S, table.data() + (size_t)m * S);
  return table;
}

// (clang -O3 turns the four scalar threefry blocks of a simulation into ~32 ns: 1.6 us per 50-simulation act, measured;
// a hand-vectorised split3 was no faster -- round 6)
// mctx muzero_policy / search key walk: (k_sample, k_dirichlet, k_search) = split(key, 3);
// per simulation (rng, simulate_key, expand_key) = split(rng, 3).  sim_keys: [S][2]
inline void derive_keys(const uint32_t key[2], int S, uint32_t k_sample[2], uint32_t* sim_keys) {
  uint32_t rk[2];
  h_split(key, 3, 0, k_sample);
  h_split(key, 3, 2, rk);
  for (int s = 0; s < S; ++s) {  // every simulation: the step-wise path takes up to 65534 of them
    uint32_t nk[2];
    h_split(rk, 3, 1, &sim_keys[2 * (size_t)s]);
    h_split(rk, 3, 0, nk);
    rk[0] = nk[0], rk[1] = nk[1];
  }
}

}  // namespace mzh
