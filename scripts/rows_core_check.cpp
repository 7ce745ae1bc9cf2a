// rows_core_check.cpp -- the row check's core (csrc/irec_rows_core.h) under the host sanitizers.
// A stand-alone program: every line of the core that rows_status_kernel runs is compiled here by g++ and runs with AddressSanitizer and
// UndefinedBehaviorSanitizer.  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Irelative-entropy-coding_amd/csrc \
//       scripts/rows_core_check.cpp -o /tmp/rows_core_check && /tmp/rows_core_check
// It walks the grid of tests/rows_status_cases.py -- bpg {1, 3, 9} x max_K {1, 5, 70} x n_groups {1, 3, 65} x packed / joined strides x
// identity / shuffled block_row x min_K {0, 1}, group g of combination c carrying plant (c + g) mod 19 (K = 0, max_K, max_K + 1, -1,
// 2^31 - 1; an index -1, S, 2^31 - 1 at positions 0, K - 1 and K; two failing blocks; a preset status; K beyond the ratio table) -- with
// K, idx and status in heap buffers of EXACTLY the size the call may read, so that one index past idx[b * idx_stride + max_K - 1] (K =
// 2^31 - 1 would walk two billion of them) is a heap-buffer-overflow report.  Every status is held against a referee written out here.
// Exit status 0 and the last line "rows_core_check: all equal" mean: same verdicts, and no sanitizer report
// (profiles/decompress/sanitizer_rows_core.log is this program's output).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "irec_rows_core.h"

namespace {
uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_state += 0x9E3779B97F4A7C15ull; uint64_t z = g_state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
int64_t below(int64_t n) { return (int64_t)(rnd() % (uint64_t)n); }
int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)

constexpr int32_t S = 36, I32MAX = 0x7fffffff, N_PLANTS = 19;
const int32_t BAD[3] = {-1, S, I32MAX};

struct Case {
  int32_t bpg, max_K, n_groups, min_K, k_limit; bool joined, shuffled;
  std::vector<int32_t> K, idx, block_row, status0;          // logical rows: K [rows], idx [rows][max_K]
};

void plant(Case &c, int which, int32_t g) {
  auto row = [&](int32_t j) { const int64_t at = (int64_t)g * c.bpg + j; return c.shuffled ? (int64_t)c.block_row[at] : at; };
  const int32_t j = (int32_t)below(c.bpg);
  int32_t &k = c.K[row(j)];
  int32_t *ix = &c.idx[row(j) * c.max_K];
  if (which == 1) k = 0;
  else if (which == 2) k = std::min(c.max_K, c.k_limit);
  else if (which == 3) k = c.max_K + 1;
  else if (which == 4) k = -1;
  else if (which == 5) k = I32MAX;
  else if (which >= 6 && which <= 14) {
    const int32_t v = BAD[(which - 6) % 3], pos = (which - 6) / 3;
    if (pos == 0) { k = std::max(1, k); ix[0] = v; }
    else if (pos == 1) { k = std::max(1, k); ix[k - 1] = v; }
    else { k = std::min(k, c.max_K - 1); ix[k] = v; }           // position K: must not count
  } else if ((which == 15 || which == 16) && c.bpg >= 2) {
    int32_t lo = (int32_t)below(c.bpg), hi = (int32_t)below(c.bpg - 1);
    if (hi >= lo) ++hi;
    if (lo > hi) std::swap(lo, hi);
    const int32_t a = which == 15 ? lo : hi, b = which == 15 ? hi : lo;
    int32_t &ka = c.K[row(a)];
    ka = std::max(1, ka); c.idx[row(a) * c.max_K + below(ka)] = S;   // an index out of range in block a
    c.K[row(b)] = c.max_K + 1;                                      // a count out of range in block b
  } else if (which == 17) { c.status0[g] = 7; k = -5; }
  else if (which == 18 && c.k_limit < c.max_K) k = c.k_limit + 1;
}

Case make(int combo, int32_t bpg, int32_t max_K, int32_t n_groups, bool joined, bool shuffled, int32_t min_K) {
  Case c{bpg, max_K, n_groups, min_K, (max_K >= 5 && combo % 3 == 0) ? std::max(1, max_K - 2) : I32MAX, joined, shuffled, {}, {}, {}, {}};
  const int64_t rows = (int64_t)n_groups * bpg;
  const int32_t top = std::min(max_K, c.k_limit);
  c.K.resize((size_t)rows); c.idx.resize((size_t)(rows * max_K)); c.status0.assign((size_t)n_groups, 0);
  for (auto &k : c.K) k = min_K + (int32_t)below(top - min_K + 1);
  for (auto &v : c.idx) v = (int32_t)below(S);
  if (shuffled) {
    c.block_row.resize((size_t)rows);
    for (int64_t r = 0; r < rows; ++r) c.block_row[(size_t)r] = (int32_t)r;
    for (int64_t r = rows - 1; r > 0; --r) std::swap(c.block_row[(size_t)r], c.block_row[(size_t)below(r + 1)]);
  }
  for (int32_t g = 0; g < n_groups; ++g) plant(c, (combo + g) % N_PLANTS, g);
  return c;
}

// the referee, written out: per group the first cause of its lowest failing block, a preset status kept
std::vector<int32_t> referee(const Case &c) {
  std::vector<int32_t> out = c.status0;
  for (int32_t g = 0; g < c.n_groups; ++g) {
    if (out[(size_t)g]) continue;
    for (int32_t j = 0; j < c.bpg && !out[(size_t)g]; ++j) {
      const int64_t at = (int64_t)g * c.bpg + j, b = c.shuffled ? (int64_t)c.block_row[(size_t)at] : at;
      const int64_t k = c.K[(size_t)b];
      if (k < c.min_K || k > c.max_K) out[(size_t)g] = 1;
      else if (k > c.k_limit) out[(size_t)g] = 3;
      else for (int64_t t = 0; t < k; ++t) { const int32_t v = c.idx[(size_t)(b * c.max_K + t)]; if (v < 0 || v >= S) out[(size_t)g] = 2; }
    }
  }
  return out;
}

int64_t g_nonzero = 0, g_groups = 0;
void run(const Case &c) {
  const int64_t rows = (int64_t)c.n_groups * c.bpg;
  // exactly-sized heap buffers (new[]: no slack behind them that the sanitizer would let a read into)
  int32_t *Kbuf = nullptr, *Ibuf = nullptr, *joined = nullptr;
  irec_rows::Call call{c.n_groups, c.bpg, c.shuffled ? c.block_row.data() : nullptr, nullptr, 1, nullptr, c.max_K, c.max_K, c.min_K, c.k_limit, S, nullptr};
  if (c.joined) {
    joined = new int32_t[(size_t)(rows * (1 + c.max_K))];
    for (int64_t b = 0; b < rows; ++b) {
      joined[b * (1 + c.max_K)] = c.K[(size_t)b];
      for (int32_t t = 0; t < c.max_K; ++t) joined[b * (1 + c.max_K) + 1 + t] = c.idx[(size_t)(b * c.max_K + t)];
    }
    call.K = joined; call.idx = joined + 1; call.k_stride = call.idx_stride = 1 + c.max_K;
  } else {
    Kbuf = new int32_t[(size_t)rows]; Ibuf = new int32_t[(size_t)(rows * c.max_K)];
    std::copy(c.K.begin(), c.K.end(), Kbuf); std::copy(c.idx.begin(), c.idx.end(), Ibuf);
    call.K = Kbuf; call.idx = Ibuf;
  }
  int32_t *status = new int32_t[(size_t)c.n_groups];
  std::copy(c.status0.begin(), c.status0.end(), status);
  call.status = status;
  CHECK(irec_rows::args_ok(call));
  irec_rows::call_host(call);
  const std::vector<int32_t> want = referee(c);
  for (int32_t g = 0; g < c.n_groups; ++g) { CHECK(status[g] == want[(size_t)g]); g_nonzero += status[g] != 0; ++g_groups; }
  // and the way the kernel deals a group's blocks out: 256 lanes, the smallest code wins
  std::copy(c.status0.begin(), c.status0.end(), status);
  for (int32_t g = 0; g < c.n_groups; ++g) {
    int32_t first = irec_rows::NONE;
    for (int32_t t = 0; t < 256; ++t) first = std::min(first, irec_rows::lane_first(call, g, t, 256));
    irec_rows::group_store(call, g, first);
    CHECK(status[g] == want[(size_t)g]);
  }
  delete[] status; delete[] Kbuf; delete[] Ibuf; delete[] joined;
}
} // namespace

int main() {
  const int32_t bpgs[3] = {1, 3, 9}, max_Ks[3] = {1, 5, 70}, groups[3] = {1, 3, 65};
  int combo = 0;
  for (int32_t bpg : bpgs) for (int32_t max_K : max_Ks) for (int32_t n_groups : groups)
    for (int joined = 0; joined < 2; ++joined) for (int shuffled = 0; shuffled < 2; ++shuffled) for (int32_t min_K = 0; min_K < 2; ++min_K) {
      run(make(combo, bpg, max_K, n_groups, joined != 0, shuffled != 0, min_K));
      ++combo;
    }
  std::printf("%d combinations, %lld groups, %lld of them with a cause: the core equals the referee, dealt out whole and over 256 lanes\n", combo,
              (long long)g_groups, (long long)g_nonzero);
  if (g_failures) { std::printf("rows_core_check: %d FAILED\n", g_failures); return 1; }
  std::printf("rows_core_check: all equal\n");
  return 0;
}
