// tri_index_test.cpp -- the pair index -> (u, v) map of the edge sampler (pymde_amd/csrc/mde_tri_index.h) at forced
// indices, against 128-bit integer arithmetic: the first and last pairs, and both sides of the first pair of a
// spread of rows, at small n and at the n where 4 n (n - 1) no longer fits a double.  Stand-alone: built with a plain
// C++17 compiler and sanitizers (float-cast-overflow among them: the map converts a square root to an integer) by
// tests/test_tri_index_host.py, which runs it as a child process.
#include <cstdio>
#include <vector>

#include "../../pymde_amd/csrc/mde_tri_index.h"

typedef unsigned __int128 u128;

static int failures = 0;
static int max_steps = 0;
static long long checked = 0;

static u128 offset128(u128 n, u128 u) { return u * n - u * (u + 1) / 2; }

// pair idx must be (u, v) with off(u) <= idx < off(u + 1), v = idx - off(u) + u + 1, u < v < n -- all in 128 bits
static void check(int64_t n, uint64_t idx, int64_t want_u) {
  int64_t u = -1, v = -1;
  const int steps = mde_tri_index(n, idx, &u, &v);
  ++checked;
  if (steps > max_steps) max_steps = steps;
  bool ok = u >= 0 && u <= n - 2 && v > u && v < n;
  if (ok) ok = offset128((u128)n, (u128)u) <= (u128)idx && (u128)idx < offset128((u128)n, (u128)u + 1);
  if (ok) ok = (u128)v == (u128)idx - offset128((u128)n, (u128)u) + (u128)u + 1;
  if (ok && want_u >= 0) ok = u == want_u;
  if (ok) ok = mde_tri_row_offset(n, u) == (uint64_t)offset128((u128)n, (u128)u);
  if (!ok || steps > 64) {
    ++failures;
    fprintf(stderr, "n=%lld idx=%llu: (u, v) = (%lld, %lld) after %d steps (expected u = %lld)\n", (long long)n,
            (unsigned long long)idx, (long long)u, (long long)v, steps, (long long)want_u);
  }
}

static void run(int64_t n) {
  const uint64_t total = (uint64_t)(offset128((u128)n, (u128)n - 1));  // C(n, 2) = off(n - 1)
  check(n, 0, 0);
  check(n, total - 1, n - 2);
  if (total > 1) check(n, 1, n > 2 ? 0 : -1);
  if (total > 2) check(n, total - 2, n - 3);
  // a spread of rows: the first few, the last few, powers of two and their neighbours, fractions of n
  std::vector<int64_t> rows;
  for (int64_t u = 1; u <= 70 && u <= n - 2; ++u) rows.push_back(u);
  for (int64_t u = n - 2; u >= 1 && u >= n - 70; --u) rows.push_back(u);
  for (int64_t b = 128; b < n - 2; b *= 2)
    for (int64_t d = -1; d <= 1; ++d) rows.push_back(b + d);
  for (int64_t q = 1; q < 64; ++q) {
    const int64_t u = (int64_t)((u128)n * (u128)q / 64);
    if (u >= 1 && u <= n - 2) rows.push_back(u);
  }
  // rows counted from the end, where the discriminant is smallest
  for (int64_t b = 128; b < n - 2; b *= 2) rows.push_back(n - 2 - b);
  for (int64_t u : rows) {
    if (u < 1 || u > n - 2) continue;
    const uint64_t off = (uint64_t)offset128((u128)n, (u128)u);
    check(n, off - 1, u - 1);
    check(n, off, u);
    if (off + 1 < total) check(n, off + 1, u < n - 2 ? u : -1);
  }
}

int main() {
  const int64_t sizes[] = {2, 3, 4, 5, 45, 60, 2000, ((int64_t)1 << 26) + 3, ((int64_t)1 << 30) + 7,
                           ((int64_t)1 << 31) - 1};
  for (int64_t n : sizes) run(n);
  // every index of the small sizes
  for (int64_t n : {2, 3, 4, 5, 45, 60}) {
    uint64_t idx = 0;
    for (int64_t u = 0; u < n - 1; ++u)
      for (int64_t v = u + 1; v < n; ++v) {
        int64_t gu = -1, gv = -1;
        (void)mde_tri_index(n, idx++, &gu, &gv);
        ++checked;
        if (gu != u || gv != v) {
          ++failures;
          fprintf(stderr, "n=%lld idx=%llu: (%lld, %lld), expected (%lld, %lld)\n", (long long)n,
                  (unsigned long long)(idx - 1), (long long)gu, (long long)gv, (long long)u, (long long)v);
        }
      }
  }
  printf("%lld indices checked, at most %d correction steps\n", checked, max_steps);
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("all cases pass\n");
  return 0;
}
