// ring_rows_test.cpp -- invariants of plan_rows (pymde_amd/csrc/mde_ring_rows.h), the host function that decides
// which rows the LDS-ring layout peels off as hubs and how it deals the rest to the row blocks.  Stand-alone: built
// with a plain C++17 compiler and sanitizers by tests/test_ring_rows_host.py, which runs it as a child process.
#include <cstdio>
#include <numeric>

#include "../../pymde_amd/csrc/mde_ring_rows.h"

static const int R = 64, NCW = 8;
static int failures = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      ++failures;                         \
      fprintf(stderr, "%s: ", name);      \
      fprintf(stderr, __VA_ARGS__);       \
      fputc('\n', stderr);                \
    }                                     \
  } while (0)

// want_hubs / want_nrb / want_permuted: -1 = whatever the rule gives
static void run(const char* name, const std::vector<int32_t>& deg, int hub_env, int perm_env, int want_hubs, int want_nrb,
                int want_permuted) {
  const int64_t nloc = (int64_t)deg.size();
  std::vector<int32_t> rowptr(deg.size() + 1, 0);
  std::partial_sum(deg.begin(), deg.end(), rowptr.begin() + 1);
  const int64_t H = rowptr.back();
  const int NRB = (int)((nloc + R - 1) / R);
  RowPlan rp;
  CHECK(plan_rows(rowptr.data(), nloc, H, R, NRB, NCW, hub_env, perm_env, &rp), "plan_rows reported an overflowing block");
  if (want_hubs >= 0) CHECK((int)rp.hub_rows.size() == want_hubs, "%zu hub rows, expected %d", rp.hub_rows.size(), want_hubs);
  if (want_nrb >= 0) CHECK(rp.nrb == want_nrb, "%d row blocks, expected %d", rp.nrb, want_nrb);
  if (want_permuted >= 0) CHECK((int)rp.permuted == want_permuted, "permuted %d, expected %d", (int)rp.permuted, want_permuted);
  if (!rp.mapped) {  // rows as they are: nothing peeled, nothing dealt
    CHECK(rp.hub_rows.empty() && !rp.permuted && rp.nrb == NRB && rp.H_ring == H, "an unmapped plan must leave everything alone");
    return;
  }
  // hub rows: over the threshold, ascending; their segments tile [rowptr[r], rowptr[r + 1]) in pieces of <= MDE_HUB_SEG
  std::vector<char> is_hub(deg.size(), 0);
  int64_t hub_he = 0;
  int32_t dmax = 0;
  CHECK(rp.hub_first.size() == rp.hub_rows.size() + 1 && rp.hub_seg.size() % 4 == 0, "hub_first / hub_seg sizes");
  for (size_t i = 0; i < rp.hub_rows.size(); ++i) {
    const int32_t r = rp.hub_rows[i];
    CHECK(deg[r] > rp.threshold && (i == 0 || rp.hub_rows[i - 1] < r), "hub row %d (degree %d, threshold %d)", r, deg[r], rp.threshold);
    is_hub[r] = 1;
    hub_he += deg[r];
    int64_t at = rowptr[r];
    for (int32_t s = rp.hub_first[i]; s < rp.hub_first[i + 1]; ++s) {
      const int32_t* g = &rp.hub_seg[4 * (size_t)s];
      CHECK(g[0] == (int32_t)i && g[1] == at && g[2] > g[1] && g[2] - g[1] <= MDE_HUB_SEG, "segment %d of hub row %d: [%d, %d)", s, r, g[1], g[2]);
      at = g[2];
    }
    CHECK(at == rowptr[r + 1], "the segments of hub row %d end at %lld, the row at %d", r, (long long)at, rowptr[r + 1]);
  }
  CHECK(rp.hub_first.back() == (int32_t)(rp.hub_seg.size() / 4), "hub_first does not close hub_seg");
  CHECK(rp.hub_half_edges == hub_he && rp.H_ring == H - hub_he && 2 * hub_he <= H, "hub half-edges %lld", (long long)rp.hub_half_edges);
  for (int64_t r = 0; r < nloc; ++r)
    if (!is_hub[r]) {
      CHECK(deg[r] <= rp.threshold || hub_env == 0 || rp.hub_rows.empty(), "row %lld (degree %d) should have been peeled", (long long)r, deg[r]);
      dmax = std::max(dmax, deg[r]);
    }
  // slots: every ring row in exactly one, row_slot and slot_row inverse, no block over R rows
  const size_t nslots = (size_t)rp.nrb * R;
  CHECK(rp.row_slot.size() == deg.size() && rp.slot_cum.size() == nslots + 1, "row_slot / slot_cum sizes");
  CHECK(rp.permuted ? rp.slot_row.size() == nslots : rp.slot_row.empty(), "slot_row size %zu", rp.slot_row.size());
  std::vector<int32_t> slot_row(nslots, -1);  // rebuilt from row_slot
  for (int64_t r = 0; r < nloc; ++r) {
    const int32_t s = rp.row_slot[r];
    CHECK(is_hub[r] ? s == -1 : (s >= 0 && (size_t)s < nslots), "row %lld sits in slot %d", (long long)r, s);
    if (s < 0 || (size_t)s >= nslots) continue;
    CHECK(slot_row[s] == -1, "slot %d holds rows %d and %lld", s, slot_row[s], (long long)r);
    slot_row[s] = (int32_t)r;
    if (!rp.permuted) CHECK(s == r, "an unpermuted layout keeps row %lld in its own slot, not %d", (long long)r, s);
  }
  if (rp.permuted) CHECK(slot_row == rp.slot_row, "slot_row is not the inverse of row_slot");
  // slot_cum: the running half-edge count of the slots, ending at H_ring; the blocks' work when dealt
  int64_t heaviest = 0, lightest = H;
  for (int b = 0; b < rp.nrb; ++b) {
    for (int s = b * R; s < (b + 1) * R; ++s) {
      const int32_t want = slot_row[s] >= 0 ? deg[slot_row[s]] : 0;
      CHECK(rp.slot_cum[s + 1] - rp.slot_cum[s] == want, "slot %d holds %d half-edges, its row has %d", s, rp.slot_cum[s + 1] - rp.slot_cum[s], want);
      if (rp.permuted && s > b * R && slot_row[s] >= 0) CHECK(slot_row[s - 1] >= 0 && slot_row[s - 1] < slot_row[s], "block %d: rows not ascending at slot %d", b, s);
    }
    const int64_t w = rp.slot_cum[(size_t)(b + 1) * R] - rp.slot_cum[(size_t)b * R];
    heaviest = std::max(heaviest, w);
    lightest = std::min(lightest, w);
  }
  CHECK(rp.slot_cum[0] == 0 && rp.slot_cum[nslots] == rp.H_ring, "slot_cum ends at %d, H_ring is %lld", rp.slot_cum[nslots], (long long)rp.H_ring);
  if (rp.permuted) CHECK(heaviest - lightest <= dmax, "dealt blocks: heaviest %lld, lightest %lld, largest ring degree %d", (long long)heaviest, (long long)lightest, dmax);
}

// `n` rows whose degrees fall from `top` along the vertex order
static std::vector<int32_t> falling(int n, int top) {
  std::vector<int32_t> d((size_t)n);
  for (int r = 0; r < n; ++r) d[(size_t)r] = 1 + (int)((int64_t)top * (n - r) / n) + (r * 7) % 5;
  return d;
}
static std::vector<int32_t> with(std::vector<int32_t> d, std::initializer_list<std::pair<int, int>> rows) {
  for (auto& p : rows) d[(size_t)p.first] = p.second;
  return d;
}

int main() {
  const std::vector<int32_t> flat500(500, 10);
  run("one row", {5}, -1, -1, 0, 1, 0);
  run("one row, dealt", {5}, -1, 1, 0, 1, 1);
  run("R * NRB rows", falling(4 * R, 60), -1, -1, 0, 4, 1);
  run("R * NRB - 1 rows", falling(4 * R - 1, 60), -1, -1, 0, 4, 1);
  run("R * NRB rows, dealt", std::vector<int32_t>(4 * R, 3), -1, 1, 0, 4, 1);
  run("degree T and T + 1, T = 300", with(flat500, {{3, 300}, {401, 301}}), 300, -1, 1, -1, -1);
  run("degree T and T + 1, default T = 256", with(flat500, {{3, 256}, {401, 257}}), -1, -1, 1, -1, -1);
  run("hub of 2 segments + 1", with(flat500, {{77, 2 * MDE_HUB_SEG + 1}}), 300, 0, 1, 8, 0);
  run("hubs hold most of the graph", with(std::vector<int32_t>(110, 5), {{0, 1000}, {9, 1000}, {50, 1000}, {109, 1000}}), 300, -1, 0, -1, -1);
  run("dealt, rows no multiple of R", falling(1000, 40), 0, 1, 0, 16, 1);
  run("so many hubs that a block goes", with(std::vector<int32_t>(130, 40), {{1, 400}, {30, 400}, {64, 400}, {100, 400}, {129, 400}}), 300, 1, 5, 2, 1);
  run("no peeling, dealt", with(falling(700, 30), {{5, 5000}}), 0, 1, 0, 11, 1);
  run("peeled, never dealt", with(falling(700, 30), {{5, 5000}}), 300, 0, 1, 11, 0);
  run("both off", with(falling(700, 30), {{5, 5000}}), 0, 0, 0, 11, 0);
  if (failures) fprintf(stderr, "%d checks failed\n", failures);
  else printf("ring rows: all cases pass\n");
  return failures ? 1 : 0;
}
