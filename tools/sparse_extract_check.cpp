// Stand-alone check of deep-video-mvs_amd/csrc/sparse_extract_grid.h on the host: the bounded binary search, the neighbour rows and the
// handling rule of the mesh extraction from the sparse TSDF volume, over hand-made key sets.  Built with the host compiler and
// -fsanitize=address,undefined by tests/test_sparse_extract_reference.py (no GPU, no HIP).  Exit status 0 = every check passed.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/sparse_extract_check.cpp -o sparse_extract_check
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "../deep-video-mvs_amd/csrc/sparse_extract_grid.h"

using namespace dvmvs;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      if (failures < 20) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

typedef std::array<int, 3> Brick;

// One pool: bricks in SLOT order.  Checks every neighbour entry against a brute-force search, then the handling rule.
static void check_pool(const char* name, const std::vector<Brick>& pool) {
  const long long n = static_cast<long long>(pool.size());
  std::vector<long long> keys(pool.size());
  for (size_t s = 0; s < pool.size(); ++s) {
    CHECK(sg_in_range(pool[s][0], pool[s][1], pool[s][2]));
    keys[s] = sg_pack(pool[s][0], pool[s][1], pool[s][2]);
  }
  // the device sort: keys ascending with the slots they came from; exactly n entries (a vector of that size: a read past it is an error)
  std::vector<long long> index(pool.size());
  for (size_t s = 0; s < pool.size(); ++s) index[s] = static_cast<long long>(s);
  std::sort(index.begin(), index.end(), [&](long long a, long long b) { return keys[a] < keys[b]; });
  std::vector<long long> sorted(pool.size());
  for (size_t r = 0; r < pool.size(); ++r) sorted[r] = keys[index[r]];
  std::map<Brick, int> slot_of;
  for (size_t s = 0; s < pool.size(); ++s) slot_of[pool[s]] = static_cast<int>(s);
  CHECK(slot_of.size() == pool.size());

  // the search finds every key and nothing else
  for (long long r = 0; r < n; ++r) CHECK(se_find(sorted.data(), n, sorted[r]) == r);
  CHECK(se_find(sorted.data(), n, kBrickEmpty) == -1 && se_find(sorted.data(), n, kBrickEmpty - 1) == -1);
  CHECK(se_find(sorted.data(), 0, 0) == -1);

  // every neighbour entry equals a brute-force search
  std::vector<int> rows(pool.size() * kExtractRow);
  for (size_t s = 0; s < pool.size(); ++s)
    for (int entry = 0; entry < kExtractRow; ++entry) {
      const int got = se_neighbour(sorted.data(), index.data(), n, pool[s][0], pool[s][1], pool[s][2], entry);
      const Brick want = {pool[s][0] + entry / 9 - 1, pool[s][1] + (entry / 3) % 3 - 1, pool[s][2] + entry % 3 - 1};
      const auto it = slot_of.find(want);
      CHECK(got == (it == slot_of.end() ? -1 : it->second));
      rows[s * kExtractRow + entry] = got;
    }
  for (size_t s = 0; s < pool.size(); ++s) CHECK(rows[s * kExtractRow + 13] == static_cast<int>(s));

  // every voxel of every unallocated brick adjacent to the set (26-neighbourhood; out-of-range bricks included: they are nobody's)
  std::set<Brick> adjacent;
  for (const Brick& b : pool)
    for (int d = 0; d < 27; ++d) {
      const Brick u = {b[0] + d / 9 - 1, b[1] + (d / 3) % 3 - 1, b[2] + d % 3 - 1};
      if (!slot_of.count(u)) adjacent.insert(u);
    }
  long long handled_voxels = 0;
  for (const Brick& u : adjacent)
    for (int v = 0; v < 512; ++v) {
      const int lu[3] = {v >> 6, (v >> 3) & 7, v & 7};
      // brute force: the allocated brick of smallest key among those the voxel's cube touches
      int want = -1;
      long long want_key = kBrickEmpty;
      for (int e = 0; e < 8; ++e) {
        const int ev[3] = {e >> 2, (e >> 1) & 1, e & 1};
        if ((ev[0] && lu[0] != 7) || (ev[1] && lu[1] != 7) || (ev[2] && lu[2] != 7)) continue;
        const auto it = slot_of.find(Brick{u[0] + ev[0], u[1] + ev[1], u[2] + ev[2]});
        if (it != slot_of.end() && keys[it->second] < want_key) want = it->second, want_key = keys[it->second];
      }
      // the bricks that say they handle it: exactly the one above, or none
      int handlers = 0;
      for (size_t s = 0; s < pool.size(); ++s) {
        const int l[3] = {8 * (u[0] - pool[s][0]) + lu[0], 8 * (u[1] - pool[s][1]) + lu[1], 8 * (u[2] - pool[s][2]) + lu[2]};
        if (l[0] < -1 || l[0] > 8 || l[1] < -1 || l[1] > 8 || l[2] < -1 || l[2] > 8) continue;
        const int* row = &rows[s * kExtractRow];
        // every brick that can see the voxel names the same handler and the same cell
        int slot, cell;
        const bool any = se_handler(row, l[0], l[1], l[2], slot, cell);
        CHECK(any == (want >= 0) && slot == want);
        if (any) {
          const int hl[3] = {8 * (u[0] - pool[slot][0]) + lu[0], 8 * (u[1] - pool[slot][1]) + lu[1], 8 * (u[2] - pool[slot][2]) + lu[2]};
          CHECK(hl[0] >= -1 && hl[0] <= 7 && hl[1] >= -1 && hl[1] <= 7 && hl[2] >= -1 && hl[2] <= 7);
          CHECK(cell == (hl[0] + 1) * 81 + (hl[1] + 1) * 9 + (hl[2] + 1) && cell >= 0 && cell < kExtractCells);
        }
        // the count / emit side: the class mask of the brick itself
        if (l[0] <= 7 && l[1] <= 7 && l[2] <= 7 && se_handles_class(row, se_class(l[0], l[1], l[2]))) {
          ++handlers;
          CHECK(static_cast<int>(s) == want);
        }
      }
      CHECK(handlers == (want >= 0 ? 1 : 0));      // exactly one handler when a brick of its cube is allocated, none otherwise
      handled_voxels += handlers;
    }
  // a brick's own voxels are its own, and a voxel of another ALLOCATED brick is never taken over
  for (size_t s = 0; s < pool.size(); ++s) {
    const int* row = &rows[s * kExtractRow];
    for (int c = 0; c < 27; ++c) {
      const bool own = c / 9 != 0 && (c / 3) % 3 != 0 && c % 3 != 0;
      if (own) CHECK(se_handles_class(row, c));
      else if (se_handles_class(row, c)) {
        const Brick u = {pool[s][0] - (c / 9 == 0), pool[s][1] - ((c / 3) % 3 == 0), pool[s][2] - (c % 3 == 0)};
        CHECK(!slot_of.count(u));
      }
    }
    for (int lx = -1; lx <= 8; ++lx)
      for (int ly = -1; ly <= 8; ++ly)
        for (int lz = -1; lz <= 8; ++lz) {
          const Brick o = {pool[s][0] + se_floor8(lx), pool[s][1] + se_floor8(ly), pool[s][2] + se_floor8(lz)};
          const auto it = slot_of.find(o);
          if (it == slot_of.end()) continue;
          int slot, cell;
          CHECK(se_handler(row, lx, ly, lz, slot, cell) && slot == it->second);
          CHECK(cell == (lx - 8 * se_floor8(lx) + 1) * 81 + (ly - 8 * se_floor8(ly) + 1) * 9 + (lz - 8 * se_floor8(lz) + 1));
        }
  }
  std::printf("%-44s %3zu bricks, %3zu unallocated neighbours, %6lld of their voxels handled\n", name, pool.size(), adjacent.size(), handled_voxels);
}

int main() {
  const int L = kBrickLimit;
  check_pool("empty pool", {});
  check_pool("one brick", {{2, 2, 2}});
  check_pool("one brick at the origin", {{0, 0, 0}});
  check_pool("two sharing a face", {{2, 2, 2}, {2, 3, 2}});
  check_pool("two sharing an edge", {{2, 2, 2}, {3, 2, 3}});
  check_pool("two sharing a corner", {{2, 2, 2}, {3, 3, 3}});
  check_pool("two sharing a corner, the other diagonal", {{2, 3, 2}, {3, 2, 3}});
  {
    std::vector<Brick> block;
    for (int x = 2; x < 4; ++x)
      for (int y = 2; y < 4; ++y)
        for (int z = 2; z < 4; ++z)
          if (!(x == 2 && y == 3 && z == 2)) block.push_back({x, y, z});
    check_pool("2x2x2 minus one", block);
    std::reverse(block.begin(), block.end());
    check_pool("2x2x2 minus one, slots in descending key order", block);
  }
  {
    std::vector<Brick> shell;
    for (int x = -1; x <= 1; ++x)
      for (int y = -1; y <= 1; ++y)
        for (int z = -1; z <= 1; ++z)
          if (x || y || z) shell.push_back({x, y, z});
    check_pool("3x3x3 minus its centre, around the origin", shell);
  }
  check_pool("corners of the coordinate range", {{L, L, L}, {-L, -L, -L}, {L, -L, L}, {-L, L, -L}, {L - 1, L, L}, {-L, -L, -L + 1}});
  check_pool("slot order that is not key order", {{5, -3, 7}, {-4, 9, 0}, {5, -3, 6}, {4, -2, 7}, {-4, 8, 1}, {6, -4, 8}, {-5, 9, 1}, {5, -2, 7}});
  {
    // a pseudo-random cloud (a linear congruential generator: the same on every host) in a 4 x 4 x 4 box across zero
    std::vector<Brick> cloud;
    std::set<Brick> seen;
    unsigned state = 12345u;
    for (int i = 0; i < 40; ++i) {
      state = state * 1664525u + 1013904223u;
      const Brick b = {static_cast<int>((state >> 8) & 3) - 2, static_cast<int>((state >> 14) & 3) - 2, static_cast<int>((state >> 20) & 3) - 2};
      if (seen.insert(b).second) cloud.push_back(b);
    }
    check_pool("a cloud in a 4x4x4 box across zero", cloud);
  }
  // the search takes the same number of steps whatever the data: a pool of 2^20 consecutive keys, first, last and missing keys
  {
    std::vector<long long> sorted(1 << 20);
    for (size_t i = 0; i < sorted.size(); ++i) sorted[i] = 3 * static_cast<long long>(i) + 1;
    const long long n = static_cast<long long>(sorted.size());
    CHECK(se_find(sorted.data(), n, 1) == 0 && se_find(sorted.data(), n, 3 * (n - 1) + 1) == n - 1 && se_find(sorted.data(), n, 3 * 77777 + 1) == 77777);
    CHECK(se_find(sorted.data(), n, 0) == -1 && se_find(sorted.data(), n, 2) == -1 && se_find(sorted.data(), n, 3 * n + 1) == -1);
  }
  if (failures == 0) std::printf("sparse_extract_check: ok\n");
  else std::printf("sparse_extract_check: %d checks failed\n", failures);
  return failures == 0 ? 0 : 1;
}
