// Stand-alone check of deep-video-mvs_amd/csrc/sparse_grid.h on the host: built with the host compiler and
// -fsanitize=address,undefined by tests/test_sparse_reference.py (no GPU, no HIP).  Exit status 0 = every check passed.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/sparse_grid_check.cpp -o sparse_grid_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../deep-video-mvs_amd/csrc/sparse_grid.h"

using namespace dvmvs;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static void round_trip(int x, int y, int z) {
  CHECK(sg_in_range(x, y, z));
  const long long key = sg_pack(x, y, z);
  CHECK(key >= 0 && key != kBrickEmpty);
  int a, b, c;
  sg_unpack(key, a, b, c);
  CHECK(a == x && b == y && c == z);
}

int main() {
  // the key round-trips at the corners of the coordinate range, around zero and for negative coordinates
  const int edge[] = {-kBrickLimit, -kBrickLimit + 1, -9, -8, -1, 0, 1, 7, 8, kBrickLimit - 1, kBrickLimit};
  for (int x : edge)
    for (int y : edge)
      for (int z : edge) round_trip(x, y, z);
  CHECK(!sg_in_range(kBrickLimit + 1, 0, 0) && !sg_in_range(0, -kBrickLimit - 1, 0) && !sg_in_range(0, 0, 1 << 20));
  // ascending keys are the lexicographic order of (x, y, z), negative coordinates included
  CHECK(sg_pack(-1, 5, 5) < sg_pack(0, -5, -5) && sg_pack(0, -1, 5) < sg_pack(0, 0, -5) && sg_pack(0, 0, -1) < sg_pack(0, 0, 0));
  CHECK(sg_pack(-kBrickLimit, -kBrickLimit, -kBrickLimit) == 0);
  CHECK(sg_pack(kBrickLimit, kBrickLimit, kBrickLimit) < kBrickEmpty);
  // the probe sequence visits every slot of a power-of-two table exactly once, from any hash
  for (unsigned long long slots = 1; slots <= 4096; slots <<= 1) {
    const uint64_t mask = slots - 1;
    const long long keys[] = {0, sg_pack(0, 0, 0), sg_pack(-3, 2, -14), sg_pack(kBrickLimit, kBrickLimit, kBrickLimit), kBrickEmpty - 1};
    for (long long key : keys) {
      std::vector<int> seen(slots, 0);
      const uint64_t hash = sg_hash(key);
      for (uint64_t i = 0; i <= mask; ++i) {
        const uint64_t slot = sg_probe(hash, i, mask);
        CHECK(slot <= mask);
        if (slot <= mask) ++seen[slot];
      }
      for (unsigned long long s = 0; s < slots; ++s) CHECK(seen[s] == 1);
    }
  }
  // a bounded insert into a full table of 8 gives up after 8 attempts: the loop of mark_brick on the host
  {
    const uint64_t mask = 7;
    long long table[8];
    for (long long& t : table) t = kBrickEmpty;
    int stored = 0, dropped = 0;
    for (int n = 0; n < 20; ++n) {
      const long long key = sg_pack(n - 10, 3 * n, -n);
      const uint64_t hash = sg_hash(key);
      bool placed = false;
      for (uint64_t i = 0; i <= mask && !placed; ++i) {
        long long& t = table[sg_probe(hash, i, mask)];
        if (t == kBrickEmpty) t = key, ++stored;
        placed = t == key;
      }
      if (!placed) ++dropped;
    }
    CHECK(stored == 8 && dropped == 12);
  }
  // neighbouring bricks spread over a table (no more than a few per slot on average load 1/4)
  {
    const uint64_t mask = 4095;
    std::vector<int> load(4096, 0);
    int worst = 0;
    for (int x = -5; x < 5; ++x)
      for (int y = -5; y < 5; ++y)
        for (int z = -5; z < 5; ++z) {
          const int l = ++load[sg_hash(sg_pack(x, y, z)) & mask];
          if (l > worst) worst = l;
        }
    CHECK(worst <= 6);
  }
  if (failures == 0) std::printf("sparse_grid_check: ok\n");
  return failures == 0 ? 0 : 1;
}
