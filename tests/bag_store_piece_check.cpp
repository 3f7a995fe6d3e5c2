// Host walk of tt_bag_store_gather's id copy (jodalrob-twotower_amd/csrc/tt_bag_store_piece.h): for tiles of random runs -- empty
// runs, a 3000-id run, fewer samples than the tile holds, odd and even tile starts, a destination at 0 and at 8 mod 16 -- every
// piece the kernel's loop visits is planned by store_piece, and every position of the tile must be written exactly once, from the
// id the concatenation of the runs puts there, with every index inside its array.  Built and run by tests/test_bag_store_host.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "tt_bag_store_piece.h"

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      printf("FAILED %s (line %d)\n", #cond, __LINE__);                    \
      return 1;                                                            \
    }                                                                      \
  } while (0)

static int walk(int nb, int64_t before, int long_at, int64_t A, int split, int threads, int trip) {
  // the store: nnz ids, value = its own index; each sample's run somewhere in it
  const int64_t nnz = 20000;
  std::vector<int64_t> start(kStoreTile + 1), src(kStoreTile), run(kStoreTile);
  int64_t at = before;
  for (int t = 0; t < kStoreTile; ++t) {
    run[t] = t >= nb ? 0 : (t == long_at ? 3000 : (int64_t)(rnd() % 4 == 0 ? 0 : rnd() % 9));
    src[t] = (int64_t)(rnd() % (uint64_t)(nnz - run[t] + 1));
    start[t] = at;
    at += run[t];
  }
  start[kStoreTile] = at;
  const int64_t ts = start[0], te = start[kStoreTile];
  std::vector<int> written(te - ts, 0);
  std::vector<int64_t> out(te - ts, -1);
  if (te <= ts) return 0;
  const int64_t q_hi = (te - 1 + A) >> 1, stride = (int64_t)split * threads;
  for (int y = 0; y < split; ++y)
    for (int tid = 0; tid < threads; ++tid)
      for (int64_t q0 = ((ts + A) >> 1) + (int64_t)y * threads + tid; q0 <= q_hi; q0 += trip * stride)
        for (int j = 0; j < trip; ++j) {
          const int64_t q = q0 + j * stride;
          if (q > q_hi) continue;
          int64_t p0, i0, i1;
          const int lv = store_piece(start.data(), src.data(), ts, te, A, q, &p0, &i0, &i1);
          CHECK(lv != 0);
          if (lv & 1) {
            CHECK(p0 >= ts && p0 < te && i0 >= 0 && i0 < nnz);
            written[p0 - ts]++;
            out[p0 - ts] = i0;
          }
          if (lv & 2) {
            CHECK(p0 + 1 >= ts && p0 + 1 < te && i1 >= 0 && i1 < nnz);
            written[p0 + 1 - ts]++;
            out[p0 + 1 - ts] = i1;
          }
          if (lv == 3) CHECK(((p0 + A) & 1) == 0);                 // a whole piece lies on the destination's 16-byte grid
        }
  int64_t p = ts;
  for (int t = 0; t < kStoreTile; ++t)
    for (int64_t r = 0; r < run[t]; ++r, ++p) {
      CHECK(written[p - ts] == 1);
      CHECK(out[p - ts] == src[t] + r);
    }
  CHECK(p == te);
  return 0;
}

int main() {
  // store_find on its own: every boundary of a tile of single ids, and of one whose first samples are empty
  {
    std::vector<int64_t> start(kStoreTile + 1);
    for (int t = 0; t <= kStoreTile; ++t) start[t] = 100 + t;
    for (int t = 0; t < kStoreTile; ++t) CHECK(store_find(start.data(), 100 + t) == t);
    for (int t = 0; t <= kStoreTile; ++t) start[t] = t < 200 ? 7 : 7 + (t - 199);
    CHECK(store_find(start.data(), 7) == 199);
    for (int t = 0; t <= kStoreTile; ++t) start[t] = t == 0 ? 0 : 5;      // one sample: the whole tile is sample 0's run
    for (int64_t p = 0; p < 5; ++p) CHECK(store_find(start.data(), p) == 0);
  }
  int cases = 0;
  for (int nb : {1, 2, 63, 255, 256})
    for (int64_t before : {0, 1, 4097})
      for (int64_t A : {0, 1})
        for (int split : {1, 3, 16})
          for (int rep = 0; rep < 3; ++rep) {
            if (walk(nb, before, rep == 0 ? -1 : (int)(rnd() % (uint64_t)nb), A, split, 256, 4)) return 1;
            ++cases;
          }
  printf("ok %d\n", cases);
  return 0;
}
