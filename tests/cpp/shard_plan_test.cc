// The host-side plan of the shard, dot, select and split calls
// (csrc/host/shard_plan.h), checked without a GPU: the slab plan against the
// two loops it replaced, restated literally; the shard split against its
// definition, with its three messages and the 2^62 boundary; the subtree
// paths against (shard << j) | i.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <optional>
#include <string>

#include "shard_plan.h"

using distributed_point_functions::StatusOr;
using distributed_point_functions::uint128;
using namespace distributed_point_functions::dpf_internal;

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// ------------------------------------------------------------------- slabs
constexpr int64_t kDotSlabBytes = int64_t{256} << 20;
constexpr int kDotMaxSlabLevels = 20;

// EvaluateDotToDevice's loop as it stood (streamed path).  j < 0: the error.
static void OldDotSlabs(int64_t rows, int cepb, int64_t esz, std::optional<int> hook, int* j_out,
                        int64_t* slabs, int64_t* slab_rows_out) {
  int j = 0;
  int slab_log = 0;
  while ((int64_t{2} << slab_log) * esz <= kDotSlabBytes) ++slab_log;
  if (hook) slab_log = *hook;
  int64_t slab_rows = int64_t{1} << std::min(std::max(slab_log, 0), 62);
  if (slab_rows < cepb) slab_rows = cepb;
  while ((rows >> j) > slab_rows) ++j;
  if (j > kDotMaxSlabLevels) {
    *j_out = -1;
    return;
  }
  *j_out = j;
  *slabs = int64_t{1} << j;
  *slab_rows_out = rows >> j;
}

// EvaluateSelectToDevice's loop as it stood.
static void OldSelectSlabs(int64_t rows, int L, int64_t Q, std::optional<int> hook, int* j_out,
                           int64_t* slabs, int64_t* slab_rows_out) {
  int slab_log = 7;
  while ((int64_t{2} << slab_log) * Q / 8 <= kDotSlabBytes) ++slab_log;
  if (hook) slab_log = std::min(std::max(*hook, 7), 62);
  int j = 0;
  while (j < L && (rows >> j) > (int64_t{1} << slab_log)) ++j;
  if (j > kDotMaxSlabLevels) {
    *j_out = -1;
    return;
  }
  *j_out = j;
  *slabs = int64_t{1} << j;
  *slab_rows_out = rows >> j;
}

static void CheckSame(const StatusOr<SlabPlan>& got, int j, int64_t slabs, int64_t slab_rows) {
  if (j < 0) {
    CHECK(!got.ok());
    if (!got.ok())
      CHECK(got.status().message() == "the database fold would take more than 2**20 slabs");
    return;
  }
  CHECK(got.ok());
  if (got.ok()) CHECK(got->j == j && got->slabs == slabs && got->slab_rows == slab_rows);
}

static long TestSlabPlan() {
  long cases = 0;
  for (int L = 0; L <= 39; ++L)
    for (int hook = -3; hook <= 40; ++hook) {   // -3: no hook; 40: clamped from far above
      std::optional<int> h;
      if (hook >= -2) h = hook == 40 ? 1000 : hook;
      // dot: uint64 (two per block) and 128-bit (one per block) elements.
      for (int esz : {8, 16}) {
        const int cepb = 16 / esz;
        const int64_t rows = (int64_t{1} << L) * cepb;
        int j = 0;
        int64_t slabs = 0, slab_rows = 0;
        OldDotSlabs(rows, cepb, esz, h, &j, &slabs, &slab_rows);
        CheckSame(PlanSlabs(rows, cepb, 8 * esz, h), j, slabs, slab_rows);
        ++cases;
      }
      // select: 128 records per leaf block, one scratch bit per record and key.
      const int64_t rows = (int64_t{1} << L) * 128;
      for (int64_t Q = 1; Q <= 64; ++Q) {
        int j = 0;
        int64_t slabs = 0, slab_rows = 0;
        OldSelectSlabs(rows, L, Q, h, &j, &slabs, &slab_rows);
        CheckSame(PlanSlabs(rows, 128, Q, h), j, slabs, slab_rows);
        ++cases;
      }
    }
  // The defaults, spelled out: 2^25 uint64 per slab; 2^31 / Q record bits.
  CHECK(PlanSlabs(int64_t{1} << 30, 2, 64, std::nullopt)->slab_rows == int64_t{1} << 25);
  CHECK(PlanSlabs(int64_t{1} << 30, 1, 128, std::nullopt)->slab_rows == int64_t{1} << 24);
  CHECK(PlanSlabs(int64_t{1} << 35, 128, 1, std::nullopt)->slab_rows == int64_t{1} << 31);
  CHECK(PlanSlabs(int64_t{1} << 35, 128, 3, std::nullopt)->slab_rows == int64_t{1} << 29);
  CHECK(PlanSlabs(int64_t{1} << 35, 128, 64, std::nullopt)->slab_rows == int64_t{1} << 25);
  // The 2^20 cap on either side.
  CHECK(PlanSlabs(int64_t{1} << 20, 1, 128, 0)->slabs == int64_t{1} << 20);
  CHECK(!PlanSlabs(int64_t{1} << 21, 1, 128, 0).ok());
  return cases;
}

// ------------------------------------------------------------- shard split
static const char kBadShard[] = "num_shards must be a power of two and 0 <= shard < num_shards";
static const char kMoreShards[] = "more shards than subtrees at this level";
static const char kTooLarge[] =
    "Output size would be larger than 2**62. Please evaluate fewer hierarchy levels at once.";

static void ExpectError(const StatusOr<int>& got, const char* message) {
  CHECK(!got.ok());
  if (got.ok()) return;
  CHECK(got.status().code() == distributed_point_functions::StatusCode::kInvalidArgument);
  CHECK(got.status().message() == message);
}

static void TestShardLevels() {
  // Every power of two up to the tree's leaves, every shard at the ends.
  for (int stop_level : {0, 1, 5, 20})
    for (int k = 0; k <= stop_level; ++k) {
      const int64_t n = int64_t{1} << k;
      for (int64_t shard : {int64_t{0}, n / 2, n - 1}) {
        StatusOr<int> got = ShardLevels(shard, n, stop_level, stop_level + 1, 0);
        CHECK(got.ok() && *got == k);
      }
      ExpectError(ShardLevels(n, n, stop_level, stop_level + 1, 0), kBadShard);
      ExpectError(ShardLevels(-1, n, stop_level, stop_level + 1, 0), kBadShard);
    }
  for (int64_t n : {int64_t{0}, int64_t{-4}, int64_t{3}, int64_t{6}, (int64_t{1} << 40) + 1})
    ExpectError(ShardLevels(0, n, 50, 50, 0), kBadShard);
  // The order: shard arguments, then the tree's depth, then the output size.
  ExpectError(ShardLevels(0, 3, 1, 100, 0), kBadShard);
  ExpectError(ShardLevels(0, 4, 1, 100, 0), kMoreShards);
  ExpectError(ShardLevels(0, int64_t{1} << 6, 5, 6, 0), kMoreShards);
  CHECK(ShardLevels(0, int64_t{1} << 5, 5, 6, 0).ok());
  ExpectError(ShardLevels(0, 2, 5, 100, 0), kTooLarge);
  // log_domain_size - k + extra == 62 passes, 63 does not.
  for (int extra : {0, 6, 7})
    for (int k : {0, 1, 9}) {
      const int64_t n = int64_t{1} << k;
      StatusOr<int> at = ShardLevels(n - 1, n, 60, 62 + k - extra, extra);
      CHECK(at.ok() && *at == k);
      ExpectError(ShardLevels(n - 1, n, 60, 63 + k - extra, extra), kTooLarge);
    }
  // The most shards a call can name: 2^62.
  StatusOr<int> most = ShardLevels(5, int64_t{1} << 62, 70, 71, 0);
  CHECK(most.ok() && *most == 62);
}

// ------------------------------------------------------------------- paths
static void TestSubtreePaths() {
  for (int64_t shard : {int64_t{0}, int64_t{1}, int64_t{5}, (int64_t{1} << 62) - 1})
    for (int j : {0, 1, 2, 7, 20}) {
      const int64_t parts = int64_t{1} << j;
      for (int64_t i : {int64_t{0}, parts / 2, parts - 1}) {
        const uint128 got = SubtreePath(shard, j, i);
        CHECK(got == (static_cast<uint128>(shard) << j | static_cast<uint128>(i)));
        CHECK(static_cast<int64_t>(got & (static_cast<uint128>(parts) - 1)) == i);   // low j bits
        CHECK(static_cast<int64_t>(got >> j) == shard);                              // the rest
      }
    }
  // Four shards of four slabs: slab 1 of shard 3 is tree node 13 at depth 4.
  CHECK(SubtreePath(3, 2, 1) == 13);
  // One part is the shard's own prefix; a wide shard index keeps its top bits.
  CHECK(SubtreePath(9, 0, 0) == 9);
  CHECK(SubtreePath(int64_t{1} << 61, 20, 3) == ((static_cast<uint128>(1) << 81) | 3));
}

int main() {
  const long cases = TestSlabPlan();
  TestShardLevels();
  TestSubtreePaths();
  std::printf("slab cases %ld\n", cases);
  std::printf("%d failures\n", failures);
  return failures != 0;
}
