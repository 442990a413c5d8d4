// shard_plan.h -- the host-side plan of a full-domain call that expands one
// key's tree as several independent subtree launches (EvaluateShardToDevice,
// EvaluateDotToDevice, EvaluateSelectToDevice, EvaluateDotBatchToDevice and
// the split first call of EvaluateUntil), as pure functions: which subtree a
// shard is, how many slabs a database fold cuts it into, and the tree paths
// of the subtrees' roots.
// Nothing here calls a dpf_hip_* entry point or touches a context, so a
// stand-alone program tests it (tests/cpp/shard_plan_test.cc).
#ifndef DPF_HOST_SHARD_PLAN_H_
#define DPF_HOST_SHARD_PLAN_H_

#include <algorithm>
#include <cstdint>
#include <optional>

#include "dpf/status.h"
#include "dpf/uint128.h"

namespace distributed_point_functions {
namespace dpf_internal {

// Shard `shard` of `num_shards` = 2^k is the subtree under the k-bit tree
// prefix `shard`; returns k.  `stop_level` is the tree depth of the hierarchy
// level, and a call's output has 2^(log_domain_size - k + extra_log_rows)
// rows: one per element (extra 0), or one per bit of an element (6 or 7).
inline StatusOr<int> ShardLevels(int64_t shard, int64_t num_shards, int stop_level,
                                 int log_domain_size, int extra_log_rows) {
  if (num_shards < 1 || (num_shards & (num_shards - 1)) || shard < 0 || shard >= num_shards)
    return InvalidArgumentError("num_shards must be a power of two and 0 <= shard < num_shards");
  int k = 0;
  while ((int64_t{1} << k) < num_shards) ++k;
  if (k > stop_level) return InvalidArgumentError("more shards than subtrees at this level");
  if (log_domain_size - k + extra_log_rows > 62)
    return InvalidArgumentError(
        "Output size would be larger than 2**62. Please evaluate fewer hierarchy levels at once.");
  return k;
}

// A streamed database fold expands its shard slab by slab into scratch: 2^j
// slabs of `slab_rows` rows each.
struct SlabPlan {
  int j;
  int64_t slabs, slab_rows;
};
constexpr int64_t kSlabScratchBits = int64_t{1} << 31;   // 256 MiB of scratch per slab
constexpr int kMaxSlabLevels = 20;                       // at most 2^20 slabs per call

// Cuts `rows` (2^L leaf blocks of `block_rows` rows, which no slab splits)
// into the fewest slabs of at most max(cap, block_rows) rows.  The cap is
// 2^slab_log with the test hook's value clamped to [0, 62], else the largest
// 2^s rows whose scratch (`row_bits` each) stays within kSlabScratchBits.
inline StatusOr<SlabPlan> PlanSlabs(int64_t rows, int64_t block_rows, int64_t row_bits,
                                    std::optional<int> slab_log) {
  int cap_log = 0;
  if (slab_log) {
    cap_log = std::min(std::max(*slab_log, 0), 62);
  } else {
    while ((int64_t{2} << cap_log) * row_bits <= kSlabScratchBits) ++cap_log;
  }
  const int64_t cap = std::max(int64_t{1} << cap_log, block_rows);
  int j = 0;
  while ((rows >> j) > cap) ++j;
  if (j > kMaxSlabLevels)
    return InvalidArgumentError("the database fold would take more than 2**20 slabs");
  return SlabPlan{j, int64_t{1} << j, rows >> j};
}

// Tree path of part i of the 2^j subtrees under `prefix`.
inline uint128 SubtreePath(int64_t prefix, int j, int64_t i) {
  return (static_cast<uint128>(prefix) << j) | static_cast<uint128>(i);
}

}  // namespace dpf_internal
}  // namespace distributed_point_functions

#endif  // DPF_HOST_SHARD_PLAN_H_
