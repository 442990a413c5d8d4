// batch_context.cc -- incremental evaluation of a whole key batch with a
// device-resident EvaluationContext (config 5b, the
// heavy-hitters hierarchy over 2^20 client keys).
//
// EvaluateUntilBatch*(h, prefixes, ctx) computes, for every key k of the batch,
// exactly what EvaluateUntil<T>(h, prefixes, ctx_k)
// (distributed_point_function.h:641-837) returns, and leaves the batch
// context in the state the per-key contexts would be in:
//   * validation and error messages of EvaluateUntil (h:655-700);
//   * unique tree indices of the prefixes in first-seen order (h:718-742);
//   * ComputePartialEvaluations (cc:351-453): each tree index is found under
//     its parent among the stored partial evaluations (or walked from the
//     root), walked down on the GPU, and stored as the new partial evaluation
//     unless this is the last hierarchy level;
//   * ExpandSeeds + HashExpandedSeeds + correction (cc:271-349, 500-524;
//     h:745-808) and the per-prefix gather (h:817-836).
// The host does O(#prefixes) bookkeeping per call; every per-key step runs in
// one dpf_hip_prefix_batch_level launch (csrc/kernels/dpf_batch.hip).
#include <algorithm>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "dpf/distributed_point_function.h"
#include "dpf/key_batch.h"
#include "dpf_hip.h"
#include "host_util.h"
#include "until_plan.h"

namespace distributed_point_functions {

using dpf_internal::AesKey;
using dpf_internal::FromBlock;
using dpf_internal::FromHip;
using dpf_internal::kPrgKeyLeft;
using dpf_internal::kPrgKeyRight;
using dpf_internal::kPrgKeyValue;
using dpf_internal::MakeDesc;
using dpf_internal::SetProtoBlock;
using dpf_internal::ToBlock;
using dpf_internal::hook_is;
using dpf_internal::hook_long;
using dpf_internal::hook_str;
using dpf_internal::PhaseTimer;
using dpf_internal::StartSource;
using dpf_internal::UntilBatchArgs;
using dpf_internal::UntilBatchShape;

namespace {
// Host-phase timing of the batched path, printed at exit when
// DPF_BATCH_HOST_TIMING is set (diagnostics for config 5a's host-bound levels).
PhaseTimer g_timing("DPF_BATCH_HOST_TIMING", 0, [](long calls, double, const double* t) {
  std::fprintf(stderr,
               "[batch host timing] calls=%ld dedup=%.3fs lookup=%.3fs tables=%.3fs "
               "upload=%.3fs device=%.3fs update=%.3fs\n",
               calls, t[0], t[1], t[2], t[3], t[4], t[5]);
});
// DPF_BATCH_NO_CACHE=1 turns the expansion cache off (every call walks down
// from the partial evaluations, as the reference does): an A/B and test hook.
bool CacheOn() { return !hook_is("DPF_BATCH_NO_CACHE", '1'); }
// How a call that reads the expansion cache writes the next one.  Default:
// into a spare buffer if one fits, else in place through a slot table, else
// (no slot table possible) in place after gathering the start seeds.
// DPF_BATCH_CACHE_MODE=spare|permute|gather forces one (a spare still only if
// it fits; permute falls back to gather when no slot table exists), and
// DPF_BATCH_CACHE_IN_PLACE=1 means gather: test and A/B hooks, read per call.
enum class CacheMode { kAuto, kSpare, kPermute, kGather };
CacheMode ForcedCacheMode() {
  if (hook_is("DPF_BATCH_CACHE_IN_PLACE", '1')) return CacheMode::kGather;
  const std::string s = hook_str("DPF_BATCH_CACHE_MODE");
  if (s == "spare") return CacheMode::kSpare;
  if (s == "permute") return CacheMode::kPermute;
  if (s == "gather") return CacheMode::kGather;
  return CacheMode::kAuto;
}

// Host buffers are recycled across calls (per thread): first touches of fresh
// pages cost more than the bookkeeping itself at 1 M prefixes per level
// (config 5a).  Not cleared first: every element a call reads it has written
// before, so vectors kept from an earlier call of about this size
// value-initialise nothing (clearing them had cost a 1 M-prefix level ~3.8 ms
// of single-threaded zeroing, r16 DPF_BATCH_HOST_TIMING).
// Start nodes are indexed by int32 on the device, so 32-bit positions
// suffice: 8-byte (position, block index) entries.
thread_local std::vector<std::pair<int32_t, int>> tl_prefix_map;
thread_local std::vector<int32_t> tl_parent_of;   // position of each tree index's stored prefix
thread_local std::vector<int64_t> tl_start_slot;  // physical cache slot of each tree index's node
thread_local std::vector<int32_t> tl_leaf_slot;   // slot table of an in-place rewrite
}  // namespace

// DPF_BATCH_ALLOC_LIMIT=<bytes>: a test hook that makes a batch context behave
// as if the device had only that much memory for it -- an allocation that
// would take the context's total above the limit fails like hipMalloc's
// out-of-memory, and MemInfo reports the limit -- so the expansion cache's
// fallbacks (no spare, eviction and retry, RESOURCE_EXHAUSTED) run
// deterministically.  Read per call.
size_t AllocLimit() { return static_cast<size_t>(hook_long("DPF_BATCH_ALLOC_LIMIT", 0)); }

bool DeviceBatchContext::TryAlloc(void** p, size_t* cap, size_t bytes) {
  *p = nullptr;
  *cap = 0;
  const size_t limit = AllocLimit();
  if (limit && device_bytes_ + bytes > limit) return false;
  if (dpf_hip_alloc(p, bytes) != 0) {
    *p = nullptr;
    return false;
  }
  *cap = bytes;
  device_bytes_ += bytes;
  return true;
}

void DeviceBatchContext::Release(void** p, size_t* cap) {
  if (*p) dpf_hip_free(*p);
  device_bytes_ -= std::min(device_bytes_, *cap);
  *p = nullptr;
  *cap = 0;
}

void DeviceBatchContext::MemInfo(size_t* free_bytes, size_t* total_bytes) const {
  *free_bytes = *total_bytes = 0;
  if (const size_t limit = AllocLimit()) {
    *total_bytes = limit;
    *free_bytes = limit - std::min(limit, device_bytes_);
    return;
  }
  (void)dpf_hip_mem_info(free_bytes, total_bytes);
}

Status DeviceBatchContext::Ensure(void** p, size_t* cap, size_t bytes) {
  if (fail_next_ > 0 && fail_skip_ > 0) {
    --fail_skip_;
  } else if (fail_next_ > 0) {
    --fail_next_;
    Release(p, cap);
    ++events_.alloc_failures;
    return ResourceExhaustedError("Memory allocation error");
  }
  if (*p && *cap >= bytes) return OkStatus();
  Release(p, cap);
  if (!TryAlloc(p, cap, std::max<size_t>(bytes, 256))) {
    ++events_.alloc_failures;
    return ResourceExhaustedError("Memory allocation error");  // cc:289-291
  }
  return OkStatus();
}

void DeviceBatchContext::ReleaseExpansionCache() {
  // hipFree waits for the device work that may still read the buffers.
  Release(&leaf_seeds_, &leaf_seeds_cap_);
  Release(&leaf_spare_, &leaf_spare_cap_);
  Release(&slots_, &slots_cap_);
  Release(&leaf_slot_, &leaf_slot_cap_);
  leaf_phys_.clear();
  leaf_level_ = -1;
}

void DeviceBatchContext::Reset(bool release_expansion_cache) {
  previous_hierarchy_level_ = -1;
  partial_evaluations_level_ = -1;
  partial_prefixes_.clear();
  partial_sorted_ = false;
  leaf_level_ = -1;
  if (release_expansion_cache) {
    (void)dpf_hip_stream_sync(nullptr);  // work still reading the cache
    ReleaseExpansionCache();
  }
}

DeviceBatchContext::~DeviceBatchContext() {
  if (tables_pending_) (void)dpf_hip_event_sync(tables_event_);
  if (tables_event_) dpf_hip_event_destroy(tables_event_);
  if (pinned_tables_) dpf_hip_host_free(pinned_tables_);
  for (void* p : {seeds_, ctrl_, next_seeds_, next_ctrl_, parent_, workspace_, stage_, stage2_,
                  leaf_seeds_, leaf_spare_, slots_, leaf_slot_, sketch_w_, sketch_acc_})
    if (p) dpf_hip_free(p);
}

bool DeviceBatchContext::Fits(size_t bytes, size_t reserve_div) const {
  size_t free_b = 0, total_b = 0;
  MemInfo(&free_b, &total_b);
  return free_b >= bytes + total_b / reserve_div;
}

Status DeviceBatchContext::GrowCache(size_t bytes, void* stream) {
  if (leaf_seeds_cap_ >= bytes) return OkStatus();
  HIP_RETURN_IF_ERROR(dpf_hip_stream_sync(stream));
  Release(&leaf_seeds_, &leaf_seeds_cap_);
  if (!Fits(bytes, 8) || !TryAlloc(&leaf_seeds_, &leaf_seeds_cap_, bytes)) ++events_.cache_refused;
  return OkStatus();
}

// This call's leaves become the next call's expansion cache (not after the
// last level).  Preferred: write them to the spare buffer while the kernel
// reads the start seeds straight from the current cache, then swap.  With
// no room for a spare, the cache is rewritten in place; a failed allocation
// only turns the cache off.
StatusOr<DeviceBatchContext::CacheTarget> DeviceBatchContext::ChooseCacheTarget(
    bool writes_cache, bool cached, int64_t leaf_stride, const std::vector<int64_t>& start_slot,
    int64_t T, int s, int E, std::vector<int32_t>* leaf_slot, void* stream) {
  CacheTarget t;
  t.stride = leaf_stride;
  t.cache_in_use = cached;
  if (!writes_cache) return t;
  const size_t cache_need = static_cast<size_t>(keys_->num_keys() * leaf_stride) * sizeof(dpf_block);
  if (!cached) {
    // The current cache is not read by this call: rewrite (or regrow) it.
    leaf_level_ = -1;  // until this call has written it
    DPF_RETURN_IF_ERROR(GrowCache(cache_need, stream));
    t.leaf_seeds = leaf_seeds_;
    return t;
  }
  const CacheMode mode = ForcedCacheMode();
  const bool want_spare = mode == CacheMode::kAuto || mode == CacheMode::kSpare;
  if (want_spare && leaf_spare_cap_ < cache_need) {
    // The spare may still be read by work in flight on the stream.
    HIP_RETURN_IF_ERROR(dpf_hip_stream_sync(stream));
    Release(&leaf_spare_, &leaf_spare_cap_);
    if (!Fits(cache_need, 4) || !TryAlloc(&leaf_spare_, &leaf_spare_cap_, cache_need))
      ++events_.spare_refused;
  }
  if (want_spare && leaf_spare_ && leaf_spare_cap_ >= cache_need) {
    t.leaf_seeds = leaf_spare_;
    t.swap = true;
  } else if (mode != CacheMode::kGather && leaf_stride <= leaf_stride_ &&
             dpf_internal::BuildSlotTable(start_slot, T, s, E, leaf_stride_, leaf_slot)) {
    // In place through the slot table: no gather, no second buffer.
    t.permute = true;
    t.leaf_seeds = leaf_seeds_;
    t.stride = leaf_stride_;
    ++events_.permuted;
  } else {
    t.gather = true;  // leaf_seeds is set once the gather is enqueued
    ++events_.in_place;
  }
  return t;
}

Status DeviceBatchContext::EnsureEvicting(void** p, size_t* cap, size_t bytes, CacheTarget* target,
                                          void* stream) {
  Status st = Ensure(p, cap, bytes);
  for (int step = 0; !st.ok() && step < 2; ++step) {
    void** victim = step == 0 ? &leaf_spare_ : &leaf_seeds_;
    size_t* victim_cap = step == 0 ? &leaf_spare_cap_ : &leaf_seeds_cap_;
    if (!*victim || (step == 1 && target->cache_in_use)) continue;
    HIP_RETURN_IF_ERROR(dpf_hip_stream_sync(stream));
    if (target->leaf_seeds == *victim) {
      target->leaf_seeds = nullptr;  // this call writes no cache
      target->swap = false;
    }
    Release(victim, victim_cap);
    ++(step == 0 ? events_.evicted_spare : events_.evicted_cache);
    if (step == 1) leaf_level_ = -1;
    st = Ensure(p, cap, bytes);
  }
  return st;
}

Status DeviceBatchContext::SendTables(size_t bytes, CacheTarget* target, void* stream) {
  DPF_RETURN_IF_ERROR(EnsureEvicting(&parent_, &parent_cap_, bytes, target, stream));
  HIP_RETURN_IF_ERROR(dpf_hip_memcpy_h2d_async(parent_, pinned_tables_, bytes, stream));
  return TablesSent(stream);
}

Status DeviceBatchContext::GatherStartSeeds(const std::vector<int64_t>& start_slot, int64_t T,
                                            int64_t leaf_stride, CacheTarget* target,
                                            void* stream) {
  const int64_t K = keys_->num_keys();
  DPF_RETURN_IF_ERROR(EnsureEvicting(&slots_, &slots_cap_, T * sizeof(int64_t), target, stream));
  HIP_RETURN_IF_ERROR(dpf_hip_memcpy_h2d(slots_, start_slot.data(), T * sizeof(int64_t), stream));
  HIP_RETURN_IF_ERROR(dpf_hip_gather_seeds_layout(
      K, T, static_cast<const int64_t*>(slots_), static_cast<const dpf_block*>(leaf_seeds_),
      leaf_stride_, static_cast<dpf_block*>(next_seeds_), static_cast<uint8_t*>(next_ctrl_),
      index_major_ ? 1 : 0, stream));
  target->cache_in_use = false;  // copied out; from here on only the write target
  leaf_level_ = -1;              // rewritten in place by this call's kernel
  // Regrow once the gather has read the old cache.
  DPF_RETURN_IF_ERROR(
      GrowCache(static_cast<size_t>(K * leaf_stride) * sizeof(dpf_block), stream));
  target->leaf_seeds = leaf_seeds_;
  return OkStatus();
}

Status DeviceBatchContext::SendSlotTable(const std::vector<int32_t>& leaf_slot, CacheTarget* target,
                                         void* stream) {
  const size_t bytes = leaf_slot.size() * sizeof(int32_t);
  DPF_RETURN_IF_ERROR(EnsureEvicting(&leaf_slot_, &leaf_slot_cap_, bytes, target, stream));
  HIP_RETURN_IF_ERROR(dpf_hip_memcpy_h2d(leaf_slot_, leaf_slot.data(), bytes, stream));
  leaf_level_ = -1;  // rewritten in place by this call's kernel
  return OkStatus();
}

void DeviceBatchContext::CommitCache(const CacheTarget& target, int hierarchy_level, int de,
                                     bool last_level, const std::vector<int32_t>& leaf_slot) {
  if (target.swap) {
    std::swap(leaf_seeds_, leaf_spare_);
    std::swap(leaf_seeds_cap_, leaf_spare_cap_);
  }
  leaf_level_ = target.leaf_seeds ? hierarchy_level : -1;
  leaf_de_ = de;
  leaf_stride_ = target.stride;
  if (target.permute)
    leaf_phys_.assign(leaf_slot.begin(), leaf_slot.end());
  else
    leaf_phys_.clear();  // written in leaf order
  // After the last level nothing reads the cache; its buffers stay allocated
  // for the next pass over the hierarchy (Reset()), because giving them back
  // and regrowing them level by level (4, 16, 64 GiB for 2^20 heavy-hitters
  // clients) cost 3.7 s per 22 s pass (profiles/r14_ab.txt).  The 1/8-of-HBM
  // headroom rule (GrowCache) bounds what they take; callers that need the
  // memory call ReleaseExpansionCache() (or Reset(true)).
  if (last_level) leaf_level_ = -1;
}

void DeviceBatchContext::CommitPartials(int hierarchy_level, int prev_level, bool has_prefixes,
                                        bool update, bool ascending,
                                        std::vector<uint128>* tree_indices) {
  previous_hierarchy_level_ = hierarchy_level;
  if (has_prefixes) {
    if (update) {
      std::swap(partial_prefixes_, *tree_indices);
      partial_sorted_ = ascending;
      std::swap(seeds_, next_seeds_);
      std::swap(seeds_cap_, next_seeds_cap_);
      std::swap(ctrl_, next_ctrl_);
      std::swap(ctrl_cap_, next_ctrl_cap_);
    } else {
      partial_prefixes_.clear();
      partial_sorted_ = false;
    }
    partial_evaluations_level_ = prev_level;
  }
  spare_prefixes_ = std::move(*tree_indices);
}

Status DeviceBatchContext::StageTables(size_t bytes) {
  if (tables_pending_) {
    HIP_RETURN_IF_ERROR(dpf_hip_event_sync(tables_event_));
    tables_pending_ = false;
  }
  if (pinned_tables_cap_ >= bytes && pinned_tables_) return OkStatus();
  if (pinned_tables_) dpf_hip_host_free(pinned_tables_);
  pinned_tables_ = nullptr;
  pinned_tables_cap_ = 0;
  const size_t want = std::max<size_t>(bytes + bytes / 2, size_t{1} << 16);
  if (dpf_hip_host_alloc(&pinned_tables_, want) != 0) {
    pinned_tables_ = nullptr;
    return ResourceExhaustedError("Memory allocation error");
  }
  pinned_tables_cap_ = want;
  return OkStatus();
}

Status DeviceBatchContext::TablesSent(void* stream) {
  if (!tables_event_) HIP_RETURN_IF_ERROR(dpf_hip_event_create(&tables_event_));
  HIP_RETURN_IF_ERROR(dpf_hip_event_record(tables_event_, stream));
  tables_pending_ = true;
  return OkStatus();
}

StatusOr<std::unique_ptr<DeviceBatchContext>> DistributedPointFunction::CreateBatchEvaluationContext(
    const DeviceKeyBatch& keys) const {
  if (keys.num_levels() != tree_levels_needed() - 1 ||
      keys.num_hierarchy_levels() != static_cast<int>(parameters().size()))
    return InvalidArgumentError("key batch does not match this DistributedPointFunction");
  std::unique_ptr<DeviceBatchContext> ctx(new DeviceBatchContext(&keys));
  // DPF_BATCH_KEY_MAJOR=1 (read at creation: one layout per context) keeps
  // the r15 key-major tables and lanes = start nodes (A/B and test hook).
  ctx->index_major_ = !hook_is("DPF_BATCH_KEY_MAJOR", '1');
  return ctx;
}

StatusOr<int64_t> DistributedPointFunction::EvaluateUntilBatchToDevice(
    int hierarchy_level, Span<const uint128> prefixes, DeviceBatchContext& ctx, void* device_out,
    int64_t capacity_bytes, void* stream) const {
  return EvaluateUntilBatchCore(hierarchy_level, prefixes, ctx, false, device_out, capacity_bytes,
                                stream);
}

StatusOr<int64_t> DistributedPointFunction::EvaluateUntilBatchSumToDevice(
    int hierarchy_level, Span<const uint128> prefixes, DeviceBatchContext& ctx, void* device_out,
    int64_t capacity_bytes, void* stream) const {
  return EvaluateUntilBatchCore(hierarchy_level, prefixes, ctx, true, device_out, capacity_bytes,
                                stream);
}

// The sketch output mode of a batched call: J rows of n weights in, K * J * nl
// uint32 out (include/dpf_hip.h, dpf_hip_sketch_rows).
struct DistributedPointFunction::BatchSketch {
  const uint32_t* weights;
  int rows;
  int64_t per_row;
  uint32_t* out;
  int64_t capacity_bytes;
};

StatusOr<int64_t> DistributedPointFunction::EvaluateUntilBatchSketchToDevice(
    int hierarchy_level, Span<const uint128> prefixes, DeviceBatchContext& ctx,
    const uint32_t* device_weights, int num_weight_rows, int64_t weights_per_row,
    void* device_sums, int64_t sums_capacity_bytes, uint32_t* device_sketch,
    int64_t sketch_capacity_bytes, void* stream) const {
  const BatchSketch sketch{device_weights, num_weight_rows, weights_per_row, device_sketch,
                           sketch_capacity_bytes};
  return EvaluateUntilBatchCore(hierarchy_level, prefixes, ctx, device_sums != nullptr,
                                device_sums, sums_capacity_bytes, stream, &sketch);
}

// EvaluateUntil's argument checks (h:655-700), in the reference's order.
Status DistributedPointFunction::CheckUntilBatchArgs(int hierarchy_level,
                                                     Span<const uint128> prefixes,
                                                     const DeviceBatchContext& ctx) const {
  const DeviceKeyBatch& keys = ctx.keys();
  const int H = static_cast<int>(parameters().size());
  if (keys.num_levels() != tree_levels_needed() - 1 || keys.num_hierarchy_levels() != H)
    return InvalidArgumentError("key batch does not match this DistributedPointFunction");
  if (hierarchy_level < 0 || hierarchy_level >= H)
    return InvalidArgumentError(
        "`hierarchy_level` must be non-negative and less than parameters_.size()");
  const int prev = ctx.previous_hierarchy_level_;
  if (hierarchy_level <= prev)
    return InvalidArgumentError(
        "`hierarchy_level` must be greater than `ctx.previous_hierarchy_level`");
  if ((prev < 0) != prefixes.empty())
    return InvalidArgumentError(
        "`prefixes` must be empty if and only if this is the first call with `ctx`.");
  int prev_log = 0;
  if (!prefixes.empty()) {
    prev_log = parameters()[prev].log_domain_size();
    const int64_t bad = dpf_internal::FirstOutOfRangePrefix(prefixes, prev_log);
    if (bad < static_cast<int64_t>(prefixes.size()))
      return InvalidArgumentError("Index " + Uint128ToString(prefixes[bad]) +
                                  " out of range for hierarchy level " + std::to_string(prev));
  }
  if (parameters()[hierarchy_level].log_domain_size() - prev_log > 62)
    return InvalidArgumentError(
        "Output size would be larger than 2**62. Please evaluate fewer hierarchy levels at once.");
  return OkStatus();
}

// What one batched call works out on the host before it touches the device.
struct DistributedPointFunction::BatchCall {
  std::vector<uint128> tree_indices;  // unique, first-seen order (the root alone without prefixes)
  bool indices_ascending = false;     // tree_indices strictly ascending
  std::vector<std::pair<int32_t, int>>& prefix_map = tl_prefix_map;
  std::vector<int32_t>& parent_of = tl_parent_of;
  std::vector<int64_t>& start_slot = tl_start_slot;
  std::vector<int32_t>& leaf_slot = tl_leaf_slot;
  bool cache_on = false;
  int start_level = 0;  // tree depth of the stored partial evaluations the call starts from
  StartSource source = StartSource::kRoot;
  dpf_value_desc desc;
  bool native_sum = false;  // the kernel sums over the keys itself
  bool fused_sketch = false;  // the key-sum kernel also computes the sketches
  UntilBatchShape shape;
  DeviceBatchContext::CacheTarget target;  // where the call's leaves go
  dpf_internal::TableLayout tables;        // the start-node table image
};

// Where each of the call's tree indices (c->tree_indices, of P prefixes)
// starts -- a stored partial evaluation or the root (ExpandAndUpdateContext
// cc:455-498, ComputePartialEvaluations cc:351-453) -- and the call's shape.
Status DistributedPointFunction::PlanBatchCall(int hierarchy_level, int64_t P,
                                               const DeviceBatchContext& ctx, bool sum,
                                               BatchCall* c) const {
  const int prev = ctx.previous_hierarchy_level_;
  const int prev_log = P > 0 ? parameters()[prev].log_domain_size() : 0;
  const std::vector<uint128>& tree_indices = c->tree_indices;
  UntilBatchArgs a;
  a.P = P;
  a.T = static_cast<int64_t>(tree_indices.size());
  a.K = ctx.keys().num_keys();
  a.Dh = hierarchy_to_tree()[hierarchy_level];
  const std::vector<uint128>& q = ctx.partial_prefixes_;
  if (P > 0) {
    a.Dprev = hierarchy_to_tree()[prev];
    if (ctx.partial_evaluations_level_ >= 0 && !q.empty() &&
        hierarchy_to_tree()[ctx.partial_evaluations_level_] <= a.Dprev) {
      a.start_level = hierarchy_to_tree()[ctx.partial_evaluations_level_];
      c->source = StartSource::kPartial;
    }
  }
  c->start_level = a.start_level;
  const auto& f = flat_[hierarchy_level];
  c->desc = MakeDesc(f, blocks_needed_[hierarchy_level]);
  a.max_e = dpf_hip_prefix_batch_max_expand(&c->desc, sum ? 1 : 0);
  c->native_sum = sum && a.max_e >= 0;
  if (a.max_e < 0) a.max_e = dpf_hip_prefix_batch_max_expand(&c->desc, 0);
  a.log_bits = parameters()[hierarchy_level].log_domain_size() - prev_log;
  a.cepb = corrected_elements_per_block(hierarchy_level);
  a.esz = f.packed_size;
  a.sum = sum;
  a.last_level = hierarchy_level == static_cast<int>(parameters().size()) - 1;
  a.cache_on = c->cache_on = CacheOn();
  a.cache_level = ctx.leaf_seeds_ ? ctx.leaf_level_ : -1;
  a.prev_level = prev;
  a.cache_de = ctx.leaf_de_;
  a.cache_stride = ctx.leaf_stride_;
  const UntilBatchShape& sh = c->shape = dpf_internal::PlanUntilBatch(a, c->prefix_map);

  // A cached call's start slots come out of the lookup's own pass (one read
  // of tree_indices instead of two).
  const bool cached = sh.cached;
  const dpf_internal::StartSlotOf slot_of(cached ? sh.W1 : 0, ctx.leaf_phys_);
  if (cached) c->start_slot.resize(sh.T);
  int64_t* start_slot = c->start_slot.data();
  if (c->source == StartSource::kPartial) {
    c->parent_of.resize(sh.T);
    int32_t* parent_of = c->parent_of.data();
    const int64_t missing = dpf_internal::LookupStoredPrefixes(
        q, ctx.partial_sorted_, tree_indices.data(), sh.T, sh.W1, [&](int64_t i, int64_t j) {
          parent_of[i] = static_cast<int32_t>(j);
          if (cached) start_slot[i] = slot_of(j, tree_indices[i]);
        });
    if (missing < sh.T)
      return InvalidArgumentError("Prefix not present in ctx.partial_evaluations at hierarchy level " +
                                  std::to_string(prev));
  } else if (cached) {
    dpf_internal::ParallelFor(sh.T, [&](int64_t lo, int64_t hi) {
      for (int64_t i = lo; i < hi; ++i) start_slot[i] = slot_of(0, tree_indices[i]);
    });
  }
  if (a.max_e < 0) return UnimplementedError("value type not supported by the batched GPU path");
  if (sh.U < 0)
    return ResourceExhaustedError(
        "Too many start nodes for one batched evaluation; evaluate fewer levels at once.");
  if (cached) c->source = StartSource::kCache;
  return OkStatus();
}

// The kernel launch and what follows it, by output mode.  The kernel writes
// `rows` rows of n_blk elements: the caller's buffer when nothing follows,
// else stage_.
//   native key sum: kernel sums (sum flag 1, workspace_), 1 row;
//   per-key rows + row sum: K rows into stage_, dpf_hip_sum_rows into the
//     caller's buffer (stage2_ when a gather follows);
//   store: K rows.
// A non-identity gather (dpf_hip_gather for one row, dpf_hip_gather_batched
// for K) then writes the caller's buffer.
//   sketch, fused (BatchCall::fused_sketch): the native key sum's launch
//     with num_weights > 0, which also writes the sketch buffer; the sums go to stage_ when the caller wants none;
//   sketch, streamed: K rows into stage_, gathered per key into stage2_ unless
//     the gather is the identity, then dpf_hip_sketch_rows over those rows into
//     the sketch buffer and, with `sum`, dpf_hip_sum_rows into the caller's.
Status DistributedPointFunction::LaunchBatchCall(int hierarchy_level, BatchCall& c,
                                                 DeviceBatchContext& ctx, bool sum,
                                                 void* device_out, void* stream,
                                                 const BatchSketch* sketch) const {
  DeviceBatchContext::CacheTarget* target = &c.target;
  const dpf_internal::TableLayout& tab = c.tables;
  const DeviceKeyBatch& keys = ctx.keys();
  const UntilBatchShape& sh = c.shape;
  const int64_t K = keys.num_keys();
  const int esz = flat_[hierarchy_level].packed_size;
  const bool row_sum = sum && !c.native_sum;
  const int64_t rows = c.native_sum ? 1 : K;
  const bool gather_out = !sh.identity;
  const char* dtab = static_cast<const char*>(ctx.parent_);
  const int64_t* d_offsets =
      gather_out ? reinterpret_cast<const int64_t*>(dtab + tab.off_offsets) : nullptr;
  auto ensure = [&](void** p, size_t* cap, size_t bytes) {
    return ctx.EnsureEvicting(p, cap, bytes, target, stream);
  };

  const bool streamed = sketch && !c.fused_sketch;
  void* kernel_out = device_out;
  if (row_sum || gather_out || streamed || !device_out) {
    DPF_RETURN_IF_ERROR(ensure(&ctx.stage_, &ctx.stage_cap_, rows * sh.n_blk * esz));
    kernel_out = ctx.stage_;
  }
  if (streamed && gather_out)
    DPF_RETURN_IF_ERROR(ensure(&ctx.stage2_, &ctx.stage2_cap_, K * sh.n * esz));
  if (c.fused_sketch) {
    DPF_RETURN_IF_ERROR(ensure(&ctx.sketch_w_, &ctx.sketch_w_cap_,
                               sh.n_blk * sketch->rows * 2 * sizeof(uint32_t)));
    DPF_RETURN_IF_ERROR(ensure(&ctx.sketch_acc_, &ctx.sketch_acc_cap_,
                               K * sketch->rows * 2 * sizeof(uint64_t)));
    // The caller's weights in the kernel's slot order, through the output
    // gather's offsets.
    HIP_RETURN_IF_ERROR(dpf_hip_sketch_slot_weights(
        gather_out ? sh.P : sh.n, gather_out ? sh.cnt : 1, d_offsets, &c.desc, sketch->rows,
        sketch->weights, ctx.sketch_w_, stream));
  }
  if (c.native_sum)
    DPF_RETURN_IF_ERROR(
        ensure(&ctx.workspace_, &ctx.workspace_cap_,
               sh.n_blk * flat_[hierarchy_level].leaves.size() * 3 * sizeof(uint64_t)));

  // Start seeds by source; cached ones carry their control bit in bit 0
  // (control_in NULL).
  const dpf_block* start_seeds = nullptr;
  const uint8_t* start_ctrl = nullptr;
  int64_t start_stride = static_cast<int64_t>(ctx.partial_prefixes_.size());
  if (c.source == StartSource::kCache) {
    start_seeds = static_cast<const dpf_block*>(ctx.leaf_seeds_);
    start_stride = ctx.leaf_stride_;
  } else if (c.source == StartSource::kGathered) {
    start_seeds = static_cast<const dpf_block*>(ctx.next_seeds_);
    start_ctrl = static_cast<const uint8_t*>(ctx.next_ctrl_);
    start_stride = sh.T;
  } else if (c.source == StartSource::kPartial) {
    start_seeds = ctx.partial_seeds();
    start_ctrl = ctx.partial_control();
  }
  const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight), kv = AesKey(kPrgKeyValue);
  // The one launch; the fused sketch is four more members of its arguments.
  dpf_prefix_batch_args args = {};
  args.struct_size = sizeof(args);
  args.num_keys = K;
  args.num_starts = sh.U;
  args.walk_levels = sh.Wk + sh.s;
  args.save_after = sh.update_ctx && !target->gather ? sh.Wk : -1;
  args.expand_levels = sh.E;
  args.cw_first =
      sh.cached ? hierarchy_to_tree()[ctx.previous_hierarchy_level_] : c.start_level;
  args.cw_stride = keys.num_levels();
  args.key_seed = keys.seed();
  args.party = keys.party();
  args.seeds_in = start_seeds;
  args.control_in = start_ctrl;
  args.in_stride = start_stride;
  args.parent = reinterpret_cast<const int32_t*>(dtab);
  if (tab.need_path) args.path = reinterpret_cast<const dpf_block*>(dtab + tab.off_path);
  if (tab.need_save) args.save_index = reinterpret_cast<const int32_t*>(dtab + tab.off_save);
  args.seeds_out = static_cast<dpf_block*>(ctx.next_seeds_);
  args.control_out = static_cast<uint8_t*>(ctx.next_ctrl_);
  args.out_stride = sh.T;
  args.cw_seed = keys.cw_seed();
  args.cw_left = keys.cw_left();
  args.cw_right = keys.cw_right();
  args.key_left = &kl;
  args.key_right = &kr;
  args.key_value = &kv;
  args.desc = &c.desc;
  args.elements_per_leaf = corrected_elements_per_block(hierarchy_level);
  args.value_correction = keys.value_correction(hierarchy_level);
  if (c.native_sum) {
    args.sum = 1;
    args.workspace = static_cast<uint64_t*>(ctx.workspace_);
  }
  args.out = kernel_out;
  args.leaf_cache = static_cast<dpf_block*>(target->leaf_seeds);
  args.leaf_stride = target->stride;
  if (target->permute) args.leaf_slot = static_cast<const int32_t*>(ctx.leaf_slot_);
  args.index_major = ctx.index_major_ ? 1 : 0;
  if (c.fused_sketch) {
    args.num_weights = sketch->rows;
    args.slot_weights = static_cast<const uint32_t*>(ctx.sketch_w_);
    args.accumulators = static_cast<uint64_t*>(ctx.sketch_acc_);
    args.sketch = sketch->out;
  }
  HIP_RETURN_IF_ERROR(dpf_hip_prefix_batch_level(&args, stream));

  if (streamed) {
    const void* key_rows = kernel_out;
    if (gather_out) {
      HIP_RETURN_IF_ERROR(dpf_hip_gather_batched(K, sh.n_blk, sh.P, sh.cnt, esz, d_offsets,
                                                 kernel_out, ctx.stage2_, stream));
      key_rows = ctx.stage2_;
    }
    HIP_RETURN_IF_ERROR(dpf_hip_sketch_rows(K, sh.n, &c.desc, key_rows, sketch->rows, 32,
                                            sketch->weights, sketch->out, stream));
    if (sum)
      HIP_RETURN_IF_ERROR(dpf_hip_sum_rows(K, sh.n, &c.desc, key_rows, device_out, stream));
    return OkStatus();
  }
  const void* gather_in = kernel_out;
  if (row_sum) {
    // Value types without an on-device key sum in the kernel: a group sum
    // over the per-key rows.
    void* summed = device_out;
    if (gather_out) {
      DPF_RETURN_IF_ERROR(ensure(&ctx.stage2_, &ctx.stage2_cap_, sh.n_blk * esz));
      summed = ctx.stage2_;
    }
    HIP_RETURN_IF_ERROR(dpf_hip_sum_rows(K, sh.n_blk, &c.desc, ctx.stage_, summed, stream));
    gather_in = summed;
  }
  if (gather_out && sum && device_out)
    HIP_RETURN_IF_ERROR(dpf_hip_gather(sh.P, sh.cnt, esz, d_offsets, gather_in, device_out, stream));
  if (gather_out && !sum && !sketch)
    HIP_RETURN_IF_ERROR(dpf_hip_gather_batched(K, sh.n_blk, sh.P, sh.cnt, esz, d_offsets, gather_in,
                                               device_out, stream));
  return OkStatus();
}

StatusOr<int64_t> DistributedPointFunction::EvaluateUntilBatchCore(
    int hierarchy_level, Span<const uint128> prefixes, DeviceBatchContext& ctx, bool sum,
    void* device_out, int64_t capacity_bytes, void* stream, const BatchSketch* sketch) const {
  DPF_RETURN_IF_ERROR(CheckUntilBatchArgs(hierarchy_level, prefixes, ctx));
  PhaseTimer::Clock clk(g_timing);
  g_timing.count_call();
  // Start nodes are indexed by int32 on the device.
  if (prefixes.size() > static_cast<size_t>(INT32_MAX))
    return ResourceExhaustedError(
        "Too many start nodes for one batched evaluation; evaluate fewer levels at once.");
  const int H = static_cast<int>(parameters().size());
  const int prev = ctx.previous_hierarchy_level_;

  // Unique tree indices in first-seen order and each prefix's (tree index,
  // block index) (h:718-742).
  BatchCall c;
  c.tree_indices = std::move(ctx.spare_prefixes_);  // recycled storage
  if (!prefixes.empty()) {
    dpf_internal::DedupTreeIndices(
        prefixes, parameters()[prev].log_domain_size() - hierarchy_to_tree()[prev], &c.tree_indices,
        &c.prefix_map, &c.indices_ascending);
  } else {
    c.tree_indices.assign(1, 0);  // the root, expanded to depth Dh
    c.prefix_map.clear();
  }
  clk.mark(0);
  // A sketch call is planned as per-key rows (every type it accepts takes the
  // same shape in both modes, so the context ends up as the sum call's).
  DPF_RETURN_IF_ERROR(PlanBatchCall(hierarchy_level, static_cast<int64_t>(prefixes.size()), ctx,
                                    sum && !sketch, &c));
  const UntilBatchShape& sh = c.shape;
  if (sketch) {
    const int64_t K = ctx.keys().num_keys();
    const int64_t nl = static_cast<int64_t>(flat_[hierarchy_level].leaves.size());
    if (sum && capacity_bytes < sh.n * flat_[hierarchy_level].packed_size)
      return InvalidArgumentError("device output buffer too small");
    if (sketch->rows < 1 || sketch->rows > DPF_HIP_SKETCH_MAX_WEIGHTS)
      return InvalidArgumentError("num_weight_rows must be in [1, 4]");
    if (sketch->per_row != sh.n)
      return InvalidArgumentError("weights_per_row does not match the number of outputs");
    if (!sketch->weights || !sketch->out ||
        sketch->capacity_bytes < K * sketch->rows * nl * static_cast<int64_t>(sizeof(uint32_t)))
      return InvalidArgumentError("device sketch buffer too small");
    if (!dpf_hip_sketch_supported(&c.desc))
      return UnimplementedError("value type not supported by the batched sketch");
    // Fused into the key-sum kernel when the launch has its shape, the outputs
    // are a permutation of its slots (no duplicate prefixes), and the
    // accumulators' 32-bit offsets and uint64 sums hold; else streamed.
    c.fused_sketch =
        sh.P > 0 && sh.P == sh.T && sh.cnt == sh.block && sh.n < (int64_t{1} << 32) &&
        K * sketch->rows * 16 < (int64_t{1} << 32) &&
        dpf_hip_prefix_batch_sketch_fused(&c.desc, sh.Wk + sh.s, sh.E,
                                          corrected_elements_per_block(hierarchy_level), 1,
                                          ctx.index_major_ ? 1 : 0, sketch->rows) != 0;
    c.native_sum = c.fused_sketch;
  } else if (!device_out || capacity_bytes < sh.out_bytes) {
    return InvalidArgumentError("device output buffer too small");
  }

  // Where this call's leaves go: the next call's expansion cache (not after
  // the last level).
  const int64_t leaf_stride = sh.U << sh.E;
  const bool writes_cache =
      c.cache_on && hierarchy_level < H - 1 && hierarchy_to_tree()[hierarchy_level] > 0;
  DPF_ASSIGN_OR_RETURN(c.target,
                       ctx.ChooseCacheTarget(writes_cache, sh.cached, leaf_stride, c.start_slot,
                                             sh.T, sh.s, sh.E, &c.leaf_slot, stream));
  DeviceBatchContext::CacheTarget& target = c.target;
  if (target.gather) c.source = StartSource::kGathered;
  clk.mark(1);

  // The start-node tables and gather offsets: built in one page-locked image,
  // sent with one copy.  The per-call buffers come before anything else that
  // allocates: when device memory runs out, the expansion cache gives way.
  const dpf_internal::TableLayout& tab = c.tables = dpf_internal::PlanTables(sh);
  DPF_RETURN_IF_ERROR(ctx.StageTables(tab.bytes));
  dpf_internal::FillTables(sh, tab, c.source, c.tree_indices.data(), c.parent_of.data(),
                           c.start_slot.data(), c.prefix_map, static_cast<char*>(ctx.pinned_tables_));
  clk.mark(2);
  DPF_RETURN_IF_ERROR(ctx.SendTables(tab.bytes, &target, stream));
  if (sh.update_ctx || target.gather) {
    const int64_t K = ctx.keys().num_keys();
    DPF_RETURN_IF_ERROR(ctx.EnsureEvicting(&ctx.next_seeds_, &ctx.next_seeds_cap_,
                                           K * sh.T * sizeof(dpf_block), &target, stream));
    DPF_RETURN_IF_ERROR(
        ctx.EnsureEvicting(&ctx.next_ctrl_, &ctx.next_ctrl_cap_, K * sh.T, &target, stream));
  }
  // The start seeds (and, with update_ctx, the new partial evaluations) are
  // read before the kernel rewrites the cache.
  if (target.gather)
    DPF_RETURN_IF_ERROR(ctx.GatherStartSeeds(c.start_slot, sh.T, leaf_stride, &target, stream));
  if (target.permute) DPF_RETURN_IF_ERROR(ctx.SendSlotTable(c.leaf_slot, &target, stream));
  clk.mark(3);

  DPF_RETURN_IF_ERROR(
      LaunchBatchCall(hierarchy_level, c, ctx, sum, device_out, stream, sketch));

  ctx.CommitCache(target, hierarchy_level, sh.dE, hierarchy_level == H - 1, c.leaf_slot);
  if (g_timing.on()) dpf_hip_stream_sync(stream);  // attribute device time to its phase
  clk.mark(4);
  ctx.CommitPartials(hierarchy_level, prev, sh.P > 0, sh.update_ctx, c.indices_ascending,
                     &c.tree_indices);
  clk.mark(5);
  return sh.n;
}

StatusOr<EvaluationContext> DistributedPointFunction::ExportEvaluationContext(
    const DeviceBatchContext& ctx, const KeyBatch& host_keys, int64_t k, void* stream) const {
  const DeviceKeyBatch& keys = ctx.keys();
  if (k < 0 || k >= keys.num_keys()) return InvalidArgumentError("key index out of range");
  DPF_ASSIGN_OR_RETURN(DpfKey key, KeyFromBatch(host_keys, keys.first_key() + k));
  DPF_ASSIGN_OR_RETURN(EvaluationContext out, CreateEvaluationContext(std::move(key)));
  out.set_previous_hierarchy_level(ctx.previous_hierarchy_level());
  if (ctx.partial_evaluations_level() >= 0)
    out.set_partial_evaluations_level(ctx.partial_evaluations_level());
  const auto& q = ctx.partial_prefixes();
  if (!q.empty()) {
    const int64_t Q = static_cast<int64_t>(q.size());
    std::vector<dpf_block> seeds(Q);
    std::vector<uint8_t> ctrl(Q);
    if (ctx.index_major()) {
      // Key k's column of the [prefix][key] tables.
      const int64_t K = keys.num_keys();
      HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h_strided(seeds.data(), ctx.partial_seeds() + k,
                                                     sizeof(dpf_block), K * sizeof(dpf_block), Q,
                                                     stream));
      HIP_RETURN_IF_ERROR(
          dpf_hip_memcpy_d2h_strided(ctrl.data(), ctx.partial_control() + k, 1, K, Q, stream));
    } else {
      HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(seeds.data(), ctx.partial_seeds() + k * Q,
                                             Q * sizeof(dpf_block), stream));
      HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(ctrl.data(), ctx.partial_control() + k * Q, Q, stream));
    }
    for (int64_t i = 0; i < Q; ++i) {
      PartialEvaluation* e = out.add_partial_evaluations();
      SetProtoBlock(q[i], e->mutable_prefix());
      SetProtoBlock(FromBlock(seeds[i]), e->mutable_seed());
      e->set_control_bit(ctrl[i] != 0);
    }
  }
  return out;
}

}  // namespace distributed_point_functions
