// distributed_point_function.h -- the DistributedPointFunction API of the
// reference (dpf/distributed_point_function.h:77-585), kept as a drop-in, with
// evaluation executed by hand-written gfx950 kernels through the C ABI of
// include/dpf_hip.h.  Key generation stays on the CPU.
//
// Public surface (same names, argument meaning and error behaviour as the
// reference): Create, CreateIncremental, ToValue, RegisterValueType,
// GenerateKeys (3 overloads), GenerateKeysIncremental (3 overloads),
// CreateEvaluationContext, EvaluateUntil<T>, EvaluateNext<T>, both
// EvaluateAt<T> overloads, parameters(); free functions ToValue, FromValue,
// ToValueType.
//
// MI355X extensions (not in the reference):
//   * *Packed variants: the type-erased core used by the templates and the
//     Python binding; output = packed elements (leaves concatenated, little-endian).
//   * EvaluateUntilToDevice: leaves the output in device memory (HBM), which is
//     how full-domain evaluations at 2^30+ elements are meant to be consumed.
//   * EvaluateAtBatchPacked: one launch for many keys x points.
//   * GenerateKeysIncrementalWithSeeds: injected root seeds for reproducible
//     fixtures (the reference draws them with RAND_bytes, cc:656-662).
//
// Thread-compatible, not thread-safe (like the reference, whose
// Aes128FixedKeyHash shares one EVP context).
#ifndef DPF_DISTRIBUTED_POINT_FUNCTION_H_
#define DPF_DISTRIBUTED_POINT_FUNCTION_H_

#include <functional>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <string_view>
#include <type_traits>
#include <utility>
#include <vector>

#include "dpf/aes_128_fixed_key_hash.h"
#include "dpf/distributed_point_function.pb.h"
#include "dpf/internal/proto_validator.h"
#include "dpf/internal/value_type_helpers.h"
#include "dpf/key_batch.h"
#include "dpf/span.h"
#include "dpf/status.h"
#include "dpf/uint128.h"

namespace distributed_point_functions {

template <typename T>
using is_supported_type = dpf_internal::is_supported_type<T>;
template <typename T>
constexpr bool is_supported_type_v = is_supported_type<T>::value;

// h:49-67
template <typename T, typename = std::enable_if_t<is_supported_type_v<T>>>
StatusOr<T> FromValue(const Value& value) {
  return dpf_internal::FromValueImpl<T>(value);
}
template <typename T, typename = std::enable_if_t<is_supported_type_v<T>>>
Value ToValue(const T& input) {
  return dpf_internal::ValueTypeHelper<T>::ToValue(input);
}
template <typename T, typename = std::enable_if_t<is_supported_type_v<T>>>
ValueType ToValueType() {
  return dpf_internal::ValueTypeHelper<T>::ToValueType();
}

namespace dpf_internal {
class DeviceScratch;
}

class DistributedPointFunction {
 public:
  static StatusOr<std::unique_ptr<DistributedPointFunction>> Create(const DpfParameters& parameters);
  static StatusOr<std::unique_ptr<DistributedPointFunction>> CreateIncremental(
      Span<const DpfParameters> parameters);

  DistributedPointFunction(const DistributedPointFunction&) = delete;
  DistributedPointFunction& operator=(const DistributedPointFunction&) = delete;
  ~DistributedPointFunction();

  template <typename T>
  StatusOr<Value> ToValue(const T& in) {
    Status status = RegisterValueType<T>();
    if (!status.ok()) return status;
    return distributed_point_functions::ToValue(in);
  }

  template <typename T>
  Status RegisterValueType() {
    return RegisterValueType(ToValueType<T>());
  }
  // Runtime form of RegisterValueType<T>() (registers the serialized type).
  Status RegisterValueType(const ValueType& value_type);

  StatusOr<std::pair<DpfKey, DpfKey>> GenerateKeys(uint128 alpha, uint128 beta) {
    return GenerateKeysIncremental(alpha, Span<const uint128>(&beta, 1));
  }
  StatusOr<std::pair<DpfKey, DpfKey>> GenerateKeys(uint128 alpha, Value beta) {
    return GenerateKeysIncremental(alpha, Span<const Value>(&beta, 1));
  }
  template <typename T, typename = std::enable_if_t<!std::is_convertible_v<T, uint128> &&
                                                    !std::is_convertible_v<T, Value> &&
                                                    is_supported_type_v<T>>>
  StatusOr<std::pair<DpfKey, DpfKey>> GenerateKeys(uint128 alpha, const T& beta) {
    StatusOr<Value> value = ToValue<T>(beta);
    if (!value.ok()) return value.status();
    return GenerateKeysIncremental(alpha, Span<const Value>(&*value, 1));
  }

  StatusOr<std::pair<DpfKey, DpfKey>> GenerateKeysIncremental(uint128 alpha,
                                                              Span<const uint128> beta) {
    std::vector<Value> values(beta.size());
    for (size_t i = 0; i < beta.size(); ++i) {
      StatusOr<Value> v = ToValue(beta[i]);
      if (!v.ok()) return v.status();
      values[i] = std::move(*v);
    }
    return GenerateKeysIncremental(alpha, Span<const Value>(values));
  }
  StatusOr<std::pair<DpfKey, DpfKey>> GenerateKeysIncremental(uint128 alpha,
                                                              Span<const Value> beta);
  template <typename T0, typename... Tn,
            typename = std::enable_if_t<
                !std::is_convertible_v<T0, Span<const Value>> &&
                !std::is_convertible_v<T0, Span<const uint128>> &&
                is_supported_type_v<std::decay_t<T0>> &&
                (is_supported_type_v<std::decay_t<Tn>> && ...)>>
  StatusOr<std::pair<DpfKey, DpfKey>> GenerateKeysIncremental(uint128 alpha, T0&& beta_0,
                                                              Tn&&... beta_n) {
    std::vector<Value> values;
    Status status = OkStatus();
    auto add = [&](const auto& b) {
      if (!status.ok()) return;
      StatusOr<Value> v = ToValue(b);
      if (v.ok()) values.push_back(std::move(*v)); else status = v.status();
    };
    add(beta_0);
    (add(beta_n), ...);
    if (!status.ok()) return status;
    return GenerateKeysIncremental(alpha, Span<const Value>(values));
  }

  // Extension: root seeds supplied by the caller (reproducible fixtures).
  StatusOr<std::pair<DpfKey, DpfKey>> GenerateKeysIncrementalWithSeeds(
      uint128 alpha, Span<const Value> beta, uint128 seed_0, uint128 seed_1);

  StatusOr<EvaluationContext> CreateEvaluationContext(DpfKey key) const;

  template <typename T>
  StatusOr<std::vector<T>> EvaluateUntil(int hierarchy_level, Span<const uint128> prefixes,
                                         EvaluationContext& ctx) const {
    ValueType t = ToValueType<T>();
    if constexpr (dpf_internal::kPackedIsMemoryImage<T>) {
      // The packed elements are T's memory image: copy them from the device
      // straight into the result.
      std::vector<T> out;
      const HostSink sink = dpf_internal::VectorSink(&out);
      Status status = EvaluateUntilToHost(hierarchy_level, prefixes, ctx, &t, sink);
      if (!status.ok()) return status;
      return out;
    } else {
      // Packed tuples / IntModN / XorWrapper values are unpacked straight out
      // of the page-locked staging buffers into the result, chunk by chunk
      // (the sink reads flat_[hierarchy_level] only after validation).
      std::vector<T> out;
      const HostSink sink = dpf_internal::UnpackSink(&flat_, hierarchy_level, &out);
      Status status = EvaluateUntilToHost(hierarchy_level, prefixes, ctx, &t, sink);
      if (!status.ok()) return status;
      return out;
    }
  }

  template <typename T>
  StatusOr<std::vector<T>> EvaluateNext(Span<const uint128> prefixes,
                                        EvaluationContext& ctx) const {
    if (prefixes.empty()) return EvaluateUntil<T>(0, prefixes, ctx);
    return EvaluateUntil<T>(ctx.previous_hierarchy_level() + 1, prefixes, ctx);
  }

  template <typename T>
  StatusOr<std::vector<T>> EvaluateAt(const DpfKey& key, int hierarchy_level,
                                      Span<const uint128> evaluation_points) const {
    return EvaluateAtImpl<T>(key, hierarchy_level, evaluation_points, nullptr);
  }

  template <typename T>
  StatusOr<std::vector<T>> EvaluateAt(int hierarchy_level, Span<const uint128> evaluation_points,
                                      EvaluationContext& ctx) const {
    return EvaluateAtImpl<T>(ctx.key(), hierarchy_level, evaluation_points, &ctx);
  }

  Span<const DpfParameters> parameters() const { return validator_->parameters(); }

  // ---- type-erased core (packed elements) --------------------------------
  // `requested_type` (may be null) plays the role of T in the templates.
  // Where the packed output is copied (dpf_internal::HostSink: storage for it,
  // and how a fresh vector becomes valid chunk by chunk during the copy).
  using HostSink = dpf_internal::HostSink;
  Status EvaluateUntilToHost(int hierarchy_level, Span<const uint128> prefixes,
                             EvaluationContext& ctx, const ValueType* requested_type,
                             const HostSink& sink) const;
  StatusOr<std::vector<uint8_t>> EvaluateUntilPacked(int hierarchy_level,
                                                     Span<const uint128> prefixes,
                                                     EvaluationContext& ctx,
                                                     const ValueType* requested_type = nullptr) const;
  // Writes the packed output to device memory `device_out` (capacity in bytes)
  // on `stream`; returns the number of elements written.
  StatusOr<int64_t> EvaluateUntilToDevice(int hierarchy_level, Span<const uint128> prefixes,
                                          EvaluationContext& ctx, void* device_out,
                                          int64_t capacity_bytes, void* stream,
                                          const ValueType* requested_type = nullptr) const;
  // Multi-GPU sharding: the first (full-domain) evaluation of
  // `hierarchy_level` restricted to shard `shard` of `num_shards` (a power of
  // two): the outputs [shard * n / num_shards, (shard + 1) * n / num_shards) of
  // EvaluateUntil(hierarchy_level, {}, ctx), i.e. the subtree under the top
  // log2(num_shards) tree bits.  Writes packed elements to device memory and
  // advances ctx like EvaluateUntil; returns the number of elements written.
  StatusOr<int64_t> EvaluateShardToDevice(int hierarchy_level, int64_t shard, int64_t num_shards,
                                          EvaluationContext& ctx, void* device_out,
                                          int64_t capacity_bytes, void* stream) const;
  // Two-server PIR: full-domain evaluation folded into a database, without
  // the share vector ever being stored.  With y = EvaluateUntil<T>(
  // hierarchy_level, {}, fresh ctx) and `device_db` a row-major device array
  // of y.size() records of `record_words` words of T's width,
  //   uint64_t:                       out[w] = sum_i y[i] * db[i][w]  (mod 2^64)
  //   XorWrapper<uint64_t / uint128>: out[w] = XOR_i (y[i] & db[i][w]);
  // the two parties' results combine with T's + to beta * db[alpha]
  // (beta & db[alpha]).  Other value types: UNIMPLEMENTED.  Stateless and
  // key-based like EvaluateAt(key, ...).  With num_shards > 1 (a power of
  // two), `device_db` holds only shard `shard`'s y.size() / num_shards
  // records and the result is that shard's partial; the shards' partials
  // combine with T's +.  Writes record_words packed elements to `device_out`
  // on `stream` (asynchronous) and returns record_words.
  StatusOr<int64_t> EvaluateDotToDevice(const DpfKey& key, int hierarchy_level, int64_t shard,
                                        int64_t num_shards, const void* device_db,
                                        int64_t db_bytes, int64_t record_words, void* device_out,
                                        int64_t out_bytes, void* stream) const;
  // The unsharded fold returned to the host (packed elements).
  StatusOr<std::vector<uint8_t>> EvaluateDotPacked(const DpfKey& key, int hierarchy_level,
                                                   const void* device_db, int64_t db_bytes,
                                                   int64_t record_words,
                                                   const ValueType* requested_type = nullptr) const;
  template <typename T>
  StatusOr<std::vector<T>> EvaluateDot(const DpfKey& key, int hierarchy_level,
                                       const void* device_db, int64_t db_bytes,
                                       int64_t record_words) const {
    ValueType t = ToValueType<T>();
    auto packed = EvaluateDotPacked(key, hierarchy_level, device_db, db_bytes, record_words, &t);
    if (!packed.ok()) return packed.status();
    return Unpack<T>(hierarchy_level, *packed);
  }
  // Dense two-server PIR, batched over queries: one output *bit* selects one
  // record.  For T = XorWrapper<uint64_t> or XorWrapper<absl::uint128> (other
  // value types: UNIMPLEMENTED) let y_q be the packed output of
  // EvaluateUntil<T>(hierarchy_level, {}, fresh ctx of keys[q]) read as a
  // byte string, bit j = (byte[j >> 3] >> (j & 7)) & 1 for j in [0, n), n =
  // 2^log_domain_size * bits of T (128 records per leaf block), and
  // `device_db` a row-major device array of n records of `record_words`
  // uint64 words, whatever T is.  Then
  //   out[q][w] = XOR over { j : bit_j(y_q) = 1 } of db[j][w];
  // the two parties' answers for query q XOR to the XOR of db[alpha*bits + b]
  // over the set bits b of beta.  The database is read once per tile of
  // queries, not once per key; keys.size() is in [1, 64].  With num_shards > 1
  // (a power of two, at most one shard per tree leaf), `device_db` holds only
  // the records [shard * n / num_shards, (shard + 1) * n / num_shards) and
  // the shards' answers XOR to the unsharded one.  Stateless and key-based
  // like EvaluateDotToDevice.  Writes keys.size() * record_words uint64 to
  // `device_out` on `stream` (asynchronous) and returns that count.
  StatusOr<int64_t> EvaluateSelectToDevice(Span<const DpfKey* const> keys, int hierarchy_level,
                                           int64_t shard, int64_t num_shards,
                                           const void* device_db, int64_t db_bytes,
                                           int64_t record_words, void* device_out,
                                           int64_t out_bytes, void* stream) const;
  // The unsharded answers returned to the host, [keys.size()][record_words].
  StatusOr<std::vector<uint64_t>> EvaluateSelect(Span<const DpfKey* const> keys,
                                                 int hierarchy_level, const void* device_db,
                                                 int64_t db_bytes, int64_t record_words) const;
  // Additive-share two-server PIR, batched over queries: EvaluateDotToDevice
  // for up to 64 keys against one pass over the database.  For T = uint64_t
  // or XorWrapper<uint64_t> (other value types: UNIMPLEMENTED) let y_q =
  // EvaluateUntil<T>(hierarchy_level, {}, fresh ctx of keys[q]) (n elements)
  // and `device_db` a row-major device array of n records of `record_words`
  // uint64 words.  Then
  //   uint64_t:             out[q][w] = sum_i y_q[i] * db[i][w]  (mod 2^64)
  //   XorWrapper<uint64_t>: out[q][w] = XOR_i (y_q[i] & db[i][w]);
  // row q is what EvaluateDotToDevice(keys[q], ...) writes, bit for bit, and
  // the two parties' rows combine with T's + to beta_q * db[alpha_q] (beta_q &
  // db[alpha_q]).  The database is read once per tile of queries, not once per
  // key; keys.size() is in [1, 64].  With num_shards > 1 (a power of two),
  // `device_db` holds only shard `shard`'s n / num_shards records and the
  // shards' answers combine with T's +.  Stateless and key-based like
  // EvaluateDotToDevice.  Writes keys.size() * record_words uint64 to
  // `device_out` on `stream` (asynchronous) and returns that count.
  StatusOr<int64_t> EvaluateDotBatchToDevice(Span<const DpfKey* const> keys, int hierarchy_level,
                                             int64_t shard, int64_t num_shards,
                                             const void* device_db, int64_t db_bytes,
                                             int64_t record_words, void* device_out,
                                             int64_t out_bytes, void* stream) const;
  // The unsharded answers returned to the host, [keys.size()][record_words].
  StatusOr<std::vector<uint64_t>> EvaluateDotBatch(Span<const DpfKey* const> keys,
                                                   int hierarchy_level, const void* device_db,
                                                   int64_t db_bytes, int64_t record_words) const;
  StatusOr<std::vector<uint8_t>> EvaluateAtPacked(const DpfKey& key, int hierarchy_level,
                                                  Span<const uint128> evaluation_points,
                                                  EvaluationContext* ctx,
                                                  const ValueType* requested_type = nullptr) const;
  // EvaluateAt's packed output copied into `sink` (EvaluateAt<T>: straight
  // into the returned std::vector<T>).
  Status EvaluateAtToHost(const DpfKey& key, int hierarchy_level,
                          Span<const uint128> evaluation_points, EvaluationContext* ctx,
                          const ValueType* requested_type, const HostSink& sink) const;
  // keys[k] is evaluated at points[k*points_per_key .. (k+1)*points_per_key).
  StatusOr<std::vector<uint8_t>> EvaluateAtBatchPacked(Span<const DpfKey* const> keys,
                                                       int hierarchy_level,
                                                       Span<const uint128> points,
                                                       int64_t points_per_key) const;

  // ---- key batches ------------------
  // SoA image of `keys` (each validated like CreateEvaluationContext does).
  StatusOr<KeyBatch> MakeKeyBatch(Span<const DpfKey* const> keys) const;
  // SoA image of serialized DpfKeys (the proto wire format), parsed and
  // validated on `num_threads` host threads (0 = hardware concurrency, at most
  // 16) -- the batched key ingestion of SURVEY.md 8f.2.  Errors name the first
  // failing key.
  StatusOr<KeyBatch> ParseKeyBatch(Span<const std::string_view> serialized_keys,
                                   int num_threads = 0) const;
  // Row k of `batch` as a DpfKey proto (inverse of MakeKeyBatch).
  StatusOr<DpfKey> KeyFromBatch(const KeyBatch& batch, int64_t k) const;
  // Every row as a serialized DpfKey (inverse of ParseKeyBatch), on
  // `num_threads` host threads (0 = hardware concurrency, at most 16).
  StatusOr<std::vector<std::string>> SerializeKeyBatch(const KeyBatch& batch,
                                                       int num_threads = 0) const;
  // Key generation for many alphas at once, straight into SoA form, on
  // `num_threads` host threads (0 = hardware concurrency).  Key k of the pair
  // is what GenerateKeysIncrementalWithSeeds(alphas[k], beta, root_seeds[2k],
  // root_seeds[2k+1]) returns; with empty root_seeds they are drawn like
  // GenerateKeysIncremental draws them.  `beta` is shared by all keys.
  StatusOr<std::pair<KeyBatch, KeyBatch>> GenerateKeyBatch(Span<const uint128> alphas,
                                                           Span<const Value> beta,
                                                           Span<const uint128> root_seeds,
                                                           int num_threads = 0) const;
  // GenerateKeyBatch with a beta of its own for every key: key k takes
  // betas[k*H .. (k+1)*H), H = parameters().size().
  StatusOr<std::pair<KeyBatch, KeyBatch>> GenerateKeyBatchWithBetas(
      Span<const uint128> alphas, Span<const Value> betas, Span<const uint128> root_seeds,
      int num_threads = 0) const;
  // The same two batches generated in device memory on `stream` (a
  // hipStream_t, may be null): bit-identical to GenerateKeyBatch /
  // GenerateKeyBatchWithBetas from the same root seeds followed by Upload.
  // `beta` holds H values shared by all keys, or alphas.size() * H of them,
  // key-major.  The argument checks are GenerateKeyBatch's and run before the
  // device is touched.  The walk runs on the GPU where GeneratesKeysOnDevice();
  // other value types are generated on the host and uploaded.  The batches
  // are written in stream order, so evaluation queued on `stream` afterwards
  // needs no synchronisation; DeviceKeyBatch::Download brings a batch back.
  using DeviceKeyBatchPair =
      std::pair<std::unique_ptr<DeviceKeyBatch>, std::unique_ptr<DeviceKeyBatch>>;
  StatusOr<DeviceKeyBatchPair> GenerateKeyBatchToDevice(Span<const uint128> alphas,
                                                        Span<const Value> beta,
                                                        Span<const uint128> root_seeds,
                                                        void* stream) const;
  // True when every hierarchy level's value type is one the device generates
  // (a single integer or XorWrapper leaf): GenerateKeyBatchToDevice then runs
  // the key generation kernel, else it falls back to the host.
  bool GeneratesKeysOnDevice() const;
  // ---- the batched generators' pieces, shared with
  // DistributedComparisonFunction (whose DPF alphas and betas derive from its own).
  // GenerateKeyBatch's argument checks, in its order and with its messages, and
  // the betas as flattened leaves.  `beta` holds rows * H values
  // (value_per_row false: row r's level h at beta[r*H + h], leaves at
  // (*leaves)[r*S + offset of level h], S = the levels' leaf counts summed) or,
  // with value_per_row, one value per row that every level takes (rows * the
  // leaf count of level 0).  rows is 1 (shared) or alphas.size().
  Status CheckKeyBatchArgs(Span<const uint128> alphas, Span<const Value> beta, int64_t rows,
                           bool value_per_row, Span<const uint128> root_seeds,
                           std::vector<uint128>* leaves) const;
  // Host generation from checked arguments: `leaves` as CheckKeyBatchArgs
  // lays out rows * H values.
  StatusOr<std::pair<KeyBatch, KeyBatch>> GenerateKeyBatchFromLeaves(
      Span<const uint128> alphas, Span<const uint128> leaves, int64_t rows,
      Span<const uint128> root_seeds, int num_threads) const;
  // Device generation from checked arguments (GeneratesKeysOnDevice() only).
  // beta_mode as dpf_hip_gen_key_batch: 0 leaves[h], 1 leaves[k*H + h], 2 the
  // DCF of dcf_bits bits with `alphas` the DCF's and leaves[k].
  StatusOr<DeviceKeyBatchPair> GenerateKeyBatchFromLeavesToDevice(
      Span<const uint128> alphas, Span<const uint128> leaves, int beta_mode, int dcf_bits,
      Span<const uint128> root_seeds, void* stream) const;
  // EvaluateAt(key_k, hierarchy_level, points_k) for every key of a device
  // batch.  `device_points` are raw domain points (uint128 memory images) in
  // device memory: points_per_key per key ([key][point]), or one shared set of
  // points_per_key points when `shared_points`.  Writes num_keys *
  // points_per_key packed elements ([key][point]) to device_out.
  StatusOr<int64_t> EvaluateAtBatchToDevice(const DeviceKeyBatch& keys, int hierarchy_level,
                                            const void* device_points, int64_t points_per_key,
                                            bool shared_points, void* device_out,
                                            int64_t capacity_bytes, void* stream) const;
  // Aggregation variant: out[j] = sum over the batch's keys of
  // EvaluateAt(key_k, hierarchy_level, point_j), in the value type's group,
  // for one shared set of num_points device points (num_points packed elements).
  Status EvaluateAtBatchSumToDevice(const DeviceKeyBatch& keys, int hierarchy_level,
                                    const void* device_points, int64_t num_points,
                                    void* device_out, void* stream) const;
  // Private table lookup, batched over keys: the full-domain expansion of
  // every key of a device batch folded into one shared public table at a
  // public rotation per key, without a share vector being stored.  For T =
  // uint64_t or XorWrapper<uint64_t> at `hierarchy_level` (other value types:
  // UNIMPLEMENTED; there is no fallback behind this call), n =
  // log_domain_size in [1, 40], N = 2^n, y_k = EvaluateUntil<T>(
  // hierarchy_level, {}, fresh ctx of key k), `device_table` a row-major
  // device array of N rows of `table_words` (W: 1, 2 or 4; others in
  // [1, 1024] UNIMPLEMENTED) uint64 and s_k = device_offsets[k] mod N:
  //   uint64_t:             out[k][w] = sum_i y_k[i] * T[(i + s_k) mod N][w]  (mod 2^64)
  //   XorWrapper<uint64_t>: out[k][w] = XOR_i (y_k[i] & T[(i + s_k) mod N][w]);
  // the two parties' results for key k combine with T's + to
  // beta_k * T[(alpha_k + s_k) mod N][w] (beta_k & ...).  Stateless and
  // key-based.  Writes K * W uint64 to `device_out` on `stream`
  // (asynchronous), whatever it held before, and returns K * W.  Checked in
  // this order, before the device is touched, the first failure reported:
  // the level, the value type and its domain size, table_words, table_bytes
  // == N * W * 8, null pointers, out_bytes >= K * W * 8, that the batch is
  // this DPF's, and the buffers' alignment (the table to min(16, 8 W) bytes,
  // offsets and output to 8).
  StatusOr<int64_t> EvaluateLookupBatchToDevice(const DeviceKeyBatch& keys, int hierarchy_level,
                                                const uint64_t* device_offsets,
                                                const void* device_table, int64_t table_bytes,
                                                int64_t table_words, void* device_out,
                                                int64_t out_bytes, void* stream) const;
  // The same with host offsets (keys.num_keys() of them) and the K * W sums
  // returned to the host.
  StatusOr<std::vector<uint64_t>> EvaluateLookupBatch(const DeviceKeyBatch& keys,
                                                      int hierarchy_level,
                                                      Span<const uint64_t> offsets,
                                                      const void* device_table,
                                                      int64_t table_bytes,
                                                      int64_t table_words) const;
  // True when `hierarchy_level` exists and its value type and domain size are
  // ones EvaluateLookupBatchToDevice takes.
  bool EvaluatesLookupOnDevice(int hierarchy_level) const;
  // EvaluateLookupBatchToDevice's argument checks, in its order and with its
  // messages, for a batch of num_keys keys that is (`batch_matches`) or is not
  // one of this DistributedPointFunction.  Touches no device.
  Status CheckLookupArgs(int64_t num_keys, bool batch_matches, int hierarchy_level,
                         const void* device_offsets, const void* device_table,
                         int64_t table_bytes, int64_t table_words, const void* device_out,
                         int64_t out_bytes) const;
  // Multi-query PIR over a bucketed database (a batch code): every key of a
  // device batch expanded over its small domain and folded into its own
  // bucket's slice of the database.  For T = uint64_t or XorWrapper<uint64_t>
  // at `hierarchy_level` (other value types: UNIMPLEMENTED; there is no
  // fallback behind this call), n = log_domain_size in [1, 24], N = 2^n,
  // y_k = EvaluateUntil<T>(hierarchy_level, {}, fresh ctx of key k),
  // `bucket_begin` a host array of B + 1 entries (bucket_begin[0] = 0,
  // nondecreasing, bucket_begin[B] = K; keys bucket_begin[b] ..
  // bucket_begin[b + 1] - 1 belong to bucket b: none, one or many) and
  // `device_db` a row-major device array [B][N][W] of uint64, W =
  // record_words in [1, 1024], with b(k) the bucket of key k:
  //   uint64_t:             out[k][w] = sum_i y_k[i] * db[b(k)][i][w]  (mod 2^64)
  //   XorWrapper<uint64_t>: out[k][w] = XOR_i (y_k[i] & db[b(k)][i][w]);
  // row k is what EvaluateDotToDevice gives for key k on slice b(k), and the
  // two parties' rows combine with T's + to beta_k * db[b(k)][alpha_k]
  // (beta_k & ...).  Stateless and key-based.  Writes K * W uint64 to
  // `device_out` on `stream` (asynchronous), whatever it held before, and
  // returns K * W; K == 0 launches nothing.  The share rows and the fold's
  // workspace live in this object's device scratch (ReleaseScratch() frees
  // them); the keys are taken in chunks of consecutive keys whose rows fit
  // 256 MiB (DPF_DOT_BUCKETS_CHUNK_KEYS=<c>, read per call, sets the chunk:
  // test hook).  Checked in this order, before the device is touched, the
  // first failure reported: the level, the value type and its domain size,
  // record_words, bucket_begin, db_bytes == B * N * W * 8, null pointers,
  // out_bytes >= K * W * 8, that the batch is this DPF's, and the buffers'
  // alignment (8 bytes).
  StatusOr<int64_t> EvaluateDotBucketsToDevice(const DeviceKeyBatch& keys, int hierarchy_level,
                                               Span<const int64_t> bucket_begin,
                                               const void* device_db, int64_t db_bytes,
                                               int64_t record_words, void* device_out,
                                               int64_t out_bytes, void* stream) const;
  // The same with the K * W sums returned to the host.
  StatusOr<std::vector<uint64_t>> EvaluateDotBuckets(const DeviceKeyBatch& keys,
                                                     int hierarchy_level,
                                                     Span<const int64_t> bucket_begin,
                                                     const void* device_db, int64_t db_bytes,
                                                     int64_t record_words) const;
  // True when `hierarchy_level` exists and its value type and domain size are
  // ones EvaluateDotBucketsToDevice takes.
  bool EvaluatesDotBucketsOnDevice(int hierarchy_level) const;
  // EvaluateDotBucketsToDevice's argument checks, in its order and with its
  // messages, for a batch of num_keys keys that is (`batch_matches`) or is not
  // one of this DistributedPointFunction.  Touches no device.
  Status CheckDotBucketsArgs(int64_t num_keys, bool batch_matches, int hierarchy_level,
                             Span<const int64_t> bucket_begin, const void* device_db,
                             int64_t db_bytes, int64_t record_words, const void* device_out,
                             int64_t out_bytes) const;
  // Fused full-domain sum over a key batch -- private histograms, private
  // writes: every key of a device batch expanded over its whole domain and
  // summed element by element, without a share vector being stored.  For T =
  // uint64_t or XorWrapper<uint64_t> at `hierarchy_level` (other value types:
  // UNIMPLEMENTED; there is no fallback behind this call), n =
  // log_domain_size in [1, 30], N = 2^n and y_k = EvaluateUntil<T>(
  // hierarchy_level, {}, fresh ctx of key k):
  //   uint64_t:             out[i] = sum_k y_k[i]  (mod 2^64)
  //   XorWrapper<uint64_t>: out[i] = XOR_k y_k[i]           for i in [0, N);
  // the two parties' vectors combine to sum_k beta_k * e_{alpha_k}.  Stateless
  // and key-based.  With `accumulate` false, out[0, N) is overwritten and
  // nothing of what it held is read; with true, the sums are added (XORed)
  // into what it holds, so that several batches stream into one accumulator.
  // An empty batch launches nothing: it writes N zeros, or with `accumulate`
  // leaves the output untouched.  Works on `stream` (asynchronous) and returns
  // N.  The call's table of correction words lives in this object's device
  // scratch (ReleaseScratch frees it).  Checked in this order, before the
  // device is touched, the first failure reported: the level, the value type
  // and its domain size, a null pointer, out_bytes >= N * 8, that the batch
  // is this DPF's, and the output's alignment to 16 bytes.
  StatusOr<int64_t> EvaluateFullDomainSumToDevice(const DeviceKeyBatch& keys, int hierarchy_level,
                                                  void* device_out, int64_t out_bytes,
                                                  bool accumulate, void* stream) const;
  // The same into a fresh vector of N sums returned to the host.
  StatusOr<std::vector<uint64_t>> EvaluateFullDomainSum(const DeviceKeyBatch& keys,
                                                        int hierarchy_level) const;
  // True when `hierarchy_level` exists and its value type and domain size are
  // ones EvaluateFullDomainSumToDevice takes.
  bool EvaluatesFullDomainSumOnDevice(int hierarchy_level) const;
  // EvaluateFullDomainSumToDevice's argument checks, in its order and with its
  // messages, for a batch of num_keys keys that is (`batch_matches`) or is not
  // one of this DistributedPointFunction.  Touches no device.
  Status CheckFullDomainSumArgs(int64_t num_keys, bool batch_matches, int hierarchy_level,
                                const void* device_out, int64_t out_bytes) const;
  // The full-domain sum for every integer width whose elements fill a leaf
  // block -- small counters, flag writes and 128-bit payloads without widening
  // the keys to 64 bits.  With B the bits of T at `hierarchy_level`, E = 128 /
  // B and y_k as above:
  //   uintB_t,             B in {8, 16, 32, 64}:      out[i] = sum_k y_k[i] (mod 2^B)
  //   XorWrapper<uintB_t>, B in {8, 16, 32, 64, 128}: out[i] = XOR_k y_k[i]
  // `out` is N = 2^n packed little-endian elements of T, N * B / 8 bytes, the
  // layout EvaluateUntil writes.  A level is taken when its tree level is n -
  // log2 E (its leaf blocks are full, so n >= log2 E), n <= 30 and the tree has
  // at most 29 levels (XorWrapper<uint128>: n <= 29).  Everything else --
  // additive uint128, IntModN, tuples, a domain below one leaf block, a
  // hierarchy level whose forced tree level leaves blocks partly used -- is
  // UNIMPLEMENTED; there is no fallback behind this call.  A tree of B-bit
  // elements is log2(E / 2) levels shallower than the 64-bit one of the same
  // domain: half the AES at 32 bits, an eighth at 8.  The two 64-bit types
  // give EvaluateFullDomainSumToDevice's bytes.  `accumulate`, the empty
  // batch, `stream`, the scratch and the order of the checks (the level, the
  // type and shape, a null pointer, out_bytes >= N * B / 8, the batch, the
  // alignment) are that call's.  Returns N.
  StatusOr<int64_t> EvaluateFullDomainSumPackedToDevice(const DeviceKeyBatch& keys,
                                                        int hierarchy_level, void* device_out,
                                                        int64_t out_bytes, bool accumulate,
                                                        void* stream) const;
  // The same into a fresh vector of N elements returned to the host.  T must
  // be the level's value type, as for EvaluateUntil<T>.
  template <typename T>
  StatusOr<std::vector<T>> EvaluateFullDomainSumPacked(const DeviceKeyBatch& keys,
                                                       int hierarchy_level) const {
    ValueType t = ToValueType<T>();
    auto packed = EvaluateFullDomainSumPackedBytes(keys, hierarchy_level, &t);
    if (!packed.ok()) return packed.status();
    return Unpack<T>(hierarchy_level, *packed);
  }
  // The packed bytes of the above; `requested_type`, if given, must equal the
  // level's value type.
  StatusOr<std::vector<uint8_t>> EvaluateFullDomainSumPackedBytes(
      const DeviceKeyBatch& keys, int hierarchy_level, const ValueType* requested_type) const;
  // True when `hierarchy_level` exists and its value type, domain size and
  // tree level are ones EvaluateFullDomainSumPackedToDevice takes.
  bool EvaluatesFullDomainSumPackedOnDevice(int hierarchy_level) const;
  // EvaluateFullDomainSumPackedToDevice's argument checks, in its order and
  // with its messages, for a batch of num_keys keys that is (`batch_matches`)
  // or is not one of this DistributedPointFunction.  Touches no device.
  Status CheckFullDomainSumPackedArgs(int64_t num_keys, bool batch_matches, int hierarchy_level,
                                      const void* device_out, int64_t out_bytes) const;
  // Checked private histograms: the full-domain sum of a key batch over a
  // field, with every key's linear sketches taken in the same launch (the
  // per-key vectors exist nowhere else).  For T = IntModN<uint32_t, N_0> or
  // Tuple<IntModN<uint32_t, N_0>, IntModN<uint32_t, N_1>> at `hierarchy_level`
  // (nl leaves; other value types: UNIMPLEMENTED, there is no fallback behind
  // this call), n = log_domain_size in [1, 28], N = 2^n, y_k =
  // EvaluateUntil<T>(hierarchy_level, {}, fresh ctx of key k) and J =
  // num_weight_rows in {0, 1, 2} rows of N public 32-bit weights
  // (`device_weights`, [j][i]):
  //   sum[i][e]       = ( sum_k y_k[i][e] ) mod N_e               uint32 at  i*nl + e
  //   sketch[k][j][e] = ( sum_i (w[j][i] mod N_e) * y_k[i][e] ) mod N_e
  //                                                               uint32 at (k*J + j)*nl + e
  // -- EvaluateUntilBatchSketchToDevice's sketches, in its layout.  J == 0 is
  // the plain field sum; `device_weights` and `device_sketch` are then not
  // read and may be null.  With `accumulate` false sum[0, N*nl) is overwritten
  // and nothing of what it held is read; with true the sums are added mod N_e
  // into what it holds, whose entries must be below N_e.  The sketches are
  // per batch and always overwritten.  An empty batch launches nothing: it
  // writes N*nl zeros, or with `accumulate` leaves the sums untouched.  Works
  // on `stream` (asynchronous) and returns N.  The call's table, accumulators
  // and reduced weights live in this object's device scratch (ReleaseScratch
  // frees it).  Checked in this order, before the device is touched, the first
  // failure reported: the level, the value type and n <= 28, J, null pointers
  // (the sketches' only when there is a key to sketch), sum_bytes >= N*nl*4, sketch_bytes >= K*J*nl*4, that the batch is this
  // DPF's, and alignment (sums to 16 bytes, weights and sketches to 4).
  StatusOr<int64_t> EvaluateFullDomainSumSketchToDevice(
      int hierarchy_level, const DeviceKeyBatch& keys, const uint32_t* device_weights,
      int num_weight_rows, void* device_sum, int64_t sum_bytes, void* device_sketch,
      int64_t sketch_bytes, bool accumulate, void* stream) const;
  // The same with host weights (J rows of N) into fresh vectors returned to
  // the host: N*nl sums and K*J*nl sketches.
  struct SumSketch {
    std::vector<uint32_t> sum, sketch;
  };
  StatusOr<SumSketch> EvaluateFullDomainSumSketch(int hierarchy_level, const DeviceKeyBatch& keys,
                                                  Span<const uint32_t> weights,
                                                  int num_weight_rows) const;
  // True when `hierarchy_level` exists and its value type and domain size are
  // ones EvaluateFullDomainSumSketchToDevice takes.
  bool EvaluatesFullDomainSumSketchOnDevice(int hierarchy_level) const;
  // EvaluateFullDomainSumSketchToDevice's argument checks, in its order and
  // with its messages, for a batch of num_keys keys that is (`batch_matches`)
  // or is not one of this DistributedPointFunction.  Touches no device.
  Status CheckFullDomainSumSketchArgs(int64_t num_keys, bool batch_matches, int hierarchy_level,
                                      const void* device_weights, int num_weight_rows,
                                      const void* device_sum, int64_t sum_bytes,
                                      const void* device_sketch, int64_t sketch_bytes) const;
  // ---- device-resident incremental evaluation of a key batch (8f.1, cfg 5b)
  // A fresh context for every key of `keys` (previous_hierarchy_level -1), as
  // CreateEvaluationContext would make per key.  `keys` must outlive it.
  StatusOr<std::unique_ptr<DeviceBatchContext>> CreateBatchEvaluationContext(
      const DeviceKeyBatch& keys) const;
  // EvaluateUntil(hierarchy_level, prefixes, ctx_k) for every key k of the
  // batch, at the same prefixes for all keys (same validation and errors as
  // EvaluateUntil): writes num_keys rows of n packed elements ([key][element])
  // to device_out and returns n.
  StatusOr<int64_t> EvaluateUntilBatchToDevice(int hierarchy_level, Span<const uint128> prefixes,
                                               DeviceBatchContext& ctx, void* device_out,
                                               int64_t capacity_bytes, void* stream) const;
  // Aggregation variant: out[j] = group sum over the batch's keys of
  // EvaluateUntil(hierarchy_level, prefixes, ctx_k)[j] (n packed elements).
  StatusOr<int64_t> EvaluateUntilBatchSumToDevice(int hierarchy_level,
                                                  Span<const uint128> prefixes,
                                                  DeviceBatchContext& ctx, void* device_out,
                                                  int64_t capacity_bytes, void* stream) const;
  // Sketch variant: besides (optionally) the key sums of
  // EvaluateUntilBatchSumToDevice in device_sums, every key's linear sketch
  // of its own output vector y_k = EvaluateUntil(hierarchy_level, prefixes,
  // ctx_k) under num_weight_rows (1..4) rows of weights_per_row == n uint32
  // weights (device, row-major):
  //   device_sketch[(k*J + j)*nl + e] = (sum_i (w[j][i] mod N_e) * y_k[i][e]) mod N_e
  // for value types whose nl leaves are all IntModN<uint32_t, N_e> (others:
  // UNIMPLEMENTED).  Leaves the context exactly as the sum call does and
  // returns n.  All argument checks run before the context is touched.
  StatusOr<int64_t> EvaluateUntilBatchSketchToDevice(
      int hierarchy_level, Span<const uint128> prefixes, DeviceBatchContext& ctx,
      const uint32_t* device_weights, int num_weight_rows, int64_t weights_per_row,
      void* device_sums /*may be null*/, int64_t sums_capacity_bytes, uint32_t* device_sketch,
      int64_t sketch_capacity_bytes, void* stream) const;
  // Key k's context as the EvaluationContext proto EvaluateUntil would have
  // left (lazy serialization; `host_keys` is the batch `ctx` was uploaded from).
  StatusOr<EvaluationContext> ExportEvaluationContext(const DeviceBatchContext& ctx,
                                                      const KeyBatch& host_keys, int64_t k,
                                                      void* stream) const;

  // Gives back the per-object host and device scratch the evaluation calls
  // keep between calls (page-locked argument images, staging, device buffers,
  // the prefix dedup's vectors): hundreds of MB after one huge hierarchical
  // call.  Waits for work in flight that reads them; the next call
  // reallocates.  Must not run concurrently with a call on this object.
  void ReleaseScratch();

  // Group sum of `num_shares` packed output vectors of `count` elements each
  // (host memory), e.g. per-GPU partial sums after an all-gather.
  StatusOr<std::vector<uint8_t>> SumPackedShares(int hierarchy_level, const uint8_t* shares,
                                                 int64_t num_shares, int64_t count) const;

  // Introspection.
  int tree_levels_needed() const { return validator_->tree_levels_needed(); }
  const std::vector<int>& hierarchy_to_tree() const { return validator_->hierarchy_to_tree(); }
  int blocks_needed(int h) const { return blocks_needed_[h]; }
  const dpf_internal::FlatValueType& flat_value_type(int h) const { return flat_[h]; }
  int corrected_elements_per_block(int h) const {
    return 1 << (parameters()[h].log_domain_size() - hierarchy_to_tree()[h]);
  }
  // Number of output elements EvaluateUntil(h, prefixes) produces.
  StatusOr<int64_t> OutputElements(int hierarchy_level, int64_t num_prefixes,
                                   int previous_hierarchy_level) const;

 private:
  struct DeviceStart;  // seeds + control bits of the expansion starts, on device

  DistributedPointFunction(std::unique_ptr<dpf_internal::ProtoValidator> validator,
                           std::vector<int> blocks_needed, std::vector<dpf_internal::FlatValueType> flat,
                           Aes128FixedKeyHash prg_left, Aes128FixedKeyHash prg_right,
                           Aes128FixedKeyHash prg_value);

  // EvaluateAt<T> (h:839-1010): the packed output copied or unpacked into
  // the result chunk by chunk, as EvaluateUntil<T> does.
  template <typename T>
  StatusOr<std::vector<T>> EvaluateAtImpl(const DpfKey& key, int hierarchy_level,
                                          Span<const uint128> evaluation_points,
                                          EvaluationContext* ctx) const {
    ValueType t = ToValueType<T>();
    std::vector<T> out;
    if constexpr (dpf_internal::kPackedIsMemoryImage<T>) {
      const HostSink sink = dpf_internal::VectorSink(&out);
      Status status = EvaluateAtToHost(key, hierarchy_level, evaluation_points, ctx, &t, sink);
      if (!status.ok()) return status;
    } else {
      const HostSink sink = dpf_internal::UnpackSink(&flat_, hierarchy_level, &out);
      Status status = EvaluateAtToHost(key, hierarchy_level, evaluation_points, ctx, &t, sink);
      if (!status.ok()) return status;
    }
    return out;
  }

  template <typename T>
  StatusOr<std::vector<T>> Unpack(int h, const std::vector<uint8_t>& packed) const {
    const auto& flat = flat_[h];
    return dpf_internal::UnpackElements<T>(flat, packed.data(),
                                           static_cast<int64_t>(packed.size() / flat.packed_size));
  }

  // Key generation pieces (cc:63-204).
  StatusOr<std::vector<uint128>> ComputeValueCorrectionLeaves(int hierarchy_level,
                                                              const uint128 seeds[2], uint128 alpha,
                                                              Span<const uint128> beta_leaves,
                                                              bool invert) const;
  Status CheckValueCorrectionKnown(int hierarchy_level) const;
  Status GenerateNextCore(int tree_level, uint128 alpha, uint128 seeds[2], bool control_bits[2],
                          uint128* seed_correction, bool ccw[2]) const;
  StatusOr<std::vector<Value>> ComputeValueCorrection(int hierarchy_level, const uint128 seeds[2],
                                                      uint128 alpha, const Value& beta,
                                                      bool invert) const;
  Status GenerateNext(int tree_level, uint128 alpha, Span<const Value> beta, uint128 seeds[2],
                      bool control_bits[2], DpfKey keys[2]) const;

  // Shared evaluation core; output goes to device_out (caller-owned device
  // memory) or, when device_out is null, to *host_out.
  Status EvaluateUntilCore(int hierarchy_level, Span<const uint128> prefixes,
                           EvaluationContext& ctx, const ValueType* requested_type,
                           void* device_out, int64_t capacity_bytes, void* stream,
                           const HostSink* host_out, int64_t* num_elements) const;
  // ComputePartialEvaluations (cc:351-453), path walk on the GPU.
  // `before_device` (may be empty) runs after the host-side lookups and before
  // any device work, so host validation errors never leave work in flight.
  Status ComputePartialEvaluations(Span<const uint128> prefixes, int hierarchy_level,
                                   bool update_ctx, EvaluationContext& ctx,
                                   DeviceStart* out, void* stream,
                                   const std::function<Status()>& before_device) const;
  StatusOr<std::vector<uint128>> ValueCorrectionLeaves(const DpfKey& key, int h) const;
  // Every argument check of EvaluateSelectToDevice, and the shard's shape
  // they derive (`shape` may be null); touches no device.
  struct SelectShape;
  Status CheckSelectArgs(Span<const DpfKey* const> keys, int hierarchy_level, int64_t shard,
                         int64_t num_shards, const void* device_db, int64_t db_bytes,
                         int64_t record_words, const void* device_out, int64_t out_bytes,
                         SelectShape* shape) const;
  // Every argument check of EvaluateDotBatchToDevice, in CheckSelectArgs'
  // order, and the shard's shape (`shape` may be null); touches no device.
  Status CheckDotBatchArgs(Span<const DpfKey* const> keys, int hierarchy_level, int64_t shard,
                           int64_t num_shards, const void* device_db, int64_t db_bytes,
                           int64_t record_words, const void* device_out, int64_t out_bytes,
                           SelectShape* shape) const;
  // Sizes `b` for n keys, and fills row k from `key` (validated).
  void ResizeKeyBatch(int64_t n, KeyBatch* b) const;
  Status FillKeyBatchRow(const DpfKey& key, int64_t k, KeyBatch* b) const;
  // Shared core of the two batched EvaluateUntil entry points, and its steps
  // (csrc/host/batch_context.cc): the argument checks, the host-side plan of
  // the call, and the kernel launch with the output gather.
  struct BatchSketch;  // the sketch output mode's arguments
  StatusOr<int64_t> EvaluateUntilBatchCore(int hierarchy_level, Span<const uint128> prefixes,
                                           DeviceBatchContext& ctx, bool sum, void* device_out,
                                           int64_t capacity_bytes, void* stream,
                                           const BatchSketch* sketch = nullptr) const;
  struct BatchCall;
  Status CheckUntilBatchArgs(int hierarchy_level, Span<const uint128> prefixes,
                             const DeviceBatchContext& ctx) const;
  Status PlanBatchCall(int hierarchy_level, int64_t num_prefixes, const DeviceBatchContext& ctx,
                       bool sum, BatchCall* call) const;
  Status LaunchBatchCall(int hierarchy_level, BatchCall& call, DeviceBatchContext& ctx, bool sum,
                         void* device_out, void* stream, const BatchSketch* sketch) const;

  std::unique_ptr<dpf_internal::ProtoValidator> validator_;
  std::vector<int> blocks_needed_;
  std::vector<dpf_internal::FlatValueType> flat_;
  Aes128FixedKeyHash prg_left_, prg_right_, prg_value_;
  std::set<std::string> registered_types_;
  std::unique_ptr<dpf_internal::DeviceScratch> scratch_;
};

}  // namespace distributed_point_functions

#endif  // DPF_DISTRIBUTED_POINT_FUNCTION_H_
