// distributed_comparison_function.h -- the reference's
// DistributedComparisonFunction (dcf/distributed_comparison_function.h:30-105)
// as a drop-in over the MI355X DPF engine.
//
// A DCF with log domain n is an n-level incremental DPF (level i has log
// domain i) whose level-i value is beta when bit (n-1-i) of alpha is set and
// 0 otherwise (cc:79-101); Evaluate(key, x) sums the levels whose bit of x is
// clear (h:83-105).  Here every evaluation -- single point, many points, many
// keys -- is ONE walk down x's path per (key, point) in the gfx950 kernel
// dpf_hip_dcf_eval_batch, instead of n root-to-level EvaluateAt walks.
#ifndef DCF_DISTRIBUTED_COMPARISON_FUNCTION_H_
#define DCF_DISTRIBUTED_COMPARISON_FUNCTION_H_

#include <memory>
#include <utility>
#include <vector>

#include "dcf/distributed_comparison_function.pb.h"
#include "dpf/distributed_point_function.h"

namespace distributed_point_functions {

namespace dpf_internal {
class DeviceScratch;
class PackedUploads;
}

class DistributedComparisonFunction {
 public:
  static StatusOr<std::unique_ptr<DistributedComparisonFunction>> Create(
      const DcfParameters& parameters);

  // Keys for x -> beta if x < alpha else 0 (cc:79-101).
  StatusOr<std::pair<DcfKey, DcfKey>> GenerateKeys(uint128 alpha, const Value& beta);
  template <typename T, typename = std::enable_if_t<!std::is_convertible_v<T, Value> &&
                                                    is_supported_type_v<T>>>
  StatusOr<std::pair<DcfKey, DcfKey>> GenerateKeys(uint128 alpha, const T& beta) {
    StatusOr<Value> value = dpf_->ToValue(beta);
    if (!value.ok()) return value.status();
    return GenerateKeys(alpha, *value);
  }

  // h:83-105.
  template <typename T>
  StatusOr<T> Evaluate(const DcfKey& key, uint128 x) {
    ValueType t = ToValueType<T>();
    StatusOr<std::vector<uint8_t>> packed = EvaluatePacked(key, Span<const uint128>(&x, 1), &t);
    if (!packed.ok()) return packed.status();
    std::vector<T> v = dpf_internal::UnpackElements<T>(dpf_->flat_value_type(0), packed->data(), 1);
    return v[0];
  }

  DistributedComparisonFunction(const DistributedComparisonFunction&) = delete;
  DistributedComparisonFunction& operator=(const DistributedComparisonFunction&) = delete;
  ~DistributedComparisonFunction();

  // ---- MI355X extensions ---------------------------------------------------
  // GenerateKeys with caller-supplied root seeds (reproducible fixtures).
  StatusOr<std::pair<DcfKey, DcfKey>> GenerateKeysWithSeeds(uint128 alpha, const Value& beta,
                                                            uint128 seed_0, uint128 seed_1);
  // Evaluate(key, x) for every x of `xs`, packed elements (one launch).
  // `requested_type` (may be null) plays the role of T.
  StatusOr<std::vector<uint8_t>> EvaluatePacked(const DcfKey& key, Span<const uint128> xs,
                                                const ValueType* requested_type = nullptr);
  // Evaluate for every key of a device batch (rows of the DCF keys' DpfKeys,
  // MakeKeyBatch) at device points: points_per_key per key ([key][point]), or
  // one shared set when `shared_points`.  Writes packed [key][point] outputs.
  StatusOr<int64_t> EvaluateBatchToDevice(const DeviceKeyBatch& keys, const void* device_points,
                                          int64_t points_per_key, bool shared_points,
                                          void* device_out, int64_t capacity_bytes,
                                          void* stream) const;
  // ---- full-domain evaluation ------------------------------------------------
  // Evaluate(key, x) at every x of the domain in one depth-first walk of the
  // key's tree (dpf_hip_dcf_expand: 2^(n+1) - 3 AES for 2^n outputs, against
  // (2n - 1) * 2^n point by point).  Only for the value types
  // EvaluatesFullDomainOnDevice() reports -- one integer or XorWrapper of 8 to
  // 128 bits; every other type is UNIMPLEMENTED: no per-point path stands in.
  // Shard `shard` of `num_shards` = 2^k is the x whose top k bits are `shard`
  // (num_shards <= 2^(n-1)).  Checked before the device is touched, in this
  // order: requested type, key or batch, shard arguments, record_words,
  // buffers, value type.
  //
  // Packed elements [x - first_x] of one key's shard into `device_out` (16-byte
  // aligned) on `stream`; returns the number of elements written.
  StatusOr<int64_t> EvaluateFullDomainToDevice(const DcfKey& key, int64_t shard,
                                               int64_t num_shards, void* device_out,
                                               int64_t capacity_bytes, void* stream);
  // The same for every key of a device batch: [key][x - first_x].
  StatusOr<int64_t> EvaluateFullDomainBatchToDevice(const DeviceKeyBatch& keys, int64_t shard,
                                                    int64_t num_shards, void* device_out,
                                                    int64_t capacity_bytes, void* stream) const;
  // The whole domain on the host.  `requested_type` (may be null) plays the
  // role of T.
  StatusOr<std::vector<uint8_t>> EvaluateFullDomainPacked(
      const DcfKey& key, const ValueType* requested_type = nullptr);
  template <typename T>
  StatusOr<std::vector<T>> EvaluateFullDomain(const DcfKey& key) {
    ValueType t = ToValueType<T>();
    StatusOr<std::vector<uint8_t>> packed = EvaluateFullDomainPacked(key, &t);
    if (!packed.ok()) return packed.status();
    const auto& f = dpf_->flat_value_type(0);
    return dpf_internal::UnpackElements<T>(f, packed->data(),
                                           static_cast<int64_t>(packed->size() / f.packed_size));
  }
  bool EvaluatesFullDomainOnDevice() const;
  // Private range query over a database of uint64 records (uint64_t DCFs
  // only, the integer type dpf_hip_dot_rows takes): out[w] = sum over the
  // shard's x of f(x) * db[x - first_x][w] mod 2^64, so the two parties'
  // results add to beta * (sum of db[x][w] over x < alpha).  `device_db` holds
  // the shard's records, record_words uint64 each.  A host composition: the
  // shard's share vector is written slab by slab -- sub-shards of the same
  // kernel -- into this object's scratch and folded by dpf_hip_dot_rows.
  // Returns record_words.
  StatusOr<int64_t> EvaluateRangeDotToDevice(const DcfKey& key, int64_t shard, int64_t num_shards,
                                             const void* device_db, int64_t db_bytes,
                                             int64_t record_words, void* device_out,
                                             int64_t out_bytes, void* stream);
  // The whole domain's fold on the host: record_words uint64.
  StatusOr<std::vector<uint64_t>> EvaluateRangeDot(const DcfKey& key, const void* device_db,
                                                   int64_t db_bytes, int64_t record_words);
  // SoA batch of the DpfKeys inside `keys` (validated like EvaluateAt does).
  StatusOr<KeyBatch> MakeKeyBatch(Span<const DcfKey* const> keys) const;
  // Key generation for many alphas at once, straight into SoA form: row k of
  // the two batches is GenerateKeysWithSeeds(alphas[k], beta_k, root_seeds[2k],
  // root_seeds[2k+1]) passed through MakeKeyBatch.  `betas` holds one value
  // for all keys or one per key; empty root_seeds are drawn as GenerateKeys
  // draws them.  On `num_threads` host threads (0 = hardware concurrency).
  StatusOr<std::pair<KeyBatch, KeyBatch>> GenerateKeyBatch(Span<const uint128> alphas,
                                                           Span<const Value> betas,
                                                           Span<const uint128> root_seeds,
                                                           int num_threads = 0) const;
  // The same batches generated in device memory on `stream`
  // (DistributedPointFunction::GenerateKeyBatchToDevice; on the GPU where
  // dpf().GeneratesKeysOnDevice(), else on the host and uploaded).
  StatusOr<DistributedPointFunction::DeviceKeyBatchPair> GenerateKeyBatchToDevice(
      Span<const uint128> alphas, Span<const Value> betas, Span<const uint128> root_seeds,
      void* stream) const;
  const DcfParameters& parameters() const { return parameters_; }
  const DistributedPointFunction& dpf() const { return *dpf_; }

 private:
  // The checks of the batched generators (those of the DPF's GenerateKeyBatch
  // on alphas >> 1), the DPF's alphas and one row of beta leaves per beta.
  Status CheckKeyBatchArgs(Span<const uint128> alphas, Span<const Value> betas,
                           Span<const uint128> root_seeds, std::vector<uint128>* dpf_alphas,
                           std::vector<uint128>* leaves) const;
  // Host generation from checked arguments.
  StatusOr<std::pair<KeyBatch, KeyBatch>> GenerateKeyBatchHost(
      Span<const uint128> alphas, const std::vector<uint128>& dpf_alphas,
      const std::vector<uint128>& leaves, Span<const uint128> root_seeds, int num_threads) const;
  DistributedComparisonFunction(DcfParameters parameters,
                                std::unique_ptr<DistributedPointFunction> dpf);
  StatusOr<std::pair<DcfKey, DcfKey>> GenerateKeysImpl(uint128 alpha, const Value& beta,
                                                       const uint128* seeds);
  // Per-level EvaluateAt loop of the reference, for value types the kernel
  // does not take (more than 4 tuple leaves).
  StatusOr<std::vector<uint8_t>> EvaluateByLevels(const DcfKey& key, Span<const uint128> xs);

  // The kernel launch shared by the device-batch and host entry points.
  Status Launch(int64_t num_keys, int64_t points_per_key, bool shared_points,
                const dpf_block* seed, const uint8_t* party, const dpf_block* points,
                const dpf_block* cw_seed, const uint8_t* cw_left, const uint8_t* cw_right,
                int cw_stride, const std::vector<const dpf_block*>& vcw, void* device_out,
                void* stream) const;

  // dpf_hip_dcf_expand for a key batch in device memory: shard `shard` of
  // 2^shard_bits, for every key of the batch.
  struct DeviceKeys;
  Status LaunchFullDomain(const DeviceKeys& keys, int shard_bits, int64_t shard, void* device_out,
                          void* stream) const;
  // Packs one key's batch into `up` (reset here, committed on `stream`).
  Status UploadKey(const KeyBatch& batch, dpf_internal::PackedUploads& up, void* stream,
                   DeviceKeys* keys) const;
  // UNIMPLEMENTED unless dpf_hip_dcf_expand takes this DCF.
  Status CheckFullDomainType() const;
  // The host checks of a range dot call (device_out only where `has_out`) and
  // what they work out; then the call itself.
  struct RangeDotCall;
  Status CheckRangeDot(const DcfKey& key, int64_t shard, int64_t num_shards,
                       const void* device_db, int64_t db_bytes, int64_t record_words,
                       bool has_out, const void* device_out, int64_t out_bytes,
                       RangeDotCall* call) const;
  Status RunRangeDot(const RangeDotCall& call, int64_t shard, const void* device_db,
                     int64_t record_words, void* device_out, void* stream);

  const DcfParameters parameters_;
  const std::unique_ptr<DistributedPointFunction> dpf_;
  // Reused device buffers and staged uploads of the host entry points.
  const std::unique_ptr<dpf_internal::DeviceScratch> scratch_;
};

}  // namespace distributed_point_functions

#endif  // DCF_DISTRIBUTED_COMPARISON_FUNCTION_H_
