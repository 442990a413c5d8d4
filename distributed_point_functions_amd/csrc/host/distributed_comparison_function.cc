// distributed_comparison_function.cc -- DistributedComparisonFunction
// (dcf/distributed_comparison_function.cc:15-102, .h:83-105) over the MI355X
// DPF engine; see the header.
#include "dcf/distributed_comparison_function.h"

#include <algorithm>
#include <cstdlib>
#include <limits>
#include <optional>

#include "dpf/key_batch.h"
#include "dpf_hip.h"
#include "host_util.h"
#include "shard_plan.h"

namespace distributed_point_functions {

using dpf_internal::AesKey;
using dpf_internal::FromHip;
using dpf_internal::kPrgKeyLeft;
using dpf_internal::kPrgKeyRight;
using dpf_internal::kPrgKeyValue;
using dpf_internal::MakeDesc;
using dpf_internal::ToBlock;

namespace {

// cc:21-32: integers, IntModN and tuples (recursively) become 0; other kinds
// (XorWrapper) are left as they are, exactly like the reference.
void SetToZero(Value& value) {
  if (value.value_case() == Value::kInteger) {
    value.mutable_integer()->set_value_uint64(0);
  } else if (value.value_case() == Value::kIntModN) {
    value.mutable_int_mod_n()->set_value_uint64(0);
  } else if (value.value_case() == Value::kTuple) {
    for (int i = 0; i < value.tuple().elements_size(); ++i)
      SetToZero(*value.mutable_tuple()->mutable_elements(i));
  }
}


}  // namespace

DistributedComparisonFunction::DistributedComparisonFunction(
    DcfParameters parameters, std::unique_ptr<DistributedPointFunction> dpf)
    : parameters_(std::move(parameters)),
      dpf_(std::move(dpf)),
      scratch_(new dpf_internal::DeviceScratch()) {}

DistributedComparisonFunction::~DistributedComparisonFunction() = default;

StatusOr<std::unique_ptr<DistributedComparisonFunction>> DistributedComparisonFunction::Create(
    const DcfParameters& parameters) {
  // cc:38-72
  if (parameters.parameters().log_domain_size() < 1)
    return InvalidArgumentError("A DCF must have log_domain_size >= 1");
  if (!parameters.parameters().has_value_type())
    return InvalidArgumentError(
        "parameters.value_type must be set for DistributedComparisonFunction::Create");
  std::vector<DpfParameters> dpf_parameters(parameters.parameters().log_domain_size());
  for (int i = 0; i < static_cast<int>(dpf_parameters.size()); ++i) {
    dpf_parameters[i].set_log_domain_size(i);
    *dpf_parameters[i].mutable_value_type() = parameters.parameters().value_type();
  }
  DPF_RETURN_IF_ERROR(dpf_internal::ProtoValidator::ValidateParameters(dpf_parameters));
  DPF_ASSIGN_OR_RETURN(std::unique_ptr<DistributedPointFunction> dpf,
                       DistributedPointFunction::CreateIncremental(dpf_parameters));
  DPF_RETURN_IF_ERROR(dpf->RegisterValueType(parameters.parameters().value_type()));
  return std::unique_ptr<DistributedComparisonFunction>(
      new DistributedComparisonFunction(parameters, std::move(dpf)));
}

StatusOr<std::pair<DcfKey, DcfKey>> DistributedComparisonFunction::GenerateKeys(
    uint128 alpha, const Value& beta) {
  return GenerateKeysImpl(alpha, beta, nullptr);
}

StatusOr<std::pair<DcfKey, DcfKey>> DistributedComparisonFunction::GenerateKeysWithSeeds(
    uint128 alpha, const Value& beta, uint128 seed_0, uint128 seed_1) {
  const uint128 seeds[2] = {seed_0, seed_1};
  return GenerateKeysImpl(alpha, beta, seeds);
}

StatusOr<std::pair<DcfKey, DcfKey>> DistributedComparisonFunction::GenerateKeysImpl(
    uint128 alpha, const Value& beta, const uint128* seeds) {
  // cc:79-101
  const int n = parameters_.parameters().log_domain_size();
  std::vector<Value> dpf_values(n, beta);
  for (int i = 0; i < n; ++i) {
    const bool current_bit = (alpha & (uint128{1} << (n - i - 1))) != 0;
    if (!current_bit) SetToZero(dpf_values[i]);
  }
  // The last bit of alpha is encoded in dpf_values.back() (cc:95-97).
  std::pair<DpfKey, DpfKey> keys;
  if (seeds) {
    DPF_ASSIGN_OR_RETURN(keys, dpf_->GenerateKeysIncrementalWithSeeds(
                                   alpha >> 1, Span<const Value>(dpf_values), seeds[0], seeds[1]));
  } else {
    DPF_ASSIGN_OR_RETURN(keys, dpf_->GenerateKeysIncremental(alpha >> 1, Span<const Value>(dpf_values)));
  }
  std::pair<DcfKey, DcfKey> result;
  *result.first.mutable_key() = std::move(keys.first);
  *result.second.mutable_key() = std::move(keys.second);
  return result;
}

// ------------------------------------------------------------ batched keygen
Status DistributedComparisonFunction::CheckKeyBatchArgs(Span<const uint128> alphas,
                                                        Span<const Value> betas,
                                                        Span<const uint128> root_seeds,
                                                        std::vector<uint128>* dpf_alphas,
                                                        std::vector<uint128>* leaves) const {
  const int64_t n = static_cast<int64_t>(alphas.size());
  if (betas.size() != 1 && static_cast<int64_t>(betas.size()) != n)
    return InvalidArgumentError("`betas` must hold one value or one per alpha");
  // The last bit of alpha is encoded in the last level's value (cc:95-97).
  dpf_alphas->resize(n);
  for (int64_t k = 0; k < n; ++k) (*dpf_alphas)[k] = alphas[k] >> 1;
  return dpf_->CheckKeyBatchArgs(MakeConstSpan(*dpf_alphas), betas,
                                 static_cast<int64_t>(betas.size()), true, root_seeds, leaves);
}

StatusOr<std::pair<KeyBatch, KeyBatch>> DistributedComparisonFunction::GenerateKeyBatchHost(
    Span<const uint128> alphas, const std::vector<uint128>& dpf_alphas,
    const std::vector<uint128>& leaves, Span<const uint128> root_seeds, int num_threads) const {
  // GenerateKeysImpl's dpf_values for every key, as leaves: level i takes beta
  // where bit n-1-i of alpha is set and SetToZero(beta) elsewhere, which
  // clears integer and IntModN leaves and leaves XorWrapper leaves alone.
  const int n = parameters_.parameters().log_domain_size();
  const int64_t keys = static_cast<int64_t>(alphas.size());
  const auto& f = dpf_->flat_value_type(0);
  const size_t nl = f.leaves.size();
  const int64_t rows = static_cast<int64_t>(leaves.size() / nl);
  std::vector<uint128> per_level(static_cast<size_t>(keys) * n * nl);
  for (int64_t k = 0; k < keys; ++k) {
    const uint128* beta = leaves.data() + (rows == 1 ? 0 : k) * nl;
    for (int i = 0; i < n; ++i) {
      const bool current_bit = (alphas[k] & (uint128{1} << (n - i - 1))) != 0;
      uint128* dst = per_level.data() + (static_cast<size_t>(k) * n + i) * nl;
      for (size_t l = 0; l < nl; ++l)
        dst[l] = current_bit || f.leaves[l].kind == dpf_internal::kLeafXor ? beta[l] : uint128{0};
    }
  }
  return dpf_->GenerateKeyBatchFromLeaves(MakeConstSpan(dpf_alphas), MakeConstSpan(per_level), keys,
                                          root_seeds, num_threads);
}

StatusOr<std::pair<KeyBatch, KeyBatch>> DistributedComparisonFunction::GenerateKeyBatch(
    Span<const uint128> alphas, Span<const Value> betas, Span<const uint128> root_seeds,
    int num_threads) const {
  std::vector<uint128> dpf_alphas, leaves;
  DPF_RETURN_IF_ERROR(CheckKeyBatchArgs(alphas, betas, root_seeds, &dpf_alphas, &leaves));
  return GenerateKeyBatchHost(alphas, dpf_alphas, leaves, root_seeds, num_threads);
}

StatusOr<DistributedPointFunction::DeviceKeyBatchPair>
DistributedComparisonFunction::GenerateKeyBatchToDevice(Span<const uint128> alphas,
                                                        Span<const Value> betas,
                                                        Span<const uint128> root_seeds,
                                                        void* stream) const {
  std::vector<uint128> dpf_alphas, leaves;
  DPF_RETURN_IF_ERROR(CheckKeyBatchArgs(alphas, betas, root_seeds, &dpf_alphas, &leaves));
  if (!dpf_->GeneratesKeysOnDevice()) {
    std::pair<KeyBatch, KeyBatch> host;
    DPF_ASSIGN_OR_RETURN(host, GenerateKeyBatchHost(alphas, dpf_alphas, leaves, root_seeds, 0));
    DistributedPointFunction::DeviceKeyBatchPair out;
    DPF_ASSIGN_OR_RETURN(out.first, DeviceKeyBatch::Upload(host.first, stream));
    DPF_ASSIGN_OR_RETURN(out.second, DeviceKeyBatch::Upload(host.second, stream));
    return out;
  }
  // One leaf per value: the kernel's DCF mode takes one beta per key.
  const int64_t keys = static_cast<int64_t>(alphas.size());
  if (static_cast<int64_t>(leaves.size()) != keys) {
    const uint128 shared = leaves.empty() ? uint128{0} : leaves[0];
    leaves.assign(keys, shared);
  }
  return dpf_->GenerateKeyBatchFromLeavesToDevice(alphas, MakeConstSpan(leaves), 2,
                                                  parameters_.parameters().log_domain_size(),
                                                  root_seeds, stream);
}

StatusOr<KeyBatch> DistributedComparisonFunction::MakeKeyBatch(
    Span<const DcfKey* const> keys) const {
  std::vector<const DpfKey*> dpf_keys;
  dpf_keys.reserve(keys.size());
  for (const DcfKey* k : keys) dpf_keys.push_back(&k->key());
  return dpf_->MakeKeyBatch(Span<const DpfKey* const>(dpf_keys));
}

StatusOr<int64_t> DistributedComparisonFunction::EvaluateBatchToDevice(
    const DeviceKeyBatch& keys, const void* device_points, int64_t points_per_key,
    bool shared_points, void* device_out, int64_t capacity_bytes, void* stream) const {
  const int n = parameters_.parameters().log_domain_size();
  if (keys.num_levels() != dpf_->tree_levels_needed() - 1 || keys.num_hierarchy_levels() != n)
    return InvalidArgumentError("key batch does not match this DistributedComparisonFunction");
  if (points_per_key < 0) return InvalidArgumentError("points_per_key must be non-negative");
  const int64_t total = keys.num_keys() * points_per_key;
  if (total == 0) return int64_t{0};
  const auto& f = dpf_->flat_value_type(0);
  if (!device_out || capacity_bytes < total * f.packed_size)
    return InvalidArgumentError("device output buffer too small");
  // EvaluateAt(key, 0, {x >> n}) rejects x >= 2^n (h:861-874).
  const int64_t num_points = shared_points ? points_per_key : total;
  if (n < 128) {
    int64_t bad = 0;
    HIP_RETURN_IF_ERROR(dpf_hip_count_out_of_range(
        num_points, static_cast<const dpf_block*>(device_points), n, &bad, stream));
    if (bad)
      return InvalidArgumentError(
          "`evaluation_points[0]` larger than the domain size at hierarchy level 0");
  }
  std::vector<const dpf_block*> vcw(n);
  for (int i = 0; i < n; ++i) vcw[i] = keys.value_correction(i);
  DPF_RETURN_IF_ERROR(Launch(keys.num_keys(), points_per_key, shared_points, keys.seed(),
                             keys.party(), static_cast<const dpf_block*>(device_points),
                             keys.cw_seed(), keys.cw_left(), keys.cw_right(), keys.num_levels(),
                             vcw, device_out, stream));
  return total;
}

Status DistributedComparisonFunction::Launch(int64_t num_keys, int64_t points_per_key,
                                             bool shared_points, const dpf_block* seed,
                                             const uint8_t* party, const dpf_block* points,
                                             const dpf_block* cw_seed, const uint8_t* cw_left,
                                             const uint8_t* cw_right, int cw_stride,
                                             const std::vector<const dpf_block*>& vcw,
                                             void* device_out, void* stream) const {
  const int n = parameters_.parameters().log_domain_size();
  const auto& f = dpf_->flat_value_type(0);
  std::vector<int32_t> depth(n), blocks(n);
  for (int i = 0; i < n; ++i) {
    depth[i] = dpf_->hierarchy_to_tree()[i];
    blocks[i] = dpf_->blocks_needed(i);
  }
  const dpf_value_desc desc = MakeDesc(f, blocks[0]);
  const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight), kv = AesKey(kPrgKeyValue);
  HIP_RETURN_IF_ERROR(dpf_hip_dcf_eval_batch(
      num_keys, points_per_key, shared_points ? 1 : 0, n, depth.data(), blocks.data(), seed, party,
      points, cw_seed, cw_left, cw_right, cw_stride, vcw.data(), &kl, &kr, &kv, &desc, device_out,
      stream));
  return OkStatus();
}

// ------------------------------------------------------- full-domain evaluation
// A key batch in device memory as dpf_hip_dcf_expand takes it.
struct DistributedComparisonFunction::DeviceKeys {
  int64_t num_keys = 0;
  const dpf_block* seed = nullptr;
  const uint8_t* party = nullptr;
  const dpf_block* cw_seed = nullptr;
  const uint8_t* cw_left = nullptr;
  const uint8_t* cw_right = nullptr;
  int cw_stride = 0;
  std::vector<const dpf_block*> vcw;   // per level
};

namespace {

// The slab hook of the database folds (DPF_DOT_SLAB_LOG, read per call; test
// hook): the log2 of a slab's rows, in place of the scratch bound.
std::optional<int> DotSlabLogHook() {
  const char* v = std::getenv("DPF_DOT_SLAB_LOG");
  return v && *v ? std::optional<int>(std::atoi(v)) : std::nullopt;
}

}  // namespace

bool DistributedComparisonFunction::EvaluatesFullDomainOnDevice() const {
  const int n = parameters_.parameters().log_domain_size();
  std::vector<int32_t> depth(n);
  for (int i = 0; i < n; ++i) depth[i] = dpf_->hierarchy_to_tree()[i];
  const dpf_value_desc desc = MakeDesc(dpf_->flat_value_type(0), dpf_->blocks_needed(0));
  return dpf_hip_dcf_expand_supported(&desc, n, depth.data()) != 0;
}

Status DistributedComparisonFunction::CheckFullDomainType() const {
  if (EvaluatesFullDomainOnDevice()) return OkStatus();
  return UnimplementedError(
      "full-domain DCF evaluation is implemented for one integer or XorWrapper value of 8, 16, "
      "32, 64 or 128 bits");
}

Status DistributedComparisonFunction::LaunchFullDomain(const DeviceKeys& keys, int shard_bits,
                                                       int64_t shard, void* device_out,
                                                       void* stream) const {
  const int n = parameters_.parameters().log_domain_size();
  const dpf_value_desc desc = MakeDesc(dpf_->flat_value_type(0), dpf_->blocks_needed(0));
  const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight), kv = AesKey(kPrgKeyValue);
  HIP_RETURN_IF_ERROR(dpf_hip_dcf_expand(keys.num_keys, n, shard_bits, shard, keys.seed, keys.party,
                                         keys.cw_seed, keys.cw_left, keys.cw_right,
                                         keys.cw_stride, keys.vcw.data(), &kl, &kr, &kv, &desc,
                                         device_out, stream));
  return OkStatus();
}

Status DistributedComparisonFunction::UploadKey(const KeyBatch& batch,
                                                dpf_internal::PackedUploads& up, void* stream,
                                                DeviceKeys* keys) const {
  const int n = parameters_.parameters().log_domain_size();
  const int L = batch.num_levels;
  std::vector<dpf_block> vcw_all;
  std::vector<size_t> vcw_off(n);
  for (int i = 0; i < n; ++i) {
    vcw_off[i] = vcw_all.size();
    vcw_all.insert(vcw_all.end(), batch.value_correction[i].begin(),
                   batch.value_correction[i].end());
  }
  DPF_RETURN_IF_ERROR(up.Reset());
  const size_t o_seed = up.Add(batch.seed.data(), 1);
  const size_t o_party = up.Add(batch.party.data(), 1);
  const size_t o_cws = up.Add(batch.cw_seed.data(), L);
  const size_t o_cwl = up.Add(batch.cw_left.data(), L);
  const size_t o_cwr = up.Add(batch.cw_right.data(), L);
  const size_t o_vcw = up.Add(vcw_all.data(), vcw_all.size());
  DPF_RETURN_IF_ERROR(up.Commit(stream));
  keys->num_keys = 1;
  keys->seed = up.Ptr<dpf_block>(o_seed);
  keys->party = up.Ptr<uint8_t>(o_party);
  keys->cw_seed = up.Ptr<dpf_block>(o_cws);
  keys->cw_left = up.Ptr<uint8_t>(o_cwl);
  keys->cw_right = up.Ptr<uint8_t>(o_cwr);
  keys->cw_stride = L;
  keys->vcw.resize(n);
  for (int i = 0; i < n; ++i) keys->vcw[i] = up.Ptr<dpf_block>(o_vcw) + vcw_off[i];
  return OkStatus();
}

StatusOr<int64_t> DistributedComparisonFunction::EvaluateFullDomainToDevice(
    const DcfKey& key, int64_t shard, int64_t num_shards, void* device_out,
    int64_t capacity_bytes, void* stream) {
  const int n = parameters_.parameters().log_domain_size();
  const DcfKey* kp = &key;
  DPF_ASSIGN_OR_RETURN(KeyBatch batch, MakeKeyBatch(Span<const DcfKey* const>(&kp, 1)));
  DPF_ASSIGN_OR_RETURN(const int k, dpf_internal::ShardLevels(shard, num_shards, n - 1, n, 0));
  const int64_t total = int64_t{1} << (n - k);
  const auto& f = dpf_->flat_value_type(0);
  if (!device_out || capacity_bytes / f.packed_size < total)
    return InvalidArgumentError("device output buffer too small");
  DPF_RETURN_IF_ERROR(CheckFullDomainType());
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  DeviceKeys keys;
  DPF_RETURN_IF_ERROR(UploadKey(batch, s->packed, stream, &keys));
  DPF_RETURN_IF_ERROR(LaunchFullDomain(keys, k, shard, device_out, stream));
  DPF_RETURN_IF_ERROR(s->packed.MarkUsed(stream));
  return total;
}

StatusOr<int64_t> DistributedComparisonFunction::EvaluateFullDomainBatchToDevice(
    const DeviceKeyBatch& keys, int64_t shard, int64_t num_shards, void* device_out,
    int64_t capacity_bytes, void* stream) const {
  const int n = parameters_.parameters().log_domain_size();
  if (keys.num_levels() != dpf_->tree_levels_needed() - 1 || keys.num_hierarchy_levels() != n)
    return InvalidArgumentError("key batch does not match this DistributedComparisonFunction");
  DPF_ASSIGN_OR_RETURN(const int k, dpf_internal::ShardLevels(shard, num_shards, n - 1, n, 0));
  const int64_t row = int64_t{1} << (n - k);
  const auto& f = dpf_->flat_value_type(0);
  if (keys.num_keys() > std::numeric_limits<int64_t>::max() / (row * f.packed_size))
    return InvalidArgumentError("device output buffer too small");
  const int64_t total = keys.num_keys() * row;
  if (total > 0 && (!device_out || capacity_bytes / f.packed_size < total))
    return InvalidArgumentError("device output buffer too small");
  DPF_RETURN_IF_ERROR(CheckFullDomainType());
  if (total == 0) return int64_t{0};
  DeviceKeys d;
  d.num_keys = keys.num_keys();
  d.seed = keys.seed();
  d.party = keys.party();
  d.cw_seed = keys.cw_seed();
  d.cw_left = keys.cw_left();
  d.cw_right = keys.cw_right();
  d.cw_stride = keys.num_levels();
  d.vcw.resize(n);
  for (int i = 0; i < n; ++i) d.vcw[i] = keys.value_correction(i);
  DPF_RETURN_IF_ERROR(LaunchFullDomain(d, k, shard, device_out, stream));
  return total;
}

StatusOr<std::vector<uint8_t>> DistributedComparisonFunction::EvaluateFullDomainPacked(
    const DcfKey& key, const ValueType* requested_type) {
  const int n = parameters_.parameters().log_domain_size();
  if (requested_type) {
    DPF_ASSIGN_OR_RETURN(bool eq, dpf_internal::ValueTypesAreEqual(
                                      *requested_type, parameters_.parameters().value_type()));
    if (!eq) return InvalidArgumentError("Value type T doesn't match parameters at `hierarchy_level`");
  }
  const DcfKey* kp = &key;
  DPF_ASSIGN_OR_RETURN(KeyBatch batch, MakeKeyBatch(Span<const DcfKey* const>(&kp, 1)));
  DPF_RETURN_IF_ERROR(dpf_internal::ShardLevels(0, 1, n - 1, n, 0).status());
  DPF_RETURN_IF_ERROR(CheckFullDomainType());
  const auto& f = dpf_->flat_value_type(0);
  const size_t bytes = (size_t{1} << n) * f.packed_size;
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  void* small = s->small_out.Get(bytes);   // small results: written to page-locked memory
  if (!small) DPF_RETURN_IF_ERROR(s->out.Reserve(bytes));
  void* const dev_out = small ? small : s->out.get();
  DeviceKeys keys;
  DPF_RETURN_IF_ERROR(UploadKey(batch, s->packed, nullptr, &keys));
  DPF_RETURN_IF_ERROR(LaunchFullDomain(keys, 0, 0, dev_out, nullptr));
  DPF_RETURN_IF_ERROR(s->packed.MarkUsed(nullptr));
  std::vector<uint8_t> out(bytes);
  if (small) {
    HIP_RETURN_IF_ERROR(dpf_hip_stream_sync(nullptr));
    std::memcpy(out.data(), small, bytes);
  } else {
    HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(out.data(), s->out.get(), out.size(), nullptr));
  }
  return out;
}

// What a range dot call is once its arguments have passed the host checks.
struct DistributedComparisonFunction::RangeDotCall {
  KeyBatch batch;
  int shard_bits = 0;
  dpf_internal::SlabPlan slab{0, 1, 0};
  int workspace_bytes = 0;
};

Status DistributedComparisonFunction::CheckRangeDot(const DcfKey& key, int64_t shard,
                                                    int64_t num_shards, const void* device_db,
                                                    int64_t db_bytes, int64_t record_words,
                                                    bool has_out, const void* device_out,
                                                    int64_t out_bytes, RangeDotCall* call) const {
  const int n = parameters_.parameters().log_domain_size();
  const DcfKey* kp = &key;
  DPF_ASSIGN_OR_RETURN(call->batch, MakeKeyBatch(Span<const DcfKey* const>(&kp, 1)));
  DPF_ASSIGN_OR_RETURN(call->shard_bits,
                       dpf_internal::ShardLevels(shard, num_shards, n - 1, n, 0));
  if (record_words < 1 || record_words > DPF_HIP_DOT_MAX_RECORD_WORDS)
    return InvalidArgumentError("`record_words` must be in [1, 1024]");
  const int W = static_cast<int>(record_words);
  const int64_t rows = int64_t{1} << (n - call->shard_bits);   // records of this shard
  constexpr int64_t kWord = 8;
  if (rows > std::numeric_limits<int64_t>::max() / (kWord * W) || db_bytes < rows * kWord * W)
    return InvalidArgumentError("database buffer too small");
  if (has_out && out_bytes < kWord * W)
    return InvalidArgumentError("device output buffer too small");
  if (!device_db || (has_out && !device_out))
    return InvalidArgumentError("`device_db` and `device_out` must not be null");
  DPF_RETURN_IF_ERROR(CheckFullDomainType());
  const dpf_value_desc desc = MakeDesc(dpf_->flat_value_type(0), dpf_->blocks_needed(0));
  if (desc.kind[0] != DPF_LEAF_INT || desc.bits[0] != 64)
    return UnimplementedError("EvaluateRangeDot is implemented for uint64_t");
  call->workspace_bytes = dpf_hip_expand_dot_workspace_bytes(&desc, W);
  if (call->workspace_bytes < 0) return UnimplementedError(dpf_hip_last_error());
  // 2^j slabs of the shard, each a sub-shard whose share vector fits the
  // scratch bound; a slab keeps at least two outputs (one last-level node).
  DPF_ASSIGN_OR_RETURN(call->slab, dpf_internal::PlanSlabs(rows, 2, 8 * kWord, DotSlabLogHook()));
  return OkStatus();
}

Status DistributedComparisonFunction::RunRangeDot(const RangeDotCall& call, int64_t shard,
                                                  const void* device_db, int64_t record_words,
                                                  void* device_out, void* stream) {
  constexpr int64_t kWord = 8;
  const int W = static_cast<int>(record_words);
  const dpf_value_desc desc = MakeDesc(dpf_->flat_value_type(0), dpf_->blocks_needed(0));
  const dpf_internal::SlabPlan& slab = call.slab;
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  DeviceKeys keys;
  DPF_RETURN_IF_ERROR(UploadKey(call.batch, s->packed, stream, &keys));
  DPF_RETURN_IF_ERROR(s->workspace_fence.Acquire(s->workspace, call.workspace_bytes, stream));
  DPF_RETURN_IF_ERROR(s->out.Reserve(static_cast<size_t>(slab.slab_rows * kWord)));
  for (int64_t i = 0; i < slab.slabs; ++i) {
    DPF_RETURN_IF_ERROR(LaunchFullDomain(keys, call.shard_bits + slab.j, (shard << slab.j) | i,
                                         s->out.get(), stream));
    HIP_RETURN_IF_ERROR(dpf_hip_dot_rows(
        slab.slab_rows, W, &desc, s->out.get(),
        static_cast<const char*>(device_db) + i * slab.slab_rows * kWord * W, i > 0,
        s->workspace.get(), device_out, stream));
  }
  DPF_RETURN_IF_ERROR(s->workspace_fence.Mark(stream));
  return s->packed.MarkUsed(stream);
}

StatusOr<int64_t> DistributedComparisonFunction::EvaluateRangeDotToDevice(
    const DcfKey& key, int64_t shard, int64_t num_shards, const void* device_db, int64_t db_bytes,
    int64_t record_words, void* device_out, int64_t out_bytes, void* stream) {
  RangeDotCall call;
  DPF_RETURN_IF_ERROR(CheckRangeDot(key, shard, num_shards, device_db, db_bytes, record_words,
                                    true, device_out, out_bytes, &call));
  DPF_RETURN_IF_ERROR(RunRangeDot(call, shard, device_db, record_words, device_out, stream));
  return record_words;
}

StatusOr<std::vector<uint64_t>> DistributedComparisonFunction::EvaluateRangeDot(
    const DcfKey& key, const void* device_db, int64_t db_bytes, int64_t record_words) {
  // Checked before the result buffer is allocated: host errors touch no device.
  RangeDotCall call;
  DPF_RETURN_IF_ERROR(CheckRangeDot(key, 0, 1, device_db, db_bytes, record_words, false, nullptr,
                                    0, &call));
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);
  const size_t bytes = static_cast<size_t>(record_words) * 8;
  DPF_RETURN_IF_ERROR(s->gathered.Reserve(bytes));
  DPF_RETURN_IF_ERROR(RunRangeDot(call, 0, device_db, record_words, s->gathered.get(), nullptr));
  std::vector<uint64_t> result(static_cast<size_t>(record_words));
  HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(result.data(), s->gathered.get(), bytes, nullptr));
  return result;
}

StatusOr<std::vector<uint8_t>> DistributedComparisonFunction::EvaluateByLevels(
    const DcfKey& key, Span<const uint128> xs) {
  // h:83-105 verbatim: one EvaluateAt per level and point.
  const int n = parameters_.parameters().log_domain_size();
  const auto& f = dpf_->flat_value_type(0);
  const int nl = static_cast<int>(f.leaves.size());
  std::vector<uint8_t> out(xs.size() * f.packed_size);
  std::vector<uint128> acc(nl), v(nl);
  for (size_t j = 0; j < xs.size(); ++j) {
    std::fill(acc.begin(), acc.end(), 0);
    const uint128 x = xs[j];
    for (int i = 0; i < n; ++i) {
      const uint128 prefix = n < 128 ? x >> (n - i) : 0;
      DPF_ASSIGN_OR_RETURN(std::vector<uint8_t> e,
                           dpf_->EvaluateAtPacked(key.key(), i, Span<const uint128>(&prefix, 1), nullptr));
      if ((x & (uint128{1} << (n - i - 1))) == 0) {
        dpf_internal::UnpackLeaves(f, e.data(), v.data());
        for (int l = 0; l < nl; ++l) acc[l] = dpf_internal::LeafAdd(f.leaves[l], acc[l], v[l]);
      }
    }
    dpf_internal::PackLeaves(f, acc.data(), out.data() + j * f.packed_size);
  }
  return out;
}

StatusOr<std::vector<uint8_t>> DistributedComparisonFunction::EvaluatePacked(
    const DcfKey& key, Span<const uint128> xs, const ValueType* requested_type) {
  const int n = parameters_.parameters().log_domain_size();
  // The checks of the reference's first EvaluateAt (level 0, point x >> n).
  if (requested_type) {
    DPF_ASSIGN_OR_RETURN(bool eq, dpf_internal::ValueTypesAreEqual(
                                      *requested_type, parameters_.parameters().value_type()));
    if (!eq) return InvalidArgumentError("Value type T doesn't match parameters at `hierarchy_level`");
  }
  for (uint128 x : xs)
    if (n < 128 && (x >> n) != 0)
      return InvalidArgumentError(
          "`evaluation_points[0]` larger than the domain size at hierarchy level 0");
  const DcfKey* kp = &key;
  DPF_ASSIGN_OR_RETURN(KeyBatch batch, MakeKeyBatch(Span<const DcfKey* const>(&kp, 1)));
  if (xs.empty()) return std::vector<uint8_t>{};
  const auto& f = dpf_->flat_value_type(0);
  if (f.leaves.size() > 4) return EvaluateByLevels(key, xs);
  // One key: its arrays and the points go through the reused scratch buffers
  // (staged, no per-call allocation), then one launch and one copy back.
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  const int64_t m = static_cast<int64_t>(xs.size());
  std::vector<dpf_block> pts(m);
  for (int64_t i = 0; i < m; ++i) pts[i] = ToBlock(xs[i]);
  const int L = batch.num_levels;
  std::vector<dpf_block> vcw_all;
  std::vector<size_t> vcw_off(n);
  for (int i = 0; i < n; ++i) {
    vcw_off[i] = vcw_all.size();
    vcw_all.insert(vcw_all.end(), batch.value_correction[i].begin(),
                   batch.value_correction[i].end());
  }
  dpf_internal::PackedUploads& up = s->packed;
  DPF_RETURN_IF_ERROR(up.Reset());
  const size_t o_seed = up.Add(batch.seed.data(), 1);
  const size_t o_party = up.Add(batch.party.data(), 1);
  const size_t o_cws = up.Add(batch.cw_seed.data(), L);
  const size_t o_cwl = up.Add(batch.cw_left.data(), L);
  const size_t o_cwr = up.Add(batch.cw_right.data(), L);
  const size_t o_vcw = up.Add(vcw_all.data(), vcw_all.size());
  const size_t o_pts = up.Add(pts.data(), pts.size());
  DPF_RETURN_IF_ERROR(up.Commit(nullptr));
  const size_t bytes = static_cast<size_t>(m) * f.packed_size;
  void* small = s->small_out.Get(bytes);   // small results: written to page-locked memory
  if (!small) DPF_RETURN_IF_ERROR(s->out.Reserve(bytes));
  void* const dev_out = small ? small : s->out.get();
  std::vector<const dpf_block*> vcw(n);
  for (int i = 0; i < n; ++i) vcw[i] = up.Ptr<dpf_block>(o_vcw) + vcw_off[i];
  DPF_RETURN_IF_ERROR(Launch(1, m, false, up.Ptr<dpf_block>(o_seed), up.Ptr<uint8_t>(o_party),
                             up.Ptr<dpf_block>(o_pts), up.Ptr<dpf_block>(o_cws),
                             up.Ptr<uint8_t>(o_cwl), up.Ptr<uint8_t>(o_cwr), L, vcw,
                             dev_out, nullptr));
  DPF_RETURN_IF_ERROR(up.MarkUsed(nullptr));
  std::vector<uint8_t> out(bytes);
  if (small) {
    HIP_RETURN_IF_ERROR(dpf_hip_stream_sync(nullptr));
    std::memcpy(out.data(), small, bytes);
  } else {
    HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(out.data(), s->out.get(), out.size(), nullptr));
  }
  return out;
}

}  // namespace distributed_point_functions
