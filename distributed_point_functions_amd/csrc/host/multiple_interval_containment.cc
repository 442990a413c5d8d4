// multiple_interval_containment.cc -- MultipleIntervalContainmentGate
// (dcf/fss_gates/multiple_interval_containment.cc:31-275; eprint 2020/1392
// Fig. 14) over the MI355X DCF engine; see the header.
#include "dcf/fss_gates/multiple_interval_containment.h"

#include <sys/random.h>

#include <algorithm>
#include <cstring>

#include "dpf_hip.h"
#include "host_util.h"

namespace distributed_point_functions {
namespace fss_gates {

using dpf_internal::AesKey;
using dpf_internal::FromBlock;
using dpf_internal::FromProtoBlock;
using dpf_internal::kPrgKeyLeft;
using dpf_internal::kPrgKeyRight;
using dpf_internal::kPrgKeyValue;
using dpf_internal::SetProtoBlock;
using dpf_internal::ToBlock;

namespace {

// The bounds are read through value_uint128 whatever the oneof holds, as the
// reference does (cc:53-59).
uint128 Bound(const Value_Integer& v) { return FromProtoBlock(v.value_uint128()); }

// The table image the kernels read: U, p, q' as blocks, then the two index
// tables.
size_t TableBlocks(size_t nu, size_t m) { return nu + 2 * m; }
size_t TableBytes(size_t nu, size_t m) {
  return TableBlocks(nu, m) * sizeof(dpf_block) + 2 * m * sizeof(int32_t);
}

}  // namespace

// ---------------------------------------------------------------- device batch
DeviceMicKeyBatch::~DeviceMicKeyBatch() {
  if (mask_share_) dpf_hip_free(mask_share_);
}

StatusOr<std::unique_ptr<DeviceMicKeyBatch>> DeviceMicKeyBatch::Upload(const MicKeyBatch& batch,
                                                                       void* stream) {
  if (static_cast<int64_t>(batch.mask_share.size()) != batch.dcf.num_keys * batch.num_intervals)
    return InvalidArgumentError("MicKeyBatch holds the wrong number of output mask shares");
  std::unique_ptr<DeviceMicKeyBatch> d(new DeviceMicKeyBatch());
  DPF_ASSIGN_OR_RETURN(d->keys_, DeviceKeyBatch::Upload(batch.dcf, stream));
  d->num_intervals_ = batch.num_intervals;
  const size_t bytes = batch.mask_share.size() * sizeof(dpf_block);
  HIP_RETURN_IF_ERROR(dpf_hip_alloc(&d->mask_share_, std::max<size_t>(bytes, 256)));
  if (bytes)
    HIP_RETURN_IF_ERROR(dpf_hip_memcpy_h2d(d->mask_share_, batch.mask_share.data(), bytes, stream));
  return d;
}

StatusOr<std::unique_ptr<DeviceMicKeyBatch>> DeviceMicKeyBatch::FromKeys(
    std::unique_ptr<DeviceKeyBatch> keys, int num_intervals,
    const std::vector<dpf_block>& mask_share, void* stream) {
  if (!keys || static_cast<int64_t>(mask_share.size()) != keys->num_keys() * num_intervals)
    return InvalidArgumentError("MicKeyBatch holds the wrong number of output mask shares");
  std::unique_ptr<DeviceMicKeyBatch> d(new DeviceMicKeyBatch());
  d->keys_ = std::move(keys);
  d->num_intervals_ = num_intervals;
  const size_t bytes = mask_share.size() * sizeof(dpf_block);
  HIP_RETURN_IF_ERROR(dpf_hip_alloc(&d->mask_share_, std::max<size_t>(bytes, 256)));
  if (bytes)
    HIP_RETURN_IF_ERROR(dpf_hip_memcpy_h2d(d->mask_share_, mask_share.data(), bytes, stream));
  return d;
}

StatusOr<MicKeyBatch> DeviceMicKeyBatch::Download(void* stream) const {
  MicKeyBatch b;
  DPF_ASSIGN_OR_RETURN(b.dcf, keys_->Download(stream));
  b.num_intervals = num_intervals_;
  b.mask_share.resize(static_cast<size_t>(keys_->num_keys()) * num_intervals_);
  if (!b.mask_share.empty())
    HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(b.mask_share.data(), mask_share_,
                                           b.mask_share.size() * sizeof(dpf_block), stream));
  HIP_RETURN_IF_ERROR(dpf_hip_stream_sync(stream));
  return b;
}

// ---------------------------------------------------------------- the gate
MultipleIntervalContainmentGate::MultipleIntervalContainmentGate(
    MicParameters mic_parameters, std::unique_ptr<DistributedComparisonFunction> dcf)
    : mic_parameters_(std::move(mic_parameters)),
      dcf_(std::move(dcf)),
      scratch_(new dpf_internal::DeviceScratch()) {
  const int n = mic_parameters_.log_group_size();
  const uint128 mask = (uint128{1} << n) - 1;
  const int m = mic_parameters_.intervals_size();
  lower_.resize(m);
  upper_next_.resize(m);
  for (int i = 0; i < m; ++i) {
    lower_[i] = Bound(mic_parameters_.intervals(i).lower_bound());
    upper_next_[i] = (Bound(mic_parameters_.intervals(i).upper_bound()) + 1) & mask;
  }
  offsets_ = lower_;
  offsets_.insert(offsets_.end(), upper_next_.begin(), upper_next_.end());
  std::sort(offsets_.begin(), offsets_.end());
  offsets_.erase(std::unique(offsets_.begin(), offsets_.end()), offsets_.end());
  lower_index_.resize(m);
  upper_index_.resize(m);
  for (int i = 0; i < m; ++i) {
    lower_index_[i] = static_cast<int32_t>(
        std::lower_bound(offsets_.begin(), offsets_.end(), lower_[i]) - offsets_.begin());
    upper_index_[i] = static_cast<int32_t>(
        std::lower_bound(offsets_.begin(), offsets_.end(), upper_next_[i]) - offsets_.begin());
  }
}

MultipleIntervalContainmentGate::~MultipleIntervalContainmentGate() = default;

StatusOr<std::unique_ptr<MultipleIntervalContainmentGate>> MultipleIntervalContainmentGate::Create(
    const MicParameters& mic_parameters) {
  // cc:36-79
  const int n = mic_parameters.log_group_size();
  if (n < 0 || n > 127) return InvalidArgumentError("log_group_size should be in > 0 and < 128");
  const uint128 N = uint128{1} << n;
  for (int i = 0; i < mic_parameters.intervals_size(); ++i) {
    const Interval& interval = mic_parameters.intervals(i);
    if (!interval.has_lower_bound() || !interval.has_upper_bound())
      return InvalidArgumentError("Intervals should be non-empty");
    const uint128 p = Bound(interval.lower_bound()), q = Bound(interval.upper_bound());
    if (p >= N || q >= N)
      return InvalidArgumentError("Interval bounds should be between 0 and 2^log_group_size");
    if (p > q) return InvalidArgumentError("Interval upper bounds should be >= lower bound");
  }
  // cc:81-93: a uint128 DCF over the same group.
  DcfParameters dcf_parameters;
  dcf_parameters.mutable_parameters()->set_log_domain_size(n);
  *dcf_parameters.mutable_parameters()->mutable_value_type() = ToValueType<uint128>();
  DPF_ASSIGN_OR_RETURN(std::unique_ptr<DistributedComparisonFunction> dcf,
                       DistributedComparisonFunction::Create(dcf_parameters));
  return std::unique_ptr<MultipleIntervalContainmentGate>(
      new MultipleIntervalContainmentGate(mic_parameters, std::move(dcf)));
}

StatusOr<std::pair<MicKey, MicKey>> MultipleIntervalContainmentGate::Gen(
    uint128 r_in, std::vector<uint128> r_out) {
  return GenImpl(r_in, r_out, nullptr, nullptr);
}

StatusOr<std::pair<MicKey, MicKey>> MultipleIntervalContainmentGate::GenWithSeeds(
    uint128 r_in, std::vector<uint128> r_out, uint128 seed_0, uint128 seed_1,
    Span<const uint128> z_0) {
  if (z_0.size() != r_out.size())
    return InvalidArgumentError("Count of mask shares should be equal to the number of output masks");
  const uint128 seeds[2] = {seed_0, seed_1};
  return GenImpl(r_in, r_out, seeds, z_0.data());
}

uint128 MultipleIntervalContainmentGate::CorrectedOutputMask(int i, uint128 r_in,
                                                             uint128 r_out) const {
  // Fig. 14 Gen, lines 3-5 (Lemma 1, Lemma 2 and Theorem 3 of the paper).
  const uint128 N = uint128{1} << mic_parameters_.log_group_size();
  const uint128 mask = N - 1;
  const uint128 p = lower_[i], q_prime = upper_next_[i];
  const uint128 q = Bound(mic_parameters_.intervals(i).upper_bound());
  const uint128 alpha_p = (p + r_in) & mask, alpha_q = (q + r_in) & mask;
  const uint128 alpha_q_prime = (q + 1 + r_in) & mask;
  uint128 z = r_out;
  if (alpha_p > alpha_q) z += 1;
  if (alpha_p > p) z -= 1;
  if (alpha_q_prime > q_prime) z += 1;
  if (alpha_q == N - 1) z += 1;
  return z & mask;
}

StatusOr<std::pair<MicKey, MicKey>> MultipleIntervalContainmentGate::GenImpl(
    uint128 r_in, const std::vector<uint128>& r_out, const uint128* seeds, const uint128* z_0) {
  // cc:106-126
  const int m = mic_parameters_.intervals_size();
  if (static_cast<int>(r_out.size()) != m)
    return InvalidArgumentError(
        "Count of output masks should be equal to the number of intervals");
  const uint128 N = uint128{1} << mic_parameters_.log_group_size();
  const uint128 mask = N - 1;
  if (r_in >= N) return InvalidArgumentError("Input mask should be between 0 and 2^log_group_size");
  for (uint128 r : r_out)
    if (r >= N) return InvalidArgumentError("Output mask should be between 0 and 2^log_group_size");
  // Fig. 14 Gen, lines 1-2: one DCF key pair for alpha = N-1 + r_in, beta = 1.
  const uint128 gamma = (N - 1 + r_in) & mask;
  std::pair<DcfKey, DcfKey> dcf_keys;
  if (seeds) {
    Value beta;  // ToValue(uint128{1})
    beta.mutable_integer()->mutable_value_uint128()->set_low(1);
    DPF_ASSIGN_OR_RETURN(dcf_keys, dcf_->GenerateKeysWithSeeds(gamma, beta, seeds[0], seeds[1]));
  } else {
    DPF_ASSIGN_OR_RETURN(dcf_keys, dcf_->GenerateKeys(gamma, uint128{1}));
  }
  // Party 0's mask shares: uniformly random (BasicRng in the reference,
  // getrandom(2) here) unless the caller supplies them.
  std::vector<uint128> random(m);
  if (!z_0 && m > 0) {
    auto* bytes = reinterpret_cast<uint8_t*>(random.data());
    size_t want = random.size() * sizeof(uint128), got = 0;
    while (got < want) {
      const ssize_t r = getrandom(bytes + got, want - got, 0);
      if (r <= 0) return InternalError("getrandom failed");
      got += static_cast<size_t>(r);
    }
  }
  std::pair<MicKey, MicKey> keys;
  *keys.first.mutable_dcfkey() = std::move(dcf_keys.first);
  *keys.second.mutable_dcfkey() = std::move(dcf_keys.second);
  for (int i = 0; i < m; ++i) {
    const uint128 z = CorrectedOutputMask(i, r_in, r_out[i]);
    const uint128 share_0 = (z_0 ? z_0[i] : random[i]) & mask;
    const uint128 share_1 = (z - share_0) & mask;
    SetProtoBlock(share_0, keys.first.add_output_mask_share()->mutable_value_uint128());
    SetProtoBlock(share_1, keys.second.add_output_mask_share()->mutable_value_uint128());
  }
  return keys;
}

// ------------------------------------------------------------ batched Gen
Status MultipleIntervalContainmentGate::GenBatchInputs(Span<const uint128> r_in,
                                                       Span<const uint128> r_out,
                                                       Span<const uint128> z_0,
                                                       std::vector<uint128>* gammas,
                                                       std::vector<dpf_block>* share_0,
                                                       std::vector<dpf_block>* share_1) const {
  // GenImpl's checks (cc:106-126), for every gate.
  const int64_t gates = static_cast<int64_t>(r_in.size());
  const int m = mic_parameters_.intervals_size();
  if (static_cast<int64_t>(r_out.size()) != gates * m)
    return InvalidArgumentError(
        "Count of output masks should be equal to the number of intervals");
  if (!z_0.empty() && z_0.size() != r_out.size())
    return InvalidArgumentError("Count of mask shares should be equal to the number of output masks");
  const uint128 N = uint128{1} << mic_parameters_.log_group_size();
  const uint128 mask = N - 1;
  for (uint128 r : r_in)
    if (r >= N) return InvalidArgumentError("Input mask should be between 0 and 2^log_group_size");
  for (uint128 r : r_out)
    if (r >= N) return InvalidArgumentError("Output mask should be between 0 and 2^log_group_size");
  std::vector<uint128> random;
  if (z_0.empty() && !r_out.empty()) {
    random.resize(r_out.size());
    auto* bytes = reinterpret_cast<uint8_t*>(random.data());
    size_t want = random.size() * sizeof(uint128), got = 0;
    while (got < want) {
      const ssize_t r = getrandom(bytes + got, want - got, 0);
      if (r <= 0) return InternalError("getrandom failed");
      got += static_cast<size_t>(r);
    }
  }
  const uint128* z0 = z_0.empty() ? random.data() : z_0.data();
  gammas->resize(gates);
  share_0->resize(r_out.size());
  share_1->resize(r_out.size());
  for (int64_t g = 0; g < gates; ++g) {
    (*gammas)[g] = (N - 1 + r_in[g]) & mask;
    for (int i = 0; i < m; ++i) {
      const uint128 z = CorrectedOutputMask(i, r_in[g], r_out[g * m + i]);
      const uint128 s0 = z0[g * m + i] & mask;
      (*share_0)[g * m + i] = ToBlock(s0);
      (*share_1)[g * m + i] = ToBlock((z - s0) & mask);
    }
  }
  return OkStatus();
}

StatusOr<std::pair<MicKeyBatch, MicKeyBatch>> MultipleIntervalContainmentGate::GenBatch(
    Span<const uint128> r_in, Span<const uint128> r_out, Span<const uint128> root_seeds,
    Span<const uint128> z_0) const {
  std::vector<uint128> gammas;
  std::pair<MicKeyBatch, MicKeyBatch> out;
  DPF_RETURN_IF_ERROR(
      GenBatchInputs(r_in, r_out, z_0, &gammas, &out.first.mask_share, &out.second.mask_share));
  Value beta;  // ToValue(uint128{1})
  beta.mutable_integer()->mutable_value_uint128()->set_low(1);
  std::pair<KeyBatch, KeyBatch> dcf;
  DPF_ASSIGN_OR_RETURN(dcf, dcf_->GenerateKeyBatch(MakeConstSpan(gammas),
                                                   Span<const Value>(&beta, 1), root_seeds));
  out.first.dcf = std::move(dcf.first);
  out.second.dcf = std::move(dcf.second);
  out.first.num_intervals = out.second.num_intervals = mic_parameters_.intervals_size();
  return out;
}

StatusOr<std::pair<std::unique_ptr<DeviceMicKeyBatch>, std::unique_ptr<DeviceMicKeyBatch>>>
MultipleIntervalContainmentGate::GenBatchToDevice(Span<const uint128> r_in,
                                                  Span<const uint128> r_out,
                                                  Span<const uint128> root_seeds,
                                                  Span<const uint128> z_0, void* stream) const {
  std::vector<uint128> gammas;
  std::vector<dpf_block> share_0, share_1;
  DPF_RETURN_IF_ERROR(GenBatchInputs(r_in, r_out, z_0, &gammas, &share_0, &share_1));
  Value beta;  // ToValue(uint128{1})
  beta.mutable_integer()->mutable_value_uint128()->set_low(1);
  DistributedPointFunction::DeviceKeyBatchPair dcf;
  DPF_ASSIGN_OR_RETURN(dcf, dcf_->GenerateKeyBatchToDevice(MakeConstSpan(gammas),
                                                           Span<const Value>(&beta, 1),
                                                           root_seeds, stream));
  const int m = mic_parameters_.intervals_size();
  std::pair<std::unique_ptr<DeviceMicKeyBatch>, std::unique_ptr<DeviceMicKeyBatch>> out;
  DPF_ASSIGN_OR_RETURN(out.first,
                       DeviceMicKeyBatch::FromKeys(std::move(dcf.first), m, share_0, stream));
  DPF_ASSIGN_OR_RETURN(out.second,
                       DeviceMicKeyBatch::FromKeys(std::move(dcf.second), m, share_1, stream));
  return out;
}

StatusOr<MicKeyBatch> MultipleIntervalContainmentGate::MakeKeyBatch(
    Span<const MicKey* const> keys) const {
  const int m = mic_parameters_.intervals_size();
  std::vector<const DcfKey*> dcf_keys;
  dcf_keys.reserve(keys.size());
  for (const MicKey* k : keys) {
    if (k->output_mask_share_size() != m)
      return InvalidArgumentError(
          "Count of output mask shares should be equal to the number of intervals");
    dcf_keys.push_back(&k->dcfkey());
  }
  MicKeyBatch batch;
  DPF_ASSIGN_OR_RETURN(batch.dcf, dcf_->MakeKeyBatch(Span<const DcfKey* const>(dcf_keys)));
  batch.num_intervals = m;
  batch.mask_share.reserve(keys.size() * m);
  for (const MicKey* k : keys)
    for (int i = 0; i < m; ++i)
      batch.mask_share.push_back(ToBlock(Bound(k->output_mask_share(i))));
  return batch;
}

Status MultipleIntervalContainmentGate::Launch(
    int64_t gates, const dpf_block* seed, const uint8_t* party, const dpf_block* cw_seed,
    const uint8_t* cw_left, const uint8_t* cw_right, int cw_stride,
    const std::vector<const dpf_block*>& vcw, const dpf_block* x, const dpf_block* tables,
    const dpf_block* mask_share, dpf_block* walks, void* out, void* stream) const {
  const size_t nu = offsets_.size(), m = lower_.size();
  const dpf_block* lower = tables + nu;
  const dpf_block* upper_next = lower + m;
  const int32_t* lower_index = reinterpret_cast<const int32_t*>(upper_next + m);
  const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight), kv = AesKey(kPrgKeyValue);
  HIP_RETURN_IF_ERROR(dpf_hip_mic_eval_batch(
      gates, mic_parameters_.log_group_size(), seed, party, cw_seed, cw_left, cw_right, cw_stride,
      vcw.data(), x, static_cast<int>(nu), tables, static_cast<int>(m), lower_index,
      lower_index + m, lower, upper_next, mask_share, walks, &kl, &kr, &kv,
      static_cast<dpf_block*>(out), stream));
  return OkStatus();
}

namespace {
// Fills `image` (TableBytes) with the gate's tables.
void FillTables(const std::vector<uint128>& offsets, const std::vector<uint128>& lower,
                const std::vector<uint128>& upper_next, const std::vector<int32_t>& lower_index,
                const std::vector<int32_t>& upper_index, char* image) {
  auto* b = reinterpret_cast<dpf_block*>(image);
  for (uint128 v : offsets) *b++ = ToBlock(v);
  for (uint128 v : lower) *b++ = ToBlock(v);
  for (uint128 v : upper_next) *b++ = ToBlock(v);
  auto* t = reinterpret_cast<int32_t*>(b);
  if (!lower_index.empty()) {
    std::memcpy(t, lower_index.data(), lower_index.size() * sizeof(int32_t));
    std::memcpy(t + lower_index.size(), upper_index.data(), upper_index.size() * sizeof(int32_t));
  }
}
}  // namespace

Status MultipleIntervalContainmentGate::EnsureDeviceTables() {
  if (tables_uploaded_) return OkStatus();
  std::vector<char> image(TableBytes(offsets_.size(), lower_.size()));
  FillTables(offsets_, lower_, upper_next_, lower_index_, upper_index_, image.data());
  DPF_RETURN_IF_ERROR(scratch_->offsets.Upload(image.data(), image.size(), nullptr));
  tables_uploaded_ = true;
  return OkStatus();
}

StatusOr<int64_t> MultipleIntervalContainmentGate::EvalBatchToDevice(
    const DeviceMicKeyBatch& keys, const void* device_x, void* device_out, int64_t capacity_bytes,
    void* stream) {
  const int n = mic_parameters_.log_group_size();
  const int m = mic_parameters_.intervals_size();
  const DeviceKeyBatch& k = keys.keys();
  if (k.num_levels() != dcf_->dpf().tree_levels_needed() - 1 || k.num_hierarchy_levels() != n ||
      keys.num_intervals() != m)
    return InvalidArgumentError("key batch does not match this MultipleIntervalContainmentGate");
  const int64_t gates = k.num_keys();
  const int64_t total = gates * m;
  if (total == 0) return int64_t{0};
  if (!device_out || capacity_bytes < total * static_cast<int64_t>(sizeof(dpf_block)))
    return InvalidArgumentError("device output buffer too small");
  if (!device_x) return InvalidArgumentError("device_x is null");
  // cc:212-215, for device-resident inputs.
  int64_t bad = 0;
  HIP_RETURN_IF_ERROR(dpf_hip_count_out_of_range(gates, static_cast<const dpf_block*>(device_x), n,
                                                 &bad, stream));
  if (bad) return InvalidArgumentError("Masked input should be between 0 and 2^log_group_size");
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  DPF_RETURN_IF_ERROR(EnsureDeviceTables());
  const size_t walk_bytes = static_cast<size_t>(gates) * offsets_.size() * sizeof(dpf_block);
  DPF_RETURN_IF_ERROR(s->workspace_fence.Acquire(s->workspace, walk_bytes, stream));
  std::vector<const dpf_block*> vcw(n);
  for (int i = 0; i < n; ++i) vcw[i] = k.value_correction(i);
  DPF_RETURN_IF_ERROR(Launch(gates, k.seed(), k.party(), k.cw_seed(), k.cw_left(), k.cw_right(),
                             k.num_levels(), vcw, static_cast<const dpf_block*>(device_x),
                             s->offsets.as<dpf_block>(), keys.mask_share(),
                             s->workspace.as<dpf_block>(), device_out, stream));
  DPF_RETURN_IF_ERROR(s->workspace_fence.Mark(stream));
  return total;
}

StatusOr<std::vector<uint128>> MultipleIntervalContainmentGate::EvalBatch(
    Span<const MicKey* const> keys, Span<const uint128> xs) {
  const int n = mic_parameters_.log_group_size();
  const size_t m = lower_.size(), nu = offsets_.size();
  if (keys.size() != xs.size())
    return InvalidArgumentError("Count of masked inputs should be equal to the number of keys");
  const uint128 N = uint128{1} << n;
  for (uint128 x : xs)
    if (x >= N) return InvalidArgumentError("Masked input should be between 0 and 2^log_group_size");
  DPF_ASSIGN_OR_RETURN(MicKeyBatch batch, MakeKeyBatch(keys));
  const int64_t gates = batch.dcf.num_keys;
  std::vector<uint128> result(static_cast<size_t>(gates) * m);
  if (result.empty()) return result;
  // The keys' arrays, the inputs and the gate's tables go through the reused
  // scratch buffers as one staged image, then the two launches and one copy
  // back (DistributedComparisonFunction::EvaluatePacked).
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  const int L = batch.dcf.num_levels;
  std::vector<dpf_block> pts(gates);
  for (int64_t i = 0; i < gates; ++i) pts[i] = ToBlock(xs[i]);
  std::vector<dpf_block> vcw_all;
  std::vector<size_t> vcw_off(n);
  for (int i = 0; i < n; ++i) {
    vcw_off[i] = vcw_all.size();
    vcw_all.insert(vcw_all.end(), batch.dcf.value_correction[i].begin(),
                   batch.dcf.value_correction[i].end());
  }
  std::vector<char> tables(TableBytes(nu, m));
  FillTables(offsets_, lower_, upper_next_, lower_index_, upper_index_, tables.data());
  dpf_internal::PackedUploads& up = s->packed;
  DPF_RETURN_IF_ERROR(up.Reset());
  const size_t o_seed = up.Add(batch.dcf.seed.data(), gates);
  const size_t o_party = up.Add(batch.dcf.party.data(), gates);
  const size_t o_cws = up.Add(batch.dcf.cw_seed.data(), gates * L);
  const size_t o_cwl = up.Add(batch.dcf.cw_left.data(), gates * L);
  const size_t o_cwr = up.Add(batch.dcf.cw_right.data(), gates * L);
  const size_t o_vcw = up.Add(vcw_all.data(), vcw_all.size());
  const size_t o_pts = up.Add(pts.data(), pts.size());
  const size_t o_tab = up.Add(tables.data(), tables.size());
  const size_t o_share = up.Add(batch.mask_share.data(), batch.mask_share.size());
  DPF_RETURN_IF_ERROR(up.Commit(nullptr));
  const size_t walk_bytes = static_cast<size_t>(gates) * nu * sizeof(dpf_block);
  DPF_RETURN_IF_ERROR(s->workspace_fence.Acquire(s->workspace, walk_bytes, nullptr));
  const size_t bytes = result.size() * sizeof(dpf_block);
  void* small = s->small_out.Get(bytes);   // small results: written to page-locked memory
  if (!small) DPF_RETURN_IF_ERROR(s->out.Reserve(bytes));
  void* const dev_out = small ? small : s->out.get();
  std::vector<const dpf_block*> vcw(n);
  for (int i = 0; i < n; ++i) vcw[i] = up.Ptr<dpf_block>(o_vcw) + vcw_off[i];
  DPF_RETURN_IF_ERROR(Launch(gates, up.Ptr<dpf_block>(o_seed), up.Ptr<uint8_t>(o_party),
                             up.Ptr<dpf_block>(o_cws), up.Ptr<uint8_t>(o_cwl),
                             up.Ptr<uint8_t>(o_cwr), L, vcw, up.Ptr<dpf_block>(o_pts),
                             reinterpret_cast<const dpf_block*>(up.Ptr<char>(o_tab)),
                             up.Ptr<dpf_block>(o_share), s->workspace.as<dpf_block>(), dev_out,
                             nullptr));
  DPF_RETURN_IF_ERROR(up.MarkUsed(nullptr));
  DPF_RETURN_IF_ERROR(s->workspace_fence.Mark(nullptr));
  std::vector<dpf_block> raw(result.size());
  if (small) {
    HIP_RETURN_IF_ERROR(dpf_hip_stream_sync(nullptr));
    std::memcpy(raw.data(), small, bytes);
  } else {
    HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(raw.data(), s->out.get(), bytes, nullptr));
  }
  for (size_t i = 0; i < result.size(); ++i) result[i] = FromBlock(raw[i]);
  return result;
}

StatusOr<std::vector<uint128>> MultipleIntervalContainmentGate::Eval(MicKey k, uint128 x) {
  const MicKey* kp = &k;
  return EvalBatch(Span<const MicKey* const>(&kp, 1), Span<const uint128>(&x, 1));
}

}  // namespace fss_gates
}  // namespace distributed_point_functions
