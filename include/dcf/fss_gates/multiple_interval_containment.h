// multiple_interval_containment.h -- the reference's
// MultipleIntervalContainmentGate (dcf/fss_gates/multiple_interval_containment
// .h:37-87; eprint 2020/1392 Fig. 14) as a drop-in over the MI355X DCF engine.
//
// A gate over Z_N, N = 2^log_group_size, with m public intervals [p_i, q_i]:
// Gen(r_in, r_out) gives two keys -- one uint128 DCF key for
// alpha = N-1 + r_in, beta = 1, plus m output-mask shares -- and Eval(k, x) on
// the masked input x gives additive shares of r_out_i + [p_i <= x - r_in <= q_i].
// Eval costs two DCF evaluations per interval, at x + N-1 - p_i and
// x + N-1 - q'_i with q'_i = q_i + 1.  The bounds are public and fixed at
// Create, so the gate keeps the sorted set U of distinct p_i and q'_i and
// evaluates the DCF once per element of U (adjacent intervals share
// q'_i = p_{i+1}: a partition of the group needs m walks, not 2m), in the
// gfx950 kernels of dpf_hip_mic_eval_batch.
#ifndef DCF_FSS_GATES_MULTIPLE_INTERVAL_CONTAINMENT_H_
#define DCF_FSS_GATES_MULTIPLE_INTERVAL_CONTAINMENT_H_

#include <memory>
#include <utility>
#include <vector>

#include "dcf/distributed_comparison_function.h"
#include "dcf/fss_gates/multiple_interval_containment.pb.h"
#include "dpf/key_batch.h"

namespace distributed_point_functions {
namespace fss_gates {

// Many MicKeys of one gate as one structure-of-arrays image: the DCF keys'
// KeyBatch plus the output-mask shares, [key][interval].
struct MicKeyBatch {
  KeyBatch dcf;
  int num_intervals = 0;
  std::vector<dpf_block> mask_share;
};

// A MicKeyBatch resident in device memory, uploaded once.
class DeviceMicKeyBatch {
 public:
  static StatusOr<std::unique_ptr<DeviceMicKeyBatch>> Upload(const MicKeyBatch& batch,
                                                             void* stream);
  // A batch around DCF keys already in device memory (GenBatchToDevice):
  // uploads the [key][interval] mask shares on `stream`.
  static StatusOr<std::unique_ptr<DeviceMicKeyBatch>> FromKeys(
      std::unique_ptr<DeviceKeyBatch> keys, int num_intervals,
      const std::vector<dpf_block>& mask_share, void* stream);
  // The inverse of Upload, once the work queued on `stream` has written the batch.
  StatusOr<MicKeyBatch> Download(void* stream) const;
  DeviceMicKeyBatch(const DeviceMicKeyBatch&) = delete;
  DeviceMicKeyBatch& operator=(const DeviceMicKeyBatch&) = delete;
  ~DeviceMicKeyBatch();

  int64_t num_keys() const { return keys_->num_keys(); }
  int num_intervals() const { return num_intervals_; }
  const DeviceKeyBatch& keys() const { return *keys_; }
  const dpf_block* mask_share() const { return static_cast<const dpf_block*>(mask_share_); }

 private:
  DeviceMicKeyBatch() = default;
  std::unique_ptr<DeviceKeyBatch> keys_;
  int num_intervals_ = 0;
  void* mask_share_ = nullptr;
};

class MultipleIntervalContainmentGate {
 public:
  static StatusOr<std::unique_ptr<MultipleIntervalContainmentGate>> Create(
      const MicParameters& mic_parameters);

  MultipleIntervalContainmentGate(const MultipleIntervalContainmentGate&) = delete;
  MultipleIntervalContainmentGate& operator=(const MultipleIntervalContainmentGate&) = delete;
  ~MultipleIntervalContainmentGate();

  // Fig. 14 Gen: r_in masks the input, r_out[i] the i-th output (h:50-68).
  StatusOr<std::pair<MicKey, MicKey>> Gen(uint128 r_in, std::vector<uint128> r_out);

  // Fig. 14 Eval: one share per interval, elements of Z_N (h:70-73).
  StatusOr<std::vector<uint128>> Eval(MicKey k, uint128 x);

  // ---- MI355X extensions ---------------------------------------------------
  // Gen with caller-supplied DCF root seeds and party-0 mask shares z_0 (one
  // per interval, reduced mod N): reproducible keys.
  StatusOr<std::pair<MicKey, MicKey>> GenWithSeeds(uint128 r_in, std::vector<uint128> r_out,
                                                   uint128 seed_0, uint128 seed_1,
                                                   Span<const uint128> z_0);
  // |U|: DCF evaluations per gate (at most twice the number of intervals).
  int num_unique_offsets() const { return static_cast<int>(offsets_.size()); }
  // SoA batch of `keys`; INVALID_ARGUMENT if a key's share count is not the
  // number of intervals.
  StatusOr<MicKeyBatch> MakeKeyBatch(Span<const MicKey* const> keys) const;
  // Eval for every key of a device batch at device_x[key] (dpf_block each,
  // one masked input per gate).  Writes [key][interval] 16-byte little-endian
  // values to device_out and returns their number.
  StatusOr<int64_t> EvalBatchToDevice(const DeviceMicKeyBatch& keys, const void* device_x,
                                      void* device_out, int64_t capacity_bytes, void* stream);
  // The same through host vectors: [key][interval].
  StatusOr<std::vector<uint128>> EvalBatch(Span<const MicKey* const> keys, Span<const uint128> xs);
  // Gen for many gates at once, straight into SoA form: gate g takes r_in[g]
  // and r_out[g*m .. (g+1)*m), m the number of intervals, and is
  // GenWithSeeds(r_in[g], r_out_g, root_seeds[2g], root_seeds[2g+1], z_0_g)
  // passed through MakeKeyBatch.  Empty root_seeds and empty z_0 (else one
  // party-0 share per output mask) are drawn as Gen draws them.
  StatusOr<std::pair<MicKeyBatch, MicKeyBatch>> GenBatch(Span<const uint128> r_in,
                                                         Span<const uint128> r_out,
                                                         Span<const uint128> root_seeds,
                                                         Span<const uint128> z_0) const;
  // The same batches in device memory: the DCF keys through
  // DistributedComparisonFunction::GenerateKeyBatchToDevice on `stream`, the
  // mask shares computed on the host and uploaded.
  StatusOr<std::pair<std::unique_ptr<DeviceMicKeyBatch>, std::unique_ptr<DeviceMicKeyBatch>>>
  GenBatchToDevice(Span<const uint128> r_in, Span<const uint128> r_out,
                   Span<const uint128> root_seeds, Span<const uint128> z_0, void* stream) const;
  const MicParameters& parameters() const { return mic_parameters_; }
  const DistributedComparisonFunction& dcf() const { return *dcf_; }

 private:
  // The i-th output mask with the corrections of Fig. 14 Gen, lines 3-5.
  uint128 CorrectedOutputMask(int i, uint128 r_in, uint128 r_out) const;
  // GenImpl's checks for every gate of a batch, the DCF alphas and both
  // parties' mask shares.
  Status GenBatchInputs(Span<const uint128> r_in, Span<const uint128> r_out,
                        Span<const uint128> z_0, std::vector<uint128>* gammas,
                        std::vector<dpf_block>* share_0, std::vector<dpf_block>* share_1) const;
  MultipleIntervalContainmentGate(MicParameters mic_parameters,
                                  std::unique_ptr<DistributedComparisonFunction> dcf);
  StatusOr<std::pair<MicKey, MicKey>> GenImpl(uint128 r_in, const std::vector<uint128>& r_out,
                                              const uint128* seeds, const uint128* z_0);
  // The offset, index and bound tables in device memory (uploaded at the
  // first device-batch call).
  Status EnsureDeviceTables();
  // Both kernels on device arrays; `walks` holds gates * |U| blocks.
  Status Launch(int64_t gates, const dpf_block* seed, const uint8_t* party,
                const dpf_block* cw_seed, const uint8_t* cw_left, const uint8_t* cw_right,
                int cw_stride, const std::vector<const dpf_block*>& vcw, const dpf_block* x,
                const dpf_block* tables, const dpf_block* mask_share, dpf_block* walks,
                void* out, void* stream) const;

  const MicParameters mic_parameters_;
  const std::unique_ptr<DistributedComparisonFunction> dcf_;
  // Fixed at Create: U sorted ascending, p_i and q'_i, and their positions in U.
  std::vector<uint128> offsets_, lower_, upper_next_;
  std::vector<int32_t> lower_index_, upper_index_;
  // Reused device buffers and staged uploads of the host entry points.
  const std::unique_ptr<dpf_internal::DeviceScratch> scratch_;
  bool tables_uploaded_ = false;
};

}  // namespace fss_gates
}  // namespace distributed_point_functions

#endif  // DCF_FSS_GATES_MULTIPLE_INTERVAL_CONTAINMENT_H_
