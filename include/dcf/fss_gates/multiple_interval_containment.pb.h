// multiple_interval_containment.pb.h -- hand-written proto3 messages of
// dcf/fss_gates/multiple_interval_containment.proto (Interval, MicParameters,
// MicKey), wire compatible with the generated classes:
//   Interval      { Value.Integer lower_bound = 1; Value.Integer upper_bound = 2; }
//   MicParameters { int32 log_group_size = 1; repeated Interval intervals = 2; }
//   MicKey        { DcfKey dcfkey = 1; repeated Value.Integer output_mask_share = 2; }
// Presence of an Interval's bounds is tracked (Create tests it).
#ifndef DCF_FSS_GATES_MULTIPLE_INTERVAL_CONTAINMENT_PB_H_
#define DCF_FSS_GATES_MULTIPLE_INTERVAL_CONTAINMENT_PB_H_

#include "dcf/distributed_comparison_function.pb.h"
#include "dpf/distributed_point_function.pb.h"

namespace distributed_point_functions {
namespace fss_gates {

class Interval {
 public:
  bool has_lower_bound() const { return has_lower_; }
  const Value_Integer& lower_bound() const { return lower_; }
  Value_Integer* mutable_lower_bound() { has_lower_ = true; return &lower_; }
  void clear_lower_bound() { has_lower_ = false; lower_ = Value_Integer(); }
  bool has_upper_bound() const { return has_upper_; }
  const Value_Integer& upper_bound() const { return upper_; }
  Value_Integer* mutable_upper_bound() { has_upper_ = true; return &upper_; }
  void clear_upper_bound() { has_upper_ = false; upper_ = Value_Integer(); }
  DPF_PROTO_MESSAGE_API(Interval)

 private:
  bool has_lower_ = false, has_upper_ = false;
  Value_Integer lower_, upper_;
};

class MicParameters {
 public:
  int32_t log_group_size() const { return log_group_size_; }
  void set_log_group_size(int32_t v) { log_group_size_ = v; }
  int intervals_size() const { return intervals_.size(); }
  const Interval& intervals(int i) const { return intervals_[i]; }
  Interval* mutable_intervals(int i) { return intervals_.Mutable(i); }
  Interval* add_intervals() { return intervals_.Add(); }
  const RepeatedField<Interval>& intervals() const { return intervals_; }
  RepeatedField<Interval>* mutable_intervals() { return &intervals_; }
  DPF_PROTO_MESSAGE_API(MicParameters)

 private:
  int32_t log_group_size_ = 0;
  RepeatedField<Interval> intervals_;
};

class MicKey {
 public:
  bool has_dcfkey() const { return has_dcfkey_; }
  const DcfKey& dcfkey() const { return dcfkey_; }
  DcfKey* mutable_dcfkey() { has_dcfkey_ = true; return &dcfkey_; }
  int output_mask_share_size() const { return shares_.size(); }
  const Value_Integer& output_mask_share(int i) const { return shares_[i]; }
  Value_Integer* mutable_output_mask_share(int i) { return shares_.Mutable(i); }
  Value_Integer* add_output_mask_share() { return shares_.Add(); }
  const RepeatedField<Value_Integer>& output_mask_share() const { return shares_; }
  RepeatedField<Value_Integer>* mutable_output_mask_share() { return &shares_; }
  DPF_PROTO_MESSAGE_API(MicKey)

 private:
  bool has_dcfkey_ = false;
  DcfKey dcfkey_;
  RepeatedField<Value_Integer> shares_;
};

}  // namespace fss_gates
}  // namespace distributed_point_functions

#endif  // DCF_FSS_GATES_MULTIPLE_INTERVAL_CONTAINMENT_PB_H_
