// mic_gate_test.cc -- the reference's MultipleIntervalContainmentGate tests
// (dcf/fss_gates/multiple_interval_containment_test.cc) restated against the
// drop-in C++ class, through the reference's public signatures only (Create,
// Gen, Eval and the message accessors): the two Gen-and-Eval reconstruction
// tests and the Create / Gen / Eval error tests with their messages.
//
// Exit status 0 and "ALL OK" on success; the first mismatch is printed.
// Run by tests/test_mic_cpp_gpu.py; built by build_native.build_tools.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "dcf/fss_gates/multiple_interval_containment.h"

namespace dpf = distributed_point_functions;
using dpf::uint128;
using dpf::fss_gates::Interval;
using dpf::fss_gates::MicKey;
using dpf::fss_gates::MicParameters;
using dpf::fss_gates::MultipleIntervalContainmentGate;

namespace {

int g_checks = 0;

[[noreturn]] void Fail(const std::string& what) {
  std::fprintf(stderr, "FAIL: %s\n", what.c_str());
  std::exit(1);
}

template <typename T>
T Must(dpf::StatusOr<T> s, const std::string& what) {
  if (!s.ok()) Fail(what + ": " + s.status().ToString());
  return std::move(s).value();
}

template <typename T>
void ExpectInvalid(const dpf::StatusOr<T>& s, const std::string& message, const std::string& what) {
  if (s.ok()) Fail(what + ": expected an error");
  if (s.status().code() != dpf::StatusCode::kInvalidArgument || s.status().message() != message)
    Fail(what + ": got " + s.status().ToString());
  ++g_checks;
}

void AddInterval(MicParameters* p, uint128 lo, uint128 hi) {
  Interval* interval = p->add_intervals();
  interval->mutable_lower_bound()->mutable_value_uint128()->set_high(dpf::Uint128High64(lo));
  interval->mutable_lower_bound()->mutable_value_uint128()->set_low(dpf::Uint128Low64(lo));
  interval->mutable_upper_bound()->mutable_value_uint128()->set_high(dpf::Uint128High64(hi));
  interval->mutable_upper_bound()->mutable_value_uint128()->set_low(dpf::Uint128Low64(hi));
}

// test.cc:37-208: shares of every input reconstruct [p_j <= x <= q_j].
void GenAndEval(int log_group_size, const std::vector<uint128>& ps, const std::vector<uint128>& qs,
                const std::vector<uint128>& xs, uint64_t seed) {
  MicParameters mic_parameters;
  mic_parameters.set_log_group_size(log_group_size);
  for (size_t i = 0; i < ps.size(); ++i) AddInterval(&mic_parameters, ps[i], qs[i]);
  std::unique_ptr<MultipleIntervalContainmentGate> gate =
      Must(MultipleIntervalContainmentGate::Create(mic_parameters), "Create");
  const uint128 N = uint128{1} << mic_parameters.log_group_size();
  std::mt19937_64 rng(seed);
  const uint128 r_in = dpf::MakeUint128(rng(), rng()) % N;
  std::vector<uint128> r_outs;
  for (size_t i = 0; i < ps.size(); ++i) r_outs.push_back(dpf::MakeUint128(rng(), rng()) % N);
  MicKey key_0, key_1;
  std::tie(key_0, key_1) = Must(gate->Gen(r_in, r_outs), "Gen");
  for (uint128 x : xs) {
    std::vector<uint128> res_0 = Must(gate->Eval(key_0, (x + r_in) % N), "Eval party 0");
    std::vector<uint128> res_1 = Must(gate->Eval(key_1, (x + r_in) % N), "Eval party 1");
    if (res_0.size() != ps.size() || res_1.size() != ps.size()) Fail("Eval result size");
    for (size_t j = 0; j < ps.size(); ++j) {
      const uint128 result = (res_0[j] + res_1[j] - r_outs[j]) % N;
      const uint128 want = x >= ps[j] && x <= qs[j] ? 1 : 0;
      if (result != want)
        Fail("n = " + std::to_string(log_group_size) + ": input " +
             std::to_string(static_cast<unsigned long long>(x)) + " interval " + std::to_string(j));
      ++g_checks;
    }
  }
}

std::unique_ptr<MultipleIntervalContainmentGate> MakeGate(int log_group_size, uint128 p, uint128 q) {
  MicParameters mic_parameters;
  mic_parameters.set_log_group_size(log_group_size);
  AddInterval(&mic_parameters, p, q);
  return Must(MultipleIntervalContainmentGate::Create(mic_parameters), "Create");
}

void Errors() {
  {  // test.cc:210-236
    MicParameters p;
    p.set_log_group_size(128);
    AddInterval(&p, 10, 45);
    ExpectInvalid(MultipleIntervalContainmentGate::Create(p),
                  "log_group_size should be in > 0 and < 128", "128-bit group");
  }
  {  // :238-265
    MicParameters p;
    p.set_log_group_size(20);
    AddInterval(&p, 4, uint128{1} << 20);
    ExpectInvalid(MultipleIntervalContainmentGate::Create(p),
                  "Interval bounds should be between 0 and 2^log_group_size", "bound outside");
  }
  {  // :267-293
    MicParameters p;
    p.set_log_group_size(20);
    AddInterval(&p, 4, 3);
    ExpectInvalid(MultipleIntervalContainmentGate::Create(p),
                  "Interval upper bounds should be >= lower bound", "p > q");
  }
  {  // :295-318: only the upper bound is set
    MicParameters p;
    p.set_log_group_size(20);
    p.add_intervals()->mutable_upper_bound()->mutable_value_uint128()->set_low(3);
    ExpectInvalid(MultipleIntervalContainmentGate::Create(p), "Intervals should be non-empty",
                  "empty interval");
  }
  {  // :320-374
    MicParameters p;
    p.set_log_group_size(64);
    const uint64_t ps[] = {10, 23, 45, 66, 15}, qs[] = {45, 30, 100, 250, 15};
    for (int i = 0; i < 5; ++i) AddInterval(&p, ps[i], qs[i]);
    auto gate = Must(MultipleIntervalContainmentGate::Create(p), "Create");
    ExpectInvalid(gate->Gen(7, std::vector<uint128>(4, 1)),
                  "Count of output masks should be equal to the number of intervals",
                  "output mask count");
  }
  {  // :376-482
    auto gate = MakeGate(10, 10, 45);
    ExpectInvalid(gate->Gen(2048, {uint128{5}}),
                  "Input mask should be between 0 and 2^log_group_size", "r_in outside");
    ExpectInvalid(gate->Gen(5, {uint128{2048}}),
                  "Output mask should be between 0 and 2^log_group_size", "r_out outside");
  }
  {  // :484-539
    auto gate = MakeGate(64, 10, 45);
    MicKey key_0, key_1;
    std::tie(key_0, key_1) = Must(gate->Gen(99, {uint128{3}}), "Gen");
    ExpectInvalid(gate->Eval(key_0, uint128{1} << 72),
                  "Masked input should be between 0 and 2^log_group_size", "x outside");
  }
}

}  // namespace

int main() {
  {
    std::vector<uint128> xs;
    for (uint64_t i = 0; i < 400; ++i) xs.push_back(i);
    GenAndEval(64, {10, 23, 45, 66, 15}, {45, 30, 100, 250, 15}, xs, 1);
  }
  {
    const uint128 two_power_127 = uint128{1} << 127, two_power_126 = uint128{1} << 126;
    GenAndEval(127, {two_power_126, two_power_127 - 1, two_power_127 - 3},
               {two_power_126 + 3, two_power_127 - 1, two_power_127 - 2},
               {two_power_126 - 1, two_power_126, two_power_126 + 1, two_power_126 + 2,
                two_power_126 + 3, two_power_126 + 4, two_power_127 - 4, two_power_127 - 3,
                two_power_127 - 2, two_power_127 - 1},
               2);
  }
  Errors();
  std::printf("ALL OK (%d checks)\n", g_checks);
  return 0;
}
