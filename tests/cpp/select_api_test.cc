// select_api_test.cc -- EvaluateSelect (dense two-server PIR: one output bit
// selects one record, several keys against one pass over the database)
// through the public headers only.  For XorWrapper<absl::uint128> at
// log_domain_size 6 (2^13 records of 3 words) and two keys per party, every
// answer must equal EvaluateUntil<T>'s bits folded into the database on the
// host, the two parties' answers must XOR to the records the betas' bits
// name, and an empty key list and a short database must be refused.
//
// Exit status 0 and "ALL OK" on success; the first mismatch is printed.
// Run by tests/test_select_cpp_gpu.py; built by build_native.build_tools.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "dpf/distributed_point_function.h"
#include "dpf/xor_wrapper.h"
#include "dpf_hip.h"

namespace dpf = distributed_point_functions;
using dpf::DistributedPointFunction;
using dpf::DpfKey;
using dpf::DpfParameters;
using dpf::uint128;
using T = dpf::XorWrapper<uint128>;

namespace {

[[noreturn]] void Fail(const std::string& what) {
  std::fprintf(stderr, "FAIL: %s\n", what.c_str());
  std::exit(1);
}

template <typename V>
V Must(dpf::StatusOr<V> s, const std::string& what) {
  if (!s.ok()) Fail(what + ": " + s.status().ToString());
  return std::move(s).value();
}

constexpr int kLog = 6, kWords = 3, kKeys = 2;
constexpr size_t kRecords = (size_t{1} << kLog) * 128;

struct DeviceDb {
  void* p = nullptr;
  ~DeviceDb() {
    if (p) dpf_hip_free(p);
  }
};

// XOR of the records whose bit is set in the share vector y (bit b of element
// i is record i * 128 + b).
std::vector<uint64_t> HostFold(const std::vector<T>& y, const std::vector<uint64_t>& db) {
  std::vector<uint64_t> out(kWords, 0);
  for (size_t i = 0; i < y.size(); ++i)
    for (int b = 0; b < 128; ++b)
      if (static_cast<uint64_t>(y[i].value() >> b) & 1)
        for (int w = 0; w < kWords; ++w) out[w] ^= db[(i * 128 + b) * kWords + w];
  return out;
}

}  // namespace

int main() {
  DpfParameters p;
  p.set_log_domain_size(kLog);
  *p.mutable_value_type() = dpf::ToValueType<T>();
  auto f = Must(DistributedPointFunction::Create(p), "Create");
  std::mt19937_64 rng(20240607);
  std::vector<uint64_t> db(kRecords * kWords);
  for (uint64_t& w : db) w = rng();
  const int64_t bytes = static_cast<int64_t>(db.size() * 8);
  DeviceDb dev;
  if (dpf_hip_alloc(&dev.p, bytes) != 0) Fail("dpf_hip_alloc");
  if (dpf_hip_memcpy_h2d(dev.p, db.data(), bytes, nullptr) != 0) Fail("dpf_hip_memcpy_h2d");

  // Key 0 asks for one record, key 1 for two records of another block.
  const uint128 alpha[kKeys] = {uint128{37}, uint128{5}};
  const uint128 beta[kKeys] = {uint128{1} << 77, (uint128{1} << 3) | (uint128{1} << 127)};
  std::vector<DpfKey> party[2];
  for (int q = 0; q < kKeys; ++q) {
    auto keys = Must(f->GenerateKeys(alpha[q], T(beta[q])), "GenerateKeys");
    party[0].push_back(keys.first);
    party[1].push_back(keys.second);
  }
  std::vector<uint64_t> got[2];
  for (int s = 0; s < 2; ++s) {
    const std::vector<const DpfKey*> ptrs = {&party[s][0], &party[s][1]};
    got[s] = Must(f->EvaluateSelect(dpf::MakeConstSpan(ptrs), 0, dev.p, bytes, kWords),
                  "EvaluateSelect party " + std::to_string(s));
    if (got[s].size() != size_t{kKeys} * kWords) Fail("result size");
    for (int q = 0; q < kKeys; ++q) {
      auto ctx = Must(f->CreateEvaluationContext(party[s][q]), "CreateEvaluationContext");
      const std::vector<T> y = Must(f->EvaluateUntil<T>(0, {}, ctx), "EvaluateUntil");
      if (y.size() != size_t{1} << kLog) Fail("EvaluateUntil size");
      const std::vector<uint64_t> want = HostFold(y, db);
      for (int w = 0; w < kWords; ++w)
        if (got[s][q * kWords + w] != want[w])
          Fail("party " + std::to_string(s) + " key " + std::to_string(q) + " word " +
               std::to_string(w) + " differs from the host fold");
    }
  }
  std::printf("ok both parties equal the host fold\n");
  for (int q = 0; q < kKeys; ++q)
    for (int w = 0; w < kWords; ++w) {
      uint64_t want = 0;
      for (int b = 0; b < 128; ++b)
        if (static_cast<uint64_t>(beta[q] >> b) & 1)
          want ^= db[(static_cast<size_t>(alpha[q]) * 128 + b) * kWords + w];
      if ((got[0][q * kWords + w] ^ got[1][q * kWords + w]) != want)
        Fail("key " + std::to_string(q) + " word " + std::to_string(w) + " does not recombine");
    }
  std::printf("ok the parties' answers recombine to the selected records\n");

  const std::vector<const DpfKey*> ptrs = {&party[0][0], &party[0][1]};
  auto small = f->EvaluateSelect(dpf::MakeConstSpan(ptrs), 0, dev.p, bytes - 1, kWords);
  if (small.ok() || small.status().code() != dpf::StatusCode::kInvalidArgument)
    Fail("short database accepted");
  auto none = f->EvaluateSelect(dpf::Span<const DpfKey* const>(), 0, dev.p, bytes, kWords);
  if (none.ok() || none.status().code() != dpf::StatusCode::kInvalidArgument)
    Fail("empty key list accepted");
  std::printf("ok errors\n");
  std::printf("ALL OK\n");
  return 0;
}
