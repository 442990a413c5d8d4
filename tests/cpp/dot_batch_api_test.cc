// dot_batch_api_test.cc -- EvaluateDotBatch (additive-share two-server PIR:
// one output word weighs one record, several keys against one pass over the
// database) through the public headers only.  For uint64_t at log_domain_size
// 12 (2^12 records of 5 words) and three keys per party, every answer must
// equal EvaluateUntil<uint64_t> folded into the database on the host (sums
// mod 2^64), the two parties' answers must add to beta * db[alpha], and an
// empty key list and a short database must be refused.
//
// Exit status 0 and "ALL OK" on success; the first mismatch is printed.
// Run by tests/test_dot_batch_cpp_gpu.py; built by build_native.build_tools.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "dpf/distributed_point_function.h"
#include "dpf_hip.h"

namespace dpf = distributed_point_functions;
using dpf::DistributedPointFunction;
using dpf::DpfKey;
using dpf::DpfParameters;
using dpf::uint128;
using T = uint64_t;

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

constexpr int kLog = 12, kWords = 5, kKeys = 3;
constexpr size_t kRecords = size_t{1} << kLog;

struct DeviceDb {
  void* p = nullptr;
  ~DeviceDb() {
    if (p) dpf_hip_free(p);
  }
};

// sum_i y[i] * db[i][w] mod 2^64.
std::vector<uint64_t> HostFold(const std::vector<T>& y, const std::vector<uint64_t>& db) {
  std::vector<uint64_t> out(kWords, 0);
  for (size_t i = 0; i < y.size(); ++i)
    for (int w = 0; w < kWords; ++w) out[w] += y[i] * db[i * kWords + w];
  return out;
}

}  // namespace

int main() {
  DpfParameters p;
  p.set_log_domain_size(kLog);
  *p.mutable_value_type() = dpf::ToValueType<T>();
  auto f = Must(DistributedPointFunction::Create(p), "Create");
  std::mt19937_64 rng(20240611);
  std::vector<uint64_t> db(kRecords * kWords);
  for (uint64_t& w : db) w = rng();
  const int64_t bytes = static_cast<int64_t>(db.size() * 8);
  DeviceDb dev;
  if (dpf_hip_alloc(&dev.p, bytes) != 0) Fail("dpf_hip_alloc");
  if (dpf_hip_memcpy_h2d(dev.p, db.data(), bytes, nullptr) != 0) Fail("dpf_hip_memcpy_h2d");

  // Full-width betas: the cross terms of the 64-bit product count.
  const uint64_t alpha[kKeys] = {37, 4095, 0};
  const uint64_t beta[kKeys] = {1, 0xFEDCBA9876543211ull, 0xFFFFFFFFFFFFFFFFull};
  std::vector<DpfKey> party[2];
  for (int q = 0; q < kKeys; ++q) {
    auto keys = Must(f->GenerateKeys(uint128{alpha[q]}, T(beta[q])), "GenerateKeys");
    party[0].push_back(keys.first);
    party[1].push_back(keys.second);
  }
  std::vector<uint64_t> got[2];
  for (int s = 0; s < 2; ++s) {
    const std::vector<const DpfKey*> ptrs = {&party[s][0], &party[s][1], &party[s][2]};
    got[s] = Must(f->EvaluateDotBatch(dpf::MakeConstSpan(ptrs), 0, dev.p, bytes, kWords),
                  "EvaluateDotBatch party " + std::to_string(s));
    if (got[s].size() != size_t{kKeys} * kWords) Fail("result size");
    for (int q = 0; q < kKeys; ++q) {
      auto ctx = Must(f->CreateEvaluationContext(party[s][q]), "CreateEvaluationContext");
      const std::vector<T> y = Must(f->EvaluateUntil<T>(0, {}, ctx), "EvaluateUntil");
      if (y.size() != kRecords) Fail("EvaluateUntil size");
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
      const uint64_t want = beta[q] * db[alpha[q] * kWords + w];
      if (got[0][q * kWords + w] + got[1][q * kWords + w] != want)
        Fail("key " + std::to_string(q) + " word " + std::to_string(w) + " does not recombine");
    }
  std::printf("ok the parties' answers recombine to beta * db[alpha]\n");

  const std::vector<const DpfKey*> ptrs = {&party[0][0], &party[0][1], &party[0][2]};
  auto small = f->EvaluateDotBatch(dpf::MakeConstSpan(ptrs), 0, dev.p, bytes - 1, kWords);
  if (small.ok() || small.status().code() != dpf::StatusCode::kInvalidArgument)
    Fail("short database accepted");
  auto none = f->EvaluateDotBatch(dpf::Span<const DpfKey* const>(), 0, dev.p, bytes, kWords);
  if (none.ok() || none.status().code() != dpf::StatusCode::kInvalidArgument)
    Fail("empty key list accepted");
  std::printf("ok errors\n");
  std::printf("ALL OK\n");
  return 0;
}
