// dcf_expand_api_test.cc -- full-domain DCF evaluation through the public
// headers only: EvaluateFullDomain<uint64_t> must equal a loop of
// Evaluate<uint64_t> at log_domain_size 6 for both parties, EvaluateRangeDot's
// two answers must add to beta times the sum of the records below alpha, and
// an IntModN DCF must be reported as UNIMPLEMENTED (no per-point path stands in).
//
// Exit status 0 and "ALL OK" on success; the first mismatch is printed.
// Run by tests/test_dcf_expand_cpp_gpu.py; built by build_native.build_tools.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "dcf/distributed_comparison_function.h"
#include "dpf/int_mod_n.h"
#include "dpf_hip.h"

namespace dpf = distributed_point_functions;
using dpf::DistributedComparisonFunction;
using dpf::uint128;

namespace {

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
std::unique_ptr<DistributedComparisonFunction> MakeDcf(int log) {
  dpf::DcfParameters p;
  p.mutable_parameters()->set_log_domain_size(log);
  *p.mutable_parameters()->mutable_value_type() = dpf::ToValueType<T>();
  return Must(DistributedComparisonFunction::Create(p), "Create");
}

struct DeviceDb {
  void* p = nullptr;
  ~DeviceDb() {
    if (p) dpf_hip_free(p);
  }
};

void FullDomainEqualsEvaluateLoop() {
  constexpr int kLog = 6;
  auto dcf = MakeDcf<uint64_t>(kLog);
  if (!dcf->EvaluatesFullDomainOnDevice()) Fail("uint64_t should evaluate on the device");
  for (uint64_t alpha : {uint64_t{0}, uint64_t{1}, uint64_t{37}, uint64_t{63}}) {
    auto keys = Must(dcf->GenerateKeys(uint128{alpha}, uint64_t{0xC0FFEE1234567ull}), "GenerateKeys");
    std::vector<uint64_t> sum(size_t{1} << kLog, 0);
    for (const dpf::DcfKey* key : {&keys.first, &keys.second}) {
      std::vector<uint64_t> all = Must(dcf->EvaluateFullDomain<uint64_t>(*key), "EvaluateFullDomain");
      if (all.size() != (size_t{1} << kLog)) Fail("EvaluateFullDomain: size");
      for (uint64_t x = 0; x < all.size(); ++x) {
        const uint64_t one = Must(dcf->Evaluate<uint64_t>(*key, uint128{x}), "Evaluate");
        if (all[x] != one)
          Fail("alpha " + std::to_string(alpha) + " x " + std::to_string(x) + ": differs from Evaluate");
        sum[x] += all[x];
      }
    }
    for (uint64_t x = 0; x < sum.size(); ++x)
      if (sum[x] != (x < alpha ? 0xC0FFEE1234567ull : 0)) Fail("shares do not add to the comparison");
  }
  // T is checked as Evaluate<T> checks it.
  auto keys = Must(dcf->GenerateKeys(uint128{5}, uint64_t{1}), "GenerateKeys");
  auto wrong = dcf->EvaluateFullDomain<uint32_t>(keys.first);
  if (wrong.ok() || wrong.status().code() != dpf::StatusCode::kInvalidArgument)
    Fail("EvaluateFullDomain<uint32_t> on a uint64_t DCF accepted");
  std::printf("ok EvaluateFullDomain<uint64_t>\n");
}

void RangeDotReconstructs() {
  constexpr int kLog = 10, kWords = 3;
  auto dcf = MakeDcf<uint64_t>(kLog);
  std::mt19937_64 rng(4711);
  const uint64_t alpha = 613, beta = 0xFEEDFACECAFEBEEFull;
  auto keys = Must(dcf->GenerateKeys(uint128{alpha}, beta), "GenerateKeys");
  const size_t n = size_t{1} << kLog;
  std::vector<uint64_t> db(n * kWords);
  for (uint64_t& w : db) w = rng();
  const int64_t bytes = static_cast<int64_t>(db.size() * sizeof(uint64_t));
  DeviceDb dev;
  if (dpf_hip_alloc(&dev.p, bytes) != 0) Fail("dpf_hip_alloc");
  if (dpf_hip_memcpy_h2d(dev.p, db.data(), bytes, nullptr) != 0) Fail("dpf_hip_memcpy_h2d");
  std::vector<uint64_t> a = Must(dcf->EvaluateRangeDot(keys.first, dev.p, bytes, kWords), "party 0");
  std::vector<uint64_t> b = Must(dcf->EvaluateRangeDot(keys.second, dev.p, bytes, kWords), "party 1");
  if (a.size() != kWords || b.size() != kWords) Fail("EvaluateRangeDot: result size");
  for (int w = 0; w < kWords; ++w) {
    uint64_t want = 0;
    for (uint64_t x = 0; x < alpha; ++x) want += db[x * kWords + w];
    want *= beta;
    if (a[w] + b[w] != want) Fail("word " + std::to_string(w) + " does not reconstruct");
  }
  auto small = dcf->EvaluateRangeDot(keys.first, dev.p, bytes - 1, kWords);
  if (small.ok() || small.status().code() != dpf::StatusCode::kInvalidArgument)
    Fail("short database accepted");
  std::printf("ok EvaluateRangeDot\n");
}

void IntModNIsUnimplemented() {
  using M = dpf::IntModN<uint64_t, 18446744073709551557ull>;
  auto dcf = MakeDcf<M>(6);
  if (dcf->EvaluatesFullDomainOnDevice()) Fail("IntModN reported as supported");
  auto keys = Must(dcf->GenerateKeys(uint128{5}, M(7)), "GenerateKeys IntModN");
  auto r = dcf->EvaluateFullDomain<M>(keys.first);
  if (r.ok()) Fail("IntModN: EvaluateFullDomain succeeded");
  if (r.status().code() != dpf::StatusCode::kUnimplemented) Fail("IntModN: " + r.status().ToString());
  DeviceDb out;
  if (dpf_hip_alloc(&out.p, 8 << 6) != 0) Fail("dpf_hip_alloc");
  auto d = dcf->EvaluateFullDomainToDevice(keys.first, 0, 1, out.p, 8 << 6, nullptr);
  if (d.ok() || d.status().code() != dpf::StatusCode::kUnimplemented)
    Fail("IntModN: EvaluateFullDomainToDevice not UNIMPLEMENTED");
  std::printf("ok IntModN UNIMPLEMENTED\n");
}

}  // namespace

int main() {
  FullDomainEqualsEvaluateLoop();
  RangeDotReconstructs();
  IntModNIsUnimplemented();
  std::printf("ALL OK\n");
  return 0;
}
