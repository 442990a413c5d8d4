// full_domain_sum_api_test.cc -- the fused full-domain sum over a key batch
// through the public headers only: EvaluateFullDomainSum and
// EvaluateFullDomainSumToDevice must equal the per-key EvaluateUntil<T> vectors
// summed on the host, for uint64_t and XorWrapper<uint64_t> and both parties,
// whose vectors must reconstruct the histogram; `accumulate` adds into what the
// output holds; uint32_t is UNIMPLEMENTED and a batch of another DPF is refused.
//
// Exit status 0 and "ALL OK" on success; the first mismatch is printed.
// Run by tests/test_full_domain_sum_cpp_gpu.py; built by build_native.build_tools.
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
std::unique_ptr<DistributedPointFunction> MakeDpf(int log) {
  dpf::DpfParameters p;
  p.set_log_domain_size(log);
  *p.mutable_value_type() = dpf::ToValueType<T>();
  return Must(DistributedPointFunction::Create(p), "Create");
}

struct DeviceMem {
  void* p = nullptr;
  ~DeviceMem() {
    if (p) dpf_hip_free(p);
  }
};

uint64_t Word(uint64_t v) { return v; }
uint64_t Word(const dpf::XorWrapper<uint64_t>& v) { return v.value(); }

template <typename T, bool kXor>
void SumEqualsEvaluateUntil(const char* name) {
  constexpr int kLog = 9, kKeys = 70;
  constexpr uint64_t kN = uint64_t{1} << kLog;
  auto d = MakeDpf<T>(kLog);
  if (!d->EvaluatesFullDomainSumOnDevice(0)) Fail(std::string(name) + " should sum on the device");
  if (d->EvaluatesFullDomainSumOnDevice(1)) Fail("a level that does not exist reported as supported");
  std::mt19937_64 rng(31);
  std::vector<uint128> alphas;
  std::vector<dpf::Value> betas;
  std::vector<uint64_t> beta_words;
  for (int k = 0; k < kKeys; ++k) {
    alphas.push_back(uint128{k == 0 ? 0 : (k == 1 ? kN - 1 : (k < 6 ? 17 : rng() % kN))});
    beta_words.push_back(rng() | 1);
    betas.push_back(Must(d->template ToValue<T>(T(beta_words.back())), "beta"));
  }
  auto host = Must(d->GenerateKeyBatchWithBetas(dpf::MakeConstSpan(alphas), dpf::MakeConstSpan(betas),
                                                dpf::Span<const uint128>()),
                   "GenerateKeyBatchWithBetas");
  const dpf::KeyBatch* batches[2] = {&host.first, &host.second};
  std::vector<uint64_t> share[2];
  for (int party = 0; party < 2; ++party) {
    auto keys = Must(dpf::DeviceKeyBatch::Upload(*batches[party], nullptr), "Upload");
    share[party] = Must(d->EvaluateFullDomainSum(*keys, 0), "EvaluateFullDomainSum");
    if (share[party].size() != kN) Fail("result size");
    std::vector<uint64_t> want(kN, 0);
    for (int k = 0; k < kKeys; ++k) {
      auto ctx = Must(d->CreateEvaluationContext(Must(d->KeyFromBatch(*batches[party], k), "key")),
                      "CreateEvaluationContext");
      std::vector<T> y = Must(d->template EvaluateUntil<T>(0, {}, ctx), "EvaluateUntil");
      if (y.size() != kN) Fail("EvaluateUntil: size");
      for (uint64_t i = 0; i < kN; ++i) {
        if (kXor) want[i] ^= Word(y[i]);
        else want[i] += Word(y[i]);
      }
    }
    if (share[party] != want)
      Fail(std::string(name) + " party " + std::to_string(party) + ": differs from the host sum");

    // ToDevice: over a prefilled buffer, then accumulated on top of itself.
    DeviceMem out;
    const int64_t bytes = static_cast<int64_t>(kN * 8);
    if (dpf_hip_alloc(&out.p, bytes) != 0) Fail("dpf_hip_alloc");
    if (dpf_hip_memset(out.p, 0xAB, bytes, nullptr) != 0) Fail("dpf_hip_memset");
    std::vector<uint64_t> got(kN);
    if (Must(d->EvaluateFullDomainSumToDevice(*keys, 0, out.p, bytes, false, nullptr), "ToDevice") !=
        static_cast<int64_t>(kN))
      Fail("ToDevice: return value");
    if (dpf_hip_memcpy_d2h(got.data(), out.p, bytes, nullptr) != 0) Fail("dpf_hip_memcpy_d2h");
    if (got != want) Fail(std::string(name) + ": ToDevice over a prefilled buffer differs");
    Must(d->EvaluateFullDomainSumToDevice(*keys, 0, out.p, bytes, true, nullptr), "accumulate");
    if (dpf_hip_memcpy_d2h(got.data(), out.p, bytes, nullptr) != 0) Fail("dpf_hip_memcpy_d2h");
    for (uint64_t i = 0; i < kN; ++i)
      if (got[i] != (kXor ? uint64_t{0} : 2 * want[i]))
        Fail(std::string(name) + ": accumulate at " + std::to_string(i));
  }
  std::vector<uint64_t> hist(kN, 0);
  for (int k = 0; k < kKeys; ++k) {
    uint64_t& h = hist[static_cast<uint64_t>(alphas[k])];
    h = kXor ? h ^ beta_words[k] : h + beta_words[k];
  }
  for (uint64_t i = 0; i < kN; ++i)
    if ((kXor ? share[0][i] ^ share[1][i] : share[0][i] + share[1][i]) != hist[i])
      Fail(std::string(name) + ": shares do not reconstruct at " + std::to_string(i));
  std::printf("ok EvaluateFullDomainSum<%s>\n", name);
}

void ErrorCodes() {
  constexpr int kLog = 5;
  auto d = MakeDpf<uint64_t>(kLog);
  std::vector<uint128> alphas = {uint128{3}, uint128{17}};
  std::vector<dpf::Value> beta = {Must(d->ToValue<uint64_t>(5), "beta")};
  auto host = Must(d->GenerateKeyBatch(dpf::MakeConstSpan(alphas), dpf::MakeConstSpan(beta),
                                       dpf::Span<const uint128>()),
                   "GenerateKeyBatch");
  auto keys = Must(dpf::DeviceKeyBatch::Upload(host.first, nullptr), "Upload");
  const int64_t bytes = (int64_t{1} << kLog) * 8;
  DeviceMem out;
  if (dpf_hip_alloc(&out.p, 2 * bytes) != 0) Fail("dpf_hip_alloc");
  auto expect = [&](const dpf::Status& st, dpf::StatusCode code, const char* what) {
    if (st.ok() || st.code() != code) Fail(std::string(what) + ": " + st.ToString());
  };
  using dpf::StatusCode;
  expect(d->EvaluateFullDomainSumToDevice(*keys, 1, out.p, bytes, false, nullptr).status(),
         StatusCode::kInvalidArgument, "level");
  expect(d->EvaluateFullDomainSumToDevice(*keys, 0, nullptr, bytes, false, nullptr).status(),
         StatusCode::kInvalidArgument, "null output");
  expect(d->EvaluateFullDomainSumToDevice(*keys, 0, out.p, bytes - 8, false, nullptr).status(),
         StatusCode::kInvalidArgument, "out_bytes");
  expect(d->EvaluateFullDomainSumToDevice(*keys, 0, static_cast<char*>(out.p) + 8, bytes, false,
                                          nullptr)
             .status(),
         StatusCode::kInvalidArgument, "alignment");
  // A batch of another DistributedPointFunction.
  auto other = MakeDpf<uint64_t>(kLog + 1);
  expect(other->EvaluateFullDomainSumToDevice(*keys, 0, out.p, 2 * bytes, false, nullptr).status(),
         StatusCode::kInvalidArgument, "foreign batch");
  expect(other->EvaluateFullDomainSum(*keys, 0).status(), StatusCode::kInvalidArgument,
         "foreign batch, host result");
  // No fallback behind the call.
  auto u32 = MakeDpf<uint32_t>(kLog);
  if (u32->EvaluatesFullDomainSumOnDevice(0)) Fail("uint32_t reported as supported");
  expect(u32->EvaluateFullDomainSumToDevice(*keys, 0, out.p, bytes, false, nullptr).status(),
         StatusCode::kUnimplemented, "uint32_t");
  expect(u32->EvaluateFullDomainSum(*keys, 0).status(), StatusCode::kUnimplemented,
         "uint32_t, host result");
  std::printf("ok error codes\n");
}

}  // namespace

int main() {
  SumEqualsEvaluateUntil<uint64_t, false>("uint64_t");
  SumEqualsEvaluateUntil<dpf::XorWrapper<uint64_t>, true>("XorWrapper<uint64_t>");
  ErrorCodes();
  std::printf("ALL OK\n");
  return 0;
}
