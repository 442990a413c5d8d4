// full_domain_sum_packed_api_test.cc -- the packed full-domain sum through the
// public headers only: EvaluateFullDomainSumPacked<T> must equal the per-key
// EvaluateUntil<T> vectors summed on the host for uint32_t, uint8_t and
// XorWrapper<uint128> and both parties, whose vectors must reconstruct the
// histogram; a wrong T, an unsupported type or shape and a batch of another
// DPF are refused with their status codes.
//
// Exit status 0 and "ALL OK" on success; the first mismatch is printed.
// Run by tests/test_full_domain_sum_packed_cpp_gpu.py; built by
// build_native.build_tools.
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

// The group of T on its raw integer.
template <typename U>
struct Add {
  using Raw = U;
  static U Of(U v) { return v; }
  static U Op(U a, U b) { return static_cast<U>(a + b); }
};
template <typename U>
struct Xor {
  using Raw = U;
  static U Of(const dpf::XorWrapper<U>& v) { return v.value(); }
  static U Op(U a, U b) { return a ^ b; }
};

template <typename T, typename G>
void SumEqualsEvaluateUntil(const char* name, int log) {
  using Raw = typename G::Raw;
  constexpr int kKeys = 70;
  const uint64_t n_elems = uint64_t{1} << log;
  auto d = MakeDpf<T>(log);
  if (!d->EvaluatesFullDomainSumPackedOnDevice(0))
    Fail(std::string(name) + " should sum on the device");
  if (d->EvaluatesFullDomainSumPackedOnDevice(1))
    Fail("a level that does not exist reported as supported");
  std::mt19937_64 rng(31);
  std::vector<uint128> alphas;
  std::vector<dpf::Value> betas;
  std::vector<Raw> beta_raw;
  for (int k = 0; k < kKeys; ++k) {
    alphas.push_back(
        uint128{k == 0 ? 0 : (k == 1 ? n_elems - 1 : (k < 6 ? 17 : rng() % n_elems))});
    // Odd, and all ones for two keys of one bin: the bin's sum wraps.
    Raw b = static_cast<Raw>((static_cast<Raw>(rng()) << (sizeof(Raw) > 8 ? 64 : 0)) | rng() | 1);
    if (k == 2 || k == 3) b = static_cast<Raw>(~Raw{0});
    beta_raw.push_back(b);
    betas.push_back(Must(d->template ToValue<T>(T(b)), "beta"));
  }
  auto host = Must(d->GenerateKeyBatchWithBetas(dpf::MakeConstSpan(alphas), dpf::MakeConstSpan(betas),
                                                dpf::Span<const uint128>()),
                   "GenerateKeyBatchWithBetas");
  const dpf::KeyBatch* batches[2] = {&host.first, &host.second};
  std::vector<Raw> share[2];
  for (int party = 0; party < 2; ++party) {
    auto keys = Must(dpf::DeviceKeyBatch::Upload(*batches[party], nullptr), "Upload");
    std::vector<T> got =
        Must(d->template EvaluateFullDomainSumPacked<T>(*keys, 0), "EvaluateFullDomainSumPacked");
    if (got.size() != n_elems) Fail("result size");
    std::vector<Raw> want(n_elems, Raw{0});
    for (int k = 0; k < kKeys; ++k) {
      auto ctx = Must(d->CreateEvaluationContext(Must(d->KeyFromBatch(*batches[party], k), "key")),
                      "CreateEvaluationContext");
      std::vector<T> y = Must(d->template EvaluateUntil<T>(0, {}, ctx), "EvaluateUntil");
      if (y.size() != n_elems) Fail("EvaluateUntil: size");
      for (uint64_t i = 0; i < n_elems; ++i) want[i] = G::Op(want[i], G::Of(y[i]));
    }
    for (uint64_t i = 0; i < n_elems; ++i) {
      share[party].push_back(G::Of(got[i]));
      if (share[party][i] != want[i])
        Fail(std::string(name) + " party " + std::to_string(party) +
             ": differs from the host sum at " + std::to_string(i));
    }
    // ToDevice over a prefilled buffer gives the same packed bytes.
    DeviceMem out;
    const int64_t bytes = static_cast<int64_t>(n_elems * sizeof(Raw));
    if (dpf_hip_alloc(&out.p, bytes) != 0) Fail("dpf_hip_alloc");
    if (dpf_hip_memset(out.p, 0xAB, bytes, nullptr) != 0) Fail("dpf_hip_memset");
    if (Must(d->EvaluateFullDomainSumPackedToDevice(*keys, 0, out.p, bytes, false, nullptr),
             "ToDevice") != static_cast<int64_t>(n_elems))
      Fail("ToDevice: return value");
    std::vector<Raw> dev(n_elems);
    if (dpf_hip_memcpy_d2h(dev.data(), out.p, bytes, nullptr) != 0) Fail("dpf_hip_memcpy_d2h");
    if (dev != want) Fail(std::string(name) + ": ToDevice over a prefilled buffer differs");
  }
  std::vector<Raw> hist(n_elems, Raw{0});
  for (int k = 0; k < kKeys; ++k) {
    Raw& h = hist[static_cast<uint64_t>(alphas[k])];
    h = G::Op(h, beta_raw[k]);
  }
  for (uint64_t i = 0; i < n_elems; ++i)
    if (G::Op(share[0][i], share[1][i]) != hist[i])
      Fail(std::string(name) + ": shares do not reconstruct at " + std::to_string(i));
  std::printf("ok EvaluateFullDomainSumPacked<%s>\n", name);
}

void ErrorCodes() {
  constexpr int kLog = 6;
  auto d = MakeDpf<uint32_t>(kLog);
  std::vector<uint128> alphas = {uint128{3}, uint128{17}};
  std::vector<dpf::Value> beta = {Must(d->ToValue<uint32_t>(5), "beta")};
  auto host = Must(d->GenerateKeyBatch(dpf::MakeConstSpan(alphas), dpf::MakeConstSpan(beta),
                                       dpf::Span<const uint128>()),
                   "GenerateKeyBatch");
  auto keys = Must(dpf::DeviceKeyBatch::Upload(host.first, nullptr), "Upload");
  const int64_t bytes = (int64_t{1} << kLog) * 4;
  DeviceMem out;
  if (dpf_hip_alloc(&out.p, 8 * bytes) != 0) Fail("dpf_hip_alloc");
  auto expect = [&](const dpf::Status& st, dpf::StatusCode code, const char* what) {
    if (st.ok() || st.code() != code) Fail(std::string(what) + ": " + st.ToString());
  };
  using dpf::StatusCode;
  // A wrong T, as EvaluateUntil<T> refuses it.
  expect(d->EvaluateFullDomainSumPacked<uint64_t>(*keys, 0).status(), StatusCode::kInvalidArgument,
         "wrong T");
  expect(d->EvaluateFullDomainSumPacked<dpf::XorWrapper<uint32_t>>(*keys, 0).status(),
         StatusCode::kInvalidArgument, "wrong T (XorWrapper)");
  expect(d->EvaluateFullDomainSumPacked<uint32_t>(*keys, 1).status(), StatusCode::kInvalidArgument,
         "level");
  expect(d->EvaluateFullDomainSumPackedToDevice(*keys, 0, nullptr, bytes, false, nullptr).status(),
         StatusCode::kInvalidArgument, "null output");
  expect(d->EvaluateFullDomainSumPackedToDevice(*keys, 0, out.p, bytes - 4, false, nullptr).status(),
         StatusCode::kInvalidArgument, "out_bytes");
  expect(d->EvaluateFullDomainSumPackedToDevice(*keys, 0, static_cast<char*>(out.p) + 8, bytes,
                                                false, nullptr)
             .status(),
         StatusCode::kInvalidArgument, "alignment");
  // A batch of another DistributedPointFunction.
  auto other = MakeDpf<uint32_t>(kLog + 1);
  expect(other->EvaluateFullDomainSumPackedToDevice(*keys, 0, out.p, 2 * bytes, false, nullptr)
             .status(),
         StatusCode::kInvalidArgument, "foreign batch");
  expect(other->EvaluateFullDomainSumPacked<uint32_t>(*keys, 0).status(),
         StatusCode::kInvalidArgument, "foreign batch, host result");
  // No fallback behind the call: additive uint128, and a domain below one leaf block.
  auto u128 = MakeDpf<uint128>(kLog);
  if (u128->EvaluatesFullDomainSumPackedOnDevice(0)) Fail("uint128 reported as supported");
  expect(u128->EvaluateFullDomainSumPackedToDevice(*keys, 0, out.p, 8 * bytes, false, nullptr)
             .status(),
         StatusCode::kUnimplemented, "uint128");
  expect(u128->EvaluateFullDomainSumPacked<uint128>(*keys, 0).status(), StatusCode::kUnimplemented,
         "uint128, host result");
  auto small = MakeDpf<uint8_t>(3);
  if (small->EvaluatesFullDomainSumPackedOnDevice(0)) Fail("uint8_t, n = 3 reported as supported");
  expect(small->EvaluateFullDomainSumPacked<uint8_t>(*keys, 0).status(), StatusCode::kUnimplemented,
         "below one leaf block");
  // The earlier call refuses what it refused.
  expect(d->EvaluateFullDomainSum(*keys, 0).status(), StatusCode::kUnimplemented,
         "uint32_t through EvaluateFullDomainSum");
  std::printf("ok error codes\n");
}

}  // namespace

int main() {
  SumEqualsEvaluateUntil<uint32_t, Add<uint32_t>>("uint32_t", 9);
  SumEqualsEvaluateUntil<uint8_t, Add<uint8_t>>("uint8_t", 9);
  SumEqualsEvaluateUntil<dpf::XorWrapper<uint128>, Xor<uint128>>("XorWrapper<uint128>", 7);
  ErrorCodes();
  std::printf("ALL OK\n");
  return 0;
}
