// lookup_api_test.cc -- the batched private table lookup through the public
// headers only: EvaluateLookupBatch must equal EvaluateUntil<T> of every key
// folded into the rotated table on the host, for uint64_t and
// XorWrapper<uint64_t> and both parties, whose answers must reconstruct
// beta * T[(alpha + s) mod N]; argument errors carry their codes and an
// IntModN DPF is UNIMPLEMENTED.
//
// Exit status 0 and "ALL OK" on success; the first mismatch is printed.
// Run by tests/test_lookup_cpp_gpu.py; built by build_native.build_tools.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "dpf/distributed_point_function.h"
#include "dpf/int_mod_n.h"
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
void LookupEqualsEvaluateUntil(const char* name) {
  constexpr int kLog = 7, kKeys = 9;
  constexpr uint64_t kN = uint64_t{1} << kLog;
  auto d = MakeDpf<T>(kLog);
  if (!d->EvaluatesLookupOnDevice(0)) Fail(std::string(name) + " should look up on the device");
  if (d->EvaluatesLookupOnDevice(1)) Fail("a level that does not exist reported as supported");
  std::mt19937_64 rng(2024);
  std::vector<uint128> alphas;
  std::vector<dpf::Value> betas;
  std::vector<uint64_t> beta_words, offsets;
  for (int k = 0; k < kKeys; ++k) {
    alphas.push_back(uint128{k == 0 ? 0 : (k == 1 ? kN - 1 : rng() % kN)});
    beta_words.push_back(rng() | 1);
    betas.push_back(Must(d->template ToValue<T>(T(beta_words.back())), "beta"));
    offsets.push_back(k == 2 ? kN + 1 + (uint64_t{3} << 50) : (k == 3 ? 0 : rng()));
  }
  auto host = Must(d->GenerateKeyBatchWithBetas(dpf::MakeConstSpan(alphas), dpf::MakeConstSpan(betas),
                                                dpf::Span<const uint128>()),
                   "GenerateKeyBatchWithBetas");
  for (int W : {1, 2, 4}) {
    std::vector<uint64_t> table(kN * W);
    for (uint64_t& w : table) w = rng();
    const int64_t bytes = static_cast<int64_t>(table.size() * sizeof(uint64_t));
    DeviceMem dev;
    if (dpf_hip_alloc(&dev.p, bytes) != 0) Fail("dpf_hip_alloc");
    if (dpf_hip_memcpy_h2d(dev.p, table.data(), bytes, nullptr) != 0) Fail("dpf_hip_memcpy_h2d");
    std::vector<uint64_t> share[2];
    const dpf::KeyBatch* batches[2] = {&host.first, &host.second};
    for (int party = 0; party < 2; ++party) {
      auto keys = Must(dpf::DeviceKeyBatch::Upload(*batches[party], nullptr), "Upload");
      share[party] = Must(d->EvaluateLookupBatch(*keys, 0, dpf::MakeConstSpan(offsets), dev.p, bytes, W),
                          "EvaluateLookupBatch");
      if (share[party].size() != static_cast<size_t>(kKeys * W)) Fail("result size");
      for (int k = 0; k < kKeys; ++k) {
        auto ctx = Must(d->CreateEvaluationContext(Must(d->KeyFromBatch(*batches[party], k), "key")),
                        "CreateEvaluationContext");
        std::vector<T> y = Must(d->template EvaluateUntil<T>(0, {}, ctx), "EvaluateUntil");
        if (y.size() != kN) Fail("EvaluateUntil: size");
        for (int w = 0; w < W; ++w) {
          uint64_t want = 0;
          for (uint64_t i = 0; i < kN; ++i) {
            const uint64_t t = table[((i + offsets[k]) % kN) * W + w];
            if (kXor) want ^= Word(y[i]) & t;
            else want += Word(y[i]) * t;
          }
          if (share[party][k * W + w] != want)
            Fail(std::string(name) + " W " + std::to_string(W) + " party " + std::to_string(party) +
                 " key " + std::to_string(k) + " word " + std::to_string(w) + ": differs from the fold");
        }
      }
    }
    for (int k = 0; k < kKeys; ++k)
      for (int w = 0; w < W; ++w) {
        const uint64_t t =
            table[((static_cast<uint64_t>(alphas[k]) + offsets[k]) % kN) * W + w];
        const uint64_t got = kXor ? share[0][k * W + w] ^ share[1][k * W + w]
                                  : share[0][k * W + w] + share[1][k * W + w];
        if (got != (kXor ? beta_words[k] & t : beta_words[k] * t)) Fail("shares do not reconstruct");
      }
  }
  std::printf("ok EvaluateLookupBatch<%s>\n", name);
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
  DeviceMem table, out, off;
  if (dpf_hip_alloc(&table.p, bytes * 4) != 0 || dpf_hip_alloc(&out.p, 64) != 0 ||
      dpf_hip_alloc(&off.p, 16) != 0)
    Fail("dpf_hip_alloc");
  const std::vector<uint64_t> offsets = {1, 2};
  auto expect = [&](const dpf::Status& st, dpf::StatusCode code, const char* what) {
    if (st.ok() || st.code() != code) Fail(std::string(what) + ": " + st.ToString());
  };
  const auto* o = static_cast<const uint64_t*>(off.p);
  using dpf::StatusCode;
  expect(d->EvaluateLookupBatchToDevice(*keys, 1, o, table.p, bytes, 1, out.p, 64, nullptr).status(),
         StatusCode::kInvalidArgument, "level");
  expect(d->EvaluateLookupBatchToDevice(*keys, 0, o, table.p, bytes, 0, out.p, 64, nullptr).status(),
         StatusCode::kInvalidArgument, "table_words 0");
  expect(d->EvaluateLookupBatchToDevice(*keys, 0, o, table.p, 3 * bytes, 3, out.p, 64, nullptr).status(),
         StatusCode::kUnimplemented, "table_words 3");
  expect(d->EvaluateLookupBatchToDevice(*keys, 0, o, table.p, bytes - 8, 1, out.p, 64, nullptr).status(),
         StatusCode::kInvalidArgument, "table_bytes");
  expect(d->EvaluateLookupBatchToDevice(*keys, 0, o, nullptr, bytes, 1, out.p, 64, nullptr).status(),
         StatusCode::kInvalidArgument, "null table");
  expect(d->EvaluateLookupBatchToDevice(*keys, 0, o, table.p, bytes, 1, out.p, 15, nullptr).status(),
         StatusCode::kInvalidArgument, "out_bytes");
  // Two faults at once: the earlier check is the one reported.
  expect(d->EvaluateLookupBatchToDevice(*keys, 0, o, nullptr, bytes, 3, out.p, 0, nullptr).status(),
         StatusCode::kUnimplemented, "table_words before null");
  expect(d->EvaluateLookupBatch(*keys, 0, dpf::Span<const uint64_t>(offsets.data(), 1), table.p, bytes, 1)
             .status(),
         StatusCode::kInvalidArgument, "offsets size");
  // A batch of another DistributedPointFunction.
  auto other = MakeDpf<uint64_t>(kLog + 1);
  expect(other->EvaluateLookupBatchToDevice(*keys, 0, o, table.p, 2 * bytes, 1, out.p, 64, nullptr)
             .status(),
         StatusCode::kInvalidArgument, "foreign batch");
  // No fallback behind the call.
  using M = dpf::IntModN<uint64_t, 18446744073709551557ull>;
  auto modn = MakeDpf<M>(kLog);
  if (modn->EvaluatesLookupOnDevice(0)) Fail("IntModN reported as supported");
  expect(modn->EvaluateLookupBatchToDevice(*keys, 0, o, table.p, bytes, 1, out.p, 64, nullptr).status(),
         StatusCode::kUnimplemented, "IntModN");
  auto u32 = MakeDpf<uint32_t>(kLog);
  expect(u32->EvaluateLookupBatch(*keys, 0, dpf::MakeConstSpan(offsets), table.p, bytes, 1).status(),
         StatusCode::kUnimplemented, "uint32_t");
  std::printf("ok error codes\n");
}

}  // namespace

int main() {
  LookupEqualsEvaluateUntil<uint64_t, false>("uint64_t");
  LookupEqualsEvaluateUntil<dpf::XorWrapper<uint64_t>, true>("XorWrapper<uint64_t>");
  ErrorCodes();
  std::printf("ALL OK\n");
  return 0;
}
