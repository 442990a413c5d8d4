// full_domain_sketch_api_test.cc -- checked private histograms through the
// public headers only: EvaluateFullDomainSumSketch and
// EvaluateFullDomainSumSketchToDevice must equal the per-key EvaluateUntil<T>
// vectors summed and sketched on the host in 64-bit integers, for
// IntModN<uint32_t, 2^32 - 5> and the 2-tuple of it and both parties, whose
// sums must reconstruct the histogram and whose sketches must add up to
// w[j][alpha_k] * beta; `accumulate` adds mod N into what the sums hold, the
// sketches are overwritten; uint64_t is UNIMPLEMENTED here and the field types
// stay UNIMPLEMENTED in EvaluateFullDomainSum; a batch of another DPF is refused.
//
// Exit status 0 and "ALL OK" on success; the first mismatch is printed.
// Run by tests/test_full_domain_sketch_cpp_gpu.py; built by build_native.build_tools.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "dpf/distributed_point_function.h"
#include "dpf/int_mod_n.h"
#include "dpf/key_batch.h"
#include "dpf/tuple.h"
#include "dpf_hip.h"

namespace dpf = distributed_point_functions;
using dpf::DistributedPointFunction;
using dpf::uint128;
constexpr uint32_t kMod = 4294967291u;
using ModN = dpf::IntModN<uint32_t, kMod>;
using Pair = dpf::Tuple<ModN, ModN>;

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
  auto d = Must(DistributedPointFunction::Create(p), "Create");
  if (!d->template RegisterValueType<T>().ok()) Fail("RegisterValueType");
  return d;
}

struct DeviceMem {
  void* p = nullptr;
  explicit DeviceMem(size_t bytes) {
    if (dpf_hip_alloc(&p, bytes) != 0) Fail("dpf_hip_alloc");
  }
  ~DeviceMem() {
    if (p) dpf_hip_free(p);
  }
};

uint32_t Leaf(const ModN& v, int) { return v.value(); }
uint32_t Leaf(const Pair& v, int e) {
  return e == 0 ? std::get<0>(v.value()).value() : std::get<1>(v.value()).value();
}
ModN MakeBeta(const uint32_t* b, ModN*) { return ModN{b[0]}; }
Pair MakeBeta(const uint32_t* b, Pair*) { return Pair{ModN{b[0]}, ModN{b[1]}}; }

template <typename T, int kLeaves>
void SumSketchEqualsEvaluateUntil(const char* name) {
  constexpr int kLog = 9, kKeys = 70, kRows = 2;
  constexpr uint64_t kN = uint64_t{1} << kLog;
  constexpr uint32_t kBeta[2] = {1, 7};
  auto d = MakeDpf<T>(kLog);
  if (!d->EvaluatesFullDomainSumSketchOnDevice(0))
    Fail(std::string(name) + " should be summed and sketched on the device");
  if (d->EvaluatesFullDomainSumSketchOnDevice(1)) Fail("a level that does not exist reported");
  if (d->EvaluatesFullDomainSumOnDevice(0)) Fail("the ring sum reports a field type");
  std::mt19937_64 rng(32);
  std::vector<uint128> alphas;
  for (int k = 0; k < kKeys; ++k)
    alphas.push_back(uint128{k == 0 ? 0 : (k == 1 ? kN - 1 : (k < 6 ? 17 : rng() % kN))});
  const std::vector<dpf::Value> beta = {
      Must(d->ToValue(MakeBeta(kBeta, static_cast<T*>(nullptr))), "beta")};
  auto host = Must(d->GenerateKeyBatch(dpf::MakeConstSpan(alphas), dpf::MakeConstSpan(beta),
                                       dpf::Span<const uint128>()),
                   "GenerateKeyBatch");
  std::vector<uint32_t> weights(kRows * kN);
  for (uint32_t& w : weights) w = static_cast<uint32_t>(rng());
  weights[0] = kMod;            // reduces to 0
  weights[1] = 0xffffffffu;     // reduces to 4
  weights[2] = kMod - 1;
  const dpf::KeyBatch* batches[2] = {&host.first, &host.second};
  DistributedPointFunction::SumSketch share[2];
  for (int party = 0; party < 2; ++party) {
    auto keys = Must(dpf::DeviceKeyBatch::Upload(*batches[party], nullptr), "Upload");
    share[party] = Must(d->EvaluateFullDomainSumSketch(0, *keys, weights, kRows),
                        "EvaluateFullDomainSumSketch");
    if (share[party].sum.size() != kN * kLeaves ||
        share[party].sketch.size() != size_t{kKeys} * kRows * kLeaves)
      Fail("result sizes");
    std::vector<uint64_t> sum(kN * kLeaves, 0);
    std::vector<uint32_t> want_sum(kN * kLeaves), want_sk(kKeys * kRows * kLeaves);
    for (int k = 0; k < kKeys; ++k) {
      auto ctx = Must(d->CreateEvaluationContext(Must(d->KeyFromBatch(*batches[party], k), "key")),
                      "CreateEvaluationContext");
      std::vector<T> y = Must(d->template EvaluateUntil<T>(0, {}, ctx), "EvaluateUntil");
      if (y.size() != kN) Fail("EvaluateUntil: size");
      for (int j = 0; j < kRows; ++j)
        for (int e = 0; e < kLeaves; ++e) {
          uint64_t s = 0;   // reduced at every step: each term is below 2^32
          for (uint64_t i = 0; i < kN; ++i)
            s = (s + uint64_t{weights[j * kN + i] % kMod} * Leaf(y[i], e) % kMod) % kMod;
          want_sk[(k * kRows + j) * kLeaves + e] = static_cast<uint32_t>(s);
        }
      for (uint64_t i = 0; i < kN; ++i)
        for (int e = 0; e < kLeaves; ++e) sum[i * kLeaves + e] += Leaf(y[i], e);
    }
    for (size_t i = 0; i < sum.size(); ++i) want_sum[i] = static_cast<uint32_t>(sum[i] % kMod);
    if (share[party].sum != want_sum)
      Fail(std::string(name) + " party " + std::to_string(party) + ": sums differ from the host's");
    if (share[party].sketch != want_sk)
      Fail(std::string(name) + " party " + std::to_string(party) + ": sketches differ");

    // The plain field sum: no weights, no sketch buffer.
    auto plain = Must(d->EvaluateFullDomainSumSketch(0, *keys, {}, 0), "J = 0");
    if (plain.sum != want_sum || !plain.sketch.empty()) Fail(std::string(name) + ": J = 0");

    // ToDevice: over prefilled buffers, then accumulated on top of itself.
    const int64_t sum_bytes = static_cast<int64_t>(kN * kLeaves * 4);
    const int64_t sk_bytes = int64_t{kKeys} * kRows * kLeaves * 4;
    DeviceMem out(sum_bytes), sk(sk_bytes), dw(weights.size() * 4);
    if (dpf_hip_memset(out.p, 0xAB, sum_bytes, nullptr) != 0 ||
        dpf_hip_memset(sk.p, 0xAB, sk_bytes, nullptr) != 0 ||
        dpf_hip_memcpy_h2d(dw.p, weights.data(), weights.size() * 4, nullptr) != 0)
      Fail("device buffers");
    std::vector<uint32_t> got(kN * kLeaves), got_sk(want_sk.size());
    auto call = [&](bool accumulate) {
      if (Must(d->EvaluateFullDomainSumSketchToDevice(0, *keys, static_cast<const uint32_t*>(dw.p),
                                                      kRows, out.p, sum_bytes, sk.p, sk_bytes,
                                                      accumulate, nullptr),
               "ToDevice") != static_cast<int64_t>(kN))
        Fail("ToDevice: return value");
      if (dpf_hip_memcpy_d2h(got.data(), out.p, sum_bytes, nullptr) != 0 ||
          dpf_hip_memcpy_d2h(got_sk.data(), sk.p, sk_bytes, nullptr) != 0)
        Fail("dpf_hip_memcpy_d2h");
    };
    call(false);
    if (got != want_sum || got_sk != want_sk)
      Fail(std::string(name) + ": ToDevice over prefilled buffers differs");
    call(true);
    for (size_t i = 0; i < got.size(); ++i)
      if (got[i] != 2 * uint64_t{want_sum[i]} % kMod)
        Fail(std::string(name) + ": accumulate at " + std::to_string(i));
    if (got_sk != want_sk) Fail(std::string(name) + ": sketches were accumulated");
  }
  // The sums reconstruct the histogram; every client's sketches add up to
  // w[j][alpha] * beta.
  std::vector<uint64_t> hist(kN * kLeaves, 0);
  for (int k = 0; k < kKeys; ++k)
    for (int e = 0; e < kLeaves; ++e) hist[static_cast<uint64_t>(alphas[k]) * kLeaves + e] += kBeta[e];
  for (size_t i = 0; i < hist.size(); ++i)
    if ((uint64_t{share[0].sum[i]} + share[1].sum[i]) % kMod != hist[i])
      Fail(std::string(name) + ": shares do not reconstruct at " + std::to_string(i));
  for (int k = 0; k < kKeys; ++k)
    for (int j = 0; j < kRows; ++j)
      for (int e = 0; e < kLeaves; ++e) {
        const size_t i = (static_cast<size_t>(k) * kRows + j) * kLeaves + e;
        const uint64_t w = weights[j * kN + static_cast<uint64_t>(alphas[k])] % kMod;
        if ((uint64_t{share[0].sketch[i]} + share[1].sketch[i]) % kMod != w * kBeta[e] % kMod)
          Fail(std::string(name) + ": sketches do not recombine for key " + std::to_string(k));
      }
  std::printf("ok EvaluateFullDomainSumSketch<%s>\n", name);
}

void ErrorCodes() {
  constexpr int kLog = 5;
  constexpr int64_t kN = int64_t{1} << kLog;
  auto d = MakeDpf<Pair>(kLog);
  std::vector<uint128> alphas = {uint128{3}, uint128{17}};
  const uint32_t b[2] = {1, 7};
  std::vector<dpf::Value> beta = {Must(d->ToValue(MakeBeta(b, static_cast<Pair*>(nullptr))), "beta")};
  auto host = Must(d->GenerateKeyBatch(dpf::MakeConstSpan(alphas), dpf::MakeConstSpan(beta),
                                       dpf::Span<const uint128>()),
                   "GenerateKeyBatch");
  auto keys = Must(dpf::DeviceKeyBatch::Upload(host.first, nullptr), "Upload");
  const int64_t sum_bytes = kN * 2 * 4, sk_bytes = 2 * 2 * 2 * 4;
  DeviceMem out(4 * sum_bytes), sk(sk_bytes), w(2 * kN * 4);
  const uint32_t* dw = static_cast<const uint32_t*>(w.p);
  auto expect = [&](const dpf::Status& st, dpf::StatusCode code, const char* what) {
    if (st.ok() || st.code() != code) Fail(std::string(what) + ": " + st.ToString());
  };
  using dpf::StatusCode;
  auto run = [&](DistributedPointFunction& f, int h, const uint32_t* weights, int rows, void* sum,
                 int64_t sb, void* sketch, int64_t kb) {
    return f.EvaluateFullDomainSumSketchToDevice(h, *keys, weights, rows, sum, sb, sketch, kb, false,
                                                 nullptr)
        .status();
  };
  expect(run(*d, 1, dw, 2, out.p, sum_bytes, sk.p, sk_bytes), StatusCode::kInvalidArgument, "level");
  expect(run(*d, 0, dw, 3, out.p, sum_bytes, sk.p, sk_bytes), StatusCode::kInvalidArgument, "rows");
  expect(run(*d, 0, dw, 2, nullptr, sum_bytes, sk.p, sk_bytes), StatusCode::kInvalidArgument,
         "null sums");
  expect(run(*d, 0, nullptr, 2, out.p, sum_bytes, sk.p, sk_bytes), StatusCode::kInvalidArgument,
         "null weights");
  expect(run(*d, 0, dw, 2, out.p, sum_bytes, nullptr, sk_bytes), StatusCode::kInvalidArgument,
         "null sketches");
  expect(run(*d, 0, dw, 2, out.p, sum_bytes - 4, sk.p, sk_bytes), StatusCode::kInvalidArgument,
         "sum_bytes");
  expect(run(*d, 0, dw, 2, out.p, sum_bytes, sk.p, sk_bytes - 1), StatusCode::kInvalidArgument,
         "sketch_bytes");
  expect(run(*d, 0, dw, 2, static_cast<char*>(out.p) + 8, sum_bytes, sk.p, sk_bytes),
         StatusCode::kInvalidArgument, "alignment");
  expect(d->EvaluateFullDomainSumSketch(0, *keys, std::vector<uint32_t>(2 * kN - 1), 2).status(),
         StatusCode::kInvalidArgument, "host weights' size");
  // A batch of another DistributedPointFunction.
  auto other = MakeDpf<Pair>(kLog + 1);
  expect(run(*other, 0, dw, 0, out.p, 4 * sum_bytes, nullptr, 0), StatusCode::kInvalidArgument,
         "foreign batch");
  expect(other->EvaluateFullDomainSumSketch(0, *keys, {}, 0).status(), StatusCode::kInvalidArgument,
         "foreign batch, host result");
  // No fallback behind either call.
  dpf::DpfParameters p;
  p.set_log_domain_size(kLog);
  *p.mutable_value_type() = dpf::ToValueType<uint64_t>();
  auto u64 = Must(DistributedPointFunction::Create(p), "Create");
  if (u64->EvaluatesFullDomainSumSketchOnDevice(0)) Fail("uint64_t reported as supported");
  expect(run(*u64, 0, dw, 2, out.p, sum_bytes, sk.p, sk_bytes), StatusCode::kUnimplemented,
         "uint64_t");
  expect(u64->EvaluateFullDomainSumSketch(0, *keys, {}, 0).status(), StatusCode::kUnimplemented,
         "uint64_t, host result");
  expect(d->EvaluateFullDomainSumToDevice(*keys, 0, out.p, 4 * sum_bytes, false, nullptr).status(),
         StatusCode::kUnimplemented, "the ring sum of a field type");
  std::printf("ok error codes\n");
}

}  // namespace

int main() {
  SumSketchEqualsEvaluateUntil<ModN, 1>("IntModN<uint32_t, 2^32 - 5>");
  SumSketchEqualsEvaluateUntil<Pair, 2>("Tuple<IntModN32, IntModN32>");
  ErrorCodes();
  std::printf("ALL OK\n");
  return 0;
}
