// sketch_api_test.cc -- EvaluateUntilBatchSketchToDevice (per-key linear
// sketches of a key batch's EvaluateUntil outputs) through the public headers
// only.  On a 3-level Tuple<IntModN32, IntModN32> hierarchy with 70 key pairs,
// every key's sketch at every level must equal host EvaluateUntil<T> folded
// with the weights on the host, the sums must equal the host sum over the keys,
// the two parties' sketches must add up to w[j][i*] * beta, and a bad weight
// row count and a short sketch buffer must be refused with the context
// untouched.
//
// Exit status 0 and "ALL OK" on success; the first mismatch is printed.
// Run by tests/test_sketch_cpp_gpu.py; built by build_native.build_tools.
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
using dpf::DpfParameters;
using dpf::uint128;
constexpr uint32_t kN = 4294967291u;
using ModN = dpf::IntModN<uint32_t, kN>;
using T = dpf::Tuple<ModN, ModN>;

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

constexpr int kLogs[3] = {4, 6, 8};
constexpr int kKeys = 70, kRows = 2;
constexpr uint32_t kBeta[2] = {1, 7};

struct DeviceBuf {
  void* p = nullptr;
  explicit DeviceBuf(size_t bytes) {
    if (dpf_hip_alloc(&p, bytes) != 0) Fail("dpf_hip_alloc");
  }
  ~DeviceBuf() {
    if (p) dpf_hip_free(p);
  }
};

uint32_t Leaf(const T& v, int e) {
  return e == 0 ? std::get<0>(v.value()).value() : std::get<1>(v.value()).value();
}

}  // namespace

int main() {
  std::vector<DpfParameters> params(3);
  for (int h = 0; h < 3; ++h) {
    params[h].set_log_domain_size(kLogs[h]);
    *params[h].mutable_value_type() = dpf::ToValueType<T>();
  }
  auto f = Must(DistributedPointFunction::CreateIncremental(params), "CreateIncremental");
  if (!f->RegisterValueType<T>().ok()) Fail("RegisterValueType");
  std::mt19937_64 rng(20250131);
  std::vector<uint128> alphas(kKeys);
  for (uint128& a : alphas) a = rng() % (uint64_t{1} << kLogs[2]);
  const T beta{ModN{kBeta[0]}, ModN{kBeta[1]}};
  const std::vector<dpf::Value> betas(3, Must(f->ToValue(beta), "ToValue"));
  auto batches = Must(f->GenerateKeyBatch(alphas, betas, dpf::Span<const uint128>()),
                      "GenerateKeyBatch");
  const dpf::KeyBatch* host[2] = {&batches.first, &batches.second};

  // Level 0: every output; then the prefixes of the first 40 keys' alphas.
  std::vector<uint128> prefixes[3];
  for (int h = 1; h < 3; ++h) {
    for (int k = 0; k < 40; ++k) {
      const uint128 p = alphas[k] >> (kLogs[2] - kLogs[h - 1]);
      bool seen = false;
      for (uint128 q : prefixes[h]) seen |= q == p;
      if (!seen) prefixes[h].push_back(p);
    }
  }
  std::vector<uint32_t> sketch[2][3];
  std::vector<std::vector<uint32_t>> weights(3);
  std::vector<std::vector<uint128>> outputs(3);   // domain value of each output
  for (int party = 0; party < 2; ++party) {
    auto dev = Must(dpf::DeviceKeyBatch::Upload(*host[party], nullptr), "Upload");
    auto ctx = Must(f->CreateBatchEvaluationContext(*dev), "CreateBatchEvaluationContext");
    std::vector<dpf::EvaluationContext> hctx;
    for (int k = 0; k < kKeys; ++k)
      hctx.push_back(Must(f->CreateEvaluationContext(Must(f->KeyFromBatch(*host[party], k), "key")),
                          "CreateEvaluationContext"));
    for (int h = 0; h < 3; ++h) {
      const int step = kLogs[h] - (h ? kLogs[h - 1] : 0);
      const int64_t n = h ? static_cast<int64_t>(prefixes[h].size()) << step : int64_t{1} << kLogs[0];
      if (party == 0) {
        weights[h].resize(kRows * n);
        for (uint32_t& w : weights[h]) w = static_cast<uint32_t>(rng());
        weights[h][0] = kN;            // reduces to 0
        weights[h][1] = 0xffffffffu;   // reduces to 4
        for (int64_t i = 0; i < n; ++i)
          outputs[h].push_back(h ? (prefixes[h][i >> step] << step) | (i & ((1 << step) - 1))
                                 : uint128(i));
      }
      DeviceBuf dw(weights[h].size() * 4), dsums(n * 8), dsk(kKeys * kRows * 2 * 4);
      if (dpf_hip_memcpy_h2d(dw.p, weights[h].data(), weights[h].size() * 4, nullptr) != 0)
        Fail("h2d");
      if (h == 1) {
        // Refused before the context is touched.
        auto bad = f->EvaluateUntilBatchSketchToDevice(
            h, prefixes[h], *ctx, static_cast<const uint32_t*>(dw.p), 5, n, dsums.p, n * 8,
            static_cast<uint32_t*>(dsk.p), kKeys * kRows * 2 * 4, nullptr);
        if (bad.ok() || bad.status().code() != dpf::StatusCode::kInvalidArgument)
          Fail("five weight rows accepted");
        bad = f->EvaluateUntilBatchSketchToDevice(
            h, prefixes[h], *ctx, static_cast<const uint32_t*>(dw.p), kRows, n, dsums.p, n * 8,
            static_cast<uint32_t*>(dsk.p), kKeys * kRows * 2 * 4 - 1, nullptr);
        if (bad.ok() || bad.status().code() != dpf::StatusCode::kInvalidArgument)
          Fail("short sketch buffer accepted");
        if (ctx->previous_hierarchy_level() != 0) Fail("a refused call moved the context");
      }
      const int64_t got_n = Must(
          f->EvaluateUntilBatchSketchToDevice(h, prefixes[h], *ctx,
                                              static_cast<const uint32_t*>(dw.p), kRows, n, dsums.p,
                                              n * 8, static_cast<uint32_t*>(dsk.p),
                                              kKeys * kRows * 2 * 4, nullptr),
          "EvaluateUntilBatchSketchToDevice");
      if (got_n != n) Fail("output count");
      sketch[party][h].resize(kKeys * kRows * 2);
      std::vector<uint32_t> sums(n * 2);
      if (dpf_hip_memcpy_d2h(sketch[party][h].data(), dsk.p, sketch[party][h].size() * 4, nullptr) ||
          dpf_hip_memcpy_d2h(sums.data(), dsums.p, sums.size() * 4, nullptr))
        Fail("d2h");
      std::vector<uint64_t> want_sums(n * 2, 0);
      for (int k = 0; k < kKeys; ++k) {
        const std::vector<T> y = Must(f->EvaluateUntil<T>(h, prefixes[h], hctx[k]), "EvaluateUntil");
        if (static_cast<int64_t>(y.size()) != n) Fail("EvaluateUntil size");
        for (int j = 0; j < kRows; ++j)
          for (int e = 0; e < 2; ++e) {
            unsigned __int128 acc = 0;
            for (int64_t i = 0; i < n; ++i)
              acc += static_cast<uint64_t>(weights[h][j * n + i] % kN) * Leaf(y[i], e);
            if (sketch[party][h][(k * kRows + j) * 2 + e] != static_cast<uint32_t>(acc % kN))
              Fail("party " + std::to_string(party) + " level " + std::to_string(h) + " key " +
                   std::to_string(k) + " differs from the host fold");
          }
        for (int64_t i = 0; i < n; ++i)
          for (int e = 0; e < 2; ++e) want_sums[i * 2 + e] = (want_sums[i * 2 + e] + Leaf(y[i], e)) % kN;
      }
      for (int64_t i = 0; i < n * 2; ++i)
        if (sums[i] != want_sums[i]) Fail("sums differ from the host sum at level " + std::to_string(h));
    }
  }
  std::printf("ok both parties' sketches and sums equal the host fold\n");
  for (int h = 0; h < 3; ++h) {
    const int64_t n = static_cast<int64_t>(outputs[h].size());
    for (int k = 0; k < kKeys; ++k) {
      const uint128 a = alphas[k] >> (kLogs[2] - kLogs[h]);
      int64_t at = -1;
      for (int64_t i = 0; i < n; ++i)
        if (outputs[h][i] == a) at = i;
      if (k < 40 && at < 0) Fail("alpha's output is missing");
      for (int j = 0; j < kRows; ++j)
        for (int e = 0; e < 2; ++e) {
          const uint64_t z = (uint64_t{sketch[0][h][(k * kRows + j) * 2 + e]} +
                              sketch[1][h][(k * kRows + j) * 2 + e]) % kN;
          const uint64_t want =
              at < 0 ? 0 : static_cast<uint64_t>(weights[h][j * n + at] % kN) * kBeta[e] % kN;
          if (z != want)
            Fail("level " + std::to_string(h) + " key " + std::to_string(k) + " does not recombine");
        }
    }
  }
  std::printf("ok the parties' sketches recombine to w[j][i*] * beta\n");
  std::printf("ok errors\n");
  std::printf("ALL OK\n");
  return 0;
}
