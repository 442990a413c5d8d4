// dot_buckets_api_test.cc -- multi-query PIR over a bucketed database through
// the public headers only: EvaluateDotBuckets must equal EvaluateDot<T> of
// every key on its bucket's slice, for uint64_t and XorWrapper<uint64_t> and
// both parties, whose answers must reconstruct beta * db[b(k)][alpha];
// argument errors carry their codes and an IntModN DPF is UNIMPLEMENTED.
//
// Exit status 0 and "ALL OK" on success; the first mismatch is printed.
// Run by tests/test_dot_buckets_cpp_gpu.py; built by build_native.build_tools.
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
void BucketsEqualEvaluateDot(const char* name) {
  constexpr int kLog = 7;
  constexpr uint64_t kN = uint64_t{1} << kLog;
  // Populations 2, 0, 18, 1: an empty bucket and a tile boundary at 16.
  const std::vector<int64_t> begin = {0, 2, 2, 20, 21};
  const int kKeys = static_cast<int>(begin.back()), kBuckets = static_cast<int>(begin.size()) - 1;
  auto d = MakeDpf<T>(kLog);
  if (!d->EvaluatesDotBucketsOnDevice(0)) Fail(std::string(name) + " should fold on the device");
  if (d->EvaluatesDotBucketsOnDevice(1)) Fail("a level that does not exist reported as supported");
  std::mt19937_64 rng(2025);
  std::vector<uint128> alphas;
  std::vector<dpf::Value> betas;
  std::vector<uint64_t> beta_words;
  std::vector<int> bucket;
  for (int b = 0; b < kBuckets; ++b)
    for (int64_t k = begin[b]; k < begin[b + 1]; ++k) bucket.push_back(b);
  for (int k = 0; k < kKeys; ++k) {
    alphas.push_back(uint128{k == 0 ? 0 : (k == 1 ? kN - 1 : rng() % kN)});
    beta_words.push_back(rng() | 1);
    betas.push_back(Must(d->template ToValue<T>(T(beta_words.back())), "beta"));
  }
  auto host = Must(d->GenerateKeyBatchWithBetas(dpf::MakeConstSpan(alphas), dpf::MakeConstSpan(betas),
                                                dpf::Span<const uint128>()),
                   "GenerateKeyBatchWithBetas");
  for (int W : {1, 3, 65}) {
    const uint64_t slice = kN * W;
    std::vector<uint64_t> db(kBuckets * slice);
    for (uint64_t& w : db) w = rng();
    const int64_t bytes = static_cast<int64_t>(db.size() * sizeof(uint64_t));
    const int64_t slice_bytes = static_cast<int64_t>(slice * sizeof(uint64_t));
    DeviceMem dev;
    if (dpf_hip_alloc(&dev.p, bytes) != 0) Fail("dpf_hip_alloc");
    if (dpf_hip_memcpy_h2d(dev.p, db.data(), bytes, nullptr) != 0) Fail("dpf_hip_memcpy_h2d");
    std::vector<uint64_t> share[2];
    const dpf::KeyBatch* batches[2] = {&host.first, &host.second};
    for (int party = 0; party < 2; ++party) {
      auto keys = Must(dpf::DeviceKeyBatch::Upload(*batches[party], nullptr), "Upload");
      share[party] = Must(d->EvaluateDotBuckets(*keys, 0, dpf::MakeConstSpan(begin), dev.p, bytes, W),
                          "EvaluateDotBuckets");
      if (share[party].size() != static_cast<size_t>(kKeys * W)) Fail("result size");
      for (int k = 0; k < kKeys; ++k) {
        const dpf::DpfKey key = Must(d->KeyFromBatch(*batches[party], k), "key");
        const char* at = static_cast<const char*>(dev.p) + bucket[k] * slice_bytes;
        std::vector<T> want = Must(d->template EvaluateDot<T>(key, 0, at, slice_bytes, W), "EvaluateDot");
        if (want.size() != static_cast<size_t>(W)) Fail("EvaluateDot: size");
        for (int w = 0; w < W; ++w)
          if (share[party][k * W + w] != Word(want[w]))
            Fail(std::string(name) + " W " + std::to_string(W) + " party " + std::to_string(party) +
                 " key " + std::to_string(k) + " word " + std::to_string(w) +
                 ": differs from EvaluateDot");
      }
    }
    for (int k = 0; k < kKeys; ++k)
      for (int w = 0; w < W; ++w) {
        const uint64_t t = db[bucket[k] * slice + static_cast<uint64_t>(alphas[k]) * W + w];
        const uint64_t got = kXor ? share[0][k * W + w] ^ share[1][k * W + w]
                                  : share[0][k * W + w] + share[1][k * W + w];
        if (got != (kXor ? beta_words[k] & t : beta_words[k] * t)) Fail("shares do not reconstruct");
      }
  }
  std::printf("ok EvaluateDotBuckets<%s>\n", name);
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
  const int64_t slice = (int64_t{1} << kLog) * 8;   // one bucket of one word
  DeviceMem db, out;
  if (dpf_hip_alloc(&db.p, slice * 8) != 0 || dpf_hip_alloc(&out.p, 64) != 0) Fail("dpf_hip_alloc");
  auto expect = [&](const dpf::Status& st, dpf::StatusCode code, const char* what) {
    if (st.ok() || st.code() != code) Fail(std::string(what) + ": " + st.ToString());
  };
  using dpf::StatusCode;
  const std::vector<int64_t> begin = {0, 1, 2}, short_begin = {0}, not_zero = {1, 1, 2},
                             decreasing = {0, 2, 1}, wrong_end = {0, 1, 3};
  auto call = [&](const DistributedPointFunction& f, int level, const std::vector<int64_t>& bb,
                  const void* p, int64_t bytes, int64_t W, void* o, int64_t out_bytes) {
    return f.EvaluateDotBucketsToDevice(*keys, level, dpf::MakeConstSpan(bb), p, bytes, W, o,
                                        out_bytes, nullptr)
        .status();
  };
  expect(call(*d, 1, begin, db.p, 2 * slice, 1, out.p, 64), StatusCode::kInvalidArgument, "level");
  expect(call(*d, 0, begin, db.p, 2 * slice, 0, out.p, 64), StatusCode::kInvalidArgument,
         "record_words 0");
  expect(call(*d, 0, short_begin, db.p, 2 * slice, 1, out.p, 64), StatusCode::kInvalidArgument,
         "bucket_begin of one entry");
  expect(call(*d, 0, not_zero, db.p, 2 * slice, 1, out.p, 64), StatusCode::kInvalidArgument,
         "bucket_begin not from 0");
  expect(call(*d, 0, decreasing, db.p, 2 * slice, 1, out.p, 64), StatusCode::kInvalidArgument,
         "bucket_begin decreasing");
  expect(call(*d, 0, wrong_end, db.p, 2 * slice, 1, out.p, 64), StatusCode::kInvalidArgument,
         "bucket_begin not to K");
  expect(call(*d, 0, begin, db.p, 2 * slice - 8, 1, out.p, 64), StatusCode::kInvalidArgument,
         "db_bytes");
  expect(call(*d, 0, begin, nullptr, 2 * slice, 1, out.p, 64), StatusCode::kInvalidArgument,
         "null db");
  expect(call(*d, 0, begin, db.p, 2 * slice, 1, out.p, 15), StatusCode::kInvalidArgument,
         "out_bytes");
  // Two faults at once: the earlier check is the one reported.
  expect(call(*d, 0, wrong_end, nullptr, 2 * slice, 0, out.p, 0), StatusCode::kInvalidArgument,
         "record_words before the rest");
  // A batch of another DistributedPointFunction.
  auto other = MakeDpf<uint64_t>(kLog + 1);
  expect(call(*other, 0, begin, db.p, 4 * slice, 1, out.p, 64), StatusCode::kInvalidArgument,
         "foreign batch");
  // No fallback behind the call.
  using M = dpf::IntModN<uint64_t, 18446744073709551557ull>;
  auto modn = MakeDpf<M>(kLog);
  if (modn->EvaluatesDotBucketsOnDevice(0)) Fail("IntModN reported as supported");
  expect(call(*modn, 0, begin, db.p, 2 * slice, 1, out.p, 64), StatusCode::kUnimplemented, "IntModN");
  auto u32 = MakeDpf<uint32_t>(kLog);
  expect(u32->EvaluateDotBuckets(*keys, 0, dpf::MakeConstSpan(begin), db.p, 2 * slice, 1).status(),
         StatusCode::kUnimplemented, "uint32_t");
  std::printf("ok error codes\n");
}

}  // namespace

int main() {
  BucketsEqualEvaluateDot<uint64_t, false>("uint64_t");
  BucketsEqualEvaluateDot<dpf::XorWrapper<uint64_t>, true>("XorWrapper<uint64_t>");
  ErrorCodes();
  std::printf("ALL OK\n");
  return 0;
}
