// dot_api_test.cc -- the C++ template EvaluateDot<T> (two-server PIR: the
// full-domain evaluation folded into a device-resident database) through the
// public headers only: for uint64_t and XorWrapper<absl::uint128> at
// log_domain_size 12 with records of 4 words, the two parties' answers must
// reconstruct record alpha scaled (masked) by beta, and uint32_t must be
// reported as UNIMPLEMENTED.
//
// Exit status 0 and "ALL OK" on success; the first mismatch is printed.
// Run by tests/test_dot_cpp_gpu.py; built by build_native.build_tools.
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
using dpf::DpfParameters;
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

constexpr int kLog = 12, kWords = 4;

template <typename T> struct Word;   // the database word of T, and beta's action on it
template <> struct Word<uint64_t> {
  using type = uint64_t;
  static uint64_t Beta() { return 0xFEEDFACECAFEBEEFull; }
  static uint64_t Select(uint64_t beta, uint64_t w) { return beta * w; }
  static uint64_t Random(std::mt19937_64& rng) { return rng(); }
};
template <> struct Word<dpf::XorWrapper<uint128>> {
  using type = uint128;
  static dpf::XorWrapper<uint128> Beta() {
    return dpf::XorWrapper<uint128>(dpf::MakeUint128(0xAAAA5555AAAA5555ull, 0x123456789ABCDEFull));
  }
  static dpf::XorWrapper<uint128> Select(dpf::XorWrapper<uint128> beta, uint128 w) {
    return dpf::XorWrapper<uint128>(beta.value() & w);
  }
  static uint128 Random(std::mt19937_64& rng) { return dpf::MakeUint128(rng(), rng()); }
};

struct DeviceDb {
  void* p = nullptr;
  ~DeviceDb() {
    if (p) dpf_hip_free(p);
  }
};

template <typename T>
void Reconstructs(const std::string& name) {
  using W = typename Word<T>::type;
  DpfParameters p;
  p.set_log_domain_size(kLog);
  *p.mutable_value_type() = dpf::ToValueType<T>();
  auto f = Must(DistributedPointFunction::Create(p), "Create " + name);
  std::mt19937_64 rng(name.size() * 7919);
  const uint128 alpha = rng() % (uint64_t{1} << kLog);
  const T beta = Word<T>::Beta();
  auto keys = Must(f->GenerateKeys(alpha, beta), "GenerateKeys " + name);
  const size_t n = size_t{1} << kLog;
  std::vector<W> db(n * kWords);
  for (W& w : db) w = Word<T>::Random(rng);
  const int64_t bytes = static_cast<int64_t>(db.size() * sizeof(W));
  DeviceDb dev;
  if (dpf_hip_alloc(&dev.p, bytes) != 0) Fail("dpf_hip_alloc");
  if (dpf_hip_memcpy_h2d(dev.p, db.data(), bytes, nullptr) != 0) Fail("dpf_hip_memcpy_h2d");
  std::vector<T> a = Must(f->template EvaluateDot<T>(keys.first, 0, dev.p, bytes, kWords),
                          "EvaluateDot party 0 " + name);
  std::vector<T> b = Must(f->template EvaluateDot<T>(keys.second, 0, dev.p, bytes, kWords),
                          "EvaluateDot party 1 " + name);
  if (a.size() != kWords || b.size() != kWords) Fail(name + ": result size");
  for (int w = 0; w < kWords; ++w) {
    const T want = Word<T>::Select(beta, db[static_cast<size_t>(alpha) * kWords + w]);
    if (!(a[w] + b[w] == want)) Fail(name + ": word " + std::to_string(w) + " does not reconstruct");
  }
  // A database one byte short is refused on the host.
  auto small = f->template EvaluateDot<T>(keys.first, 0, dev.p, bytes - 1, kWords);
  if (small.ok() || small.status().code() != dpf::StatusCode::kInvalidArgument)
    Fail(name + ": short database accepted");
  std::printf("ok %s\n", name.c_str());
}

void Uint32IsUnimplemented() {
  DpfParameters p;
  p.set_log_domain_size(kLog);
  *p.mutable_value_type() = dpf::ToValueType<uint32_t>();
  auto f = Must(DistributedPointFunction::Create(p), "Create uint32");
  auto keys = Must(f->GenerateKeys(uint128{5}, uint32_t{7}), "GenerateKeys uint32");
  DeviceDb dev;
  const int64_t bytes = (int64_t{1} << kLog) * 4;
  if (dpf_hip_alloc(&dev.p, bytes) != 0) Fail("dpf_hip_alloc");
  auto r = f->EvaluateDot<uint32_t>(keys.first, 0, dev.p, bytes, 1);
  if (r.ok()) Fail("uint32_t: EvaluateDot succeeded");
  if (r.status().code() != dpf::StatusCode::kUnimplemented)
    Fail("uint32_t: " + r.status().ToString());
  std::printf("ok uint32_t UNIMPLEMENTED\n");
}

}  // namespace

int main() {
  Reconstructs<uint64_t>("uint64_t");
  Reconstructs<dpf::XorWrapper<uint128>>("XorWrapper<uint128>");
  Uint32IsUnimplemented();
  std::printf("ALL OK\n");
  return 0;
}
