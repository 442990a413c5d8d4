// keygen_api_test.cc -- batched key generation on the device through the public
// headers only: DistributedPointFunction::GenerateKeyBatchToDevice,
// DistributedComparisonFunction::GenerateKeyBatchToDevice and
// MultipleIntervalContainmentGate::GenBatchToDevice, each downloaded
// (DeviceKeyBatch::Download) and compared row by row with the single-key
// ...WithSeeds call for the same root seeds; SerializeKeyBatch then
// ParseKeyBatch of a downloaded batch gives the batch back; and two host
// errors are reported before the device is touched.
//
// Exit status 0 and "ALL OK" on success; the first mismatch is printed.
// Run by tests/test_keygen_cpp_gpu.py; built by build_native.build_tools.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <string_view>
#include <vector>

#include "dcf/distributed_comparison_function.h"
#include "dcf/fss_gates/multiple_interval_containment.h"
#include "dpf/distributed_point_function.h"
#include "dpf/key_batch.h"

namespace dpf = distributed_point_functions;
using dpf::DistributedPointFunction;
using dpf::DpfParameters;
using dpf::KeyBatch;
using dpf::uint128;
using dpf::Value;

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

template <typename V>
bool SameBytes(const std::vector<V>& a, const std::vector<V>& b) {
  return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(V)));
}

void ExpectEqual(const KeyBatch& a, const KeyBatch& b, const std::string& what) {
  if (a.num_keys != b.num_keys || a.num_levels != b.num_levels) Fail(what + ": shape");
  if (!SameBytes(a.seed, b.seed)) Fail(what + ": seed");
  if (!SameBytes(a.party, b.party)) Fail(what + ": party");
  if (!SameBytes(a.cw_seed, b.cw_seed)) Fail(what + ": cw_seed");
  if (!SameBytes(a.cw_left, b.cw_left)) Fail(what + ": cw_left");
  if (!SameBytes(a.cw_right, b.cw_right)) Fail(what + ": cw_right");
  if (a.value_correction.size() != b.value_correction.size()) Fail(what + ": hierarchy levels");
  for (size_t h = 0; h < a.value_correction.size(); ++h)
    if (!SameBytes(a.value_correction[h], b.value_correction[h]))
      Fail(what + ": value correction " + std::to_string(h));
}

constexpr int kKeys = 70;

std::vector<uint128> Random128(std::mt19937_64& rng, int n, int bits) {
  std::vector<uint128> v(n);
  for (auto& x : v) {
    x = dpf::MakeUint128(rng(), rng());
    if (bits < 128) x &= (uint128{1} << bits) - 1;
  }
  return v;
}

}  // namespace

int main() {
  std::mt19937_64 rng(7);
  const std::vector<uint128> seeds = Random128(rng, 2 * kKeys, 128);

  // ---- DPF: a two-level uint32 / uint64 hierarchy, one beta per key and level.
  std::vector<DpfParameters> params(2);
  params[0].set_log_domain_size(5);
  *params[0].mutable_value_type() = dpf::ToValueType<uint32_t>();
  params[1].set_log_domain_size(40);
  *params[1].mutable_value_type() = dpf::ToValueType<uint64_t>();
  auto d = Must(DistributedPointFunction::CreateIncremental(dpf::MakeConstSpan(params)), "create");
  if (!d->GeneratesKeysOnDevice()) Fail("integer hierarchy should generate on the device");
  const std::vector<uint128> alphas = Random128(rng, kKeys, 40);
  std::vector<Value> betas;
  for (int k = 0; k < kKeys; ++k) {
    betas.push_back(Must(d->ToValue<uint32_t>(static_cast<uint32_t>(rng())), "beta"));
    betas.push_back(Must(d->ToValue<uint64_t>(rng()), "beta"));
  }
  auto dev = Must(d->GenerateKeyBatchToDevice(dpf::MakeConstSpan(alphas), dpf::MakeConstSpan(betas),
                                              dpf::MakeConstSpan(seeds), nullptr),
                  "GenerateKeyBatchToDevice");
  const KeyBatch got[2] = {Must(dev.first->Download(nullptr), "download"),
                           Must(dev.second->Download(nullptr), "download")};
  std::vector<dpf::DpfKey> single[2];
  for (int k = 0; k < kKeys; ++k) {
    auto pair = Must(d->GenerateKeysIncrementalWithSeeds(
                         alphas[k], dpf::Span<const Value>(&betas[2 * k], 2), seeds[2 * k],
                         seeds[2 * k + 1]),
                     "GenerateKeysIncrementalWithSeeds");
    single[0].push_back(std::move(pair.first));
    single[1].push_back(std::move(pair.second));
  }
  for (int p = 0; p < 2; ++p) {
    std::vector<const dpf::DpfKey*> ptrs;
    for (const auto& k : single[p]) ptrs.push_back(&k);
    ExpectEqual(got[p], Must(d->MakeKeyBatch(dpf::MakeConstSpan(ptrs)), "MakeKeyBatch"),
                "DPF party " + std::to_string(p));
    // The dealer's path: serialize the downloaded batch, parse it back.
    const std::vector<std::string> wire = Must(d->SerializeKeyBatch(got[p]), "SerializeKeyBatch");
    for (int k = 0; k < kKeys; ++k)
      if (wire[k] != single[p][k].SerializeAsString()) Fail("serialized key " + std::to_string(k));
    std::vector<std::string_view> views(wire.begin(), wire.end());
    ExpectEqual(Must(d->ParseKeyBatch(dpf::MakeConstSpan(views)), "ParseKeyBatch"), got[p],
                "round trip party " + std::to_string(p));
  }
  // Shared betas: H values for all keys.
  {
    auto shared = Must(d->GenerateKeyBatchToDevice(dpf::MakeConstSpan(alphas),
                                                   dpf::Span<const Value>(betas.data(), 2),
                                                   dpf::MakeConstSpan(seeds), nullptr),
                       "GenerateKeyBatchToDevice shared");
    auto host = Must(d->GenerateKeyBatch(dpf::MakeConstSpan(alphas),
                                         dpf::Span<const Value>(betas.data(), 2),
                                         dpf::MakeConstSpan(seeds)),
                     "GenerateKeyBatch");
    ExpectEqual(Must(shared.first->Download(nullptr), "download"), host.first, "shared party 0");
    ExpectEqual(Must(shared.second->Download(nullptr), "download"), host.second, "shared party 1");
  }
  // Two host errors, GenerateKeyBatch's.
  {
    std::vector<uint128> bad = alphas;
    bad[3] = uint128{1} << 40;
    auto r = d->GenerateKeyBatchToDevice(dpf::MakeConstSpan(bad), dpf::MakeConstSpan(betas),
                                         dpf::MakeConstSpan(seeds), nullptr);
    if (r.ok() || r.status().message() != "`alpha` must be smaller than the output domain size")
      Fail("alpha out of range: " + r.status().ToString());
    auto r2 = d->GenerateKeyBatchToDevice(dpf::MakeConstSpan(alphas), dpf::MakeConstSpan(betas),
                                          dpf::Span<const uint128>(seeds.data(), 3), nullptr);
    if (r2.ok() || r2.status().message() != "root_seeds must be empty or hold two seeds per alpha")
      Fail("root_seeds size: " + r2.status().ToString());
  }

  // ---- DCF over 24 bits, uint64, one beta per key.
  {
    dpf::DcfParameters dp;
    dp.mutable_parameters()->set_log_domain_size(24);
    *dp.mutable_parameters()->mutable_value_type() = dpf::ToValueType<uint64_t>();
    auto dcf = Must(dpf::DistributedComparisonFunction::Create(dp), "dcf create");
    const std::vector<uint128> a = Random128(rng, kKeys, 24);
    std::vector<Value> b;
    for (int k = 0; k < kKeys; ++k) b.push_back(dpf::ToValue<uint64_t>(rng()));
    auto pair = Must(dcf->GenerateKeyBatchToDevice(dpf::MakeConstSpan(a), dpf::MakeConstSpan(b),
                                                   dpf::MakeConstSpan(seeds), nullptr),
                     "dcf GenerateKeyBatchToDevice");
    std::vector<dpf::DcfKey> keys[2];
    for (int k = 0; k < kKeys; ++k) {
      auto one = Must(dcf->GenerateKeysWithSeeds(a[k], b[k], seeds[2 * k], seeds[2 * k + 1]),
                      "GenerateKeysWithSeeds");
      keys[0].push_back(std::move(one.first));
      keys[1].push_back(std::move(one.second));
    }
    for (int p = 0; p < 2; ++p) {
      std::vector<const dpf::DcfKey*> ptrs;
      for (const auto& k : keys[p]) ptrs.push_back(&k);
      const KeyBatch down = Must((p ? pair.second : pair.first)->Download(nullptr), "download");
      ExpectEqual(down, Must(dcf->MakeKeyBatch(dpf::MakeConstSpan(ptrs)), "dcf MakeKeyBatch"),
                  "DCF party " + std::to_string(p));
    }
  }

  // ---- MIC gate over Z_2^20, three intervals.
  {
    namespace fg = dpf::fss_gates;
    fg::MicParameters mp;
    mp.set_log_group_size(20);
    const uint64_t bounds[3][2] = {{0, 9}, {100, 5000}, {(1u << 20) - 2, (1u << 20) - 1}};
    for (const auto& iv : bounds) {
      fg::Interval* i = mp.add_intervals();
      i->mutable_lower_bound()->mutable_value_uint128()->set_low(iv[0]);
      i->mutable_upper_bound()->mutable_value_uint128()->set_low(iv[1]);
    }
    auto gate = Must(fg::MultipleIntervalContainmentGate::Create(mp), "mic create");
    const std::vector<uint128> r_in = Random128(rng, kKeys, 20);
    const std::vector<uint128> r_out = Random128(rng, 3 * kKeys, 20);
    const std::vector<uint128> z_0 = Random128(rng, 3 * kKeys, 20);
    auto pair = Must(gate->GenBatchToDevice(dpf::MakeConstSpan(r_in), dpf::MakeConstSpan(r_out),
                                            dpf::MakeConstSpan(seeds), dpf::MakeConstSpan(z_0),
                                            nullptr),
                     "GenBatchToDevice");
    std::vector<fg::MicKey> keys[2];
    for (int k = 0; k < kKeys; ++k) {
      auto one = Must(gate->GenWithSeeds(r_in[k],
                                         std::vector<uint128>(r_out.begin() + 3 * k,
                                                              r_out.begin() + 3 * k + 3),
                                         seeds[2 * k], seeds[2 * k + 1],
                                         dpf::Span<const uint128>(&z_0[3 * k], 3)),
                      "GenWithSeeds");
      keys[0].push_back(std::move(one.first));
      keys[1].push_back(std::move(one.second));
    }
    for (int p = 0; p < 2; ++p) {
      std::vector<const fg::MicKey*> ptrs;
      for (const auto& k : keys[p]) ptrs.push_back(&k);
      const fg::MicKeyBatch want = Must(gate->MakeKeyBatch(dpf::MakeConstSpan(ptrs)), "mic batch");
      const fg::MicKeyBatch down = Must((p ? pair.second : pair.first)->Download(nullptr), "download");
      ExpectEqual(down.dcf, want.dcf, "MIC party " + std::to_string(p));
      if (down.num_intervals != 3 || !SameBytes(down.mask_share, want.mask_share))
        Fail("MIC mask shares party " + std::to_string(p));
    }
  }
  std::printf("ALL OK\n");
  return 0;
}
