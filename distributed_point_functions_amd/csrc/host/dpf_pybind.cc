// dpf_pybind.cc -- Python binding of the host C++ DistributedPointFunction.
// Protos cross the boundary as serialized bytes (the reference's wire format);
// 128-bit integers as numpy uint64 arrays of shape (n, 2) = {low, high}.
// Errors raise _dpf_host.StatusError("<code>|<message>"); the Python wrapper
// (distributed_point_functions_amd/dpf.py) turns it into DpfStatusError.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "dcf/distributed_comparison_function.h"
#include "dcf/fss_gates/multiple_interval_containment.h"
#include "dpf/distributed_point_function.h"
#include "synthetic_data_benchmarks.h"

namespace py = pybind11;
using namespace distributed_point_functions;
using fss_gates::DeviceMicKeyBatch;
using fss_gates::MicKey;
using fss_gates::MicKeyBatch;
using fss_gates::MicParameters;
using fss_gates::MultipleIntervalContainmentGate;

namespace {

struct StatusError : std::exception {
  std::string what_;
  explicit StatusError(const Status& s) : what_(std::to_string(s.raw_code()) + "|" + s.message()) {}
  const char* what() const noexcept override { return what_.c_str(); }
};

void Check(const Status& s) {
  if (!s.ok()) throw StatusError(s);
}
template <typename T>
T Take(StatusOr<T> s) {
  if (!s.ok()) throw StatusError(s.status());
  return std::move(*s);
}

template <typename M>
M Parse(const py::bytes& b) {
  M m;
  std::string s = b;
  if (!m.ParseFromString(s)) throw StatusError(InvalidArgumentError("failed to parse proto bytes"));
  return m;
}
template <typename M>
py::bytes Ser(const M& m) {
  return py::bytes(m.SerializeAsString());
}

std::vector<uint128> ToU128(const py::array_t<uint64_t, py::array::c_style | py::array::forcecast>& a) {
  if (a.size() == 0) return {};
  if (a.ndim() != 2 || a.shape(1) != 2) throw std::invalid_argument("expected uint64 array (n, 2)");
  std::vector<uint128> r(a.shape(0));
  auto v = a.unchecked<2>();
  for (py::ssize_t i = 0; i < a.shape(0); ++i) r[i] = MakeUint128(v(i, 1), v(i, 0));
  return r;
}

uint128 IntToU128(const py::int_& x) {
  py::int_ mask((1ULL << 63) * 2 - 1);  // 2^64 - 1 via unsigned wrap
  uint64_t lo = PyLong_AsUnsignedLongLongMask(x.ptr());
  py::object hi_o = x.attr("__rshift__")(64);
  uint64_t hi = PyLong_AsUnsignedLongLongMask(hi_o.ptr());
  return MakeUint128(hi, lo);
}

// The result vector itself becomes the numpy array's storage (no copy: a
// multi-GiB output would otherwise be faulted in and copied on one thread).
py::array_t<uint8_t> ToArray(std::vector<uint8_t>&& v) {
  auto* owned = new std::vector<uint8_t>(std::move(v));
  py::capsule free_when_done(owned, [](void* p) { delete static_cast<std::vector<uint8_t>*>(p); });
  return py::array_t<uint8_t>({static_cast<py::ssize_t>(owned->size())}, {py::ssize_t{1}},
                              owned->data(), free_when_done);
}

std::unique_ptr<ValueType> OptType(const py::object& o) {
  if (o.is_none()) return nullptr;
  return std::make_unique<ValueType>(Parse<ValueType>(o.cast<py::bytes>()));
}

struct PyKeyBatch {
  std::shared_ptr<KeyBatch> b;
  int64_t NumKeys() const { return b->num_keys; }
  int NumLevels() const { return b->num_levels; }
  py::array_t<uint64_t> Seeds() const {
    py::array_t<uint64_t> a({static_cast<py::ssize_t>(b->num_keys), py::ssize_t{2}});
    if (b->num_keys) std::memcpy(a.mutable_data(), b->seed.data(), b->num_keys * 16);
    return a;
  }
  py::array_t<uint8_t> Party() const {
    py::array_t<uint8_t> a(static_cast<py::ssize_t>(b->num_keys));
    if (b->num_keys) std::memcpy(a.mutable_data(), b->party.data(), b->num_keys);
    return a;
  }
  // The correction words, [key][level]: seeds as {low, high}, control bytes.
  py::array_t<uint64_t> CwSeeds() const { return Blocks(b->cw_seed); }
  py::array_t<uint8_t> CwLeft() const { return Bytes(b->cw_left); }
  py::array_t<uint8_t> CwRight() const { return Bytes(b->cw_right); }
  int NumHierarchyLevels() const { return static_cast<int>(b->value_correction.size()); }
  // Level h's value corrections, [key][element * leaf] as {low, high}.
  py::array_t<uint64_t> ValueCorrection(int h) const {
    if (h < 0 || h >= NumHierarchyLevels()) throw std::invalid_argument("hierarchy level out of range");
    return Blocks(b->value_correction[h]);
  }
  static py::array_t<uint64_t> Blocks(const std::vector<dpf_block>& v) {
    py::array_t<uint64_t> a({static_cast<py::ssize_t>(v.size()), py::ssize_t{2}});
    if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * 16);
    return a;
  }
  static py::array_t<uint8_t> Bytes(const std::vector<uint8_t>& v) {
    py::array_t<uint8_t> a(static_cast<py::ssize_t>(v.size()));
    if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size());
    return a;
  }
};

struct PyDeviceKeyBatch {
  std::shared_ptr<DeviceKeyBatch> d;
  int64_t NumKeys() const { return d->num_keys(); }
  int64_t FirstKey() const { return d->first_key(); }
  PyKeyBatch Download(uintptr_t stream) const {
    py::gil_scoped_release nogil;
    auto r = d->Download(reinterpret_cast<void*>(stream));
    if (!r.ok()) {
      py::gil_scoped_acquire g;
      throw StatusError(r.status());
    }
    return PyKeyBatch{std::make_shared<KeyBatch>(std::move(*r))};
  }
};

using U64Array = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>;
std::vector<uint128> OptU128(const py::object& o) {
  if (o.is_none()) return {};
  return ToU128(o.cast<U64Array>());
}
py::tuple DevicePair(DistributedPointFunction::DeviceKeyBatchPair&& r) {
  return py::make_tuple(PyDeviceKeyBatch{std::shared_ptr<DeviceKeyBatch>(r.first.release())},
                        PyDeviceKeyBatch{std::shared_ptr<DeviceKeyBatch>(r.second.release())});
}
py::tuple HostPair(std::pair<KeyBatch, KeyBatch>&& r) {
  return py::make_tuple(PyKeyBatch{std::make_shared<KeyBatch>(std::move(r.first))},
                        PyKeyBatch{std::make_shared<KeyBatch>(std::move(r.second))});
}
// Runs f() without the GIL and unwraps its StatusOr.
template <typename F>
auto TakeNoGil(F f) {
  py::gil_scoped_release nogil;
  auto r = f();
  if (!r.ok()) {
    py::gil_scoped_acquire g;
    throw StatusError(r.status());
  }
  return std::move(*r);
}

// Holds the device key batch alive as long as its context.
struct PyBatchContext {
  std::shared_ptr<DeviceKeyBatch> keys;
  std::shared_ptr<DeviceBatchContext> ctx;
  int PreviousHierarchyLevel() const { return ctx->previous_hierarchy_level(); }
  int PartialEvaluationsLevel() const { return ctx->partial_evaluations_level(); }
  int ExpansionCacheLevel() const { return ctx->expansion_cache_level(); }
  int64_t NumPartialEvaluations() const {
    return static_cast<int64_t>(ctx->partial_prefixes().size());
  }
};

class PyDpf {
 public:
  static PyDpf CreateIncremental(const std::vector<py::bytes>& params) {
    std::vector<DpfParameters> p;
    for (const auto& b : params) p.push_back(Parse<DpfParameters>(b));
    PyDpf r;
    r.dpf_ = std::shared_ptr<DistributedPointFunction>(
        Take(DistributedPointFunction::CreateIncremental(MakeConstSpan(p))).release());
    return r;
  }
  void RegisterValueType(const py::bytes& vt) { Check(dpf_->RegisterValueType(Parse<ValueType>(vt))); }
  py::tuple GenerateKeys(const py::int_& alpha, const std::vector<py::bytes>& betas) {
    std::vector<Value> v;
    for (const auto& b : betas) v.push_back(Parse<Value>(b));
    auto keys = Take(dpf_->GenerateKeysIncremental(IntToU128(alpha), MakeConstSpan(v)));
    return py::make_tuple(Ser(keys.first), Ser(keys.second));
  }
  py::tuple GenerateKeysWithSeeds(const py::int_& alpha, const std::vector<py::bytes>& betas,
                                  const py::int_& s0, const py::int_& s1) {
    std::vector<Value> v;
    for (const auto& b : betas) v.push_back(Parse<Value>(b));
    auto keys = Take(dpf_->GenerateKeysIncrementalWithSeeds(IntToU128(alpha), MakeConstSpan(v),
                                                            IntToU128(s0), IntToU128(s1)));
    return py::make_tuple(Ser(keys.first), Ser(keys.second));
  }
  // API-level timing of the drop-in EvaluateUntil<T>(level, {}, ctx) that
  // returns std::vector<T> in host memory (uint64_t or absl::uint128 by
  // `bits`): `reps` calls on fresh copies of ctx, wall seconds each (the
  // vector's allocation, the kernel and the D2H copy included; freeing the
  // previous vector is not).  Returns (seconds list, elements, sample of the
  // last output: (index, low, high) at `probe` positions).
  py::tuple TimeEvaluateUntil(int level, const py::bytes& ctx_bytes, int bits, int reps,
                              const std::vector<int64_t>& probe) {
    const EvaluationContext ctx0 = Parse<EvaluationContext>(ctx_bytes);
    std::vector<double> secs;
    int64_t n = 0;
    std::vector<py::tuple> samples;
    auto run = [&](auto tag) {
      using T = decltype(tag);
      std::vector<T> out;
      for (int r = 0; r < reps; ++r) {
        EvaluationContext ctx = ctx0;
        out = std::vector<T>();  // free before the timed call
        const auto t0 = std::chrono::steady_clock::now();
        {
          py::gil_scoped_release nogil;
          out = Take(dpf_->EvaluateUntil<T>(level, {}, ctx));
        }
        secs.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
      }
      n = static_cast<int64_t>(out.size());
      for (int64_t i : probe)
        if (i >= 0 && i < n)
          samples.push_back(py::make_tuple(i, static_cast<uint64_t>(out[i]),
                                           static_cast<uint64_t>(uint128(out[i]) >> 64)));
    };
    if (bits == 64) run(uint64_t{});
    else if (bits == 128) run(uint128{});
    else throw StatusError(InvalidArgumentError("bits must be 64 or 128"));
    return py::make_tuple(secs, n, samples);
  }
  py::bytes CreateEvaluationContext(const py::bytes& key) {
    return Ser(Take(dpf_->CreateEvaluationContext(Parse<DpfKey>(key))));
  }
  py::tuple EvaluateUntil(int level, const py::array_t<uint64_t, py::array::c_style | py::array::forcecast>& prefixes,
                          const py::bytes& ctx_bytes, const py::object& vt) {
    EvaluationContext ctx = Parse<EvaluationContext>(ctx_bytes);
    auto p = ToU128(prefixes);
    auto t = OptType(vt);
    std::vector<uint8_t> out;
    {
      py::gil_scoped_release nogil;
      auto r = dpf_->EvaluateUntilPacked(level, MakeConstSpan(p), ctx, t.get());
      if (!r.ok()) {
        py::gil_scoped_acquire g;
        throw StatusError(r.status());
      }
      out = std::move(*r);
    }
    return py::make_tuple(ToArray(std::move(out)), Ser(ctx));
  }
  py::tuple EvaluateUntilToDevice(int level,
                                  const py::array_t<uint64_t, py::array::c_style | py::array::forcecast>& prefixes,
                                  const py::bytes& ctx_bytes, uintptr_t out_ptr, int64_t capacity,
                                  uintptr_t stream, const py::object& vt) {
    EvaluationContext ctx = Parse<EvaluationContext>(ctx_bytes);
    auto p = ToU128(prefixes);
    auto t = OptType(vt);
    int64_t n = 0;
    {
      py::gil_scoped_release nogil;
      auto r = dpf_->EvaluateUntilToDevice(level, MakeConstSpan(p), ctx, reinterpret_cast<void*>(out_ptr),
                                           capacity, reinterpret_cast<void*>(stream), t.get());
      if (!r.ok()) {
        py::gil_scoped_acquire g;
        throw StatusError(r.status());
      }
      n = *r;
    }
    return py::make_tuple(n, Ser(ctx));
  }
  py::tuple EvaluateShardToDevice(int level, int64_t shard, int64_t num_shards,
                                  const py::bytes& ctx_bytes, uintptr_t out_ptr, int64_t capacity,
                                  uintptr_t stream) {
    EvaluationContext ctx = Parse<EvaluationContext>(ctx_bytes);
    int64_t n = 0;
    {
      py::gil_scoped_release nogil;
      auto r = dpf_->EvaluateShardToDevice(level, shard, num_shards, ctx,
                                           reinterpret_cast<void*>(out_ptr), capacity,
                                           reinterpret_cast<void*>(stream));
      if (!r.ok()) {
        py::gil_scoped_acquire g;
        throw StatusError(r.status());
      }
      n = *r;
    }
    return py::make_tuple(n, Ser(ctx));
  }
  int64_t EvaluateDotToDevice(const py::bytes& key_bytes, int level, int64_t shard,
                              int64_t num_shards, uintptr_t db_ptr, int64_t db_bytes,
                              int64_t record_words, uintptr_t out_ptr, int64_t out_bytes,
                              uintptr_t stream) {
    DpfKey key = Parse<DpfKey>(key_bytes);
    py::gil_scoped_release nogil;
    auto r = dpf_->EvaluateDotToDevice(key, level, shard, num_shards,
                                       reinterpret_cast<const void*>(db_ptr), db_bytes,
                                       record_words, reinterpret_cast<void*>(out_ptr), out_bytes,
                                       reinterpret_cast<void*>(stream));
    if (!r.ok()) {
      py::gil_scoped_acquire g;
      throw StatusError(r.status());
    }
    return *r;
  }
  py::array_t<uint8_t> EvaluateDot(const py::bytes& key_bytes, int level, uintptr_t db_ptr,
                                   int64_t db_bytes, int64_t record_words) {
    DpfKey key = Parse<DpfKey>(key_bytes);
    std::vector<uint8_t> out;
    {
      py::gil_scoped_release nogil;
      auto r = dpf_->EvaluateDotPacked(key, level, reinterpret_cast<const void*>(db_ptr), db_bytes,
                                       record_words);
      if (!r.ok()) {
        py::gil_scoped_acquire g;
        throw StatusError(r.status());
      }
      out = std::move(*r);
    }
    py::array_t<uint8_t> a(static_cast<py::ssize_t>(out.size()));
    if (!out.empty()) std::memcpy(a.mutable_data(), out.data(), out.size());
    return a;
  }
  int64_t EvaluateSelectToDevice(const std::vector<py::bytes>& key_bytes, int level, int64_t shard,
                                 int64_t num_shards, uintptr_t db_ptr, int64_t db_bytes,
                                 int64_t record_words, uintptr_t out_ptr, int64_t out_bytes,
                                 uintptr_t stream) {
    std::vector<DpfKey> keys;
    for (const auto& b : key_bytes) keys.push_back(Parse<DpfKey>(b));
    std::vector<const DpfKey*> ptrs;
    for (const auto& k : keys) ptrs.push_back(&k);
    py::gil_scoped_release nogil;
    auto r = dpf_->EvaluateSelectToDevice(MakeConstSpan(ptrs), level, shard, num_shards,
                                          reinterpret_cast<const void*>(db_ptr), db_bytes,
                                          record_words, reinterpret_cast<void*>(out_ptr),
                                          out_bytes, reinterpret_cast<void*>(stream));
    if (!r.ok()) {
      py::gil_scoped_acquire g;
      throw StatusError(r.status());
    }
    return *r;
  }
  py::array_t<uint64_t> EvaluateSelect(const std::vector<py::bytes>& key_bytes, int level,
                                       uintptr_t db_ptr, int64_t db_bytes, int64_t record_words) {
    std::vector<DpfKey> keys;
    for (const auto& b : key_bytes) keys.push_back(Parse<DpfKey>(b));
    std::vector<const DpfKey*> ptrs;
    for (const auto& k : keys) ptrs.push_back(&k);
    std::vector<uint64_t> out;
    {
      py::gil_scoped_release nogil;
      auto r = dpf_->EvaluateSelect(MakeConstSpan(ptrs), level,
                                    reinterpret_cast<const void*>(db_ptr), db_bytes, record_words);
      if (!r.ok()) {
        py::gil_scoped_acquire g;
        throw StatusError(r.status());
      }
      out = std::move(*r);
    }
    py::array_t<uint64_t> a({static_cast<py::ssize_t>(keys.size()),
                             static_cast<py::ssize_t>(record_words)});
    if (!out.empty()) std::memcpy(a.mutable_data(), out.data(), out.size() * 8);
    return a;
  }
  int64_t EvaluateDotBatchToDevice(const std::vector<py::bytes>& key_bytes, int level,
                                   int64_t shard, int64_t num_shards, uintptr_t db_ptr,
                                   int64_t db_bytes, int64_t record_words, uintptr_t out_ptr,
                                   int64_t out_bytes, uintptr_t stream) {
    std::vector<DpfKey> keys;
    for (const auto& b : key_bytes) keys.push_back(Parse<DpfKey>(b));
    std::vector<const DpfKey*> ptrs;
    for (const auto& k : keys) ptrs.push_back(&k);
    py::gil_scoped_release nogil;
    auto r = dpf_->EvaluateDotBatchToDevice(MakeConstSpan(ptrs), level, shard, num_shards,
                                            reinterpret_cast<const void*>(db_ptr), db_bytes,
                                            record_words, reinterpret_cast<void*>(out_ptr),
                                            out_bytes, reinterpret_cast<void*>(stream));
    if (!r.ok()) {
      py::gil_scoped_acquire g;
      throw StatusError(r.status());
    }
    return *r;
  }
  py::array_t<uint64_t> EvaluateDotBatch(const std::vector<py::bytes>& key_bytes, int level,
                                         uintptr_t db_ptr, int64_t db_bytes,
                                         int64_t record_words) {
    std::vector<DpfKey> keys;
    for (const auto& b : key_bytes) keys.push_back(Parse<DpfKey>(b));
    std::vector<const DpfKey*> ptrs;
    for (const auto& k : keys) ptrs.push_back(&k);
    std::vector<uint64_t> out;
    {
      py::gil_scoped_release nogil;
      auto r = dpf_->EvaluateDotBatch(MakeConstSpan(ptrs), level,
                                      reinterpret_cast<const void*>(db_ptr), db_bytes,
                                      record_words);
      if (!r.ok()) {
        py::gil_scoped_acquire g;
        throw StatusError(r.status());
      }
      out = std::move(*r);
    }
    py::array_t<uint64_t> a({static_cast<py::ssize_t>(keys.size()),
                             static_cast<py::ssize_t>(record_words)});
    if (!out.empty()) std::memcpy(a.mutable_data(), out.data(), out.size() * 8);
    return a;
  }
  py::array_t<uint8_t> EvaluateAt(const py::bytes& key_bytes, int level,
                                  const py::array_t<uint64_t, py::array::c_style | py::array::forcecast>& points,
                                  const py::object& vt) {
    DpfKey key = Parse<DpfKey>(key_bytes);
    auto p = ToU128(points);
    auto t = OptType(vt);
    return ToArray(Take(dpf_->EvaluateAtPacked(key, level, MakeConstSpan(p), nullptr, t.get())));
  }
  py::tuple EvaluateAtCtx(int level,
                          const py::array_t<uint64_t, py::array::c_style | py::array::forcecast>& points,
                          const py::bytes& ctx_bytes, const py::object& vt) {
    EvaluationContext ctx = Parse<EvaluationContext>(ctx_bytes);
    auto p = ToU128(points);
    auto t = OptType(vt);
    auto out = Take(dpf_->EvaluateAtPacked(ctx.key(), level, MakeConstSpan(p), &ctx, t.get()));
    return py::make_tuple(ToArray(std::move(out)), Ser(ctx));
  }
  py::array_t<uint8_t> EvaluateAtBatch(const std::vector<py::bytes>& keys, int level,
                                       const py::array_t<uint64_t, py::array::c_style | py::array::forcecast>& points,
                                       int64_t points_per_key) {
    std::vector<DpfKey> k;
    k.reserve(keys.size());
    for (const auto& b : keys) k.push_back(Parse<DpfKey>(b));
    std::vector<const DpfKey*> ptrs;
    for (const auto& x : k) ptrs.push_back(&x);
    auto p = ToU128(points);
    return ToArray(Take(dpf_->EvaluateAtBatchPacked(MakeConstSpan(ptrs), level, MakeConstSpan(p),
                                                    points_per_key)));
  }
  PyKeyBatch MakeKeyBatch(const std::vector<py::bytes>& keys) {
    std::vector<DpfKey> k;
    k.reserve(keys.size());
    for (const auto& b : keys) k.push_back(Parse<DpfKey>(b));
    std::vector<const DpfKey*> ptrs;
    for (const auto& x : k) ptrs.push_back(&x);
    return PyKeyBatch{std::make_shared<KeyBatch>(Take(dpf_->MakeKeyBatch(MakeConstSpan(ptrs))))};
  }
  py::bytes KeyFromBatch(const PyKeyBatch& b, int64_t k) { return Ser(Take(dpf_->KeyFromBatch(*b.b, k))); }
  py::list SerializeKeyBatch(const PyKeyBatch& b, int threads) {
    StatusOr<std::vector<std::string>> r = InternalError("unset");
    {
      py::gil_scoped_release nogil;
      r = dpf_->SerializeKeyBatch(*b.b, threads);
    }
    std::vector<std::string> v = Take(std::move(r));
    py::list out(v.size());
    for (size_t i = 0; i < v.size(); ++i) out[i] = py::bytes(v[i]);
    return out;
  }
  PyKeyBatch ParseKeyBatch(const std::vector<py::bytes>& keys, int threads) {
    std::vector<std::string_view> views;
    views.reserve(keys.size());
    for (const auto& b : keys)
      views.emplace_back(PyBytes_AS_STRING(b.ptr()), static_cast<size_t>(PyBytes_GET_SIZE(b.ptr())));
    StatusOr<KeyBatch> r = InternalError("unset");
    {
      py::gil_scoped_release nogil;
      r = dpf_->ParseKeyBatch(Span<const std::string_view>(views), threads);
    }
    return PyKeyBatch{std::make_shared<KeyBatch>(Take(std::move(r)))};
  }
  py::tuple GenerateKeyBatch(const py::array_t<uint64_t, py::array::c_style | py::array::forcecast>& alphas,
                             const std::vector<py::bytes>& betas, const py::object& root_seeds,
                             int threads) {
    std::vector<Value> v;
    for (const auto& b : betas) v.push_back(Parse<Value>(b));
    auto a = ToU128(alphas);
    std::vector<uint128> seeds;
    if (!root_seeds.is_none())
      seeds = ToU128(root_seeds.cast<py::array_t<uint64_t, py::array::c_style | py::array::forcecast>>());
    std::pair<KeyBatch, KeyBatch> r;
    {
      py::gil_scoped_release nogil;
      auto s = dpf_->GenerateKeyBatch(MakeConstSpan(a), MakeConstSpan(v), MakeConstSpan(seeds), threads);
      if (!s.ok()) {
        py::gil_scoped_acquire g;
        throw StatusError(s.status());
      }
      r = std::move(*s);
    }
    return py::make_tuple(PyKeyBatch{std::make_shared<KeyBatch>(std::move(r.first))},
                          PyKeyBatch{std::make_shared<KeyBatch>(std::move(r.second))});
  }
  py::tuple GenerateKeyBatchWithBetas(const U64Array& alphas, const std::vector<py::bytes>& betas,
                                      const py::object& root_seeds, int threads) {
    std::vector<Value> v;
    for (const auto& b : betas) v.push_back(Parse<Value>(b));
    const auto a = ToU128(alphas);
    const auto seeds = OptU128(root_seeds);
    return HostPair(TakeNoGil([&] {
      return dpf_->GenerateKeyBatchWithBetas(MakeConstSpan(a), MakeConstSpan(v),
                                             MakeConstSpan(seeds), threads);
    }));
  }
  py::tuple GenerateKeyBatchToDevice(const U64Array& alphas, const std::vector<py::bytes>& betas,
                                     const py::object& root_seeds, uintptr_t stream) {
    std::vector<Value> v;
    for (const auto& b : betas) v.push_back(Parse<Value>(b));
    const auto a = ToU128(alphas);
    const auto seeds = OptU128(root_seeds);
    return DevicePair(TakeNoGil([&] {
      return dpf_->GenerateKeyBatchToDevice(MakeConstSpan(a), MakeConstSpan(v),
                                            MakeConstSpan(seeds), reinterpret_cast<void*>(stream));
    }));
  }
  bool GeneratesKeysOnDevice() const { return dpf_->GeneratesKeysOnDevice(); }
  int64_t EvaluateAtBatchToDevice(const PyDeviceKeyBatch& keys, int level, uintptr_t points,
                                  int64_t points_per_key, bool shared, uintptr_t out,
                                  int64_t capacity, uintptr_t stream) {
    py::gil_scoped_release nogil;
    auto r = dpf_->EvaluateAtBatchToDevice(*keys.d, level, reinterpret_cast<const void*>(points),
                                           points_per_key, shared, reinterpret_cast<void*>(out),
                                           capacity, reinterpret_cast<void*>(stream));
    if (!r.ok()) {
      py::gil_scoped_acquire g;
      throw StatusError(r.status());
    }
    return *r;
  }
  void EvaluateAtBatchSumToDevice(const PyDeviceKeyBatch& keys, int level, uintptr_t points,
                                  int64_t num_points, uintptr_t out, uintptr_t stream) {
    py::gil_scoped_release nogil;
    Status st = dpf_->EvaluateAtBatchSumToDevice(*keys.d, level, reinterpret_cast<const void*>(points),
                                                 num_points, reinterpret_cast<void*>(out),
                                                 reinterpret_cast<void*>(stream));
    if (!st.ok()) {
      py::gil_scoped_acquire g;
      throw StatusError(st);
    }
  }
  int64_t EvaluateLookupBatchToDevice(const PyDeviceKeyBatch& keys, int level, uintptr_t offsets,
                                      uintptr_t table, int64_t table_bytes, int64_t table_words,
                                      uintptr_t out, int64_t out_bytes, uintptr_t stream) {
    return TakeNoGil([&] {
      return dpf_->EvaluateLookupBatchToDevice(
          *keys.d, level, reinterpret_cast<const uint64_t*>(offsets),
          reinterpret_cast<const void*>(table), table_bytes, table_words,
          reinterpret_cast<void*>(out), out_bytes, reinterpret_cast<void*>(stream));
    });
  }
  py::array_t<uint64_t> EvaluateLookupBatch(const PyDeviceKeyBatch& keys, int level,
                                            const U64Array& offsets, uintptr_t table,
                                            int64_t table_bytes, int64_t table_words) {
    const std::vector<uint64_t> off(offsets.data(), offsets.data() + offsets.size());
    const std::vector<uint64_t> r = TakeNoGil([&] {
      return dpf_->EvaluateLookupBatch(*keys.d, level, MakeConstSpan(off),
                                       reinterpret_cast<const void*>(table), table_bytes,
                                       table_words);
    });
    py::array_t<uint64_t> a(static_cast<py::ssize_t>(r.size()));
    if (!r.empty()) std::memcpy(a.mutable_data(), r.data(), r.size() * 8);
    return a;
  }
  bool EvaluatesLookupOnDevice(int level) const { return dpf_->EvaluatesLookupOnDevice(level); }
  // The lookup call's host checks for a batch of `num_keys` keys (no device,
  // no batch object needed).
  void CheckLookupArgs(int64_t num_keys, bool batch_matches, int level, uintptr_t offsets,
                       uintptr_t table, int64_t table_bytes, int64_t table_words, uintptr_t out,
                       int64_t out_bytes) const {
    Status st = dpf_->CheckLookupArgs(num_keys, batch_matches, level,
                                      reinterpret_cast<const void*>(offsets),
                                      reinterpret_cast<const void*>(table), table_bytes,
                                      table_words, reinterpret_cast<const void*>(out), out_bytes);
    if (!st.ok()) throw StatusError(st);
  }
  int64_t EvaluateDotBucketsToDevice(const PyDeviceKeyBatch& keys, int level,
                                     const std::vector<int64_t>& bucket_begin, uintptr_t db,
                                     int64_t db_bytes, int64_t record_words, uintptr_t out,
                                     int64_t out_bytes, uintptr_t stream) {
    return TakeNoGil([&] {
      return dpf_->EvaluateDotBucketsToDevice(
          *keys.d, level, MakeConstSpan(bucket_begin), reinterpret_cast<const void*>(db), db_bytes,
          record_words, reinterpret_cast<void*>(out), out_bytes, reinterpret_cast<void*>(stream));
    });
  }
  py::array_t<uint64_t> EvaluateDotBuckets(const PyDeviceKeyBatch& keys, int level,
                                           const std::vector<int64_t>& bucket_begin, uintptr_t db,
                                           int64_t db_bytes, int64_t record_words) {
    const std::vector<uint64_t> r = TakeNoGil([&] {
      return dpf_->EvaluateDotBuckets(*keys.d, level, MakeConstSpan(bucket_begin),
                                      reinterpret_cast<const void*>(db), db_bytes, record_words);
    });
    py::array_t<uint64_t> a(static_cast<py::ssize_t>(r.size()));
    if (!r.empty()) std::memcpy(a.mutable_data(), r.data(), r.size() * 8);
    return a;
  }
  bool EvaluatesDotBucketsOnDevice(int level) const {
    return dpf_->EvaluatesDotBucketsOnDevice(level);
  }
  // The bucketed fold's host checks for a batch of `num_keys` keys (no device,
  // no batch object needed).
  void CheckDotBucketsArgs(int64_t num_keys, bool batch_matches, int level,
                           const std::vector<int64_t>& bucket_begin, uintptr_t db,
                           int64_t db_bytes, int64_t record_words, uintptr_t out,
                           int64_t out_bytes) const {
    Status st = dpf_->CheckDotBucketsArgs(num_keys, batch_matches, level,
                                          MakeConstSpan(bucket_begin),
                                          reinterpret_cast<const void*>(db), db_bytes,
                                          record_words, reinterpret_cast<const void*>(out),
                                          out_bytes);
    if (!st.ok()) throw StatusError(st);
  }
  int64_t EvaluateFullDomainSumToDevice(const PyDeviceKeyBatch& keys, int level, uintptr_t out,
                                        int64_t out_bytes, bool accumulate, uintptr_t stream) {
    return TakeNoGil([&] {
      return dpf_->EvaluateFullDomainSumToDevice(*keys.d, level, reinterpret_cast<void*>(out),
                                                 out_bytes, accumulate,
                                                 reinterpret_cast<void*>(stream));
    });
  }
  py::array_t<uint64_t> EvaluateFullDomainSum(const PyDeviceKeyBatch& keys, int level) {
    const std::vector<uint64_t> r =
        TakeNoGil([&] { return dpf_->EvaluateFullDomainSum(*keys.d, level); });
    py::array_t<uint64_t> a(static_cast<py::ssize_t>(r.size()));
    if (!r.empty()) std::memcpy(a.mutable_data(), r.data(), r.size() * 8);
    return a;
  }
  bool EvaluatesFullDomainSumOnDevice(int level) const {
    return dpf_->EvaluatesFullDomainSumOnDevice(level);
  }
  // The full-domain sum's host checks for a batch of `num_keys` keys (no
  // device, no batch object needed).
  void CheckFullDomainSumArgs(int64_t num_keys, bool batch_matches, int level, uintptr_t out,
                              int64_t out_bytes) const {
    Status st = dpf_->CheckFullDomainSumArgs(num_keys, batch_matches, level,
                                             reinterpret_cast<const void*>(out), out_bytes);
    if (!st.ok()) throw StatusError(st);
  }
  int64_t EvaluateFullDomainSumPackedToDevice(const PyDeviceKeyBatch& keys, int level,
                                              uintptr_t out, int64_t out_bytes, bool accumulate,
                                              uintptr_t stream) {
    return TakeNoGil([&] {
      return dpf_->EvaluateFullDomainSumPackedToDevice(*keys.d, level,
                                                       reinterpret_cast<void*>(out), out_bytes,
                                                       accumulate, reinterpret_cast<void*>(stream));
    });
  }
  // The N packed elements as bytes; dpf.py views them by the level's width.
  py::array_t<uint8_t> EvaluateFullDomainSumPacked(const PyDeviceKeyBatch& keys, int level) {
    const std::vector<uint8_t> r = TakeNoGil(
        [&] { return dpf_->EvaluateFullDomainSumPackedBytes(*keys.d, level, nullptr); });
    py::array_t<uint8_t> a(static_cast<py::ssize_t>(r.size()));
    if (!r.empty()) std::memcpy(a.mutable_data(), r.data(), r.size());
    return a;
  }
  bool EvaluatesFullDomainSumPackedOnDevice(int level) const {
    return dpf_->EvaluatesFullDomainSumPackedOnDevice(level);
  }
  // The packed full-domain sum's host checks for a batch of `num_keys` keys
  // (no device, no batch object needed).
  void CheckFullDomainSumPackedArgs(int64_t num_keys, bool batch_matches, int level,
                                    uintptr_t out, int64_t out_bytes) const {
    Status st = dpf_->CheckFullDomainSumPackedArgs(num_keys, batch_matches, level,
                                                   reinterpret_cast<const void*>(out), out_bytes);
    if (!st.ok()) throw StatusError(st);
  }
  int64_t EvaluateFullDomainSumSketchToDevice(int level, const PyDeviceKeyBatch& keys,
                                              uintptr_t weights, int num_weight_rows,
                                              uintptr_t sum, int64_t sum_bytes, uintptr_t sketch,
                                              int64_t sketch_bytes, bool accumulate,
                                              uintptr_t stream) {
    return TakeNoGil([&] {
      return dpf_->EvaluateFullDomainSumSketchToDevice(
          level, *keys.d, reinterpret_cast<const uint32_t*>(weights), num_weight_rows,
          reinterpret_cast<void*>(sum), sum_bytes, reinterpret_cast<void*>(sketch), sketch_bytes,
          accumulate, reinterpret_cast<void*>(stream));
    });
  }
  // (sums uint32 [N * nl], sketches uint32 [K * J * nl]); weights: J rows of N.
  py::tuple EvaluateFullDomainSumSketch(
      int level, const PyDeviceKeyBatch& keys,
      py::array_t<uint32_t, py::array::c_style | py::array::forcecast> weights,
      int num_weight_rows) {
    const Span<const uint32_t> w(weights.data(), static_cast<size_t>(weights.size()));
    const DistributedPointFunction::SumSketch r = TakeNoGil(
        [&] { return dpf_->EvaluateFullDomainSumSketch(level, *keys.d, w, num_weight_rows); });
    py::array_t<uint32_t> a(static_cast<py::ssize_t>(r.sum.size()));
    py::array_t<uint32_t> b(static_cast<py::ssize_t>(r.sketch.size()));
    if (!r.sum.empty()) std::memcpy(a.mutable_data(), r.sum.data(), r.sum.size() * 4);
    if (!r.sketch.empty()) std::memcpy(b.mutable_data(), r.sketch.data(), r.sketch.size() * 4);
    return py::make_tuple(a, b);
  }
  bool EvaluatesFullDomainSumSketchOnDevice(int level) const {
    return dpf_->EvaluatesFullDomainSumSketchOnDevice(level);
  }
  // The checked full-domain sum's host checks for a batch of `num_keys` keys
  // (no device, no batch object needed).
  void CheckFullDomainSumSketchArgs(int64_t num_keys, bool batch_matches, int level,
                                    uintptr_t weights, int num_weight_rows, uintptr_t sum,
                                    int64_t sum_bytes, uintptr_t sketch,
                                    int64_t sketch_bytes) const {
    Status st = dpf_->CheckFullDomainSumSketchArgs(
        num_keys, batch_matches, level, reinterpret_cast<const void*>(weights), num_weight_rows,
        reinterpret_cast<const void*>(sum), sum_bytes, reinterpret_cast<const void*>(sketch),
        sketch_bytes);
    if (!st.ok()) throw StatusError(st);
  }
  PyBatchContext CreateBatchEvaluationContext(const PyDeviceKeyBatch& keys) {
    auto c = Take(dpf_->CreateBatchEvaluationContext(*keys.d));
    return PyBatchContext{keys.d, std::shared_ptr<DeviceBatchContext>(c.release())};
  }
  int64_t EvaluateUntilBatchToDevice(int level,
                                     const py::array_t<uint64_t, py::array::c_style | py::array::forcecast>& prefixes,
                                     PyBatchContext& ctx, bool sum, uintptr_t out, int64_t capacity,
                                     uintptr_t stream) {
    auto p = ToU128(prefixes);
    py::gil_scoped_release nogil;
    auto r = sum ? dpf_->EvaluateUntilBatchSumToDevice(level, MakeConstSpan(p), *ctx.ctx,
                                                       reinterpret_cast<void*>(out), capacity,
                                                       reinterpret_cast<void*>(stream))
                 : dpf_->EvaluateUntilBatchToDevice(level, MakeConstSpan(p), *ctx.ctx,
                                                    reinterpret_cast<void*>(out), capacity,
                                                    reinterpret_cast<void*>(stream));
    if (!r.ok()) {
      py::gil_scoped_acquire g;
      throw StatusError(r.status());
    }
    return *r;
  }
  int64_t EvaluateUntilBatchSketchToDevice(
      int level, const py::array_t<uint64_t, py::array::c_style | py::array::forcecast>& prefixes,
      PyBatchContext& ctx, uintptr_t weights, int weight_rows, int64_t weights_per_row,
      uintptr_t sums, int64_t sums_capacity, uintptr_t sketch, int64_t sketch_capacity,
      uintptr_t stream) {
    auto p = ToU128(prefixes);
    py::gil_scoped_release nogil;
    auto r = dpf_->EvaluateUntilBatchSketchToDevice(
        level, MakeConstSpan(p), *ctx.ctx, reinterpret_cast<const uint32_t*>(weights), weight_rows,
        weights_per_row, reinterpret_cast<void*>(sums), sums_capacity,
        reinterpret_cast<uint32_t*>(sketch), sketch_capacity, reinterpret_cast<void*>(stream));
    if (!r.ok()) {
      py::gil_scoped_acquire g;
      throw StatusError(r.status());
    }
    return *r;
  }
  py::bytes ExportEvaluationContext(const PyBatchContext& ctx, const PyKeyBatch& host, int64_t k,
                                    uintptr_t stream) {
    return Ser(Take(dpf_->ExportEvaluationContext(*ctx.ctx, *host.b, k,
                                                  reinterpret_cast<void*>(stream))));
  }
  py::array_t<uint8_t> SumPackedShares(int level, const py::array_t<uint8_t, py::array::c_style>& shares,
                                       int64_t num_shares, int64_t count) {
    if (static_cast<int64_t>(shares.size()) != num_shares * count * dpf_->flat_value_type(level).packed_size)
      throw StatusError(InvalidArgumentError("shares has the wrong size"));
    return ToArray(Take(dpf_->SumPackedShares(level, shares.data(), num_shares, count)));
  }
  std::vector<py::bytes> Parameters() const {
    std::vector<py::bytes> r;
    for (const auto& p : dpf_->parameters()) r.push_back(Ser(p));
    return r;
  }
  int TreeLevelsNeeded() const { return dpf_->tree_levels_needed(); }
  std::vector<int> HierarchyToTree() const { return dpf_->hierarchy_to_tree(); }
  int BlocksNeeded(int h) const { return dpf_->blocks_needed(h); }
  int ElementsPerBlock(int h) const { return dpf_->flat_value_type(h).elements_per_block; }
  int PackedSize(int h) const { return dpf_->flat_value_type(h).packed_size; }
  int CorrectedElementsPerBlock(int h) const { return dpf_->corrected_elements_per_block(h); }
  int64_t OutputElements(int h, int64_t n, int prev) const {
    return Take(dpf_->OutputElements(h, n, prev));
  }

 private:
  std::shared_ptr<DistributedPointFunction> dpf_;
};

class PyDcf {
 public:
  static PyDcf Create(const py::bytes& params) {
    PyDcf r;
    r.dcf_ = std::shared_ptr<DistributedComparisonFunction>(
        Take(DistributedComparisonFunction::Create(Parse<DcfParameters>(params))).release());
    return r;
  }
  py::tuple GenerateKeys(const py::int_& alpha, const py::bytes& beta, const py::object& s0,
                         const py::object& s1) {
    std::pair<DcfKey, DcfKey> keys;
    if (s0.is_none())
      keys = Take(dcf_->GenerateKeys(IntToU128(alpha), Parse<Value>(beta)));
    else
      keys = Take(dcf_->GenerateKeysWithSeeds(IntToU128(alpha), Parse<Value>(beta),
                                              IntToU128(s0.cast<py::int_>()),
                                              IntToU128(s1.cast<py::int_>())));
    return py::make_tuple(Ser(keys.first), Ser(keys.second));
  }
  py::array_t<uint8_t> Evaluate(const py::bytes& key,
                                const py::array_t<uint64_t, py::array::c_style | py::array::forcecast>& xs,
                                const py::object& vt) {
    auto x = ToU128(xs);
    auto t = OptType(vt);
    return ToArray(Take(dcf_->EvaluatePacked(Parse<DcfKey>(key), MakeConstSpan(x), t.get())));
  }
  PyKeyBatch MakeKeyBatch(const std::vector<py::bytes>& keys) {
    std::vector<DcfKey> k;
    k.reserve(keys.size());
    for (const auto& b : keys) k.push_back(Parse<DcfKey>(b));
    std::vector<const DcfKey*> ptrs;
    for (const auto& x : k) ptrs.push_back(&x);
    return PyKeyBatch{std::make_shared<KeyBatch>(Take(dcf_->MakeKeyBatch(MakeConstSpan(ptrs))))};
  }
  int64_t EvaluateBatchToDevice(const PyDeviceKeyBatch& keys, uintptr_t points, int64_t ppk,
                                bool shared, uintptr_t out, int64_t capacity, uintptr_t stream) {
    py::gil_scoped_release nogil;
    auto r = dcf_->EvaluateBatchToDevice(*keys.d, reinterpret_cast<const void*>(points), ppk, shared,
                                         reinterpret_cast<void*>(out), capacity,
                                         reinterpret_cast<void*>(stream));
    if (!r.ok()) {
      py::gil_scoped_acquire g;
      throw StatusError(r.status());
    }
    return *r;
  }
  int64_t EvaluateFullDomainToDevice(const py::bytes& key_bytes, int64_t shard, int64_t num_shards,
                                     uintptr_t out, int64_t capacity, uintptr_t stream) {
    const DcfKey key = Parse<DcfKey>(key_bytes);
    return TakeNoGil([&] {
      return dcf_->EvaluateFullDomainToDevice(key, shard, num_shards, reinterpret_cast<void*>(out),
                                              capacity, reinterpret_cast<void*>(stream));
    });
  }
  int64_t EvaluateFullDomainBatchToDevice(const PyDeviceKeyBatch& keys, int64_t shard,
                                          int64_t num_shards, uintptr_t out, int64_t capacity,
                                          uintptr_t stream) {
    return TakeNoGil([&] {
      return dcf_->EvaluateFullDomainBatchToDevice(*keys.d, shard, num_shards,
                                                   reinterpret_cast<void*>(out), capacity,
                                                   reinterpret_cast<void*>(stream));
    });
  }
  py::array_t<uint8_t> EvaluateFullDomainPacked(const py::bytes& key_bytes, const py::object& vt) {
    const DcfKey key = Parse<DcfKey>(key_bytes);
    auto t = OptType(vt);
    return ToArray(TakeNoGil([&] { return dcf_->EvaluateFullDomainPacked(key, t.get()); }));
  }
  bool EvaluatesFullDomainOnDevice() const { return dcf_->EvaluatesFullDomainOnDevice(); }
  int64_t EvaluateRangeDotToDevice(const py::bytes& key_bytes, int64_t shard, int64_t num_shards,
                                   uintptr_t db, int64_t db_bytes, int64_t record_words,
                                   uintptr_t out, int64_t out_bytes, uintptr_t stream) {
    const DcfKey key = Parse<DcfKey>(key_bytes);
    return TakeNoGil([&] {
      return dcf_->EvaluateRangeDotToDevice(key, shard, num_shards,
                                            reinterpret_cast<const void*>(db), db_bytes,
                                            record_words, reinterpret_cast<void*>(out), out_bytes,
                                            reinterpret_cast<void*>(stream));
    });
  }
  py::array_t<uint64_t> EvaluateRangeDot(const py::bytes& key_bytes, uintptr_t db, int64_t db_bytes,
                                         int64_t record_words) {
    const DcfKey key = Parse<DcfKey>(key_bytes);
    const std::vector<uint64_t> v = TakeNoGil([&] {
      return dcf_->EvaluateRangeDot(key, reinterpret_cast<const void*>(db), db_bytes,
                                    record_words);
    });
    py::array_t<uint64_t> a(static_cast<py::ssize_t>(v.size()));
    if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * 8);
    return a;
  }
  py::tuple GenerateKeyBatch(const U64Array& alphas, const std::vector<py::bytes>& betas,
                             const py::object& root_seeds, int threads) {
    std::vector<Value> v;
    for (const auto& b : betas) v.push_back(Parse<Value>(b));
    const auto a = ToU128(alphas);
    const auto seeds = OptU128(root_seeds);
    return HostPair(TakeNoGil([&] {
      return dcf_->GenerateKeyBatch(MakeConstSpan(a), MakeConstSpan(v), MakeConstSpan(seeds),
                                    threads);
    }));
  }
  py::tuple GenerateKeyBatchToDevice(const U64Array& alphas, const std::vector<py::bytes>& betas,
                                     const py::object& root_seeds, uintptr_t stream) {
    std::vector<Value> v;
    for (const auto& b : betas) v.push_back(Parse<Value>(b));
    const auto a = ToU128(alphas);
    const auto seeds = OptU128(root_seeds);
    return DevicePair(TakeNoGil([&] {
      return dcf_->GenerateKeyBatchToDevice(MakeConstSpan(a), MakeConstSpan(v),
                                            MakeConstSpan(seeds), reinterpret_cast<void*>(stream));
    }));
  }
  bool GeneratesKeysOnDevice() const { return dcf_->dpf().GeneratesKeysOnDevice(); }
  int PackedSize() const { return dcf_->dpf().flat_value_type(0).packed_size; }
  std::vector<int> HierarchyToTree() const { return dcf_->dpf().hierarchy_to_tree(); }

 private:
  std::shared_ptr<DistributedComparisonFunction> dcf_;
};

py::array_t<uint64_t> FromU128(const std::vector<uint128>& v) {
  py::array_t<uint64_t> a({static_cast<py::ssize_t>(v.size()), py::ssize_t{2}});
  auto w = a.mutable_unchecked<2>();
  for (size_t i = 0; i < v.size(); ++i) {
    w(i, 0) = Uint128Low64(v[i]);
    w(i, 1) = Uint128High64(v[i]);
  }
  return a;
}

struct PyMicKeyBatch;
struct PyDeviceMicKeyBatch {
  std::shared_ptr<DeviceMicKeyBatch> d;
  int64_t NumKeys() const { return d->num_keys(); }
  int NumIntervals() const { return d->num_intervals(); }
  PyMicKeyBatch Download(uintptr_t stream) const;
};

struct PyMicKeyBatch {
  std::shared_ptr<MicKeyBatch> b;
  int64_t NumKeys() const { return b->dcf.num_keys; }
  int NumIntervals() const { return b->num_intervals; }
  PyKeyBatch Dcf() const {
    return PyKeyBatch{std::shared_ptr<KeyBatch>(b, &b->dcf)};
  }
  py::array_t<uint64_t> MaskShares() const {
    py::array_t<uint64_t> a({static_cast<py::ssize_t>(b->mask_share.size()), py::ssize_t{2}});
    if (!b->mask_share.empty())
      std::memcpy(a.mutable_data(), b->mask_share.data(), b->mask_share.size() * 16);
    return a;
  }
};

PyMicKeyBatch PyDeviceMicKeyBatch::Download(uintptr_t stream) const {
  return PyMicKeyBatch{std::make_shared<MicKeyBatch>(
      TakeNoGil([&] { return d->Download(reinterpret_cast<void*>(stream)); }))};
}

class PyMic {
 public:
  py::tuple GenBatch(const U64Array& r_in, const U64Array& r_out, const py::object& root_seeds,
                     const py::object& z0) {
    const auto ri = ToU128(r_in), ro = ToU128(r_out);
    const auto seeds = OptU128(root_seeds), z = OptU128(z0);
    auto r = TakeNoGil([&] {
      return mic_->GenBatch(MakeConstSpan(ri), MakeConstSpan(ro), MakeConstSpan(seeds),
                            MakeConstSpan(z));
    });
    return py::make_tuple(PyMicKeyBatch{std::make_shared<MicKeyBatch>(std::move(r.first))},
                          PyMicKeyBatch{std::make_shared<MicKeyBatch>(std::move(r.second))});
  }
  py::tuple GenBatchToDevice(const U64Array& r_in, const U64Array& r_out,
                             const py::object& root_seeds, const py::object& z0, uintptr_t stream) {
    const auto ri = ToU128(r_in), ro = ToU128(r_out);
    const auto seeds = OptU128(root_seeds), z = OptU128(z0);
    auto r = TakeNoGil([&] {
      return mic_->GenBatchToDevice(MakeConstSpan(ri), MakeConstSpan(ro), MakeConstSpan(seeds),
                                    MakeConstSpan(z), reinterpret_cast<void*>(stream));
    });
    return py::make_tuple(
        PyDeviceMicKeyBatch{std::shared_ptr<DeviceMicKeyBatch>(r.first.release())},
        PyDeviceMicKeyBatch{std::shared_ptr<DeviceMicKeyBatch>(r.second.release())});
  }
  static PyMic Create(const py::bytes& params) {
    PyMic r;
    r.mic_ = std::shared_ptr<MultipleIntervalContainmentGate>(
        Take(MultipleIntervalContainmentGate::Create(Parse<MicParameters>(params))).release());
    return r;
  }
  py::tuple Gen(const py::int_& r_in,
                const py::array_t<uint64_t, py::array::c_style | py::array::forcecast>& r_out,
                const py::object& s0, const py::object& s1, const py::object& z0) {
    std::pair<MicKey, MicKey> keys;
    if (s0.is_none()) {
      keys = Take(mic_->Gen(IntToU128(r_in), ToU128(r_out)));
    } else {
      auto z = ToU128(z0.cast<py::array_t<uint64_t, py::array::c_style | py::array::forcecast>>());
      keys = Take(mic_->GenWithSeeds(IntToU128(r_in), ToU128(r_out), IntToU128(s0.cast<py::int_>()),
                                     IntToU128(s1.cast<py::int_>()), MakeConstSpan(z)));
    }
    return py::make_tuple(Ser(keys.first), Ser(keys.second));
  }
  py::array_t<uint64_t> Eval(const py::bytes& key, const py::int_& x) {
    return FromU128(Take(mic_->Eval(Parse<MicKey>(key), IntToU128(x))));
  }
  py::array_t<uint64_t> EvalBatch(const std::vector<py::bytes>& keys,
                                  const py::array_t<uint64_t, py::array::c_style | py::array::forcecast>& xs) {
    std::vector<MicKey> k;
    k.reserve(keys.size());
    for (const auto& b : keys) k.push_back(Parse<MicKey>(b));
    std::vector<const MicKey*> ptrs;
    for (const auto& x : k) ptrs.push_back(&x);
    auto x = ToU128(xs);
    return FromU128(Take(mic_->EvalBatch(MakeConstSpan(ptrs), MakeConstSpan(x))));
  }
  PyMicKeyBatch MakeKeyBatch(const std::vector<py::bytes>& keys) {
    std::vector<MicKey> k;
    k.reserve(keys.size());
    for (const auto& b : keys) k.push_back(Parse<MicKey>(b));
    std::vector<const MicKey*> ptrs;
    for (const auto& x : k) ptrs.push_back(&x);
    return PyMicKeyBatch{std::make_shared<MicKeyBatch>(Take(mic_->MakeKeyBatch(MakeConstSpan(ptrs))))};
  }
  int64_t EvalBatchToDevice(const PyDeviceMicKeyBatch& keys, uintptr_t x, uintptr_t out,
                            int64_t capacity, uintptr_t stream) {
    py::gil_scoped_release nogil;
    auto r = mic_->EvalBatchToDevice(*keys.d, reinterpret_cast<const void*>(x),
                                     reinterpret_cast<void*>(out), capacity,
                                     reinterpret_cast<void*>(stream));
    if (!r.ok()) {
      py::gil_scoped_acquire g;
      throw StatusError(r.status());
    }
    return *r;
  }
  int NumUniqueOffsets() const { return mic_->num_unique_offsets(); }

 private:
  std::shared_ptr<MultipleIntervalContainmentGate> mic_;
};

}  // namespace

PYBIND11_MODULE(_dpf_host, m) {
  m.doc() = "Host C++ DistributedPointFunction (MI355X engine) -- serialized-proto binding";
  py::register_exception<StatusError>(m, "StatusError");
  py::class_<PyDeviceKeyBatch>(m, "DeviceKeyBatch")
      .def_property_readonly("num_keys", &PyDeviceKeyBatch::NumKeys)
      .def_property_readonly("first_key", &PyDeviceKeyBatch::FirstKey)
      .def("download", &PyDeviceKeyBatch::Download);
  py::class_<PyBatchContext>(m, "DeviceBatchContext")
      .def_property_readonly("previous_hierarchy_level", &PyBatchContext::PreviousHierarchyLevel)
      .def_property_readonly("partial_evaluations_level", &PyBatchContext::PartialEvaluationsLevel)
      .def_property_readonly("expansion_cache_level", &PyBatchContext::ExpansionCacheLevel)
      .def_property_readonly("num_partial_evaluations", &PyBatchContext::NumPartialEvaluations)
      .def_property_readonly("device_bytes", [](const PyBatchContext& c) { return c.ctx->device_bytes(); })
      .def_property_readonly("cache_events", [](const PyBatchContext& c) {
        const auto& e = c.ctx->cache_events();
        py::dict d;
        d["cache_refused"] = e.cache_refused;
        d["spare_refused"] = e.spare_refused;
        d["in_place"] = e.in_place;
        d["permuted"] = e.permuted;
        d["evicted_spare"] = e.evicted_spare;
        d["evicted_cache"] = e.evicted_cache;
        d["alloc_failures"] = e.alloc_failures;
        return d;
      })
      .def("fail_next_allocations_for_testing",
           [](PyBatchContext& c, int n, int skip) { c.ctx->FailNextAllocationsForTesting(n, skip); },
           py::arg("n"), py::arg("skip") = 0)
      .def("reset", [](PyBatchContext& c, bool release) { c.ctx->Reset(release); },
           py::arg("release_expansion_cache") = false)
      .def("release_expansion_cache", [](PyBatchContext& c) { c.ctx->ReleaseExpansionCache(); });
  py::class_<PyKeyBatch>(m, "KeyBatch")
      .def_property_readonly("num_keys", &PyKeyBatch::NumKeys)
      .def_property_readonly("num_levels", &PyKeyBatch::NumLevels)
      .def("seeds", &PyKeyBatch::Seeds)
      .def("party", &PyKeyBatch::Party)
      .def_property_readonly("num_hierarchy_levels", &PyKeyBatch::NumHierarchyLevels)
      .def("cw_seeds", &PyKeyBatch::CwSeeds)
      .def("cw_left", &PyKeyBatch::CwLeft)
      .def("cw_right", &PyKeyBatch::CwRight)
      .def("value_correction", &PyKeyBatch::ValueCorrection)
      .def("upload", [](const PyKeyBatch& b, int64_t begin, int64_t end, uintptr_t stream) {
        auto d = Take(DeviceKeyBatch::Upload(*b.b, begin, end, reinterpret_cast<void*>(stream)));
        return PyDeviceKeyBatch{std::shared_ptr<DeviceKeyBatch>(d.release())};
      });
  py::class_<PyDpf>(m, "DistributedPointFunction")
      .def_static("create_incremental", &PyDpf::CreateIncremental)
      .def("register_value_type", &PyDpf::RegisterValueType)
      .def("generate_keys_incremental", &PyDpf::GenerateKeys)
      .def("generate_keys_incremental_with_seeds", &PyDpf::GenerateKeysWithSeeds)
      .def("create_evaluation_context", &PyDpf::CreateEvaluationContext)
      .def("time_evaluate_until", &PyDpf::TimeEvaluateUntil)
      .def("evaluate_until", &PyDpf::EvaluateUntil)
      .def("evaluate_until_to_device", &PyDpf::EvaluateUntilToDevice)
      .def("evaluate_shard_to_device", &PyDpf::EvaluateShardToDevice)
      .def("evaluate_dot_to_device", &PyDpf::EvaluateDotToDevice)
      .def("evaluate_dot", &PyDpf::EvaluateDot)
      .def("evaluate_select_to_device", &PyDpf::EvaluateSelectToDevice)
      .def("evaluate_select", &PyDpf::EvaluateSelect)
      .def("evaluate_dot_batch_to_device", &PyDpf::EvaluateDotBatchToDevice)
      .def("evaluate_dot_batch", &PyDpf::EvaluateDotBatch)
      .def("evaluate_at", &PyDpf::EvaluateAt)
      .def("evaluate_at_ctx", &PyDpf::EvaluateAtCtx)
      .def("evaluate_at_batch", &PyDpf::EvaluateAtBatch)
      .def("make_key_batch", &PyDpf::MakeKeyBatch)
      .def("key_from_batch", &PyDpf::KeyFromBatch)
      .def("parse_key_batch", &PyDpf::ParseKeyBatch)
      .def("serialize_key_batch", &PyDpf::SerializeKeyBatch)
      .def("generate_key_batch", &PyDpf::GenerateKeyBatch)
      .def("generate_key_batch_with_betas", &PyDpf::GenerateKeyBatchWithBetas)
      .def("generate_key_batch_to_device", &PyDpf::GenerateKeyBatchToDevice)
      .def("generates_keys_on_device", &PyDpf::GeneratesKeysOnDevice)
      .def("evaluate_at_batch_to_device", &PyDpf::EvaluateAtBatchToDevice)
      .def("evaluate_at_batch_sum_to_device", &PyDpf::EvaluateAtBatchSumToDevice)
      .def("evaluate_lookup_batch_to_device", &PyDpf::EvaluateLookupBatchToDevice)
      .def("evaluate_lookup_batch", &PyDpf::EvaluateLookupBatch)
      .def("evaluates_lookup_on_device", &PyDpf::EvaluatesLookupOnDevice)
      .def("check_lookup_args", &PyDpf::CheckLookupArgs)
      .def("evaluate_dot_buckets_to_device", &PyDpf::EvaluateDotBucketsToDevice)
      .def("evaluate_dot_buckets", &PyDpf::EvaluateDotBuckets)
      .def("evaluates_dot_buckets_on_device", &PyDpf::EvaluatesDotBucketsOnDevice)
      .def("check_dot_buckets_args", &PyDpf::CheckDotBucketsArgs)
      .def("evaluate_full_domain_sum_to_device", &PyDpf::EvaluateFullDomainSumToDevice)
      .def("evaluate_full_domain_sum", &PyDpf::EvaluateFullDomainSum)
      .def("evaluates_full_domain_sum_on_device", &PyDpf::EvaluatesFullDomainSumOnDevice)
      .def("check_full_domain_sum_args", &PyDpf::CheckFullDomainSumArgs)
      .def("evaluate_full_domain_sum_packed_to_device",
           &PyDpf::EvaluateFullDomainSumPackedToDevice)
      .def("evaluate_full_domain_sum_packed", &PyDpf::EvaluateFullDomainSumPacked)
      .def("evaluates_full_domain_sum_packed_on_device",
           &PyDpf::EvaluatesFullDomainSumPackedOnDevice)
      .def("check_full_domain_sum_packed_args", &PyDpf::CheckFullDomainSumPackedArgs)
      .def("evaluate_full_domain_sum_sketch_to_device",
           &PyDpf::EvaluateFullDomainSumSketchToDevice)
      .def("evaluate_full_domain_sum_sketch", &PyDpf::EvaluateFullDomainSumSketch)
      .def("evaluates_full_domain_sum_sketch_on_device",
           &PyDpf::EvaluatesFullDomainSumSketchOnDevice)
      .def("check_full_domain_sum_sketch_args", &PyDpf::CheckFullDomainSumSketchArgs)
      .def("create_batch_evaluation_context", &PyDpf::CreateBatchEvaluationContext)
      .def("evaluate_until_batch_to_device", &PyDpf::EvaluateUntilBatchToDevice)
      .def("evaluate_until_batch_sketch_to_device", &PyDpf::EvaluateUntilBatchSketchToDevice)
      .def("export_evaluation_context", &PyDpf::ExportEvaluationContext)
      .def("sum_packed_shares", &PyDpf::SumPackedShares)
      .def("parameters", &PyDpf::Parameters)
      .def("tree_levels_needed", &PyDpf::TreeLevelsNeeded)
      .def("hierarchy_to_tree", &PyDpf::HierarchyToTree)
      .def("blocks_needed", &PyDpf::BlocksNeeded)
      .def("elements_per_block", &PyDpf::ElementsPerBlock)
      .def("packed_size", &PyDpf::PackedSize)
      .def("corrected_elements_per_block", &PyDpf::CorrectedElementsPerBlock)
      .def("output_elements", &PyDpf::OutputElements);
  py::class_<PyDcf>(m, "DistributedComparisonFunction")
      .def_static("create", &PyDcf::Create)
      .def("generate_keys", &PyDcf::GenerateKeys, py::arg("alpha"), py::arg("beta"),
           py::arg("seed_0") = py::none(), py::arg("seed_1") = py::none())
      .def("evaluate", &PyDcf::Evaluate)
      .def("make_key_batch", &PyDcf::MakeKeyBatch)
      .def("generate_key_batch", &PyDcf::GenerateKeyBatch)
      .def("generate_key_batch_to_device", &PyDcf::GenerateKeyBatchToDevice)
      .def("generates_keys_on_device", &PyDcf::GeneratesKeysOnDevice)
      .def("evaluate_batch_to_device", &PyDcf::EvaluateBatchToDevice)
      .def("evaluate_full_domain_to_device", &PyDcf::EvaluateFullDomainToDevice)
      .def("evaluate_full_domain_batch_to_device", &PyDcf::EvaluateFullDomainBatchToDevice)
      .def("evaluate_full_domain_packed", &PyDcf::EvaluateFullDomainPacked)
      .def("evaluates_full_domain_on_device", &PyDcf::EvaluatesFullDomainOnDevice)
      .def("evaluate_range_dot_to_device", &PyDcf::EvaluateRangeDotToDevice)
      .def("evaluate_range_dot", &PyDcf::EvaluateRangeDot)
      .def("packed_size", &PyDcf::PackedSize)
      .def("hierarchy_to_tree", &PyDcf::HierarchyToTree);
  py::class_<PyDeviceMicKeyBatch>(m, "DeviceMicKeyBatch")
      .def_property_readonly("num_keys", &PyDeviceMicKeyBatch::NumKeys)
      .def_property_readonly("num_intervals", &PyDeviceMicKeyBatch::NumIntervals)
      .def("download", &PyDeviceMicKeyBatch::Download);
  py::class_<PyMicKeyBatch>(m, "MicKeyBatch")
      .def_property_readonly("num_keys", &PyMicKeyBatch::NumKeys)
      .def_property_readonly("num_intervals", &PyMicKeyBatch::NumIntervals)
      .def("dcf", &PyMicKeyBatch::Dcf)
      .def("mask_shares", &PyMicKeyBatch::MaskShares)
      .def("upload", [](const PyMicKeyBatch& b, uintptr_t stream) {
        auto d = Take(DeviceMicKeyBatch::Upload(*b.b, reinterpret_cast<void*>(stream)));
        return PyDeviceMicKeyBatch{std::shared_ptr<DeviceMicKeyBatch>(d.release())};
      });
  py::class_<PyMic>(m, "MultipleIntervalContainmentGate")
      .def_static("create", &PyMic::Create)
      .def("gen", &PyMic::Gen, py::arg("r_in"), py::arg("r_out"), py::arg("seed_0") = py::none(),
           py::arg("seed_1") = py::none(), py::arg("z_0") = py::none())
      .def("eval", &PyMic::Eval)
      .def("eval_batch", &PyMic::EvalBatch)
      .def("make_key_batch", &PyMic::MakeKeyBatch)
      .def("gen_batch", &PyMic::GenBatch)
      .def("gen_batch_to_device", &PyMic::GenBatchToDevice)
      .def("eval_batch_to_device", &PyMic::EvalBatchToDevice)
      .def("num_unique_offsets", &PyMic::NumUniqueOffsets);
  m.def("synthetic_levels", [](int log, int64_t count, double concentration, uint64_t seed, int mef) {
    auto nz = experiments::MakeSyntheticNonzeros(count, log, concentration, seed);
    auto prefixes = experiments::ComputePrefixes(nz, log);
    auto levels = experiments::ComputeLevelsToEvaluate(prefixes, log, mef);
    std::vector<int64_t> per_bit;
    for (const auto& p : prefixes) per_bit.push_back(static_cast<int64_t>(p.size()));
    py::array_t<uint64_t> a({static_cast<py::ssize_t>(nz.size()), py::ssize_t{2}});
    if (!nz.empty()) std::memcpy(a.mutable_data(), nz.data(), nz.size() * 16);
    return py::make_tuple(levels, per_bit, a);
  });
  m.def("run_synthetic_data_benchmark",
        [](int log, int64_t count, double concentration, uint64_t seed, int mef, int iters,
           bool only_nonzeros, bool verify, bool device_context) {
          experiments::BenchmarkOptions o;
          o.log_domain_size = log;
          o.num_nonzeros = count;
          o.concentration = concentration;
          o.seed = seed;
          o.max_expansion_factor = mef;
          o.num_iterations = iters;
          o.only_nonzeros = only_nonzeros;
          o.verify = verify;
          o.device_context = device_context;
          experiments::BenchmarkReport r;
          {
            py::gil_scoped_release nogil;
            auto s = experiments::RunSyntheticDataBenchmark(o);
            if (!s.ok()) {
              py::gil_scoped_acquire g;
              throw StatusError(s.status());
            }
            r = std::move(*s);
          }
          py::dict d;
          d["levels_to_evaluate"] = r.levels_to_evaluate;
          d["prefixes_per_level"] = r.prefixes_per_level;
          d["outputs_per_level"] = r.outputs_per_level;
          d["key_size_bytes"] = r.key_size_bytes;
          d["seconds_per_iteration"] = r.seconds_per_iteration;
          d["checksum_seconds_excluded"] = r.checksum_seconds;
          d["verified"] = r.verified;
          return d;
        },
        py::arg("log"), py::arg("count"), py::arg("concentration"), py::arg("seed"),
        py::arg("mef"), py::arg("iters"), py::arg("only_nonzeros"), py::arg("verify"),
        py::arg("device_context") = false);
  m.def("bits_needed", [](const py::bytes& vt, double sec) {
    return Take(dpf_internal::BitsNeeded(Parse<ValueType>(vt), sec));
  });
  m.def("value_types_are_equal", [](const py::bytes& a, const py::bytes& b) {
    return Take(dpf_internal::ValueTypesAreEqual(Parse<ValueType>(a), Parse<ValueType>(b)));
  });
  m.def("roundtrip", [](const std::string& name, const py::bytes& b) -> py::bytes {
    // Parses and re-serializes one message (wire-format conformance tests).
    if (name == "DpfKey") return Ser(Parse<DpfKey>(b));
    if (name == "EvaluationContext") return Ser(Parse<EvaluationContext>(b));
    if (name == "DpfParameters") return Ser(Parse<DpfParameters>(b));
    if (name == "Value") return Ser(Parse<Value>(b));
    if (name == "ValueType") return Ser(Parse<ValueType>(b));
    if (name == "CorrectionWord") return Ser(Parse<CorrectionWord>(b));
    if (name == "PartialEvaluation") return Ser(Parse<PartialEvaluation>(b));
    if (name == "Block") return Ser(Parse<Block>(b));
    if (name == "DcfParameters") return Ser(Parse<DcfParameters>(b));
    if (name == "DcfKey") return Ser(Parse<DcfKey>(b));
    if (name == "Interval") return Ser(Parse<fss_gates::Interval>(b));
    if (name == "MicParameters") return Ser(Parse<MicParameters>(b));
    if (name == "MicKey") return Ser(Parse<MicKey>(b));
    throw std::invalid_argument("unknown message " + name);
  });
  m.def("debug_string", [](const std::string& name, const py::bytes& b) -> std::string {
    if (name == "DpfKey") return Parse<DpfKey>(b).DebugString();
    if (name == "EvaluationContext") return Parse<EvaluationContext>(b).DebugString();
    if (name == "ValueType") return Parse<ValueType>(b).DebugString();
    if (name == "Value") return Parse<Value>(b).DebugString();
    if (name == "Interval") return Parse<fss_gates::Interval>(b).DebugString();
    if (name == "MicParameters") return Parse<MicParameters>(b).DebugString();
    if (name == "MicKey") return Parse<MicKey>(b).DebugString();
    throw std::invalid_argument("unknown message " + name);
  });
  m.def("validate_context", [](const std::vector<py::bytes>& params, const py::bytes& ctx) {
    std::vector<DpfParameters> p;
    for (const auto& b : params) p.push_back(Parse<DpfParameters>(b));
    auto v = Take(dpf_internal::ProtoValidator::Create(MakeConstSpan(p)));
    Check(v->ValidateEvaluationContext(Parse<EvaluationContext>(ctx)));
  });
}
