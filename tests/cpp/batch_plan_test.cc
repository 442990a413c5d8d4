// The host-side plan of an EvaluateUntil call (csrc/host/until_plan.h), checked
// without a GPU: the slot table of an in-place cache rewrite against its
// contract, the lookup of the stored partial-evaluation prefixes (and the
// start slots it fills in the same pass) against a plain map, the first
// out-of-range prefix, the identity-gather test and the gather offsets
// against the naive loops, and the start-node table image against its
// per-start-node definition.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "until_plan.h"

using distributed_point_functions::Span;
using distributed_point_functions::uint128;
using namespace distributed_point_functions::dpf_internal;

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// ---------------------------------------------------------------- slot table
// The contract of dpf_hip_prefix_batch_level's slot table, restated:
// start node u (of T << s) reads slot start_slot[u >> s] and writes its 2^E
// leaves to slot[(u << E) + l].  Every slot is below the stride; no slot is
// written twice; a slot some start node reads is written only as a leaf of
// that node, and only if no other node reads it.
static void CheckSlotContract(const std::vector<int64_t>& start_slot, int64_t T, int s, int E,
                              int64_t stride, const std::vector<int32_t>& slot) {
  const int64_t U = T << s;
  CHECK(static_cast<int64_t>(slot.size()) == U << E);
  std::vector<int64_t> reader(stride, -1);  // -1: nobody, -2: several
  for (int64_t u = 0; u < U; ++u) {
    const int64_t r = start_slot[u >> s];
    reader[r] = reader[r] == -1 ? u : -2;
  }
  std::vector<char> written(stride, 0);
  bool in_range = true, once = true, readers_safe = true;
  for (int64_t i = 0; i < static_cast<int64_t>(slot.size()); ++i) {
    const int64_t v = slot[i];
    if (v < 0 || v >= stride) {
      in_range = false;
      continue;
    }
    if (written[v]++) once = false;
    if (reader[v] == -2 || (reader[v] >= 0 && reader[v] != (i >> E))) readers_safe = false;
  }
  CHECK(in_range);
  CHECK(once);
  CHECK(readers_safe);
  if (s == 0)  // each start node's leaf 0 lands in the slot that node read
    for (int64_t u = 0; u < U; ++u) CHECK(slot[u << E] == start_slot[u]);
}

static void TestSlotTable() {
  for (int64_t T : {1, 2, 5})
    for (int s : {0, 1, 2})
      for (int E : {1, 2}) {
        const int64_t leaves = (T << s) << E;
        // s == 0: leaf 0 reuses the slot read; else every leaf needs an unread slot.
        const int64_t enough = leaves + (s > 0 ? T : 0);
        for (int64_t stride : {enough, enough - 1})
          for (bool scattered : {false, true}) {
            std::vector<int64_t> start_slot(T);
            for (int64_t i = 0; i < T; ++i)
              start_slot[i] = scattered ? stride - 1 - i * (stride / T) : i;
            std::vector<int32_t> slot(3, -7);  // recycled storage is overwritten
            const bool ok = BuildSlotTable(start_slot, T, s, E, stride, &slot);
            CHECK(ok == (stride == enough));
            if (ok) CheckSlotContract(start_slot, T, s, E, stride, slot);
          }
      }
}

// ------------------------------------------------------ stored-prefix lookup
struct LookupCase {
  std::vector<uint128> q;     // stored prefixes
  std::vector<uint128> want;  // lookups (tree indices)
  int shift;
  bool known_sorted;
};

static void CheckLookup(const LookupCase& c, bool with_phys) {
  std::map<uint128, int64_t> pos;
  for (size_t j = 0; j < c.q.size(); ++j) pos.emplace(c.q[j], static_cast<int64_t>(j));
  const int64_t nt = static_cast<int64_t>(c.want.size());
  int64_t first_missing = nt;
  std::vector<int64_t> want_j(nt, -1);
  for (int64_t i = 0; i < nt; ++i) {
    auto it = pos.find(c.shift < 128 ? c.want[i] >> c.shift : uint128{0});
    if (it == pos.end()) {
      first_missing = std::min(first_missing, i);
    } else {
      want_j[i] = it->second;
    }
  }
  // Start slots: only where a cached call would compute them (shift <= 62).
  const bool slots = c.shift <= 62;
  std::vector<int32_t> phys;
  if (slots && with_phys) {
    phys.resize(c.q.size() << c.shift);
    for (size_t k = 0; k < phys.size(); ++k) phys[k] = static_cast<int32_t>((k * 7 + 3) % phys.size());
  }
  const StartSlotOf slot_of(slots ? c.shift : 0, phys);
  std::vector<int64_t> got_j(nt, -1), got_slot(nt, -1);
  const int64_t missing =
      LookupStoredPrefixes(c.q, c.known_sorted, c.want.data(), nt, c.shift, [&](int64_t i, int64_t j) {
        got_j[i] = j;
        if (slots) got_slot[i] = slot_of(j, c.want[i]);
      });
  CHECK(missing == first_missing);
  if (first_missing < nt) return;  // a failed lookup promises no more than the index
  CHECK(got_j == want_j);
  if (!slots) return;
  const uint128 mask = (uint128{1} << c.shift) - 1;
  bool slots_ok = true;
  for (int64_t i = 0; i < nt; ++i) {
    const int64_t logical = (want_j[i] << c.shift) | static_cast<int64_t>(c.want[i] & mask);
    if (got_slot[i] != (phys.empty() ? logical : phys[logical])) slots_ok = false;
  }
  CHECK(slots_ok);
}

static void TestLookup(std::mt19937_64& rng) {
  const int64_t N = int64_t{1} << 18;  // 8 chunks of 2^15 with DPF_HOST_THREADS=8
  std::printf("chunks %d\n", NumChunks(N));
  std::vector<uint128> sorted_q;
  uint128 x = (static_cast<uint128>(rng() >> 8) << 64) | rng();
  for (int64_t j = 0; j < N / 4; ++j) {
    x += 1 + (rng() % 200);  // gaps on both sides of the merge cursor's 64
    sorted_q.push_back(x);
  }
  std::vector<uint128> shuffled_q = sorted_q;
  std::shuffle(shuffled_q.begin(), shuffled_q.end(), rng);
  for (int shift : {0, 2})
    for (bool q_sorted : {true, false})
      for (bool ascending : {true, false}) {
        const std::vector<uint128>& q = q_sorted ? sorted_q : shuffled_q;
        LookupCase c{q, {}, shift, false};
        for (int64_t i = 0; i < N; ++i) {
          // Every stored prefix in turn, each with all its 2^shift children.
          const uint128 parent = sorted_q[(i >> shift) % sorted_q.size()];
          c.want.push_back((parent << shift) | (static_cast<uint128>(i) & ((uint128{1} << shift) - 1)));
        }
        std::sort(c.want.begin(), c.want.end());
        if (!ascending) std::shuffle(c.want.begin(), c.want.end(), rng);
        CheckLookup(c, false);
        CheckLookup(c, true);
        if (q_sorted) {
          c.known_sorted = true;  // the context knows: no check pass
          CheckLookup(c, false);
        }
        // One missing prefix, then two in different chunks: the lower index is reported.
        LookupCase one = c;
        one.want[N - 5] = (sorted_q.back() + 1) << shift;
        CheckLookup(one, false);
        LookupCase two = one;
        two.want[N / 8 + 11] = (sorted_q.back() + 2) << shift;
        CheckLookup(two, false);
      }
  // shift >= 128: every lookup is prefix 0 (the root's), stored or not.
  for (int shift : {128, 130}) {
    std::vector<uint128> with_zero = sorted_q;
    with_zero[0] = 0;
    std::vector<uint128> want(sorted_q.begin(), sorted_q.begin() + 1000);
    CheckLookup({with_zero, want, shift, true}, false);
    CheckLookup({sorted_q, want, shift, false}, false);  // no 0 stored: index 0 is missing
  }
}

// ------------------------------------------------- first out-of-range prefix
static void TestFirstOutOfRange(std::mt19937_64& rng) {
  const int64_t N = int64_t{1} << 18;
  const int log = 40;
  std::vector<uint128> p(N);
  for (auto& v : p) v = rng() & ((uint64_t{1} << log) - 1);
  auto first = [&](const std::vector<uint128>& v, int l) {
    return FirstOutOfRangePrefix(Span<const uint128>(v.data(), v.size()), l);
  };
  CHECK(first(p, log) == N);  // none
  std::vector<uint128> a = p;
  a[0] = uint128{1} << log;
  CHECK(first(a, log) == 0);
  a = p;
  a[N - 1] = (uint128{1} << log) + 5;
  CHECK(first(a, log) == N - 1);
  a[N / 2 + 77] = uint128{1} << 100;  // two offenders in different chunks
  CHECK(first(a, log) == N / 2 + 77);
  a[N / 8 - 1] = ~uint128{0};
  CHECK(first(a, log) == N / 8 - 1);
  // log domain size 127: only the top bit is out of range; 128: nothing is.
  std::vector<uint128> wide(N);
  for (auto& v : wide) v = ((static_cast<uint128>(rng()) << 64) | rng()) >> 1;
  CHECK(first(wide, 127) == N);
  wide[N - 3] |= uint128{1} << 127;
  CHECK(first(wide, 127) == N - 3);
  CHECK(first(wide, 128) == N);
  CHECK(first({}, 5) == 0);
}

// ------------------------------------------------ identity test and offsets
template <typename Pos>
static void TestIdentityAndOffsets(std::mt19937_64& rng) {
  const int64_t P = (int64_t{1} << 18) + 3;
  auto naive_identity = [](const std::vector<std::pair<Pos, int>>& m, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
      if (static_cast<int64_t>(m[i].first) != i || m[i].second != 0) return false;
    return true;
  };
  auto check = [&](const std::vector<std::pair<Pos, int>>& m) {
    CHECK(IsIdentityMap(m, P) == naive_identity(m, P));
    const int64_t block = 48, cnt = 3;
    std::vector<int64_t> got(P, -1), want(P);
    for (int64_t i = 0; i < P; ++i) want[i] = m[i].first * block + m[i].second * cnt;
    FillGatherOffsets(m, P, block, cnt, got.data());
    CHECK(got == want);
  };
  std::vector<std::pair<Pos, int>> m(P);
  for (int64_t i = 0; i < P; ++i) m[i] = {static_cast<Pos>(i), 0};
  CHECK(IsIdentityMap(m, P));
  check(m);
  auto last = m;
  last[P - 1].second = 1;  // the identity except for its last entry
  CHECK(!IsIdentityMap(last, P));
  check(last);
  auto first = m;
  first[0].first = 1;
  CHECK(!IsIdentityMap(first, P));
  check(first);
  for (auto& e : m) e = {static_cast<Pos>(rng() % 1000), static_cast<int>(rng() % 16)};
  check(m);
  CHECK(IsIdentityMap(m, 0));
}

// -------------------------------------------------------------- table image
static void TestTables(std::mt19937_64& rng) {
  const int64_t T = (int64_t{1} << 16) + 5;  // two chunks
  std::vector<uint128> tree_indices(T);
  std::vector<int32_t> parent_of(T);
  std::vector<int64_t> start_slot(T);
  std::vector<std::pair<int32_t, int>> prefix_map(T);
  for (int64_t i = 0; i < T; ++i) {
    tree_indices[i] = (static_cast<uint128>(rng()) << 64) | rng();
    parent_of[i] = static_cast<int32_t>(rng() % 5000);
    start_slot[i] = static_cast<int64_t>(rng() % 100000);
    prefix_map[i] = {static_cast<int32_t>(rng() % T), static_cast<int>(rng() % 4)};
  }
  for (StartSource source : {StartSource::kCache, StartSource::kGathered, StartSource::kPartial,
                             StartSource::kRoot})
    for (int s : {0, 2})
      for (int Wk : {0, 3, 128})
        for (bool identity : {true, false}) {
          UntilBatchShape sh;
          sh.P = sh.T = T;
          sh.s = s;
          sh.Wk = Wk;
          sh.U = T << s;
          sh.identity = identity;
          sh.block = 16;
          sh.cnt = 4;
          const TableLayout t = PlanTables(sh);
          const size_t U = static_cast<size_t>(sh.U);
          auto align = [](size_t b) { return (b + 255) & ~size_t{255}; };
          CHECK(t.need_save == (s > 0) && t.need_path == (Wk + s > 0) && t.need_offsets == !identity);
          CHECK(t.off_save == align(U * 4));
          CHECK(t.off_path == t.off_save + (s > 0 ? align(U * 4) : 0));
          CHECK(t.off_offsets == t.off_path + (Wk + s > 0 ? align(U * 16) : 0));
          CHECK(t.bytes == t.off_offsets + (identity ? 0 : static_cast<size_t>(T) * 8));
          std::vector<char> img(t.bytes + 64, '\x5a');
          FillTables(sh, t, source, tree_indices.data(),
                     source == StartSource::kPartial ? parent_of.data() : nullptr,
                     source == StartSource::kCache ? start_slot.data() : nullptr, prefix_map,
                     img.data());
          const int32_t* parent = reinterpret_cast<const int32_t*>(img.data());
          const int32_t* save = reinterpret_cast<const int32_t*>(img.data() + t.off_save);
          const dpf_block* path = reinterpret_cast<const dpf_block*>(img.data() + t.off_path);
          const uint128 mask = Wk >= 128 ? ~uint128{0} : (uint128{1} << Wk) - 1;
          bool parents_ok = true, saves_ok = true, paths_ok = true;
          for (int64_t u = 0; u < sh.U; ++u) {
            const int64_t i = u >> s, sub = u & ((int64_t{1} << s) - 1);
            const int32_t want_parent = source == StartSource::kCache      ? static_cast<int32_t>(start_slot[i])
                                        : source == StartSource::kGathered ? static_cast<int32_t>(i)
                                        : source == StartSource::kPartial  ? parent_of[i]
                                                                           : 0;
            if (parent[u] != want_parent) parents_ok = false;
            if (t.need_save && save[u] != (sub == 0 ? static_cast<int32_t>(i) : -1)) saves_ok = false;
            if (t.need_path) {
              const uint128 want_path = ((tree_indices[i] & mask) << s) | static_cast<uint128>(sub);
              if (FromBlock(path[u]) != want_path) paths_ok = false;
            }
          }
          CHECK(parents_ok);
          CHECK(saves_ok);
          CHECK(paths_ok);
          if (!identity) {
            const int64_t* offsets = reinterpret_cast<const int64_t*>(img.data() + t.off_offsets);
            bool offsets_ok = true;
            for (int64_t i = 0; i < T; ++i)
              if (offsets[i] != prefix_map[i].first * sh.block + prefix_map[i].second * sh.cnt)
                offsets_ok = false;
            CHECK(offsets_ok);
          }
          bool tail_untouched = true;  // nothing written past the image
          for (size_t k = t.bytes; k < img.size(); ++k)
            if (img[k] != '\x5a') tail_untouched = false;
          CHECK(tail_untouched);
        }
}

// --------------------------------------------------------------- call shape
static void TestShape() {
  UntilBatchArgs a;
  a.P = 3;
  a.T = 3;
  a.K = 10;
  a.Dprev = 6;
  a.start_level = 4;
  a.Dh = 9;
  a.log_bits = 3;
  a.cepb = 1;
  a.esz = 4;
  a.max_e = 2;
  a.cache_on = true;
  a.cache_level = a.prev_level = 1;
  a.cache_de = 2;
  a.cache_stride = 64;
  std::vector<std::pair<int32_t, int>> id = {{0, 0}, {1, 0}, {2, 0}};
  UntilBatchShape sh = PlanUntilBatch(a, id);
  CHECK(sh.cached && sh.W1 == 2 && sh.Wk == 0 && sh.dE == 3 && sh.E == 2 && sh.s == 1 && sh.U == 6);
  CHECK(sh.block == 8 && sh.n_blk == 24 && sh.cnt == 8 && sh.n == 24 && sh.identity);
  CHECK(sh.update_ctx && sh.out_bytes == 10 * 24 * 4);
  a.sum = true;
  CHECK(PlanUntilBatch(a, id).out_bytes == 24 * 4);
  a.cache_de = 3;  // another depth: not this call's tree nodes
  sh = PlanUntilBatch(a, id);
  CHECK(!sh.cached && sh.Wk == 2);
  a.cache_de = 2;
  a.cache_level = -1;
  CHECK(!PlanUntilBatch(a, id).cached);
  a.cache_level = 1;
  a.cache_on = false;
  CHECK(!PlanUntilBatch(a, id).cached);
  a.cache_on = true;
  a.last_level = true;
  CHECK(!PlanUntilBatch(a, id).update_ctx);
  id[2].second = 1;
  CHECK(!PlanUntilBatch(a, id).identity);
  a.Dh = 6 + 40;  // 38 levels walked per start node: too many start nodes
  CHECK(PlanUntilBatch(a, id).U == -1);
  a.max_e = -1;
  CHECK(PlanUntilBatch(a, id).U == -1);
  // The first call: no prefixes, the root alone.
  UntilBatchArgs r;
  r.T = 1;
  r.K = 2;
  r.Dh = 5;
  r.log_bits = 7;
  r.cepb = 4;
  r.esz = 1;
  r.max_e = 3;
  r.cache_on = true;
  sh = PlanUntilBatch(r, {});
  CHECK(!sh.cached && !sh.update_ctx && sh.identity && sh.E == 3 && sh.s == 2 && sh.U == 4);
  CHECK(sh.n == 128 && sh.n_blk == 128 && sh.out_bytes == 256);
}

int main() {
  std::mt19937_64 rng(11);
  TestSlotTable();
  TestLookup(rng);
  TestFirstOutOfRange(rng);
  TestIdentityAndOffsets<int32_t>(rng);
  TestIdentityAndOffsets<int64_t>(rng);
  TestTables(rng);
  TestShape();
  std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
