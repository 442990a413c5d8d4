// until_plan.h -- the host-side plan of one EvaluateUntil call as pure
// functions: the prefix range check, the identity-gather test and the gather
// offsets (both EvaluateUntil paths), and, for the batched path
// (batch_context.cc), the lookup of the stored partial-evaluation prefixes,
// the start slots in the expansion cache, the slot table of an in-place
// rewrite, the call's shape and the start-node table image.  Nothing here
// calls a dpf_hip_* entry point or touches a context, so a stand-alone
// program tests it (tests/cpp/batch_plan_test.cc).
#ifndef DPF_HOST_UNTIL_PLAN_H_
#define DPF_HOST_UNTIL_PLAN_H_

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <unordered_map>
#include <utility>
#include <vector>

#include "host_util.h"

namespace distributed_point_functions {
namespace dpf_internal {

// Lowers `a` to `i` if `i` is smaller (chunks of a parallel scan reporting
// the lowest index they found).
inline void AtomicMin(std::atomic<int64_t>& a, int64_t i) {
  int64_t cur = a.load();
  while (i < cur && !a.compare_exchange_weak(cur, i)) {
  }
}

// The lowest index whose prefix is not below 2^log_domain_size; the number of
// prefixes if there is none (h:689-700 reports the first one).  The scan runs
// on host threads.
inline int64_t FirstOutOfRangePrefix(Span<const uint128> prefixes, int log_domain_size) {
  const int64_t np = static_cast<int64_t>(prefixes.size());
  if (log_domain_size >= 128) return np;
  const uint128 limit = static_cast<uint128>(1) << log_domain_size;
  std::atomic<int64_t> bad{np};
  ParallelFor(np, [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i)
      if (prefixes[i] >= limit) {
        AtomicMin(bad, i);
        return;
      }
  });
  return bad.load();
}

// True when prefix i maps to tree index i, block 0, for every i < P: with
// matching sizes the output gather (h:822-835) is then the identity.
template <typename Pos>
bool IsIdentityMap(const std::vector<std::pair<Pos, int>>& prefix_map, int64_t P) {
  std::atomic<bool> identity{true};
  ParallelFor(P, [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i)
      if (static_cast<int64_t>(prefix_map[i].first) != i || prefix_map[i].second != 0) {
        identity.store(false);
        return;
      }
  });
  return identity.load();
}

// Element offset of each prefix's outputs in the expanded blocks: `block`
// elements per tree index, `cnt` per prefix.
template <typename Pos>
void FillGatherOffsets(const std::vector<std::pair<Pos, int>>& prefix_map, int64_t P, int64_t block,
                       int64_t cnt, int64_t* offsets) {
  ParallelFor(P, [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i)
      offsets[i] = prefix_map[i].first * block + prefix_map[i].second * cnt;
  });
}

// Finds tree_indices[i] >> shift among the stored partial-evaluation prefixes
// `q` for every i < nt and calls hit(i, j) with its position j (from host
// threads, each i once).  Returns the lowest i that has none (then hit() may
// have been skipped for later i too), nt when all were found.  Sorted `q`
// (`known_sorted`, else checked here) takes a merge cursor that restarts with
// lower_bound; unsorted `q` a hash map.
template <typename Hit>
int64_t LookupStoredPrefixes(const std::vector<uint128>& q, bool known_sorted,
                             const uint128* tree_indices, int64_t nt, int shift, Hit hit) {
  bool sorted = known_sorted;
  if (!sorted) {
    const int64_t nq = static_cast<int64_t>(q.size());
    const int qchunks = NumChunks(nq);
    std::vector<char> q_ok(qchunks, 1);
    ParallelChunks(nq, qchunks, [&](int c, int64_t lo, int64_t hi) {
      for (int64_t j = std::max<int64_t>(lo, 1); j < hi; ++j)
        if (q[j] < q[j - 1]) {
          q_ok[c] = 0;
          return;
        }
    });
    sorted = std::all_of(q_ok.begin(), q_ok.end(), [](char x) { return x != 0; });
  }
  std::unordered_map<uint128, int32_t, U128Hash> pos;
  if (!sorted) {
    pos.reserve(q.size() * 2);
    for (size_t j = 0; j < q.size(); ++j) pos.emplace(q[j], static_cast<int32_t>(j));
  }
  std::atomic<int64_t> first_missing{nt};
  ParallelFor(nt, [&](int64_t lo, int64_t hi) {
    size_t cursor = 0;  // merge pointer while the lookups ascend too
    bool fresh = true;
    for (int64_t i = lo; i < hi; ++i) {
      const uint128 want = shift < 128 ? tree_indices[i] >> shift : 0;
      int64_t j = -1;
      if (sorted) {
        if (fresh || cursor >= q.size() || q[cursor] > want) {
          cursor = std::lower_bound(q.begin(), q.end(), want) - q.begin();
          fresh = false;
        } else if (want - q[cursor] < 64) {
          while (cursor < q.size() && q[cursor] < want) ++cursor;
        } else {
          cursor = std::lower_bound(q.begin() + cursor, q.end(), want) - q.begin();
        }
        if (cursor < q.size() && q[cursor] == want) j = static_cast<int64_t>(cursor);
      } else {
        auto it = pos.find(want);
        if (it != pos.end()) j = it->second;
      }
      if (j < 0) {
        AtomicMin(first_missing, i);
        return;
      }
      hit(i, j);
    }
  });
  return first_missing.load();
}

// Physical expansion-cache slot of a tree index: the cache's logical leaf
// (j << w1) | low w1 bits of the tree index, j being the position of its
// stored prefix (0 from the root), through the cache's logical -> physical
// map `phys` when that is not empty.  w1 <= 62.
class StartSlotOf {
 public:
  StartSlotOf(int w1, const std::vector<int32_t>& phys)
      : w1_(w1), mask_((uint128{1} << w1) - 1), phys_(phys.empty() ? nullptr : phys.data()) {}
  int64_t operator()(int64_t j, uint128 tree_index) const {
    const int64_t logical = (j << w1_) | static_cast<int64_t>(tree_index & mask_);
    return phys_ ? phys_[logical] : logical;
  }

 private:
  int w1_;
  uint128 mask_;
  const int32_t* phys_;
};

// The slot table of an in-place rewrite (leaf_slot of dpf_prefix_batch_args):
// start node u = (tree index u >> s, sub-node) reads physical slot
// start_slot[u >> s]; its 2^E leaves go to slot[(u << E) + l].  A slot read by
// exactly one start node (s == 0) takes that node's leaf 0; every other leaf
// takes the next slot no start node reads.  False if those run out.
inline bool BuildSlotTable(const std::vector<int64_t>& start_slot, int64_t T, int s, int E,
                           int64_t phys_stride, std::vector<int32_t>* slot) {
  static thread_local std::vector<uint8_t> tl_read;
  std::vector<uint8_t>& read = tl_read;
  read.assign(static_cast<size_t>(phys_stride), 0);
  for (int64_t i = 0; i < T; ++i) read[start_slot[i]] = 1;
  const int64_t leaves = (T << s) << E;
  slot->resize(static_cast<size_t>(leaves));
  int64_t g = 0;  // next unread slot candidate
  auto next_free = [&]() -> int64_t {
    while (g < phys_stride && read[g]) ++g;
    return g < phys_stride ? g++ : -1;
  };
  for (int64_t u = 0; u < (T << s); ++u) {
    for (int64_t l = 0; l < (int64_t{1} << E); ++l) {
      int64_t v;
      if (l == 0 && s == 0) {
        v = start_slot[u];
      } else if ((v = next_free()) < 0) {
        return false;
      }
      (*slot)[(u << E) + l] = static_cast<int32_t>(v);
    }
  }
  return true;
}

// What the shape of a batched call is computed from.
struct UntilBatchArgs {
  int64_t P = 0;         // prefixes
  int64_t T = 0;         // unique tree indices (1, the root, when P == 0)
  int64_t K = 0;         // keys
  int Dprev = 0;         // tree depth of the tree indices
  int start_level = 0;   // tree depth of the stored partial evaluations (0: root)
  int Dh = 0;            // tree depth of this call's leaves
  int log_bits = 0;      // log domain size of this level minus the previous one's
  int cepb = 1;          // corrected elements per block
  int esz = 1;           // packed element size
  int max_e = 0;         // levels the kernel can expand per start node (< 0: none)
  bool sum = false;      // one summed row instead of one row per key
  bool last_level = false;
  // The expansion cache as the context holds it.
  bool cache_on = false;
  int cache_level = -1;      // hierarchy level whose call wrote it (-1: none)
  int prev_level = -1;       // the previous call's hierarchy level
  int cache_de = 0;          // levels from that call's tree indices to its leaves
  int64_t cache_stride = 0;  // physical row stride
};

// The shape of one batched EvaluateUntil call.
struct UntilBatchShape {
  int64_t P = 0, T = 0;
  int64_t U = -1;    // start nodes, T << s; -1: too many for one call (nothing below is set)
  int W1 = 0;        // levels from the stored partial evaluations to the tree indices
  int Wk = 0;        // of those, levels the kernel walks (0 when it reads the cache)
  int dE = 0;        // levels from the tree indices to the leaves
  int E = 0, s = 0;  // dE = s + E: walked per start node below the tree index, expanded
  // The previous call's expansion cache holds this call's tree nodes (its
  // leaves are the children, W1 levels down, of the tree indices the partial
  // evaluations stand for): the kernel reads their seeds from it and the
  // W1-level path walk is skipped.  Outputs and the
  // partial evaluations are the same either way.
  bool cached = false;
  int64_t block = 0;    // elements per tree index
  int64_t n_blk = 0;    // elements per key before the gather
  int64_t cnt = 0;      // elements per prefix
  int64_t n = 0;        // elements per key of the result
  bool identity = true;  // the output gather is the identity
  bool update_ctx = false;  // the tree indices become the stored partial evaluations
  int64_t out_bytes = 0;    // bytes the caller's buffer must hold
};

inline UntilBatchShape PlanUntilBatch(const UntilBatchArgs& a,
                                      const std::vector<std::pair<int32_t, int>>& prefix_map) {
  UntilBatchShape sh;
  sh.P = a.P;
  sh.T = a.T;
  sh.W1 = a.Dprev - a.start_level;
  sh.dE = a.Dh - a.Dprev;
  sh.cached = a.cache_on && a.P > 0 && a.cache_level >= 0 && a.cache_level == a.prev_level &&
              a.cache_de == sh.W1 && a.cache_stride <= INT32_MAX;
  sh.Wk = sh.cached ? 0 : sh.W1;
  sh.update_ctx = a.P > 0 && !a.last_level;
  if (a.max_e < 0) return sh;
  sh.E = std::min(sh.dE, a.max_e);
  sh.s = sh.dE - sh.E;
  if (sh.s > 30 || (sh.T << sh.s) > INT32_MAX) return sh;
  sh.U = sh.T << sh.s;
  sh.block = (int64_t{1} << sh.dE) * a.cepb;
  sh.n_blk = sh.T * sh.block;
  sh.cnt = int64_t{1} << a.log_bits;
  sh.n = a.P == 0 ? sh.n_blk : a.P * sh.cnt;
  sh.identity = a.P == 0 || (sh.T == a.P && sh.cnt == sh.block && IsIdentityMap(prefix_map, a.P));
  sh.out_bytes = (a.sum ? sh.n : a.K * sh.n) * a.esz;
  return sh;
}

// Where a call's start seeds come from.
enum class StartSource {
  kCache,     // read in place from the expansion cache: parent = physical slot
  kGathered,  // gathered out of the cache first: parent = tree index position
  kPartial,   // the stored partial evaluations: parent = position of the stored prefix
  kRoot,      // the keys' roots: parent 0
};

// Start-node tables (u = tree index i * 2^s + sub) and the output gather's
// offsets in ONE image, sent with one asynchronous H2D into one device
// buffer: parent[U] int32 | save[U] int32 (only with s > 0: with s == 0 start
// node u IS tree index u, save_index NULL) | path[U] (only when the kernel
// walks, Wk + s > 0) | offsets[P] int64 (non-identity gathers).  Three
// synchronous pageable copies of 24 MiB had cost a 1 M-prefix level (config
// 5a) milliseconds.
struct TableLayout {
  bool need_save = false, need_path = false, need_offsets = false;
  size_t off_save = 0, off_path = 0, off_offsets = 0, bytes = 0;
};

inline TableLayout PlanTables(const UntilBatchShape& sh) {
  auto align = [](size_t b) { return (b + 255) & ~size_t{255}; };
  const size_t U = static_cast<size_t>(sh.U);
  TableLayout t;
  t.need_path = sh.Wk + sh.s > 0;
  t.need_save = sh.s > 0;
  t.need_offsets = !sh.identity;
  t.off_save = align(U * sizeof(int32_t));
  t.off_path = t.off_save + (t.need_save ? align(U * sizeof(int32_t)) : 0);
  t.off_offsets = t.off_path + (t.need_path ? align(U * sizeof(dpf_block)) : 0);
  t.bytes = t.off_offsets + (t.need_offsets ? static_cast<size_t>(sh.P) * sizeof(int64_t) : 0);
  return t;
}

// Fills the image `img` (t.bytes) on host threads.  For start node
// u = (i << s) + sub of tree index i:
//   parent[u] = start_slot[i] | i | parent_of[i] | 0, by `source`;
//   path[u]   = (low Wk bits of tree_indices[i]) << s | sub;
//   save[u]   = i for sub == 0, else -1.
// `parent_of` is read only for kPartial, `start_slot` only for kCache.
inline void FillTables(const UntilBatchShape& sh, const TableLayout& t, StartSource source,
                       const uint128* tree_indices, const int32_t* parent_of,
                       const int64_t* start_slot,
                       const std::vector<std::pair<int32_t, int>>& prefix_map, char* img) {
  int32_t* parent = reinterpret_cast<int32_t*>(img);
  int32_t* save = t.need_save ? reinterpret_cast<int32_t*>(img + t.off_save) : nullptr;
  dpf_block* path = t.need_path ? reinterpret_cast<dpf_block*>(img + t.off_path) : nullptr;
  const int s = sh.s;
  const uint128 walk_mask = sh.Wk >= 128 ? ~uint128{0} : ((uint128{1} << sh.Wk) - 1);
  auto start_of = [&](int64_t i) -> int32_t {
    switch (source) {
      case StartSource::kCache: return static_cast<int32_t>(start_slot[i]);
      case StartSource::kGathered: return static_cast<int32_t>(i);
      case StartSource::kPartial: return parent_of[i];
      default: return 0;
    }
  };
  ParallelFor(sh.T, [&](int64_t lo, int64_t hi) {
    if (!path && s == 0) {
      // One start node per tree index and no walk (the cached steady state):
      // the parents alone, without reading the tree indices.
      for (int64_t i = lo; i < hi; ++i) parent[i] = start_of(i);
      return;
    }
    for (int64_t i = lo; i < hi; ++i) {
      const uint128 low = tree_indices[i] & walk_mask;
      const int32_t start = start_of(i);
      for (int64_t sub = 0; sub < (int64_t{1} << s); ++sub) {
        const int64_t u = (i << s) + sub;
        parent[u] = start;
        if (path) path[u] = ToBlock(s ? ((low << s) | static_cast<uint128>(sub)) : low);
        if (save) save[u] = sub == 0 ? static_cast<int32_t>(i) : -1;
      }
    }
  });
  if (t.need_offsets)
    FillGatherOffsets(prefix_map, sh.P, sh.block, sh.cnt,
                      reinterpret_cast<int64_t*>(img + t.off_offsets));
}

}  // namespace dpf_internal
}  // namespace distributed_point_functions

#endif  // DPF_HOST_UNTIL_PLAN_H_
