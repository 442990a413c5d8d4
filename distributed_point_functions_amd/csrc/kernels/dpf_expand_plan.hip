// dpf_expand_plan.hip -- the launch plan of a full-domain expansion: which
// subtree depth, whether the small-tree launch or the tree-top pass apply,
// and the chunk schedule of a dynamic launch.  Pure host functions of the
// launch's shape, the CU count and the hooks (declared in dpf_runtime.h);
// nothing here launches a kernel or allocates, and no device header is
// included.  dpf_kernels.hip acts on them.
#include <stdint.h>

#include "../../../include/dpf_hip.h"
#include "dpf_runtime.h"

namespace dpf_rt {

// Choose the depth-first subtree depth S (items = num_starts * 2^(L - S)
// subtrees, each walked k0 = L - S levels from its start seed) by the
// per-thread critical path: rounds of items over the launch's threads times
// the AES of one item, the ILP1 walk counted twice.  Small trees get shallow
// subtrees and more items, so a launch far below one workgroup per CU is not
// serialised on a few lanes' DFS; start counts that are not powers of two
// (5 starts x 2^27: 1.25 subtrees of depth 11 per thread = 2 rounds) get
// subtrees shallow enough to divide evenly (depth 9: 5 rounds of 1, +53%).
int choose_subtree_depth(int64_t num_starts, int num_levels) {
  const int S = num_levels < max_subtree_depth() ? num_levels : max_subtree_depth();
#if defined(DPF_FORCE_S)
  if (num_levels >= DPF_FORCE_S) return DPF_FORCE_S;  // variant builds (tools/variant_bench.py)
#endif
  double best = -1;
  int best_s = S;
  for (int cand = S; cand >= (num_levels > 0 ? 1 : 0); --cand) {
    const int64_t items = num_starts << (num_levels - cand);
    const int blk = block_for(items);
    const int64_t threads = (int64_t)grid_for(items, blk) * blk;
    const int64_t rounds = (items + threads - 1) / threads;
    const double cost = (double)rounds * (2.0 * (num_levels - cand) + 3.0 * (double)(1ll << cand));
    if (best < 0 || cost < best * 0.999) {
      best = cost;
      best_s = cand;
    }
  }
  return best_s;
}

// Latency mode for small trees (expand_small_kernel): num_starts << t
// workgroups, t as large as keeps them within one per CU, and D = L - t
// levels breadth-first in each; D must be 1..kSmallMaxD.  Returns false (and
// launches nothing) when the tree does not fit that shape.  DPF_EXPAND_SMALL=0
// (read per launch) turns it off: the A/B and test hook.
bool small_shape(int64_t num_starts, int num_levels, int* t, int* D) {
  const int64_t cus = num_cus();
  if (hook_is("DPF_EXPAND_SMALL", '0') || num_levels < 1 || num_starts < 1 || num_starts > cus)
    return false;
  int tt = 0;
  while (tt < num_levels - 1 && (num_starts << (tt + 1)) <= cus) ++tt;
  const int d = num_levels - tt;
  if (d < 1 || d > kSmallMaxD) return false;
  *t = tt;
  *D = d;
  return true;
}

// The tree-top pass (expand_top, dpf_kernels.hip).  DPF_EXPAND_TOP=0 (read
// per launch) keeps the per-lane walk.
bool top_shape(int64_t num_items, int k0, int* t, int* D) {
  const int64_t starts = num_items >> k0;
  // Few start seeds (full-domain calls and their shards): with many starts
  // every item's walk is short and a workgroup per start would idle.
  if (hook_is("DPF_EXPAND_TOP", '0') || k0 < 8 || starts > num_cus() ||
      num_items < 4 * (int64_t)num_cus())
    return false;
  // Workgroups: one per subtree at depth t under each start, at least one
  // per CU; D = k0 - t levels breadth-first (1..kSmallMaxD).
  int tt = 0;
  while ((starts << tt) < num_cus() && tt < k0 - 1) ++tt;
  if (k0 - tt > kSmallMaxD) tt = k0 - kSmallMaxD;
  if (k0 - tt < 1 || (starts << tt) > INT32_MAX) return false;
  *t = tt;
  *D = k0 - tt;
  return true;
}

// Dynamic item distribution for the octet kernel (ExpandParams::dyn_chunks):
// a launch with at least 4 items per thread of one full workgroup per CU
// gets subtrees two levels shallower (4x the items, the two levels above
// them done by the tree-top pass) so every wave can take several chunks of
// 64 items from its workgroup's counter.  Applied only when the tree-top
// pass starts the items (k0 = 0 after it): otherwise every item would walk
// two more levels.  DPF_OCTET_DYNAMIC=0 (read per launch) keeps the static
// one-item-per-thread shape, =<1..4> sets the levels taken off the subtrees
// (2^that items per thread; A/B and test hook).  Default: 4 levels off
// subtrees of >= 11 (config 2 15.00 vs 15.05-15.17 ms, config 3's uint128
// shard 58.2 vs 60.9 ms, Tuple<IntModN32 x 2> 39.2 vs 40.9 ms), else 2 (the
// 2^27 / 2^28 shards 1.96 / 3.82 ms at 2 vs 2.04 / 3.90 at 4; 3 was worse than
// both everywhere; profiles/r16/octet_dynamic_ab.txt).
static int octet_dynamic_shift(int S) {
  return hook_int("DPF_OCTET_DYNAMIC", S >= 11 ? 4 : 2, 0, 4);
}
// Levels each dynamically taken item walks below the tree-top pass's roots
// (DPF_OCTET_WALK=<n>, read per launch; 0: the pass goes down to the items).
int octet_walk_levels() { return hook_int("DPF_OCTET_WALK", 2, 0, 4); }
// Who takes which chunk, and how the chunks shrink towards the end of the
// launch (r17; ExpandParams::ph_end, take_expand_chunk).
//   * One counter for all workgroups: with a fixed range per workgroup, a CU
//     that starts late or runs slow finishes late and nobody takes its
//     chunks.  DPF_OCTET_GLOBAL=0 (read per launch) keeps a counter and an
//     equal share of every phase per workgroup (A/B and test hook).
//   * Tapered chunks (guided self-scheduling): when the counter runs out
//     every wave is somewhere inside a chunk, so the launch drains for up to
//     one chunk's time on fewer and fewer waves -- launch / chunks-per-wave,
//     a quarter of the 2^27 shard's launch at its 4 chunks per wave.  So the
//     item range is cut into up to three phases, taken in order: phase j's
//     items are subtrees of depth S - 2j (4^j times smaller) that walk 2j more
//     levels from the same tree-top roots.  A phase hands over to the next
//     finer one when at most DPF_OCTET_TAPER_AT (default 2) of its chunks
//     per resident wave are left; a phase exists only while its depth is >=
//     the kernel's minimum.  DPF_OCTET_TAPER=<0..2> (read per launch) caps
//     the number of finer phases; 0: uniform chunks.
// The plan is a pure function of the launch's shape, the CU count and the
// hooks, exported as dpf_hip_octet_schedule for the CPU tests.
ChunkPlan plan_chunks(int64_t num_items, int k0, int S, int min_S, int64_t cus, bool sched_ok) {
  ChunkPlan c{};
  const int sh = octet_dynamic_shift(S);
  if (sh <= 0 || S - sh < min_S || k0 + sh > 62 || cus <= 0 || num_items <= 0 ||
      num_items > (INT64_MAX >> (sh + 4)) || (num_items << sh) % (cus * 64) != 0 ||
      (num_items << sh) < 4 * cus * max_block() || (num_items << sh) / 64 > (INT32_MAX >> 4))
    return c;
  c.shift = sh;
  // Both are on by default from 2^20 leaf blocks per CU: measured against the
  // parent build, 2^29 / 2^28 blocks ran 1.025x / 1.035x faster (15.31 vs
  // 15.70 ms, 7.41 vs 7.67 ms), 2^27 / 2^26 blocks 0.7% / 4% slower (3.85 vs
  // 3.82 ms, 2.01 vs 1.94 ms; at 2^26 each half alone was slower too), so the
  // smaller launches keep a counter per workgroup and uniform chunks
  // (profiles/r17/octet_taper_ab.txt).
  const int big = sched_ok && (num_items << S) / cus >= ((int64_t)1 << 20);
  c.global = hook_int("DPF_OCTET_GLOBAL", big, 0, 1);
  c.groups = c.global ? 1 : cus;
  const int k = k0 + sh, s = S - sh;
  const int64_t coarse = (num_items << sh) / 64;   // chunks of shape (k, s)
  // Chunks (in phase 0's size) from each phase's start to the end of the
  // launch: per resident wave `at` of phase 0's, then `at` of phase 1's.
  const int finer = hook_int("DPF_OCTET_TAPER", big ? 2 : 0, 0, 2);
  const int64_t at = hook_int("DPF_OCTET_TAPER_AT", 2, 1, 16) * cus * (max_block() / 64);
  auto exists = [&](int j) { return j <= finer && s - 2 * j >= min_S && k + 2 * j <= 62; };
  int64_t start[4] = {0, coarse, coarse, coarse};
  if (exists(1)) start[1] = coarse - (coarse < at ? coarse : at);
  if (exists(2)) start[2] = coarse - (coarse - start[1] < (at >> 2) ? coarse - start[1] : (at >> 2));
  for (int j = 0; j < 3; ++j) {
    c.k0[j] = k + 2 * j;
    c.S[j] = s - 2 * j;
    c.chunks[j] = (start[j + 1] - start[j]) << (2 * j);
    c.first_item[j] = (start[j] * 64) << (2 * j);
  }
  return c;
}

void write_plan(const ChunkPlan& c, int64_t* out) {
  for (int i = 0; i < 15; ++i) out[i] = 0;
  out[0] = c.shift;
  if (!c.shift) return;
  out[1] = c.global;
  out[2] = c.groups;
  for (int j = 0; j < 3; ++j) {
    out[3 + 4 * j] = c.chunks[j];
    out[4 + 4 * j] = c.first_item[j];
    out[5 + 4 * j] = c.k0[j];
    out[6 + 4 * j] = c.S[j];
  }
}

}  // namespace dpf_rt

using namespace dpf_rt;

extern "C" int dpf_hip_octet_schedule(int64_t num_items, int k0, int subtree_depth, int min_depth,
                                      int compute_units, int64_t* out) {
  if (!out) return fail(kInvalidArgument, "NULL pointer");
  if (num_items < 1 || k0 < 0 || subtree_depth < 0 || k0 + subtree_depth > 62 ||
      compute_units < 1)
    return fail(kInvalidArgument, "launch shape out of range");
  write_plan(plan_chunks(num_items, k0, subtree_depth, min_depth, compute_units, true), out);
  return kOk;
}
