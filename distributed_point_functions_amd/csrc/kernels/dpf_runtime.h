// dpf_runtime.h -- host-side plumbing shared by the kernel translation units:
// absl status codes, the thread-local last-error message
// behind dpf_hip_last_error() (defined in dpf_kernels.hip), the launch hooks,
// the launch-shape helpers (block_for, grid_for, chunked_shape: dpf_kernels.hip;
// the expand plan: dpf_expand_plan.hip) and with_bits, the dispatch on an
// integer leaf's width.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <string>
#include <type_traits>

#include "../../../include/dpf_hip.h"

namespace dpf_rt {

constexpr int kOk = 0, kInvalidArgument = 3, kResourceExhausted = 8, kFailedPrecondition = 9,
              kUnimplemented = 12, kInternal = 13;

// Records `msg` as the calling thread's last error and returns `code`.
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

// Launch hooks: the DPF_* environment variables, read at every call (nothing
// is cached).  hook_is: the hook's first character is `c` (unset or empty: no).
inline bool hook_is(const char* name, char c) {
  const char* v = getenv(name);
  return v && v[0] == c;
}
inline bool hook_set(const char* name) { return getenv(name) != nullptr; }
// The hook as a number; unset or empty: `dflt`.  hook_int clamps to [lo, hi].
inline long long hook_long(const char* name, long long dflt) {
  const char* v = getenv(name);
  return v && *v ? strtoll(v, nullptr, 10) : dflt;
}
inline int hook_int(const char* name, int dflt, int lo = INT32_MIN, int hi = INT32_MAX) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  const int k = atoi(v);
  return k < lo ? lo : (k > hi ? hi : k);
}

int num_cus();                                 // compute units of the current device
int max_block();                               // kBlock and kSMax (dpf_device.h), for the
int max_subtree_depth();                       // files that include no device header
int block_for(int64_t work_items);             // threads per workgroup: kBlock, or fewer
                                               // (multiple of 64) to spread a small launch over more CUs
int grid_for(int64_t work_items, int block);   // workgroups of `block` threads, <= one per CU
// Shape of a launch whose kernel takes its items through ItemLoop
// (dpf_device.h): block_for / grid_for of `items`, and dyn_per_wg, the chunks
// of 64 items per workgroup, or 0 (a fixed share per thread).  Dynamic when
// the launch gives every wave at least 4 chunks and the hook `hook` is not
// "0" (A/B and test hooks, read per launch); dpf_hip_last_dynamic_chunks
// reports dyn_per_wg.
struct LaunchShape {
  int block, grid;
  int64_t dyn_per_wg;
};
LaunchShape chunked_shape(int64_t items, const char* hook);
// f(std::integral_constant<int, B>) for the leaf width B = `bits` of 8, 16, 32
// or 64, else 128.
template <class F>
auto with_bits(int bits, F&& f) {
  switch (bits) {
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    default: return f(std::integral_constant<int, 128>{});
  }
}
// Chunk schedule of a full-domain expand launch of `num_items` subtrees of
// depth S, each k0 levels below its start seed, on `cus` workgroups of 16
// waves (dpf_expand_plan.hip, "Who takes which chunk"; reads the DPF_OCTET_*
// hooks).  shift == 0: a static launch, nothing else is set.  Else phase j
// (taken in order) is chunks[j] chunks of 64 items of shape (k0[j], S[j]),
// the first of them item first_item[j] in that shape; absent phases have no
// chunks.
struct ChunkPlan {
  int shift;     // levels taken off the subtrees for dynamic distribution
  int global;    // 1: one counter for the launch; 0: one per workgroup
  int64_t groups;   // counters: 1, or cus (each then takes chunks[j] / cus of phase j)
  int k0[3], S[3];
  int64_t chunks[3], first_item[3];
};
// sched_ok false: the counter per launch and the taper only where the hooks ask.
ChunkPlan plan_chunks(int64_t num_items, int k0, int S, int min_S, int64_t cus, bool sched_ok);
// The plan as the 15 words of dpf_hip_octet_schedule / dpf_hip_last_expand_schedule.
void write_plan(const ChunkPlan& c, int64_t* out);
// The rest of the launch plan of a full-domain expansion (dpf_expand_plan.hip):
// pure functions of the shape, the CU count and the hooks; they launch nothing.
constexpr int kSmallMaxD = 11;   // levels expand_small_kernel takes breadth-first through LDS
// Depth-first subtree depth S of an expansion of `num_levels` below `num_starts` seeds.
int choose_subtree_depth(int64_t num_starts, int num_levels);
// Shape (t levels walked, D breadth-first) of the small-tree launch; false: not that shape.
bool small_shape(int64_t num_starts, int num_levels, int* t, int* D);
// Shape of the tree-top pass above `num_items` items k0 levels below their
// start seeds; false: no pass.
bool top_shape(int64_t num_items, int k0, int* t, int* D);
// Levels each dynamically taken item walks below the tree-top pass's roots.
int octet_walk_levels();
int validate_desc(const dpf_value_desc* d);    // kOk or the failure code
int packed_size(const dpf_value_desc* d);      // bytes of one packed element
bool fast_int(const dpf_value_desc* d);        // one plain/XOR integer leaf, direct, b == 1

// The dot calls (dpf_dot.hip).  dot_type: kOk and the uint64 words of one
// element and whether the group is XOR for uint64_t, XorWrapper<uint64_t> and
// XorWrapper<uint128>, else UNIMPLEMENTED.  launch_dot_fold: out[j] (row_words
// uint64 words) = the group sum of word j of the partial rows the last kernel
// left in `workspace`, combined with out's old value when `accumulate`.
extern thread_local const char* g_last_dot;   // dpf_hip_last_dot_kernel
int dot_type(const dpf_value_desc* d, int* words, int* xor_type);
int launch_dot_fold(int row_words, int xor_type, int accumulate, const void* workspace, void* out,
                    hipStream_t s);

constexpr int kHHSketchMaxRows = 2;
// out[(slot*rows + j)*2 + e] = weights[j*n + i] mod mod[e] for output i at slot
// src_offset[i / count] + i % count (NULL: slot i).
int launch_sketch_slot_weights(int64_t n, int64_t count, const int64_t* src_offset, int rows,
                               const uint32_t* weights, const uint32_t mod[2], uint32_t* out,
                               hipStream_t s);
// One steady-state heavy-hitters level (dpf_batch_hh.hip) of the launch `a`:
// start seeds from the expansion cache or gathered partial evaluations, no
// path walk, two expanded levels, `b` blocks sampled per
// Tuple/IntModN<uint32_t> value, summed over the keys.
//   a.index_major == 0: sums into the 192-bit [slot][leaf][3] workspace
//     (hh_level_kernel);
//   a.index_major != 0: lanes are keys (hh_keys_kernel) and the sums go to one
//     uint64 per [slot][leaf] (finalize with words == 1); with a.num_weights >
//     0 (<= kHHSketchMaxRows) the fused per-key sketch too.
int launch_hh_level(const dpf_prefix_batch_args& a, int b, hipStream_t s);
int launch_hh_keys(const dpf_prefix_batch_args& a, int b, hipStream_t s);

// The per-key tables of a batched prefix evaluation out of the C ABI's struct
// into a kernel's parameter block: the members that BatchLevelParams
// (dpf_batch.hip), HHParams and HHKeysParams (dpf_batch_hh.hip) all declare,
// each in the order its kernel was tuned with.  The one copy of them.
template <class Params>
void set_batch_tables(Params* p, const dpf_prefix_batch_args& a) {
  p->num_keys = a.num_keys;
  p->num_starts = a.num_starts;
  p->cw_stride = a.cw_stride;
  p->seeds_in = a.seeds_in;
  p->ctrl_in = a.control_in;
  p->parent = a.parent;
  p->save_index = a.save_index;
  p->seeds_out = a.save_after >= 0 ? a.seeds_out : nullptr;
  p->ctrl_out = a.control_out;
  p->cw_seed = a.cw_seed;
  p->cw_left = a.cw_left;
  p->cw_right = a.cw_right;
  p->vcw = a.value_correction;
  p->vcw_stride = a.desc->elements_per_block * a.desc->num_leaves;
  p->party = a.party;
  p->leaf_seeds = a.leaf_cache;   // NULL: no cache is written, leaf_slot is not read
  p->leaf_slot = a.leaf_slot;
}

}  // namespace dpf_rt

#define HIP_TRY(expr)                                           \
  do {                                                          \
    hipError_t _e = (expr);                                     \
    if (_e != hipSuccess) return ::dpf_rt::hip_fail(_e, #expr); \
  } while (0)
