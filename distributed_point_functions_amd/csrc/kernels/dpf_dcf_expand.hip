// dpf_dcf_expand.hip -- full-domain DistributedComparisonFunction evaluation
// on gfx950: the shares of x -> [x < alpha] * beta at every x of the domain
// (or of one shard of it) in one depth-first walk of the key's tree, in which
// every node is hashed once.
//
// The DCF's DPF maps hierarchy level i to tree depth i with block index 0 and
// element 0 (the comment above dcf_fast_kernel, dpf_dcf.hip).  For the node at
// depth d with prefix p,
//   v_d(p) = element 0 of H_value(node), + cw_d's element 0 where t is set,
// and Evaluate(key, x) sums v_d over the depths d at which bit (n-1-d) of x is
// clear, i.e. over the nodes of x's path that the path leaves to the left (at
// depth n-1: where x is even).  So with
//   acc(left child) = acc(parent) + v_d(parent),  acc(right child) = acc(parent)
// a depth-(n-1) node with prefix p gives f(2p) = acc + v_{n-1}(p), f(2p+1) = acc.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "../../../include/dpf_hip.h"
#include "dpf_device.h"
#include "dpf_runtime.h"

using namespace dpf_rt;

namespace {

constexpr int kDcfExpandMaxLevels = 128;
// Parked nodes of an item's depth-first walk.  A slot is seed, control bit
// and acc; beside the three AES chains of a node, four slots are what the 128
// VGPRs of 4 waves per SIMD hold without spilling for values of up to 64 bits
// (the pair kernel's kGMax slots spilled 164 to 588 bytes per lane in every
// instance, six slots 124 bytes for uint64; 128-bit values still spill 24 to
// 27 registers with four: DESIGN.md section 6e).
constexpr int kDcfStack = 4;
constexpr int kDcfGMax = kDcfStack + 1;   // levels of an item that writes outputs
static_assert(kDcfGMax <= kGMax, "the plan promises G <= kGMax");
// An item that starts from a stored node reads it from the first bytes of its
// own output range: 2^(G+1) elements must hold a seed and an acc.
constexpr int kDcfTopMinG = 4;
// Keys whose items fill whole waves: the instance with the stack.
constexpr int kDcfUniformLog = 6;

// The launch plan.  A work item is (key, subtree): the subtree's root lies at
// depth walk = n - 1 - G and the item writes 2^(G+1) outputs.  top_G >= 0: a
// first launch of top_items items of top_G levels, rooted top_G + 1 levels
// above, leaves the items their roots, and only its items walk from the
// key's root; top_G < 0: every item walks.
struct DcfExpandPlan {
  int G, walk, top_G;
  int64_t items, items_per_key, top_items;
};

// G is the deepest subtree, up to the stack's, that still leaves one wave of
// items per SIMD of the chip and whole waves of items per key; a launch
// smaller than that is a few microseconds of hashing whatever its shape.
DcfExpandPlan plan_dcf_expand(int64_t num_keys, int n, int shard_bits, int num_cus) {
  const int levels = n - 1 - shard_bits;   // depths below the shard's root, above the outputs
  const int64_t want = (int64_t)(num_cus < 1 ? 1 : num_cus) * (kBlock / 4);
  int G = levels - kDcfUniformLog < kDcfGMax ? levels - kDcfUniformLog : kDcfGMax;
  if (G < 0) G = 0;
  while (G > 0) {
    const int sh = levels - G;
    if (sh >= 62 || num_keys >= ((want + ((int64_t)1 << sh) - 1) >> sh)) break;
    --G;
  }
  DcfExpandPlan pl;
  pl.G = G;
  pl.walk = n - 1 - G;
  pl.items_per_key = (int64_t)1 << (levels - G);
  pl.items = num_keys * pl.items_per_key;
  // The top launch: as deep as the stack allows while its items, too, fill
  // whole waves per key.
  pl.top_G = -1;
  pl.top_items = 0;
  if (G >= kDcfTopMinG) {
    const int room = levels - G - 1 - kDcfUniformLog;   // levels left for its items' roots
    pl.top_G = room < kDcfStack ? room : kDcfStack;
    if (pl.top_G >= 0) pl.top_items = pl.items >> (pl.top_G + 1);
  }
  return pl;
}

enum DcfExpandMode {
  kDcfLeafNode = 0,   // G == 0: the item is one depth-(n-1) node
  kDcfOutputs = 1,    // depth-first over `stack` + 1 levels, four outputs per bottom node
  kDcfEmit = 2,       // depth-first over `stack` levels, the bottom nodes' children stored
};

struct DcfExpandParams {
  int64_t num_items;
  int n;            // hierarchy levels = log domain size
  int mode;         // DcfExpandMode
  int stack;        // depth of the item's bottom nodes below its root (<= kDcfStack)
  int root_depth;   // tree depth of an item's root
  int walk_levels;  // levels an item walks from the key's root: root_depth, or 0 with
  int stored_root;  // the root the top launch left in the item's outputs
  int child_log;    // kDcfEmit: log2 of the elements below an emitted child
  int shard_bits;   // top path bits fixed by shard_index
  int cw_stride;
  int vcw_stride;   // dpf_blocks per key row of a level's value correction
  int64_t shard_index;
  const dpf_block* key_seed;
  const uint8_t* party;
  const dpf_block* cw_seed;
  const uint8_t* cw_left;
  const uint8_t* cw_right;
  char* out;
  RoundKeys rkl, rkr, rkv, rkd;
  int64_t dyn_per_wg;  // ItemLoop's per_wg (0: grid stride)
};

struct DcfExpandVcw {
  const dpf_block* level[kDcfExpandMaxLevels];  // per level: [key][E] value corrections
};

// The accumulator: element 0 of a block, as wide as the value.
template <int BITS>
using DcfAcc = typename std::conditional<BITS == 128, u128,
               typename std::conditional<BITS == 64, uint64_t, uint32_t>::type>::type;

template <int BITS>
__device__ __forceinline__ DcfAcc<BITS> element0(Block4 h) {
  if constexpr (BITS == 128) return block_u128(h);
  else if constexpr (BITS == 64) return ((uint64_t)h.w1 << 32) | h.w0;
  else return h.w0;
}
template <int BITS>
__device__ __forceinline__ DcfAcc<BITS> element0(dpf_block c) {
  if constexpr (BITS == 128) return dpf_u128(c);
  else return (DcfAcc<BITS>)c.low;
}

// K consecutive outputs (K = 2 or 4) as one store of K * BITS / 8 contiguous
// bytes per lane where that is at most 16 bytes, else 16 bytes at a time.
// `o` is aligned to the bytes written (the entry point checks `out`).
template <int BITS, int K>
__device__ __forceinline__ void store_run(char* o, const DcfAcc<BITS>* f) {
  if constexpr (BITS == 128) {
#pragma unroll
    for (int i = 0; i < K; ++i) store_bits<128>(o + 16 * i, f[i]);
  } else if constexpr (BITS == 64) {
#pragma unroll
    for (int i = 0; i < K; i += 2)
      *reinterpret_cast<uint4*>(o + 8 * i) =
          make_uint4((uint32_t)f[i], (uint32_t)(f[i] >> 32), (uint32_t)f[i + 1],
                     (uint32_t)(f[i + 1] >> 32));
  } else if constexpr (BITS == 32) {
    if constexpr (K == 4) *reinterpret_cast<uint4*>(o) = make_uint4(f[0], f[1], f[2], f[3]);
    else *reinterpret_cast<uint2*>(o) = make_uint2(f[0], f[1]);
  } else {
    // 8 and 16 bits: the run packed into one word or two.
    uint64_t w = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) w |= (uint64_t)(f[i] & ((1u << BITS) - 1u)) << (BITS * i);
    if constexpr (K * BITS == 64) *reinterpret_cast<uint2*>(o) = make_uint2((uint32_t)w, (uint32_t)(w >> 32));
    else if constexpr (K * BITS == 32) *reinterpret_cast<uint32_t*>(o) = (uint32_t)w;
    else *reinterpret_cast<uint16_t*>(o) = (uint16_t)w;
  }
}

// A node between the two launches: its seed with the control bit in bit 0
// (which a seed keeps clear), then its acc.
template <int BITS>
__device__ __forceinline__ void store_node(char* o, Block4 s, uint32_t t, DcfAcc<BITS> acc) {
  *reinterpret_cast<uint4*>(o) = make_uint4(s.w0 | t, s.w1, s.w2, s.w3);
  *reinterpret_cast<DcfAcc<BITS>*>(o + 16) = acc;
}
template <int BITS>
__device__ __forceinline__ void load_node(const char* o, Block4& s, uint32_t& t, DcfAcc<BITS>& acc) {
  const uint4 v = *reinterpret_cast<const uint4*>(o);
  acc = *reinterpret_cast<const DcfAcc<BITS>*>(o + 16);
  t = v.x & 1u;
  s = Block4{v.x & ~1u, v.y, v.z, v.w};
}

// One thread = one (key, subtree).  STACK > 0: the items of a wave share one
// key (items per key is a multiple of 64), whose correction words are then
// wave-uniform loads, and the item visits its subtree depth-first; the depth
// is wave-uniform.  STACK == 0: kDcfLeafNode items with one key per lane.
template <int BITS, bool XOR, int STACK>
__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void dcf_expand_kernel(DcfExpandParams p,
                                                                           DcfExpandVcw vc) {
  __shared__ LdsImage lds;
  __shared__ int next_chunk;   // ItemLoop (dpf_device.h)
  fill_tables(lds.tab);
  if (threadIdx.x == 0) next_chunk = 0;
  __syncthreads();
  const LdsLookup lk = make_lookup(lds, KeySet{key_ref(p.rkl), key_ref(p.rkr), key_ref(p.rkv), key_ref(p.rkd)});
  using Acc = DcfAcc<BITS>;
  constexpr int kEsz = BITS / 8;
  constexpr bool UNIFORM = STACK > 0;
  const int n = p.n, rd = p.root_depth, sb = p.shard_bits;
  auto add = [](Acc a, Acc v) -> Acc {
    if constexpr (XOR) return a ^ v; else return a + v;
  };
  // v_d of a node from its value hash.
  auto value = [&](Block4 h, uint32_t t, int64_t k, int d) -> Acc {
    const Acc cv = element0<BITS>(vc.level[d][k * p.vcw_stride]);
    return add(element0<BITS>(h), t ? cv : (Acc)0);
  };
  const ItemLoop items{&next_chunk, p.dyn_per_wg, (p.num_items + 63) / 64, p.num_items};
  for (int64_t u = items.first(); u < p.num_items; u = items.next(u)) {
    int64_t k = u >> (rd - sb);
    if (UNIFORM) k = (int64_t)__builtin_amdgcn_readfirstlane((int)k);
    const int64_t j = u - (k << (rd - sb));   // the subtree's index in the key's shard
    const uint32_t party = p.party[k] & 1u;
    const int64_t row0 = k * p.cw_stride;
    // The item's outputs: 2^(n - rd) elements of the key's row.
    char* const base = p.out + ((k << (n - sb)) + (j << (n - rd))) * (int64_t)kEsz;
    Block4 s;
    uint32_t t;
    Acc acc;
    if (p.stored_root) {
      load_node<BITS>(base, s, t, acc);   // left there by the top launch
    } else {
      s = load_block(p.key_seed + k);
      t = party;
      acc = 0;
    }
    // 1. walk to the subtree root as dcf_fast_kernel walks: value hash and
    //    path step interleaved; v_d joins acc where the path goes left.
    for (int d = 0; d < p.walk_levels; ++d) {
      const uint32_t bit = d < sb ? (uint32_t)((p.shard_index >> (sb - 1 - d)) & 1)
                                  : (uint32_t)((j >> (rd - 1 - d)) & 1);
      const uint4 cs = cw_u4(p.cw_seed[row0 + d]);
      const uint32_t cc = cw_ctrl2(p.cw_left, p.cw_right, row0 + d);
      Block4 hv = s, hn = s;
      dpf_aes::mmo_hash2(hv, hn, lk, UniformRK{lk.ks.v}, SelectRK{lk.ks.l, lk.ks.d, 0u - bit});
      const Acc v = value(hv, t, k, d);
      acc = add(acc, bit ? (Acc)0 : v);
      correct_child(hn, t, bit, cs, cc);
      s = hn;
    }
    const bool negate = !XOR && party;
    if (STACK == 0 || p.mode == kDcfLeafNode) {
      // The item is one depth-(n-1) node (n == 1: the key's root).
      const Block4 hv = dpf_aes::mmo_hash(s, lk, UniformRK{lk.ks.v});
      Acc f[2] = {add(acc, value(hv, t, k, n - 1)), acc};
      if (negate) { f[0] = (Acc)0 - f[0]; f[1] = (Acc)0 - f[1]; }
      store_run<BITS, 2>(base, f);
      continue;
    }
    if constexpr (STACK > 0) {
      // 2. depth-first over the levels below.  A node hashes its left child,
      //    right child and value as one group of three chains; the right
      //    child is parked with the parent's acc, the left one descended into
      //    with acc + v.  The walk ends at the bottom nodes, `stack` levels
      //    down: the parents of the depth-(n-1) nodes, which hash both of
      //    those together and store four outputs (kDcfOutputs), or the parents
      //    of the next launch's roots (kDcfEmit).
      const UniformRK rk3[3] = {UniformRK{lk.ks.l}, UniformRK{lk.ks.r}, UniformRK{lk.ks.v}};
      auto expand_node = [&](Block4 node, uint32_t nt, int d, Block4& c0, uint32_t& t0,
                             Block4& c1, uint32_t& t1) -> Acc {
        const uint4 cs = cw_u4(p.cw_seed[row0 + d]);
        const uint32_t cc = cw_ctrl2(p.cw_left, p.cw_right, row0 + d);
        Block4 h[3] = {node, node, node};
        dpf_aes::mmo_hashN<3>(h, lk, rk3);
        const Acc v = value(h[2], nt, k, d);
        t0 = nt; t1 = nt;
        correct_child(h[0], t0, 0u, cs, cc);
        correct_child(h[1], t1, 1u, cs, cc);
        c0 = h[0]; c1 = h[1];
        return v;
      };
      const int D = p.stack;
      const int ngroups = 1 << D;
      Block4 sib[STACK];   // sib[d - 1] = parked right child at DFS depth d
      Acc sacc[STACK];     // its acc
      uint32_t tb = 0;     // bit d = its control bit
      for (int g = 0; g < ngroups; ++g) {
        Block4 node = s;
        uint32_t nt = t;
        Acc na = acc;
        int ds = 0;  // DFS depth of `node` (wave-uniform)
        if (g != 0) {
          ds = D - __builtin_ctz((unsigned)g);
#pragma unroll
          for (int d = 1; d <= STACK; ++d)
            if (d == ds) { node = sib[d - 1]; na = sacc[d - 1]; nt = (tb >> d) & 1u; }
        }
        for (int d = ds; d < D; ++d) {
          Block4 c0, c1;
          uint32_t t0, t1;
          const Acc v = expand_node(node, nt, rd + d, c0, t0, c1, t1);
#pragma unroll
          for (int e = 1; e <= STACK; ++e)
            if (e == d + 1) { sib[e - 1] = c1; sacc[e - 1] = na; }
          tb = (tb & ~(1u << (d + 1))) | (t1 << (d + 1));
          node = c0;
          nt = t0;
          na = add(na, v);
        }
        Block4 c0, c1;
        uint32_t t0, t1;
        const Acc v = expand_node(node, nt, rd + D, c0, t0, c1, t1);
        const Acc al = add(na, v);
        if (p.mode == kDcfEmit) {
          char* o = base + (((int64_t)(2 * g) << p.child_log)) * kEsz;
          store_node<BITS>(o, c0, t0, al);
          store_node<BITS>(o + ((int64_t)kEsz << p.child_log), c1, t1, na);
        } else {
          // `node` is at depth n - 2: its children are the last nodes.
          Block4 hv0 = c0, hv1 = c1;
          dpf_aes::mmo_hash2(hv0, hv1, lk, UniformRK{lk.ks.v}, UniformRK{lk.ks.v});
          Acc f[4] = {add(al, value(hv0, t0, k, n - 1)), al, add(na, value(hv1, t1, k, n - 1)), na};
          if (negate) {
#pragma unroll
            for (int i = 0; i < 4; ++i) f[i] = (Acc)0 - f[i];
          }
          store_run<BITS, 4>(base + (int64_t)g * (4 * kEsz), f);
        }
      }
    }
  }
}

bool expand_type_ok(const dpf_value_desc* d) {
  if (!d || d->num_leaves != 1 || !fast_int(d)) return false;
  const int b = d->bits[0];
  if (!(b == 8 || b == 16 || b == 32 || b == 64 || b == 128)) return false;
  return d->kind[0] == DPF_LEAF_INT || d->kind[0] == DPF_LEAF_XOR;
}

// One launch of the kernel over `items` items rooted at `root_depth`.
void launch_dcf_expand(DcfExpandParams p, const DcfExpandVcw& vc, int64_t items, int root_depth,
                       int bits, bool xor_mode, bool uniform, hipStream_t s) {
  p.num_items = items;
  p.root_depth = root_depth;
  const LaunchShape sh = chunked_shape(items, "DPF_DCF_EXPAND_DYNAMIC");
  const dim3 grid(sh.grid), block(sh.block);
  p.dyn_per_wg = sh.dyn_per_wg;
  with_bits(bits, [&](auto b) {
    constexpr int B = decltype(b)::value;
    if (xor_mode) {
      if (uniform) hipLaunchKernelGGL((dcf_expand_kernel<B, true, kDcfStack>), grid, block, 0, s, p, vc);
      else hipLaunchKernelGGL((dcf_expand_kernel<B, true, 0>), grid, block, 0, s, p, vc);
    } else {
      if (uniform) hipLaunchKernelGGL((dcf_expand_kernel<B, false, kDcfStack>), grid, block, 0, s, p, vc);
      else hipLaunchKernelGGL((dcf_expand_kernel<B, false, 0>), grid, block, 0, s, p, vc);
    }
  });
}

}  // namespace

extern "C" int dpf_hip_dcf_expand_supported(const dpf_value_desc* desc, int num_levels,
                                            const int32_t* level_depth) {
  if (!expand_type_ok(desc) || !level_depth || num_levels < 1 || num_levels > kDcfExpandMaxLevels)
    return 0;
  for (int i = 0; i < num_levels; ++i)
    if (level_depth[i] != i) return 0;
  return 1;
}

extern "C" int dpf_hip_dcf_expand_plan(int64_t num_keys, int num_levels, int shard_bits,
                                       int num_cus, int64_t out[6]) {
  if (!out) return fail(kInvalidArgument, "NULL plan output");
  if (num_keys < 1 || num_levels < 1 || num_levels > kDcfExpandMaxLevels || shard_bits < 0 ||
      shard_bits > num_levels - 1 || shard_bits > 62 || num_levels - shard_bits > 62 ||
      num_keys > (INT64_MAX >> (num_levels - shard_bits)) || num_cus < 1)
    return fail(kInvalidArgument, "num_keys, num_levels, shard_bits or num_cus out of range");
  const DcfExpandPlan pl = plan_dcf_expand(num_keys, num_levels, shard_bits, num_cus);
  out[0] = pl.G;
  out[1] = pl.walk;
  out[2] = pl.items;
  out[3] = pl.items_per_key;
  out[4] = pl.top_G;
  out[5] = pl.top_items;
  return kOk;
}

extern "C" int dpf_hip_dcf_expand(int64_t num_keys, int num_levels, int shard_bits,
                                  int64_t shard_index, const dpf_block* key_seed,
                                  const uint8_t* party, const dpf_block* cw_seed,
                                  const uint8_t* cw_left, const uint8_t* cw_right, int cw_stride,
                                  const dpf_block* const* value_correction,
                                  const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                                  const dpf_aes_key* key_value, const dpf_value_desc* desc,
                                  void* out, void* stream) {
  const int n = num_levels;
  if (num_keys < 0 || n < 1 || n > kDcfExpandMaxLevels)
    return fail(kInvalidArgument, "num_keys or num_levels out of range");
  if (shard_bits < 0 || shard_bits > n - 1 || shard_bits > 62)
    return fail(kInvalidArgument, "shard_bits must be in [0, num_levels - 1]");
  if (shard_index < 0 || shard_index >= ((int64_t)1 << shard_bits))
    return fail(kInvalidArgument, "shard_index must be in [0, 2^shard_bits)");
  if (n - shard_bits > 62 || num_keys > (INT64_MAX >> (n - shard_bits)))
    return fail(kInvalidArgument, "Output size would be larger than 2**62");
  if (!value_correction || !key_left || !key_right || !key_value)
    return fail(kInvalidArgument, "NULL table");
  for (int i = 0; i < n; ++i)
    if (!value_correction[i]) return fail(kInvalidArgument, "NULL value correction");
  if (cw_stride < n - 1) return fail(kInvalidArgument, "cw_stride too small");
  if (!expand_type_ok(desc))
    return fail(kUnimplemented,
                "full-domain DCF evaluation takes one integer or XorWrapper leaf of 8 to 128 bits");
  if (num_keys == 0) return kOk;
  if (!key_seed || !party || !out || (n > 1 && (!cw_seed || !cw_left || !cw_right)))
    return fail(kInvalidArgument, "NULL table");
  if (((uintptr_t)out & 15) != 0) return fail(kInvalidArgument, "`out` must be 16-byte aligned");
  const DcfExpandPlan pl = plan_dcf_expand(num_keys, n, shard_bits, num_cus());
  DcfExpandParams p;
  memset(&p, 0, sizeof(p));
  p.n = n;
  p.shard_bits = shard_bits;
  p.cw_stride = cw_stride;
  p.vcw_stride = desc->elements_per_block * desc->num_leaves;
  p.shard_index = shard_index;
  p.key_seed = key_seed;
  p.party = party;
  p.cw_seed = cw_seed;
  p.cw_left = cw_left;
  p.cw_right = cw_right;
  p.out = (char*)out;
  const RoundKeys rkr = expand_key(key_right);
  p.rkl = expand_key(key_left);
  p.rkr = rkr;
  p.rkv = expand_key(key_value);
  p.rkd = xor_keys(p.rkl, rkr);
  DcfExpandVcw vc;
  memset(&vc, 0, sizeof(vc));
  for (int i = 0; i < n; ++i) vc.level[i] = value_correction[i];
  const bool xor_mode = desc->kind[0] == DPF_LEAF_XOR;
  hipStream_t s = (hipStream_t)stream;
  const bool top = pl.top_G >= 0;
  if (top) {
    // The items' roots, each left in the first bytes of its item's outputs.
    const int top_root = pl.walk - pl.top_G - 1;
    p.mode = kDcfEmit;
    p.stack = pl.top_G;
    p.walk_levels = top_root;
    p.child_log = pl.G + 1;
    launch_dcf_expand(p, vc, pl.top_items, top_root, desc->bits[0], xor_mode, true, s);
    HIP_TRY(hipGetLastError());
  }
  p.mode = pl.G == 0 ? kDcfLeafNode : kDcfOutputs;
  p.stack = pl.G == 0 ? 0 : pl.G - 1;
  p.walk_levels = top ? 0 : pl.walk;
  p.stored_root = top ? 1 : 0;
  p.child_log = 0;
  launch_dcf_expand(p, vc, pl.items, pl.walk, desc->bits[0], xor_mode,
                    pl.G > 0 && pl.items_per_key % 64 == 0, s);
  HIP_TRY(hipGetLastError());
  return kOk;
}
