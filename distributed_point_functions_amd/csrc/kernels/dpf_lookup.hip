// dpf_lookup.hip -- batched private table lookup on gfx950: the full-domain
// expansion of every key of a key batch folded into one shared public table
// at a per-key rotation,
//   out[k][w] = sum_i y_k[i] * T[(i + s_k) mod N][w]      (uint64_t, mod 2^64)
//   out[k][w] = XOR_i (y_k[i] & T[(i + s_k) mod N][w])    (XorWrapper<uint64_t>)
// with y_k the 2^n shares EvaluateUntil gives for key k.  No share vector is
// stored: a leaf is multiplied with its two table rows as soon as it is hashed.
//
// One thread = one (key, subtree) item.  It walks from the key's root to its
// subtree's root along the bits of its index (one AES per level, as
// eval_points_kernel walks), then visits the subtree depth-first with the
// stack of parked right children in VGPRs (expand_kernel's loop).  The
// correction words are the key's own, read from global memory as
// dcf_expand_kernel reads them: wave-uniform loads where the 64 items of a
// wave share a key, per-lane loads in the instance with several keys per wave.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/dpf_hip.h"
#include "dpf_device.h"
#include "dpf_runtime.h"

using namespace dpf_rt;

namespace {

constexpr int kLookupMaxLogDomain = 40;
// Parked nodes of an item's depth-first walk, per table width: what the 128
// VGPRs of 4 waves per SIMD hold without a spilled VGPR in every instance,
// beside the two AES chains, the W sums and the table rows in flight
// (profiles/r30/kernel_resources_lookup.txt; the instance with a key per lane
// is the one that sets them: one slot more spills 13 to 20 VGPRs there).  An
// item visits at most stack + 1 levels: the leaf pairs share their parent.
template <int W> struct LookupStack;
template <> struct LookupStack<1> { static constexpr int value = 4; };
template <> struct LookupStack<2> { static constexpr int value = 4; };
template <> struct LookupStack<4> { static constexpr int value = 3; };
int lookup_stack(int table_words) {
  return table_words == 1 ? LookupStack<1>::value
                          : (table_words == 2 ? LookupStack<2>::value : LookupStack<4>::value);
}
// Items per CU below which a launch gives up subtree depth for more items.
constexpr int64_t kLookupItemsPerCu = 256;

struct LookupPlan {
  int S, walk;
  int64_t items_per_key, items;
};

// S is the deepest subtree the stack allows -- the deepest S walks the fewest
// levels twice: a key costs L * (walk + 2 (2^S - 1) + 2^S) AES with L = 2^walk
// items -- lowered until the launch has kLookupItemsPerCu items per CU.
LookupPlan plan_lookup(int64_t num_keys, int D, int table_words, int num_cus) {
  const int64_t want = (int64_t)(num_cus < 1 ? 1 : num_cus) * kLookupItemsPerCu;
  const int limit = lookup_stack(table_words) + 1;
  int S = D < limit ? D : limit;
  while (S > 0 && num_keys < ((want + ((int64_t)1 << (D - S)) - 1) >> (D - S))) --S;
  LookupPlan pl;
  pl.S = S;
  pl.walk = D - S;
  pl.items_per_key = (int64_t)1 << pl.walk;
  pl.items = num_keys * pl.items_per_key;
  return pl;
}

struct LookupParams {
  int64_t num_items;
  int walk;         // levels an item walks from its key's root
  int S;            // levels it then visits depth-first
  int log_domain;   // n: the table has 2^n rows
  int seg;          // lanes of a wave that hold one key's items: min(2^walk, 64)
  int atomic;       // 2^walk > 64: the waves of a key meet in `out` by atomics
  int cw_stride;
  const dpf_block* key_seed;
  const uint8_t* party;
  const dpf_block* cw_seed;
  const uint8_t* cw_left;
  const uint8_t* cw_right;
  const dpf_block* vcw;     // [key][2]: the value correction's two elements
  const uint64_t* offsets;  // [key]
  const char* table;        // [2^n][W] uint64
  uint64_t* out;            // [key][W]
  RoundKeys rkl, rkr, rkv, rkd;
  int64_t dyn_per_wg;  // ItemLoop's per_wg (0: grid stride)
};

// One table row: W uint64 words.
template <int W>
struct Row {
  uint64_t w[W];
};
template <int W>
__device__ __forceinline__ Row<W> load_row(const char* table, uint64_t r) {
  Row<W> x;
  const char* p = table + r * (uint64_t)(8 * W);
  if constexpr (W == 1) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    x.w[0] = ((uint64_t)v.y << 32) | v.x;
  } else {
#pragma unroll
    for (int i = 0; i < W; i += 2) {
      const uint4 v = *reinterpret_cast<const uint4*>(p + 8 * i);
      x.w[i] = ((uint64_t)v.y << 32) | v.x;
      x.w[i + 1] = ((uint64_t)v.w << 32) | v.z;
    }
  }
  return x;
}

// The sums of one item: W words.  A leaf block holds elements 2j and 2j + 1,
// which meet the rows (2j + s) mod N and (2j + 1 + s) mod N.
template <bool XOR, int W>
struct LookupAcc {
  uint64_t a[W];
  __device__ __forceinline__ void add(Block4 h, const Row<W>& r0, const Row<W>& r1) {
    const uint64_t y0 = ((uint64_t)h.w1 << 32) | h.w0, y1 = ((uint64_t)h.w3 << 32) | h.w2;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      if (XOR) a[w] ^= (y0 & r0.w[w]) ^ (y1 & r1.w[w]);
      else a[w] += y0 * r0.w[w] + y1 * r1.w[w];
      // Taken leaf by leaf, as DotLeaf::add: left free, the compiler
      // reassociates the chain and keeps the leaves' blocks live.
      asm volatile("" : "+v"(a[w]));
    }
  }
};

// UNIFORM: every wave's items belong to one key (2^walk is a multiple of 64).
template <bool XOR, int W, bool UNIFORM>
__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void lookup_kernel(LookupParams p) {
  __shared__ LdsImage lds;
  __shared__ int next_chunk;   // ItemLoop (dpf_device.h)
  fill_tables(lds.tab);
  if (threadIdx.x == 0) next_chunk = 0;
  __syncthreads();
  const LdsLookup lk = make_lookup(lds, KeySet{key_ref(p.rkl), key_ref(p.rkr), key_ref(p.rkv), key_ref(p.rkd)});
  constexpr int STACK = LookupStack<W>::value;
  // Issuing a leaf pair's four rows before its value hashes holds 8 W VGPRs
  // across them: done where they fit.  The instance with a key per lane also
  // holds its correction words in VGPRs and has room for W = 1 only.
  constexpr bool kLoadFirst = UNIFORM ? W <= 2 : W == 1;
  const int walk = p.walk, S = p.S;
  const int B = S >= 1 ? 1 : 0;   // leaf pairs share their parent
  const int G = S - B;             // depth of the DFS stack
  const int ngroups = 1 << G;
  const uint64_t mask = ((uint64_t)1 << p.log_domain) - 1;
  const int64_t lane = (int64_t)(threadIdx.x & 63);
  // The loop's condition is the wave's: the lanes past the last item of a
  // partly filled wave stay for the cross-lane sums and add zero.
  const ItemLoop items{&next_chunk, p.dyn_per_wg, (p.num_items + 63) / 64, INT64_MAX};
  for (int64_t u = items.first(); u - lane < p.num_items; u = items.next(u)) {
    LookupAcc<XOR, W> acc;
#pragma unroll
    for (int w = 0; w < W; ++w) acc.a[w] = 0;
    const bool live = u < p.num_items;
    int64_t k = u >> walk;
    if (live) {
      if (UNIFORM) k = (int64_t)__builtin_amdgcn_readfirstlane((int)k);
      const int64_t j = u - (k << walk);   // the subtree's index in the key's tree
      const uint32_t party = p.party[k] & 1u;
      const int64_t row0 = k * p.cw_stride;
      const uint64_t s_k = p.offsets[k];
      FastIntLeaf<64, XOR> leaf;
      leaf.party = (int)party;
      {
        const uint64_t c0 = p.vcw[2 * k].low, c1 = p.vcw[2 * k + 1].low;
        leaf.vcw = Block4{(uint32_t)c0, (uint32_t)(c0 >> 32), (uint32_t)c1, (uint32_t)(c1 >> 32)};
      }
      // 1. walk from the key's root to this item's subtree root.
      Block4 s = load_block(p.key_seed + k);
      uint32_t t = party;
      for (int d = 0; d < walk; ++d) {
        const uint32_t bit = (uint32_t)((j >> (walk - 1 - d)) & 1);
        const uint4 cs = cw_u4(p.cw_seed[row0 + d]);
        const uint32_t cc = cw_ctrl2(p.cw_left, p.cw_right, row0 + d);
        Block4 h = dpf_aes::mmo_hash(s, lk, SelectRK{lk.ks.l, lk.ks.d, 0u - bit});
        correct_child(h, t, bit, cs, cc);
        s = h;
      }
      const uint64_t elem_base = ((uint64_t)j << (S + 1)) + s_k;   // element 0 of the item, rotated
      if (S == 0) {
        // The item is one leaf block (n == 1: the key's root).
        const Row<W> r0 = load_row<W>(p.table, elem_base & mask);
        const Row<W> r1 = load_row<W>(p.table, (elem_base + 1) & mask);
        acc.add(leaf.correct(dpf_aes::mmo_hash(s, lk, UniformRK{lk.ks.v}), t), r0, r1);
      } else {
        // 2. depth-first over the subtree (expand_kernel's loop): every inner
        //    node is expanded into both children at once, the left one
        //    descended into and the right one parked; the leaf pairs are
        //    hashed with their parent's two children.
        auto children = [&](Block4 node, uint32_t nt, int d, Block4& c0, uint32_t& t0, Block4& c1,
                            uint32_t& t1) {
          const uint4 cs = cw_u4(p.cw_seed[row0 + d]);
          const uint32_t cc = cw_ctrl2(p.cw_left, p.cw_right, row0 + d);
          children_step(lk, lk.ks.l, lk.ks.r, node, nt, cs, cc, c0, t0, c1, t1);
        };
        Block4 sib[STACK];   // sib[d - 1] = parked right child at depth d
        uint32_t tb = 0;     // bit d = its control bit
        for (int g = 0; g < ngroups; ++g) {
          Block4 node = s;
          uint32_t nt = t;
          int ds = 0;   // depth of `node` (wave-uniform)
          if (g != 0) {
            ds = G - __builtin_ctz((unsigned)g);
#pragma unroll
            for (int d = 1; d <= STACK; ++d)
              if (d == ds) { node = sib[d - 1]; nt = (tb >> d) & 1u; }
          }
          for (int d = ds; d < G; ++d) {
            Block4 c0, c1;
            uint32_t t0, t1;
            children(node, nt, walk + d, c0, t0, c1, t1);
#pragma unroll
            for (int e = 1; e <= STACK; ++e)
              if (e == d + 1) sib[e - 1] = c1;
            tb = (tb & ~(1u << (d + 1))) | (t1 << (d + 1));
            node = c0;
            nt = t0;
          }
          Block4 c0, c1;
          uint32_t t0, t1;
          children(node, nt, walk + G, c0, t0, c1, t1);
          // Leaf blocks 2g and 2g + 1 of the item: four consecutive elements.
          const uint64_t e0 = elem_base + ((uint64_t)g << 2);
          if constexpr (kLoadFirst) {
            const Row<W> r0 = load_row<W>(p.table, e0 & mask);
            const Row<W> r1 = load_row<W>(p.table, (e0 + 1) & mask);
            const Row<W> r2 = load_row<W>(p.table, (e0 + 2) & mask);
            const Row<W> r3 = load_row<W>(p.table, (e0 + 3) & mask);
            dpf_aes::mmo_hash2(c0, c1, lk, UniformRK{lk.ks.v}, UniformRK{lk.ks.v});
            acc.add(leaf.correct(c0, t0), r0, r1);
            acc.add(leaf.correct(c1, t1), r2, r3);
          } else {
            dpf_aes::mmo_hash2(c0, c1, lk, UniformRK{lk.ks.v}, UniformRK{lk.ks.v});
            asm volatile("" ::: "memory");   // the loads follow the hashes
            {
              const Row<W> r0 = load_row<W>(p.table, e0 & mask);
              const Row<W> r1 = load_row<W>(p.table, (e0 + 1) & mask);
              acc.add(leaf.correct(c0, t0), r0, r1);
            }
            {
              const Row<W> r2 = load_row<W>(p.table, (e0 + 2) & mask);
              const Row<W> r3 = load_row<W>(p.table, (e0 + 3) & mask);
              acc.add(leaf.correct(c1, t1), r2, r3);
            }
          }
        }
      }
    }
    // 3. the key's sum: its items sit in `seg` consecutive lanes (a power of
    //    two), so a butterfly below `seg` leaves every lane of the segment
    //    the segment's sum.  The lanes past the last item hold zero and form
    //    whole segments of their own.
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      if (off < p.seg) {
#pragma unroll
        for (int w = 0; w < W; ++w) {
          const uint64_t y = __shfl_xor(acc.a[w], off, 64);
          acc.a[w] = XOR ? acc.a[w] ^ y : acc.a[w] + y;
        }
      }
    }
    if (live && (u & (int64_t)(p.seg - 1)) == 0) {
      uint64_t* o = p.out + k * W;
      if (p.atomic) {
        // Several waves per key: 64-bit atomics onto the row the call
        // cleared in stream order.  Both groups are exact in any order.
#pragma unroll
        for (int w = 0; w < W; ++w) {
          unsigned long long* q = reinterpret_cast<unsigned long long*>(o + w);
          if (XOR) __hip_atomic_fetch_xor(q, (unsigned long long)acc.a[w], __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
          else __hip_atomic_fetch_add(q, (unsigned long long)acc.a[w], __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
        }
      } else {
#pragma unroll
        for (int w = 0; w < W; ++w) o[w] = acc.a[w];
      }
    }
  }
}

bool lookup_type_ok(const dpf_value_desc* d) {
  if (!d || d->num_leaves != 1 || !fast_int(d) || d->bits[0] != 64 || d->elements_per_block != 2)
    return false;
  return d->kind[0] == DPF_LEAF_INT || d->kind[0] == DPF_LEAF_XOR;
}
bool lookup_words_ok(int w) { return w == 1 || w == 2 || w == 4; }

template <bool XOR, int W>
void launch_lookup_w(const LookupParams& p, bool uniform, dim3 grid, dim3 block, hipStream_t s) {
  if (uniform) hipLaunchKernelGGL((lookup_kernel<XOR, W, true>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((lookup_kernel<XOR, W, false>), grid, block, 0, s, p);
}
template <bool XOR>
void launch_lookup(const LookupParams& p, int W, bool uniform, dim3 grid, dim3 block,
                   hipStream_t s) {
  if (W == 1) launch_lookup_w<XOR, 1>(p, uniform, grid, block, s);
  else if (W == 2) launch_lookup_w<XOR, 2>(p, uniform, grid, block, s);
  else launch_lookup_w<XOR, 4>(p, uniform, grid, block, s);
}

}  // namespace

extern "C" int dpf_hip_lookup_supported(const dpf_value_desc* desc, int table_words) {
  return lookup_type_ok(desc) && lookup_words_ok(table_words) ? 1 : 0;
}

extern "C" int dpf_hip_lookup_plan(int64_t num_keys, int tree_depth, int table_words, int num_cus,
                                   int64_t out[4]) {
  if (!out) return fail(kInvalidArgument, "NULL plan output");
  if (num_keys < 1 || num_keys > INT32_MAX || tree_depth < 0 ||
      tree_depth > kLookupMaxLogDomain - 1 || num_cus < 1)
    return fail(kInvalidArgument, "num_keys, tree_depth or num_cus out of range");
  if (!lookup_words_ok(table_words)) return fail(kInvalidArgument, "table_words must be 1, 2 or 4");
  const LookupPlan pl = plan_lookup(num_keys, tree_depth, table_words, num_cus);
  out[0] = pl.S;
  out[1] = pl.walk;
  out[2] = pl.items_per_key;
  out[3] = pl.items;
  return kOk;
}

extern "C" int dpf_hip_lookup_batch(int64_t num_keys, int num_levels, int cw_stride,
                                    int log_domain_size, const dpf_block* key_seed,
                                    const uint8_t* party, const dpf_block* cw_seed,
                                    const uint8_t* cw_left, const uint8_t* cw_right,
                                    const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                                    const dpf_aes_key* key_value, const dpf_value_desc* desc,
                                    const dpf_block* value_correction, const uint64_t* offsets,
                                    const void* table, int table_words, uint64_t* out,
                                    void* stream) {
  if (num_keys < 0 || num_keys > INT32_MAX)
    return fail(kInvalidArgument, "num_keys out of range");
  if (log_domain_size < 1 || log_domain_size > kLookupMaxLogDomain)
    return fail(kInvalidArgument, "log_domain_size must be in [1, 40]");
  if (num_levels != log_domain_size - 1)
    return fail(kInvalidArgument, "num_levels must be log_domain_size - 1");
  if (!desc || !key_left || !key_right || !key_value)
    return fail(kInvalidArgument, "NULL value descriptor or AES key");
  if (!lookup_type_ok(desc))
    return fail(kUnimplemented,
                "the table lookup is implemented for uint64_t and XorWrapper<uint64_t> only");
  if (table_words < 1 || table_words > DPF_HIP_DOT_MAX_RECORD_WORDS)
    return fail(kInvalidArgument, "`table_words` must be in [1, 1024]");
  if (!lookup_words_ok(table_words))
    return fail(kUnimplemented, "the table lookup is implemented for table_words 1, 2 and 4 only");
  if (cw_stride < num_levels) return fail(kInvalidArgument, "cw_stride < num_levels");
  if (num_keys == 0) return kOk;
  if (!key_seed || !party || !value_correction || !offsets || !table || !out ||
      (num_levels > 0 && (!cw_seed || !cw_left || !cw_right)))
    return fail(kInvalidArgument, "NULL pointer");
  if (((uintptr_t)table & (table_words == 1 ? 7 : 15)) != 0 || ((uintptr_t)out & 7) != 0 ||
      ((uintptr_t)offsets & 7) != 0)
    return fail(kInvalidArgument,
                "`table` must be aligned to min(16, 8 * table_words) bytes, `offsets` and `out` to 8");
  const int W = table_words;
  const LookupPlan pl = plan_lookup(num_keys, num_levels, W, num_cus());
  LookupParams p;
  memset(&p, 0, sizeof(p));
  p.num_items = pl.items;
  p.walk = pl.walk;
  p.S = pl.S;
  p.log_domain = log_domain_size;
  p.seg = pl.items_per_key < 64 ? (int)pl.items_per_key : 64;
  p.atomic = pl.items_per_key > 64 ? 1 : 0;
  p.cw_stride = cw_stride;
  p.key_seed = key_seed;
  p.party = party;
  p.cw_seed = cw_seed;
  p.cw_left = cw_left;
  p.cw_right = cw_right;
  p.vcw = value_correction;
  p.offsets = offsets;
  p.table = (const char*)table;
  p.out = out;
  const RoundKeys rkr = expand_key(key_right);
  p.rkl = expand_key(key_left);
  p.rkr = rkr;
  p.rkv = expand_key(key_value);
  p.rkd = xor_keys(p.rkl, rkr);
  hipStream_t s = (hipStream_t)stream;
  if (p.atomic) HIP_TRY(hipMemsetAsync(out, 0, (size_t)num_keys * W * sizeof(uint64_t), s));
  const LaunchShape sh = chunked_shape(pl.items, "DPF_LOOKUP_DYNAMIC");
  p.dyn_per_wg = sh.dyn_per_wg;
  const bool uniform = pl.items_per_key >= 64;
  if (desc->kind[0] == DPF_LEAF_XOR) launch_lookup<true>(p, W, uniform, dim3(sh.grid), dim3(sh.block), s);
  else launch_lookup<false>(p, W, uniform, dim3(sh.grid), dim3(sh.block), s);
  HIP_TRY(hipGetLastError());
  return kOk;
}
