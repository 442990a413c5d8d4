// dpf_expand_rows.hip -- the stateless full-domain expansion of a whole key
// batch into [key][element] share rows in one launch, behind
// dpf_hip_expand_rows (include/dpf_hip.h):
//   rows[k][i] = y_k[i]        for every key k of the batch, i < 2^n,
// with y_k the 2^n shares EvaluateUntil gives for key k (uint64_t or
// XorWrapper<uint64_t>).
//
// lookup_kernel's work shape (dpf_lookup.hip) with the leaf stored where that
// kernel multiplies it with table rows: one thread = one (key, subtree) item,
// which walks from the key's root to its subtree's root along the bits of its
// index and then visits the subtree depth-first with the parked right
// children in VGPRs.  The correction words are the key's own: wave-uniform
// loads where the 64 items of a wave share a key, per-lane loads in the
// instance with several keys per wave.
//
// Stores: a leaf pair is four consecutive elements, so a lane writes 32
// contiguous bytes per pair with two 16-byte stores, and the pairs of an item
// follow one another in its 2^(S+1) * 8 bytes; the lanes of a wave lie one
// item apart.  The L2 is write-back, so the four pairs that fill a 128-byte
// line meet there before the line leaves for memory.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/dpf_hip.h"
#include "dpf_device.h"
#include "dpf_runtime.h"

using namespace dpf_rt;

namespace {

constexpr int kRowsMaxLogDomain = 24;
// Parked nodes of an item's depth-first walk: what the 128 VGPRs of 4 waves
// per SIMD hold without a spilled VGPR in every instance beside the two AES
// chains (profiles/r34/kernel_resources_dot_buckets.txt).  An item visits at
// most stack + 1 levels: the leaf pairs share their parent.
constexpr int kRowsStack = DPF_HIP_EXPAND_ROWS_MAX_SUBTREE - 1;
// Items per CU below which a launch gives up subtree depth for more items.
constexpr int64_t kRowsItemsPerCu = 256;

struct RowsPlan {
  int S, walk;
  int64_t items_per_key, items;
};

// plan_lookup's rule: the deepest subtree the stack allows -- it walks the
// fewest levels twice -- lowered until the launch has kRowsItemsPerCu items
// per CU.
RowsPlan plan_rows(int64_t num_keys, int D, int num_cus) {
  const int64_t want = (int64_t)(num_cus < 1 ? 1 : num_cus) * kRowsItemsPerCu;
  const int limit = kRowsStack + 1;
  int S = D < limit ? D : limit;
  while (S > 0 && num_keys < ((want + ((int64_t)1 << (D - S)) - 1) >> (D - S))) --S;
  RowsPlan pl;
  pl.S = S;
  pl.walk = D - S;
  pl.items_per_key = (int64_t)1 << pl.walk;
  pl.items = num_keys * pl.items_per_key;
  return pl;
}

struct RowsParams {
  int64_t num_items;
  int walk;         // levels an item walks from its key's root
  int S;            // levels it then visits depth-first
  int cw_stride;
  const dpf_block* key_seed;
  const uint8_t* party;
  const dpf_block* cw_seed;
  const uint8_t* cw_left;
  const uint8_t* cw_right;
  const dpf_block* vcw;     // [key][2]: the value correction's two elements
  char* rows;               // [key] rows of 2^n uint64, row_stride bytes apart
  int64_t row_stride;
  RoundKeys rkl, rkr, rkv, rkd;
  int64_t dyn_per_wg;  // ItemLoop's per_wg (0: grid stride)
};

__device__ __forceinline__ void store_leaf(char* p, Block4 b) {
  *reinterpret_cast<uint4*>(p) = make_uint4(b.w0, b.w1, b.w2, b.w3);
}

// UNIFORM: every wave's items belong to one key (2^walk is a multiple of 64).
template <bool XOR, bool UNIFORM>
__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void expand_rows_kernel(RowsParams p) {
  __shared__ LdsImage lds;
  __shared__ int next_chunk;   // ItemLoop (dpf_device.h)
  fill_tables(lds.tab);
  if (threadIdx.x == 0) next_chunk = 0;
  __syncthreads();
  const LdsLookup lk = make_lookup(lds, KeySet{key_ref(p.rkl), key_ref(p.rkr), key_ref(p.rkv), key_ref(p.rkd)});
  constexpr int STACK = kRowsStack;
  const int walk = p.walk, S = p.S;
  const int B = S >= 1 ? 1 : 0;   // leaf pairs share their parent
  const int G = S - B;             // depth of the DFS stack
  const int ngroups = 1 << G;
  const ItemLoop items{&next_chunk, p.dyn_per_wg, (p.num_items + 63) / 64, p.num_items};
  for (int64_t u = items.first(); u < p.num_items; u = items.next(u)) {
    int64_t k = u >> walk;
    if (UNIFORM) k = (int64_t)__builtin_amdgcn_readfirstlane((int)k);
    const int64_t j = u - (k << walk);   // the subtree's index in the key's tree
    const uint32_t party = p.party[k] & 1u;
    const int64_t row0 = k * p.cw_stride;
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
    // The item's 2^(S+1) elements: 2^S leaf blocks of 16 bytes.
    char* const o = p.rows + k * p.row_stride + (j << (S + 4));
    if (S == 0) {
      // The item is one leaf block (n == 1: the key's root).
      store_leaf(o, leaf.correct(dpf_aes::mmo_hash(s, lk, UniformRK{lk.ks.v}), t));
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
        // Leaf blocks 2g and 2g + 1 of the item: 32 contiguous bytes.
        dpf_aes::mmo_hash2(c0, c1, lk, UniformRK{lk.ks.v}, UniformRK{lk.ks.v});
        store_leaf(o + ((int64_t)g << 5), leaf.correct(c0, t0));
        store_leaf(o + ((int64_t)g << 5) + 16, leaf.correct(c1, t1));
      }
    }
  }
}

bool rows_type_ok(const dpf_value_desc* d) {
  if (!d || d->num_leaves != 1 || !fast_int(d) || d->bits[0] != 64 || d->elements_per_block != 2)
    return false;
  return d->kind[0] == DPF_LEAF_INT || d->kind[0] == DPF_LEAF_XOR;
}

template <bool XOR>
void launch_rows(const RowsParams& p, bool uniform, dim3 grid, dim3 block, hipStream_t s) {
  if (uniform) hipLaunchKernelGGL((expand_rows_kernel<XOR, true>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((expand_rows_kernel<XOR, false>), grid, block, 0, s, p);
}

}  // namespace

extern "C" int dpf_hip_expand_rows_supported(const dpf_value_desc* desc) {
  return rows_type_ok(desc) ? 1 : 0;
}

extern "C" int dpf_hip_expand_rows_plan(int64_t num_keys, int tree_depth, int num_cus,
                                        int64_t out[4]) {
  if (!out) return fail(kInvalidArgument, "NULL plan output");
  if (num_keys < 1 || num_keys > INT32_MAX || tree_depth < 0 ||
      tree_depth > kRowsMaxLogDomain - 1 || num_cus < 1)
    return fail(kInvalidArgument, "num_keys, tree_depth or num_cus out of range");
  const RowsPlan pl = plan_rows(num_keys, tree_depth, num_cus);
  out[0] = pl.S;
  out[1] = pl.walk;
  out[2] = pl.items_per_key;
  out[3] = pl.items;
  return kOk;
}

extern "C" int dpf_hip_expand_rows(int64_t num_keys, int num_levels, int cw_stride,
                                   int log_domain_size, const dpf_block* key_seed,
                                   const uint8_t* party, const dpf_block* cw_seed,
                                   const uint8_t* cw_left, const uint8_t* cw_right,
                                   const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                                   const dpf_aes_key* key_value, const dpf_value_desc* desc,
                                   const dpf_block* value_correction, uint64_t* rows,
                                   int64_t row_stride_bytes, void* stream) {
  if (num_keys < 0 || num_keys > INT32_MAX)
    return fail(kInvalidArgument, "num_keys out of range");
  if (log_domain_size < 1 || log_domain_size > kRowsMaxLogDomain)
    return fail(kInvalidArgument, "log_domain_size must be in [1, 24]");
  if (num_levels != log_domain_size - 1)
    return fail(kInvalidArgument, "num_levels must be log_domain_size - 1");
  if (!desc || !key_left || !key_right || !key_value)
    return fail(kInvalidArgument, "NULL value descriptor or AES key");
  if (!rows_type_ok(desc))
    return fail(kUnimplemented,
                "the row expansion is implemented for uint64_t and XorWrapper<uint64_t> only");
  if (cw_stride < num_levels) return fail(kInvalidArgument, "cw_stride < num_levels");
  if (row_stride_bytes < 0 || row_stride_bytes % 16 != 0 ||
      row_stride_bytes < ((int64_t)8 << log_domain_size))
    return fail(kInvalidArgument,
                "row_stride_bytes must be a multiple of 16 and at least 8 * 2^log_domain_size");
  if (num_keys == 0) return kOk;
  if (!key_seed || !party || !value_correction || !rows ||
      (num_levels > 0 && (!cw_seed || !cw_left || !cw_right)))
    return fail(kInvalidArgument, "NULL pointer");
  if (((uintptr_t)rows & 15) != 0)
    return fail(kInvalidArgument, "`rows` must be aligned to 16 bytes");
  const RowsPlan pl = plan_rows(num_keys, num_levels, num_cus());
  RowsParams p;
  memset(&p, 0, sizeof(p));
  p.num_items = pl.items;
  p.walk = pl.walk;
  p.S = pl.S;
  p.cw_stride = cw_stride;
  p.key_seed = key_seed;
  p.party = party;
  p.cw_seed = cw_seed;
  p.cw_left = cw_left;
  p.cw_right = cw_right;
  p.vcw = value_correction;
  p.rows = reinterpret_cast<char*>(rows);
  p.row_stride = row_stride_bytes;
  const RoundKeys rkr = expand_key(key_right);
  p.rkl = expand_key(key_left);
  p.rkr = rkr;
  p.rkv = expand_key(key_value);
  p.rkd = xor_keys(p.rkl, rkr);
  hipStream_t s = (hipStream_t)stream;
  const LaunchShape sh = chunked_shape(pl.items, "DPF_EXPAND_ROWS_DYNAMIC");
  p.dyn_per_wg = sh.dyn_per_wg;
  const bool uniform = pl.items_per_key >= 64;
  if (desc->kind[0] == DPF_LEAF_XOR) launch_rows<true>(p, uniform, dim3(sh.grid), dim3(sh.block), s);
  else launch_rows<false>(p, uniform, dim3(sh.grid), dim3(sh.block), s);
  HIP_TRY(hipGetLastError());
  return kOk;
}
