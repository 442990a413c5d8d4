// dpf_expand_sum.hip -- fused full-domain sum over a key batch on gfx950: the
// private histogram,
//   out[i] = sum_{k<K} y_k[i]  (uint64_t, mod 2^64)
//   out[i] = XOR_{k<K} y_k[i]  (XorWrapper<uint64_t>)          for i in [0, 2^n)
// with y_k the 2^n shares EvaluateUntil gives for key k.  Every key's tree is
// expanded once and no share vector is stored.
//
// Lanes are keys.  A wave is 64 consecutive keys (a key chunk) at one
// wave-uniform tree position; a work item is (key chunk, subtree): the wave
// walks `walk` levels from its keys' roots to the subtree's root along the
// subtree's index and visits the S levels below it depth-first, every lane at
// the same node of its own key's tree, so control flow is uniform as in
// expand_octet_kernel.  The parked siblings are an explicitly indexed scratch
// array per lane, each entry a seed with the control bit in bit 0.  A subtree is
// finished as leaf groups of kSumGroup levels kept in registers (pairs: 2
// leaf blocks, 4 outputs -- octets and quads spill, see kSumGroup); the 64
// keys' outputs of a group are reduced by a halving butterfly across the lanes
// (reduce_lanes) and 4 lanes issue one 64-bit atomic each into one 32-byte
// sector of `out`.
//
// The correction words come from a [level][key] table that
// expand_sum_table_kernel transposes out of the batch's [key][level] rows for
// this call into the caller's workspace, so that every per-level read of a
// wave is coalesced.
//
// K < 64 is correct but uses only K lanes of one wave per item; making tiny
// batches efficient (several subtrees per wave) is not attempted.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../../include/dpf_hip.h"
#include "dpf_device.h"
#include "dpf_runtime.h"

using namespace dpf_rt;

namespace {

constexpr int kSumMaxLogDomain = 30;
// Levels of a leaf group: 1 = pairs (2 leaf blocks, 4 outputs).  The two
// interleaved AES chains of children_step and the per-lane correction word
// already take 101 of the 128 VGPRs of 4 waves per SIMD; a quad's 8 sums and
// second parked node on top spill 12 (add) to 40 (XOR) VGPRs, an octet's 64 to
// 170 (profiles/r31/kernel_resources_expand_sum.txt).  A pair costs 7 cross-lane
// sums and one atomic instruction of 4 lanes per 6 AES hashes.
constexpr int kSumGroup = 1;
// Parked siblings of the deepest walk: a tree of 29 levels less the leaf group.
constexpr int kSumStack = kSumMaxLogDomain - 1 - kSumGroup;
// Wave items per CU below which a launch gives up subtree depth for more
// items: 16 waves per workgroup times the 4 chunks per wave from which
// chunked_shape takes the items dynamically.
constexpr int64_t kSumWaveItemsPerCu = DPF_HIP_EXPAND_SUM_WAVE_ITEMS_PER_CU;

struct SumPlan {
  int S, walk, group;
  int64_t subtrees, wave_items, want;
};

// walk is the smallest depth at which the launch has `want` wave items, as
// long as a subtree keeps the leaf group's levels.  A tree shallower than a
// leaf group (D < kSumGroup, D == 0 included: the root is value-hashed) is one
// smaller group per key chunk: group = D, walk = 0.
SumPlan plan_sum(int64_t num_keys, int D, int num_cus) {
  SumPlan pl;
  const int64_t chunks = (num_keys + 63) / 64;
  pl.group = D < kSumGroup ? D : kSumGroup;
  pl.want = (int64_t)(num_cus < 1 ? 1 : num_cus) * kSumWaveItemsPerCu;
  pl.walk = 0;
  while (pl.walk < D - pl.group && (chunks << pl.walk) < pl.want) ++pl.walk;
  pl.S = D - pl.walk;
  pl.subtrees = (int64_t)1 << pl.walk;
  pl.wave_items = chunks << pl.walk;
  return pl;
}

// Key chunks of the table: the keys rounded up to whole waves.
int64_t padded_keys(int64_t num_keys) { return (num_keys + 63) / 64 * 64; }
// Table layout in the workspace, kp = padded_keys: cw seeds [D][kp] uint4,
// value corrections [kp] uint4, control pairs [D][kp] uint32, party [kp] uint32.
int64_t table_bytes(int64_t num_keys, int D) {
  return padded_keys(num_keys) * ((int64_t)20 * D + 20);
}

struct SumParams {
  int64_t num_keys, kp;
  int64_t wave_items;
  int walk, S;
  const dpf_block* key_seed;
  const uint4* cs;          // [D][kp]
  const uint4* vcw;         // [kp]: the value correction's two elements
  const uint32_t* cc;       // [D][kp]: cw_ctrl2
  const uint32_t* party;    // [kp]
  uint64_t* out;            // [2^n]
  RoundKeys rkl, rkr, rkv, rkd;
  int64_t dyn_per_wg;  // ItemLoop's per_wg (0: grid stride)
};

// Column kk of the table is key min(kk, K - 1): the lanes past the last key of
// a partly filled chunk read a valid key.
__global__ void expand_sum_table_kernel(int64_t K, int64_t kp, int D, int cw_stride,
                                        const dpf_block* cw_seed, const uint8_t* cw_left,
                                        const uint8_t* cw_right, const dpf_block* vcw_in,
                                        const uint8_t* party_in, uint4* cs, uint4* vcw,
                                        uint32_t* cc, uint32_t* party) {
  const int64_t n = kp * (D + 1);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t d = i / kp, kk = i - d * kp;
    const int64_t k = kk < K ? kk : K - 1;
    if (d < D) {
      const int64_t r = k * cw_stride + d;
      cs[i] = cw_u4(cw_seed[r]);
      cc[i] = cw_ctrl2(cw_left, cw_right, r);
    } else {
      const uint64_t c0 = vcw_in[2 * k].low, c1 = vcw_in[2 * k + 1].low;
      vcw[kk] = make_uint4((uint32_t)c0, (uint32_t)(c0 >> 32), (uint32_t)c1, (uint32_t)(c1 >> 32));
      party[kk] = party_in[k] & 1u;
    }
  }
}

// Per-lane correction words of one tree level.
struct SumCws {
  const uint4* cs;
  const uint32_t* cc;
  int64_t kp, kk;
  __device__ __forceinline__ void load(int level, uint4& s, uint32_t& c) const {
    const int64_t i = level * kp + kk;
    s = cs[i];
    c = cc[i];
  }
};

// The leaf group under `node` (L levels, at tree level `level`), depth-first in
// registers: its 2^L leaf blocks' corrected elements into v[BASE, BASE + 2^(L+1)).
template <bool XOR, int L, int BASE, int NV>
__device__ __forceinline__ void sum_group(const LdsLookup& lk, const FastIntLeaf<64, XOR>& leaf,
                                          const SumCws& cws, Block4 node, uint32_t nt, int level,
                                          uint64_t (&v)[NV]) {
  if constexpr (L == 0) {
    const Block4 h = leaf.correct(dpf_aes::mmo_hash(node, lk, UniformRK{lk.ks.v}), nt);
    v[BASE] = ((uint64_t)h.w1 << 32) | h.w0;
    v[BASE + 1] = ((uint64_t)h.w3 << 32) | h.w2;
  } else {
    uint4 cs;
    uint32_t cc;
    cws.load(level, cs, cc);
    Block4 c0, c1;
    uint32_t t0, t1;
    children_step(lk, lk.ks.l, lk.ks.r, node, nt, cs, cc, c0, t0, c1, t1);
    if constexpr (L == 1) {
      dpf_aes::mmo_hash2(c0, c1, lk, UniformRK{lk.ks.v}, UniformRK{lk.ks.v});
      const Block4 a = leaf.correct(c0, t0), b = leaf.correct(c1, t1);
      v[BASE] = ((uint64_t)a.w1 << 32) | a.w0;
      v[BASE + 1] = ((uint64_t)a.w3 << 32) | a.w2;
      v[BASE + 2] = ((uint64_t)b.w1 << 32) | b.w0;
      v[BASE + 3] = ((uint64_t)b.w3 << 32) | b.w2;
    } else {
      sum_group<XOR, L - 1, BASE, NV>(lk, leaf, cws, c0, t0, level + 1, v);
      sum_group<XOR, L - 1, BASE + (1 << L), NV>(lk, leaf, cws, c1, t1, level + 1, v);
    }
  }
}

// Halving butterfly over the 64 lanes of NV = 2^H values each: step s (offset
// 32 >> s) leaves a lane the half of its remaining values that its lane bit
// 5 - s selects (set: the upper half), summed with the partner's; after H steps
// one value is left, output o = lane >> (6 - H), and the remaining 6 - H
// offsets sum it over the lanes that share o.  Every lane then holds the
// 64-key total of output lane >> (6 - H): 2^H - 1 + 6 - H sums (7 for a
// pair's 4 values, whose output o sits in lanes 16 o .. 16 o + 15; 17 for an
// octet's 16, output o in lanes 4 o .. 4 o + 3).
template <bool XOR, int NV>
__device__ __forceinline__ uint64_t reduce_lanes(uint64_t (&v)[NV], int lane) {
  constexpr int H = NV == 16 ? 4 : (NV == 8 ? 3 : (NV == 4 ? 2 : 1));
#pragma unroll
  for (int st = 0; st < H; ++st) {
    const int off = 32 >> st, half = NV >> (st + 1);
    const bool up = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < NV / 2; ++i) {
      if (i < half) {
        const uint64_t send = up ? v[i] : v[i + half];
        const uint64_t keep = up ? v[i + half] : v[i];
        const uint64_t got = __shfl_xor(send, off, 64);
        v[i] = XOR ? keep ^ got : keep + got;
      }
    }
  }
#pragma unroll
  for (int off = 32 >> H; off > 0; off >>= 1) {
    const uint64_t got = __shfl_xor(v[0], off, 64);
    v[0] = XOR ? v[0] ^ got : v[0] + got;
  }
  return v[0];
}

// LG: the levels of a leaf group, kSumGroup or the whole of a shallower tree.
template <bool XOR, int LG>
__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void expand_sum_kernel(SumParams p) {
  __shared__ LdsImage lds;
  __shared__ int next_chunk;   // ItemLoop (dpf_device.h)
  fill_tables(lds.tab);
  if (threadIdx.x == 0) next_chunk = 0;
  __syncthreads();
  const LdsLookup lk = make_lookup(lds, KeySet{key_ref(p.rkl), key_ref(p.rkr), key_ref(p.rkv), key_ref(p.rkd)});
  constexpr int NV = 2 << LG;       // outputs of a leaf group
  constexpr int OSHIFT = 5 - LG;    // reduce_lanes: output o in lanes o << OSHIFT ...
  const int walk = p.walk;
  const int G = p.S - LG;           // depth of the DFS stack above the leaf groups
  const int64_t ngroups = (int64_t)1 << G;
  const int lane = (int)(threadIdx.x & 63);
  // The loop runs over wave items: the 64 lanes of a wave take the 64 "items"
  // of one chunk, which are one wave item.
  const ItemLoop items{&next_chunk, p.dyn_per_wg, p.wave_items, INT64_MAX};
  const int64_t end = p.wave_items * 64;
  for (int64_t u = items.first(); u < end; u = items.next(u)) {
    const int w = __builtin_amdgcn_readfirstlane((int)(u >> 6));
    const int chunk = w >> walk;
    // Each key chunk starts its round over the subtrees at a subtree of its
    // own, and visits a subtree's leaf groups in an order of its own (`rot`
    // swaps the children at the levels whose bit is set): resident waves do
    // not all add into the same line of `out` at the same moment.
    const int j = (w + chunk) & ((1 << walk) - 1);
    const uint32_t rot = G > 0 ? ((uint32_t)chunk * 0x9E3779B1u) >> (32 - G) : 0u;
    const int64_t kk = (int64_t)chunk * 64 + lane;
    const bool live = kk < p.num_keys;
    const SumCws cws{p.cs, p.cc, p.kp, kk};
    FastIntLeaf<64, XOR> leaf;
    const uint32_t party = p.party[kk];
    leaf.party = (int)party;
    {
      const uint4 c = p.vcw[kk];
      leaf.vcw = Block4{c.x, c.y, c.z, c.w};
    }
    // 1. walk from the keys' roots to this item's subtree root.
    Block4 s = load_block(p.key_seed + (live ? kk : p.num_keys - 1));
    uint32_t t = party;
    for (int d = 0; d < walk; ++d) {
      const uint32_t bit = (uint32_t)((j >> (walk - 1 - d)) & 1);
      uint4 cs;
      uint32_t cc;
      cws.load(d, cs, cc);
      Block4 h = dpf_aes::mmo_hash(s, lk, SelectRK{lk.ks.l, lk.ks.d, 0u - bit});
      correct_child(h, t, bit, cs, cc);
      s = h;
    }
    // 2. depth-first down to the leaf groups' roots (expand_octet_kernel's
    //    loop): the child visited second is parked in sib[d] (scratch) with
    //    its control bit in bit 0, which a corrected seed has clear.
    Block4 sib[kSumStack > 0 ? kSumStack : 1];
    for (int64_t g = 0; g < ngroups; ++g) {
      Block4 node = s;
      uint32_t nt = t;
      int ds = 0;
      if (g != 0) {
        ds = G - (int)__builtin_ctzll((unsigned long long)g);
        node = sib[ds - 1];
        nt = node.w0 & 1u;
        node.w0 &= ~1u;
      }
      for (int d = ds; d < G; ++d) {
        uint4 cs;
        uint32_t cc;
        cws.load(walk + d, cs, cc);
        Block4 c0, c1;
        uint32_t t0, t1;
        children_step(lk, lk.ks.l, lk.ks.r, node, nt, cs, cc, c0, t0, c1, t1);
        const bool swap = ((rot >> (G - 1 - d)) & 1u) != 0;   // wave-uniform
        const Block4 first = swap ? c1 : c0, second = swap ? c0 : c1;
        sib[d] = Block4{second.w0 | (swap ? t0 : t1), second.w1, second.w2, second.w3};
        node = first;
        nt = swap ? t1 : t0;
      }
      // 3. the leaf group, its reduction over the 64 keys, and the atomics.
      uint64_t v[NV];
      sum_group<XOR, LG, 0, NV>(lk, leaf, cws, node, nt, walk + G, v);
      if (!live) {
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = 0;
      }
      const uint64_t total = reduce_lanes<XOR, NV>(v, lane);
      if ((lane & ((1 << OSHIFT) - 1)) == 0) {
        const int64_t group = ((int64_t)j << G) | (int64_t)((uint32_t)g ^ rot);
        unsigned long long* q = reinterpret_cast<unsigned long long*>(
            p.out + (group << (LG + 1)) + (lane >> OSHIFT));
        // Both groups are exact in any order.
        if (XOR) __hip_atomic_fetch_xor(q, (unsigned long long)total, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
        else __hip_atomic_fetch_add(q, (unsigned long long)total, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

bool sum_type_ok(const dpf_value_desc* d) {
  if (!d || d->num_leaves != 1 || !fast_int(d) || d->bits[0] != 64 || d->elements_per_block != 2)
    return false;
  return d->kind[0] == DPF_LEAF_INT || d->kind[0] == DPF_LEAF_XOR;
}

template <bool XOR>
void launch_sum(const SumParams& p, int group, dim3 grid, dim3 block, hipStream_t s) {
  static_assert(kSumGroup == 1, "one instance per leaf-group depth up to kSumGroup");
  if (group == 0) hipLaunchKernelGGL((expand_sum_kernel<XOR, 0>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((expand_sum_kernel<XOR, 1>), grid, block, 0, s, p);
}

}  // namespace

extern "C" int dpf_hip_expand_sum_supported(const dpf_value_desc* desc) {
  return sum_type_ok(desc) ? 1 : 0;
}

extern "C" int64_t dpf_hip_expand_sum_workspace_bytes(int64_t num_keys, int num_levels) {
  if (num_keys < 0 || num_keys > INT32_MAX || num_levels < 0 ||
      num_levels > kSumMaxLogDomain - 1)
    return -1;
  return table_bytes(num_keys, num_levels);
}

extern "C" int dpf_hip_expand_sum_plan(int64_t num_keys, int tree_depth, int num_cus,
                                       int64_t out[6]) {
  if (!out) return fail(kInvalidArgument, "NULL plan output");
  if (num_keys < 1 || num_keys > INT32_MAX || tree_depth < 0 ||
      tree_depth > kSumMaxLogDomain - 1 || num_cus < 1 || num_cus > 65536)
    return fail(kInvalidArgument, "num_keys, tree_depth or num_cus out of range");
  const SumPlan pl = plan_sum(num_keys, tree_depth, num_cus);
  out[0] = pl.S;
  out[1] = pl.walk;
  out[2] = pl.subtrees;
  out[3] = pl.wave_items;
  out[4] = pl.group;
  out[5] = pl.want;
  return kOk;
}

extern "C" int dpf_hip_expand_sum(int64_t num_keys, int num_levels, int cw_stride,
                                  int log_domain_size, const dpf_block* key_seed,
                                  const uint8_t* party, const dpf_block* cw_seed,
                                  const uint8_t* cw_left, const uint8_t* cw_right,
                                  const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                                  const dpf_aes_key* key_value, const dpf_value_desc* desc,
                                  const dpf_block* value_correction, void* workspace,
                                  int64_t workspace_bytes, uint64_t* out, int accumulate,
                                  void* stream) {
  if (num_keys < 0 || num_keys > INT32_MAX)
    return fail(kInvalidArgument, "num_keys out of range");
  if (log_domain_size < 1 || log_domain_size > kSumMaxLogDomain)
    return fail(kInvalidArgument, "log_domain_size must be in [1, 30]");
  if (num_levels != log_domain_size - 1)
    return fail(kInvalidArgument, "num_levels must be log_domain_size - 1");
  if (!desc || !key_left || !key_right || !key_value)
    return fail(kInvalidArgument, "NULL value descriptor or AES key");
  if (!sum_type_ok(desc))
    return fail(kUnimplemented,
                "the full-domain sum is implemented for uint64_t and XorWrapper<uint64_t> only");
  if (cw_stride < num_levels) return fail(kInvalidArgument, "cw_stride < num_levels");
  if (!out) return fail(kInvalidArgument, "`out` is NULL");
  hipStream_t s = (hipStream_t)stream;
  const size_t out_bytes = ((size_t)1 << log_domain_size) * sizeof(uint64_t);
  if (num_keys == 0) {
    // The empty sum.
    if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, out_bytes, s));
    return kOk;
  }
  if (!key_seed || !party || !value_correction ||
      (num_levels > 0 && (!cw_seed || !cw_left || !cw_right)))
    return fail(kInvalidArgument, "NULL pointer");
  const int64_t need = table_bytes(num_keys, num_levels);
  if (!workspace || workspace_bytes < need)
    return fail(kResourceExhausted, "the full-domain sum needs a workspace of " +
                                        std::to_string((long long)need) + " bytes");
  if (((uintptr_t)out & 15) != 0 || ((uintptr_t)workspace & 15) != 0)
    return fail(kInvalidArgument, "`out` and `workspace` must be aligned to 16 bytes");
  const int D = num_levels;
  const SumPlan pl = plan_sum(num_keys, D, num_cus());
  SumParams p;
  memset(&p, 0, sizeof(p));
  p.num_keys = num_keys;
  p.kp = padded_keys(num_keys);
  p.wave_items = pl.wave_items;
  p.walk = pl.walk;
  p.S = pl.S;
  p.key_seed = key_seed;
  char* ws = static_cast<char*>(workspace);
  uint4* cs = reinterpret_cast<uint4*>(ws);
  uint4* vcw = cs + (int64_t)D * p.kp;
  uint32_t* cc = reinterpret_cast<uint32_t*>(vcw + p.kp);
  uint32_t* pty = cc + (int64_t)D * p.kp;
  p.cs = cs;
  p.vcw = vcw;
  p.cc = cc;
  p.party = pty;
  p.out = out;
  const RoundKeys rkr = expand_key(key_right);
  p.rkl = expand_key(key_left);
  p.rkr = rkr;
  p.rkv = expand_key(key_value);
  p.rkd = xor_keys(p.rkl, rkr);
  {
    const int64_t n = p.kp * (D + 1);
    int64_t g = (n + 255) / 256;
    const int64_t cap = (int64_t)num_cus() * 8;
    if (g > cap) g = cap;
    hipLaunchKernelGGL(expand_sum_table_kernel, dim3((unsigned)g), dim3(256), 0, s, num_keys, p.kp,
                       D, cw_stride, cw_seed, cw_left, cw_right, value_correction, party, cs, vcw,
                       cc, pty);
    HIP_TRY(hipGetLastError());
  }
  if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, out_bytes, s));
  const LaunchShape sh = chunked_shape(pl.wave_items * 64, "DPF_EXPAND_SUM_DYNAMIC");
  p.dyn_per_wg = sh.dyn_per_wg;
  if (desc->kind[0] == DPF_LEAF_XOR) launch_sum<true>(p, pl.group, dim3(sh.grid), dim3(sh.block), s);
  else launch_sum<false>(p, pl.group, dim3(sh.grid), dim3(sh.block), s);
  HIP_TRY(hipGetLastError());
  return kOk;
}
