// dpf_expand_sum.hip -- fused full-domain sum over a key batch on gfx950: the
// private histogram,
//   out[i] = sum_{k<K} y_k[i]  (uintB_t, mod 2^B, B in {8, 16, 32, 64})
//   out[i] = XOR_{k<K} y_k[i]  (XorWrapper<uintB_t>, B up to 128)  for i in [0, 2^n)
// with y_k the 2^n shares EvaluateUntil gives for key k.  Every key's tree is
// expanded once and no share vector is stored.  A leaf block is E = 128 / B
// packed elements and, whatever B, two 64-bit words of `out`: the walk, the
// stack and the plan see only the tree (depth n - log2 E), and the width
// enters in the correction (FastIntLeaf<B>), in the element-wise word sum of
// the reduction (word_add) and in the atomics (add_into).  XOR of words is XOR
// of their packed elements: every XOR width runs the 64-bit instance.
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
// (reduce_lanes) and 4 lanes issue one 64-bit atomic each (two 32-bit ones,
// or a compare-exchange loop below 32 bits: add_into) into one 32-byte sector
// of `out`.
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
  const uint4* vcw;         // [kp]: the value correction's E packed elements
  const uint32_t* cc;       // [D][kp]: cw_ctrl2
  const uint32_t* party;    // [kp]
  uint64_t* out;            // [2^(D + 1)] words: 2^n packed elements
  RoundKeys rkl, rkr, rkv, rkd;
  int64_t dyn_per_wg;  // ItemLoop's per_wg (0: grid stride)
};

// Column kk of the table is key min(kk, K - 1): the lanes past the last key of
// a partly filled chunk read a valid key.  A key's E = 128 / bits value
// correction elements (one dpf_block each, key-major) are packed into one
// block, element e at bit e * bits: FastIntLeaf::init's layout.
__global__ void expand_sum_table_kernel(int64_t K, int64_t kp, int D, int cw_stride, int bits,
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
      uint64_t c0, c1;
      if (bits == 128) {
        c0 = vcw_in[k].low;
        c1 = vcw_in[k].high;
      } else {
        const int per = 64 / bits;   // elements of a word
        const uint64_t mask = bits == 64 ? ~(uint64_t)0 : ((uint64_t)1 << bits) - 1;
        const dpf_block* in = vcw_in + k * (2 * per);
        c0 = c1 = 0;
        for (int e = 0; e < per; ++e) {
          c0 |= (in[e].low & mask) << (e * bits);
          c1 |= (in[per + e].low & mask) << (e * bits);
        }
      }
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
template <int BITS, bool XOR, int L, int BASE, int NV>
__device__ __forceinline__ void sum_group(const LdsLookup& lk, const FastIntLeaf<BITS, XOR>& leaf,
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
      sum_group<BITS, XOR, L - 1, BASE, NV>(lk, leaf, cws, c0, t0, level + 1, v);
      sum_group<BITS, XOR, L - 1, BASE + (1 << L), NV>(lk, leaf, cws, c1, t1, level + 1, v);
    }
  }
}

// Element-wise sum mod 2^BITS of two words of 64 / BITS packed elements.  Below
// 32 bits the elements' top bits H are added apart from the rest, so that no
// carry crosses an element's top (lanes_add's form, on a word).
template <int BITS>
__device__ __forceinline__ uint64_t word_add(uint64_t a, uint64_t b) {
  if constexpr (BITS == 64) {
    return a + b;
  } else if constexpr (BITS == 32) {
    const uint32_t lo = (uint32_t)a + (uint32_t)b, hi = (uint32_t)(a >> 32) + (uint32_t)(b >> 32);
    return ((uint64_t)hi << 32) | lo;
  } else {
    constexpr uint64_t H = BITS == 16 ? 0x8000800080008000ull : 0x8080808080808080ull;
    return ((a & ~H) + (b & ~H)) ^ ((a ^ b) & H);
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
template <int BITS, bool XOR, int NV>
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
        v[i] = XOR ? keep ^ got : word_add<BITS>(keep, got);
      }
    }
  }
#pragma unroll
  for (int off = 32 >> H; off > 0; off >>= 1) {
    const uint64_t got = __shfl_xor(v[0], off, 64);
    v[0] = XOR ? v[0] ^ got : word_add<BITS>(v[0], got);
  }
  return v[0];
}

// A word's total into `out`.  Both groups are exact in any order.  64 bits and
// XOR: one atomic; 32 bits: one native add per element.  Below that there is
// no packed atomic add and a plain add would carry into the neighbour: a
// compare-exchange loop on the word.  It waits on no other wave (an exchange
// fails only because another one succeeded), so it ends under any schedule.
template <int BITS, bool XOR>
__device__ __forceinline__ void add_into(uint64_t* out, uint64_t total) {
  unsigned long long* q = reinterpret_cast<unsigned long long*>(out);
  if constexpr (XOR) {
    __hip_atomic_fetch_xor(q, (unsigned long long)total, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  } else if constexpr (BITS == 64) {
    __hip_atomic_fetch_add(q, (unsigned long long)total, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  } else if constexpr (BITS == 32) {
    uint32_t* q32 = reinterpret_cast<uint32_t*>(out);
    __hip_atomic_fetch_add(q32, (uint32_t)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(q32 + 1, (uint32_t)(total >> 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  } else {
    unsigned long long seen = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (!__hip_atomic_compare_exchange_weak(q, &seen,
                                               (unsigned long long)word_add<BITS>(seen, total),
                                               __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT)) {
    }
  }
}

// The kernel of every width.  SHAPE is sum_shape(bits, LG): the levels LG of a
// leaf group (kSumGroup, or the whole of a shallower tree) with the additive
// element's bits 8, 16 or 32 above them, and nothing there for 64 bits and for
// XOR (which is blind to the element width: one instance runs every XOR
// type).  So the 64-bit instances have the template arguments, the symbols and
// the code they had when the kernel took 64 bits alone
// (profiles/r35/kernel_digest_compare.txt).
constexpr int sum_shape(int bits, int lg) { return lg | ((bits == 64 ? 0 : bits) << 8); }

template <bool XOR, int SHAPE>
__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void expand_sum_kernel(SumParams p) {
  constexpr int LG = SHAPE & 255;
  constexpr int BITS = (SHAPE >> 8) == 0 ? 64 : (SHAPE >> 8);
  static_assert(BITS == 64 || (!XOR && (BITS == 8 || BITS == 16 || BITS == 32)), "element width");
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
    FastIntLeaf<BITS, XOR> leaf;
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
      sum_group<BITS, XOR, LG, 0, NV>(lk, leaf, cws, node, nt, walk + G, v);
      if (!live) {
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = 0;
      }
      const uint64_t total = reduce_lanes<BITS, XOR, NV>(v, lane);
      if ((lane & ((1 << OSHIFT) - 1)) == 0) {
        const int64_t group = ((int64_t)j << G) | (int64_t)((uint32_t)g ^ rot);
        add_into<BITS, XOR>(p.out + (group << (LG + 1)) + (lane >> OSHIFT), total);
      }
    }
  }
}

bool sum_type_ok(const dpf_value_desc* d) {
  if (!d || d->num_leaves != 1 || !fast_int(d) || d->bits[0] != 64 || d->elements_per_block != 2)
    return false;
  return d->kind[0] == DPF_LEAF_INT || d->kind[0] == DPF_LEAF_XOR;
}

// The packed call's types: one unsigned integer leaf of 8 to 64 bits, or
// XorWrapper of one of 8 to 128 bits, E = 128 / bits elements to a block.
bool packed_type_ok(const dpf_value_desc* d) {
  if (!d || d->num_leaves != 1 || !fast_int(d)) return false;
  const int bits = d->bits[0];
  if (bits != 8 && bits != 16 && bits != 32 && bits != 64 && bits != 128) return false;
  if (d->elements_per_block != 128 / bits) return false;
  if (d->kind[0] == DPF_LEAF_XOR) return true;
  return d->kind[0] == DPF_LEAF_INT && bits != 128;
}

int log2_elements(int bits) {
  int l = 0;
  while ((128 / bits) >> (l + 1)) ++l;
  return l;
}

template <bool XOR, int BITS>
void launch_sum(const SumParams& p, int group, dim3 grid, dim3 block, hipStream_t s) {
  static_assert(kSumGroup == 1, "one instance per leaf-group depth up to kSumGroup");
  if (group == 0)
    hipLaunchKernelGGL((expand_sum_kernel<XOR, sum_shape(BITS, 0)>), grid, block, 0, s, p);
  else
    hipLaunchKernelGGL((expand_sum_kernel<XOR, sum_shape(BITS, 1)>), grid, block, 0, s, p);
}

// Both entry points from the empty batch on (their checks 6 to 9 and the two
// launches): a tree of D levels over blocks of 128 / bits elements, `out` of
// 16 * 2^D bytes.
int run_sum(int64_t num_keys, int D, int cw_stride, int bits, bool is_xor,
            const dpf_block* key_seed, const uint8_t* party, const dpf_block* cw_seed,
            const uint8_t* cw_left, const uint8_t* cw_right, const dpf_aes_key* key_left,
            const dpf_aes_key* key_right, const dpf_aes_key* key_value,
            const dpf_block* value_correction, void* workspace, int64_t workspace_bytes,
            void* out, int accumulate, hipStream_t s) {
  const size_t out_bytes = (size_t)16 << D;
  if (num_keys == 0) {
    // The empty sum.
    if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, out_bytes, s));
    return kOk;
  }
  if (!key_seed || !party || !value_correction || (D > 0 && (!cw_seed || !cw_left || !cw_right)))
    return fail(kInvalidArgument, "NULL pointer");
  const int64_t need = table_bytes(num_keys, D);
  if (!workspace || workspace_bytes < need)
    return fail(kResourceExhausted, "the full-domain sum needs a workspace of " +
                                        std::to_string((long long)need) + " bytes");
  if (((uintptr_t)out & 15) != 0 || ((uintptr_t)workspace & 15) != 0)
    return fail(kInvalidArgument, "`out` and `workspace` must be aligned to 16 bytes");
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
  p.out = static_cast<uint64_t*>(out);
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
                       D, cw_stride, bits, cw_seed, cw_left, cw_right, value_correction, party, cs,
                       vcw, cc, pty);
    HIP_TRY(hipGetLastError());
  }
  if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, out_bytes, s));
  const LaunchShape sh = chunked_shape(pl.wave_items * 64, "DPF_EXPAND_SUM_DYNAMIC");
  p.dyn_per_wg = sh.dyn_per_wg;
  const dim3 grid(sh.grid), block(sh.block);
  if (is_xor) launch_sum<true, 64>(p, pl.group, grid, block, s);
  else if (bits == 64) launch_sum<false, 64>(p, pl.group, grid, block, s);
  else if (bits == 32) launch_sum<false, 32>(p, pl.group, grid, block, s);
  else if (bits == 16) launch_sum<false, 16>(p, pl.group, grid, block, s);
  else launch_sum<false, 8>(p, pl.group, grid, block, s);
  HIP_TRY(hipGetLastError());
  return kOk;
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
  return run_sum(num_keys, num_levels, cw_stride, 64, desc->kind[0] == DPF_LEAF_XOR, key_seed,
                 party, cw_seed, cw_left, cw_right, key_left, key_right, key_value,
                 value_correction, workspace, workspace_bytes, out, accumulate,
                 (hipStream_t)stream);
}

extern "C" int dpf_hip_expand_sum_packed_supported(const dpf_value_desc* desc) {
  return packed_type_ok(desc) ? 1 : 0;
}

extern "C" int dpf_hip_expand_sum_packed(int64_t num_keys, int num_levels, int cw_stride,
                                         int log_domain_size, const dpf_block* key_seed,
                                         const uint8_t* party, const dpf_block* cw_seed,
                                         const uint8_t* cw_left, const uint8_t* cw_right,
                                         const dpf_aes_key* key_left,
                                         const dpf_aes_key* key_right,
                                         const dpf_aes_key* key_value, const dpf_value_desc* desc,
                                         const dpf_block* value_correction, void* workspace,
                                         int64_t workspace_bytes, void* out, int64_t out_bytes,
                                         int accumulate, void* stream) {
  if (num_keys < 0 || num_keys > INT32_MAX)
    return fail(kInvalidArgument, "num_keys out of range");
  if (log_domain_size < 0 || log_domain_size > kSumMaxLogDomain)
    return fail(kInvalidArgument, "log_domain_size must be in [0, 30]");
  if (!desc || !key_left || !key_right || !key_value)
    return fail(kInvalidArgument, "NULL value descriptor or AES key");
  if (!packed_type_ok(desc))
    return fail(kUnimplemented,
                "the packed full-domain sum is implemented for uint8_t, uint16_t, uint32_t, "
                "uint64_t and XorWrapper of these and of absl::uint128, over a domain of at "
                "least one full leaf block");
  const int bits = desc->bits[0];
  if (num_levels != log_domain_size - log2_elements(bits) || num_levels < 0 ||
      num_levels > kSumMaxLogDomain - 1)
    return fail(kInvalidArgument,
                "num_levels must be log_domain_size - log2(elements per block), in [0, 29]: "
                "at least one full leaf block");
  if (cw_stride < num_levels) return fail(kInvalidArgument, "cw_stride < num_levels");
  if (!out) return fail(kInvalidArgument, "`out` is NULL");
  if (out_bytes < ((int64_t)16 << num_levels))
    return fail(kInvalidArgument, "`out` is smaller than 2^log_domain_size elements");
  return run_sum(num_keys, num_levels, cw_stride, bits, desc->kind[0] == DPF_LEAF_XOR, key_seed,
                 party, cw_seed, cw_left, cw_right, key_left, key_right, key_value,
                 value_correction, workspace, workspace_bytes, out, accumulate,
                 (hipStream_t)stream);
}
