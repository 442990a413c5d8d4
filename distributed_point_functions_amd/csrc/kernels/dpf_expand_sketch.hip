// dpf_expand_sketch.hip -- checked private histograms on gfx950: the fused
// full-domain field sum over a key batch with every key's linear sketches
// (DESIGN.md section 6h).  For IntModN<uint32_t, N_0> or a 2-tuple of such
// (nl leaves, E == 1, tree depth D = n), y_k the 2^n shares EvaluateUntil
// gives for key k and J <= 2 rows of public 32-bit weights:
//   sum[i][e]       = ( sum_{k<K} y_k[i][e] ) mod N_e
//   sketch[k][j][e] = ( sum_{i<2^n} (w[j][i] mod N_e) * y_k[i][e] ) mod N_e
// Every key's tree is expanded once and no share vector is stored.
//
// The work shape is expand_sum_kernel's (dpf_expand_sum.hip): lanes are keys,
// a wave is 64 consecutive keys at one wave-uniform tree position, a wave item
// is (key chunk, subtree): `walk` levels from the roots, then S levels
// depth-first over an explicitly indexed per-lane stack, finishing in leaf
// pairs (one children_step and Mod32Leaf<2>::hash2 of the two children).
// What differs:
//   - leaves are sampled (Mod32Leaf<2>::convert) from b = nl hashed blocks;
//   - the 64 keys' values of a leaf pair are reduced over the lanes as
//     unreduced 64-bit integers (each below 2^32: a 64-key total is below
//     2^38) and added with 64-bit atomics to a uint64 [2^n][nl] accumulator
//     in the workspace, exact for any K < 2^31;
//   - a key's sketch is a lane-private sum: J * nl 64-bit accumulators per
//     lane across the wave item, the leaf's reduced weights read from
//     wred[i][j][e] with scalar loads (the leaf index is wave-uniform), one
//     mul_mod per (j, e) and leaf (a term is below 2^32, at most 2^28 leaves),
//     and one 64-bit atomic per (j, e) and lane at the end of the item into a
//     uint64 [Kp][J][nl] accumulator;
//   - expand_sketch_finish_kernel reduces both accumulators mod N_e into the
//     caller's uint32 outputs (adding what `sum` held when accumulating).
// expand_sketch_table_kernel mirrors expand_sum_table_kernel (the value
// corrections are nl 32-bit words per key here), expand_sketch_weights_kernel
// writes wred.
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

constexpr int kSkMaxLogDomain = DPF_HIP_EXPAND_SKETCH_MAX_LOG_DOMAIN;   // tree depth D = n
constexpr int kSkMaxWeights = 2;
// Levels of a leaf group: 1 = pairs (one children_step, hash2 of its children).
constexpr int kSkGroup = 1;
// Parked siblings of the deepest walk: a tree of 28 levels less the leaf group.
constexpr int kSkStack = kSkMaxLogDomain - kSkGroup;
constexpr int64_t kSkWaveItemsPerCu = DPF_HIP_EXPAND_SKETCH_WAVE_ITEMS_PER_CU;

struct SkPlan {
  int S, walk, group;
  int64_t subtrees, wave_items, want;
};

// The wave-items threshold: kSkWaveItemsPerCu per CU, or the whole launch's
// figure from DPF_EXPAND_SKETCH_WAVE_ITEMS (read per call; test and A/B hook).
int64_t want_items(int num_cus) {
  const long long h = hook_long("DPF_EXPAND_SKETCH_WAVE_ITEMS", 0);
  if (h >= 1) return h > (1 << 24) ? (int64_t)1 << 24 : (int64_t)h;   // wave items fit an int
  return (int64_t)(num_cus < 1 ? 1 : num_cus) * kSkWaveItemsPerCu;
}

// walk is the smallest depth at which the launch has `want` wave items, as
// long as a subtree keeps the leaf group's level.  Small case: a tree with no
// level (D == 0) has no leaf group: group = walk = S = 0.  The value types of
// this call have D = n >= 1, so that case is planned and never launched.
SkPlan plan_sketch(int64_t num_keys, int D, int num_cus) {
  SkPlan pl;
  const int64_t chunks = (num_keys + 63) / 64;
  pl.group = D < kSkGroup ? D : kSkGroup;
  pl.want = want_items(num_cus);
  pl.walk = 0;
  while (pl.walk < D - pl.group && (chunks << pl.walk) < pl.want) ++pl.walk;
  pl.S = D - pl.walk;
  pl.subtrees = (int64_t)1 << pl.walk;
  pl.wave_items = chunks << pl.walk;
  return pl;
}

int64_t padded_keys(int64_t num_keys) { return (num_keys + 63) / 64 * 64; }

// Workspace layout, kp = padded_keys, N = 2^n (every part a multiple of 256
// bytes, or the last):
//   cw seeds [D][kp] uint4 | control pairs [D][kp] uint32 | value corrections
//   [kp] uint2 | party [kp] uint32 | sum accumulator [N][nl] uint64 | sketch
//   accumulator [kp][J][nl] uint64 | wred [N][J][nl] uint32
struct SkLayout {
  int64_t cs, cc, vcw, party, acc_sum, acc_sk, wred, bytes;
};
SkLayout layout(int64_t num_keys, int D, int n, int nl, int J) {
  const int64_t kp = padded_keys(num_keys), N = (int64_t)1 << n;
  SkLayout l;
  l.cs = 0;
  l.cc = l.cs + 16 * D * kp;
  l.vcw = l.cc + 4 * D * kp;
  l.party = l.vcw + 8 * kp;
  l.acc_sum = l.party + 4 * kp;
  l.acc_sk = l.acc_sum + 8 * N * nl;
  l.wred = l.acc_sk + 8 * kp * J * nl;
  l.bytes = l.wred + 4 * N * J * nl;
  return l;
}

struct SkParams {
  int64_t num_keys, kp;
  int64_t wave_items;
  int walk, S;
  const dpf_block* key_seed;
  const uint4* cs;          // [D][kp]
  const uint32_t* cc;       // [D][kp]: cw_ctrl2
  const uint2* vcw;         // [kp]: the value correction's nl words
  const uint32_t* party;    // [kp]
  const uint32_t* wred;     // [N][J][nl]
  unsigned long long* acc_sum;   // [N][nl]
  unsigned long long* acc_sk;    // [kp][J][nl]
  Div32 div0, div1;
  RoundKeys rkl, rkr, rkv, rkd;
  int64_t dyn_per_wg;  // ItemLoop's per_wg (0: grid stride)
};

// Column kk of the table is key min(kk, K - 1): the lanes past the last key of
// a partly filled chunk read a valid key.
__global__ void expand_sketch_table_kernel(int64_t K, int64_t kp, int D, int cw_stride, int nl,
                                           const dpf_block* cw_seed, const uint8_t* cw_left,
                                           const uint8_t* cw_right, const dpf_block* vcw_in,
                                           const uint8_t* party_in, uint4* cs, uint32_t* cc,
                                           uint2* vcw, uint32_t* party) {
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
      vcw[kk] = make_uint2((uint32_t)vcw_in[nl * k].low,
                           nl > 1 ? (uint32_t)vcw_in[nl * k + 1].low : 0u);
      party[kk] = party_in[k] & 1u;
    }
  }
}

// wred[i][j][e] = w[j][i] mod N_e.
__global__ void expand_sketch_weights_kernel(int64_t N, int J, int nl, Div32 d0, Div32 d1,
                                             const uint32_t* __restrict__ w,
                                             uint32_t* __restrict__ wred) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N;
       i += (int64_t)gridDim.x * blockDim.x)
    for (int j = 0; j < J; ++j) {
      const uint32_t x = w[j * N + i];
      for (int e = 0; e < nl; ++e) wred[(i * J + j) * nl + e] = mod32(x, e ? d1 : d0);
    }
}

// sum[i][e] = acc_sum mod N_e (plus what it held, below N_e, when
// accumulating); sketch[k][j][e] = acc_sk mod N_e.
__global__ void expand_sketch_finish_kernel(int64_t n_sum, int64_t n_sk, int nl, int accumulate,
                                            Div32 d0, Div32 d1,
                                            const unsigned long long* __restrict__ acc_sum,
                                            const unsigned long long* __restrict__ acc_sk,
                                            uint32_t* __restrict__ sum, uint32_t* __restrict__ sk) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_sum + n_sk;
       i += (int64_t)gridDim.x * blockDim.x) {
    const bool is_sum = i < n_sum;
    const int64_t q = is_sum ? i : i - n_sum;
    const Div32& d = (nl > 1 && (q & 1)) ? d1 : d0;
    uint32_t r = mod64(is_sum ? acc_sum[q] : acc_sk[q], d);
    if (is_sum) {
      if (accumulate) {   // IntModN += (int_mod_n.h:116-120)
        const uint32_t s = r + sum[q];
        r = (s < r || s >= d.n) ? s - d.n : s;
      }
      sum[q] = r;
    } else {
      sk[q] = r;
    }
  }
}

// Per-lane correction words of one tree level.
struct SkCws {
  const uint4* cs;
  const uint32_t* cc;
  int64_t kp, kk;
  __device__ __forceinline__ void load(int level, uint4& s, uint32_t& c) const {
    const int64_t i = level * kp + kk;
    s = cs[i];
    c = cc[i];
  }
};

// dpf_expand_sum.hip's reduce_lanes for sums: a halving butterfly over the 64
// lanes of NV = 2^H values each.  Step s (offset 32 >> s) leaves a lane the
// half of its remaining values that its lane bit 5 - s selects (set: the upper
// half), summed with the partner's; after H steps one value is left, output
// o = lane >> (6 - H), and the remaining 6 - H offsets sum it over the lanes
// that share o.  Every lane then holds the 64-key total of output
// lane >> (6 - H): NV = 4 (nl = 2: leaf 0's two elements, leaf 1's two) in
// lanes 16 o .. 16 o + 15, NV = 2 (nl = 1: the two leaves) in lanes
// 32 o .. 32 o + 31.  tests/test_full_domain_sketch_cpu.py pins this map.
template <int NV>
__device__ __forceinline__ uint64_t reduce_lanes(uint64_t (&v)[NV], int lane) {
  constexpr int H = NV == 4 ? 2 : 1;
#pragma unroll
  for (int st = 0; st < H; ++st) {
    const int off = 32 >> st, half = NV >> (st + 1);
    const bool up = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < NV / 2; ++i) {
      if (i < half) {
        const uint64_t send = up ? v[i] : v[i + half];
        const uint64_t keep = up ? v[i + half] : v[i];
        v[i] = keep + __shfl_xor(send, off, 64);
      }
    }
  }
#pragma unroll
  for (int off = 32 >> H; off > 0; off >>= 1) v[0] += __shfl_xor(v[0], off, 64);
  return v[0];
}

typedef uint32_t __attribute__((address_space(4))) ConstU32;

// NL: the leaves of the value type, and the hashed blocks its sampling reads;
// J: the weight rows.
template <int NL, int J>
__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void expand_sketch_kernel(SkParams p) {
  __shared__ LdsImage lds;
  __shared__ int next_chunk;   // ItemLoop (dpf_device.h)
  fill_tables(lds.tab);
  if (threadIdx.x == 0) next_chunk = 0;
  __syncthreads();
  const LdsLookup lk = make_lookup(lds, KeySet{key_ref(p.rkl), key_ref(p.rkr), key_ref(p.rkv), key_ref(p.rkd)});
  constexpr int NV = 2 * NL;            // values of a leaf pair
  constexpr int OSHIFT = NL == 2 ? 4 : 5;   // reduce_lanes: output o in lanes o << OSHIFT ...
  constexpr int JN = J * NL;
  const uint32_t* __restrict__ wred = p.wred;
  const int walk = p.walk;
  const int G = p.S - kSkGroup;         // depth of the DFS stack above the leaf pairs
  const int64_t ngroups = (int64_t)1 << G;
  const int lane = (int)(threadIdx.x & 63);
  // The loop runs over wave items: the 64 lanes of a wave take the 64 "items"
  // of one chunk, which are one wave item.
  const ItemLoop items{&next_chunk, p.dyn_per_wg, p.wave_items, INT64_MAX};
  const int64_t end = p.wave_items * 64;
  for (int64_t u = items.first(); u < end; u = items.next(u)) {
    const int w = __builtin_amdgcn_readfirstlane((int)(u >> 6));
    const int chunk = w >> walk;
    // As expand_sum_kernel: each key chunk starts its round over the subtrees
    // at a subtree of its own and visits a subtree's leaf pairs in an order of
    // its own, so that resident waves do not all add into one line at once.
    const int j = (w + chunk) & ((1 << walk) - 1);
    const uint32_t rot = G > 0 ? ((uint32_t)chunk * 0x9E3779B1u) >> (32 - G) : 0u;
    const int64_t kk = (int64_t)chunk * 64 + lane;
    const bool live = kk < p.num_keys;
    const SkCws cws{p.cs, p.cc, p.kp, kk};
    Mod32Leaf<2> leaf;
    leaf.vcw_elems = nullptr;
    leaf.nl = NL;
    leaf.b = NL;
    leaf.div[0] = p.div0;
    leaf.div[1] = p.div1;
    const uint32_t party = p.party[kk];
    leaf.party = (int)party;
    {
      const uint2 c = p.vcw[kk];
      leaf.c[0] = c.x;
      leaf.c[1] = c.y;
    }
    uint64_t acc[JN > 0 ? JN : 1];
#pragma unroll
    for (int a = 0; a < (JN > 0 ? JN : 1); ++a) acc[a] = 0;
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
    // 2. depth-first down to the leaf pairs' parents: the child visited second
    //    is parked in sib[d] (scratch) with its control bit in bit 0, which a
    //    corrected seed has clear.
    Block4 sib[kSkStack];
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
      // 3. the leaf pair: its two leaves sampled and corrected.
      uint32_t x0[2], x1[2];
      {
        uint4 cs;
        uint32_t cc;
        cws.load(walk + G, cs, cc);
        Block4 c0, c1;
        uint32_t t0, t1;
        children_step(lk, lk.ks.l, lk.ks.r, node, nt, cs, cc, c0, t0, c1, t1);
        uint32_t w0[8], w1[8];
        leaf.hash2(lk, lk.ks.v, c0, c1, w0, w1);
        leaf.convert(w0, t0, x0);
        leaf.convert(w1, t1, x1);
      }
      if (!live) x0[0] = x0[1] = x1[0] = x1[1] = 0;
      // Leaf pair `pair` holds leaves 2 pair and 2 pair + 1 (below 2^27: the
      // weight index fits 32 bits).
      const int pair = __builtin_amdgcn_readfirstlane(
          (int)(((uint32_t)j << G) | ((uint32_t)g ^ rot)));
      // 4. the sketch: lane-private, the weights wave-uniform.
      if constexpr (JN > 0) {
        // Read through the constant address space: the table is written before
        // this launch and by no one during it, which the compiler cannot see
        // beside the kernel's atomics; a uniform constant address is a scalar load.
        const ConstU32* wp = (const ConstU32*)(uintptr_t)(wred + (int64_t)pair * (2 * JN));
#pragma unroll
        for (int jj = 0; jj < J; ++jj) {
#pragma unroll
          for (int e = 0; e < NL; ++e) {
            const Div32& dv = e ? p.div1 : p.div0;
            acc[jj * NL + e] += (uint64_t)mul_mod(wp[jj * NL + e], x0[e], dv) +
                                mul_mod(wp[JN + jj * NL + e], x1[e], dv);
          }
        }
      }
      // 5. the key sum: the pair's values over the 64 keys, one atomic per value.
      uint64_t v[NV];
#pragma unroll
      for (int e = 0; e < NL; ++e) {
        v[e] = x0[e];
        v[NL + e] = x1[e];
      }
      const uint64_t total = reduce_lanes<NV>(v, lane);
      if ((lane & ((1 << OSHIFT) - 1)) == 0)
        __hip_atomic_fetch_add(p.acc_sum + (int64_t)pair * NV + (lane >> OSHIFT),
                               (unsigned long long)total, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    // 6. the item's share of its keys' sketches (clamped lanes hold zeros).
    if constexpr (JN > 0) {
      if (live) {
#pragma unroll
        for (int a = 0; a < JN; ++a)
          __hip_atomic_fetch_add(p.acc_sk + kk * JN + a, (unsigned long long)acc[a],
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

bool sketch_type_ok(const dpf_value_desc* d) {
  int b = 0;
  return d && validate_desc(d) == kOk && mod32_eligible(d, &b) && d->num_leaves <= 2 &&
         b == d->num_leaves;
}

template <int NL>
void launch_sketch(const SkParams& p, int J, dim3 grid, dim3 block, hipStream_t s) {
  if (J == 0) hipLaunchKernelGGL((expand_sketch_kernel<NL, 0>), grid, block, 0, s, p);
  else if (J == 1) hipLaunchKernelGGL((expand_sketch_kernel<NL, 1>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((expand_sketch_kernel<NL, 2>), grid, block, 0, s, p);
}

unsigned capped_grid(int64_t n) {
  int64_t g = (n + 255) / 256;
  const int64_t cap = (int64_t)num_cus() * 8;
  if (g > cap) g = cap;
  return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace

extern "C" int dpf_hip_expand_sketch_supported(const dpf_value_desc* desc) {
  return sketch_type_ok(desc) ? 1 : 0;
}

extern "C" int64_t dpf_hip_expand_sketch_workspace_bytes(int64_t num_keys, int num_levels,
                                                         int log_domain_size, int num_leaves,
                                                         int num_weights) {
  if (num_keys < 0 || num_keys > INT32_MAX || log_domain_size < 1 ||
      log_domain_size > kSkMaxLogDomain || num_levels != log_domain_size || num_leaves < 1 ||
      num_leaves > 2 || num_weights < 0 || num_weights > kSkMaxWeights)
    return -1;
  return layout(num_keys, num_levels, log_domain_size, num_leaves, num_weights).bytes;
}

extern "C" int dpf_hip_expand_sketch_plan(int64_t num_keys, int tree_depth, int num_cus,
                                          int64_t out[6]) {
  if (!out) return fail(kInvalidArgument, "NULL plan output");
  if (num_keys < 1 || num_keys > INT32_MAX || tree_depth < 0 || tree_depth > kSkMaxLogDomain ||
      num_cus < 1 || num_cus > 65536)
    return fail(kInvalidArgument, "num_keys, tree_depth or num_cus out of range");
  const SkPlan pl = plan_sketch(num_keys, tree_depth, num_cus);
  out[0] = pl.S;
  out[1] = pl.walk;
  out[2] = pl.subtrees;
  out[3] = pl.wave_items;
  out[4] = pl.group;
  out[5] = pl.want;
  return kOk;
}

extern "C" int dpf_hip_expand_sketch(int64_t num_keys, int num_levels, int cw_stride,
                                     int log_domain_size, const dpf_block* key_seed,
                                     const uint8_t* party, const dpf_block* cw_seed,
                                     const uint8_t* cw_left, const uint8_t* cw_right,
                                     const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                                     const dpf_aes_key* key_value, const dpf_value_desc* desc,
                                     const dpf_block* value_correction, int num_weights,
                                     const uint32_t* weights, void* workspace,
                                     int64_t workspace_bytes, uint32_t* sum_out,
                                     uint32_t* sketch_out, int accumulate, void* stream) {
  if (num_keys < 0 || num_keys > INT32_MAX)
    return fail(kInvalidArgument, "num_keys out of range");
  if (log_domain_size < 1 || log_domain_size > kSkMaxLogDomain)
    return fail(kInvalidArgument, "log_domain_size must be in [1, 28]");
  if (num_levels != log_domain_size)
    return fail(kInvalidArgument, "num_levels must be log_domain_size");
  if (!desc || !key_left || !key_right || !key_value)
    return fail(kInvalidArgument, "NULL value descriptor or AES key");
  if (!sketch_type_ok(desc))
    return fail(kUnimplemented,
                "the checked full-domain sum is implemented for IntModN<uint32_t, N> and "
                "2-tuples of it only");
  if (num_weights < 0 || num_weights > kSkMaxWeights)
    return fail(kInvalidArgument, "num_weights must be in [0, 2]");
  if (cw_stride < num_levels) return fail(kInvalidArgument, "cw_stride < num_levels");
  if (!sum_out) return fail(kInvalidArgument, "`sum_out` is NULL");
  if (num_weights > 0 && (!weights || (!sketch_out && num_keys > 0)))
    return fail(kInvalidArgument, "`weights` or `sketch_out` is NULL");
  hipStream_t s = (hipStream_t)stream;
  const int nl = desc->num_leaves, J = num_weights, D = num_levels;
  const int64_t N = (int64_t)1 << log_domain_size;
  if (num_keys == 0) {
    // The empty sum; there is no key to sketch.
    if (!accumulate) HIP_TRY(hipMemsetAsync(sum_out, 0, (size_t)N * nl * 4, s));
    return kOk;
  }
  if (!key_seed || !party || !value_correction || !cw_seed || !cw_left || !cw_right)
    return fail(kInvalidArgument, "NULL pointer");
  const SkLayout l = layout(num_keys, D, log_domain_size, nl, J);
  if (!workspace || workspace_bytes < l.bytes)
    return fail(kResourceExhausted, "the checked full-domain sum needs a workspace of " +
                                        std::to_string((long long)l.bytes) + " bytes");
  if (((uintptr_t)sum_out & 15) != 0 || ((uintptr_t)workspace & 15) != 0 ||
      ((uintptr_t)weights & 3) != 0 || ((uintptr_t)sketch_out & 3) != 0)
    return fail(kInvalidArgument,
                "`sum_out` and `workspace` must be aligned to 16 bytes, `weights` and "
                "`sketch_out` to 4");
  const SkPlan pl = plan_sketch(num_keys, D, num_cus());
  SkParams p;
  memset(&p, 0, sizeof(p));
  p.num_keys = num_keys;
  p.kp = padded_keys(num_keys);
  p.wave_items = pl.wave_items;
  p.walk = pl.walk;
  p.S = pl.S;
  p.key_seed = key_seed;
  char* ws = static_cast<char*>(workspace);
  uint4* cs = reinterpret_cast<uint4*>(ws + l.cs);
  uint32_t* cc = reinterpret_cast<uint32_t*>(ws + l.cc);
  uint2* vcw = reinterpret_cast<uint2*>(ws + l.vcw);
  uint32_t* pty = reinterpret_cast<uint32_t*>(ws + l.party);
  uint32_t* wred = reinterpret_cast<uint32_t*>(ws + l.wred);
  p.cs = cs;
  p.cc = cc;
  p.vcw = vcw;
  p.party = pty;
  p.wred = wred;
  p.acc_sum = reinterpret_cast<unsigned long long*>(ws + l.acc_sum);
  p.acc_sk = reinterpret_cast<unsigned long long*>(ws + l.acc_sk);
  p.div0 = make_div32((uint32_t)desc->mod_low[0]);
  p.div1 = make_div32((uint32_t)desc->mod_low[nl - 1]);
  const RoundKeys rkr = expand_key(key_right);
  p.rkl = expand_key(key_left);
  p.rkr = rkr;
  p.rkv = expand_key(key_value);
  p.rkd = xor_keys(p.rkl, rkr);
  hipLaunchKernelGGL(expand_sketch_table_kernel, dim3(capped_grid(p.kp * (D + 1))), dim3(256), 0, s,
                     num_keys, p.kp, D, cw_stride, nl, cw_seed, cw_left, cw_right,
                     value_correction, party, cs, cc, vcw, pty);
  HIP_TRY(hipGetLastError());
  if (J > 0) {
    hipLaunchKernelGGL(expand_sketch_weights_kernel, dim3(capped_grid(N)), dim3(256), 0, s, N, J,
                       nl, p.div0, p.div1, weights, wred);
    HIP_TRY(hipGetLastError());
  }
  // Both accumulators are adjacent.
  HIP_TRY(hipMemsetAsync(ws + l.acc_sum, 0, (size_t)(l.wred - l.acc_sum), s));
  const LaunchShape sh = chunked_shape(pl.wave_items * 64, "DPF_EXPAND_SKETCH_DYNAMIC");
  p.dyn_per_wg = sh.dyn_per_wg;
  if (nl == 2) launch_sketch<2>(p, J, dim3(sh.grid), dim3(sh.block), s);
  else launch_sketch<1>(p, J, dim3(sh.grid), dim3(sh.block), s);
  HIP_TRY(hipGetLastError());
  const int64_t n_sum = N * nl, n_sk = num_keys * J * nl;
  hipLaunchKernelGGL(expand_sketch_finish_kernel, dim3(capped_grid(n_sum + n_sk)), dim3(256), 0, s,
                     n_sum, n_sk, nl, accumulate ? 1 : 0, p.div0, p.div1, p.acc_sum, p.acc_sk,
                     sum_out, sketch_out);
  HIP_TRY(hipGetLastError());
  return kOk;
}
