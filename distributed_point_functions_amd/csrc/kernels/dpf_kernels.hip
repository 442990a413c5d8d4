// dpf_kernels.hip -- MI355X (gfx950) kernels for incremental-DPF evaluation and
// the C ABI declared in include/dpf_hip.h.
//
// Hot path:
//   * AES-128 MMO hash with the four T-tables replicated 32x across LDS banks
//     (128 KiB): lane l reads copy (l & 31), so every ds_read_b32 of a wave is
//     bank-conflict-free whatever the table index.  Tables are laid out in
//     256-byte rows so one v_perm_b32 forms each lookup address; 3-input XORs
//     are single v_bitop3_b32 (gfx950).  One 1024-thread workgroup per CU.
//     Measured (tools/aes_microbench.hip): 97 G AES/s with two interleaved
//     chains, 88% of the chip's ds_read_b32 ceiling.
//   * expand_kernel: one thread = one subtree.  It walks from its start seed to
//     the subtree root along the bits of its work-item index (per-lane key
//     select), then visits the subtree depth-first with the path stack held in
//     VGPRs (uniform control flow: every lane of a wave is at the same leaf
//     pair), hashing each leaf with the value key, converting, correcting and
//     storing it.  Intermediate seeds never touch HBM; only leaves are written.
//   * Point evaluation (eval_points*_kernel) lives in dpf_points.hip.
//   * Correction words live in LDS (broadcast reads).
// All arithmetic is integer/bitwise; no MFMA (nothing here is a contraction).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <type_traits>
#include <vector>
#include <string>

#include "../../../include/dpf_hip.h"
#include "dpf_device.h"
#include "dpf_dot.h"
#include "dpf_runtime.h"

namespace dpf_rt {
thread_local std::string g_last_error;
thread_local const char* g_last_expand = "";
thread_local int g_last_expand_s = -1;
thread_local int64_t g_last_dynamic_chunks = 0;   // dpf_hip_last_dynamic_chunks
// dpf_hip_clock_probe's device accumulator (NULL: off), read by every
// dpf_hip_expand launch.
std::atomic<unsigned long long*> g_clock_acc{nullptr};

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
int hip_fail(hipError_t e, const char* what) {
  return fail(e == hipErrorOutOfMemory ? kResourceExhausted : kInternal,
              std::string(what) + ": " + hipGetErrorString(e));
}
}  // namespace dpf_rt

using namespace dpf_rt;

namespace {

// ------------------------------------------------------------------------
// Kernels
// ------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void hash_kernel(int64_t n, const dpf_block* __restrict__ in,
                                                      dpf_block* __restrict__ out,
                                                      RoundKeys rk, int64_t dyn_per_wg) {
  __shared__ LdsImage lds;
  __shared__ int next_chunk;   // ItemLoop (dpf_device.h)
  fill_tables(lds.tab);
  if (threadIdx.x == 0) next_chunk = 0;
  __syncthreads();
  const KeyRef kr = key_ref(rk);
  LdsLookup lk = make_lookup(lds, KeySet{kr, kr, kr, kr});
  const ItemLoop items{&next_chunk, dyn_per_wg, (n + 63) / 64, n};
  for (int64_t i = items.first(); i < n; i = items.next(i)) {
    store_block(out + i, dpf_aes::mmo_hash(load_block(in + i), lk, UniformRK{lk.ks.v}));
  }
}

struct PathParams {
  int64_t n;
  int num_levels;
  const dpf_block* seeds_in;
  const uint8_t* ctrl_in;
  const dpf_block* paths;
  const dpf_block* cw_seed;
  const uint8_t* cw_left;
  const uint8_t* cw_right;
  dpf_block* seeds_out;
  uint8_t* ctrl_out;
  RoundKeys rkl, rkd;
  int64_t dyn_per_wg;  // ItemLoop's per_wg (0: grid stride)
};


__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void eval_paths_kernel(PathParams p) {
  __shared__ LdsImage lds;
  __shared__ int next_chunk;   // ItemLoop (dpf_device.h)
  fill_tables(lds.tab);
  fill_cws(lds, p.cw_seed, p.cw_left, p.cw_right, p.num_levels);
  if (threadIdx.x == 0) next_chunk = 0;
  __syncthreads();
  LdsLookup lk = make_lookup(lds, KeySet{key_ref(p.rkl), KeyRef{}, KeyRef{}, key_ref(p.rkd)});
  const ItemLoop items{&next_chunk, p.dyn_per_wg, (p.n + 63) / 64, p.n};
  for (int64_t i = items.first(); i < p.n; i = items.next(i)) {
    Block4 s = load_block(p.seeds_in + i);
    uint32_t t = p.ctrl_in[i] & 1u;
    Block4 path = load_block(p.paths + i);
    for (int j = 0; j < p.num_levels; ++j) {
      uint32_t bit = path_bit(path, p.num_levels - 1 - j);
      path_step(lk, lk.ks.l, lk.ks.d, s, t, bit, lds.cw_seed[j], lds.cw_ctrl[j]);
    }
    store_block(p.seeds_out + i, s);
    p.ctrl_out[i] = (uint8_t)t;
  }
}

// SCHED: the instance for launches with a chunk schedule (one counter for
// the launch or tapered chunks; always dynamic).  Its k0 and S change from
// chunk to chunk, which costs every instance 3-5 VGPRs and some of them
// spills, so the static launches and the uniform per-workgroup chunks keep
// an instance in which both are launch constants.
template <class Leaf, bool SCHED = false>
__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void expand_kernel(ExpandParams p, Leaf leaf) {
  __shared__ LdsImage lds;
  __shared__ int next_chunk;   // take_chunk / take_expand_chunk (dpf_device.h), dynamic launches
  leaf.init();
  fill_tables(lds.tab);
  fill_cws(lds, p.cw_seed, p.cw_left, p.cw_right, p.num_levels);
  if (threadIdx.x == 0) next_chunk = 0;
  __syncthreads();
  const LdsLookup lk = make_lookup(lds, KeySet{key_ref(p.rkl), key_ref(p.rkr), key_ref(p.rkv), key_ref(p.rkd)});
  int k0 = p.k0, S = p.S;
  if constexpr (SCHED) ClockStamp::first_begin(p.clock);
  // Items by grid stride, or 64 at a time per wave (dyn_chunks > 0, as the
  // octet kernel; SCHED: the chunk's shape (k0, S) comes with it).
  const int64_t nch = (p.num_items + 63) / 64;
  const int64_t end = SCHED ? INT64_MAX : p.num_items;
  auto take = [&]() -> int64_t {
    if constexpr (SCHED) return take_expand_chunk(p, &next_chunk, end, k0, S);
    else return take_chunk(&next_chunk, p.dyn_chunks, nch, p.num_items);
  };
  for (int64_t item = SCHED || p.dyn_chunks ? take()
                                            : blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       item < end;
       item = SCHED || p.dyn_chunks ? take() : item + (int64_t)gridDim.x * blockDim.x) {
    const int B = S >= 1 ? 1 : 0;  // leaf pairs share their parent
    const int G = S - B;            // depth of the DFS stack
    const int64_t ngroups = (int64_t)1 << G;
    // 1. walk from the start seed to this item's subtree root.
    const int64_t r = item >> k0;
    Block4 s = load_block(p.seeds_in + r);
    uint32_t t = p.ctrl_in[r] & 1u;
    for (int j = 0; j < k0; ++j) {
      uint32_t bit = (uint32_t)((item >> (k0 - 1 - j)) & 1);
      path_step(lk, lk.ks.l, lk.ks.d, s, t, bit, lds.cw_seed[j], lds.cw_ctrl[j]);
    }
    // 2. depth-first over the subtree.  Every inner node is expanded into both
    //    children at once (two interleaved hashes); the left child is descended
    //    into and the right one parked in sib[d] until the walk returns to it,
    //    so each node is hashed exactly once and always in a pair.
    Block4 sib[kGMax];  // sib[d - 1] = parked right child at depth d
    uint32_t tb = 0;  // bit d = control bit of sib[d]
    const int64_t leaf_base = item << S;
    for (int64_t g = 0; g < ngroups; ++g) {
      Block4 node = s;
      uint32_t nt = t;
      int ds = 0;  // depth of `node` (wave-uniform)
      if (g != 0) {
        ds = G - (int)__builtin_ctzll((unsigned long long)g);
#pragma unroll
        for (int d = 1; d <= kGMax; ++d)
          if (d == ds) { node = sib[d - 1]; nt = (tb >> d) & 1u; }
      }
      for (int d = ds; d < G; ++d) {
        Block4 c0, c1;
        uint32_t t0, t1;
        children_step(lk, lk.ks.l, lk.ks.r, node, nt, lds.cw_seed[k0 + d], lds.cw_ctrl[k0 + d],
                      c0, t0, c1, t1);
#pragma unroll
        for (int e = 1; e <= kGMax; ++e)
          if (e == d + 1) sib[e - 1] = c1;
        tb = (tb & ~(1u << (d + 1))) | (t1 << (d + 1));
        node = c0;
        nt = t0;
      }
      if (B == 0) {
        leaf.emit(lk, lk.ks.v, node, nt, leaf_base + g, p.out);
      } else {
        const int lvl = k0 + G;
        Block4 c0, c1;
        uint32_t t0, t1;
        children_step(lk, lk.ks.l, lk.ks.r, node, nt, lds.cw_seed[lvl], lds.cw_ctrl[lvl], c0, t0,
                      c1, t1);
        leaf.emit2(lk, lk.ks.v, c0, t0, c1, t1, leaf_base + 2 * g, p.out);
      }
    }
  }
  if constexpr (SCHED) ClockStamp::exits(p.clock);
  if constexpr (HasFinish<Leaf>::value) leaf.finish();
}

// Octet form of expand_kernel for integer leaves that fill whole 16-byte
// blocks (uint64, uint128, XorWrapper, uniform tuples; the default for them):
// the bottom three levels of every subtree are expanded breadth-first as an
// octet -- the node's 2 children (ILP2), its 4 grandchildren (ILP4), then per
// half its 4 leaf seeds and their 4 value hashes (ILP4 each) -- and each lane
// writes its 8 corrected blocks as 2 x 64 contiguous bytes, i.e. whole
// 128-byte lines (expand_kernel's 32-byte leaf-pair pieces measured write
// amplification 1.25).  The DFS stack above the octets lives in scratch (one
// 16-byte store per push, one load per octet, issued an octet ahead) so the
// VGPRs go to the ILP4 chains (128 VGPRs plus 160 B/lane of spills remain;
// that scratch traffic, not the outputs, is most of its HBM bytes beyond the
// 8 GiB written).  Measured same-box at config 2: 18.58 vs 18.87-18.98 ms per
// 2^30 outputs with identical outputs (tools/octet_check.py); in the bench
// 17.9 ms per step (59.95 G leaves/s).
// Half an octet's leaves (4 consecutive leaf blocks): integer leaves filling
// whole blocks store 4 x 16 contiguous bytes; other policies use their emit4.
template <int BITS, bool XOR>
__device__ __forceinline__ void octet_half(const FastIntLeaf<BITS, XOR>& leaf, const LdsLookup& lk,
                                           KeyRef rkv, Block4* l, const uint32_t* lt,
                                           int64_t first_leaf, char* out, Block4*) {
  const UniformRK rv[4] = {UniformRK{rkv}, UniformRK{rkv}, UniformRK{rkv}, UniformRK{rkv}};
  dpf_aes::mmo_hashN<4>(l, lk, rv);
  uint4* o = reinterpret_cast<uint4*>(out + first_leaf * 16);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const Block4 h = leaf.correct(l[j], lt[j]);
    o[j] = make_uint4(h.w0, h.w1, h.w2, h.w3);
  }
}
template <class Leaf>
__device__ __forceinline__ void octet_half(const Leaf& leaf, const LdsLookup& lk,
                                           KeyRef rkv, Block4* l, const uint32_t* lt,
                                           int64_t first_leaf, char* out, Block4* park) {
  leaf.emit4(lk, rkv, l, lt, first_leaf, out);
}
// Tuples of IntModN<uint32_t>: the half's second leaf pair (seed | control
// bit in bit 0) waits in two scratch slots beside the DFS stack while the
// first pair's four value hashes run, instead of in 8 + 2 VGPRs -- that group
// was the register-starved one (~3 lookups in flight, r15 ISA).
template <class Leaf> struct OctetStash;
template <int NL>
__device__ __forceinline__ void octet_half(const Mod32Leaf<NL>& leaf, const LdsLookup& lk,
                                           KeyRef rkv, Block4* l, const uint32_t* lt,
                                           int64_t first_leaf, char* out, Block4* park) {
  static_assert(OctetStash<Mod32Leaf<NL>>::value >= 2, "park slots hold the octet stash");
  park[0] = Block4{l[2].w0 | lt[2], l[2].w1, l[2].w2, l[2].w3};
  park[1] = Block4{l[3].w0 | lt[3], l[3].w1, l[3].w2, l[3].w3};
  asm volatile("" ::: "memory");   // read them back from scratch, not from registers
  uint32_t x[4][NL];
  {
    uint32_t w0[8], w1[8];
    leaf.hash2(lk, rkv, l[0], l[1], w0, w1);
    leaf.convert(w0, lt[0], x[0]);
    leaf.convert(w1, lt[1], x[1]);
  }
  asm volatile("" ::: "memory");
  {
    const Block4 a = park[0], b = park[1];
    uint32_t w0[8], w1[8];
    leaf.hash2(lk, rkv, Block4{a.w0 & ~1u, a.w1, a.w2, a.w3}, Block4{b.w0 & ~1u, b.w1, b.w2, b.w3},
               w0, w1);
    leaf.convert(w0, a.w0 & 1u, x[2]);
    leaf.convert(w1, b.w0 & 1u, x[3]);
  }
  leaf.store4(x, first_leaf, out);
}

// Where the octet keeps its second half's two grandchildren during the first
// half: 1 = q[3] in LDS (16 B per lane), q[2] in scratch beside the DFS
// stack, 2 = also q[2]'s upper 12 bytes in LDS, its low word in a VGPR -- the
// LDS left over by the T-tables and correction words (150 + 12 KiB of 160).
// Config 2, from both in scratch: 17.21 -> 17.08 (1) -> 16.96 ms (2),
// WRITE_SIZE 1.30 -> 1.21 -> 1.18x the 8 GiB written; SwarLeaf runs out of
// VGPRs at 2 (profiles/r11_ws_ab.txt).
template <class Leaf> struct OctetStash { static constexpr int value = 2; };
template <> struct OctetStash<SwarLeaf> { static constexpr int value = 1; };

template <class Leaf, bool SCHED = false>   // SCHED: as expand_kernel's
__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void expand_octet_kernel(ExpandParams p,
                                                                             Leaf leaf) {
  __shared__ LdsImage lds;
  constexpr int kStash = OctetStash<Leaf>::value;
  __shared__ uint4 stash[kBlock];
  __shared__ uint3 stash2[kStash >= 2 ? kBlock : 1];
  __shared__ int next_chunk;   // dynamic distribution: the workgroup's own chunk counter
  static_assert(sizeof(LdsImage) + 16 * kBlock + (kStash >= 2 ? 12 * kBlock : 0) + 16 <= 160 * 1024,
                "LDS over 160 KiB");
  leaf.init();
  fill_tables(lds.tab);
  fill_cws(lds, p.cw_seed, p.cw_left, p.cw_right, p.num_levels);
  if (threadIdx.x == 0) next_chunk = 0;
  __syncthreads();
  const LdsLookup lk = make_lookup(lds, KeySet{key_ref(p.rkl), key_ref(p.rkr), key_ref(p.rkv), key_ref(p.rkd)});
  int k0 = p.k0, S = p.S;
  ClockStamp stamp;
  stamp.begin(p.clock);
  // Items: thread u takes u, u + threads, ... (static), or -- dyn_chunks > 0
  // -- each wave takes the next 64 items from the launch's counter (or its
  // workgroup's share from its LDS counter) until they are used up.  The CU's
  // arbiter favours its oldest waves (in config 2 wave 0 of a workgroup
  // finished in 7.8 ms, wave 15 in 16.6 ms of a 16.9 ms launch): with a fixed
  // share the last third of a launch runs on fewer and fewer waves, while
  // taken dynamically the fast waves and the fast CUs do more and all finish
  // together; the last chunks are of smaller subtrees (take_expand_chunk), so
  // the waves also stop within a small chunk's time of each other.  Every
  // lane of a wave holds the same chunk, so the DFS stays wave-uniform.
  const int lane = (int)(threadIdx.x & 63);
  const int64_t end = SCHED ? INT64_MAX : p.num_items;
  auto take = [&]() -> int64_t {
    if constexpr (SCHED) {
      return take_expand_chunk(p, &next_chunk, end, k0, S);
    } else {   // the workgroup's own range of uniform chunks
      int c = 0;
      if (lane == 0) c = atomicAdd(&next_chunk, 1);
      c = __builtin_amdgcn_readfirstlane(c);
      return c < p.dyn_chunks ? ((int64_t)blockIdx.x * p.dyn_chunks + c) * 64 + lane
                              : p.num_items;
    }
  };
  for (int64_t item = SCHED || p.dyn_chunks ? take()
                                            : blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       item < end;
       item = SCHED || p.dyn_chunks ? take() : item + (int64_t)gridDim.x * blockDim.x) {
    const int G = S - 3;
    const int64_t ngroups = (int64_t)1 << G;
    // 1. walk from the start seed to this item's subtree root.
    const int64_t r = item >> k0;
    Block4 s = load_block(p.seeds_in + r);
    uint32_t t = p.ctrl_in[r] & 1u;
    for (int j = 0; j < k0; ++j) {
      const uint32_t bit = (uint32_t)((item >> (k0 - 1 - j)) & 1);
      path_step(lk, lk.ks.l, lk.ks.d, s, t, bit, lds.cw_seed[j], lds.cw_ctrl[j]);
    }
    // 2. depth-first down to the octet roots; right children parked in
    //    sib[d] (scratch), their control bits in tb.
    Block4 sib[kGMax];
    uint32_t tb = 0;
    const int64_t leaf_base = item << S;
    Block4 next = s;
    for (int64_t g = 0; g < ngroups; ++g) {
      Block4 node = next;
      uint32_t nt = t;
      int ds = 0;
      if (g != 0) {
        ds = G - (int)__builtin_ctzll((unsigned long long)g);
        nt = (tb >> ds) & 1u;
      }
      for (int d = ds; d < G; ++d) {
        Block4 c0, c1;
        uint32_t t0, t1;
        children_step(lk, lk.ks.l, lk.ks.r, node, nt, lds.cw_seed[k0 + d], lds.cw_ctrl[k0 + d],
                      c0, t0, c1, t1);
        sib[d] = c1;
        tb = (tb & ~(1u << (d + 1))) | (t1 << (d + 1));
        node = c0;
        nt = t0;
      }
      // The next octet's root (written by now), loaded an octet ahead.
      if (g + 1 < ngroups) next = sib[G - (int)__builtin_ctzll((unsigned long long)(g + 1)) - 1];
      // 3. the octet.
      const int lvl = k0 + G;
      Block4 c[2], q[4];
      uint32_t ct[2], qt[4];
      children_step(lk, lk.ks.l, lk.ks.r, node, nt, lds.cw_seed[lvl], lds.cw_ctrl[lvl], c[0],
                    ct[0], c[1], ct[1]);
      children_step_x2(lk, lk.ks.l, lk.ks.r, c[0], ct[0], c[1], ct[1], lds.cw_seed[lvl + 1],
                       lds.cw_ctrl[lvl + 1], q, qt);
      // The second half's two grandchildren wait outside the VGPRs during the
      // first half (OctetStash: lane-private LDS slots, for SwarLeaf's
      // q[2] scratch beside the DFS stack) instead of 8 VGPRs: 128 VGPRs with 37 spilled -> 110
      // with none, +3.5%, HBM traffic 17.7 -> 12.1 GB per config-2 launch in
      // scratch, 10.9 GB in LDS (profiles/r11_ws_ab.txt).  The DFS uses
      // sib[0 .. S-4], S <= kSMax.  Each lane reads back only its own slot.
      static_assert(kSMax - 3 <= kGMax - 2, "stash overlaps the DFS stack");
      uint32_t q2w0 = 0;
      if constexpr (kStash >= 2) {
        q2w0 = q[2].w0;
        stash2[threadIdx.x] = make_uint3(q[2].w1, q[2].w2, q[2].w3);
      } else {
        sib[kGMax - 2] = q[2];
      }
      stash[threadIdx.x] = make_uint4(q[3].w0, q[3].w1, q[3].w2, q[3].w3);
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        Block4 l[4];
        uint32_t lt[4];
        if (hf == 1) {
          if constexpr (kStash >= 2) {
            const uint3 u = stash2[threadIdx.x];
            q[2] = Block4{q2w0, u.x, u.y, u.z};
          } else {
            q[2] = sib[kGMax - 2];
          }
          const uint4 v = stash[threadIdx.x];
          q[3] = Block4{v.x, v.y, v.z, v.w};
        }
        children_step_x2(lk, lk.ks.l, lk.ks.r, q[2 * hf], qt[2 * hf], q[2 * hf + 1],
                         qt[2 * hf + 1], lds.cw_seed[lvl + 2], lds.cw_ctrl[lvl + 2], l, lt);
        // The half's four value hashes (ILP4), conversion, correction, stores
        // (integer leaves: 64 contiguous bytes per lane).
        // sib[kGMax - 2 ..] is free when the stash lives in LDS (kStash == 2):
        // Mod32Leaf parks a leaf pair there.
        octet_half(leaf, lk, lk.ks.v, l, lt, leaf_base + 8 * g + 4 * hf, p.out, &sib[kGMax - 2]);
      }
    }
  }
  stamp.end(p.clock);
  if constexpr (HasFinish<Leaf>::value) leaf.finish();
}

// Latency mode of full-domain expansion for small trees (r15; config 1 and
// the reference's BM_EvaluateRegularDpf below ~2^20 outputs).  expand_kernel /
// the octet kernel give every lane its own subtree and walk each one from the
// start seed: at 2^19 leaves that is 262144 walks of 18 levels, 3.7x the
// algorithmic AES, and each lane's chain is latency-bound.  Here workgroup w
// owns the subtree at depth t = p.k0 under start w >> t (one workgroup per CU
// at most) and expands its D = p.S levels breadth-first through LDS, so every
// node is hashed once:
//   * wave 0 walks the t levels to the subtree root, one chain per lane QUAD
//     (quad::path_step);
//   * a level of <= 256 parents: quad q expands parent q into both children
//     (quad::children, the two hashes interleaved);
//   * a wider level: lane i expands parent i (children_step, ILP2);
//   * level D: lane i expands parent i and value-hashes its two leaves
//     (Leaf::emit2), stored side by side at (w << D) + 2i; integer leaves of
//     a level of <= 256 parents do that in quads.
// Nodes live in nodes[] / tbits[] (<= 1024 per level, so D <= 11), read into
// registers before a barrier and rewritten after it.
template <class Leaf> struct IsFastInt : std::false_type {};
template <int BITS, bool XOR> struct IsFastInt<FastIntLeaf<BITS, XOR>> : std::true_type {};
template <int BITS, bool XOR> struct IsFastInt<DotLeaf<BITS, XOR>> : std::true_type {};
template <class Leaf>
__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void expand_small_kernel(ExpandParams p, Leaf leaf) {
  __shared__ LdsImage lds;
  __shared__ uint4 nodes[kBlock];
  __shared__ uint32_t tbits[kBlock];
  leaf.init();
  fill_tables(lds.tab);
  fill_cws(lds, p.cw_seed, p.cw_left, p.cw_right, p.num_levels);
  __syncthreads();
  const LdsLookup lk =
      make_lookup(lds, KeySet{key_ref(p.rkl), key_ref(p.rkr), key_ref(p.rkv), key_ref(p.rkd)});
  const quad::Keys ql = quad::keys_of(p.rkl), qd = quad::keys_of(p.rkd);
  const int t = p.k0, D = p.S;
  const int64_t w = blockIdx.x;
  const int tid = threadIdx.x, c = quad::column(), q = tid >> 2;
  auto word = [](const uint4& v, int i) { return reinterpret_cast<const uint32_t*>(&v)[i]; };
  if (tid < 64) {
    const int64_t r = w >> t;
    uint32_t s = reinterpret_cast<const uint32_t*>(p.seeds_in + r)[c];
    uint32_t tt = p.ctrl_in[r] & 1u;
    for (int j = 0; j < t; ++j) {
      const uint32_t bit = (uint32_t)((w >> (t - 1 - j)) & 1);
      quad::path_step(lk, ql, qd, s, tt, bit, word(lds.cw_seed[j], c), lds.cw_ctrl[j]);
    }
    if (tid < 4) {
      reinterpret_cast<uint32_t*>(&nodes[0])[c] = s;
      if (c == 0) tbits[0] = tt;
    }
  }
  __syncthreads();
  for (int j = 1; j < D; ++j) {
    const int lvl = t + j - 1, npar = 1 << (j - 1);
    if (npar <= kBlock / 4) {
      const bool on = q < npar;
      uint32_t c0 = 0, c1 = 0, t0 = 0, t1 = 0;
      if (on)
        quad::children(lk, ql, qd, word(nodes[q], c), tbits[q], word(lds.cw_seed[lvl], c),
                       lds.cw_ctrl[lvl], c0, t0, c1, t1);
      __syncthreads();
      if (on) {
        reinterpret_cast<uint32_t*>(&nodes[2 * q])[c] = c0;
        reinterpret_cast<uint32_t*>(&nodes[2 * q + 1])[c] = c1;
        if (c == 0) {
          tbits[2 * q] = t0;
          tbits[2 * q + 1] = t1;
        }
      }
      __syncthreads();
    } else {
      const bool on = tid < npar;
      Block4 c0{}, c1{};
      uint32_t t0 = 0, t1 = 0;
      if (on) {
        const uint4 v = nodes[tid];
        children_step(lk, lk.ks.l, lk.ks.r, Block4{v.x, v.y, v.z, v.w}, tbits[tid],
                      lds.cw_seed[lvl], lds.cw_ctrl[lvl], c0, t0, c1, t1);
      }
      __syncthreads();
      if (on) {
        nodes[2 * tid] = make_uint4(c0.w0, c0.w1, c0.w2, c0.w3);
        nodes[2 * tid + 1] = make_uint4(c1.w0, c1.w1, c1.w2, c1.w3);
        tbits[2 * tid] = t0;
        tbits[2 * tid + 1] = t1;
      }
      __syncthreads();
    }
  }
  const int lvl = t + D - 1, npar = 1 << (D - 1);
  const int64_t leaf0 = w << D;
  bool quad_last = false;
  if constexpr (IsFastInt<Leaf>::value) quad_last = npar <= kBlock / 4;
  if (quad_last) {
    if constexpr (IsFastInt<Leaf>::value) if (q < npar) {
      const quad::Keys qv = quad::keys_of(p.rkv);
      uint32_t c0, c1, t0, t1;
      quad::children(lk, ql, qd, word(nodes[q], c), tbits[q], word(lds.cw_seed[lvl], c),
                     lds.cw_ctrl[lvl], c0, t0, c1, t1);
      quad::hash2(lk, qv, c0, c1);
      const Block4 h0 = quad::gather(c0), h1 = quad::gather(c1);
      if (c == 0) {
        leaf.store(leaf.correct(h0, t0), leaf0 + 2 * q, p.out);
        leaf.store(leaf.correct(h1, t1), leaf0 + 2 * q + 1, p.out);
      }
    }
  } else if (tid < npar) {
    const uint4 v = nodes[tid];
    Block4 c0, c1;
    uint32_t t0, t1;
    children_step(lk, lk.ks.l, lk.ks.r, Block4{v.x, v.y, v.z, v.w}, tbits[tid], lds.cw_seed[lvl],
                  lds.cw_ctrl[lvl], c0, t0, c1, t1);
    leaf.emit2(lk, lk.ks.v, c0, t0, c1, t1, leaf0 + 2 * tid, p.out);
  }
  if constexpr (HasFinish<Leaf>::value) leaf.finish();
}

// Leaf policy of the tree-top pass (expand_top, below): expand_small_kernel's
// last breadth-first level is not hashed; its nodes are stored as the start
// seeds (seed, control bit) of the octet kernel's items.
struct SeedLeaf {
  dpf_block* seeds;
  uint8_t* ctrl;
  // The chunk counter of the launch that follows (ExpandParams::chunk_counter)
  // or NULL: zeroed here, in stream order before that launch.
  unsigned int* counter;
  __device__ __forceinline__ void init() const {
    if (counter != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *counter = 0u;
  }
  __device__ __forceinline__ void emit2(const LdsLookup&, KeyRef, Block4 s0, uint32_t t0, Block4 s1,
                                        uint32_t t1, int64_t first, char*) const {
    store_block(seeds + first, s0);
    store_block(seeds + first + 1, s1);
    ctrl[first] = (uint8_t)t0;
    ctrl[first + 1] = (uint8_t)t1;
  }
};

// Counts points >= 2^log_domain_size (EvaluateAt's range check, h:861-874).
__global__ void count_out_of_range_kernel(int64_t n, const dpf_block* __restrict__ pts, int log,
                                          unsigned long long* __restrict__ bad) {
  unsigned long long c = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const dpf_block b = pts[i];
    bool out;
    if (log >= 128) out = false;
    else if (log >= 64) out = (b.high >> (log - 64)) != 0;
    else out = b.high != 0 || (b.low >> log) != 0;
    c += out ? 1 : 0;
  }
  // Wave-level reduction, one atomic per wave.
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(bad, c);
}

__global__ void gather_kernel(int64_t rows, int64_t count, int elem_size,
                              const int64_t* __restrict__ src, const char* __restrict__ in,
                              char* __restrict__ out) {
  const int64_t total = rows * count * elem_size;
  const int64_t row_bytes = count * elem_size;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i / row_bytes, c = i - r * row_bytes;
    out[i] = in[src[r] * elem_size + c];
  }
}

__global__ void sum_shares_kernel(int64_t num_keys, int64_t row_len, int bits, int xor_mode,
                                  const char* __restrict__ shares, uint64_t* __restrict__ sums) {
  const int eb = bits / 8;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < row_len;
       j += (int64_t)gridDim.x * blockDim.x) {
    uint64_t acc = 0;
    for (int64_t k = 0; k < num_keys; ++k) {
      const char* p = shares + (k * row_len + j) * eb;
      uint64_t v = 0;
      if (eb == 8) v = *reinterpret_cast<const uint64_t*>(p);
      else if (eb == 4) v = *reinterpret_cast<const uint32_t*>(p);
      else if (eb == 2) v = *reinterpret_cast<const uint16_t*>(p);
      else v = *reinterpret_cast<const uint8_t*>(p);
      acc = xor_mode ? (acc ^ v) : (acc + v);
    }
    sums[j] = acc;
  }
}

// ------------------------------------------------------------------------
// Host-side launch helpers
// ------------------------------------------------------------------------
}  // namespace

namespace dpf_rt {
int num_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0)
      cus = 256;
  }
  return cus;
}

int max_block() { return kBlock; }
int max_subtree_depth() { return kSMax; }

int block_for(int64_t work_items) {
  // A launch smaller than one full workgroup per CU runs LDS-bound on the few
  // CUs it occupies: give each CU a smaller workgroup instead (the tables cost
  // ~1 us to fill whatever the workgroup size).
  const int64_t cus = num_cus();
  int64_t per_cu = (work_items + cus - 1) / cus;
  int64_t b = (per_cu + 63) / 64 * 64;
  if (b < 64) b = 64;
  if (b > kBlock) b = kBlock;
  return (int)b;
}

int grid_for(int64_t work_items, int block) {
  int64_t g = (work_items + block - 1) / block;
  int64_t cap = num_cus() * kWgPerCu;  // one 128 KiB-LDS workgroup per CU
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

LaunchShape chunked_shape(int64_t items, const char* hook) {
  LaunchShape sh{block_for(items), 0, 0};
  sh.grid = grid_for(items, sh.block);
  const int64_t chunks = (items + 63) / 64;
  if (!hook_is(hook, '0') && chunks >= (int64_t)sh.grid * (sh.block / 64) * 4)
    sh.dyn_per_wg = (chunks + sh.grid - 1) / sh.grid;
  g_last_dynamic_chunks = sh.dyn_per_wg;
  return sh;
}

int validate_desc(const dpf_value_desc* d) {
  if (!d) return fail(kInvalidArgument, "value descriptor is NULL");
  if (d->num_leaves < 1 || d->num_leaves > DPF_MAX_LEAVES)
    return fail(kUnimplemented, "value type has too many leaves for the GPU path");
  if (d->blocks_needed < 1 || d->blocks_needed > kBMax)
    return fail(kUnimplemented, "value type needs too many AES blocks for the GPU path");
  if (d->elements_per_block < 1) return fail(kInvalidArgument, "elements_per_block < 1");
  for (int k = 0; k < d->num_leaves; ++k) {
    int b = d->bits[k];
    if (b < 8 || b > 128 || (b & (b - 1)))
      return fail(kUnimplemented, "leaf bit size must be a power of two in [8, 128]");
    if (d->kind[k] == DPF_LEAF_INTMODN && d->mod_low[k] == 0 && d->mod_high[k] == 0)
      return fail(kInvalidArgument, "IntModN modulus is zero");
  }
  return kOk;
}

int packed_size(const dpf_value_desc* d) {
  int s = 0;
  for (int k = 0; k < d->num_leaves; ++k) s += d->bits[k] / 8;
  return s;
}

bool fast_int(const dpf_value_desc* d) {
  return d->num_leaves == 1 && d->direct && d->blocks_needed == 1 &&
         d->kind[0] != DPF_LEAF_INTMODN;
}


}  // namespace dpf_rt

namespace {

template <class Leaf>
const char* leaf_name() {
  if constexpr (std::is_same_v<Leaf, SwarLeaf>) return "swar";
  else if constexpr (std::is_same_v<Leaf, GenericLeaf>) return "generic";
  else if constexpr (std::is_same_v<Leaf, Mod32Leaf<2>> || std::is_same_v<Leaf, Mod32Leaf<4>> ||
                     std::is_same_v<Leaf, Mod32Leaf<kMod32MaxLeaves>>) return "mod32";
  else return "fast";
}

// Records the launch for dpf_hip_last_expand_kernel().
template <class Leaf>
void note_expand(const ExpandParams& p, bool octet) {
  static const std::string pair = std::string("pair/") + leaf_name<Leaf>();
  static const std::string oct = std::string("octet/") + leaf_name<Leaf>();
  g_last_expand = octet ? oct.c_str() : pair.c_str();
  g_last_expand_s = p.S;
}

// Launches expand_small_kernel<Leaf> when the tree has the small shape.
template <class Leaf>
bool try_small(const ExpandParams& p0, const Leaf& leaf, hipStream_t s) {
  int t = 0, D = 0;
  const int64_t starts = p0.num_items >> p0.k0;
  if (!small_shape(starts, p0.num_levels, &t, &D)) return false;
  ExpandParams p = p0;
  p.k0 = t;
  p.S = D;
  p.num_items = starts << t;
  static const std::string name = std::string("small/") + leaf_name<Leaf>();
  g_last_expand = name.c_str();
  g_last_expand_s = D;
  hipLaunchKernelGGL((expand_small_kernel<Leaf>), dim3((unsigned)p.num_items), dim3(kBlock), 0, s,
                     p, leaf);
  return true;
}


// Tree-top pass of an octet launch (r16).  Every octet-kernel item walks k0
// levels from its start seed to its subtree root, one dependent AES per level
// per lane: at config 2's 2^30 outputs 18 of each lane's ~6160 AES, but at
// the 2^27-output shard a rank evaluates in an 8-GPU run (784 AES per lane)
// the walk is ~4.5% of the kernel.  Instead, expand_small_kernel<SeedLeaf>
// expands the top of the tree breadth-first -- each workgroup's wave 0 walks
// to its subtree root in lane quads, then up to 11 levels through LDS, every
// node hashed once -- and writes the 2^k0-per-start item roots (17 B each,
// stream-ordered scratch); the octet kernel then starts at them (k0 = 0).
// top_shape (dpf_expand_plan.hip) says whether the pass applies and its shape.
struct TopScratch {
  void* mem = nullptr;
  hipStream_t s = nullptr;
  ~TopScratch() {
    if (mem) (void)hipFreeAsync(mem, s);
  }
};
// Returns the error of a failed launch, else kOk (p rewritten when the pass ran).
// With `counter`, the scratch also holds the launch's chunk counter on a
// 128-byte line of its own, zeroed by the pass (*counter set when it ran).
int expand_top(ExpandParams& p, hipStream_t s, TopScratch& scratch,
               unsigned int** counter = nullptr) {
  const int64_t starts = p.num_items >> p.k0;
  int t = 0, D = 0;
  if (!top_shape(p.num_items, p.k0, &t, &D)) return kOk;
  static const bool pool_kept = [] {
    int dev = 0;
    hipMemPool_t pool;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetDefaultMemPool(&pool, dev) != hipSuccess)
      return false;
    uint64_t keep = UINT64_MAX;
    return hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep) == hipSuccess;
  }();
  (void)pool_kept;
  const size_t items = (size_t)p.num_items;
  void* mem = nullptr;
  const size_t roots = (items * (sizeof(dpf_block) + 1) + 127) / 128 * 128;
  HIP_TRY(hipMallocAsync(&mem, roots + (counter ? 128 : 0), s));
  scratch.mem = mem;
  scratch.s = s;
  SeedLeaf leaf{static_cast<dpf_block*>(mem),
                static_cast<uint8_t*>(mem) + items * sizeof(dpf_block),
                counter ? reinterpret_cast<unsigned int*>(static_cast<char*>(mem) + roots)
                        : nullptr};
  if (counter) *counter = leaf.counter;
  ExpandParams q = p;
  q.k0 = t;
  q.S = D;
  q.num_levels = p.k0;
  q.num_items = starts << t;
  q.clock = nullptr;
  hipLaunchKernelGGL((expand_small_kernel<SeedLeaf>), dim3((unsigned)q.num_items), dim3(kBlock), 0,
                     s, q, leaf);
  HIP_TRY(hipGetLastError());
  // The octet kernel starts at the item roots: k0 = 0, correction words from
  // level k0 on.
  p.seeds_in = leaf.seeds;
  p.ctrl_in = leaf.ctrl;
  p.cw_seed += p.k0;
  p.cw_left += p.k0;
  p.cw_right += p.k0;
  p.num_levels = p.S;
  p.k0 = 0;
  return kOk;
}

// Runs the tree-top pass and sets p's shape (and *grid, *blk) for the octet
// kernel launch.
thread_local ChunkPlan g_last_plan{};   // dpf_hip_last_expand_schedule
// sched_ok: whether launches of this kernel and leaf type get the chip-wide
// counter and the taper by default (SchedDefault; the hooks still set them).
int subtree_shape(ExpandParams& p, int min_S, hipStream_t s, TopScratch& top, int* grid,
                  int* blk, bool sched_ok) {
  p.dyn_chunks = 0;
  p.chunk_counter = nullptr;
  g_last_plan = ChunkPlan{};
  const int64_t cus = num_cus();
  const ChunkPlan plan = plan_chunks(p.num_items, p.k0, p.S, min_S, cus, sched_ok);
  if (const int sh = plan.shift) {
    ExpandParams q = p;
    q.S -= sh;
    q.k0 += sh;
    q.num_items <<= sh;
    q.dyn_chunks = (int)(q.num_items / (cus * 64));
    int64_t taken = 0;
    for (int j = 0; j < 3; ++j) {
      taken += plan.chunks[j] / plan.groups;
      q.ph_end[j] = (int)taken;
      q.ph_item[j] = plan.first_item[j];
    }
    unsigned int* counter = nullptr;
    unsigned int** want_counter = plan.global ? &counter : nullptr;
    // The tree-top pass stops `up` levels above the items (a quarter of the
    // roots for 2: fewer rounds of its latency-bound workgroups), and every
    // item walks those levels itself (one path step per level, in the octet
    // kernel's throughput mode).  Where it does not apply at that height, it
    // is tried again down to the items (up = 0).
    const int w = octet_walk_levels();
    int up = w > 0 && q.k0 - w >= 8 ? w : 0;
    ExpandParams t;
    for (;; up = 0) {
      t = q;
      t.k0 = q.k0 - up;
      t.S = q.S + up;
      t.num_items = q.num_items >> up;
      if (int st = expand_top(t, s, top, want_counter)) return st;
      if (t.k0 == 0 || up == 0) break;
    }
    if (t.k0 == 0) {   // the pass ran: the items start `up` levels below its roots
      q.chunk_counter = counter;
      q.seeds_in = t.seeds_in;
      q.ctrl_in = t.ctrl_in;
      q.cw_seed = t.cw_seed;
      q.cw_left = t.cw_left;
      q.cw_right = t.cw_right;
      q.num_levels = q.S + up;
      q.k0 = up;
      p = q;
      g_last_plan = plan;
      *grid = (int)cus;
      *blk = kBlock;
      return kOk;
    }
  }
  if (int st = expand_top(p, s, top)) return st;
  *blk = block_for(p.num_items);
  *grid = grid_for(p.num_items, *blk);
  return kOk;
}
// The two SCHED instances that spill are not a default: the octet kernel
// with SwarLeaf (4 VGPRs) and the pair kernel with Mod32Leaf<5> (20 B of
// scratch per lane); every other SCHED instance has none.
template <class Leaf, bool OCTET> struct SchedDefault { static constexpr bool value = true; };
template <> struct SchedDefault<SwarLeaf, true> { static constexpr bool value = false; };
template <> struct SchedDefault<Mod32Leaf<kMod32MaxLeaves>, false> {
  static constexpr bool value = false;
};
// Launches with one counter for the launch or with finer phases run the
// kernels' SCHED instance; static launches and uniform chunks per workgroup
// the one whose subtree shape is a launch constant.
bool has_schedule(const ExpandParams& p) {
  return p.dyn_chunks && (p.chunk_counter || p.ph_end[0] != p.ph_end[2]);
}
// Leaf policies with an expand_octet_kernel instance: integer leaves (whole
// 16-byte blocks only: dispatch_expand's octet_ok), SWAR tuples and pairs of
// IntModN<uint32_t> (the half's four leaves hashed as two ILP4 groups).
template <class Leaf> struct HasOctet : std::false_type {};
template <int BITS, bool XOR> struct HasOctet<FastIntLeaf<BITS, XOR>> : std::true_type {};
template <int BITS, bool XOR> struct HasOctet<DotLeaf<BITS, XOR>> : std::true_type {};
template <> struct HasOctet<SwarLeaf> : std::true_type {};
template <> struct HasOctet<Mod32Leaf<2>> : std::true_type {};

// The one launch path of full-domain expansion: the small-tree kernel where
// the tree has that shape, else the octet kernel for leaf policies that have
// one whenever the subtrees have >= 8 leaves (DPF_EXPAND_NO_OCTET=1, read per
// launch, forces expand_kernel), else the pair kernel.  The latter two take
// the shape subtree_shape gives them (tree-top pass, dynamic 64-item chunks):
// subtrees of >= 3 levels for octets, >= 1 for leaf pairs.
template <class Leaf>
int dispatch_expand(const ExpandParams& p0, const Leaf& leaf, bool octet_ok, hipStream_t s) {
  TopScratch top;
  // GenericLeaf's conversion spills in the small kernel's register budget and
  // measured 0.93-1.07x there (profiles/r15_ab.txt part 13): not dispatched.
  const bool small = !std::is_same_v<Leaf, GenericLeaf> && try_small(p0, leaf, s);
  if (!small) {
    const bool octet = HasOctet<Leaf>::value && octet_ok && p0.S >= 3 &&
                       !hook_is("DPF_EXPAND_NO_OCTET", '1');
    note_expand<Leaf>(p0, octet);
    ExpandParams p = p0;
    int grid = 0, blk = 0;
    const bool sched_ok = octet ? SchedDefault<Leaf, true>::value : SchedDefault<Leaf, false>::value;
    if (int st = subtree_shape(p, octet ? 3 : 1, s, top, &grid, &blk, sched_ok)) return st;
    const bool sched = has_schedule(p);
    if (octet) {
      if constexpr (HasOctet<Leaf>::value) {
        if (sched)
          hipLaunchKernelGGL((expand_octet_kernel<Leaf, true>), dim3(grid), dim3(blk), 0, s, p, leaf);
        else
          hipLaunchKernelGGL((expand_octet_kernel<Leaf, false>), dim3(grid), dim3(blk), 0, s, p, leaf);
      }
    } else if (sched) {
      hipLaunchKernelGGL((expand_kernel<Leaf, true>), dim3(grid), dim3(blk), 0, s, p, leaf);
    } else {
      hipLaunchKernelGGL((expand_kernel<Leaf, false>), dim3(grid), dim3(blk), 0, s, p, leaf);
    }
  }
  HIP_TRY(hipGetLastError());
  return kOk;
}

// The leaf policies of dpf_hip_expand, each built from the value descriptor
// and dispatched.  Integer leaves (and uniform tuples as E * num_leaves
// lanes): the octet kernel only where a leaf fills its whole 16-byte block.
template <int BITS>
int expand_fast_leaf(const ExpandParams& p, bool xor_leaf, const dpf_block* vcw, int E, int party,
                     int store_bytes, hipStream_t s) {
  const bool octet_ok = store_bytes == 16;
  if (xor_leaf)
    return dispatch_expand(p, FastIntLeaf<BITS, true>{vcw, E, party, store_bytes, {}}, octet_ok, s);
  return dispatch_expand(p, FastIntLeaf<BITS, false>{vcw, E, party, store_bytes, {}}, octet_ok, s);
}
int expand_fast(const ExpandParams& p, const dpf_value_desc* d, const dpf_block* vcw, int E,
                int party, int store_bytes, hipStream_t s) {
  const bool x = d->kind[0] == DPF_LEAF_XOR;
  return with_bits(d->bits[0], [&](auto bits) {
    return expand_fast_leaf<decltype(bits)::value>(p, x, vcw, E, party, store_bytes, s);
  });
}
// Direct tuples of plain integers / XorWrappers of mixed widths or kinds:
// lane i of the hashed block is element i % num_leaves.
SwarLeaf make_swar_leaf(const dpf_value_desc* desc, const dpf_block* vcw, int lanes, int party,
                        int store_bytes) {
  SwarLeaf w;
  memset(&w, 0, sizeof(w));
  w.vcw_elems = vcw;
  w.lanes = lanes;
  w.party = party;
  w.store_bytes = store_bytes;
  const int nl = desc->num_leaves;
  int off = 0;
  for (int i = 0; i < lanes; ++i) {
    const int b = desc->bits[i % nl];
    w.lane_off[i] = (uint8_t)off;
    w.lane_bits[i] = (uint8_t)b;
    w.top |= (u128)1 << (off + b - 1);
    if (desc->kind[i % nl] == DPF_LEAF_XOR)
      w.xmask |= (b >= 128 ? ~(u128)0 : (((u128)1 << b) - 1)) << off;
    off += b;
  }
  return w;
}
// Tuples of IntModN<uint32_t, N>: Moller-Granlund sampling.
template <int NL>
Mod32Leaf<NL> make_mod32_leaf(const dpf_value_desc* desc, const dpf_block* vcw, int b, int party) {
  Mod32Leaf<NL> m;
  memset(&m, 0, sizeof(m));
  m.vcw_elems = vcw;
  m.nl = desc->num_leaves;
  m.b = b;
  m.party = party;
  for (int k = 0; k < desc->num_leaves; ++k) m.div[k] = make_div32((uint32_t)desc->mod_low[k]);
  return m;
}
GenericLeaf make_generic_leaf(const dpf_value_desc* desc, const dpf_block* vcw, int party,
                              int elements_per_leaf) {
  GenericLeaf g;
  g.d = *desc;
  g.vcw = vcw;
  g.party = party;
  g.elements_per_leaf = elements_per_leaf;
  g.esz = packed_size(desc);
  return g;
}

}  // namespace

// ==========================================================================
// C ABI
// ==========================================================================
extern "C" {

int dpf_hip_abi_version(void) { return DPF_HIP_ABI_VERSION; }
const char* dpf_hip_last_error(void) { return dpf_rt::g_last_error.c_str(); }

int dpf_hip_last_dynamic_chunks(int64_t* per_wg) {
  if (!per_wg) return fail(kInvalidArgument, "per_wg is NULL");
  *per_wg = dpf_rt::g_last_dynamic_chunks;
  return kOk;
}
const char* dpf_hip_last_expand_kernel(int* subtree_depth) {
  if (subtree_depth) *subtree_depth = dpf_rt::g_last_expand_s;
  return dpf_rt::g_last_expand;
}

int dpf_hip_clock_probe(int on) {
  unsigned long long* old = dpf_rt::g_clock_acc.exchange(nullptr);
  if (old) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipFree(old));
  }
  if (!on) return kOk;
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, kProbeBytes));
  HIP_TRY(hipMemset(p, 0, kProbeBytes));
  HIP_TRY(hipDeviceSynchronize());
  dpf_rt::g_clock_acc.store(static_cast<unsigned long long*>(p));
  return kOk;
}

int dpf_hip_clock_probe_exits(double* out) {
  unsigned long long* acc = dpf_rt::g_clock_acc.load();
  if (!acc) return fail(kFailedPrecondition, "clock probe is off (dpf_hip_clock_probe(1))");
  if (!out) return fail(kInvalidArgument, "NULL pointer");
  std::vector<unsigned long long> h(kProbeWords + kProbeWorkgroups);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h.data(), acc, kProbeBytes, hipMemcpyDeviceToHost));
  for (int i = 0; i < 6; ++i) out[i] = 0.0;
  if (h[kProbeLastExit] == 0 || h[kProbeFirstBegin] == 0) return kOk;   // nothing stamped
  const unsigned long long t0 = ~h[kProbeFirstBegin];
  auto sec = [&](unsigned long long t) { return (double)(int64_t)(t - t0) * 1e-8; };
  double lo = 0, hi = 0, sum = 0;
  int n = 0;
  for (int i = 0; i < kProbeWorkgroups; ++i) {
    if (!h[kProbeWords + i]) continue;
    const double t = sec(h[kProbeWords + i]);
    lo = n ? (t < lo ? t : lo) : t;
    hi = n ? (t > hi ? t : hi) : t;
    sum += t;
    ++n;
  }
  out[0] = sec(~h[kProbeFirstExit]);
  out[1] = sec(h[kProbeLastExit]);
  out[2] = lo;
  out[3] = hi;
  out[4] = n ? sum / n : 0.0;
  out[5] = n;
  return kOk;
}

int dpf_hip_last_expand_schedule(int64_t* out) {
  if (!out) return fail(kInvalidArgument, "NULL pointer");
  dpf_rt::write_plan(g_last_plan, out);
  return kOk;
}

int dpf_hip_clock_probe_read(double* clock_ghz, int64_t* workgroups, double* mean_workgroup_s) {
  unsigned long long* acc = dpf_rt::g_clock_acc.load();
  if (!acc) return fail(kFailedPrecondition, "clock probe is off (dpf_hip_clock_probe(1))");
  unsigned long long h[4] = {0, 0, 0, 0};
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h, acc, sizeof(h), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(acc, 0, kProbeBytes));
  HIP_TRY(hipDeviceSynchronize());
  // s_memtime counts shader clocks, s_memrealtime a constant 100 MHz.
  if (clock_ghz) *clock_ghz = h[1] ? (double)h[0] / (double)h[1] * 0.1 : 0.0;
  if (workgroups) *workgroups = (int64_t)h[2];
  if (mean_workgroup_s) *mean_workgroup_s = h[2] ? (double)h[1] / (double)h[2] * 1e-8 : 0.0;
  return kOk;
}

int dpf_hip_packed_element_size(const dpf_value_desc* desc) {
  if (!desc) return -1;
  return packed_size(desc);
}

int dpf_hip_hash(int64_t n, const dpf_block* in, const dpf_aes_key* key, dpf_block* out,
                 void* stream) {
  if (n < 0) return fail(kInvalidArgument, "n < 0");
  if (n == 0) return kOk;
  if (!in || !out || !key) return fail(kInvalidArgument, "NULL pointer");
  // DPF_HASH_DYNAMIC=0: a fixed share of blocks per thread (A/B hook).
  const LaunchShape sh = chunked_shape(n, "DPF_HASH_DYNAMIC");
  hipLaunchKernelGGL(hash_kernel, dim3(sh.grid), dim3(sh.block), 0, (hipStream_t)stream, n, in,
                     out, expand_key(key), sh.dyn_per_wg);
  HIP_TRY(hipGetLastError());
  return kOk;
}

int dpf_hip_eval_paths(int64_t num_seeds, int num_levels, const dpf_block* seeds_in,
                       const uint8_t* control_in, const dpf_block* paths,
                       const dpf_block* cw_seed, const uint8_t* cw_left, const uint8_t* cw_right,
                       const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                       dpf_block* seeds_out, uint8_t* control_out, void* stream) {
  if (num_seeds < 0 || num_levels < 0 || num_levels > kMaxCwLevels)
    return fail(kInvalidArgument, "num_seeds or num_levels out of range");
  if (num_seeds == 0) return kOk;
  hipStream_t s = (hipStream_t)stream;
  if (num_levels == 0) {
    if (seeds_out != seeds_in)
      HIP_TRY(hipMemcpyAsync(seeds_out, seeds_in, num_seeds * sizeof(dpf_block),
                             hipMemcpyDeviceToDevice, s));
    if (control_out != control_in)
      HIP_TRY(hipMemcpyAsync(control_out, control_in, num_seeds, hipMemcpyDeviceToDevice, s));
    return kOk;
  }
  if (!seeds_in || !control_in || !paths || !cw_seed || !cw_left || !cw_right || !key_left ||
      !key_right || !seeds_out || !control_out)
    return fail(kInvalidArgument, "NULL pointer");
  PathParams p;
  p.n = num_seeds;
  p.num_levels = num_levels;
  p.seeds_in = seeds_in;
  p.ctrl_in = control_in;
  p.paths = paths;
  p.cw_seed = cw_seed;
  p.cw_left = cw_left;
  p.cw_right = cw_right;
  p.seeds_out = seeds_out;
  p.ctrl_out = control_out;
  p.rkl = expand_key(key_left);
  p.rkd = xor_keys(p.rkl, expand_key(key_right));
  const LaunchShape sh = chunked_shape(num_seeds, "DPF_PATHS_DYNAMIC");
  p.dyn_per_wg = sh.dyn_per_wg;
  hipLaunchKernelGGL(eval_paths_kernel, dim3(sh.grid), dim3(sh.block), 0, s, p);
  HIP_TRY(hipGetLastError());
  return kOk;
}

// Argument checks and launch parameters dpf_hip_expand and dpf_hip_expand_dot
// share (`out` apart).
static int expand_params(int64_t num_starts, const dpf_block* seeds_in, const uint8_t* control_in,
                         int num_levels, const dpf_block* cw_seed, const uint8_t* cw_left,
                         const uint8_t* cw_right, const dpf_aes_key* key_left,
                         const dpf_aes_key* key_right, const dpf_aes_key* key_value,
                         const dpf_value_desc* desc, int elements_per_leaf,
                         const dpf_block* value_correction, ExpandParams* out) {
  int st = validate_desc(desc);
  if (st) return st;
  if (num_starts < 0 || num_levels < 0 || num_levels > 62)
    return fail(kInvalidArgument, "num_starts or num_levels out of range");
  if (elements_per_leaf < 1 || elements_per_leaf > desc->elements_per_block)
    return fail(kInvalidArgument, "elements_per_leaf must be in [1, elements_per_block]");
  if (num_starts == 0) return kOk;
  if (!seeds_in || !control_in || !key_left || !key_right || !key_value || !value_correction ||
      (num_levels > 0 && (!cw_seed || !cw_left || !cw_right)))
    return fail(kInvalidArgument, "NULL pointer");
  if (num_starts > (INT64_MAX >> num_levels))
    return fail(kInvalidArgument, "expansion too large");
  ExpandParams p{};   // static launch, no chunk schedule
  p.num_levels = num_levels;
  p.S = choose_subtree_depth(num_starts, num_levels);
  p.k0 = num_levels - p.S;
  p.num_items = num_starts << p.k0;
  p.seeds_in = seeds_in;
  p.ctrl_in = control_in;
  p.cw_seed = cw_seed;
  p.cw_left = cw_left;
  p.cw_right = cw_right;
  p.rkl = expand_key(key_left);
  p.rkr = expand_key(key_right);
  p.rkv = expand_key(key_value);
  p.rkd = xor_keys(p.rkl, p.rkr);
  p.clock = dpf_rt::g_clock_acc.load(std::memory_order_relaxed);
  *out = p;
  return kOk;
}

int dpf_hip_expand(int64_t num_starts, const dpf_block* seeds_in, const uint8_t* control_in,
                   int num_levels, const dpf_block* cw_seed, const uint8_t* cw_left,
                   const uint8_t* cw_right, const dpf_aes_key* key_left,
                   const dpf_aes_key* key_right, const dpf_aes_key* key_value,
                   const dpf_value_desc* desc, int elements_per_leaf,
                   const dpf_block* value_correction, int party, void* out, void* stream) {
  ExpandParams p{};
  if (int st = expand_params(num_starts, seeds_in, control_in, num_levels, cw_seed, cw_left,
                             cw_right, key_left, key_right, key_value, desc, elements_per_leaf,
                             value_correction, &p))
    return st;
  if (num_starts == 0) return kOk;
  if (!out) return fail(kInvalidArgument, "NULL pointer");
  p.out = (char*)out;
  hipStream_t s = (hipStream_t)stream;
  if (fast_int(desc))
    return expand_fast(p, desc, value_correction, desc->elements_per_block, party,
                       elements_per_leaf * desc->bits[0] / 8, s);
  const int esz = packed_size(desc);
  if (desc->direct && desc->blocks_needed == 1) {
    // Direct tuples of plain integers / XorWrappers: the hashed block is E
    // packed elements (value_type_helpers.h:199-211).
    const int nl = desc->num_leaves, bits = desc->bits[0], kind = desc->kind[0];
    bool uniform = true;
    for (int k = 1; k < nl; ++k) uniform = uniform && desc->bits[k] == bits && desc->kind[k] == kind;
    const int lanes = desc->elements_per_block * nl;
    // Every lane the same width and kind: the integer fast path with E * nl lanes.
    if (uniform && lanes * bits <= 128)
      return expand_fast(p, desc, value_correction, lanes, party, elements_per_leaf * esz, s);
    if (lanes <= 16 && desc->elements_per_block * esz <= 16)
      return dispatch_expand(
          p, make_swar_leaf(desc, value_correction, lanes, party, elements_per_leaf * esz), true, s);
  }
  int b = 0;
  if (elements_per_leaf == 1 && mod32_eligible(desc, &b)) {
    if (desc->num_leaves <= 2)
      return dispatch_expand(p, make_mod32_leaf<2>(desc, value_correction, b, party), true, s);
    if (desc->num_leaves <= 4)   // no spills (Mod32Leaf<5> in expand_kernel: 36 B)
      return dispatch_expand(p, make_mod32_leaf<4>(desc, value_correction, b, party), true, s);
    return dispatch_expand(p, make_mod32_leaf<kMod32MaxLeaves>(desc, value_correction, b, party),
                           true, s);
  }
  return dispatch_expand(p, make_generic_leaf(desc, value_correction, party, elements_per_leaf),
                         true, s);
}

// Full-domain expansion folded into the database at the leaves: the launch
// plan, kernels and chunk schedule are dpf_hip_expand's, with DotLeaf in
// FastIntLeaf's place; then the workgroups' partials are folded into `out`.
int dpf_hip_expand_dot(int64_t num_starts, const dpf_block* seeds_in, const uint8_t* control_in,
                       int num_levels, const dpf_block* cw_seed, const uint8_t* cw_left,
                       const uint8_t* cw_right, const dpf_aes_key* key_left,
                       const dpf_aes_key* key_right, const dpf_aes_key* key_value,
                       const dpf_value_desc* desc, int elements_per_leaf,
                       const dpf_block* value_correction, int party, const void* db,
                       int record_words, void* workspace, void* out, void* stream) {
  ExpandParams p{};
  if (int st = expand_params(num_starts, seeds_in, control_in, num_levels, cw_seed, cw_left,
                             cw_right, key_left, key_right, key_value, desc, elements_per_leaf,
                             value_correction, &p))
    return st;
  int words = 0, xor_type = 0;
  if (int st = dot_type(desc, &words, &xor_type)) return st;
  if (record_words < 1 || record_words > DPF_HIP_DOT_MAX_RECORD_WORDS)
    return fail(kInvalidArgument, "record_words must be in [1, 1024]");
  if (!db || !workspace || !out) return fail(kInvalidArgument, "NULL pointer");
  if (!dpf_hip_expand_dot_fused(desc, record_words))
    return fail(kUnimplemented,
                "no fused kernel for this record width: dpf_hip_expand into scratch, then "
                "dpf_hip_dot_rows");
  if (num_cus() > kDotMaxGroups) return fail(kInternal, "more workgroups than partial rows");
  hipStream_t s = (hipStream_t)stream;
  if (num_starts == 0) {   // an empty sum
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)words * 8, s));
    return kOk;
  }
  const int store_bytes = elements_per_leaf * desc->bits[0] / 8;
  char* ws = static_cast<char*>(workspace);
  const char* d = static_cast<const char*>(db);
  const int E = desc->elements_per_block;
  int st;
  if (desc->bits[0] == 128)
    st = dispatch_expand(p, DotLeaf<128, true>{{value_correction, E, party, store_bytes, {}}, d, ws, 0, 0},
                         true, s);
  else if (xor_type)
    st = dispatch_expand(p, DotLeaf<64, true>{{value_correction, E, party, store_bytes, {}}, d, ws, 0, 0},
                         store_bytes == 16, s);
  else
    st = dispatch_expand(p, DotLeaf<64, false>{{value_correction, E, party, store_bytes, {}}, d, ws, 0, 0},
                         store_bytes == 16, s);
  if (st) return st;
  const char* k = dpf_rt::g_last_expand;
  g_last_dot = k[0] == 's' ? "small" : (k[0] == 'o' ? "octet" : "pair");
  // The kernel's first workgroup wrote the number of partial rows.
  return launch_dot_fold(words, xor_type, 0, workspace, out, s);
}

int dpf_hip_count_out_of_range(int64_t n, const dpf_block* points, int log_domain_size,
                               int64_t* count, void* stream) {
  if (!count || n < 0 || log_domain_size < 0 || log_domain_size > 128)
    return fail(kInvalidArgument, "bad arguments");
  *count = 0;
  if (n == 0 || log_domain_size == 128) return kOk;
  if (!points) return fail(kInvalidArgument, "NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* d = nullptr;
  HIP_TRY(hipMallocAsync((void**)&d, sizeof(*d), s));
  HIP_TRY(hipMemsetAsync(d, 0, sizeof(*d), s));
  int64_t g = (n + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(count_out_of_range_kernel, dim3((unsigned)g), dim3(256), 0, s, n, points,
                     log_domain_size, d);
  HIP_TRY(hipGetLastError());
  unsigned long long h = 0;
  HIP_TRY(hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipFreeAsync(d, s));
  HIP_TRY(hipStreamSynchronize(s));
  *count = (int64_t)h;
  return kOk;
}

int dpf_hip_gather(int64_t num_rows, int64_t count, int elem_size, const int64_t* src_offset,
                   const void* in, void* out, void* stream) {
  if (num_rows < 0 || count < 0 || elem_size < 1) return fail(kInvalidArgument, "bad sizes");
  int64_t total = num_rows * count * elem_size;
  if (total == 0) return kOk;
  int64_t g = (total + 255) / 256;
  if (g > 65536) g = 65536;
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                     num_rows, count, elem_size, src_offset, (const char*)in, (char*)out);
  HIP_TRY(hipGetLastError());
  return kOk;
}

int dpf_hip_sum_shares_u64(int64_t num_keys, int64_t row_len, int bits, int xor_mode,
                           const void* shares, uint64_t* sums, void* stream) {
  if (num_keys < 0 || row_len < 0 || !(bits == 8 || bits == 16 || bits == 32 || bits == 64))
    return fail(kInvalidArgument, "bad arguments");
  if (row_len == 0) return kOk;
  int64_t g = (row_len + 255) / 256;
  if (g > 65536) g = 65536;
  hipLaunchKernelGGL(sum_shares_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                     num_keys, row_len, bits, xor_mode, (const char*)shares, sums);
  HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
