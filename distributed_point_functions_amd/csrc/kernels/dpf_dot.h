// dpf_dot.h -- full-domain expansion folded into a database at the leaves
// (dpf_hip_expand_dot): the leaf policy that replaces FastIntLeaf's stores by
// out = sum_i y[i] * db[i] (uint64_t, mod 2^64) or XOR_i (y[i] & db[i])
// (XorWrapper<uint64_t>, XorWrapper<uint128>), one database word per element
// (record_words == 1), and the layout of the workspace its partials go to.
// Included by dpf_kernels.hip after dpf_device.h.
#pragma once
#include "dpf_device.h"

namespace {

// Workspace of the dot calls: a header line whose first word is the number of
// partial rows the last kernel wrote (its workgroups), then the rows, each
// record_words elements as uint64 words.  The fold kernel (dpf_dot.hip) reads
// the count, so nothing depends on what the workspace held before.
constexpr int kDotHeaderBytes = 128;
constexpr int kDotMaxGroups = 1024;   // partial rows a workspace has room for

// Integer leaves filling whole blocks, multiplied (ANDed) with the database
// instead of stored.  The sums live in two uint64 per lane: the block's two
// halves (two uint64_t elements, or the halves of one uint128), combined at
// the end.  Correction and party negation are FastIntLeaf's, before the
// product.
template <int BITS, bool XOR>
struct DotLeaf {
  static_assert(BITS == 64 || (BITS == 128 && XOR), "uint64_t, XorWrapper<uint64_t / uint128>");
  FastIntLeaf<BITS, XOR> f;
  const char* db;    // element i of the expansion order at db + i * BITS / 8
  char* workspace;   // header, then one partial (BITS / 8 bytes) per workgroup
  mutable uint64_t a0, a1;

  __device__ __forceinline__ void init() {
    f.init();
    a0 = a1 = 0;
  }
  __device__ __forceinline__ Block4 correct(Block4 h, uint32_t t) const { return f.correct(h, t); }
  // The database words under leaf block `leaf`: 16 bytes, or the one kept
  // element's 8 (the block's other half then meets zero).
  __device__ __forceinline__ uint4 load(int64_t leaf) const {
    if (f.store_bytes == 16) return *reinterpret_cast<const uint4*>(db + leaf * 16);
    const uint2 v = *reinterpret_cast<const uint2*>(db + leaf * 8);
    return make_uint4(v.x, v.y, 0u, 0u);
  }
  __device__ __forceinline__ void add(Block4 h, uint4 d) const {
    const uint64_t hl = ((uint64_t)h.w1 << 32) | h.w0, hh = ((uint64_t)h.w3 << 32) | h.w2;
    const uint64_t dl = ((uint64_t)d.y << 32) | d.x, dh = ((uint64_t)d.w << 32) | d.z;
    if (XOR) {
      a0 ^= hl & dl;
      a1 ^= hh & dh;
    } else {
      a0 += hl * dl;
      a1 += hh * dh;
    }
    // The sums are taken leaf by leaf: left free, the compiler reassociates
    // the chain over an octet's eight leaves and keeps their blocks live
    // (96 spilled VGPRs in the octet kernel).
    asm volatile("" : "+v"(a0), "+v"(a1));
  }
  // expand_small_kernel's quad ending: the corrected block of leaf `leaf`.
  __device__ __forceinline__ void store(Block4 h, int64_t leaf, char*) const { add(h, load(leaf)); }

  // The database loads are issued before the value hashes they wait behind.
  __device__ __forceinline__ void emit(const LdsLookup& lk, KeyRef rkv, Block4 seed, uint32_t t,
                                       int64_t leaf, char*) const {
    const uint4 d = load(leaf);
    add(correct(dpf_aes::mmo_hash(seed, lk, UniformRK{rkv}), t), d);
  }
  __device__ __forceinline__ void emit2(const LdsLookup& lk, KeyRef rkv, Block4 s0, uint32_t t0,
                                        Block4 s1, uint32_t t1, int64_t leaf, char*) const {
    const uint4 d0 = load(leaf), d1 = load(leaf + 1);
    dpf_aes::mmo_hash2(s0, s1, lk, UniformRK{rkv}, UniformRK{rkv});
    add(correct(s0, t0), d0);
    add(correct(s1, t1), d1);
  }
  // Half an octet: 64 contiguous database bytes per lane (octets only run
  // with whole blocks kept).
  __device__ __forceinline__ void emit4(const LdsLookup& lk, KeyRef rkv, Block4* s,
                                        const uint32_t* t, int64_t leaf, char*) const {
    const uint4* p = reinterpret_cast<const uint4*>(db + leaf * 16);
    const UniformRK rk[4] = {UniformRK{rkv}, UniformRK{rkv}, UniformRK{rkv}, UniformRK{rkv}};
    if constexpr (XOR) {
      const uint4 d[4] = {p[0], p[1], p[2], p[3]};
      dpf_aes::mmo_hashN<4>(s, lk, rk);
#pragma unroll
      for (int i = 0; i < 4; ++i) add(correct(s[i], t[i]), d[i]);
    } else {
      // uint64_t: the 16 VGPRs of loads in flight across the ILP4 hashes do
      // not fit beside the 64-bit products (21-24 spilled VGPRs), so the
      // loads follow the hashes; the workgroup's other waves cover them.
      dpf_aes::mmo_hashN<4>(s, lk, rk);
      asm volatile("" ::: "memory");
#pragma unroll
      for (int i = 0; i < 4; ++i) add(correct(s[i], t[i]), p[i]);
    }
  }

  // Kernel end (every thread of the workgroup, after its last item): the
  // lanes' sums across the wave by cross-lane moves, the waves' through LDS,
  // and one partial per workgroup by a plain store.  Waves and workgroups
  // that took no item contribute zero.
  __device__ __forceinline__ void finish() const {
    __shared__ uint64_t red[2 * (kBlock / 64)];
    uint64_t x0 = a0, x1 = a1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t y0 = __shfl_xor(x0, off, 64), y1 = __shfl_xor(x1, off, 64);
      x0 = XOR ? x0 ^ y0 : x0 + y0;
      x1 = XOR ? x1 ^ y1 : x1 + y1;
    }
    const int wave = (int)(threadIdx.x >> 6), waves = (int)(blockDim.x >> 6);
    if ((threadIdx.x & 63) == 0) {
      red[2 * wave] = x0;
      red[2 * wave + 1] = x1;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < waves; ++w) {
      x0 = XOR ? x0 ^ red[2 * w] : x0 + red[2 * w];
      x1 = XOR ? x1 ^ red[2 * w + 1] : x1 + red[2 * w + 1];
    }
    if (blockIdx.x == 0) *reinterpret_cast<uint32_t*>(workspace) = gridDim.x;
    uint64_t* part = reinterpret_cast<uint64_t*>(workspace + kDotHeaderBytes);
    if (BITS == 128) {
      part[2 * (int64_t)blockIdx.x] = x0;
      part[2 * (int64_t)blockIdx.x + 1] = x1;
    } else {
      part[blockIdx.x] = XOR ? x0 ^ x1 : x0 + x1;
    }
  }
};

// Leaf policies whose sums outlive the items: combined by finish() at the
// end of the expand kernels (nothing for every other policy).
template <class Leaf> struct HasFinish : std::false_type {};
template <int BITS, bool XOR> struct HasFinish<DotLeaf<BITS, XOR>> : std::true_type {};

}  // namespace
