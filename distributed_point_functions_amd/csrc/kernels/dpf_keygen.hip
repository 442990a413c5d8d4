// dpf_keygen.hip -- batched DPF key generation on gfx950 (GenerateKeysIncremental,
// distributed_point_function.cc:103-204, 619-687, for many alphas at once),
// written straight into the KeyBatch layout (include/dpf/key_batch.h).
//
// One lane PAIR per key pair: the even lane holds party 0's (seed, t), the odd
// lane party 1's.  Per tree level each lane hashes both children of its own
// seed (children_step, 2 AES), the two lanes swap what the correction word
// needs (one DPP quad_perm per word), and both keep the child on alpha's path.
// At a tree level that carries a hierarchy level each lane hashes its seed
// under the value key and the pair forms the value correction
// (ComputeValueCorrectionFor, value_type_helpers.h:597-631) in the lanes of the
// hashed block.  Value types: one integer or XorWrapper leaf of 8..128 bits,
// converted directly (what FastIntLeaf covers); everything else is generated on
// the host (dpf_hip_gen_keys_supported).
//
// Stores: the batch is key-major, so neighbouring lanes are 16 L bytes apart.
// The even lane keeps four levels of correction seeds and writes 64 contiguous
// bytes; the odd lane writes the four levels' control bytes as one dword per
// array and the value corrections.
// Built with the iterative-ilp scheduler (build_native.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../../include/dpf_hip.h"
#include "dpf_device.h"
#include "dpf_runtime.h"

using namespace dpf_rt;

namespace {

constexpr int kKgMaxLevels = 128;   // hierarchy levels, and correction words per key

struct KeygenLevels {
  int H;
  uint8_t tree_level[kKgMaxLevels];   // hierarchy_to_tree
  uint8_t log_domain[kKgMaxLevels];
  uint8_t bits[kKgMaxLevels];         // leaf width: 8, 16, 32, 64 or 128
  uint8_t xr[kKgMaxLevels];           // XorWrapper
  dpf_block* vc[kKgMaxLevels];        // [key][128 / bits] value corrections
};

struct KeygenParams {
  int64_t num_keys;
  int L;             // correction words per key
  int last_log;      // log domain size of the last hierarchy level
  int beta_mode;     // 0: beta[h]; 1: beta[key][h]; 2: DCF, beta[key]
  int dcf_bits;
  const dpf_block* alphas;
  const dpf_block* root_seeds;   // [key][party]
  const dpf_block* beta;
  dpf_block* cw_seed;
  uint8_t* cw_left;
  uint8_t* cw_right;
  RoundKeys rkl, rkr, rkv;
  int64_t dyn_per_wg;   // ItemLoop's per_wg (0: grid stride)
};

// The other lane of the pair's value (quad_perm [1, 0, 3, 2]); both lanes of a
// pair are always active together.
__device__ __forceinline__ uint32_t pair_swap(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 1 | 0 << 2 | 3 << 4 | 2 << 6, 0xf, 0xf, false);
}
__device__ __forceinline__ Block4 pair_swap(Block4 b) {
  return Block4{pair_swap(b.w0), pair_swap(b.w1), pair_swap(b.w2), pair_swap(b.w3)};
}
__device__ __forceinline__ Block4 xor_blocks(Block4 a, Block4 b) {
  return Block4{a.w0 ^ b.w0, a.w1 ^ b.w1, a.w2 ^ b.w2, a.w3 ^ b.w3};
}
__device__ __forceinline__ Block4 select_block(uint32_t take_b, Block4 a, Block4 b) {
  return take_b ? b : a;
}
__device__ __forceinline__ Block4 u128_block(u128 x) {
  return Block4{(uint32_t)x, (uint32_t)(x >> 32), (uint32_t)(x >> 64), (uint32_t)(x >> 96)};
}
__device__ __forceinline__ u128 shr_or_zero(u128 x, int s) { return s >= 128 ? (u128)0 : x >> s; }

// c + beta - a in the block's lanes of BITS, negated for `invert`
// (value_type_helpers.h:597-631 on a directly converted block).
template <int BITS>
__device__ __forceinline__ Block4 correction_lanes(Block4 a, Block4 c, Block4 beta, uint32_t invert) {
  const Block4 v = lanes_add<BITS>(lanes_add<BITS>(c, beta), lanes_neg<BITS>(a));
  return invert ? lanes_neg<BITS>(v) : v;
}

// Four one-byte control bits at p: one dword store where p is aligned.
__device__ __forceinline__ void store_ctrl(uint8_t* p, uint32_t packed, int count) {
  if (count == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p) = packed;
  } else {
    for (int i = 0; i < count; ++i) p[i] = (uint8_t)(packed >> (8 * i));
  }
}

__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void keygen_kernel(KeygenParams p,
                                                                       KeygenLevels lv) {
  __shared__ LdsImage lds;
  __shared__ int next_chunk;   // ItemLoop (dpf_device.h)
  fill_tables(lds.tab);
  if (threadIdx.x == 0) next_chunk = 0;
  __syncthreads();
  const LdsLookup lk =
      make_lookup(lds, KeySet{key_ref(p.rkl), key_ref(p.rkr), key_ref(p.rkv), KeyRef{}});
  const int L = p.L, H = lv.H;
  const int64_t num_items = 2 * p.num_keys;   // lanes; a chunk is one wave's 32 key pairs
  const ItemLoop items{&next_chunk, p.dyn_per_wg, (num_items + 63) / 64, num_items};
  for (int64_t u = items.first(); u < num_items; u = items.next(u)) {
    const int64_t k = u >> 1;
    const uint32_t party = (uint32_t)(u & 1);
    const u128 alpha_in = dpf_u128(p.alphas[k]);
    const u128 alpha = p.beta_mode == 2 ? alpha_in >> 1 : alpha_in;   // the DPF's alpha
    Block4 s = load_block(p.root_seeds + u);
    uint32_t t = party;
    // Correction seeds of up to four levels (oldest first) and their control bits.
    Block4 q0{}, q1{}, q2{}, q3{};
    uint32_t left4 = 0, right4 = 0;
    int h = 0;
    for (int d = 0;; ++d) {
      if (h < H && lv.tree_level[h] == d) {
        // Value correction of hierarchy level h from the seeds at tree level d.
        const int bits = lv.bits[h];
        const int logd = lv.log_domain[h];
        const u128 prefix = shr_or_zero(alpha, p.last_log - logd);
        const int idx = (int)((uint32_t)prefix & ((1u << (logd - d)) - 1u));
        u128 beta;
        if (p.beta_mode == 0) {
          beta = dpf_u128(p.beta[h]);
        } else if (p.beta_mode == 1) {
          beta = dpf_u128(p.beta[k * H + h]);
        } else {
          // DCF (distributed_comparison_function.cc:79-101): beta where bit
          // n-1-h of alpha is set, else zero -- except that SetToZero leaves
          // an XorWrapper as it is.
          const uint32_t bit = (uint32_t)(alpha_in >> (p.dcf_bits - 1 - h)) & 1u;
          beta = (bit || lv.xr[h]) ? dpf_u128(p.beta[k]) : (u128)0;
        }
        if (bits < 128) beta = (beta & (((u128)1 << (bits & 127)) - 1)) << ((idx * bits) & 127);
        const Block4 mine = dpf_aes::mmo_hash(s, lk, UniformRK{lk.ks.v});
        const Block4 other = pair_swap(mine);
        if (party) {
          // `invert` is party 1's control bit: this lane's t.
          const Block4 a = other, c = mine, b = u128_block(beta);
          Block4 v;
          if (lv.xr[h]) {
            v = xor_blocks(xor_blocks(a, b), c);
          } else {
            switch (bits) {
              case 8: v = correction_lanes<8>(a, c, b, t); break;
              case 16: v = correction_lanes<16>(a, c, b, t); break;
              case 32: v = correction_lanes<32>(a, c, b, t); break;
              case 64: v = correction_lanes<64>(a, c, b, t); break;
              default: v = correction_lanes<128>(a, c, b, t); break;
            }
          }
          const int E = 128 / bits;
          dpf_block* o = lv.vc[h] + k * E;
          if (bits == 128) {
            store_block(o, v);
          } else {
            const u128 x = block_u128(v), m = ((u128)1 << (bits & 127)) - 1;
            for (int e = 0; e < E; ++e) store_block(o + e, u128_block((x >> (e * bits)) & m));
          }
        }
        ++h;
      }
      if (d == L) break;
      // GenerateNextCore (distributed_point_function.cc:138-201) for tree level d + 1.
      Block4 c0, c1;
      uint32_t t0, tr;
      children_step(lk, lk.ks.l, lk.ks.r, s, 0u, make_uint4(0, 0, 0, 0), 0u, c0, t0, c1, tr);
      const int shift = p.last_log - (d + 1);
      const uint32_t bit = shift < 128 ? (uint32_t)(alpha >> shift) & 1u : 0u;
      const Block4 lose = select_block(bit, c1, c0);
      const Block4 sc = xor_blocks(lose, pair_swap(lose));
      const uint32_t ccw_l = t0 ^ pair_swap(t0) ^ bit ^ 1u;
      const uint32_t ccw_r = tr ^ pair_swap(tr) ^ bit;
      const Block4 keep = select_block(bit, c0, c1);
      const uint32_t m = 0u - t;
      s = Block4{keep.w0 ^ (sc.w0 & m), keep.w1 ^ (sc.w1 & m), keep.w2 ^ (sc.w2 & m),
                 keep.w3 ^ (sc.w3 & m)};
      t = (bit ? tr : t0) ^ (t & (bit ? ccw_r : ccw_l));
      q0 = q1; q1 = q2; q2 = q3; q3 = sc;
      left4 = (left4 >> 8) | (ccw_l << 24);
      right4 = (right4 >> 8) | (ccw_r << 24);
      const int filled = (d & 3) + 1;
      if (filled == 4 || d == L - 1) {
        // Levels d - filled + 1 .. d: the even lane writes the seeds, the odd
        // lane the control bytes.
        const int64_t first = k * L + (d - filled + 1);
        if (party == 0) {
          dpf_block* o = p.cw_seed + first;
          if (filled == 4) {
            store_block(o, q0); store_block(o + 1, q1); store_block(o + 2, q2); store_block(o + 3, q3);
          } else if (filled == 3) {
            store_block(o, q1); store_block(o + 1, q2); store_block(o + 2, q3);
          } else if (filled == 2) {
            store_block(o, q2); store_block(o + 1, q3);
          } else {
            store_block(o, q3);
          }
        } else {
          const int drop = 8 * (4 - filled);
          store_ctrl(p.cw_left + first, left4 >> drop, filled);
          store_ctrl(p.cw_right + first, right4 >> drop, filled);
        }
      }
    }
  }
}

// One integer or XorWrapper leaf converted directly from one hashed block.
bool keygen_type(const dpf_value_desc* d) {
  if (!d || d->num_leaves != 1 || !d->direct || d->blocks_needed != 1) return false;
  if (d->kind[0] != DPF_LEAF_INT && d->kind[0] != DPF_LEAF_XOR) return false;
  const int b = d->bits[0];
  if (b != 8 && b != 16 && b != 32 && b != 64 && b != 128) return false;
  return d->elements_per_block == 128 / b;
}

}  // namespace

extern "C" {

int dpf_hip_gen_keys_supported(const dpf_value_desc* desc) { return keygen_type(desc) ? 1 : 0; }

int dpf_hip_gen_key_batch(int64_t num_keys, int num_levels, int num_hierarchy_levels,
                          const int32_t* tree_level, const int32_t* log_domain,
                          const int32_t* blocks, const dpf_value_desc* desc,
                          const dpf_block* alphas, const dpf_block* root_seeds,
                          const dpf_block* beta, int beta_mode, int dcf_bits,
                          const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                          const dpf_aes_key* key_value, dpf_block* cw_seed, uint8_t* cw_left,
                          uint8_t* cw_right, dpf_block* const* value_correction, void* stream) {
  const int L = num_levels, H = num_hierarchy_levels;
  if (num_keys < 0 || L < 0 || H < 1) return fail(kInvalidArgument, "negative count");
  if (beta_mode < 0 || beta_mode > 2) return fail(kInvalidArgument, "beta_mode must be 0, 1 or 2");
  if (num_keys == 0) return kOk;
  if (!tree_level || !log_domain || !blocks || !desc)
    return fail(kInvalidArgument, "NULL level table");
  for (int h = 0; h < H; ++h)
    if (!keygen_type(&desc[h]) || blocks[h] != 1)
      return fail(kUnimplemented, "gen_key_batch: value type is not a single integer or XorWrapper leaf");
  if (L > kKgMaxLevels || H > kKgMaxLevels)
    return fail(kUnimplemented, "gen_key_batch: more than 128 levels");
  if (beta_mode == 2 && (dcf_bits != H || dcf_bits > 128))
    return fail(kInvalidArgument, "dcf_bits must be the number of hierarchy levels");
  KeygenLevels lv;
  memset(&lv, 0, sizeof(lv));
  lv.H = H;
  for (int h = 0; h < H; ++h) {
    const int tl = tree_level[h], ld = log_domain[h];
    // One hierarchy level per tree level, the last one at the leaves, and the
    // block index within the level's elements per block.
    if (tl < 0 || tl > L || (h > 0 && tl <= tree_level[h - 1]) || (h == H - 1 && tl != L) ||
        ld < tl || ld > 128 || ld - tl > 7 || (1 << (ld - tl)) > desc[h].elements_per_block ||
        (h > 0 && ld < log_domain[h - 1]))
      return fail(kInvalidArgument, "level tables are not a DPF hierarchy");
    lv.tree_level[h] = (uint8_t)tl;
    lv.log_domain[h] = (uint8_t)ld;
    lv.bits[h] = (uint8_t)desc[h].bits[0];
    lv.xr[h] = desc[h].kind[0] == DPF_LEAF_XOR;
  }
  if (!alphas || !root_seeds || !beta || !key_left || !key_right || !key_value ||
      !value_correction || (L > 0 && (!cw_seed || !cw_left || !cw_right)))
    return fail(kInvalidArgument, "NULL pointer");
  for (int h = 0; h < H; ++h) {
    if (!value_correction[h]) return fail(kInvalidArgument, "NULL value correction");
    lv.vc[h] = value_correction[h];
  }
  KeygenParams p;
  memset(&p, 0, sizeof(p));
  p.num_keys = num_keys;
  p.L = L;
  p.last_log = log_domain[H - 1];
  p.beta_mode = beta_mode;
  p.dcf_bits = dcf_bits;
  p.alphas = alphas;
  p.root_seeds = root_seeds;
  p.beta = beta;
  p.cw_seed = cw_seed;
  p.cw_left = cw_left;
  p.cw_right = cw_right;
  p.rkl = expand_key(key_left);
  p.rkr = expand_key(key_right);
  p.rkv = expand_key(key_value);
  const LaunchShape sh = chunked_shape(2 * num_keys, "DPF_KEYGEN_DYNAMIC");
  p.dyn_per_wg = sh.dyn_per_wg;
  hipLaunchKernelGGL(keygen_kernel, dim3(sh.grid), dim3(sh.block), 0, (hipStream_t)stream, p, lv);
  HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
