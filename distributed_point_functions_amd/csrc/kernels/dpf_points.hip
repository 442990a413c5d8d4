// dpf_points.hip -- batched point evaluation (EvaluateAt) on gfx950: one
// path walk per (key, point), fused with the leaf hash, conversion, correction
// and the store (or the sum over keys) of the selected element.
//   * eval_points_kernel: two chains per lane (ILP2), any value type; one
//     chain per lane for launches below a wave per CU.
//   * eval_points4_kernel: four chains per lane (ILP4), integer leaves.
//   * eval_points_quad_kernel: one chain per lane quad, small calls.
// launch_points_t picks among them; the C ABI entry points are at the end.
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


// Batched point evaluation (row a11).  Work item u covers
// key k and the point PAIR (q, q + half) of that key, hashed as two
// interleaved chains (ILP2).  With UNIFORM, half % 64 == 0, so all 64 lanes of
// a wave share k: `k` is made wave-uniform and the key's correction words come
// through scalar loads.  In sum mode (SUM) item u covers the pair for a chunk
// of `chunk_keys` consecutive keys and accumulates the shares in the value
// type's group before one wide atomic add per point.
struct PointParams {
  int64_t num_keys;
  int64_t points_per_key;   // P
  int64_t half;             // ceil(P / 2)
  int64_t num_items;
  int64_t chunk_keys;       // SUM: keys per item
  int shared_points;        // tree_index/block_index indexed by point only
  int num_levels;
  int cw_stride;            // correction words per key row (>= num_levels)
  int bib;                  // block-index bits: tree_index holds raw domain points
                            // (path = point >> bib, element = point & (2^bib - 1))
  const dpf_block* key_seed;
  const uint8_t* party;
  const dpf_block* seeds_in;
  const uint8_t* ctrl_in;
  const dpf_block* tree_index;
  const int32_t* block_index;
  const dpf_block* cw_seed;   // [key][level]
  const uint8_t* cw_left;
  const uint8_t* cw_right;
  const dpf_block* vcw;       // [key][E * num_leaves]
  int vcw_stride;             // E * num_leaves
  char* out;
  unsigned long long* wide;   // SUM: [point][leaf][3] 192-bit exact sums
  int esz;
  int xor_mode;               // fast leaves: XorWrapper
  RoundKeys rkl, rkd, rkv;
  int64_t dyn_per_wg;         // ItemLoop's per_wg (0: grid stride)
  int top_levels;             // nonzero: eval_points4_kernel's TOP instance (6 / 4 levels walked once per wave)
};

// PAIRED = false (launches below one wave per CU, never in sum mode): one
// chain per lane, half = P, so a small call spreads over twice the CUs and each
// wave's dependent AES chain issues half the LDS reads per round.
template <class Leaf, int BITS, bool FAST, bool UNIFORM, bool SUM, bool PAIRED = true>
__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void eval_points_kernel(PointParams p, Leaf leaf) {
  __shared__ LdsImage lds;
  __shared__ int next_chunk;   // ItemLoop (dpf_device.h)
  fill_tables(lds.tab);
  if (threadIdx.x == 0) next_chunk = 0;
  __syncthreads();
  const LdsLookup lk = make_lookup(lds, KeySet{key_ref(p.rkl), KeyRef{}, key_ref(p.rkv), key_ref(p.rkd)});
  const int L = p.num_levels;
  const int64_t P = p.points_per_key, half = p.half;
  const ItemLoop items{&next_chunk, p.dyn_per_wg, (p.num_items + 63) / 64, p.num_items};
  for (int64_t u = items.first(); u < p.num_items; u = items.next(u)) {
    int64_t grp = u / half;
    if (UNIFORM) grp = (int64_t)__builtin_amdgcn_readfirstlane((int)grp);
    const int64_t q0 = u - grp * half;
    const int64_t q1raw = q0 + half;
    const bool has1 = q1raw < P;
    const int64_t q1 = has1 ? q1raw : q0;
    int64_t k_begin = grp, k_end = grp + 1;
    if (SUM) {
      k_begin = grp * p.chunk_keys;
      k_end = k_begin + p.chunk_keys < p.num_keys ? k_begin + p.chunk_keys : p.num_keys;
    }
    // Points are shared by all keys (sum mode always) or per key.
    const int64_t pi0 = p.shared_points ? q0 : grp * P + q0;
    const int64_t pi1 = p.shared_points ? q1 : grp * P + q1;
    const Block4 path0 = load_block(p.tree_index + pi0);
    const Block4 path1 = load_block(p.tree_index + pi1);
    const int bb = p.bib;
    const uint32_t bmask = (1u << bb) - 1u;
    const int bi0 = p.block_index ? p.block_index[pi0] : (int)(path0.w0 & bmask);
    const int bi1 = p.block_index ? p.block_index[pi1] : (int)(path1.w0 & bmask);
    u128 acc0[FAST ? 1 : DPF_MAX_LEAVES], acc1[FAST ? 1 : DPF_MAX_LEAVES];
    const int nl = FAST ? 1 : leaf.d.num_leaves;
    for (int k = 0; k < nl; ++k) { acc0[k] = 0; acc1[k] = 0; }
    for (int64_t k = k_begin; k < k_end; ++k) {
      const int party = p.party[k] & 1;
      Block4 s0, s1;
      uint32_t t0, t1;
      if (p.seeds_in) {
        const int64_t o0 = k * P + q0, o1 = k * P + q1;
        s0 = load_block(p.seeds_in + o0);
        t0 = p.ctrl_in[o0] & 1u;
        s1 = load_block(p.seeds_in + o1);
        t1 = p.ctrl_in[o1] & 1u;
      } else {
        s0 = s1 = load_block(p.key_seed + k);
        t0 = t1 = (uint32_t)party;
      }
      const dpf_block* cws = p.cw_seed + k * p.cw_stride;
      const uint8_t* cl = p.cw_left + k * p.cw_stride;
      const uint8_t* cr = p.cw_right + k * p.cw_stride;
      for (int j = 0; j < L; ++j) {
        const uint32_t b0 = path_bit(path0, L - 1 - j + bb), b1 = path_bit(path1, L - 1 - j + bb);
        const uint4 cs = cw_u4(cws[j]);
        const uint32_t cctl = cw_ctrl2(cl, cr, j);
        if constexpr (PAIRED)
          path_step2(lk, lk.ks.l, lk.ks.d, s0, t0, b0, s1, t1, b1, cs, cctl);
        else
          path_step(lk, lk.ks.l, lk.ks.d, s0, t0, b0, cs, cctl);
      }
      const dpf_block* vcw = p.vcw + k * p.vcw_stride;
      if constexpr (FAST) {
        Block4 h0 = s0, h1 = s1;
        if constexpr (PAIRED)
          dpf_aes::mmo_hash2(h0, h1, lk, UniformRK{lk.ks.v}, UniformRK{lk.ks.v});
        else
          h0 = dpf_aes::mmo_hash(h0, lk, UniformRK{lk.ks.v});
        const u128 v0 = fast_point_value<BITS>(h0, t0, bi0, dpf_u128(vcw[bi0]), party, p.xor_mode);
        const u128 v1 =
            PAIRED ? fast_point_value<BITS>(h1, t1, bi1, dpf_u128(vcw[bi1]), party, p.xor_mode) : v0;
        if (SUM) {
          acc0[0] = p.xor_mode ? (acc0[0] ^ v0) : (acc0[0] + v0);
          acc1[0] = p.xor_mode ? (acc1[0] ^ v1) : (acc1[0] + v1);
        } else {
          store_bits<BITS>(p.out + (k * P + q0) * (int64_t)p.esz, v0);
          if (has1) store_bits<BITS>(p.out + (k * P + q1) * (int64_t)p.esz, v1);
        }
      } else {
        if (SUM) {
          u128 v[DPF_MAX_LEAVES];
          generic_point_values(leaf, lk, lk.ks.v, s0, t0, bi0, vcw, party, v);
          for (int e = 0; e < nl; ++e) acc0[e] = leaf_group_add(leaf.d, e, acc0[e], v[e]);
          generic_point_values(leaf, lk, lk.ks.v, s1, t1, bi1, vcw, party, v);
          for (int e = 0; e < nl; ++e) acc1[e] = leaf_group_add(leaf.d, e, acc1[e], v[e]);
        } else {
          GenericLeaf lf = leaf;
          lf.vcw = vcw;
          lf.party = party;
          lf.convert_store(lk, lk.ks.v, s0, t0, bi0, 1, p.out + (k * P + q0) * (int64_t)p.esz);
          if (has1)
            lf.convert_store(lk, lk.ks.v, s1, t1, bi1, 1, p.out + (k * P + q1) * (int64_t)p.esz);
        }
      }
    }
    if (SUM && k_begin < k_end) {
      for (int e = 0; e < nl; ++e) {
        const bool x = FAST ? p.xor_mode != 0 : leaf.d.kind[e] == DPF_LEAF_XOR;
        unsigned long long* w0 = p.wide + (q0 * nl + e) * 3;
        if (x) wide_xor(w0, acc0[e]); else wide_add(w0, acc0[e]);
        if (has1) {
          unsigned long long* w1 = p.wide + (q1 * nl + e) * 3;
          if (x) wide_xor(w1, acc1[e]); else wide_add(w1, acc1[e]);
        }
      }
    }
  }
}

// Integer leaves, four path chains per lane (ILP4): item u covers key grp and
// the points q + j * quarter, j < 4 (p.half holds the quarter).  Same
// arithmetic as eval_points_kernel<GenericLeaf, BITS, true, ...>, one more
// pair of chains in flight per wave (points_ilp below picks it).
template <int BITS, bool UNIFORM, bool SUM, bool TOP>
__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void eval_points4_kernel(PointParams p) {
  __shared__ LdsImage lds;
  __shared__ int next_chunk;   // ItemLoop (dpf_device.h)
  fill_tables(lds.tab);
  if (threadIdx.x == 0) next_chunk = 0;
  __syncthreads();
  const LdsLookup lk = make_lookup(lds, KeySet{key_ref(p.rkl), KeyRef{}, key_ref(p.rkv), key_ref(p.rkd)});
  const int L = p.num_levels;
  const int64_t P = p.points_per_key, quarter = p.half;
  // Sums of <= 64-bit values wrap mod 2^64 exactly (the group is mod 2^BITS).
  using Acc = typename std::conditional<(BITS <= 64), uint64_t, u128>::type;
  const ItemLoop items{&next_chunk, p.dyn_per_wg, (p.num_items + 63) / 64, p.num_items};
  for (int64_t u = items.first(); u < p.num_items; u = items.next(u)) {
    int64_t grp = u / quarter;
    if (UNIFORM) grp = (int64_t)__builtin_amdgcn_readfirstlane((int)grp);
    const int64_t q0 = u - grp * quarter;
    // Point i of the item: q0 + i * quarter (clamped to q0 past the key's last point).
    auto qi = [&](int i) { return q0 + i * quarter < P ? q0 + i * quarter : q0; };
    auto pidx = [&](int i) { return p.shared_points ? qi(i) : grp * P + qi(i); };
    int64_t k_begin = grp, k_end = grp + 1;
    if (SUM) {
      k_begin = grp * p.chunk_keys;
      k_end = k_begin + p.chunk_keys < p.num_keys ? k_begin + p.chunk_keys : p.num_keys;
    }
    Block4 path[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) path[i] = load_block(p.tree_index + pidx(i));
    Acc acc[4] = {0, 0, 0, 0};
    for (int64_t k = k_begin; k < k_end; ++k) {
      const int party = p.party[k] & 1;
      Block4 st[4];
      uint32_t t[4];
      if (p.seeds_in) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          st[i] = load_block(p.seeds_in + k * P + qi(i));
          t[i] = p.ctrl_in[k * P + qi(i)] & 1u;
        }
      } else {
        const Block4 root = load_block(p.key_seed + k);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          st[i] = root;
          t[i] = (uint32_t)party;
        }
      }
      const dpf_block* cws = p.cw_seed + k * p.cw_stride;
      const uint8_t* cl = p.cw_left + k * p.cw_stride;
      const uint8_t* cr = p.cw_right + k * p.cw_stride;
      // Shared top (top_levels = 6, walks from the root): the wave's 256
      // points of this key share its top 6 levels, so lane l walks them once
      // for the prefix whose 6 path bits are l (one AES per level instead of
      // four), and each chain takes its depth-6 node from the lane its own
      // top bits name (ds_bpermute, no LDS allocation).
      // 6 levels in the key sum; 4 per key, whose instance schedules its path
      // loop as the full walk does only with the shorter top (ISA: 9 waits in
      // the round block vs 40 with 6 levels).
      constexpr int j0 = TOP ? (SUM ? 6 : 4) : 0;
      if (TOP) {
        const uint32_t lane = threadIdx.x & 63;
        Block4 ts = st[0];
        uint32_t tt = t[0];
        for (int j = 0; j < j0; ++j) {
          const uint4 cs = cw_u4(cws[j]);
          const uint32_t b = (lane >> (j0 - 1 - j)) & 1u;
          Block4 h = dpf_aes::mmo_hash(ts, lk, SelectRK{lk.ks.l, lk.ks.d, 0u - b});
          correct_child(h, tt, b, cs, cw_ctrl2(cl, cr, j));
          ts = h;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          uint32_t src = 0;
          for (int j = 0; j < j0; ++j) src = (src << 1) | path_bit(path[i], L - 1 - j + p.bib);
          const int a = (int)(src << 2);
          st[i] = Block4{(uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)ts.w0),
                         (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)ts.w1),
                         (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)ts.w2),
                         (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)ts.w3)};
          t[i] = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)tt);
        }
      }
      for (int j = j0; j < L; ++j) {
        const uint4 cs = cw_u4(cws[j]);
        const uint32_t cctl = cw_ctrl2(cl, cr, j);
        uint32_t b[4];
        SelectRK rk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          b[i] = path_bit(path[i], L - 1 - j + p.bib);
          rk[i] = SelectRK{lk.ks.l, lk.ks.d, 0u - b[i]};
        }
        Block4 h[4] = {st[0], st[1], st[2], st[3]};
        dpf_aes::mmo_hashN<4>(h, lk, rk);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          correct_child(h[i], t[i], b[i], cs, cctl);
          st[i] = h[i];
        }
      }
      const dpf_block* vcw = p.vcw + k * p.vcw_stride;
      const UniformRK vk[4] = {UniformRK{lk.ks.v}, UniformRK{lk.ks.v}, UniformRK{lk.ks.v},
                               UniformRK{lk.ks.v}};
      dpf_aes::mmo_hashN<4>(st, lk, vk);
      const uint32_t bmask = (1u << p.bib) - 1u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int bi = p.block_index ? p.block_index[pidx(i)] : (int)(path[i].w0 & bmask);
        const u128 v = fast_point_value<BITS>(st[i], t[i], bi, dpf_u128(vcw[bi]), party, p.xor_mode);
        if (SUM)
          acc[i] = p.xor_mode ? (acc[i] ^ (Acc)v) : (acc[i] + (Acc)v);
        else if (q0 + i * quarter < P)
          store_bits<BITS>(p.out + (k * P + qi(i)) * (int64_t)p.esz, v);
      }
    }
    if (SUM && k_begin < k_end) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (q0 + i * quarter >= P) continue;
        unsigned long long* w = p.wide + qi(i) * 3;
        if (p.xor_mode) wide_xor(w, (u128)acc[i]); else wide_add(w, (u128)acc[i]);
      }
    }
  }
}

// Latency mode of eval_points_kernel<GenericLeaf, BITS, true, ..> for small
// calls (no sum): one (key, point) per lane QUAD, lane c computing column c
// of every AES (dpf_device.h quad::), so one path walk runs ~2x faster than
// on one lane when the launch is far below a wave per SIMD.
template <int BITS>
__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void eval_points_quad_kernel(PointParams p) {
  __shared__ LdsImage lds;
  fill_tables(lds.tab);
  __syncthreads();
  const LdsLookup lk = make_lookup(lds);
  const quad::Keys kl = quad::keys_of(p.rkl), kd = quad::keys_of(p.rkd), kv = quad::keys_of(p.rkv);
  const int L = p.num_levels;
  const int64_t P = p.points_per_key;
  const int c = quad::column();
  const uint32_t bmask = (1u << p.bib) - 1u;
  // The stride is a multiple of 64, so the four lanes of a quad stay together.
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; (g >> 2) < p.num_items;
       g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u = g >> 2;  // item = key k, point q
    const int64_t k = u / P, q = u - k * P;
    const int64_t pi = p.shared_points ? q : u;
    const Block4 path = load_block(p.tree_index + pi);
    const int bi = p.block_index ? p.block_index[pi] : (int)(path.w0 & bmask);
    const int party = p.party[k] & 1;
    uint32_t s, t;
    if (p.seeds_in) {
      s = reinterpret_cast<const uint32_t*>(p.seeds_in + u)[c];
      t = p.ctrl_in[u] & 1u;
    } else {
      s = reinterpret_cast<const uint32_t*>(p.key_seed + k)[c];
      t = (uint32_t)party;
    }
    const dpf_block* cws = p.cw_seed + k * p.cw_stride;
    const uint8_t* cl = p.cw_left + k * p.cw_stride;
    const uint8_t* cr = p.cw_right + k * p.cw_stride;
    for (int j = 0; j < L; ++j) {
      const uint32_t bit = path_bit(path, L - 1 - j + p.bib);
      const uint32_t cs = reinterpret_cast<const uint32_t*>(cws + j)[c];
      quad::path_step(lk, kl, kd, s, t, bit, cs, cw_ctrl2(cl, cr, j));
    }
    const Block4 h = quad::gather(quad::mmo(s, lk, kv, kv, 0u));
    if (c == 0) {
      const dpf_block* vcw = p.vcw + k * p.vcw_stride;
      store_bits<BITS>(p.out + u * (int64_t)p.esz,
                       fast_point_value<BITS>(h, t, bi, dpf_u128(vcw[bi]), party, p.xor_mode));
    }
  }
}

// DPF_POINTS_QUAD=0 (read per launch) turns the latency mode off (A/B hook).
bool points_quad_on() { return !hook_is("DPF_POINTS_QUAD", '0'); }
// Launches of at most this many points run in latency mode: num_cus x 256 by
// default, i.e. as many lane quads as one pass of 1024-thread workgroups on
// every CU holds.  BatchEvaluation/10/40000 (40000 points per call) 2.54-2.63
// -> 1.46-1.58 ms; /1/400000 stays on the lane chains (the quads would loop:
// 1.01-1.17 vs 0.97-1.00 ms); profiles/r15_ab.txt part 19.
// DPF_POINTS_QUAD_MAX=<points> (read per launch) moves the cut-over (A/B hook).
int64_t points_quad_max() {
  const long long m = hook_long("DPF_POINTS_QUAD_MAX", 0);
  return m > 0 ? (int64_t)m : (int64_t)num_cus() * 256;
}

// DPF_POINTS_ILP=2|4 (read per launch) forces two or four chains per lane
// (four only where a quarter of a key's points is a whole number of waves);
// by default integer leaves take four chains when the launch fills every CU
// with 1024-thread workgroups (config 4: +0.7% per key, +1.4% summed over
// keys, profiles/r14_ab.txt) and two otherwise.
int points_ilp() {
  return hook_is("DPF_POINTS_ILP", '2') ? 2 : hook_is("DPF_POINTS_ILP", '4') ? 4 : 0;
}
thread_local const char* g_last_points_kernel = "";

template <class Leaf, int BITS, bool FAST, bool SUM>
int launch_points_t(const PointParams& pp, const Leaf& leaf, hipStream_t s) {
  if constexpr (FAST) {
    // ILP4: quarter = ceil(P / 4) points per chain row; enough items to fill the chip.
    const int64_t quarter = (pp.points_per_key + 3) / 4;
    const int64_t items = SUM ? pp.num_items / pp.half * quarter : pp.num_keys * quarter;
    const int ilp = points_ilp();
    if (quarter % 64 == 0 &&
        (ilp == 4 || (ilp == 0 && items >= (int64_t)num_cus() * 1024))) {
      g_last_points_kernel = "points/ilp4";
      PointParams p = pp;
      p.half = quarter;
      p.num_items = items;
      // DPF_POINTS_DYNAMIC=0: a fixed share of items per thread (A/B hook).
      const LaunchShape sh = chunked_shape(p.num_items, "DPF_POINTS_DYNAMIC");
      const dim3 grid(sh.grid), blk(sh.block);
      p.dyn_per_wg = sh.dyn_per_wg;
      // The shared top (profiles/r16/points_shared_top_ab.txt): summed over
      // keys 6 levels, 1236 vs 1275 ms; per key 4 levels (6 measured 1358 vs
      // 1258 ms, r16h).  DPF_POINTS_SHARED_TOP=0 turns it off (A/B hook).
      const bool want_top = !hook_is("DPF_POINTS_SHARED_TOP", '0');
      p.top_levels = want_top && !p.seeds_in && p.num_levels >= 6 ? 6 : 0;
      if (p.top_levels)
        hipLaunchKernelGGL((eval_points4_kernel<BITS, true, SUM, true>), grid, blk, 0, s, p);
      else
        hipLaunchKernelGGL((eval_points4_kernel<BITS, true, SUM, false>), grid, blk, 0, s, p);
      HIP_TRY(hipGetLastError());
      return kOk;
    }
  }
  if constexpr (!SUM) {
    // Up to one pass of lane quads over every CU: one lane quad per point.
    const int64_t points = pp.num_keys * pp.points_per_key;
    if (FAST && points <= points_quad_max() && points_ilp() == 0 && points_quad_on()) {
      g_last_points_kernel = "points/quad";
      PointParams p = pp;
      p.num_items = points;
      const int blk = block_for(points * 4);
      hipLaunchKernelGGL((eval_points_quad_kernel<BITS>), dim3(grid_for(points * 4, blk)),
                         dim3(blk), 0, s, p);
      HIP_TRY(hipGetLastError());
      return kOk;
    }
    // Fewer paired items than one wave per CU: latency-bound, run unpaired.
    if (pp.num_items < (int64_t)num_cus() * 64 && points_ilp() != 2) {
      g_last_points_kernel = "points/single";
      PointParams p = pp;
      p.half = p.points_per_key;
      p.num_items = p.num_keys * p.points_per_key;
      const int blk = block_for(p.num_items);
      const dim3 grid(grid_for(p.num_items, blk)), block(blk);
      if (p.half % 64 == 0)
        hipLaunchKernelGGL((eval_points_kernel<Leaf, BITS, FAST, true, false, false>), grid, block,
                           0, s, p, leaf);
      else
        hipLaunchKernelGGL((eval_points_kernel<Leaf, BITS, FAST, false, false, false>), grid,
                           block, 0, s, p, leaf);
      HIP_TRY(hipGetLastError());
      return kOk;
    }
  }
  g_last_points_kernel = "points/ilp2";
  PointParams p = pp;
  const LaunchShape sh = chunked_shape(p.num_items, "DPF_POINTS_DYNAMIC");
  const dim3 grid(sh.grid), block(sh.block);
  p.dyn_per_wg = sh.dyn_per_wg;
  if (p.half % 64 == 0)
    hipLaunchKernelGGL((eval_points_kernel<Leaf, BITS, FAST, true, SUM>), grid, block, 0, s, p, leaf);
  else
    hipLaunchKernelGGL((eval_points_kernel<Leaf, BITS, FAST, false, SUM>), grid, block, 0, s, p, leaf);
  HIP_TRY(hipGetLastError());
  return kOk;
}

template <bool SUM>
int launch_points(const PointParams& p, const dpf_value_desc* desc, const dpf_block* vcw,
                  hipStream_t s) {
  if (fast_int(desc))
    return with_bits(desc->bits[0], [&](auto bits) {
      return launch_points_t<GenericLeaf, decltype(bits)::value, true, SUM>(p, GenericLeaf{}, s);
    });
  GenericLeaf g;
  g.d = *desc;
  g.vcw = vcw;
  g.party = 0;
  g.elements_per_leaf = 1;
  g.esz = packed_size(desc);
  return launch_points_t<GenericLeaf, 8, false, SUM>(p, g, s);
}

// Shared argument checks and parameter block of the two point entry points.
int make_point_params(int64_t num_keys, int64_t points_per_key, int num_levels,
                      const dpf_block* key_seed, const uint8_t* party, const dpf_block* seeds_in,
                      const uint8_t* control_in, const dpf_block* tree_index,
                      const int32_t* block_index, const dpf_block* cw_seed,
                      const uint8_t* cw_left, const uint8_t* cw_right,
                      const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                      const dpf_aes_key* key_value, const dpf_value_desc* desc,
                      const dpf_block* value_correction, PointParams* p) {
  int st = validate_desc(desc);
  if (st) return st;
  if (num_keys < 0 || points_per_key < 1 || num_levels < 0 || num_levels > 128)
    return fail(kInvalidArgument, "num_keys, points_per_key or num_levels out of range");
  if (!party || !tree_index || !key_left || !key_right || !key_value || !value_correction ||
      (!seeds_in && !key_seed) || (seeds_in && !control_in) ||
      (num_levels > 0 && (!cw_seed || !cw_left || !cw_right)))
    return fail(kInvalidArgument, "NULL pointer");
  memset(p, 0, sizeof(*p));
  p->num_keys = num_keys;
  p->points_per_key = points_per_key;
  p->half = (points_per_key + 1) / 2;
  p->num_levels = num_levels;
  p->cw_stride = num_levels;
  p->key_seed = key_seed;
  p->party = party;
  p->seeds_in = seeds_in;
  p->ctrl_in = control_in;
  p->tree_index = tree_index;
  p->block_index = block_index;
  p->cw_seed = cw_seed;
  p->cw_left = cw_left;
  p->cw_right = cw_right;
  p->vcw = value_correction;
  p->vcw_stride = desc->elements_per_block * desc->num_leaves;
  p->esz = packed_size(desc);
  p->xor_mode = desc->kind[0] == DPF_LEAF_XOR;
  p->dyn_per_wg = 0;
  p->top_levels = 0;
  p->rkl = expand_key(key_left);
  p->rkd = xor_keys(p->rkl, expand_key(key_right));
  p->rkv = expand_key(key_value);
  return kOk;
}

}  // namespace

extern "C" {

const char* dpf_hip_last_points_kernel(void) { return g_last_points_kernel; }

int dpf_hip_eval_points(int64_t num_points, int64_t points_per_key, int num_levels,
                        const dpf_block* key_seed, const uint8_t* party,
                        const dpf_block* seeds_in, const uint8_t* control_in,
                        const dpf_block* tree_index, const int32_t* block_index,
                        const dpf_block* cw_seed, const uint8_t* cw_left, const uint8_t* cw_right,
                        const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                        const dpf_aes_key* key_value, const dpf_value_desc* desc,
                        const dpf_block* value_correction, void* out, void* stream) {
  if (num_points < 0 || points_per_key < 1 || num_points % points_per_key != 0)
    return fail(kInvalidArgument, "num_points must be a non-negative multiple of points_per_key");
  PointParams p;
  int st = make_point_params(num_points / points_per_key, points_per_key, num_levels, key_seed,
                             party, seeds_in, control_in, tree_index, block_index, cw_seed,
                             cw_left, cw_right, key_left, key_right, key_value, desc,
                             value_correction, &p);
  if (st) return st;
  if (num_points == 0) return kOk;
  if (!out) return fail(kInvalidArgument, "NULL pointer");
  p.num_items = p.num_keys * p.half;
  p.out = (char*)out;
  return launch_points<false>(p, desc, value_correction, (hipStream_t)stream);
}

int dpf_hip_eval_points_batch(int64_t num_keys, int64_t points_per_key, int shared_points,
                              int num_levels, int cw_stride, int block_index_bits,
                              const dpf_block* key_seed,
                              const uint8_t* party, const dpf_block* points,
                              const dpf_block* cw_seed, const uint8_t* cw_left,
                              const uint8_t* cw_right, const dpf_aes_key* key_left,
                              const dpf_aes_key* key_right, const dpf_aes_key* key_value,
                              const dpf_value_desc* desc, const dpf_block* value_correction,
                              void* out, void* stream) {
  if (block_index_bits < 0 || block_index_bits > 7 || num_levels + block_index_bits > 128)
    return fail(kInvalidArgument, "block_index_bits out of range");
  PointParams p;
  int st = make_point_params(num_keys, points_per_key, num_levels, key_seed, party, nullptr,
                             nullptr, points, nullptr, cw_seed, cw_left, cw_right, key_left,
                             key_right, key_value, desc, value_correction, &p);
  if (st) return st;
  if (!key_seed) return fail(kInvalidArgument, "NULL pointer");
  if (cw_stride < num_levels) return fail(kInvalidArgument, "cw_stride < num_levels");
  if (num_keys == 0) return kOk;
  if (!out) return fail(kInvalidArgument, "NULL pointer");
  p.cw_stride = cw_stride;
  p.bib = block_index_bits;
  p.shared_points = shared_points ? 1 : 0;
  p.num_items = p.num_keys * p.half;
  p.out = (char*)out;
  return launch_points<false>(p, desc, value_correction, (hipStream_t)stream);
}

int dpf_hip_eval_points_sum(int64_t num_keys, int64_t num_points, int num_levels, int cw_stride,
                            int block_index_bits, const dpf_block* key_seed, const uint8_t* party,
                            const dpf_block* points, const dpf_block* cw_seed,
                            const uint8_t* cw_left, const uint8_t* cw_right,
                            const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                            const dpf_aes_key* key_value, const dpf_value_desc* desc,
                            const dpf_block* value_correction, uint64_t* workspace, void* out,
                            void* stream) {
  if (num_points == 0 && num_keys >= 0) return kOk;
  if (block_index_bits < 0 || block_index_bits > 7 || num_levels + block_index_bits > 128)
    return fail(kInvalidArgument, "block_index_bits out of range");
  PointParams p;
  int st = make_point_params(num_keys, num_points, num_levels, key_seed, party, nullptr, nullptr,
                             points, nullptr, cw_seed, cw_left, cw_right, key_left, key_right,
                             key_value, desc, value_correction, &p);
  if (st) return st;
  if (!key_seed) return fail(kInvalidArgument, "NULL pointer");
  if (cw_stride < num_levels) return fail(kInvalidArgument, "cw_stride < num_levels");
  p.cw_stride = cw_stride;
  p.bib = block_index_bits;
  if (!out || !workspace) return fail(kInvalidArgument, "NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  const size_t wide_bytes = (size_t)num_points * desc->num_leaves * 3 * sizeof(uint64_t);
  HIP_TRY(hipMemsetAsync(workspace, 0, wide_bytes, s));
  if (num_keys > 0) {
    // Enough (chunk, pair) items to fill every CU's 1024 threads a few times
    // (16 times when the waves take them dynamically: enough chunks per wave
    // for take_chunk; each item then sums fewer keys before its atomics).
    const int64_t want = (int64_t)num_cus() * kBlock * (hook_is("DPF_POINTS_DYNAMIC", '0') ? 4 : 16);
    int64_t chunks = (want + p.half - 1) / p.half;
    if (chunks > num_keys) chunks = num_keys;
    p.chunk_keys = (num_keys + chunks - 1) / chunks;
    chunks = (num_keys + p.chunk_keys - 1) / p.chunk_keys;
    p.shared_points = 1;
    p.num_items = chunks * p.half;
    p.wide = reinterpret_cast<unsigned long long*>(workspace);
    st = launch_points<true>(p, desc, value_correction, s);
    if (st) return st;
  }
  int64_t g = (num_points + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(finalize_sums_kernel, dim3((unsigned)g), dim3(256), 0, s, num_points, *desc,
                     reinterpret_cast<const unsigned long long*>(workspace), (char*)out, 3);
  HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
