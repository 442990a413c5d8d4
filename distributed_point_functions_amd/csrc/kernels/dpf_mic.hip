// dpf_mic.hip -- batched MultipleIntervalContainmentGate::Eval on gfx950
// (eprint 2020/1392 Fig. 14; dcf/fss_gates/multiple_interval_containment.cc:
// 206-275).  A gate with m public intervals [p_i, q_i] over Z_N, N = 2^n,
// evaluates ONE uint128 DCF key at the 2m points x + N-1 - p_i and
// x + N-1 - q'_i (q'_i = q_i + 1 mod N) and combines the two values per
// interval.  The bounds are public and fixed, so the host keeps the sorted
// set U of distinct p_i and q'_i: adjacent intervals share q'_i = p_{i+1},
// and a partition of the group needs m walks per gate instead of 2m.
//
//   mic_walk_kernel     one DCF walk per lane over items (gate, u in U),
//                       gate-major, into scratch[gate][u];
//   mic_combine_kernel  one lane per (gate, interval): two indexed reads of
//                       scratch, the party-1 comparison term, the mask share.
//
// Its own translation unit, self-contained (it shares no device function with
// dpf_dcf.hip beyond dpf_device.h), built with the iterative-ilp scheduler.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/dpf_hip.h"
#include "dpf_device.h"
#include "dpf_runtime.h"

using namespace dpf_rt;

namespace {

constexpr int kMicMaxLevels = 127;   // log_group_size <= 127 (cc:36-41)

struct MicWalkParams {
  int64_t num_items, num_groups;   // items (gate, u); groups of 64 items
  int num_offsets;                 // |U|
  int n;
  int cw_stride;
  const dpf_block* key_seed;
  const uint8_t* party;
  const dpf_block* x;              // [gate]
  const dpf_block* offsets;        // [|U|]
  const dpf_block* cw_seed;
  const uint8_t* cw_left;
  const uint8_t* cw_right;
  dpf_block* scratch;              // [gate][|U|]
  RoundKeys rkl, rkd, rkv;
  int64_t dyn_per_wg;              // ItemLoop's per_wg (0: grid stride)
};

struct MicVcw {
  const dpf_block* level[kMicMaxLevels];  // per level: [key] value corrections
};

// The DCF of a gate is the uint128 DCF of log domain n: hierarchy level i is
// tree depth i (proto_validator.cc:131-136), one element per block, so level
// d's value is H_value(node_d) (+ cw_d if t_d), summed iff bit (n-1-d) of the
// point is 0 -- the bit that also steers the walk to node_{d+1}.  Per level
// the value hash and the path step run as one interleaved pair of AES chains
// (value key | per-lane key select); level d + 1's correction words are loaded
// while level d is hashed.  With UNIFORM (|U| % 64 == 0) a wave's items share
// one gate, whose key is then read through wave-uniform loads.
template <bool UNIFORM>
__global__ __launch_bounds__(kBlock) DPF_WAVES_ATTR void mic_walk_kernel(MicWalkParams p,
                                                                         MicVcw vc) {
  __shared__ LdsImage lds;
  __shared__ int next_chunk;   // ItemLoop (dpf_device.h)
  fill_tables(lds.tab);
  if (threadIdx.x == 0) next_chunk = 0;
  __syncthreads();
  const LdsLookup lk = make_lookup(lds, KeySet{key_ref(p.rkl), KeyRef{}, key_ref(p.rkv), key_ref(p.rkd)});
  const int n = p.n;
  const u128 mask = ((u128)1 << n) - 1;   // n <= 127
  const ItemLoop items{&next_chunk, p.dyn_per_wg, p.num_groups, p.num_groups * 64};
  for (int64_t g = items.first(); (g >> 6) < p.num_groups; g = items.next(g)) {
    const bool valid = g < p.num_items;
    const int64_t u = valid ? g : p.num_items - 1;
    int64_t k = u / p.num_offsets;
    const int j = (int)(u - k * p.num_offsets);
    if (UNIFORM) k = (int64_t)__builtin_amdgcn_readfirstlane((int)k);
    // The point (x + N-1 - U[j]) mod N, formed here (cc:236-239).
    const u128 pt = (dpf_u128(p.x[k]) + mask - dpf_u128(p.offsets[j])) & mask;
    const Block4 x{(uint32_t)pt, (uint32_t)(pt >> 32), (uint32_t)(pt >> 64), (uint32_t)(pt >> 96)};
    const uint32_t party = p.party[k] & 1u;
    Block4 s = load_block(p.key_seed + k);
    uint32_t t = party;
    u128 acc = 0;
    // Level d's correction words, loaded one level ahead.
    uint4 cw;
    uint32_t cc;
    u128 cv;
    auto load_level = [&](int d) {
      const int64_t row = k * p.cw_stride + d;
      cw = d + 1 < n ? *reinterpret_cast<const uint4*>(p.cw_seed + row) : make_uint4(0, 0, 0, 0);
      cc = d + 1 < n ? cw_ctrl2(p.cw_left, p.cw_right, row) : 0u;
      cv = dpf_u128(vc.level[d][k]);
    };
    load_level(0);
    for (int d = 0; d < n; ++d) {
      const uint4 cwd = cw;
      const uint32_t ccd = cc;
      const u128 cvd = cv;
      if (d + 1 < n) load_level(d + 1);
      const uint32_t xb = path_bit(x, n - 1 - d);  // decides level d's sum and the next step
      Block4 h[2];
      h[0] = s;
      if (d + 1 < n) {
        h[1] = s;
        UniformRK rv[1] = {UniformRK{lk.ks.v}};
        SelectRK rs[1] = {SelectRK{lk.ks.l, lk.ks.d, 0u - xb}};
        dpf_aes::mmo_hashAB<1, 1>(h, lk, rv, rs);
      } else {
        UniformRK rv[1] = {UniformRK{lk.ks.v}};
        dpf_aes::mmo_hashN<1>(h, lk, rv);
      }
      const u128 tc = t ? cvd : (u128)0;
      const u128 take = xb ? (u128)0 : ~(u128)0;
      acc += (block_u128(h[0]) + tc) & take;
      if (d + 1 < n) {  // step to node d + 1 (distributed_point_function.cc:323-343)
        Block4 hn = h[1];
        correct_child(hn, t, xb, cwd, ccd);
        s = hn;
      }
    }
    if (party) acc = (u128)0 - acc;   // party 1 negates, once (value_type_helpers.h:199-211)
    if (valid) store_bits<128>(reinterpret_cast<char*>(p.scratch + u), acc);
  }
}

struct MicCombineParams {
  int64_t num_out;       // gates * m
  int num_intervals;     // m
  int num_offsets;       // |U|
  int n;
  const uint8_t* party;
  const dpf_block* x;
  const int32_t* lower_index;   // [m] position of p_i in U
  const int32_t* upper_index;   // [m] position of q'_i in U
  const dpf_block* lower;       // [m] p_i
  const dpf_block* upper_next;  // [m] q'_i
  const dpf_block* mask_share;  // [gate][m]
  const dpf_block* scratch;     // [gate][|U|]
  dpf_block* out;               // [gate][m]
};

// cc:258-270.  The index tables come from device memory the caller owns:
// clamped, so a bad table gives wrong values, never an access outside scratch.
__global__ __launch_bounds__(256) void mic_combine_kernel(MicCombineParams p) {
  const u128 mask = ((u128)1 << p.n) - 1;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < p.num_out;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = t / p.num_intervals;
    const int i = (int)(t - g * p.num_intervals);
    const int top = p.num_offsets - 1;
    const int li = min(max(p.lower_index[i], 0), top), ui = min(max(p.upper_index[i], 0), top);
    const dpf_block* row = p.scratch + g * p.num_offsets;
    const u128 sp = dpf_u128(row[li]), sq = dpf_u128(row[ui]);
    u128 y = dpf_u128(p.mask_share[t]) - sp + sq;
    if (p.party[g] & 1) {
      const u128 x = dpf_u128(p.x[g]);
      y += (u128)(x > dpf_u128(p.lower[i]) ? 1 : 0) - (u128)(x > dpf_u128(p.upper_next[i]) ? 1 : 0);
    }
    store_bits<128>(reinterpret_cast<char*>(p.out + t), y & mask);
  }
}

}  // namespace

extern "C" int dpf_hip_mic_eval_batch(
    int64_t num_gates, int log_group_size, const dpf_block* key_seed, const uint8_t* party,
    const dpf_block* cw_seed, const uint8_t* cw_left, const uint8_t* cw_right, int cw_stride,
    const dpf_block* const* value_correction, const dpf_block* x, int num_offsets,
    const dpf_block* offsets, int num_intervals, const int32_t* lower_index,
    const int32_t* upper_index, const dpf_block* lower_bound, const dpf_block* upper_bound_next,
    const dpf_block* mask_share, dpf_block* scratch, const dpf_aes_key* key_left,
    const dpf_aes_key* key_right, const dpf_aes_key* key_value, dpf_block* out, void* stream) {
  const int n = log_group_size;
  if (num_gates < 0 || num_intervals < 0 || num_offsets < 0)
    return fail(kInvalidArgument, "num_gates, num_intervals or num_offsets is negative");
  if (n < 1 || n > kMicMaxLevels)
    return fail(kInvalidArgument, "log_group_size must be between 1 and 127");
  if (cw_stride < n - 1) return fail(kInvalidArgument, "cw_stride too small");
  if (num_offsets > 2 * (int64_t)num_intervals || (num_intervals > 0 && num_offsets < 1))
    return fail(kInvalidArgument, "num_offsets must be between 1 and 2 * num_intervals");
  if (num_gates > 0 && (int64_t)num_offsets + num_intervals > 0 &&
      num_gates > (INT64_MAX / 64) / ((int64_t)num_offsets + num_intervals))
    return fail(kInvalidArgument, "num_gates * (num_offsets + num_intervals) is too large");
  if (num_gates == 0 || num_intervals == 0) return kOk;
  if (!key_seed || !party || !x || !offsets || !lower_index || !upper_index || !lower_bound ||
      !upper_bound_next || !mask_share || !scratch || !out || !key_left || !key_right ||
      !key_value || !value_correction || (n > 1 && (!cw_seed || !cw_left || !cw_right)))
    return fail(kInvalidArgument, "NULL pointer");
  MicVcw vc;
  memset(&vc, 0, sizeof(vc));
  for (int i = 0; i < n; ++i) {
    if (!value_correction[i]) return fail(kInvalidArgument, "NULL value correction");
    vc.level[i] = value_correction[i];
  }
  hipStream_t s = (hipStream_t)stream;
  MicWalkParams w;
  memset(&w, 0, sizeof(w));
  w.num_items = num_gates * num_offsets;
  w.num_groups = (w.num_items + 63) / 64;
  w.num_offsets = num_offsets;
  w.n = n;
  w.cw_stride = cw_stride;
  w.key_seed = key_seed;
  w.party = party;
  w.x = x;
  w.offsets = offsets;
  w.cw_seed = cw_seed;
  w.cw_left = cw_left;
  w.cw_right = cw_right;
  w.scratch = scratch;
  w.rkl = expand_key(key_left);
  w.rkd = xor_keys(w.rkl, expand_key(key_right));
  w.rkv = expand_key(key_value);
  {
    // The DCF kernel's hook: DPF_DCF_DYNAMIC=0 gives a fixed share per thread.
    const LaunchShape sh = chunked_shape(w.num_groups * 64, "DPF_DCF_DYNAMIC");
    const dim3 grid(sh.grid), block(sh.block);
    w.dyn_per_wg = sh.dyn_per_wg;
    if (num_offsets % 64 == 0)
      hipLaunchKernelGGL((mic_walk_kernel<true>), grid, block, 0, s, w, vc);
    else
      hipLaunchKernelGGL((mic_walk_kernel<false>), grid, block, 0, s, w, vc);
    HIP_TRY(hipGetLastError());
  }
  MicCombineParams c;
  memset(&c, 0, sizeof(c));
  c.num_out = num_gates * num_intervals;
  c.num_intervals = num_intervals;
  c.num_offsets = num_offsets;
  c.n = n;
  c.party = party;
  c.x = x;
  c.lower_index = lower_index;
  c.upper_index = upper_index;
  c.lower = lower_bound;
  c.upper_next = upper_bound_next;
  c.mask_share = mask_share;
  c.scratch = scratch;
  c.out = out;
  int64_t cg = (c.num_out + 255) / 256;
  if (cg > (int64_t)num_cus() * 8) cg = (int64_t)num_cus() * 8;
  hipLaunchKernelGGL(mic_combine_kernel, dim3((unsigned)cg), dim3(256), 0, s, c);
  HIP_TRY(hipGetLastError());
  return kOk;
}
