// dpf_sketch.hip -- per-key linear sketches of [key][element] rows of a
// Tuple<IntModN<uint32_t, N_e>...> value type (the types mod32_eligible
// accepts): for J <= 4 rows of 32-bit weights,
//   out[k][j][e] = ( sum_{i < row_len} (w[j][i] mod N_e) * in[k][i][e] ) mod N_e.
// This is the reduction the heavy-hitters servers run before a client counts
// (DESIGN.md 6c): the two parties' sketches add up mod N_e to w[j][i*] * beta_e
// for a well-formed key pair.  One wave owns a key: its lanes walk the row
// (coalesced), keep uint64 sums of reduced products (< 2^32 each, row_len <
// 2^32 of them) and fold them across the wave; no atomics, no workspace.
// Built with the iterative-ilp scheduler (build_native.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/dpf_hip.h"
#include "dpf_device.h"
#include "dpf_runtime.h"

using namespace dpf_rt;

namespace {

constexpr int kSketchBlock = 256;

struct SketchParams {
  int64_t num_keys, row_len;
  int nl;
  const uint32_t* in;       // [key][row_len][nl]
  const uint32_t* weights;  // [J][row_len]
  uint32_t* out;            // [key][J][nl]
  Div32 div[kMod32MaxLeaves];
};

template <int J>
__global__ __launch_bounds__(kSketchBlock) void sketch_rows_kernel(SketchParams p) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t waves_per_block = kSketchBlock / 64;
  const int nl = p.nl;
  for (int64_t k = (int64_t)blockIdx.x * waves_per_block + (threadIdx.x >> 6); k < p.num_keys;
       k += (int64_t)gridDim.x * waves_per_block) {
    uint64_t acc[J][kMod32MaxLeaves];
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
      for (int e = 0; e < kMod32MaxLeaves; ++e) acc[j][e] = 0;
    const uint32_t* row = p.in + k * p.row_len * nl;
    for (int64_t i = lane; i < p.row_len; i += 64) {
      uint32_t w[J];
#pragma unroll
      for (int j = 0; j < J; ++j) w[j] = p.weights[j * p.row_len + i];
#pragma unroll
      for (int e = 0; e < kMod32MaxLeaves; ++e) {
        if (e < nl) {
          const uint32_t y = row[i * nl + e];
#pragma unroll
          for (int j = 0; j < J; ++j) acc[j][e] += mul_mod(mod32(w[j], p.div[e]), y, p.div[e]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
      for (int e = 0; e < kMod32MaxLeaves; ++e) {
        if (e < nl) {
          uint64_t s = acc[j][e];
#pragma unroll
          for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
          if (lane == 0) p.out[(k * J + j) * nl + e] = mod64(s, p.div[e]);
        }
      }
    }
  }
}

}  // namespace

extern "C" {

int dpf_hip_sketch_supported(const dpf_value_desc* desc) {
  int b = 0;
  return desc && validate_desc(desc) == kOk && mod32_eligible(desc, &b) ? 1 : 0;
}

int dpf_hip_sketch_rows(int64_t num_keys, int64_t row_len, const dpf_value_desc* desc,
                        const void* in, int num_weights, int weight_bits, const void* weights,
                        void* out, void* stream) {
  if (!desc) return fail(kInvalidArgument, "NULL pointer");
  if (int st = validate_desc(desc)) return st;
  int b = 0;
  if (!mod32_eligible(desc, &b))
    return fail(kUnimplemented, "sketch_rows: value type is not a tuple of IntModN<uint32_t>");
  if (weight_bits != 32) return fail(kUnimplemented, "sketch_rows: only 32-bit weights");
  if (num_keys < 0 || row_len < 0 || num_weights < 1 || num_weights > DPF_HIP_SKETCH_MAX_WEIGHTS)
    return fail(kInvalidArgument, "bad sizes");
  // The per-lane uint64 sums hold row_len terms below 2^32.
  if (row_len >= (int64_t{1} << 32)) return fail(kInvalidArgument, "row_len must be below 2^32");
  if (num_keys == 0) return kOk;
  if (!out || (row_len > 0 && (!in || !weights))) return fail(kInvalidArgument, "NULL pointer");
  SketchParams p;
  memset(&p, 0, sizeof(p));
  p.num_keys = num_keys;
  p.row_len = row_len;
  p.nl = desc->num_leaves;
  p.in = static_cast<const uint32_t*>(in);
  p.weights = static_cast<const uint32_t*>(weights);
  p.out = static_cast<uint32_t*>(out);
  for (int e = 0; e < p.nl; ++e) p.div[e] = make_div32((uint32_t)desc->mod_low[e]);
  const int64_t waves_per_block = kSketchBlock / 64;
  int64_t g = (num_keys + waves_per_block - 1) / waves_per_block;
  const int64_t cap = (int64_t)num_cus() * 32;
  if (g > cap) g = cap;
  const dim3 grid((unsigned)g), block(kSketchBlock);
  hipStream_t s = (hipStream_t)stream;
  switch (num_weights) {
    case 1: hipLaunchKernelGGL(sketch_rows_kernel<1>, grid, block, 0, s, p); break;
    case 2: hipLaunchKernelGGL(sketch_rows_kernel<2>, grid, block, 0, s, p); break;
    case 3: hipLaunchKernelGGL(sketch_rows_kernel<3>, grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL(sketch_rows_kernel<4>, grid, block, 0, s, p); break;
  }
  HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
