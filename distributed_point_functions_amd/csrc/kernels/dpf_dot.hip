// dpf_dot.hip -- the database fold of two-server PIR behind the C ABI's dot
// calls (include/dpf_hip.h): dot_rows, the bandwidth-bound fold of a share
// vector that is already in device memory into a row-major database, and the
// fold of the workgroups' partial rows into the result, which the fused
// expansion (dpf_hip_expand_dot, dpf_kernels.hip; DotLeaf, dpf_dot.h) ends
// with too.  Sums mod 2^64 and XOR are associative and commutative, so the
// result does not depend on the order the hardware adds in.  No atomics:
// every workgroup writes one partial row with plain stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/dpf_hip.h"
#include "dpf_dot.h"
#include "dpf_runtime.h"

namespace dpf_rt {
thread_local const char* g_last_dot = "";
}
using namespace dpf_rt;

namespace {

constexpr int kRowsBlock = 256;
constexpr int kRowsWordsPerLane = DPF_HIP_DOT_MAX_RECORD_WORDS / kRowsBlock;
constexpr int kRowsUnroll = 4;   // rows a lane has in flight

// One element of EW uint64 words, loaded whole (16 bytes for uint128).
template <int EW> struct Elem;
template <> struct Elem<1> {
  uint64_t w[1];
  static __device__ __forceinline__ Elem load(const uint64_t* p) { return Elem{{*p}}; }
};
template <> struct Elem<2> {
  uint64_t w[2];
  static __device__ __forceinline__ Elem load(const uint64_t* p) {
    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(p);
    return Elem{{v.x, v.y}};
  }
};

// partial[g][w] = sum over the rows i workgroup g takes of y[i] * db[i][w]
// (XOR: y[i] & db[i][w]).  A row's W words lie along P = 2^log_p lanes
// (P >= min(W, 256); lane `col` takes words col, col + P, ...), so a wave
// reads whole contiguous pieces of the database for wide records, and for
// narrow ones the 256 / P rows of a workgroup pass are consecutive rows, i.e.
// again one contiguous piece; the row lanes' sums meet in LDS at the end.
template <int EW, bool XOR>
__global__ __launch_bounds__(kRowsBlock) void dot_rows_kernel(int64_t n, int W, int log_p,
                                                              const uint64_t* __restrict__ y,
                                                              const uint64_t* __restrict__ db,
                                                              char* __restrict__ workspace) {
  constexpr int K = kRowsWordsPerLane;
  __shared__ uint64_t red[kRowsBlock][K * EW];
  const int tid = (int)threadIdx.x, P = 1 << log_p, R = kRowsBlock >> log_p;
  const int col = tid & (P - 1), r = tid >> log_p;
  uint64_t acc[K][EW];
#pragma unroll
  for (int k = 0; k < K; ++k)
    for (int e = 0; e < EW; ++e) acc[k][e] = 0;
  // kRowsUnroll rows per pass, all their loads issued before the first
  // product: one 8- or 16-byte load per lane and pass keeps too few bytes in
  // flight for HBM.  A row past the end counts as zero.
  const int64_t stride = (int64_t)gridDim.x * R;
  for (int64_t i = (int64_t)blockIdx.x * R + r; i < n; i += kRowsUnroll * stride) {
    Elem<EW> yv[kRowsUnroll], d[kRowsUnroll][K];
#pragma unroll
    for (int u = 0; u < kRowsUnroll; ++u) {
      const int64_t ii = i + u * stride;
      const bool row_ok = ii < n;
      yv[u] = row_ok ? Elem<EW>::load(y + ii * EW) : Elem<EW>{};
      const uint64_t* row = db + ii * W * EW;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int w = col + (k << log_p);
        d[u][k] = row_ok && w < W ? Elem<EW>::load(row + (int64_t)w * EW) : Elem<EW>{};
      }
    }
#pragma unroll
    for (int u = 0; u < kRowsUnroll; ++u)
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int e = 0; e < EW; ++e)
          acc[k][e] = XOR ? acc[k][e] ^ (yv[u].w[e] & d[u][k].w[e])
                          : acc[k][e] + yv[u].w[e] * d[u][k].w[e];
  }
#pragma unroll
  for (int k = 0; k < K; ++k)
    for (int e = 0; e < EW; ++e) red[tid][k * EW + e] = acc[k][e];
  __syncthreads();
  if (tid == 0 && blockIdx.x == 0) *reinterpret_cast<uint32_t*>(workspace) = gridDim.x;
  if (tid >= P) return;
  for (int rr = 1; rr < R; ++rr)
#pragma unroll
    for (int j = 0; j < K * EW; ++j)
      acc[j / EW][j % EW] = XOR ? acc[j / EW][j % EW] ^ red[(rr << log_p) + tid][j]
                                : acc[j / EW][j % EW] + red[(rr << log_p) + tid][j];
  uint64_t* part = reinterpret_cast<uint64_t*>(workspace + kDotHeaderBytes) +
                   (int64_t)blockIdx.x * W * EW;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int w = col + (k << log_p);
    if (w < W)
      for (int e = 0; e < EW; ++e) part[(int64_t)w * EW + e] = acc[k][e];
  }
}

// out[j] = group sum over the partial rows of word j (the row count is the
// workspace header's first word, written by the kernel that wrote the rows).
__global__ void dot_fold_kernel(int row_words, int xor_type, int accumulate,
                                const char* __restrict__ workspace, uint64_t* __restrict__ out) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= row_words) return;
  const uint32_t rows = *reinterpret_cast<const uint32_t*>(workspace);
  const uint64_t* part = reinterpret_cast<const uint64_t*>(workspace + kDotHeaderBytes);
  uint64_t a = accumulate ? out[j] : 0;
  for (uint32_t g = 0; g < rows; ++g) {
    const uint64_t v = part[(int64_t)g * row_words + j];
    a = xor_type ? a ^ v : a + v;
  }
  out[j] = a;
}

}  // namespace

namespace dpf_rt {

int dot_type(const dpf_value_desc* d, int* words, int* xor_type) {
  if (int st = validate_desc(d)) return st;
  const bool x = d->kind[0] == DPF_LEAF_XOR;
  const int bits = d->bits[0];
  if (!fast_int(d) || !((bits == 64 && d->elements_per_block == 2) ||
                        (bits == 128 && x && d->elements_per_block == 1)))
    return fail(kUnimplemented,
                "the database fold is implemented for uint64_t, XorWrapper<uint64_t> and "
                "XorWrapper<absl::uint128> only");
  *words = bits / 64;
  *xor_type = x ? 1 : 0;
  return kOk;
}

int launch_dot_fold(int row_words, int xor_type, int accumulate, const void* workspace, void* out,
                    hipStream_t s) {
  hipLaunchKernelGGL(dot_fold_kernel, dim3((row_words + 255) / 256), dim3(256), 0, s, row_words,
                     xor_type, accumulate, static_cast<const char*>(workspace),
                     static_cast<uint64_t*>(out));
  HIP_TRY(hipGetLastError());
  return kOk;
}

}  // namespace dpf_rt

extern "C" {

const char* dpf_hip_last_dot_kernel(void) { return dpf_rt::g_last_dot; }

int dpf_hip_expand_dot_workspace_bytes(const dpf_value_desc* desc, int record_words) {
  int words = 0, xor_type = 0;
  if (dot_type(desc, &words, &xor_type)) return -1;
  if (record_words < 1 || record_words > DPF_HIP_DOT_MAX_RECORD_WORDS) {
    fail(kInvalidArgument, "record_words must be in [1, 1024]");
    return -1;
  }
  return kDotHeaderBytes + kDotMaxGroups * record_words * words * 8;
}

int dpf_hip_expand_dot_fused(const dpf_value_desc* desc, int record_words) {
  int words = 0, xor_type = 0;
  if (dot_type(desc, &words, &xor_type)) return 0;
  // DPF_DOT_STREAM=1 (read per call): every width takes the streamed path.
  return record_words == 1 && !hook_is("DPF_DOT_STREAM", '1');
}

int dpf_hip_dot_rows(int64_t num_rows, int record_words, const dpf_value_desc* desc,
                     const void* y, const void* db, int accumulate, void* workspace, void* out,
                     void* stream) {
  int words = 0, xor_type = 0;
  if (int st = dot_type(desc, &words, &xor_type)) return st;
  if (record_words < 1 || record_words > DPF_HIP_DOT_MAX_RECORD_WORDS)
    return fail(kInvalidArgument, "record_words must be in [1, 1024]");
  if (num_rows < 0 || num_rows > (INT64_MAX >> 15))
    return fail(kInvalidArgument, "num_rows out of range");
  if (!workspace || !out || (num_rows > 0 && (!y || !db)))
    return fail(kInvalidArgument, "NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  const int row_words = record_words * words;
  if (num_rows == 0) {   // an empty sum
    if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, (size_t)row_words * 8, s));
    return kOk;
  }
  int log_p = 0;
  while ((1 << log_p) < record_words && (1 << log_p) < kRowsBlock) ++log_p;
  const int64_t rows_per_pass = kRowsBlock >> log_p;
  int64_t grid = (num_rows + rows_per_pass - 1) / rows_per_pass;
  if (grid > kDotMaxGroups) grid = kDotMaxGroups;
  const uint64_t* yy = static_cast<const uint64_t*>(y);
  const uint64_t* dd = static_cast<const uint64_t*>(db);
  char* ws = static_cast<char*>(workspace);
  if (words == 2)
    hipLaunchKernelGGL((dot_rows_kernel<2, true>), dim3((unsigned)grid), dim3(kRowsBlock), 0, s,
                       num_rows, record_words, log_p, yy, dd, ws);
  else if (xor_type)
    hipLaunchKernelGGL((dot_rows_kernel<1, true>), dim3((unsigned)grid), dim3(kRowsBlock), 0, s,
                       num_rows, record_words, log_p, yy, dd, ws);
  else
    hipLaunchKernelGGL((dot_rows_kernel<1, false>), dim3((unsigned)grid), dim3(kRowsBlock), 0, s,
                       num_rows, record_words, log_p, yy, dd, ws);
  HIP_TRY(hipGetLastError());
  g_last_dot = "rows";
  return launch_dot_fold(row_words, xor_type, accumulate, workspace, out, s);
}

}  // extern "C"
