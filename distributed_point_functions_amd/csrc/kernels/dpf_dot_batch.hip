// dpf_dot_batch.hip -- additive-share PIR batched over queries, behind
// dpf_hip_dot_rows_batch (include/dpf_hip.h): every query q has one 64-bit
// share per record, and out[q] = sum_i y_q[i] * db[i] mod 2^64 (uint64_t) or
// XOR_i (y_q[i] & db[i]) (XorWrapper<uint64_t>), for up to 64 queries against
// one pass (or a few) over the database.  The word-valued sibling of
// dpf_select.hip, with its layout: a record's words lie along the lanes, and a
// lane keeps one accumulator per query of the tile.  Sums mod 2^64 and XOR
// are associative and commutative, so the result does not depend on the order
// the hardware folds in.  No atomics: every workgroup writes one partial
// [queries][W] with plain stores, and a second small kernel folds the
// partials (dpf_dot.hip's conventions and workspace header).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../../include/dpf_hip.h"
#include "dpf_dot.h"
#include "dpf_runtime.h"

using namespace dpf_rt;

namespace {

constexpr int kBatBlock = 256;     // four waves
constexpr int kBatWaves = kBatBlock / 64;
constexpr int kBatUnroll = 4;      // rows a lane has in flight
constexpr int kBatMaxTile = 16;    // queries a lane accumulates at once
constexpr int kFoldCols = 32, kFoldRows = 32;

thread_local int64_t g_batch_shape[3] = {0, 0, 0};

// Record word (j, w), or the nearest word that exists (n >= 1) for a row or
// column that does not: the load is unconditional.  A row past n meets a share
// of zero, and the lanes of a column past W are dropped at the end.
__device__ __forceinline__ uint64_t load_word(const uint64_t* __restrict__ db, int64_t n, int W,
                                              int64_t j, int w, bool col_ok) {
  return db[(j < n ? j : n - 1) * W + (col_ok ? w : W - 1)];
}

// The 64-bit value lane `src` holds (two cross-lane reads with one address).
__device__ __forceinline__ uint64_t from_lane(uint64_t v, int src) {
  const int a = src << 2;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)(uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

template <bool XOR>
__device__ __forceinline__ uint64_t combine(uint64_t a, uint64_t b) {
  return XOR ? a ^ b : a + b;
}

// partial[g][q][w] = group sum over the rows j workgroup g takes of
// y_q[j] * db[j][w] (XOR: y_q[j] & db[j][w]), for the nq <= QB queries of this
// pass (the accumulators beyond nq repeat query nq - 1 and are dropped).
//
// A record's W words lie along PW = 2^log_pw lanes of a wave (PW >= min(W,
// 64)); its RW = 64 / PW rows per step are consecutive, so a wave reads one
// contiguous piece of the database per step for narrow records and 512
// contiguous bytes of one record for wide ones (blockIdx.y: the chunk of 64
// columns).  Every lane keeps one word, i.e. QB 64-bit accumulators.
//
// A wave takes whole groups of 64 rows, PW steps each.  The shares of a group
// are read once, coalesced: lane l holds y_q[64 g + l] for every query (zero
// past n), and a step's lanes fetch their row's share from the lane that
// holds it.  So every share and every database word is read from memory once
// per pass, whatever the width.
template <int QB, bool XOR>
__global__ __launch_bounds__(kBatBlock) void dot_rows_batch_kernel(
    int64_t n, int W, int log_pw, int nq, const char* __restrict__ y, int64_t y_stride,
    const uint64_t* __restrict__ db, char* __restrict__ workspace) {
  constexpr int U = kBatUnroll;
  __shared__ uint64_t red[QB][64];
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int PW = 1 << log_pw, log_rw = 6 - log_pw;
  const int sub = lane >> log_pw;
  const int w = (int)blockIdx.y * PW + (lane & (PW - 1));
  const bool col_ok = w < W;
  const int64_t waves = (int64_t)gridDim.x * kBatWaves;
  const int64_t gw = (int64_t)blockIdx.x * kBatWaves + wave;
  const uint64_t* row[QB];
#pragma unroll
  for (int q = 0; q < QB; ++q)
    row[q] = reinterpret_cast<const uint64_t*>(y + (int64_t)(q < nq ? q : nq - 1) * y_stride);
  uint64_t acc[QB];
#pragma unroll
  for (int q = 0; q < QB; ++q) acc[q] = 0;

  const int64_t groups = (n + 63) >> 6;
  for (int64_t g = gw; g < groups; g += waves) {
    const int64_t j0 = g << 6;
    const bool y_ok = j0 + lane < n;
    const int64_t jy = y_ok ? j0 + lane : n - 1;   // the load is unconditional
    uint64_t yv[QB];
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      const uint64_t v = row[q][jy];
      yv[q] = y_ok ? v : 0;
    }
    // kBatUnroll steps' loads issued before the first product: one 8-byte
    // load per lane keeps too few bytes in flight for HBM.  Narrow records
    // (PW < kBatUnroll) have fewer steps: the spare loads repeat the last
    // step's (a cache hit) and their products are skipped.
    for (int t = 0; t < PW; t += U) {
      uint64_t d[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int tu = t + u < PW ? t + u : PW - 1;
        d[u] = load_word(db, n, W, j0 + ((int64_t)tu << log_rw) + sub, w, col_ok);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t + u >= PW) break;   // (uniform)
        const int src = ((t + u) << log_rw) + sub;
#pragma unroll
        for (int q = 0; q < QB; ++q) {
          const uint64_t yy = from_lane(yv[q], src);
          acc[q] = XOR ? acc[q] ^ (yy & d[u]) : acc[q] + yy * d[u];
        }
      }
    }
  }

  // The wave's row lanes by cross-lane moves, then the waves through LDS,
  // one after the other into wave 0.
#pragma unroll
  for (int q = 0; q < QB; ++q) {
    uint64_t x = acc[q];
    for (int off = 32; off >= PW; off >>= 1) x = combine<XOR>(x, __shfl_xor(x, off, 64));
    acc[q] = x;
  }
  for (int v = 1; v < kBatWaves; ++v) {
    if (wave == v) {
#pragma unroll
      for (int q = 0; q < QB; ++q) red[q][lane] = acc[q];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int q = 0; q < QB; ++q) acc[q] = combine<XOR>(acc[q], red[q][lane]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0)
    *reinterpret_cast<uint32_t*>(workspace) = gridDim.x;
  if (wave != 0 || lane >= PW || !col_ok) return;
  uint64_t* part = reinterpret_cast<uint64_t*>(workspace + kDotHeaderBytes) +
                   (int64_t)blockIdx.x * nq * W + w;
#pragma unroll
  for (int q = 0; q < QB; ++q)
    if (q < nq) part[(int64_t)q * W] = acc[q];
}

// out[j] (+)= group sum over the partial rows of word j (row_words = queries
// * W; the row count is the workspace header's first word, written by the
// kernel that wrote the rows).  kFoldCols words by kFoldRows row lanes per
// workgroup.
template <bool XOR>
__global__ __launch_bounds__(kFoldCols* kFoldRows) void dot_batch_fold_kernel(
    int row_words, int accumulate, const char* __restrict__ workspace, uint64_t* __restrict__ out) {
  __shared__ uint64_t red[kFoldRows][kFoldCols];
  const int c = (int)threadIdx.x % kFoldCols, r = (int)threadIdx.x / kFoldCols;
  const int j = (int)blockIdx.x * kFoldCols + c;
  const uint32_t rows = *reinterpret_cast<const uint32_t*>(workspace);
  const uint64_t* part = reinterpret_cast<const uint64_t*>(workspace + kDotHeaderBytes);
  uint64_t a = 0;
  if (j < row_words)
    for (uint32_t g = r; g < rows; g += kFoldRows)
      a = combine<XOR>(a, part[(int64_t)g * row_words + j]);
  red[r][c] = a;
  __syncthreads();
  if (r != 0 || j >= row_words) return;
  for (int rr = 1; rr < kFoldRows; ++rr) a = combine<XOR>(a, red[rr][c]);
  out[j] = accumulate ? combine<XOR>(out[j], a) : a;
}

// Launch shape for records of W words and Q queries: the lanes a record lies
// along, the column chunks (grid y), the cap on grid x -- dot_rows' cap on
// the workgroups, shared among the column chunks -- and the query tile.
struct BatchShape {
  int log_pw, chunks, cap, tile;
};
BatchShape batch_shape(int W, int Q) {
  BatchShape s{0, 1, kDotMaxGroups, 1};
  while ((1 << s.log_pw) < W && s.log_pw < 6) ++s.log_pw;
  s.chunks = (W + 63) / 64;
  s.cap = kDotMaxGroups / s.chunks;
  while (s.tile < Q && s.tile < kBatMaxTile) s.tile *= 2;
  return s;
}

// Room for cap * tile * W words whatever the column chunks leave of the cap
// (cap * W <= kDotMaxGroups * min(W, 64)), so the size never shrinks as W or
// Q grows.
int batch_workspace_bytes(int W, int Q) {
  return kDotHeaderBytes + kDotMaxGroups * batch_shape(W, Q).tile * (W < 64 ? W : 64) * 8;
}

bool batch_counts_ok(int record_words, int num_queries) {
  if (record_words < 1 || record_words > DPF_HIP_DOT_MAX_RECORD_WORDS) {
    fail(kInvalidArgument, "record_words must be in [1, 1024]");
    return false;
  }
  if (num_queries < 1 || num_queries > DPF_HIP_DOT_BATCH_MAX_QUERIES) {
    fail(kInvalidArgument, "num_queries must be in [1, 64]");
    return false;
  }
  return true;
}

// kOk and whether the group is XOR for uint64_t and XorWrapper<uint64_t>.
int batch_type(const dpf_value_desc* desc, int* xor_type) {
  int words = 0;
  if (!desc || dot_type(desc, &words, xor_type) != kOk || words != 1)
    return fail(kUnimplemented,
                "the batched database fold is implemented for uint64_t and XorWrapper<uint64_t> "
                "only");
  return kOk;
}

template <int QB>
void launch_batch(bool xor_type, dim3 grid, hipStream_t s, int64_t n, int W, int log_pw, int nq,
                  const char* y, int64_t stride, const uint64_t* db, char* ws) {
  if (xor_type)
    hipLaunchKernelGGL((dot_rows_batch_kernel<QB, true>), grid, dim3(kBatBlock), 0, s, n, W,
                       log_pw, nq, y, stride, db, ws);
  else
    hipLaunchKernelGGL((dot_rows_batch_kernel<QB, false>), grid, dim3(kBatBlock), 0, s, n, W,
                       log_pw, nq, y, stride, db, ws);
}

}  // namespace

extern "C" {

int dpf_hip_dot_rows_batch_workspace_bytes(const dpf_value_desc* desc, int record_words,
                                           int num_queries) {
  int xor_type = 0;
  if (!batch_counts_ok(record_words, num_queries) || batch_type(desc, &xor_type)) return -1;
  return batch_workspace_bytes(record_words, num_queries);
}

int dpf_hip_last_dot_batch_shape(int64_t* out3) {
  if (!out3) return fail(kInvalidArgument, "NULL pointer");
  for (int i = 0; i < 3; ++i) out3[i] = g_batch_shape[i];
  return kOk;
}

int dpf_hip_dot_rows_batch(int64_t num_rows, int record_words, int num_queries,
                           const dpf_value_desc* desc, const void* y, int64_t y_stride_bytes,
                           const void* db, int accumulate, void* workspace, void* out,
                           void* stream) {
  if (!batch_counts_ok(record_words, num_queries)) return kInvalidArgument;
  if (num_rows < 0 || num_rows > (INT64_MAX >> 15))
    return fail(kInvalidArgument, "num_rows out of range");
  if (!desc || !out || (num_rows > 0 && (!y || !db)))
    return fail(kInvalidArgument, "NULL pointer");
  if (y_stride_bytes < 0 || y_stride_bytes % 16 || y_stride_bytes / 8 < num_rows)
    return fail(kInvalidArgument,
                "y_stride_bytes must be a multiple of 16 and at least 8 * num_rows");
  int xor_type = 0;
  if (int st = batch_type(desc, &xor_type)) return st;
  const int W = record_words, Q = num_queries;
  if (!workspace)
    return fail(kResourceExhausted, "the batched database fold needs a workspace of " +
                                        std::to_string(batch_workspace_bytes(W, Q)) + " bytes");
  hipStream_t s = (hipStream_t)stream;
  const BatchShape sh = batch_shape(W, Q);
  const int passes = (Q + sh.tile - 1) / sh.tile;
  if (num_rows == 0) {   // an empty sum
    if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, (size_t)Q * W * 8, s));
    g_batch_shape[0] = sh.tile, g_batch_shape[1] = passes, g_batch_shape[2] = 0;
    g_last_dot = "rows_batch";
    return kOk;
  }
  // 256 rows per workgroup and step, whatever the width, as dot_rows counts.
  int64_t gx = (num_rows + kBatBlock - 1) / kBatBlock;
  if (gx > sh.cap) gx = sh.cap;
  const dim3 grid((unsigned)gx, (unsigned)sh.chunks);
  const char* yy = static_cast<const char*>(y);
  const uint64_t* dd = static_cast<const uint64_t*>(db);
  char* ws = static_cast<char*>(workspace);
  for (int p = 0; p < passes; ++p) {
    const int q0 = p * sh.tile, nq = Q - q0 < sh.tile ? Q - q0 : sh.tile;
    const char* yp = yy + (int64_t)q0 * y_stride_bytes;
    auto launch = [&](auto qb) {
      launch_batch<decltype(qb)::value>(xor_type != 0, grid, s, num_rows, W, sh.log_pw, nq, yp,
                                        y_stride_bytes, dd, ws);
    };
    // The smallest instance that holds the pass's queries.
    if (nq > 8) launch(std::integral_constant<int, 16>{});
    else if (nq > 4) launch(std::integral_constant<int, 8>{});
    else if (nq > 2) launch(std::integral_constant<int, 4>{});
    else if (nq > 1) launch(std::integral_constant<int, 2>{});
    else launch(std::integral_constant<int, 1>{});
    HIP_TRY(hipGetLastError());
    const int row_words = nq * W;
    const dim3 fgrid((row_words + kFoldCols - 1) / kFoldCols), fblock(kFoldCols * kFoldRows);
    uint64_t* op = static_cast<uint64_t*>(out) + (int64_t)q0 * W;
    if (xor_type)
      hipLaunchKernelGGL(dot_batch_fold_kernel<true>, fgrid, fblock, 0, s, row_words, accumulate,
                         ws, op);
    else
      hipLaunchKernelGGL(dot_batch_fold_kernel<false>, fgrid, fblock, 0, s, row_words, accumulate,
                         ws, op);
    HIP_TRY(hipGetLastError());
  }
  g_batch_shape[0] = sh.tile, g_batch_shape[1] = passes, g_batch_shape[2] = gx * sh.chunks;
  g_last_dot = "rows_batch";
  return kOk;
}

}  // extern "C"
