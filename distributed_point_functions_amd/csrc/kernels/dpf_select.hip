// dpf_select.hip -- the dense (bit-packed) database fold of two-server PIR
// behind dpf_hip_select_rows (include/dpf_hip.h): every query q has one bit
// per record, and out[q] = XOR of the records whose bit is set, for up to 64
// queries against one pass (or a few) over the database.  Bound by HBM and
// plain VALU bit operations: no AES, no LDS tables.  XOR is associative and
// commutative, so the result does not depend on the order the hardware folds
// in.  No atomics: every workgroup writes one partial [queries][W] with plain
// stores, and a second small kernel folds the partials (dpf_dot.hip's
// conventions and workspace layout).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/dpf_hip.h"
#include "dpf_dot.h"
#include "dpf_runtime.h"

using namespace dpf_rt;

namespace {

constexpr int kSelBlock = 256;     // four waves
constexpr int kSelWaves = kSelBlock / 64;
constexpr int kSelUnroll = 4;      // rows a lane has in flight
constexpr int kSelMaxTile = 16;    // queries a lane accumulates at once
constexpr int kFoldCols = 32, kFoldRows = 32;

thread_local int64_t g_select_shape[3] = {0, 0, 0};

// acc ^= d & (bit `pos` of `word`, spread over 32 bits): one signed bit-field
// extract for the mask, then one three-input bit operation per half (0x78:
// a ^ (b & c); left to itself the compiler picks v_bitop3_b32 for the first
// row of an unrolled pass only and v_and + v_xor for the rest).
__device__ __forceinline__ void fold_word(uint32_t& lo, uint32_t& hi, uint2 d, uint32_t word,
                                          uint32_t pos) {
  const uint32_t m = (uint32_t)__builtin_amdgcn_sbfe((int)word, pos, 1u);
  lo = __builtin_amdgcn_bitop3_b32(lo, d.x, m, 0x78);
  hi = __builtin_amdgcn_bitop3_b32(hi, d.y, m, 0x78);
}

// Record word (j, w), or the nearest word that exists (n >= 1) for a row or
// column that does not: the load is unconditional, since loads under a branch
// each are not issued back to back.  What a row past n loads meets a cleared
// selection bit (keep_bits), and the lanes of a column past W are dropped at
// the end.
__device__ __forceinline__ uint2 load_word(const uint64_t* __restrict__ db, int64_t n, int W,
                                           int64_t j, int w, bool col_ok) {
  return *reinterpret_cast<const uint2*>(db + (j < n ? j : n - 1) * W + (col_ok ? w : W - 1));
}

// Mask of the selection word of rows [base, base + 64) that keeps rows < n
// (base < n): bits past n are ignored whatever they hold.
__device__ __forceinline__ uint64_t keep_bits(int64_t n, int64_t base) {
  const int64_t rem = n - base;
  return rem >= 64 ? ~uint64_t{0} : (uint64_t{1} << rem) - 1;
}

// partial[g][q][w] = XOR over the rows j workgroup g takes, whose bit j of
// query q's selection row is set, of db[j][w], for the nq <= QB queries of
// this pass (the accumulators beyond nq repeat query nq - 1 and are dropped).
//
// A record's W words lie along PW = 2^log_pw lanes of a wave (PW >= min(W,
// 64)); its RW = 64 / PW rows per step are consecutive, so a wave reads one
// contiguous piece of the database per step for narrow records and 512
// contiguous bytes of one record for wide ones (blockIdx.y: the chunk of 64
// columns).  Every lane keeps one word, i.e. 2 * QB accumulator registers.
//
// The selection words are wave-uniform and come through the scalar cache:
//   WIDE  (RW <= 16): a wave takes whole groups of 64 rows; the QB words of a
//         group are fetched once and shifted down per step (scalar), the
//         lane's row picks its bit;
//   !WIDE (RW = 32, 64; W <= 2): a step is half a selection word or a whole
//         one, fetched once per step and query; a wave takes chunks of
//         kSelUnroll << log_g consecutive steps.
// Selection bits past n are cleared in the words as they arrive.
template <int QB, bool WIDE>
__global__ __launch_bounds__(kSelBlock) void select_rows_kernel(
    int64_t n, int W, int log_pw, int log_g, int nq, const char* __restrict__ sel,
    int64_t sel_stride, const uint64_t* __restrict__ db, char* __restrict__ workspace) {
  constexpr int U = kSelUnroll;
  __shared__ uint64_t red[QB][64];
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int PW = 1 << log_pw, log_rw = 6 - log_pw, RW = 1 << log_rw;
  const uint32_t sub = (uint32_t)(lane >> log_pw);
  const int w = (int)blockIdx.y * PW + (lane & (PW - 1));
  const bool col_ok = w < W;
  const int64_t waves = (int64_t)gridDim.x * kSelWaves;
  const int64_t gw = (int64_t)blockIdx.x * kSelWaves + wave;
  const char* row[QB];
#pragma unroll
  for (int q = 0; q < QB; ++q) row[q] = sel + (int64_t)(q < nq ? q : nq - 1) * sel_stride;
  uint32_t lo[QB], hi[QB];
#pragma unroll
  for (int q = 0; q < QB; ++q) lo[q] = hi[q] = 0;

  // A wave takes 2^log_g consecutive groups (steps) at a time: their
  // selection words share cache lines, and a scalar load that misses is slow
  // (16 misses per 64 narrow rows made the kernel five times slower).
  if constexpr (WIDE) {
    const int64_t groups = (n + 63) >> 6;
    for (int64_t c = gw << log_g; c < groups; c += waves << log_g) {
      for (int64_t g = c; g < c + (1 << log_g) && g < groups; ++g) {
        const uint64_t keep = keep_bits(n, g << 6);
        uint64_t s[QB];
#pragma unroll
        for (int q = 0; q < QB; ++q)
          s[q] = *reinterpret_cast<const uint64_t*>(row[q] + g * 8) & keep;
        // kSelUnroll steps' loads issued before the first fold: one 8-byte
        // load per lane keeps too few bytes in flight for HBM.
        for (int t = 0; t < PW; t += U) {
          uint2 d[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int64_t j = (g << 6) + ((int64_t)(t + u) << log_rw) + sub;
            d[u] = load_word(db, n, W, j, w, col_ok);
          }
          // A step uses up the low RW bits of every word (shifted in place:
          // a shift by the step's first row into a fresh register pair per
          // step and query is hoisted by the scheduler until the SGPRs spill;
          // the barrier keeps the steps' shifts apart for the same reason).
#pragma unroll
          for (int u = 0; u < U; ++u) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < QB; ++q) {
              fold_word(lo[q], hi[q], d[u], (uint32_t)s[q], sub);
              s[q] >>= RW;
            }
          }
        }
      }
    }
  } else {
    const int64_t steps = (n + RW - 1) >> log_rw;
    const int log_c = log_g + 2;   // kSelUnroll << log_g steps
    static_assert(U == 4, "a chunk is U << log_g steps");
    for (int64_t c = gw << log_c; c < steps; c += waves << log_c) {
      for (int64_t st = c; st < c + (1 << log_c) && st < steps; st += U) {
        uint2 d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) d[u] = load_word(db, n, W, ((st + u) << log_rw) + sub, w, col_ok);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t r0 = (st + u) << log_rw;   // the step's first row
          if (r0 >= n) break;                       // (uniform) no word to read
          const uint32_t pos = (uint32_t)(r0 & 63) + sub;
          const uint64_t keep = keep_bits(n, r0 & ~int64_t{63});
#pragma unroll
          for (int q = 0; q < QB; ++q) {
            const uint64_t s = *reinterpret_cast<const uint64_t*>(row[q] + (r0 >> 6) * 8) & keep;
            fold_word(lo[q], hi[q], d[u], pos & 32 ? (uint32_t)(s >> 32) : (uint32_t)s, pos & 31);
          }
        }
      }
    }
  }

  // The wave's row lanes by cross-lane moves, then the waves through LDS,
  // one after the other into wave 0.
  uint64_t acc[QB];
#pragma unroll
  for (int q = 0; q < QB; ++q) {
    uint64_t x = ((uint64_t)hi[q] << 32) | lo[q];
    for (int off = 32; off >= PW; off >>= 1) x ^= __shfl_xor(x, off, 64);
    acc[q] = x;
  }
  for (int v = 1; v < kSelWaves; ++v) {
    if (wave == v) {
#pragma unroll
      for (int q = 0; q < QB; ++q) red[q][lane] = acc[q];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int q = 0; q < QB; ++q) acc[q] ^= red[q][lane];
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

// out[j] (^)= XOR over the partial rows of word j (row_words = queries * W;
// the row count is the workspace header's first word, written by the kernel
// that wrote the rows).  kFoldCols words by kFoldRows row lanes per workgroup.
__global__ __launch_bounds__(kFoldCols* kFoldRows) void select_fold_kernel(
    int row_words, int accumulate, const char* __restrict__ workspace, uint64_t* __restrict__ out) {
  __shared__ uint64_t red[kFoldRows][kFoldCols];
  const int c = (int)threadIdx.x % kFoldCols, r = (int)threadIdx.x / kFoldCols;
  const int j = (int)blockIdx.x * kFoldCols + c;
  const uint32_t rows = *reinterpret_cast<const uint32_t*>(workspace);
  const uint64_t* part = reinterpret_cast<const uint64_t*>(workspace + kDotHeaderBytes);
  uint64_t a = 0;
  if (j < row_words)
    for (uint32_t g = r; g < rows; g += kFoldRows) a ^= part[(int64_t)g * row_words + j];
  red[r][c] = a;
  __syncthreads();
  if (r != 0 || j >= row_words) return;
  for (int rr = 1; rr < kFoldRows; ++rr) a ^= red[rr][c];
  out[j] = accumulate ? out[j] ^ a : a;
}

// Launch shape for records of W words and Q queries: the lanes a record lies
// along, the column chunks (grid y), the cap on grid x -- dot_rows' cap on
// the workgroups, shared among the column chunks -- and the query tile.
struct SelectShape {
  int log_pw, chunks, cap, tile;
};
SelectShape select_shape(int W, int Q) {
  SelectShape s{0, 1, kDotMaxGroups, 1};
  while ((1 << s.log_pw) < W && s.log_pw < 6) ++s.log_pw;
  s.chunks = (W + 63) / 64;
  s.cap = kDotMaxGroups / s.chunks;
  while (s.tile < Q && s.tile < kSelMaxTile) s.tile *= 2;
  return s;
}

bool select_args_ok(int record_words, int num_queries) {
  if (record_words < 1 || record_words > DPF_HIP_DOT_MAX_RECORD_WORDS) {
    fail(kInvalidArgument, "record_words must be in [1, 1024]");
    return false;
  }
  if (num_queries < 1 || num_queries > DPF_HIP_SELECT_MAX_QUERIES) {
    fail(kInvalidArgument, "num_queries must be in [1, 64]");
    return false;
  }
  return true;
}

template <int QB>
void launch_select(bool wide, dim3 grid, hipStream_t s, int64_t n, int W, int log_pw, int log_g,
                   int nq, const char* sel, int64_t stride, const uint64_t* db, char* ws) {
  if (wide)
    hipLaunchKernelGGL((select_rows_kernel<QB, true>), grid, dim3(kSelBlock), 0, s, n, W, log_pw,
                       log_g, nq, sel, stride, db, ws);
  else
    hipLaunchKernelGGL((select_rows_kernel<QB, false>), grid, dim3(kSelBlock), 0, s, n, W, log_pw,
                       log_g, nq, sel, stride, db, ws);
}

}  // namespace

extern "C" {

int dpf_hip_select_workspace_bytes(int record_words, int num_queries) {
  if (!select_args_ok(record_words, num_queries)) return -1;
  const SelectShape sh = select_shape(record_words, num_queries);
  return kDotHeaderBytes + sh.cap * sh.tile * record_words * 8;
}

int dpf_hip_last_select_shape(int64_t* out3) {
  if (!out3) return fail(kInvalidArgument, "NULL pointer");
  for (int i = 0; i < 3; ++i) out3[i] = g_select_shape[i];
  return kOk;
}

int dpf_hip_select_rows(int64_t num_rows, int record_words, int num_queries, const void* sel,
                        int64_t sel_stride_bytes, const void* db, int accumulate, void* workspace,
                        void* out, void* stream) {
  if (!select_args_ok(record_words, num_queries)) return kInvalidArgument;
  if (num_rows < 0 || num_rows > (INT64_MAX >> 15))
    return fail(kInvalidArgument, "num_rows out of range");
  if (sel_stride_bytes < 0 || sel_stride_bytes % 16 || sel_stride_bytes < (num_rows + 7) / 8)
    return fail(kInvalidArgument,
                "sel_stride_bytes must be a multiple of 16 and at least ceil(num_rows / 8)");
  if (!workspace || !out || (num_rows > 0 && (!sel || !db)))
    return fail(kInvalidArgument, "NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  const int W = record_words, Q = num_queries;
  const SelectShape sh = select_shape(W, Q);
  const int passes = (Q + sh.tile - 1) / sh.tile;
  if (num_rows == 0) {   // an empty XOR
    if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, (size_t)Q * W * 8, s));
    g_select_shape[0] = sh.tile, g_select_shape[1] = passes, g_select_shape[2] = 0;
    g_last_dot = "select";
    return kOk;
  }
  // 256 rows per workgroup and step, whatever the width, as dot_rows counts.
  int64_t gx = (num_rows + kSelBlock - 1) / kSelBlock;
  if (gx > sh.cap) gx = sh.cap;
  const dim3 grid((unsigned)gx, (unsigned)sh.chunks);
  const bool wide = sh.log_pw >= 2;
  // Consecutive groups of 64 rows (wide) or chunks of kSelUnroll steps a wave
  // takes at a time: as many, up to 8 or 2, as leave every wave one.
  const int64_t units = wide ? (num_rows + 63) >> 6
                             : (num_rows + (kSelUnroll << (6 - sh.log_pw)) - 1) /
                                   (kSelUnroll << (6 - sh.log_pw));
  int log_g = 0;
  while (log_g < (wide ? 3 : 1) && (units >> (log_g + 1)) >= gx * kSelWaves) ++log_g;
  const char* ss = static_cast<const char*>(sel);
  const uint64_t* dd = static_cast<const uint64_t*>(db);
  char* ws = static_cast<char*>(workspace);
  for (int p = 0; p < passes; ++p) {
    const int q0 = p * sh.tile, nq = Q - q0 < sh.tile ? Q - q0 : sh.tile;
    const char* sp = ss + (int64_t)q0 * sel_stride_bytes;
    auto launch = [&](auto qb) {
      launch_select<decltype(qb)::value>(wide, grid, s, num_rows, W, sh.log_pw, log_g, nq, sp,
                                         sel_stride_bytes, dd, ws);
    };
    // The smallest instance that holds the pass's queries.
    if (nq > 8) launch(std::integral_constant<int, 16>{});
    else if (nq > 4) launch(std::integral_constant<int, 8>{});
    else if (nq > 2) launch(std::integral_constant<int, 4>{});
    else if (nq > 1) launch(std::integral_constant<int, 2>{});
    else launch(std::integral_constant<int, 1>{});
    HIP_TRY(hipGetLastError());
    const int row_words = nq * W;
    hipLaunchKernelGGL(select_fold_kernel, dim3((row_words + kFoldCols - 1) / kFoldCols),
                       dim3(kFoldCols * kFoldRows), 0, s, row_words, accumulate, ws,
                       static_cast<uint64_t*>(out) + (int64_t)q0 * W);
    HIP_TRY(hipGetLastError());
  }
  g_select_shape[0] = sh.tile, g_select_shape[1] = passes, g_select_shape[2] = gx * sh.chunks;
  g_last_dot = "select";
  return kOk;
}

}  // extern "C"
