// dpf_dot_buckets.hip -- the segmented fold of multi-query PIR over a bucketed
// database, behind dpf_hip_dot_buckets (include/dpf_hip.h; DESIGN.md section
// 6j): every key k has one 64-bit share per row of its bucket b(k), and
//   out[k] = sum_i y_k[i] * db[b(k)][i] mod 2^64 (uint64_t) or
//            XOR_i (y_k[i] & db[b(k)][i]) (XorWrapper<uint64_t>).
// dot_rows_batch_kernel's layout (dpf_dot_batch.hip) with a bucket in the work
// item: a record's words lie along the lanes, a lane keeps one accumulator
// per key of its tile, and the shares of a group of 64 rows are loaded once
// and handed between lanes.  A workgroup takes (bucket, tile of at most 16 of
// the bucket's keys, block of the bucket's rows, chunk of 64 columns): the
// keys of a tile share the pass over the slice, an empty bucket has no work
// item, and a tile never spans two buckets.
//
// Sums mod 2^64 and XOR are associative and commutative, so the result does
// not depend on the order the hardware folds in.  The row blocks of one tile
// meet in `out` by 64-bit atomics after a stream-ordered clear (dpf_lookup's
// convention); a call whose slices fit one block each stores plainly and
// clears nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../../include/dpf_hip.h"
#include "dpf_runtime.h"

using namespace dpf_rt;

namespace {

constexpr int kBktBlock = 256;     // four waves
constexpr int kBktWaves = kBktBlock / 64;
constexpr int kBktUnroll = 4;      // rows a lane has in flight
constexpr int kBktMaxTile = 16;    // keys a lane accumulates at once
constexpr int kBktClasses = 5;     // kernel instances: tiles of up to 1, 2, 4, 8, 16 keys
// Workgroups a call spreads its slices over: with fewer (tile, column chunk)
// pairs than this, the rows of a slice are cut into blocks (of whole steps of
// kBktBlock rows).  A constant, so that the workspace size is a pure function
// of the counts: eight workgroups for each of 256 compute units.
constexpr int64_t kBktTargetGroups = 2048;
constexpr int kBktMaxLogDomain = 24;
constexpr int64_t kBktMaxBuckets = (int64_t)1 << 20;

thread_local int64_t g_buckets_shape[4] = {0, 0, 0, 0};

// One work item; blockIdx.y adds the column chunk.
struct BucketItem {
  int32_t bucket, key0, nkeys, block;
};
static_assert(sizeof(BucketItem) == 16, "the workspace holds 16 bytes per work item");

// Record word (j, w) of a slice of n rows, or the nearest word that exists for
// a row or column that does not: the load is unconditional.  A row past n
// meets a share of zero, and the lanes of a column past W are dropped at the
// end.
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

// Workgroup x takes items[x]: rows [block * block_rows, (block + 1) *
// block_rows) of slice db[bucket] (n rows of W words) against the nq <= QB
// keys key0 .. key0 + nq - 1 (the accumulators beyond nq repeat key nq - 1 and
// are dropped).  The lane layout and the share hand-over are
// dot_rows_batch_kernel's: a record's W words lie along PW = 2^log_pw lanes,
// its RW = 64 / PW rows per step are consecutive, a wave takes whole groups of
// 64 rows and reads the shares of a group once, lane l holding y_q[64 g + l].
// block_rows is a multiple of kBktBlock.
template <int QB, bool XOR>
__global__ __launch_bounds__(kBktBlock) void dot_buckets_kernel(
    int64_t n, int64_t block_rows, int W, int log_pw, int atomic,
    const BucketItem* __restrict__ items, const char* __restrict__ y, int64_t y_stride,
    const uint64_t* __restrict__ db_all, uint64_t* __restrict__ out) {
  constexpr int U = kBktUnroll;
  __shared__ uint64_t red[QB][64];
  const BucketItem it = items[blockIdx.x];
  const int nq = it.nkeys;
  const uint64_t* __restrict__ db = db_all + (int64_t)it.bucket * n * W;
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int PW = 1 << log_pw, log_rw = 6 - log_pw;
  const int sub = lane >> log_pw;
  const int w = (int)blockIdx.y * PW + (lane & (PW - 1));
  const bool col_ok = w < W;
  const uint64_t* row[QB];
#pragma unroll
  for (int q = 0; q < QB; ++q)
    row[q] = reinterpret_cast<const uint64_t*>(
        y + (int64_t)(it.key0 + (q < nq ? q : nq - 1)) * y_stride);
  uint64_t acc[QB];
#pragma unroll
  for (int q = 0; q < QB; ++q) acc[q] = 0;

  const int64_t r0 = (int64_t)it.block * block_rows;
  const int64_t r1 = r0 + block_rows < n ? r0 + block_rows : n;
  const int64_t g1 = (r1 + 63) >> 6;
  for (int64_t g = (r0 >> 6) + wave; g < g1; g += kBktWaves) {
    const int64_t j0 = g << 6;
    const bool y_ok = j0 + lane < n;
    const int64_t jy = y_ok ? j0 + lane : n - 1;   // the load is unconditional
    uint64_t yv[QB];
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      const uint64_t v = row[q][jy];
      yv[q] = y_ok ? v : 0;
    }
    // kBktUnroll steps' loads issued before the first product; narrow records
    // (PW < kBktUnroll) have fewer steps: the spare loads repeat the last
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
  for (int v = 1; v < kBktWaves; ++v) {
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
  if (wave != 0 || lane >= PW || !col_ok) return;
  uint64_t* o = out + (int64_t)it.key0 * W + w;
#pragma unroll
  for (int q = 0; q < QB; ++q) {
    if (q >= nq) break;
    if (atomic) {
      // Several row blocks per tile: 64-bit atomics onto the rows the call
      // cleared in stream order.  Both groups are exact in any order.
      unsigned long long* p = reinterpret_cast<unsigned long long*>(o + (int64_t)q * W);
      if (XOR) __hip_atomic_fetch_xor(p, (unsigned long long)acc[q], __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
      else __hip_atomic_fetch_add(p, (unsigned long long)acc[q], __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
    } else {
      o[(int64_t)q * W] = acc[q];
    }
  }
}

// Shape of a call, a pure function of its counts: the lanes a record lies
// along, the column chunks (grid y) and the rows of a block.
struct BucketsShape {
  int log_pw, chunks;
  int64_t blocks, block_rows;
};
BucketsShape buckets_shape(int W, int64_t N, int64_t tiles) {
  BucketsShape s{0, 1, 1, N};
  while ((1 << s.log_pw) < W && s.log_pw < 6) ++s.log_pw;
  s.chunks = (W + 63) / 64;
  const int64_t pairs = (tiles < 1 ? 1 : tiles) * s.chunks;
  int64_t blocks = (kBktTargetGroups + pairs - 1) / pairs;
  const int64_t steps = (N + kBktBlock - 1) / kBktBlock;   // a block is whole steps
  if (blocks > steps) blocks = steps;
  const int64_t block_steps = (steps + blocks - 1) / blocks;
  s.block_rows = block_steps * kBktBlock;
  s.blocks = (steps + block_steps - 1) / block_steps;
  return s;
}

// The most tiles num_keys keys in num_buckets buckets make: every bucket adds
// at most one tile that is not full.
int64_t max_tiles(int64_t num_buckets, int64_t num_keys) {
  return num_keys / kBktMaxTile + (num_buckets < num_keys ? num_buckets : num_keys);
}
// tiles * blocks <= kBktTargetGroups + tiles (blocks <= target / tiles + 1).
int64_t workspace_bytes(int64_t num_buckets, int64_t num_keys) {
  return (kBktTargetGroups + max_tiles(num_buckets, num_keys)) * (int64_t)sizeof(BucketItem);
}

bool counts_ok(int64_t num_buckets, int log_domain_size, int record_words, int64_t num_keys) {
  if (num_buckets < 1 || num_buckets > kBktMaxBuckets) {
    fail(kInvalidArgument, "num_buckets must be in [1, 2^20]");
    return false;
  }
  if (log_domain_size < 1 || log_domain_size > kBktMaxLogDomain) {
    fail(kInvalidArgument, "log_domain_size must be in [1, 24]");
    return false;
  }
  if (record_words < 1 || record_words > DPF_HIP_DOT_MAX_RECORD_WORDS) {
    fail(kInvalidArgument, "record_words must be in [1, 1024]");
    return false;
  }
  if (num_keys < 0 || num_keys > INT32_MAX) {
    fail(kInvalidArgument, "num_keys out of range");
    return false;
  }
  return true;
}

// kOk and whether the group is XOR for uint64_t and XorWrapper<uint64_t>.
int buckets_type(const dpf_value_desc* desc, int* xor_type) {
  int words = 0;
  if (dot_type(desc, &words, xor_type) != kOk || words != 1)
    return fail(kUnimplemented,
                "the bucketed database fold is implemented for uint64_t and "
                "XorWrapper<uint64_t> only");
  return kOk;
}

int tile_class(int nkeys) {   // the smallest instance that holds the tile
  int c = 0;
  while ((1 << c) < nkeys) ++c;
  return c;
}

template <int QB>
void launch_class(bool xor_type, dim3 grid, hipStream_t s, int64_t n, int64_t block_rows, int W,
                  int log_pw, int atomic, const BucketItem* items, const char* y, int64_t stride,
                  const uint64_t* db, uint64_t* out) {
  if (xor_type)
    hipLaunchKernelGGL((dot_buckets_kernel<QB, true>), grid, dim3(kBktBlock), 0, s, n, block_rows,
                       W, log_pw, atomic, items, y, stride, db, out);
  else
    hipLaunchKernelGGL((dot_buckets_kernel<QB, false>), grid, dim3(kBktBlock), 0, s, n,
                       block_rows, W, log_pw, atomic, items, y, stride, db, out);
}

}  // namespace

extern "C" {

int64_t dpf_hip_dot_buckets_workspace_bytes(const dpf_value_desc* desc, int record_words,
                                            int64_t num_buckets, int64_t num_keys,
                                            int log_domain_size) {
  int xor_type = 0;
  if (!counts_ok(num_buckets, log_domain_size, record_words, num_keys)) return -1;
  if (!desc) {
    fail(kInvalidArgument, "NULL value descriptor");
    return -1;
  }
  if (buckets_type(desc, &xor_type)) return -1;
  return workspace_bytes(num_buckets, num_keys);
}

int dpf_hip_last_dot_buckets_shape(int64_t out[4]) {
  if (!out) return fail(kInvalidArgument, "NULL pointer");
  for (int i = 0; i < 4; ++i) out[i] = g_buckets_shape[i];
  return kOk;
}

int dpf_hip_dot_buckets(int64_t num_buckets, int log_domain_size, int record_words,
                        const int64_t* bucket_begin, int64_t num_keys,
                        const dpf_value_desc* desc, const void* y, int64_t y_stride_bytes,
                        const void* db, uint64_t* out, void* workspace, int64_t workspace_bytes_in,
                        void* stream) {
  if (!counts_ok(num_buckets, log_domain_size, record_words, num_keys)) return kInvalidArgument;
  if (!desc) return fail(kInvalidArgument, "NULL value descriptor");
  int xor_type = 0;
  if (int st = buckets_type(desc, &xor_type)) return st;
  if (!bucket_begin) return fail(kInvalidArgument, "NULL bucket_begin");
  if (bucket_begin[0] != 0) return fail(kInvalidArgument, "bucket_begin must start at 0");
  for (int64_t b = 0; b < num_buckets; ++b)
    if (bucket_begin[b + 1] < bucket_begin[b])
      return fail(kInvalidArgument, "bucket_begin must be nondecreasing");
  if (bucket_begin[num_buckets] != num_keys)
    return fail(kInvalidArgument, "bucket_begin must end at num_keys");
  const int64_t N = (int64_t)1 << log_domain_size;
  if (y_stride_bytes < 0 || y_stride_bytes % 16 != 0 || y_stride_bytes < 8 * N)
    return fail(kInvalidArgument,
                "y_stride_bytes must be a multiple of 16 and at least 8 * 2^log_domain_size");
  if (num_keys == 0) return kOk;
  if (!y || !db || !out) return fail(kInvalidArgument, "NULL pointer");
  const int64_t need = workspace_bytes(num_buckets, num_keys);
  if (!workspace || workspace_bytes_in < need)
    return fail(kResourceExhausted, "the bucketed database fold needs a workspace of " +
                                        std::to_string(need) + " bytes");
  if (((uintptr_t)y & 15) != 0 || ((uintptr_t)workspace & 15) != 0 || ((uintptr_t)db & 7) != 0 ||
      ((uintptr_t)out & 7) != 0)
    return fail(kInvalidArgument,
                "`y` and `workspace` must be aligned to 16 bytes, `db` and `out` to 8");

  const int W = record_words;
  // The tiles, then the work items class by class (a class is one kernel
  // instance: tiles of up to 1, 2, 4, 8, 16 keys), a tile's row blocks
  // consecutive.
  int64_t tiles = 0, largest = 0;
  int64_t class_tiles[kBktClasses] = {0, 0, 0, 0, 0};
  for (int64_t b = 0; b < num_buckets; ++b)
    for (int64_t k = bucket_begin[b]; k < bucket_begin[b + 1]; k += kBktMaxTile) {
      const int64_t nk = bucket_begin[b + 1] - k < kBktMaxTile ? bucket_begin[b + 1] - k
                                                               : (int64_t)kBktMaxTile;
      ++class_tiles[tile_class((int)nk)];
      ++tiles;
      if (nk > largest) largest = nk;
    }
  const BucketsShape sh = buckets_shape(W, N, tiles);
  int64_t class_first[kBktClasses + 1];
  class_first[0] = 0;
  for (int c = 0; c < kBktClasses; ++c) class_first[c + 1] = class_first[c] + class_tiles[c] * sh.blocks;
  const int64_t num_items = class_first[kBktClasses];
  if (num_items * (int64_t)sizeof(BucketItem) > need)
    return fail(kInternal, "work-item table larger than its bound");
  std::vector<BucketItem> table((size_t)num_items);
  int64_t fill[kBktClasses];
  for (int c = 0; c < kBktClasses; ++c) fill[c] = class_first[c];
  for (int64_t b = 0; b < num_buckets; ++b)
    for (int64_t k = bucket_begin[b]; k < bucket_begin[b + 1]; k += kBktMaxTile) {
      const int64_t nk = bucket_begin[b + 1] - k < kBktMaxTile ? bucket_begin[b + 1] - k
                                                               : (int64_t)kBktMaxTile;
      const int c = tile_class((int)nk);
      for (int64_t r = 0; r < sh.blocks; ++r)
        table[(size_t)fill[c]++] = BucketItem{(int32_t)b, (int32_t)k, (int32_t)nk, (int32_t)r};
    }

  hipStream_t s = (hipStream_t)stream;
  // The table is pageable host memory: the copy has left it when the call
  // returns, and is ordered on the stream before the kernels.
  HIP_TRY(hipMemcpyAsync(workspace, table.data(), (size_t)num_items * sizeof(BucketItem),
                         hipMemcpyHostToDevice, s));
  const int atomic = sh.blocks > 1 ? 1 : 0;
  if (atomic) HIP_TRY(hipMemsetAsync(out, 0, (size_t)num_keys * W * sizeof(uint64_t), s));
  const BucketItem* items = static_cast<const BucketItem*>(workspace);
  const char* yy = static_cast<const char*>(y);
  const uint64_t* dd = static_cast<const uint64_t*>(db);
  for (int c = 0; c < kBktClasses; ++c) {
    const int64_t cnt = class_first[c + 1] - class_first[c];
    if (cnt == 0) continue;
    const dim3 grid((unsigned)cnt, (unsigned)sh.chunks);
    auto launch = [&](auto qb) {
      launch_class<decltype(qb)::value>(xor_type != 0, grid, s, N, sh.block_rows, W, sh.log_pw,
                                        atomic, items + class_first[c], yy, y_stride_bytes, dd,
                                        out);
    };
    if (c == 0) launch(std::integral_constant<int, 1>{});
    else if (c == 1) launch(std::integral_constant<int, 2>{});
    else if (c == 2) launch(std::integral_constant<int, 4>{});
    else if (c == 3) launch(std::integral_constant<int, 8>{});
    else launch(std::integral_constant<int, 16>{});
    HIP_TRY(hipGetLastError());
  }
  g_buckets_shape[0] = num_items, g_buckets_shape[1] = tiles, g_buckets_shape[2] = largest,
  g_buckets_shape[3] = sh.chunks;
  g_last_dot = "buckets";
  return kOk;
}

}  // extern "C"
