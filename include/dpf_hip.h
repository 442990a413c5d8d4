/*
 * dpf_hip.h -- C ABI of the MI355X (gfx950) DPF evaluation engine.
 *
 * This is the drop-in seam between a host DistributedPointFunction and the
 * HIP kernels.  It replaces the reference's CPU hot loops:
 *
 *   dpf_hip_hash        <- Aes128FixedKeyHash::Evaluate
 *                          (dpf/aes_128_fixed_key_hash.h:51-52, .cc:47-85)
 *   dpf_hip_eval_paths  <- dpf_internal::EvaluateSeeds
 *                          (dpf/internal/evaluate_prg_hwy.h:58-64, .cc:495-506)
 *   dpf_hip_expand      <- DistributedPointFunction::ExpandSeeds + HashExpandedSeeds
 *                          + the EvaluateUntil value-correction loop, fused
 *                          (dpf/distributed_point_function.cc:271-349, 500-524;
 *                           dpf/distributed_point_function.h:785-808)
 *   dpf_hip_eval_points <- EvaluateAtImpl's EvaluateSeeds + HashExpandedSeeds +
 *                          per-point correction, fused, for one or many keys
 *                          (dpf/distributed_point_function.h:839-1010)
 *
 * Conventions
 *   - Every function returns an int status: 0 = OK, otherwise the absl status
 *     code number (3 INVALID_ARGUMENT, 8 RESOURCE_EXHAUSTED, 12 UNIMPLEMENTED,
 *     13 INTERNAL).  dpf_hip_last_error() returns a message for the last failure
 *     on the calling thread.
 *   - All array pointers passed to compute entry points are DEVICE pointers,
 *     caller-owned.  Allocation only crosses the ABI through dpf_hip_alloc /
 *     dpf_hip_free; copies through dpf_hip_memcpy_*.
 *   - A 128-bit block (dpf_block) is the absl::uint128 memory image:
 *     {low, high}, little-endian.  Booleans are one byte (0/1).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Compute
 *     entry points are asynchronous on that stream (no host synchronisation);
 *     dpf_hip_stream_sync() waits.
 *   - Not thread-safe per stream (the reference is single-threaded too,
 *     dpf/aes_128_fixed_key_hash.h:77).
 */
#ifndef DPF_HIP_H_
#define DPF_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPF_HIP_ABI_VERSION 2
#define DPF_MAX_LEAVES 16

typedef struct dpf_block {
  uint64_t low;
  uint64_t high;
} dpf_block;

/* One fixed AES-128 key: the 16-byte memory image of the uint128 key
 * (aes_128_fixed_key_hash.cc:38-40). */
typedef struct dpf_aes_key {
  uint8_t bytes[16];
} dpf_aes_key;

/* Leaf kinds of a flattened ValueType (distributed_point_function.proto:25-60). */
enum dpf_leaf_kind { DPF_LEAF_INT = 0, DPF_LEAF_INTMODN = 1, DPF_LEAF_XOR = 2 };

/* A ValueType flattened into its integer leaves in declaration order, plus the
 * per-hierarchy-level sampling parameters the host computed:
 *   direct            CanBeConvertedDirectly (value_type_helpers.h:342-344)
 *   elements_per_block ElementsPerBlock<T>() (value_type_helpers.h:508-520)
 *   blocks_needed     ceil(BitsNeeded / 128) (distributed_point_function.cc:578-587) */
typedef struct dpf_value_desc {
  int32_t num_leaves;
  int32_t direct;
  int32_t elements_per_block;
  int32_t blocks_needed;
  int32_t kind[DPF_MAX_LEAVES];
  int32_t bits[DPF_MAX_LEAVES];
  uint64_t mod_low[DPF_MAX_LEAVES];
  uint64_t mod_high[DPF_MAX_LEAVES];
} dpf_value_desc;

/* ---- runtime / memory ---------------------------------------------------- */
int dpf_hip_abi_version(void);
const char* dpf_hip_last_error(void);
int dpf_hip_device_count(int* count);
int dpf_hip_set_device(int device);
int dpf_hip_alloc(void** ptr, size_t bytes);
int dpf_hip_free(void* ptr);
/* Free and total device memory of the current device (hipMemGetInfo). */
int dpf_hip_mem_info(size_t* free_bytes, size_t* total_bytes);
int dpf_hip_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
/* Page-locked host memory, and an H2D copy that does not wait: `src` must be
 * page-locked (dpf_hip_host_alloc) and stay unchanged until `stream` has run
 * the copy.  The host API stages its small per-call uploads this way. */
int dpf_hip_host_alloc(void** ptr, size_t bytes);
int dpf_hip_host_free(void* ptr);
int dpf_hip_memcpy_h2d_async(void* dst, const void* src, size_t bytes, void* stream);
int dpf_hip_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
/* D2H copy into FRESH host storage that the caller initialises chunk by chunk
 * (e.g. a std::vector<T> being value-initialised by resize): before each
 * chunk's DMA, `before_chunk(ctx, bytes_ready)` is called and must make
 * [0, bytes_ready) of `dst` valid; the DMA of one chunk overlaps the
 * initialisation of the next.  Large copies DMA straight into `dst`
 * (registered for the copy; a fresh pageable range is mapped and registered
 * piece by piece on a helper thread while the DMA fills the pieces already
 * registered), others go through page-locked staging.  The drop-in
 * EvaluateUntil<T> returns its std::vector<T> this way. */
/* FRESH host ranges (pages not yet mapped) of at least this many bytes are
 * registered (page-locked) for a copy and DMAed straight into; smaller ones go
 * through page-locked staging.  Ranges whose pages are already mapped (every
 * dpf_hip_memcpy_h2d source; dpf_hip_memcpy_d2h destinations the caller has
 * touched) are registered from 32 MiB. */
#define DPF_HIP_REGISTER_MIN_BYTES ((size_t)512 << 20)

/* D2H copy handed to the host chunk by chunk: the bytes arrive in the
 * library's page-locked staging buffers, and `consume(ctx, chunk, offset,
 * len)` gets [offset, offset + len) of the source (len a multiple of `align`,
 * <= 16 MiB) while the next chunk's DMA runs.  Returns after the last
 * consume.  The drop-in EvaluateUntil<T> unpacks packed tuples / IntModN
 * values straight into its result vector this way (no host copy of the packed
 * bytes), and mid-sized integer outputs are copied into theirs. */
int dpf_hip_memcpy_d2h_chunked(const void* src, size_t bytes, size_t align,
                               void (*consume)(void* ctx, const void* chunk, size_t offset,
                                               size_t len),
                               void* ctx, void* stream);
int dpf_hip_memcpy_d2h_staged(void* dst, const void* src, size_t bytes,
                              void (*before_chunk)(void* ctx, size_t bytes_ready), void* ctx,
                              void* stream);
/* _staged for a source produced in parts on `stream`: [0, part_end_bytes[j])
 * of `src` is complete once part_events[j] (dpf_hip_event_record on `stream`)
 * has completed (ends non-decreasing, the last >= bytes).  A fresh pageable
 * `dst` of >= DPF_HIP_REGISTER_MIN_BYTES is copied on a stream of the call's
 * own, each DMA chunk waiting on the device for the first part that covers
 * it, so the copy of part j overlaps the kernels producing the later parts;
 * every other destination is copied on `stream` after all parts.  The
 * drop-in EvaluateUntil<T> returns a >= 512 MiB first-call output this way,
 * its expansion launched as 8 subtrees. */
int dpf_hip_memcpy_d2h_staged_after(void* dst, const void* src, size_t bytes,
                                    void (*before_chunk)(void* ctx, size_t bytes_ready), void* ctx,
                                    int num_parts, void* const* part_events,
                                    const size_t* part_end_bytes, void* stream);
int dpf_hip_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
int dpf_hip_memset(void* dst, int value, size_t bytes, void* stream);
int dpf_hip_stream_sync(void* stream);
/* Waits for an event (dpf_hip_event_create/record, declared with the timing
 * helpers below).  The host API marks the end of the work that reads its
 * staging buffers with one, so reusing them never depends on the caller's
 * stream still existing. */
int dpf_hip_event_sync(void* event);
/* Makes later work on `stream` wait for `event` on the device (no host wait). */
int dpf_hip_stream_wait_event(void* stream, void* event);
/* Packed size in bytes of one output element: sum of leaf bits / 8. */
int dpf_hip_packed_element_size(const dpf_value_desc* desc);

/* ---- a1: out[i] = AES_key(sigma(in[i])) ^ sigma(in[i]) --------------------
 * Replaces Aes128FixedKeyHash::Evaluate (aes_128_fixed_key_hash.cc:47-85).
 * in/out may alias. */
int dpf_hip_hash(int64_t n, const dpf_block* in, const dpf_aes_key* key,
                 dpf_block* out, void* stream);

/* ---- a9: path evaluation --------------------------------------------------
 * Replaces dpf_internal::EvaluateSeeds (evaluate_prg_hwy.h:58-64).  For each
 * seed i and level j < num_levels: bit = (paths[i] >> (num_levels-1-j)) & 1,
 * s = H_{bit ? right : left}(s); if t: s ^= cw_seed[j]; t' = s & 1; s &= ~1;
 * if t: t' ^= bit ? cw_right[j] : cw_left[j].  Outputs may alias inputs.
 * With num_levels == 0 the inputs are copied to the outputs. */
int dpf_hip_eval_paths(int64_t num_seeds, int num_levels, const dpf_block* seeds_in,
                       const uint8_t* control_in, const dpf_block* paths,
                       const dpf_block* cw_seed, const uint8_t* cw_left,
                       const uint8_t* cw_right, const dpf_aes_key* key_left,
                       const dpf_aes_key* key_right, dpf_block* seeds_out,
                       uint8_t* control_out, void* stream);

/* ---- a4+a5+a6+a12+a13: fused subtree expansion + leaf hashing/correction ---
 * Replaces ExpandSeeds (cc:271-349) + HashExpandedSeeds (cc:500-524) + the
 * EvaluateUntil correction loop (h:785-808).  Expands each of num_starts
 * (seed, control) pairs through num_levels levels (child 2j = left, 2j+1 =
 * right), hashes every leaf seed with key_value into desc->blocks_needed blocks
 * (seed + j), converts them to desc->elements_per_block elements, keeps the
 * first `elements_per_leaf` (= corrected_elements_per_block), adds
 * value_correction (elements_per_block * num_leaves dpf_blocks, one per leaf
 * value) when the leaf's control bit is set and negates when party == 1.
 * Writes (num_starts << num_levels) * elements_per_leaf packed elements to
 * `out` in expansion order. */
int dpf_hip_expand(int64_t num_starts, const dpf_block* seeds_in, const uint8_t* control_in,
                   int num_levels, const dpf_block* cw_seed, const uint8_t* cw_left,
                   const uint8_t* cw_right, const dpf_aes_key* key_left,
                   const dpf_aes_key* key_right, const dpf_aes_key* key_value,
                   const dpf_value_desc* desc, int elements_per_leaf,
                   const dpf_block* value_correction, int party, void* out, void* stream);

/* ---- full-domain expansion folded into a database (two-server PIR) ---------
 * No reference counterpart: the reference returns the share vector and leaves
 * the fold to its caller.  With y[0 .. n) what dpf_hip_expand writes for the
 * same arguments (n = (num_starts << num_levels) * elements_per_leaf) and `db`
 * a row-major device array of n records of record_words words of the value
 * type's width,
 *   uint64_t:                        out[w] = sum_i y[i] * db[i*W + w] (mod 2^64)
 *   XorWrapper<uint64_t / uint128>:  out[w] = XOR_i (y[i] & db[i*W + w]).
 * Both maps are linear in the type's group, so the two parties' results
 * combine with its + to beta * db[alpha] (beta & db[alpha]); sums mod 2^64
 * and XOR commute, so the result is bit-exact whatever the order.  Every
 * other value type: 12 UNIMPLEMENTED.  `out` gets record_words packed
 * elements.  `workspace` (device, dpf_hip_expand_dot_workspace_bytes) holds
 * one partial row per workgroup, written with plain stores (no atomics) and
 * folded by a second small kernel; the calls do not depend on what it held
 * before.
 *
 * dpf_hip_expand_dot: dpf_hip_expand's kernels with the leaf's stores
 * replaced by the product, accumulated in registers (no share vector is
 * written).  Only for the widths dpf_hip_expand_dot_fused reports (today
 * record_words == 1); others: 12 UNIMPLEMENTED -- expand into scratch and
 * call dpf_hip_dot_rows per slab, as EvaluateDotToDevice does. */
#define DPF_HIP_DOT_MAX_RECORD_WORDS 1024
int dpf_hip_expand_dot(int64_t num_starts, const dpf_block* seeds_in, const uint8_t* control_in,
                       int num_levels, const dpf_block* cw_seed, const uint8_t* cw_left,
                       const uint8_t* cw_right, const dpf_aes_key* key_left,
                       const dpf_aes_key* key_right, const dpf_aes_key* key_value,
                       const dpf_value_desc* desc, int elements_per_leaf,
                       const dpf_block* value_correction, int party, const void* db,
                       int record_words, void* workspace, void* out, void* stream);
/* out[w] (+)= the fold of y[0 .. num_rows) (packed elements, device) into
 * db[0 .. num_rows)[record_words]; accumulate != 0 combines with out's old
 * value (the next slab of a streamed fold), else out is overwritten.
 * Bandwidth-bound: a record's words lie along the lanes, several rows per
 * wave for narrow records.  record_words need not be a power of two. */
int dpf_hip_dot_rows(int64_t num_rows, int record_words, const dpf_value_desc* desc,
                     const void* y, const void* db, int accumulate, void* workspace, void* out,
                     void* stream);
/* Bytes of workspace either call needs for this type and width (-1 and a
 * last error for an unsupported type or width).  No device is touched. */
int dpf_hip_expand_dot_workspace_bytes(const dpf_value_desc* desc, int record_words);
/* 1 when dpf_hip_expand_dot has a fused kernel for this type and width, else
 * 0.  DPF_DOT_STREAM=1 (read per call; A/B and test hook) turns it off. */
int dpf_hip_expand_dot_fused(const dpf_value_desc* desc, int record_words);
/* Diagnostic: the path the calling thread's last dot call took: "small",
 * "pair" or "octet" (dpf_hip_expand_dot, the expand kernel it ran), "rows"
 * (dpf_hip_dot_rows), "select" (dpf_hip_select_rows), "rows_batch"
 * (dpf_hip_dot_rows_batch) or "buckets" (dpf_hip_dot_buckets); "" before the
 * first call. */
const char* dpf_hip_last_dot_kernel(void);

/* ---- dense PIR: a bit-selected database fold batched over queries ----------
 * No reference counterpart.  `db` is a row-major device array of num_rows
 * records of record_words uint64 words; row q of `sel` (device, at sel +
 * q * sel_stride_bytes) is query q's bit vector, bit j = (byte[j >> 3] >>
 * (j & 7)) & 1 -- the packed output of dpf_hip_expand for XorWrapper<uint64_t
 * / uint128>, 128 records per leaf block.  For q < num_queries, w < W:
 *   out[q*W + w] (^)= XOR over { j < num_rows : bit j of row q } of db[j*W + w]
 * (accumulate != 0 XORs into out's old value -- the next slab of a streamed
 * fold --, else out is overwritten; num_rows == 0 is an empty XOR).  The
 * database is read once per tile of queries (dpf_hip_last_select_shape), not
 * once per query.  num_rows is arbitrary; bits at positions >= num_rows are
 * ignored whatever they hold.  sel_stride_bytes: a multiple of 16 and at
 * least ceil(num_rows / 8).  record_words in [1, DPF_HIP_DOT_MAX_RECORD_WORDS],
 * num_queries in [1, DPF_HIP_SELECT_MAX_QUERIES]; else 3 INVALID_ARGUMENT.
 * `workspace` (device, dpf_hip_select_workspace_bytes) holds one partial
 * [tile][record_words] per workgroup, written with plain stores (no atomics)
 * and folded by a second small kernel; the call does not depend on what it
 * held before.  dpf_hip_last_dot_kernel reports "select" after this call. */
#define DPF_HIP_SELECT_MAX_QUERIES 64
int dpf_hip_select_rows(int64_t num_rows, int record_words, int num_queries, const void* sel,
                        int64_t sel_stride_bytes, const void* db, int accumulate, void* workspace,
                        void* out, void* stream);
/* Bytes of workspace the call needs (-1 and a last error for arguments out of
 * range).  No device is touched. */
int dpf_hip_select_workspace_bytes(int record_words, int num_queries);
/* Diagnostic: the shape of the calling thread's last dpf_hip_select_rows:
 * {queries per tile, passes over the database = ceil(num_queries / tile),
 * workgroups of one pass}. */
int dpf_hip_last_select_shape(int64_t* out3);

/* ---- additive-share PIR: a word-weighted database fold batched over queries -
 * No reference counterpart.  The word-valued sibling of dpf_hip_select_rows:
 * `db` is a row-major device array of num_rows records of record_words uint64
 * words; row q of `y` (device, at y + q * y_stride_bytes) is query q's share
 * vector, num_rows packed 8-byte elements -- the packed output of
 * dpf_hip_expand for uint64_t or XorWrapper<uint64_t>.  For q < num_queries,
 * w < W:
 *   uint64_t:              out[q*W + w] (+)= sum_i y_q[i] * db[i*W + w] (mod 2^64)
 *   XorWrapper<uint64_t>:  out[q*W + w] (^)= XOR_i (y_q[i] & db[i*W + w])
 * (accumulate != 0 combines with out's old value -- the next slab of a
 * streamed fold --, else out is overwritten; num_rows == 0 is an empty sum).
 * Row q is what dpf_hip_dot_rows writes for y_q, bit for bit: both maps are
 * exact in any order.  The database is read once per tile of queries
 * (dpf_hip_last_dot_batch_shape), not once per query.  num_rows is arbitrary
 * and record_words need not be a power of two.  Checked in this order, before
 * any device call:
 *   record_words in [1, DPF_HIP_DOT_MAX_RECORD_WORDS], num_queries in [1,
 *   DPF_HIP_DOT_BATCH_MAX_QUERIES], num_rows in range; desc, out and (for
 *   num_rows > 0) y and db not NULL; y_stride_bytes a multiple of 16 and at
 *   least 8 * num_rows: else 3 INVALID_ARGUMENT;
 *   a value type other than uint64_t or XorWrapper<uint64_t>: 12
 *   UNIMPLEMENTED (no fallback);
 *   no workspace: 8 RESOURCE_EXHAUSTED, naming the bytes it needs.
 * `workspace` (device, dpf_hip_dot_rows_batch_workspace_bytes) holds one
 * partial [tile][record_words] per workgroup, written with plain stores (no
 * atomics) and folded by a second small kernel; the call does not depend on
 * what it held before.  Asynchronous on `stream`; allocates nothing.
 * dpf_hip_last_dot_kernel reports "rows_batch" after this call. */
#define DPF_HIP_DOT_BATCH_MAX_QUERIES 64
int dpf_hip_dot_rows_batch(int64_t num_rows, int record_words, int num_queries,
                           const dpf_value_desc* desc, const void* y, int64_t y_stride_bytes,
                           const void* db, int accumulate, void* workspace, void* out,
                           void* stream);
/* Bytes of workspace the call needs; never less for a larger record_words or
 * num_queries (-1 and a last error for counts out of range or an unsupported
 * type).  No device is touched. */
int dpf_hip_dot_rows_batch_workspace_bytes(const dpf_value_desc* desc, int record_words,
                                           int num_queries);
/* Diagnostic: the shape of the calling thread's last dpf_hip_dot_rows_batch:
 * {queries per tile, passes over the database = ceil(num_queries / tile),
 * workgroups of one pass}. */
int dpf_hip_last_dot_batch_shape(int64_t* out3);

/* Diagnostic: which kernel the calling thread's last successful dpf_hip_expand
 * launched ("octet/<leaf>" or "pair/<leaf>", leaf = fast, swar, mod32,
 * generic; "" before the first call), and the depth-first subtree depth it
 * chose.  Tests use it to pin the dispatch. */
const char* dpf_hip_last_expand_kernel(int* subtree_depth);

/* Diagnostic (bench.py): the sustained shader clock of the expand launches
 * themselves.  dpf_hip_clock_probe(1) allocates and zeroes a device
 * accumulator on the current device; from then on wave 0 of every
 * workgroup of every octet expand launch (the full-domain kernel) adds its
 * s_memtime (shader clocks) and s_memrealtime (100 MHz) deltas around its
 * work into it -- two stamps per workgroup, nothing on the outputs' path.
 * dpf_hip_clock_probe_read waits for the device, returns the clock in GHz
 * (sum of shader-clock deltas / sum of real-time deltas), the number of
 * stamped workgroups and their mean duration in seconds, and zeroes the
 * accumulator.  dpf_hip_clock_probe(0) turns it off.  No reference
 * counterpart (SURVEY.md 8d asks for the sustained clock). */
int dpf_hip_clock_probe(int on);
int dpf_hip_clock_probe_read(double* clock_ghz, int64_t* workgroups, double* mean_workgroup_s);

/* Diagnostic: when the waves of the expand launches (octet and pair kernels)
 * left the kernel.  While the probe is on, lane 0 of every wave folds its
 * s_memrealtime exit stamp into the accumulator.  Waits for the device and
 * writes six doubles, times in seconds after the first workgroup's begin
 * stamp: out[0] first wave exit, out[1] last wave exit, out[2] / out[3] /
 * out[4] the earliest / latest / mean of the workgroups' last exits, out[5]
 * the number of workgroups seen (all zero when nothing was stamped).  The
 * stamps are absolute, so the figures describe one launch: call it after
 * each launch, then dpf_hip_clock_probe_read, which zeroes the accumulator
 * (this call does not). */
int dpf_hip_clock_probe_exits(double* out);

/* The chunk schedule dpf_hip_expand gives a launch of `num_items` subtrees
 * of depth `subtree_depth`, each `k0` levels below its start seed, with
 * `compute_units` workgroups and the kernel's minimum subtree depth (3 for
 * the octet kernel, 1 for the pair kernel); no device is touched, the
 * DPF_OCTET_* environment hooks are read.  Writes 15 values: out[0] the
 * levels taken off the subtrees for dynamic distribution (0: a static
 * launch, the rest is zero), out[1] whether the launch has one chunk counter
 * (else one per workgroup), out[2] the number of counters, then for each of
 * the three phases, in the order they are taken, the number of 64-item
 * chunks, the first item, the levels walked and the subtree depth of its
 * items (out[3 + 4 j] ..).  A phase without chunks is absent. */
int dpf_hip_octet_schedule(int64_t num_items, int k0, int subtree_depth, int min_depth,
                           int compute_units, int64_t* out);

/* Diagnostic: the chunk schedule the calling thread's last dpf_hip_expand
 * launch of the octet or pair kernel really ran with on its device, in
 * dpf_hip_octet_schedule's layout (out[0] == 0: a static launch, also when
 * the tree-top pass could not start the items).  Tests use it to pin that a
 * mode took the path it names. */
int dpf_hip_last_expand_schedule(int64_t* out);

/* Diagnostic: which kernel the calling thread's last
 * dpf_hip_prefix_batch_level launched: "hh_level" (the lean
 * heavy-hitters kernel: cached or gathered start seeds, two expanded levels,
 * IntModN<uint32_t> sums), "batch_level/fast", "batch_level/mod32" or
 * "batch_level/generic"; "" before the first call. */
const char* dpf_hip_last_batch_kernel(void);

/* Diagnostic: which point kernel the calling thread's last point evaluation
 * (dpf_hip_eval_points*, per key or summed) launched: "points/ilp4" (integer
 * leaves, four path chains per lane), "points/ilp2" (two) or "points/single"
 * (one, for launches below one wave per CU); "" before the first call. */
const char* dpf_hip_last_points_kernel(void);

/* Chunks of 64 items per workgroup chosen for the calling thread's most recent
 * launch that can distribute its work dynamically (0: a fixed grid-stride share). */
int dpf_hip_last_dynamic_chunks(int64_t* per_wg);

/* ---- a11: fused point evaluation for many keys ----------------------------
 * Replaces EvaluateAtImpl's path walk + hash + correction (h:930-1003).
 * Point i belongs to key k = i / points_per_key.  Its walk starts at
 * (seeds_in[i], control_in[i]) if seeds_in != NULL, else at the key's root
 * (key_seed[k], party[k]).  The path is tree_index[i] over num_levels levels
 * using key k's correction words cw_seed[k*num_levels + j], cw_left[...],
 * cw_right[...].  The element block_index[i] (NULL = 0) of the hashed leaf is
 * corrected with value_correction[k * E*num_leaves ...] and negated if
 * party[k] == 1, then written packed to out[i]. */
int dpf_hip_eval_points(int64_t num_points, int64_t points_per_key, int num_levels,
                        const dpf_block* key_seed, const uint8_t* party,
                        const dpf_block* seeds_in, const uint8_t* control_in,
                        const dpf_block* tree_index, const int32_t* block_index,
                        const dpf_block* cw_seed, const uint8_t* cw_left,
                        const uint8_t* cw_right, const dpf_aes_key* key_left,
                        const dpf_aes_key* key_right, const dpf_aes_key* key_value,
                        const dpf_value_desc* desc, const dpf_block* value_correction,
                        void* out, void* stream);

/* ---- a11 + SURVEY 8e: batched point evaluation over a key batch ------------
 * Config 4 (2^20 keys x 2^10 points).  Key k < num_keys is the SoA row k of a
 * key batch: root key_seed[k], party[k], correction words cw_seed[k*cw_stride
 * + j], cw_left[...], cw_right[...] (j < num_levels = the hierarchy level's
 * tree depth <= cw_stride, the key's correction-word count) and value
 * corrections value_correction[k*E*num_leaves ...].
 * `points` are raw domain points (dpf_block = uint128): the tree path is
 * point >> block_index_bits and the element index point & (2^bits - 1)
 * (distributed_point_function.cc:206-221).  Point j of key k is
 * points[shared_points ? j : k*points_per_key + j]; the output element
 * k*points_per_key + j (packed) equals EvaluateAt(key_k, {point}).
 * When points_per_key is even and (points_per_key / 2) % 64 == 0 every
 * wavefront works on one key (scalar correction-word loads). */
int dpf_hip_eval_points_batch(int64_t num_keys, int64_t points_per_key, int shared_points,
                              int num_levels, int cw_stride, int block_index_bits,
                              const dpf_block* key_seed,
                              const uint8_t* party, const dpf_block* points,
                              const dpf_block* cw_seed, const uint8_t* cw_left,
                              const uint8_t* cw_right, const dpf_aes_key* key_left,
                              const dpf_aes_key* key_right, const dpf_aes_key* key_value,
                              const dpf_value_desc* desc, const dpf_block* value_correction,
                              void* out, void* stream);

/* Aggregation variant: every key is evaluated at the SAME num_points points
 * and   out[j] = sum over k < num_keys of EvaluateAt(key_k, points[j])
 * is written packed, the sum taken in the value type's group (integers mod
 * 2^bits, IntModN mod N, XorWrapper by XOR; tuples element-wise).
 * `workspace` (device) holds num_points * desc->num_leaves * 3 uint64 (192-bit
 * exact per-leaf sums) and is cleared by the call. */
int dpf_hip_eval_points_sum(int64_t num_keys, int64_t num_points, int num_levels, int cw_stride,
                            int block_index_bits, const dpf_block* key_seed, const uint8_t* party,
                            const dpf_block* points, const dpf_block* cw_seed,
                            const uint8_t* cw_left, const uint8_t* cw_right,
                            const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                            const dpf_aes_key* key_value, const dpf_value_desc* desc,
                            const dpf_block* value_correction, uint64_t* workspace, void* out,
                            void* stream);

/* Number of points[i] >= 2^log_domain_size (the EvaluateAt range check,
 * distributed_point_function.h:861-874, for device-resident points).
 * Synchronous: *count is a host int64. */
int dpf_hip_count_out_of_range(int64_t n, const dpf_block* points, int log_domain_size,
                               int64_t* count, void* stream);

/* ---- gather for EvaluateUntil with prefixes (h:822-835) -------------------
 * out[i*count + j] = in[src_offset[i] + j], elements of elem_size bytes. */
int dpf_hip_gather(int64_t num_rows, int64_t count, int elem_size, const int64_t* src_offset,
                   const void* in, void* out, void* stream);

/* ---- multi-key share aggregation ------------------------------
 * sums[j] = sum over k < num_keys of shares[k*row_len + j] for plain integer
 * leaves of `bits` (8..64) widened to uint64 (mod 2^64), or XOR for xor != 0. */
int dpf_hip_sum_shares_u64(int64_t num_keys, int64_t row_len, int bits, int xor_mode,
                           const void* shares, uint64_t* sums, void* stream);

/* ---- a7+a8+a9+a4+a5+a6 over a key batch at shared prefixes ----------------
 * One EvaluateUntil step (distributed_point_function.h:641-837) of every key
 * of a batch with a device-resident context: the
 * path walk of ComputePartialEvaluations (cc:351-453, EvaluateSeeds
 * evaluate_prg_hwy.cc:452-486), ExpandSeeds (cc:271-349), HashExpandedSeeds
 * (cc:500-524) and the value correction (h:785-808), fused.  The call takes
 * its arguments in one struct, dpf_prefix_batch_args (zero it, set struct_size
 * and the members the launch needs; stream apart).
 *
 * For key k < num_keys and start node u < num_starts:
 *   start  = (seeds_in[k*in_stride + parent[u]], control_in[...]), or key k's
 *            root (key_seed[k], party[k]) when seeds_in == NULL; with
 *            control_in == NULL the control bit is bit 0 of the seed (the
 *            expansion cache layout below) and is cleared before use;
 *   walk   walk_levels levels along path[u] (bit walk_levels-1-j at step j)
 *          with key k's correction words cw_first + j (rows of cw_stride);
 *          after save_after steps (-1 = never) the node is stored at
 *          seeds_out/control_out[k*out_stride + save_index[u]] when
 *          save_index[u] >= 0 (save_index == NULL: at index u);
 *   expand expand_levels (<= dpf_hip_prefix_batch_max_expand) full levels
 *          below it (correction words cw_first + walk_levels + d), hash
 *          every leaf, convert it and keep its first elements_per_leaf
 *          corrected elements (value_correction[k*E*num_leaves ...], party
 *          negation).
 * Slot (u << expand_levels) + leaf, element e is output element
 * ((u << expand_levels) + leaf) * elements_per_leaf + e.
 * sum == 0: out[k][slot] packed, one row of num_starts << expand_levels
 *           elements per key (== EvaluateUntil's block for that node).
 * sum != 0: out[slot] = group sum over keys (integers mod 2^bits, IntModN mod
 *           N, XorWrapper by XOR); workspace holds slots * num_leaves * 3
 *           uint64 and is cleared by the call.  Returns 12 UNIMPLEMENTED for
 *           value types without an on-device key sum
 *           (dpf_hip_prefix_batch_max_expand(desc, 1) < 0): use sum == 0 and
 *           dpf_hip_sum_rows.
 *
 * The expansion cache (leaf_cache != NULL): every tree leaf of the call
 * (2^expand_levels per start node u) also goes to
 * leaf_cache[k*leaf_stride + (u << expand_levels) + l] (leaf_stride >=
 * num_starts << expand_levels), the node's seed with its control bit in bit 0
 * (clear in every non-root seed).  The next level's tree nodes are among these
 * leaves, so the next call reads its start seeds straight from them
 * (seeds_in = the cache, control_in = NULL, parent[u] = the node's cache slot)
 * instead of re-deriving them by a path walk from the partial evaluations two
 * calls back (distributed_point_function.cc:351-453).
 * The leaves must not be the root (depth > 0).  leaf_cache must not overlap
 * seeds_in (the caller double-buffers) except through a slot table.
 *
 * The slot table (leaf_slot != NULL; device, num_starts << expand_levels
 * entries) rewrites the cache IN PLACE: leaf l of start node u goes to
 * leaf_cache[k*leaf_stride + leaf_slot[(u << expand_levels) + l]], and
 * leaf_cache may be seeds_in itself (in_stride == leaf_stride, control_in ==
 * NULL).  Contract on the table: a slot that
 * some start node reads (parent[u]) may appear only among the leaves of that
 * start node, and only if no other start node reads it; every other entry is
 * a slot no start node reads.  Each (key, start node) is one thread that
 * reads its start seed before it writes any leaf, so no entry is overwritten
 * before it has been read -- no gather of the start seeds and no second
 * cache buffer (the heavy-hitters steady state at 2^20
 * clients, where a 64 GiB spare does not fit).  DPF_HIP_CHECK_SLOTS=1 checks
 * the table against this contract on the host first (INVALID_ARGUMENT if
 * broken).
 *
 * The layout of the per-key tables: with index_major == 0 element (key k,
 * slot j) of seeds_in / control_in, seeds_out / control_out and leaf_cache is
 * at k*stride + j.  index_major == 1 puts it at j*num_keys + k for all three
 * (in_stride, out_stride and leaf_stride then only give the slots per key):
 * the layout of the device batch context (DeviceBatchContext), in which 64
 * consecutive keys at one slot are one 1 KiB access.  With index_major == 1
 * the heavy-hitters steady state (no walk, two expanded levels, sum mode,
 * IntModN<uint32_t> tuples) runs with lanes = keys ("hh_keys" in
 * dpf_hip_last_batch_kernel); outputs are identical in both layouts.
 *
 * The fused sketch (num_weights > 0; 0: none): a launch with sum != 0 in the
 * shape the lanes-are-keys kernel takes (index_major, no walk, two expanded
 * levels, start seeds given, one element per leaf, at most two
 * IntModN<uint32_t> leaves) besides the key sums leaves
 *   sketch[(k*num_weights + j)*num_leaves + e] =
 *       ( sum over slots of slot_weights[(slot*num_weights + j)*2 + e] * y_k[slot][e] ) mod N_e
 * without storing any key's row.  slot_weights holds, for every slot (u << 2)
 * + leaf of the launch, num_weights x 2 uint32 already reduced per modulus
 * (dpf_hip_sketch_slot_weights writes them from weights in output order);
 * `accumulators` is num_weights * 2 * num_keys uint64 of device scratch,
 * cleared by the call.  Integer sums below 2^64 added with atomics: the
 * result does not depend on their order.  Every other launch, and
 * num_weights above 2: 12 UNIMPLEMENTED and nothing is launched -- store the
 * rows and call dpf_hip_sketch_rows.  dpf_hip_last_batch_kernel reports
 * "hh_keys_sketch". */
typedef struct dpf_prefix_batch_args {
  uint32_t struct_size; /* sizeof(dpf_prefix_batch_args) */
  int64_t num_keys, num_starts;
  int walk_levels, save_after, expand_levels, cw_first, cw_stride;
  const dpf_block* key_seed;
  const uint8_t* party;
  const dpf_block* seeds_in;
  const uint8_t* control_in;
  int64_t in_stride;
  const int32_t* parent;
  const dpf_block* path;
  const int32_t* save_index;
  dpf_block* seeds_out;
  uint8_t* control_out;
  int64_t out_stride;
  const dpf_block* cw_seed;
  const uint8_t* cw_left;
  const uint8_t* cw_right;
  const dpf_aes_key* key_left;
  const dpf_aes_key* key_right;
  const dpf_aes_key* key_value;
  const dpf_value_desc* desc;
  int elements_per_leaf;
  const dpf_block* value_correction;
  int sum;
  uint64_t* workspace;
  void* out;
  dpf_block* leaf_cache;
  int64_t leaf_stride;
  const int32_t* leaf_slot;
  int index_major;
  int num_weights;
  const uint32_t* slot_weights;
  uint64_t* accumulators;
  uint32_t* sketch;
} dpf_prefix_batch_args;
/* args == NULL or args->struct_size != sizeof(dpf_prefix_batch_args): 3
 * INVALID_ARGUMENT, before anything else is read. */
int dpf_hip_prefix_batch_level(const dpf_prefix_batch_args* args, void* stream);

/* seeds_out[k*num_rows + i] / control_out[k*num_rows + i] = the seed (bit 0
 * cleared) and control bit (bit 0) of cache[k*cache_stride + slot[i]]: a
 * call's start seeds from the previous call's expansion cache.  With
 * index_major == 1: seeds_out / control_out[i*num_keys + k] from
 * cache[slot[i]*num_keys + k] (cache_stride unused). */
int dpf_hip_gather_seeds_layout(int64_t num_keys, int64_t num_rows, const int64_t* slot,
                                const dpf_block* cache, int64_t cache_stride, dpf_block* seeds_out,
                                uint8_t* control_out, int index_major, void* stream);

/* Device-to-host copy of `count` elements of `elem_bytes` each, element i
 * read at src + i*src_stride_bytes and written packed to dst (a column of an
 * index-major table: one key's partial evaluations, ExportEvaluationContext). */
int dpf_hip_memcpy_d2h_strided(void* dst, const void* src, size_t elem_bytes,
                               size_t src_stride_bytes, int64_t count, void* stream);

/* Largest expand_levels dpf_hip_prefix_batch_level accepts for this value type
 * (register-resident subtree), or -1 if `sum` mode is not available. */
int dpf_hip_prefix_batch_max_expand(const dpf_value_desc* desc, int sum);

/* out[j] = group sum over r < num_rows of in[r*row_len + j], packed elements of
 * the value type (the generic on-device key sum). */
int dpf_hip_sum_rows(int64_t num_rows, int64_t row_len, const dpf_value_desc* desc,
                     const void* in, void* out, void* stream);

/* ---- per-key linear sketches of [key][element] rows -------------------------
 * No reference counterpart.  For a value type whose leaves are all
 * IntModN<uint32_t, N_e> sampled from at most two blocks (what
 * dpf_hip_sketch_supported reports; up to five leaves), `in` holds num_keys
 * rows of row_len packed elements and `weights` num_weights rows of row_len
 * uint32 (any 32-bit value), row-major.  For k < num_keys, j < num_weights and
 * leaf e:
 *   out[(k*num_weights + j)*num_leaves + e] =
 *       ( sum_{i < row_len} (weights[j*row_len + i] mod N_e) * in[k][i][e] ) mod N_e
 * as uint32.  Exact integer arithmetic: the map is linear mod N_e, so the two
 * parties' sketches of one key pair add up to weights[j][i*] * beta_e (0 when
 * no element lies on alpha's path).  One wave reduces one key's row; no
 * atomics, no workspace.  num_weights in [1, DPF_HIP_SKETCH_MAX_WEIGHTS] and
 * row_len < 2^32, else 3 INVALID_ARGUMENT; weight_bits must be 32 (wider
 * fields: 12 UNIMPLEMENTED), as is every other value type. */
#define DPF_HIP_SKETCH_MAX_WEIGHTS 4
int dpf_hip_sketch_rows(int64_t num_keys, int64_t row_len, const dpf_value_desc* desc,
                        const void* in, int num_weights, int weight_bits, const void* weights,
                        void* out, void* stream);
/* 1 when dpf_hip_sketch_rows accepts this value type, else 0.  No device is
 * touched. */
int dpf_hip_sketch_supported(const dpf_value_desc* desc);

/* 1 when dpf_hip_prefix_batch_level takes a launch of this shape with
 * num_weights > 0 (the fused sketch), else 0.  DPF_BATCH_SKETCH_FUSED=0 (read
 * per call; A/B and test hook) turns the fused path off, DPF_BATCH_NO_LEAN=1
 * too.  No device is touched. */
int dpf_hip_prefix_batch_sketch_fused(const dpf_value_desc* desc, int walk_levels,
                                      int expand_levels, int elements_per_leaf, int has_seeds_in,
                                      int index_major, int num_weights);
/* Slot-order weights for the fused call: output i = r * count + c (r <
 * num_rows, c < count) lies at slot src_offset[r] + c of the launch (the
 * output gather's offsets; NULL: slot i), and
 *   out[(slot*num_weights + j)*2 + e] = weights[j*num_rows*count + i] mod N_e
 * (e = 1 repeats modulus 0 for a single leaf).  The outputs must cover every
 * slot once (no duplicate prefixes). */
int dpf_hip_sketch_slot_weights(int64_t num_rows, int64_t count, const int64_t* src_offset,
                                const dpf_value_desc* desc, int num_weights, const void* weights,
                                void* out, void* stream);

/* Per-key gather (h:822-835 for a key batch):
 * out[k*num_rows*count + i*count + j] = in[k*in_row_elems + src_offset[i] + j]. */
int dpf_hip_gather_batched(int64_t num_keys, int64_t in_row_elems, int64_t num_rows,
                           int64_t count, int elem_size, const int64_t* src_offset,
                           const void* in, void* out, void* stream);

/* ---- batched DCF evaluation ------------------------------
 * DistributedComparisonFunction::Evaluate (dcf/distributed_comparison_function
 * .h:83-105) for every (key, point) of a key batch of the DCF's incremental
 * DPF (num_levels = the DCF's log domain size n, level i has log domain i):
 *   out[k*points_per_key + j] = sum over levels i with bit (n-1-i) of x == 0
 *                               of EvaluateAt(key_k, i, {x >> (n - i)})
 * (for n == 128 the reference uses prefix 0 at every level; mirrored), with
 * x = points[shared_points ? j : k*points_per_key + j] and the sum in the
 * value type's group.  level_depth / level_blocks (host arrays of n) are
 * hierarchy_to_tree and blocks_needed; value_correction (host array of n
 * device pointers) holds level i's value corrections [key][E*num_leaves]. */
int dpf_hip_dcf_eval_batch(int64_t num_keys, int64_t points_per_key, int shared_points,
                           int num_levels, const int32_t* level_depth,
                           const int32_t* level_blocks, const dpf_block* key_seed,
                           const uint8_t* party, const dpf_block* points,
                           const dpf_block* cw_seed, const uint8_t* cw_left,
                           const uint8_t* cw_right, int cw_stride,
                           const dpf_block* const* value_correction,
                           const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                           const dpf_aes_key* key_value, const dpf_value_desc* desc,
                           void* out, void* stream);

/* ---- full-domain DCF evaluation --------------------------------------------
 * No reference counterpart.  The shares of Evaluate(key_k, x) at every x of
 * the DCF's domain, or of shard `shard_index` of its 2^shard_bits equal
 * parts, in one depth-first walk of each key's tree (every node hashed once:
 * 2^(n+1) - 3 AES for 2^n outputs, against (2n - 1) * 2^n point by point):
 *   out[k * 2^(n - shard_bits) + (x - first_x)] = Evaluate(key_k, x),
 *   first_x = shard_index * 2^(n - shard_bits),
 * packed elements.  The key batch is passed as dpf_hip_dcf_eval_batch takes
 * it.  Only for the DCFs dpf_hip_dcf_expand_supported reports: one integer or
 * XorWrapper leaf of 8, 16, 32, 64 or 128 bits and level_depth[i] == i (every
 * DCF the validator builds for such a type); others: 12 UNIMPLEMENTED -- there
 * is no per-point fallback behind this call.  Argument errors are reported
 * before any device call: 3 for negative counts, NULL tables, shard_bits
 * outside [0, n - 1], shard_index outside [0, 2^shard_bits), n - shard_bits >
 * 62 and an `out` that is not 16-byte aligned.  num_keys == 0 returns 0
 * without a launch.  The item loop is dynamic as chunked launches are
 * (DPF_DCF_EXPAND_DYNAMIC=0, read per launch: a fixed share per thread; A/B
 * and test hook), and dpf_hip_last_dynamic_chunks reports it. */
int dpf_hip_dcf_expand_supported(const dpf_value_desc* desc, int num_levels,
                                 const int32_t* level_depth);
int dpf_hip_dcf_expand(int64_t num_keys, int num_levels, int shard_bits, int64_t shard_index,
                       const dpf_block* key_seed, const uint8_t* party,
                       const dpf_block* cw_seed, const uint8_t* cw_left,
                       const uint8_t* cw_right, int cw_stride,
                       const dpf_block* const* value_correction,
                       const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                       const dpf_aes_key* key_value, const dpf_value_desc* desc, void* out,
                       void* stream);
/* The launch plan of dpf_hip_dcf_expand on a device of num_cus compute units,
 * a pure function (no device is touched): a work item is (key, subtree), the
 * subtree's root lies at depth walk = n - 1 - G and the item visits G levels
 * depth-first and writes 2^(G+1) outputs.  out = {G, walk, items, items per
 * key, top_G, top_items}: with top_G >= 0 a first launch of top_items items,
 * each walking from its key's root and visiting top_G levels, leaves every
 * item its root in the first bytes of the item's own outputs, and the items
 * walk nothing; with top_G == -1 every item walks from its key's root.  3 for
 * arguments dpf_hip_dcf_expand rejects, num_keys < 1 or num_cus < 1. */
int dpf_hip_dcf_expand_plan(int64_t num_keys, int num_levels, int shard_bits, int num_cus,
                            int64_t out[6]);

/* ---- batched private table lookup ------------------------------------------
 * No reference counterpart.  The full-domain expansion of every key of a key
 * batch, folded into one shared public table at a public rotation per key,
 * without storing a share vector.  With n = log_domain_size, N = 2^n, y_k the
 * N shares EvaluateUntil gives for key k, W = table_words and
 * s_k = offsets[k] mod N (only the low n bits of an offset are read):
 *   uint64_t:              out[k*W + w] = sum_{i<N} y_k[i] * T[(i + s_k) mod N][w]  (mod 2^64)
 *   XorWrapper<uint64_t>:  out[k*W + w] = XOR_{i<N} (y_k[i] & T[(i + s_k) mod N][w])
 * `table` is N rows of W uint64, row-major.  The two parties' outputs add
 * (XOR) to beta_k * T[(alpha_k + s_k) mod N][w] (beta_k & ...).  The key batch
 * is passed as dpf_hip_eval_points_batch takes it, with num_levels the
 * hierarchy level's tree depth (n - 1 for these value types), cw_stride the
 * key's correction-word count and value_correction that level's, two blocks
 * per key.  The call is asynchronous on `stream`, overwrites out[0, K*W) and
 * reads nothing of what it held before.
 * Checks, all before any device call, the first failing one reported:
 *   1. num_keys outside [0, 2^31 - 1], log_domain_size outside [1, 40],
 *      num_levels != log_domain_size - 1: 3;
 *   2. NULL desc or AES keys: 3;
 *   3. a value type other than uint64_t / XorWrapper<uint64_t>: 12
 *      UNIMPLEMENTED (there is no fallback behind this call);
 *   4. table_words outside [1, 1024]: 3;   5. table_words not 1, 2 or 4: 12;
 *   6. cw_stride < num_levels: 3;          7. num_keys == 0: returns 0, no launch;
 *   8. NULL key arrays, offsets, table or out (correction words only when
 *      num_levels > 0): 3;
 *   9. `table` not aligned to min(16, 8 * table_words) bytes, `offsets` or
 *      `out` not to 8: 3.
 * The item loop is dynamic as chunked launches are (DPF_LOOKUP_DYNAMIC=0, read
 * per launch: a fixed share per thread; A/B and test hook), and
 * dpf_hip_last_dynamic_chunks reports it. */
int dpf_hip_lookup_supported(const dpf_value_desc* desc, int table_words);
int dpf_hip_lookup_batch(int64_t num_keys, int num_levels, int cw_stride, int log_domain_size,
                         const dpf_block* key_seed, const uint8_t* party,
                         const dpf_block* cw_seed, const uint8_t* cw_left,
                         const uint8_t* cw_right, const dpf_aes_key* key_left,
                         const dpf_aes_key* key_right, const dpf_aes_key* key_value,
                         const dpf_value_desc* desc, const dpf_block* value_correction,
                         const uint64_t* offsets, const void* table, int table_words,
                         uint64_t* out, void* stream);
/* The launch plan of dpf_hip_lookup_batch on a device of num_cus compute
 * units, a pure function (no device is touched).  A work item is (key,
 * subtree): it walks `walk` levels from the key's root and visits S levels
 * depth-first, tree_depth = walk + S.  out = {S, walk, items per key = 2^walk,
 * items}.  S is the deepest the kernel's register stack allows for the table
 * width (5 levels for table_words 1 and 2, 4 for 4), lowered while the launch
 * has fewer than 256 items per compute unit.  A key costs
 * 2^walk * (walk + 2 (2^S - 1) + 2^S) AES.  Items per key below 64: several
 * keys per wave, summed by a segmented cross-lane reduction; 64: one wave per
 * key; above: the waves of a key meet by 64-bit atomics on `out`, which the
 * call clears first in stream order.  3 for num_keys outside [1, 2^31 - 1],
 * tree_depth outside [0, 39], table_words not 1, 2 or 4, num_cus < 1. */
int dpf_hip_lookup_plan(int64_t num_keys, int tree_depth, int table_words, int num_cus,
                        int64_t out[4]);

/* ---- fused full-domain sum over a key batch: private histograms -------------
 * No reference counterpart.  The full-domain expansion of every key of a key
 * batch summed element by element, without storing a share vector.  With n =
 * log_domain_size, N = 2^n and y_k the N shares EvaluateUntil gives for key k:
 *   uint64_t:              out[i] = sum_{k<K} y_k[i]  (mod 2^64)
 *   XorWrapper<uint64_t>:  out[i] = XOR_{k<K} y_k[i]          for i in [0, N)
 * The two parties' vectors combine to the histogram sum_k beta_k * e_{alpha_k}.
 * The key batch is passed as dpf_hip_lookup_batch takes it (num_levels the
 * hierarchy level's tree depth n - 1, cw_stride the key's correction-word
 * count, value_correction that level's, two blocks per key).  `workspace` is
 * device memory of at least dpf_hip_expand_sum_workspace_bytes(num_keys,
 * num_levels) bytes that the call fills with its [level][key] table of
 * correction words; it must stay untouched until the call's work on `stream`
 * is done.  accumulate == 0: out[0, N) is overwritten and nothing of what it
 * held is read; otherwise the sums are added (XORed) into what it holds.  The
 * call is asynchronous on `stream`.
 * Checks, all before any device call, the first failing one reported:
 *   1. num_keys outside [0, 2^31 - 1], log_domain_size outside [1, 30],
 *      num_levels != log_domain_size - 1: 3;
 *   2. NULL desc or AES keys: 3;
 *   3. a value type other than uint64_t / XorWrapper<uint64_t>: 12
 *      UNIMPLEMENTED (there is no fallback behind this call);
 *   4. cw_stride < num_levels: 3;          5. NULL out: 3;
 *   6. num_keys == 0: clears out[0, N) unless accumulating, returns 0, no
 *      kernel is launched;
 *   7. NULL key arrays (correction words only when num_levels > 0): 3;
 *   8. NULL workspace or workspace_bytes too small: 8, the message names the
 *      size needed;
 *   9. `out` or `workspace` not aligned to 16 bytes: 3.
 * The item loop is dynamic as chunked launches are (DPF_EXPAND_SUM_DYNAMIC=0,
 * read per launch: a fixed share per wave; A/B and test hook), and
 * dpf_hip_last_dynamic_chunks reports it. */
#define DPF_HIP_EXPAND_SUM_WAVE_ITEMS_PER_CU 64
int dpf_hip_expand_sum_supported(const dpf_value_desc* desc);
/* Bytes of the call's table: 20 * (num_levels + 1) per key, the keys rounded
 * up to a multiple of 64.  Monotone in both arguments; -1 for num_keys outside
 * [0, 2^31 - 1] or num_levels outside [0, 29].  No device is touched. */
int64_t dpf_hip_expand_sum_workspace_bytes(int64_t num_keys, int num_levels);
int dpf_hip_expand_sum(int64_t num_keys, int num_levels, int cw_stride, int log_domain_size,
                       const dpf_block* key_seed, const uint8_t* party,
                       const dpf_block* cw_seed, const uint8_t* cw_left,
                       const uint8_t* cw_right, const dpf_aes_key* key_left,
                       const dpf_aes_key* key_right, const dpf_aes_key* key_value,
                       const dpf_value_desc* desc, const dpf_block* value_correction,
                       void* workspace, int64_t workspace_bytes, uint64_t* out, int accumulate,
                       void* stream);
/* The launch plan of dpf_hip_expand_sum on a device of num_cus compute units,
 * a pure function (no device is touched).  A wave item is (key chunk of 64
 * consecutive keys, subtree): the wave walks `walk` levels from its keys'
 * roots and visits S levels depth-first, tree_depth = walk + S, finishing the
 * subtree as leaf groups of `group` levels (pairs: 1).  out = {S, walk,
 * subtrees per chunk = 2^walk, wave items = ceil(K / 64) * 2^walk, group,
 * threshold}.  walk is the smallest value with wave items >= threshold =
 * DPF_HIP_EXPAND_SUM_WAVE_ITEMS_PER_CU * num_cus (what the dynamic item loop
 * needs), but at most tree_depth - group.  Small case: tree_depth 0 (n = 1:
 * the root is value-hashed, below a leaf group's depth) is group = S = walk =
 * 0, one wave item per chunk.  A key costs 2^walk * (walk + 2 (2^S - 1)
 * + 2^S) AES.  3 for num_keys outside [1, 2^31 - 1], tree_depth outside
 * [0, 29], num_cus outside [1, 65536]. */
int dpf_hip_expand_sum_plan(int64_t num_keys, int tree_depth, int num_cus, int64_t out[6]);

/* ---- the full-domain sum for packed 8/16/32/64-bit counters and 128-bit XOR ---
 * No reference counterpart.  dpf_hip_expand_sum for every integer width whose
 * elements fill a leaf block: with B the element's bits, E = 128 / B elements
 * per block, n = log_domain_size, N = 2^n and y_k as above,
 *   uintB_t,             B in {8, 16, 32, 64}:      out[i] = sum_{k<K} y_k[i] (mod 2^B)
 *   XorWrapper<uintB_t>, B in {8, 16, 32, 64, 128}: out[i] = XOR_{k<K} y_k[i]
 * `out` is N packed little-endian elements, N * B / 8 bytes, the layout
 * EvaluateUntil writes; out_bytes is its size.  The tree has num_levels = n -
 * log2 E levels (a 32-bit level is one level shallower than a 64-bit one of the
 * same domain, 8 bits three: an eighth of the AES), so the domain holds at
 * least one full leaf block, n >= log2 E.  value_correction holds E blocks per
 * key.  The plan, the workspace and its size are dpf_hip_expand_sum's, by
 * num_levels (dpf_hip_expand_sum_plan, dpf_hip_expand_sum_workspace_bytes);
 * the two 64-bit types run the kernels dpf_hip_expand_sum launches and give
 * its bytes.  Additive 32-bit elements are summed by native 32-bit atomics,
 * 16- and 8-bit ones by a compare-exchange loop on the 64-bit word (carries
 * stop at element tops); every XOR by 64-bit atomic XOR.
 * Checks, all before any device call, the first failing one reported:
 *   1. num_keys outside [0, 2^31 - 1], log_domain_size outside [0, 30]: 3;
 *   2. NULL desc or AES keys: 3;
 *   3. a value type dpf_hip_expand_sum_packed_supported refuses (additive
 *      128-bit, IntModN, tuples): 12 UNIMPLEMENTED (there is no fallback
 *      behind this call);
 *   3a. num_levels != log_domain_size - log2 E, or outside [0, 29] (a domain
 *      below one leaf block; XorWrapper<uint128> at n = 30): 3;
 *   4. cw_stride < num_levels: 3;
 *   5. NULL out, then out_bytes < N * B / 8: 3;
 *   6. to 9. as dpf_hip_expand_sum. */
int dpf_hip_expand_sum_packed_supported(const dpf_value_desc* desc);
int dpf_hip_expand_sum_packed(int64_t num_keys, int num_levels, int cw_stride,
                              int log_domain_size, const dpf_block* key_seed,
                              const uint8_t* party, const dpf_block* cw_seed,
                              const uint8_t* cw_left, const uint8_t* cw_right,
                              const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                              const dpf_aes_key* key_value, const dpf_value_desc* desc,
                              const dpf_block* value_correction, void* workspace,
                              int64_t workspace_bytes, void* out, int64_t out_bytes,
                              int accumulate, void* stream);

/* ---- checked private histograms: fused field sum and per-key sketches -------
 * No reference counterpart.  dpf_hip_expand_sum over a field, with the linear
 * sketches of every key's own vector (dpf_hip_sketch_rows' definition) taken
 * in the same pass, where alone the per-key vectors exist.  Value types:
 * IntModN<uint32_t, N_0> and Tuple<IntModN<uint32_t, N_0>, IntModN<uint32_t,
 * N_1>> (nl = num_leaves <= 2, one element per block, tree depth = n).  With
 * n = log_domain_size in [1, 28], N = 2^n, y_k the N shares EvaluateUntil
 * gives for key k and J = num_weights in {0, 1, 2} rows of N 32-bit weights
 * (`weights`, device, [j][i]):
 *   sum_out[i*nl + e]          = ( sum_{k<K} y_k[i][e] ) mod N_e
 *   sketch_out[(k*J + j)*nl+e] = ( sum_{i<N} (w[j][i] mod N_e) * y_k[i][e] ) mod N_e
 * Exact for any K < 2^31.  The key batch is passed as dpf_hip_expand_sum takes
 * it, with num_levels = the hierarchy level's tree depth = log_domain_size,
 * cw_stride the key's correction-word count and value_correction that level's,
 * nl blocks per key.  `workspace` is device memory of at least
 * dpf_hip_expand_sketch_workspace_bytes(...) bytes holding the call's
 * [level][key] table, its 64-bit accumulators and the reduced weights; it must
 * stay untouched until the call's work on `stream` is done.  accumulate == 0:
 * sum_out[0, N*nl) is overwritten and nothing of what it held is read;
 * otherwise the sums are added mod N_e into what it holds, whose entries must
 * be below N_e.  sketch_out[0, K*J*nl) is always overwritten.  With J == 0
 * `weights` and `sketch_out` are not read and may be NULL.  The call is
 * asynchronous on `stream` and allocates nothing.
 * Checks, all before any device call, the first failing one reported:
 *   1. num_keys outside [0, 2^31 - 1], log_domain_size outside [1, 28],
 *      num_levels != log_domain_size: 3;
 *   2. NULL desc or AES keys: 3;
 *   3. a value type dpf_hip_expand_sketch_supported refuses: 12 UNIMPLEMENTED
 *      (there is no fallback behind this call);
 *   4. num_weights outside [0, 2]: 3;      5. cw_stride < num_levels: 3;
 *   6. NULL sum_out; with num_weights > 0, NULL weights, or NULL sketch_out
 *      unless num_keys == 0 (no sketch is written): 3;
 *   7. num_keys == 0: clears sum_out[0, N*nl) unless accumulating, returns 0,
 *      no kernel is launched, sketch_out is untouched;
 *   8. NULL key arrays: 3;
 *   9. NULL workspace or workspace_bytes too small: 8, the message names the
 *      size needed;
 *  10. sum_out or workspace not aligned to 16 bytes, weights or sketch_out
 *      not to 4: 3.
 * The item loop is dynamic as chunked launches are (DPF_EXPAND_SKETCH_DYNAMIC=0,
 * read per launch: a fixed share per wave; A/B and test hook), and
 * dpf_hip_last_dynamic_chunks reports it. */
#define DPF_HIP_EXPAND_SKETCH_WAVE_ITEMS_PER_CU 64
#define DPF_HIP_EXPAND_SKETCH_MAX_LOG_DOMAIN 28
int dpf_hip_expand_sketch_supported(const dpf_value_desc* desc);
/* Bytes of the call's workspace, the keys rounded up to a multiple of 64 (kp):
 * kp * (20 * num_levels + 12) for the table, 8 * N * num_leaves and
 * 8 * kp * num_weights * num_leaves for the accumulators, 4 * N * num_weights
 * * num_leaves for the reduced weights.  Monotone in every argument; -1 for
 * num_keys outside [0, 2^31 - 1], log_domain_size outside [1, 28], num_levels
 * != log_domain_size, num_leaves outside [1, 2] or num_weights outside [0, 2].
 * No device is touched. */
int64_t dpf_hip_expand_sketch_workspace_bytes(int64_t num_keys, int num_levels,
                                              int log_domain_size, int num_leaves,
                                              int num_weights);
int dpf_hip_expand_sketch(int64_t num_keys, int num_levels, int cw_stride, int log_domain_size,
                          const dpf_block* key_seed, const uint8_t* party,
                          const dpf_block* cw_seed, const uint8_t* cw_left,
                          const uint8_t* cw_right, const dpf_aes_key* key_left,
                          const dpf_aes_key* key_right, const dpf_aes_key* key_value,
                          const dpf_value_desc* desc, const dpf_block* value_correction,
                          int num_weights, const uint32_t* weights, void* workspace,
                          int64_t workspace_bytes, uint32_t* sum_out, uint32_t* sketch_out,
                          int accumulate, void* stream);
/* The launch plan of dpf_hip_expand_sketch on a device of num_cus compute
 * units (no device is touched), dpf_hip_expand_sum_plan's analogue: a wave
 * item is (key chunk of 64 consecutive keys, subtree), the wave walks `walk`
 * levels from its keys' roots and visits S levels depth-first, tree_depth =
 * walk + S, finishing the subtree in leaf pairs (`group` = 1 level).  out =
 * {S, walk, subtrees per chunk = 2^walk, wave items = ceil(K / 64) * 2^walk,
 * group, threshold}.  walk is the smallest value with wave items >= threshold,
 * but at most tree_depth - group.  threshold is
 * DPF_HIP_EXPAND_SKETCH_WAVE_ITEMS_PER_CU * num_cus, or, when the environment
 * holds DPF_EXPAND_SKETCH_WAVE_ITEMS=<t> with t >= 1 (read per call; test and
 * A/B hook), min(t, 2^24) for the whole launch.  Small case: tree_depth 0 has
 * no level for a leaf pair and is group = S = walk = 0; the value types of
 * dpf_hip_expand_sketch have tree_depth = n >= 1 (n = 1 is exactly one leaf
 * pair), so this case is planned but never launched.  A key costs 2^walk *
 * (walk + 2 (2^S - 1) + nl 2^S) AES.  3 for num_keys outside [1, 2^31 - 1],
 * tree_depth outside [0, 28], num_cus outside [1, 65536]. */
int dpf_hip_expand_sketch_plan(int64_t num_keys, int tree_depth, int num_cus, int64_t out[6]);

/* ---- multi-query PIR over a bucketed database --------------------------------
 * No reference counterpart.  Two calls: the stateless full-domain expansion of
 * every key of a key batch into [key][element] share rows in one launch, and
 * the fold of those rows in which every key meets its own bucket's slice of a
 * database [bucket][row][word].
 *
 * dpf_hip_expand_rows: with n = log_domain_size in [1, 24], N = 2^n and y_k
 * the N shares EvaluateUntil gives for key k (uint64_t or
 * XorWrapper<uint64_t>),
 *   rows[k * row_stride_bytes / 8 + i] = y_k[i]      for k < num_keys, i < N.
 * The key batch is passed as dpf_hip_lookup_batch takes it (num_levels the
 * hierarchy level's tree depth n - 1, cw_stride the key's correction-word
 * count, value_correction that level's, two blocks per key).  row_stride_bytes
 * is a multiple of 16 and at least 8 N; the bytes of a row past 8 N are not
 * written.  The call is asynchronous on `stream`, overwrites the N elements
 * of every row and reads nothing of what they held before.
 * Checks, all before any device call, the first failing one reported:
 *   1. num_keys outside [0, 2^31 - 1], log_domain_size outside [1, 24],
 *      num_levels != log_domain_size - 1: 3;
 *   2. NULL desc or AES keys: 3;
 *   3. a value type other than uint64_t / XorWrapper<uint64_t>: 12
 *      UNIMPLEMENTED (there is no fallback behind this call);
 *   4. cw_stride < num_levels: 3;
 *   5. row_stride_bytes not a multiple of 16 or below 8 N: 3;
 *   6. num_keys == 0: returns 0, no launch;
 *   7. NULL key arrays or rows (correction words only when num_levels > 0): 3;
 *   8. `rows` not aligned to 16 bytes: 3.
 * The item loop is dynamic as chunked launches are (DPF_EXPAND_ROWS_DYNAMIC=0,
 * read per launch: a fixed share per thread; A/B and test hook), and
 * dpf_hip_last_dynamic_chunks reports it. */
int dpf_hip_expand_rows_supported(const dpf_value_desc* desc);
int dpf_hip_expand_rows(int64_t num_keys, int num_levels, int cw_stride, int log_domain_size,
                        const dpf_block* key_seed, const uint8_t* party,
                        const dpf_block* cw_seed, const uint8_t* cw_left,
                        const uint8_t* cw_right, const dpf_aes_key* key_left,
                        const dpf_aes_key* key_right, const dpf_aes_key* key_value,
                        const dpf_value_desc* desc, const dpf_block* value_correction,
                        uint64_t* rows, int64_t row_stride_bytes, void* stream);
/* The launch plan of dpf_hip_expand_rows on a device of num_cus compute units,
 * a pure function (no device is touched), by dpf_hip_lookup_plan's rule.  A
 * work item is (key, subtree): it walks `walk` levels from the key's root,
 * visits S levels depth-first and stores 2^(S+1) elements, tree_depth = walk
 * + S.  out = {S, walk, items per key = 2^walk, items}.  S is the deepest the
 * kernel's register stack allows (DPF_HIP_EXPAND_ROWS_MAX_SUBTREE levels),
 * lowered while the launch has fewer than 256 items per compute unit.  A key
 * costs 2^walk * (walk + 2 (2^S - 1) + 2^S) AES.  3 for num_keys outside
 * [1, 2^31 - 1], tree_depth outside [0, 23], num_cus < 1. */
#define DPF_HIP_EXPAND_ROWS_MAX_SUBTREE 6
int dpf_hip_expand_rows_plan(int64_t num_keys, int tree_depth, int num_cus, int64_t out[4]);

/* dpf_hip_dot_buckets: the segmented fold.  The num_keys rows of `y` (device,
 * row k at y + k * y_stride_bytes, N = 2^log_domain_size uint64 shares each)
 * are grouped by bucket: bucket_begin is a HOST array of num_buckets + 1
 * entries, read before the call returns, with bucket_begin[0] == 0,
 * nondecreasing, bucket_begin[num_buckets] == num_keys; keys bucket_begin[b]
 * .. bucket_begin[b + 1] - 1 belong to bucket b (none, one or many).  `db` is
 * the device array [num_buckets][N][W] of uint64, W = record_words.  With
 * b(k) the bucket of key k:
 *   uint64_t:              out[k*W + w] = sum_{i<N} y_k[i] * db[b(k)][i][w]  (mod 2^64)
 *   XorWrapper<uint64_t>:  out[k*W + w] = XOR_{i<N} (y_k[i] & db[b(k)][i][w])
 * Both are exact in any order.  A workgroup takes (bucket, tile of at most 16
 * of its keys, block of its rows, chunk of 64 columns); an empty bucket's
 * slice is not read.  The work-item table is built on the host and copied
 * into `workspace` (device, at least dpf_hip_dot_buckets_workspace_bytes(...)
 * bytes, untouched until the call's work on `stream` is done) with one
 * asynchronous copy.  The call is asynchronous on `stream`, overwrites
 * out[0, K*W) and reads nothing of what `out` or the workspace held before.
 * Checks, all before any device call, the first failing one reported:
 *   1. num_buckets outside [1, 2^20], log_domain_size outside [1, 24],
 *      record_words outside [1, 1024], num_keys outside [0, 2^31 - 1]: 3;
 *   2. NULL desc: 3;
 *   3. a value type other than uint64_t / XorWrapper<uint64_t>: 12
 *      UNIMPLEMENTED (there is no fallback behind this call);
 *   4. bucket_begin NULL, not starting at 0, decreasing or not ending at
 *      num_keys: 3;
 *   5. y_stride_bytes not a multiple of 16 or below 8 N: 3;
 *   6. num_keys == 0: returns 0, no launch;
 *   7. NULL y, db or out: 3;
 *   8. NULL workspace or workspace_bytes too small: 8, the message names the
 *      size needed;
 *   9. `y` or `workspace` not aligned to 16 bytes, `db` or `out` not to 8: 3. */
/* Bytes of the work-item table: 16 per work item, for the most work items a
 * call of these counts can have.  Monotone in every count; -1 for counts
 * dpf_hip_dot_buckets rejects or a value type it does not take.  No device is
 * touched. */
int64_t dpf_hip_dot_buckets_workspace_bytes(const dpf_value_desc* desc, int record_words,
                                            int64_t num_buckets, int64_t num_keys,
                                            int log_domain_size);
int dpf_hip_dot_buckets(int64_t num_buckets, int log_domain_size, int record_words,
                        const int64_t* bucket_begin, int64_t num_keys,
                        const dpf_value_desc* desc, const void* y, int64_t y_stride_bytes,
                        const void* db, uint64_t* out, void* workspace, int64_t workspace_bytes,
                        void* stream);
/* {work items, tiles, largest tile, column chunks} of the calling thread's
 * last dpf_hip_dot_buckets call that launched (test hook). */
int dpf_hip_last_dot_buckets_shape(int64_t out[4]);

/* ---- batched multiple-interval-containment gate (eprint 2020/1392 Fig. 14) -
 * MultipleIntervalContainmentGate::Eval (dcf/fss_gates/
 * multiple_interval_containment.cc:206-275) for num_gates gates over
 * Z_N, N = 2^log_group_size (1..127), each with its own key and masked input
 * x[g] < N, all with the same num_intervals public intervals [p_i, q_i]:
 *   out[g*num_intervals + i] = (party_g ? [x_g > p_i] - [x_g > q'_i] : 0)
 *                              - DCF(key_g, x_g + N-1 - p_i)
 *                              + DCF(key_g, x_g + N-1 - q'_i)
 *                              + mask_share[g*num_intervals + i]      (mod N)
 * with q'_i = q_i + 1 mod N.  The DCF is the uint128 DCF of log domain
 * log_group_size; key_seed .. value_correction are its key batch as
 * dpf_hip_dcf_eval_batch takes them (value_correction: host array of
 * log_group_size device pointers, one dpf_block per key and level).
 * `offsets` (device, num_offsets values < N) is the set of distinct p_i and
 * q'_i; lower_index[i] / upper_index[i] (device) are the positions of p_i and
 * q'_i in it, lower_bound / upper_bound_next (device) p_i and q'_i themselves.
 * One DCF walk runs per (gate, offset) -- not per (gate, bound) -- into
 * `scratch` (device, num_gates * num_offsets blocks, caller-owned), then one
 * lane per (gate, interval) combines.  Every argument is validated before any
 * device work. */
int dpf_hip_mic_eval_batch(int64_t num_gates, int log_group_size, const dpf_block* key_seed,
                           const uint8_t* party, const dpf_block* cw_seed,
                           const uint8_t* cw_left, const uint8_t* cw_right, int cw_stride,
                           const dpf_block* const* value_correction, const dpf_block* x,
                           int num_offsets, const dpf_block* offsets, int num_intervals,
                           const int32_t* lower_index, const int32_t* upper_index,
                           const dpf_block* lower_bound, const dpf_block* upper_bound_next,
                           const dpf_block* mask_share, dpf_block* scratch,
                           const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                           const dpf_aes_key* key_value, dpf_block* out, void* stream);

/* ---- batched key generation (SURVEY.md 8f.4 on the device) -----------------
 * GenerateKeysIncrementalWithSeeds (distributed_point_function.cc:619-687) for
 * num_keys alphas at once, written in the KeyBatch layout
 * (include/dpf/key_batch.h): key pair k gets alpha alphas[k] and the root seeds
 * root_seeds[2k] (party 0) and root_seeds[2k + 1] (party 1); the correction
 * words, which both parties' keys share, go to cw_seed / cw_left / cw_right
 * [k*num_levels + j] and hierarchy level h's value correction to
 * value_correction[h][k*E_h + e] (value_correction: host array of
 * num_hierarchy_levels device pointers).  tree_level, log_domain, blocks and
 * desc are host arrays of num_hierarchy_levels (hierarchy_to_tree, the levels'
 * log domain sizes, blocks_needed and value types); num_levels is the last
 * tree level, at most 128.  `beta` holds flattened leaves (device):
 *   beta_mode 0: beta[h], shared by all keys;
 *   beta_mode 1: beta[k*num_hierarchy_levels + h];
 *   beta_mode 2: the DCF of log domain dcf_bits == num_hierarchy_levels
 *     (dcf/distributed_comparison_function.cc:79-101): alphas[k] is the DCF's
 *     alpha, the DPF's is alphas[k] >> 1, and level h takes beta[k] where bit
 *     dcf_bits-1-h of alphas[k] is set, else zero -- an XorWrapper is never
 *     zeroed, as in the reference.
 * Bit-identical to host generation from the same seeds.  Value types: those
 * dpf_hip_gen_keys_supported reports, at every level; others 12 UNIMPLEMENTED.
 * num_keys == 0 returns 0; NULL pointers, negative counts, level tables that
 * are no hierarchy and other beta modes 3 INVALID_ARGUMENT.  Every check runs
 * before any device work. */
int dpf_hip_gen_key_batch(int64_t num_keys, int num_levels, int num_hierarchy_levels,
                          const int32_t* tree_level, const int32_t* log_domain,
                          const int32_t* blocks, const dpf_value_desc* desc,
                          const dpf_block* alphas, const dpf_block* root_seeds,
                          const dpf_block* beta, int beta_mode, int dcf_bits,
                          const dpf_aes_key* key_left, const dpf_aes_key* key_right,
                          const dpf_aes_key* key_value, dpf_block* cw_seed, uint8_t* cw_left,
                          uint8_t* cw_right, dpf_block* const* value_correction, void* stream);
/* 1 when dpf_hip_gen_key_batch generates keys of this value type (one integer
 * or XorWrapper leaf of 8 to 128 bits, converted directly from one block),
 * else 0.  No device is touched. */
int dpf_hip_gen_keys_supported(const dpf_value_desc* desc);

/* ---- timing helpers (hipEvents on the given stream) ------------------------ */
int dpf_hip_event_create(void** ev);
int dpf_hip_event_destroy(void* ev);
int dpf_hip_event_record(void* ev, void* stream);
int dpf_hip_event_elapsed_ms(void* start, void* stop, float* ms);

#ifdef __cplusplus
}
#endif

#endif /* DPF_HIP_H_ */
