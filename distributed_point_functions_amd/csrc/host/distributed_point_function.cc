// distributed_point_function.cc -- host orchestration of the DPF API.
//
// Semantics follow dpf/distributed_point_function.{h,cc} of the reference
// (file:line references below: cc = .cc, h = .h).  The hot loops -- the
// path walk (EvaluateSeeds), the subtree expansion (ExpandSeeds), leaf hashing
// (HashExpandedSeeds) and the value-correction loop -- run on the GPU through
// the C ABI of include/dpf_hip.h.  There is no CPU evaluation fallback: a
// missing GPU surfaces as an INTERNAL status from the C ABI.
#include "dpf/distributed_point_function.h"

#include <sys/random.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <optional>
#include <unordered_map>

#include "dpf_hip.h"
#include "host_util.h"
#include "shard_plan.h"
#include "until_plan.h"

namespace distributed_point_functions {

using dpf_internal::AesKey;
using dpf_internal::CopyToHostSink;
using dpf_internal::CopyToHostVector;
using dpf_internal::PackedUploads;
using dpf_internal::FromBlock;
using dpf_internal::FromHip;
using dpf_internal::FromProtoBlock;
using dpf_internal::kPrgKeyLeft;
using dpf_internal::kPrgKeyRight;
using dpf_internal::kPrgKeyValue;
using dpf_internal::MakeDesc;
using dpf_internal::SetProtoBlock;
using dpf_internal::ToBlock;
using dpf_internal::U128Hash;

// Expansion starts resident on the device.
struct DistributedPointFunction::DeviceStart {
  int64_t n = 0;
  dpf_block* seeds = nullptr;
  uint8_t* ctrl = nullptr;
};

// What CheckSelectArgs derives: the shard's tree levels, the tree depth of the
// hierarchy level and the records of the shard.
struct DistributedPointFunction::SelectShape {
  int k = 0, stop_level = 0;
  int64_t rows = 0;
};

DistributedPointFunction::DistributedPointFunction(
    std::unique_ptr<dpf_internal::ProtoValidator> validator, std::vector<int> blocks_needed,
    std::vector<dpf_internal::FlatValueType> flat, Aes128FixedKeyHash prg_left,
    Aes128FixedKeyHash prg_right, Aes128FixedKeyHash prg_value)
    : validator_(std::move(validator)),
      blocks_needed_(std::move(blocks_needed)),
      flat_(std::move(flat)),
      prg_left_(prg_left),
      prg_right_(prg_right),
      prg_value_(prg_value),
      scratch_(new dpf_internal::DeviceScratch()) {}

DistributedPointFunction::~DistributedPointFunction() = default;

StatusOr<std::unique_ptr<DistributedPointFunction>> DistributedPointFunction::Create(
    const DpfParameters& parameters) {
  return CreateIncremental(Span<const DpfParameters>(&parameters, 1));
}

StatusOr<std::unique_ptr<DistributedPointFunction>> DistributedPointFunction::CreateIncremental(
    Span<const DpfParameters> parameters) {
  // cc:566-617
  DPF_ASSIGN_OR_RETURN(std::unique_ptr<dpf_internal::ProtoValidator> validator,
                       dpf_internal::ProtoValidator::Create(parameters));
  std::vector<int> blocks_needed(parameters.size());
  std::vector<dpf_internal::FlatValueType> flat(parameters.size());
  for (size_t i = 0; i < parameters.size(); ++i) {
    DPF_ASSIGN_OR_RETURN(int bits, dpf_internal::BitsNeeded(parameters[i].value_type(),
                                                             validator->parameters()[i].security_parameter()));
    blocks_needed[i] = (bits + 127) / 128;
    DPF_ASSIGN_OR_RETURN(flat[i], dpf_internal::Flatten(parameters[i].value_type()));
  }
  DPF_ASSIGN_OR_RETURN(Aes128FixedKeyHash prg_left, Aes128FixedKeyHash::Create(kPrgKeyLeft));
  DPF_ASSIGN_OR_RETURN(Aes128FixedKeyHash prg_right, Aes128FixedKeyHash::Create(kPrgKeyRight));
  DPF_ASSIGN_OR_RETURN(Aes128FixedKeyHash prg_value, Aes128FixedKeyHash::Create(kPrgKeyValue));
  std::unique_ptr<DistributedPointFunction> dpf(new DistributedPointFunction(
      std::move(validator), std::move(blocks_needed), std::move(flat), prg_left, prg_right,
      prg_value));
  // All unsigned integers are registered for backwards compatibility (cc:597-610).
  DPF_RETURN_IF_ERROR(dpf->RegisterValueType<uint8_t>());
  DPF_RETURN_IF_ERROR(dpf->RegisterValueType<uint16_t>());
  DPF_RETURN_IF_ERROR(dpf->RegisterValueType<uint32_t>());
  DPF_RETURN_IF_ERROR(dpf->RegisterValueType<uint64_t>());
  DPF_RETURN_IF_ERROR(dpf->RegisterValueType<uint128>());
  return dpf;
}

Status DistributedPointFunction::RegisterValueType(const ValueType& value_type) {
  registered_types_.insert(dpf_internal::SerializeValueTypeDeterministically(value_type));
  return OkStatus();
}

// ============================================================ key generation
StatusOr<std::vector<uint128>> DistributedPointFunction::ComputeValueCorrectionLeaves(
    int hierarchy_level, const uint128 seeds[2], uint128 alpha, Span<const uint128> beta_leaves,
    bool invert) const {
  // cc:63-99 and ComputeValueCorrectionFor<T> (value_type_helpers.h:597-631),
  // on flattened leaves: E * num_leaves values, element-major.
  const int b = blocks_needed_[hierarchy_level];
  uint128 expanded[2 * 8];
  std::vector<uint128> big;
  uint128* ex = expanded;
  if (b > 8) {
    big.resize(2 * b);
    ex = big.data();
  }
  for (int j = 0; j < b; ++j) {
    ex[j] = seeds[0] + static_cast<uint128>(j);
    ex[b + j] = seeds[1] + static_cast<uint128>(j);
  }
  DPF_RETURN_IF_ERROR(prg_value_.Evaluate(Span<const uint128>(ex, 2 * b), Span<uint128>(ex, 2 * b)));
  const DpfParameters& params = parameters()[hierarchy_level];
  const int block_index_bits = params.log_domain_size() - hierarchy_to_tree()[hierarchy_level];
  const int index_in_block =
      static_cast<int>(alpha & ((static_cast<uint128>(1) << block_index_bits) - 1));
  const dpf_internal::FlatValueType& f = flat_[hierarchy_level];
  const int nl = static_cast<int>(f.leaves.size()), E = f.elements_per_block;
  std::vector<uint128> a(E * nl), c(E * nl);
  dpf_internal::ConvertBytesToLeaves(f, reinterpret_cast<const uint8_t*>(ex), a.data());
  dpf_internal::ConvertBytesToLeaves(f, reinterpret_cast<const uint8_t*>(ex + b), c.data());
  for (int k = 0; k < nl; ++k)
    c[index_in_block * nl + k] = dpf_internal::LeafAdd(f.leaves[k], c[index_in_block * nl + k], beta_leaves[k]);
  for (int i = 0; i < E * nl; ++i) {
    const auto& leaf = f.leaves[i % nl];
    uint128 v = dpf_internal::LeafSub(leaf, c[i], a[i]);
    c[i] = invert ? dpf_internal::LeafNeg(leaf, v) : v;
  }
  return c;
}

Status DistributedPointFunction::CheckValueCorrectionKnown(int hierarchy_level) const {
  // GetValueCorrectionFunction (cc:544-559)
  const DpfParameters& params = parameters()[hierarchy_level];
  if (!registered_types_.count(dpf_internal::SerializeValueTypeDeterministically(params.value_type())))
    return FailedPreconditionError(
        "No value correction function known for the following parameters:\n" +
        params.DebugString() + "Did you call RegisterValueType<T>() with your value type?");
  return OkStatus();
}

StatusOr<std::vector<Value>> DistributedPointFunction::ComputeValueCorrection(
    int hierarchy_level, const uint128 seeds[2], uint128 alpha, const Value& beta,
    bool invert) const {
  const DpfParameters& params = parameters()[hierarchy_level];
  DPF_RETURN_IF_ERROR(CheckValueCorrectionKnown(hierarchy_level));
  DPF_ASSIGN_OR_RETURN(std::vector<uint128> beta_leaves,
                       dpf_internal::ValueToLeaves(params.value_type(), beta));
  DPF_ASSIGN_OR_RETURN(std::vector<uint128> c,
                       ComputeValueCorrectionLeaves(hierarchy_level, seeds, alpha,
                                                    MakeConstSpan(beta_leaves), invert));
  const int nl = static_cast<int>(flat_[hierarchy_level].leaves.size());
  const int E = flat_[hierarchy_level].elements_per_block;
  std::vector<Value> result;
  result.reserve(E);
  for (int e = 0; e < E; ++e) {
    int pos = 0;
    result.push_back(dpf_internal::LeavesToValue(params.value_type(), c.data() + e * nl, &pos));
  }
  return result;
}

Status DistributedPointFunction::GenerateNextCore(int tree_level, uint128 alpha, uint128 seeds[2],
                                                  bool control_bits[2], uint128* seed_correction_out,
                                                  bool ccw[2]) const {
  // cc:138-201: expand both parties' seeds, keep the child on alpha's path,
  // correct the other one away.
  uint128 ex[2][2];
  DPF_RETURN_IF_ERROR(prg_left_.Evaluate(Span<const uint128>(seeds, 2), Span<uint128>(ex[0], 2)));
  DPF_RETURN_IF_ERROR(prg_right_.Evaluate(Span<const uint128>(seeds, 2), Span<uint128>(ex[1], 2)));
  bool ec[2][2];
  for (int br = 0; br < 2; ++br)
    for (int p = 0; p < 2; ++p) {
      ec[br][p] = (ex[br][p] & 1) != 0;
      ex[br][p] &= ~static_cast<uint128>(1);
    }
  const int last_log = parameters().back().log_domain_size();
  bool bit = false;
  if (last_log - tree_level < 128) bit = ((alpha >> (last_log - tree_level)) & 1) != 0;
  const int keep = bit ? 1 : 0, lose = bit ? 0 : 1;
  const uint128 seed_correction = ex[lose][0] ^ ex[lose][1];
  ccw[0] = ec[0][0] ^ ec[0][1] ^ bit ^ 1;
  ccw[1] = ec[1][0] ^ ec[1][1] ^ bit;
  for (int p = 0; p < 2; ++p) {
    seeds[p] = ex[keep][p] ^ (control_bits[p] ? seed_correction : 0);
    control_bits[p] = ec[keep][p] ^ (control_bits[p] && ccw[keep]);
  }
  *seed_correction_out = seed_correction;
  return OkStatus();
}

Status DistributedPointFunction::GenerateNext(int tree_level, uint128 alpha, Span<const Value> beta,
                                              uint128 seeds[2], bool control_bits[2],
                                              DpfKey keys[2]) const {
  // cc:103-204 (line numbers of arXiv 2012.14884 Fig. 11 in the reference comments)
  CorrectionWord* cw = keys[0].add_correction_words();
  const auto& t2h = validator_->tree_to_hierarchy();
  const int last_log = parameters().back().log_domain_size();
  auto it = t2h.find(tree_level - 1);
  if (it != t2h.end()) {
    const int h = it->second;
    uint128 alpha_prefix = 0;
    const int shift = last_log - parameters()[h].log_domain_size();
    if (shift < 128) alpha_prefix = alpha >> shift;
    DPF_ASSIGN_OR_RETURN(std::vector<Value> vc,
                         ComputeValueCorrection(h, seeds, alpha_prefix, beta[h], control_bits[1]));
    for (Value& v : vc) *cw->add_value_correction() = std::move(v);
  }
  uint128 seed_correction;
  bool ccw[2];
  DPF_RETURN_IF_ERROR(GenerateNextCore(tree_level, alpha, seeds, control_bits, &seed_correction, ccw));
  SetProtoBlock(seed_correction, cw->mutable_seed());
  cw->set_control_left(ccw[0]);
  cw->set_control_right(ccw[1]);
  *keys[1].add_correction_words() = *cw;
  return OkStatus();
}

StatusOr<std::pair<DpfKey, DpfKey>> DistributedPointFunction::GenerateKeysIncremental(
    uint128 alpha, Span<const Value> beta) {
  uint128 seeds[2];
  // RAND_bytes in the reference (cc:656-658); getrandom(2) here.
  if (getrandom(seeds, sizeof(seeds), 0) != static_cast<ssize_t>(sizeof(seeds)))
    return InternalError("getrandom failed");
  return GenerateKeysIncrementalWithSeeds(alpha, beta, seeds[0], seeds[1]);
}

StatusOr<std::pair<DpfKey, DpfKey>> DistributedPointFunction::GenerateKeysIncrementalWithSeeds(
    uint128 alpha, Span<const Value> beta, uint128 seed_0, uint128 seed_1) {
  // cc:619-687
  const int H = static_cast<int>(parameters().size());
  if (static_cast<int>(beta.size()) != H)
    return InvalidArgumentError(
        "`beta` has to have the same size as `parameters` passed at construction");
  for (int i = 0; i < H; ++i) DPF_RETURN_IF_ERROR(validator_->ValidateValue(beta[i], i));
  const int last_log = parameters().back().log_domain_size();
  if (last_log < 128 && alpha >= (static_cast<uint128>(1) << last_log))
    return InvalidArgumentError("`alpha` must be smaller than the output domain size");
  DpfKey keys[2];
  keys[0].set_party(0);
  keys[1].set_party(1);
  uint128 seeds[2] = {seed_0, seed_1};
  SetProtoBlock(seeds[0], keys[0].mutable_seed());
  SetProtoBlock(seeds[1], keys[1].mutable_seed());
  bool control_bits[2] = {false, true};
  const int T = tree_levels_needed();
  keys[0].mutable_correction_words()->Reserve(T - 1);
  keys[1].mutable_correction_words()->Reserve(T - 1);
  for (int i = 1; i < T; ++i)
    DPF_RETURN_IF_ERROR(GenerateNext(i, alpha, beta, seeds, control_bits, keys));
  DPF_ASSIGN_OR_RETURN(std::vector<Value> last,
                       ComputeValueCorrection(H - 1, seeds, alpha, beta.back(), control_bits[1]));
  for (const Value& v : last) {
    *keys[0].add_last_level_value_correction() = v;
    *keys[1].add_last_level_value_correction() = v;
  }
  return std::make_pair(std::move(keys[0]), std::move(keys[1]));
}

StatusOr<EvaluationContext> DistributedPointFunction::CreateEvaluationContext(DpfKey key) const {
  // cc:689-704
  DPF_RETURN_IF_ERROR(validator_->ValidateDpfKey(key));
  EvaluationContext result;
  for (const DpfParameters& p : parameters()) *result.add_parameters() = p;
  *result.mutable_key() = std::move(key);
  result.set_previous_hierarchy_level(-1);
  return result;
}

// ============================================================ evaluation
StatusOr<std::vector<uint128>> DistributedPointFunction::ValueCorrectionLeaves(const DpfKey& key,
                                                                               int h) const {
  // h:761-780 / h:883-902
  const RepeatedField<Value>* vc;
  if (h < static_cast<int>(parameters().size()) - 1) {
    vc = &key.correction_words(hierarchy_to_tree()[h]).value_correction();
  } else {
    vc = &key.last_level_value_correction();
  }
  return dpf_internal::ValuesToLeafArray(parameters()[h].value_type(), flat_[h], *vc);
}

namespace {

// Correction words [start, stop) of `key` added to a packed upload.
struct PackedCws {
  size_t seed, left, right;
};
PackedCws AddCorrectionWords(const DpfKey& key, int start, int stop, PackedUploads& up) {
  const int L = stop - start;
  std::vector<dpf_block> seeds(std::max(L, 1));
  std::vector<uint8_t> cl(std::max(L, 1)), cr(std::max(L, 1));
  for (int j = 0; j < L; ++j) {
    const CorrectionWord& cw = key.correction_words(start + j);
    seeds[j] = ToBlock(FromProtoBlock(cw.seed()));
    cl[j] = cw.control_left();
    cr[j] = cw.control_right();
  }
  PackedCws o;
  o.seed = up.Add(seeds.data(), seeds.size());
  o.left = up.Add(cl.data(), cl.size());
  o.right = up.Add(cr.data(), cr.size());
  return o;
}

// Value-correction leaves added to a packed upload as blocks.
size_t AddLeafBlocks(const std::vector<uint128>& leaves, PackedUploads& up) {
  size_t off;
  dpf_block* b = up.Reserve<dpf_block>(leaves.size(), &off);
  for (size_t i = 0; i < leaves.size(); ++i) b[i] = ToBlock(leaves[i]);
  return off;
}

// One key's tree expanded as `parts` independent subtree launches: the split
// first call of EvaluateUntil (the 2^kSplitLevels subtrees under the root), a
// shard (the one subtree under its prefix) and the slabs of the database
// folds (the 2^j subtrees under the shard's prefix).  Everything the launches
// read goes up in ONE packed image and one async H2D (seven synchronous
// uploads had cost ~30 us per call, as much as config 1's whole expansion
// kernel): per part a copy of the key's root and party, which one
// dpf_hip_eval_paths walks in place down the part's path to its subtree root
// at depth `top`, then the value correction and the correction words cut at
// `top`.  Offsets are into the image.
struct SubtreeParts {
  int64_t parts;
  int top, stop_level, party;
  size_t seed, ctrl, vcw;
  PackedCws top_cw, cw;   // correction words [0, top) and [top, stop_level)
};

// The parts' paths, (prefix << j) | i: once per call, whatever the number of keys.
size_t AddSubtreePaths(int64_t prefix, int j, PackedUploads& up) {
  const int64_t parts = int64_t{1} << j;
  size_t off;
  dpf_block* paths = up.Reserve<dpf_block>(parts, &off);
  for (int64_t i = 0; i < parts; ++i) paths[i] = ToBlock(dpf_internal::SubtreePath(prefix, j, i));
  return off;
}

SubtreeParts AddSubtreeParts(const DpfKey& key, int64_t parts, int top, int stop_level,
                             const std::vector<uint128>& vcw, PackedUploads& up) {
  SubtreeParts p{parts, top, stop_level, static_cast<int>(key.party() & 1), 0, 0, 0, {}, {}};
  std::fill_n(up.Reserve<dpf_block>(parts, &p.seed), parts, ToBlock(FromProtoBlock(key.seed())));
  std::fill_n(up.Reserve<uint8_t>(parts, &p.ctrl), parts, static_cast<uint8_t>(p.party));
  p.vcw = AddLeafBlocks(vcw, up);
  p.top_cw = AddCorrectionWords(key, 0, top, up);
  p.cw = AddCorrectionWords(key, top, stop_level, up);
  return p;
}

// The parts' roots walked in place to depth `top` (EvaluateSeeds); the image
// is committed.
Status WalkSubtreeRoots(const SubtreeParts& p, size_t o_path, const PackedUploads& up,
                        void* stream) {
  if (p.top == 0) return OkStatus();
  const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight);
  dpf_block* seed = up.Ptr<dpf_block>(p.seed);
  uint8_t* ctrl = up.Ptr<uint8_t>(p.ctrl);
  return FromHip(dpf_hip_eval_paths(p.parts, p.top, seed, ctrl, up.Ptr<dpf_block>(o_path),
                                    up.Ptr<dpf_block>(p.top_cw.seed), up.Ptr<uint8_t>(p.top_cw.left),
                                    up.Ptr<uint8_t>(p.top_cw.right), &kl, &kr, seed, ctrl, stream));
}

// Part i's subtree expanded into `out`.
Status ExpandSubtree(const SubtreeParts& p, int64_t i, const dpf_value_desc& desc, int cepb,
                     const PackedUploads& up, void* out, void* stream) {
  const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight), kv = AesKey(kPrgKeyValue);
  return FromHip(dpf_hip_expand(1, up.Ptr<dpf_block>(p.seed) + i, up.Ptr<uint8_t>(p.ctrl) + i,
                                p.stop_level - p.top, up.Ptr<dpf_block>(p.cw.seed),
                                up.Ptr<uint8_t>(p.cw.left), up.Ptr<uint8_t>(p.cw.right), &kl, &kr,
                                &kv, &desc, cepb, up.Ptr<dpf_block>(p.vcw), p.party, out, stream));
}

// The shard, dot and select calls alternate between `packed` and `packed_alt`,
// so a call waits (PackedUploads::Reset) for the launch two calls back, not
// for the one still running: back-to-back shard calls keep the GPU busy while
// the host builds the next call's image.
PackedUploads& NextShardImage(dpf_internal::DeviceScratch& s) {
  PackedUploads& up = s.shard_alt ? s.packed_alt : s.packed;
  s.shard_alt = !s.shard_alt;
  return up;
}

// Argument checks the full-domain entry points share.
Status CheckLevel(int hierarchy_level, size_t num_levels) {
  if (hierarchy_level < 0 || hierarchy_level >= static_cast<int>(num_levels))
    return InvalidArgumentError(
        "`hierarchy_level` must be non-negative and less than parameters_.size()");
  return OkStatus();
}
Status CheckRecordWords(int64_t record_words) {
  if (record_words < 1 || record_words > DPF_HIP_DOT_MAX_RECORD_WORDS)
    return InvalidArgumentError("`record_words` must be in [1, 1024]");
  return OkStatus();
}

// A slab hook (DPF_DOT_SLAB_LOG, DPF_SELECT_SLAB_LOG, DPF_DOT_BATCH_SLAB_LOG;
// read per call; test hooks): the log2 of a slab's rows, in place of the
// scratch bound.
std::optional<int> SlabLogHook(const char* name) {
  const char* v = std::getenv(name);
  return v && *v ? std::optional<int>(std::atoi(v)) : std::nullopt;
}

// Keys of EvaluateDotBatchToDevice whose share rows lie in the scratch
// together, or the A/B hook's value, at least 1.  Measured at 4 and 32 words
// only: 8 keys for wide records, 4 for narrow ones, where the
// shares outweigh the records and larger slabs count for more than fewer
// passes over the database.
int DotBatchHostTile(int64_t record_words) { return record_words >= 16 ? 8 : 4; }
int64_t TileHook(const char* name, int dflt) {
  const char* v = std::getenv(name);
  return v && *v ? std::max(std::atoi(v), 1) : dflt;
}

// Phase split of the prefix walk (ComputePartialEvaluations), printed at exit
// with DPF_HOST_TIMING: the lookup of the stored evaluations, the image and
// its upload, the walk on the device (with the walked seeds' D2H), and the
// context rewrite.
dpf_internal::PhaseTimer g_walk_timing(
    "DPF_HOST_TIMING", 0, [](long calls, double n, const double* t) {
      std::fprintf(stderr,
                   "[prefix walk host timing] calls=%ld per call: lookup=%.2fus upload=%.2fus "
                   "device=%.2fus context=%.2fus\n",
                   calls, t[0] * 1e6 / n, t[1] * 1e6 / n, t[2] * 1e6 / n, t[3] * 1e6 / n);
    });
}  // namespace

Status DistributedPointFunction::ComputePartialEvaluations(
    Span<const uint128> prefixes, int hierarchy_level, bool update_ctx, EvaluationContext& ctx,
    DeviceStart* out, void* stream, const std::function<Status()>& before_device) const {
  // cc:351-453
  const int64_t n = static_cast<int64_t>(prefixes.size());
  int start_level = hierarchy_to_tree()[ctx.partial_evaluations_level()];
  const int stop_level = hierarchy_to_tree()[hierarchy_level];
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  dpf_internal::PhaseTimer::Clock wclk(g_walk_timing);
  g_walk_timing.count_call();
  // The walk's inputs -- start seeds, control bits, paths, correction words --
  // go up as ONE packed image (read in place by the kernel when small); the
  // start seeds and control bits are written straight into it.
  PackedUploads& pu = s->packed_pe;
  DPF_RETURN_IF_ERROR(pu.Reset());
  const int max_levels = std::max(stop_level - start_level, stop_level);
  pu.Prepare(static_cast<size_t>(std::max<int64_t>(n, 1)) * (2 * sizeof(dpf_block) + 1) +
             static_cast<size_t>(max_levels + 1) * (sizeof(dpf_block) + 2) + 6 * 256);
  size_t o_seed, o_ctrl, o_paths;
  dpf_block* seeds = pu.Reserve<dpf_block>(std::max<int64_t>(n, 1), &o_seed);
  uint8_t* ctrl = pu.Reserve<uint8_t>(std::max<int64_t>(n, 1), &o_ctrl);
  dpf_block* paths = pu.Reserve<dpf_block>(std::max<int64_t>(n, 1), &o_paths);
  if (ctx.partial_evaluations_size() > 0 && start_level <= stop_level) {
    const int shift = stop_level - start_level;
    auto parent_of = [&](int64_t i) -> uint128 { return shift < 128 ? prefixes[i] >> shift : 0; };
    const auto& pe = ctx.partial_evaluations();
    const int64_t m = pe.size();
    // Sorted fast path (the usual hierarchical case: both the stored prefixes
    // and the lookups come out of EvaluateUntil in ascending order): two
    // chunked passes on host threads instead of a hash map.  The first checks
    // that the stored prefixes ascend and applies the reference's duplicate
    // check (cc:365-383) to adjacent equal ones; the second checks that the
    // lookups' parents ascend and merges them against the stored prefixes,
    // with the reference's lookup error (cc:392-407).  Either order broken:
    // the hash map below redoes the lookup.
    auto stored_at = [&](int64_t j) -> uint128 { return FromProtoBlock(pe[j].prefix()); };
    const int chunks_m = dpf_internal::NumChunks(m), chunks_n = dpf_internal::NumChunks(n);
    std::vector<char> ok_m(chunks_m, 1), dup_ok(chunks_m, 1);
    dpf_internal::ParallelChunks(m, chunks_m, [&](int c, int64_t lo, int64_t hi) {
      if (lo >= hi) return;
      const int64_t first = std::max<int64_t>(lo, 1);
      uint128 prev = stored_at(first - 1);
      for (int64_t j = first; j < hi; ++j) {
        const uint128 cur = stored_at(j);
        if (prev > cur) { ok_m[c] = 0; return; }
        if (prev == cur && dup_ok[c] &&
            (FromProtoBlock(pe[j - 1].seed()) != FromProtoBlock(pe[j].seed()) ||
             pe[j - 1].control_bit() != pe[j].control_bit()))
          dup_ok[c] = 0;
        prev = cur;
      }
    });
    auto all = [](const std::vector<char>& v) {
      return std::all_of(v.begin(), v.end(), [](char x) { return x != 0; });
    };
    bool sorted = all(ok_m);
    if (sorted && !all(dup_ok))
      return InvalidArgumentError(
          "Duplicate prefix in `ctx.partial_evaluations()` with mismatching seed or control bit");
    std::vector<char> ok_n(chunks_n, 1), missing(chunks_n, 0);
    if (sorted) {
      dpf_internal::ParallelChunks(n, chunks_n, [&](int c, int64_t lo, int64_t hi) {
        if (lo >= hi) return;
        int64_t j = std::partition_point(pe.begin(), pe.end(),
                                         [&](const PartialEvaluation& e) {
                                           return FromProtoBlock(e.prefix()) < parent_of(lo);
                                         }) -
                    pe.begin();
        uint128 prev = lo > 0 ? parent_of(lo - 1) : 0;
        for (int64_t i = lo; i < hi; ++i) {
          const uint128 want = parent_of(i);
          if (want < prev) { ok_n[c] = 0; return; }
          prev = want;
          while (j < m && stored_at(j) < want) ++j;
          if (j == m || stored_at(j) != want) { missing[c] = 1; return; }
          seeds[i] = ToBlock(FromProtoBlock(pe[j].seed()));
          ctrl[i] = pe[j].control_bit();
        }
      });
      sorted = all(ok_n);
    }
    if (sorted) {
      if (std::any_of(missing.begin(), missing.end(), [](char x) { return x != 0; }))
        return InvalidArgumentError("Prefix not present in ctx.partial_evaluations at hierarchy level " +
                                    std::to_string(hierarchy_level));
    } else {
    std::unordered_map<uint128, std::pair<uint128, bool>, U128Hash> previous;
    previous.reserve(ctx.partial_evaluations_size() * 2);
    for (const PartialEvaluation& e : ctx.partial_evaluations()) {
      auto value = std::make_pair(FromProtoBlock(e.seed()), e.control_bit());
      auto [it, inserted] = previous.try_emplace(FromProtoBlock(e.prefix()), value);
      if (!inserted && it->second != value)
        return InvalidArgumentError(
            "Duplicate prefix in `ctx.partial_evaluations()` with mismatching seed or control bit");
    }
    for (int64_t i = 0; i < n; ++i) {
      uint128 previous_prefix = 0;
      if (stop_level - start_level < 128) previous_prefix = prefixes[i] >> (stop_level - start_level);
      auto it = previous.find(previous_prefix);
      if (it == previous.end())
        return InvalidArgumentError("Prefix not present in ctx.partial_evaluations at hierarchy level " +
                                    std::to_string(hierarchy_level));
      seeds[i] = ToBlock(it->second.first);
      ctrl[i] = it->second.second;
    }
    }
  } else {
    const dpf_block root = ToBlock(FromProtoBlock(ctx.key().seed()));
    const uint8_t party = static_cast<uint8_t>(ctx.key().party() & 1);
    for (int64_t i = 0; i < n; ++i) {
      seeds[i] = root;
      ctrl[i] = party;
    }
    start_level = 0;
  }
  // Everything that can fail on the host is checked before device work starts.
  if (before_device) DPF_RETURN_IF_ERROR(before_device());
  wclk.mark(0);
  dpf_internal::ParallelFor(n, [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i) paths[i] = ToBlock(prefixes[i]);
  });
  const PackedCws o_cw = AddCorrectionWords(ctx.key(), start_level, stop_level, pu);
  DPF_RETURN_IF_ERROR(pu.Commit(stream));
  wclk.mark(1);
  dpf_block* dev_seed = pu.Ptr<dpf_block>(o_seed);
  uint8_t* dev_ctrl = pu.Ptr<uint8_t>(o_ctrl);
  const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight);
  HIP_RETURN_IF_ERROR(dpf_hip_eval_paths(
      n, stop_level - start_level, dev_seed, dev_ctrl, pu.Ptr<dpf_block>(o_paths),
      pu.Ptr<dpf_block>(o_cw.seed), pu.Ptr<uint8_t>(o_cw.left), pu.Ptr<uint8_t>(o_cw.right), &kl,
      &kr, dev_seed, dev_ctrl, stream));
  // Whatever reads the walked seeds later (the caller's expansion) is
  // ordered after this on `stream`; the caller marks the image used again
  // after its launches (MarkStartUsed) so the next call waits for them too.
  DPF_RETURN_IF_ERROR(pu.MarkUsed(stream));
  if (!update_ctx) ctx.clear_partial_evaluations();
  if (update_ctx) {
    // The walked seeds and control bits back into the host image (in place
    // when the kernel wrote them there), then into the context.
    const size_t span = o_ctrl + static_cast<size_t>(n) - o_seed;
    if (pu.zero_copy()) {
      HIP_RETURN_IF_ERROR(dpf_hip_stream_sync(stream));
    } else {
      HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(seeds, dev_seed, span, stream));
    }
    wclk.mark(2);
    // Resized, not cleared first: a context whose previous level stored as
    // many partial evaluations constructs none, and every field is rewritten.
    auto& pes = ctx.mutable_partial_evaluations()->vec();
    pes.resize(n);
    dpf_internal::ParallelFor(n, [&](int64_t lo, int64_t hi) {
      for (int64_t i = lo; i < hi; ++i) {
        PartialEvaluation* e = &pes[i];
        SetProtoBlock(prefixes[i], e->mutable_prefix());
        SetProtoBlock(FromBlock(seeds[i]), e->mutable_seed());
        e->set_control_bit(ctrl[i] != 0);
      }
    });
    wclk.mark(3);
  }
  ctx.set_partial_evaluations_level(hierarchy_level);
  out->n = n;
  out->seeds = dev_seed;
  out->ctrl = dev_ctrl;
  return OkStatus();
}

StatusOr<int64_t> DistributedPointFunction::OutputElements(int hierarchy_level,
                                                           int64_t num_prefixes,
                                                           int previous_hierarchy_level) const {
  const int prev_log =
      num_prefixes == 0 ? 0 : parameters()[previous_hierarchy_level].log_domain_size();
  const int log = parameters()[hierarchy_level].log_domain_size();
  if (log - prev_log > 62)
    return InvalidArgumentError(
        "Output size would be larger than 2**62. Please evaluate fewer hierarchy levels at once.");
  return std::max<int64_t>(num_prefixes, 1) << (log - prev_log);
}

namespace {
// Host-phase timing of EvaluateUntil, printed at exit when DPF_HOST_TIMING is
// set: where a small call's microseconds go (validation, uploads, launch,
// output copy).
// The first 100 calls (allocations, page-locked buffers) are not counted.
dpf_internal::PhaseTimer g_until_timing(
    "DPF_HOST_TIMING", 100, [](long calls, double n, const double* t) {
      std::fprintf(stderr,
                   "[EvaluateUntil host timing] calls=%ld per call: validate=%.2fus "
                   "dedup=%.2fus walk+vcw=%.2fus pack=%.2fus commit=%.2fus launch=%.2fus "
                   "reserve=%.2fus copy=%.2fus\n",
                   calls, t[7] * 1e6 / n, t[0] * 1e6 / n, t[5] * 1e6 / n, t[6] * 1e6 / n,
                   t[1] * 1e6 / n, t[2] * 1e6 / n, t[3] * 1e6 / n, t[4] * 1e6 / n);
    });
}  // namespace

namespace {
// The split first-call expansion (EvaluateUntilCore): 2^kSplitLevels subtree
// launches.  DPF_EVAL_SPLIT=0 (read per call) launches the whole tree at
// once: an A/B hook.
constexpr int kSplitLevels = 3;
constexpr int kSplitParts = 1 << kSplitLevels;
bool SplitOn() { return !dpf_internal::hook_is("DPF_EVAL_SPLIT", '0'); }
}  // namespace

Status DistributedPointFunction::EvaluateUntilCore(int hierarchy_level, Span<const uint128> prefixes,
                                                   EvaluationContext& ctx,
                                                   const ValueType* requested_type,
                                                   void* device_out, int64_t capacity_bytes,
                                                   void* stream, const HostSink* host_out,
                                                   int64_t* num_elements) const {
  // h:641-837
  dpf_internal::PhaseTimer::Clock clk(g_until_timing);
  DPF_RETURN_IF_ERROR(validator_->ValidateEvaluationContext(ctx));
  const int H = static_cast<int>(parameters().size());
  DPF_RETURN_IF_ERROR(CheckLevel(hierarchy_level, parameters().size()));
  if (requested_type) {
    DPF_ASSIGN_OR_RETURN(bool eq, dpf_internal::ValueTypesAreEqual(
                                      *requested_type, parameters()[hierarchy_level].value_type()));
    if (!eq) return InvalidArgumentError("Value type T doesn't match parameters at `hierarchy_level`");
  }
  if (hierarchy_level <= ctx.previous_hierarchy_level())
    return InvalidArgumentError(
        "`hierarchy_level` must be greater than `ctx.previous_hierarchy_level`");
  if ((ctx.previous_hierarchy_level() < 0) != prefixes.empty())
    return InvalidArgumentError(
        "`prefixes` must be empty if and only if this is the first call with `ctx`.");
  int previous_log_domain_size = 0;
  const int previous_hierarchy_level = ctx.previous_hierarchy_level();
  if (!prefixes.empty()) {
    previous_log_domain_size = parameters()[previous_hierarchy_level].log_domain_size();
    // The first out-of-range prefix is the one reported, as the reference's
    // loop does.
    const int64_t bad = dpf_internal::FirstOutOfRangePrefix(prefixes, previous_log_domain_size);
    if (bad < static_cast<int64_t>(prefixes.size()))
      return InvalidArgumentError("Index " + Uint128ToString(prefixes[bad]) +
                                  " out of range for hierarchy level " +
                                  std::to_string(previous_hierarchy_level));
  }
  const int log_domain_size = parameters()[hierarchy_level].log_domain_size();
  if (log_domain_size - previous_log_domain_size > 62)
    return InvalidArgumentError(
        "Output size would be larger than 2**62. Please evaluate fewer hierarchy levels at once.");

  // The output size is known before anything touches `ctx`: a too-small
  // device buffer is rejected here, so the caller can retry with the same
  // context and a larger buffer.
  const int64_t num_prefixes = static_cast<int64_t>(prefixes.size());
  {
    const int64_t per_prefix = int64_t{1} << (log_domain_size - previous_log_domain_size);
    const int64_t out_total =
        num_prefixes == 0
            ? (int64_t{1} << hierarchy_to_tree()[hierarchy_level]) *
                  corrected_elements_per_block(hierarchy_level)
            : num_prefixes * per_prefix;
    if (device_out && capacity_bytes < out_total * flat_[hierarchy_level].packed_size)
      return InvalidArgumentError("device output buffer too small");
  }

  clk.mark(7);
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  // Unique tree indices of the prefixes, in first-seen order (h:718-742).
  std::vector<uint128>& tree_indices = s->tree_indices;
  std::vector<std::pair<int64_t, int>>& prefix_map = s->prefix_map;
  if (num_prefixes > 0) {
    dpf_internal::DedupTreeIndices(prefixes,
                                   parameters()[previous_hierarchy_level].log_domain_size() -
                                       hierarchy_to_tree()[previous_hierarchy_level],
                                   &tree_indices, &prefix_map);
  } else {
    tree_indices.clear();
    prefix_map.clear();
  }

  // ExpandAndUpdateContext (cc:455-498): starting seeds on the device.  The
  // value correction of this level (h:761-780) is parsed before device work.
  g_until_timing.count_call();
  clk.mark(0);
  std::vector<uint128> vcw;
  auto parse_vcw = [&]() -> Status {
    DPF_ASSIGN_OR_RETURN(vcw, ValueCorrectionLeaves(ctx.key(), hierarchy_level));
    return OkStatus();
  };
  DeviceStart start;
  int start_level = 0;
  PackedUploads& up = s->packed;
  DPF_RETURN_IF_ERROR(up.Reset());
  size_t o_root = 0, o_party = 0;
  if (tree_indices.empty()) {
    DPF_RETURN_IF_ERROR(parse_vcw());
    const dpf_block root = ToBlock(FromProtoBlock(ctx.key().seed()));
    const uint8_t party = static_cast<uint8_t>(ctx.key().party() & 1);
    o_root = up.Add(&root, 1);
    o_party = up.Add(&party, 1);
    start.n = 1;
  } else {
    const bool update_ctx = hierarchy_level < H - 1;
    DPF_RETURN_IF_ERROR(ComputePartialEvaluations(MakeConstSpan(tree_indices),
                                                  previous_hierarchy_level, update_ctx, ctx,
                                                  &start, stream, parse_vcw));
    start_level = hierarchy_to_tree()[previous_hierarchy_level];
  }
  const int stop_level = hierarchy_to_tree()[hierarchy_level];
  ctx.set_previous_hierarchy_level(hierarchy_level);
  const dpf_internal::FlatValueType& f = flat_[hierarchy_level];
  const int cepb = corrected_elements_per_block(hierarchy_level);
  const int esz = f.packed_size;
  const int L = stop_level - start_level;
  const int64_t expansion = start.n << L;
  const int64_t corrected = expansion * cepb;
  const int64_t outputs_per_prefix = int64_t{1} << (log_domain_size - previous_log_domain_size);
  const int64_t total = num_prefixes == 0 ? corrected : num_prefixes * outputs_per_prefix;
  *num_elements = total;

  clk.mark(5);
  // A first call's output of >= DPF_HIP_REGISTER_MIN_BYTES bound for a fresh
  // host vector: the expansion runs as kSplitParts subtree launches, each
  // followed by an event, and the copy of part j (dpf_hip_memcpy_d2h_staged_after)
  // overlaps the expansion of the later parts (2^30 uint64: the 17 ms kernel
  // no longer precedes the 150 ms DMA).
  const bool split = host_out && host_out->grow && tree_indices.empty() && SplitOn() &&
                     L >= kSplitLevels + 12 &&
                     static_cast<size_t>(total) * esz >= DPF_HIP_REGISTER_MIN_BYTES;
  size_t o_vcw = 0, o_sub_path = 0;
  PackedCws o_cw{};
  SubtreeParts sub{};
  if (split) {
    o_sub_path = AddSubtreePaths(0, kSplitLevels, up);
    sub = AddSubtreeParts(ctx.key(), kSplitParts, kSplitLevels, stop_level, vcw, up);
  } else {
    o_vcw = AddLeafBlocks(vcw, up);
    o_cw = AddCorrectionWords(ctx.key(), start_level, stop_level, up);
  }
  clk.mark(6);
  DPF_RETURN_IF_ERROR(up.Commit(stream));
  if (tree_indices.empty()) {
    start.seeds = up.Ptr<dpf_block>(o_root);
    start.ctrl = up.Ptr<uint8_t>(o_party);
  }

  // Is the gather (h:822-835) the identity?  Yes when every prefix maps to its
  // own tree index in order and covers the whole expanded block range.
  const int64_t blocks_per_tree_prefix = num_prefixes ? (expansion / start.n) : 0;
  bool identity = true;
  if (num_prefixes > 0) {
    identity = (outputs_per_prefix == blocks_per_tree_prefix * cepb) &&
               static_cast<int64_t>(tree_indices.size()) == num_prefixes &&
               dpf_internal::IsIdentityMap(prefix_map, num_prefixes);
  }
  // A small host result is written by the kernels straight into page-locked
  // memory (PinnedOut): no D2H copy.
  void* small = (!device_out && host_out) ? s->small_out.Get(static_cast<size_t>(total) * esz)
                                          : nullptr;
  void* expand_out = nullptr;
  if (device_out && identity) {
    if (capacity_bytes < total * esz) return InvalidArgumentError("device output buffer too small");
    expand_out = device_out;
  } else if (small && identity) {
    expand_out = small;
  } else {
    DPF_RETURN_IF_ERROR(s->out.Reserve(static_cast<size_t>(corrected) * esz));
    expand_out = s->out.get();
  }
  const dpf_value_desc desc = MakeDesc(f, blocks_needed_[hierarchy_level]);
  clk.mark(1);
  dpf_internal::PartEvents parts;
  if (split) {
    // The subtree roots at depth kSplitLevels (EvaluateSeeds, in place), then
    // one expansion per subtree into its slice of the output.
    DPF_RETURN_IF_ERROR(WalkSubtreeRoots(sub, o_sub_path, up, stream));
    const size_t part_bytes = static_cast<size_t>(corrected / kSplitParts) * esz;
    for (int j = 0; j < kSplitParts; ++j) {
      DPF_RETURN_IF_ERROR(ExpandSubtree(sub, j, desc, cepb, up,
                                        static_cast<char*>(expand_out) + j * part_bytes, stream));
      DPF_RETURN_IF_ERROR(parts.Record(part_bytes * (j + 1), stream));
    }
  } else {
    const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight), kv = AesKey(kPrgKeyValue);
    HIP_RETURN_IF_ERROR(dpf_hip_expand(start.n, start.seeds, start.ctrl, L,
                                       up.Ptr<dpf_block>(o_cw.seed), up.Ptr<uint8_t>(o_cw.left),
                                       up.Ptr<uint8_t>(o_cw.right), &kl, &kr, &kv, &desc, cepb,
                                       up.Ptr<dpf_block>(o_vcw), ctx.key().party() & 1, expand_out,
                                       stream));
  }
  DPF_RETURN_IF_ERROR(up.MarkUsed(stream));
  // The expansion read its start seeds out of the walk's image: the next
  // call's ComputePartialEvaluations must not rewrite it before that is done.
  if (!tree_indices.empty()) DPF_RETURN_IF_ERROR(s->packed_pe.MarkUsed(stream));
  void* result = expand_out;
  if (!identity) {
    std::vector<int64_t> offsets(num_prefixes);
    dpf_internal::FillGatherOffsets(prefix_map, num_prefixes, blocks_per_tree_prefix * cepb,
                                    outputs_per_prefix, offsets.data());
    DPF_RETURN_IF_ERROR(s->Upload(s->offsets, offsets.data(), offsets.size(), stream));
    if (device_out) {
      if (capacity_bytes < total * esz) return InvalidArgumentError("device output buffer too small");
      result = device_out;
    } else if (small) {
      result = small;
    } else {
      DPF_RETURN_IF_ERROR(s->gathered.Reserve(static_cast<size_t>(total) * esz));
      result = s->gathered.get();
    }
    HIP_RETURN_IF_ERROR(dpf_hip_gather(num_prefixes, outputs_per_prefix, esz,
                                       s->offsets.as<int64_t>(), expand_out, result, stream));
  }
  clk.mark(2);
  if (!device_out) {
    const size_t bytes = static_cast<size_t>(total) * esz;
    if (small) {
      clk.mark(3);
      DPF_RETURN_IF_ERROR(dpf_internal::ConsumePinnedOut(*host_out, small, bytes, stream));
      clk.mark(4);
      return OkStatus();
    }
    void* dst = host_out->reserve(bytes);
    clk.mark(3);
    HIP_RETURN_IF_ERROR(CopyToHostSink(*host_out, dst, result, bytes, stream, &parts));
    clk.mark(4);
  }
  return OkStatus();
}

StatusOr<std::vector<uint8_t>> DistributedPointFunction::EvaluateUntilPacked(
    int hierarchy_level, Span<const uint128> prefixes, EvaluationContext& ctx,
    const ValueType* requested_type) const {
  std::vector<uint8_t> out;
  int64_t n = 0;
  const HostSink sink = dpf_internal::VectorSink(&out);
  DPF_RETURN_IF_ERROR(EvaluateUntilCore(hierarchy_level, prefixes, ctx, requested_type, nullptr, 0,
                                        nullptr, &sink, &n));
  return out;
}

Status DistributedPointFunction::EvaluateUntilToHost(int hierarchy_level,
                                                     Span<const uint128> prefixes,
                                                     EvaluationContext& ctx,
                                                     const ValueType* requested_type,
                                                     const HostSink& sink) const {
  int64_t n = 0;
  return EvaluateUntilCore(hierarchy_level, prefixes, ctx, requested_type, nullptr, 0, nullptr,
                           &sink, &n);
}

StatusOr<int64_t> DistributedPointFunction::EvaluateUntilToDevice(
    int hierarchy_level, Span<const uint128> prefixes, EvaluationContext& ctx, void* device_out,
    int64_t capacity_bytes, void* stream, const ValueType* requested_type) const {
  if (!device_out) return InvalidArgumentError("device_out must not be null");
  int64_t n = 0;
  DPF_RETURN_IF_ERROR(EvaluateUntilCore(hierarchy_level, prefixes, ctx, requested_type, device_out,
                                        capacity_bytes, stream, nullptr, &n));
  return n;
}

void DistributedPointFunction::ReleaseScratch() {
  // The old scratch's destructors wait for the events of its images and free
  // its buffers (long-lived objects kept their largest call's).
  std::unique_ptr<dpf_internal::DeviceScratch> fresh(new dpf_internal::DeviceScratch());
  {
    std::lock_guard<std::recursive_mutex> lock(scratch_->mu);
  }
  scratch_.swap(fresh);
}

StatusOr<int64_t> DistributedPointFunction::EvaluateShardToDevice(
    int hierarchy_level, int64_t shard, int64_t num_shards, EvaluationContext& ctx,
    void* device_out, int64_t capacity_bytes, void* stream) const {
  DPF_RETURN_IF_ERROR(validator_->ValidateEvaluationContext(ctx));
  DPF_RETURN_IF_ERROR(CheckLevel(hierarchy_level, parameters().size()));
  if (ctx.previous_hierarchy_level() >= 0)
    return InvalidArgumentError("sharded evaluation is only defined for the first call with `ctx`");
  const int stop_level = hierarchy_to_tree()[hierarchy_level];
  DPF_ASSIGN_OR_RETURN(const int k, dpf_internal::ShardLevels(
                                        shard, num_shards, stop_level,
                                        parameters()[hierarchy_level].log_domain_size(), 0));
  DPF_ASSIGN_OR_RETURN(std::vector<uint128> vcw, ValueCorrectionLeaves(ctx.key(), hierarchy_level));
  const dpf_internal::FlatValueType& f = flat_[hierarchy_level];
  const int cepb = corrected_elements_per_block(hierarchy_level);
  const int64_t total = (int64_t{1} << (stop_level - k)) * cepb;
  if (!device_out || capacity_bytes < total * f.packed_size)
    return InvalidArgumentError("device output buffer too small");
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  // One part: the subtree under the shard's k-bit prefix.
  PackedUploads& up = NextShardImage(*s);
  DPF_RETURN_IF_ERROR(up.Reset());
  const size_t o_path = AddSubtreePaths(shard, 0, up);
  const SubtreeParts sub = AddSubtreeParts(ctx.key(), 1, k, stop_level, vcw, up);
  DPF_RETURN_IF_ERROR(up.Commit(stream));
  DPF_RETURN_IF_ERROR(WalkSubtreeRoots(sub, o_path, up, stream));
  const dpf_value_desc desc = MakeDesc(f, blocks_needed_[hierarchy_level]);
  DPF_RETURN_IF_ERROR(ExpandSubtree(sub, 0, desc, cepb, up, device_out, stream));
  DPF_RETURN_IF_ERROR(up.MarkUsed(stream));
  ctx.set_previous_hierarchy_level(hierarchy_level);
  return total;
}

StatusOr<int64_t> DistributedPointFunction::EvaluateDotToDevice(
    const DpfKey& key, int hierarchy_level, int64_t shard, int64_t num_shards,
    const void* device_db, int64_t db_bytes, int64_t record_words, void* device_out,
    int64_t out_bytes, void* stream) const {
  DPF_RETURN_IF_ERROR(CheckLevel(hierarchy_level, parameters().size()));
  const int stop_level = hierarchy_to_tree()[hierarchy_level];
  DPF_ASSIGN_OR_RETURN(const int k, dpf_internal::ShardLevels(
                                        shard, num_shards, stop_level,
                                        parameters()[hierarchy_level].log_domain_size(), 0));
  DPF_RETURN_IF_ERROR(CheckRecordWords(record_words));
  const dpf_internal::FlatValueType& f = flat_[hierarchy_level];
  const int cepb = corrected_elements_per_block(hierarchy_level);
  const int W = static_cast<int>(record_words);
  const int L = stop_level - k;                       // tree levels below the shard's root
  const int64_t rows = (int64_t{1} << L) * cepb;      // records of this shard
  const int64_t esz = f.packed_size;
  if (rows > (std::numeric_limits<int64_t>::max() / (esz * W)) || db_bytes < rows * esz * W)
    return InvalidArgumentError("database buffer too small");
  if (out_bytes < esz * W) return InvalidArgumentError("device output buffer too small");
  if (!device_db || !device_out)
    return InvalidArgumentError("`device_db` and `device_out` must not be null");
  DPF_RETURN_IF_ERROR(validator_->ValidateDpfKey(key));
  const dpf_value_desc desc = MakeDesc(f, blocks_needed_[hierarchy_level]);
  const int workspace_bytes = dpf_hip_expand_dot_workspace_bytes(&desc, W);
  if (workspace_bytes < 0) return UnimplementedError(dpf_hip_last_error());
  DPF_ASSIGN_OR_RETURN(std::vector<uint128> vcw, ValueCorrectionLeaves(key, hierarchy_level));

  // Fused (no share vector), or streamed: the shard cut into 2^j slabs whose
  // share vectors fit the scratch bound, each expanded by dpf_hip_expand and
  // folded by dpf_hip_dot_rows.
  const bool fused = dpf_hip_expand_dot_fused(&desc, W) != 0;
  dpf_internal::SlabPlan slab{0, 1, rows};
  if (!fused) {
    DPF_ASSIGN_OR_RETURN(slab, dpf_internal::PlanSlabs(rows, cepb, 8 * esz,
                                                       SlabLogHook("DPF_DOT_SLAB_LOG")));
  }

  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  PackedUploads& up = NextShardImage(*s);
  DPF_RETURN_IF_ERROR(up.Reset());
  const size_t o_path = AddSubtreePaths(shard, slab.j, up);
  const SubtreeParts sub = AddSubtreeParts(key, slab.slabs, k + slab.j, stop_level, vcw, up);
  DPF_RETURN_IF_ERROR(up.Commit(stream));
  DPF_RETURN_IF_ERROR(WalkSubtreeRoots(sub, o_path, up, stream));
  DPF_RETURN_IF_ERROR(s->workspace_fence.Acquire(s->workspace, workspace_bytes, stream));
  if (fused) {
    const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight), kv = AesKey(kPrgKeyValue);
    HIP_RETURN_IF_ERROR(dpf_hip_expand_dot(
        1, up.Ptr<dpf_block>(sub.seed), up.Ptr<uint8_t>(sub.ctrl), L, up.Ptr<dpf_block>(sub.cw.seed),
        up.Ptr<uint8_t>(sub.cw.left), up.Ptr<uint8_t>(sub.cw.right), &kl, &kr, &kv, &desc, cepb,
        up.Ptr<dpf_block>(sub.vcw), sub.party, device_db, W, s->workspace.get(), device_out,
        stream));
  } else {
    DPF_RETURN_IF_ERROR(s->out.Reserve(static_cast<size_t>(slab.slab_rows * esz)));
    for (int64_t i = 0; i < slab.slabs; ++i) {
      DPF_RETURN_IF_ERROR(ExpandSubtree(sub, i, desc, cepb, up, s->out.get(), stream));
      HIP_RETURN_IF_ERROR(dpf_hip_dot_rows(
          slab.slab_rows, W, &desc, s->out.get(),
          static_cast<const char*>(device_db) + i * slab.slab_rows * esz * W, i > 0,
          s->workspace.get(), device_out, stream));
    }
  }
  DPF_RETURN_IF_ERROR(s->workspace_fence.Mark(stream));
  DPF_RETURN_IF_ERROR(up.MarkUsed(stream));
  return record_words;
}

StatusOr<std::vector<uint8_t>> DistributedPointFunction::EvaluateDotPacked(
    const DpfKey& key, int hierarchy_level, const void* device_db, int64_t db_bytes,
    int64_t record_words, const ValueType* requested_type) const {
  DPF_RETURN_IF_ERROR(CheckLevel(hierarchy_level, parameters().size()));
  if (requested_type) {
    DPF_ASSIGN_OR_RETURN(bool eq, dpf_internal::ValueTypesAreEqual(
                                      *requested_type, parameters()[hierarchy_level].value_type()));
    if (!eq) return InvalidArgumentError("Value type T doesn't match parameters at `hierarchy_level`");
  }
  DPF_RETURN_IF_ERROR(CheckRecordWords(record_words));
  const size_t bytes = static_cast<size_t>(record_words) * flat_[hierarchy_level].packed_size;
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);
  // Checked before the result buffer is allocated: host errors touch no device.
  if (!device_db) return InvalidArgumentError("`device_db` and `device_out` must not be null");
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  if (dpf_hip_expand_dot_workspace_bytes(&desc, static_cast<int>(record_words)) < 0)
    return UnimplementedError(dpf_hip_last_error());
  const int cepb = corrected_elements_per_block(hierarchy_level);
  const int64_t rows = (int64_t{1} << hierarchy_to_tree()[hierarchy_level]) * cepb;
  if (parameters()[hierarchy_level].log_domain_size() > 62 ||
      db_bytes / static_cast<int64_t>(bytes) < rows)
    return InvalidArgumentError("database buffer too small");
  DPF_RETURN_IF_ERROR(validator_->ValidateDpfKey(key));
  DPF_RETURN_IF_ERROR(s->gathered.Reserve(bytes));
  DPF_RETURN_IF_ERROR(EvaluateDotToDevice(key, hierarchy_level, 0, 1, device_db, db_bytes,
                                          record_words, s->gathered.get(),
                                          static_cast<int64_t>(bytes), nullptr)
                          .status());
  std::vector<uint8_t> out(bytes);
  HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(out.data(), s->gathered.get(), bytes, nullptr));
  return out;
}

// Private table lookup over a key batch: one fused launch (dpf_lookup.hip).
// The host's part is the argument checks, in the order the header gives.
bool DistributedPointFunction::EvaluatesLookupOnDevice(int hierarchy_level) const {
  if (!CheckLevel(hierarchy_level, parameters().size()).ok()) return false;
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  const int n = parameters()[hierarchy_level].log_domain_size();
  return dpf_hip_lookup_supported(&desc, 1) != 0 && n >= 1 && n <= 40;
}

Status DistributedPointFunction::CheckLookupArgs(int64_t num_keys, bool batch_matches,
                                                 int hierarchy_level, const void* device_offsets,
                                                 const void* device_table, int64_t table_bytes,
                                                 int64_t table_words, const void* device_out,
                                                 int64_t out_bytes) const {
  DPF_RETURN_IF_ERROR(CheckLevel(hierarchy_level, parameters().size()));
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  if (!dpf_hip_lookup_supported(&desc, 1))
    return UnimplementedError(
        "the table lookup is implemented for uint64_t and XorWrapper<uint64_t> only");
  const int n = parameters()[hierarchy_level].log_domain_size();
  if (n < 1 || n > 40)
    return InvalidArgumentError("the table lookup takes a log_domain_size in [1, 40]");
  if (table_words < 1 || table_words > DPF_HIP_DOT_MAX_RECORD_WORDS)
    return InvalidArgumentError("`table_words` must be in [1, 1024]");
  if (!dpf_hip_lookup_supported(&desc, static_cast<int>(table_words)))
    return UnimplementedError("the table lookup is implemented for table_words 1, 2 and 4 only");
  if (table_bytes != (int64_t{1} << n) * table_words * 8)
    return InvalidArgumentError("`table_bytes` must be 2^log_domain_size * table_words * 8");
  if (!device_offsets || !device_table || !device_out)
    return InvalidArgumentError(
        "`device_offsets`, `device_table` and `device_out` must not be null");
  if (num_keys < 0 || out_bytes / (table_words * 8) < num_keys)
    return InvalidArgumentError("device output buffer too small");
  if (!batch_matches)
    return InvalidArgumentError("key batch does not match this DistributedPointFunction");
  if ((reinterpret_cast<uintptr_t>(device_table) & (table_words == 1 ? 7 : 15)) != 0 ||
      (reinterpret_cast<uintptr_t>(device_out) & 7) != 0 ||
      (reinterpret_cast<uintptr_t>(device_offsets) & 7) != 0)
    return InvalidArgumentError(
        "`device_table` must be aligned to min(16, 8 * table_words) bytes, `device_offsets` "
        "and `device_out` to 8");
  return OkStatus();
}

StatusOr<int64_t> DistributedPointFunction::EvaluateLookupBatchToDevice(
    const DeviceKeyBatch& keys, int hierarchy_level, const uint64_t* device_offsets,
    const void* device_table, int64_t table_bytes, int64_t table_words, void* device_out,
    int64_t out_bytes, void* stream) const {
  const int64_t K = keys.num_keys();
  const bool matches = keys.num_levels() == tree_levels_needed() - 1 &&
                       keys.num_hierarchy_levels() == static_cast<int>(parameters().size());
  DPF_RETURN_IF_ERROR(CheckLookupArgs(K, matches, hierarchy_level, device_offsets, device_table,
                                      table_bytes, table_words, device_out, out_bytes));
  const int W = static_cast<int>(table_words);
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight), kv = AesKey(kPrgKeyValue);
  HIP_RETURN_IF_ERROR(dpf_hip_lookup_batch(
      K, hierarchy_to_tree()[hierarchy_level], keys.num_levels(),
      parameters()[hierarchy_level].log_domain_size(), keys.seed(), keys.party(), keys.cw_seed(),
      keys.cw_left(), keys.cw_right(), &kl, &kr, &kv, &desc,
      keys.value_correction(hierarchy_level), device_offsets, device_table, W,
      static_cast<uint64_t*>(device_out), stream));
  return K * W;
}

StatusOr<std::vector<uint64_t>> DistributedPointFunction::EvaluateLookupBatch(
    const DeviceKeyBatch& keys, int hierarchy_level, Span<const uint64_t> offsets,
    const void* device_table, int64_t table_bytes, int64_t table_words) const {
  // The device call's checks first, with stand-ins for the two buffers this
  // call makes itself: host errors touch no device.
  const int64_t K = keys.num_keys();
  const bool matches = keys.num_levels() == tree_levels_needed() - 1 &&
                       keys.num_hierarchy_levels() == static_cast<int>(parameters().size());
  alignas(8) static const uint64_t stand_in = 0;
  DPF_RETURN_IF_ERROR(CheckLookupArgs(K, matches, hierarchy_level, &stand_in, device_table,
                                      table_bytes, table_words, &stand_in,
                                      std::numeric_limits<int64_t>::max()));
  if (static_cast<int64_t>(offsets.size()) != K)
    return InvalidArgumentError("`offsets` must hold one offset per key of the batch");
  std::vector<uint64_t> out(static_cast<size_t>(K * table_words));
  if (K == 0) return out;
  dpf_internal::DeviceBuffer d_off, d_out;
  DPF_RETURN_IF_ERROR(d_off.Upload(offsets.data(), offsets.size(), nullptr));
  DPF_RETURN_IF_ERROR(d_out.Reserve(out.size() * sizeof(uint64_t)));
  DPF_RETURN_IF_ERROR(EvaluateLookupBatchToDevice(keys, hierarchy_level, d_off.as<uint64_t>(),
                                                  device_table, table_bytes, table_words,
                                                  d_out.get(),
                                                  static_cast<int64_t>(out.size() * 8), nullptr)
                          .status());
  HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(out.data(), d_out.get(), out.size() * 8, nullptr));
  return out;
}

// Multi-query PIR over a bucketed database: the key batch expanded into share
// rows in one launch (dpf_expand_rows.hip) and the rows folded into every
// key's own bucket's slice (dpf_dot_buckets.hip).  The host's part is the
// argument checks, in the order the header gives, the rows' and the fold's
// room in the device scratch, and the cut into chunks of keys.
bool DistributedPointFunction::EvaluatesDotBucketsOnDevice(int hierarchy_level) const {
  if (!CheckLevel(hierarchy_level, parameters().size()).ok()) return false;
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  const int n = parameters()[hierarchy_level].log_domain_size();
  return dpf_hip_expand_rows_supported(&desc) != 0 && n >= 1 && n <= 24;
}

Status DistributedPointFunction::CheckDotBucketsArgs(
    int64_t num_keys, bool batch_matches, int hierarchy_level, Span<const int64_t> bucket_begin,
    const void* device_db, int64_t db_bytes, int64_t record_words, const void* device_out,
    int64_t out_bytes) const {
  DPF_RETURN_IF_ERROR(CheckLevel(hierarchy_level, parameters().size()));
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  if (!dpf_hip_expand_rows_supported(&desc))
    return UnimplementedError(
        "the bucketed database fold is implemented for uint64_t and XorWrapper<uint64_t> only");
  const int n = parameters()[hierarchy_level].log_domain_size();
  if (n < 1 || n > 24)
    return InvalidArgumentError("the bucketed database fold takes a log_domain_size in [1, 24]");
  DPF_RETURN_IF_ERROR(CheckRecordWords(record_words));
  const int64_t B = static_cast<int64_t>(bucket_begin.size()) - 1;
  if (B < 1 || B > (int64_t{1} << 20))
    return InvalidArgumentError("`bucket_begin` must hold between 2 and 2^20 + 1 entries");
  if (bucket_begin[0] != 0) return InvalidArgumentError("`bucket_begin` must start at 0");
  for (int64_t b = 0; b < B; ++b)
    if (bucket_begin[b + 1] < bucket_begin[b])
      return InvalidArgumentError("`bucket_begin` must be nondecreasing");
  if (num_keys < 0 || bucket_begin[B] != num_keys)
    return InvalidArgumentError("`bucket_begin` must end at the number of keys of the batch");
  if (db_bytes != B * (int64_t{1} << n) * record_words * 8)
    return InvalidArgumentError(
        "`db_bytes` must be num_buckets * 2^log_domain_size * record_words * 8");
  if (!device_db || !device_out)
    return InvalidArgumentError("`device_db` and `device_out` must not be null");
  if (out_bytes / (record_words * 8) < num_keys)
    return InvalidArgumentError("device output buffer too small");
  if (!batch_matches)
    return InvalidArgumentError("key batch does not match this DistributedPointFunction");
  if ((reinterpret_cast<uintptr_t>(device_db) & 7) != 0 ||
      (reinterpret_cast<uintptr_t>(device_out) & 7) != 0)
    return InvalidArgumentError("`device_db` and `device_out` must be aligned to 8 bytes");
  return OkStatus();
}

StatusOr<int64_t> DistributedPointFunction::EvaluateDotBucketsToDevice(
    const DeviceKeyBatch& keys, int hierarchy_level, Span<const int64_t> bucket_begin,
    const void* device_db, int64_t db_bytes, int64_t record_words, void* device_out,
    int64_t out_bytes, void* stream) const {
  const int64_t K = keys.num_keys();
  const bool matches = keys.num_levels() == tree_levels_needed() - 1 &&
                       keys.num_hierarchy_levels() == static_cast<int>(parameters().size());
  DPF_RETURN_IF_ERROR(CheckDotBucketsArgs(K, matches, hierarchy_level, bucket_begin, device_db,
                                          db_bytes, record_words, device_out, out_bytes));
  if (K == 0) return int64_t{0};
  const int W = static_cast<int>(record_words);
  const int n = parameters()[hierarchy_level].log_domain_size();
  const int depth = hierarchy_to_tree()[hierarchy_level];
  const int64_t B = static_cast<int64_t>(bucket_begin.size()) - 1;
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight), kv = AesKey(kPrgKeyValue);
  // Chunks of consecutive keys whose share rows fit the dot calls' scratch
  // bound (n <= 24: at least two keys).
  const int64_t stride = int64_t{8} << n;   // bytes of a key's share row (n >= 1: 16 | stride)
  const int64_t chunk =
      std::min(K, TileHook("DPF_DOT_BUCKETS_CHUNK_KEYS",
                           static_cast<int>(std::min<int64_t>(
                               std::max<int64_t>(dpf_internal::kSlabScratchBits / 8 / stride, 1),
                               std::numeric_limits<int>::max()))));
  const int64_t fold_bytes = dpf_hip_dot_buckets_workspace_bytes(&desc, W, B, chunk, n);
  if (fold_bytes < 0) return InvalidArgumentError(dpf_hip_last_error());
  const int64_t rows_at = (fold_bytes + 255) & ~int64_t{255};

  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  // The fold's table and the share rows, one after the other in the fenced
  // workspace: a call on another stream waits for this one's last kernel, and
  // a chunk follows the one before it in stream order.
  DPF_RETURN_IF_ERROR(s->workspace_fence.Acquire(
      s->workspace, static_cast<size_t>(rows_at + chunk * stride), stream));
  char* const ws = static_cast<char*>(s->workspace.get());
  uint64_t* const rows = reinterpret_cast<uint64_t*>(ws + rows_at);
  const int64_t cws = keys.num_levels();
  std::vector<int64_t> begin(static_cast<size_t>(B) + 1);
  for (int64_t k0 = 0; k0 < K; k0 += chunk) {
    const int64_t nk = std::min(chunk, K - k0);
    for (int64_t b = 0; b <= B; ++b)
      begin[b] = std::min(std::max(bucket_begin[b], k0), k0 + nk) - k0;
    HIP_RETURN_IF_ERROR(dpf_hip_expand_rows(
        nk, depth, static_cast<int>(cws), n, keys.seed() + k0, keys.party() + k0,
        keys.cw_seed() + k0 * cws, keys.cw_left() + k0 * cws, keys.cw_right() + k0 * cws, &kl, &kr,
        &kv, &desc, keys.value_correction(hierarchy_level) + 2 * k0, rows, stride, stream));
    HIP_RETURN_IF_ERROR(dpf_hip_dot_buckets(B, n, W, begin.data(), nk, &desc, rows, stride,
                                            device_db,
                                            static_cast<uint64_t*>(device_out) + k0 * W, ws,
                                            fold_bytes, stream));
  }
  DPF_RETURN_IF_ERROR(s->workspace_fence.Mark(stream));
  return K * W;
}

StatusOr<std::vector<uint64_t>> DistributedPointFunction::EvaluateDotBuckets(
    const DeviceKeyBatch& keys, int hierarchy_level, Span<const int64_t> bucket_begin,
    const void* device_db, int64_t db_bytes, int64_t record_words) const {
  // The device call's checks first, with a stand-in for the buffer this call
  // makes itself: host errors touch no device.
  const int64_t K = keys.num_keys();
  const bool matches = keys.num_levels() == tree_levels_needed() - 1 &&
                       keys.num_hierarchy_levels() == static_cast<int>(parameters().size());
  alignas(8) static const uint64_t stand_in = 0;
  DPF_RETURN_IF_ERROR(CheckDotBucketsArgs(K, matches, hierarchy_level, bucket_begin, device_db,
                                          db_bytes, record_words, &stand_in,
                                          std::numeric_limits<int64_t>::max()));
  std::vector<uint64_t> out(static_cast<size_t>(K * record_words));
  if (K == 0) return out;
  dpf_internal::DeviceBuffer d_out;
  DPF_RETURN_IF_ERROR(d_out.Reserve(out.size() * sizeof(uint64_t)));
  DPF_RETURN_IF_ERROR(EvaluateDotBucketsToDevice(keys, hierarchy_level, bucket_begin, device_db,
                                                 db_bytes, record_words, d_out.get(),
                                                 static_cast<int64_t>(out.size() * 8), nullptr)
                          .status());
  HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(out.data(), d_out.get(), out.size() * 8, nullptr));
  return out;
}

// Full-domain sum over a key batch: a table kernel and one fused launch
// (dpf_expand_sum.hip).  The host's part is the argument checks, in the order
// the header gives, and the table's room in the device scratch.
bool DistributedPointFunction::EvaluatesFullDomainSumOnDevice(int hierarchy_level) const {
  if (!CheckLevel(hierarchy_level, parameters().size()).ok()) return false;
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  const int n = parameters()[hierarchy_level].log_domain_size();
  return dpf_hip_expand_sum_supported(&desc) != 0 && n >= 1 && n <= 30;
}

Status DistributedPointFunction::CheckFullDomainSumArgs(int64_t num_keys, bool batch_matches,
                                                        int hierarchy_level,
                                                        const void* device_out,
                                                        int64_t out_bytes) const {
  DPF_RETURN_IF_ERROR(CheckLevel(hierarchy_level, parameters().size()));
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  if (!dpf_hip_expand_sum_supported(&desc))
    return UnimplementedError(
        "the full-domain sum is implemented for uint64_t and XorWrapper<uint64_t> only");
  const int n = parameters()[hierarchy_level].log_domain_size();
  if (n < 1 || n > 30)
    return InvalidArgumentError("the full-domain sum takes a log_domain_size in [1, 30]");
  if (!device_out) return InvalidArgumentError("`device_out` must not be null");
  if (num_keys < 0 || out_bytes < (int64_t{1} << n) * 8)
    return InvalidArgumentError("device output buffer too small");
  if (!batch_matches)
    return InvalidArgumentError("key batch does not match this DistributedPointFunction");
  if ((reinterpret_cast<uintptr_t>(device_out) & 15) != 0)
    return InvalidArgumentError("`device_out` must be aligned to 16 bytes");
  return OkStatus();
}

StatusOr<int64_t> DistributedPointFunction::EvaluateFullDomainSumToDevice(
    const DeviceKeyBatch& keys, int hierarchy_level, void* device_out, int64_t out_bytes,
    bool accumulate, void* stream) const {
  const int64_t K = keys.num_keys();
  const bool matches = keys.num_levels() == tree_levels_needed() - 1 &&
                       keys.num_hierarchy_levels() == static_cast<int>(parameters().size());
  DPF_RETURN_IF_ERROR(CheckFullDomainSumArgs(K, matches, hierarchy_level, device_out, out_bytes));
  const int n = parameters()[hierarchy_level].log_domain_size();
  const int depth = hierarchy_to_tree()[hierarchy_level];
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight), kv = AesKey(kPrgKeyValue);
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  const int64_t workspace_bytes = dpf_hip_expand_sum_workspace_bytes(K, depth);
  if (workspace_bytes < 0) return InvalidArgumentError("key batch too large for the full-domain sum");
  if (K > 0)
    DPF_RETURN_IF_ERROR(s->workspace_fence.Acquire(s->workspace,
                                                   static_cast<size_t>(workspace_bytes), stream));
  HIP_RETURN_IF_ERROR(dpf_hip_expand_sum(
      K, depth, keys.num_levels(), n, keys.seed(), keys.party(), keys.cw_seed(), keys.cw_left(),
      keys.cw_right(), &kl, &kr, &kv, &desc, keys.value_correction(hierarchy_level),
      K > 0 ? s->workspace.get() : nullptr, workspace_bytes, static_cast<uint64_t*>(device_out),
      accumulate ? 1 : 0, stream));
  if (K > 0) DPF_RETURN_IF_ERROR(s->workspace_fence.Mark(stream));
  return int64_t{1} << n;
}

StatusOr<std::vector<uint64_t>> DistributedPointFunction::EvaluateFullDomainSum(
    const DeviceKeyBatch& keys, int hierarchy_level) const {
  // The device call's checks first, with a stand-in for the buffer this call
  // makes itself: host errors touch no device.
  const bool matches = keys.num_levels() == tree_levels_needed() - 1 &&
                       keys.num_hierarchy_levels() == static_cast<int>(parameters().size());
  alignas(16) static const uint64_t stand_in[2] = {0, 0};
  DPF_RETURN_IF_ERROR(CheckFullDomainSumArgs(keys.num_keys(), matches, hierarchy_level, stand_in,
                                             std::numeric_limits<int64_t>::max()));
  const size_t N = size_t{1} << parameters()[hierarchy_level].log_domain_size();
  std::vector<uint64_t> out(N);
  if (keys.num_keys() == 0) return out;   // the empty sum
  dpf_internal::DeviceBuffer d_out;
  DPF_RETURN_IF_ERROR(d_out.Reserve(N * sizeof(uint64_t)));
  DPF_RETURN_IF_ERROR(EvaluateFullDomainSumToDevice(keys, hierarchy_level, d_out.get(),
                                                    static_cast<int64_t>(N * 8), false, nullptr)
                          .status());
  HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(out.data(), d_out.get(), N * 8, nullptr));
  return out;
}

// The full-domain sum over packed elements of every width that fills a leaf
// block (dpf_hip_expand_sum_packed): the checks in EvaluateFullDomainSumToDevice's
// order, the shape refusals with the type's, and the same scratch and fence.
namespace {
constexpr char kPackedSumTypeMessage[] =
    "the packed full-domain sum is implemented for uint8_t, uint16_t, uint32_t, uint64_t and "
    "XorWrapper of these and of absl::uint128, at a tree level that gives a domain of at least "
    "one full leaf block (log_domain_size <= 30, at most 29 tree levels)";
}  // namespace

bool DistributedPointFunction::EvaluatesFullDomainSumPackedOnDevice(int hierarchy_level) const {
  if (!CheckLevel(hierarchy_level, parameters().size()).ok()) return false;
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  if (!dpf_hip_expand_sum_packed_supported(&desc)) return false;
  const int n = parameters()[hierarchy_level].log_domain_size();
  const int depth = hierarchy_to_tree()[hierarchy_level];
  // Full leaf blocks: 2^depth blocks of E elements are the 2^n outputs.
  return n <= 30 && depth >= 0 && depth <= 29 &&
         (int64_t{desc.elements_per_block} << depth) == (int64_t{1} << n);
}

Status DistributedPointFunction::CheckFullDomainSumPackedArgs(int64_t num_keys,
                                                              bool batch_matches,
                                                              int hierarchy_level,
                                                              const void* device_out,
                                                              int64_t out_bytes) const {
  DPF_RETURN_IF_ERROR(CheckLevel(hierarchy_level, parameters().size()));
  if (!EvaluatesFullDomainSumPackedOnDevice(hierarchy_level))
    return UnimplementedError(kPackedSumTypeMessage);
  if (!device_out) return InvalidArgumentError("`device_out` must not be null");
  const int depth = hierarchy_to_tree()[hierarchy_level];
  if (num_keys < 0 || out_bytes < (int64_t{16} << depth))
    return InvalidArgumentError("device output buffer too small");
  if (!batch_matches)
    return InvalidArgumentError("key batch does not match this DistributedPointFunction");
  if ((reinterpret_cast<uintptr_t>(device_out) & 15) != 0)
    return InvalidArgumentError("`device_out` must be aligned to 16 bytes");
  return OkStatus();
}

StatusOr<int64_t> DistributedPointFunction::EvaluateFullDomainSumPackedToDevice(
    const DeviceKeyBatch& keys, int hierarchy_level, void* device_out, int64_t out_bytes,
    bool accumulate, void* stream) const {
  const int64_t K = keys.num_keys();
  const bool matches = keys.num_levels() == tree_levels_needed() - 1 &&
                       keys.num_hierarchy_levels() == static_cast<int>(parameters().size());
  DPF_RETURN_IF_ERROR(
      CheckFullDomainSumPackedArgs(K, matches, hierarchy_level, device_out, out_bytes));
  const int n = parameters()[hierarchy_level].log_domain_size();
  const int depth = hierarchy_to_tree()[hierarchy_level];
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight), kv = AesKey(kPrgKeyValue);
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  const int64_t workspace_bytes = dpf_hip_expand_sum_workspace_bytes(K, depth);
  if (workspace_bytes < 0) return InvalidArgumentError("key batch too large for the full-domain sum");
  if (K > 0)
    DPF_RETURN_IF_ERROR(s->workspace_fence.Acquire(s->workspace,
                                                   static_cast<size_t>(workspace_bytes), stream));
  HIP_RETURN_IF_ERROR(dpf_hip_expand_sum_packed(
      K, depth, keys.num_levels(), n, keys.seed(), keys.party(), keys.cw_seed(), keys.cw_left(),
      keys.cw_right(), &kl, &kr, &kv, &desc, keys.value_correction(hierarchy_level),
      K > 0 ? s->workspace.get() : nullptr, workspace_bytes, device_out, out_bytes,
      accumulate ? 1 : 0, stream));
  if (K > 0) DPF_RETURN_IF_ERROR(s->workspace_fence.Mark(stream));
  return int64_t{1} << n;
}

StatusOr<std::vector<uint8_t>> DistributedPointFunction::EvaluateFullDomainSumPackedBytes(
    const DeviceKeyBatch& keys, int hierarchy_level, const ValueType* requested_type) const {
  DPF_RETURN_IF_ERROR(CheckLevel(hierarchy_level, parameters().size()));
  if (requested_type) {
    DPF_ASSIGN_OR_RETURN(bool eq, dpf_internal::ValueTypesAreEqual(
                                      *requested_type, parameters()[hierarchy_level].value_type()));
    if (!eq) return InvalidArgumentError("Value type T doesn't match parameters at `hierarchy_level`");
  }
  // The device call's checks first, with a stand-in for the buffer this call
  // makes itself: host errors touch no device.
  const bool matches = keys.num_levels() == tree_levels_needed() - 1 &&
                       keys.num_hierarchy_levels() == static_cast<int>(parameters().size());
  alignas(16) static const uint64_t stand_in[2] = {0, 0};
  DPF_RETURN_IF_ERROR(CheckFullDomainSumPackedArgs(keys.num_keys(), matches, hierarchy_level,
                                                   stand_in,
                                                   std::numeric_limits<int64_t>::max()));
  const size_t bytes = size_t{16} << hierarchy_to_tree()[hierarchy_level];
  std::vector<uint8_t> out(bytes);
  if (keys.num_keys() == 0) return out;   // the empty sum
  dpf_internal::DeviceBuffer d_out;
  DPF_RETURN_IF_ERROR(d_out.Reserve(bytes));
  DPF_RETURN_IF_ERROR(EvaluateFullDomainSumPackedToDevice(keys, hierarchy_level, d_out.get(),
                                                          static_cast<int64_t>(bytes), false,
                                                          nullptr)
                          .status());
  HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(out.data(), d_out.get(), bytes, nullptr));
  return out;
}

// Checked private histograms: the field sum of a key batch's full domain with
// every key's sketches, one fused launch between a table and a finish kernel
// (dpf_expand_sketch.hip).  The host's part is the argument checks, in the
// order the header gives, and the workspace's room in the device scratch.
bool DistributedPointFunction::EvaluatesFullDomainSumSketchOnDevice(int hierarchy_level) const {
  if (!CheckLevel(hierarchy_level, parameters().size()).ok()) return false;
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  const int n = parameters()[hierarchy_level].log_domain_size();
  return dpf_hip_expand_sketch_supported(&desc) != 0 && n >= 1 &&
         n <= DPF_HIP_EXPAND_SKETCH_MAX_LOG_DOMAIN;
}

Status DistributedPointFunction::CheckFullDomainSumSketchArgs(
    int64_t num_keys, bool batch_matches, int hierarchy_level, const void* device_weights,
    int num_weight_rows, const void* device_sum, int64_t sum_bytes, const void* device_sketch,
    int64_t sketch_bytes) const {
  DPF_RETURN_IF_ERROR(CheckLevel(hierarchy_level, parameters().size()));
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  if (!dpf_hip_expand_sketch_supported(&desc))
    return UnimplementedError(
        "the checked full-domain sum is implemented for IntModN<uint32_t, N> and 2-tuples of "
        "it only");
  const int n = parameters()[hierarchy_level].log_domain_size();
  if (n < 1 || n > DPF_HIP_EXPAND_SKETCH_MAX_LOG_DOMAIN)
    return InvalidArgumentError("the checked full-domain sum takes a log_domain_size in [1, 28]");
  const int64_t J = num_weight_rows, nl = desc.num_leaves;
  if (J < 0 || J > 2) return InvalidArgumentError("`num_weight_rows` must be in [0, 2]");
  if (!device_sum) return InvalidArgumentError("`device_sum` must not be null");
  if (J > 0 && (!device_weights || (!device_sketch && num_keys > 0)))
    return InvalidArgumentError(
        "`device_weights` and `device_sketch` must not be null when num_weight_rows > 0");
  if (sum_bytes < (int64_t{1} << n) * nl * 4)
    return InvalidArgumentError("device sum buffer too small");
  if (num_keys < 0 || (J > 0 && sketch_bytes / (J * nl * 4) < num_keys))
    return InvalidArgumentError("device sketch buffer too small");
  if (!batch_matches)
    return InvalidArgumentError("key batch does not match this DistributedPointFunction");
  if ((reinterpret_cast<uintptr_t>(device_sum) & 15) != 0 ||
      (J > 0 && ((reinterpret_cast<uintptr_t>(device_weights) & 3) != 0 ||
                 (reinterpret_cast<uintptr_t>(device_sketch) & 3) != 0)))
    return InvalidArgumentError(
        "`device_sum` must be aligned to 16 bytes, `device_weights` and `device_sketch` to 4");
  return OkStatus();
}

StatusOr<int64_t> DistributedPointFunction::EvaluateFullDomainSumSketchToDevice(
    int hierarchy_level, const DeviceKeyBatch& keys, const uint32_t* device_weights,
    int num_weight_rows, void* device_sum, int64_t sum_bytes, void* device_sketch,
    int64_t sketch_bytes, bool accumulate, void* stream) const {
  const int64_t K = keys.num_keys();
  const bool matches = keys.num_levels() == tree_levels_needed() - 1 &&
                       keys.num_hierarchy_levels() == static_cast<int>(parameters().size());
  DPF_RETURN_IF_ERROR(CheckFullDomainSumSketchArgs(K, matches, hierarchy_level, device_weights,
                                                   num_weight_rows, device_sum, sum_bytes,
                                                   device_sketch, sketch_bytes));
  const int n = parameters()[hierarchy_level].log_domain_size();
  const int depth = hierarchy_to_tree()[hierarchy_level];
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight), kv = AesKey(kPrgKeyValue);
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  const int64_t workspace_bytes =
      dpf_hip_expand_sketch_workspace_bytes(K, depth, n, desc.num_leaves, num_weight_rows);
  if (workspace_bytes < 0)
    return InvalidArgumentError("key batch too large for the checked full-domain sum");
  if (K > 0)
    DPF_RETURN_IF_ERROR(s->workspace_fence.Acquire(s->workspace,
                                                   static_cast<size_t>(workspace_bytes), stream));
  HIP_RETURN_IF_ERROR(dpf_hip_expand_sketch(
      K, depth, keys.num_levels(), n, keys.seed(), keys.party(), keys.cw_seed(), keys.cw_left(),
      keys.cw_right(), &kl, &kr, &kv, &desc, keys.value_correction(hierarchy_level),
      num_weight_rows, device_weights, K > 0 ? s->workspace.get() : nullptr, workspace_bytes,
      static_cast<uint32_t*>(device_sum), static_cast<uint32_t*>(device_sketch),
      accumulate ? 1 : 0, stream));
  if (K > 0) DPF_RETURN_IF_ERROR(s->workspace_fence.Mark(stream));
  return int64_t{1} << n;
}

StatusOr<DistributedPointFunction::SumSketch> DistributedPointFunction::EvaluateFullDomainSumSketch(
    int hierarchy_level, const DeviceKeyBatch& keys, Span<const uint32_t> weights,
    int num_weight_rows) const {
  // The device call's checks first, with stand-ins for the buffers this call
  // makes itself: host errors touch no device.
  const int64_t K = keys.num_keys();
  const bool matches = keys.num_levels() == tree_levels_needed() - 1 &&
                       keys.num_hierarchy_levels() == static_cast<int>(parameters().size());
  alignas(16) static const uint32_t stand_in[4] = {0, 0, 0, 0};
  DPF_RETURN_IF_ERROR(CheckFullDomainSumSketchArgs(
      K, matches, hierarchy_level, stand_in, num_weight_rows, stand_in,
      std::numeric_limits<int64_t>::max(), stand_in, std::numeric_limits<int64_t>::max()));
  const size_t N = size_t{1} << parameters()[hierarchy_level].log_domain_size();
  const size_t J = static_cast<size_t>(num_weight_rows);
  const size_t nl = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]).num_leaves;
  if (weights.size() != J * N)
    return InvalidArgumentError("`weights` must hold num_weight_rows rows of 2^log_domain_size");
  SumSketch out;
  out.sum.assign(N * nl, 0);
  out.sketch.assign(static_cast<size_t>(K) * J * nl, 0);
  if (K == 0) return out;   // the empty sum
  dpf_internal::DeviceBuffer d_w, d_sum, d_sk;
  if (J > 0) {
    DPF_RETURN_IF_ERROR(d_w.Upload(weights.data(), weights.size(), nullptr));
    DPF_RETURN_IF_ERROR(d_sk.Reserve(out.sketch.size() * 4));
  }
  DPF_RETURN_IF_ERROR(d_sum.Reserve(out.sum.size() * 4));
  DPF_RETURN_IF_ERROR(EvaluateFullDomainSumSketchToDevice(
                          hierarchy_level, keys, J > 0 ? d_w.as<uint32_t>() : nullptr,
                          num_weight_rows, d_sum.get(), static_cast<int64_t>(out.sum.size() * 4),
                          J > 0 ? d_sk.get() : nullptr,
                          static_cast<int64_t>(out.sketch.size() * 4), false, nullptr)
                          .status());
  HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(out.sum.data(), d_sum.get(), out.sum.size() * 4, nullptr));
  if (J > 0)
    HIP_RETURN_IF_ERROR(
        dpf_hip_memcpy_d2h(out.sketch.data(), d_sk.get(), out.sketch.size() * 4, nullptr));
  return out;
}

// Dense PIR: the streamed path of EvaluateDotToDevice with one bit per record
// and up to 64 keys per pass over the database.  The shard is cut into slabs
// of whole leaf blocks whose Q bit rows fit the dot call's scratch bound
// together; every key's slab is expanded by the unchanged dpf_hip_expand into
// its row of the scratch, and dpf_hip_select_rows folds the slab of the
// database into all Q answers at once.  DPF_SELECT_SLAB_LOG (read per call;
// test hook) sets the log2 of a slab's records instead, at least 7.
Status DistributedPointFunction::CheckSelectArgs(
    Span<const DpfKey* const> keys, int hierarchy_level, int64_t shard, int64_t num_shards,
    const void* device_db, int64_t db_bytes, int64_t record_words, const void* device_out,
    int64_t out_bytes, SelectShape* shape) const {
  DPF_RETURN_IF_ERROR(CheckLevel(hierarchy_level, parameters().size()));
  const dpf_internal::FlatValueType& f = flat_[hierarchy_level];
  const dpf_value_desc desc = MakeDesc(f, blocks_needed_[hierarchy_level]);
  const int bits = desc.bits[0];
  if (desc.num_leaves != 1 || !desc.direct || desc.kind[0] != DPF_LEAF_XOR ||
      desc.blocks_needed != 1 || !(bits == 64 || bits == 128) ||
      desc.elements_per_block != 128 / bits)
    return UnimplementedError(
        "the bit-selected database fold is implemented for XorWrapper<uint64_t> and "
        "XorWrapper<absl::uint128> only");
  // The cap of EvaluateDotToDevice, on the records: one per output bit.
  const int stop_level = hierarchy_to_tree()[hierarchy_level];
  DPF_ASSIGN_OR_RETURN(const int k, dpf_internal::ShardLevels(
                                        shard, num_shards, stop_level,
                                        parameters()[hierarchy_level].log_domain_size(),
                                        bits == 64 ? 6 : 7));
  DPF_RETURN_IF_ERROR(CheckRecordWords(record_words));
  const int64_t Q = static_cast<int64_t>(keys.size());
  if (Q < 1 || Q > DPF_HIP_SELECT_MAX_QUERIES)
    return InvalidArgumentError("`keys` must hold between 1 and 64 keys");
  const int64_t rows = (int64_t{1} << (stop_level - k)) *
                       corrected_elements_per_block(hierarchy_level) * f.packed_size * 8;
  if (shape) *shape = SelectShape{k, stop_level, rows};
  if (rows > (std::numeric_limits<int64_t>::max() / (8 * record_words)) ||
      db_bytes < rows * 8 * record_words)
    return InvalidArgumentError("database buffer too small");
  if (out_bytes < Q * record_words * 8)
    return InvalidArgumentError("device output buffer too small");
  if (!device_db || !device_out)
    return InvalidArgumentError("`device_db` and `device_out` must not be null");
  for (int64_t q = 0; q < Q; ++q) {
    if (!keys[q])
      return InvalidArgumentError("`keys[" + std::to_string(q) + "]` must not be null");
    if (Status st = validator_->ValidateDpfKey(*keys[q]); !st.ok())
      return Status(st.code(), "DpfKey " + std::to_string(q) + ": " + st.message());
  }
  return OkStatus();
}

StatusOr<int64_t> DistributedPointFunction::EvaluateSelectToDevice(
    Span<const DpfKey* const> keys, int hierarchy_level, int64_t shard, int64_t num_shards,
    const void* device_db, int64_t db_bytes, int64_t record_words, void* device_out,
    int64_t out_bytes, void* stream) const {
  SelectShape shape;
  DPF_RETURN_IF_ERROR(CheckSelectArgs(keys, hierarchy_level, shard, num_shards, device_db,
                                      db_bytes, record_words, device_out, out_bytes, &shape));
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  const int cepb = corrected_elements_per_block(hierarchy_level);
  const int W = static_cast<int>(record_words);
  const int64_t Q = static_cast<int64_t>(keys.size());
  const int workspace_bytes = dpf_hip_select_workspace_bytes(W, static_cast<int>(Q));
  if (workspace_bytes < 0) return InvalidArgumentError(dpf_hip_last_error());

  // Slabs of whole leaf blocks (128 records) whose Q bit rows fit the scratch bound.
  DPF_ASSIGN_OR_RETURN(const dpf_internal::SlabPlan slab,
                       dpf_internal::PlanSlabs(shape.rows, 128, Q,
                                               SlabLogHook("DPF_SELECT_SLAB_LOG")));
  const int64_t stride = (slab.slab_rows / 8 + 15) & ~int64_t{15};   // bytes of a key's bit row

  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  // One image for all keys: the slabs' paths once, then each key's parts.
  PackedUploads& up = NextShardImage(*s);
  DPF_RETURN_IF_ERROR(up.Reset());
  const size_t o_path = AddSubtreePaths(shard, slab.j, up);
  std::vector<SubtreeParts> sub(Q);
  for (int64_t q = 0; q < Q; ++q) {
    DPF_ASSIGN_OR_RETURN(std::vector<uint128> vcw, ValueCorrectionLeaves(*keys[q], hierarchy_level));
    sub[q] = AddSubtreeParts(*keys[q], slab.slabs, shape.k + slab.j, shape.stop_level, vcw, up);
  }
  DPF_RETURN_IF_ERROR(up.Commit(stream));
  for (int64_t q = 0; q < Q; ++q) DPF_RETURN_IF_ERROR(WalkSubtreeRoots(sub[q], o_path, up, stream));
  DPF_RETURN_IF_ERROR(s->workspace_fence.Acquire(s->workspace, workspace_bytes, stream));
  DPF_RETURN_IF_ERROR(s->out.Reserve(static_cast<size_t>(Q * stride)));
  char* sel = static_cast<char*>(s->out.get());
  for (int64_t i = 0; i < slab.slabs; ++i) {
    for (int64_t q = 0; q < Q; ++q)
      DPF_RETURN_IF_ERROR(ExpandSubtree(sub[q], i, desc, cepb, up, sel + q * stride, stream));
    HIP_RETURN_IF_ERROR(dpf_hip_select_rows(
        slab.slab_rows, W, static_cast<int>(Q), sel, stride,
        static_cast<const char*>(device_db) + i * slab.slab_rows * 8 * W, i > 0, s->workspace.get(),
        device_out, stream));
  }
  DPF_RETURN_IF_ERROR(s->workspace_fence.Mark(stream));
  DPF_RETURN_IF_ERROR(up.MarkUsed(stream));
  return Q * record_words;
}

StatusOr<std::vector<uint64_t>> DistributedPointFunction::EvaluateSelect(
    Span<const DpfKey* const> keys, int hierarchy_level, const void* device_db, int64_t db_bytes,
    int64_t record_words) const {
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);
  // Checked before the result buffer is allocated: host errors touch no device.
  DPF_RETURN_IF_ERROR(CheckSelectArgs(keys, hierarchy_level, 0, 1, device_db, db_bytes,
                                      record_words, /*device_out=*/this,
                                      std::numeric_limits<int64_t>::max(), /*shape=*/nullptr));
  const size_t words = keys.size() * static_cast<size_t>(record_words);
  DPF_RETURN_IF_ERROR(s->gathered.Reserve(words * 8));
  DPF_RETURN_IF_ERROR(EvaluateSelectToDevice(keys, hierarchy_level, 0, 1, device_db, db_bytes,
                                             record_words, s->gathered.get(),
                                             static_cast<int64_t>(words * 8), nullptr)
                          .status());
  std::vector<uint64_t> out(words);
  HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(out.data(), s->gathered.get(), words * 8, nullptr));
  return out;
}

// Additive-share PIR batched over queries: the streamed path of
// EvaluateSelectToDevice with 64 bits per record and query instead of one.
// The keys are taken a tile at a time, and the shard is cut into slabs of
// whole leaf blocks of which a tile's share rows fit the scratch bound
// together; every key's slab is expanded by the unchanged dpf_hip_expand into
// its row of the scratch, and dpf_hip_dot_rows_batch folds the slab of the
// database into the tile's answers at once.  DPF_DOT_BATCH_SLAB_LOG (read per
// call; test hook) sets the log2 of a slab's records instead.
Status DistributedPointFunction::CheckDotBatchArgs(
    Span<const DpfKey* const> keys, int hierarchy_level, int64_t shard, int64_t num_shards,
    const void* device_db, int64_t db_bytes, int64_t record_words, const void* device_out,
    int64_t out_bytes, SelectShape* shape) const {
  DPF_RETURN_IF_ERROR(CheckLevel(hierarchy_level, parameters().size()));
  const dpf_internal::FlatValueType& f = flat_[hierarchy_level];
  const dpf_value_desc desc = MakeDesc(f, blocks_needed_[hierarchy_level]);
  if (dpf_hip_dot_rows_batch_workspace_bytes(&desc, 1, 1) < 0)
    return UnimplementedError(
        "the batched database fold is implemented for uint64_t and XorWrapper<uint64_t> only");
  // The cap of EvaluateDotToDevice: one record per element.
  const int stop_level = hierarchy_to_tree()[hierarchy_level];
  DPF_ASSIGN_OR_RETURN(const int k, dpf_internal::ShardLevels(
                                        shard, num_shards, stop_level,
                                        parameters()[hierarchy_level].log_domain_size(), 0));
  DPF_RETURN_IF_ERROR(CheckRecordWords(record_words));
  const int64_t Q = static_cast<int64_t>(keys.size());
  if (Q < 1 || Q > DPF_HIP_DOT_BATCH_MAX_QUERIES)
    return InvalidArgumentError("`keys` must hold between 1 and 64 keys");
  const int64_t rows =
      (int64_t{1} << (stop_level - k)) * corrected_elements_per_block(hierarchy_level);
  if (shape) *shape = SelectShape{k, stop_level, rows};
  if (rows > (std::numeric_limits<int64_t>::max() / (8 * record_words)) ||
      db_bytes < rows * 8 * record_words)
    return InvalidArgumentError("database buffer too small");
  if (out_bytes < Q * record_words * 8)
    return InvalidArgumentError("device output buffer too small");
  if (!device_db || !device_out)
    return InvalidArgumentError("`device_db` and `device_out` must not be null");
  for (int64_t q = 0; q < Q; ++q) {
    if (!keys[q])
      return InvalidArgumentError("`keys[" + std::to_string(q) + "]` must not be null");
    if (Status st = validator_->ValidateDpfKey(*keys[q]); !st.ok())
      return Status(st.code(), "DpfKey " + std::to_string(q) + ": " + st.message());
  }
  return OkStatus();
}

StatusOr<int64_t> DistributedPointFunction::EvaluateDotBatchToDevice(
    Span<const DpfKey* const> keys, int hierarchy_level, int64_t shard, int64_t num_shards,
    const void* device_db, int64_t db_bytes, int64_t record_words, void* device_out,
    int64_t out_bytes, void* stream) const {
  SelectShape shape;
  DPF_RETURN_IF_ERROR(CheckDotBatchArgs(keys, hierarchy_level, shard, num_shards, device_db,
                                        db_bytes, record_words, device_out, out_bytes, &shape));
  const dpf_value_desc desc = MakeDesc(flat_[hierarchy_level], blocks_needed_[hierarchy_level]);
  const int cepb = corrected_elements_per_block(hierarchy_level);
  const int W = static_cast<int>(record_words);
  const int64_t Q = static_cast<int64_t>(keys.size());
  // The keys go through the scratch a tile at a time: the database is read
  // once per tile whatever the scratch holds, and the fewer share rows lie in
  // it together, the larger the slabs and the fewer, larger expansions a call
  // takes.  DPF_DOT_BATCH_TILE=<t> (read per call; A/B hook) sets the tile.
  const int64_t T = std::min<int64_t>(
      std::min<int64_t>(Q, TileHook("DPF_DOT_BATCH_TILE", DotBatchHostTile(record_words))),
      DPF_HIP_DOT_BATCH_MAX_QUERIES);
  const int workspace_bytes =
      dpf_hip_dot_rows_batch_workspace_bytes(&desc, W, static_cast<int>(T));
  if (workspace_bytes < 0) return InvalidArgumentError(dpf_hip_last_error());

  // Slabs of whole leaf blocks whose T rows of 64-bit shares fit the scratch bound.
  DPF_ASSIGN_OR_RETURN(const dpf_internal::SlabPlan slab,
                       dpf_internal::PlanSlabs(shape.rows, cepb, 64 * T,
                                               SlabLogHook("DPF_DOT_BATCH_SLAB_LOG")));
  const int64_t stride = (slab.slab_rows * 8 + 15) & ~int64_t{15};   // bytes of a key's share row

  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  // One image for all keys: the slabs' paths once, then each key's parts.
  PackedUploads& up = NextShardImage(*s);
  DPF_RETURN_IF_ERROR(up.Reset());
  const size_t o_path = AddSubtreePaths(shard, slab.j, up);
  std::vector<SubtreeParts> sub(Q);
  for (int64_t q = 0; q < Q; ++q) {
    DPF_ASSIGN_OR_RETURN(std::vector<uint128> vcw, ValueCorrectionLeaves(*keys[q], hierarchy_level));
    sub[q] = AddSubtreeParts(*keys[q], slab.slabs, shape.k + slab.j, shape.stop_level, vcw, up);
  }
  DPF_RETURN_IF_ERROR(up.Commit(stream));
  for (int64_t q = 0; q < Q; ++q) DPF_RETURN_IF_ERROR(WalkSubtreeRoots(sub[q], o_path, up, stream));
  DPF_RETURN_IF_ERROR(s->workspace_fence.Acquire(s->workspace, workspace_bytes, stream));
  DPF_RETURN_IF_ERROR(s->out.Reserve(static_cast<size_t>(T * stride)));
  char* y = static_cast<char*>(s->out.get());
  for (int64_t i = 0; i < slab.slabs; ++i) {
    for (int64_t q0 = 0; q0 < Q; q0 += T) {
      const int64_t nq = std::min(T, Q - q0);
      for (int64_t q = 0; q < nq; ++q)
        DPF_RETURN_IF_ERROR(
            ExpandSubtree(sub[q0 + q], i, desc, cepb, up, y + q * stride, stream));
      HIP_RETURN_IF_ERROR(dpf_hip_dot_rows_batch(
          slab.slab_rows, W, static_cast<int>(nq), &desc, y, stride,
          static_cast<const char*>(device_db) + i * slab.slab_rows * 8 * W, i > 0,
          s->workspace.get(), static_cast<uint64_t*>(device_out) + q0 * W, stream));
    }
  }
  DPF_RETURN_IF_ERROR(s->workspace_fence.Mark(stream));
  DPF_RETURN_IF_ERROR(up.MarkUsed(stream));
  return Q * record_words;
}

StatusOr<std::vector<uint64_t>> DistributedPointFunction::EvaluateDotBatch(
    Span<const DpfKey* const> keys, int hierarchy_level, const void* device_db, int64_t db_bytes,
    int64_t record_words) const {
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);
  // Checked before the result buffer is allocated: host errors touch no device.
  DPF_RETURN_IF_ERROR(CheckDotBatchArgs(keys, hierarchy_level, 0, 1, device_db, db_bytes,
                                        record_words, /*device_out=*/this,
                                        std::numeric_limits<int64_t>::max(), /*shape=*/nullptr));
  const size_t words = keys.size() * static_cast<size_t>(record_words);
  DPF_RETURN_IF_ERROR(s->gathered.Reserve(words * 8));
  DPF_RETURN_IF_ERROR(EvaluateDotBatchToDevice(keys, hierarchy_level, 0, 1, device_db, db_bytes,
                                               record_words, s->gathered.get(),
                                               static_cast<int64_t>(words * 8), nullptr)
                          .status());
  std::vector<uint64_t> out(words);
  HIP_RETURN_IF_ERROR(dpf_hip_memcpy_d2h(out.data(), s->gathered.get(), words * 8, nullptr));
  return out;
}

namespace {
// Host-phase timing of EvaluateAt, printed at exit when DPF_HOST_TIMING is
// set (the first 10 calls, allocations and page-locked buffers, not counted):
// checks = the fused domain check + path / block-index pass over the points,
// key = key validation, value correction, context lookups and correction
// words, upload = the one packed H2D, launch = the point kernel's launch,
// device = waiting for the upload and the kernel (timing runs only: the
// stream is synchronised there), copy = the D2H into the caller's vector
// (unpacked chunk by chunk).
dpf_internal::PhaseTimer g_at_timing(
    "DPF_HOST_TIMING", 10, [](long calls, double n, const double* t) {
      std::fprintf(stderr,
                   "[EvaluateAt host timing] calls=%ld per call: checks=%.2fus key=%.2fus "
                   "upload=%.2fus launch=%.2fus device=%.2fus copy=%.2fus\n",
                   calls, t[0] * 1e6 / n, t[1] * 1e6 / n, t[2] * 1e6 / n, t[3] * 1e6 / n,
                   t[4] * 1e6 / n, t[5] * 1e6 / n);
    });

// First index in [0, n) whose point exceeds max_point (n if none), found on
// host threads while `fill(lo, hi)` writes the kernel's per-point arrays.
template <typename Fill>
int64_t CheckAndFillPoints(Span<const uint128> points, uint128 max_point, Fill fill) {
  const int64_t n = static_cast<int64_t>(points.size());
  std::atomic<int64_t> bad{n};
  dpf_internal::ParallelFor(
      n,
      [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i)
          if (points[i] > max_point) {
            int64_t cur = bad.load();
            while (i < cur && !bad.compare_exchange_weak(cur, i)) {
            }
            return;
          }
        fill(lo, hi);
      },
      int64_t{1} << 16);
  return bad.load();
}
}  // namespace

Status DistributedPointFunction::EvaluateAtToHost(const DpfKey& key, int hierarchy_level,
                                                  Span<const uint128> evaluation_points,
                                                  EvaluationContext* ctx,
                                                  const ValueType* requested_type,
                                                  const HostSink& sink) const {
  // h:839-1010
  g_at_timing.count_call();
  dpf_internal::PhaseTimer::Clock clk(g_at_timing);
  if (ctx != nullptr && &key != &ctx->key())
    return InvalidArgumentError("`key` and `ctx->key()` must refer to the same object");
  if (hierarchy_level < 0) return InvalidArgumentError("`hierarchy_level` must be non-negative");
  if (hierarchy_level >= static_cast<int>(parameters().size()))
    return InvalidArgumentError(
        "`hierarchy_level` must be less than the number of parameters passed at construction");
  if (requested_type) {
    // EvaluateAt<T> converts with T; a mismatching T is reported like EvaluateUntil does.
    DPF_ASSIGN_OR_RETURN(bool eq, dpf_internal::ValueTypesAreEqual(
                                      *requested_type, parameters()[hierarchy_level].value_type()));
    if (!eq) return InvalidArgumentError("Value type T doesn't match parameters at `hierarchy_level`");
  }
  const int64_t n = static_cast<int64_t>(evaluation_points.size());
  const int log_domain_size = parameters()[hierarchy_level].log_domain_size();
  const uint128 max_point =
      log_domain_size < 128 ? (static_cast<uint128>(1) << log_domain_size) - 1 : Uint128Max();
  const dpf_internal::FlatValueType& f = flat_[hierarchy_level];
  const int E = f.elements_per_block;
  const int stop_level = hierarchy_to_tree()[hierarchy_level];
  const int bib = log_domain_size - stop_level;
  const int start_level = ctx ? stop_level : 0;
  const int L = stop_level - start_level;
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  PackedUploads& up = s->packed;
  DPF_RETURN_IF_ERROR(up.Reset());
  // The domain check (h:861-874), tree indices and block indices (h:907-925)
  // in ONE pass on host threads, written straight into the page-locked
  // upload image.
  const size_t nvcw = static_cast<size_t>(E) * f.leaves.size();
  up.Prepare(7 * 256 + static_cast<size_t>(n) * (sizeof(dpf_block) + sizeof(int32_t)) +
             static_cast<size_t>(L + 1) * (sizeof(dpf_block) + 2) + nvcw * sizeof(dpf_block) + 32);
  size_t o_paths, o_bi;
  dpf_block* paths = up.Reserve<dpf_block>(n, &o_paths);
  int32_t* block_index = up.Reserve<int32_t>(n, &o_bi);
  const uint128 bmask = (static_cast<uint128>(1) << bib) - 1;
  const int64_t bad = CheckAndFillPoints(evaluation_points, max_point, [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i) {
      const uint128 x = evaluation_points[i];
      paths[i] = ToBlock(E > 1 ? x >> bib : x);
      block_index[i] = E > 1 ? static_cast<int32_t>(x & bmask) : 0;
    }
  });
  if (bad < n)
    return InvalidArgumentError("`evaluation_points[" + std::to_string(bad) +
                                "]` larger than the domain size at hierarchy level " +
                                std::to_string(hierarchy_level));
  clk.mark(0);
  DPF_RETURN_IF_ERROR(validator_->ValidateDpfKey(key));
  if (n == 0) {
    (void)sink.reserve(0);
    return OkStatus();
  }
  DPF_ASSIGN_OR_RETURN(std::vector<uint128> vcw, ValueCorrectionLeaves(key, hierarchy_level));
  DeviceStart start;
  if (ctx) {
    // The tree indices, as uint128 memory images (paths is 256-byte aligned).
    const Span<const uint128> tree_indices(reinterpret_cast<const uint128*>(paths),
                                           static_cast<size_t>(n));
    DPF_RETURN_IF_ERROR(ComputePartialEvaluations(tree_indices, hierarchy_level,
                                                  /*update_ctx=*/true, *ctx, &start, nullptr,
                                                  nullptr));
  }
  const dpf_block root = ToBlock(FromProtoBlock(key.seed()));
  const uint8_t party = static_cast<uint8_t>(key.party() & 1);
  const PackedCws o_cw = AddCorrectionWords(key, start_level, stop_level, up);
  const size_t o_vcw = AddLeafBlocks(vcw, up);
  const size_t o_root = up.Add(&root, 1);
  const size_t o_party = up.Add(&party, 1);
  clk.mark(1);
  DPF_RETURN_IF_ERROR(up.Commit(nullptr));
  const size_t bytes = static_cast<size_t>(n) * f.packed_size;
  void* small = s->small_out.Get(bytes);   // small results: written to page-locked memory
  if (!small) DPF_RETURN_IF_ERROR(s->out.Reserve(bytes));
  void* const out = small ? small : s->out.get();
  clk.mark(2);
  const dpf_value_desc desc = MakeDesc(f, blocks_needed_[hierarchy_level]);
  const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight), kv = AesKey(kPrgKeyValue);
  HIP_RETURN_IF_ERROR(dpf_hip_eval_points(
      n, n, L, up.Ptr<dpf_block>(o_root), up.Ptr<uint8_t>(o_party),
      ctx ? start.seeds : nullptr, ctx ? start.ctrl : nullptr, up.Ptr<dpf_block>(o_paths),
      up.Ptr<int32_t>(o_bi), up.Ptr<dpf_block>(o_cw.seed), up.Ptr<uint8_t>(o_cw.left),
      up.Ptr<uint8_t>(o_cw.right), &kl, &kr, &kv, &desc, up.Ptr<dpf_block>(o_vcw), out, nullptr));
  DPF_RETURN_IF_ERROR(up.MarkUsed(nullptr));
  if (ctx) DPF_RETURN_IF_ERROR(s->packed_pe.MarkUsed(nullptr));   // start seeds read from it
  clk.mark(3);
  if (g_at_timing.on()) {
    HIP_RETURN_IF_ERROR(dpf_hip_stream_sync(nullptr));
    clk.mark(4);
  }
  // Packed elements straight into the caller's result (h:983-1003 outputs):
  // integers copied, tuples / IntModN / XorWrapper unpacked chunk by chunk out
  // of the page-locked staging buffers.
  if (small) {
    DPF_RETURN_IF_ERROR(dpf_internal::ConsumePinnedOut(sink, small, bytes, nullptr));
  } else {
    HIP_RETURN_IF_ERROR(dpf_internal::CopyToHostSink(sink, sink.reserve(bytes), s->out.get(), bytes,
                                                     nullptr));
  }
  clk.mark(5);
  if (ctx) ctx->set_previous_hierarchy_level(hierarchy_level);
  return OkStatus();
}

StatusOr<std::vector<uint8_t>> DistributedPointFunction::EvaluateAtPacked(
    const DpfKey& key, int hierarchy_level, Span<const uint128> evaluation_points,
    EvaluationContext* ctx, const ValueType* requested_type) const {
  std::vector<uint8_t> out;
  DPF_RETURN_IF_ERROR(EvaluateAtToHost(key, hierarchy_level, evaluation_points, ctx,
                                       requested_type, dpf_internal::VectorSink(&out)));
  return out;
}

StatusOr<std::vector<uint8_t>> DistributedPointFunction::EvaluateAtBatchPacked(
    Span<const DpfKey* const> keys, int hierarchy_level, Span<const uint128> points,
    int64_t points_per_key) const {
  if (hierarchy_level < 0 || hierarchy_level >= static_cast<int>(parameters().size()))
    return InvalidArgumentError("`hierarchy_level` out of range");
  const int64_t num_keys = static_cast<int64_t>(keys.size());
  if (points_per_key < 1 || static_cast<int64_t>(points.size()) != num_keys * points_per_key)
    return InvalidArgumentError("points.size() must equal keys.size() * points_per_key");
  const int log_domain_size = parameters()[hierarchy_level].log_domain_size();
  const uint128 max_point =
      log_domain_size < 128 ? (static_cast<uint128>(1) << log_domain_size) - 1 : Uint128Max();
  const int64_t n = static_cast<int64_t>(points.size());
  const dpf_internal::FlatValueType& f = flat_[hierarchy_level];
  const int E = f.elements_per_block, nl = static_cast<int>(f.leaves.size());
  const int L = hierarchy_to_tree()[hierarchy_level];
  const int bib = log_domain_size - L;
  auto* s = scratch_.get();
  std::lock_guard<std::recursive_mutex> scratch_lock(s->mu);  // one call at a time per object
  PackedUploads& up = s->packed;
  DPF_RETURN_IF_ERROR(up.Reset());
  const int64_t rows = std::max<int64_t>(num_keys * L, 1);
  up.Prepare(9 * 256 + static_cast<size_t>(n) * (sizeof(dpf_block) + sizeof(int32_t)) +
             static_cast<size_t>(num_keys) * (sizeof(dpf_block) + 1 + E * nl * sizeof(dpf_block)) +
             static_cast<size_t>(rows) * (sizeof(dpf_block) + 2) + 64);
  // The points: domain check, tree indices and block indices in one threaded
  // pass into the upload image (EvaluateAt's order: points before keys).
  size_t o_paths, o_bi;
  dpf_block* paths = up.Reserve<dpf_block>(n, &o_paths);
  int32_t* block_index = up.Reserve<int32_t>(n, &o_bi);
  const uint128 bmask = (static_cast<uint128>(1) << bib) - 1;
  const int64_t bad = CheckAndFillPoints(points, max_point, [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; ++i) {
      paths[i] = ToBlock(E > 1 ? points[i] >> bib : points[i]);
      block_index[i] = E > 1 ? static_cast<int32_t>(points[i] & bmask) : 0;
    }
  });
  if (bad < n)
    return InvalidArgumentError("`evaluation_points[" + std::to_string(bad) +
                                "]` larger than the domain size at hierarchy level " +
                                std::to_string(hierarchy_level));
  if (n == 0) return std::vector<uint8_t>{};
  // The keys: validated and flattened (SoA, [key][level]) on host threads;
  // the first failing key's error is returned.
  size_t o_seed, o_party, o_cws, o_cl, o_cr, o_vcw;
  dpf_block* seeds = up.Reserve<dpf_block>(num_keys, &o_seed);
  uint8_t* party = up.Reserve<uint8_t>(num_keys, &o_party);
  dpf_block* cw_seed = up.Reserve<dpf_block>(rows, &o_cws);
  uint8_t* cl = up.Reserve<uint8_t>(rows, &o_cl);
  uint8_t* cr = up.Reserve<uint8_t>(rows, &o_cr);
  dpf_block* vcw = up.Reserve<dpf_block>(std::max<int64_t>(num_keys * E * nl, 1), &o_vcw);
  std::atomic<int64_t> first_bad{num_keys};
  dpf_internal::ParallelFor(
      num_keys,
      [&](int64_t lo, int64_t hi) {
        for (int64_t k = lo; k < hi; ++k) {
          const DpfKey& key = *keys[k];
          StatusOr<std::vector<uint128>> v = validator_->ValidateDpfKey(key).ok()
                                                 ? ValueCorrectionLeaves(key, hierarchy_level)
                                                 : StatusOr<std::vector<uint128>>(
                                                       InvalidArgumentError("invalid key"));
          if (!v.ok()) {
            int64_t cur = first_bad.load();
            while (k < cur && !first_bad.compare_exchange_weak(cur, k)) {
            }
            return;
          }
          seeds[k] = ToBlock(FromProtoBlock(key.seed()));
          party[k] = static_cast<uint8_t>(key.party() & 1);
          for (int j = 0; j < L; ++j) {
            const CorrectionWord& cw = key.correction_words(j);
            cw_seed[k * L + j] = ToBlock(FromProtoBlock(cw.seed()));
            cl[k * L + j] = cw.control_left();
            cr[k * L + j] = cw.control_right();
          }
          for (int i = 0; i < E * nl; ++i) vcw[k * E * nl + i] = ToBlock((*v)[i]);
        }
      },
      int64_t{256});
  if (first_bad.load() < num_keys) {
    // The failing key's own error, as the one-by-one loop reported it.
    const DpfKey& key = *keys[first_bad.load()];
    DPF_RETURN_IF_ERROR(validator_->ValidateDpfKey(key));
    return ValueCorrectionLeaves(key, hierarchy_level).status();
  }
  DPF_RETURN_IF_ERROR(up.Commit(nullptr));
  const size_t bytes = static_cast<size_t>(n) * f.packed_size;
  DPF_RETURN_IF_ERROR(s->out.Reserve(bytes));
  const dpf_value_desc desc = MakeDesc(f, blocks_needed_[hierarchy_level]);
  const dpf_aes_key kl = AesKey(kPrgKeyLeft), kr = AesKey(kPrgKeyRight), kv = AesKey(kPrgKeyValue);
  HIP_RETURN_IF_ERROR(dpf_hip_eval_points(
      n, points_per_key, L, up.Ptr<dpf_block>(o_seed), up.Ptr<uint8_t>(o_party), nullptr, nullptr,
      up.Ptr<dpf_block>(o_paths), up.Ptr<int32_t>(o_bi), up.Ptr<dpf_block>(o_cws),
      up.Ptr<uint8_t>(o_cl), up.Ptr<uint8_t>(o_cr), &kl, &kr, &kv, &desc,
      up.Ptr<dpf_block>(o_vcw), s->out.get(), nullptr));
  DPF_RETURN_IF_ERROR(up.MarkUsed(nullptr));
  std::vector<uint8_t> out;
  HIP_RETURN_IF_ERROR(CopyToHostVector(&out, s->out.get(), bytes, nullptr));
  return out;
}

}  // namespace distributed_point_functions
