// The requested-type check of EvaluateDot<T> (EvaluateDotPacked), which only
// the C++ template reaches: with two faults at once it is reported after the
// hierarchy level and before `record_words`.  Host errors only: the database
// is a fake non-null address that nothing reads, so no GPU is needed.
#include <cstdint>
#include <cstdio>
#include <string>

#include "dpf/distributed_point_function.h"

namespace dpf = distributed_point_functions;

static int failures = 0;
static void Expect(const dpf::Status& got, const std::string& message, const char* what) {
  if (got.code() == dpf::StatusCode::kInvalidArgument && got.message() == message) return;
  std::printf("FAILED %s: got \"%s\"\n", what, got.ToString().c_str());
  ++failures;
}

int main() {
  dpf::DpfParameters p;
  p.set_log_domain_size(10);
  *p.mutable_value_type() = dpf::ToValueType<uint64_t>();
  auto f = dpf::DistributedPointFunction::Create(p);
  if (!f.ok()) return std::printf("Create: %s\n", f.status().ToString().c_str()), 1;
  auto keys = (*f)->GenerateKeys(3, uint64_t{1});
  if (!keys.ok()) return std::printf("GenerateKeys: %s\n", keys.status().ToString().c_str()), 1;
  const void* db = reinterpret_cast<const void*>(0x1000);
  const int64_t db_bytes = int64_t{1} << 13;
  const std::string level = "`hierarchy_level` must be non-negative and less than parameters_.size()";
  const std::string type = "Value type T doesn't match parameters at `hierarchy_level`";
  // Level out of range, T mismatching and record_words out of range: the level.
  Expect((*f)->EvaluateDot<uint32_t>(keys->first, 1, db, db_bytes, 0).status(), level,
         "level before type");
  // T mismatching with bad record_words, with a null database, with a short one: the type.
  Expect((*f)->EvaluateDot<uint32_t>(keys->first, 0, db, db_bytes, 1025).status(), type,
         "type before record_words");
  Expect((*f)->EvaluateDot<uint32_t>(keys->first, 0, nullptr, db_bytes, 1).status(), type,
         "type before null database");
  Expect((*f)->EvaluateDot<dpf::uint128>(keys->first, 0, db, db_bytes - 1, 1).status(), type,
         "type before database size");
  // The matching T goes on to the next check.
  Expect((*f)->EvaluateDot<uint64_t>(keys->first, 0, db, db_bytes, 1025).status(),
         "`record_words` must be in [1, 1024]", "matching type, record_words");
  std::printf("%d failures\n", failures);
  return failures != 0;
}
