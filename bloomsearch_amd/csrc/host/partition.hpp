// partition.hpp — one row's partition text on the host (the mirror of csrc/partition.hip.h; contract: include/bloomgpu.h "keyed
// streaming ingest").  Exact for every row: json.hpp validate_object_row decodes every key and value, so this is what the rows a
// keyed ingest hands back are decided with, and what the engine has always partitioned by.  bsh_partition_key (host_api.cpp) is a
// shim over partition_key; tests/partition_scan_check.cpp runs it under the sanitizers.
#pragma once
#include <cstdint>
#include <string>
#include <string_view>

#include "json.hpp"

namespace bsh {

constexpr uint32_t kPartitionMaxName = 64;      // bloomgpu.h BSG_PARTITION_MAX_NAME

// false: the name is empty or too long, or the row is not one valid JSON object.  text: the FIRST top-level member with the key —
// a string's decoded bytes, a number's raw literal, "true" / "false"; empty for null, an object, an array or no such member.
inline bool partition_key(std::string_view row, std::string_view name, std::string &text)
{
    if (name.empty() || name.size() > kPartitionMaxName) return false;
    std::string scratch;
    bool has = false;
    if (!validate_object_row(row, name, text, has, scratch)) return false;
    if (!has) text.clear();
    return true;
}

}  // namespace bsh
