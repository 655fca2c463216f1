// sortdedup_pack.h -- what other host translation units use of sortdedup_pack.cpp.
#pragma once
#include <cstdint>
namespace mgx {
// the Illumina tile / x / y fields of a qname (pair.cpp:22-49), strtol fallback included
void qname_tile_x_y(const char* q, uint64_t len, uint16_t out[3]);
}  // namespace mgx
