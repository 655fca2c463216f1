// sam_host.h -- the reference-name table of SAM text input (include/mgx_sam.h) as its translation units see it: the host
// functions (sam_host.cpp) and the device batch (mgx_sam.hip), which uploads `blob` as it stands.
#pragma once
#include <cstdint>
#include <vector>

#include "cli/sam_text.h"

struct mgx_sam_table {
    std::vector<uint32_t> blob;            // the table of sam_line_core.h (table_view)
    samtext::Header header;                // the same names for the full parser, which completes the declined lines
};
