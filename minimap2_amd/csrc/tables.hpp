// Constant tables shared by host translation units (tables.cpp).
#pragma once
#include <cstdint>
namespace mm2amd {
// ASCII -> nt4: A/a 0, C/c 1, G/g 2, T/t/U/u 3, already-encoded 0..3 map to themselves, anything else 4
// (same mapping as the reference's seq_nt4_table, sketch.c:9-26)
extern const uint8_t kNt4Table[256];
} // namespace mm2amd
