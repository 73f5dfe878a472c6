// rt_records.h -- the child reference of an inner record (traverse_bvh semantics,
// volumeRender.cl:829-856), shared by everything that writes or reads one: the host encoding
// (csrc/host/scene_encode.cpp), the render kernels, the refit, the on-GPU scene build and the
// SAH query.  Plain C++: constexpr only, so it compiles for host and device alike.
//
//   inner child:  the id of its record (< 2^31)
//   leaf child:   kLeafBit | count << 26 | offset of its first triangle reference record;
//                 count kCntEscape: the low 26 bits index the escape table {offset, count}
//   kRefError:    a malformed inner node; popped -> traversal returns -1
#pragma once
#include <cstdint>

namespace rtrec {

constexpr uint32_t kLeafBit = 0x80000000u;
constexpr uint32_t kRefError = 0x7FFFFFFFu;
constexpr uint32_t kCntEscape = 31u;
constexpr uint32_t kCntShift = 26;
constexpr uint32_t kOffMask = 0x03FFFFFFu;
constexpr uint32_t kOffLimit = 1u << kCntShift;   // offsets and escape entries stay below it

constexpr uint32_t leaf_ref(uint32_t cnt, uint32_t off) { return kLeafBit | (cnt << kCntShift) | off; }
constexpr uint32_t ref_count(uint32_t ref) { return (ref >> kCntShift) & 31u; }
constexpr uint32_t ref_offset(uint32_t ref) { return ref & kOffMask; }

}  // namespace rtrec
