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

// Walk references: a second form of an inner record's two child references, derived
// from the records of an installed scene and kept in a side array after the triangle records, 8 B
// per inner record.  One unit is 16 B of the record allocation (inner records, triangle records,
// walk array: below 2 GiB, so a unit offset has 27 bits), and a walk reference is the cursor the
// depth-1 traversal walks by, with nothing left to decode:
//   inner child:            the unit offset of its record, 4 * id
//   leaf child, 1..16 refs: kLeafBit | (count - 1) << 27 | unit offset of its first triangle record
//                           (escape leaves resolved); the cursor's next record is + 3 - (1 << 27),
//                           and a count field of 0 says that this record is the leaf's last
//   empty leaf:             kLeafBit | unit offset of the all-zero pad record after the last triangle record
//   kWalkNone:              not expressible (more than 16 references, kRefError, an escape entry or
//                           a record outside the arrays); a scene with one has no walk array
constexpr uint32_t kWalkCntShift = 27;
constexpr uint32_t kWalkMaxLeaf = 16;
constexpr uint32_t kWalkUnitMask = (1u << kWalkCntShift) - 1u;
constexpr uint32_t kWalkNone = 0x7FFFFFFFu;
constexpr uint32_t kWalkNext = 3u - (1u << kWalkCntShift);   // one triangle record on, one reference fewer
constexpr uint32_t kWalkLastBelow = kLeafBit | (1u << kWalkCntShift);   // a leaf cursor below it stands on its leaf's last record

// table: the escape leaves as {offset, count} pairs of int32 (n_table of them); tri_unit: the unit
// offset of the first triangle record (the inner records, n_rec of them, end there); n_refs: triangle
// reference records, with the pad record after the last.
constexpr uint32_t walk_ref(uint32_t ref, const int32_t* table, uint32_t n_table, uint32_t n_rec, uint32_t tri_unit, uint32_t n_refs) {
    if (!(ref & kLeafBit)) return ref < n_rec && ref < (1u << (kWalkCntShift - 2)) ? ref << 2 : kWalkNone;
    uint32_t off = ref_offset(ref), cnt = ref_count(ref);
    if (cnt == kCntEscape) {
        if (off >= n_table) return kWalkNone;
        const int32_t o = table[2 * off], c = table[2 * off + 1];
        if (o < 0 || c < 0) return kWalkNone;
        off = (uint32_t)o;
        cnt = (uint32_t)c;
    }
    if (cnt > kWalkMaxLeaf) return kWalkNone;
    if (cnt == 0) off = n_refs;   // the pad record
    else if (off > n_refs || cnt > n_refs - off) return kWalkNone;
    const uint64_t unit = (uint64_t)tri_unit + 3ull * off;
    if (unit + 3ull * (cnt ? cnt : 1u) > kWalkUnitMask) return kWalkNone;
    return kLeafBit | ((cnt ? cnt - 1u : 0u) << kWalkCntShift) | (uint32_t)unit;
}
constexpr uint32_t walk_unit(uint32_t w) { return w & kWalkUnitMask; }
constexpr uint32_t walk_count(uint32_t w) { return ((w >> kWalkCntShift) & 15u) + 1u; }   // of a leaf; an empty one reads 1: the pad

}  // namespace rtrec
