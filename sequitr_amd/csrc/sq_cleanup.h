// What the clean-up entries check first (sq_maskops.hip, sq_volumeops.hip, sq_component_ops.hip, sq_split.hip), with a frame counted as
// a volume of one plane.  The two morphology kernels share no device code: the column-validity word and the start value
// of a 4-pixel group as functions left their registers, LDS and occupancy alone but made the planar launch 0.3-0.5 %
// slower, and the dilating-step rule and the merge of a plane's bits changed its register allocation.
#pragma once
#include "sq_ccl.h"

namespace {

inline bool ranges_overlap(const void *a, int64_t abytes, const void *b, int64_t bbytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)bbytes && y < x + (uintptr_t)abytes;
}

inline bool ranges_overlap(const void *a, const void *b, int64_t bytes) { return ranges_overlap(a, bytes, b, bytes); }

inline int64_t volume_elements(int N, int D, int H, int W) {   // -1: an extent < 1, or 2^31 or more elements
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0) return -1;
    const int64_t lim = (int64_t)1 << 31;
    int64_t total = (int64_t)N * D;                             // < 2^62
    if (total >= lim) return -1;
    total *= H;
    if (total >= lim) return -1;
    total *= W;
    return total >= lim ? -1 : total;
}

}  // namespace

// mask, out, N, H, W, C are the entry's arguments; D is its fourth extent, or 1 for a frame.  fmt and what follows print
// the extents as the entry takes them.
#define SQ_CLEANUP_COMMON(who, D, fmt, ...)                                                                              \
    SQ_REQUIRE(mask && out, "%s: null pointer", who);                                                                    \
    SQ_REQUIRE(C >= 2 && C <= 256, "%s: C must be 2 .. 256 classes, got %d", who, C);                                    \
    SQ_REQUIRE(volume_elements(N, D, H, W) > 0,                                                                          \
               "%s: the mask must have at least one and fewer than 2^31 elements, got " fmt, who, __VA_ARGS__);          \
    SQ_REQUIRE(!ranges_overlap(mask, out, volume_elements(N, D, H, W)), "%s: out must not overlap mask", who)
