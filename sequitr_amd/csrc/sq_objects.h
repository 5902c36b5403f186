// What the object measurements (sq_objects.hip) and the shape columns (sq_objects_shape.hip) share: the layout of the
// measure call's workspace -- the per-object table, then parent and slot, 4 B per pixel each -- and the host-side record
// of which workspace was filled under which geometry.  The record lives in sq_objects.hip; the layout sits in an unnamed
// namespace like the other shared headers.
#pragma once
#include "sq_ccl.h"

namespace {

// one object's accumulators, 88 bytes; rows of the table at the start of the workspace
struct ObjAcc {
    u64 area, srow, scol, splane;                              // pixel count and the three coordinate sums
    u64 isum, isumsq;                                          // integer images: u64; float32 images: the bits of a double
    int lo[3], hi[3];                                          // box along (plane, row, column), hi exclusive
    unsigned imin, imax;                                       // integer images: the value; float32: ord_f32 of it
    int root, pad;
};
static_assert(sizeof(ObjAcc) == 88, "ObjAcc layout");

inline int64_t obj_table_bytes(int max_out) { return ((int64_t)max_out * (int64_t)sizeof(ObjAcc) + 15) / 16 * 16; }

}  // namespace

// what the last sq_objects_measure calls left in which workspace (host side): the entry points that read a workspace do
// so only under the geometry it was filled with
struct SqObjFilled {
    const void *workspace;
    int N, planes, H, W, max_out;
};
void sq_obj_remember(const void *workspace, int N, int planes, int H, int W, int max_out);
bool sq_obj_recall(const void *workspace, SqObjFilled *out);
