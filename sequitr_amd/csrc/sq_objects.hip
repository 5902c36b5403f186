// Mask (+ intensity image) -> connected components -> one row of measurements per object: area, bounding box, centre of
// mass, and the sum, sum of squares, minimum and maximum of the image under the object; optionally a label image and the
// mask with the objects outside a size range removed.  Labelling, connectivity and numbering are those of the centroid
// path (sq_ccl.h): a component's root is its first pixel in raster order.
//   1-3. row scan, merge, compress (sq_ccl.h): parent = root
//   4. slots      : every root draws a slot with one returning atomicAdd on `found` and initialises that row of the
//                   per-OBJECT accumulator table (the centroid path indexes its sums by pixel, 32 B/pixel; ~14 quantities
//                   that way would be > 100 B/pixel).  Per pixel there are only parent and slot, 8 B.
//   5. accumulate : one wave per image row; per run segment one group of atomics into the object's row.  With an image the
//                   segment's pixels are first reduced across its lanes (a segmented wave scan keyed on the run start).
//   6. emit       : every slot whose area lies in [min_area, max_area] writes one int64 and one float64 row
//   relabel (second entry point): labels = rank[slot[parent]], mask_out = mask where rank != 0
// Integer images (uint8 / uint16) accumulate sum and sum of squares in unsigned 64-bit integers: exact and independent of
// the order in which the atomics arrive.  float32 images accumulate them with float64 atomicAdd: every x*x is exact in
// float64, a run segment's partial sum is formed in a fixed order, but the segments of an object arrive in ANY order, so
// the last bits of sum and sumsq may differ from run to run.  Minimum and maximum of float32 images go through an
// order-preserving unsigned encoding and integer atomicMin / atomicMax: exact, and NaN pixels are left out of them (a NaN
// pixel makes sum and sumsq NaN).
#include "sq_objects.h"

#include <mutex>

namespace {

__device__ __forceinline__ unsigned ord_f32(float x) {          // a < b  <=>  ord(a) < ord(b), for all non-NaN a, b
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord_f32(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

__device__ __forceinline__ u64 shfl_up_u64(u64 v, int d) {
    const unsigned lo = (unsigned)__shfl_up((int)(unsigned)(v & 0xFFFFFFFFULL), d);
    const unsigned hi = (unsigned)__shfl_up((int)(unsigned)(v >> 32), d);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ double shfl_up_f64(double v, int d) {
    return __longlong_as_double((long long)shfl_up_u64((u64)__double_as_longlong(v), d));
}

__global__ __launch_bounds__(256) void obj_slots_kernel(const int *__restrict__ parent, int *__restrict__ slot,
                                                        ObjAcc *__restrict__ acc, int64_t total, int *__restrict__ found,
                                                        int max_out, int dtype) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        if (parent[g] != (int)g) continue;
        const int s = atomicAdd(found, 1);
        if (s >= max_out) {                                     // counted, not measured: the caller comes back with more room
            slot[g] = -1;
            continue;
        }
        slot[g] = s;
        ObjAcc a;
        a.area = a.srow = a.scol = a.splane = 0ULL;
        a.isum = a.isumsq = 0ULL;                               // also the bits of the double 0.0
        a.lo[0] = a.lo[1] = a.lo[2] = 0x7FFFFFFF;
        a.hi[0] = a.hi[1] = a.hi[2] = -1;
        a.imin = dtype == SQ_PIX_F32 ? ord_f32(INFINITY) : 0xFFFFFFFFu;
        a.imax = dtype == SQ_PIX_F32 ? ord_f32(-INFINITY) : 0u;
        a.root = (int)g;
        a.pad = 0;
        acc[s] = a;
    }
}

// PIX: -1 no image, else SQ_PIX_*
template <int PIX>
__global__ __launch_bounds__(256) void obj_accumulate_kernel(const uint8_t *__restrict__ mask, const void *__restrict__ image,
                                                             const int *__restrict__ parent, const int *__restrict__ slot,
                                                             ObjAcc *__restrict__ acc, int rows, int planes, int H, int W) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const uint8_t *row = mask + (size_t)r * W;
    const int base = r * W, rowi = r % H, plane = (r / H) % planes;
    int prev_last = 0;
    for (int c0 = 0; c0 < W; c0 += 64) {
        const SegScan s = seg_scan(row, W, c0, lane, prev_last);
        const bool next_same = __shfl_down((int)s.same, 1) != 0 && lane != 63;
        const int j = s.j >= 0 ? s.j : 0;                        // the part of the run inside this segment starts at lane j
        const int col = c0 + lane;
        // inclusive scan over the lanes j .. lane of my run segment; every lane takes part in the shuffles
        unsigned isum = 0, imin = 0xFFFFFFFFu, imax = 0u;
        u64 isq = 0;
        double fsum = 0.0, fsq = 0.0;
        if (PIX >= 0) {
            if (s.v != 0) {                                      // col < W here
                if (PIX == SQ_PIX_F32) {
                    const float x = reinterpret_cast<const float *>(image)[(size_t)base + col];
                    fsum = (double)x;
                    fsq = (double)x * (double)x;
                    if (x == x) imin = imax = ord_f32(x);
                    else { imin = ord_f32(INFINITY); imax = ord_f32(-INFINITY); }
                } else {
                    const unsigned x = PIX == SQ_PIX_U8 ? (unsigned)reinterpret_cast<const uint8_t *>(image)[(size_t)base + col]
                                                        : (unsigned)reinterpret_cast<const uint16_t *>(image)[(size_t)base + col];
                    isum = x;
                    isq = (u64)x * (u64)x;
                    imin = imax = x;
                }
            }
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const bool take = s.v != 0 && lane - d >= j;
                if (PIX == SQ_PIX_F32) {
                    const double a = shfl_up_f64(fsum, d), b = shfl_up_f64(fsq, d);
                    if (take) { fsum += a; fsq += b; }
                } else {
                    const unsigned a = (unsigned)__shfl_up((int)isum, d);
                    const u64 b = shfl_up_u64(isq, d);
                    if (take) { isum += a; isq += b; }
                }
                const unsigned mn = (unsigned)__shfl_up((int)imin, d), mx = (unsigned)__shfl_up((int)imax, d);
                if (take) {
                    imin = mn < imin ? mn : imin;
                    imax = mx > imax ? mx : imax;
                }
            }
        }
        if (s.v != 0 && !next_same) {                           // last lane of a run segment
            const unsigned len = (unsigned)(lane - j + 1);
            const int sl = slot[parent[base + col]];
            if (sl >= 0) {
                ObjAcc *a = acc + sl;
                atomicAdd(&a->area, (u64)len);
                atomicAdd(&a->srow, (u64)len * (u64)rowi);
                atomicAdd(&a->scol, (u64)len * (u64)(2 * c0 + lane + j) / 2ULL);
                atomicMin(&a->lo[1], rowi);
                atomicMax(&a->hi[1], rowi + 1);
                atomicMin(&a->lo[2], c0 + j);
                atomicMax(&a->hi[2], col + 1);
                if (planes > 1) {
                    atomicAdd(&a->splane, (u64)len * (u64)plane);
                    atomicMin(&a->lo[0], plane);
                    atomicMax(&a->hi[0], plane + 1);
                }
                if (PIX == SQ_PIX_F32) {
                    atomicAdd(reinterpret_cast<double *>(&a->isum), fsum);
                    atomicAdd(reinterpret_cast<double *>(&a->isumsq), fsq);
                } else if (PIX >= 0) {
                    atomicAdd(&a->isum, (u64)isum);
                    atomicAdd(&a->isumsq, isq);
                }
                if (PIX >= 0) {
                    atomicMin(&a->imin, imin);
                    atomicMax(&a->imax, imax);
                }
            }
        }
        prev_last = __shfl(s.v, 63);
    }
}

__global__ __launch_bounds__(256) void obj_emit_kernel(const uint8_t *__restrict__ mask, const ObjAcc *__restrict__ acc,
                                                       const int *__restrict__ found, int planes, int H, int W, int dtype,
                                                       long long min_area, long long max_area, int *__restrict__ count,
                                                       long long *__restrict__ rows_i, double *__restrict__ rows_f,
                                                       int *__restrict__ slots, int max_out) {
    const int n = found[0] < max_out ? found[0] : max_out;
    const int64_t per_frame = (int64_t)planes * H * W;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
        const ObjAcc a = acc[s];
        const long long area = (long long)a.area;
        if (area < min_area || (max_area > 0 && area > max_area)) continue;
        const int idx = atomicAdd(count, 1);                    // idx < n <= max_out
        const int cls = mask[a.root];
        long long *ri = rows_i + 12 * (size_t)idx;
        double *rf = rows_f + 7 * (size_t)idx;
        ri[0] = a.root / per_frame;
        ri[1] = cls;
        ri[2] = a.root % per_frame;
        ri[3] = area;
        ri[4] = planes > 1 ? a.lo[0] : 0;
        ri[5] = a.lo[1];
        ri[6] = a.lo[2];
        ri[7] = planes > 1 ? a.hi[0] : 1;
        ri[8] = a.hi[1];
        ri[9] = a.hi[2];
        const bool integer = dtype == SQ_PIX_U8 || dtype == SQ_PIX_U16;
        ri[10] = integer ? (long long)a.isum : 0;
        ri[11] = integer ? (long long)a.isumsq : 0;
        // scipy.ndimage.center_of_mass(out, labels, index): sum(out * grid) / sum(out) in float64, out == c
        const double c = (double)cls, norm = c * (double)a.area;
        rf[0] = c * (double)a.splane / norm;
        rf[1] = c * (double)a.srow / norm;
        rf[2] = c * (double)a.scol / norm;
        if (integer) {
            rf[3] = (double)a.isum;
            rf[4] = (double)a.isumsq;
            rf[5] = (double)a.imin;
            rf[6] = (double)a.imax;
        } else if (dtype == SQ_PIX_F32) {
            rf[3] = __longlong_as_double((long long)a.isum);
            rf[4] = __longlong_as_double((long long)a.isumsq);
            rf[5] = (double)unord_f32(a.imin);
            rf[6] = (double)unord_f32(a.imax);
        } else {
            rf[3] = rf[4] = rf[5] = rf[6] = 0.0;
        }
        slots[idx] = s;
    }
}

__global__ __launch_bounds__(256) void obj_relabel_kernel(const uint8_t *__restrict__ mask, const int *__restrict__ parent,
                                                          const int *__restrict__ slot, const int *__restrict__ rank,
                                                          int n_slots, int64_t total, int *__restrict__ labels,
                                                          uint8_t *__restrict__ mask_out) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int p = parent[g];
        int rk = 0;
        if (p >= 0) {
            const int s = slot[p];
            if (s >= 0 && s < n_slots) rk = rank[s];
        }
        if (labels) labels[g] = rk;
        if (mask_out) mask_out[g] = rk ? mask[g] : (uint8_t)0;
    }
}

// sq_objects.h: sq_objects_relabel and sq_objects_shape read a workspace only under the geometry it was filled with
typedef SqObjFilled ObjFilled;
std::mutex obj_filled_lock;
ObjFilled obj_filled[16];
unsigned obj_filled_next = 0;

}  // namespace

void sq_obj_remember(const void *workspace, int N, int planes, int H, int W, int max_out) {
    std::lock_guard<std::mutex> hold(obj_filled_lock);
    ObjFilled *e = nullptr;
    for (ObjFilled &f : obj_filled)
        if (f.workspace == workspace) e = &f;
    if (!e) e = &obj_filled[obj_filled_next++ % 16];
    *e = ObjFilled{workspace, N, planes, H, W, max_out};
}

bool sq_obj_recall(const void *workspace, SqObjFilled *out) {
    std::lock_guard<std::mutex> hold(obj_filled_lock);
    for (const ObjFilled &f : obj_filled)
        if (f.workspace == workspace) {
            *out = f;
            return true;
        }
    return false;
}

extern "C" int64_t sq_objects_workspace(int N, int planes, int H, int W, int max_out) {
    if (N <= 0 || planes <= 0 || H <= 0 || W <= 0 || max_out <= 0) return -1;
    const int64_t total = (int64_t)N * planes * H * W;
    if (total >= ((int64_t)1 << 31)) return -1;
    return obj_table_bytes(max_out) + total * 8;               // the table, then parent and slot
}

extern "C" int sq_objects_measure(const uint8_t *mask, int N, int planes, int H, int W, const void *image, int dtype,
                                  int64_t min_area, int64_t max_area, void *workspace, int32_t *count, int32_t *found,
                                  int64_t *rows_i, double *rows_f, int32_t *slots, int max_out, void *stream) {
    const char *who = "sq_objects_measure";
    SQ_REQUIRE(mask && workspace && count && found && rows_i && rows_f && slots, "%s: null pointer", who);
    SQ_REQUIRE(!image || dtype == SQ_PIX_U8 || dtype == SQ_PIX_U16 || dtype == SQ_PIX_F32,
               "%s: the image dtype must be SQ_PIX_U8, SQ_PIX_U16 or SQ_PIX_F32, got %d", who, dtype);
    SQ_REQUIRE(min_area >= 1, "%s: min_area must be at least 1, got %lld", who, (long long)min_area);
    SQ_REQUIRE(max_out >= 1, "%s: max_out must be at least 1, got %d", who, max_out);
    SQ_REQUIRE(N > 0 && planes > 0 && H > 0 && W > 0 && (int64_t)N * planes * H * W < ((int64_t)1 << 31),
               "%s: the mask must have fewer than 2^31 elements", who);
    SQ_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "%s: workspace must be 16-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = (int64_t)N * planes * H * W;
    ObjAcc *acc = reinterpret_cast<ObjAcc *>(workspace);
    int *parent = reinterpret_cast<int *>(reinterpret_cast<char *>(workspace) + obj_table_bytes(max_out));
    int *slot = parent + total;
    const int rows = N * planes * H;
    const int pix = image ? dtype : -1;
    sq_obj_remember(workspace, N, planes, H, W, max_out);
    if (hipMemsetAsync(count, 0, sizeof(int32_t), st) != hipSuccess || hipMemsetAsync(found, 0, sizeof(int32_t), st) != hipSuccess) {
        sq_set_error("%s: cannot clear the counters", who);
        return SQ_ELAUNCH;
    }
    const dim3 rgrid((rows + 3) / 4), tgrid(cc_grid(total)), blk(256);
    hipLaunchKernelGGL(cc_rowscan_kernel<false>, rgrid, blk, 0, st, mask, parent, (unsigned *)nullptr, (u64 *)nullptr, rows, W);
    hipLaunchKernelGGL(cc_merge_kernel, tgrid, blk, 0, st, mask, parent, total, planes, H, W);
    hipLaunchKernelGGL(cc_compress_kernel, tgrid, blk, 0, st, parent, total);
    hipLaunchKernelGGL(obj_slots_kernel, tgrid, blk, 0, st, parent, slot, acc, total, found, max_out, pix);
    if (pix == SQ_PIX_U8)
        hipLaunchKernelGGL(obj_accumulate_kernel<SQ_PIX_U8>, rgrid, blk, 0, st, mask, image, parent, slot, acc, rows, planes, H, W);
    else if (pix == SQ_PIX_U16)
        hipLaunchKernelGGL(obj_accumulate_kernel<SQ_PIX_U16>, rgrid, blk, 0, st, mask, image, parent, slot, acc, rows, planes, H, W);
    else if (pix == SQ_PIX_F32)
        hipLaunchKernelGGL(obj_accumulate_kernel<SQ_PIX_F32>, rgrid, blk, 0, st, mask, image, parent, slot, acc, rows, planes, H, W);
    else
        hipLaunchKernelGGL(obj_accumulate_kernel<-1>, rgrid, blk, 0, st, mask, image, parent, slot, acc, rows, planes, H, W);
    hipLaunchKernelGGL(obj_emit_kernel, dim3(cc_grid(max_out)), blk, 0, st, mask, acc, found, planes, H, W, pix,
                       (long long)min_area, (long long)max_area, count, reinterpret_cast<long long *>(rows_i), rows_f, slots,
                       max_out);
    return sq_check_launch(who);
}

extern "C" int sq_objects_relabel(const uint8_t *mask, int N, int planes, int H, int W, const void *workspace,
                                  const int32_t *rank, int n_slots, int32_t *labels, uint8_t *mask_out, void *stream) {
    const char *who = "sq_objects_relabel";
    SQ_REQUIRE(mask && workspace && rank, "%s: null pointer", who);
    SQ_REQUIRE(labels || mask_out, "%s: labels and mask_out are both NULL, nothing to write", who);
    SQ_REQUIRE(N > 0 && planes > 0 && H > 0 && W > 0 && (int64_t)N * planes * H * W < ((int64_t)1 << 31),
               "%s: the mask must have fewer than 2^31 elements", who);
    SQ_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "%s: workspace must be 16-byte aligned", who);
    ObjFilled f;
    SQ_REQUIRE(sq_obj_recall(workspace, &f),"%s: n_slots %d matches nothing: sq_objects_measure has not filled this workspace",
               who, n_slots);
    SQ_REQUIRE(f.N == N && f.planes == planes && f.H == H && f.W == W && f.max_out == n_slots,
               "%s: n_slots %d and mask (%d,%d,%d,%d) do not match the sq_objects_measure call that filled this workspace "
               "(max_out %d, mask (%d,%d,%d,%d))", who, n_slots, N, planes, H, W, f.max_out, f.N, f.planes, f.H, f.W);
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = (int64_t)N * planes * H * W;
    const int *parent = reinterpret_cast<const int *>(reinterpret_cast<const char *>(workspace) + obj_table_bytes(n_slots));
    const int *slot = parent + total;
    hipLaunchKernelGGL(obj_relabel_kernel, dim3(cc_grid(total)), dim3(256), 0, st, mask, parent, slot, rank, n_slots, total,
                       labels, mask_out);
    return sq_check_launch(who);
}
