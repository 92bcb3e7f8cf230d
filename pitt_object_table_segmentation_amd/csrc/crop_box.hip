// crop_box.hip -- the arm filter's four chained pcl::CropBox<PointXYZ> passes as one device stream, so
// the frame stays in HBM between pitt_deep_filter and pitt_transform_cloud:
//
//   pitt_crop_boxes         CropBox<PointT>::applyFilter(std::vector<int>&) (PCL 1.7 filters/impl/
//                           crop_box.hpp) applied n_boxes times in a row, as filter() does through
//                           armFiltering (src/segmentation_services/arm_filter_srv.cpp:66-103, :134-140;
//                           called at src/obj_segmentation.cpp:244).
//   pitt_crop_box_from_rpy  what CropBox computes before its point loop (host): the float matrix of
//                           pcl::getTransformation, Eigen's 3x3 inverse, the fuzzy isIdentity skip (A12).
//
// Four PCL passes of read-all, write-survivors become one pass: 12 B read per point, 12 B written per
// kept point.  Three launches, no block ever waits for another:
//   k_crop_mark   one block per 2048-point tile: every point walks the stages in order (always from its
//                 original coordinates); the block stores one 64-bit keep ballot per 64-point slice, the
//                 tile's kept count and, per stage, how many points failed there first.
//   k_crop_scan   one block: the tile counts summed into 16,384-point super-tiles (the deep filter's
//                 scan granularity) and scanned into output offsets; the per-stage removed totals.
//   k_crop_write  one block per tile: ranks from the mask (a block scan of the super-tile's 256 mask
//                 words, mbcnt inside a slice), then only the surviving lanes load and store -- a slice
//                 without survivors is never read again.  The boxes (~30 float operations per rotated
//                 stage and point) are not evaluated twice.
// The boxes travel as a kernel argument (uniform scalar loads), never as a global read per point.
// The rotation is evaluated left to right in float without FMA, as the reference's x86 build does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "compact.hpp"
#include "ctx.hpp"
#include "device_common.hpp"

#pragma clang fp contract(off)

namespace pitt {

struct CropArgs {
    pitt_crop_box b[PITT_CROP_MAX_BOXES];
    int32_t n_boxes, negative, dense;
};

constexpr int kXSlices = kCTile / kBlock;       // 8 slices of 64 points per wave
constexpr int kXTileWords = kCTile / 64;        // 32 mask words per tile
constexpr int kXSuper = 8;                      // tiles per super-tile (one scan entry)
constexpr int kXSuperWords = kXSuper * kXTileWords;  // 256: one mask word per thread of a block

__host__ __device__ inline int64_t xsupers(int64_t n) {
    return (n + (int64_t)kCTile * kXSuper - 1) / ((int64_t)kCTile * kXSuper);
}

__device__ __forceinline__ int crop_lane_rank(uint64_t b) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// Steps 2-5 of one stage for one point: true when the point passes box `b`.
__device__ __forceinline__ bool crop_pass(const pitt_crop_box& b, int negative, float lx, float ly, float lz) {
    if (b.has_translation) {
        lx -= b.translation[0];
        ly -= b.translation[1];
        lz -= b.translation[2];
    }
    if (b.has_rotation) {
        const float* r = b.inv_rotation;
        const float tx = (r[0] * lx + r[1] * ly) + r[2] * lz;
        const float ty = (r[3] * lx + r[4] * ly) + r[5] * lz;
        const float tz = (r[6] * lx + r[7] * ly) + r[8] * lz;
        lx = tx;
        ly = ty;
        lz = tz;
    }
    const bool outside = lx < b.min[0] || ly < b.min[1] || lz < b.min[2] || lx > b.max[0] || ly > b.max[1] ||
                         lz > b.max[2];
    return negative ? outside : !outside;
}

// mask: 32 words per tile (slices past n are written as 0); tile_kept[t]; tile_removed[8 t + k] for
// k < n_boxes.  Wave w owns points [512 w, 512 w + 512) of the tile as 8 slices of 64 (lane l: point
// 64 j + l of slice j), so a ballot is the slice's mask word.
__global__ __launch_bounds__(kBlock) void k_crop_mark(const float* __restrict__ x, const float* __restrict__ y,
                                                      const float* __restrict__ z, int64_t n, CropArgs a,
                                                      uint64_t* __restrict__ mask, int32_t* __restrict__ tile_kept,
                                                      int32_t* __restrict__ tile_removed) {
    __shared__ int32_t part[kBlock / 64][1 + PITT_CROP_MAX_BOXES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t nt = ctiles(n);
    for (int64_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const int64_t b = t * kCTile + w * (kXSlices * 64) + lane;
        float px[kXSlices], py[kXSlices], pz[kXSlices];
        bool alive[kXSlices];
#pragma unroll
        for (int j = 0; j < kXSlices; ++j) {
            const int64_t i = b + 64 * j;
            const bool in = i < n;
            px[j] = in ? x[i] : 0.0f;
            py[j] = in ? y[i] : 0.0f;
            pz[j] = in ? z[i] : 0.0f;
            alive[j] = in;
        }
        int rem[PITT_CROP_MAX_BOXES];
#pragma unroll
        for (int k = 0; k < PITT_CROP_MAX_BOXES; ++k) rem[k] = 0;
        // CropBox skips a non-finite point of a non-dense cloud: it fails the first stage there is
        if (!a.dense && a.n_boxes > 0) {
#pragma unroll
            for (int j = 0; j < kXSlices; ++j) {
                const bool fin = __builtin_isfinite(px[j]) && __builtin_isfinite(py[j]) && __builtin_isfinite(pz[j]);
                rem[0] += __builtin_popcountll(__builtin_amdgcn_ballot_w64(alive[j] && !fin));
                alive[j] = alive[j] && fin;
            }
        }
#pragma unroll
        for (int k = 0; k < PITT_CROP_MAX_BOXES; ++k) {
            if (k < a.n_boxes) {
#pragma unroll
                for (int j = 0; j < kXSlices; ++j) {
                    const bool pass = crop_pass(a.b[k], a.negative, px[j], py[j], pz[j]);
                    rem[k] += __builtin_popcountll(__builtin_amdgcn_ballot_w64(alive[j] && !pass));
                    alive[j] = alive[j] && pass;
                }
            }
        }
        int kept = 0;
#pragma unroll
        for (int j = 0; j < kXSlices; ++j) {
            const uint64_t word = __builtin_amdgcn_ballot_w64(alive[j]);
            kept += __builtin_popcountll(word);
            if (lane == 0) mask[t * kXTileWords + w * kXSlices + j] = word;
        }
        if (lane == 0) {
            part[w][0] = kept;
#pragma unroll
            for (int k = 0; k < PITT_CROP_MAX_BOXES; ++k) part[w][1 + k] = rem[k];
        }
        __syncthreads();
        if (threadIdx.x <= PITT_CROP_MAX_BOXES) {
            int s = 0;
#pragma unroll
            for (int v = 0; v < kBlock / 64; ++v) s += part[v][threadIdx.x];
            if (threadIdx.x == 0)
                tile_kept[t] = s;
            else
                tile_removed[t * PITT_CROP_MAX_BOXES + (threadIdx.x - 1)] = s;
        }
        __syncthreads();
    }
}

// One block.  off[s] for s < ns = kept points in front of super-tile s, off[ns] = the kept total;
// off[ns + 1 + k] = points removed at stage k (contiguous with the total: one copy to the host).
__global__ __launch_bounds__(kBlock) void k_crop_scan(const int32_t* __restrict__ tile_kept,
                                                      const int32_t* __restrict__ tile_removed, int64_t nt,
                                                      int64_t ns, int32_t* __restrict__ off) {
    __shared__ int32_t lds4[kBlock / 64];
    __shared__ int32_t rsum[kBlock / 64][PITT_CROP_MAX_BOXES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carry = 0;
    for (int64_t base = 0; base < ns; base += kBlock) {
        const int64_t s = base + threadIdx.x;
        int v = 0;
        if (s < ns) {
#pragma unroll
            for (int u = 0; u < kXSuper; ++u) v += s * kXSuper + u < nt ? tile_kept[s * kXSuper + u] : 0;
        }
        int total;
        const int ex = block_exscan(v, lds4, &total);
        if (s < ns) off[s] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) off[ns] = carry;
    int r[PITT_CROP_MAX_BOXES];
#pragma unroll
    for (int k = 0; k < PITT_CROP_MAX_BOXES; ++k) r[k] = 0;
    for (int64_t t = threadIdx.x; t < nt; t += kBlock) {
#pragma unroll
        for (int k = 0; k < PITT_CROP_MAX_BOXES; ++k) r[k] += tile_removed[t * PITT_CROP_MAX_BOXES + k];
    }
#pragma unroll
    for (int k = 0; k < PITT_CROP_MAX_BOXES; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) r[k] += __shfl_xor(r[k], d, 64);
        if (lane == 0) rsum[w][k] = r[k];
    }
    __syncthreads();
    if (threadIdx.x < PITT_CROP_MAX_BOXES) {
        int s = 0;
#pragma unroll
        for (int v = 0; v < kBlock / 64; ++v) s += rsum[v][threadIdx.x];
        off[ns + 1 + threadIdx.x] = s;
    }
}

// One block per tile.  Thread i takes mask word i of the tile's super-tile; the block's exclusive scan of
// the popcounts ranks every slice of the super-tile, and wave w writes the survivors of its 8 slices.
__global__ __launch_bounds__(kBlock) void k_crop_write(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ z, int64_t n,
                                                       const uint64_t* __restrict__ mask,
                                                       const int32_t* __restrict__ off, float* __restrict__ ox,
                                                       float* __restrict__ oy, float* __restrict__ oz) {
    __shared__ int32_t lds4[kBlock / 64];
    __shared__ uint64_t s_word[kXSuperWords];
    __shared__ int32_t s_rank[kXSuperWords];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t nt = ctiles(n), nwords = nt * kXTileWords;
    for (int64_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const int64_t sup = t / kXSuper;
        const int u = (int)(t - sup * kXSuper);
        const int64_t wi = sup * kXSuperWords + threadIdx.x;
        const uint64_t mine = wi < nwords ? mask[wi] : 0;
        int total;
        const int ex = block_exscan(__builtin_popcountll(mine), lds4, &total);
        s_word[threadIdx.x] = mine;
        s_rank[threadIdx.x] = ex;
        __syncthreads();
        const int base = off[sup];
        const int s0 = u * kXTileWords + w * kXSlices;
        float qx[kXSlices], qy[kXSlices], qz[kXSlices];
#pragma unroll
        for (int j = 0; j < kXSlices; ++j) {  // a set bit is a point below n
            const int64_t i = (sup * kXSuperWords + s0 + j) * 64 + lane;
            const bool on = (s_word[s0 + j] >> lane) & 1;
            qx[j] = on ? x[i] : 0.0f;
            qy[j] = on ? y[i] : 0.0f;
            qz[j] = on ? z[i] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < kXSlices; ++j) {
            const uint64_t word = s_word[s0 + j];
            if ((word >> lane) & 1) {
                const int o = base + s_rank[s0 + j] + crop_lane_rank(word);
                ox[o] = qx[j];
                oy[o] = qy[j];
                oz[o] = qz[j];
            }
        }
        __syncthreads();
    }
}

static bool planes_overlap(const float* a, const float* b, int64_t n) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b, nb = (uintptr_t)n * 4;
    return pa < pb + nb && pb < pa + nb;
}

static int crop_boxes_impl(pitt_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                           const pitt_crop_box* boxes, int32_t n_boxes, int32_t negative, int32_t dense, float* ox,
                           float* oy, float* oz, int64_t* n_out, int64_t* removed) {
    hipStream_t s = ctx->stream;
    for (int k = 0; k < n_boxes && removed; ++k) removed[k] = 0;
    *n_out = 0;
    if (n == 0) return PITT_OK;
    if (n_boxes == 0) {  // no stage: every point is kept
        PITT_HIP_TRY(hipMemcpyAsync(ox, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        PITT_HIP_TRY(hipMemcpyAsync(oy, y, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        PITT_HIP_TRY(hipMemcpyAsync(oz, z, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        PITT_HIP_TRY(hipStreamSynchronize(s));
        *n_out = n;
        return PITT_OK;
    }
    const int64_t nt = ctiles(n), ns = xsupers(n);
    const size_t mask_bytes = (size_t)nt * kXTileWords * 8;
    uint64_t* mask = (uint64_t*)ctx->buf("crop_mask", mask_bytes);
    int32_t* cnt = (int32_t*)ctx->buf("crop_cnt", (size_t)nt * (1 + PITT_CROP_MAX_BOXES) * 4);
    int32_t* off = (int32_t*)ctx->buf("crop_off", (size_t)(ns + 1 + PITT_CROP_MAX_BOXES) * 4);
    int32_t* h = (int32_t*)ctx->pinned("crop_total", (1 + PITT_CROP_MAX_BOXES) * 4);
    if (!mask || !cnt || !off || !h) return ctx->fail(PITT_E_NOMEM, "crop box scratch");
    int32_t *tile_kept = cnt, *tile_removed = cnt + nt;
    CropArgs a;
    for (int k = 0; k < PITT_CROP_MAX_BOXES; ++k) a.b[k] = boxes[k < n_boxes ? k : 0];
    a.n_boxes = n_boxes;
    a.negative = negative ? 1 : 0;
    a.dense = dense ? 1 : 0;
    const int grid = grid_for_tiles(nt);
    // algorithmic bytes: 12 B read per point and the mask written here; the mask read and 12 B written
    // per kept point in the write pass (set once the kept count is known; the survivors' second read is
    // the implementation's, not the algorithm's)
    int rec = ctx->prof_begin("k_crop_mark", (double)n * 12.0 + (double)mask_bytes);
    hipLaunchKernelGGL(k_crop_mark, dim3(grid), dim3(kBlock), 0, s, x, y, z, n, a, mask, tile_kept, tile_removed);
    ctx->prof_end(rec);
    rec = ctx->prof_begin("k_crop_scan", (double)nt * (1 + PITT_CROP_MAX_BOXES) * 4.0 + (double)(ns + 1) * 4.0);
    hipLaunchKernelGGL(k_crop_scan, dim3(1), dim3(kBlock), 0, s, tile_kept, tile_removed, nt, ns, off);
    ctx->prof_end(rec);
    const int rec_w = ctx->prof_begin("k_crop_write", (double)mask_bytes);
    hipLaunchKernelGGL(k_crop_write, dim3(grid), dim3(kBlock), 0, s, x, y, z, n, mask, off, ox, oy, oz);
    ctx->prof_end(rec_w);
    PITT_HIP_TRY(hipGetLastError());
    PITT_HIP_TRY(hipMemcpyAsync(h, off + ns, (1 + PITT_CROP_MAX_BOXES) * 4, hipMemcpyDeviceToHost, s));
    PITT_HIP_TRY(hipStreamSynchronize(s));
    *n_out = h[0];
    for (int k = 0; k < n_boxes && removed; ++k) removed[k] = h[1 + k];
    ctx->prof_set_bytes(rec_w, (double)mask_bytes + 12.0 * (double)h[0]);
    return PITT_OK;
}

}  // namespace pitt

extern "C" {

int pitt_crop_box_from_rpy(const float min[3], const float max[3], const float translation[3], const float rpy[3],
                           pitt_crop_box* out) {
    if (!min || !max || !translation || !rpy || !out) return PITT_E_INVALID;
    for (int c = 0; c < 3; ++c) {
        out->min[c] = min[c];
        out->max[c] = max[c];
        out->translation[c] = translation[c];
    }
    // translation_ != Eigen::Vector3f::Zero()
    out->has_translation = (translation[0] != 0.0f || translation[1] != 0.0f || translation[2] != 0.0f) ? 1 : 0;
    for (int i = 0; i < 9; ++i) out->inv_rotation[i] = (i % 4 == 0) ? 1.0f : 0.0f;
    out->has_rotation = 0;
    // rotation_ != Eigen::Vector3f::Zero(): otherwise transform and its inverse stay the identity
    if (!(rpy[0] != 0.0f || rpy[1] != 0.0f || rpy[2] != 0.0f)) return PITT_OK;
    // pcl::getTransformation(0, 0, 0, roll, pitch, yaw, t) (common/impl/eigen.hpp), Scalar = float
    const float roll = rpy[0], pitch = rpy[1], yaw = rpy[2];
    const float A = cosf(yaw), B = sinf(yaw), C = cosf(pitch), D = sinf(pitch), E = cosf(roll), F = sinf(roll);
    const float DE = D * E, DF = D * F;
    const float m[3][3] = {{A * C, A * DF - B * E, B * F + A * DE},
                           {B * C, A * E + B * DF, B * DE - A * F},
                           {-D, C * F, C * E}};
    // Eigen 3.2 LU/Inverse.h compute_inverse<.., 3>: cofactor_3x3<i, j> = m(i1, j1) m(i2, j2) - m(i1, j2) m(i2, j1),
    // det = (cofactors of column 0) . (column 0) summed as c0 + (c1 + c2) (the unrolled redux), the
    // result's (j, i) entry = cofactor<i, j> * (1 / det)
    auto cof = [&](int i, int j) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
    };
    const float c0 = cof(0, 0), c1 = cof(1, 0), c2 = cof(2, 0);
    const float det = c0 * m[0][0] + (c1 * m[1][0] + c2 * m[2][0]);
    const float invdet = 1.0f / det;
    float inv[3][3];
    inv[0][0] = c0 * invdet;
    inv[0][1] = c1 * invdet;
    inv[0][2] = c2 * invdet;
    for (int j = 1; j < 3; ++j)
        for (int i = 0; i < 3; ++i) inv[j][i] = cof(i, j) * invdet;
    // MatrixBase::isIdentity(prec = 1e-5f) on inverse_transform.matrix(): isApprox(d, 1) on the diagonal,
    // isMuchSmallerThan(o, 1) off it (the 4x4's last row is exact; its translation -R^-1 * 0 is +-0)
    bool identity = true;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const float v = inv[i][j];
            if (i == j)
                identity = identity && (fabsf(v - 1.0f) <= std::min(fabsf(v), 1.0f) * 1e-5f);
            else
                identity = identity && (fabsf(v) <= 1e-5f);
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out->inv_rotation[3 * i + j] = inv[i][j];
    out->has_rotation = identity ? 0 : 1;
    return PITT_OK;
}

int pitt_crop_boxes(pitt_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                    const pitt_crop_box* boxes, int32_t n_boxes, int32_t negative, int32_t dense, float* ox, float* oy,
                    float* oz, int64_t* n_out, int64_t* removed) {
    if (!ctx) return PITT_E_INVALID;
    if (n < 0 || (n > 0 && (!x || !y || !z))) return ctx->fail(PITT_E_INVALID, "null argument");
    if (n > 0x7fffffff) return ctx->fail(PITT_E_INVALID, "cloud larger than 2^31 points");
    if (n_boxes < 0 || n_boxes > PITT_CROP_MAX_BOXES || (n_boxes > 0 && !boxes))
        return ctx->fail(PITT_E_INVALID, "n_boxes outside [0, PITT_CROP_MAX_BOXES]");
    if (!ox || !oy || !oz || !n_out) return ctx->fail(PITT_E_INVALID, "null output");
    const float* in[3] = {x, y, z};
    float* out[3] = {ox, oy, oz};
    for (int i = 0; i < 3 && n > 0; ++i)
        for (int j = 0; j < 3; ++j) {
            if (pitt::planes_overlap(in[i], out[j], n)) return ctx->fail(PITT_E_INVALID, "output aliases input");
            if (j > i && pitt::planes_overlap(out[i], out[j], n))
                return ctx->fail(PITT_E_INVALID, "output planes overlap");
        }
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(PITT_E_HIP, "hipSetDevice");
    return pitt::crop_boxes_impl(ctx, x, y, z, n, boxes, n_boxes, negative, dense, ox, oy, oz, n_out, removed);
}

int pitt_crop_boxes_host(pitt_ctx* ctx, const float* xyz16, int64_t n, const pitt_crop_box* boxes, int32_t n_boxes,
                         int32_t negative, int32_t dense, float* xyz16_out, int64_t* n_out, int64_t* removed) {
    using namespace pitt;
    if (!ctx) return PITT_E_INVALID;
    if (n < 0 || (n > 0 && (!xyz16 || !xyz16_out)) || !n_out) return ctx->fail(PITT_E_INVALID, "null argument");
    if (n > 0x7fffffff) return ctx->fail(PITT_E_INVALID, "cloud larger than 2^31 points");
    if (n_boxes < 0 || n_boxes > PITT_CROP_MAX_BOXES || (n_boxes > 0 && !boxes))
        return ctx->fail(PITT_E_INVALID, "n_boxes outside [0, PITT_CROP_MAX_BOXES]");
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(PITT_E_HIP, "hipSetDevice");
    const size_t nb = (size_t)std::max<int64_t>(n, 1) * 4;
    void* aos = ctx->buf("crop_haos", nb * 4);
    float* in = (float*)ctx->buf("crop_hin", nb * 3);
    float* out = (float*)ctx->buf("crop_hout", nb * 3);
    if (!aos || !in || !out) return ctx->fail(PITT_E_NOMEM, "crop box staging");
    hipStream_t s = ctx->stream;
    const int64_t st = std::max<int64_t>(n, 1);  // plane stride (floats)
    PITT_HIP_TRY(upload_aos(s, aos, xyz16, n, 16, in, in + st, in + 2 * st));
    const int rc = pitt_crop_boxes(ctx, in, in + st, in + 2 * st, n, boxes, n_boxes, negative, dense, out, out + st,
                                   out + 2 * st, n_out, removed);
    if (rc < 0) return rc;
    const int64_t m = *n_out;
    if (m > 0) {
        float* hp = (float*)ctx->pinned("crop_hplanes", (size_t)m * 12);
        if (!hp) return ctx->fail(PITT_E_NOMEM, "crop box staging");
        for (int c = 0; c < 3; ++c)
            PITT_HIP_TRY(hipMemcpyAsync(hp + c * m, out + c * st, (size_t)m * 4, hipMemcpyDeviceToHost, s));
        PITT_HIP_TRY(hipStreamSynchronize(s));
        for (int64_t i = 0; i < m; ++i) {
            xyz16_out[4 * i] = hp[i];
            xyz16_out[4 * i + 1] = hp[m + i];
            xyz16_out[4 * i + 2] = hp[2 * m + i];
            xyz16_out[4 * i + 3] = 1.0f;
        }
    }
    return PITT_OK;
}

}  // extern "C"
